// All-hits ray queries through the C++20 mirror: bvh::v2::amd::intersect_all_batch (host form, device form with fixed slots, original
// ids) on a stack of large overlapping triangles, against the walk the feature replaces: Bvh::intersect<false, IsRobust> per ray with
// a leaf_fn that records every hit and never shortens the ray. That walk visits the nearer child first and the batch query the left
// one, so both lists are compared sorted by (t, prim) - which is also how a caller gets hits along the ray.
// tests/test_gpu_intersect_all_cpp.py runs it.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/ray.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/stack.h>
#include <bvh/v2/tri.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

template <typename Scalar, bool IsRobust>
static int run(const char* name) {
    using Vec3 = bvh::v2::Vec<Scalar, 3>;
    using BBox = bvh::v2::BBox<Scalar, 3>;
    using Tri = bvh::v2::Tri<Scalar, 3>;
    using Node = bvh::v2::Node<Scalar, 3>;
    using Bvh = bvh::v2::Bvh<Node>;
    using Ray = bvh::v2::Ray<Scalar, 3>;
    using Hit = bvh::v2::amd::Hit<Scalar>;
    using PrecomputedTri = bvh::v2::PrecomputedTri<Scalar>;
    namespace amd = bvh::v2::amd;

    // 160 large triangles in the unit cube from a small generator: most rays through the cube cross many of them
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return static_cast<Scalar>((state >> 8) * (1.0 / 16777216.0)); };
    std::vector<Tri> tris;
    for (int i = 0; i < 160; ++i) {
        const Vec3 a(next(), next(), next()), b(next(), next(), next()), c(next(), next(), next());
        tris.emplace_back(a, b, c);
    }
    const size_t np = tris.size();
    std::vector<BBox> bboxes(np);
    std::vector<Vec3> centers(np);
    for (size_t i = 0; i < np; ++i) { bboxes[i] = tris[i].get_bbox(); centers[i] = tris[i].get_center(); }
    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    Bvh bvh = bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
    auto d_prims = amd::permuted_triangles(bvh, std::span<const Tri>(tris));
    std::vector<PrecomputedTri> prims(np);
    for (size_t i = 0; i < np; ++i) prims[i] = PrecomputedTri(tris[bvh.prim_ids[i]]);

    std::vector<Ray> rays;                                    // from outside the cube through points inside it; some end inside
    for (int k = 0; k < 300; ++k) {
        const Vec3 org(Scalar(-1) + Scalar(3) * next(), Scalar(-1) + Scalar(3) * next(), k % 2 ? Scalar(-1) : Scalar(2));
        const Vec3 target(next(), next(), next());
        rays.emplace_back(org, target - org, k % 5 == 0 ? Scalar(0.5) : Scalar(0), k % 3 == 0 ? Scalar(1) : Scalar(4));
    }

    // the walk this query replaces: one ray at a time, a leaf_fn that records and never shortens
    std::vector<std::vector<Hit>> want(rays.size());
    size_t total = 0, longest = 0;
    for (size_t r = 0; r < rays.size(); ++r) {
        bvh::v2::SmallStack<typename Node::Index, 64> stack;
        bvh.template intersect<false, IsRobust>(rays[r], bvh.get_root().index, stack, [&](size_t begin, size_t end) {
            for (size_t i = begin; i < end; ++i)
                if (auto hit = prims[i].intersect(rays[r])) {
                    Hit h{};
                    h.prim = static_cast<uint32_t>(i);
                    std::tie(h.t, h.u, h.v) = *hit;
                    want[r].push_back(h);
                }
            return false;
        });
        total += want[r].size();
        longest = std::max(longest, want[r].size());
    }

    auto by_t = [](const Hit& a, const Hit& b) { return a.t < b.t || (a.t == b.t && a.prim < b.prim); };
    auto close = [](Scalar a, Scalar b) { return std::abs(a - b) <= 8 * std::numeric_limits<Scalar>::epsilon() * std::max(Scalar(1), std::abs(b)); };
    int bad = 0;
    auto expect = [&](const std::vector<uint64_t>& offsets, const std::vector<Hit>& list, bool original_ids, const char* what) {
        bool ok = offsets.size() == rays.size() + 1 && offsets[0] == 0 && offsets.back() == list.size();
        for (size_t r = 0; ok && r < rays.size(); ++r) {
            ok = offsets[r + 1] - offsets[r] == want[r].size();
            if (!ok) break;
            std::vector<Hit> got(list.begin() + offsets[r], list.begin() + offsets[r + 1]), exp = want[r];
            if (original_ids) for (Hit& h : exp) h.prim = static_cast<uint32_t>(bvh.prim_ids[h.prim]);
            std::sort(got.begin(), got.end(), by_t);
            std::sort(exp.begin(), exp.end(), by_t);
            for (size_t e = 0; ok && e < exp.size(); ++e)
                ok = got[e].prim == exp[e].prim && close(got[e].t, exp[e].t) && close(got[e].u, exp[e].u) && close(got[e].v, exp[e].v);
        }
        if (!ok) { std::printf("%s: %s differs from the per-ray walk\n", name, what); ++bad; }
    };

    std::vector<uint64_t> offsets;
    std::vector<Hit> list;
    amd::intersect_all_batch<IsRobust>(bvh, d_prims, std::span<const Ray>(rays), offsets, list);
    expect(offsets, list, false, "intersect_all_batch (host form)");
    const std::vector<Hit> exact = list;
    const std::vector<uint64_t> exact_offsets = offsets;
    amd::intersect_all_batch<IsRobust>(bvh, d_prims, std::span<const Ray>(rays), offsets, list, BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_SORTED);
    expect(offsets, list, true, "intersect_all_batch (original ids, sorted batch)");
    {   // device form, one pass into k slots per ray: untruncated counts, the prefix of the exact list, the miss record in the rest
        const size_t k = 4;
        amd::DeviceArray<Ray> d_rays{std::span<const Ray>(rays)};
        amd::DeviceArray<uint32_t> d_counts(rays.size());
        std::vector<uint64_t> fixed(rays.size() + 1);
        for (size_t r = 0; r <= rays.size(); ++r) fixed[r] = k * r;
        amd::DeviceArray<uint64_t> d_offsets{std::span<const uint64_t>(fixed)};
        amd::DeviceArray<Hit> d_list(k * rays.size());
        amd::intersect_all_batch<IsRobust>(bvh, d_prims, d_rays, &d_counts, &d_offsets, &d_list);
        std::vector<uint32_t> counts(rays.size());
        std::vector<Hit> slots(k * rays.size());
        d_counts.download(std::span<uint32_t>(counts));
        d_list.download(std::span<Hit>(slots));
        bool ok = true;
        for (size_t r = 0; ok && r < rays.size(); ++r) {
            ok = counts[r] == want[r].size();
            for (size_t e = 0; ok && e < k; ++e) {
                const Hit& h = slots[k * r + e];
                if (e < counts[r]) { const Hit& x = exact[exact_offsets[r] + e]; ok = h.prim == x.prim && h.t == x.t && h.u == x.u && h.v == x.v; }
                else ok = h.prim == Hit::invalid && h.t == rays[r].tmax && h.u == 0 && h.v == 0;
            }
        }
        if (!ok) { std::printf("%s: intersect_all_batch (device form, %zu slots) differs\n", name, k); ++bad; }
    }
    if (longest < 8 || total < 3 * rays.size()) { std::printf("%s: the scene is too sparse: %zu hits, longest list %zu\n", name, total, longest); ++bad; }

    std::printf("%s: %zu triangles, %zu rays cross %zu (longest list %zu): %s\n", name, np, rays.size(), total, longest,
                bad ? "MISMATCH" : "intersect_all_batch == per-ray walk");
    return bad;
}

int main() {
    return run<float, false>("float") + run<float, true>("float robust") + run<double, false>("double");
}
