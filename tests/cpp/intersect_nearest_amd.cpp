// Nearest-hits ray queries through the C++20 mirror: bvh::v2::amd::intersect_nearest_batch (host form, device form, original ids) on a
// stack of large overlapping triangles, against what a caller had to do before: Bvh::intersect<false, IsRobust> per ray with a leaf_fn
// that records every hit and never shortens the ray, the list sorted by (t, prim) and cut at k. k = 1 is also held to the ordinary
// closest-hit walk. tests/test_gpu_intersect_nearest_cpp.py runs it.
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

    // what a caller had before: every hit of the unshortened ray, sorted by (t, prim)
    auto by_t = [](const Hit& a, const Hit& b) { return a.t < b.t || (a.t == b.t && a.prim < b.prim); };
    std::vector<std::vector<Hit>> want(rays.size());
    std::vector<Hit> closest(rays.size());
    size_t longest = 0;
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
        std::sort(want[r].begin(), want[r].end(), by_t);
        longest = std::max(longest, want[r].size());
        // the ordinary closest-hit walk, which shortens the ray
        Ray ray = rays[r];
        Hit best{};
        best.prim = Hit::invalid; best.t = ray.tmax;
        bvh.template intersect<false, IsRobust>(ray, bvh.get_root().index, stack, [&](size_t begin, size_t end) {
            for (size_t i = begin; i < end; ++i)
                if (auto hit = prims[i].intersect(ray)) {
                    best.prim = static_cast<uint32_t>(i);
                    std::tie(best.t, best.u, best.v) = *hit;
                    ray.tmax = best.t;
                }
            return best.prim != Hit::invalid;
        });
        closest[r] = best;
    }

    auto close = [](Scalar a, Scalar b) { return std::abs(a - b) <= 8 * std::numeric_limits<Scalar>::epsilon() * std::max(Scalar(1), std::abs(b)); };
    int bad = 0;
    size_t cut = 0;
    // A k counts only where the per-ray walk's own lists show what it does to the rows: k = 1 .. 17 must CUT rows (lists longer than
    // k exist), and at k = 64 no list of this scene is that long, so every row must be the WHOLE sorted list and its padding.
    auto cut_at = [&](unsigned k) { size_t c = 0; for (const auto& w : want) c += w.size() > k; return c; };
    auto expect = [&](unsigned k, const std::vector<Hit>& rows, const std::vector<uint32_t>& counts, bool original_ids, const char* what) {
        bool ok = rows.size() == rays.size() * k && counts.size() == rays.size();
        for (size_t r = 0; ok && r < rays.size(); ++r) {
            const size_t m = std::min<size_t>(want[r].size(), k);
            ok = counts[r] == m;
            for (size_t e = 0; ok && e < k; ++e) {
                const Hit& h = rows[k * r + e];
                if (e < m) {
                    const Hit& x = want[r][e];
                    ok = h.prim == (original_ids ? static_cast<uint32_t>(bvh.prim_ids[x.prim]) : x.prim) && close(h.t, x.t) && close(h.u, x.u) && close(h.v, x.v);
                } else ok = h.prim == Hit::invalid && h.t == rays[r].tmax && h.u == 0 && h.v == 0;
            }
        }
        if (!ok) { std::printf("%s: %s, k = %u, differs from the sorted per-ray walk\n", name, what, k); ++bad; }
    };

    std::vector<Hit> rows;
    std::vector<uint32_t> counts;
    for (unsigned k : {1u, 2u, 3u, 8u, 17u, 64u}) {
        amd::intersect_nearest_batch<IsRobust>(bvh, d_prims, std::span<const Ray>(rays), k, rows, &counts);
        expect(k, rows, counts, false, "intersect_nearest_batch (host form)");
        cut += cut_at(k);
        if (k < 64 ? cut_at(k) == 0 : cut_at(k) != 0) { std::printf("%s: k = %u: %zu rows cut (longest list %zu): the scene does not exercise it\n", name, k, cut_at(k), longest); ++bad; }
        if (k == 1) {                                         // the closest-hit walk's record
            bool ok = true;
            for (size_t r = 0; ok && r < rays.size(); ++r)
                ok = rows[r].prim == closest[r].prim && (closest[r].prim == Hit::invalid ? rows[r].t == rays[r].tmax : close(rows[r].t, closest[r].t));
            if (!ok) { std::printf("%s: k = 1 differs from the closest-hit walk\n", name); ++bad; }
        }
    }
    amd::intersect_nearest_batch<IsRobust>(bvh, d_prims, std::span<const Ray>(rays), 4u, rows, &counts, BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_SORTED);
    expect(4u, rows, counts, true, "intersect_nearest_batch (original ids, sorted batch)");
    {   // device form, with and without counts: the same rows as the host form
        const unsigned k = 4;
        amd::DeviceArray<Ray> d_rays{std::span<const Ray>(rays)};
        amd::DeviceArray<Hit> d_hits(k * rays.size());
        amd::DeviceArray<uint32_t> d_counts(rays.size());
        amd::intersect_nearest_batch<IsRobust>(bvh, d_prims, d_rays, k, d_hits, &d_counts);
        std::vector<Hit> got(k * rays.size());
        std::vector<uint32_t> got_counts(rays.size());
        d_hits.download(std::span<Hit>(got));
        d_counts.download(std::span<uint32_t>(got_counts));
        expect(k, got, got_counts, false, "intersect_nearest_batch (device form)");
        amd::DeviceArray<Hit> d_hits2(k * rays.size());
        amd::intersect_nearest_batch<IsRobust>(bvh, d_prims, d_rays, k, d_hits2, nullptr);
        std::vector<Hit> got2(k * rays.size());
        d_hits2.download(std::span<Hit>(got2));
        bool ok = true;
        for (size_t e = 0; ok && e < got.size(); ++e) ok = got[e].prim == got2[e].prim && got[e].t == got2[e].t && got[e].u == got2[e].u && got[e].v == got2[e].v;
        if (!ok) { std::printf("%s: intersect_nearest_batch (device form, no counts) differs\n", name); ++bad; }
        bool threw = false;
        try { amd::intersect_nearest_batch<IsRobust>(bvh, d_prims, std::span<const Ray>(rays), 65u, rows, &counts); } catch (const amd::Error&) { threw = true; }
        if (!threw) { std::printf("%s: k = 65 was not refused\n", name); ++bad; }
    }
    if (longest <= 17 || longest > 64 || cut_at(1) < rays.size() / 2) { std::printf("%s: the scene is too sparse: longest list %zu, %zu rows cut\n", name, longest, cut); ++bad; }

    std::printf("%s: %zu triangles, %zu rays (longest list %zu; rows cut at k = 1, 8, 17, 64: %zu, %zu, %zu, %zu; %zu in all): %s\n", name, np, rays.size(), longest,
                cut_at(1), cut_at(8), cut_at(17), cut_at(64), cut,
                bad ? "MISMATCH" : "intersect_nearest_batch == sorted per-ray walk");
    return bad;
}

int main() {
    return run<float, false>("float") + run<float, true>("float robust") + run<double, false>("double");
}
