// Convex-region queries through the C++20 mirror: bvh::v2::amd::region_tris_batch (device form and host form) and region_spheres_batch on
// a small height field with integer coordinates against planes with small integer coefficients, so that every plane value is exact
// and a brute force written here (listed in the tree's left-first depth-first order) must be met exactly: the plane-by-plane test and
// the inside flags by their definitions; BVH_AMD_REGION_EXACT as a subset of it that equals it for a single plane and drops the
// triangle beside the corner of a crafted wedge. tests/test_gpu_region_cpp.py runs it.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/tri.h>
#include <bvh/v2/sphere.h>

#include <cstdio>
#include <vector>

template <typename Scalar>
static int run(const char* name) {
    using Vec3 = bvh::v2::Vec<Scalar, 3>;
    using BBox = bvh::v2::BBox<Scalar, 3>;
    using Tri = bvh::v2::Tri<Scalar, 3>;
    using Sphere = bvh::v2::Sphere<Scalar, 3>;
    using Node = bvh::v2::Node<Scalar, 3>;
    using Bvh = bvh::v2::Bvh<Node>;
    namespace amd = bvh::v2::amd;
    using Plane = amd::RegionPlane<Scalar>;
    static_assert(sizeof(Tri) == 9 * sizeof(Scalar) && sizeof(Sphere) == 4 * sizeof(Scalar) && sizeof(Plane) == 4 * sizeof(Scalar));

    const int side = 12;                                      // a 12 x 12 height field with integer heights, two triangles per cell
    auto height = [](int i, int j) { return Scalar((i * 7 + j * 3) % 5); };
    std::vector<Tri> tris;
    std::vector<Sphere> spheres;
    for (int i = 0; i < side; ++i)
        for (int j = 0; j < side; ++j) {
            const Vec3 a(Scalar(i), height(i, j), Scalar(j)), b(Scalar(i + 1), height(i + 1, j), Scalar(j));
            const Vec3 c(Scalar(i + 1), height(i + 1, j + 1), Scalar(j + 1)), d(Scalar(i), height(i, j + 1), Scalar(j + 1));
            tris.emplace_back(a, b, c);
            tris.emplace_back(a, c, d);
            spheres.emplace_back(a, Scalar((i + j) % 3));
            spheres.emplace_back(c, Scalar(1));
        }
    const size_t np = tris.size();
    auto build = [&](auto bbox_of, auto center_of) {
        std::vector<BBox> bboxes(np);
        std::vector<Vec3> centers(np);
        for (size_t i = 0; i < np; ++i) { bboxes[i] = bbox_of(i); centers[i] = center_of(i); }
        typename bvh::v2::DefaultBuilder<Node>::Config config;
        config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
        return bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
    };
    Bvh tri_bvh = build([&](size_t i) { return tris[i].get_bbox(); }, [&](size_t i) { return tris[i].get_center(); });
    Bvh sph_bvh = build([&](size_t i) { return spheres[i].get_bbox(); }, [&](size_t i) { return spheres[i].get_center(); });
    amd::DeviceArray<Tri> d_tris{std::span<const Tri>(tris)};
    amd::DeviceArray<Sphere> d_spheres{std::span<const Sphere>(spheres)};

    // regions of m = 4 planes: axis-aligned and slanted slabs and wedges with integer coefficients (normals of integer length for the
    // spheres: (1,0,0), (0,0,1), (3,0,4)), padded with {0, 0, 0, 0}; a half-space; everything; nothing
    const size_t m = 4;
    std::vector<Plane> planes;
    auto region = [&](std::vector<Plane> p) { while (p.size() < m) p.push_back(Plane{0, 0, 0, 0}); planes.insert(planes.end(), p.begin(), p.end()); };
    for (int k = 0; k < 40; ++k) {
        // (off the grid by a half and a quarter: the cell that holds a corner of the column has a triangle that passes every plane on
        //  its own and misses the column)
        const Scalar x0 = Scalar(k % 11) + Scalar(0.5), z0 = Scalar((k * 5) % 9) + Scalar(0.25), w = Scalar(1 + k % 4);
        region({Plane{-1, 0, 0, x0}, Plane{1, 0, 0, -(x0 + w)}, Plane{0, 0, -1, z0}, Plane{0, 0, 1, -(z0 + w)}});      // a column x0 <= x <= x0 + w, z0 <= z <= z0 + w
        region({Plane{3, 0, 4, Scalar(-5 * (k + 2))}, Plane{-3, 0, -4, Scalar(5 * k)}});                              // a slanted slab
        region({Plane{1, 0, 0, -x0}});                                                                                // a half-space
    }
    region({Plane{0, 0, 0, 0}});
    region({Plane{0, 0, 0, 1}});
    const size_t single_from = planes.size() / m;
    region({Plane{1, 0, 1, -1}});                                                                                     // x + z <= 1: one plane
    // a wedge whose corner (-1.5, *, -1.5) lies half a unit beyond the long edge x + z = -2 of a triangle that reaches into each of
    // the two half-spaces: it passes each plane on its own
    const size_t wedge = planes.size() / m;
    region({Plane{1, 0, 0, Scalar(1.5)}, Plane{0, 0, 1, Scalar(1.5)}});                                               // x <= -1.5, z <= -1.5
    tris.emplace_back(Vec3(Scalar(-3), Scalar(0), Scalar(1)), Vec3(Scalar(1), Scalar(0), Scalar(-3)), Vec3(Scalar(1), Scalar(0), Scalar(1)));
    const size_t nq = planes.size() / m;

    auto value = [](const Plane& p, const Vec3& x) { return ((p.nx * x[0] + p.ny * x[1]) + p.nz * x[2]) + p.d; };
    auto dfs_of = [](const Bvh& bvh) {
        std::vector<size_t> dfs, stack{0};
        while (!stack.empty()) {
            const Node& node = bvh.nodes[stack.back()];
            stack.pop_back();
            if (node.is_leaf()) { for (size_t i = 0; i < node.index.prim_count(); ++i) dfs.push_back(node.index.first_id() + i); }
            else { stack.push_back(node.index.first_id() + 1); stack.push_back(node.index.first_id()); }
        }
        return dfs;
    };

    int bad = 0;
    auto expect = [&](const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& list, const std::vector<std::vector<uint32_t>>& want, const char* what) {
        bool ok = offsets.size() == want.size() + 1 && offsets[0] == 0;
        for (size_t q = 0; ok && q < want.size(); ++q) {
            ok = offsets[q + 1] - offsets[q] == want[q].size() && offsets[q + 1] <= list.size();
            for (size_t e = 0; ok && e < want[q].size(); ++e) ok = list[offsets[q] + e] == want[q][e];
        }
        if (ok) ok = offsets.back() == list.size();
        if (!ok) { std::printf("%s: %s differs from the brute force\n", name, what); ++bad; }
    };

    // triangles (the tree does not know the extra triangle: it is tested on its own below)
    const std::vector<size_t> tri_dfs = dfs_of(tri_bvh);
    std::vector<std::vector<uint32_t>> want(nq), want_ids(nq), want_in(nq);
    size_t total = 0, inside_total = 0;
    for (size_t q = 0; q < nq; ++q)
        for (size_t i : tri_dfs) {
            const Tri& t = tris[tri_bvh.prim_ids[i]];
            bool pass = true, in = true;
            for (size_t p = 0; p < m; ++p) {
                const Plane& pl = planes[q * m + p];
                const bool i0 = value(pl, t.p0) <= 0, i1 = value(pl, t.p1) <= 0, i2 = value(pl, t.p2) <= 0;
                pass = pass && (i0 || i1 || i2);
                in = in && i0 && i1 && i2;
            }
            if (pass) { want[q].push_back(uint32_t(i)); want_ids[q].push_back(uint32_t(tri_bvh.prim_ids[i])); want_in[q].push_back(in); ++total; inside_total += in; }
        }
    std::vector<uint64_t> offsets, e_offsets;
    std::vector<uint32_t> list, e_list;
    std::vector<uint8_t> inside;
    amd::region_tris_batch(tri_bvh, d_tris, std::span<const Plane>(planes), m, offsets, list, &inside);
    expect(offsets, list, want, "region_tris_batch (host form)");
    {
        std::vector<uint32_t> flags(inside.begin(), inside.end());
        expect(offsets, flags, want_in, "region_tris_batch (inside flags)");
    }
    amd::region_tris_batch(tri_bvh, d_tris, std::span<const Plane>(planes), m, offsets, list, nullptr, BVH_AMD_RAY_ORIGINAL_IDS);
    expect(offsets, list, want_ids, "region_tris_batch (original ids)");
    {
        amd::DeviceArray<Plane> d_planes{std::span<const Plane>(planes)};
        amd::DeviceArray<uint32_t> d_counts(nq);
        amd::DeviceArray<uint64_t> d_offsets(nq + 1);
        amd::region_tris_batch(tri_bvh, d_tris, d_planes, m, &d_counts, nullptr, nullptr);
        bvh::v2::amd::check(bvh_amd_offsets_from_counts(d_counts.data(), nq, d_offsets.data(), nullptr), "offsets_from_counts");
        std::vector<uint64_t> off(nq + 1);
        d_offsets.download(std::span<uint64_t>(off));
        amd::DeviceArray<uint32_t> d_list(off.back() + 1);
        amd::region_tris_batch(tri_bvh, d_tris, d_planes, m, nullptr, &d_offsets, &d_list);
        std::vector<uint32_t> got(off.back() + 1);
        d_list.download(std::span<uint32_t>(got));
        got.pop_back();
        expect(off, got, want, "region_tris_batch (device form)");
    }
    // EXACT: a subset of the plane-by-plane lists in the same order; equal for the regions of a single plane
    amd::region_tris_batch(tri_bvh, d_tris, std::span<const Plane>(planes), m, e_offsets, e_list, nullptr, BVH_AMD_REGION_EXACT);
    size_t exact_total = e_list.size();
    for (size_t q = 0; q < nq; ++q) {
        size_t at = 0;
        for (uint64_t e = e_offsets[q]; e < e_offsets[q + 1]; ++e) {
            while (at < want[q].size() && want[q][at] != e_list[e]) ++at;
            if (at == want[q].size()) { std::printf("%s: EXACT lists a triangle of region %zu that the plane-by-plane test does not\n", name, q); ++bad; break; }
        }
        const bool single = q % 3 == 2 || q >= single_from - 2;
        if (single && q != wedge && e_offsets[q + 1] - e_offsets[q] != want[q].size()) { std::printf("%s: EXACT differs for the one-plane region %zu\n", name, q); ++bad; }
    }
    if (exact_total >= total || want[single_from - 2].size() != np || !want[single_from - 1].empty()) { std::printf("%s: EXACT lists %zu of %zu; everything %zu, nothing %zu\n", name, exact_total, total, want[single_from - 2].size(), want[single_from - 1].size()); ++bad; }
    {   // the triangle beside the wedge's corner, alone in a tree of one leaf
        std::vector<Tri> one{tris.back()};
        std::vector<BBox> bb{one[0].get_bbox()};
        std::vector<Vec3> cc{one[0].get_center()};
        Bvh leaf = bvh::v2::DefaultBuilder<Node>::build(bb, cc);
        amd::DeviceArray<Tri> d_one{std::span<const Tri>(one)};
        std::vector<Plane> w(planes.begin() + wedge * m, planes.begin() + (wedge + 1) * m);
        amd::region_tris_batch(leaf, d_one, std::span<const Plane>(w), m, offsets, list);
        amd::region_tris_batch(leaf, d_one, std::span<const Plane>(w), m, e_offsets, e_list, nullptr, BVH_AMD_REGION_EXACT);
        if (list.size() != 1 || !e_list.empty()) { std::printf("%s: beside the wedge's corner: the plane-by-plane test lists %zu, EXACT %zu\n", name, list.size(), e_list.size()); ++bad; }
    }

    // spheres: integer centres, radii and normal lengths
    const std::vector<size_t> sph_dfs = dfs_of(sph_bvh);
    std::vector<std::vector<uint32_t>> s_want(nq), s_in(nq);
    size_t s_total = 0;
    for (size_t q = 0; q < nq; ++q)
        for (size_t i : sph_dfs) {
            const Sphere& s = spheres[sph_bvh.prim_ids[i]];
            bool pass = true, in = true;
            for (size_t p = 0; p < m; ++p) {
                const Plane& pl = planes[q * m + p];
                const Scalar len = pl.nx == 3 || pl.nx == -3 ? Scalar(5) : (pl.nx != 0 && pl.nz != 0) ? Scalar(-1) : Scalar((pl.nx != 0) + (pl.nz != 0));
                if (len < 0) { pass = false; break; }                                                                 // (x + z <= 1: no integer length; skipped below)
                const Scalar c = value(pl, s.center), rl = s.radius * len;
                pass = pass && c <= rl;
                in = in && c <= -rl;
            }
            if (pass) { s_want[q].push_back(uint32_t(i)); s_in[q].push_back(in); ++s_total; }
        }
    amd::region_spheres_batch(sph_bvh, d_spheres, std::span<const Plane>(planes), m, offsets, list, &inside);
    {   // (leave the region with the normal (1, 0, 1) out of the comparison)
        std::vector<uint64_t> off(offsets.begin(), offsets.begin() + single_from + 1);
        std::vector<uint32_t> lst(list.begin(), list.begin() + off.back()), flg(inside.begin(), inside.begin() + off.back());
        s_want.resize(single_from);
        s_in.resize(single_from);
        expect(off, lst, s_want, "region_spheres_batch");
        expect(off, flg, s_in, "region_spheres_batch (inside flags)");
    }

    std::printf("%s: %zu triangles, %zu regions list %zu triangles (%zu wholly inside, EXACT %zu) and %zu spheres: %s\n", name, np, nq, total, inside_total,
                exact_total, s_total, bad ? "MISMATCH" : "region_tris == region_spheres == brute force");
    return bad;
}

int main() {
    return run<float>("float") + run<double>("double");
}
