// Instanced ray queries through the C++20 mirror: bvh::v2::amd::instance_prepare and intersect_instanced_batch on a small two-level
// scene (a height field and a tetrahedron, placed 24 times), against a brute force written here with the mirror's own
// PrecomputedTri::intersect: every ray carried into every instance's object space by the prepared inverse, every triangle tested. Then
// every instance moves, the top tree is refitted to the new boxes (no geometry is touched) and the scene is traced again.
// tests/test_gpu_instanced_cpp.py runs it.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/ray.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/tri.h>

#include <cmath>
#include <cstdio>
#include <vector>

template <typename Scalar>
static int run(const char* name) {
    using Vec3 = bvh::v2::Vec<Scalar, 3>;
    using BBox = bvh::v2::BBox<Scalar, 3>;
    using Tri = bvh::v2::Tri<Scalar, 3>;
    using PTri = bvh::v2::PrecomputedTri<Scalar>;
    using Ray = bvh::v2::Ray<Scalar, 3>;
    using Node = bvh::v2::Node<Scalar, 3>;
    using Bvh = bvh::v2::Bvh<Node>;
    namespace amd = bvh::v2::amd;
    using Affine = amd::Affine<Scalar>;
    using Hit = amd::Hit<Scalar>;

    // two geometries around the origin: an 8 x 8 height field, and a tetrahedron
    std::vector<std::vector<Tri>> meshes(2);
    const int side = 8;
    auto height = [](int i, int j) { return static_cast<Scalar>(0.2 * std::sin(0.9 * i) * std::cos(0.6 * j)); };
    auto corner = [&](int i, int j) { return Vec3(Scalar(i - side / 2) / Scalar(side / 2), height(i, j), Scalar(j - side / 2) / Scalar(side / 2)); };
    for (int i = 0; i < side; ++i)
        for (int j = 0; j < side; ++j) {
            meshes[0].emplace_back(corner(i, j), corner(i + 1, j), corner(i + 1, j + 1));
            meshes[0].emplace_back(corner(i, j), corner(i + 1, j + 1), corner(i, j + 1));
        }
    const Vec3 a(Scalar(1), Scalar(1), Scalar(1)), b(Scalar(1), Scalar(-1), Scalar(-1)), c(Scalar(-1), Scalar(1), Scalar(-1)), d(Scalar(-1), Scalar(-1), Scalar(1));
    meshes[1] = { Tri(a, b, c), Tri(a, c, d), Tri(a, d, b), Tri(b, d, c) };

    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    std::vector<Bvh> trees;
    std::vector<amd::DeviceArray<PTri>> d_prims;
    std::vector<std::vector<PTri>> prims(2);                  // BVH order, for the brute force
    for (size_t g = 0; g < 2; ++g) {
        std::vector<BBox> bboxes;
        std::vector<Vec3> centers;
        for (const Tri& t : meshes[g]) { bboxes.push_back(t.get_bbox()); centers.push_back(t.get_center()); }
        trees.push_back(bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config));
    }
    for (size_t g = 0; g < 2; ++g) {
        d_prims.push_back(amd::permuted_triangles(trees[g], std::span<const Tri>(meshes[g])));
        for (size_t i = 0; i < meshes[g].size(); ++i) { const Tri& t = meshes[g][trees[g].prim_ids[i]]; prims[g].emplace_back(t.p0, t.p1, t.p2); }
    }
    const std::vector<amd::Geometry<Node>> geoms = { { &trees[0], &d_prims[0] }, { &trees[1], &d_prims[1] } };
    const std::span<const amd::Geometry<Node>> geom_span(geoms);

    // 24 instances on a ring: rotation about y x non-uniform scale, and a translation; `phase` moves all of them
    const size_t n_inst = 24;
    std::vector<uint32_t> geometry(n_inst);
    for (size_t k = 0; k < n_inst; ++k) geometry[k] = static_cast<uint32_t>(k % 2);
    auto placement = [&](double phase) {
        std::vector<Affine> m(n_inst);
        for (size_t k = 0; k < n_inst; ++k) {
            const double ang = 0.7 * k + phase, co = std::cos(ang), si = std::sin(ang), sx = 0.8 + 0.05 * (k % 5), sy = 1.2 - 0.04 * (k % 7), sz = 0.9 + 0.03 * (k % 3);
            const double ring = 2.0 * 3.14159265358979 * k / n_inst + 0.5 * phase, radius = 6.0 + 1.5 * std::sin(3 * ring + phase);
            const double rows[12] = { co * sx, 0.0, si * sz, radius * std::cos(ring), 0.1 * sx, sy, 0.0, 0.8 * std::sin(2 * ring), -si * sx, 0.0, co * sz, radius * std::sin(ring) };
            for (int e = 0; e < 12; ++e) m[k].m[e] = static_cast<Scalar>(rows[e]);
        }
        return m;
    };

    std::vector<Ray> rays;                                    // from a point above the ring's centre towards a grid across the scene
    for (int i = 0; i < 48; ++i)
        for (int j = 0; j < 48; ++j) {
            const Vec3 org(Scalar(0.3), Scalar(5), Scalar(-0.2));
            const Vec3 target(Scalar(-9.0 + 18.0 * (i + 0.37) / 48), Scalar(0), Scalar(-9.0 + 18.0 * (j + 0.61) / 48));
            rays.emplace_back(org, target - org, Scalar(0), Scalar(1.5));
        }
    amd::DeviceArray<Ray> d_rays{std::span<const Ray>(rays)};
    amd::DeviceArray<uint32_t> d_geometry{std::span<const uint32_t>(geometry)};
    amd::DeviceArray<Hit> d_hits(rays.size());
    amd::DeviceArray<uint32_t> d_inst(rays.size());
    amd::DeviceArray<Affine> d_world2obj;
    amd::DeviceArray<BBox> d_bboxes;
    amd::DeviceArray<Vec3> d_centers;

    int bad = 0;
    size_t hits_total = 0;
    Bvh top;
    for (int frame = 0; frame < 2; ++frame) {
        const std::vector<Affine> placed = placement(0.8 * frame);
        amd::DeviceArray<Affine> d_obj2world{std::span<const Affine>(placed)};
        amd::instance_prepare(geom_span, d_obj2world, &d_geometry, d_world2obj, d_bboxes, d_centers);
        std::vector<Affine> w(n_inst);
        d_world2obj.download(std::span<Affine>(w));
        if (frame == 0) {
            std::vector<BBox> bboxes(n_inst);
            std::vector<Vec3> centers(n_inst);
            d_bboxes.download(std::span<BBox>(bboxes));
            d_centers.download(std::span<Vec3>(centers));
            top = bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
        } else {
            amd::refit_boxes(top, d_bboxes);                  // rigid motion: the small top tree is refitted, nothing else
        }
        amd::intersect_instanced_batch<false, true>(top, geom_span, d_world2obj, &d_geometry, d_rays, d_hits, d_inst);
        std::vector<Hit> hits(rays.size());
        std::vector<uint32_t> inst(rays.size());
        d_hits.download(std::span<Hit>(hits));
        d_inst.download(std::span<uint32_t>(inst));
        amd::intersect_instanced_batch<true, false>(top, geom_span, d_world2obj, &d_geometry, d_rays, d_hits, d_inst);
        std::vector<Hit> any(rays.size());
        d_hits.download(std::span<Hit>(any));

        for (size_t r = 0; r < rays.size(); ++r) {            // brute force: the nearest accepted hit over all instances and triangles
            Scalar best = rays[r].tmax;
            bool found = false;
            for (size_t k = 0; k < n_inst; ++k) {
                const Scalar* m = w[k].m;
                Ray local = rays[r];
                for (int e = 0; e < 3; ++e) {
                    local.org[e] = ((Scalar(0) + m[4 * e] * rays[r].org[0]) + m[4 * e + 1] * rays[r].org[1]) + m[4 * e + 2] * rays[r].org[2] + m[4 * e + 3];
                    local.dir[e] = ((Scalar(0) + m[4 * e] * rays[r].dir[0]) + m[4 * e + 1] * rays[r].dir[1]) + m[4 * e + 2] * rays[r].dir[2];
                }
                local.tmax = best;
                for (const PTri& tri : prims[geometry[k]])
                    if (auto h = tri.intersect(local)) { best = std::get<0>(*h); local.tmax = best; found = true; }
            }
            const bool hit = hits[r].prim != Hit::invalid;
            // the nearest t is the same whatever the order, up to the rounding of a ray that meets two instances at one t
            const bool ok = hit == found && (hit ? std::abs(hits[r].t - best) <= Scalar(1e-5) * best && inst[r] < n_inst && hits[r].prim < prims[geometry[inst[r]]].size()
                                                 : inst[r] == BVH_AMD_INVALID && hits[r].t == rays[r].tmax);
            if (!ok || (any[r].prim != Hit::invalid) != found) {
                if (bad < 5) std::printf("%s: frame %d ray %zu: hit %d t %g instance %u, brute force %d t %g\n", name, frame, r, int(hit), double(hits[r].t), inst[r], int(found), double(best));
                ++bad;
            }
            hits_total += hit;
        }
    }
    if (hits_total < rays.size() / 4 || hits_total >= 2 * rays.size()) { std::printf("%s: %zu hits in two frames of %zu rays\n", name, hits_total, rays.size()); ++bad; }
    std::printf("%s: %zu instances of 2 geometries, 2 frames of %zu rays, %zu hits: %s\n", name, n_inst, rays.size(), hits_total,
                bad ? "MISMATCH" : "intersect_instanced == brute force");
    return bad;
}

int main() {
    return run<float>("float") + run<double>("double");
}
