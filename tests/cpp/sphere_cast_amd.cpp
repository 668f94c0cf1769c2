// Sphere-cast queries through the C++20 mirror (bvh::v2::amd::sphere_cast_batch, host form): a small deterministic mesh, serial High
// build, permuted PrecomputedTri, a batch of rays with one radius per ray, then the first 50 of them again with one radius for all
// and the robust box test. Prints the tree's prim ids, then one line per record "prim t u v" (t, u, v as hexadecimal floats: exact);
// tests/test_gpu_sphere_cast_cpp.py compares them with bvh_amd.sphere_cast.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/ray.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/tri.h>

#include <cmath>
#include <cstdio>
#include <vector>

using Scalar = float;
using Vec3 = bvh::v2::Vec<Scalar, 3>;
using BBox = bvh::v2::BBox<Scalar, 3>;
using Tri = bvh::v2::Tri<Scalar, 3>;
using Node = bvh::v2::Node<Scalar, 3>;
using Bvh = bvh::v2::Bvh<Node>;
using Ray = bvh::v2::Ray<Scalar, 3>;
using Hit = bvh::v2::amd::Hit<Scalar>;

int main() {
    std::vector<Tri> tris;                                    // a 12 x 12 height field, two triangles per cell
    const int side = 12;
    auto h = [](int i, int j) { return static_cast<Scalar>(0.1 * std::sin(0.7 * i) * std::cos(0.4 * j)); };
    for (int i = 0; i < side; ++i)
        for (int j = 0; j < side; ++j) {
            const Vec3 a(Scalar(i), h(i, j), Scalar(j)), b(Scalar(i + 1), h(i + 1, j), Scalar(j));
            const Vec3 c(Scalar(i + 1), h(i + 1, j + 1), Scalar(j + 1)), d(Scalar(i), h(i, j + 1), Scalar(j + 1));
            tris.emplace_back(a, b, c);
            tris.emplace_back(a, c, d);
        }
    std::vector<BBox> bboxes(tris.size());
    std::vector<Vec3> centers(tris.size());
    for (size_t i = 0; i < tris.size(); ++i) { bboxes[i] = tris[i].get_bbox(); centers[i] = tris[i].get_center(); }
    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    auto bvh = bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
    auto prims = bvh::v2::amd::permuted_triangles(bvh, std::span<const Tri>(tris));

    std::vector<Ray> rays;
    std::vector<Scalar> radii;
    for (int k = 0; k < 200; ++k) {
        const Scalar x = Scalar(-1.5 + 15.0 * ((k * 37) % 200) / 200.0), y = Scalar(0.5 + 2.0 * ((k * 53) % 200) / 200.0);
        const Scalar z = Scalar(-1.5 + 15.0 * ((k * 91) % 200) / 200.0);
        const Scalar dx = Scalar(-1.0 + 2.0 * ((k * 29) % 200) / 200.0), dz = Scalar(-1.0 + 2.0 * ((k * 71) % 200) / 200.0);
        rays.emplace_back(Vec3(x, y, z), Vec3(dx, Scalar(-1), dz), Scalar(0), k % 3 ? Scalar(INFINITY) : Scalar(1));
        radii.push_back(Scalar(0.125) * Scalar(k % 5));
    }
    std::vector<Hit> hits, hits_one;
    bvh::v2::amd::sphere_cast_batch<false>(bvh, prims, std::span<const Ray>(rays), std::span<const Scalar>(radii), hits);
    const Scalar one = Scalar(0.25);
    bvh::v2::amd::sphere_cast_batch<true>(bvh, prims, std::span<const Ray>(rays.data(), 50), std::span<const Scalar>(&one, 1), hits_one);

    std::printf("prim_ids:");
    for (size_t id : bvh.prim_ids) std::printf(" %zu", id);
    std::printf("\n");
    for (const Hit& hit : hits) std::printf("%u %a %a %a\n", hit.prim, double(hit.t), double(hit.u), double(hit.v));
    for (const Hit& hit : hits_one) std::printf("%u %a %a %a\n", hit.prim, double(hit.t), double(hit.u), double(hit.v));
    return 0;
}
