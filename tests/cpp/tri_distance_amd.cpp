// Triangle-distance queries through the C++20 mirror (bvh::v2::amd::tri_distance_batch, host form over the device form): a small
// deterministic height field, serial High build, the triangles by original id on the device, a batch of query triangles (every 5th a
// segment {a, b, b}: the capsule recipe) with one max_distance per query and the query barycentrics asked for, then the first 50 of
// them again with one max_distance for all and original ids. Prints the tree's prim ids, then one line per record "prim t u v s w"
// (hexadecimal floats: exact; s, w only in the first part); tests/test_gpu_tri_distance_cpp.py compares them with
// bvh_amd.tri_distance.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
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
using Hit = bvh::v2::amd::Hit<Scalar>;

int main() {
    namespace amd = bvh::v2::amd;
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
    amd::DeviceArray<Tri> d_tris{std::span<const Tri>(tris)};

    std::vector<Tri> queries;
    std::vector<Scalar> limits;
    for (int k = 0; k < 200; ++k) {
        const Scalar x = Scalar(-1.5 + 15.0 * ((k * 37) % 200) / 200.0), y = Scalar(-0.25 + 1.0 * ((k * 53) % 200) / 200.0);
        const Scalar z = Scalar(-1.5 + 15.0 * ((k * 91) % 200) / 200.0);
        const Scalar dx = Scalar(-0.5 + 1.0 * ((k * 29) % 200) / 200.0), dz = Scalar(-0.5 + 1.0 * ((k * 71) % 200) / 200.0);
        const Vec3 a(x, y, z), b(x + dx, y - Scalar(0.25), z + dz), c(x - dz, y + Scalar(0.125), z + dx);
        queries.emplace_back(a, b, k % 5 ? c : b);
        limits.push_back(k % 3 ? Scalar(INFINITY) : Scalar(0.25));
    }
    std::vector<Hit> hits, hits_one;
    std::vector<Scalar> uv;
    amd::tri_distance_batch(bvh, d_tris, std::span<const Tri>(queries), std::span<const Scalar>(limits), hits, &uv);
    const Scalar one = Scalar(0.5);
    amd::tri_distance_batch(bvh, d_tris, std::span<const Tri>(queries.data(), 50), std::span<const Scalar>(&one, 1), hits_one, nullptr, BVH_AMD_RAY_ORIGINAL_IDS);

    std::printf("prim_ids:");
    for (size_t id : bvh.prim_ids) std::printf(" %zu", id);
    std::printf("\n");
    for (size_t k = 0; k < hits.size(); ++k)
        std::printf("%u %a %a %a %a %a\n", hits[k].prim, double(hits[k].t), double(hits[k].u), double(hits[k].v), double(uv[2 * k]), double(uv[2 * k + 1]));
    for (const Hit& hit : hits_one) std::printf("%u %a %a %a\n", hit.prim, double(hit.t), double(hit.u), double(hit.v));
    return 0;
}
