// Winding numbers through the C++20 mirror (bvh::v2::amd::winding_prepare, winding_numbers_batch, signed_distance_batch): a closed,
// outward-oriented cube of 432 triangles with integer vertices, serial High build, permuted PrecomputedTri, a batch of queries inside and
// outside. Prints the tree's prim ids, then one line per query "w prim t u v" (w, t, u, v as hexadecimal floats: exact);
// tests/test_gpu_winding_cpp.py compares them with the C ABI's results on the same tree.
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
using Query = bvh::v2::amd::PointQuery<Scalar>;

int main() {
    std::vector<Tri> tris;                                    // the six faces of [0, 6]^3, 6 x 6 cells each, normals outward
    const int side = 6;
    for (int a = 0; a < 3; ++a)
        for (int s = 0; s < 2; ++s)
            for (int i = 0; i < side; ++i)
                for (int j = 0; j < side; ++j) {
                    auto corner = [&](int di, int dj) {
                        Scalar p[3];
                        p[a] = Scalar(s * side); p[(a + 1) % 3] = Scalar(i + di); p[(a + 2) % 3] = Scalar(j + dj);
                        return Vec3(p[0], p[1], p[2]);
                    };
                    const Vec3 p00 = corner(0, 0), p10 = corner(1, 0), p11 = corner(1, 1), p01 = corner(0, 1);
                    if (s) { tris.emplace_back(p00, p10, p11); tris.emplace_back(p00, p11, p01); }
                    else   { tris.emplace_back(p00, p11, p10); tris.emplace_back(p00, p01, p11); }
                }
    std::vector<BBox> bboxes(tris.size());
    std::vector<Vec3> centers(tris.size());
    for (size_t i = 0; i < tris.size(); ++i) { bboxes[i] = tris[i].get_bbox(); centers[i] = tris[i].get_center(); }
    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    auto bvh = bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
    auto prims = bvh::v2::amd::permuted_triangles(bvh, std::span<const Tri>(tris));

    std::vector<Query> queries;
    for (int k = 0; k < 200; ++k) {
        const Scalar x = Scalar(-1.5 + 9.0 * ((k * 37) % 200) / 200.0), y = Scalar(-1.5 + 9.0 * ((k * 53) % 200) / 200.0);
        const Scalar z = Scalar(-1.5 + 9.0 * ((k * 91) % 200) / 200.0);
        queries.push_back(Query{ Vec3(x, y, z), Scalar(INFINITY) });
    }
    bvh::v2::amd::DeviceArray<Query> d_queries{std::span<const Query>(queries)};
    bvh::v2::amd::DeviceArray<Scalar> moments((bvh.nodes.size() + 1) * 8), d_w(queries.size());
    bvh::v2::amd::DeviceArray<Hit> d_hits(queries.size());
    bvh::v2::amd::winding_prepare(bvh, prims, moments);
    bvh::v2::amd::winding_numbers_batch(bvh, prims, moments, d_queries, d_w, 2.0);
    bvh::v2::amd::signed_distance_batch(bvh, prims, moments, d_queries, d_hits, 2.0);
    std::vector<Scalar> w(queries.size());
    std::vector<Hit> hits(queries.size());
    d_w.download(w);
    d_hits.download(hits);

    std::printf("prim_ids:");
    for (size_t id : bvh.prim_ids) std::printf(" %zu", id);
    std::printf("\n");
    for (size_t k = 0; k < queries.size(); ++k)
        std::printf("%a %u %a %a %a\n", double(w[k]), hits[k].prim, double(hits[k].t), double(hits[k].u), double(hits[k].v));
    return 0;
}
