// k-nearest queries through the C++20 mirror (bvh::v2::amd::knn_batch): the small deterministic mesh of radius_search_amd.cpp, serial
// High build, permuted PrecomputedTri, the same batch of queries of three radii, k = 6. Prints the tree's prim ids, the counts, then
// one line per slot "query slot prim distance" (the distance as a hexadecimal float: exact); tests/test_gpu_knn.py compares them with
// bvh_amd.knn. Also runs the device form without the optional outputs and checks it against the host form.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/tri.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

using Scalar = float;
using Vec3 = bvh::v2::Vec<Scalar, 3>;
using BBox = bvh::v2::BBox<Scalar, 3>;
using Tri = bvh::v2::Tri<Scalar, 3>;
using Node = bvh::v2::Node<Scalar, 3>;
using Bvh = bvh::v2::Bvh<Node>;
using Query = bvh::v2::amd::PointQuery<Scalar>;
template <typename T> using DeviceArray = bvh::v2::amd::DeviceArray<T>;
static_assert(sizeof(Query) == 4 * sizeof(Scalar));

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

    std::vector<Query> queries;
    const Scalar radii[3] = { Scalar(0.25), Scalar(1.5), Scalar(INFINITY) };
    for (int k = 0; k < 200; ++k) {
        const Scalar x = Scalar(-1.5 + 15.0 * ((k * 37) % 200) / 200.0), y = Scalar(-1.0 + 2.0 * ((k * 53) % 200) / 200.0);
        const Scalar z = Scalar(-1.5 + 15.0 * ((k * 91) % 200) / 200.0);
        queries.push_back(Query{ Vec3(x, y, z), k % 50 == 49 ? radii[2] : radii[k % 2] });
    }
    const unsigned k = 6;
    std::vector<uint32_t> ids, counts;
    std::vector<Scalar> dist;
    bvh::v2::amd::knn_batch(bvh, prims, std::span<const Query>(queries), k, ids, &dist, &counts);

    // the device form, ids only: the same rows
    const size_t n = queries.size();
    DeviceArray<Query> d_queries{std::span<const Query>(queries)};
    DeviceArray<uint32_t> d_ids(n * k);
    bvh::v2::amd::knn_batch(bvh, prims, d_queries, k, d_ids);
    std::vector<uint32_t> ids2(n * k);
    d_ids.download(std::span<uint32_t>(ids2));
    if (ids2 != ids) { std::fprintf(stderr, "device form: rows differ from the host form's\n"); return 1; }

    std::printf("prim_ids:");
    for (size_t id : bvh.prim_ids) std::printf(" %zu", id);
    std::printf("\ncounts:");
    for (uint32_t c : counts) std::printf(" %u", c);
    std::printf("\n");
    for (size_t q = 0; q < n; ++q)
        for (unsigned s = 0; s < k; ++s) std::printf("%zu %u %u %a\n", q, s, ids[q * k + s], double(dist[q * k + s]));
    return 0;
}
