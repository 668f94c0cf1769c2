// Moving geometry through the C++20 mirror: the loop a user of the reference writes —
//     bvh.refit([&](Node& leaf) { box = BBox::make_empty(); for (i in leaf) box.extend(bboxes[prim_ids[i]]); leaf.set_bbox(box); });
// — on the host mirror of one tree, against bvh::v2::amd::refit_tris (and refit_boxes) on a copy of it, where the fold runs on the
// device from primitives in HBM. The trees must compare equal (operator== and byte for byte), and so must the BVH-order
// PrecomputedTri arrays. tests/test_gpu_refit_prims_cpp.py runs it.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/tri.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

template <typename Scalar>
static int run(const char* name) {
    using Vec3 = bvh::v2::Vec<Scalar, 3>;
    using BBox = bvh::v2::BBox<Scalar, 3>;
    using Tri = bvh::v2::Tri<Scalar, 3>;
    using PrecomputedTri = bvh::v2::PrecomputedTri<Scalar>;
    using Node = bvh::v2::Node<Scalar, 3>;
    using Bvh = bvh::v2::Bvh<Node>;
    namespace amd = bvh::v2::amd;
    static_assert(sizeof(Tri) == 9 * sizeof(Scalar) && sizeof(PrecomputedTri) == 12 * sizeof(Scalar) && sizeof(BBox) == 6 * sizeof(Scalar));

    const int side = 24;                                      // a 24 x 24 height field, two triangles per cell
    auto height = [](int i, int j, double phase) { return static_cast<Scalar>(0.3 * std::sin(0.7 * i + phase) * std::cos(0.4 * j - phase)); };
    auto mesh = [&](double phase) {
        std::vector<Tri> tris;
        for (int i = 0; i < side; ++i)
            for (int j = 0; j < side; ++j) {
                const Vec3 a(Scalar(i), height(i, j, phase), Scalar(j)), b(Scalar(i + 1), height(i + 1, j, phase), Scalar(j));
                const Vec3 c(Scalar(i + 1), height(i + 1, j + 1, phase), Scalar(j + 1)), d(Scalar(i), height(i, j + 1, phase), Scalar(j + 1));
                tris.emplace_back(a, b, c);
                tris.emplace_back(a, c, d);
            }
        return tris;
    };
    const std::vector<Tri> tris = mesh(0.0), moved = mesh(0.9);
    std::vector<BBox> bboxes(tris.size()), moved_bboxes(tris.size());
    std::vector<Vec3> centers(tris.size());
    for (size_t i = 0; i < tris.size(); ++i) { bboxes[i] = tris[i].get_bbox(); centers[i] = tris[i].get_center(); moved_bboxes[i] = moved[i].get_bbox(); }
    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    auto build = [&] { return bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config); };
    Bvh on_host = build(), from_tris = build(), from_boxes = build();
    if (!(on_host == from_tris)) { std::printf("%s: two builds of the same input differ\n", name); return 1; }
    const double cost_before = amd::traversal_cost(from_tris);

    // the reference user's loop, on the host mirror
    on_host.refit([&](Node& leaf) {
        BBox box = BBox::make_empty();
        for (size_t i = leaf.index.first_id(); i < leaf.index.first_id() + leaf.index.prim_count(); ++i) box.extend(moved_bboxes[on_host.prim_ids[i]]);
        leaf.set_bbox(box);
    });
    // the device's
    amd::DeviceArray<Tri> d_moved{std::span<const Tri>(moved)};
    amd::DeviceArray<PrecomputedTri> d_prims;
    amd::refit_tris(from_tris, d_moved, d_prims);
    amd::DeviceArray<BBox> d_boxes{std::span<const BBox>(moved_bboxes)};
    amd::refit_boxes(from_boxes, d_boxes);

    int bad = 0;
    auto same = [&](const Bvh& a, const Bvh& b, const char* what) {
        const bool eq = a == b && a.nodes.size() == b.nodes.size() && std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(Node)) == 0;
        if (!eq) { std::printf("%s: %s differs from the host loop\n", name, what); ++bad; }
    };
    same(on_host, from_tris, "amd::refit_tris");
    same(on_host, from_boxes, "amd::refit_boxes");
    if (on_host == build()) { std::printf("%s: the refit changed nothing\n", name); ++bad; }

    std::vector<PrecomputedTri> want(tris.size()), got(tris.size());
    for (size_t i = 0; i < tris.size(); ++i) want[i] = PrecomputedTri(moved[on_host.prim_ids[i]]);
    if (d_prims.size() != tris.size()) { std::printf("%s: %zu precomputed triangles\n", name, d_prims.size()); return 1; }
    d_prims.download(std::span<PrecomputedTri>(got));
    if (std::memcmp(want.data(), got.data(), want.size() * sizeof(PrecomputedTri)) != 0) { std::printf("%s: PrecomputedTri arrays differ\n", name); ++bad; }

    const double cost_after = amd::traversal_cost(from_tris);
    if (!(cost_before > 0.0 && cost_after > 0.0)) { std::printf("%s: traversal_cost %g -> %g\n", name, cost_before, cost_after); ++bad; }
    std::printf("%s: %zu nodes, %zu triangles, traversal cost %.4f -> %.4f: %s\n", name, on_host.nodes.size(), tris.size(), cost_before, cost_after,
                bad ? "MISMATCH" : "refit_tris == refit_boxes == host loop");
    return bad;
}

int main() {
    return run<float>("float") + run<double>("double");
}
