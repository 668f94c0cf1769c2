// Box-overlap queries through the C++20 mirror: bvh::v2::amd::overlap_boxes_batch (device form and host form) and overlap_self_batch on
// a small moving height field, against a brute force written here (closed intervals, listed in the tree's left-first depth-first order).
// The tree is refitted to the moved boxes first, so the lists must equal the brute force exactly. tests/test_gpu_overlap_cpp.py runs it.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
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
    using Node = bvh::v2::Node<Scalar, 3>;
    using Bvh = bvh::v2::Bvh<Node>;
    namespace amd = bvh::v2::amd;
    static_assert(sizeof(BBox) == 6 * sizeof(Scalar));

    const int side = 16;                                      // a 16 x 16 height field, two triangles per cell
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
    const size_t np = tris.size();
    std::vector<BBox> bboxes(np), moved_bboxes(np);
    std::vector<Vec3> centers(np);
    for (size_t i = 0; i < np; ++i) { bboxes[i] = tris[i].get_bbox(); centers[i] = tris[i].get_center(); moved_bboxes[i] = moved[i].get_bbox(); }
    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    Bvh bvh = bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
    amd::DeviceArray<BBox> d_boxes{std::span<const BBox>(moved_bboxes)};
    amd::refit_boxes(bvh, d_boxes);

    std::vector<BBox> queries;                                // cubes of several sizes (one of zero extent per 8), one box over everything, one far away
    for (int k = 0; k < 150; ++k) {
        const Scalar cx = Scalar(-1.0 + 18.0 * ((k * 37) % 150) / 150.0), cy = Scalar(-0.5 + 1.0 * ((k * 53) % 150) / 150.0), cz = Scalar(-1.0 + 18.0 * ((k * 91) % 150) / 150.0);
        const Scalar h = k % 8 == 0 ? Scalar(0) : Scalar(0.25 * (k % 5));
        queries.emplace_back(Vec3(cx - h, cy - h, cz - h), Vec3(cx + h, cy + h, cz + h));
    }
    queries.emplace_back(Vec3(Scalar(-1)), Vec3(Scalar(side + 1)));
    queries.emplace_back(Vec3(Scalar(100)), Vec3(Scalar(101)));
    queries.emplace_back(Vec3(Scalar(3), Scalar(-1), Scalar(3)), Vec3(Scalar(4), Scalar(1), Scalar(4)));     // the faces of a cell: touching counts

    auto overlaps = [](const BBox& a, const BBox& b) {
        for (int k = 0; k < 3; ++k) if (!(a.min[k] <= b.max[k] && b.min[k] <= a.max[k])) return false;
        return true;
    };
    std::vector<size_t> dfs;                                  // BVH-order primitive indices in the walk's order
    std::vector<size_t> stack{0};
    while (!stack.empty()) {
        const Node& node = bvh.nodes[stack.back()];
        stack.pop_back();
        if (node.is_leaf()) { for (size_t i = 0; i < node.index.prim_count(); ++i) dfs.push_back(node.index.first_id() + i); }
        else { stack.push_back(node.index.first_id() + 1); stack.push_back(node.index.first_id()); }
    }
    auto box_of = [&](size_t i) -> const BBox& { return moved_bboxes[bvh.prim_ids[i]]; };

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

    // query boxes: host form, device form (count pass, offsets, fill pass), original ids
    std::vector<std::vector<uint32_t>> want(queries.size()), want_ids(queries.size());
    size_t total = 0;
    for (size_t q = 0; q < queries.size(); ++q)
        for (size_t i : dfs)
            if (overlaps(box_of(i), queries[q])) { want[q].push_back(uint32_t(i)); want_ids[q].push_back(uint32_t(bvh.prim_ids[i])); ++total; }
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> list;
    amd::overlap_boxes_batch(bvh, d_boxes, std::span<const BBox>(queries), offsets, list);
    expect(offsets, list, want, "overlap_boxes_batch (host form)");
    amd::overlap_boxes_batch(bvh, d_boxes, std::span<const BBox>(queries), offsets, list, BVH_AMD_RAY_ORIGINAL_IDS);
    expect(offsets, list, want_ids, "overlap_boxes_batch (original ids)");
    {
        amd::DeviceArray<BBox> d_queries{std::span<const BBox>(queries)};
        amd::DeviceArray<uint32_t> d_counts(queries.size());
        amd::DeviceArray<uint64_t> d_offsets(queries.size() + 1);
        amd::overlap_boxes_batch(bvh, d_boxes, d_queries, &d_counts, nullptr, nullptr);
        bvh::v2::amd::check(bvh_amd_offsets_from_counts(d_counts.data(), queries.size(), d_offsets.data(), nullptr), "offsets_from_counts");
        std::vector<uint64_t> off(queries.size() + 1);
        d_offsets.download(std::span<uint64_t>(off));
        amd::DeviceArray<uint32_t> d_list(off.back() + 1);
        amd::overlap_boxes_batch(bvh, d_boxes, d_queries, nullptr, &d_offsets, &d_list);
        std::vector<uint32_t> got(off.back() + 1);
        d_list.download(std::span<uint32_t>(got));
        got.pop_back();
        expect(off, got, want, "overlap_boxes_batch (device form)");
    }
    if (want[150].size() != np || !want[151].empty() || want[152].size() < 2) { std::printf("%s: the crafted queries list %zu / %zu / %zu\n", name, want[150].size(), want[151].size(), want[152].size()); ++bad; }

    // self mode: row q lists the i > q whose boxes overlap box q
    std::vector<std::vector<uint32_t>> self(np);
    size_t pairs = 0;
    for (size_t q = 0; q < np; ++q)
        for (size_t i : dfs)
            if (i > q && overlaps(box_of(i), box_of(q))) { self[q].push_back(uint32_t(i)); ++pairs; }
    amd::overlap_self_batch(bvh, d_boxes, offsets, list);
    expect(offsets, list, self, "overlap_self_batch");
    if (pairs < np) { std::printf("%s: only %zu pairs\n", name, pairs); ++bad; }

    std::printf("%s: %zu triangles, %zu queries list %zu primitives, %zu self pairs: %s\n", name, np, queries.size(), total, pairs,
                bad ? "MISMATCH" : "overlap_boxes == overlap_self == brute force");
    return bad;
}

int main() {
    return run<float>("float") + run<double>("double");
}
