// Triangle-intersection queries through the C++20 mirror: bvh::v2::amd::intersect_tris_batch (device form and host form) and
// intersect_tris_self_batch on two small moving height fields that pass through each other, against a brute force written here: a
// separating-axis test in integers (the coordinates are small integers, so the library's determinants are exact and the lists must
// equal the brute force exactly), listed in the tree's left-first depth-first order. The tree is refitted to the moved triangles
// first. tests/test_gpu_tri_intersect_cpp.py runs it.
#include <bvh/v2/bvh.h>
#include <bvh/v2/vec.h>
#include <bvh/v2/node.h>
#include <bvh/v2/default_builder.h>
#include <bvh/v2/tri.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <vector>

using I3 = std::array<long long, 3>;
using ITri = std::array<I3, 3>;

static I3 sub(const I3& a, const I3& b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
static I3 cross(const I3& a, const I3& b) { return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}; }
static long long dot(const I3& a, const I3& b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static bool zero(const I3& a) { return a[0] == 0 && a[1] == 0 && a[2] == 0; }

// closed triangles intersect iff none of the 17 axes separates them strictly; a triangle without area intersects nothing
static bool sat(const ITri& a, const ITri& b) {
    const I3 ea[3] = {sub(a[1], a[0]), sub(a[2], a[1]), sub(a[0], a[2])}, eb[3] = {sub(b[1], b[0]), sub(b[2], b[1]), sub(b[0], b[2])};
    const I3 na = cross(ea[0], ea[1]), nb = cross(eb[0], eb[1]);
    if (zero(na) || zero(nb)) return false;
    std::vector<I3> axes{na, nb};
    for (const I3& u : ea) for (const I3& v : eb) axes.push_back(cross(u, v));
    for (const I3& u : ea) axes.push_back(cross(na, u));
    for (const I3& v : eb) axes.push_back(cross(nb, v));
    for (const I3& ax : axes) {
        if (zero(ax)) continue;
        const long long pa[3] = {dot(ax, a[0]), dot(ax, a[1]), dot(ax, a[2])}, pb[3] = {dot(ax, b[0]), dot(ax, b[1]), dot(ax, b[2])};
        if (*std::max_element(pa, pa + 3) < *std::min_element(pb, pb + 3) || *std::max_element(pb, pb + 3) < *std::min_element(pa, pa + 3)) return false;
    }
    return true;
}

static bool shares(const ITri& a, const ITri& b) {
    for (const I3& p : a) for (const I3& q : b) if (p == q) return true;
    return false;
}

template <typename Scalar>
static int run(const char* name) {
    using Vec3 = bvh::v2::Vec<Scalar, 3>;
    using BBox = bvh::v2::BBox<Scalar, 3>;
    using Tri = bvh::v2::Tri<Scalar, 3>;
    using Node = bvh::v2::Node<Scalar, 3>;
    using Bvh = bvh::v2::Bvh<Node>;
    namespace amd = bvh::v2::amd;
    static_assert(sizeof(Tri) == 9 * sizeof(Scalar));

    const int side = 10;                                      // two 10 x 10 height fields, two triangles per cell, on interleaved integer grids
    auto height = [](int i, int j, int phase, int sheet) { return (long long)((i * (sheet ? 5 : 7) + j * (sheet ? 11 : 3) + phase) % 5) - 2; };
    auto mesh = [&](int phase, int shift) {
        std::vector<ITri> tris;
        for (int sheet = 0; sheet < 2; ++sheet)
            for (int i = 0; i < side; ++i)
                for (int j = 0; j < side; ++j) {
                    auto at = [&](int ii, int jj) { return I3{2 * ii + sheet + shift, height(ii, jj, phase, sheet), 2 * jj + sheet}; };
                    tris.push_back({at(i, j), at(i + 1, j), at(i + 1, j + 1)});
                    tris.push_back({at(i, j), at(i + 1, j + 1), at(i, j + 1)});
                }
        return tris;
    };
    auto as_tris = [](const std::vector<ITri>& it) {
        std::vector<Tri> out;
        for (const ITri& t : it)
            out.emplace_back(Vec3(Scalar(t[0][0]), Scalar(t[0][1]), Scalar(t[0][2])), Vec3(Scalar(t[1][0]), Scalar(t[1][1]), Scalar(t[1][2])),
                             Vec3(Scalar(t[2][0]), Scalar(t[2][1]), Scalar(t[2][2])));
        return out;
    };
    const std::vector<ITri> rest = mesh(0, 0), moved = mesh(3, 0);
    std::vector<ITri> queries_i = mesh(1, 1);                 // a third pose, one unit along x
    queries_i.resize(150);
    for (size_t k = 0; k < 10; ++k) queries_i[k] = moved[17 * k];                           // ... and some of the moved mesh's own triangles: shared vertices
    queries_i.push_back({I3{100, 0, 0}, I3{101, 0, 0}, I3{100, 1, 0}});                    // far away
    queries_i.push_back({I3{-50, -1, -50}, I3{90, -1, -50}, I3{-50, -1, 90}});              // a sheet through everything
    queries_i.push_back({I3{0, 0, 0}, I3{2, 2, 2}, I3{4, 4, 4}});                           // no area: intersects nothing
    const std::vector<Tri> tris = as_tris(rest), moved_tris = as_tris(moved), queries = as_tris(queries_i);
    const size_t np = tris.size();
    std::vector<BBox> bboxes(np);
    std::vector<Vec3> centers(np);
    for (size_t i = 0; i < np; ++i) { bboxes[i] = tris[i].get_bbox(); centers[i] = tris[i].get_center(); }
    typename bvh::v2::DefaultBuilder<Node>::Config config;
    config.quality = bvh::v2::DefaultBuilder<Node>::Quality::High;
    Bvh bvh = bvh::v2::DefaultBuilder<Node>::build(bboxes, centers, config);
    amd::DeviceArray<Tri> d_tris{std::span<const Tri>(moved_tris)};
    amd::DeviceArray<bvh::v2::PrecomputedTri<Scalar>> d_pre;
    amd::refit_tris(bvh, d_tris, d_pre);

    std::vector<size_t> dfs;                                  // BVH-order primitive indices in the walk's order
    std::vector<size_t> stack{0};
    while (!stack.empty()) {
        const Node& node = bvh.nodes[stack.back()];
        stack.pop_back();
        if (node.is_leaf()) { for (size_t i = 0; i < node.index.prim_count(); ++i) dfs.push_back(node.index.first_id() + i); }
        else { stack.push_back(node.index.first_id() + 1); stack.push_back(node.index.first_id()); }
    }
    auto tri_of = [&](size_t i) -> const ITri& { return moved[bvh.prim_ids[i]]; };

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

    // query triangles: host form, device form (count pass, offsets, fill pass), original ids, without pairs that share a vertex
    const size_t nq = queries.size();
    std::vector<std::vector<uint32_t>> want(nq), want_ids(nq), want_skip(nq);
    size_t total = 0, total_skip = 0;
    for (size_t q = 0; q < nq; ++q)
        for (size_t i : dfs)
            if (sat(queries_i[q], tri_of(i))) {
                want[q].push_back(uint32_t(i)); want_ids[q].push_back(uint32_t(bvh.prim_ids[i])); ++total;
                if (!shares(queries_i[q], tri_of(i))) { want_skip[q].push_back(uint32_t(i)); ++total_skip; }
            }
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> list;
    amd::intersect_tris_batch(bvh, d_tris, std::span<const Tri>(queries), offsets, list);
    expect(offsets, list, want, "intersect_tris_batch (host form)");
    amd::intersect_tris_batch(bvh, d_tris, std::span<const Tri>(queries), offsets, list, BVH_AMD_RAY_ORIGINAL_IDS);
    expect(offsets, list, want_ids, "intersect_tris_batch (original ids)");
    amd::intersect_tris_batch(bvh, d_tris, std::span<const Tri>(queries), offsets, list, BVH_AMD_TRI_SKIP_SHARED);
    expect(offsets, list, want_skip, "intersect_tris_batch (skip shared)");
    {
        amd::DeviceArray<Tri> d_queries{std::span<const Tri>(queries)};
        amd::DeviceArray<uint32_t> d_counts(nq);
        amd::DeviceArray<uint64_t> d_offsets(nq + 1);
        amd::intersect_tris_batch(bvh, d_tris, d_queries, &d_counts, nullptr, nullptr);
        bvh::v2::amd::check(bvh_amd_offsets_from_counts(d_counts.data(), nq, d_offsets.data(), nullptr), "offsets_from_counts");
        std::vector<uint64_t> off(nq + 1);
        d_offsets.download(std::span<uint64_t>(off));
        amd::DeviceArray<uint32_t> d_list(off.back() + 1);
        amd::intersect_tris_batch(bvh, d_tris, d_queries, nullptr, &d_offsets, &d_list);
        std::vector<uint32_t> got(off.back() + 1);
        d_list.download(std::span<uint32_t>(got));
        got.pop_back();
        expect(off, got, want, "intersect_tris_batch (device form)");
    }
    if (!want[150].empty() || want[151].size() < 20 || !want[152].empty() || total_skip == total || total_skip == 0) {
        std::printf("%s: the crafted queries list %zu / %zu / %zu, %zu of %zu without shared vertices\n", name, want[150].size(), want[151].size(), want[152].size(), total_skip, total);
        ++bad;
    }

    // self mode: row q lists the i > q whose triangles intersect triangle q; with and without the mesh's own neighbours
    std::vector<std::vector<uint32_t>> self(np), self_skip(np);
    size_t pairs = 0, pairs_skip = 0;
    for (size_t q = 0; q < np; ++q)
        for (size_t i : dfs)
            if (i > q && sat(tri_of(q), tri_of(i))) {
                self[q].push_back(uint32_t(i)); ++pairs;
                if (!shares(tri_of(q), tri_of(i))) { self_skip[q].push_back(uint32_t(i)); ++pairs_skip; }
            }
    amd::intersect_tris_self_batch(bvh, d_tris, offsets, list);
    expect(offsets, list, self, "intersect_tris_self_batch");
    amd::intersect_tris_self_batch(bvh, d_tris, offsets, list, BVH_AMD_TRI_SKIP_SHARED);
    expect(offsets, list, self_skip, "intersect_tris_self_batch (skip shared)");
    if (pairs < np || pairs_skip == 0 || pairs_skip >= pairs) { std::printf("%s: %zu pairs, %zu without shared vertices\n", name, pairs, pairs_skip); ++bad; }

    std::printf("%s: %zu triangles, %zu queries list %zu triangles, %zu self pairs (%zu without shared vertices): %s\n", name, np, nq, total, pairs, pairs_skip,
                bad ? "MISMATCH" : "intersect_tris == intersect_tris_self == brute force");
    return bad;
}

int main() {
    return run<float>("float") + run<double>("double");
}
