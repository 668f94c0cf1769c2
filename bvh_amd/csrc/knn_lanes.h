// The block size of the kernels that keep k candidates per lane in dynamic LDS (knn.hip, ray_nearest.hip), once. Expects common.h and
// trace_device.h (kBlock, kWave) to have been included.
#pragma once

#include <algorithm>

#include "knn_heap.inc"

namespace bvh_amd {

namespace {

// Lanes per block (knn_heap.inc has the LDS layout): of 256 / 128 / 64, the size that keeps the most lanes resident on a CU — whole
// blocks of (k + kKnnLds) * (sizeof(T) + 4) bytes per lane in the 160 KB of LDS, a block within 64 KB, at most 8 waves per SIMD — ties to the larger block. The
// LDS a lane needs is fixed by k; the block size only decides how much of the CU's LDS the rounding to whole blocks wastes, so the
// choice is not monotonic in k: floats take 256 lanes at k = 1, 8, 17, 128 at k = 9, 32 and 64 at k = 16, 33 .. 64; doubles 256 at
// k = 5, 9, 128 at k = 7, 16, 17 and 64 at k = 1, 8, 32 .. 64 ("k-nearest queries", has the table).
constexpr size_t kKnnBlockLds = size_t{64} << 10;
constexpr size_t kKnnCuLds = size_t{160} << 10;
constexpr size_t kKnnCuLanes = 8 * 4 * kWave;
template <typename T>
unsigned knn_block_lanes(unsigned k) {
    unsigned best = kWave;
    size_t best_resident = 0;
    for (unsigned lanes = kBlock; lanes >= unsigned(kWave); lanes /= 2) {
        const size_t bytes = knn_lds_bytes<T>(k, lanes);
        if (bytes > kKnnBlockLds) continue;
        const size_t resident = std::min(kKnnCuLds / bytes * lanes, kKnnCuLanes);
        if (resident > best_resident) { best = lanes; best_resident = resident; }
    }
    return best;
}

} // namespace

} // namespace bvh_amd
