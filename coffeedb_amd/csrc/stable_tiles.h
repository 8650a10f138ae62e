// stable_tiles.h — stable ranking of flagged slots, tile by tile, without atomics: what a stream compaction (remove.hip) and a
// two-way merge (append.hip) both need.  A tile is ST_TILE consecutive slots handled by one workgroup of 256 threads in
// ST_ROUNDS rounds; thread t of round k has slot tile * ST_TILE + k * 256 + t, so the rounds read and write coalesced.
//
//   pass A   tile_count_kernel: flagged slots per tile;  tile_bases: a scan (scan.h) turns the counts into every tile's base
//   pass B   the caller's own kernel: every round it loads its slot (tile_slot), asks a TileRanker how many flagged slots lie in
//            front of it in the whole array, and stores — flagged slot number r of the input is the r-th flagged slot of the
//            output, whatever the schedule: the order is the input's
// 64-bit ranks throughout; the counts inside a tile fit 32 bits.
#pragma once
#include <string>

#include "index_impl.h"
#include "scan.h"

namespace cdb {

constexpr int ST_ROUNDS = 16;              // slots per thread and tile
constexpr int ST_TILE = 256 * ST_ROUNDS;   // slots per tile (one workgroup)

__device__ __forceinline__ uint64_t tile_slot(int k) { return (uint64_t)blockIdx.x * ST_TILE + (uint64_t)k * 256 + threadIdx.x; }

// pass A.  Pred: (uint64_t slot) -> bool, asked for slots below n only
template <typename Pred>
__global__ __launch_bounds__(256) void tile_count_kernel(Pred flagged, uint64_t n, uint64_t* __restrict__ tile_count) {
    __shared__ uint32_t s_w[4];
    uint32_t c = 0;
#pragma unroll 4
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t i = tile_slot(k);
        if (i < n) c += flagged(i) ? 1u : 0u;
    }
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = (uint64_t)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
struct TileBaseOut {
    uint64_t* base;
    __device__ __forceinline__ void operator()(uint64_t t, uint64_t ex, uint64_t) const { base[t] = ex; }
};

// Counts the flagged slots of [0, n) per tile on ix.stream and leaves tile_base[t] = flagged slots in front of tile t (one u64 per
// tile, allocated here).  Returns their total (synchronises); the caller knows what it must be.  `op` names the caller in the
// error text, `label` and `bytes` are the count kernel's line in the profile.
template <typename Pred>
uint64_t tile_bases(Index& ix, const char* op, Pred flagged, uint64_t n, DevBuf& tile_base, const char* label, uint64_t bytes) {
    hipStream_t s = ix.stream;
    const uint64_t ntiles = ceil_div(n, ST_TILE);
    if (ntiles >= (1ull << 31)) throw InternalError(std::string(op) + ": the array has too many tiles for one launch (internal)");
    DevBuf tile_count;
    tile_count.alloc(ntiles * 8);
    tile_base.alloc(ntiles * 8);
    const int t = ix.prof.begin(s);
    hipLaunchKernelGGL((tile_count_kernel<Pred>), dim3((unsigned)ntiles), dim3(256), 0, s, flagged, n, tile_count.as<uint64_t>());
    ix.prof.end(t, label, bytes, s);
    CDB_HIP(hipGetLastError());
    PartialsIn<uint64_t> tin{tile_count.as<uint64_t>()};
    const uint64_t total = scan_totals<uint64_t>(s, ix.scan_partials, tin, ntiles, OpAdd{}, (uint64_t)0);
    scan_apply<uint64_t>(s, ix.scan_partials, tin, ntiles, OpAdd{}, (uint64_t)0, TileBaseOut{tile_base.as<uint64_t>()});
    CDB_HIP(hipGetLastError());
    return total;
}

// pass B, per thread: flagged slots in front of this thread's slot = tile base + flagged in earlier rounds + flagged in earlier
// waves of this round + flagged in earlier lanes of its wave (ballot).  Every thread of the workgroup calls before() once per
// round, k = 0 .. ST_ROUNDS - 1 in order, outside divergent code (it holds a barrier); slots past the end pass flag = false.
struct TileRanker {
    uint64_t run;  // flagged slots in front of the current round
    __device__ __forceinline__ explicit TileRanker(const uint64_t* __restrict__ tile_base) : run(tile_base[blockIdx.x]) {}
    __device__ __forceinline__ uint64_t before(int k, bool flag) {
        __shared__ uint32_t s_w[2][4];  // the four waves' counts of this round, in the half k & 1
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint64_t bal = __ballot(flag);
        if (lane == 0) s_w[k & 1][wave] = (uint32_t)__popcll(bal);
        __syncthreads();  // (the other half of s_w is still being read by the slowest wave of round k - 1: two halves, one barrier)
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t c = s_w[k & 1][w];
            before += w < wave ? c : 0u;
            all += c;
        }
        const uint64_t r = run + before + (uint64_t)__popcll(bal & ((1ull << lane) - 1));
        run += all;
        return r;
    }
};

}  // namespace cdb
