// radix_sort.h — stable LSD radix sort for gfx950 (digits of up to 8 bits, one read + one write of the
// data per pass: "onesweep" with chained-scan decoupled look-back).
//
// This is the bandwidth-dominant primitive of the suffix-array build (replaces the reference's
// multithreaded MSD radix + std::sort leaves, /root/reference/src/index.cpp:75-128) and of the
// hit->document grouping in the query path (replaces index.cpp:294-315).
//
// Per pass and per element the kernel moves sizeof(K)+sizeof(V) (+ sizeof(W) for an auxiliary low-digit array)
// bytes in and the same out; that is the "algorithmic bytes" figure used for the HBM roofline.
//
// In this file, the host half: the histogram and digit-start kernels, the workspace and the variant table, rs_launch_pass (the
// one launcher of rs_onesweep_kernel), the drivers (radix_sort, radix_sort_split, ...) and the segmented, MSD and tile-base
// parts.  The device half of a pass — configurations, generators, segment descriptions, the kernel and its hardware mapping —
// is radix_pass.h.
#pragma once
#include <cstdlib>

#include "common.h"
#include "radix_pass.h"

namespace cdb {

constexpr int RS_MAX_PASSES = 16;

// ---------------------------------------------------------------------------------------------
// upfront histogram of every pass's digit (one read of the keys)
// ---------------------------------------------------------------------------------------------
template <typename K>
__global__ __launch_bounds__(256) void rs_hist_kernel(const K* __restrict__ keys, uint64_t n, int begin_bit,
                                                      int npass, int dbits, uint32_t last_mask,
                                                      unsigned long long* __restrict__ ghist) {
    __shared__ uint32_t sh[RS_MAX_PASSES * 256];
    for (int i = threadIdx.x; i < npass * 256; i += 256) sh[i] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const K k = keys[i];
#pragma unroll
        for (int p = 0; p < RS_MAX_PASSES; ++p) {
            if (p < npass) {
                uint32_t d = (uint32_t)(k >> (begin_bit + dbits * p)) & ((1u << dbits) - 1u);
                if (p == npass - 1) d &= last_mask;
                // (keys that arrive nearly sorted — the hit keys of a query batch come in pattern order — agree on their high
                //  digits: 64 same-address atomics serialise, one add of the lane count does not.  8 GiB Zipf batch: 0.92 -> ms below)
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
                const uint64_t same = __builtin_amdgcn_ballot_w64(d == d0);
                const uint64_t act = __builtin_amdgcn_ballot_w64(true);
                if (same == act) {
                    if ((uint32_t)__builtin_ffsll((long long)act) - 1u == (threadIdx.x & 63u)) atomicAdd(&sh[p * 256 + d0], (uint32_t)__popcll(act));
                } else {
                    atomicAdd(&sh[p * 256 + d], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < npass * 256; i += 256)
        if (sh[i]) atomicAdd(&ghist[i], (unsigned long long)sh[i]);
}

// exclusive scan of each pass's 256 counts -> first output slot of each digit
static __global__ __launch_bounds__(256) void rs_digit_start_kernel(const unsigned long long* __restrict__ ghist,
                                                             unsigned long long* __restrict__ gstart) {
    __shared__ unsigned long long s[256];
    const int p = blockIdx.x, t = threadIdx.x;
    const unsigned long long c = ghist[p * 256 + t];
    s[t] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned long long v = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    gstart[p * 256 + t] = s[t] - c;
}



// floor(x / d) for x < 2^24 as one multiply-high: with L = ceil(log2 d) and m = ceil(2^(24+L) / d) (< 2^25, error
// m d - 2^(24+L) < d <= 2^L, so x < 2^24 keeps the quotient exact), mul = m << 7 and sh = L + 7
struct RsDiv24 { uint32_t mul, sh; };
inline RsDiv24 rs_div24_make(uint32_t d) {
    uint32_t L = 0;
    while ((1ull << L) < d) ++L;
    const uint64_t m = ((1ull << (24 + L)) + d - 1) / d;
    return RsDiv24{(uint32_t)(m << 7), L + 7};
}
__device__ __forceinline__ uint32_t rs_div24(uint32_t x, uint32_t mul, uint32_t sh) { return __umulhi(x << 8, mul) >> sh; }

// Pair form of the generated pass (TextGenPair): constants for top = floor(a / span), a < base^2, as one 24-bit multiply and a
// shift, and the range conditions of its 24-bit products.  false = this (base, span) cannot take the pair form.
template <typename G>
inline bool rs_pair_setup(G& gen, uint32_t base, uint32_t span) {
    const uint64_t b2 = (uint64_t)base * base;
    if (base < 2 || base > 255 || span == 0 || span >= (1u << 24) || b2 >= (1u << 24)) return false;
    if ((uint64_t)span * b2 >= (1u << 24)) return false;              // (a - top span) B^2 + m stays below 2^24
    if ((uint64_t)span * b2 * b2 > (1ull << 32)) return false;         // key - top M < M <= 2^32
    for (uint32_t sh = 0; sh < 32; ++sh) {
        const uint64_t r = ((1ull << sh) + span - 1) / span;
        if (r >= (1u << 24) || (b2 - 1) * r >= (1ull << 32)) break;
        bool ok = true;
        for (uint64_t a = 0; a < b2 && ok; ++a) ok = ((a * r) >> sh) == a / span;
        if (ok) {
            gen.pair_span = span;
            gen.pair_r = (uint32_t)r;
            gen.pair_s = sh;
            return true;
        }
    }
    return false;
}

// document holding the first position of every tile (tile_doc[tiles] = the last document): turns the
// two ~log2(D)-step searches per tile into one parallel pre-pass
static __global__ __launch_bounds__(256) void rs_tiledoc_kernel(const uint64_t* __restrict__ doc_start, uint64_t ndocs,
                                                                uint64_t n, uint64_t tile_elems, uint64_t tiles,
                                                                uint64_t* __restrict__ tile_doc) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > tiles) return;
    const uint64_t p = t * tile_elems < n ? t * tile_elems : n - 1;
    tile_doc[t] = rs_doc_upper(doc_start, 0, ndocs - 1, p);
}


// Settles the provisional flags at the ends of the per-digit runs of a segmented final pass: for every run (tile t,
// digit d) the run in front of it in the output is the nearest earlier tile of the same segment that holds digit d
// — its last element sits right in front of this run's first.  Equal keys there: the first element is no group head,
// and both elements belong to an unresolved group unless the key ends inside the document.
// (the body is shared by the two record types: the accessors below are all it knows of a record.  CELL records — seg_cell_edge.h —
//  belong to unrotated cells)
__device__ __forceinline__ unsigned long long rs_edge_pos(const SegEdge& e) { return e.pos; }
__device__ __forceinline__ uint32_t rs_edge_cnt(const SegEdge& e) { return e.cnt; }
__device__ __forceinline__ unsigned long long rs_edge_first(const SegEdge& e) { return e.first; }
__device__ __forceinline__ unsigned long long rs_edge_last(const SegEdge& e) { return e.last; }
__device__ __forceinline__ unsigned long long rs_edge_pos(const SegCellEdge& e) { return seg_cell_edge_pos(e.pos_cnt); }
__device__ __forceinline__ uint32_t rs_edge_cnt(const SegCellEdge& e) { return seg_cell_edge_cnt(e.pos_cnt); }
__device__ __forceinline__ unsigned long long rs_edge_first(const SegCellEdge& e) { return e.first; }
__device__ __forceinline__ unsigned long long rs_edge_last(const SegCellEdge& e) { return e.last; }
template <typename E>
__device__ __forceinline__ void rs_seg_edge_fix_body(const E* __restrict__ edges, const uint32_t* __restrict__ tile_seg,
                                                     const SegInfo* __restrict__ segs, uint32_t tiles, uint8_t* __restrict__ flags, uint32_t kbase,
                                                     unsigned long long kmagic, unsigned long long* __restrict__ tile_sums, uint32_t sums_tile,
                                                     const uint32_t* __restrict__ err) {
    constexpr bool CELL = std::is_same<E, SegCellEdge>::value;
    const uint32_t t = blockIdx.x, d = threadIdx.x;
    if (t >= tiles) return;
    if (err && *err) return;  // (a failed pass left edge records unwritten: their stale slots must not be touched)
    const E e = edges[(size_t)t * 256 + d];
    if (!rs_edge_cnt(e)) return;
    const unsigned long long epos = rs_edge_pos(e), efirst = rs_edge_first(e);
    const SegInfo si = segs[tile_seg ? tile_seg[t] : 0u];
    const uint32_t t0 = si.tile_begin;
    if (t == t0) return;
    // largest t' in [t0, t) whose run starts in front of this one (runs of tiles without the digit share its start)
    uint32_t lo = t0, hi = t;  // invariant: answer (if any) in [lo, hi)
    if (rs_edge_pos(edges[(size_t)(t - 1) * 256 + d]) < epos) {
        lo = t - 1;
    } else {
        if (rs_edge_pos(edges[(size_t)t0 * 256 + d]) >= epos) return;  // first run of this digit in the segment
        hi = t - 1;
        while (hi - lo > 1) {  // pos[lo] < e.pos <= pos[hi]
            const uint32_t mid = lo + (hi - lo) / 2;
            if (rs_edge_pos(edges[(size_t)mid * 256 + d]) < epos) lo = mid; else hi = mid;
        }
    }
    if (rs_edge_last(edges[(size_t)lo * 256 + d]) != efirst) return;
    const bool exhausted = kmagic ? (efirst - __umul64hi(efirst, kmagic) * kbase) == 0 : (efirst & (uint64_t)(kbase - 1u)) == 0;
    // one atomic per change; the old value each one returns says exactly what that change did to the tile sums
    auto change = [&](unsigned long long slot, uint32_t clear, uint32_t set) {
        // (the word that holds the byte: `flags` points at the group's first flag, which need not be 4-byte aligned;
        //  the flag array itself is a 256-byte-aligned device block, so the word lies inside it)
        const uintptr_t a = reinterpret_cast<uintptr_t>(flags + slot);
        unsigned int* w = reinterpret_cast<unsigned int*>(a & ~(uintptr_t)3);
        const uint32_t sh = 8u * (uint32_t)(a & 3u);
        uint32_t before, after;
        if (clear) {
            before = (atomicAnd(w, ~(clear << sh)) >> sh) & 0xFFu;
            after = before & ~clear;
        } else {
            before = (atomicOr(w, set << sh) >> sh) & 0xFFu;
            after = before | set;
        }
        if (tile_sums && before != after) {
            const long long da = (long long)((after >> 1) & 1u) - (long long)((before >> 1) & 1u);
            const long long db = (long long)((after >> 1) & after & 1u) - (long long)((before >> 1) & before & 1u);
            unsigned long long* ts = tile_sums + 2 * (slot / sums_tile);
            if (da) atomicAdd(ts, (unsigned long long)da);
            if (db) atomicAdd(ts + 1, (unsigned long long)db);
        }
    };
    const unsigned long long sb = CELL ? epos : rs_seg_rotated(si, epos), sa_ = CELL ? epos - 1 : rs_seg_rotated(si, epos - 1);
    change(sb, 1u, 0u);                    // first of this run: not a head
    if (!exhausted) {
        change(sb, 0u, 2u);                // ... and part of an unresolved group, like
        change(sa_, 0u, 2u);               // the last of the run in front: not a tail
    }
}
static __global__ __launch_bounds__(256) void rs_seg_edge_fix_kernel(const SegEdge* __restrict__ edges, const uint32_t* __restrict__ tile_seg,
                                                                     const SegInfo* __restrict__ segs, uint32_t tiles,
                                                                     uint8_t* __restrict__ flags, uint32_t kbase, unsigned long long kmagic,
                                                                     unsigned long long* __restrict__ tile_sums = nullptr,
                                                                     uint32_t sums_tile = 1, const uint32_t* __restrict__ err = nullptr) {
    rs_seg_edge_fix_body(edges, tile_seg, segs, tiles, flags, kbase, kmagic, tile_sums, sums_tile, err);
}
// ... over the 16-byte records of a last pass over cells: variable-length keys (a key ends inside the document <=> bit 0 clear),
// no rotation, no tile sums
static __global__ __launch_bounds__(256) void rs_seg_edge_fix_cell_kernel(const SegCellEdge* __restrict__ edges, const uint32_t* __restrict__ tile_seg,
                                                                          const SegInfo* __restrict__ segs, uint32_t tiles,
                                                                          uint8_t* __restrict__ flags, const uint32_t* __restrict__ err) {
    rs_seg_edge_fix_body(edges, tile_seg, segs, tiles, flags, 2u, 0ull, (unsigned long long*)nullptr, 1u, err);
}

// ---------------------------------------------------------------------------------------------
// self-test behind the ATOMRANK configurations
// ---------------------------------------------------------------------------------------------
// The one-atomic ranking is only a stable rank if same-address LDS atomics issued by ONE wave instruction
// complete in ascending lane order.  gfx950 does that (the LDS resolves a conflict lowest lane first), but
// it is observed behaviour, not an ISA guarantee — so every process checks it once per device against the
// ballot ranking on conflict patterns from "all 64 lanes on one counter" to "256 counters", and the sorts
// fall back to the ballot configurations if a single return value differs.
static __global__ __launch_bounds__(256) void rs_lane_order_probe_kernel(uint32_t* __restrict__ bad) {
    __shared__ uint32_t cnt[4][256];
    __shared__ uint32_t ref[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 4 * 256; i += 256) {
        (&cnt[0][0])[i] = 0;
        (&ref[0][0])[i] = 0;
    }
    __syncthreads();
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint32_t wrong = 0;
    for (uint32_t r = 0; r < 64; ++r) {
        uint32_t h = (blockIdx.x * 64u + r) * 256u + (uint32_t)tid;
        h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
        const uint32_t mode = blockIdx.x & 3u;
        const uint32_t d = mode == 0 ? 7u : mode == 1 ? (h & 1u) * 64u : mode == 2 ? (h & 15u) * 4u : (h & 255u);
        const uint32_t got = atomicAdd(&cnt[wave][d], 1u);
        uint64_t m = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        const uint32_t below = __popcll(m & lt_mask);
        uint32_t old = 0;
        if (below == 0) {
            old = ref[wave][d];
            ref[wave][d] = old + __popcll(m);
        }
        old = __shfl(old, __ffsll((unsigned long long)m) - 1);
        wrong += got != old + below ? 1u : 0u;
    }
    if (wrong) atomicAdd(bad, wrong);
}

// true when the device passed the probe (cached per device; CDB_RANK=ballot forces the ballot ranking)
struct RsRankCache {
    std::mutex mu;
    std::map<int, bool> ok;
    std::map<int, bool> starved;  // a pass in XCD-aware tile order starved on this device: the process keeps plain tickets there
    static RsRankCache& get() {
        static RsRankCache c;
        return c;
    }
};
// the builds' spot check failed with the one-atomic ranking in use: this process ranks with ballots on that device
inline void rs_atomic_rank_disable(int dev) {
    RsRankCache& c = RsRankCache::get();
    std::lock_guard<std::mutex> g(c.mu);
    c.ok[dev] = false;
}
// An XCD-ordered pass starved on `dev` (other kernels — another process sharing the GPU — held the CUs its reserved tiles
// needed): every later build of this process on that device takes plain ticket order from the start instead of paying the
// look-back timeout again per handle (database.cpp builds a fresh index object per rebuild).
inline void rs_group_order_disable(int dev) {
    RsRankCache& c = RsRankCache::get();
    std::lock_guard<std::mutex> g(c.mu);
    c.starved[dev] = true;
}
inline bool rs_group_order_starved(int dev) {
    RsRankCache& c = RsRankCache::get();
    std::lock_guard<std::mutex> g(c.mu);
    auto it = c.starved.find(dev);
    return it != c.starved.end() && it->second;
}
inline bool rs_atomic_rank_ok(hipStream_t s) {
    std::mutex& mu = RsRankCache::get().mu;
    std::map<int, bool>& cache = RsRankCache::get().ok;
    int dev = 0;
    CDB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    bool ok = false;
    const char* env = std::getenv("CDB_RANK");
    if (!(env && std::string(env) == "ballot")) {
        DevBuf d_bad;
        d_bad.alloc(sizeof(uint32_t));
        CDB_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(rs_lane_order_probe_kernel, dim3(512), dim3(256), 0, s, d_bad.as<uint32_t>());
        uint32_t bad = 1;
        CDB_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(bad), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        ok = bad == 0;
    }
    cache[dev] = ok;
    return ok;
}

// ---------------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------------
struct RadixWorkspace {
    DevBuf hist;     // [2][RS_MAX_PASSES][256] u64 : counts, then digit starts
    DevBuf status;   // [tiles][256] u64
    DevBuf tickets;  // [256] u32 tickets (indexed by epoch) + [4] u32 error flag / counters + [256][8] per-class tickets
    DevBuf tile_doc; // [tiles + 1] u64, generated first pass only
    // optional third value buffer for the NEXT sort (cleared by it): with it an odd number of passes still ends
    // with the values in buffer 0 (v0 -> spare -> v1 -> spare ... -> v0) instead of needing a copy back;
    // value_result says where the values ended up (0 = v0, 1 = v1)
    void* value_spare = nullptr;
    int value_result = 0;
    DevBuf seg1;               // one SegInfo: the whole array as a single segment (flags written by the last pass)
    SegInfo h_seg1 = {};
    bool keep_applied = false;  // the last pass of the previous sort wrote the group flags (SegFinalKeepArgs)
    uint32_t epoch = 0;
    uint64_t min_tile = 0;
    // XCD-aware tile order (RS_GROUP) is used only where the caller can redo the sort after a starved pass: the
    // suffix-array build sets allow_group for its own sorts and falls back to plain_order after a look-back timeout
    bool allow_group = false;
    bool plain_order = false;
    bool debug_poison = false;  // test hook: the next sort finds the error flag already up — what the passes BEHIND a starved
                                // pass see: they must leave their (stale) buffers alone, and the host must notice

    void prepare(uint64_t n, int tile, hipStream_t s) {
        const uint64_t tiles = ceil_div(n, (uint64_t)tile);
        if (!hist.p) hist.alloc(2 * RS_MAX_PASSES * 256 * sizeof(uint64_t));
        if (!tickets.p) {
            tickets.alloc((260 + 256 * 8) * sizeof(uint32_t));
            CDB_HIP(hipMemsetAsync(tickets.p, 0, tickets.bytes, s));
        }
        if (debug_poison) {
            CDB_HIP(hipMemsetAsync(err_ptr(), 0xFF, sizeof(uint32_t), s));
            debug_poison = false;
        }
        const size_t need = (size_t)tiles * 256 * sizeof(uint64_t);
        if (need > status.bytes) {
            status.alloc(need + need / 4);
            CDB_HIP(hipMemsetAsync(status.p, 0, status.bytes, s));
            CDB_HIP(hipMemsetAsync(tickets.p, 0, 256 * sizeof(uint32_t), s));
            CDB_HIP(hipMemsetAsync(tickets.as<uint32_t>() + 260, 0, 256 * 8 * sizeof(uint32_t), s));
            epoch = 0;
        }
    }
    uint32_t next_epoch(hipStream_t s) {
        if (epoch == 255) {  // tags wrap: forget every published word
            CDB_HIP(hipMemsetAsync(status.p, 0, status.bytes, s));
            CDB_HIP(hipMemsetAsync(tickets.p, 0, 256 * sizeof(uint32_t), s));
            CDB_HIP(hipMemsetAsync(tickets.as<uint32_t>() + 260, 0, 256 * 8 * sizeof(uint32_t), s));
            epoch = 0;
        }
        return ++epoch;
    }
    uint32_t* ticket_ptr(uint32_t e) { return tickets.as<uint32_t>() + (e & 255u); }
    uint32_t* xticket_ptr(uint32_t e) { return tickets.as<uint32_t>() + 260 + (e & 255u) * 8; }
    uint32_t* err_ptr() { return tickets.as<uint32_t>() + 256; }
    void release() { hist.release(); status.release(); tickets.release(); tile_doc.release(); seg1.release(); epoch = 0; }
};

template <typename K, typename V> inline const char* rs_kernel_name();
template <> inline const char* rs_kernel_name<uint64_t, uint32_t>() { return "rs_onesweep_k64_v32"; }
template <> inline const char* rs_kernel_name<uint64_t, uint64_t>() { return "rs_onesweep_k64_v64"; }
template <> inline const char* rs_kernel_name<uint64_t, NoVal>() { return "rs_onesweep_k64"; }
template <> inline const char* rs_kernel_name<uint32_t, uint32_t>() { return "rs_onesweep_k32_v32"; }
template <> inline const char* rs_kernel_name<uint32_t, uint64_t>() { return "rs_onesweep_k32_v64"; }
template <> inline const char* rs_kernel_name<uint32_t, NoVal>() { return "rs_onesweep_k32"; }

struct SortStats {
    int passes_run = 0, passes_skipped = 0;
};

// ---- the variant table: what the `variant` of radix_sort / radix_sort_split (the sort_variant option) selects
enum : int {
    RS_VARIANT_BY_SIZE = 0,       // big tiles (the longest per-digit runs, so the best-coalesced scatter) need a few hundred
                                  // tiles to fill 256 CUs: RsBig from RS_BIG_MIN_N keys on, RsMid from RS_MID_MIN_N, else RsSmall
    RS_VARIANT_SMALL_BALLOT = 1,  // RsSmallBallot
    RS_VARIANT_BIG_BALLOT = 21,   // RsBigBallot
    RS_VARIANT_MID_BALLOT = 26,   // RsMidBallot
    RS_VARIANT_BIG_GROUPED = 31,  // RsGrouped<RsBig>
    RS_VARIANT_SMALL = 32,        // RsSmall
    RS_VARIANT_BIG = 33,          // RsBig (plain ticket order)
    RS_VARIANT_MID = 36,          // RsMid
    RS_VARIANT_FIRST = 4,         // RsFirstVersion   (A/B only: pair sorts, no generated first pass)
    RS_VARIANT_DMA = 41,          // RsDmaLoads       (A/B only)
};
constexpr uint64_t RS_BIG_MIN_N = 1ull << 23, RS_MID_MIN_N = 1ull << 19;

// the production variants: every one of them has a generated first pass (the A/B configurations have none)
inline bool rs_variant_production(int v) {
    return v == RS_VARIANT_BY_SIZE || v == RS_VARIANT_SMALL_BALLOT || v == RS_VARIANT_BIG_BALLOT || v == RS_VARIANT_MID_BALLOT ||
           v == RS_VARIANT_BIG_GROUPED || v == RS_VARIANT_SMALL || v == RS_VARIANT_BIG || v == RS_VARIANT_MID;
}
// true when the requested variant sorts n keys in 16 Ki-key one-atomic tiles (on a device that passed rs_atomic_rank_ok)
inline bool rs_variant_big_atomic(int v, uint64_t n) {
    return (v == RS_VARIANT_BY_SIZE && n >= RS_BIG_MIN_N) || v == RS_VARIANT_BIG_GROUPED || v == RS_VARIANT_BIG;
}
// ... or, the looser question of a caller that only prepares for such a pass: ANY variant counts from RS_BIG_MIN_N keys on (a forced
// small-tile variant then finds the preparation unused: radix_sort_cfg's CAN_KEEP is false for it and keep_applied stays down)
inline bool rs_variant_maybe_big_atomic(int v, uint64_t n) { return n >= RS_BIG_MIN_N || rs_variant_big_atomic(v, n); }

// the variant that runs: by size for RS_VARIANT_BY_SIZE, plain ticket order where the caller may not use the grouped one, the
// ballot twins on a device without the one-atomic ranking
inline int rs_resolve_variant(hipStream_t s, const RadixWorkspace& ws, int v, uint64_t n) {
    if (v == RS_VARIANT_BY_SIZE) v = n >= RS_BIG_MIN_N ? RS_VARIANT_BIG_GROUPED : (n >= RS_MID_MIN_N ? RS_VARIANT_MID : RS_VARIANT_SMALL);
    if (v == RS_VARIANT_BIG_GROUPED && (!ws.allow_group || ws.plain_order)) v = RS_VARIANT_BIG;
    if (rs_atomic_rank_ok(s)) return v;
    return v == RS_VARIANT_BIG_GROUPED || v == RS_VARIANT_BIG ? RS_VARIANT_BIG_BALLOT
         : v == RS_VARIANT_MID ? RS_VARIANT_MID_BALLOT : (v == RS_VARIANT_SMALL ? RS_VARIANT_SMALL_BALLOT : v);
}
// ... and its configuration: run(Cfg(), has_gen).  IPT_BIG = keys per thread of the big tile; AB = offer the A/B configurations
// (any other number runs RsBigBallot)
template <int IPT_BIG, bool AB, typename F>
int rs_dispatch_variant(int resolved, F&& run) {
    if constexpr (AB) {
        if (resolved == RS_VARIANT_FIRST) return run(RsFirstVersion(), std::false_type());
        if (resolved == RS_VARIANT_DMA) return run(RsDmaLoads(), std::false_type());
    }
    switch (resolved) {
        default:
        case RS_VARIANT_BIG_BALLOT: return run(RsBigBallot<IPT_BIG>(), std::true_type());
        case RS_VARIANT_MID_BALLOT: return run(RsMidBallot(), std::true_type());
        case RS_VARIANT_SMALL_BALLOT: return run(RsSmallBallot(), std::true_type());
        case RS_VARIANT_BIG_GROUPED: return run(RsGrouped<RsBig<IPT_BIG>>(), std::true_type());
        case RS_VARIANT_BIG: return run(RsBig<IPT_BIG>(), std::true_type());
        case RS_VARIANT_MID: return run(RsMid(), std::true_type());
        case RS_VARIANT_SMALL: return run(RsSmall(), std::true_type());
    }
}

// ---- the one place that launches rs_onesweep_kernel: one pass over `tiles` tiles of Cfg.  Owns the grid (whole groups of
// 8 * GROUP tiles in XCD-aware order), the pass's epoch, the ticket counter that goes with the order, status and error words.
template <typename T> struct RsId { using type = T; };  // (input pointers may be a plain nullptr: K, V come from the outputs, W is named)
template <typename Cfg, typename W = NoVal, typename K, typename V, typename Gen = NoGen, typename Seg = NoSeg>
void rs_launch_pass(hipStream_t s, RadixWorkspace& ws, uint32_t tiles, typename RsId<const K*>::type kin, K* kout,
                    typename RsId<const V*>::type vin, V* vout, uint64_t n, int shift, uint32_t dmask, const unsigned long long* digit_start,
                    const Gen& gen = Gen(), typename RsId<const W*>::type win = nullptr, typename RsId<W*>::type wout = nullptr,
                    int aux_shift = -1, const Seg& seg = Seg()) {
    constexpr uint32_t G = 8u * Cfg::GROUP;
    uint32_t grid = tiles;
    if constexpr (G > 0) grid = (uint32_t)(ceil_div(tiles, G) * G);
    const uint32_t e = ws.next_epoch(s);
    hipLaunchKernelGGL((rs_onesweep_kernel<K, V, Cfg, Gen, W, Seg>), dim3(grid), dim3(Cfg::NT), 0, s, kin, kout, vin, vout, n, shift, dmask,
                       digit_start, ws.status.as<uint64_t>(), G > 0 ? ws.xticket_ptr(e) : ws.ticket_ptr(e), e, ws.err_ptr(), gen, win, wout,
                       aux_shift, seg);
}
// ... in the order the workspace allows: Cfg's grouped twin where the caller can redo the sort after a starved pass
template <typename Cfg, typename W = NoVal, typename... A>
void rs_launch_pass_ordered(hipStream_t s, RadixWorkspace& ws, A&&... a) {
    if (ws.allow_group && !ws.plain_order) rs_launch_pass<RsGrouped<Cfg>, W>(s, ws, a...);
    else rs_launch_pass<Cfg, W>(s, ws, a...);
}

// the per-tile document table of a generated pass over n positions in tiles of `tile` (gen.tile_doc)
template <typename G>
void rs_gen_tile_docs(hipStream_t s, RadixWorkspace& ws, G& gen, uint64_t n, uint64_t tile) {
    const uint64_t tiles = ceil_div(n, tile);
    ws.tile_doc.ensure((tiles + 1) * sizeof(uint64_t));
    hipLaunchKernelGGL(rs_tiledoc_kernel, dim3((unsigned)ceil_div(tiles + 1, 256)), dim3(256), 0, s, gen.doc_start, gen.ndocs, n, tile, tiles,
                       ws.tile_doc.as<uint64_t>());
    gen.tile_doc = ws.tile_doc.as<uint64_t>();
}

struct SortPlan {
    int npass, begin_bit;
    uint32_t last_mask;
    std::vector<uint64_t> h_hist;
};

// One sort.  `h_hist_in` (optional, host, [npass][256]) supplies the per-pass digit histograms when the
// caller can derive them more cheaply than by reading the keys; `gen` (optional) makes the first pass
// produce its (key, value) input on the fly (buffers 0 are then never read).
template <typename K, typename V, typename Cfg, typename Gen = NoGen, typename W = NoVal>
int radix_sort_cfg(hipStream_t s, RadixWorkspace& ws, Profiler& prof, K* k0, K* k1, V* v0, V* v1, uint64_t n,
                   int begin_bit, int end_bit, SortStats* stats, int dbits, const uint64_t* h_hist_in = nullptr,
                   const Gen* gen = nullptr, W* w0 = nullptr, W* w1 = nullptr, int lead_in = 0,
                   const unsigned long long* d_hist_in = nullptr, const SegFinalKeepArgs* keep = nullptr) {
    constexpr int IPT = Cfg::IPT;
    constexpr int TILE = Cfg::NT * IPT;
    constexpr bool HAS_V = !std::is_same<V, NoVal>::value;
    constexpr bool HAS_W = !std::is_same<W, NoVal>::value;
    constexpr bool GEN = !std::is_same<Gen, NoGen>::value;
    // split keys: the first `lead` passes sort on the auxiliary low digits (a generated first pass produces
    // them: lead = low_bits / dbits; materialised records say how many digits their auxiliary array holds:
    // lead_in); the passes over the key bits [begin_bit, end_bit) follow.  h_hist_in has `lead` leading rows.
    if (dbits < 1 || dbits > 8) dbits = 8;
    int lead = 0;
    if constexpr (GEN && HAS_W) lead = gen->low_bits / dbits;
    else if constexpr (HAS_W) lead = lead_in;
    if (HAS_W && !GEN && !h_hist_in && !d_hist_in) throw InternalError("radix_sort: split records need caller-supplied histograms (internal)");
    const int LEAD = lead;
    if (n == 0 || end_bit < begin_bit || (!LEAD && end_bit == begin_bit)) return 0;  // (value_result / value_spare stay as the previous sort left them)
    const int nbits = end_bit - begin_bit;
    const int kpass = (int)ceil_div(nbits, dbits);  // passes over the key proper
    const int npass = kpass + LEAD;
    if (npass > RS_MAX_PASSES) throw Error("radix_sort: too many passes requested");
    const int last_bits = kpass ? nbits - dbits * (kpass - 1) : dbits;
    const uint32_t last_mask = (1u << last_bits) - 1u;
    ws.prepare(n, TILE, s);
    ws.keep_applied = false;

    unsigned long long* d_hist = ws.hist.as<unsigned long long>();
    unsigned long long* d_start = d_hist + RS_MAX_PASSES * 256;
    std::vector<uint64_t> h_hist((size_t)npass * 256);
    if (d_hist_in) {
        // histograms already on the device ([npass][256], lowest digit first): no host round trip at all — the
        // bucket-wise build queues hundreds of sorts back to back (no pass is skipped: the host never sees the counts)
        CDB_HIP(hipMemcpyAsync(d_hist, d_hist_in, (size_t)npass * 256 * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(rs_digit_start_kernel, dim3(npass), dim3(256), 0, s, d_hist, d_start);
    } else if (h_hist_in) {
        std::copy(h_hist_in, h_hist_in + h_hist.size(), h_hist.begin());
        CDB_HIP(hipMemcpyAsync(d_hist, h_hist.data(), h_hist.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(rs_digit_start_kernel, dim3(npass), dim3(256), 0, s, d_hist, d_start);
        CDB_HIP(hipStreamSynchronize(s));  // h_hist is pageable host memory
    } else {
        if (GEN) throw InternalError("radix_sort: a generated first pass needs caller-supplied histograms (internal)");
        CDB_HIP(hipMemsetAsync(d_hist, 0, RS_MAX_PASSES * 256 * sizeof(uint64_t), s));
        const int grid = (int)std::min<uint64_t>(ceil_div(n, 256 * 16), 256 * 8);
        int t = prof.begin(s);
        hipLaunchKernelGGL(rs_hist_kernel<K>, dim3(grid), dim3(256), 0, s, (const K*)k0, n, begin_bit, npass,
                           dbits, last_mask, d_hist);
        prof.end(t, "rs_hist", n * sizeof(K), s);
        hipLaunchKernelGGL(rs_digit_start_kernel, dim3(npass), dim3(256), 0, s, d_hist, d_start);
        CDB_HIP(hipMemcpyAsync(h_hist.data(), d_hist, h_hist.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
    }

    K* kb[2] = {k0, k1};
    W* wb[2] = {w0, w1};
    int cur = 0;
    bool materialised = !GEN;  // with a generator the input exists only after the first executed pass
    const uint32_t tiles = (uint32_t)ceil_div(n, (uint64_t)TILE);
    const size_t pair_bytes = sizeof(K) + (HAS_V ? sizeof(V) : 0) + (HAS_W ? sizeof(W) : 0);
    // which passes run (a constant digit is skipped; the leading pass of a generated sort always runs: it
    // produces the records) and through which value buffers
    std::vector<int> run;
    {
        bool mat = materialised;
        for (int p = 0; p < npass; ++p) {
            bool trivial = false;
            for (int d = 0; d < 256; ++d)
                if (h_hist[(size_t)p * 256 + d] == n) trivial = true;
            if (trivial && (mat || p + 1 < npass) && !(GEN && LEAD > 0 && p == 0)) {
                if (stats) stats->passes_skipped++;
                continue;
            }
            run.push_back(p);
            mat = true;
        }
    }
    V* spare = static_cast<V*>(ws.value_spare);
    ws.value_spare = nullptr;
    const size_t k = run.size();
    std::vector<V*> vseq(k + 1);
    for (size_t i = 0; i <= k; ++i) vseq[i] = (i & 1) ? v1 : v0;
    if (HAS_V && !GEN && spare && (k & 1) && k >= 3) {
        for (size_t i = 1; i < k; ++i) vseq[i] = (i & 1) ? spare : v1;
        vseq[k] = v0;
    }
    ws.value_result = vseq[k] == v0 ? 0 : 1;
    for (size_t ri = 0; ri < k; ++ri) {
        const int p = run[ri];
        V* const vin_p = vseq[ri];
        V* const vout_p = vseq[ri + 1];
        const uint32_t dmask = p == npass - 1 && kpass ? last_mask : ((1u << dbits) - 1u);
        const int shift = begin_bit + dbits * (p - LEAD);  // (unused by the leading passes of a split sort)
        const int aux_shift = p < LEAD ? dbits * p : -1;
        const unsigned long long* dstart = d_start + p * 256;
        int t = prof.begin(s);
        if (!materialised) {
            if constexpr (GEN) {
                Gen g2 = *gen;
                rs_gen_tile_docs(s, ws, g2, n, TILE);
                rs_launch_pass<Cfg, W>(s, ws, tiles, nullptr, kb[cur ^ 1], nullptr, vout_p, n, shift, dmask, dstart, g2, nullptr, wb[cur ^ 1], aux_shift);
            }
            prof.end(t, (std::string("rs_onesweep_textgen") + (HAS_W ? "_split" : "") + "_t" + std::to_string(TILE)).c_str(),
                     n * (1 + (kb[cur ^ 1] ? sizeof(K) : 0) + (HAS_V ? sizeof(V) : 0) + (HAS_W ? sizeof(W) : 0)), s);
            materialised = true;
        } else {
            // the last pass can write the group flags beside its records (16 Ki-tile one-atomic configurations, split records)
            constexpr bool CAN_KEEP = HAS_W && HAS_V && sizeof(K) == 4 && sizeof(V) == 4 && Cfg::NT == 1024 && Cfg::ATOMRANK && Cfg::REUSE && !Cfg::DMA;
            bool kept = false;
            if constexpr (CAN_KEEP) {
                if (keep && ri + 1 == k) {
                    ws.h_seg1 = SegInfo{0ull, (unsigned long long)n, 0u, 0u, 0ull, 0ull};
                    ws.seg1.ensure(sizeof(SegInfo));
                    CDB_HIP(hipMemcpyAsync(ws.seg1.p, &ws.h_seg1, sizeof(SegInfo), hipMemcpyHostToDevice, s));
                    SegFinalKeepArgs ka = *keep;
                    ka.tile_seg = nullptr;
                    ka.segs = ws.seg1.as<SegInfo>();
                    ka.tiles = tiles;
                    ka.start_stride = 0;
                    rs_launch_pass<Cfg, W>(s, ws, tiles, kb[cur], kb[cur ^ 1], vin_p, vout_p, n, shift, dmask, dstart, NoGen(), wb[cur], wb[cur ^ 1], aux_shift, ka);
                    hipLaunchKernelGGL(rs_seg_edge_fix_kernel, dim3(tiles), dim3(256), 0, s, (const SegEdge*)ka.edges, (const uint32_t*)nullptr,
                                       (const SegInfo*)ws.seg1.as<SegInfo>(), tiles, ka.flags, ka.kbase, ka.kmagic, ka.tile_sums, ka.sums_tile, (const uint32_t*)ws.err_ptr());
                    kept = true;
                    ws.keep_applied = true;
                }
            }
            if (!kept) rs_launch_pass<Cfg, W>(s, ws, tiles, kb[cur], kb[cur ^ 1], vin_p, vout_p, n, shift, dmask, dstart, NoGen(), wb[cur], wb[cur ^ 1], aux_shift);
            prof.end(t, (std::string(rs_kernel_name<K, V>()) + (HAS_W ? (sizeof(W) == 1 ? "_w8" : (sizeof(W) == 2 ? "_w16" : "_w32")) : "") +
                         (kept ? "_flags" : "") + "_t" + std::to_string(TILE)).c_str(),
                     2 * n * pair_bytes + (kept ? n : 0), s);
        }
        cur ^= 1;
        if (stats) stats->passes_run++;
    }
    CDB_HIP(hipGetLastError());
    return cur;
}

// Sorts n (key, value) pairs by key bits [begin_bit, end_bit), stable.  Buffers 0 hold the input; the
// result ends up in buffers `return value` (0 or 1).  Passes whose digit is constant are skipped.
// `variant` selects a kernel configuration (0 = by size; others exist for A/B measurements).
template <typename K, typename V>
int radix_sort(hipStream_t s, RadixWorkspace& ws, Profiler& prof, K* k0, K* k1, V* v0, V* v1, uint64_t n,
               int begin_bit, int end_bit, SortStats* stats = nullptr, int variant = 0, int dbits = 8,
               const uint64_t* h_hist_in = nullptr, const TextGen* gen = nullptr, const unsigned long long* d_hist_in = nullptr) {
    if constexpr (std::is_same<V, NoVal>::value) {
        // key-only: RS_VARIANT_BIG_BALLOT forces the ballot ranking, RS_VARIANT_BIG the plain ticket order; no generated pass, and
        // d_hist_in is not passed on (cdb_debug_radix_sort_ex refuses the flag for key-only sorts)
        auto run = [&](auto cfg) { return radix_sort_cfg<K, V, decltype(cfg)>(s, ws, prof, k0, k1, v0, v1, n, begin_bit, end_bit, stats, dbits, h_hist_in); };
        const bool atomrank = rs_atomic_rank_ok(s) && variant != RS_VARIANT_BIG_BALLOT;
        if (n < RS_BIG_MIN_N) return atomrank ? run(RsKeySmall()) : run(RsKeySmallBallot());
        if (!atomrank) return run(RsKeyBigBallot());
        return variant != RS_VARIANT_BIG && ws.allow_group && !ws.plain_order ? run(RsGrouped<RsKeyBig>()) : run(RsKeyBig());
    } else {
        variant = rs_resolve_variant(s, ws, variant, n);
        if (gen && !rs_variant_production(variant))
            throw InternalError("radix_sort: this kernel configuration has no generated first pass (internal)");
        return rs_dispatch_variant<16, true>(variant, [&](auto cfg, auto has_gen) {
            using Cfg = decltype(cfg);
            if constexpr (decltype(has_gen)::value)
                if (gen) return radix_sort_cfg<K, V, Cfg, TextGen>(s, ws, prof, k0, k1, v0, v1, n, begin_bit, end_bit, stats, dbits, h_hist_in, gen);
            return radix_sort_cfg<K, V, Cfg>(s, ws, prof, k0, k1, v0, v1, n, begin_bit, end_bit, stats, dbits, h_hist_in,
                                             (const NoGen*)nullptr, (NoVal*)nullptr, (NoVal*)nullptr, 0, d_hist_in);
        });
    }
}

// throws if any look-back spin hit its bound (the sort result is then garbage)
inline void radix_check_error(hipStream_t s, RadixWorkspace& ws) {
    if (!ws.tickets.p) return;
    uint32_t e = 0;
    CDB_HIP(hipMemcpyAsync(&e, ws.err_ptr(), sizeof(e), hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    if (e) {
        CDB_HIP(hipMemsetAsync(ws.err_ptr(), 0, sizeof(uint32_t), s));
        throw LookbackTimeout("radix sort look-back timed out (internal error)");
    }
    if (getenv("CDB_LOOKBACK_STATS")) {
        uint32_t c[3] = {0, 0, 0};
        CDB_HIP(hipMemcpy(c, ws.err_ptr(), sizeof(c), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[lookback] consumed=%u round_trips=%u\n", c[1], c[2]);
    }
}

// Split sort for keys of up to 32 + low_bits bits: the lowest one or two digits (W = u8 / u16, gen->low_bits =
// digits x dbits) are sorted first — the generated pass takes the lowest — and dropped from the key, so the
// remaining passes move (u32 key >> low_bits, value, W) = 9 or 10 bytes per element instead of 12 for a
// (u64, u32) pair.  h_hist = [all passes][256], lowest digit first.
// gen == nullptr: the records already exist in buffers 0 (their auxiliary array holds sizeof(W) digits).
template <typename V, typename W>
int radix_sort_split(hipStream_t s, RadixWorkspace& ws, Profiler& prof, uint32_t* k0, uint32_t* k1, V* v0, V* v1,
                     W* w0, W* w1, uint64_t n, int hi_bits, SortStats* stats, int variant, int dbits,
                     const uint64_t* h_hist, const TextGen* gen, int key_begin = 0, const unsigned long long* d_hist = nullptr,
                     int lead_digits = -1, const SegFinalKeepArgs* keep = nullptr) {
    // lead_digits: sort digits in the auxiliary array of materialised records (default: every byte of W); the bytes
    // above them are carried along untouched (the bucket-wise build keeps bits 32..39 of its entries there)
    const int lead_in = lead_digits >= 0 ? lead_digits : (int)sizeof(W);
    return rs_dispatch_variant<RS_SPLIT_BIG_IPT<V>, false>(rs_resolve_variant(s, ws, variant, n), [&](auto cfg, auto) {
        using Cfg = decltype(cfg);
        if constexpr (sizeof(W) <= 2)  // (a generated first pass produces one or two low digits)
            if (gen) return radix_sort_cfg<uint32_t, V, Cfg, TextGen, W>(s, ws, prof, k0, k1, v0, v1, n, key_begin, hi_bits, stats, dbits, h_hist, gen, w0, w1, 0, nullptr, keep);
        return radix_sort_cfg<uint32_t, V, Cfg, NoGen, W>(s, ws, prof, k0, k1, v0, v1, n, key_begin, hi_bits, stats, dbits, h_hist,
                                                          (const NoGen*)nullptr, w0, w1, lead_in, d_hist, keep);
    });
}

// ---------------------------------------------------------------------------------------------
// segmented sort of packed bucket records (the bucket-wise build of corpora >= 2^32)
// ---------------------------------------------------------------------------------------------
constexpr int RS_SEG_TILE = 16384;  // 1024 threads x 16 records (u32 key, u32 value, W)

// first tile of every segment is known on the host; the tile -> segment map is a search per tile
static __global__ __launch_bounds__(256) void rs_seg_tilemap_kernel(const SegInfo* __restrict__ segs, uint32_t nseg, uint32_t tiles,
                                                                    uint32_t* __restrict__ tile_seg) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= tiles) return;
    uint32_t lo = 0, hi = nseg - 1;  // largest g with segs[g].tile_begin <= t
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (segs[mid].tile_begin <= t) lo = mid; else hi = mid - 1;
    }
    tile_seg[t] = lo;
}

// starts[g][p][d] = first output slot of digit d of pass p inside segment g (hist and starts: [nseg][8][256])
static __global__ __launch_bounds__(256) void rs_seg_digit_start_kernel(const unsigned long long* __restrict__ hist,
                                                                        const SegInfo* __restrict__ segs, int npass,
                                                                        unsigned long long* __restrict__ starts) {
    __shared__ unsigned long long s[256];
    const uint32_t g = blockIdx.x;
    const int t = threadIdx.x;
    const unsigned long long b0 = segs[g].begin;
    for (int p = 0; p < npass; ++p) {
        const unsigned long long c = hist[((size_t)g * 8 + p) * 256 + t];
        s[t] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned long long v = t >= off ? s[t - off] : 0;
            __syncthreads();
            s[t] += v;
            __syncthreads();
        }
        starts[((size_t)g * 8 + p) * 256 + t] = b0 + s[t] - c;
        __syncthreads();
    }
}

// One stable LSD sort per segment, all segments of a pass in ONE launch.  Records (k32, value, aux) of m elements in
// buffers 0; `lead` low digits sit in the auxiliary word (sorted first), key_bits bits in k32.  The last pass writes
// entries and group flags through `fin` (eout / flags / edges filled in by the caller) instead of records.
// d_hist: digit counts [nseg][8][256], lowest digit first; d_starts: scratch of the same shape.
// Fin = SegFinalCellArgs: the last pass over the cells of a top-digit-first sort (byte-wide aux words without key bits, 32-bit
// keys, no rotation), with 16-byte edge records and their edge fix.
template <typename W, typename Fin = SegFinalArgs>
void radix_sort_segmented(hipStream_t s, RadixWorkspace& ws, Profiler& prof, uint32_t* k0, uint32_t* k1, uint32_t* v0, uint32_t* v1,
                          W* w0, W* w1, uint64_t m, const SegInfo* d_segs, const uint32_t* d_tile_seg, uint32_t nseg, uint32_t tiles,
                          const unsigned long long* d_hist, unsigned long long* d_starts, int key_bits, int lead, Fin fin,
                          SortStats* stats) {
    constexpr bool CELL = std::is_same<Fin, SegFinalCellArgs>::value;
    if (!rs_atomic_rank_ok(s)) throw InternalError("radix_sort_segmented: needs the one-atomic ranking (internal)");
    const int kpass = (int)ceil_div((uint64_t)key_bits, 8);
    const int npass = kpass + lead;
    if (npass < 1 || npass > 8 || kpass < 1) throw InternalError("radix_sort_segmented: unsupported pass count (internal)");
    if constexpr (CELL) {
        static_assert(std::is_same<W, uint8_t>::value, "last pass over cells: byte-wide aux words");
        if (lead != 0 || key_bits != 32 || fin.hi_mask > 0xFFu) throw InternalError("radix_sort_segmented: cell form (internal)");
        seg_cell_edge_check_limits(m, RS_SEG_TILE);  // (the output slots of a group are [0, m))
    }
    const int last_bits = key_bits - 8 * (kpass - 1);
    const uint32_t last_mask = (1u << last_bits) - 1u;
    ws.prepare((uint64_t)tiles * RS_SEG_TILE, RS_SEG_TILE, s);
    hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nseg), dim3(256), 0, s, d_hist, d_segs, npass, d_starts);
    SegArgs sa;
    sa.tile_seg = d_tile_seg;
    sa.segs = d_segs;
    sa.tiles = tiles;
    sa.start_stride = 8 * 256;
    static_cast<SegArgs&>(fin) = sa;
    uint32_t* kb[2] = {k0, k1};
    uint32_t* vb[2] = {v0, v1};
    W* wb[2] = {w0, w1};
    int cur = 0;
    const char* wn = sizeof(W) == 1 ? "_w8" : (sizeof(W) == 2 ? "_w16" : "_w32");
    const size_t rec = 8 + sizeof(W);
    for (int p = 0; p < npass; ++p) {
        const uint32_t dmask = p == npass - 1 ? last_mask : 0xFFu;
        const int shift = 8 * (p - lead);
        const int aux_shift = p < lead ? 8 * p : -1;
        const unsigned long long* dstart = d_starts + (size_t)p * 256;
        int t = prof.begin(s);
        if (p == npass - 1) {
            rs_launch_pass_ordered<RsBig<>, W>(s, ws, tiles, kb[cur], kb[cur ^ 1], vb[cur], vb[cur ^ 1], m, shift, dmask, dstart, NoGen(), wb[cur],
                                               wb[cur ^ 1], aux_shift, fin);
            prof.end(t, (std::string("rs_seg_final") + wn + "_t16384").c_str(), m * (rec + (fin.elo ? 6 : 9)), s);
        } else {
            rs_launch_pass_ordered<RsBig<>, W>(s, ws, tiles, kb[cur], kb[cur ^ 1], vb[cur], vb[cur ^ 1], m, shift, dmask, dstart, NoGen(), wb[cur],
                                               wb[cur ^ 1], aux_shift, sa);
            prof.end(t, (std::string("rs_seg_k32_v32") + wn + "_t16384").c_str(), 2 * m * rec, s);
        }
        cur ^= 1;
        if (stats) stats->passes_run++;
    }
    int t = prof.begin(s);
    if constexpr (CELL) {
        hipLaunchKernelGGL(rs_seg_edge_fix_cell_kernel, dim3(tiles), dim3(256), 0, s, (const SegCellEdge*)fin.edges, d_tile_seg, d_segs, tiles,
                           fin.flags, (const uint32_t*)ws.err_ptr());
        prof.end(t, "rs_seg_edge_fix", (uint64_t)tiles * 256 * sizeof(SegCellEdge), s);
    } else {
        hipLaunchKernelGGL(rs_seg_edge_fix_kernel, dim3(tiles), dim3(256), 0, s, (const SegEdge*)fin.edges, d_tile_seg, d_segs, tiles,
                           fin.flags, fin.kbase, fin.kmagic, (unsigned long long*)nullptr, 1u, (const uint32_t*)ws.err_ptr());
        prof.end(t, "rs_seg_edge_fix", (uint64_t)tiles * 256 * sizeof(SegEdge), s);
    }
    CDB_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// MSD-first sort of generated split records (suffix-array builds below 2^32 whose key is 33..40 bits wide)
// ---------------------------------------------------------------------------------------------
// The LSD split sort drops the digit its generated pass sorts on into a byte that then travels through every other
// pass (the group flags at the end need the whole key): 9 bytes per record and pass, scattered over the whole array.
// Here the generated pass sorts on the TOP digit instead (key >> 32): an element's bucket then implies that digit, the
// records are (u32 key, u32 entry) = 8 bytes, and the remaining four passes sort every bucket on its own — one
// segmented launch per pass, the scatter of a tile stays inside its bucket (tools/experiments/seg_bench.hip: 3.6 ms per
// pass of 2^30 records against 4.45 ms for the 9-byte records of the LSD form).  The price: the digit histograms of the
// buckets cannot come from the text sweep (bucket x pass x digit counters do not fit the LDS), they are counted from
// the partitioned keys (rs_seg_hist_kernel: 4 B read per record).
constexpr int RS_MSD_HIST_TILES = 32;  // consecutive tiles per workgroup of the histogram sweep

// hist[g][p][d] (the [nseg][8][256] layout of rs_seg_digit_start_kernel) from the materialised records of every segment:
// digit p < lead is byte p of the auxiliary word, digit lead + q byte q of the key (the order the segmented passes sort in).
// KEYS = false: only auxiliary digits are counted (npass <= lead) and the keys are never loaded — sizeof(W) bytes per record
// (the top-digit histogram of radix_sort_top_first)
template <typename W, bool KEYS = true>
__global__ __launch_bounds__(1024) void rs_seg_hist_kernel(const uint32_t* __restrict__ keys, const W* __restrict__ aux, int lead, int npass,
                                                           const uint32_t* __restrict__ tile_seg, const SegInfo* __restrict__ segs,
                                                           uint32_t tiles, unsigned long long* __restrict__ hist) {
    // (round 5) NC copies of the counters, by lane, 64 / NC banks apart: inside a bucket the high digits take few values (the symbols
    // that can follow the bucket's symbol — 64 continuation bytes behind a UTF-8 lead byte), and 64 lanes on one copy collide on the
    // same ADDRESS (SQ_LDS_ADDR_CONFLICT as large as the kernel's LDS issue cycles, profiles/r05e_sq_counters.txt); a copy stride of a
    // multiple of 64 words would leave the four counters of one digit on one bank
    constexpr int NC = 4, HC = 8 * 256 + 64 / NC;  // (8 copies: -3 % at 16 GiB, +3 % at C1 where a workgroup flushes more often)
    __shared__ uint32_t sh4[NC * HC];
    const int tid = threadIdx.x;
    uint32_t* const sh = sh4 + (tid & (NC - 1)) * HC;
    const uint32_t t0 = blockIdx.x * RS_MSD_HIST_TILES;
    const uint32_t t1 = t0 + RS_MSD_HIST_TILES < tiles ? t0 + RS_MSD_HIST_TILES : tiles;
    uint32_t cur = ~0u;
    auto flush = [&]() {
        __syncthreads();
        if (cur != ~0u)
            for (int i = tid; i < npass * 256; i += 1024) {
                uint32_t c = 0;
#pragma unroll
                for (int q = 0; q < NC; ++q) c += sh4[q * HC + i];
                if (c) atomicAdd(&hist[((size_t)cur * 8 + i / 256) * 256 + i % 256], (unsigned long long)c);
            }
        __syncthreads();  // (the sums read all four copies: nobody clears a counter another thread still has to read)
        for (int i = tid; i < NC * HC; i += 1024) sh4[i] = 0;
        __syncthreads();
    };
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t g = tile_seg[t];
        if (g != cur) {  // (uniform)
            flush();
            cur = g;
        }
        const SegInfo si = segs[g];
        const uint64_t base = si.begin + (uint64_t)(t - si.tile_begin) * RS_SEG_TILE;
        const uint32_t valid = (uint32_t)((si.end - base) < (uint64_t)RS_SEG_TILE ? (si.end - base) : (uint64_t)RS_SEG_TILE);
        // 16-byte loads (four records per lane and instruction; round 4: 4-byte loads left the sweep issue-bound at 3.4 TB/s):
        // the tile's records [base, end) = up to three in front of the first 4-aligned index, whole quads, up to three behind
        auto count = [&](uint32_t k, uint32_t a) {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                if (p < npass) {
                    const uint32_t dg = p < lead ? (a >> (8 * p)) & 0xFFu : (k >> (8 * (p - lead))) & 0xFFu;
                    atomicAdd(&sh[p * 256 + dg], 1u);
                }
            }
        };
        const uint64_t end = base + valid;
        const uint64_t a0 = (base + 3) & ~3ull;  // (the arrays are 256-byte aligned blocks: index alignment = address alignment)
        const uint64_t q0 = a0 < end ? a0 : end;
        const uint32_t nquad = (uint32_t)((end - q0) / 4);
        constexpr bool need_k = KEYS;
        if ((uint64_t)tid < q0 - base) count(need_k ? keys[base + tid] : 0u, lead > 0 ? (uint32_t)aux[base + tid] : 0u);
        {
            const uint64_t tb = q0 + 4ull * nquad;
            if ((uint64_t)tid < end - tb) count(need_k ? keys[tb + tid] : 0u, lead > 0 ? (uint32_t)aux[tb + tid] : 0u);
        }
        constexpr int QPT = RS_SEG_TILE / 4 / 1024;  // quads per thread of a full tile
        uint4 kq[QPT];
        uint32_t aq[QPT][4];
#pragma unroll
        for (int r = 0; r < QPT; ++r) {
            const uint32_t g = (uint32_t)r * 1024u + (uint32_t)tid;
            kq[r] = make_uint4(0, 0, 0, 0);
            aq[r][0] = aq[r][1] = aq[r][2] = aq[r][3] = 0;
            if (g < nquad) {
                if (need_k) kq[r] = *reinterpret_cast<const uint4*>(keys + q0 + 4ull * g);
                if (lead > 0) {
                    if constexpr (sizeof(W) == 4) {
                        const uint4 w = *reinterpret_cast<const uint4*>(aux + q0 + 4ull * g);
                        aq[r][0] = w.x; aq[r][1] = w.y; aq[r][2] = w.z; aq[r][3] = w.w;
                    } else if constexpr (sizeof(W) == 2) {
                        const uint2 w = *reinterpret_cast<const uint2*>(aux + q0 + 4ull * g);
                        aq[r][0] = w.x & 0xFFFFu; aq[r][1] = w.x >> 16; aq[r][2] = w.y & 0xFFFFu; aq[r][3] = w.y >> 16;
                    } else {
                        const uint32_t w = *reinterpret_cast<const uint32_t*>(aux + q0 + 4ull * g);
                        aq[r][0] = w & 0xFFu; aq[r][1] = (w >> 8) & 0xFFu; aq[r][2] = (w >> 16) & 0xFFu; aq[r][3] = w >> 24;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < QPT; ++r) {
            const uint32_t g = (uint32_t)r * 1024u + (uint32_t)tid;
            if (g < nquad) {
                count(kq[r].x, aq[r][0]);
                count(kq[r].y, aq[r][1]);
                count(kq[r].z, aq[r][2]);
                count(kq[r].w, aq[r][3]);
            }
        }
    }
    flush();
}

// ---------------------------------------------------------------------------------------------
// segmented sort, top key digit first (bucket-wise builds with 40-bit keys in (u32, u32, u16) records)
// ---------------------------------------------------------------------------------------------
// The five-pass form sorts on the key's low byte first and then carries it through four more passes, because the group flags
// of the last pass need the whole key.  Here the records hold the key's TOP byte in the aux word's low byte and its low 32
// bits in k32 (VlTables::top_in_aux); one stable pass per bucket sorts on that byte and drops it (SegShrinkArgs), a CELL =
// (bucket, top byte) implies it from then on, and the other four passes run per cell over (u32, u32, u8) records — the same
// order, ties included, as five stable LSD passes.  Equal keys never span cells, so flags and the edge fix work per cell.
// The cells come from the top-digit histogram on the HOST (one synchronise per bucket group).
constexpr uint64_t TOP_FIRST_MIN_N = 1ull << 26;
struct TopFirstWork {
    DevBuf cells, tile_seg, hist, starts;  // capacities: cell_cap cells, tile_cap tiles (radix_sort_top_first checks them)
    uint32_t cell_cap = 0, tile_cap = 0;
    std::vector<SegInfo> h_cells;            // (stays alive until the caller has synchronised: source of an asynchronous upload)
    std::vector<unsigned long long> h_hist;
    void alloc(uint32_t cells_max, uint32_t tiles_max) {
        cell_cap = cells_max;
        tile_cap = tiles_max;
        cells.alloc((size_t)cells_max * sizeof(SegInfo));
        tile_seg.alloc((size_t)tiles_max * sizeof(uint32_t));
        hist.alloc((size_t)cells_max * 8 * 256 * sizeof(uint64_t));
        starts.alloc((size_t)cells_max * 8 * 256 * sizeof(uint64_t));
    }
};
// the non-empty cells of a bucket group in (bucket, digit) order from its top-digit counts top[b][8][256] (row 0 of every bucket);
// returns their tiles.  Throws where the counts do not add up to the buckets or the tiles leave 32 bits.
inline uint32_t rs_top_first_cells(const SegInfo* h_segs, uint32_t nseg, const unsigned long long* top, std::vector<SegInfo>& cells) {
    cells.clear();
    uint64_t tiles = 0;
    for (uint32_t b = 0; b < nseg; ++b) {
        unsigned long long at = h_segs[b].begin;
        for (uint32_t d = 0; d < 256; ++d) {
            const unsigned long long c = top[((size_t)b * 8) * 256 + d];
            if (!c) continue;
            cells.push_back(SegInfo{at, at + c, (uint32_t)tiles, d, 0ull, 0ull});
            tiles += ceil_div((uint64_t)c, (uint64_t)RS_SEG_TILE);
            at += c;
            if (tiles > 0xFFFFFFFFull) throw InternalError("radix_sort_top_first: tile count (internal)");
        }
        if (at != h_segs[b].end) throw InternalError("radix_sort_top_first: top-digit counts do not add up to the bucket (internal)");
    }
    return (uint32_t)tiles;
}
// ... checked once more by an independent walk before anything is launched over it: a cell table whose tiles do not cover its
// cells would let a pass scatter outside the record buffers
inline void rs_check_cells(const std::vector<SegInfo>& cells, uint32_t tiles, const SegInfo* h_segs, uint32_t nseg) {
    uint64_t t = 0;
    size_t c = 0;
    for (uint32_t b = 0; b < nseg; ++b) {
        unsigned long long at = h_segs[b].begin;
        while (c < cells.size() && cells[c].begin == at && at < h_segs[b].end) {
            const SegInfo& ci = cells[c];
            if (ci.end <= ci.begin || ci.end > h_segs[b].end || (uint64_t)ci.tile_begin != t || ci.rot_b)
                throw InternalError("radix_sort_top_first: cell table (internal)");
            t += (ci.end - ci.begin + (uint64_t)RS_SEG_TILE - 1) / (uint64_t)RS_SEG_TILE;
            at = ci.end;
            ++c;
        }
        if (at != h_segs[b].end) throw InternalError("radix_sort_top_first: cells do not cover their bucket (internal)");
    }
    if (c != cells.size() || t != (uint64_t)tiles) throw InternalError("radix_sort_top_first: cell tiles (internal)");
}
// the last pass over cells from the arguments the five-pass form would take: the byte-wide aux word behind the top pass holds
// entry bits 32.. (ehb of them) | carried bits and nothing of the key, which is why the pass has a type of its own
// (SegFinalCellArgs).  The edge records of `fin` are reused as 16-byte ones.
inline SegFinalCellArgs rs_top_first_fin(const SegFinalArgs& fin, int ehb) {
    if (fin.kbase != 2 || fin.kmagic != 0 || ehb < 0 || ehb > 8) throw InternalError("radix_sort_top_first: variable-length keys, at most 8 entry bits in the aux byte (internal)");
    SegFinalCellArgs c;
    c.eout = fin.eout;
    c.elo = fin.elo;
    c.ehi = fin.ehi;
    c.flags = fin.flags;
    c.edges = reinterpret_cast<SegCellEdge*>(fin.edges);
    c.hi_mask = (1u << ehb) - 1u;
    c.carry_mask = fin.carry_mask;
    c.carry_shift = ehb;
    return c;
}
// Records of m elements in buffers 0 (w0: u16 = top key byte | everything else << 8), the buckets as for radix_sort_segmented
// (h_segs: their host copy, no rotations); d_hist / d_starts: scratch [nseg][8][256].  The passes leave buffers 0 and 1 as the
// five-pass form does (the last pass reads buffers 0); fin: the last pass over the cells (rs_top_first_fin).
template <typename W>  // (uint16_t; a template so that only the build instantiates its kernels)
uint32_t radix_sort_top_first(hipStream_t s, RadixWorkspace& ws, Profiler& prof, uint32_t* k0, uint32_t* k1, uint32_t* v0, uint32_t* v1,
                                     W* w0, W* w1, uint64_t m, const SegInfo* d_segs, const SegInfo* h_segs, const uint32_t* d_tile_seg,
                                     uint32_t nseg, uint32_t tiles, unsigned long long* d_hist, unsigned long long* d_starts, TopFirstWork& tw,
                                     SegFinalCellArgs fin, SortStats* stats) {
    static_assert(std::is_same<W, uint16_t>::value, "top digit first: (u32, u32, u16) records");
    if (!rs_atomic_rank_ok(s)) throw InternalError("radix_sort_top_first: needs the one-atomic ranking (internal)");
    for (uint32_t b = 0; b < nseg; ++b)
        if (h_segs[b].rot_b) throw InternalError("radix_sort_top_first: rotated bucket (internal)");
    // top-digit histogram of every bucket (2 B per record) and the pass on it
    CDB_HIP(hipMemsetAsync(d_hist, 0, (size_t)nseg * 8 * 256 * sizeof(uint64_t), s));
    int t = prof.begin(s);
    hipLaunchKernelGGL((rs_seg_hist_kernel<W, false>), dim3((unsigned)ceil_div(tiles, (uint32_t)RS_MSD_HIST_TILES)), dim3(1024), 0, s,
                       (const uint32_t*)k0, (const W*)w0, 1, 1, d_tile_seg, d_segs, tiles, d_hist);
    prof.end(t, "rs_seg_hist_top", m * sizeof(W), s);
    tw.h_hist.resize((size_t)nseg * 8 * 256);
    CDB_HIP(hipMemcpyAsync(tw.h_hist.data(), d_hist, tw.h_hist.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));  // (the counts are on the host; the top pass is launched next and runs while the cells are built)
    hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nseg), dim3(256), 0, s, (const unsigned long long*)d_hist, d_segs, 1, d_starts);
    ws.prepare((uint64_t)tiles * RS_SEG_TILE, RS_SEG_TILE, s);
    SegShrinkArgs sh;
    sh.tile_seg = d_tile_seg;
    sh.segs = d_segs;
    sh.tiles = tiles;
    sh.start_stride = 8 * 256;
    sh.wout8 = reinterpret_cast<uint8_t*>(w1);
    t = prof.begin(s);
    rs_launch_pass_ordered<RsBig<>, W>(s, ws, tiles, k0, k1, v0, v1, m, -8, 0xFFu, (const unsigned long long*)d_starts, NoGen(), w0, w1, 0, sh);
    prof.end(t, "rs_seg_top_w16_t16384", m * (10 + 9), s);
    if (stats) stats->passes_run++;
    // the cells, built and checked on the host while the top pass runs; the synchronise behind them waits for that pass alone
    const uint32_t ctiles = rs_top_first_cells(h_segs, nseg, tw.h_hist.data(), tw.h_cells);
    rs_check_cells(tw.h_cells, ctiles, h_segs, nseg);
    CDB_HIP(hipStreamSynchronize(s));
    const uint32_t ncell = (uint32_t)tw.h_cells.size();
    if (ncell == 0 || ncell > tw.cell_cap || ctiles > tw.tile_cap) throw InternalError("radix_sort_top_first: cell scratch (internal)");
    CDB_HIP(hipMemcpyAsync(tw.cells.p, tw.h_cells.data(), (size_t)ncell * sizeof(SegInfo), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(rs_seg_tilemap_kernel, dim3((unsigned)ceil_div(ctiles, 256u)), dim3(256), 0, s, (const SegInfo*)tw.cells.as<SegInfo>(), ncell,
                       ctiles, tw.tile_seg.as<uint32_t>());
    // key-digit histograms per cell (4 B per record), then four passes over (u32, u32, u8) records from buffers 1
    uint8_t* const b0 = reinterpret_cast<uint8_t*>(w0);
    uint8_t* const b1 = reinterpret_cast<uint8_t*>(w1);
    CDB_HIP(hipMemsetAsync(tw.hist.p, 0, (size_t)ncell * 8 * 256 * sizeof(uint64_t), s));
    t = prof.begin(s);
    hipLaunchKernelGGL((rs_seg_hist_kernel<uint8_t>), dim3((unsigned)ceil_div(ctiles, (uint32_t)RS_MSD_HIST_TILES)), dim3(1024), 0, s, (const uint32_t*)k1,
                       (const uint8_t*)b1, 0, 4, (const uint32_t*)tw.tile_seg.as<uint32_t>(), (const SegInfo*)tw.cells.as<SegInfo>(), ctiles,
                       tw.hist.as<unsigned long long>());
    prof.end(t, "rs_seg_hist_cells", m * sizeof(uint32_t), s);
    radix_sort_segmented<uint8_t, SegFinalCellArgs>(s, ws, prof, k1, k0, v1, v0, b1, b0, m, (const SegInfo*)tw.cells.as<SegInfo>(), (const uint32_t*)tw.tile_seg.as<uint32_t>(), ncell,
                                  ctiles, (const unsigned long long*)tw.hist.as<unsigned long long>(), tw.starts.as<unsigned long long>(), 32, 0, fin, stats);
    return ncell;
}

// ---------------------------------------------------------------------------------------------
// tile bases of the look-back-free generated passes (TextGen::tile_base)
// ---------------------------------------------------------------------------------------------
// counts[rows][256] (u32) = how many elements of tile `row` carry each digit, from a counting sweep over the text (the digit of a
// generated pass is a function of one or two symbols).  base[row][d] = digit_start[d] + sum of counts[r][d] over r < row: the
// output slot of the tile's first element of digit d.  Column d of the result reads column src_col[d] of the counts (nullptr =
// identity; 0xFFFF = no such column: the bucket-wise passes count raw bytes and sort on bucket slots).  Three small kernels:
// column sums per block of RS_TB_ROWS rows, a scan over the blocks, the running sums inside every block.
constexpr int RS_GEN8_TILE = 8192;  // 512 threads x 16 keys: two workgroups per CU
constexpr uint32_t RS_TB_ROWS = 256;
static __global__ __launch_bounds__(256) void rs_tilecol_sum_kernel(const uint32_t* __restrict__ counts, uint32_t rows, const uint16_t* __restrict__ src_col,
                                                                    unsigned long long* __restrict__ partial) {
    const uint32_t d = threadIdx.x, b = blockIdx.x;
    const uint32_t c = src_col ? (uint32_t)src_col[d] : d;
    const uint32_t r0 = b * RS_TB_ROWS, r1 = r0 + RS_TB_ROWS < rows ? r0 + RS_TB_ROWS : rows;
    unsigned long long sum = 0;
    if (c < 256u)
        for (uint32_t r = r0; r < r1; ++r) sum += counts[(size_t)r * 256 + c];
    partial[(size_t)b * 256 + d] = sum;
}
// totals[d] = column sums over all blocks (what the host wants as the digit histogram).  ONE workgroup (the result is 256 numbers),
// but 1024 threads: four quarters of the blocks side by side, eight loads in flight per thread — a 256-thread loop with one load
// per trip took 2.9 ms for the 8192 blocks of a 16 GiB text, all of it latency
static __global__ __launch_bounds__(1024) void rs_tilecol_total_kernel(const unsigned long long* __restrict__ partial, uint32_t blocks,
                                                                       unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long s_q[4][256];
    const uint32_t d = threadIdx.x & 255u, g = threadIdx.x >> 8;
    const uint32_t per = (blocks + 3u) / 4u;
    const uint32_t b0 = g * per, b1 = b0 + per < blocks ? b0 + per : blocks;
    unsigned long long sum = 0;
    uint32_t b = b0;
    for (; b + 8 <= b1; b += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = partial[(size_t)(b + i) * 256 + d];
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
    }
    for (; b < b1; ++b) sum += partial[(size_t)b * 256 + d];
    s_q[g][d] = sum;
    __syncthreads();
    if (g == 0) totals[d] = s_q[0][d] + s_q[1][d] + s_q[2][d] + s_q[3][d];
}
// blockbase[b][d] = digit_start[d] + sum of partial[b'][d], b' < b (same shape: quarter sums first, then every quarter's running sums)
static __global__ __launch_bounds__(1024) void rs_tilecol_scan_kernel(const unsigned long long* __restrict__ partial, uint32_t blocks,
                                                                      const unsigned long long* __restrict__ digit_start,
                                                                      unsigned long long* __restrict__ blockbase) {
    __shared__ unsigned long long s_q[4][256];
    const uint32_t d = threadIdx.x & 255u, g = threadIdx.x >> 8;
    const uint32_t per = (blocks + 3u) / 4u;
    const uint32_t b0 = g * per < blocks ? g * per : blocks, b1 = b0 + per < blocks ? b0 + per : blocks;
    unsigned long long sum = 0;
    uint32_t b = b0;
    for (; b + 8 <= b1; b += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = partial[(size_t)(b + i) * 256 + d];
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
    }
    for (; b < b1; ++b) sum += partial[(size_t)b * 256 + d];
    s_q[g][d] = sum;
    __syncthreads();
    unsigned long long run = digit_start[d];
    for (uint32_t q = 0; q < g; ++q) run += s_q[q][d];
    b = b0;
    for (; b + 8 <= b1; b += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = partial[(size_t)(b + i) * 256 + d];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            blockbase[(size_t)(b + i) * 256 + d] = run;
            run += v[i];
        }
    }
    for (; b < b1; ++b) {
        blockbase[(size_t)b * 256 + d] = run;
        run += partial[(size_t)b * 256 + d];
    }
}
static __global__ __launch_bounds__(256) void rs_tilecol_apply_kernel(const uint32_t* __restrict__ counts, uint32_t rows, const uint16_t* __restrict__ src_col,
                                                                      const unsigned long long* __restrict__ blockbase,
                                                                      unsigned long long* __restrict__ base) {
    const uint32_t d = threadIdx.x, b = blockIdx.x;
    const uint32_t c = src_col ? (uint32_t)src_col[d] : d;
    const uint32_t r0 = b * RS_TB_ROWS, r1 = r0 + RS_TB_ROWS < rows ? r0 + RS_TB_ROWS : rows;
    unsigned long long run = blockbase[(size_t)b * 256 + d];
    for (uint32_t r = r0; r < r1; ++r) {
        base[(size_t)r * 256 + d] = run;
        if (c < 256u) run += counts[(size_t)r * 256 + c];
    }
}
struct TileBaseWorkspace {
    DevBuf partial, blockbase, totals, base;
    void release() { partial.release(); blockbase.release(); totals.release(); base.release(); }
};
// column totals of the counts (device, [256] u64) — the digit histogram the host builds its buckets from
inline const unsigned long long* rs_tile_totals(hipStream_t s, TileBaseWorkspace& tb, const uint32_t* d_counts, uint32_t rows, const uint16_t* d_src_col) {
    const uint32_t blocks = (uint32_t)ceil_div((uint64_t)rows, (uint64_t)RS_TB_ROWS);
    tb.partial.ensure((size_t)blocks * 256 * sizeof(uint64_t));
    tb.totals.ensure(256 * sizeof(uint64_t));
    hipLaunchKernelGGL(rs_tilecol_sum_kernel, dim3(blocks), dim3(256), 0, s, d_counts, rows, d_src_col, tb.partial.as<unsigned long long>());
    hipLaunchKernelGGL(rs_tilecol_total_kernel, dim3(1), dim3(1024), 0, s, (const unsigned long long*)tb.partial.as<unsigned long long>(), blocks,
                       tb.totals.as<unsigned long long>());
    return tb.totals.as<unsigned long long>();
}
// ... and the tile bases, once the digit starts are on the device (the block sums are taken again: the column map may differ
// from the one the totals were made with — raw bytes there, bucket slots here)
inline const unsigned long long* rs_tile_bases(hipStream_t s, TileBaseWorkspace& tb, const uint32_t* d_counts, uint32_t rows, const uint16_t* d_src_col,
                                               const unsigned long long* d_digit_start) {
    const uint32_t blocks = (uint32_t)ceil_div((uint64_t)rows, (uint64_t)RS_TB_ROWS);
    tb.partial.ensure((size_t)blocks * 256 * sizeof(uint64_t));
    tb.blockbase.ensure((size_t)blocks * 256 * sizeof(uint64_t));
    tb.base.ensure((size_t)rows * 256 * sizeof(uint64_t));
    hipLaunchKernelGGL(rs_tilecol_sum_kernel, dim3(blocks), dim3(256), 0, s, d_counts, rows, d_src_col, tb.partial.as<unsigned long long>());
    hipLaunchKernelGGL(rs_tilecol_scan_kernel, dim3(1), dim3(1024), 0, s, (const unsigned long long*)tb.partial.as<unsigned long long>(), blocks,
                       d_digit_start, tb.blockbase.as<unsigned long long>());
    hipLaunchKernelGGL(rs_tilecol_apply_kernel, dim3(blocks), dim3(256), 0, s, d_counts, rows, d_src_col,
                       (const unsigned long long*)tb.blockbase.as<unsigned long long>(), tb.base.as<unsigned long long>());
    return tb.base.as<unsigned long long>();
}

// (records_sweep.h) the generated pass of radix_sort_msd in two phases: rank on the staged top digits, generate in output order
__global__ __launch_bounds__(512, 8) void rs_sweep_msd_kernel(TextGen gen, uint64_t n, uint32_t tiles, uint32_t* __restrict__ kout,
                                                              uint32_t* __restrict__ vout);

struct MsdWorkspace {
    DevBuf segs, tile_seg, hist, starts;
    void release() { segs.release(); tile_seg.release(); hist.release(); starts.release(); }
};

// Sorts the records the generator produces (key = up to 32 + 8 bits, msd_shift = 32) — see above.  h_top[256] = counts of
// the top digit (host).  Result: entries in v1, kept search keys (u32)(key >> 8) in k1 and key & 0xFF in wout, the group
// flags / edge fixes / tile sums of `keep` written by the last pass.  k0 / v0 are scratch.
inline void radix_sort_msd(hipStream_t s, RadixWorkspace& ws, MsdWorkspace& mw, Profiler& prof, uint32_t* k0, uint32_t* k1,
                           uint32_t* v0, uint32_t* v1, uint8_t* wout, uint64_t n, const uint64_t* h_top, const TextGen& gen_in,
                           unsigned long long msd_m, const SegFinalKeepArgs& keep_in, SortStats* stats,
                           const uint32_t* d_tile_counts = nullptr, TileBaseWorkspace* tbw = nullptr, bool sweep_form = true) {
    // gen_in says how the generated pass splits a key into (top digit, u32 rest): msd_shift = 32 (msd_m = 2^32) or the pair
    // form (msd_m = span * base^4); the last pass puts the full key together again as top * msd_m + rest
    if (!rs_atomic_rank_ok(s)) throw InternalError("radix_sort_msd: needs the one-atomic ranking (internal)");
    constexpr int TILE = RS_SEG_TILE;
    constexpr int KPASS = 4;
    // segments = the non-empty buckets of the top digit
    std::vector<SegInfo> h_segs;
    uint32_t seg_tiles = 0;
    {
        uint64_t at = 0;
        for (int d = 0; d < 256; ++d) {
            if (!h_top[d]) continue;
            h_segs.push_back(SegInfo{(unsigned long long)at, (unsigned long long)(at + h_top[d]), seg_tiles, (uint32_t)d, 0ull, 0ull});
            seg_tiles += (uint32_t)ceil_div(h_top[d], (uint64_t)TILE);
            at += h_top[d];
        }
        if (at != n) throw InternalError("radix_sort_msd: top-digit histogram does not add up (internal)");
    }
    const uint32_t nseg = (uint32_t)h_segs.size();
    const uint32_t gen_tiles = (uint32_t)ceil_div(n, (uint64_t)TILE);
    ws.prepare((uint64_t)seg_tiles * TILE, TILE, s);
    ws.keep_applied = false;
    unsigned long long* d_hist = ws.hist.as<unsigned long long>();
    unsigned long long* d_start = d_hist + RS_MAX_PASSES * 256;
    mw.segs.ensure(nseg * sizeof(SegInfo));
    mw.tile_seg.ensure((size_t)seg_tiles * sizeof(uint32_t));
    mw.hist.ensure((size_t)nseg * 8 * 256 * sizeof(uint64_t));
    mw.starts.ensure((size_t)nseg * 8 * 256 * sizeof(uint64_t));
    CDB_HIP(hipMemcpyAsync(d_hist, h_top, 256 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    CDB_HIP(hipMemcpyAsync(mw.segs.p, h_segs.data(), nseg * sizeof(SegInfo), hipMemcpyHostToDevice, s));
    CDB_HIP(hipStreamSynchronize(s));  // (pageable host memory)
    hipLaunchKernelGGL(rs_digit_start_kernel, dim3(1), dim3(256), 0, s, d_hist, d_start);
    hipLaunchKernelGGL(rs_seg_tilemap_kernel, dim3((unsigned)ceil_div(seg_tiles, 256u)), dim3(256), 0, s, mw.segs.as<SegInfo>(), nseg,
                       seg_tiles, mw.tile_seg.as<uint32_t>());
    CDB_HIP(hipMemsetAsync(mw.hist.p, 0, (size_t)nseg * 8 * 256 * sizeof(uint64_t), s));
    // ---- generated pass: partition by the top digit, records (u32 key, entry)
    if (d_tile_counts && tbw && gen_in.msd_pair) {
        // look-back-free form: per-tile counts of the top digit (sa_build.hip: sa_tile_paircount_kernel, rs_tile_totals already ran on
        // them) -> tile bases; 8 Ki-key tiles, two workgroups per CU, no status words, no waiting for other tiles
        constexpr int GT = RS_GEN8_TILE;
        const uint32_t gen_tiles8 = (uint32_t)ceil_div(n, (uint64_t)GT);
        TextGenPair gp;
        static_cast<TextGen&>(gp) = gen_in;
        gp.low_bits = 0;
        gp.tile_base = rs_tile_bases(s, *tbw, d_tile_counts, gen_tiles8, nullptr, (const unsigned long long*)d_start);
        rs_gen_tile_docs(s, ws, gp, n, GT);
        int t = prof.begin(s);
        if (sweep_form)  // (no record crosses the LDS, three workgroups per CU; static XCD-aware tile map)
            hipLaunchKernelGGL(rs_sweep_msd_kernel, dim3((uint32_t)(ceil_div(gen_tiles8, 8u * RS_GROUP) * 8u * RS_GROUP)), dim3(512), 0, s,
                               static_cast<const TextGen&>(gp), n, gen_tiles8, k1, v1);
        else
            rs_launch_pass_ordered<RsGen8, uint8_t>(s, ws, gen_tiles8, nullptr, k1, nullptr, v1, n, 0, 0xFFu, d_start, gp, nullptr, nullptr, 0);
        prof.end(t, sweep_form ? "rs_sweep_msd" : "rs_onesweep_textgen_msd_t8192", n * 9, s);
        if (stats) stats->passes_run++;
    } else {
        TextGen g2 = gen_in;
        g2.low_bits = 0;
        rs_gen_tile_docs(s, ws, g2, n, TILE);
        int t = prof.begin(s);
        if (g2.msd_pair) {  // (the generator's form is part of the kernel's type)
            TextGenPair gp;
            static_cast<TextGen&>(gp) = g2;
            rs_launch_pass_ordered<RsBig<>, uint8_t>(s, ws, gen_tiles, nullptr, k1, nullptr, v1, n, 0, 0xFFu, d_start, gp, nullptr, nullptr, 0);
        } else {
            rs_launch_pass_ordered<RsBig<>, uint8_t>(s, ws, gen_tiles, nullptr, k1, nullptr, v1, n, 0, 0xFFu, d_start, g2, nullptr, nullptr, 0);
        }
        prof.end(t, "rs_onesweep_textgen_msd_t16384", n * 9, s);
        if (stats) stats->passes_run++;
    }
    // ---- digit histograms of every bucket's four passes
    {
        int t = prof.begin(s);
        hipLaunchKernelGGL((rs_seg_hist_kernel<uint8_t>), dim3((unsigned)ceil_div(seg_tiles, (uint32_t)RS_MSD_HIST_TILES)), dim3(1024), 0, s,
                           (const uint32_t*)k1, (const uint8_t*)nullptr, 0, KPASS, (const uint32_t*)mw.tile_seg.as<uint32_t>(),
                           (const SegInfo*)mw.segs.as<SegInfo>(), seg_tiles, mw.hist.as<unsigned long long>());
        prof.end(t, "rs_seg_hist", n * 4, s);
        hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nseg), dim3(256), 0, s, (const unsigned long long*)mw.hist.as<unsigned long long>(),
                           (const SegInfo*)mw.segs.as<SegInfo>(), KPASS, mw.starts.as<unsigned long long>());
    }
    // ---- the buckets' LSD passes, one segmented launch each; the last one writes flags + kept keys
    SegArgs sa;
    sa.tile_seg = mw.tile_seg.as<uint32_t>();
    sa.segs = mw.segs.as<SegInfo>();
    sa.tiles = seg_tiles;
    sa.start_stride = 8 * 256;
    SegFinalKeepMsdArgs ka;
    static_cast<SegFinalKeepArgs&>(ka) = keep_in;
    static_cast<SegArgs&>(ka) = sa;
    ka.low_bits = 0;
    ka.msd_m = msd_m;
    uint32_t* kb[2] = {k0, k1};
    uint32_t* vb[2] = {v0, v1};
    int cur = 1;
    for (int p = 0; p < KPASS; ++p) {
        const unsigned long long* dstart = mw.starts.as<unsigned long long>() + (size_t)p * 256;
        int t = prof.begin(s);
        if (p + 1 < KPASS) {
            rs_launch_pass_ordered<RsMsdBucket>(s, ws, seg_tiles, kb[cur], kb[cur ^ 1], vb[cur], vb[cur ^ 1], n, 8 * p, 0xFFu, dstart, NoGen(), nullptr,
                                                nullptr, -1, sa);
            prof.end(t, "rs_seg_k32_v32_t16384", 2 * n * 8, s);
        } else {
            rs_launch_pass_ordered<RsMsdBucket, uint8_t>(s, ws, seg_tiles, kb[cur], kb[cur ^ 1], vb[cur], vb[cur ^ 1], n, 8 * p, 0xFFu, dstart, NoGen(),
                                                         nullptr, wout, -1, ka);
            prof.end(t, "rs_seg_k32_v32_flags_t16384", n * (8 + 9 + 1), s);
        }
        cur ^= 1;
        if (stats) stats->passes_run++;
    }
    // (cur == 1: four passes from buffers 1 end in buffers 1)
    {
        int t = prof.begin(s);
        hipLaunchKernelGGL(rs_seg_edge_fix_kernel, dim3(seg_tiles), dim3(256), 0, s, (const SegEdge*)ka.edges, (const uint32_t*)mw.tile_seg.as<uint32_t>(),
                           (const SegInfo*)mw.segs.as<SegInfo>(), seg_tiles, ka.flags, ka.kbase, ka.kmagic, ka.tile_sums, ka.sums_tile, (const uint32_t*)ws.err_ptr());
        prof.end(t, "rs_seg_edge_fix", (uint64_t)seg_tiles * 256 * sizeof(SegEdge), s);
    }
    ws.keep_applied = true;
    CDB_HIP(hipGetLastError());
}

// Bucket-wise build (>= 2^32 suffixes), fused form: ONE generated pass writes the packed bucket records (TextGen::rec_mode)
// of every first-symbol bucket into buffers (k, v, w) — the entries are never partitioned on their own and no gather
// re-reads the text in bucket order — and a sweep over the records counts the digit histograms of every bucket's passes
// (d_hist_out: [nseg][8][256], zeroed here).  h_first[256]: suffixes per bucket slot.  radix_sort_segmented follows.
template <typename W>
void radix_gen_records(hipStream_t s, RadixWorkspace& ws, Profiler& prof, uint32_t* k, uint32_t* v, W* w, uint64_t n, const uint64_t* h_first,
                       const TextGen& gen_in, const uint32_t* d_tile_seg, const SegInfo* d_segs, uint32_t nseg, uint32_t seg_tiles, int lead,
                       int npass, unsigned long long* d_hist_out, SortStats* stats,
                       const uint32_t* d_tile_counts = nullptr, const uint16_t* d_src_col = nullptr, TileBaseWorkspace* tbw = nullptr) {
    if (!rs_atomic_rank_ok(s)) throw InternalError("radix_gen_records: needs the one-atomic ranking (internal)");
    constexpr int TILE = RS_SEG_TILE;
    const uint32_t gen_tiles = (uint32_t)ceil_div(n, (uint64_t)TILE);
    ws.prepare((uint64_t)std::max(gen_tiles, seg_tiles) * TILE, TILE, s);
    unsigned long long* d_hist = ws.hist.as<unsigned long long>();
    unsigned long long* d_start = d_hist + RS_MAX_PASSES * 256;
    CDB_HIP(hipMemcpyAsync(d_hist, h_first, 256 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    CDB_HIP(hipStreamSynchronize(s));  // (pageable host memory)
    hipLaunchKernelGGL(rs_digit_start_kernel, dim3(1), dim3(256), 0, s, d_hist, d_start);
    CDB_HIP(hipMemsetAsync(d_hist_out, 0, (size_t)nseg * 8 * 256 * sizeof(uint64_t), s));
    TextGenRec g2;
    static_cast<TextGen&>(g2) = gen_in;
    rs_gen_tile_docs(s, ws, g2, n, TILE);
    int t = prof.begin(s);
    if (d_tile_counts && tbw) {
        // look-back-free form (TextGen::tile_base): per-tile byte counts (sa_build.hip: sa_tile_bytecount_kernel), columns mapped
        // byte -> bucket slot, scanned over the tiles; 8 Ki-key tiles, two workgroups per CU
        constexpr int GT = RS_GEN8_TILE;
        const uint32_t tiles8 = (uint32_t)ceil_div(n, (uint64_t)GT);
        g2.tile_base = rs_tile_bases(s, *tbw, d_tile_counts, tiles8, d_src_col, (const unsigned long long*)d_start);
        rs_gen_tile_docs(s, ws, g2, n, GT);  // (again, for this form's tiles)
        rs_launch_pass_ordered<RsGen8, W>(s, ws, tiles8, nullptr, k, nullptr, v, n, 0, 0xFFu, d_start, g2, nullptr, w, -1);
    } else {
        rs_launch_pass_ordered<RsBig<>, W>(s, ws, gen_tiles, nullptr, k, nullptr, v, n, 0, 0xFFu, d_start, g2, nullptr, w, -1);
    }
    prof.end(t, (std::string("rs_onesweep_textgen_records") + (sizeof(W) == 1 ? "_w8" : (sizeof(W) == 2 ? "_w16" : "_w32")) + "_t16384").c_str(),
             n * (1 + 8 + sizeof(W)), s);
    if (stats) stats->passes_run++;
    t = prof.begin(s);
    hipLaunchKernelGGL((rs_seg_hist_kernel<W>), dim3((unsigned)ceil_div(seg_tiles, (uint32_t)RS_MSD_HIST_TILES)), dim3(1024), 0, s, (const uint32_t*)k,
                       (const W*)w, lead, npass, d_tile_seg, d_segs, seg_tiles, d_hist_out);
    prof.end(t, "rs_seg_hist", n * (4 + (lead > 0 ? sizeof(W) : 0)), s);
    CDB_HIP(hipGetLastError());
}

}  // namespace cdb
