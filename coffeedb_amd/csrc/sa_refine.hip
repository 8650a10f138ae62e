// sa_refine.hip — the refinement rounds of the suffix-array build (step 4 of sa_build.hip): only groups of still-equal keys are
// touched again, by text extension while few suffixes are open, by carried bits where the initial sort left some, then by prefix
// doubling over an inverse array.  refine_groups is the phase; its buffers (RefineBuffers) belong to build_typed.
#include <algorithm>
#include <cstdlib>

#include "sa_build_phases.h"
#include "scan.h"
#include "carried_inplace.h"

namespace cdb {
namespace {

// (FlagIn, the group flags as scan input with their 16-byte loader: scan.h)

// compaction of the unresolved entries + construction of their sort keys
// compaction of the unresolved entries: slot number, entry and group id of every unresolved entry
// (the sort key's minor part is filled in by sa_round_keys_kernel, one dense thread per entry)
// (SAW = how the suffix array is stored: SaRW<V> or the packed Sa40RW, index_impl.h)
template <typename SAW, typename I>
struct CompactOut {
    using V = typename SAW::val;
    SAW sa;
    I* U;
    uint64_t* skey;
    V* sval;
    int kbits;
    __device__ __forceinline__ void operator()(uint64_t i, const U2& ex, const U2& in) const {
        if (in.a == ex.a) return;  // not an unresolved entry
        const uint64_t j = ex.a;
        U[j] = (I)i;
        skey[j] = (in.b - 1) << kbits;  // group id
        sval[j] = sa.load(i);
    }
};

// The compaction of the CARRIED round (refine_groups): the minor key is complete at once — the code-stream bits the initial sort
// left in bits 2.. of the entry's flag byte (the sweep has just read that byte: the line is hot), so no sa_round_keys launch follows.
template <typename SAW, typename I>
struct CompactCarriedOut {
    using V = typename SAW::val;
    SAW sa;
    const uint8_t* flags;
    I* U;
    uint64_t* skey;
    V* sval;
    int kbits;  // = carried bits
    __device__ __forceinline__ void operator()(uint64_t i, const U2& ex, const U2& in) const {
        if (in.a == ex.a) return;  // not an unresolved entry
        const uint64_t j = ex.a;
        U[j] = (I)i;
        skey[j] = ((in.b - 1) << kbits) | (uint64_t)(((uint32_t)flags[i] >> 2) & ((1u << kbits) - 1u));
        sval[j] = sa.load(i);
    }
};

// The same compaction from the PREVIOUS round's list (text-extension rounds behind the first): only entries of that list can still be
// open, and sa_update left their new flag bytes in list order (`lf`), so the wave-autonomous flag sweeps run over m bytes instead of
// the array's n, and the entries come from the sorted list instead of a gather through the suffix array.
template <typename V, typename I>
struct CompactListOut {
    const I* Uo;
    const V* svo;
    I* U;
    uint64_t* skey;
    V* sval;
    int kbits;
    __device__ __forceinline__ void operator()(uint64_t j, const U2& ex, const U2& in) const {
        if (in.a == ex.a) return;  // not an unresolved entry
        const uint64_t jj = ex.a;
        U[jj] = Uo[j];
        skey[jj] = (in.b - 1) << kbits;  // group id
        sval[jj] = svo[j];
    }
};

// minor sort key of every compacted entry: the rank of the suffix h symbols further on (prefix
// doubling) or the next nsym2 symbols read from the text (text extension)
template <typename V, typename R, bool USE_ISA>
__global__ __launch_bounds__(256) void sa_round_keys_kernel(const V* __restrict__ sval, uint64_t m,
                                                            const uint64_t* __restrict__ doc_start,
                                                            const uint8_t* __restrict__ text,
                                                            const uint16_t* __restrict__ symmap,
                                                            const R* __restrict__ rank, int bits, uint64_t mask, uint64_t h,
                                                            int nsym2, int symbits, uint64_t* __restrict__ skey, uint64_t n_text,
                                                            const uint8_t* __restrict__ vl_len = nullptr, uint32_t vl_kb1 = 0,
                                                            uint32_t h_extra = 0, uint8_t* __restrict__ hcov = nullptr) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const V v = sval[j];
    const uint64_t d = (uint64_t)v & mask, off = (uint64_t)v >> bits;
    const uint64_t ds = doc_start[d];
    if (!USE_ISA && vl_len) {
        // variable-length keys (vl_code.h): the symbols the initial key covered IN FULL — the bucket symbol + the code words that fit
        // its vl_kb1 bits — are equal throughout the entry's group (equal keys decode alike), so the round may start behind them
        const uint64_t len = doc_start[d + 1] - ds - off;
        const uint8_t* q = text + ds + off;
        // (the first symbols by aligned 8-byte loads, like the keys below: byte loads in suffix order cost a line each)
        const uint64_t pa = (uint64_t)q & ~7ull;
        const uint32_t sh = (uint32_t)((uint64_t)q & 7ull) * 8u;
        const uint64_t tend = (uint64_t)(text + n_text);
        const uint64_t w0 = *reinterpret_cast<const uint64_t*>(pa);
        const uint64_t w1 = pa + 8 < tend ? *reinterpret_cast<const uint64_t*>(pa + 8) : 0ull;
        const uint64_t w2 = pa + 16 < tend ? *reinterpret_cast<const uint64_t*>(pa + 16) : 0ull;
        const uint64_t b0 = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;  // bytes q[0] .. q[7]
        const uint64_t b1 = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;  // bytes q[8] .. q[15]
        uint32_t used = 0, cov = 1;
        while ((uint64_t)cov < len && cov < 200u) {
            const uint32_t byte = cov < 8u ? (uint32_t)(b0 >> (8u * cov)) & 0xFFu : (cov < 16u ? (uint32_t)(b1 >> (8u * (cov - 8u))) & 0xFFu : (uint32_t)q[cov]);
            used += vl_len[byte];
            if (used > vl_kb1) break;
            ++cov;
        }
        hcov[j] = (uint8_t)cov;
        h = (uint64_t)cov + h_extra;
    }
    uint64_t key2 = 0;
    if constexpr (USE_ISA) {
        key2 = (uint64_t)rank[ds + d + off + h];  // extended position: one end slot per document
    } else {
        const uint64_t rem = doc_start[d + 1] - ds - off - h;  // >= 0: unresolved => length >= h
        const uint8_t* p = text + ds + off + h;
        if (nsym2 <= 9 && rem > 0) {
            // the next symbols by TWO aligned 8-byte loads instead of one load per byte: the entries arrive in suffix order, every
            // load instruction of a wave touches 64 different lines, and with thousands of gathers in flight per CU a line does not
            // survive in the L1 from one byte to the next (16 GiB shard: 310 B of fabric traffic per entry with byte loads).  The
            // second word is read only where it holds a byte of the text (an aligned word never crosses a page)
            const uint64_t pa = (uint64_t)p & ~7ull;
            const uint32_t sh = (uint32_t)((uint64_t)p & 7ull) * 8u;
            const uint64_t w0 = *reinterpret_cast<const uint64_t*>(pa);
            const uint64_t w1 = pa + 8 < (uint64_t)(text + n_text) ? *reinterpret_cast<const uint64_t*>(pa + 8) : 0ull;
            const uint64_t lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;  // bytes p[0] .. p[7]
            const uint32_t b8 = (uint32_t)(w1 >> sh) & 0xFFu;                 // byte p[8]
            for (int k = 0; k < nsym2; ++k) {
                const uint32_t byte = k < 8 ? (uint32_t)(lo >> (8 * k)) & 0xFFu : b8;
                const uint64_t sym = (uint64_t)k < rem ? (uint64_t)symmap[byte] : 0ull;
                key2 = (key2 << symbits) | sym;
            }
        } else {
            for (int k = 0; k < nsym2; ++k) {
                const uint64_t sym = (uint64_t)k < rem ? (uint64_t)symmap[p[k]] : 0ull;
                key2 = (key2 << symbits) | sym;
            }
        }
    }
    skey[j] |= key2;
}

// Compaction of the unresolved entries, specialised for the byte-flag array (the generic scan spends most of its time carrying
// 16 (u64, u64) pairs per thread for entries that are almost all resolved).  Round 4: WAVE-autonomous — a wavefront owns whole
// tiles of the scan geometry (SC_TILE = 4096 flags = four 1 KiB chunks of 16 bytes per lane), counts with SWAR popcounts, scans
// with wave shuffles and takes its tiles one after the other: no LDS, no workgroup barrier, millions of 4 KiB workgroups less
// (the compaction itself stays bound by its gather of the unresolved entries).  sa_flag_count_kernel leaves the raw tile sums (unresolved entries, unresolved group
// heads) in the partials of scan.h's layout; sa_flag_compact_kernel uses their exclusive scan.
// (FC_TILES_PER_WAVE, fc_load, fc_count: carried_inplace.h, shared with the in-place carried round)
__global__ __launch_bounds__(256) void sa_flag_count_kernel(const uint8_t* __restrict__ flags, uint64_t n, uint64_t tiles, U2* __restrict__ partials) {
    static_assert(SC_TILE == 4096, "flag compaction assumes 4096-flag tiles");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4 + wave) * FC_TILES_PER_WAVE;
#pragma unroll
    for (uint32_t k = 0; k < FC_TILES_PER_WAVE; ++k) {
        const uint64_t tile = t0 + k;
        if (tile >= tiles) break;  // (uniform per wavefront)
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t x[4];
            fc_load(flags, n, tile * SC_TILE + (uint64_t)c * 1024 + (uint64_t)lane * 16, x);
            v += fc_count(x);  // (both halves stay below 2^16: at most 4096 per tile)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) partials[tile] = U2{(uint64_t)(v & 0xFFFFu), (uint64_t)(v >> 16)};
    }
}
// Round 6: the flagged entries of a tile are first LISTED (12-bit offset + head bit, in order, in a wave-private stretch of the
// LDS) and then handed to `out` DENSELY, 64 per wave instruction.  The round-4 form called `out` — a gather through the suffix
// array and three stores — from a 16-trip loop over the lane's bytes: with 2.4 % of the flags set (8 GiB of Zipf text) that were 64
// sparse trips per tile, ~450 memory instructions with one or two lanes alive each, and the sweep took 10.4 ms where the bare
// count over the same flags takes 1.5 ms.
template <typename Out>
__global__ __launch_bounds__(256) void sa_flag_compact_kernel(const uint8_t* __restrict__ flags, uint64_t n, uint64_t tiles,
                                                              const U2* __restrict__ partials, Out out) {
    static_assert(SC_TILE == 4096, "flag compaction assumes 4096-flag tiles");
    __shared__ uint16_t s_list[4][SC_TILE];  // per wave: the tile's unresolved positions (offset | head << 12), worst case all of them
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint16_t* const list = s_list[wave];
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4 + wave) * FC_TILES_PER_WAVE;
    for (uint32_t k = 0; k < FC_TILES_PER_WAVE; ++k) {
        const uint64_t tile = t0 + k;
        if (tile >= tiles) break;  // (uniform per wavefront)
        uint32_t x[4][4], v[4], incl[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) fc_load(flags, n, tile * SC_TILE + (uint64_t)c * 1024 + (uint64_t)lane * 16, x[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) incl[c] = v[c] = fc_count(x[c]);
        // element order inside the tile = (chunk, lane, byte): one wave scan per chunk (independent: their shuffles interleave)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t y = __shfl_up(incl[c], off);
                if (lane >= off) incl[c] += y;
            }
        }
        uint32_t any = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) any |= v[c];
        if (__builtin_amdgcn_ballot_w64(any != 0) == 0) continue;  // (nothing unresolved in the tile)
        const U2 tile_run = partials[tile];
        // ---- phase 1: list the unresolved positions in order (a lane walks the SET bits of its 16 bytes only)
        uint32_t cpre = 0;  // packed counts of the chunks in front
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t ctot = __shfl(incl[c], 63);
            if (v[c] & 0xFFFFu) {
                uint32_t slot = (cpre + incl[c] - v[c]) & 0xFFFFu;
                uint32_t um = 0, hm = 0;  // bit q: byte q is unresolved / an unresolved group head
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint32_t u = (x[c][w] >> 1) & 0x01010101u;
                    um |= (((u * 0x01020408u) >> 24) & 0xFu) << (4 * w);
                    hm |= ((((u & x[c][w]) * 0x01020408u) >> 24) & 0xFu) << (4 * w);
                }
                const uint32_t off0 = (uint32_t)c * 1024u + (uint32_t)lane * 16u;
                while (um) {
                    const uint32_t q = (uint32_t)__builtin_ctz(um);
                    um &= um - 1u;
                    list[slot++] = (uint16_t)((off0 + q) | (((hm >> q) & 1u) << 12));
                }
            }
            cpre += ctot;
        }
        const uint32_t total = cpre & 0xFFFFu;
        // (the list is the wave's own: its LDS operations execute in program order — the fences keep the compiler from moving them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- phase 2: one unresolved entry per lane
        uint32_t heads = 0;  // unresolved group heads in front of this trip
        for (uint32_t b0 = 0; b0 < total; b0 += 64u) {
            const uint32_t t = b0 + (uint32_t)lane;
            const bool live = t < total;
            const uint32_t e = live ? (uint32_t)list[t] : 0u;
            const uint32_t head = (e >> 12) & 1u;
            const uint64_t hb = __builtin_amdgcn_ballot_w64(head != 0);
            if (live) {
                const U2 run{tile_run.a + t, tile_run.b + heads + (uint64_t)__popcll(hb & lt_mask)};
                const U2 nxt{run.a + 1, run.b + head};
                out(tile * SC_TILE + (uint64_t)(e & 0xFFFu), run, nxt);
            }
            heads += (uint32_t)__popcll(hb);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next tile's list overwrites this one's)
        __builtin_amdgcn_wave_barrier();
    }
}

// The refinement's sort, specialised for what it sorts: the compacted list is ALREADY ordered by group (the group id sits in the
// key's high bits and ascends with the list), so "sort by (group, minor key)" only permutes entries INSIDE their group — runs of two
// or three entries on every named configuration (8 GiB of Zipf text: 28 242 of 2.07 x 10^8 entries sit in groups of more than 49,
// 6 in groups of more than 257).  One pass instead of the general sort's eight: an entry looks at the members of its group on both
// sides (neighbouring list slots: cached lines) and takes the slot
//     j - #{members in front with a greater key} + #{members behind with a smaller key}
// — the stable order, slot for slot what the LSD passes produce.  The work is the sum of the SQUARED group sizes, so it is bounded:
// an entry that walks more than GS_FREE members reports its walk to a global counter, and once the walks add up to more than
// `budget` members (16 per entry of the list), or a group exceeds `cap` members on one side of an entry, `state[0]` is raised — every
// thread gives up at its next look at it and the caller falls back to the general sort (duplicated documents: groups of thousands).
constexpr uint32_t GS_FREE = 32;  // (walks this short cost no more than the general sort would: never reported)
template <typename V>
__global__ __launch_bounds__(256) void sa_group_sort_kernel(const uint64_t* __restrict__ kin, const V* __restrict__ vin, uint64_t m, int kbits, uint32_t cap,
                                                            unsigned long long budget, uint64_t* __restrict__ kout, V* __restrict__ vout,
                                                            unsigned long long* __restrict__ state /* [0] gave up, [1] members walked by long walks */) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const volatile unsigned long long* vstate = state;
    if (vstate[0]) return;
    const uint64_t k = kin[j];
    const uint64_t g = kbits >= 64 ? 0ull : k >> kbits;
    auto gid = [&](uint64_t x) { return kbits >= 64 ? 0ull : x >> kbits; };
    uint64_t pos = j;
    uint32_t walked = 0;
    bool too = false;
    {
        uint32_t d = 1;
        for (; d <= cap && j >= d; ++d) {
            const uint64_t o = kin[j - d];
            if (gid(o) != g) break;
            pos -= (uint64_t)(o > k);
            if ((d & 127u) == 0 && vstate[0]) return;
        }
        too = d > cap && j >= d && gid(kin[j - d]) == g;
        walked += d - 1;
    }
    if (!too) {
        uint32_t d = 1;
        for (; d <= cap && j + d < m; ++d) {
            const uint64_t o = kin[j + d];
            if (gid(o) != g) break;
            pos += (uint64_t)(o < k);
            if ((d & 127u) == 0 && vstate[0]) return;
        }
        too = d > cap && j + d < m && gid(kin[j + d]) == g;
        walked += d - 1;
    }
    if (walked > GS_FREE && !too) too = atomicAdd(&state[1], (unsigned long long)walked) + walked > budget;
    if (too) {
        atomicExch(&state[0], 1ull);
        return;
    }
    kout[pos] = k;
    vout[pos] = vin[j];
}

template <typename I>
__global__ __launch_bounds__(256) void sa_newhead_kernel(const uint64_t* __restrict__ skey, const I* __restrict__ U,
                                                         const uint8_t* __restrict__ flags, uint64_t m,
                                                         uint8_t* __restrict__ nh) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const bool oldhead = flags[U[j]] & 1;
    nh[j] = (uint8_t)(oldhead || j == 0 || skey[j] != skey[j - 1]);
}

// CARRIED: the write-back of the carried round (refine_groups) — its depth is a number of code bits, not of symbols, so "the
// suffix ends inside the compared prefix" is not tested: a group of several stays open and the text round behind it closes it
// (no gather from the document table at all)
template <typename SAW, typename I, bool WANT_POS = true, bool CARRIED = false>
__device__ __forceinline__ void sa_place(uint64_t j, uint64_t m, const typename SAW::val* sval, const I* U, const uint8_t* nh,
                                         const uint64_t* doc_start, int bits, uint64_t mask, uint64_t hnew, SAW sa,
                                         uint8_t* flags, uint64_t& ext_pos, unsigned long long* still_open,
                                         const uint8_t* hcov = nullptr, uint32_t h_add = 0, uint8_t* lf = nullptr) {
    if (hcov) hnew = (uint64_t)hcov[j] + h_add;  // (variable-length keys: the group's own depth; slot j stays inside its group through the sort)
    const typename SAW::val v = sval[j];
    const uint64_t i = U[j];
    const bool head = nh[j];
    const bool last = j + 1 == m || nh[j + 1];
    const uint64_t d = (uint64_t)v & mask, off = (uint64_t)v >> bits;
    // (a group of one is settled whatever is left of its document: most entries of a round, and their two random loads from the
    //  document table are the kernel's only gathers — skipped unless the caller wants the entry's text position)
    uint64_t ds = 0;
    bool exhausted = false;
    if (!CARRIED && (WANT_POS || !(head && last))) {
        ds = doc_start[d];
        exhausted = doc_start[d + 1] - ds - off < hnew;
    }
    const bool open = !(head && last) && !exhausted;
    sa.store(i, v);
    flags[i] = (uint8_t)((head ? 1 : 0) | (open ? 2 : 0));
    if (lf) lf[j] = (uint8_t)((head ? 1 : 0) | (open ? 2 : 0));  // (the same byte in list order: the next round compacts from the list)
    // (the carried round leaves a share of its entries open — millions of adds to one address — and its successor counts its
    //  list anyway: not counted there)
    if (!CARRIED && open) atomicAdd(still_open, 1ull);  // the compiler folds this into one add per wave
    ext_pos = ds + d + off;
}

template <typename SAW, typename I, bool CARRIED = false>
__global__ __launch_bounds__(256) void sa_update_kernel(const typename SAW::val* __restrict__ sval, const I* __restrict__ U,
                                                        const uint8_t* __restrict__ nh, uint64_t m,
                                                        const uint64_t* __restrict__ doc_start, int bits,
                                                        uint64_t mask, uint64_t hnew, SAW sa,
                                                        uint8_t* __restrict__ flags,
                                                        unsigned long long* __restrict__ still_open,
                                                        const uint8_t* __restrict__ hcov = nullptr, uint32_t h_add = 0, uint8_t* __restrict__ lf = nullptr) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    uint64_t q;
    sa_place<SAW, I, false, CARRIED>(j, m, sval, U, nh, doc_start, bits, mask, hnew, sa, flags, q, still_open, hcov, h_add, lf);
}

template <typename I>
struct HeadIn {  // group start (+1) of compacted entry j, 0 for non-heads  -> max-scan
    const uint8_t* nh;
    const I* U;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return nh[j] ? (uint64_t)U[j] + 1 : 0ull; }
};
// Prefix doubling compares RANKS, and a rank is a slot number of the array: it orders suffixes correctly only while the
// array's slot order is the plain unsigned order.  When the bucket-wise build lays blocks out in the reference's order
// (first-symbol buckets by signed byte, the two byte blocks of radix-node buckets swapped) a rank is taken through the
// inverse of that block permutation first: slot -> where the slot would sit in unsigned order.  nseg = 0: identity.
struct SlotOrder {
    const unsigned long long* a_start = nullptr;  // [nseg] block starts in the array, ascending
    const unsigned long long* u_start = nullptr;  // [nseg] where each block starts in unsigned order
    uint32_t nseg = 0;
    __device__ __forceinline__ uint64_t operator()(uint64_t slot) const {
        if (nseg == 0) return slot;
        uint32_t lo = 0, hi = nseg - 1;  // last block with a_start <= slot
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (a_start[mid] <= slot) lo = mid; else hi = mid - 1;
        }
        return slot - a_start[lo] + u_start[lo];
    }
};

template <typename SAW, typename I, typename R>
struct UpdateOut {
    using V = typename SAW::val;
    const V* sval;
    const I* U;
    const uint8_t* nh;
    uint64_t m;
    const uint64_t* doc_start;
    int bits;
    uint64_t mask, hnew;
    SAW sa;
    uint8_t* flags;
    R* rank;
    unsigned long long* still_open;
    SlotOrder order;
    __device__ __forceinline__ void operator()(uint64_t j, uint64_t, uint64_t incl) const {
        uint64_t q;
        sa_place<SAW, I>(j, m, sval, U, nh, doc_start, bits, mask, hnew, sa, flags, q, still_open);
        rank[q] = (R)(order(incl - 1) + 1);  // (incl = the group's first slot + 1)
    }
};

// inverse array from the current grouping: rank[ext(sa[i])] = group start + 1
struct AllHeadIn {
    const uint8_t* flags;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return (flags[i] & 1) ? i + 1 : 0ull; }
};
template <typename SAW, typename R>
struct IsaOut {
    SAW sa;
    const uint64_t* doc_start;
    int bits;
    uint64_t mask;
    R* rank;
    SlotOrder order;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t, uint64_t incl) const {
        const auto v = sa.load(i);
        const uint64_t d = (uint64_t)v & mask, off = (uint64_t)v >> bits;
        rank[doc_start[d] + d + off] = (R)(order(incl - 1) + 1);
    }
};

// most symbols a text-extension round compares: what a 64-bit round key holds at one bit per symbol (this was the prologue's
// KG_LOOK, a tile look-ahead of the same value; (64 - gbits) / symbits never exceeds it)
constexpr int EXT_MAX_SYM = 64;

// slot order of the array as the bucket-wise build laid it out -> plain unsigned order (ranks of prefix doubling)
SlotOrder make_slot_order(Index& ix, const InitialSort& is, const Alphabet& al, DevBuf& d_order) {
    SlotOrder order;
    if (is.folded_roots.empty()) return order;
    const std::vector<Depth1Fold>& depth1 = is.depth1;
    struct Blk { unsigned long long a, len; int code, cls; };  // cls: 0 = end of document, 1 = bytes < 0x80, 2 = bytes >= 0x80
    std::vector<Blk> blks;
    std::vector<int> code_of_root;  // first-symbol code of every root bucket, in array order
    {
        for (int b = 128; b < 256; ++b) if (al.h_map[b]) code_of_root.push_back(al.h_map[b]);
        for (int b = 0; b < 128; ++b) if (al.h_map[b]) code_of_root.push_back(al.h_map[b]);
    }
    for (size_t b = 0; b < is.folded_roots.size(); ++b) {
        const CompatBucket r = is.folded_roots[b];
        if (!depth1.empty() && depth1[b].done) {  // written as [end][high][low]
            blks.push_back(Blk{r.lo, depth1[b].nend, code_of_root[b], 0});
            blks.push_back(Blk{r.lo + depth1[b].nend, depth1[b].nhigh, code_of_root[b], 2});
            blks.push_back(Blk{r.lo + depth1[b].nend + depth1[b].nhigh, depth1[b].nlow, code_of_root[b], 1});
        } else {
            blks.push_back(Blk{r.lo, r.hi - r.lo, code_of_root[b], 0});
        }
    }
    // unsigned order: by first-symbol code, inside a bucket [end][low][high]
    std::vector<size_t> by_u(blks.size());
    for (size_t i = 0; i < by_u.size(); ++i) by_u[i] = i;
    std::sort(by_u.begin(), by_u.end(), [&](size_t x, size_t y) {
        return blks[x].code != blks[y].code ? blks[x].code < blks[y].code : blks[x].cls < blks[y].cls;
    });
    std::vector<unsigned long long> tab(2 * blks.size());
    unsigned long long at = 0;
    for (size_t i : by_u) {
        tab[blks.size() + i] = at;
        at += blks[i].len;
    }
    for (size_t i = 0; i < blks.size(); ++i) tab[i] = blks[i].a;
    d_order.alloc(tab.size() * sizeof(unsigned long long));
    CDB_HIP(hipMemcpyAsync(d_order.p, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ix.stream));
    CDB_HIP(hipStreamSynchronize(ix.stream));
    order.a_start = d_order.as<unsigned long long>();
    order.u_start = d_order.as<unsigned long long>() + blks.size();
    order.nseg = (uint32_t)blks.size();
    return order;
}

}  // namespace

// (generic over the array's storage: SaRW<V> = plain entries, Sa40RW = packed 5-byte entries, index_impl.h)
// returns the depth every suffix is sorted to
template <typename V, typename I, typename R, typename SAW>
uint64_t refine_groups(Index& ix, SAW sa, InitialSort& is, const Alphabet& al, const KeyPlan& kp, SortStats& ss, RefineBuffers& rb) {
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size, D = ix.ndocs;
    BuildStats& st = ix.bstats;
    const uint8_t* text = ix.d_text;
    const uint64_t* doc_start = ix.d_doc_start.as<uint64_t>();
    const int symbits = al.symbits;
    const DevBuf& flags = is.flags;
    const uint32_t vl_kb1 = is.vl_kb1;
    const SlotOrder order = make_slot_order(ix, is, al, rb.d_order);
    DevBuf &U = rb.U, (&skey)[2] = rb.skey, (&sval)[2] = rb.sval, &nh = rb.nh, &rank = rb.rank, &hcov = rb.hcov;
    DevBuf &d_open = rb.d_open, &U2b = rb.U2b, &lf = rb.lf, &d_gs_state = rb.d_gs_state;
    uint32_t h_acc = 0;  // symbols the text-extension rounds so far added behind every group's own depth (variable-length keys)
    uint64_t h = is.refine_depth0 ? is.refine_depth0 : (uint64_t)kp.nsym;
    bool isa = false;
    uint64_t cap = 0;
    d_open.alloc(sizeof(uint64_t));
    bool have_list = false;  // the last round was a text-extension round: lf / U / sval[list_rs] describe its list
    uint64_t m_list = 0;
    int list_rs = 0;
    d_gs_state.alloc(2 * sizeof(unsigned long long));
    bool group_sort_on = ix.group_sort;
    // The carried round: where the initial sort left `carry` more code-stream bits of every entry in its flag byte (run_segmented),
    // the first round sorts the tied groups on those bits — a round like any other (compaction, sort inside the groups, new heads,
    // write-back, list) without one read of the text.  It counts in carried_rounds only: rounds, ext_rounds, list_rounds and
    // group_sorts, and the limits of the text-or-doubling rule below, see the text and doubling rounds alone.
    const uint32_t carry = is.carry;
    bool carried_pending = carry > 0, list_is_carried = false;
    uint32_t kb_shared = vl_kb1;  // code bits every member of a group shares (equal bits decode alike: where hcov starts)
    st.carried_rounds = 0;
    // The carried round IN PLACE (carried_inplace.h) in front of it: one sweep over the flag bytes settles every tied group that lies
    // inside one tile of the sweep and has at most 64 members — a permutation of neighbouring slots — and leaves the raw tile sums
    // of what is still open, so the list round below compacts the few groups left (those across a tile boundary, the long ones
    // and the ones whose carried bits are equal) without a flag count.  It is a no-op on the settled groups: they are in order and
    // their carried bits moved with them.
    const bool inplace = carry > 0 && n > 0 && n < CI_MAX_N && (ix.carried_inplace < 0 ? n >= CARRIED_INPLACE_MIN_N : ix.carried_inplace != 0);
    uint64_t met_inplace = 0;
    st.carried_inplace = 0;
    if (inplace) {
        const uint64_t nb = ceil_div(n, SC_TILE);
        ix.scan_partials.ensure(scan_partials_slots(nb) * sizeof(U2));
        rb.d_inplace.alloc(CI_COUNT_SLOTS * sizeof(unsigned long long));
        CDB_HIP(hipMemsetAsync(rb.d_inplace.p, 0, CI_COUNT_SLOTS * sizeof(unsigned long long), s));
        int t = ix.prof.begin(s);
        launch_carried_inplace(s, flags.as<uint8_t>(), n, (int)carry, sa, ix.scan_partials.as<U2>(), rb.d_inplace.as<unsigned long long>());
        ix.prof.end(t, "sa_carried_inplace", n, s);
        unsigned long long cnt[CI_COUNT_SLOTS] = {};
        CDB_HIP(hipMemcpyAsync(cnt, rb.d_inplace.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        uint64_t moved_inplace = 0;
        carried_inplace_totals(cnt, met_inplace, moved_inplace);
        if (t >= 0) ix.prof.pending[t].bytes = n + moved_inplace * 2 * (std::is_same<SAW, Sa40RW>::value ? 5 : sizeof(V));
        is.tile_sums_ready = true;
        st.carried_inplace = 1;
    }
    for (uint32_t iter = 0;; ++iter) {
        if (iter > 0 && !list_is_carried) {  // (the carried round does not count its open entries: the flag count below does)
            uint64_t still = 0;
            CDB_HIP(hipMemcpyAsync(&still, d_open.p, sizeof(still), hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
            if (still == 0) break;
        }
        const bool carried = carried_pending;
        carried_pending = false;
        CDB_HIP(hipMemsetAsync(d_open.p, 0, sizeof(uint64_t), s));
        auto flag_tile_sums = [&]() {  // raw tile sums of the flag array into the scan's partials (wave-autonomous sweep)
            const uint64_t nb = ceil_div(n, SC_TILE);
            ix.scan_partials.ensure(scan_partials_slots(nb) * sizeof(U2));
            int t = ix.prof.begin(s);
            hipLaunchKernelGGL(sa_flag_count_kernel, dim3((unsigned)ceil_div(nb, (uint64_t)(4 * FC_TILES_PER_WAVE))), dim3(256), 0, s,
                               (const uint8_t*)flags.as<uint8_t>(), n, nb, ix.scan_partials.as<U2>());
            ix.prof.end(t, "sa_flag_count", n, s);
        };
        bool from_list = have_list && ix.list_rounds;  // (this round's unresolved entries are a subset of the previous round's list)
        have_list = false;
        if (from_list) {
            const uint64_t nb = ceil_div(m_list, SC_TILE);
            ix.scan_partials.ensure(scan_partials_slots(nb) * sizeof(U2));
            int t = ix.prof.begin(s);
            hipLaunchKernelGGL(sa_flag_count_kernel, dim3((unsigned)ceil_div(nb, (uint64_t)(4 * FC_TILES_PER_WAVE))), dim3(256), 0, s,
                               (const uint8_t*)lf.as<uint8_t>(), m_list, nb, ix.scan_partials.as<U2>());
            ix.prof.end(t, "sa_flag_count", m_list, s);
        } else if (!is.tile_sums_ready) {
            flag_tile_sums();
        }
        U2 tot = scan_totals_from_partials<U2>(s, ix.scan_partials, from_list ? m_list : n, OpAdd{}, U2{0, 0});
        is.tile_sums_ready = false;
        uint64_t m = tot.a, G = tot.b;
        if (iter == 0) {
            st.unresolved_initial = inplace ? met_inplace : m;
            st.unresolved_after_inplace = st.unresolved_after_carried = m;
            if (inplace && met_inplace > 0) st.carried_rounds = 1;  // (also where the sweep left nothing open)
            st.unresolved_max = std::max(st.unresolved_max, st.unresolved_initial);
        }
        if (list_is_carried) st.unresolved_after_carried = m;
        st.unresolved_max = std::max(st.unresolved_max, m);
        if (m == 0) break;
        // (the per-entry kernels of a round address one thread per unresolved entry: a launch holds < 2^32 of them)
        if (m >= (1ull << 32) - 4096) throw InternalError("too many unresolved suffixes for one refinement round (internal limit: 2^32)");
        const int gbits = bit_width64(G - 1);
        int nsym2 = std::min((64 - gbits) / symbits, EXT_MAX_SYM);
        if (!isa && !carried) {
            // Re-keying m suffixes from the text costs ~ m x (one random line + a sort); the inverse array of prefix
            // doubling costs n random writes before its first round.  Text extension therefore gets up to four
            // rounds while few suffixes are open, and two rounds even for a larger share (e.g. Zipf text, 5 % open
            // after the initial sort, resolved by 2 x 5 more symbols); only then the inverse array is built.
            const bool use_text = !ix.force_doubling && nsym2 >= 1 &&
                                  ((m <= n / 32 && st.ext_rounds < 4) || (m <= n / 8 && st.ext_rounds < 2));
            if (!use_text) {
                rank.alloc((n + D + 1) * sizeof(R));
                CDB_HIP(hipMemsetAsync(rank.p, 0, (n + D + 1) * sizeof(R), s));
                AllHeadIn ain{flags.as<uint8_t>()};
                (void)scan_totals<uint64_t>(s, ix.scan_partials, ain, n, OpMax{}, (uint64_t)0);
                IsaOut<SAW, R> iout{sa, doc_start, (int)ix.bits, ix.mask, rank.as<R>(), order};
                int t = ix.prof.begin(s);
                scan_apply<uint64_t>(s, ix.scan_partials, ain, n, OpMax{}, (uint64_t)0, iout);
                ix.prof.end(t, "sa_isa_init", n * (1 + sizeof(V) + sizeof(R)), s);
                isa = true;
                st.isa_built = 1;
                // the partials buffer now belongs to the max-scan: redo the compaction totals (from the array: the doubling rounds
                // do not keep a list)
                from_list = false;
                flag_tile_sums();
                (void)scan_totals_from_partials<U2>(s, ix.scan_partials, n, OpAdd{}, U2{0, 0});
            }
        }
        const int kbits = carried ? (int)carry : (isa ? bit_width64(n) : nsym2 * symbits);
        if (kbits + gbits > 64) throw InternalError("refinement key does not fit 64 bits (internal limit)");
        if (m > cap) {
            cap = m;
            U.alloc(m * sizeof(I));
            skey[0].alloc(m * 8);
            skey[1].alloc(m * 8);
            sval[0].alloc(m * sizeof(V));
            sval[1].alloc(m * sizeof(V));
            nh.alloc(m);
            lf.alloc(m + 16);
            if (vl_kb1) hcov.alloc(m);
        }
        {
            int t = ix.prof.begin(s);
            if (from_list) {
                if (list_rs == 0) {  // the sorted list must not be the compaction's target
                    std::swap(skey[0], skey[1]);
                    std::swap(sval[0], sval[1]);
                    list_rs = 1;
                }
                U2b.ensure(cap * sizeof(I));
                CompactListOut<V, I> co{(const I*)U.as<I>(), (const V*)sval[1].as<V>(), U2b.as<I>(), skey[0].as<uint64_t>(), sval[0].as<V>(), kbits};
                hipLaunchKernelGGL((sa_flag_compact_kernel<decltype(co)>), dim3((unsigned)ceil_div(ceil_div(m_list, SC_TILE), (uint64_t)(4 * FC_TILES_PER_WAVE))),
                                   dim3(256), 0, s, (const uint8_t*)lf.as<uint8_t>(), m_list, (uint64_t)ceil_div(m_list, SC_TILE),
                                   (const U2*)ix.scan_partials.as<U2>(), co);
                std::swap(U, U2b);
                if (!list_is_carried) st.list_rounds++;
            } else if (carried) {
                CompactCarriedOut<SAW, I> co{sa, (const uint8_t*)flags.as<uint8_t>(), U.as<I>(), skey[0].as<uint64_t>(), sval[0].as<V>(), kbits};
                hipLaunchKernelGGL((sa_flag_compact_kernel<decltype(co)>), dim3((unsigned)ceil_div(ceil_div(n, SC_TILE), (uint64_t)(4 * FC_TILES_PER_WAVE))),
                                   dim3(256), 0, s, (const uint8_t*)flags.as<uint8_t>(), n, (uint64_t)ceil_div(n, SC_TILE),
                                   (const U2*)ix.scan_partials.as<U2>(), co);
            } else {
            CompactOut<SAW, I> co{sa, U.as<I>(), skey[0].as<uint64_t>(), sval[0].as<V>(), kbits};
            hipLaunchKernelGGL((sa_flag_compact_kernel<decltype(co)>), dim3((unsigned)ceil_div(ceil_div(n, SC_TILE), (uint64_t)(4 * FC_TILES_PER_WAVE))),
                               dim3(256), 0, s, (const uint8_t*)flags.as<uint8_t>(), n, (uint64_t)ceil_div(n, SC_TILE),
                               (const U2*)ix.scan_partials.as<U2>(), co);
            }
            if (carried) {
                // (the minor keys are complete: no sa_round_keys launch)
            } else if (isa)
                hipLaunchKernelGGL((sa_round_keys_kernel<V, R, true>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s,
                                   (const V*)sval[0].as<V>(), m, doc_start, text, (const uint16_t*)al.d_symmap.as<uint16_t>(),
                                   (const R*)rank.as<R>(), (int)ix.bits, ix.mask, h, nsym2, symbits, skey[0].as<uint64_t>(), n);
            else
                hipLaunchKernelGGL((sa_round_keys_kernel<V, R, false>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s,
                                   (const V*)sval[0].as<V>(), m, doc_start, text, (const uint16_t*)al.d_symmap.as<uint16_t>(),
                                   (const R*)nullptr, (int)ix.bits, ix.mask, h, nsym2, symbits, skey[0].as<uint64_t>(), n,
                                   vl_kb1 ? (const uint8_t*)is.d_vl_bytelen.as<uint8_t>() : nullptr, kb_shared, h_acc, vl_kb1 ? hcov.as<uint8_t>() : nullptr);
            ix.prof.end(t, "sa_compact", n + m * (sizeof(I) + 8 + 2 * sizeof(V)), s);
        }
        int rs = -1;
        if (group_sort_on) {  // one pass inside the groups (sa_group_sort_kernel); groups too long for it: the general sort, from now on
            CDB_HIP(hipMemsetAsync(d_gs_state.p, 0, 2 * sizeof(unsigned long long), s));
            int t = ix.prof.begin(s);
            hipLaunchKernelGGL((sa_group_sort_kernel<V>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s, (const uint64_t*)skey[0].as<uint64_t>(),
                               (const V*)sval[0].as<V>(), m, kbits, (uint32_t)ix.group_sort_cap, (unsigned long long)(16 * m + (1u << 20)),
                               skey[1].as<uint64_t>(), sval[1].as<V>(), d_gs_state.as<unsigned long long>());
            ix.prof.end(t, "sa_group_sort", m * 2 * (8 + sizeof(V)), s);
            unsigned long long gave_up = 0;
            CDB_HIP(hipMemcpyAsync(&gave_up, d_gs_state.p, sizeof(gave_up), hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
            if (gave_up) {
                group_sort_on = false;
                st.group_sort_fallbacks++;
            } else {
                rs = 1;
                if (!carried) st.group_sorts++;
            }
        }
        if (rs < 0) {
            rs = radix_sort<uint64_t, V>(s, ix.rws, ix.prof, skey[0].as<uint64_t>(), skey[1].as<uint64_t>(),
                                         sval[0].as<V>(), sval[1].as<V>(), m, 0, kbits + gbits, &ss, ix.sort_variant);
            radix_check_error(s, ix.rws);  // (sa_update scatters through the sorted values: never after a failed sort)
        }
        hipLaunchKernelGGL((sa_newhead_kernel<I>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s,
                           (const uint64_t*)skey[rs].as<uint64_t>(), (const I*)U.as<I>(),
                           (const uint8_t*)flags.as<uint8_t>(), m, nh.as<uint8_t>());
        const uint64_t hnew = isa ? 2 * h : h + (uint64_t)nsym2;
        {
            int t = ix.prof.begin(s);
            if (carried) {
                hipLaunchKernelGGL((sa_update_kernel<SAW, I, true>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s,
                                   (const V*)sval[rs].as<V>(), (const I*)U.as<I>(), (const uint8_t*)nh.as<uint8_t>(), m,
                                   doc_start, (int)ix.bits, ix.mask, (uint64_t)0, sa, flags.as<uint8_t>(), (unsigned long long*)nullptr,
                                   (const uint8_t*)nullptr, 0u, lf.as<uint8_t>());
                st.carried_rounds = 1;  // (sweep, list round or both: one carried round)
                kb_shared = vl_kb1 + carry;  // (the groups now share the carried bits too)
                have_list = true;
                m_list = m;
                list_rs = rs;
            } else if (isa) {
                HeadIn<I> hin{nh.as<uint8_t>(), U.as<I>()};
                (void)scan_totals<uint64_t>(s, ix.scan_partials, hin, m, OpMax{}, (uint64_t)0);
                UpdateOut<SAW, I, R> uo{sval[rs].as<V>(), U.as<I>(), nh.as<uint8_t>(), m, doc_start, (int)ix.bits,
                                      ix.mask, hnew, sa, flags.as<uint8_t>(), rank.as<R>(), d_open.as<unsigned long long>(), order};
                scan_apply<uint64_t>(s, ix.scan_partials, hin, m, OpMax{}, (uint64_t)0, uo);
                st.dbl_rounds++;
            } else {
                hipLaunchKernelGGL((sa_update_kernel<SAW, I>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s,
                                   (const V*)sval[rs].as<V>(), (const I*)U.as<I>(), (const uint8_t*)nh.as<uint8_t>(), m,
                                   doc_start, (int)ix.bits, ix.mask, hnew, sa, flags.as<uint8_t>(), d_open.as<unsigned long long>(),
                                   vl_kb1 ? (const uint8_t*)hcov.as<uint8_t>() : nullptr, h_acc + (uint32_t)nsym2, lf.as<uint8_t>());
                h_acc += (uint32_t)nsym2;
                st.ext_rounds++;
                have_list = true;
                m_list = m;
                list_rs = rs;
            }
            ix.prof.end(t, "sa_update", m * (2 * sizeof(V) + sizeof(I) + 2 + (isa ? sizeof(R) : 0)), s);
        }
        list_is_carried = carried;
        if (carried) continue;  // (no symbol was compared: h stays, and no round statistic counts this round)
        h = hnew;
        st.rounds++;
        if (st.rounds > 80) throw InternalError("suffix-array refinement did not converge (internal error)");
    }
    return h;
}

// the forms build_typed calls: plain entries for every (V, I, R), packed 5-byte entries for V = uint64_t
#define CDB_REFINE_FOR(V, I, R, SAW) \
    template uint64_t refine_groups<V, I, R, SAW>(Index&, SAW, InitialSort&, const Alphabet&, const KeyPlan&, SortStats&, RefineBuffers&);
CDB_REFINE_FOR(uint32_t, uint32_t, uint32_t, SaRW<uint32_t>)
CDB_REFINE_FOR(uint64_t, uint32_t, uint32_t, SaRW<uint64_t>)
CDB_REFINE_FOR(uint32_t, uint64_t, uint64_t, SaRW<uint32_t>)
CDB_REFINE_FOR(uint64_t, uint64_t, uint64_t, SaRW<uint64_t>)
CDB_REFINE_FOR(uint64_t, uint32_t, uint32_t, Sa40RW)
CDB_REFINE_FOR(uint64_t, uint64_t, uint64_t, Sa40RW)
#undef CDB_REFINE_FOR

}  // namespace cdb
