// carried_inplace.h — the flag sweeps' shared pieces (16-byte flag loader, SWAR counts) and the in-place form of the carried
// round: sa_carried_inplace_kernel.  A header, because two translation units instantiate the kernel: sa_refine.hip
// (refine_groups) and debug_carried.hip (the test hook).
//
// After the initial sort a tied group is a run of adjacent array slots — a head with flag bits 0 and 1 set, then members with
// bit 1 set, up to the next head — and with carried bits its minor key lies beside it, in bits 2.. of the same flag bytes.  The
// groups are tiny (8 GiB of Zipf text: 28 242 of 2.07 x 10^8 open entries sit in groups of more than 49), so the carried round is
// a permutation of two or three neighbouring slots decided by bytes the flag sweep holds in registers anyway: no global list, no
// scan, no 64-bit keys, no second and third launch over the same entries.
#pragma once
#include "common.h"
#include "scan.h"

namespace cdb {

constexpr uint32_t FC_TILES_PER_WAVE = 4;
__device__ __forceinline__ void fc_load(const uint8_t* __restrict__ flags, uint64_t n, uint64_t base, uint32_t (&x)[4]) {
    x[0] = x[1] = x[2] = x[3] = 0;
    if (base + 16 <= n) {
        const uint4 w = *reinterpret_cast<const uint4*>(flags + base);
        x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
    } else if (base < n) {
        for (int k = 0; k < 16 && base + k < n; ++k) x[k >> 2] |= (uint32_t)flags[base + k] << (8 * (k & 3));
    }
}
__device__ __forceinline__ uint32_t fc_count(const uint32_t (&x)[4]) {  // unresolved entries | unresolved group heads << 16
    uint32_t cu = 0, ch = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t u = (x[q] >> 1) & 0x01010101u;
        cu += __popc(u);
        ch += __popc(u & x[q] & 0x01010101u);
    }
    return cu | (ch << 16);
}

// The carried round in place.  Shape of sa_flag_compact_kernel: a wave owns whole tiles of SC_TILE flags, lists a tile's open
// positions in order in its own stretch of the LDS (12-bit offset + head bit, the carried bits beside them) and takes 64 listed
// entries per trip.
//
// OWNERSHIP IS TILE-LOCAL, which makes the kernel race-free without any protocol between waves: a group is handled only if its
// head lies in the wave's tile, it ends in that tile (the wave reads the one flag byte behind its tile, or knows the array ends,
// to decide that for the last group) and it has at most CI_GROUP_MAX members.  Every other open group — head-less leading members
// (the previous tile's group), a group running past the tile end, a longer group — stays byte for byte as it was, entries and
// flag bytes alike, and the list round behind the sweep sorts it.  Slots that are not open are never written.  (The byte behind
// the tile may be rewritten by the tile's owner meanwhile, but its bit 0 never changes there — a tile's first slot is a head or
// belongs to no group its owner handles — and an open byte stays open or is a head: the test reads the same either way.)
//
// A trip never splits a group: it ends in front of the first group that does not end inside its 64 entries.  An entry's slot
// inside its group is sa_group_sort_kernel's rule, j - #{members in front with a greater key} + #{members behind with a smaller
// one}: the stable order, so the finished array is bit-identical.  New flags are sa_place's CARRIED rule (a member whose key differs
// from its sorted predecessor's becomes a head; a group of one closes; no "ends inside the prefix" test), and bits 2.. travel with
// the entry, because the list round behind reads them.  All gathers of the planned trips complete before any of their stores issue: the
// stores carry the loaded values, and a wave's loads return before an instruction that consumes one of them issues.
//
// partials[tile] = (open entries, open heads) of the tile AS THE KERNEL LEAVES IT, for every tile — the raw tile sums the next
// round's compaction scans.  The open entries met and the entries moved are added to `counts`, one atomic per wave at most.
constexpr uint32_t CI_GROUP_MAX = 64;
// Option carried_inplace = -1 (automatic): the sweep runs from this many suffixes upward.  Below it the whole carried round is a
// fraction of a millisecond and one more launch buys nothing; the 256 MiB builds and everything larger take the sweep.
constexpr uint64_t CARRIED_INPLACE_MIN_N = 1ull << 26;
// The kernel is bound by the latency of its dependent memory steps (flag bytes -> gather -> store), so it keeps its LDS small for
// occupancy — the list holds CI_LIST entries, a denser tile is listed again, window by window, from the flag bytes in registers —
// and PLANS CI_TRIPS trips before it touches the array: their gathers issue back to back, then their stores.
constexpr uint32_t CI_LIST = 1024;
constexpr int CI_TRIPS = 4;
// counts: CI_COUNT_SLOTS words, one per workgroup number modulo the slots (a single word would take an add from every wave of the
// grid); a word = open entries met | entries moved << 32 (a workgroup adds at most 2^16 to either: exact below 2^37 slots)
constexpr uint32_t CI_COUNT_SLOTS = 64;
constexpr uint64_t CI_MAX_N = 1ull << 37;
template <typename SAW>
__global__ __launch_bounds__(256) void sa_carried_inplace_kernel(uint8_t* flags, uint64_t n, uint64_t tiles, int xbits, SAW sa,
                                                                 U2* __restrict__ partials, unsigned long long* __restrict__ counts) {
    static_assert(SC_TILE == 4096, "flag sweeps assume 4096-flag tiles");
    static_assert(CI_GROUP_MAX == 64, "a group is ranked inside one 64-entry trip");
    static_assert(CI_LIST >= 128 && CI_LIST <= SC_TILE, "a window holds a trip and the entry behind it");
    using V = typename SAW::val;
    __shared__ uint16_t s_list[4][CI_LIST];      // per wave: open positions of the tile (offset | head << 12), one window of them
    __shared__ uint8_t s_key[4][CI_LIST];        // ... and bits 2.. of their flag bytes
    __shared__ uint8_t s_src[4][CI_TRIPS][64];   // per wave and trip: the window lane whose entry comes to this lane's slot
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t le_mask = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
    uint16_t* const list = s_list[wave];
    uint8_t* const key = s_key[wave];
    const uint32_t kmask = (1u << xbits) - 1u;
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4 + wave) * FC_TILES_PER_WAVE;
    uint32_t met = 0, moved_n = 0;
    for (uint32_t k = 0; k < FC_TILES_PER_WAVE; ++k) {
        const uint64_t tile = t0 + k;
        if (tile >= tiles) break;  // (uniform per wavefront)
        const uint64_t tbase = tile * SC_TILE;
        uint32_t x[4][4], v[4], incl[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) fc_load(flags, n, tbase + (uint64_t)c * 1024 + (uint64_t)lane * 16, x[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) incl[c] = v[c] = fc_count(x[c]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t y = __shfl_up(incl[c], off);
                if (lane >= off) incl[c] += y;
            }
        }
        uint32_t total = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) total += __shfl(incl[c], 63) & 0xFFFFu;
        if (total == 0) {  // (nothing open in the tile)
            if (lane == 0) partials[tile] = U2{0, 0};
            continue;
        }
        met += total;
        // does the tile's last open group end inside the tile?  (a last open entry in front of the tile's last slot is followed by a
        // slot that is not open, or by nothing)
        uint32_t tail_closed = 1;
        if (__shfl((x[3][3] >> 25) & 1u, 63) != 0 && tbase + SC_TILE < n) {
            const uint32_t f = flags[tbase + SC_TILE];
            tail_closed = (!((f >> 1) & 1u) || (f & 1u)) ? 1u : 0u;
        }
        uint32_t left_open = 0, left_heads = 0;
        for (uint32_t pass_lo = 0; pass_lo < total;) {
            // ---- phase 1: list the open positions [pass_lo, pass_lo + CI_LIST) in order (a lane walks the SET bits of its bytes only)
            uint32_t cpre = 0;  // packed counts of the chunks in front
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t ctot = __shfl(incl[c], 63);
                if (v[c] & 0xFFFFu) {
                    uint32_t slot = ((cpre + incl[c] - v[c]) & 0xFFFFu) - pass_lo;  // (in front of the window: wraps past it)
                    uint32_t um = 0, hm = 0;  // bit q: byte q is open / an open group head
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
                        if (slot < CI_LIST) {
                            const uint32_t word = q < 8u ? (q < 4u ? x[c][0] : x[c][1]) : (q < 12u ? x[c][2] : x[c][3]);
                            list[slot] = (uint16_t)((off0 + q) | (((hm >> q) & 1u) << 12));
                            key[slot] = (uint8_t)(((word >> (8u * (q & 3u))) & 0xFFu) >> 2);
                        }
                        ++slot;
                    }
                }
                cpre += ctot;
            }
            // (the lists are the wave's own: its LDS operations execute in program order — the fences keep the compiler from moving them)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t wend = total - pass_lo < CI_LIST ? total : pass_lo + CI_LIST;  // the window holds entries [pass_lo, wend)
            // ---- phase 2: trips of up to 64 listed entries, whole groups only; a trip needs its window and, where the list goes on,
            // the entry behind it
            uint32_t b0 = pass_lo;
            // (inside the window: the trip's own entries and, where the list goes on behind them, the next one)
            auto in_window = [&](uint32_t b) { return b < wend && (b + 64u < total ? b + 64u < wend : total <= wend); };
            while (in_window(b0)) {
                uint32_t t_off[CI_TRIPS], t_src[CI_TRIPS], t_nf[CI_TRIPS];
                bool t_moved[CI_TRIPS], t_wr[CI_TRIPS];
#pragma unroll
                for (int u = 0; u < CI_TRIPS; ++u) {
                    t_off[u] = t_src[u] = t_nf[u] = 0;
                    t_moved[u] = t_wr[u] = false;
                    if (!in_window(b0)) continue;  // (uniform)
                    uint8_t* const src = s_src[wave][u];
                    const uint32_t r0 = b0 - pass_lo;  // the trip's first entry in the window
                    const bool live = b0 + (uint32_t)lane < total;
                    const uint32_t e = live ? (uint32_t)list[r0 + lane] : 0u;
                    const uint32_t kf = live ? (uint32_t)key[r0 + lane] : 0u;
                    const uint32_t km = kf & kmask;
                    const bool head = ((e >> 12) & 1u) != 0;
                    const uint64_t hb = __builtin_amdgcn_ballot_w64(head);
                    const uint32_t wlen = total - b0 < 64u ? total - b0 : 64u;
                    const bool more = b0 + 64u < total;  // (the list goes on behind the trip)
                    // the trip's last group is whole when a head follows the trip or, at the end of the list, the tile's last group is
                    const uint32_t next_bound = more ? ((uint32_t)list[r0 + 64u] >> 12) & 1u : tail_closed;
                    const uint32_t last_head = hb ? 63u - (uint32_t)__builtin_clzll(hb) : 0u;
                    // lanes [0, whole) lie in whole groups (or in front of the first head); the trip consumes `adv` entries: all of
                    // them, or, where the list goes on, the part in front of a cut group — which then gets a trip of its own and,
                    // if it still does not fit, is passed over 64 entries at a time (head-less trips)
                    const uint32_t whole = next_bound ? wlen : (hb ? last_head : 0u);
                    const uint32_t adv = (!next_bound && more && hb && last_head > 0u) ? last_head : wlen;
                    const bool owned = live && (uint32_t)lane < whole && (hb & le_mask) != 0;
                    uint32_t gs = 0, ge = 0;  // the group's first and last lane
                    if (owned) {
                        gs = 63u - (uint32_t)__builtin_clzll(hb & le_mask);
                        const uint64_t above = hb & ~le_mask;
                        ge = above ? (uint32_t)__builtin_ctzll(above) - 1u : wlen - 1u;
                    }
                    uint32_t pos = (uint32_t)lane;
                    if (owned) {
                        for (uint32_t p = gs; p <= ge; ++p) {
                            const uint32_t kp = (uint32_t)key[r0 + p] & kmask;
                            pos -= (uint32_t)(p < (uint32_t)lane && kp > km);
                            pos += (uint32_t)(p > (uint32_t)lane && kp < km);
                        }
                    }
                    src[pos] = (uint8_t)lane;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const uint32_t sl = (uint32_t)src[lane];                  // the entry that comes to this lane's slot sat at lane sl
                    const uint32_t skf = live ? (uint32_t)key[r0 + sl] : 0u;  // ... with these carried bits
                    const uint32_t skm = skf & kmask;
                    const uint32_t pkm = __shfl(skm, lane > 0 ? lane - 1 : 0);
                    const bool nhead = head || (owned && skm != pkm);  // (an owned lane that is no head has its group's predecessor in front)
                    const uint64_t nhb = __builtin_amdgcn_ballot_w64(nhead);
                    const bool last = (uint32_t)lane == ge || ((nhb >> ((lane + 1) & 63)) & 1ull) != 0;
                    const bool nopen = owned ? !(nhead && last) : live;
                    const uint64_t cons = adv >= 64u ? ~0ull : (1ull << adv) - 1ull;  // (the entries behind `adv` are taken again)
                    left_open += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nopen) & cons);
                    left_heads += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nopen && nhead) & cons);
                    t_moved[u] = owned && sl != (uint32_t)lane;
                    moved_n += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(t_moved[u]));
                    t_off[u] = e & 0xFFFu;
                    t_src[u] = live ? (uint32_t)list[r0 + sl] & 0xFFFu : 0u;
                    t_nf[u] = (nhead ? 1u : 0u) | (nopen ? 2u : 0u) | (skf << 2);
                    t_wr[u] = owned && t_nf[u] != ((head ? 1u : 0u) | 2u | (kf << 2));
                    b0 += adv;
                }
                // the planned trips touch disjoint slots: every gather of theirs in front of every store
                V val[CI_TRIPS];
#pragma unroll
                for (int u = 0; u < CI_TRIPS; ++u) {
                    val[u] = 0;
                    if (t_moved[u]) val[u] = sa.load(tbase + (uint64_t)t_src[u]);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
                for (int u = 0; u < CI_TRIPS; ++u) {
                    if (t_moved[u]) sa.store(tbase + (uint64_t)t_off[u], val[u]);
                    if (t_wr[u]) flags[tbase + (uint64_t)t_off[u]] = (uint8_t)t_nf[u];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next trips overwrite `src`)
                __builtin_amdgcn_wave_barrier();
            }
            pass_lo = b0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next window and the next tile overwrite the lists)
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) partials[tile] = U2{(uint64_t)left_open, (uint64_t)left_heads};
    }
    if (lane == 0 && (met | moved_n))
        atomicAdd(&counts[blockIdx.x % CI_COUNT_SLOTS], (unsigned long long)met | ((unsigned long long)moved_n << 32));
}

// the launch, as refine_groups runs it (`partials` holds a slot for every tile of n; `counts` = CI_COUNT_SLOTS zeroed words, n < CI_MAX_N)
template <typename SAW>
inline void launch_carried_inplace(hipStream_t s, uint8_t* flags, uint64_t n, int xbits, SAW sa, U2* partials, unsigned long long* counts) {
    const uint64_t nb = ceil_div(n, (uint64_t)SC_TILE);
    if (!nb) return;
    hipLaunchKernelGGL((sa_carried_inplace_kernel<SAW>), dim3((unsigned)ceil_div(nb, (uint64_t)(4 * FC_TILES_PER_WAVE))), dim3(256), 0, s, flags,
                       n, nb, xbits, sa, partials, counts);
}
// the two totals from the kernel's count words
inline void carried_inplace_totals(const unsigned long long (&w)[CI_COUNT_SLOTS], uint64_t& met, uint64_t& moved) {
    met = moved = 0;
    for (unsigned long long c : w) {
        met += c & 0xFFFFFFFFull;
        moved += c >> 32;
    }
}

}  // namespace cdb
