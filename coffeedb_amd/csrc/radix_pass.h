// radix_pass.h — the device half of one radix pass: kernel configurations, the producers and segment descriptions a pass can
// be instantiated with, and rs_onesweep_kernel itself.
//
// Hardware mapping:
//   * 64-wide wavefronts: the rank of an element among the equal digits of its wave comes from ONE returning
//     LDS atomic on the wave's private counters (ATOMRANK; stable because same-address LDS atomics of one
//     instruction complete in lane order on gfx950 — verified per device by rs_lane_order_probe_kernel), or
//     from 8 ballots, one per digit bit, when that self-test fails;
//   * LDS: keys, then values, of one tile are staged in sorted-by-digit order so that the global
//     write-out has consecutive lanes writing consecutive addresses inside each digit run; the
//     production tile is 1024 threads x 16 keys (150 KB of the CU's 160 KB LDS, one workgroup per CU);
//   * 8 XCDs with non-coherent L2s: tiles exchange {epoch,state,count} words only through agent-scope
//     relaxed atomic loads/stores (one 8-byte granule is both flag and payload — MI355X guide §G16 R2),
//     tile ids come from an atomic ticket so a tile only ever waits on tiles that already started, and
//     every spin is bounded (a stuck look-back raises an error flag instead of hanging the GPU).
//
// In this file: RsCfg and the named configurations; rs_load / rs_store; TextGen*, Seg*Args, SegEdge (SegCellEdge: seg_cell_edge.h); rs_pack_key,
// rs_doc_upper; the status-word accessors; RsTraits (every compile-time switch of an instantiation, derived once); the rules the
// kernel body uses more than once as functions (rs_group_flag, rs_load_striped) and the kernel.  radix_sort.h includes it and holds the host half: histograms, workspace, variant
// table, rs_launch_pass, the drivers and the segmented, MSD and tile-base parts.
#pragma once
#include <cstdlib>

#include "common.h"
#include "seg_cell_edge.h"

namespace cdb {

constexpr uint64_t RS_VAL_MASK = (1ull << 54) - 1;
// bounded look-back spins.  XCD-ordered (grouped) passes reserve tiles for workgroups that have not started: a predecessor that has
// not answered after ~0.3-0.5 s of polling is not coming (starved pass; the build retries in plain ticket order), and 2^22 held a
// starved build for ~8 s per wait.  In plain ticket order a tile only waits for tiles that already RUN, so a long wait means the
// predecessor was descheduled (two processes on one GPU, CWSR preemption, a profiler): that pass keeps the patient bound — nothing
// retries it.
constexpr uint32_t RS_SPIN_LIMIT_GROUPED = 1u << 18;
constexpr uint32_t RS_SPIN_LIMIT_PLAIN = 1u << 22;
// XCD-aware tile order of the big-tile configurations: groups of RS_GROUP consecutive tiles go to one XCD (RsCfg::GROUP).
// Tiles are reserved for workgroups that have not started yet, so up to 7 * RS_GROUP resident workgroups can wait for
// one that is still to be dispatched: the pass needs more than that many resident at a time (it has 256 when it runs
// alone; concurrent kernels can take some away) — a pass that starves raises the look-back error flag (bounded
// spins), and the callers redo the sort in plain ticket order (RS_VARIANT_BIG), which needs one.
constexpr int RS_GROUP = 8;

struct NoVal {};

__device__ __forceinline__ uint64_t rs_ld_status(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rs_st_status(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// one radix pass: rank inside the tile, look back for the global prefix, scatter
// ---------------------------------------------------------------------------------------------
// Kernel configuration.  IPT = keys per thread (tile = 256 * IPT); REUSE = keys and values share one
// LDS staging buffer (two write-out phases, smaller footprint -> more workgroups per CU); EARLYV =
// values are fetched together with the keys instead of after the look-back.
template <int IPT_, bool REUSE_, bool EARLYV_, int NT_ = 256, bool NONTEMP_ = false, int MINW_ = 1, int ABL_ = 0,
          int LB_ = 1, bool DMA_ = false, bool ATOMRANK_ = false, bool TICKET_ = true, int LOAD_ = 0, int GROUP_ = 0>
struct RsCfg {
    static constexpr int GROUP = GROUP_;      // > 0: XCD-aware tile order — workgroup b draws from the ticket counter of
                                              // class b % 8 (the XCD it runs on, as observed) and class x owns the tile
                                              // groups x, x + 8, ... of GROUP consecutive tiles each, so neighbouring
                                              // tiles (whose digit runs touch) are written through the same L2
    static constexpr int LOAD = LOAD_;        // plain load path: 0 = predicated loads, keys -> values -> auxiliary digits;
                                              // 1 = unpredicated, keys -> digits -> values (values in flight under the
                                              // ranking); 2 = unpredicated, keys -> values -> digits
    static constexpr bool TICKET = TICKET_;   // tile id from an atomic ticket (false: blockIdx.x — relies on in-order
                                              // dispatch of workgroups; every spin is bounded either way)
    static constexpr bool ATOMRANK = ATOMRANK_;  // rank inside the wave with one returning LDS atomic per element
                                              // instead of 8 ballots (relies on same-address LDS atomics of one
                                              // instruction completing in lane order — checked by a self-test)
    static constexpr bool DMA = DMA_;         // keys/values reach the registers through LDS by 16-byte global->LDS DMA
    static constexpr int LB = LB_;            // look-back window: predecessors polled per round trip
    static constexpr int ABL = ABL_;          // timing-only ablations (WRONG results): 1 = no look-back,
                                              // 2 = linear (unscattered) write-out, 8 = look-back depth counters
    static constexpr int MINW = MINW_;        // min waves per SIMD the register allocator must allow
    static constexpr int IPT = IPT_;
    static constexpr bool REUSE = REUSE_;
    static constexpr bool EARLYV = EARLYV_;
    static constexpr int NT = NT_;            // threads per workgroup (>= 256, multiple of 64)
    static constexpr bool NONTEMP = NONTEMP_;  // streaming (non-temporal) global loads/stores
};

// ---- every configuration the library instantiates (the design points that were measured and dropped — other tile shapes,
// look-back depths, tile orders, non-temporal accesses, timing ablations — are recorded in DESIGN.md §4.1 and can be re-run
// with tools/experiments/pass_bench.hip).  A shape is spelled once, with ballot ranking; its twins are derived from it:
// the one-atomic ranking (devices that passed rs_atomic_rank_ok) ...
template <typename C>
using RsAtomic = RsCfg<C::IPT, C::REUSE, C::EARLYV, C::NT, C::NONTEMP, C::MINW, C::ABL, C::LB, C::DMA, true>;
// ... and the XCD-aware tile order on top of it (with the unpredicated load path that has the values in flight under the ranking)
template <typename C>
using RsGrouped = RsCfg<C::IPT, C::REUSE, C::EARLYV, C::NT, C::NONTEMP, C::MINW, C::ABL, C::LB, C::DMA, C::ATOMRANK, C::TICKET, 1, RS_GROUP>;
// pairs and split records, three tile shapes:   IPT, REUSE, EARLYV, NT, NONTEMP, MINW, ABL, LB
template <int IPT = 16>
using RsBigBallot = RsCfg<IPT, true, true, 1024, false, 1, 0, 4>;   // 16 Ki-key tile, 1 WG/CU
using RsMidBallot = RsCfg<18, true, true, 256, false, 1, 0, 4>;     // 4.5 Ki-key tile, 3 WG/CU
using RsSmallBallot = RsCfg<15, true, true, 256, false, 1, 0, 1>;   // 3.75 Ki-key tile, 4 WG/CU
template <int IPT = 16>
using RsBig = RsAtomic<RsBigBallot<IPT>>;
using RsMid = RsAtomic<RsMidBallot>;
using RsSmall = RsAtomic<RsSmallBallot>;
// the big tile of the split sort: with 8-byte values 12 keys per thread keep staging + auxiliary bytes inside the 160 KB of LDS
template <typename V> constexpr int RS_SPLIT_BIG_IPT = sizeof(V) == 8 ? 12 : 16;
// key-only: the same 16 Ki-key tile from 2^23 keys on, a 4 Ki-key tile below
using RsKeyBigBallot = RsCfg<16, false, false, 1024, false, 1, 0, 4>;
using RsKeySmallBallot = RsCfg<16, false, false>;
using RsKeyBig = RsAtomic<RsKeyBigBallot>;
using RsKeySmall = RsAtomic<RsKeySmallBallot>;
// look-back-free generated passes (TextGen::tile_base): 512 threads x 16 keys, two workgroups per CU
using RsGen8 = RsAtomic<RsCfg<16, true, true, 512, false, 1, 0, 4>>;
// in-bucket passes of the MSD-first sort: records of 8 bytes, so keys AND values of a 16 Ki tile fit the staging buffer at once — one
// write-out phase instead of two (3.45 instead of 3.62 ms per pass in tools/experiments/seg_bench.hip)
using RsMsdBucket = RsAtomic<RsCfg<16, false, true, 1024, false, 1, 0, 4>>;
// kept for A/B measurements (tools/sort_bench.py), pair sorts only, no generated first pass
using RsFirstVersion = RsCfg<15, false, false, 256, false, 1, 0, 1>;  // round-1 first version
using RsDmaLoads = RsCfg<16, true, true, 1024, false, 1, 0, 4, true>;  // 16 Ki tile, LDS-DMA loads, ballot ranking

template <bool NT_, typename T> __device__ __forceinline__ T rs_load(const T* p) {
    if constexpr (NT_) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT_, typename T> __device__ __forceinline__ void rs_store(T* p, T v) {
    if constexpr (NT_) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// Optional producer for the FIRST pass of the suffix-array sort: instead of reading (key, entry) pairs
// that a separate kernel would have to write first, the pass computes them from the text on the fly —
// key = the suffix's first `nsym` symbol codes (0 = end of document) as a number in base `base`, entry =
// (off << bits) | doc.  base = 2^symbits gives bit-aligned symbols; base = alphabet + 1 the densest key.
// Saves one write and one read of 8+w bytes per suffix plus the key read of the histogram kernel.
struct NoGen {};
struct TextGen {
    const uint8_t* text;
    const uint64_t* doc_start;
    const uint16_t* symmap;
    uint64_t ndocs;
    int bits;
    uint32_t base;
    int nsym;
    int low_bits = 0;  // split keys: the generated pass sorts on the key's low_bits lowest bits, which then travel
                       // as a separate byte per element; the remaining passes see key >> low_bits (32-bit keys)
    bool padded = false;  // text buffer has >= RS_GEN_LOOK + 16 readable bytes behind n
    bool first_only = false;  // entries-only partition by the first symbol: the key is just that symbol's digit
    int msd_shift = 0;  // > 0 (split records, MSD-first sort): the generated pass sorts on the key's TOP digit, key >> msd_shift,
                        // which is then implied by the bucket an element sits in — the records are (u32 key, entry) with no
                        // auxiliary byte at all, and the remaining passes sort every bucket on its own (radix_sort_msd)
    // Bucket-wise build, fused form (sa_build.hip): the generated pass writes the bucket RECORDS itself instead of partitioning
    // the entries for a later gather — sort digit = bucket slot of the suffix's first symbol (slotmap[code]), key = the
    // nsym - 1 symbols behind it as a dense number (k32 = key >> rec_low_bits), W = its low digits | entry bits 32.. above
    // them, value = entry bits 0..31.  16 Ki-key tiles only (thread-consecutive rolling keys); kernels of type TextGenRec.
    const uint8_t* slotmap = nullptr;  // [257] symbol code -> bucket slot
    int rec_low_bits = 0;
    // Leftover key bits (round 5, sweep form only): a key of nsym - 1 symbols in whole 8-bit passes leaves room for part_m >= 2 more
    // values below it — they hold the NEXT symbol quantised to part_m levels, floor(code * part_m / base) = (code * part_r) >>
    // part_s (monotone in the code, so the key stays order-preserving): key = dense * part_m + level.  part_m = 1: none.
    uint32_t part_m = 1, part_r = 0, part_s = 0;
    // MSD-first sort, pair form (6-symbol keys; kernels of type TextGenPair): top digit = (first two symbols as a number A) /
    // span, i.e. key / M with M = span * base^4 <= 2^32 — a function of two symbols, so its histogram comes from a pair count
    // of the text instead of a sweep that evaluates every key.  The generated pass works in 32-bit part arithmetic (G = three
    // symbols as a number, key = G(p) base^3 + G(p + 3)), lane-striped: every element straight from the staged codes.
    bool msd_pair = false;
    uint32_t pair_span = 0, pair_r = 0, pair_s = 0;  // floor(a / span) = (a * pair_r) >> pair_s for every a < base^2 (rs_pair_setup)
    const uint64_t* tile_doc = nullptr;  // [tiles + 1] document of each tile's first position (set by the driver)
    // Look-back-free form (round 4): tile_base[tile * 256 + d] = the output slot of the tile's first element of digit d, from a
    // counting pre-pass over the text + a scan over the tiles (the digit of a generated pass is a function of one or two symbols, so
    // its per-tile counts cost one cheap sweep).  The pass then needs no status words, no tile order and waits for nobody — which
    // is what lets two 8 Ki-key workgroups share a CU (with the chained scan, twice the tiles cost more than the overlap gained)
    const unsigned long long* tile_base = nullptr;
    uint8_t* vout_hi = nullptr;  // 8-byte values (first_only partition): write them packed — low words to (uint32_t*)vout, bits 32..39 here
};
// The generator's FORM is part of the kernel's type: the 16 Ki-tile pass is ~15 k instructions of straight-line code per
// form (everything is unrolled 16 x), and a kernel that carries all three runs 4 % slower than one that carries its own
// (tools/experiments/gen_bench.hip, -DRS_GEN_MODES: 5.55 vs 5.31 ms).  TextGen itself = the rolling-key form.
struct TextGenPair : TextGen {};  // MSD-first sort, pair form (msd_pair)
struct TextGenRec : TextGen {};   // bucket records (rec_mode), thread-consecutive rolling keys
constexpr int RS_GEN_LOOK = 64;
// timing-only ablations of the generated pass (tools/experiments/gen_bench.hip; WRONG results): 1 = no key arithmetic,
// 2 = no transposition through LDS, 4 = no text staging
#ifndef RS_GEN_ABL
#define RS_GEN_ABL 0
#endif
// ... and of the final pass of a segmented sort (WRONG results): 1 = no flag stores, 2 = no entry stores, 4 = no neighbour
// compares.  Compile-time (make HIPFLAGS+=-DRS_SEG_ABL=n): the product kernel carries no checks for them.
#ifndef RS_SEG_ABL
#define RS_SEG_ABL 0
#endif

// Segmented passes (the bucket-wise build of corpora >= 2^32, sa_build.hip): ONE launch sorts every first-symbol
// bucket ("segment") of a bucket group on its own — a tile belongs to exactly one segment (tile_seg), takes its digit
// starts from that segment's table, and the look-back chain restarts at the segment's first tile.  Replaces one
// launch per bucket and pass (~1000 launches per 4 GiB build) by one launch per pass.
struct NoSeg {};
struct SegInfo {
    unsigned long long begin, end;  // element range of the segment inside the group's record buffers
    uint32_t tile_begin, top;       // its first tile; MSD-first sort: the top digit every key of the segment shares
    // final pass only: the sorted segment [0, a) [a, b) [b, len) is written as [0, a) [b, len) [a, b) — the reference's child
    // order inside a radix node (end of document, bytes 0x80..0xFF, bytes 0x00..0x7F; index.h:66-73).  a = b = 0: as sorted
    unsigned long long rot_a, rot_b;
};
// where slot r of a segment goes under that block swap
__device__ __forceinline__ unsigned long long rs_seg_rotated(const SegInfo& si, unsigned long long slot) {
    if (si.rot_b == 0) return slot;
    const unsigned long long r = slot - si.begin, len = si.end - si.begin;
    if (r < si.rot_a) return slot;
    return r < si.rot_b ? slot + (len - si.rot_b) : slot - (si.rot_b - si.rot_a);
}
struct SegArgs {
    const uint32_t* tile_seg = nullptr;  // [tiles] segment of every tile
    const SegInfo* segs = nullptr;
    uint32_t tiles = 0;                  // tiles of all segments together
    uint32_t start_stride = 0;           // digit starts of segment g at digit_start[g * start_stride + d]
};
// A segmented pass on the low byte of u16 aux words that writes them WITHOUT that byte, as bytes: the top-digit-first sort
// (radix_sort_top_first) sorts on the key's top byte here, and the cell a record lands in implies it from then on.
struct SegShrinkArgs : SegArgs {
    uint8_t* wout8 = nullptr;  // [m] aux >> 8 of every record, in output order (the pass's own wout is not written)
};
// The LAST pass of a segmented sort of packed bucket records writes the finished suffix-array entries and their
// group flags instead of the records: entry = (aux >> hi_shift) << 32 | value, flag bit0 = first of a group of equal
// keys, bit1 = still unresolved (sa_initial_direct.hip: sa_flags_of).  A tile sees the neighbours of all its elements except
// across the ends of its per-digit runs, whose true neighbours sit in other tiles: those elements get provisional
// flags (head / tail assumed), every (tile, digit) run leaves an edge record, and rs_seg_edge_fix_kernel settles them.
struct SegEdge {
    unsigned long long first, last;  // full keys of the run's first and last element
    unsigned long long pos;          // output slot (inside the group) of the run's first element
    uint32_t cnt, pad;
};
struct SegFinalArgs : SegArgs {
    uint64_t* eout = nullptr;   // entries of the group (already offset to the group's first slot)
    uint32_t* elo = nullptr;    // ... or, packed storage (index_impl.h: Sa40): their low words and
    uint8_t* ehi = nullptr;     //     their bits 32..39 (elo != nullptr selects this form)
    uint8_t* flags = nullptr;   // ... and its flags
    SegEdge* edges = nullptr;   // [tiles][256]
    int hi_shift = 0;           // entry bits 32.. sit above this many bits of the auxiliary word
    int low_bits = 0;           // key = (k32 << low_bits) | (aux & (2^low_bits - 1))
    uint32_t kbase = 2;
    unsigned long long kmagic = 0;
    // carried bits (records_sweep.h: VlTables::carry): the aux word may hold code-stream bits above the entry's high bits; they
    // leave in bits 2.. of the flag byte, and the entry takes the aux high part masked to its real width
    uint32_t hi_mask = 0xFFFFFFFFu;  // entry bits 32.. = (aux >> hi_shift) & hi_mask
    uint32_t carry_mask = 0;         // flag byte = f | ((aux >> carry_shift) & carry_mask) << 2
    int carry_shift = 0;
};

// ... as a type of its own for the last pass over the CELLS of a top-digit-first sort (radix_sort_top_first): byte-wide aux words
// that hold nothing of the key (entry bits 32.. from bit 0, carried bits above them), 32-bit keys of variable-length code (a key
// ends inside the document <=> its bit 0 is clear), no bucket written rotated.  What SegFinalArgs reads from runtime fields per
// element is fixed here: head and tail come from the neighbouring keys alone, the aux byte is read from the LDS once and serves
// the flag byte and the entry, and a (tile, digit) run leaves a 16-byte edge record (seg_cell_edge.h).
struct SegFinalCellArgs : SegArgs {
    uint64_t* eout = nullptr;   // entries / packed entries / flags of the group: as in SegFinalArgs
    uint32_t* elo = nullptr;
    uint8_t* ehi = nullptr;
    uint8_t* flags = nullptr;
    SegCellEdge* edges = nullptr;  // [tiles][256]
    uint32_t hi_mask = 0xFFu;      // entry bits 32.. = aux & hi_mask
    uint32_t carry_mask = 0;       // flag byte = f | ((aux >> carry_shift) & carry_mask) << 2
    int carry_shift = 0;
};

// The last pass of an ordinary (single-segment) sort of split records can do the same and still write its records (the
// kept search keys): the suffix-array build below 2^32 then needs no flag kernel (5-6 B read + 1 B written per suffix).
// tile_sums (optional): per scan tile of `sums_tile` flags {unresolved entries, unresolved group heads} as pairs of u64 —
// what the first compaction of the refinement wants; counted here (unresolved entries are rare), corrected by the edge fix.
struct SegFinalKeepArgs : SegArgs {
    uint8_t* flags = nullptr;
    SegEdge* edges = nullptr;
    int low_bits = 0;
    uint32_t kbase = 2;
    unsigned long long kmagic = 0;
    unsigned long long* tile_sums = nullptr;
    uint32_t sums_tile = 1;
    // MSD-first sort (radix_sort_msd): the records have no auxiliary array (win == nullptr), the full key of an element is
    // (segment's top digit << msd_shift) | k32, and the pass writes the kept search keys in the layout of the LSD split sort —
    // (u32)(full >> 8) and the low byte — so that everything downstream of the sort is the same
    unsigned long long msd_m = 0;  // full key = top * msd_m + k32 (0: not an MSD-first sort)
};

// ... as a type of its own for the last pass of an MSD-first sort (no auxiliary input, full key = top * msd_m + k32): the
// auxiliary loads, their LDS traffic and the byte compares of the LSD form are not compiled into it
struct SegFinalKeepMsdArgs : SegFinalKeepArgs {};

// Key of the suffix at tile-local position li from symbol CODES staged in LDS (dword view, code of position i
// in byte i): Horner over the first nsym (<= 16) codes in base `base`, first symbol most significant; codes
// at or behind the end of the document (rem symbols left) count as 0.  Four codes at a time are combined
// with 32-bit operations (base <= 256, so four of them stay below 2^32).
__device__ __forceinline__ uint64_t rs_pack_key(const uint32_t* __restrict__ s_words, uint32_t li, int nsym, uint32_t base,
                                                uint32_t rem) {
    const uint32_t wi = li >> 2, sel = li & 3u;
    const uint32_t b2 = base * base, b3 = b2 * base;
    const uint32_t pw[5] = {1u, base, b2, b3, b3 * base};  // pw[4] wraps to 0 for base = 256: handled below
    uint64_t kk = 0;
    uint32_t lo = s_words[wi];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int q = 4 * w;
        if (q >= nsym) break;                           // uniform
        const int r = nsym - q < 4 ? nsym - q : 4;      // symbols taken from this window (uniform)
        const uint32_t hi = s_words[wi + w + 1];
        uint32_t x = __builtin_amdgcn_alignbyte(hi, lo, sel);  // codes of li + q .. li + q + 3
        lo = hi;
        if (rem < (uint32_t)(q + 4)) x = rem <= (uint32_t)q ? 0u : (x & ((1u << (8u * (rem - (uint32_t)q))) - 1u));
        uint32_t v = x & 0xFFu;
        if (r > 1) v = v * base + ((x >> 8) & 0xFFu);
        if (r > 2) v = v * base + ((x >> 16) & 0xFFu);
        if (r > 3) v = v * base + (x >> 24);
        kk = (r == 4 && pw[4] == 0u) ? ((kk << 32) | v) : kk * pw[r] + v;
    }
    return kk;
}

__device__ __forceinline__ uint64_t rs_doc_upper(const uint64_t* __restrict__ doc_start, uint64_t lo, uint64_t hi,
                                                 uint64_t p) {
    while (lo < hi) {  // largest d in [lo, hi] with doc_start[d] <= p
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (doc_start[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// every compile-time switch of one instantiation, derived once; the kernel body and its helpers read them from here
template <typename K_, typename V_, typename Cfg_, typename Gen_, typename W_, typename Seg_>
struct RsTraits {
    using K = K_;
    using V = V_;
    using Cfg = Cfg_;
    using Gen = Gen_;
    using W = W_;
    using Seg = Seg_;
    static constexpr bool GEN = !std::is_same<Gen, NoGen>::value;
    static constexpr bool SEG = !std::is_same<Seg, NoSeg>::value;
    static constexpr bool FINAL = std::is_same<Seg, SegFinalArgs>::value;
    static constexpr bool KEEPM = std::is_same<Seg, SegFinalKeepMsdArgs>::value;  // ... of an MSD-first sort (no auxiliary input)
    static constexpr bool KEEP = std::is_same<Seg, SegFinalKeepArgs>::value || KEEPM;  // flags + edge records beside the ordinary record write-out
    static constexpr bool CELL = std::is_same<Seg, SegFinalCellArgs>::value;  // last pass over the cells of a top-digit-first sort
    static constexpr bool FLAGS = FINAL || KEEP || CELL;
    static constexpr bool SHRINK = std::is_same<Seg, SegShrinkArgs>::value;  // the aux word leaves without its low byte, as a byte (seg.wout8)
    static constexpr bool HAS_V = !std::is_same<V, NoVal>::value;
    static constexpr bool HAS_W = !std::is_same<W, NoVal>::value;
    using WS = typename std::conditional<HAS_W, W, uint8_t>::type;
    using VS = typename std::conditional<HAS_V, V, uint32_t>::type;
    static constexpr int IPT = Cfg::IPT;
    static constexpr bool REUSE = Cfg::REUSE && HAS_V;
    static constexpr bool EARLYV = (Cfg::EARLYV || REUSE) && HAS_V;
    static constexpr int NT = Cfg::NT;
    static constexpr int NW = NT / 64;
    static constexpr bool NTM = Cfg::NONTEMP;
    static constexpr int TILE = NT * IPT;
    static constexpr int WCHUNK = 64 * IPT;  // elements owned by one wave (contiguous => stable)
    static constexpr size_t STAGE_K = sizeof(K) * TILE;
    static constexpr size_t STAGE_V = HAS_V ? sizeof(VS) * TILE : 0;
    static constexpr size_t STAGE_BYTES = REUSE ? (STAGE_K > STAGE_V ? STAGE_K : STAGE_V) : STAGE_K + STAGE_V;
    // the three generator forms (the form is part of the kernel's type, see TextGenPair)
    static constexpr bool GM_PAIR = std::is_same<Gen, TextGenPair>::value;
    static constexpr bool GM_REC = std::is_same<Gen, TextGenRec>::value;
    // BLK: the generated pass of the big 32-bit-record configuration computes its keys thread-consecutively
    // (rolling: the `else if constexpr (T::BLK)` branch of the kernel's generated load); text codes, code table and document table then live in their own LDS region
    // because the staging buffer carries the transposition
    static constexpr bool BLK = GEN && sizeof(K) == 4 && sizeof(VS) == 4 && IPT == 16 && (NT == 1024 || NT == 512);
    static constexpr uint32_t GEN_TEXTB = ((TILE + RS_GEN_LOOK + 15) / 16) * 16;
    static constexpr uint32_t GEN_DOCS = 1024;
    static constexpr uint32_t GEN_SLOTS = 320;  // code -> bucket slot (records mode), behind the document table
    static constexpr size_t GEN_BYTES = BLK ? GEN_TEXTB + 512 + GEN_DOCS * 8 + GEN_SLOTS : 16;
    // layout of the generator's LDS region (s_gen when BLK, else the still unused staging buffer): text codes, code map,
    // document table, slot map
    static constexpr uint32_t MAP_OFF = GEN_TEXTB;
    static constexpr uint32_t DOC_OFF = GEN_TEXTB + 512;
    static constexpr uint32_t DOC_CAP = BLK ? GEN_DOCS : (uint32_t)((STAGE_BYTES - DOC_OFF) / 8);
    static constexpr uint32_t SLOT_OFF = GEN_TEXTB + 512 + GEN_DOCS * 8;
    // W32G: a generated pass with 4-byte auxiliary words (bucket records with two or three low digits) has no room for them
    // beside text + records: they cross the tile through the staging buffer in a phase of their own, like keys and values
    static constexpr bool W32G = GEN && HAS_W && sizeof(WS) == 4;
    static constexpr bool AUX_LDS = HAS_W && !W32G && !KEEPM;  // the tile's auxiliary words have an LDS array of their own (s_aux)
    static constexpr size_t AUX_ELEMS = AUX_LDS ? TILE : 1;
    static constexpr bool LOAD_W = HAS_W && !KEEPM;  // (the final pass of an MSD-first sort has no auxiliary input)
    // keys and values reach the registers through LDS by DMA (RsCfg::DMA) — materialised 8-byte keys with early values only
    static constexpr bool DMA_PATH = !GEN && Cfg::DMA && HAS_V && EARLYV && sizeof(K) == 8 && (IPT % 4) == 0;

    static_assert(!SHRINK || (std::is_same<W, uint16_t>::value && Cfg::REUSE && !std::is_same<V, NoVal>::value), "shrinking pass: u16 aux words, shared staging");
    static_assert(!SEG || (!GEN && !Cfg::DMA), "segmented passes: materialised records");
    static_assert(!CELL || (std::is_same<K, uint32_t>::value && std::is_same<V, uint32_t>::value && std::is_same<W, uint8_t>::value && (IPT % 4) == 0),
                  "last pass over cells: (u32, u32, u8) records");
    static_assert(!FLAGS || Cfg::REUSE || KEEPM, "flag-writing passes: shared staging (the MSD-first last pass also runs with keys and values staged at once)");
    static_assert(!HAS_W || KEEPM || (Cfg::REUSE && HAS_V && !Cfg::DMA), "the auxiliary byte needs the shared-staging configuration");
    static_assert(!(GM_PAIR || GM_REC) || (BLK && HAS_W), "pair / records generators: 16 Ki tiles with an auxiliary word");
    static_assert(!GEN || EARLYV, "generator pass needs early values");
    static_assert(!GEN || STAGE_BYTES >= (size_t)TILE + RS_GEN_LOOK + 2048, "staging buffer too small for the text tile");
};
// The group-flag rule of the flag-writing passes: flag byte of an element — bit0 = first of a group of equal keys, bit1 = still
// unresolved, `carry` above them — from its neighbours' equality and its composite key kc; written to flags[slot] and counted
// in tile_sums.  (the "key ends inside the document" test — a 64-bit division by the alphabet size — only for the rare element
// that has an equal neighbour: the pass stays memory-bound)
template <typename T>
__device__ __forceinline__ uint32_t rs_group_flag(const typename T::Seg& seg, bool head, bool tail, uint64_t kc, uint64_t slot,
                                                  uint32_t carry) {
    uint32_t f = head ? 1u : 0u;
    if (!(head && tail)) {
        const bool exhausted = seg.kmagic ? (kc - __umul64hi(kc, seg.kmagic) * seg.kbase) == 0
                                          : (kc & (uint64_t)(seg.kbase - 1u)) == 0;
        if (!exhausted) f |= 2u;
    }
    f |= carry;
    if (!(T::FINAL && (RS_SEG_ABL & 1))) seg.flags[slot] = (uint8_t)f;
    if constexpr (T::KEEP) {
        if ((f & 2u) && seg.tile_sums) {  // (rare: a fraction of a percent of the suffixes stays unresolved)
            atomicAdd(seg.tile_sums + 2 * (slot / seg.sums_tile), 1ull);
            if (f & 1u) atomicAdd(seg.tile_sums + 2 * (slot / seg.sums_tile) + 1, 1ull);
        }
    }
    return f;
}

// One array of the tile, wave-striped (element j of a thread is tile slot wbase + j * 64: lane-contiguous 512 B per load
// instruction).  PRED: predicated loads, slots behind the tile's elements take `pad`; else every slot loads (slots behind the end
// re-read the last element and are masked afterwards).
template <bool NTM, bool PRED, typename E, typename R, int N>
__device__ __forceinline__ void rs_load_striped(const E* src, uint64_t base, uint32_t wbase, uint32_t valid, R (&dst)[N], R pad) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const uint32_t li = wbase + j * 64;
        if constexpr (PRED) dst[j] = li < valid ? rs_load<NTM>(src + base + li) : pad;
        else dst[j] = rs_load<NTM>(src + base + (li < valid ? li : valid - 1));  // (valid >= 1: the grid has ceil(n / TILE) tiles)
    }
}

// one radix pass: rank inside the tile, look back for the global prefix, scatter.
// W (optional, u8 or u16) = auxiliary low digits of a split key that travel with the pair (TextGen::low_bits);
// aux_shift >= 0 makes this pass sort on (aux >> aux_shift) & dmask instead of a key digit (the leading
// passes of a split sort: the first, generated one, and for two low digits the one after it).
template <typename K, typename V, typename Cfg, typename Gen = NoGen, typename W = NoVal, typename Seg = NoSeg>
__global__ __launch_bounds__(Cfg::NT, Cfg::MINW) void rs_onesweep_kernel(
    const K* __restrict__ kin, K* __restrict__ kout, const V* __restrict__ vin, V* __restrict__ vout, uint64_t n,
    int shift, uint32_t dmask, const unsigned long long* __restrict__ digit_start, uint64_t* __restrict__ status,
    uint32_t* __restrict__ ticket, uint32_t epoch, uint32_t* __restrict__ err, Gen gen = Gen(),
    const W* __restrict__ win = nullptr, W* __restrict__ wout = nullptr, int aux_shift = -1, Seg seg = Seg()) {
    using T = RsTraits<K, V, Cfg, Gen, W, Seg>;
    using WS = typename T::WS;
    using VS = typename T::VS;
    __shared__ __attribute__((aligned(16))) unsigned char s_stage[T::STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char s_gen[T::GEN_BYTES];
    __shared__ WS s_aux[T::AUX_ELEMS];
    __shared__ uint64_t s_gbase[256];
    __shared__ uint32_t s_whist[T::NW][256];
    __shared__ uint32_t s_tstart[256];
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_tile;
    K* s_keys = reinterpret_cast<K*>(s_stage);
    VS* s_vals = reinterpret_cast<VS*>(s_stage + (T::REUSE ? 0 : T::STAGE_K));

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (Cfg::GROUP > 0 && !Cfg::TICKET) {
        // static form of the XCD-aware order (experiment): no atomic round trip in front of the tile; relies on workgroups
        // being dispatched in blockIdx order inside an XCD (bounded spins catch a violation)
    } else if constexpr (Cfg::GROUP > 0) {
        if (tid == 0) {
            const uint32_t x = blockIdx.x & 7u;
            const uint32_t slot = atomicAdd(ticket + x, 1u);
            s_tile = ((slot / Cfg::GROUP) * 8u + x) * Cfg::GROUP + slot % Cfg::GROUP;
        }
    } else if constexpr (Cfg::TICKET) {
        if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    }
    // A pass whose look-back timed out leaves its output partly unwritten; a LATER pass over that output would see digit
    // counts its digit starts were not made for and scatter out of bounds (seen as GPU memory faults when two processes
    // shared one device and starved each other's XCD-ordered passes).  Once the error flag is up every tile only publishes
    // an (empty) inclusive prefix — nobody waits for it — and leaves; the host finds the flag and redoes the sort.
    __shared__ uint32_t s_bad;
    if (tid == 0) s_bad = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = tid; i < T::NW * 256; i += T::NT) (&s_whist[0][0])[i] = 0;
    __syncthreads();
    uint64_t tile;
    if constexpr (Cfg::GROUP > 0 && !Cfg::TICKET) {
        const uint32_t x = blockIdx.x & 7u, slot = blockIdx.x >> 3;
        tile = (uint64_t)((slot / Cfg::GROUP) * 8u + x) * Cfg::GROUP + slot % Cfg::GROUP;
    } else {
        tile = (Cfg::TICKET || Cfg::GROUP > 0) ? (uint64_t)s_tile : (uint64_t)blockIdx.x;
    }
    uint64_t base = tile * T::TILE;
    uint64_t tile0 = 0;     // first tile of the look-back chain this tile belongs to
    uint64_t seg_n = n;     // end of the element range the tile may read
    uint32_t sg = 0;
    SegInfo si = {};
    uint64_t ktop = 0;  // MSD-first final pass: the segment's top digit, in place above the 32 key bits
    if constexpr (T::SEG) {
        if (tile >= (uint64_t)seg.tiles) return;  // (the grid is rounded up to whole tile groups)
        sg = seg.tile_seg ? seg.tile_seg[tile] : 0u;  // (no map: one segment)
        si = seg.segs[sg];
        tile0 = si.tile_begin;
        base = si.begin + (tile - tile0) * T::TILE;
        seg_n = si.end;
        if constexpr (T::KEEPM) ktop = (uint64_t)si.top * seg.msd_m;
    } else if constexpr (Cfg::GROUP > 0) {
        if (base >= n) return;  // (the grid is rounded up to whole groups; nobody looks back at a tile behind the input)
    }
    const uint32_t valid = (uint32_t)((seg_n - base) < (uint64_t)T::TILE ? (seg_n - base) : (uint64_t)T::TILE);
    if (s_bad) {
        if constexpr (T::GEN) {
            if (gen.tile_base) return;  // (no status words in the look-back-free form: nobody waits for this tile)
        }
        if (tid < 256) rs_st_status(status + tile * 256 + tid, ((uint64_t)epoch << 56) | (2ull << 54));
        return;
    }

    // ---- load keys (and values), wave-striped: lane-contiguous 512 B per load instruction
    K key[T::IPT];
    VS val[T::EARLYV ? T::IPT : 1];
    WS aux[T::HAS_W ? T::IPT : 1] = {};
    uint32_t gdig[T::GM_REC ? T::IPT / 4 : 1] = {};  // records generators: the elements' sort digits, four per register
    auto digit_of = [&](K k, WS a) -> uint32_t {
        if constexpr (T::HAS_W && !T::CELL) {  // (a cell's aux byte holds no digit)
            if (aux_shift >= 0) return ((uint32_t)a >> aux_shift) & dmask;
        }
        return (uint32_t)(k >> shift) & dmask;
    };
    const uint32_t wbase = wave * T::WCHUNK + lane;
    if constexpr (T::GEN) {
        // stage the text of this tile (+ look-ahead) in the still unused LDS staging buffer
        unsigned char* const gbuf = T::BLK ? s_gen : s_stage;
        uint8_t* s_text = gbuf;
        uint16_t* s_map = reinterpret_cast<uint16_t*>(gbuf + T::MAP_OFF);
        // document boundaries of this tile, copied to LDS when they fit (binary searches then cost
        // LDS instead of L2 latency); s_docs[i] = doc_start[dlo + i]
        uint64_t* s_docs = reinterpret_cast<uint64_t*>(gbuf + T::DOC_OFF);
        // (one workgroup per CU: every dependent global round trip at the head of a tile — ~1-2 us each — is dead time for
        //  the whole CU.  The text of a 16 Ki tile is ONE 16-byte load per thread: it is issued first, beside the tile's
        //  document range, and lands while the document table and the code map are staged)
        constexpr bool PRELOAD = T::BLK;  // (16 Ki tiles: TILE == 16 * NT; the look-ahead is a second load of the first threads)
        uint4 tw0 = make_uint4(0, 0, 0, 0), tw1 = make_uint4(0, 0, 0, 0);
        bool tw0_ok = false, tw1_ok = false;
        if constexpr (PRELOAD) {
            const uint64_t g0 = base + (uint64_t)tid * 16, g1 = base + (uint64_t)T::TILE + (uint64_t)tid * 16;
            tw0_ok = gen.padded ? (g0 < n + RS_GEN_LOOK) : (g0 + 16 <= n);
            tw1_ok = (uint32_t)tid * 16 < (uint32_t)RS_GEN_LOOK && (gen.padded ? (g1 < n + RS_GEN_LOOK) : (g1 + 16 <= n));
            if (tw0_ok) tw0 = *reinterpret_cast<const uint4*>(gen.text + g0);
            if (tw1_ok) tw1 = *reinterpret_cast<const uint4*>(gen.text + g1);
        }
        const uint64_t dlo = gen.tile_doc[tile], dhi = gen.tile_doc[tile + 1];
        for (int i = tid; i < 256; i += T::NT) s_map[i] = gen.symmap[i];
        if constexpr (T::GM_REC) {
            if (tid < 257) (gbuf + T::SLOT_OFF)[tid] = gen.slotmap[tid];
        }
        const bool docs_in_lds = dhi - dlo + 2 <= (uint64_t)T::DOC_CAP;
        if (docs_in_lds)
            for (uint32_t i = tid; i < (uint32_t)(dhi - dlo + 2); i += T::NT) s_docs[i] = gen.doc_start[dlo + i];
        __syncthreads();
        // bytes -> symbol codes on their way into LDS: one table lookup per text byte instead of one per
        // (suffix, symbol)
        for (uint32_t i = tid * 16; i < (uint32_t)T::TILE + RS_GEN_LOOK; i += T::NT * 16) {
            if (RS_GEN_ABL & 4) break;
            const uint64_t g = base + i;
            uint32_t x[4];
            if (PRELOAD && (i < (uint32_t)T::TILE ? tw0_ok : tw1_ok)) {
                const uint4 w = i < (uint32_t)T::TILE ? tw0 : tw1;
                x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
            } else if (!PRELOAD && (gen.padded ? (g < n + RS_GEN_LOOK) : (g + 16 <= n))) {
                const uint4 w = *reinterpret_cast<const uint4*>(gen.text + g);
                x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    x[q] = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        x[q] |= (uint32_t)((g + 4 * q + b < n) ? gen.text[g + 4 * q + b] : (uint8_t)0) << (8 * b);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                x[q] = (uint32_t)s_map[x[q] & 0xFF] | ((uint32_t)s_map[(x[q] >> 8) & 0xFF] << 8) |
                       ((uint32_t)s_map[(x[q] >> 16) & 0xFF] << 16) | ((uint32_t)s_map[x[q] >> 24] << 24);
            *reinterpret_cast<uint4*>(&s_text[i]) = make_uint4(x[0], x[1], x[2], x[3]);
        }
        __syncthreads();
        // Per-document state lives in registers and changes only when a thread's positions (ascending by 64)
        // leave the document: its end in tile-local 32-bit coordinates (clamped — only "fewer than nsym symbols
        // left" matters) and ebase = doc - (doc_start << bits), so that entry = (position << bits) + ebase.
        uint64_t d = dlo;
        uint32_t dend_l = 0;  // tile-local end of the current document (0 = not looked up yet)
        uint64_t ebase = 0;
        const int nsym = gen.nsym;
        const uint32_t* s_words = reinterpret_cast<const uint32_t*>(s_text);
        if constexpr (T::GM_PAIR) {
            // Lane-striped generation of the pair form: a key is two 3-symbol parts of the six codes at its position — cheap
            // enough (four multiply-adds) to be evaluated per element straight from the staged codes, in the order the ranking
            // wants them: no transposition of keys, digits and entries through the staging buffer, no barriers.
            // Arithmetic (round 4): the six codes at a position are three PAIRS a = c0 B + c1, m = c2 B + c3, r = c4 B + c5 — one
            // v_dot4_u32_u8 each on the byte-aligned code windows — and with top = floor(a / span), M = span B^4:
            //     key - top M = ((a - top span) B^2 + m) B^2 + r,
            // all products of operands below 2^24 (v_mul_u32_u24 / v_mad_u32_u24, full rate; the 3-symbol parts of round 3
            // needed two 32-bit multiplies and a multiply-high per suffix, quarter rate each).  floor(a / span) = (a R) >> s
            // with (R, s) checked on the host for every a < B^2 (rs_pair_setup).
            const uint32_t B = gen.base, B2 = B * B;
            const uint32_t wlo = B | (1u << 8), whi = (B << 16) | (1u << 24);  // dot4 weights: bytes 0,1 / bytes 2,3
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) {
                const uint32_t li = wbase + j * 64;
                key[j] = (K)~(K)0;
                val[j] = VS(0);
                aux[j] = WS(0);
                if (li < valid) {
                    if (li >= dend_l) {  // (also the first element: dend_l = 0)
                        const uint64_t p = base + li;
                        uint64_t ds, de;
                        if (docs_in_lds) {
                            d = dlo + rs_doc_upper(s_docs, d - dlo, dhi - dlo, p);
                            ds = s_docs[d - dlo];
                            de = s_docs[d - dlo + 1];
                        } else {
                            d = rs_doc_upper(gen.doc_start, d, dhi, p);
                            ds = gen.doc_start[d];
                            de = gen.doc_start[d + 1];
                        }
                        const uint64_t rel = de - base;
                        dend_l = rel < (1ull << 30) ? (uint32_t)rel : (1u << 30);
                        ebase = d - (ds << gen.bits);
                    }
                    const uint32_t wi = li >> 2, sel = li & 3u;
                    const uint32_t w0 = s_words[wi], w1 = s_words[wi + 1], w2 = s_words[wi + 2];
                    uint32_t x0 = __builtin_amdgcn_alignbyte(w1, w0, sel);  // codes of li .. li + 3
                    uint32_t x1 = __builtin_amdgcn_alignbyte(w2, w1, sel);  // codes of li + 4 .. li + 7
                    const uint32_t rem = dend_l - li;  // symbols left in the document (>= 1)
                    if (rem < 6u) {  // (rare) the symbols behind the document end count as 0
                        x0 = rem >= 4u ? x0 : (x0 & ((1u << (8u * rem)) - 1u));
                        x1 = rem <= 4u ? 0u : (x1 & 0xFFu);
                    }
                    const uint32_t a = __builtin_amdgcn_udot4(x0, wlo, 0u, false);
                    const uint32_t m = __builtin_amdgcn_udot4(x0, whi, 0u, false);
                    const uint32_t r = __builtin_amdgcn_udot4(x1, wlo, 0u, false);
                    const uint32_t top = __umul24(a, gen.pair_r) >> gen.pair_s;
                    const uint32_t a2 = a - __umul24(top, gen.pair_span);
                    key[j] = (K)(__umul24(__umul24(a2, B2) + m, B2) + r);  // key - top * M (< M <= 2^32)
                    aux[j] = (WS)top;
                    val[j] = (VS)((((uint32_t)base + li) << gen.bits) + (uint32_t)ebase);
                }
            }
        } else if constexpr (T::BLK) {
            // Thread-consecutive generation: a thread owns IPT consecutive positions, so inside a document
            //   key(q + 1) = (key(q) - code(q) * base^(nsym-1)) * base + code(q + nsym)   [0 behind the document end]
            // and only the first position of a thread or of a document pays for a full Horner evaluation; the
            // document state changes at most a few times per thread.  The records then cross to the
            // lane-consecutive order of the ranking through the (XOR-swizzled, conflict-free) staging buffer.
            uint32_t* kt = reinterpret_cast<uint32_t*>(s_stage);
            auto swz = [](uint32_t q) -> uint32_t { return (q & ~15u) | ((q & 15u) ^ ((q >> 6) & 15u)); };
            const uint32_t q0 = (uint32_t)tid * T::IPT;
            // (GM_REC, bucket records: key = the nsym - 1 symbols BEHIND the first one, 40-bit entries)
            constexpr uint32_t OFF = T::GM_REC ? 1u : 0u;  // the key's window starts this far behind the position
            const int nwin = nsym - (int)OFF;           // symbols in the window
            uint64_t top = 1;  // weight of the symbol that leaves the window
            for (int q = 1; q < nwin; ++q) top *= gen.base;
            uint64_t lmask = 0;
            if constexpr (T::GM_REC) lmask = (1ull << gen.rec_low_bits) - 1ull;
            uint32_t ent[T::IPT];
            uint32_t auxc[T::W32G ? T::IPT : 1] = {};  // (W32G) the auxiliary words of the thread's consecutive positions
            uint64_t kk = 0;
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) {
                const uint32_t q = q0 + j;
                ent[j] = 0;
                if (q < valid) {
                    bool fresh = j == 0;
                    if (j == 0 || q >= dend_l) {
                        const uint64_t p = base + q;
                        uint64_t ds, de;
                        if (docs_in_lds) {
                            d = dlo + rs_doc_upper(s_docs, d - dlo, dhi - dlo, p);
                            ds = s_docs[d - dlo];
                            de = s_docs[d - dlo + 1];
                        } else {
                            d = rs_doc_upper(gen.doc_start, d, dhi, p);
                            ds = gen.doc_start[d];
                            de = gen.doc_start[d + 1];
                        }
                        const uint64_t rel = de - base;
                        dend_l = rel < (1ull << 30) ? (uint32_t)rel : (1u << 30);
                        ebase = d - (ds << gen.bits);
                        fresh = true;
                    }
                    if (fresh) {
                        kk = rs_pack_key(s_words, q + OFF, nwin, gen.base, dend_l - q - OFF);
                    } else {
                        const bool more = T::GM_REC ? q + (uint32_t)nsym - 1u < dend_l : q + (uint32_t)nsym <= dend_l;
                        const uint64_t cin = more ? (uint64_t)s_text[q + nsym - 1] : 0ull;
                        kk = (kk - (uint64_t)s_text[q - 1 + OFF] * top) * gen.base + cin;
                    }
                    if constexpr (T::GM_REC) {
                        const uint64_t e64 = ((base + q) << gen.bits) + ebase;
                        kt[swz(q)] = (uint32_t)(kk >> gen.rec_low_bits);
                        if constexpr (T::W32G) auxc[j] = (uint32_t)((kk & lmask) | ((e64 >> 32) << gen.rec_low_bits));
                        else if constexpr (T::HAS_W) s_aux[swz(q)] = (WS)((kk & lmask) | ((e64 >> 32) << gen.rec_low_bits));
                        ent[j] = (uint32_t)e64;
                    } else {
                        const uint64_t kx = kk;
                        if (gen.msd_shift) {  // (uniform)
                            kt[swz(q)] = (uint32_t)kx;
                            if constexpr (T::HAS_W && !T::W32G) s_aux[swz(q)] = (WS)(kx >> gen.msd_shift);
                        } else {
                            kt[swz(q)] = (uint32_t)(kx >> gen.low_bits);
                            if constexpr (T::HAS_W && !T::W32G) s_aux[swz(q)] = (WS)(kx & ((1ull << gen.low_bits) - 1ull));
                        }
                        ent[j] = (((uint32_t)base + q) << gen.bits) + (uint32_t)ebase;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) {
                const uint32_t li = wbase + j * 64;
                key[j] = li < valid ? (K)kt[swz(li)] : (K)~(K)0;
                if constexpr (T::HAS_W && !T::W32G) aux[j] = li < valid ? s_aux[swz(li)] : WS(0);
            }
            __syncthreads();
            if constexpr (T::W32G) {
#pragma unroll
                for (int j = 0; j < T::IPT; ++j) kt[swz(q0 + j)] = auxc[j];
                __syncthreads();
#pragma unroll
                for (int j = 0; j < T::IPT; ++j) {
                    const uint32_t li = wbase + j * 64;
                    aux[j] = li < valid ? (WS)kt[swz(li)] : WS(0);
                }
                __syncthreads();
            }
            if (RS_GEN_ABL & 2) {
#pragma unroll
                for (int j = 0; j < T::IPT; ++j) val[j] = (VS)ent[j];
            } else {
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) kt[swz(q0 + j)] = ent[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) {
                const uint32_t li = wbase + j * 64;
                val[j] = li < valid ? (VS)kt[swz(li)] : VS(0);
            }
            }
            if constexpr (T::GM_REC) {  // sort digits of the thread's (lane-striped) elements: bucket slot of the first symbol
                const uint8_t* s_slot = gbuf + T::SLOT_OFF;
#pragma unroll
                for (int j = 0; j < T::IPT; ++j) {
                    const uint32_t li = wbase + j * 64;
                    gdig[j >> 2] |= (uint32_t)s_slot[s_text[li < valid ? li : 0u]] << (8 * (j & 3));
                }
            }
        } else {
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t li = wbase + j * 64;
            key[j] = (K)~(K)0;
            val[j] = VS(0);
            if constexpr (T::HAS_W) aux[j] = WS(0);
            if (li < valid) {
                if (li >= dend_l) {  // (also the first element: dend_l = 0)
                    const uint64_t p = base + li;
                    uint64_t ds, de;
                    if (docs_in_lds) {
                        d = dlo + rs_doc_upper(s_docs, d - dlo, dhi - dlo, p);
                        ds = s_docs[d - dlo];
                        de = s_docs[d - dlo + 1];
                    } else {
                        d = rs_doc_upper(gen.doc_start, d, dhi, p);
                        ds = gen.doc_start[d];
                        de = gen.doc_start[d + 1];
                    }
                    const uint64_t rel = de - base;
                    dend_l = rel < (1ull << 30) ? (uint32_t)rel : (1u << 30);
                    ebase = d - (ds << gen.bits);
                }
                uint64_t kk = gen.first_only ? ((uint64_t)s_text[li] << shift)
                                             : rs_pack_key(s_words, li, nsym, gen.base, dend_l - li);
                if constexpr (T::HAS_W) {
                    if (gen.msd_shift) {  // (uniform)
                        aux[j] = (WS)(kk >> gen.msd_shift);
                        key[j] = (K)kk;
                    } else {
                        aux[j] = (WS)(kk & ((1ull << gen.low_bits) - 1ull));
                        key[j] = (K)(kk >> gen.low_bits);
                    }
                } else {
                    key[j] = (K)kk;
                }
                if constexpr (sizeof(VS) == 4) val[j] = (VS)((((uint32_t)base + li) << gen.bits) + (uint32_t)ebase);
                else val[j] = (VS)(((base + li) << gen.bits) + ebase);
            }
        }
        }
        // the staging buffer is reused for the sorted keys below (the pair generator never touched it: its codes, code table and
        // document table live in s_gen, which nothing writes before the next barrier)
        if constexpr (!T::GM_PAIR) __syncthreads();
    } else if constexpr (T::DMA_PATH) {
        // Keys and values travel global -> LDS by 16-byte-per-lane DMA (global_load_lds: full-rate 1 KiB
        // per wave instruction, no staging registers) into this wave's slice of the still unused
        // staging buffer, and are read back striped.  The value DMA overlaps the ranking below.
        typedef __attribute__((address_space(1))) const void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        unsigned char* wdst = s_stage + (size_t)wave * T::WCHUNK * sizeof(K);
        // clamp to the last 16-byte vector that holds a real element (device blocks are padded to 256 B)
        const uint64_t last_pair = (n - 1) & ~1ull;
#pragma unroll
        for (int i = 0; i < T::IPT / 2; ++i) {
            uint64_t e = base + (uint64_t)wave * T::WCHUNK + i * 128 + 2 * lane;
            e = e < last_pair ? e : last_pair;
            __builtin_amdgcn_global_load_lds((gptr_t)(kin + e), (lptr_t)(wdst + i * 1024), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t li = wbase + j * 64;
            const K kk = reinterpret_cast<const K*>(wdst)[j * 64 + lane];
            key[j] = li < valid ? kk : (K)~(K)0;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slice is free again: reuse it for the values
        constexpr int VPL = 16 / (int)sizeof(VS);             // values per lane per DMA
        const uint64_t last_vec = (n - 1) & ~(uint64_t)(VPL - 1);
#pragma unroll
        for (int i = 0; i < T::IPT / VPL; ++i) {
            uint64_t e = base + (uint64_t)wave * T::WCHUNK + i * (64 * VPL) + VPL * lane;
            e = e < last_vec ? e : last_vec;
            __builtin_amdgcn_global_load_lds((gptr_t)(vin + e), (lptr_t)(wdst + i * 1024), 16, 0, 0);
        }
    } else {
        // RsCfg::LOAD 0: predicated loads, keys -> values -> auxiliary digits.  1, 2: unpredicated — straight-line code lets the
        // compiler count outstanding loads exactly, so the ranking starts as soon as what it needs has landed (loads return in
        // issue order); 1 = keys -> digits -> values (values in flight under the ranking), 2 = keys -> values -> digits
        constexpr bool PRED = Cfg::LOAD == 0;
        rs_load_striped<T::NTM, PRED>(kin, base, wbase, valid, key, (K)~(K)0);
        if constexpr (T::LOAD_W && Cfg::LOAD == 1) rs_load_striped<T::NTM, PRED>(win, base, wbase, valid, aux, WS(0));
        if constexpr (T::EARLYV) rs_load_striped<T::NTM, PRED>(vin, base, wbase, valid, val, VS(0));
        if constexpr (T::LOAD_W && Cfg::LOAD != 1) rs_load_striped<T::NTM, PRED>(win, base, wbase, valid, aux, WS(0));
        if constexpr (!PRED) {
#pragma unroll
            for (int j = 0; j < T::IPT; ++j)
                if (wbase + j * 64 >= valid) key[j] = (K)~(K)0;
        }
    }

    // ---- rank inside the wave: lanes with the same digit find each other with 8 ballots, or (ATOMRANK) one
    // returning atomic on the wave's private counter hands every element its rank directly
    uint32_t rank[T::IPT];
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    if constexpr (Cfg::ATOMRANK) {
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t li = wbase + j * 64;
            uint32_t d = digit_of(key[j], aux[T::HAS_W ? j : 0]);
            if constexpr (T::GM_REC) d = (gdig[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            d = li < valid ? d : 255u;
            rank[j] = atomicAdd(&s_whist[wave][d], 1u);
        }
    } else {
#pragma unroll
    for (int j = 0; j < T::IPT; ++j) {
        const uint32_t li = wbase + j * 64;
        // out-of-range slots take digit 255: they have the largest indices of the tile, so they end
        // up behind every real element and are simply not written out.
        uint32_t d = digit_of(key[j], aux[T::HAS_W ? j : 0]);
        if constexpr (T::GM_REC) d = (gdig[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        d = li < valid ? d : 255u;
        uint64_t m = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        const uint32_t below = __popcll(m & lt_mask);
        uint32_t old = 0;
        if (below == 0) {  // lowest lane of the group owns the counter update
            old = s_whist[wave][d];
            s_whist[wave][d] = old + __popcll(m);
        }
        old = __shfl(old, __ffsll((unsigned long long)m) - 1);
        rank[j] = old + below;
    }
    }
    if constexpr (T::DMA_PATH) {
        // the value DMA issued before the ranking has had the whole loop to land
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const VS* wv = reinterpret_cast<const VS*>(s_stage + (size_t)wave * T::WCHUNK * sizeof(K));
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) val[j] = wv[j * 64 + lane];
    }
    __syncthreads();

    // ---- per-digit totals of the tile, exclusive prefix across waves and across digits
    // (threads 0..255 own one digit each; wider workgroups leave the other waves idle here)
    const int d = tid;
    uint32_t cnt = 0, incl = 0;
    uint64_t real = 0;
    const uint64_t tag = (uint64_t)epoch << 56;
    uint64_t* my = status + tile * 256 + (d & 255);
    bool prebased = false;  // (generated passes with counted tile bases: no status words, no look-back)
    uint64_t pre = 0;
    if constexpr (T::GEN) {
        prebased = gen.tile_base != nullptr;
        if (prebased && tid < 256) pre = (uint64_t)gen.tile_base[tile * 256 + (uint64_t)d];
    }
    if (tid < 256) {
#pragma unroll
        for (int w = 0; w < T::NW; ++w) {
            const uint32_t t = s_whist[w][d];
            s_whist[w][d] = cnt;
            cnt += t;
        }
        // real (in-range) count of this digit: padding only ever sits in digit 255
        real = d == 255 ? (uint64_t)cnt - (uint64_t)(T::TILE - valid) : (uint64_t)cnt;
        // publish the aggregate as early as possible: successors can already add it up
        if (!prebased) rs_st_status(my, tag | ((tile == tile0 ? 2ull : 1ull) << 54) | real);
        // exclusive scan of cnt over the 256 digits: wave scan, then across the 4 digit-owning waves
        incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) s_wsum[wave] = incl;
    }
    __syncthreads();
    uint32_t tstart = 0;
    if (tid < 256) {
        uint32_t wpre = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (w < wave) wpre += s_wsum[w];
        tstart = wpre + incl - cnt;
        s_tstart[d] = tstart;
    }

    __syncthreads();

    // ---- place keys in LDS in sorted-by-digit order
#pragma unroll
    for (int j = 0; j < T::IPT; ++j) {
        const uint32_t li = wbase + j * 64;
        uint32_t dd = digit_of(key[j], aux[T::HAS_W ? j : 0]);
        if constexpr (T::GM_REC) dd = (gdig[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        dd = li < valid ? dd : 255u;
        const uint32_t pos = s_tstart[dd] + s_whist[wave][dd] + rank[j];
        rank[j] = pos;
        s_keys[pos] = key[j];
        if constexpr (T::AUX_LDS) s_aux[pos] = aux[j];
        if constexpr (T::GM_REC) s_gen[pos] = (unsigned char)dd;  // (the text codes are dead: their LDS carries the digits to the write-out)
    }
    if constexpr (T::HAS_V && !T::REUSE) {
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t li = wbase + j * 64;
            if constexpr (T::EARLYV) {
                s_vals[rank[j]] = val[j];
            } else {
                if (li < valid) s_vals[rank[j]] = rs_load<T::NTM>(vin + base + li);
            }
        }
    }
    // (the keys now live in LDS: their registers are free during the look-back below)

    // ---- chained scan: look back over the predecessors, then publish the inclusive prefix.
    // A tile becomes ready every pass_time / tiles (~0.1 us at 1 Gi keys) while one agent-scope load
    // costs ~1 us on this part (it has to leave the XCD's L2), so a one-at-a-time walk falls behind and
    // the walk gets ever longer.  LB predecessors are therefore fetched per round trip and consumed
    // nearest-first up to the first inclusive prefix.
    uint64_t excl = 0;
    if (tid < 256 && tile != tile0 && !(Cfg::ABL & 1) && !prebased) {
        constexpr int LB = Cfg::LB;
        int64_t p = (int64_t)tile - 1;
        uint32_t spins = 0;
        bool done = false;
        while (!done) {
            uint64_t sw[LB];
#pragma unroll
            for (int k = 0; k < LB; ++k)
                sw[k] = p - k >= (int64_t)tile0 ? rs_ld_status(status + (uint64_t)(p - k) * 256 + d) : 0ull;
            int used = 0;
            bool open = true;
#pragma unroll
            for (int k = 0; k < LB; ++k) {
                const uint32_t st = (sw[k] >> 56) == (uint64_t)epoch ? ((uint32_t)(sw[k] >> 54) & 3u) : 0u;
                const bool take = open && st != 0;
                excl += take ? (sw[k] & RS_VAL_MASK) : 0ull;
                used += take ? 1 : 0;
                done = done || (take && st == 2);
                open = take && st != 2;
            }
            if ((Cfg::ABL & 8) && d == 0) {  // measurement only: look-back depth / round trips
                atomicAdd(err + 1, (uint32_t)used);
                atomicAdd(err + 2, 1u);
            }
            p -= used;  // the chain's first tile always publishes an inclusive prefix, so p never underflows
            if (used == 0) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (Cfg::GROUP > 0 ? RS_SPIN_LIMIT_GROUPED : RS_SPIN_LIMIT_PLAIN)) {
                    atomicExch(err, 1u);
                    break;
                }
            } else {
                spins = 0;
            }
        }
        rs_st_status(my, tag | (2ull << 54) | (excl + real));
    }
    uint64_t dstart = 0;
    if (tid < 256) {
        if constexpr (T::SEG) dstart = (uint64_t)digit_start[(size_t)sg * seg.start_stride + d];
        else dstart = (uint64_t)digit_start[d];
        s_gbase[d] = (Cfg::ABL & 2) ? base : (prebased ? pre : dstart + excl) - (uint64_t)tstart;
    }
    __syncthreads();
    if constexpr (T::CELL) {
        if (tid < 256) {  // edge record of this tile's run of digit d, 16 bytes: the keys are the 32 bits in LDS
            const uint32_t a = tstart, b = tstart + (uint32_t)real - 1u;
            seg.edges[tile * 256 + d] = seg_cell_edge_pack(real ? s_keys[a] : 0u, real ? s_keys[b] : 0u, dstart + excl, (uint32_t)real);
        }
    } else if constexpr (T::FLAGS) {
        if (tid < 256) {  // edge record of this tile's run of digit d (the sorted keys sit in LDS until the next barrier)
            SegEdge e;
            e.first = e.last = 0;
            e.pos = dstart + excl;
            e.cnt = (uint32_t)real;
            e.pad = 0;
            if (real) {
                const uint64_t lmask = (1ull << seg.low_bits) - 1ull;
                const uint32_t a = tstart, b = tstart + (uint32_t)real - 1u;
                if constexpr (T::KEEPM) {
                    e.first = ktop + (uint64_t)s_keys[a];
                    e.last = ktop + (uint64_t)s_keys[b];
                } else {
                    e.first = ((uint64_t)s_keys[a] << seg.low_bits) | ((uint64_t)s_aux[T::HAS_W ? a : 0] & lmask);
                    e.last = ((uint64_t)s_keys[b] << seg.low_bits) | ((uint64_t)s_aux[T::HAS_W ? b : 0] & lmask);
                }
            }
            seg.edges[tile * 256 + d] = e;
        }
    }

    // ---- coalesced write-out: consecutive lanes -> consecutive slots of one digit run
    if constexpr (!T::REUSE) {
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t i = j * T::NT + tid;
            if (i < valid) {
                const K k = s_keys[i];
                const uint32_t dd = (uint32_t)(k >> shift) & dmask;
                const uint64_t dst = s_gbase[dd] + i;
                if constexpr (T::KEEPM) {
                    // last pass of an MSD-first sort with keys and values staged at once: flags, kept search keys (full key >> 8 and
                    // its low byte) and entries in ONE write-out phase (rs_group_flag, as in the shared-staging branch below)
                    bool head = true, tail = true;
                    if (i > 0) head = s_keys[i - 1] != k;
                    if (i + 1 < valid) tail = s_keys[i + 1] != k;
                    const uint64_t kf = ktop + (uint64_t)k;
                    rs_group_flag<T>(seg, head, tail, kf, dst, 0u);
                    rs_store<T::NTM>(kout + dst, (K)(kf >> 8));
                    if constexpr (T::HAS_W) rs_store<T::NTM>(wout + dst, (W)(kf & 0xFFu));
                    rs_store<T::NTM>(vout + dst, (V)s_vals[i]);
                    continue;
                }
                if (!T::GEN || kout) rs_store<T::NTM>(kout + dst, k);  // generated pass: kout may be null (entries only)
                if constexpr (T::HAS_V) rs_store<T::NTM>(vout + dst, (V)s_vals[i]);
            }
        }
    } else if constexpr (T::CELL) {
        // last pass over cells: flags from the neighbouring keys; digit and aux byte of every element stay packed in registers,
        // four to a word, across the barrier — the entry phase reads neither s_keys nor s_aux again
        uint32_t dig4[T::IPT / 4] = {}, aux4[T::IPT / 4] = {};
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t i = j * T::NT + tid;
            if (i < valid) {
                const uint32_t k = s_keys[i];
                const uint32_t dd = (k >> shift) & dmask;
                const uint32_t a = (uint32_t)s_aux[i];
                dig4[j >> 2] |= dd << (8 * (j & 3));
                aux4[j >> 2] |= a << (8 * (j & 3));
                bool head = true, tail = true;
                if (!(RS_SEG_ABL & 4)) {
                    if (i > 0) head = s_keys[i - 1] != k;
                    if (i + 1 < valid) tail = s_keys[i + 1] != k;
                }
                uint32_t f = head ? 1u : 0u;
                if (!(head && tail) && (k & 1u)) f |= 2u;  // (bit 0 clear: the key ends inside the document)
                f |= ((a >> seg.carry_shift) & seg.carry_mask) << 2;
                if (!(RS_SEG_ABL & 1)) seg.flags[s_gbase[dd] + i] = (uint8_t)f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) s_vals[rank[j]] = val[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t i = j * T::NT + tid;
            if (i < valid && !(RS_SEG_ABL & 2)) {
                const unsigned long long slot = s_gbase[(dig4[j >> 2] >> (8 * (j & 3))) & 0xFFu] + i;
                const uint32_t hi32 = (aux4[j >> 2] >> (8 * (j & 3))) & seg.hi_mask;  // (hi_mask <= 0xFF: the byte's neighbours drop out)
                if (seg.elo) {  // (uniform) 5 bytes per entry instead of 8
                    seg.elo[slot] = (uint32_t)s_vals[i];
                    seg.ehi[slot] = (uint8_t)hi32;
                } else {
                    seg.eout[slot] = ((uint64_t)hi32 << 32) | (uint64_t)s_vals[i];
                }
            }
        }
    } else {
        uint8_t dig[T::IPT];
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t i = j * T::NT + tid;
            dig[j] = 0;
            if (i < valid) {
                const K k = s_keys[i];
                uint32_t dd;
                if constexpr (T::KEEPM) dd = (uint32_t)(k >> shift) & dmask;  // (no auxiliary word: the digit is a key digit)
                else dd = digit_of(k, s_aux[T::HAS_W ? i : 0]);
                if constexpr (T::GM_REC) dd = (uint32_t)s_gen[i];
                dig[j] = (uint8_t)dd;
                if constexpr (T::FLAGS) {
                    // group flags from the neighbours in the sorted tile (equal keys have equal digits, so the ends of
                    // a digit run come out as head / tail: provisional there, settled by rs_seg_edge_fix_kernel)
                    // (32-bit compares)
                    const uint32_t lmask = seg.low_bits >= 32 ? 0xFFFFFFFFu : (1u << seg.low_bits) - 1u;
                    uint32_t ac = 0;
                    if constexpr (!T::KEEPM) ac = (uint32_t)s_aux[T::HAS_W ? i : 0] & lmask;
                    bool head = true, tail = true;
                    bool cmp = true;
                    if constexpr (T::FINAL) cmp = !(RS_SEG_ABL & 4);
                    if constexpr (T::KEEPM) {
                        if (i > 0) head = s_keys[i - 1] != k;
                        if (i + 1 < valid) tail = s_keys[i + 1] != k;
                    } else if (cmp) {
                        if (i > 0) head = s_keys[i - 1] != k || ((uint32_t)s_aux[T::HAS_W ? i - 1 : 0] & lmask) != ac;
                        if (i + 1 < valid) tail = s_keys[i + 1] != k || ((uint32_t)s_aux[T::HAS_W ? i + 1 : 0] & lmask) != ac;
                    }
                    const uint64_t kc = T::KEEPM ? ktop + (uint64_t)k : (((uint64_t)k << seg.low_bits) | (uint64_t)ac);
                    if constexpr (T::FINAL) {
                        const uint32_t carry = (((uint32_t)s_aux[T::HAS_W ? i : 0] >> seg.carry_shift) & seg.carry_mask) << 2;
                        rs_group_flag<T>(seg, head, tail, kc, rs_seg_rotated(si, s_gbase[dd] + i), carry);
                        continue;
                    } else {
                        rs_group_flag<T>(seg, head, tail, kc, s_gbase[dd] + i, 0u);
                    }
                }
                if constexpr (T::KEEPM) {  // kept search keys in the layout of the LSD split sort: full key >> 8, low byte
                    const uint64_t kf = ktop + (uint64_t)k;
                    rs_store<T::NTM>(kout + s_gbase[dd] + i, (K)(kf >> 8));
                    if constexpr (T::HAS_W) rs_store<T::NTM>(wout + s_gbase[dd] + i, (W)(kf & 0xFFu));
                    continue;
                }
                if (!T::GEN || kout) rs_store<T::NTM>(kout + s_gbase[dd] + i, k);
                if constexpr (T::SHRINK) {  // the digit this pass sorted on leaves the record: the cell implies it from here on
                    seg.wout8[s_gbase[dd] + i] = (uint8_t)((uint32_t)s_aux[i] >> 8);
                } else if constexpr (T::HAS_W && !T::W32G) {
                    if (!T::GEN || wout) rs_store<T::NTM>(wout + s_gbase[dd] + i, (W)s_aux[i]);
                }
            }
        }
        __syncthreads();
        if constexpr (T::W32G) {  // the auxiliary words' own phase through the staging buffer
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) s_vals[rank[j]] = (VS)aux[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < T::IPT; ++j) {
                const uint32_t i = j * T::NT + tid;
                if (i < valid) rs_store<T::NTM>(wout + s_gbase[dig[j]] + i, (W)s_vals[i]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) s_vals[rank[j]] = val[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < T::IPT; ++j) {
            const uint32_t i = j * T::NT + tid;
            if constexpr (T::FINAL) {
                if (i < valid && !(RS_SEG_ABL & 2)) {
                    const unsigned long long slot = rs_seg_rotated(si, s_gbase[dig[j]] + i);
                    const uint32_t hi32 = ((uint32_t)s_aux[T::HAS_W ? i : 0] >> seg.hi_shift) & seg.hi_mask;
                    if (seg.elo) {  // (uniform) 5 bytes per entry instead of 8
                        seg.elo[slot] = (uint32_t)s_vals[i];
                        seg.ehi[slot] = (uint8_t)hi32;
                    } else {
                        seg.eout[slot] = ((uint64_t)hi32 << 32) | (uint64_t)s_vals[i];
                    }
                }
            } else {
                if constexpr (T::GEN && sizeof(VS) == 8) {
                    if (gen.vout_hi) {  // (uniform) entries-only partition of 8-byte entries below 2^40: written packed (Sa40)
                        if (i < valid) {
                            const uint64_t dst = s_gbase[dig[j]] + i;
                            const uint64_t e = (uint64_t)s_vals[i];
                            reinterpret_cast<uint32_t*>(vout)[dst] = (uint32_t)e;
                            gen.vout_hi[dst] = (uint8_t)(e >> 32);
                        }
                        continue;
                    }
                }
                if (i < valid) rs_store<T::NTM>(vout + s_gbase[dig[j]] + i, (V)s_vals[i]);
            }
        }
    }
}

}  // namespace cdb
