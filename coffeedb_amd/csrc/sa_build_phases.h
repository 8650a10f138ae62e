// sa_build_phases.h — what the phases of the suffix-array build hand to each other (sa_build.hip: build_typed), and the phase
// functions that live in a file of their own.  No kernel and no launch lives here.
//   sa_initial_direct.hip   initial_sort_direct, the group-flag kernels (write_group_flags*), the shared sorts of 4-byte entries
//   sa_sorts.hip            the shared sorts of 8-byte entries
//   sa_refine.hip           refine_groups: the refinement rounds and their kernels
//   sa_reference_order.hip  finish_reference_order: the walk into the reference's order (apply_reference_order*)
//   sa_build.hip            the prologue (alphabet, key width, digit histograms, generate_keys), the bucket-wise initial sort
//                           and the driver (build_typed, build_suffix_array)
#pragma once
#include <vector>

#include "index_impl.h"
#include "scan.h"

namespace cdb {

double now_ms();

// ---- 1. alphabet -> order-preserving dense codes
struct Alphabet {
    DevBuf d_counts, d_symmap;
    // bucket-wise builds with look-back-free generated passes count the bytes per 8 Ki-position tile (the rows become the tile
    // bases of the records / partition pass, radix_sort.h: TextGen::tile_base); their column sums are the histogram
    DevBuf d_tbc;
    uint32_t tiles8 = 0;
    bool tile_bytes = false;
    DevBuf d_pair_hi;      // per byte value: positions whose next byte is >= 0x80 (counted beside the bytes, PAIR form)
    bool pair_hi_counted = false;
    uint64_t h_counts[256];
    uint16_t h_map[256];
    int sigma = 0, symbits = 1;
    bool high_bytes = false;
};

// per-tile top-digit counts of the MSD-first sort's look-back-free generated pass (option gen_prebased)
struct TopCounts {
    DevBuf d_tc;
    const unsigned long long* totals = nullptr;  // their column sums: the top-digit histogram
    bool counted = false;
    struct AuxJoin {  // (declared after the buffer: an exception on the way still waits for the second stream before the
        hipStream_t a = nullptr;  //  buffer goes back to the pool)
        ~AuxJoin() { if (a) (void)hipStreamSynchronize(a); }
    } aux_join;
};

// key width and coding of the initial sort (plan_keys)
struct KeyPlan {
    int nsym = 0, dbits = 8, key_bits = 0;
    uint32_t kbase = 0;
    uint64_t kmagic = 0;
    bool dense = false;
    double est_k0 = 0;  // the sample's measured pair-collision probability at est_k0n symbols (>= 50 colliding pairs: meaningful)
    int est_k0n = 0;
};

// the digit histograms of the fused key generation, and the top-digit histogram of the MSD-first sort
struct DigitHist {
    bool fused = false, use_msd = false;
    std::vector<uint64_t> h_hist;  // [nsym][256] digit histograms of the LSD passes (fused path)
    std::vector<uint64_t> h_top;
    // pair form: 6-symbol keys whose top digit is a function of the first two symbols (TextGen::msd_pair); otherwise the
    // top digit is key >> 32, counted by the key sweep
    unsigned long long msd_m = 1ull << 32;
    uint32_t msd_span = 0;
    struct { uint32_t pair_span = 0, pair_r = 0, pair_s = 0; } pair_consts;
};

// a bucket of the reference-order walk: the array slots [lo, hi) (sa_reference_order.hip: apply_reference_order)
struct CompatBucket {
    unsigned long long lo, hi;
};

// bucket-wise build in the reference's order, one level below a root bucket (sa_build.hip: fold_root_buckets): how many of the
// bucket's suffixes end behind their first symbol or go on with a byte below / from 0x80
struct Depth1Fold {
    uint64_t nend = 0, nlow = 0, nhigh = 0;
    bool fold = false, done = false;  // done: the segmented sort really wrote the bucket with its blocks swapped
};

// what the initial sort hands to the refinement and the finish
struct InitialSort {
    DevBuf sa_buf, flags;
    DevBuf sa_hi_buf;         // packed output (index_impl.h: Sa40): bits 32..39 of every entry; sa_buf then holds the low words
    bool packed_out = false;
    bool flags_by_sort = false;    // the sort's last pass wrote the group flags and the tile sums of the first compaction
    bool tile_sums_ready = false;  // the raw tile sums of the first compaction are in scan_partials already
    DevBuf sorted_keys, sorted_k32, sorted_low;
    int low_bits = 0, low_bytes = 0;
    std::vector<Depth1Fold> depth1;          // ... per bucket: how its suffixes split by the class of their second symbol
    std::vector<CompatBucket> folded_roots;  // bucket-wise build in the reference's root order: the first-symbol buckets
    uint64_t refine_depth0 = 0;  // symbols every key of the initial sort covers for certain (0: nsym; variable-length keys: fewer)
    DevBuf d_vl_bytelen;         // variable-length keys: text byte -> code-word length (the refinement recovers every group's exact depth)
    uint32_t vl_kb1 = 0;
    uint32_t carry = 0;          // carried bits: the next `carry` code-stream bits behind the key sit in bits 2.. of every flag byte
};

// the buffers of the refinement rounds: build_typed owns them, so that they live until the build ends (the reference-order
// finish sizes its second array against the memory left)
struct RefineBuffers {
    DevBuf d_order;
    DevBuf U, skey[2], sval[2], nh, rank, hcov;
    DevBuf d_open;  // entries still unresolved after the last round (saves a full flag scan to learn "none")
    DevBuf U2b, lf;       // list-based rounds: the other list of positions, the flag bytes of the current list in list order
    DevBuf d_gs_state;  // sa_group_sort_kernel: [0] it gave up (groups too long for it), [1] members walked by its long walks
    DevBuf d_inplace;   // sa_carried_inplace_kernel: its count words (open entries met, entries moved)
};

// ---- the phases that cross a file.  V = entry type, I = type of suffix-array slot numbers, R = type of ranks / extended text
// positions; each is explicitly instantiated in its own file, for the forms build_typed uses.
// (the unfused direct sort: every suffix's 64-bit key and entry, in text order — sa_build.hip: sa_keygen_kernel)
template <typename V>
void generate_keys(Index& ix, const Alphabet& al, const KeyPlan& kp, uint64_t* keys, V* vals);
template <typename V>
InitialSort initial_sort_direct(Index& ix, const Alphabet& al, const KeyPlan& kp, const DigitHist& dh, TopCounts& tc, SortStats& ss);
// sa_refine.hip (SAW = how the array is stored: SaRW<V>, or Sa40RW for packed 8-byte entries); returns the depth every suffix
// is sorted to
template <typename V, typename I, typename R, typename SAW>
uint64_t refine_groups(Index& ix, SAW sa, InitialSort& is, const Alphabet& al, const KeyPlan& kp, SortStats& ss, RefineBuffers& rb);
// sa_reference_order.hip: the array goes to the index
template <typename V>
void finish_reference_order(Index& ix, InitialSort& is, Alphabet& al);

// group flags of n sorted keys (sa_initial_direct.hip: sa_initflags_kernel / sa_initflags32_kernel) — the direct sort and the
// bucket-wise build's per-bucket sorts both end in them
void write_group_flags(hipStream_t s, const uint64_t* keys, uint64_t n, uint32_t kbase, uint64_t kmagic, uint8_t* flags, bool flags_aligned);
template <typename W>
void write_group_flags32(hipStream_t s, const uint32_t* k32, const W* low, int low_bits, uint64_t n, uint32_t kbase, uint64_t kmagic,
                         uint8_t* flags, bool flags_aligned, U2* tile_sums = nullptr);

// ---- the sorts more than one phase calls: every kernel configuration of each lives in ONE object — 4-byte entries in
// sa_initial_direct.hip, 8-byte entries in sa_sorts.hip
#define CDB_SA_SORT_ARGS(K, V) \
    hipStream_t, RadixWorkspace&, Profiler&, K*, K*, V*, V*, uint64_t, int, int, SortStats*, int, int, const uint64_t*, const TextGen*, const unsigned long long*
#define CDB_SA_SPLIT_ARGS(V, W)                                                                                                          \
    hipStream_t, RadixWorkspace&, Profiler&, uint32_t*, uint32_t*, V*, V*, W*, W*, uint64_t, int, SortStats*, int, int, const uint64_t*, \
        const TextGen*, int, const unsigned long long*, int, const SegFinalKeepArgs*
extern template int radix_sort<uint64_t, uint32_t>(CDB_SA_SORT_ARGS(uint64_t, uint32_t));
extern template int radix_sort<uint64_t, uint64_t>(CDB_SA_SORT_ARGS(uint64_t, uint64_t));
extern template int radix_sort<uint32_t, uint32_t>(CDB_SA_SORT_ARGS(uint32_t, uint32_t));
extern template int radix_sort<uint32_t, uint64_t>(CDB_SA_SORT_ARGS(uint32_t, uint64_t));
extern template int radix_sort_split<uint32_t, uint8_t>(CDB_SA_SPLIT_ARGS(uint32_t, uint8_t));
extern template int radix_sort_split<uint32_t, uint16_t>(CDB_SA_SPLIT_ARGS(uint32_t, uint16_t));
extern template int radix_sort_split<uint64_t, uint8_t>(CDB_SA_SPLIT_ARGS(uint64_t, uint8_t));
extern template int radix_sort_split<uint64_t, uint16_t>(CDB_SA_SPLIT_ARGS(uint64_t, uint16_t));

}  // namespace cdb
