// index_impl.h — state of one GPU string index (the object behind the opaque cdb_index handle).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "common.h"
#include "radix_sort.h"

namespace cdb {

constexpr int TEXT_PAD = 128;  // readable zero bytes behind library-owned text

struct BuildStats {
    double build_ms = 0, alloc_ms = 0, free_ms = 0;
    int rounds = 0;              // refinement rounds after the initial key sort
    int ext_rounds = 0;          // ... of which text-extension rounds
    int dbl_rounds = 0;          // ... of which prefix-doubling rounds
    uint64_t unresolved_initial = 0;
    uint64_t unresolved_max = 0;
    int sort_passes = 0;         // onesweep launches
    int sort_passes_skipped = 0;
    int isa_built = 0;
    int fused_keygen = 0;
    int key_layout = 0;          // sort records: 0 = (u64 key, entry), 1 = (u32 key, entry), 2 / 3 = (u32 key, entry, u8 / u16 low digits)
    int dense_keys = 0;          // initial keys in base (alphabet + 1) instead of bit-aligned symbols
    int bucketed = 0;            // streamed bucket-wise initial sort (corpora >= 2^32)
    int bucket_low_digits = 0;   // ... low digits (bytes) carried beside the 32-bit bucket key
    int bucket_groups = 0;       // ... bucket groups whose records were gathered in one text-ordered sweep
    int root_folded = 0;         // ... first-symbol buckets laid out in the reference's root order (bytes >= 0x80 first)
    int flags_in_last_pass = 0;  // single sort: group flags written by the last radix pass (no flag kernel)
    int msd_first = 0;           // single sort: top digit first, then (u32, u32) records sorted bucket by bucket (radix_sort_msd)
    int gen_prebased = 0;        // ... generated pass without look-back (counted tile bases)
    int fused_records = 0;       // ... bucket records written by the generated pass itself (one bucket group): no partition + gather
    int sweep_records = 0;       // ... bucket records of every bucket group written by a sweep over the text (records_sweep.h): no partition + gather
    int pairclass_fused = 0;     // reference order, one level below the root: next-byte classes counted beside the bytes (no second sweep over the text)
    int list_rounds = 0;         // refinement rounds compacted from the previous round's list instead of the whole flag array
    int group_sorts = 0, group_sort_fallbacks = 0;  // refinement rounds sorted inside their groups in one pass / sent to the general sort
    int carried_key_bits = 0;    // code-stream bits behind the key that ride in the records' spare aux bits and the flag bytes (0 = none)
    int carried_rounds = 0;      // refinement rounds sorted on those bits (no text read); counted in none of the round statistics above
    uint64_t unresolved_after_carried = 0;  // entries still open behind that round (= unresolved_initial where none ran)
    int carried_inplace = 0;     // the carried round's in-place sweep ran (carried_inplace.h): 0 / 1
    uint64_t unresolved_after_inplace = 0;  // entries still open behind that sweep, in front of the carried list round (= unresolved_initial where it did not run)
    int top_first = 0;           // segmented sort: top key digit first, then 9-byte records inside (bucket, top byte) cells (0 / 1)
    uint64_t top_first_cells = 0;  // ... non-empty cells of all bucket groups
    int partial_levels = 0;      // ... leftover key bits hold the next symbol quantised to this many levels (sweep form; 0 / 1 = none)
    int vl_key_bits = 0;         // ... keys = the first vl_key_bits - 1 bits of the alphabetic code stream + a "continues" bit (vl_code.h); 0 = dense keys
    double vl_avg_len = 0, vl_rate = 0, vl_est_unresolved = 0, fixed_est_unresolved = 0;
    int segmented = 0;           // ... sorted by segmented passes: one launch per pass for all buckets of a group
    uint64_t gather_items = 0;
    int key_symbols = 0, symbol_bits = 0, alphabet = 0, digit_bits = 8;
    uint64_t final_depth = 0;    // symbols compared when the last group was resolved
    uint64_t compat_rotations = 0, compat_depth = 0;  // reference_compat pass (bytes >= 0x80)
};

struct QueryStats {
    double query_ms = 0;
    double upload_ms = 0, device_ms = 0, download_ms = 0;  // host batches: patterns in, search + rows, results out
    uint64_t nhits = 0, nrows = 0;
    // which row builder answered the batched queries of this handle (query.hip: query_typed), counted since the handle was
    // created — builds, loads and proof repairs leave them alone.  spec + wave + sort + empty - spec_spills == batches.
    uint64_t batches = 0;
    uint64_t spec_batches = 0, spec_spills = 0;  // speculation attempted / attempted and redone the ordinary way
    uint64_t wave_batches = 0;                   // one wavefront per pattern with the totals known
    uint64_t sort_batches = 0, sort_chunks = 0;  // expand + radix sort + runs, and the chunks it was cut into
    uint64_t empty_batches = 0;                  // nothing to look up (no pattern, no text) or no hit at all
};

// ---- the kept search keys as kernels see them, slot for slot beside the array, in whichever form a handle holds them (d_keys, or
// d_keys32 = key >> low_bits with the low digits in one or two bytes of d_keylow; a form that is absent is a null pointer; a handle
// without keys gives the empty view: keys_of below)
struct KeptKeys {
    uint64_t* k64 = nullptr;
    uint32_t* k32 = nullptr;
    uint8_t* low = nullptr;
    int low_bits = 0, low_bytes = 0;
    __host__ __device__ __forceinline__ bool present() const { return k64 != nullptr || k32 != nullptr; }
    __device__ __forceinline__ uint64_t low_at(uint64_t i) const {
        return low_bytes == 2 ? (uint64_t)reinterpret_cast<const uint16_t*>(low)[i] : (uint64_t)low[i];
    }
    __device__ __forceinline__ uint64_t at(uint64_t i) const {
        if (k64) return k64[i];
        const uint64_t h = k32[i];
        if (!low_bits) return h;
        return (h << low_bits) | low_at(i);
    }
    // slot i against the key range [klo, khi]: -1 its key lies below, +1 above, 0 inside (the suffix starts with the symbols the
    // range was coded from: query.hip, key_range).  Split keys: the 32-bit part alone decides unless it equals the truncated range
    // end it is compared with, and the low digits are fetched only then.  (The lone-keyword kernels fetch them beside the high
    // part and keep their own compare: query.hip, q_single_answer.)
    __device__ __forceinline__ int cmp_range(uint64_t i, uint64_t klo, uint64_t khi) const {
        uint64_t key;
        if (k64) {
            key = k64[i];
        } else {
            const uint64_t h = k32[i];
            if (low) {
                const uint64_t a = klo >> low_bits, b = khi >> low_bits;
                if (h < a) return -1;
                if (h > b) return 1;
                if (h > a && h < b) return 0;
                key = (h << low_bits) | low_at(i);
            } else {
                key = h;
            }
        }
        return key < klo ? -1 : (key > khi ? 1 : 0);
    }
    __device__ __forceinline__ void put(uint64_t i, uint64_t key) const {
        if (k64) k64[i] = key;
        if (k32) k32[i] = (uint32_t)(key >> low_bits);
        if (low) {
            const uint64_t l = key & ((1ull << low_bits) - 1ull);
            if (low_bytes == 2) reinterpret_cast<uint16_t*>(low)[i] = (uint16_t)l;
            else low[i] = (uint8_t)l;
        }
    }
    // slot `from` of src into slot `to`, every stored form as it is (src holds the same forms)
    __device__ __forceinline__ void copy(const KeptKeys& src, uint64_t from, uint64_t to) const {
        if (k64) k64[to] = src.k64[from];
        if (k32) k32[to] = src.k32[from];
        if (low) {
            if (low_bytes == 2) reinterpret_cast<uint16_t*>(low)[to] = reinterpret_cast<const uint16_t*>(src.low)[from];
            else low[to] = src.low[from];
        }
    }
    uint64_t bytes_per_slot() const { return (k64 ? 8 : 0) + (k32 ? 4 : 0) + (low ? low_bytes : 0); }
};
// the kept keys for the lone-keyword kernels (query.hip): suffixes starting with the keyword's first min(m, nsym) symbols are exactly
// those with key in [klo, khi] (coded on the host); decisive = the keyword has at most nsym symbols.  nsym = 0: no keys, the text
// decides every probe
struct SingleKeys {
    KeptKeys keys;
    int nsym = 0;
    bool decisive = false;
    uint64_t klo = 0, khi = 0;
    // slots the lower bound can lie in, from the host-side key directory (query.hip: query_keydir_ensure): every slot in
    // front of lo0 holds a key below klo, slot hi0 (if it exists) a key above khi
    bool ranged = false;
    uint64_t lo0 = 0, hi0 = 0;
};

// ---- suffix-array storage as the kernels see it ------------------------------------------------------------------------
// Plain: an array of V (u32 / u64 — the reference's own widths, index.cpp:203-208).  Packed: 8-byte entries whose bits all lie
// below 2^40 (document bits + offset bits <= 40: every >= 2^32 configuration of BASELINE.json) are STORED as u32 low words +
// u8 high bytes — 5 instead of 8 bytes per suffix; cdb_sa_copy / cdb_save expand them to the reference's u64 encoding, so
// nothing outside the library sees the difference.  Kernels are templated on a tag T (uint32_t, uint64_t, Packed40);
// SaOf<T>::ptr is what they index, SaOf<T>::val the entry type they compute with.
struct Sa40 {
    const uint32_t* __restrict__ lo;
    const uint8_t* __restrict__ hi;
    __device__ __forceinline__ uint64_t operator[](uint64_t i) const { return (uint64_t)lo[i] | ((uint64_t)hi[i] << 32); }
};
struct Packed40 {};
template <typename T> struct SaOf {
    using val = T;
    using ptr = const T* __restrict__;
};
template <> struct SaOf<Packed40> {
    using val = uint64_t;
    using ptr = Sa40;
};
// ... and as the build's refinement writes it
template <typename V> struct SaRW {
    V* p;
    using val = V;
    __device__ __forceinline__ V load(uint64_t i) const { return p[i]; }
    __device__ __forceinline__ void store(uint64_t i, V v) const { p[i] = v; }
};
struct Sa40RW {
    uint32_t* lo;
    uint8_t* hi;
    using val = uint64_t;
    __device__ __forceinline__ uint64_t load(uint64_t i) const { return (uint64_t)lo[i] | ((uint64_t)hi[i] << 32); }
    __device__ __forceinline__ void store(uint64_t i, uint64_t v) const {
        lo[i] = (uint32_t)v;
        hi[i] = (uint8_t)(v >> 32);
    }
};

struct Index {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;  // serialises device work of one index (queries from several host threads)
    // coalescing of concurrent single-keyword queries (capi_query.hip: cdb_query)
    std::mutex qmu;
    std::condition_variable qcv;
    std::vector<void*> qpending;
    bool qleader = false;
    bool coalesce_queries = true;
    bool keep_keys = true;        // keep d_keys when it costs <= 16 GiB (8 bytes per suffix)
    bool use_wave_rows = true;    // wavefront-per-pattern row building when every hit list has <= 64 entries
    bool use_single_query = true; // a lone cdb_query is answered by one wavefront in one launch (query.hip)
    void* h_single = nullptr;     // host-mapped result block of that kernel (+ its device address)
    void* d_single = nullptr;
    // resident_query: one workgroup stays on the device and answers lone keywords from a host-mapped mailbox (query.hip)
    // resident_mode (option resident_query): 0 = never, 1 = always, 2 = automatic (default) — a caller that sends lone keywords back
    // to back (interface.cpp:79-113 loops over a query's keywords; RESIDENT_AUTO_STREAK calls less than RESIDENT_AUTO_GAP_US apart)
    // gets the resident workgroup without asking for it; it idles out by itself ~3 ms after the last keyword.  resident_query is
    // what the call in progress uses (decided in query_single_launch under ix.mu).
    int resident_mode = 2;
    bool resident_query = false;
    uint32_t single_streak = 0;
    int64_t last_single_ns = 0;
    uint64_t res_answers = 0, launched_answers = 0;  // lone keywords answered by the resident workgroup / by a launched kernel (stats)
    void* h_res = nullptr;        // the mailbox (+ its device address)
    void* d_res = nullptr;
    hipStream_t res_stream = nullptr;
    // second stream of the build (sa_build.hip): the pair count of the MSD-first sort runs beside the key-width sample
    hipStream_t aux_stream = nullptr;
    hipEvent_t aux_ev[2] = {nullptr, nullptr};
    bool overlap_paircount = true;  // option: 0 = the pair count waits for the sample (one stream)
    bool res_running = false;
    uint32_t res_seq = 0;         // requests posted so far
    SingleKeys res_keys;          // the key arrays the running workgroup was started with
    bool use_fast_search = true;  // pivot-table / galloping search on sorted arrays (query.hip)

    // ---- host staging (cdb_add)
    std::vector<int64_t> ids;
    std::vector<uint64_t> doc_start{0};
    std::string host_text;
    bool host_tables_valid = true;  // false after cdb_build_resident until ids / doc_start are fetched back
    bool host_text_valid = true;    // false while the column lives on the device only (after cdb_build frees its staging
                                    // copy, cdb_load, device builds): cdb_add* fetch it back first (capi.hip)

    // ---- reference-visible parameters (src/index.h:56-57)
    uint64_t bits = 1, mask = 1, size = 0;
    int off_bits = 1;  // bits of the largest document length (the offset field really in use)
    int width = 0;  // 4 / 8, 0 = never built
    uint64_t ndocs = 0;

    // ---- device state
    DevBuf d_text_owned;
    const uint8_t* d_text = nullptr;  // n bytes (+TEXT_PAD when owned)
    bool text_padded = false;
    DevBuf d_doc_start;               // ndocs + 1 u64
    DevBuf d_ids;                     // ndocs i64
    DevBuf d_sa;                      // size * width bytes — or, packed, the entries' low words (size * 4 bytes)
    DevBuf d_sa_hi;                   // packed: bits 32..39 of every entry (size bytes)
    bool sa_packed = false;           // 5-byte storage of 8-byte entries (Sa40 above)
    bool gen_prebased = true;         // option: generated passes take their tile bases from counted per-tile digits (no look-back, two
                                      // 8 Ki-key workgroups per CU; radix_sort.h: TextGen::tile_base).  Bucket-wise builds only: the
                                      // MSD-first sort below 2^32 always counts its top digits per tile
    TileBaseWorkspace tbw;
    bool key_cost_model = true;       // option: bucket-wise builds weigh one key symbol fewer (a pass saved) against the refinement it costs
    bool pack_sa = true;              // option: builds with 8-byte entries below 2^40 store them packed
    void release_sa() {
        d_sa.release();
        d_sa_hi.release();
        sa_packed = false;
        clu.drop();  // (the class table of cdb_cluster describes the array that just went)
        idt.drop();  // (... and the id table goes with it: every build and load passes here, so it never outlives d_ids)
    }
    template <typename T> typename SaOf<T>::ptr sa_view() const;  // (below)
    bool sa_sorted = false;           // SA is globally sorted in unsigned byte order (false only for
                                      // reference_compat orderings of text with bytes >= 0x80)
    DevBuf d_keys;                    // optional: the sorted initial keys (first key_nsym symbol codes of every
                                      // suffix, packed) kept for the search: one load decides most probes
    DevBuf d_symmap_q;                // byte -> symbol code (u16[256]) matching d_keys
    uint16_t h_symmap_q[256] = {};    // ... and its host copy (the lone-keyword path codes its keyword on the host)
    DevBuf d_keys32, d_keylow;        // ... or, after a narrow / split sort, key >> key_low_bits as u32 and (split) the
    int key_low_bits = 0;             // low digit(s) in one or two bytes per suffix: 5-6 instead of 8 bytes per suffix
    int key_low_bytes = 0;
    int key_nsym = 0;
    uint32_t key_base = 0;            // key = the first key_nsym symbol codes as a number in this base
    void drop_keys() {
        d_keys.release();
        d_keys32.release();
        d_keylow.release();
        key_nsym = 0;
        key_low_bits = 0;
        key_low_bytes = 0;
        h_keydir.clear();
        h_keydir.shrink_to_fit();
        keydir_tried = false;
    }
    // Host-side key directory of the lone-keyword path: h_keydir[c] = first slot whose kept key is >= c << keydir_shift
    // (2^keydir_bits + 1 entries), built once per index at its first lone keyword.  The 64-ary search then starts from the
    // few dozen slots between two directory entries instead of the whole array: 1-2 rounds of dependent loads instead of 5-6.
    std::vector<uint32_t> h_keydir;
    int keydir_shift = 0, keydir_bits = 0;
    bool keydir_tried = false;
    bool key_directory = true;  // option: 0 = every lone keyword searches the whole array
    DevBuf d_pivots;                  // top levels of the lower-bound search tree (query.hip), built lazily
    int pivot_levels = 0;

    // ---- scratch kept across calls
    RadixWorkspace rws;
    MsdWorkspace msd_ws;  // segments / per-bucket digit tables of the MSD-first initial sort
    DevBuf scan_partials;
    uint64_t q_spec_cap = 0;  // > 0: hits the next batch's buffers are sized for without asking (query.hip)
    DevBuf q_spec;
    DevBuf q_pat, q_offs, q_left, q_right, q_hoff, q_keys0, q_keys1, q_flags, q_rowptr, q_ids, q_counts, q_hitptr, q_hitoff;

    // ---- options
    bool reference_compat = true;   // bit-parity with the reference also for bytes >= 0x80
    bool force_doubling = false;
    int initial_passes = 0;
    int key_symbols = 0;       // test hook: symbols in the initial sort key (0 = chosen from the text)
    int sort_variant = 0;
    int search_lanes = 0;      // lanes per keyword in the fast batched search: 0 = by batch size, 1 or 8
    bool flags_in_last_pass = true;  // builds below 2^32: the last radix pass writes the group flags (0 = the flag kernel)
    bool fold_depth1 = true;     // ... and (segmented sort) the two byte blocks of big first-symbol buckets swapped by the last pass
    bool fold_root = true;       // bucket-wise build under reference_compat: bucket order = the reference's root child order
    bool segmented_sort = true;  // bucket-wise build: one launch per radix pass for all buckets of a group, entries and flags
                                 // written by the last pass (0 = one sort per bucket + assemble + flag kernels: round 2)
    bool fuse_records = true;  // bucket-wise build with ONE bucket group: the generated pass writes the records (0 = partition + gather)
    bool fuse_pairclass = true; // bucket-wise build of text with bytes >= 0x80: next-byte classes counted by the tile byte count (0 = separate sweep)
    int carried_inplace = -1;   // the carried round's in-place sweep in front of its list round: -1 = from CARRIED_INPLACE_MIN_N suffixes upward, 0 = off, 1 = on
    int top_digit_first = -1;   // segmented sort of 40-bit variable-length keys: top key byte first, the other passes per (bucket, top byte) cell
                                // over 9-byte records (run_segmented): -1 = from TOP_FIRST_MIN_N suffixes upward, 0 = off, 1 = on where it applies
    int carried_bits = -1;      // code-stream bits carried behind variable-length keys (sa_refine.hip: carried round): -1 = as many as fit, 0 = none, 1..6 = at most
    bool list_rounds = true;    // text-extension rounds behind the first compact from the previous round's list (0 = from the flag array)
    int group_sort_cap = 4096;  // ... members of a group on one side of an entry beyond which the pass gives up (its work is also bounded, sa_refine.hip)
    bool group_sort = true;     // refinement rounds: one pass inside the groups instead of the general sort (0 = always the general sort)
    bool partial_symbol = true; // bucket-wise build, dense keys in the sweep form: leftover key bits hold the next symbol, quantised (0 = off)
    int vl_keys = 2;           // bucket-wise build, variable-length keys (vl_code.h): 0 off, 2 when the cost model says so, 1 always, 16..56 always with that many key bits
    bool vl_off_once = false;  // (this build only: the sweep form turned out not to apply — dense keys after all)
    bool sweep_records = true; // bucket-wise build with several bucket groups: one sweep over the text per group writes its records (0 = partition + gather)
    bool pack_entries = true;  // bucket-wise build: 8-byte entries below 2^40 travel through the bucket sorts as u32 + u8
    bool msd_first = true;    // keys of 33..40 bits below 2^32 suffixes: top digit first, then every bucket on its own with
                              // (u32, u32) records (radix_sort_msd); 0 = LSD split sort with the low digit as a travelling byte
    bool msd_pair = true;     // ... 6-symbol keys: top digit from the first two symbols (pair count of the text, 32-bit part arithmetic)
    bool keyhist3 = true;     // 24-bit part arithmetic in the key-histogram sweep when the key has 3 P symbols (0 = rolling 64-bit keys)
    int dense_key_retries = 0;  // builds redone with dense keys after the sweep-only key form did not apply (sa_build.hip: RetryWithDenseKeys)
    int group_fallbacks = 0;  // builds redone in plain ticket order after a starved XCD-ordered pass (sa_build.hip)
    uint64_t bucket_group_limit = 0;  // test hook: cap on suffixes per bucket group (0 = what memory allows)
    uint64_t self_check_pairs = 0;    // adjacent pairs the last build's check compared (size - 1 with self_check = 2)
    double self_check_ms = 0;
    // 0 off; 1 a sample of random adjacent pairs behind every build (verify.hip): a failure makes the build fall back to the ballot
    // ranking once, then fail; 2 EVERY adjacent pair before the build returns (a proof, 1.2-1.5 x the build); 3 (default) the sample
    // before the build returns + the proof AFTER it, off the caller's path (verify.hip: proof_start)
    int self_check = 3;
    int self_check_fallbacks = 0;
    bool debug_fail_self_check = false;  // test hook: the first spot check of a build reports a failure
    // ---- proof after publish (self_check = 3).  The reference's array is sorted by construction (std::sort leaves, index.cpp:86-95);
    // here the order rests on an observed LDS lane order (radix_pass.h: hardware mapping, RsCfg::ATOMRANK) and a sample proves nothing about one stray pair.  So
    // the build publishes as before and a helper thread then compares EVERY adjacent pair against the text on a low-priority stream
    // of its own, slice by slice, beside the queries (it reads arrays that nothing changes until proof_stop).  Damage found: the
    // thread takes ix.mu (queries wait: a wrong array is not served while it is being replaced), switches the device to the ballot
    // ranking, rebuilds with the full check inline and counts self_check_fallbacks.  Every path that replaces or frees the arrays
    // (reset_unbuilt, build_suffix_array, cdb_destroy) calls proof_stop first; it may be called with ix.mu held.
    struct Proof {
        std::thread th;
        std::atomic<int> state{0};       // 0 none, 1 running, 2 proved, 3 damage found and repaired, 4 repair failed, 5 cancelled, 6 could not run
        std::atomic<bool> cancel{false};
        hipStream_t stream = nullptr;    // lowest priority
        void* d_out = nullptr;           // 2 x u64 on the device
        double ms = 0, repair_ms = 0;    // wall time of the sweep / of the repair
        uint64_t pairs = 0;              // adjacent pairs compared
        uint64_t found[2] = {0, 0};      // pairs out of order, invalid entries
        uint64_t skipped = 0;            // pairs left unjudged (0: mixed pairs are judged in place; kept as a stat)
        uint64_t mixed = 0;              // pairs whose first differing bytes lie on both sides of 0x80, judged by the size of their bucket
        uint64_t runs = 0;
        bool of_loaded_file = false;     // the array came from cdb_load: damage says nothing about this device's ranking
        std::atomic<bool> busy{false};   // the helper thread is at work (pre-mapping and / or proof)
        bool want_proof = false;         // (this run of the thread: self_check >= 3)
        double premap_ms = 0;
        uint64_t premap_bytes = 0;       // device memory the helper mapped for the next generation (DevPool::premap)
    } proof;
    // option (default off): behind every build the helper thread maps, into the block cache, the blocks a REBUILD beside this index
    // will ask for and not find (the arrays this index keeps) — database.cpp:276-280 builds the next generation while this one
    // serves.  Off by default: hipMalloc of tens of GB holds a driver lock that kernel launches wait for — the lone keywords of the
    // first half second after a 4 GiB build took 496 instead of 21 ms.  cdb_reserve maps the second generation BEFORE the process
    // serves anything (start-up: server.cpp:43-44), which is where that time belongs.
    bool premap_generation = false;
    bool proof_in_repair = false;        // (build_suffix_array called BY the proof thread: no stop / start of itself)
    uint64_t debug_damage_after_build = 0;  // test hook: swap entries k, k + 1 behind the build's own check (once)
    bool debug_no_segcap = false;   // test hook: the bucket-wise build takes its per-bucket fallback ("a bucket does not fit the record memory")
    int debug_starve_group = 0;     // test hook: a build in XCD-aware tile order reports a look-back timeout once
    bool debug_fail_build = false;  // test hook: the build throws after its sorts (exercises the failure paths)
    bool debug_fail_prepare = false;  // test hook: the prepare half of a removal throws behind its device work (index and column alike)
    bool debug_fail_append_prepare = false;  // test hook: ... of an append (append_prepare, column_append_prepare)
    bool force_big_path = false;  // test hook: use the >= 2^32 code path (u64 ranks, bucket-wise sort) at any size
    bool fuse_keygen = true;  // first radix pass computes keys from the text (no key/entry materialisation)
    int digit_bits = 0;
    bool narrow_keys = true;      // 32-bit sort keys (+ a byte for the dropped low digit) when the key width allows
    int key_coding = 0;           // initial sort keys: 0 = dense when that saves a pass, 1 = bit-aligned symbols, 2 = dense
    uint64_t query_hit_budget = 1ull << 31;  // hits resolved per chunk of a batch (16 B of scratch each)

    // ---- cluster tables (cluster.hip): built under ix.mu at the first cdb_cluster on a built array, dropped where the array goes
    // (release_sa above: reset_unbuilt, every build, and the order proof's repair of a damaged array — a table made from an array the
    // proof later judges wrong must not outlive it).  4 * ndocs + 4 * nclasses bytes, plus the id table below.
    struct ClusterTables {
        bool valid = false;
        uint64_t nclasses = 0;     // distinct documents (the empty document included when there is one)
        bool resorted = false;     // classes were put into std::string order on the host (array in the reference's order)
        DevBuf class_of_doc;       // u32[ndocs]
        DevBuf class_rep;          // u32[nclasses]: one document of every class
        double prepare_ms = 0, last_ms = 0;
        uint64_t bytes() const { return class_of_doc.bytes + class_rep.bytes; }
        void drop() {
            valid = false;
            nclasses = 0;
            class_of_doc.release();
            class_rep.release();
        }
    } clu;
    // ---- id -> document (cluster.hip: id_table_prepare; read by cdb_cluster and cdb_render_rows): the ids are insertion timestamps
    // and usually ascend, then d_ids is the table; otherwise a sorted (id, document) copy, 12 * ndocs bytes.  Made under ix.mu by the
    // first call that needs it, without the class table (a render never pays for that), dropped with it in release_sa.
    struct IdTable {
        bool valid = false;
        bool ids_ascend = true;    // d_ids is its own id -> document table
        DevBuf id_sorted, id_doc;  // !ids_ascend: the ids ascending (i64) and the document of each (u32)
        uint64_t bytes() const { return id_sorted.bytes + id_doc.bytes; }
        void drop() {
            valid = false;
            ids_ascend = true;
            id_sorted.release();
            id_doc.release();
        }
    } idt;
    // ---- cdb_render_rows (render.hip): the last call's wall time, page positions (bytes of the found rows' documents) and spans
    struct RenderStats {
        double last_ms = 0;
        uint64_t page_bytes = 0, spans = 0;
    } rnd;

    // ---- cdb_remove (remove.hip): calls that dropped something, by the path they took; the last call's documents, text bytes and wall time
    struct RemoveStats {
        uint64_t calls = 0, compactions = 0, rebuilds = 0;
        uint64_t docs = 0, bytes = 0;
        double last_ms = 0;
    } rm;
    // ---- cdb_append (append.hip): calls that added something, by the path they took; the last call's documents, text bytes, wall
    // time and whether the search keys came along
    struct AppendStats {
        uint64_t calls = 0, merges = 0, rebuilds = 0;
        uint64_t docs = 0, bytes = 0;
        double last_ms = 0;
        int with_keys = 0;
    } ap;
    int debug_append_path = 0;  // test hook: 0 = automatic, 1 = merge where it is valid, 2 = always rebuild
    // ---- cdb_insert_objects (insert.hip), kept on the handle that leads a call (its first field): calls that reached the commit, and
    // the fields, objects and wall time of the last one
    struct InsertStats {
        uint64_t calls = 0, fields = 0, objects = 0;
        double last_ms = 0;
    } ins;

    double host_upload_ms = 0, host_free_ms = 0;  // cdb_build: staged column to the device / staging copy released
    Profiler prof;
    BuildStats bstats;
    QueryStats qstats;
    mutable std::mutex err_mu;  // guards err (concurrent failing queries)
    std::string err;
};

// every entry point that touches the device: the handle's device current (a column's or a row set's handle is its `ws`), and the
// block cache told which stream this thread issues work on (common.h: blocks released meanwhile are tagged with it)
struct DeviceScope {
    StreamScope ss;
    explicit DeviceScope(Index& ix) : ss(ix.stream) { CDB_HIP(hipSetDevice(ix.device)); }
};

// capi.hip — ids / doc_start on the host (fetched from the device after a resident build)
void ensure_host_tables(Index& ix);
void ensure_host_staging(Index& ix);

// capi.hip — pieces shared with shards.hip
void read_raw_dir(const char* dir, const char* key, std::vector<int64_t>& ids, std::vector<uint64_t>& doc_start, std::string& text,
                  uint64_t& nrec, uint64_t& nadd);

// sa_build.hip
void build_suffix_array(Index& ix);

// cluster.hip — fills ix.idt on ix.stream (ix.mu held, device set); a no-op while the table is valid
void id_table_prepare(Index& ix);
// first slot of the ascending ids[0 .. n) that is not below id (n: none)
__device__ __forceinline__ uint64_t lower_bound_id(const int64_t* __restrict__ ids, uint64_t n, int64_t id) {
    uint64_t a = 0, b = n;
    while (a < b) {
        const uint64_t m = (a + b) >> 1;
        if (ids[m] < id) a = m + 1;
        else b = m;
    }
    return a;
}

// the ascending ids a field holds, as the calls that span fields read them (cdb_rowset_all, cdb_insert_objects)
struct IdList {
    const int64_t* ids;
    uint64_t n;
};
// ... of a string index (empty: never built, or built over nothing); the field's lock is held, its stream idle on return
inline IdList index_id_list(Index& ix) {
    if (!ix.width || !ix.ndocs) return IdList{nullptr, 0};
    DeviceScope scope(ix);
    id_table_prepare(ix);  // (synchronises where it makes the table)
    return IdList{ix.idt.ids_ascend ? ix.d_ids.as<int64_t>() : ix.idt.id_sorted.as<int64_t>(), ix.ndocs};
}
// the fields' locks, taken together in address order (columns.hip: filter_rows_on_lead's rule)
struct FieldLocks {
    std::vector<std::unique_lock<std::mutex>> locks;
    explicit FieldLocks(std::vector<std::mutex*> mus) {
        std::sort(mus.begin(), mus.end());
        mus.erase(std::unique(mus.begin(), mus.end()), mus.end());
        for (std::mutex* m : mus) locks.emplace_back(*m);
    }
};

inline KeptKeys keys_of(const Index& ix) {
    return KeptKeys{ix.d_keys.as<uint64_t>(), ix.d_keys32.as<uint32_t>(), ix.d_keylow.as<uint8_t>(), ix.key_low_bits,
                    ix.d_keylow.p ? std::max(ix.key_low_bytes, 1) : 0};
}
inline bool keys_recomputable(const Index& ix) {  // the handle holds keys, their code table, and every part of a split key
    return ix.key_nsym > 0 && (ix.d_keys.p || ix.d_keys32.p) && ix.d_symmap_q.p && ix.key_low_bytes >= 0 && ix.key_low_bytes <= 2 &&
           (ix.d_keys.p || ix.key_low_bits == 0 || (ix.d_keylow.p && ix.key_low_bytes >= 1));
}

// An array that arrives with its column instead of being built over it (cdb_load, cdb_remove, cdb_append), and the search keys that
// come along with the parameters they were made with (key_nsym = 0: none; the symbol maps of the handle stay as they are)
struct ArrivedArray {
    DevBuf sa, sa_hi;  // sa_hi: the packed storage's fifth bytes
    DevBuf keys, keys32, keylow;
    int key_nsym = 0, key_low_bits = 0, key_low_bytes = 0;
    uint32_t key_base = 0;
    void alloc(uint64_t n, int width, bool packed) {
        if (packed) {
            sa.alloc(std::max<uint64_t>(n, 4) * 4);
            sa_hi.alloc(std::max<uint64_t>(n, 16));
        } else {
            sa.alloc(std::max<uint64_t>(n * (uint64_t)width, 16));
        }
    }
    // key blocks of n slots in the forms ix holds, under its parameters
    KeptKeys alloc_keys_like(const Index& ix, uint64_t n) {
        const KeptKeys src = keys_of(ix);
        key_nsym = ix.key_nsym;
        key_base = ix.key_base;
        key_low_bits = ix.key_low_bits;
        key_low_bytes = ix.key_low_bytes;
        if (src.k64) keys.alloc(n * 8);
        if (src.k32) keys32.alloc(n * 4);
        if (src.low) keylow.alloc(n * (uint64_t)src.low_bytes);
        return KeptKeys{keys.as<uint64_t>(), keys32.as<uint32_t>(), keylow.as<uint8_t>(), src.low_bits, src.low_bytes};
    }
};
// the device blocks of a column: what cdb_remove and cdb_append make beside the old index and the commit (capi.hip) takes as a whole
struct ColumnBlocks {
    DevBuf d_start, d_ids, text;  // the tables and the library's own padded text
    ArrivedArray arr;             // empty: the array is built over them
};

// the rows' ids: a host array, or an array that already lies on the field's GPU (a row set's: rowset.hip), complete when the call
// is made and unchanged during it
struct RowIds {
    const int64_t* host = nullptr;
    const int64_t* device = nullptr;
};
// ... where the kernels read them: uploaded into d on s, or the caller's device array as it is
inline const int64_t* resident_ids(hipStream_t s, DevBuf& d, RowIds ids, uint64_t nrows) {
    if (ids.device) return ids.device;
    d.alloc(nrows * 8);
    CDB_HIP(hipMemcpyAsync(d.p, ids.host, nrows * 8, hipMemcpyHostToDevice, s));
    return d.as<int64_t>();
}

// remove.hip — the pieces of cdb_remove (capi.hip commits them), all on ix.stream with ix.mu held.  Everything is made in fresh
// blocks of the plan while the old index stands.
struct RemovePlan : ColumnBlocks {
    uint64_t removed = 0, missing = 0;         // distinct documents dropped, entries of ids the index does not hold
    uint64_t ndocs = 0, size = 0, longest = 0;  // the surviving column
    DevBuf drop, newdoc, src_start;            // u8[old ndocs] flag, u32[old ndocs] old -> new document, u64[ndocs] old start of every survivor
};
void remove_mark(Index& ix, RowIds ids, uint64_t nids, RemovePlan& p);  // flags, counts, and (something to drop) the new tables; synchronises
void remove_text(Index& ix, RemovePlan& p);                                      // the kept documents gathered into p.text
void remove_compact(Index& ix, RemovePlan& p, int new_bits, int new_width, bool new_packed);  // the array and its keys in the new layout
// out (zeroed by the caller) = the longest document among those whose drop flag is 0 (drop = nullptr: among all), queued on s
void longest_document(hipStream_t s, const uint8_t* drop, const uint64_t* doc_start, uint64_t ndocs, unsigned long long* out);

// append.hip — the pieces of cdb_append (capi.hip uploads the new text between them and commits), all on ix.stream with ix.mu held.
// Everything is made in fresh blocks of the plan while the old index stands (old then new: the tables and the padded text).
struct AppendPlan : ColumnBlocks {
    uint64_t ndocs = 0, size = 0, longest = 0;  // the new documents (filled by the caller) ...
    uint64_t in_bits = 1, in_mask = 1;          // ... and the layout of an index over them alone (the inner build)
    int in_width = 4, in_off_bits = 1;
    uint64_t old_longest = 0;                        // the built column's longest document
    bool high_bytes = false, unmapped_bytes = false;  // the new text holds bytes >= 0x80 / bytes the handle's symbol map codes as 0
};
void append_old_longest(Index& ix, AppendPlan& p);  // synchronises
void append_tables(Index& ix, AppendPlan& p, const int64_t* ids, const uint64_t* new_start);  // new_start[ndocs + 1]: based at the old size
void append_text_old(Index& ix, AppendPlan& p);     // p.text allocated, the old bytes copied in front, the padding zeroed
void append_scan_bytes(Index& ix, AppendPlan& p);   // the byte values of the new text (behind its upload); synchronises
void append_merge(Index& ix, AppendPlan& p, int new_bits, uint64_t new_mask, int new_width, bool new_packed);  // inner build, rank, merge; synchronises
// capi.hip — cdb_remove and cdb_append in two halves.  Prepare checks the call and makes everything new (text, tables, and where the
// array is kept its compacted / merged form) in fresh blocks beside the old index, which goes on serving; it throws what the entry
// point reports, and returns nullptr where there is nothing to commit (nids / ndocs = 0, no held id, a handle that holds nothing on
// remove: *removed / *missing are complete either way).  column_commit installs a prepared change and counts the call in the
// handle's stats; only a build over the new text (the reference-order path, or an append to a handle that held nothing) can fail in
// it, and leaves the handle "never built".  A change that is dropped uncommitted releases its blocks; the handle never knew of it.
// All three take ix.mu from the caller and set the device and stream themselves.  cdb_remove / cdb_append call the halves back to
// back; cdb_shards_remove / cdb_shards_append prepare on every shard before they commit on any.
struct ColumnChange;
struct ColumnChangeDelete {
    void operator()(ColumnChange* c) const;
};
using ColumnChangePtr = std::unique_ptr<ColumnChange, ColumnChangeDelete>;
ColumnChangePtr remove_prepare(Index& ix, RowIds ids, uint64_t nids, uint64_t* removed, uint64_t* missing);
ColumnChangePtr append_prepare(Index& ix, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs);
void column_commit(Index& ix, ColumnChange& c);
// cdb_remove / cdb_append change a built column only.  Returns its documents (0: never built, or built over nothing)
inline uint64_t built_docs_or_refuse(const Index& ix, const char* op) {
    const uint64_t built_docs = ix.width ? ix.ndocs : 0;
    if (ix.host_text_valid && ix.ids.size() > built_docs) throw Error(std::string(op) + ": documents were added since the last build");
    return built_docs;
}
void reserve_wait();  // a cdb_reserve still running in the background has finished (every build entry point waits for it first)
// out = {slots whose kept key differs from the key recomputed from the suffix, slots checked (0: no keys kept)}
void verify_kept_keys(Index& ix, uint64_t out[2]);

// verify.hip — out = {inversions, tie-order violations, wrapped sum of entries, invalid entries, expected sum}
void verify_suffix_array(Index& ix, uint64_t out[5]);
void sa_expand(Index& ix, uint64_t first, uint64_t cnt, uint64_t* d_out);  // verify.hip: packed entries -> u64 (on ix.stream)
void sa_pack_inplace(Index& ix);                                           // verify.hip: u64 entries in d_sa -> packed storage
void sa_pack_chunk(hipStream_t s, const uint64_t* d_in, uint64_t cnt, uint32_t* lo, uint8_t* hi, uint64_t first);  // verify.hip
inline bool sa_packable(const Index& ix) { return ix.pack_sa && ix.width == 8 && (int)ix.bits + ix.off_bits <= 40; }
void spot_check_suffix_array(Index& ix, uint32_t samples, uint64_t out[2]);  // verify.hip: the check behind every build
void proof_start(Index& ix);   // verify.hip: the full check behind a published build, on its own thread and stream (ix.mu held)
void proof_stop(Index& ix);    // ... cancelled and joined (before the arrays change; callable with ix.mu held)
void proof_forget(Index& ix);  // ... and the handle forgotten (cdb_destroy)
// sizes (>= 16 MiB) of the device blocks a published index holds on to: its arrays and the work spaces a handle keeps across calls —
// what a second generation built beside it will ask the block cache for once more (cdb_reserve, DevPool::premap)
inline std::vector<size_t> retained_block_sizes(const Index& ix) {
    std::vector<size_t> out;
    for (const DevBuf* b : {&ix.d_text_owned, &ix.d_sa, &ix.d_sa_hi, &ix.d_keys, &ix.d_keys32, &ix.d_keylow, &ix.d_doc_start, &ix.d_ids,
                            &ix.rws.status, &ix.rws.tile_doc, &ix.msd_ws.segs, &ix.msd_ws.tile_seg, &ix.msd_ws.hist, &ix.msd_ws.starts,
                            &ix.scan_partials, &ix.tbw.partial, &ix.tbw.blockbase, &ix.tbw.totals, &ix.tbw.base})
        if (b->p && b->bytes >= (16u << 20)) out.push_back(b->bytes);
    return out;
}
void debug_swap_entries(Index& ix, uint64_t k);  // verify.hip (test hook): entries k and k + 1 of the finished array swapped
// the REFERENCE's order (signed child order inside radix nodes, unsigned below), checked pair by pair:
// out = {pairs out of reference order, pairs whose next bytes differ in sign class, of those inside radix nodes,
// equal suffixes not ascending by document}
void verify_reference_order(Index& ix, uint64_t out[4]);
// number of entries of a suffix array (device pointers) that do not name a real (document, offset)
uint64_t count_invalid_entries(hipStream_t s, const void* d_sa, int width, uint64_t n, const uint64_t* d_doc_start, uint64_t ndocs,
                               int bits, uint64_t mask);

// query.hip — patterns already on the device; leaves CSR results in ix.q_rowptr / q_ids / q_counts
struct DeviceCsr {
    uint64_t npat = 0, nrows = 0, nhits = 0;
};
// with_offsets: additionally ix.q_hitptr[nrows+1] / ix.q_hitoff[nhits] = byte offsets of every occurrence,
// grouped by result row, ascending
DeviceCsr query_batch_on_device(Index& ix, const uint8_t* d_blob, const uint64_t* d_offs, uint64_t npat,
                                bool with_offsets = false);
// one keyword through the single-wavefront kernel; false = not applicable, use the batched path
bool query_single_on_device(Index& ix, const char* kw, size_t len, int64_t** ids_out, int64_t** counts_out, size_t* nrows);
// ... in two halves (several indexes queried at once, shards.hip): launch, then collect (false = handed over to the
// batched path); Absent = a byte the text never holds, the answer is empty without a launch (query_single_empty)
enum class SingleLaunch { NotApplicable, Absent, Launched };
SingleLaunch query_single_launch(Index& ix, const char* kw, size_t len);
bool query_single_collect(Index& ix, int64_t** ids_out, int64_t** counts_out, size_t* nrows);
void query_single_empty(Index& ix, int64_t** ids_out, int64_t** counts_out, size_t* nrows);
void query_resident_stop(Index& ix);  // the resident workgroup leaves (before the arrays it reads are replaced or freed)
// highlight spans of all documents matching any pattern: ids -> ix.q_ids, span_ptr -> ix.q_rowptr, span begins ->
// ix.q_keys0, inclusive span ends -> ix.q_keys1
struct SpanResult {
    uint64_t ndocs = 0, nspans = 0, nhits = 0;
};
SpanResult query_spans_on_device(Index& ix, const uint8_t* d_blob, const uint64_t* d_offs, uint64_t npat,
                                 uint64_t total_pattern_bytes);
// union over the patterns by object id with summed counts, rows ascending by id, in ix.q_ids / q_counts
DeviceCsr query_or_on_device(Index& ix, const uint8_t* d_blob, const uint64_t* d_offs, uint64_t npat);
// ... filtered to lo <= count < hi and ranked: descending count, ties ascending id, at most `limit` rows (0 = all)
DeviceCsr query_ranked_on_device(Index& ix, const uint8_t* d_blob, const uint64_t* d_offs, uint64_t npat, int64_t lo, int64_t hi,
                                 uint64_t limit);

// AND across keys (interface.cpp:114-134): intersection of row lists (each ascending by id, ids unique within a list)
// by object id with summed counts, on ix's stream; rows land in ix.q_ids / q_counts — ascending id, or filtered to
// lo <= count < hi and ranked (descending count, ties ascending id, at most `limit` rows) when `ranked`
struct DeviceRows {
    const int64_t* d_ids;
    const int64_t* d_counts;
    uint64_t n;
};
DeviceCsr and_merge_on_device(Index& ix, const std::vector<DeviceRows>& lists, bool ranked, int64_t lo, int64_t hi, uint64_t limit);
// rows (ids ascending) in ix.q_ids / q_counts -> filtered to lo <= count < hi and ranked in place (the tail of and_merge_on_device;
// columns.hip runs its probe filters between the merge and this step)
DeviceCsr rank_rows_on_device(Index& ix, DeviceCsr r, int64_t lo, int64_t hi, uint64_t limit);


template <> inline SaOf<uint32_t>::ptr Index::sa_view<uint32_t>() const { return d_sa.as<uint32_t>(); }
template <> inline SaOf<uint64_t>::ptr Index::sa_view<uint64_t>() const { return d_sa.as<uint64_t>(); }
template <> inline SaOf<Packed40>::ptr Index::sa_view<Packed40>() const { return Sa40{d_sa.as<uint32_t>(), d_sa_hi.as<uint8_t>()}; }
// f(tag) with the tag of the index's storage: the one place that knows the three forms
template <typename F> inline auto sa_dispatch(const Index& ix, F&& f) {
    if (ix.sa_packed) return f(Packed40{});
    if (ix.width == 8) return f(uint64_t{});
    return f(uint32_t{});
}

}  // namespace cdb

// the object behind the C ABI's opaque handle (capi.hip, capi_query.hip, shards.hip)
struct cdb_index {
    cdb::Index ix;
};
// ... and behind cdb_column (columns.hip builds and queries it, cluster.hip groups by it)
struct cdb_column {
    int kind = 1;
    cdb::Index ws;  // stream, device, lock, error text, radix / scan work spaces, profiler; result rows of an AND it leads (q_ids / q_counts)
    std::vector<int64_t> staged_ids;
    std::vector<uint64_t> staged_raw;
    uint64_t n = 0;
    uint64_t n_false = 0;  // bool: rows with value false (they come first in key order)
    cdb::DevBuf keys_v, ids_v, id_sorted, vpos;
    cdb::DevBuf d_bounds;  // scratch: bound values, tags, positions
    double build_ms = 0;
    double last_union_ms = 0;  // the last materialisation (windows uploaded .. ids on the device), host wall clock
    int id_sort_skipped = 0;
    int debug_query_path = 0;
    uint64_t sparse_queries = 0, dense_queries = 0, probe_filters = 0, materialised_keys = 0, last_k = 0;
    // cluster.hip: where every run of equal keys starts (u64[runs + 1]), made at the first dense cluster of this build
    uint64_t generation = 0;  // counts builds
    uint64_t clu_generation = UINT64_MAX, clu_runs = 0;
    cdb::DevBuf clu_run_start;
    int debug_cluster_path = 0;  // 0 = automatic, 1 = always sparse, 2 = always dense
    uint64_t sparse_clusters = 0, dense_clusters = 0;
    double cluster_ms = 0;
    // column_maintain.hip: cdb_column_append / cdb_column_remove
    int debug_maintain_path = 0;  // 0 = automatic, 1 = the device path wherever it is valid, 2 = the host filter / stage + column_build
    uint64_t appends = 0, append_merges = 0, append_rebuilds = 0, append_rows = 0, append_id_concat = 0;
    uint64_t removes = 0, remove_compactions = 0, remove_rebuilds = 0, remove_rows = 0;
    double append_ms = 0, remove_ms = 0;
};
// ... and behind cdb_rowset (rowset.hip makes and pages it, select.hip reads a page's fields)
struct cdb_rowset {
    cdb::Index ws;  // stream, device, lock, error text, radix / scan work spaces, profiler
    cdb::DevBuf ids, counts;  // m rows, ascending id
    uint64_t m = 0;
    cdb::DevBuf state;        // ST_* words
    uint64_t key_diff = 0;    // bits in which the rows' keys differ
    int debug_page_path = 0;  // 0 automatic, 1 select (where K < m), 2 sort
    uint64_t page_selects = 0, page_sorts = 0, select_passes = 0, clusters = 0;
    double page_ms = 0, cluster_ms = 0;
    uint64_t selects = 0, select_rows = 0;  // select.hip: cdb_rowset_select calls, and the rows of the last one
    double select_ms = 0;
    // rowset_maintain.hip: cdb_rowset_remove calls that ran, and the fields and wall time of the last one; cdb_rowset_all: the fields
    // and id-list entries the set was made from, and the wall time of that
    uint64_t removes = 0, remove_fields = 0, all_fields = 0, all_input_rows = 0;
    double remove_ms = 0, all_ms = 0;
};
struct cdb_key_query;
namespace cdb {
// rowset.hip — a page in two halves: rows [first, min(last, m)) of the ranking left in device buffers on the row set's stream
// (nothing is synchronised; the sort's buffers live on in the page until it goes), and rows from the device into result arrays
// (synchronises).  cdb_rowset_page is the two back to back; cdb_rowset_select keeps the device ids for its fields.  The caller
// holds the row set's lock and has its stream and device set.
struct DevicePage {
    DevBuf k0, k1, v0, v1, ids, counts;
    uint64_t n = 0;  // rows in ids / counts (0: neither is allocated)
};
void rowset_page_device(cdb_rowset* rs, uint64_t first, uint64_t last, DevicePage& pg);
// rowset.hip — an empty row set with a stream of its own on `device`; its end (stream drained and destroyed); and the end of a
// set's creation when every count is equal (cdb_rowset_all: no key bit differs, no pass over the counts is needed; synchronises s)
cdb_rowset* rowset_new(int device);
void rowset_delete(cdb_rowset* rs);
void rowset_adopt_equal_counts(cdb_rowset* rs, hipStream_t s, int64_t count);
// render.hip — cdb_render_rows over ids that already lie in device memory on the handle's GPU (complete when the call is made; the
// caller keeps them unchanged during it).  Takes the handle's lock and throws.
void render_index_device_rows(cdb_index* h, const int64_t* d_ids, uint64_t nrows, const char* blob, const uint64_t* offsets, uint64_t nkw,
                              const char* left, uint64_t left_len, const char* right, uint64_t right_len, int what, cdb_rendered* out);
// columns.hip — the four arrays of a column (layout: columns.hip's head) while they are made, before they are published
struct ColumnArrays {
    DevBuf keys_v, ids_v, id_sorted, vpos;
    uint64_t n = 0, n_false = 0;
    int id_sort_skipped = 0;
};
constexpr uint64_t COLUMN_MAX_ROWS = 0xFFFFFFFFull;  // vpos and the carried ranks are 32-bit
// The sort part of a build: idk (object ids) and key (order keys below first_new, raw values from there on), n rows each on the
// device, become the four arrays.  Both inputs are consumed.  `who` names the entry point in the duplicate-id error.
void column_sort_rows(cdb_column* c, DevBuf& idk, DevBuf& key, uint64_t n, uint64_t first_new, const char* who, ColumnArrays& out);
// the raw values of staged rows as add_bulk keeps them (NaN refused; `who` names the entry point)
std::vector<uint64_t> column_raw_values(int kind, const void* values, uint64_t n, const char* who);
// the arrays replace the column's own; the stream is idle.  Bumps `generation` (cluster.hip remakes its run table).
void column_publish(cdb_column* c, ColumnArrays& a);
void column_build(cdb_column* c, const char* who = "cdb_column_build");
// cdb_column_remove's host path: download, filter on the host, column_build over the rest (built and staged rows alike)
void column_remove_host(cdb_column* c, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing);
// column_maintain.hip — the device path of a removal (no staged rows) in two halves, as a string index has them (remove_prepare /
// column_commit above).  Prepare: mark, two stable compactions, one gather of the positions, all into fresh blocks beside the
// serving arrays; removed / missing are complete when it returns, `changed` says whether there is anything to commit; it throws
// and leaves the column untouched.  Commit: column_publish plus the stats of a cdb_column_remove; it cannot fail.  A removal that
// is dropped uncommitted hands its blocks back (release: on the column's device and stream); the column never knew of it.
// The caller holds the column's lock and, for prepare and commit, a DeviceScope on c->ws.
struct ColumnRemoval {
    ColumnArrays a;
    uint64_t removed = 0, missing = 0;
    bool changed = false;
    double t0 = 0;  // wall_ms() when the call began (remove_ms)
    void release(cdb_column* c) {
        (void)hipSetDevice(c->ws.device);
        StreamScope ss(c->ws.stream);
        a = ColumnArrays{};
        changed = false;
    }
};
void column_remove_prepare(cdb_column* c, RowIds ids, uint64_t nids, ColumnRemoval& r);
void column_remove_commit(cdb_column* c, ColumnRemoval& r);
// column_maintain.hip — cdb_column_append in the same two halves (cdb_insert_objects, insert.hip, prepares every field of a call before
// it commits any).  The caller has checked the call (no staged rows, the row limit, raw = column_raw_values) and sets t0 and `merge`:
// true = the two-way merge of a built column with rows (c->n > 0); false = the build over the old rows and the batch, which for a
// column without rows is column_sort_rows of the batch alone.  Prepare leaves the new arrays in fresh blocks beside the serving ones
// and throws what cdb_column_append reports (the duplicate-id refusal among it), the column untouched.  Commit: column_publish plus
// the stats of a cdb_column_append; it cannot fail.  release: as ColumnRemoval's.  Lock and DeviceScope as for the removal.
struct ColumnAppendChange {
    ColumnArrays a;
    uint64_t rows = 0;
    bool merge = false;    // in: which path
    bool concat = false;   // merge: the id order was a concatenation
    bool changed = false;  // prepared and not yet committed
    double t0 = 0;         // wall_ms() when the call began (append_ms); the build path's own start is build_t0
    double build_t0 = 0;
    void release(cdb_column* c) {
        (void)hipSetDevice(c->ws.device);
        StreamScope ss(c->ws.stream);
        a = ColumnArrays{};
        changed = false;
    }
};
void column_append_prepare(cdb_column* c, const int64_t* ids, const std::vector<uint64_t>& raw, uint64_t m, ColumnAppendChange& r);
void column_append_commit(cdb_column* c, ColumnAppendChange& r);
// the value (bit pattern) behind a column's order-preserving key (columns.hip: order_key; kind: 0 bool, 1 int64, 2 double)
__host__ __device__ __forceinline__ uint64_t column_key_raw(int kind, uint64_t key) {
    constexpr uint64_t S = 1ull << 63;
    if (kind == 1) return key ^ S;
    if (kind == 2) return (key & S) ? (key ^ S) : ~key;
    return key;
}
// The body of every C-ABI entry point that can fail: the call counts itself in (common.h: ForegroundCall), and an exception
// becomes its CDB_E_* code (errors.h) plus the object's last-error text.  Calls run concurrently on one object (database.cpp:388),
// so the text has its own lock.
template <typename F>
int guarded_call(std::mutex& err_mu, std::string& err, F&& f) {
    ForegroundCall fg;
    try {
        f();
        return CDB_OK;
    } catch (...) {
        Failure fail = classify_current_exception();
        std::lock_guard<std::mutex> g(err_mu);
        err = std::move(fail.message);
        return fail.code;
    }
}
// ... for an object that reports through an Index (string indexes, columns, clusters)
template <typename F>
int guarded_ix(Index& ix, F&& f) {
    return guarded_call(ix.err_mu, ix.err, std::forward<F>(f));
}
inline void set_error(Index& ix, const std::string& msg) {
    std::lock_guard<std::mutex> g(ix.err_mu);
    ix.err = msg;
}
// What a *_last_error accessor returns: the text copied under its lock into the accessor's own per-thread string, so that
// another thread's failing call cannot pull it away under the reader.
inline const char* last_error_copy(std::mutex& err_mu, const std::string& err, std::string& copy) {
    std::lock_guard<std::mutex> g(err_mu);
    copy = err;
    return copy.c_str();
}
// columns.hip — the body cdb_query_and (capi_query.hip: no column keys), cdb_query_and_columns and cdb_filter (rowset.hip) share:
// filter_lead names the handle that runs the merge and carries the error (nullptr: CDB_E_INVALID); filter_rows_on_lead validates,
// locks, resolves and merges the keys and calls `consume` under those locks with the rows in ix.q_ids / q_counts on ix.stream.
// The errors speak in the entry point's name.
struct FilterNames {
    const char* who;
    const char* one_gpu;  // the refusal of keys on several GPUs, whole
};
constexpr FilterNames QUERY_AND_NAMES{"cdb_query_and", "cdb_query_and: all string keys must live on one GPU"};
constexpr FilterNames QUERY_AND_COLUMNS_NAMES{"cdb_query_and_columns", "cdb_query_and_columns: all keys must live on one GPU"};
Index* filter_lead(const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols);
void filter_rows_on_lead(Index& ix, const FilterNames& names, const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols,
                         bool ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit,
                         const std::function<void(hipStream_t, DeviceCsr)>& consume);
// cluster.hip — cdb_cluster / cdb_column_cluster over ids that already lie in device memory on the field's GPU (complete when the
// call is made; the caller keeps them unchanged during it).  They take the field's lock and throw.
void cluster_index_device_rows(cdb_index* h, const int64_t* d_ids, uint64_t nrows, bool with_values, cdb_clusters* out);
void cluster_column_device_rows(cdb_column* c, const int64_t* d_ids, uint64_t nrows, cdb_clusters* out);
// capi_query.hip — cdb_query_and on `lead`'s device and stream (shards.hip: every key of a sharded AND arrives as a row list)
int query_and_with_lead(cdb_index* lead, const cdb_key_query* keys, int nkeys, int ranked, int64_t corr_lo, int64_t corr_hi,
                        uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows);
}
