/* coffeedb_gpu.h — C ABI of libcoffeedb_gpu.so, the MI355X (gfx950) implementation of CoffeeDB's
 * string-index hot path (suffix-array build + substring-match scan).
 *
 * Every entry point states the reference interface it replaces (paths relative to the CoffeeDB tree,
 * /root/reference in the build container).  The reference-side binding is a ~60-line C++ shim
 * (coffeedb_amd/csrc/index.h + index.cpp, shown in INTEGRATION.md) that keeps the reference's
 * `index` / `string_index` classes so src/database.cpp compiles and behaves unchanged.
 *
 * Conventions: plain C types, no exceptions across the boundary.  Functions returning `int` return
 * CDB_OK (0) or a CDB_E_* code; the message for the last failure on a handle is cdb_last_error(h)
 * and uses the reference's own wording where the reference throws (index.cpp:196,199,240).
 * A handle may be used from several host threads at once for queries (reference contract:
 * query() is const and runs under a shared lock, database.cpp:388); build is exclusive.
 * Device pointers handed to the *_device entry points must hold complete data when the call is made:
 * the library works on its own non-blocking HIP stream and does not wait for the caller's streams
 * (callers synchronise first, e.g. torch.cuda.synchronize()); every entry point returns only after its
 * own device work has finished.
 */
#ifndef COFFEEDB_GPU_H
#define COFFEEDB_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDB_OK 0
#define CDB_E_INVALID 1   /* bad argument / empty keyword / capacity limit (reference: std::runtime_error) */
#define CDB_E_DEVICE 2    /* HIP runtime failure, no usable gfx950 device, out of device memory */
#define CDB_E_INTERNAL 3  /* internal invariant violated (e.g. bounded look-back spin expired) */

typedef struct cdb_index cdb_index; /* opaque; replaces `string_index` (src/index.h:54-86) */

/* Result of a batched query in CSR form: pattern j owns rows [row_ptr[j], row_ptr[j+1]); each row is
 * (ids[r], counts[r]) = (object id, number of overlapping occurrences = $correlation), rows of one
 * pattern ascending by document insertion index — the order string_index::query returns
 * (src/index.cpp:316-322).  Host memory, owned by the library until cdb_result_free(). */
typedef struct cdb_result {
    uint64_t npat;
    uint64_t nrows;
    uint64_t nhits;      /* total suffix-array entries matched over the batch */
    uint64_t* row_ptr;   /* npat + 1 */
    int64_t* ids;        /* nrows */
    int64_t* counts;     /* nrows */
} cdb_result;

/* ---- lifetime -------------------------------------------------------------------------------- */

/* replaces std::make_unique<string_index>() (src/database.cpp:255, :303).  device < 0 selects the
 * current HIP device.  Fails with CDB_E_DEVICE when no gfx950 GPU is usable: there is no CPU path. */
int cdb_create(cdb_index** out, int device);

/* replaces string_index::~string_index (src/index.h:80-84) */
void cdb_destroy(cdb_index* h);

const char* cdb_last_error(const cdb_index* h);

/* ---- ingest ---------------------------------------------------------------------------------- */

/* replaces string_index::add(int64_t id, std::string_view value) (src/index.cpp:174-177).
 * The bytes are copied into a host staging buffer (the reference keeps a non-owning view instead).  cdb_build
 * frees that staging copy once the column is on the device; adding to an index that was built, loaded
 * (cdb_load) or built from device memory first fetches the column back, so "load, add, rebuild" works. */
int cdb_add(cdb_index* h, int64_t id, const char* value, size_t len);

/* Bulk form of cdb_add for callers that already hold a concatenated column:
 * document d = blob[doc_start[d] .. doc_start[d+1]), ndocs documents. */
int cdb_add_bulk(cdb_index* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs);

/* Raw-record ingest — the step before add() in database.cpp:170-275: CoffeeDB keeps one
 * binary file per object (writer database.cpp:334-378):
 *   int64 id | int32 nfields | nfields x { int32 keylen | key | int8 type | value },
 *   value = 1 byte (type 0 bool) | 8 bytes (1 integer, 2 double) | int32 len + bytes (3 string).
 * cdb_raw_record_find_string locates the string value stored under `key` in one in-memory record
 * (returns 1 found, 0 absent / not a string, -1 malformed; no handle or GPU needed);
 * cdb_add_raw_record adds that value under the record's id (a record without the key is skipped). */
int cdb_raw_record_find_string(const void* record, size_t len, const char* key, int64_t* id, const char** value,
                               size_t* value_len);
int cdb_add_raw_record(cdb_index* h, const char* key, const void* record, size_t len);
/* Bulk form: every record file of directory `dir` (CoffeeDB's storage_location/raw/, one file per object) in ascending
 * file-name order; the string under `key` of each record goes straight into the staged column.  *records = files
 * parsed, *added = documents added.  All or nothing: a malformed or unreadable file fails the call and leaves the
 * staged column as it was. */
int cdb_add_raw_dir(cdb_index* h, const char* dir, const char* key, uint64_t* records, uint64_t* added);

/* Persistence of a built index (the reference has none and rebuilds every index at start,
 * server.cpp:44): header + ids + doc_start + text + suffix array.  cdb_load restores a queryable index
 * without rebuilding. */
int cdb_save(cdb_index* h, const char* path);
int cdb_load(cdb_index* h, const char* path);

/* ---- build ----------------------------------------------------------------------------------- */

/* replaces string_index::build() (src/index.cpp:178-236): computes bits/mask/size and the entry width
 * exactly as the reference does (index.cpp:182-208), uploads the staged text and constructs the
 * suffix array on the GPU.  Errors reuse the reference's messages (index.cpp:196,199). */
int cdb_build(cdb_index* h);

/* Build straight from the caller's host column, without the staging copy cdb_add_bulk makes — string_index itself
 * holds non-owning string_views into the caller's strings (src/index.h:58, database.cpp:262-264).  ids[ndocs],
 * doc_start[ndocs + 1] (offsets into blob, non-decreasing; blob[doc_start[0] .. doc_start[ndocs]) is the column).
 * Replaces whatever cdb_add* staged.  The text travels through a chunked pinned upload (~50 GB/s); afterwards the
 * handle holds device copies only (a later cdb_add fetches the column back first). */
int cdb_build_view(cdb_index* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs);
/* The same for documents that are separate strings: document d = lens[d] bytes at ptrs[d] — what string_index::add
 * collects (index.cpp:174-177) and what the shim's build() passes.  The strings must stay valid during the call only. */
int cdb_build_views(cdb_index* h, const int64_t* ids, const char* const* ptrs, const uint64_t* lens, uint64_t ndocs);

/* Same build, but over text that already resides in device memory (HBM-resident timing in bench.py,
 * multi-GPU shards).  d_text must stay valid for the lifetime of the index (the reference's
 * string_view contract, database.cpp:262-264); doc_start/ids are host arrays and are copied. */
int cdb_build_device(cdb_index* h, const void* d_text, const uint64_t* doc_start, const int64_t* ids,
                     uint64_t ndocs);

/* The same with the document table resident as well: d_doc_start (ndocs + 1 offsets into d_text, d_doc_start[0]
 * = 0) and d_ids are DEVICE arrays; they are validated and copied on the device, nothing but a few scalars
 * crosses PCIe.  (Host copies of the tables — and of the text, for cdb_add* followed by a rebuild — are fetched
 * back from the device when cdb_save / cdb_add* need them later; d_text must still be valid then.) */
int cdb_build_resident(cdb_index* h, const void* d_text, const uint64_t* d_doc_start, const int64_t* d_ids,
                       uint64_t ndocs);

/* ---- query ----------------------------------------------------------------------------------- */

/* replaces string_index::query(const std::string& keyword) (src/index.cpp:237-326).  On success
 * *ids / *counts point to *nrows entries allocated by the library (release with cdb_free).
 * Empty keyword -> CDB_E_INVALID, message "Empty keywords are not allowed" (index.cpp:239-241).
 * A never-built index returns zero rows (the reference reads uninitialised state there). */
int cdb_query(cdb_index* h, const char* keyword, size_t len, int64_t** ids, int64_t** counts, size_t* nrows);
void cdb_free(void* p);

/* Batched form (no reference counterpart — interface.cpp:79-113 loops query() per keyword): pattern j
 * = blob[offsets[j] .. offsets[j+1]).  Any empty pattern fails the whole call like cdb_query. */
int cdb_query_batch(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out);
void cdb_result_free(cdb_result* r);

/* Batched query that also emits WHERE every occurrence sits (BASELINE config 2: "highlight offset
 * emission"): row r of the CSR result owns occurrences [hit_ptr[r], hit_ptr[r+1]) of `offsets`, the byte
 * offsets of the keyword inside that row's document, ascending.  The offsets are the `entry >> bits`
 * fields of the matched suffix-array range, sorted along with (pattern, document). */
typedef struct cdb_hits {
    uint64_t* hit_ptr;  /* nrows + 1 */
    uint64_t* offsets;  /* nhits */
} cdb_hits;
int cdb_query_batch_offsets(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out,
                            cdb_hits* hits);
void cdb_hits_free(cdb_hits* x);

/* OR over the keywords of ONE string key — replaces the per-key merge loop of interface.cpp:78-113
 * (query each keyword, sort by id, merge lists by id summing the counts): returns the union of the
 * matching objects with their summed $correlation, rows ascending by object id — exactly the list
 * filter() holds for that key before the AND across keys, the $correlation range filter and the final
 * ranking (which stay host-side in the shim: coffeedb_amd/csrc/shim/ranking.h).  Object ids are assumed
 * unique (they are insertion timestamps, interface.cpp:151,178).  Release ids/counts with cdb_free. */
int cdb_query_or(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t** ids, int64_t** counts,
                 size_t* nrows);

/* The same union, then the $correlation range filter (interface.cpp:137-143: corr_lo <= count < corr_hi) and
 * the final ranking (interface.cpp:144-146) on the device: rows by descending count, at most `limit` of them
 * (0 = all).  The reference ranks with an unstable std::sort, so its order among equal counts is arbitrary;
 * here ties ascend by object id (the shim's host-side rank_by_correlation reproduces the reference's own
 * tie order when that is wanted bit for bit).  Release ids/counts with cdb_free. */
int cdb_query_ranked(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t corr_lo, int64_t corr_hi,
                     uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows);

/* AND across keys — replaces the second half of filter() (interface.cpp:114-146): the per-key row lists are intersected
 * by object id with the counts added up, then optionally filtered by the $correlation range and ranked, all on the
 * device.  A key is either a string column (index + its keyword list: resolved here with the OR of cdb_query_or) or a
 * row list resolved elsewhere (index = NULL: numeric and bool keys return (id, 0) rows, ascending by id, each id once).
 * ranked = 0: rows ascending by object id (the list filter() holds after line 134; corr_* and limit ignored);
 * ranked = 1: corr_lo <= count < corr_hi, descending count, ties ascending id, at most `limit` rows (0 = all).
 * All string keys must live on one GPU; errors are reported on the first string key's handle.  Release ids / counts
 * with cdb_free. */
typedef struct cdb_key_query {
    cdb_index* index;        /* string key, or NULL */
    const char* blob;        /* its keywords: blob[offsets[j] .. offsets[j+1]) */
    const uint64_t* offsets;
    uint64_t nkw;
    const int64_t* ids;      /* index == NULL: host rows */
    const int64_t* counts;
    size_t nrows;
} cdb_key_query;
int cdb_query_and(const cdb_key_query* keys, int nkeys, int ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit, int64_t** ids,
                  int64_t** counts, size_t* nrows);

/* ---- numeric and bool columns (columns.hip) ------------------------------------------------------
 * A column replaces bool_index / integer_index / double_index (src/index.h:23-52, index.cpp:63-74, 129-173) on the
 * device.  kind = the reference's `number` tag: 0 bool, 1 int64, 2 double.  Like cdb_create, cdb_column_create fails
 * with CDB_E_DEVICE when no gfx950 GPU is usable: there is no CPU path.  Object ids must be unique within a column
 * (database.cpp guarantees it); cdb_column_build refuses a duplicate with CDB_E_INVALID.  At most 2^32 - 1 rows. */
typedef struct cdb_column cdb_column;
int cdb_column_create(cdb_column** out, int device, int kind);
void cdb_column_destroy(cdb_column* c);
const char* cdb_column_last_error(const cdb_column* c);
/* values: int64_t[n] (kind 1), double[n] (kind 2) or uint8_t[n] (kind 0, nonzero = true).  May be called repeatedly;
 * rows become visible at the next cdb_column_build, which indexes every row added so far.  NaN is refused. */
int cdb_column_add_bulk(cdb_column* c, const int64_t* ids, const void* values, uint64_t n);
int cdb_column_build(cdb_column* c);
/* numeric_query / bool_index::query for one range: int64 and double rows in (value, id) order, bool rows in insertion
 * order; the reference's range grammar and messages ("Invalid range: ...", "Invalid value: ...", "Invalid query: \"...\"").
 * Release ids with cdb_free. */
int cdb_column_query(cdb_column* c, const char* range, size_t len, int64_t** ids, size_t* nrows);
/* OR over the ranges blob[offsets[j] .. offsets[j+1]) of one numeric / bool key (interface.cpp:78-113): the union of their
 * rows, ascending object id, each id once.  Release ids with cdb_free. */
int cdb_column_query_any(cdb_column* c, const char* blob, const uint64_t* offsets, uint64_t nranges, int64_t** ids, size_t* nrows);
/* AND across string keys / host row lists (keys, as in cdb_query_and) and column keys, all on one GPU: the result equals
 * cdb_query_and given the same keys plus each column's cdb_column_query_any rows as (id, 0) host rows, ranked or not.
 * nkeys may be 0 (keys = NULL) and ncols may be 0.  Errors are reported on the first string key's handle, or, without
 * one, on the first column (cdb_column_last_error). */
typedef struct cdb_column_key {
    cdb_column* column;
    const char* blob;        /* its ranges: blob[offsets[j] .. offsets[j+1]) */
    const uint64_t* offsets;
    uint64_t nranges;
} cdb_column_key;
int cdb_query_and_columns(const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols, int ranked, int64_t corr_lo,
                          int64_t corr_hi, uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows);
/* "rows", "staged_rows", "build_ms", "id_sort_skipped", "sparse_queries", "dense_queries", "probe_filters",
 * "materialised_keys", "last_k" (rows inside the last query's windows), "last_union_ms" (the last query_any's or
 * materialised key's union on the device, result download excluded), "sparse_clusters", "dense_clusters", "cluster_ms" (the last
 * cdb_column_cluster: ids uploaded .. groups on the host), and the append_* / remove_* stats named at cdb_column_append and
 * cdb_column_remove */
int cdb_column_get_stat(const cdb_column* c, const char* name, double* value);
/* Test and measurement hooks of the columns — NOT part of the stable ABI (like the other cdb_debug_* entry points they may change
 * or go without notice; the library chooses every path itself, a caller never needs them):
 * cdb_debug_column_set_option: "profile" (0/1: time the column's kernels with HIP events, read by cdb_debug_column_profile_dump as
 * "name ms launches bytes" lines) and "debug_query_path" (0 = automatic, 1 = always sparse, 2 = always dense: the tests of both
 * union paths and the crossover measurement of tools/bench_columns.py); "debug_maintain_path" (0 = automatic,
 * 1 = the device path of cdb_column_append / cdb_column_remove wherever it is valid, 2 = stage + build / host filter + build:
 * DESIGN.md §7.8); "debug_fail_prepare" (0/1: the prepare half of a device removal throws a device error behind its queued work, the
 * column stays as it was — like cdb_set_option's "debug_fail_build" and "debug_fail_prepare" for a string index: cdb_rowset_remove); "debug_fail_append_prepare" (0/1: the same for the
 * prepare half of an append: cdb_insert_objects). */
int cdb_debug_column_set_option(cdb_column* c, const char* name, int64_t value);
int cdb_debug_column_profile_dump(cdb_column* c, char* buf, size_t cap);

/* ---- cluster (cluster.hip) ---------------------------------------------------------------------------
 * replaces database.cpp:442-460 (`cluster`, driven by interface.cpp:249-273): "how many of the rows filter() left over have
 * which value in field F".  The reference walks the rows through its host object store into a std::map<std::string, int64_t>;
 * here the rows are grouped on the device by the column / string index that already holds the field.
 *
 * Input: the ids of the rows (the counts of a result row play no part).  nrows = 0 is valid and yields zero groups; so does a
 * column / index that was never built (every row is then `missing`, the choice cdb_query makes for an unbuilt index).
 * An id the column / index does not hold is skipped and counted in `missing` (the reference dereferences data[id].find(field)
 * unchecked there: undefined behaviour); sum(counts) + missing == nrows always.  A repeated id counts as often as it is given.
 * Group order — column: ascending by value, compared as the column compares; string index: ascending by
 * std::string::operator< (unsigned bytes, a proper prefix first, the empty string first of all) whatever reference_compat is
 * and whatever bytes the text holds.
 * KNOWN DIVERGENCE: a double column folds -0.0 onto +0.0 when it is built, so the two zeros form ONE group whose value is
 * +0.0; the reference would print "-0.000000" and "0.000000" separately.
 * The strings the reference prints for numeric values (std::to_string, with distinct values that print alike merged) are
 * made on the host by cdb_shim::cluster_rows (coffeedb_amd/csrc/shim/cluster.h).
 * All arrays are host memory owned by the library (pinned result cache when large): release with cdb_clusters_free only.
 * Both calls are queries: several host threads may run them on one handle, they wait out a rebuild; the string index's class
 * table (4 bytes per document + 4 per distinct document, stats "cluster_table_bytes", "cluster_classes",
 * "cluster_prepare_ms", "cluster_ms"; "cluster_resorted" = 1 when its classes had to be ordered on the host) is made once per
 * built array under the handle's lock, at the first cdb_cluster, and goes wherever that array goes: every build and load, and the
 * order proof's repair of a damaged array.  Cost to know: when the array is in the reference's order (reference_compat = 1 and text
 * with bytes >= 0x80) the classes are put into std::string order on the HOST — one document per class is downloaded and sorted
 * while the handle's lock is held; for a column of mostly distinct documents that is nearly the whole text (254 ms for 256 MiB
 * of distinct 256-byte documents on an MI355X host), once per build.  Pure ASCII text and reference_compat = 0 skip that step.
 * cdb_debug_column_set_option "debug_cluster_path" (0 automatic, 1 sort + run lengths, 2 counters per position) forces one of
 * the column's two paths (tests, tools/bench_cluster.py).  A sharded string column clusters with cdb_shards_cluster. */
typedef struct cdb_clusters {
    uint64_t ngroups;
    uint64_t missing;      /* input rows whose id the column / index does not hold (skipped) */
    int64_t* counts;       /* ngroups: input rows in the group */
    int64_t* rep_ids;      /* ngroups: the smallest object id of the group among the input rows */
    uint64_t* values;      /* column: ngroups raw values (int64 / double bit pattern / 0, 1); string index: NULL */
    uint64_t* value_ptr;   /* string index with with_values != 0: ngroups + 1 offsets into value_blob; else NULL */
    char* value_blob;      /* the groups' strings, concatenated */
} cdb_clusters;
int cdb_column_cluster(cdb_column* c, const int64_t* ids, uint64_t nrows, cdb_clusters* out);
int cdb_cluster(cdb_index* h, const int64_t* ids, uint64_t nrows, int with_values, cdb_clusters* out);
void cdb_clusters_free(cdb_clusters* r);

/* ---- row sets (rowset.hip) -----------------------------------------------------------------------------
 * The reference's read operations — `count`, `query` with `span`, `cluster`, and the row list `remove` takes — all start with the same
 * filter() (interface.cpp:46-148) and then use a sliver of its result.  A row set is that result left in device memory: filter once,
 * then count, page and cluster without the rows crossing PCIe in between.
 *
 * cdb_filter is filter() up to interface.cpp:143: keys / cols exactly as cdb_query_and_columns takes and validates them (same errors,
 * same messages, reported on the same handle / column: the first string key's, or without one the first column's); has_corr != 0
 * keeps rows with corr_lo <= count < corr_hi (signed).  The rows — ascending object id, each id once, counts summed — stay in device
 * memory owned by the row set, which holds copies of its own: it survives later queries on the handles that produced it, their
 * rebuild and their destruction, and holds none of their locks once cdb_filter has returned.  Sharded keys go in as host rows
 * resolved with cdb_shards_query_or.  Calls on one row set serialise on its lock; the cluster calls take the row set's lock and then
 * the field's, and wait out a rebuild as cdb_cluster does.  Release result arrays with cdb_free / cdb_clusters_free.
 *
 * ORDER OF A PAGE: descending count compared as SIGNED int64 (the reference's comparator, interface.cpp:144-146), ties ascending id.
 * cdb_query_ranked / cdb_query_and(_columns) with ranked = 1 order counts as unsigned, so a negative count (possible only in host
 * rows) ranks first there and last here; the two agree on every non-negative count. */
typedef struct cdb_rowset cdb_rowset;
int cdb_filter(const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols, int has_corr, int64_t corr_lo,
               int64_t corr_hi, cdb_rowset** out);
void cdb_rowset_free(cdb_rowset* rs);
const char* cdb_rowset_last_error(const cdb_rowset* rs);
uint64_t cdb_rowset_size(const cdb_rowset* rs);  /* the `count` operation: no download */
/* all rows, ascending id (what `remove` needs; what cdb_query_and_columns(ranked = 0) returns, after the corr filter) */
int cdb_rowset_rows(cdb_rowset* rs, int64_t** ids, int64_t** counts, size_t* nrows);
/* rows [first, last) of the ranking (interface.cpp:144-146, then `span`, :228-241).  last > size is clamped; first >= min(last, size)
 * gives zero rows.  From 2^22 rows on only the rows up to the end of the page are sorted: a radix select over the counts finds them.
 * Smaller sets key and sort all their rows, which measured faster there. */
int cdb_rowset_page(cdb_rowset* rs, uint64_t first, uint64_t last, int64_t** ids, int64_t** counts, size_t* nrows);
/* cluster (database.cpp:442-460) of the row set's ids by a string index / a column on the same GPU (another device: CDB_E_INVALID);
 * result rules of cdb_cluster / cdb_column_cluster; nothing is uploaded.  Errors are reported on the row set. */
int cdb_rowset_cluster(cdb_rowset* rs, cdb_index* field, int with_values, cdb_clusters* out);
int cdb_rowset_cluster_column(cdb_rowset* rs, cdb_column* field, cdb_clusters* out);
/* "rows", "page_selects", "page_sorts" (pages answered by either path; a page without rows runs neither), "select_passes" (key
 * bytes the last select visited), "page_ms", "clusters", "cluster_ms", "selects", "select_ms", "select_rows" (cdb_rowset_select),
 * "removes", "remove_fields", "remove_ms" (cdb_rowset_remove), "all_fields", "all_input_rows", "all_ms" (cdb_rowset_all) */
int cdb_rowset_get_stat(const cdb_rowset* rs, const char* name, double* value);
/* Test and measurement hooks — NOT part of the stable ABI: a row set over the caller's rows (ids ascending, taken as given);
 * options "debug_page_path" (0 automatic: select from 2^22 rows on; 1 select wherever the page ends before the last row; 2 always sort) and "profile" (the
 * page's kernels timed as pg_*, read as "name ms launches bytes" lines). */
int cdb_debug_rowset_from_rows(int device, const int64_t* ids, const int64_t* counts, uint64_t n, cdb_rowset** out);
int cdb_debug_rowset_set_option(cdb_rowset* rs, const char* name, int64_t value);
/* CDB_E_INVALID when the table does not fit cap bytes (buf then holds its NUL-terminated head) */
int cdb_debug_rowset_profile_dump(cdb_rowset* rs, char* buf, size_t cap);

/* Highlight spans — replaces the per-document re-scan of ac_automaton::render (database.cpp:58-76) that
 * select() runs for every returned object (database.cpp:394-441): for the keyword list of ONE string
 * key, every matching document's merged highlight spans [begin, end] (byte offsets, end inclusive), with
 * the reference's merge rule — overlapping keyword occurrences fuse, merely adjacent ones do not.
 * Documents ascend by insertion index; document r owns spans [span_ptr[r], span_ptr[r+1]).  The
 * occurrences come straight from the suffix-array ranges (offset = entry >> bits), no text is scanned. */
typedef struct cdb_spans {
    uint64_t ndocs, nspans;
    int64_t* ids;        /* ndocs */
    uint64_t* span_ptr;  /* ndocs + 1 */
    uint64_t* begin;     /* nspans */
    uint64_t* end;       /* nspans, inclusive */
} cdb_spans;
int cdb_query_spans(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, cdb_spans* out);
void cdb_spans_free(cdb_spans* r);

/* A page of result rows rendered on the device — the tail of select() (database.cpp:394-441): for the rows `ids` (the page that
 * `span` cut from the ranked list) and the keyword list of ONE string key, every row's document, its merged highlight spans and the
 * document with `left` / `right` put around them, as ac_automaton::render does (database.cpp:58-90).  Only the resident text of
 * those documents is read: the cost follows the page, not the corpus, and a caller that built from device memory (cdb_build_device,
 * cdb_build_resident, shards) needs no host copy of the column.  It is a text scan like the reference's highlighter, so it reports the
 * true occurrences whatever order the suffix array is in (reference_compat, bytes >= 0x80); the array is never read.
 *   Rows.  Output row i belongs to ids[i], in the caller's order (rank order, not id order); a repeated id is rendered as often as
 * it is given.  An id the index does not hold gets found[i] = 0, an empty string and no spans, and is counted in `missing`; an index
 * that was never built answers all rows missing (as cdb_cluster does).  nrows = 0 is valid.
 *   Keywords.  nkw = 0 returns the plain documents (select without highlight).  An empty keyword fails the call with CDB_E_INVALID
 * and "Empty keywords are not allowed", like every other keyword entry point.  There is no limit on the number or length of keywords.
 *   Occurrences.  A keyword of m bytes occurs at offset p of a document of L bytes iff p + m <= L and the bytes are equal;
 * occurrences never cross into the next document.
 *   Spans.  The union of all occurrences of the document: overlapping occurrences fuse, merely adjacent ones stay apart; `end` is
 * inclusive (the reference's pop / extend / append rule, database.cpp:62-77; the same spans as cdb_query_spans).
 *   Rendering.  `left` goes before byte `begin`, `right` after byte `end` (database.cpp:78-90); either may be empty, neither need be
 * text.  Row i's string is text_blob[text_ptr[i] .. text_ptr[i + 1]), its spans are [span_ptr[i], span_ptr[i + 1]).
 *   `what` selects the arrays filled (CDB_RENDER_TEXT | CDB_RENDER_SPANS); the others stay NULL.  `found` is always filled.
 * The call is a query: several host threads may call it on one handle, and it waits out a rebuild under the handle's lock.  Large
 * result arrays are pinned blocks of the result cache (below); release them with cdb_rendered_free.  Stats: "render_ms",
 * "render_page_bytes" (bytes of the found rows' documents), "render_spans"; with option profile the kernels are timed as rnd_*.
 * Documents of 4 GiB and more are refused.  One key per call: the reference keeps one automaton per key. */
#define CDB_RENDER_TEXT  1   /* fill text_ptr / text_blob */
#define CDB_RENDER_SPANS 2   /* fill span_ptr / begin / end */
typedef struct cdb_rendered {
    uint64_t nrows, missing, nspans, text_bytes;
    uint8_t*  found;      /* nrows: 1 = the index holds ids[i] */
    uint64_t* text_ptr;   /* nrows + 1 offsets into text_blob, or NULL */
    char*     text_blob;  /* rendered documents, concatenated in input order */
    uint64_t* span_ptr;   /* nrows + 1, or NULL */
    uint64_t* begin;      /* nspans, byte offsets inside the ORIGINAL document */
    uint64_t* end;        /* nspans, inclusive, as ac_automaton's spans */
} cdb_rendered;
int cdb_render_rows(cdb_index* h, const int64_t* ids, uint64_t nrows, const char* blob, const uint64_t* offsets, uint64_t nkw,
                    const char* left, size_t left_len, const char* right, size_t right_len, int what, cdb_rendered* out);
void cdb_rendered_free(cdb_rendered* r);

/* ---- select (select.hip) -------------------------------------------------------------------------------
 * The value of row `id` in a built column — replaces data[id][field] of select() for a numeric or bool field (database.cpp:406-409 with
 * keys, :413-415 without).  ids is in any order and may repeat; row i answers ids[i].  A row whose id the column does not hold gets
 * found[i] = 0 and values[i] = 0 and is counted in *missing (may be NULL); a column that was never built answers every row missing, as
 * cdb_column_cluster does; rows staged since the last build are not seen.  nrows = 0 is valid.  values[i] is what cdb_clusters.values
 * holds for a group: the int64, the double's bit pattern, or 0 / 1.
 * KNOWN DIVERGENCE: a double column folds -0.0 onto +0.0 when it is built (see cdb_column_cluster), so a row added as -0.0 reads +0.0.
 * The call is a query: it waits out a build under the column's lock.  With option profile the kernel is timed as sel_values. */
int cdb_column_values(cdb_column* c, const int64_t* ids, uint64_t nrows, uint64_t* values, uint8_t* found, uint64_t* missing);

/* A page of a row set with its fields in one call — replaces the tail of the `query` operation (interface.cpp:225-248: span, then
 * select(fields, highlight), database.cpp:394-441).  The page is cdb_rowset_page's in every respect: first / last, the clamping, the
 * signed ranking with ties ascending id, the automatic select / sort rule and the counters "page_selects" / "page_sorts".  Its ids stay
 * in device memory and every field is read where it lies; nfields = 0 is valid and is then cdb_rowset_page.
 *   Fields, in the caller's order; exactly one of index / shards / column is set (else CDB_E_INVALID).
 *   index: row i is what cdb_render_rows(index, page ids, keywords, left, right, CDB_RENDER_TEXT) returns — found and text; nkw = 0 gives
 * the plain document (a string field without constraints, database.cpp:400-405); an empty keyword fails the call with "Empty keywords
 * are not allowed".  Each string field has its own keyword list, as the reference keeps one automaton per key (database.cpp:396-399).
 *   shards: the same through cdb_shards_render_rows with the host copy of the page's ids.
 *   column: cdb_column_values of the page's ids; keywords on a column field are CDB_E_INVALID.  All column fields of a call are read by
 * one kernel launch and come back in one copy.
 *   An index or column on another GPU than the row set is CDB_E_INVALID, as for cdb_rowset_cluster.
 *   Result.  kind = 3 for a string field (the reference's tag), else the column's kind.  All arrays are host memory owned by the library
 * (pinned result cache when large; the values and found bytes of all column fields share ONE block): release with cdb_selected_free
 * only.  A failed call leaves *out zeroed and nothing allocated; errors are reported on the row set (cdb_rowset_last_error; a sharded
 * field's failure keeps its code and text).
 *   Locks.  The row set's lock is held for the whole call; the columns' locks are taken together in address order and released before
 * the string fields run, each of which takes its own handle's lock alone and waits out a rebuild as cdb_render_rows does.
 *   Stats (cdb_rowset_get_stat): "selects", and of the last call "select_ms", "select_rows"; with option profile the column kernel is
 * timed as sel_values next to the page's pg_*. */
typedef struct cdb_select_field {
    cdb_index*  index;    /* exactly one of index / shards / column is non-NULL */
    struct cdb_shards* shards;   /* (cdb_shards, declared with the sharded entry points below) */
    cdb_column* column;
    const char* kw_blob; const uint64_t* kw_offsets; uint64_t nkw;   /* string fields: keywords to highlight; 0 = plain document */
} cdb_select_field;
typedef struct cdb_selected_field {
    int kind;             /* 3 = string (the reference's tag), else the column's kind 0 / 1 / 2 */
    uint64_t missing;     /* rows of the page whose id the field does not hold */
    uint8_t*  found;      /* nrows */
    uint64_t* values;     /* columns: nrows raw values exactly as cdb_clusters.values (column_key_raw); strings: NULL */
    uint64_t* text_ptr;   /* strings: nrows + 1 offsets into text_blob; columns: NULL */
    char*     text_blob;
} cdb_selected_field;
typedef struct cdb_selected {
    uint64_t nrows; int nfields;
    int64_t* ids; int64_t* counts;        /* the page, as cdb_rowset_page returns it */
    cdb_selected_field* fields;           /* nfields, in the caller's order */
} cdb_selected;
int  cdb_rowset_select(cdb_rowset* rs, uint64_t first, uint64_t last, const cdb_select_field* fields, int nfields,
                       const char* left, size_t left_len, const char* right, size_t right_len, cdb_selected* out);
void cdb_selected_free(cdb_selected* r);

/* Documents leave a built index on the device, without a rebuild — replaces "remove + build" (interface.cpp:274-285,
 * database.cpp:461-466 followed by :170-282) for one string key.  The reference deletes the raw files and the objects stay visible until
 * the next build re-reads every file and rebuilds every index; here the resident text, tables and array are enough: suffixes never
 * cross documents, equal suffixes ascend by document and the survivors keep their order, so the survivors' array is the old one with the
 * removed documents' entries dropped and the rest re-encoded (remove.hip: a stable compaction, nothing but `ids` is uploaded).
 *   Result.  After a successful call the handle cannot be told from a fresh handle built over the surviving documents in their
 * original order: cdb_size / cdb_bits / cdb_mask / cdb_sa_width / cdb_sa_copy, every query entry point, cdb_cluster, cdb_render_rows,
 * cdb_save and the cdb_debug_verify* hooks.  The layout is recomputed with the build's own rule (index.cpp:182-208): bits, mask, the
 * entry width and the packed storage may all change.
 *   Counting.  *removed = distinct documents dropped; *missing = entries of `ids` the index does not hold — every such entry counts,
 * as cdb_cluster counts them; a held id given twice is removed once and is not missing (either pointer may be NULL).  nids = 0 is
 * valid and changes nothing.  On a handle that was never built every id is missing.  Removing every document leaves what cdb_build
 * leaves for an empty column.
 *   Pending additions.  If documents were added since the last build the call fails with CDB_E_INVALID and "remove: documents were
 * added since the last build"; nothing changes.  A host staging copy that equals the built column is dropped (cdb_add* fetch the
 * survivors back on demand: "remove, add, rebuild" works).
 *   Borrowed text.  For a handle built with cdb_build_device / cdb_build_resident the compacted text goes into a library-owned block:
 * after a removal that dropped at least one document the handle NO LONGER READS THE CALLER'S BUFFER.
 *   Locking and failure.  The call is exclusive, like a build: queries wait under the handle's lock.  Everything new is made in fresh
 * blocks while the old index stands; a failure before the commit leaves the old index serving (cdb_last_error tells why).
 *   Paths.  A sorted array (pure ASCII text, or reference_compat = 0) is compacted, and its search keys with it.  An array in the
 * reference's order (reference_compat = 1 and bytes >= 0x80) depends on bucket sizes that change with n (index.cpp:96-126,218): there
 * text and tables are compacted on the device and the array is built over them — a failure of that build leaves a "never built"
 * handle, as after any failed build.  With self_check >= 3 the order proof runs behind either path; damage found in a compacted
 * array is treated like damage behind a build.
 *   Stats: "removes" (calls that dropped something), "remove_compactions", "remove_rebuilds", and of the last such call "remove_docs",
 * "remove_bytes" (text bytes dropped), "remove_ms" (wall, under the lock); with option profile the kernels are timed as rm_*.
 * A sharded string column removes with cdb_shards_remove. */
int cdb_remove(cdb_index* h, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing);
/* The same for a column, with the same counting rules.  The result equals a fresh column built from the surviving rows; a failure
 * leaves the column as it was.
 *   Paths.  With no rows staged since the last build the four arrays are compacted on the device (column_maintain.hip): only `ids`
 * is uploaded, one lane per id marks its row in id order and in value order, both orders are compacted stably (stable_tiles.h) and
 * the positions follow through one gather; fresh blocks are published as a build publishes them.  With staged rows the rows leave
 * the built and the staged rows alike on the host path: the built rows are downloaded, filtered with the staged ones and the
 * column's own build runs over the rest.  Option "debug_maintain_path" (cdb_debug_column_set_option) = 2 forces the host path.
 *   Stats: "removes" (calls that dropped something), "remove_compactions" (device path), "remove_rebuilds" (host path), and of the
 * last such call "remove_rows" and "remove_ms" (wall, under the lock); with option profile the kernels are timed as col_rm_*. */
int cdb_column_remove(cdb_column* c, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing);

/* Rows join a built column on the device, without sorting the old rows again — "insert ... build" for a numeric or bool field.
 * values is as for cdb_column_add_bulk (uint8_t / int64_t / double by kind); NaN is refused ("cdb_column_append: NaN is not a valid
 * value (row i)").  Only the new rows are uploaded and sorted; they are ranked against the old (value, id) order and the old id order
 * by binary search and merged in stably (column_maintain.hip).  A new bool row lands behind every old row of its value.
 *   Result.  After a successful call the column cannot be told from one that got the same rows by cdb_column_add_bulk +
 * cdb_column_build: every query entry point, cdb_column_cluster, cdb_query_and_columns, cdb_filter, the stats "rows" and "kind";
 * the device arrays are equal bit for bit.  *appended (may be NULL) = n.
 *   Edges.  n = 0 is valid and changes nothing.  On a column that was never built, or holds no rows, the call is the build of the
 * batch.  An id the column already holds, or one given twice in the batch, is refused with CDB_E_INVALID and "cdb_column_append:
 * duplicate object id N in one column"; more than 2^32 - 1 rows in all are refused before anything is touched.  With n > 0 neither
 * ids nor values may be NULL (CDB_E_INVALID).
 *   Pending additions.  Rows staged with cdb_column_add_bulk and not yet built make the call fail with CDB_E_INVALID and "append:
 * rows were added since the last build"; nothing changes.
 *   Locking and failure.  The call is exclusive, like a build.  Everything new is made in fresh blocks while the old arrays stand;
 * a failure leaves the old column serving (cdb_column_last_error tells why).
 *   Paths.  "debug_maintain_path" = 2 stages the rows and runs the column's own build over old and new rows (the path of
 * cdb_column_add_bulk + cdb_column_build); 0 and 1 merge wherever the column holds rows.
 *   Stats: "appends", "append_merges", "append_rebuilds" (the build of the batch, and path 2), "append_id_concat" (merges whose new
 * ids all exceeded the old ones: the id order was a concatenation), and of the last call "append_rows", "append_ms" (wall, under
 * the lock); with option profile the kernels are timed as col_ap_*. */
int cdb_column_append(cdb_column* c, const int64_t* ids, const void* values, uint64_t n, uint64_t* appended);
/* Test hook, NOT part of the stable ABI: the four device arrays of a built column (keys_v u64, ids_v i64, id_sorted i64, vpos u32;
 * "rows" entries each, any pointer may be NULL) copied to the host. */
int cdb_debug_column_arrays(cdb_column* c, uint64_t* keys_v, int64_t* ids_v, int64_t* id_sorted, uint32_t* vpos);

/* ---- row sets that change and span the database (rowset_maintain.hip) ----------------------------------------
 * cdb_rowset_remove — replaces the `remove` operation (interface.cpp:274-285: filter(), then database::remove of every row, :283 returns
 * their number) for all fields of the objects at once.  The rows of the set leave every field given, ALL OR NONE: the ids are the set's
 * own device array (nothing is downloaded, nothing uploaded), every field prepares its new column beside the serving one, and only
 * when every field stands does any commit.  Before, the rows had to come down with cdb_rowset_rows and go up again once per field
 * through cdb_remove / cdb_column_remove, and a failure in field 3 of 5 left fields 1 and 2 without the objects for good.
 *   Fields.  Exactly one of index / column is set in every entry; nfields >= 1; no handle twice; every field on the set's GPU.
 *   Results.  *rows (may be NULL) = the set's size, the count the reference returns.  Per field, removed / missing follow the rules of
 * cdb_remove / cdb_column_remove; a set holds each id once, so removed + missing == *rows.  A field that was never built, or built
 * over nothing, holds no id: missing = *rows, status CDB_OK, committed = 0 — as for any field that loses nothing.  An empty set
 * changes nothing and counts no call in any field.  After a successful call every field cannot be told from one that lost the same
 * ids through its own entry point, stats included ("removes", "remove_compactions" / "remove_rebuilds", ...).
 *   Order of the call.  A cdb_reserve still running is waited for; the row set's lock; every field's lock together in address order
 * (cdb_filter's rule, so a concurrent cdb_filter over the same fields cannot invert it); validation; every field PREPARES, one after
 * another in the caller's order; every field commits; unlock.  Queries on the fields wait, as during cdb_remove.
 *   Refused as a whole with CDB_E_INVALID before any device work: a field entry with none or both pointers set, nfields < 1, the same
 * handle twice (these three like a NULL argument: the code alone, before any handle is read), a field on another GPU ("cdb_rowset_remove: the field lives on another GPU"), a column with rows staged since its last
 * build ("remove: rows were added since the last build"), an index with pending additions ("remove: documents were added since the
 * last build").  The column option debug_maintain_path is not consulted: this call has only the device path.
 *   A failure in a prepare.  The call returns that field's code (the first in the caller's order; the prepares behind it do not run),
 * cdb_rowset_last_error says "field <i>: <message>", that field's status carries the code, every committed and every removed / missing
 * is 0, every prepared column is dropped and every field answers exactly as before.
 *   One step can still fail behind the commit point: on the reference-order path (reference_compat = 1 and bytes >= 0x80, see
 * cdb_remove "Paths") the array is built over the compacted text AFTER the field's commit.  The single-handle rule then applies per
 * field.  What a caller finds after such a failure: the call returns the failing field's error; that field is "never built" (it
 * answers {} and holds no document: the documents it served are gone from the column), its status carries the code and its
 * committed is 1; every other field has committed its change.  The database is consistent and answers every query, but that field is
 * neither the old nor the new one: rebuild it from the source.
 *   Memory.  At the peak every field's new column stands beside its old one AT THE SAME TIME (the per-field calls hold one pair at a
 * time).  A caller short of memory gets CDB_E_DEVICE and an unchanged database — that is the point of the call.
 *   The row set itself is left as it is.  Its ids are simply no longer held by the fields: a later cdb_rowset_select finds nothing,
 * a later cluster reports them missing.
 *   Sharded string columns stay out: use cdb_rowset_rows + cdb_shards_remove as before.
 *   Stats (cdb_rowset_get_stat): "removes" (calls that reached the commit), and of the last one "remove_fields", "remove_ms".
 *   Test hook, NOT part of the stable ABI (beside debug_fail_build): option "debug_fail_prepare" of cdb_set_option and
 * cdb_debug_column_set_option makes the prepare half of a removal from that field throw a device error after its device work has been
 * queued and its blocks allocated, so that the release path runs. */
typedef struct cdb_remove_field {
    cdb_index*  index;      /* a string field, or NULL            — exactly one of the two */
    cdb_column* column;     /* a numeric / bool field, or NULL                              */
    uint64_t    removed;    /* out: rows of the set the field held and lost                 */
    uint64_t    missing;    /* out: rows of the set the field did not hold                  */
    int32_t     status;     /* out: CDB_OK, or the code of the failure that arose in this field */
    int32_t     committed;  /* out: 1 = the field's old column no longer serves             */
} cdb_remove_field;
int cdb_rowset_remove(cdb_rowset* rs, cdb_remove_field* fields, int nfields, uint64_t* rows);
/* cdb_rowset_all — the row set of every object: replaces query() of database.cpp:380-386 (every object with count 0), which filter()
 * returns for a request without constraints (interface.cpp:51-53; README: "You can get all objects in the database by omitting
 * `constraints`"; `count` without constraints is the size of the database).  "Every object" is the union of the ids the given fields
 * hold: database.cpp:170-282 stores data[id][key] and calls add(id, value) side by side, so the union over all fields of a database is
 * its object store.  Rows ascend by id as SIGNED int64, each id once, every count 0; the set owns its arrays as cdb_filter's does, and
 * cdb_rowset_size / _page / _select / _cluster* / _remove work over it unchanged.  A page of it is the ids [first, last) in ascending
 * order (all counts equal, ties ascending id).
 *   Only built rows count, as for every query.  A field that was never built contributes nothing; all fields never built give a valid
 * set of size 0.  nindexes + ncolumns < 1, a null entry, and fields on different GPUs ("cdb_rowset_all: all fields must live on one
 * GPU") are CDB_E_INVALID; errors before a set exists are reported where cdb_filter reports them: on the first index's handle, or
 * without one on the first column's.  Every field's lock is held, in address order, while its ids are read.
 *   How.  The fields' ascending id lists (an index's id table, a column's id order) are laid end to end keyed id ^ 2^63, sorted key-only
 * (one list alone is not sorted) and compacted to the first of every run of equal keys (stable_tiles.h); 16 bytes of scratch per listed
 * id.  Stats: "all_fields", "all_input_rows" (ids listed by all fields together), "all_ms"; when the lead handle's option profile is on,
 * the set's profile (cdb_debug_rowset_profile_dump) holds the kernels as all_* lines.  Sharded string columns stay out. */
int cdb_rowset_all(cdb_index* const* indexes, int nindexes, cdb_column* const* columns, int ncolumns, cdb_rowset** out);

/* Documents join a built index on the device, without a rebuild — replaces "insert ... build" (interface.cpp:157-180, :286-288, and
 * database.cpp:276-280, which constructs the next generation beside the serving one) for one string key.  The arguments are those of
 * cdb_build_view: doc_start[ndocs + 1] holds non-decreasing offsets into `blob`.  Suffixes never cross documents, so the old suffixes
 * keep their mutual order and the new ones get theirs from a build over the new documents alone; equal suffixes ascend by document and
 * every new document is numbered behind every old one.  The array over "old documents, then new documents" is therefore the stable
 * merge of the old array and the new documents' array, ties old first (append.hip: only the new documents are uploaded and sorted).
 *   Result.  After a successful call the handle cannot be told from a fresh handle built over the old documents in their order
 * followed by the new ones in theirs: cdb_size / cdb_bits / cdb_mask / cdb_sa_width / cdb_sa_copy, every query entry point, cdb_cluster,
 * cdb_render_rows, cdb_save and the cdb_debug_verify* hooks.
 *   Layout.  It is recomputed with the build's own rule (index.cpp:182-208; the longest document is the maximum of old and new): bits,
 * mask, the entry width and the packed storage may all grow.
 *   Capacity.  The reference's capacity errors (index.cpp:195-200) can fire; they fire before anything is touched, and the old index
 * goes on serving.
 *   Edges.  ndocs = 0 is valid and changes nothing.  On a handle that was never built, or was built over nothing, the call is
 * cdb_build_view of the given documents.  Ids are assumed unique, as everywhere: there is no check.  *appended (may be NULL) = the
 * number of documents that joined.  With ndocs > 0 none of ids, blob and doc_start may be NULL (CDB_E_INVALID).
 *   Pending additions.  If documents were staged with cdb_add* since the last build the call fails with CDB_E_INVALID and "append:
 * documents were added since the last build"; nothing changes.  A host staging copy that equals the built column is dropped (cdb_add*
 * and cdb_save fetch the column back on demand).
 *   Borrowed text.  Old and new text go into one library-owned padded block (a device copy of the old bytes, a chunked upload of the
 * new ones): after an append that added at least one document a cdb_build_device / cdb_build_resident handle NO LONGER READS THE
 * CALLER'S BUFFER.
 *   Locking and failure.  The call is exclusive, like a build: queries wait under the handle's lock.  Everything new is made in fresh
 * blocks while the old index stands; a failure before the commit leaves the old index serving (cdb_last_error tells why).
 *   Paths.  The merge runs only where the fresh array would be globally sorted: reference_compat = 0, or the old array is sorted and
 * the new text holds no byte >= 0x80.  Otherwise the array is in the reference's order, which depends on bucket sizes max(4096, n / 256)
 * (index.cpp:96-126,218): text and tables are extended on the device and the array is built over them — only there a failed build
 * leaves a "never built" handle, as after any failed build.  With self_check >= 3 the order proof runs behind either path; damage
 * found in a merged array is treated like damage behind a build.  Option "debug_append_path" (test hook): 0 = automatic, 1 = merge
 * where it is valid, 2 = always rebuild.
 *   Search keys.  Where the handle keeps search keys and its symbol map codes every byte of the new text, the new suffixes' keys are
 * computed under that map and merged with the old ones ("append_keys_kept" = 1).  New text with a byte the old text never held is
 * installed without keys, as after cdb_load ("append_keys_kept" = 0): queries stay exact, lone keywords lose the key shortcut until
 * the next build.
 *   Stats: "appends" (calls that added something), "append_merges", "append_rebuilds", and of the last such call "append_docs",
 * "append_bytes" (text bytes added), "append_ms" (wall, under the lock), "append_keys_kept"; with option profile the kernels are
 * timed as ap_*.
 * A sharded string column appends with cdb_shards_append. */
int cdb_append(cdb_index* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs, uint64_t* appended);

/* ---- objects join every field at once (insert.hip) --------------------------------------------------------------
 * cdb_insert_objects — replaces "insert ... build" (interface.cpp:157-180, :286-288; database.cpp:283-379, then :170-282) for all
 * fields of the objects at once, the counterpart of cdb_rowset_remove.  The objects join every field given, ALL OR NONE: every field
 * prepares its new column beside the serving one, and only when every field stands does any commit.  Before, an object with five
 * fields took five calls of cdb_append / cdb_column_append, and a failure in field 3 of 5 left fields 1 and 2 with the objects and
 * the others without them for good.
 *   Arguments.  ids[nobjects]: one id per object (the reference has one timestamp per insert).  Field k receives the pairs
 * (ids[rows[j]], value j), j < nrows: `rows` are strictly ascending indices into ids[], or NULL = every object (nrows == nobjects).
 * A string field's documents are blob / doc_start[nrows + 1] as for cdb_append, a column's values are `values` as for
 * cdb_column_append (by kind).  nrows = 0 is valid: the field takes part in the id check and the locks only.  Exactly one of index /
 * column is set in every entry; nfields >= 1; no handle twice; every field on one GPU.
 *   Results.  *inserted (may be NULL) = nobjects.  Per field, appended = the rows that joined it.  nobjects = 0 is valid, changes
 * nothing and counts no call in any field.  After a successful call every field cannot be told from one that received the same rows
 * through its own cdb_append / cdb_column_append, the counting stats included ("appends", "append_merges" / "append_rebuilds",
 * "append_docs" / "append_rows", ...): a field that was never built, or holds nothing, is built over its rows of the batch.  The TIME
 * stats differ: a field's "append_ms" (and a column's "build_ms" on the build path) runs from its own prepare to its own commit, and
 * every commit comes behind every prepare, so it includes the prepares of the fields behind it in the call.
 *   Order of the call.  A cdb_reserve still running is waited for; every field's lock together in address order (cdb_filter's rule);
 * validation; the id check on the device; every field with rows PREPARES, one after another in the caller's order; every field
 * commits; unlock.  Queries on the fields wait, as during cdb_append.
 *   Refused as a whole with CDB_E_INVALID before any device work: nfields < 1 or > 65535, fields NULL, a field entry with none or both pointers
 * set, the same handle twice, ids NULL with nobjects > 0, a field with nrows > 0 that lacks its payload pointers (blob and doc_start,
 * or values), rows NULL with nrows != nobjects (these like a NULL argument: the code alone, before any handle is read); fields on
 * different GPUs ("cdb_insert_objects: all fields must live on one GPU"), an index or a column with pending additions ("append:
 * documents / rows were added since the last build"), rows not strictly ascending or >= nobjects, an object that no field lists
 * ("cdb_insert_objects: object <i> holds no field": the reference's "Empty objects are not allowed", database.cpp:284-286), NaN in a
 * double field and the column row limit (cdb_column_append's messages).  The column option debug_maintain_path is not consulted:
 * this call has only the device path.
 *   The id check (CDB_E_INVALID, nothing changed).  No id may stand twice in ids[] ("cdb_insert_objects: object id N twice in the
 * batch", N the smallest such id), and no id of the batch may be held by any field given, whether the object lists that field or not
 * ("cdb_insert_objects: object id N is already held by field <k>": N the smallest such id as a signed number, k the first field in
 * the caller's order that holds it).  ONE STATED DIVERGENCE: the reference overwrites raw/<id>, so inserting an id again replaces
 * the object at the next build; here a replace is cdb_rowset_remove followed by this call.  Only built rows count, as for every query.
 *   A failure in a prepare.  The call returns that field's code (the first in the caller's order; the prepares behind it do not run),
 * the error text says "field <i>: <message>", that field's status carries the code, every committed and every appended is 0, every
 * prepared column is dropped and every field answers exactly as before.
 *   One step can still fail behind the commit point: on the reference-order path (reference_compat = 1 and bytes >= 0x80, see
 * cdb_append "Paths"), and for a string field that held nothing, the array is built over the new text AFTER the field's commit.  The
 * single-handle rule then applies per field.  What a caller finds after such a failure: the call returns the failing field's error;
 * that field is "never built" (it answers {} and holds no document: the documents it served are gone from the column), its status
 * carries the code and its committed is 1; every other field has committed its change.  The database is consistent and answers every
 * query, but that field is neither the old nor the new one: rebuild it from the source.
 *   Memory.  At the peak every field's new column stands beside its old one AT THE SAME TIME (the per-field calls hold one pair at a
 * time).  In front of that the id check holds 24 bytes per object on the first field's GPU (the ids, their keys and the sort's second
 * buffer), 8 bytes per 4096 objects of tile counts and bases, and the radix sort's work space that the first field's handle keeps across
 * calls; the check's blocks are released before the first prepare.  A caller short of memory gets CDB_E_DEVICE and an unchanged database.
 *   Errors are reported where cdb_rowset_all reports them: on the FIRST field's handle (cdb_last_error / cdb_column_last_error).
 *   Sharded string columns stay out: use cdb_shards_append for them as before.
 *   Stats live on that first field's handle too and are read with cdb_insert_get_stat(index, column, ...), exactly one of the two
 * set: "inserts" (calls that reached the commit), and of the last one "insert_fields", "insert_objects", "insert_ms".  With the first
 * field's option profile on, its profile holds the id check's kernels as ins_* lines.
 *   Test hook, NOT part of the stable ABI (beside debug_fail_prepare): option "debug_fail_append_prepare" of cdb_set_option and
 * cdb_debug_column_set_option makes the prepare half of an append to that field throw a device error after its device work has been
 * queued and its blocks allocated, so that the release path runs. */
typedef struct cdb_insert_field {
    cdb_index*      index;      /* a string field, or NULL            — exactly one of the two          */
    cdb_column*     column;     /* a numeric / bool field, or NULL                                       */
    const uint64_t* rows;       /* which objects of the batch hold this field: strictly ascending indices
                                   into ids[], nrows of them; NULL = every object (nrows == nobjects)   */
    uint64_t        nrows;      /* 0 is valid: the field takes part in the id check and the locks only   */
    const char*     blob;       /* string field: the documents, as for cdb_append ...                    */
    const uint64_t* doc_start;  /* ... doc_start[nrows + 1]                                              */
    const void*     values;     /* column field: nrows values, as for cdb_column_append (by kind)        */
    uint64_t        appended;   /* out: rows that joined this field                                      */
    int32_t         status;     /* out: CDB_OK, or the code of the failure that arose in this field      */
    int32_t         committed;  /* out: 1 = the field's old column no longer serves                      */
} cdb_insert_field;
int cdb_insert_objects(const int64_t* ids, uint64_t nobjects, cdb_insert_field* fields, int nfields, uint64_t* inserted);
int cdb_insert_get_stat(const cdb_index* index, const cdb_column* column, const char* name, double* value);

/* Batched query with patterns and results left in device memory (multi-GPU merge over RCCL, HBM-
 * resident timing).  d_blob/d_offsets are device pointers.  On return the library-owned device arrays
 * d_row_ptr (npat+1 u64), d_ids (nrows i64), d_counts (nrows i64) stay valid until the next query on
 * this handle or cdb_destroy.  The offsets are not pre-validated on the host: an empty pattern yields zero
 * rows here (the host entry points reject it like the reference does). */
typedef struct cdb_device_result {
    uint64_t npat, nrows, nhits;
    const uint64_t* d_row_ptr;
    const int64_t* d_ids;
    const int64_t* d_counts;
} cdb_device_result;
int cdb_query_batch_device(cdb_index* h, const void* d_blob, const uint64_t* d_offsets, uint64_t npat,
                           uint64_t blob_bytes, cdb_device_result* out);

/* The same with occurrence offsets (cdb_query_batch_offsets), everything left in device memory: d_hit_ptr
 * (nrows + 1 u64) and d_offsets (nhits u64) are library-owned like the arrays of cdb_device_result. */
typedef struct cdb_device_hits {
    const uint64_t* d_hit_ptr;
    const uint64_t* d_offsets;
} cdb_device_hits;
int cdb_query_batch_offsets_device(cdb_index* h, const void* d_blob, const uint64_t* d_offsets, uint64_t npat,
                                   uint64_t blob_bytes, cdb_device_result* out, cdb_device_hits* hits);

/* ---- several GPUs: document-aligned shards (no reference counterpart: the reference is one process on one host) ----
 * Suffixes never cross documents (src/index.h:61-65) and a result row belongs to one document (src/index.cpp:317-321),
 * so a column splits into document-aligned byte ranges, one independent suffix array per GPU.  Every shard answers
 * the whole pattern batch; the per-shard match lists are merged on the devices: all-gather of the row counts, one scan,
 * all-gatherv of the rows over RCCL / xGMI (grouped broadcasts, every peer one hop away), a placement kernel — rows of a
 * pattern stay ascending in document order because shards are document ranges.
 *
 * cdb_shards: ONE process owning several GPUs — what replaces string_index when the column exceeds one GPU (the shim
 * switches to it).  Same surface as cdb_index: add / build / query / query_batch.  build() spreads the
 * column over as many devices as max_shard_bytes requires (option "max_shard_bytes", default 12 GiB per GPU;
 * "use_all_devices" = 1 spreads over all of them regardless); other options are forwarded to every shard. */
typedef struct cdb_shards cdb_shards;
int cdb_shards_create(cdb_shards** out, const int* devices, int ndev); /* devices may repeat (tests on a one-GPU box) */
void cdb_shards_destroy(cdb_shards* h);
const char* cdb_shards_last_error(const cdb_shards* h);
int cdb_shards_add(cdb_shards* h, int64_t id, const char* value, size_t len);                 /* index.cpp:174-177 */
int cdb_shards_add_bulk(cdb_shards* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs);
int cdb_shards_set_option(cdb_shards* h, const char* name, int64_t value);
int cdb_shards_build(cdb_shards* h);                                                           /* index.cpp:178-236 */
/* build straight from the caller's separate strings (cdb_build_views per shard; replaces whatever cdb_shards_add* staged) */
int cdb_shards_build_views(cdb_shards* h, const int64_t* ids, const char* const* ptrs, const uint64_t* lens, uint64_t ndocs);
int cdb_shards_query(cdb_shards* h, const char* keyword, size_t len, int64_t** ids, int64_t** counts, size_t* nrows);
int cdb_shards_query_batch(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out);
/* cdb_query_or / cdb_query_ranked / cdb_query_spans over all shards (object ids are disjoint across shards: the shard
 * answers are concatenated and ordered the way the single-GPU calls order them) */
int cdb_shards_query_or(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t** ids, int64_t** counts,
                        size_t* nrows);
int cdb_shards_query_ranked(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t corr_lo, int64_t corr_hi,
                            uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows);
int cdb_shards_query_spans(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, cdb_spans* out);
/* cdb_render_rows over all shards: every shard renders the rows it holds, the answers are put back into the caller's row order; a
 * row no shard holds is missing */
int cdb_shards_render_rows(cdb_shards* h, const int64_t* ids, uint64_t nrows, const char* blob, const uint64_t* offsets, uint64_t nkw,
                           const char* left, size_t left_len, const char* right, size_t right_len, int what, cdb_rendered* out);
/* cdb_query_batch_offsets over all shards (occurrence offsets are relative to their document, so they need no re-basing) */
int cdb_shards_query_batch_offsets(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out,
                                   cdb_hits* hits);
/* AND across keys (interface.cpp:114-146) with sharded string keys: a key is a sharded column + its keyword list, or a
 * row list resolved elsewhere (shards = NULL), exactly like cdb_key_query.  Different columns are cut at different
 * documents, so every sharded key is first resolved with its own OR over its shards; the row lists then meet in one device
 * merge (on the first shard of the first sharded key).  Same result rules as cdb_query_and. */
typedef struct cdb_shards_key_query {
    cdb_shards* shards;      /* sharded string key, or NULL */
    const char* blob;
    const uint64_t* offsets;
    uint64_t nkw;
    const int64_t* ids;      /* shards == NULL: host rows */
    const int64_t* counts;
    size_t nrows;
} cdb_shards_key_query;
int cdb_shards_query_and(const cdb_shards_key_query* keys, int nkeys, int ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit,
                         int64_t** ids, int64_t** counts, size_t* nrows);
/* raw-file ingest into the sharded column (cdb_add_raw_dir, database.cpp:170-275) and persistence (cdb_save / cdb_load per
 * shard: `path` holds the shard count and document bounds, `path.<i>` shard i's file).  Loading replaces the column;
 * a failed load leaves the serving shards untouched. */
int cdb_shards_add_raw_dir(cdb_shards* h, const char* dir, const char* key, uint64_t* records, uint64_t* added);
int cdb_shards_save(cdb_shards* h, const char* path);
int cdb_shards_load(cdb_shards* h, const char* path);
/* cdb_remove, cdb_append and cdb_cluster for the sharded column.  Arguments, NULL rules, error codes and messages are those of the
 * single-handle calls; errors are read with cdb_shards_last_error, and a shard's failure keeps its own code and text.
 *   The contract.  After a successful call every cdb_shards_* query entry point (query, query_batch and query_batch_offsets with the
 * host merge and with device_merge = 1, query_or, query_ranked, query_and, query_spans, render_rows, cluster, save followed by load)
 * answers as ONE cdb_index over the same documents in the same order would: the survivors in their original order after a remove,
 * the old documents and then the new ones after an append.  It is about answers, not about where the cuts lie: a fresh
 * cdb_shards_build of the same documents may cut them differently.  One limit, which a plain cdb_shards_build shares: where the
 * arrays are in the reference's order (reference_compat = 1 and bytes >= 0x80) the answers follow the reference's own search over
 * each array, and above its bucket size (4096 suffixes, index.cpp:218) they depend on how many suffixes ONE array holds — there a
 * sharded set and a single index differ even when both were just built, and what holds is that every shard equals a fresh index
 * over its own documents.
 *   All or nothing.  Both writers hold the set exclusively (queries wait, as during the swap of a build) and the locks of the shards
 * they touch.  Every shard first PREPARES its new column beside the serving one; if any shard fails there, every prepared column is
 * dropped, the call returns that shard's error and the old column goes on serving on every shard.  Only when all stand does every
 * shard commit.  One step can still fail behind the commit point: on the reference-order path (reference_compat = 1 and bytes >= 0x80,
 * see cdb_remove / cdb_append "Paths") and for an append into a shard that holds nothing, the array is built over the new text AFTER
 * the shard's commit.  The single-handle rule then applies per shard.  What a caller finds after such a failure: the call returns the
 * failing shard's error; that shard is "never built" (it answers {} and holds no document: the documents it served are gone from the
 * column); every other shard has committed its change; cdb_shards_count is unchanged and cdb_shards_first_doc describes exactly the
 * documents that are still served; the host staging copy is dropped.  The column is consistent and answers every query, but it is
 * neither the old nor the new one: rebuild it from the source.
 *   Pending additions.  Documents staged with cdb_shards_add* since the last build or load make remove and append fail with
 * CDB_E_INVALID and cdb_remove's / cdb_append's message ("remove: / append: documents were added since the last build"); nothing
 * changes.  After a call that changed the column the ONE host staging copy is dropped; cdb_shards_add* and cdb_shards_build fetch the
 * column back from the shards on demand, so "remove, add, rebuild" works.
 *
 * cdb_shards_remove.  Every shard removes the ids it holds (cdb_remove's paths, the shards in parallel).  *removed is the sum over the
 * shards; *missing is the number of entries of `ids` that no shard holds (a held id given twice is removed once and is not missing).
 * The document bounds are recomputed from the shards' surviving documents and cdb_shards_first_doc follows.  A shard that loses all
 * its documents STAYS IN PLACE, empty: cdb_shards_count does not change, nothing is re-cut, and every query path (the device merge
 * included) answers correctly with an empty shard in the middle or at either end.  nids = 0 changes nothing; a set that was never
 * built answers every id missing; removing every document leaves a column that answers like an empty one.  Per-shard stats
 * ("removes", "remove_compactions", ...) are read through cdb_shards_get.
 *
 * cdb_shards_append.  The new documents are numbered behind all old ones, so they go to the end of the column.  If no shard is in use
 * the call is cdb_shards_build_views over the given documents.  Otherwise, if the last shard in use stays within max_shard_bytes with
 * the new bytes, or no idle device slot is left (as the initial build lets its last shards grow once all devices are in use), they
 * join that shard through cdb_append.  Otherwise the last shard stays as it is: the new documents are cut at document boundaries into
 * pieces of at most max_shard_bytes (a lone larger document is its own piece; when the slots run out the last slot takes the rest)
 * and built on the next idle slots — cdb_shards_count grows, and the merge ranks and the transport are remade for the new count.
 * The options set so far reach the new shards.  ndocs = 0 changes nothing; the reference's capacity errors fire before anything is
 * touched.  *appended (may be NULL) = the documents that joined.
 *
 * cdb_shards_cluster.  A query (it runs beside other queries).  Every shard clusters the rows it holds; the per-shard group lists,
 * each in std::string order whatever reference_compat is, are merged on the host (csrc/cluster_merge.h): groups with equal strings
 * fuse, their counts add, rep_id is the minimum; missing = rows no shard holds; sum(counts) + missing == nrows always.  The strings are
 * fetched from every shard even with with_values = 0 (the merge compares them); value_ptr / value_blob are then NULL.  `values` is
 * always NULL.  nrows = 0 and a set that was never built behave as in cdb_cluster.  Release the result with cdb_clusters_free. */
int cdb_shards_remove(cdb_shards* h, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing);
int cdb_shards_append(cdb_shards* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs, uint64_t* appended);
int cdb_shards_cluster(cdb_shards* h, const int64_t* ids, uint64_t nrows, int with_values, cdb_clusters* out);
/* introspection: shards in use after build, the handle of shard i (per-shard parity: its suffix array is that of its
 * documents alone), its first document, and how the shards exchange ("rccl" / "device copies" / "none") */
int cdb_shards_count(const cdb_shards* h);
cdb_index* cdb_shards_get(cdb_shards* h, int i);
uint64_t cdb_shards_first_doc(const cdb_shards* h, int i);
const char* cdb_shards_transport(const cdb_shards* h);

/* cdb_comm: one process per GPU (bench.py under torchrun; MPI-style services).  Rank 0 draws a 128-byte id
 * (ncclGetUniqueId) and distributes it by whatever means the processes share; every rank then creates its communicator
 * (ncclCommInitRank) and merges its shard's device-resident result with the others' — a collective call.  On return
 * `merged` (identical on every rank) points to device arrays owned by the communicator, valid until its next merge. */
typedef struct cdb_comm cdb_comm;
int cdb_comm_unique_id(void* id128);
int cdb_comm_create(cdb_comm** out, const void* id128, int rank, int world, int device);
/* The same communicator for ranks that live in ONE process (a host thread per rank calls the collectives): out[world]
 * receives one handle per rank, rank i on devices[i].  Distinct devices exchange over RCCL (ncclCommInitAll); ranks that
 * share a device — e.g. BASELINE config 3's four 8 GiB shards co-resident on one MI355X — through device-to-device copies
 * (cdb_comm_transport says which).  Destroy every handle with cdb_comm_destroy. */
int cdb_comm_create_group(cdb_comm** out, int world, const int* devices);
void cdb_comm_destroy(cdb_comm* c);
const char* cdb_comm_last_error(const cdb_comm* c);
int cdb_comm_merge(cdb_comm* c, const cdb_device_result* local, cdb_device_result* merged);
/* Counts-only merge for consumers that keep (or download) their own slice — SURVEY §8e: when the consumer is not on the
 * GPU "each GPU D2H's its slice".  Collective; exchanges nothing but the per-pattern row counts (npat x u32 per rank).
 * Every rank learns the merged row_ptr and, per pattern, where ITS rows start in the merged row stream:
 * merged rows [d_row_base[j], d_row_base[j] + local count of j) are this rank's rows of pattern j, in order.  No rank holds
 * another rank's rows (the full all-gatherv of C4 — 10^7 patterns x 8 shards — would put ~10^9 rows on every GPU). */
typedef struct cdb_shard_slice {
    uint64_t npat, nrows_total, nrows_local;
    const uint64_t* d_row_ptr;   /* npat + 1, merged, identical on every rank; device memory owned by the communicator */
    const uint64_t* d_row_base;  /* npat, this rank's first merged row of every pattern */
} cdb_shard_slice;
int cdb_comm_merge_counts(cdb_comm* c, const cdb_device_result* local, cdb_shard_slice* out);
int cdb_comm_world(const cdb_comm* c);
const char* cdb_comm_transport(const cdb_comm* c);

/* ---- introspection (parity tests; mirrors the private members src/index.h:56-60) -------------- */
uint64_t cdb_size(const cdb_index* h);  /* number of suffixes = text bytes */
uint64_t cdb_bits(const cdb_index* h);  /* doc-index bits of an entry */
uint64_t cdb_mask(const cdb_index* h);
int cdb_sa_width(const cdb_index* h);   /* 4 or 8 bytes per entry; 0 before build */
/* copies the suffix array ((offset << bits) | doc entries, cdb_sa_width bytes each) to host memory */
int cdb_sa_copy(cdb_index* h, void* host_out, uint64_t capacity_bytes);

/* ---- options & measurements -------------------------------------------------------------------- */
/* name: "profile" (0/1: time kernels with HIP events), "reference_compat" (default 1: reproduce the
 * reference's signed-char bucket order for text with bytes >= 0x80 — SURVEY.md Q2 — so that the suffix
 * array and the (then partly wrong) counts are bit-identical to the reference's; 0 = plain unsigned
 * order with true counts; no effect and no cost on pure-ASCII text), "initial_passes" (radix
 * passes of the initial key sort, 0 = automatic), "force_doubling" (0/1), "sort_variant" (radix kernel
 * configuration, 0 = default); further tuning and test hooks are listed in DESIGN.md. */
int cdb_set_option(cdb_index* h, const char* name, int64_t value);

/* statistic by name: "build_ms", "rounds", "unresolved_after_initial", "sort_passes", "isa_built",
 * "key_symbols", "symbol_bits", "query_ms", ... returns CDB_E_INVALID for unknown names.
 * Which row builder answered the batched queries (cdb_query_batch*, and lone keywords handed over to them), counted per handle
 * since cdb_create and left alone by builds, loads and proof repairs: "query_batches"; "query_spec_batches" (run speculatively
 * in buffers sized from the previous batch) and "query_spec_spills" (of those, redone because a hit list or the total did not
 * fit); "query_wave_batches" (one wavefront per pattern, totals known); "query_sort_batches" and "query_sort_chunks" (expand +
 * radix sort, and the chunks query_hit_budget cut them into); "query_empty_batches" (nothing to look up, or no hit).
 * spec + wave + sort + empty - spills == batches.  Shards: through cdb_shards_get(i), as every other statistic. */
int cdb_get_stat(const cdb_index* h, const char* name, double* value);

/* accumulated HIP-event time of one kernel family since cdb_profile_reset (needs option profile=1).
 * bytes = algorithmic bytes moved by those launches. */
int cdb_profile_get(cdb_index* h, const char* kernel, double* total_ms, uint64_t* launches, uint64_t* bytes);
/* writes up to cap bytes of a NUL-terminated, newline-separated "name ms launches bytes" table */
int cdb_profile_dump(cdb_index* h, char* buf, size_t cap);
void cdb_profile_reset(cdb_index* h);

/* The first build of a fresh process pays for device memory the driver maps (and scrubs) on first use: 0.3-2.6 s for a 4 GiB
 * column against 0.13 s warm.  The reference loads its data and only then builds (server.cpp:43-44: init(); build();), so
 * that cost can hide behind the ingest: cdb_reserve — called as soon as the size of the column is roughly known, e.g. with
 * the size of the raw directory at the start of init() — builds and destroys a throw-away index over synthetic text of that
 * size on a helper thread (bytes drawn from the byte histogram of `sample`, e.g. the first document; NULL = printable ASCII;
 * ndocs = 0: 1 KiB documents), which leaves the build's working set in the block cache below — and then maps, as spare blocks
 * of that cache, twins of the arrays an index of that size KEEPS: the first `build` operation after start-up constructs the
 * next generation while this one serves (database.cpp:276-280) and would otherwise pay 0.6-1 s of hipMalloc for them (4 GiB
 * column: second build 947 -> 244 ms).  Skipped where the device has no room for it.  Returns at once; cdb_build* / cdb_load
 * wait for a reservation in flight, cdb_reserve_wait() does so explicitly.  Best effort. */
int cdb_reserve(int device, uint64_t text_bytes, uint64_t ndocs, const char* sample, size_t sample_len);
void cdb_reserve_wait(void);

/* Device blocks released by builds/queries are cached process-wide for the next build (hipMalloc of the
 * ~30 GiB working set of a 1 GiB build costs ~1 s on MI355X — the driver maps and clears VRAM).  This
 * returns every cached block to the driver; cdb_cached_memory_bytes reports the cache size.  Result
 * arrays of 1 MiB and more (cdb_query_batch*, cdb_query_or, cdb_query_spans) are pinned host blocks from a
 * similar cache (up to 8 GiB kept; device-to-host copies into fresh pageable memory run at a few GB/s);
 * always release them through cdb_result_free / cdb_hits_free / cdb_spans_free / cdb_free. */
void cdb_release_cached_memory(void);
uint64_t cdb_cached_memory_bytes(void);
/* upper bound of the block cache (default: unlimited); blocks released beyond it go back to the driver */
void cdb_set_cache_limit(uint64_t bytes);
/* Device memory of the whole process as the library's allocator sees it: bytes handed out right now (indexes + builds
 * in flight), the most ever handed out since cdb_memory_reset_peak(), and the bytes sitting in the block cache.  What
 * database.cpp:276-280 needs to know before it builds a new index beside the serving one: peak - in_use of one build is
 * the head room a rebuild wants.  Buffers the caller owns (cdb_build_device / _resident: the text) are not counted. */
void cdb_memory_stats(uint64_t* in_use_bytes, uint64_t* peak_bytes, uint64_t* cached_bytes);
void cdb_memory_reset_peak(void);

/* Test hook: size-independent checks of the built suffix array, computed on the GPU by plain adjacent-
 * suffix comparison (verify.hip).  out[0] = adjacent pairs out of unsigned byte order, out[1] = equal
 * suffixes not ascending by document, out[2] = wrapped sum of all entries, out[3] = entries that are not
 * a valid (doc, off), out[4] = closed-form expected value of out[2].  (With reference_compat and bytes
 * >= 0x80 the reference's order is not globally sorted, so out[0] > 0 is expected there.) */
int cdb_debug_verify(cdb_index* h, uint64_t out[5]);

/* Test hook: the same kind of check against the REFERENCE's order (reference_compat = 1): inside a radix
 * node — a bucket of more than chuck_size = max(4096, n / 256) suffixes (index.cpp:96-126,218) — children follow the
 * signed-char symbol order of index.h:66-73 (end of document, 0x80..0xFF, 0x00..0x7F); smaller buckets are in unsigned
 * order (std::sort leaves, index.cpp:86-95).  Adjacent pairs are classified by their common prefix and, where the two
 * orders disagree, by the size of the bucket sharing that prefix (found by galloping over the array).
 * out[0] = pairs out of reference order (0 for a correct array), out[1] = pairs whose next bytes lie on different
 * sides of 0x80, out[2] = of those, pairs inside radix nodes (laid out high byte first), out[3] = equal suffixes not
 * ascending by document.  On pure-ASCII text, or with reference_compat = 0 on text without big mixed buckets, it
 * degenerates to the plain sortedness check. */
int cdb_debug_verify_reference(cdb_index* h, uint64_t out[4]);
/* Test hook: the check every build ends with (option self_check), run on the index as it stands — on 2^15 random adjacent
 * pairs, or (full != 0) on every adjacent pair.  out[0] = pairs out of order, out[1] = entries that are no valid (doc, off). */
int cdb_debug_self_check(cdb_index* h, int full, uint64_t out[2]);
/* Test hook: the kept search keys against the text.  out[0] = slots whose kept key (in whichever of the three arrays the handle
 * holds: 64-bit keys, 32-bit keys, 32-bit keys + low digits) differs from the key recomputed from that suffix's bytes under the
 * handle's symbol map; out[1] = slots checked, 0 when no keys are kept (after cdb_load, or an append that dropped them). */
int cdb_debug_verify_keys(cdb_index* h, uint64_t out[2]);

/* The order proof behind a published build (option self_check = 3, the default).  The reference's array is sorted by
 * construction (std::sort leaves, index.cpp:86-95); this library's passes rest on an observed LDS lane order, so after
 * cdb_build* / cdb_load return (with a sample of adjacent pairs checked) a helper thread compares EVERY adjacent pair of the
 * published array against the text on a low-priority stream of its own, beside the queries (text with bytes >= 0x80 in the
 * reference's order: also the pairs whose order depends on the size of the reference's radix buckets, index.h:66-73).  cdb_get_stat "order_proved" goes
 * 0 -> 1 when it is through; damage makes the handle rebuild itself with the ballot ranking under its lock (queries wait; stat
 * "self_check_fallbacks" counts it).  cdb_proof_wait blocks until the proof of the CURRENT array has ended, at most timeout_ms
 * (< 0: no limit), and returns its state: 0 no proof was started (self_check < 3, or not built), 1 still running, 2 proved,
 * 3 damage found and repaired (the replacement was checked pair by pair before it was served), 4 damage found and the rebuild
 * failed (the handle is unbuilt), 5 cancelled by a build that replaced the array, 6 the proof could not run; < 0: an error. */
int cdb_proof_wait(cdb_index* h, double timeout_ms);

/* Test hook for the radix-sort primitive (tests/test_gpu_sort.py, tools/sort_bench.py): stable sort of
 * n 64-bit keys (+ optional 4- or 8-byte values, val_bytes = 0/4/8) held in DEVICE memory by key bits
 * [0, key_bits), in place.  variant = kernel configuration (0 = default).  Reports the summed HIP-event
 * time of the onesweep launches and how many passes ran. */
int cdb_debug_radix_sort(int device, void* d_keys, void* d_vals, uint64_t n, int val_bytes, int key_bits,
                         int variant, double* onesweep_ms, int* passes);

/* Test hooks that call the radix-sort primitive the way the library itself does (tests/test_gpu_sort_edges.py; debug_sort.hip).
 * Not part of the stable ABI.  flags: */
#define CDB_DEBUG_SORT_DEVICE_HIST 1u  /* digit histograms counted on the device and handed over there: no pass is skipped */
#define CDB_DEBUG_SORT_SPARE_VALUES 2u /* a third value buffer (RadixWorkspace::value_spare) */
#define CDB_DEBUG_SORT_POISON 4u       /* the sort finds the look-back error flag already up (RadixWorkspace::debug_poison) */
#define CDB_DEBUG_SORT_GROUPED 8u      /* XCD-aware tile order allowed (allow_group); after a look-back timeout the hook restores
                                        * the input, sorts once more in plain ticket order and reports fell_back = 1 */
#define CDB_DEBUG_SORT_PROFILE 16u     /* time the onesweep launches with HIP events (onesweep_ms) */
typedef struct cdb_debug_sort_result {
    int passes_run, passes_skipped;
    int key_result;     /* the sort's return value: the buffer (0 / 1) the keys (and auxiliary words) ended in */
    int value_result;   /* RadixWorkspace::value_result: the buffer the values ended in */
    int fell_back;
    uint32_t epoch;     /* the workspace's epoch after the sort */
    double onesweep_ms;
} cdb_debug_sort_result;
/* A workspace that outlives one sort, with the stream it sorts on: a sequence of hook calls on one handle sees what a library
 * handle's workspace sees (epoch wrap, status array growth, stale status words of other tile sizes and key types). */
typedef struct cdb_debug_sort_ws cdb_debug_sort_ws;
int cdb_debug_sort_ws_create(int device, cdb_debug_sort_ws** out);
void cdb_debug_sort_ws_destroy(cdb_debug_sort_ws* ws);
/* radix_sort<K, V>: stable sort of n keys of key_bytes (4 / 8) with values of val_bytes (0 / 4 / 8) in DEVICE memory by key bits
 * [begin_bit, end_bit) in digits of dbits (1..8) bits; the other key bits travel along.  variant: 0, 1, 21, 26, 31, 33, 36, 32, and for
 * 8-byte keys 4 and 41.  ws = NULL: a fresh workspace for this call.  The result is always left in d_keys / d_vals, whatever buffer
 * the sort ended in; after an error they hold what buffers 0 held when the sort gave up.  Returns the status of the error thrown. */
int cdb_debug_radix_sort_ex(int device, cdb_debug_sort_ws* ws, void* d_keys, void* d_vals, uint64_t n, int key_bytes, int val_bytes,
                            int begin_bit, int end_bit, int dbits, int variant, unsigned flags, cdb_debug_sort_result* out);
/* radix_sort_split over materialised records (no generated pass): 4-byte keys sorted by their low hi_bits bits below which the
 * lead_digits lowest bytes of the auxiliary word (aux_bytes 1 / 2 / 4) sort first; values of 4 bytes (any aux_bytes) or 8 bytes
 * (aux_bytes 1 / 2).  The histograms the sort requires are counted by the hook: on the host from a copy, or with
 * CDB_DEBUG_SORT_DEVICE_HIST by a kernel. */
int cdb_debug_radix_sort_split(int device, cdb_debug_sort_ws* ws, void* d_keys, void* d_vals, void* d_aux, uint64_t n, int val_bytes,
                               int aux_bytes, int hi_bits, int lead_digits, int variant, unsigned flags, cdb_debug_sort_result* out);

/* Test hooks for the device-wide scan (scan.h) and the stable tile ranks (stable_tiles.h), called the way the library itself calls
 * them (tests/test_gpu_scan_edges.py; debug_scan.hip).  Not part of the stable ABI.  Every array lies in HOST memory; an item is a
 * uint64_t, or for the pair kinds two uint64_t (16 bytes: U2 = (a, b), DocMax = (document, maximum)).  kind = the value type and
 * operator of a production instantiation: */
#define CDB_DEBUG_SCAN_U64_ADD 0    /* uint64_t, sum modulo 2^64, identity 0 */
#define CDB_DEBUG_SCAN_U64_MAX 1    /* uint64_t, maximum, identity 0 */
#define CDB_DEBUG_SCAN_U2_ADD 2     /* pairs, both halves summed, identity (0, 0) */
#define CDB_DEBUG_SCAN_U2_SUMMAX 3  /* pairs, (sum, maximum), identity (0, 0) */
#define CDB_DEBUG_SCAN_DOCMAX 4     /* pairs, maximum inside runs of equal documents; {~0, 0} is a LEFT identity only */
#define CDB_DEBUG_SCAN_FLAGS_ADD 5  /* input = n flag BYTES f read 16 at a time, item = (f >> 1 & 1, f >> 1 & f & 1), summed as pairs */
/* scan_totals then scan_apply over n items: out_exclusive[i] = fold of items [0, i), out_inclusive[i] = fold of items [0, i],
 * *out_total = what scan_totals returned (the fold of everything, begun from the identity).  n = 0 is legal. */
int cdb_debug_scan(int device, int kind, const void* in, uint64_t n, void* out_exclusive, void* out_inclusive, void* out_total);
/* scan_partials_inplace over nb raw tile sums (kinds 0..4), in a device block of exactly the elements scan_totals reserves for nb
 * tiles with guard_words poisoned elements behind them.  partials_inout[nb + 1]: the sums in; their exclusive prefixes and, in slot
 * nb, the grand total out.  *out_guard_ok = 1 when the poison is untouched. */
int cdb_debug_scan_partials(int device, int kind, void* partials_inout, uint64_t nb, uint64_t guard_words, int* out_guard_ok);
/* tile_bases + TileRanker over n >= 1 flag bytes (non-zero = flagged; n = 0: CDB_E_INVALID): out_before[i] = flagged slots in front
 * of slot i, for every slot; out_tile_base[t] = flagged slots in front of tile t of 4096 slots (ceil(n / 4096) entries); *out_total =
 * what tile_bases returned. */
int cdb_debug_stable_ranks(int device, const uint8_t* flags, uint64_t n, uint64_t* out_before, uint64_t* out_tile_base, uint64_t* out_total);

/* Test hook for the record sweeps of the bucket-wise build (records_sweep.h) and the bucket histograms counted from their records
 * (tests/test_gpu_sweep_edges.py; debug_sweep.hip).  Not part of the stable ABI.  Every array lies in HOST memory.  The hook runs
 * ONE bucket group the way the build does: tile bases from the per-tile byte counts, the tile -> document table, the tile ->
 * segment map, then the dense (vl = 0) or the variable-length (vl = 1) sweep with aux_bytes-wide auxiliary words and the histogram
 * sweep.  It refuses (CDB_E_INVALID) tables under which a record could land outside the group: tile_counts must be the text's, a
 * byte whose slot lies in [g0, g1) must be src_col of that slot and be named by slotmap / vl_dec again, slot d's records are
 * [slot_start[d] - gstart, ... + its count) = segment d - g0, inside [0, gelems), tile_begin in running order.  CDB_E_INTERNAL on a
 * device without the one-atomic ranking, as the build would not sweep there. */
typedef struct cdb_debug_sweep_args {
    const uint8_t* text;        /* [n] */
    uint64_t n;
    const uint64_t* doc_start;  /* [ndocs + 1], doc_start[ndocs] = n */
    uint64_t ndocs;
    int bits;                   /* entry = (offset << bits) + document */
    int padded;                 /* 0: a device buffer of exactly n bytes; 1: n + 128 bytes, those behind n filled with 0xA5 */
    const uint16_t* codeslot;   /* [256] byte -> symbol code | bucket slot << 8 */
    const uint8_t* slotmap;     /* [257] symbol code -> bucket slot */
    const uint16_t* src_col;    /* [256] bucket slot -> the byte whose counts feed it (0xFFFF: none) */
    const uint64_t* slot_start; /* [256] array-wide first record of every bucket slot */
    int vl;
    uint32_t base;              /* dense keys: nsym - 1 symbols behind the bucket symbol in base `base`, */
    int nsym;
    uint32_t part_m;            /* ... times part_m plus the next symbol quantised to part_m levels (1: none) */
    const uint16_t* vl_sym;     /* variable-length keys: [256] and [128], the tables of cdb_debug_vl_tables */
    const uint16_t* vl_dec;
    int key_bits, end_len, carry, carry_shift;
    int rec_low_bits;           /* key bits kept in the auxiliary word */
    int aux_bytes;              /* 1, 2 or 4 */
    uint32_t g0, g1;            /* the group's bucket slots */
    uint64_t gstart, gelems;    /* its first record array-wide, its records */
    const uint64_t* seg_begin;  /* [g1 - g0] group-local record range and first tile (of 16384 records) of every bucket */
    const uint64_t* seg_end;
    const uint32_t* seg_tile_begin;
    int lead, npass;            /* histogram: digit p < lead = byte p of the auxiliary word, digit lead + q = byte q of the key */
    const uint32_t* tile_counts;  /* [ceil(n / 8192)][256] bytes of every text tile */
    uint32_t* out_k;            /* [gelems] */
    uint32_t* out_v;            /* [gelems] */
    void* out_w;                /* [gelems] of aux_bytes */
    uint64_t* out_hist;         /* [g1 - g0][8][256] */
    uint64_t* out_tile_base;    /* optional [tiles][256] */
    uint64_t* out_tile_doc;     /* optional [tiles + 1] */
    int* out_guard_ok;          /* 1: the 4096 poisoned records in front of and behind k, v and w are untouched */
} cdb_debug_sweep_args;
int cdb_debug_sweep_records(int device, const cdb_debug_sweep_args* args);
/* vl_build + vl_fill_tables (vl_code.h), host only: the code the build would choose for counts[0] documents and counts[c]
 * occurrences of symbol code c = 1 .. sigma (2 <= sigma <= 127), as the sweep's tables sym_out[256] / dec_out[128] with
 * slot_of_code[c] the bucket slot of code c; *end_len_out = length of END's word.  CDB_E_INVALID: no code. */
int cdb_debug_vl_tables(const uint64_t* counts, int sigma, const uint8_t* slot_of_code, uint16_t* sym_out, uint16_t* dec_out, int* end_len_out);

/* Test hook for the in-place carried round of the refinement (carried_inplace.h: sa_carried_inplace_kernel;
 * tests/test_gpu_carried_inplace.py; debug_carried.hip).  Not part of the stable ABI.  Every array lies in HOST memory.  The hook
 * uploads n entries (one uint64_t each; stored on the device in the form named below) and their n flag bytes (bit 0 = head of a
 * group, bit 1 = open, bits 2.. = the carried bits, of which the low xbits = 1..6 are the sort key), launches the sweep the way the
 * build does and returns the entries and flag bytes as it leaves them, out_partials[tile] = (open entries, open heads) of every tile
 * of 4096 slots (two uint64_t each, ceil(n / 4096) tiles), out_counts[0] = open entries met and out_counts[1] = entries moved.
 * *out_guard_ok = 1 when the 4096 poisoned bytes in front of and behind every device array are untouched.  n = 0: CDB_E_INVALID. */
#define CDB_DEBUG_CARRIED_PACKED40 0  /* 5-byte entries: a uint32_t array and a byte array (bits 32..39) */
#define CDB_DEBUG_CARRIED_U32 1       /* plain uint32_t entries */
#define CDB_DEBUG_CARRIED_U64 2       /* plain uint64_t entries */
int cdb_debug_carried_inplace(int device, int form, uint64_t* entries_inout, uint8_t* flags_inout, uint64_t n, int xbits,
                              uint64_t* out_partials, uint64_t* out_counts, int* out_guard_ok);

/* Test hook for the segmented sort of bucket records (radix_sort.h: radix_sort_segmented, radix_sort_top_first;
 * tests/test_gpu_segsort_top_first.py; debug_segsort.hip).  Not part of the stable ABI.  Every array lies in HOST memory.  n records
 * (u32 k32, u32 v32 = entry bits 0..31, u16 w16) in nb buckets, bucket b = records [bucket_begin[b], bucket_begin[b + 1]), with
 * 40-bit variable-length keys in the split the form sorts: FIVE_PASS: k32 = key >> 8, w16 = key & 0xFF | hi << 8; TOP_FIRST:
 * k32 = (uint32_t)key, w16 = key >> 32 | hi << 8; hi = entry bits 32.. (ehb of them) | carried bits << ehb (carry of them,
 * ehb + carry <= 8, carry <= 6).  The hook runs the form as the build does for one bucket group and returns the entries
 * (packed = 1: written as 5-byte entries and put together again here) and the flag bytes (bit 0 head, bit 1 open, bits 2.. the
 * carried bits); TOP_FIRST also returns its cells as (begin, end, tile_begin) triples in out_cells (cells_cap >= 256 nb) and
 * their count.  *out_guard_ok = 1 when the poisoned elements around every record and output array are untouched. */
#define CDB_DEBUG_SEGSORT_FIVE_PASS 0
#define CDB_DEBUG_SEGSORT_TOP_FIRST 1
int cdb_debug_segsort(int device, int form, int packed, uint64_t n, uint32_t nb, const uint64_t* bucket_begin, const uint32_t* k32,
                      const uint32_t* v32, const uint16_t* w16, int ehb, int carry, uint64_t* out_entries, uint8_t* out_flags,
                      uint64_t* out_cells, uint32_t cells_cap, uint32_t* out_ncells, int* out_guard_ok);

/* Measurement hook: wall time of `reps` back-to-back cdb_query calls for each of `nkw` keywords (blob + offsets like
 * cdb_query_batch), taken inside the library with a steady clock — what a C++ caller such as database.cpp:392 sees,
 * without a language binding in between.  us_out[nkw] receives the MEDIAN microseconds per call of every keyword;
 * results are freed immediately. */
int cdb_debug_query_latency(cdb_index* h, const char* blob, const uint64_t* offsets, size_t nkw, int reps, double* us_out);

/* The build prologue's layout rule as a pure host function (no device, no handle): entry layout of an index over
 * `ndocs` documents whose longest has `longest` bytes — index.cpp:182-208: masks grown by `mask = (mask << 1) + 1`,
 * bits = popcount, 4-byte entries while bits + offset bits <= 32.  Returns CDB_OK and fills bits / mask / width /
 * off_bits, or CDB_E_INVALID with the reference's own message in `err` (index.cpp:195-200: "The amount of data
 * exceeds the maximum range that CoffeeDB can handle" beyond 64 bits, "The number of objects exceeds ..." beyond 2^32
 * documents).  What cdb_build* apply before they touch the device. */
int cdb_layout_rule(uint64_t ndocs, uint64_t longest, uint64_t* bits, uint64_t* mask, int* width, int* off_bits,
                    char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* COFFEEDB_GPU_H */
