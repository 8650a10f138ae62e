// rowset_maintain.hip — the two operations of interface.cpp that were left to host id lists (include/coffeedb_gpu.h):
//
// cdb_rowset_remove   `remove` (interface.cpp:274-285): the rows of a set leave every field given, all or none.  The ids are the
//                     set's own device array; every field PREPARES its new column beside the serving one (string index:
//                     remove_prepare, capi.hip; column: column_remove_prepare, column_maintain.hip), one after another in the
//                     caller's order, and only when all stand does every field commit.  A failed prepare drops every prepared
//                     change: the blocks go back and no handle ever knew of them.
// cdb_rowset_all      query() of database.cpp:380-386, "every object with count 0": the union of the ids the given fields hold.
//                     The fields' id lists (each ascending, read under the field's lock) are laid end to end as keys id ^ 2^63, so
//                     that unsigned order is the signed order of the ids, sorted key-only (radix_sort skips constant digits; one
//                     list alone is in order already and is not sorted), and compacted to the first key of every run of equal
//                     ones: a head is a key that differs from its predecessor, ranked tile by tile (stable_tiles.h).  One pass
//                     writes ids and zero counts.  Every count being 0, the OR and the AND of the page keys (rowset.hip) are the
//                     same constant: no key byte differs, and a page of the set is the ids [first, last) in ascending order.
// 64-bit indices throughout: the lists together may pass 2^32 entries.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"
#include "scan.h"
#include "stable_tiles.h"

using namespace cdb;

namespace {

constexpr uint64_t SIGN = 1ull << 63;

// ---- cdb_rowset_all ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void all_keys_kernel(const int64_t* __restrict__ ids, uint64_t n, uint64_t* __restrict__ key) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) key[i] = (uint64_t)ids[i] ^ SIGN;
}
struct KeyHead {  // the flag of the ranking: slot i opens a run of equal keys
    const uint64_t* key;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return i == 0 || key[i] != key[i - 1]; }
};
// head number r of the sorted keys is row r of the set: its id, and the count 0
__global__ __launch_bounds__(256) void all_unique_kernel(const uint64_t* __restrict__ key, uint64_t n, const uint64_t* __restrict__ tile_base,
                                                         int64_t* __restrict__ ids, int64_t* __restrict__ counts) {
    TileRanker ranker(tile_base);
    const KeyHead head{key};
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t i = tile_slot(k);
        const bool h = i < n && head(i);
        const uint64_t at = ranker.before(k, h);
        if (h) {
            ids[at] = (int64_t)(key[i] ^ SIGN);
            counts[at] = 0;
        }
    }
}

// the device half of cdb_rowset_all on the set's stream; synchronises
void rowset_all_device(cdb_rowset* rs, const std::vector<IdList>& lists, int nonempty, uint64_t N) {
    Index& ws = rs->ws;
    hipStream_t s = ws.stream;
    Profiler& prof = ws.prof;
    if (N) {
        // 1. the lists end to end, keyed (the fields' streams are idle: every call on a field synchronises before it returns)
        DevBuf k0, k1, tile_base;
        k0.alloc(N * 8);
        uint64_t at = 0;
        int t = prof.begin(s);
        for (const IdList& l : lists) {
            if (!l.n) continue;
            hipLaunchKernelGGL(all_keys_kernel, dim3(grid_for(l.n)), dim3(256), 0, s, l.ids, l.n, k0.as<uint64_t>() + at);
            at += l.n;
        }
        prof.end(t, "all_keys", N * 16, s);
        CDB_HIP(hipGetLastError());
        // 2. sorted (one list alone ascends already)
        int sel = 0;
        if (nonempty > 1) {
            k1.alloc(N * 8);
            sel = radix_sort<uint64_t, NoVal>(s, ws.rws, prof, k0.as<uint64_t>(), k1.as<uint64_t>(), (NoVal*)nullptr, (NoVal*)nullptr, N, 0, 64, nullptr);
        }
        const uint64_t* key = (sel ? k1 : k0).as<uint64_t>();
        // 3. the first key of every run
        const uint64_t ntiles = ceil_div(N, ST_TILE);
        const uint64_t m = tile_bases(ws, "rowset all", KeyHead{key}, N, tile_base, "all_count", N * 8 + ntiles * 8);  // (synchronises)
        if (m == 0 || m > N) throw InternalError("rowset all: the runs of equal ids were miscounted (internal)");
        rs->ids.alloc(m * 8);
        rs->counts.alloc(m * 8);
        t = prof.begin(s);
        hipLaunchKernelGGL(all_unique_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, key, N, (const uint64_t*)tile_base.as<uint64_t>(),
                           rs->ids.as<int64_t>(), rs->counts.as<int64_t>());
        prof.end(t, "all_unique", N * 8 + m * 16 + ntiles * 8, s);
        CDB_HIP(hipGetLastError());
        radix_check_error(s, ws.rws);
        rs->m = m;
    } else {
        rs->ids.alloc(0);
        rs->counts.alloc(0);
    }
    rowset_adopt_equal_counts(rs, s, 0);  // (synchronises: the lists are read, the locks may go)
}

void rowset_all(cdb_rowset* rs, cdb_index* const* indexes, int nindexes, cdb_column* const* columns, int ncolumns) {
    const double t0 = wall_ms();
    std::vector<std::mutex*> mus;
    for (int k = 0; k < nindexes; ++k) mus.push_back(&indexes[k]->ix.mu);
    for (int j = 0; j < ncolumns; ++j) mus.push_back(&columns[j]->ws.mu);
    FieldLocks held(std::move(mus));
    std::vector<IdList> lists;
    uint64_t N = 0;
    for (int k = 0; k < nindexes; ++k) lists.push_back(index_id_list(indexes[k]->ix));
    for (int j = 0; j < ncolumns; ++j) lists.push_back(IdList{columns[j]->id_sorted.as<int64_t>(), columns[j]->n});  // (built rows only)
    int nonempty = 0;
    for (const IdList& l : lists) {
        N += l.n;
        nonempty += l.n ? 1 : 0;
    }
    DeviceScope scope(rs->ws);
    Index& ws = rs->ws;
    hipStream_t s = ws.stream;
    Profiler& prof = ws.prof;
    rs->all_fields = (uint64_t)(nindexes + ncolumns);
    rs->all_input_rows = N;
    rs->m = 0;
    try {
        rowset_all_device(rs, lists, nonempty, N);
    } catch (...) {
        (void)hipStreamSynchronize(s);  // (the lists were being read on the set's stream: the fields' locks go only behind that)
        throw;
    }
    prof.resolve();
    rs->all_ms = wall_ms() - t0;
}

// ---- cdb_rowset_remove ---------------------------------------------------------------------------------------------------------
struct FieldWork {
    ColumnChangePtr index_change;  // a prepared string field (null: nothing to commit)
    ColumnRemoval column_change;   // a prepared column (changed = false: nothing to commit)
};

void rowset_remove(cdb_rowset* rs, cdb_remove_field* fields, int nfields, uint64_t* rows) {
    // 3. every field's lock together, in address order
    std::vector<std::mutex*> mus;
    for (int k = 0; k < nfields; ++k) mus.push_back(fields[k].index ? &fields[k].index->ix.mu : &fields[k].column->ws.mu);
    FieldLocks held(std::move(mus));
    // 4. everything that is refused is refused here, before any device work
    for (int k = 0; k < nfields; ++k) {
        const cdb_remove_field& f = fields[k];
        if ((f.index ? f.index->ix.device : f.column->ws.device) != rs->ws.device) throw Error("cdb_rowset_remove: the field lives on another GPU");
        if (f.index) (void)built_docs_or_refuse(f.index->ix, "remove");
        else if (!f.column->staged_ids.empty()) throw Error("remove: rows were added since the last build");
    }
    const uint64_t m = rs->m;
    if (rows) *rows = m;
    if (!m) return;  // an empty set changes nothing and counts no call
    const double t0 = wall_ms();
    const RowIds ids{nullptr, rs->ids.as<int64_t>()};  // (complete: every call on the set synchronises its stream before it returns)
    // 5. prepare, one field after another in the caller's order; the first failure ends it
    std::vector<FieldWork> work((size_t)nfields);
    int failed = -1;
    Failure fail{CDB_OK, ""};
    for (int k = 0; k < nfields && failed < 0; ++k) {
        cdb_remove_field& f = fields[k];
        try {
            if (f.index) {
                work[k].index_change = remove_prepare(f.index->ix, ids, m, &f.removed, &f.missing);
            } else {
                DeviceScope cs(f.column->ws);
                work[k].column_change.t0 = wall_ms();
                column_remove_prepare(f.column, ids, m, work[k].column_change);
                f.removed = work[k].column_change.removed;
                f.missing = work[k].column_change.missing;
            }
        } catch (...) {
            fail = classify_current_exception();
            failed = k;
        }
    }
    if (failed >= 0) {  // 6'. every prepared change is dropped: the blocks go back, every field answers as before
        for (int k = 0; k < nfields; ++k) {
            work[k].index_change.reset();
            if (fields[k].column) work[k].column_change.release(fields[k].column);
            fields[k].removed = fields[k].missing = 0;
        }
        fields[failed].status = fail.code;
        throw Error((Status)fail.code, "field " + std::to_string(failed) + ": " + fail.message);
    }
    // 6. commit.  Only the build over the compacted text of a reference-order string field can fail in here (capi.hip: column_commit);
    // that field is then "never built", the others commit all the same
    failed = -1;
    for (int k = 0; k < nfields; ++k) {
        cdb_remove_field& f = fields[k];
        try {
            if (f.index) {
                if (!work[k].index_change) continue;
                f.committed = 1;
                column_commit(f.index->ix, *work[k].index_change);
                work[k].index_change.reset();
            } else if (work[k].column_change.changed) {
                DeviceScope cs(f.column->ws);
                f.committed = 1;
                column_remove_commit(f.column, work[k].column_change);
            }
        } catch (...) {
            const Failure cf = classify_current_exception();
            f.status = cf.code;
            if (failed < 0) {
                failed = k;
                fail = cf;
            }
        }
    }
    ++rs->removes;
    rs->remove_fields = (uint64_t)nfields;
    rs->remove_ms = wall_ms() - t0;
    if (failed >= 0) throw Error((Status)fail.code, "field " + std::to_string(failed) + ": " + fail.message);
}

}  // namespace

extern "C" {

int cdb_rowset_all(cdb_index* const* indexes, int nindexes, cdb_column* const* columns, int ncolumns, cdb_rowset** out) {
    if (!out) return CDB_E_INVALID;
    *out = nullptr;
    if (nindexes < 0 || ncolumns < 0 || nindexes + ncolumns < 1 || (nindexes && !indexes) || (ncolumns && !columns)) return CDB_E_INVALID;
    for (int k = 0; k < nindexes; ++k)
        if (!indexes[k]) return CDB_E_INVALID;
    for (int j = 0; j < ncolumns; ++j)
        if (!columns[j]) return CDB_E_INVALID;
    Index& lead = nindexes ? indexes[0]->ix : columns[0]->ws;  // carries the error, as cdb_filter's lead does
    int device = lead.device;
    if (!usable_device(device)) return CDB_E_DEVICE;
    return guarded_ix(lead, [&] {
        for (int k = 0; k < nindexes; ++k)
            if (indexes[k]->ix.device != lead.device) throw Error("cdb_rowset_all: all fields must live on one GPU");
        for (int j = 0; j < ncolumns; ++j)
            if (columns[j]->ws.device != lead.device) throw Error("cdb_rowset_all: all fields must live on one GPU");
        cdb_rowset* rs = rowset_new(lead.device);
        try {
            rs->ws.prof.enabled = lead.prof.enabled;  // (the set has no option of its own yet: the lead's decides)
            rowset_all(rs, indexes, nindexes, columns, ncolumns);
        } catch (...) {
            rowset_delete(rs);  // (drains the set's stream first)
            throw;
        }
        *out = rs;
    });
}

int cdb_rowset_remove(cdb_rowset* rs, cdb_remove_field* fields, int nfields, uint64_t* rows) {
    if (rows) *rows = 0;
    if (!rs || !fields || nfields < 1) return CDB_E_INVALID;
    for (int k = 0; k < nfields; ++k) {
        fields[k].removed = fields[k].missing = 0;
        fields[k].status = CDB_OK;
        fields[k].committed = 0;
    }
    for (int k = 0; k < nfields; ++k) {
        if ((fields[k].index != nullptr) + (fields[k].column != nullptr) != 1) return CDB_E_INVALID;  // none or both
        for (int j = 0; j < k; ++j)
            if (fields[j].index == fields[k].index && fields[j].column == fields[k].column) return CDB_E_INVALID;  // the same handle twice
    }
    int device = rs->ws.device;
    if (!usable_device(device)) return CDB_E_DEVICE;
    return guarded_ix(rs->ws, [&] {
        reserve_wait();                               // 1.
        std::lock_guard<std::mutex> g(rs->ws.mu);     // 2.
        rowset_remove(rs, fields, nfields, rows);     // 3. - 7.
    });
}

}  // extern "C"
