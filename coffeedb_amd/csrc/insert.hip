// insert.hip — cdb_insert_objects (include/coffeedb_gpu.h): `insert ... build` (interface.cpp:157-180, :286-288; database.cpp:283-379,
// then :170-282) for all fields of the objects at once, ALL OR NONE — the counterpart of cdb_rowset_remove (rowset_maintain.hip), whose
// order it follows step for step: argument checks, waits and locks, validation, the id check, every field PREPARES its new column
// beside the serving one (string index: append_prepare, capi.hip; column: column_append_prepare, column_maintain.hip) in the caller's
// order, and only when all stand does every field commit.  A failed prepare drops every prepared change: the blocks go back and no
// handle ever knew of them.
//
// The id check, on the lead field's stream (the batch ids go up once):
//   (a) no id twice in the batch   the ids keyed id ^ 2^63 (unsigned order = signed order), sorted key-only, heads of runs of equal
//                                  keys counted tile by tile (stable_tiles.h) as cdb_rowset_all counts them: heads == nobjects or a
//                                  small kernel finds the smallest repeated key for the message
//   (b) no id held by a field      ins_fresh_kernel: a lane is a batch id, blockIdx.y a field's ascending id list (an index's id table,
//                                  a column's id_sorted).  The lane bisects (lower_bound_id: ProbeIn's lower bound) and tests
//                                  a < n && list[a] == id; a wave that has a hit adds its ballot's popcount to the field's counter and
//                                  its smallest offending key to the field's minimum, one vector atomic each.  One copy brings back
//                                  nfields counters and minima.
// 64-bit indices throughout.
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
constexpr unsigned INS_MAX_FIELDS = 65535;  // gridDim.y

__global__ __launch_bounds__(256) void ins_keys_kernel(const int64_t* __restrict__ ids, uint64_t n, uint64_t* __restrict__ key) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) key[i] = (uint64_t)ids[i] ^ SIGN;
}
struct InsKeyHead {  // the flag of the ranking: slot i opens a run of equal keys
    const uint64_t* key;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return i == 0 || key[i] != key[i - 1]; }
};
// out[0] = the smallest key of the sorted keys that equals its predecessor (the caller sets it to all ones)
__global__ __launch_bounds__(256) void ins_twice_kernel(const uint64_t* __restrict__ key, uint64_t n, unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long least = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        if (i > 0 && key[i] == key[i - 1]) least = min(least, (unsigned long long)key[i]);
    for (int off = 32; off; off >>= 1) least = min(least, (unsigned long long)__shfl_xor(least, off));
    if ((threadIdx.x & 63) == 0 && least != ~0ull) atomicMin(out, least);
}

// hits[y] += batch ids that list y holds; least[y] = the smallest of them as a key (the caller sets it to all ones)
__global__ __launch_bounds__(256) void ins_fresh_kernel(const int64_t* __restrict__ ids, uint64_t nobjects, const IdList* __restrict__ lists,
                                                        unsigned long long* __restrict__ hits, unsigned long long* __restrict__ least) {
    const IdList l = lists[blockIdx.y];
    if (!l.n) return;  // (the whole workgroup: a field that holds nothing runs no loop)
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    unsigned long long k = ~0ull;
    if (i < nobjects) {
        const int64_t id = ids[i];
        const uint64_t a = lower_bound_id(l.ids, l.n, id);
        hit = a < l.n && l.ids[a] == id;
        if (hit) k = (unsigned long long)id ^ SIGN;
    }
    const uint64_t bal = __ballot(hit);
    if (!bal) return;  // (wave-uniform)
    for (int off = 32; off; off >>= 1) k = min(k, (unsigned long long)__shfl_xor(k, off));
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&hits[blockIdx.y], (unsigned long long)__popcll(bal));
        atomicMin(&least[blockIdx.y], k);
    }
}

inline Index& index_of(const cdb_insert_field& f) { return f.index ? f.index->ix : f.column->ws; }

// step 4, on the lead's stream with its work spaces; every field's lock is held and every field's stream idle.  Throws the refusal.
void check_ids(Index& lead, const int64_t* ids, uint64_t N, cdb_insert_field* fields, int nfields) {
    DeviceScope scope(lead);
    hipStream_t s = lead.stream;
    Profiler& prof = lead.prof;
    std::vector<IdList> lists((size_t)nfields);
    uint64_t levels = 0;
    for (int k = 0; k < nfields; ++k) {
        const cdb_insert_field& f = fields[k];
        lists[k] = f.index ? index_id_list(f.index->ix) : IdList{f.column->id_sorted.as<int64_t>(), f.column->n};  // (built rows only)
        levels += (uint64_t)bit_width64(lists[k].n);
    }
    DevBuf d_ids, k0, k1, tile_base, d_lists, d_out;
    const uint64_t F = (uint64_t)nfields;
    std::vector<unsigned long long> out(2 * F + 1, ~0ull);  // [hits | least | the smallest repeated key]
    std::fill(out.begin(), out.begin() + nfields, 0ull);
    try {
        d_ids.alloc(N * 8);
        k0.alloc(N * 8);
        d_lists.alloc(F * sizeof(IdList));
        d_out.alloc(out.size() * 8);
        CDB_HIP(hipMemcpyAsync(d_ids.p, ids, N * 8, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(d_lists.p, lists.data(), F * sizeof(IdList), hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(d_out.p, out.data(), out.size() * 8, hipMemcpyHostToDevice, s));
        // (a) no id twice in the batch
        int t = prof.begin(s);
        hipLaunchKernelGGL(ins_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, (const int64_t*)d_ids.as<int64_t>(), N, k0.as<uint64_t>());
        prof.end(t, "ins_keys", N * 16, s);
        CDB_HIP(hipGetLastError());
        int sel = 0;
        if (N > 1) {
            k1.alloc(N * 8);
            sel = radix_sort<uint64_t, NoVal>(s, lead.rws, prof, k0.as<uint64_t>(), k1.as<uint64_t>(), (NoVal*)nullptr, (NoVal*)nullptr, N, 0, 64, nullptr);
        }
        const uint64_t* key = (sel ? k1 : k0).as<uint64_t>();
        const uint64_t ntiles = ceil_div(N, ST_TILE);
        const uint64_t heads = tile_bases(lead, "insert objects", InsKeyHead{key}, N, tile_base, "ins_count", N * 8 + ntiles * 8);  // (synchronises)
        radix_check_error(s, lead.rws);
        if (heads == 0 || heads > N) throw InternalError("insert objects: the runs of equal ids were miscounted (internal)");
        if (heads != N) {
            t = prof.begin(s);
            hipLaunchKernelGGL(ins_twice_kernel, dim3(grid_for(N)), dim3(256), 0, s, key, N, d_out.as<unsigned long long>() + 2 * F);
            prof.end(t, "ins_twice", N * 8, s);
            CDB_HIP(hipGetLastError());
            CDB_HIP(hipMemcpyAsync(&out[2 * F], d_out.as<unsigned long long>() + 2 * F, 8, hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
            prof.resolve();
            throw Error("cdb_insert_objects: object id " + std::to_string((long long)(int64_t)(out[2 * F] ^ SIGN)) + " twice in the batch");
        }
        // (b) no id held by any listed field
        t = prof.begin(s);
        hipLaunchKernelGGL(ins_fresh_kernel, dim3((unsigned)ceil_div(N, 256), (unsigned)nfields), dim3(256), 0, s, (const int64_t*)d_ids.as<int64_t>(), N,
                           (const IdList*)d_lists.as<IdList>(), d_out.as<unsigned long long>(), d_out.as<unsigned long long>() + F);
        prof.end(t, "ins_fresh", N * (F * 8 + 8 * levels), s);  // the id per field; the probes
        CDB_HIP(hipGetLastError());
        CDB_HIP(hipMemcpyAsync(out.data(), d_out.p, 2 * F * 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));  // (ids and the lists are read: the blocks may go)
        prof.resolve();
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
    // the smallest offending id as a signed number, and the first field in the caller's order that holds it
    unsigned long long least = ~0ull;
    int who = -1;
    for (int k = 0; k < nfields; ++k)
        if (out[k] && (who < 0 || out[F + k] < least)) {  // (the key of INT64_MAX is all ones)
            least = out[F + k];
            who = k;
        }
    if (who >= 0)
        throw Error("cdb_insert_objects: object id " + std::to_string((long long)(int64_t)(least ^ SIGN)) + " is already held by field " +
                    std::to_string(who));
}

struct FieldWork {
    std::vector<int64_t> ids;          // the ids of the field's rows (rows given: gathered; else the batch's own array is used)
    std::vector<uint64_t> raw;         // a column's values as cdb_column_append keeps them
    ColumnChangePtr index_change;      // a prepared string field (null: nothing to commit)
    ColumnAppendChange column_change;  // a prepared column (changed = false: nothing to commit)
};

void insert_objects(Index& lead, const int64_t* ids, uint64_t nobjects, cdb_insert_field* fields, int nfields, uint64_t* inserted) {
    // 2. every field's lock together, in address order
    std::vector<std::mutex*> mus;
    for (int k = 0; k < nfields; ++k) mus.push_back(&index_of(fields[k]).mu);
    FieldLocks held(std::move(mus));
    // 3. everything that is refused is refused here, before any device work
    std::vector<FieldWork> work((size_t)nfields);
    std::vector<uint8_t> listed(nobjects, 0);
    for (int k = 0; k < nfields; ++k) {
        const cdb_insert_field& f = fields[k];
        if (index_of(f).device != lead.device) throw Error("cdb_insert_objects: all fields must live on one GPU");
        if (f.index) (void)built_docs_or_refuse(f.index->ix, "append");
        else if (!f.column->staged_ids.empty()) throw Error("append: rows were added since the last build");
        if (f.rows) {
            work[k].ids.resize(f.nrows);
            for (uint64_t j = 0; j < f.nrows; ++j) {
                if (f.rows[j] >= nobjects || (j && f.rows[j] <= f.rows[j - 1]))
                    throw Error("cdb_insert_objects: field " + std::to_string(k) + ": rows must ascend strictly and stay below nobjects");
                listed[f.rows[j]] = 1;
                work[k].ids[j] = ids[f.rows[j]];
            }
        } else {
            std::fill(listed.begin(), listed.end(), 1);
        }
        if (f.column) {
            if (f.nrows) work[k].raw = column_raw_values(f.column->kind, f.values, f.nrows, "cdb_column_append");
            if (f.column->n + f.nrows > COLUMN_MAX_ROWS) throw Error("cdb_column_append: a column holds at most 2^32 - 1 rows");
        }
    }
    for (uint64_t i = 0; i < nobjects; ++i)
        if (!listed[i]) throw Error("cdb_insert_objects: object " + std::to_string(i) + " holds no field");  // database.cpp:284-286
    if (!nobjects) return;  // an empty batch changes nothing and counts no call
    const double t0 = wall_ms();
    // 4. the id check
    check_ids(lead, ids, nobjects, fields, nfields);
    // 5. prepare, one field after another in the caller's order; the first failure ends it
    int failed = -1;
    Failure fail{CDB_OK, ""};
    for (int k = 0; k < nfields && failed < 0; ++k) {
        cdb_insert_field& f = fields[k];
        if (!f.nrows) continue;
        const int64_t* fid = f.rows ? work[k].ids.data() : ids;
        try {
            if (f.index) {
                work[k].index_change = append_prepare(f.index->ix, fid, f.blob, f.doc_start, f.nrows);
            } else {
                DeviceScope cs(f.column->ws);
                work[k].column_change.t0 = wall_ms();
                work[k].column_change.merge = f.column->n > 0;
                column_append_prepare(f.column, fid, work[k].raw, f.nrows, work[k].column_change);
            }
        } catch (...) {
            fail = classify_current_exception();
            failed = k;
        }
    }
    if (failed >= 0) {  // 5'. every prepared change is dropped: the blocks go back, every field answers as before
        for (int k = 0; k < nfields; ++k) {
            work[k].index_change.reset();
            if (fields[k].column) work[k].column_change.release(fields[k].column);
        }
        fields[failed].status = fail.code;
        throw Error((Status)fail.code, "field " + std::to_string(failed) + ": " + fail.message);
    }
    // 6. commit.  Only the build over the new text of a reference-order string field (or of one that held nothing) can fail in here
    // (capi.hip: column_commit); that field is then "never built", the others commit all the same
    for (int k = 0; k < nfields; ++k) {
        cdb_insert_field& f = fields[k];
        try {
            if (f.index) {
                if (!work[k].index_change) continue;
                f.committed = 1;
                column_commit(f.index->ix, *work[k].index_change);
                work[k].index_change.reset();
                f.appended = f.nrows;
            } else if (work[k].column_change.changed) {
                DeviceScope cs(f.column->ws);
                f.committed = 1;
                column_append_commit(f.column, work[k].column_change);
                f.appended = f.nrows;
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
    ++lead.ins.calls;
    lead.ins.fields = (uint64_t)nfields;
    lead.ins.objects = nobjects;
    lead.ins.last_ms = wall_ms() - t0;
    if (failed >= 0) throw Error((Status)fail.code, "field " + std::to_string(failed) + ": " + fail.message);
    if (inserted) *inserted = nobjects;
}

}  // namespace

extern "C" {

int cdb_insert_objects(const int64_t* ids, uint64_t nobjects, cdb_insert_field* fields, int nfields, uint64_t* inserted) {
    if (inserted) *inserted = 0;
    if (!fields || nfields < 1 || (unsigned)nfields > INS_MAX_FIELDS) return CDB_E_INVALID;  // (a field is a row of the check's grid)
    for (int k = 0; k < nfields; ++k) {
        fields[k].appended = 0;
        fields[k].status = CDB_OK;
        fields[k].committed = 0;
    }
    if (nobjects && !ids) return CDB_E_INVALID;
    for (int k = 0; k < nfields; ++k) {
        const cdb_insert_field& f = fields[k];
        if ((f.index != nullptr) + (f.column != nullptr) != 1) return CDB_E_INVALID;  // none or both
        for (int j = 0; j < k; ++j)
            if (fields[j].index == f.index && fields[j].column == f.column) return CDB_E_INVALID;  // the same handle twice
        if (!f.rows && f.nrows != nobjects) return CDB_E_INVALID;
        if (f.nrows && (f.index ? (!f.blob || !f.doc_start) : !f.values)) return CDB_E_INVALID;  // the payload of its kind
    }
    Index& lead = index_of(fields[0]);  // carries the error and the stats, as cdb_rowset_all's lead does
    int device = lead.device;
    if (!usable_device(device)) return CDB_E_DEVICE;
    return guarded_ix(lead, [&] {
        reserve_wait();                                                  // 2.
        insert_objects(lead, ids, nobjects, fields, nfields, inserted);  // 2. - 7.
    });
}

int cdb_insert_get_stat(const cdb_index* index, const cdb_column* column, const char* name, double* value) {
    if ((index != nullptr) + (column != nullptr) != 1 || !name || !value) return CDB_E_INVALID;
    Index& lead = const_cast<Index&>(index ? index->ix : column->ws);
    std::lock_guard<std::mutex> g(lead.mu);  // (the counters change under the lead's lock)
    struct { const char* n; double v; } tab[] = {
        {"inserts", (double)lead.ins.calls}, {"insert_fields", (double)lead.ins.fields}, {"insert_objects", (double)lead.ins.objects},
        {"insert_ms", lead.ins.last_ms},
    };
    for (auto& e : tab)
        if (!std::strcmp(e.n, name)) {
            *value = e.v;
            return CDB_OK;
        }
    return CDB_E_INVALID;
}

}  // extern "C"
