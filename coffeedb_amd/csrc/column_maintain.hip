// column_maintain.hip — rows join and leave a built numeric / bool column on the device (cdb_column_append, and the device path
// of cdb_column_remove; include/coffeedb_gpu.h).  The four arrays of a column (columns.hip's head) are two orders of the same
// rows — (value, id) and id — tied by vpos, so a change is two stable passes (stable_tiles.h) and one gather:
//
//   remove   mark      one lane per given id: bisect id_sorted, a hit flags its id rank (dead_r) and its position (dead_v)
//            value     kept positions ranked tile by tile: keys_v / ids_v compacted, newpos[old position] = new position
//            id        kept id ranks ranked the same way: id_sorted compacted, vpos_new[R] = newpos[vpos[r]] (the one gather)
//   append   batch     the new rows alone become four arrays of their own (columns.hip: column_sort_rows)
//            rank      one lane per new row: its lower bound in the old (key, id) order (bool: the upper bound by key, so a new
//                      row lands behind every old row of its value) and, by id, in id_sorted — an equal id there is a duplicate
//            value     output slot a[j] + j is new row j: flags, tile ranks, a two-way merge that also writes
//                      newpos_old[old position] = its slot
//            id        the same over id_sorted — or, when the smallest new id exceeds the largest old one (ids are insertion
//                      timestamps), a plain concatenation; vpos_new follows through newpos_old and the new rows' slots
// Everything is written into fresh blocks while the old arrays stand and published at the end as column_build publishes.  A removal
// does so in two halves (index_impl.h: column_remove_prepare / column_remove_commit): cdb_column_remove runs them back to back,
// cdb_rowset_remove (rowset_maintain.hip) prepares every field of a call, from the row set's device ids, before it commits any.
// An append has the same halves (column_append_prepare / column_append_commit) for cdb_insert_objects (insert.hip).
#include <algorithm>
#include <cstring>

#include "../../include/coffeedb_gpu.h"
#include "index_impl.h"
#include "scan.h"
#include "stable_tiles.h"

using namespace cdb;

namespace {

struct ByteSet {  // the flag of a ranking: slot i is flagged
    const uint8_t* f;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return f[i] != 0; }
};
struct ByteClear {  // ... slot i is not marked dead
    const uint8_t* f;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return f[i] == 0; }
};

// ---- remove ------------------------------------------------------------------------------------------------------------
// out[0] += entries of ids the column does not hold; a held id given twice writes the same flags twice
__global__ __launch_bounds__(256) void col_rm_mark_kernel(const int64_t* __restrict__ ids, uint64_t nids, const int64_t* __restrict__ id_sorted,
                                                          const uint32_t* __restrict__ vpos, uint64_t n, uint8_t* __restrict__ dead_r,
                                                          uint8_t* __restrict__ dead_v, unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t miss = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nids; i += stride) {
        const int64_t id = ids[i];
        const uint64_t r = lower_bound_id(id_sorted, n, id);
        const bool hit = r < n && id_sorted[r] == id;
        if (hit) {
            dead_r[r] = 1;
            dead_v[vpos[r]] = 1;
        }
        miss += hit ? 0 : 1;
    }
    for (int off = 32; off; off >>= 1) miss += __shfl_xor(miss, off);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(out, (unsigned long long)miss);
}

// kept position number r of the input is position r of the output; nf_out = kept positions in front of slot n_false (bool)
__global__ __launch_bounds__(256) void col_rm_value_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ ids, uint64_t n,
                                                           const uint8_t* __restrict__ dead_v, const uint64_t* __restrict__ tile_base,
                                                           uint64_t* __restrict__ keys_out, int64_t* __restrict__ ids_out,
                                                           uint32_t* __restrict__ newpos, uint64_t n_false, uint64_t* __restrict__ nf_out) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t p = tile_slot(k);
        const bool keep = p < n && dead_v[p] == 0;
        const uint64_t at = ranker.before(k, keep);
        if (p < n && p == n_false) nf_out[0] = at;
        if (keep) {
            keys_out[at] = keys[p];
            ids_out[at] = ids[p];
            newpos[p] = (uint32_t)at;
        }
    }
}
// kept id rank number R: its id, and where its row went
__global__ __launch_bounds__(256) void col_rm_id_kernel(const int64_t* __restrict__ id_sorted, const uint32_t* __restrict__ vpos, uint64_t n,
                                                        const uint8_t* __restrict__ dead_r, const uint64_t* __restrict__ tile_base,
                                                        const uint32_t* __restrict__ newpos, int64_t* __restrict__ id_out,
                                                        uint32_t* __restrict__ vpos_out) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t r = tile_slot(k);
        const bool keep = r < n && dead_r[r] == 0;
        const uint64_t at = ranker.before(k, keep);
        if (keep) {
            id_out[at] = id_sorted[r];
            vpos_out[at] = newpos[vpos[r]];
        }
    }
}

// ---- append ------------------------------------------------------------------------------------------------------------
// new row j (in the batch's key order) goes to output position apos[j] = a[j] + j, a[j] = old rows in front of it; the new id of
// rank j goes to id rank epos[j] = e[j] + j.  An old row with a new id sets dup[0] and leaves the id in dup[1].
template <bool IS_BOOL>
__global__ __launch_bounds__(256) void col_ap_rank_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ ids,
                                                          const int64_t* __restrict__ id_sorted, uint64_t n, const uint64_t* __restrict__ bk,
                                                          const int64_t* __restrict__ bi, const int64_t* __restrict__ b_id_sorted, uint64_t m,
                                                          uint32_t* __restrict__ apos, uint32_t* __restrict__ epos,
                                                          unsigned long long* __restrict__ dup) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += stride) {
        const uint64_t key = bk[j];
        const int64_t id = bi[j];
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            const uint64_t mk = keys[mid];
            const bool before = IS_BOOL ? mk <= key : (mk < key || (mk == key && ids[mid] < id));
            if (before) lo = mid + 1;
            else hi = mid;
        }
        apos[j] = (uint32_t)(lo + j);
        const int64_t nid = b_id_sorted[j];
        const uint64_t e = lower_bound_id(id_sorted, n, nid);
        if (e < n && id_sorted[e] == nid) {
            atomicExch(dup + 1, (unsigned long long)nid);
            atomicOr(dup, 1ull);
        }
        epos[j] = (uint32_t)(e + j);
    }
}
__global__ __launch_bounds__(256) void col_ap_flag_kernel(const uint32_t* __restrict__ pos, uint64_t m, uint8_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += stride) flag[pos[j]] = 1;
}
// output position o is new row q or old row o - q, q = new rows in front of o
__global__ __launch_bounds__(256) void col_ap_value_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ ids,
                                                           const uint64_t* __restrict__ bk, const int64_t* __restrict__ bi, uint64_t N,
                                                           const uint8_t* __restrict__ flag, const uint64_t* __restrict__ tile_base,
                                                           uint64_t* __restrict__ keys_out, int64_t* __restrict__ ids_out,
                                                           uint32_t* __restrict__ newpos_old) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t o = tile_slot(k);
        const bool valid = o < N;
        const bool isnew = valid && flag[o] != 0;
        const uint64_t q = ranker.before(k, isnew);
        if (valid) {
            if (isnew) {
                keys_out[o] = bk[q];
                ids_out[o] = bi[q];
            } else {
                const uint64_t i = o - q;
                keys_out[o] = keys[i];
                ids_out[o] = ids[i];
                newpos_old[i] = (uint32_t)o;
            }
        }
    }
}
// id rank R is the new id of rank q or the old one of rank R - q
__global__ __launch_bounds__(256) void col_ap_id_kernel(const int64_t* __restrict__ id_sorted, const uint32_t* __restrict__ vpos,
                                                        const int64_t* __restrict__ b_id_sorted, const uint32_t* __restrict__ b_vpos,
                                                        const uint32_t* __restrict__ apos, const uint32_t* __restrict__ newpos_old, uint64_t N,
                                                        const uint8_t* __restrict__ flag, const uint64_t* __restrict__ tile_base,
                                                        int64_t* __restrict__ id_out, uint32_t* __restrict__ vpos_out) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t R = tile_slot(k);
        const bool valid = R < N;
        const bool isnew = valid && flag[R] != 0;
        const uint64_t q = ranker.before(k, isnew);
        if (valid) {
            if (isnew) {
                id_out[R] = b_id_sorted[q];
                vpos_out[R] = apos[b_vpos[q]];
            } else {
                const uint64_t r = R - q;
                id_out[R] = id_sorted[r];
                vpos_out[R] = newpos_old[vpos[r]];
            }
        }
    }
}
// ... when every new id exceeds every old one: the old id ranks, then the new ones
__global__ __launch_bounds__(256) void col_ap_id_concat_kernel(const int64_t* __restrict__ id_sorted, const uint32_t* __restrict__ vpos, uint64_t n,
                                                               const int64_t* __restrict__ b_id_sorted, const uint32_t* __restrict__ b_vpos,
                                                               const uint32_t* __restrict__ apos, const uint32_t* __restrict__ newpos_old,
                                                               uint64_t N, int64_t* __restrict__ id_out, uint32_t* __restrict__ vpos_out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t R = (uint64_t)blockIdx.x * 256 + threadIdx.x; R < N; R += stride) {
        if (R < n) {
            id_out[R] = id_sorted[R];
            vpos_out[R] = newpos_old[vpos[R]];
        } else {
            const uint64_t q = R - n;
            id_out[R] = b_id_sorted[q];
            vpos_out[R] = apos[b_vpos[q]];
        }
    }
}

// the merge of cdb_column_append: n = c->n > 0 old rows, m > 0 new ones (ids, raw values on the host), left in r.a
void column_append_merge(cdb_column* c, const int64_t* ids, const std::vector<uint64_t>& raw, uint64_t m, ColumnAppendChange& r) {
    Index& ws = c->ws;
    hipStream_t s = ws.stream;
    Profiler& prof = ws.prof;
    const uint64_t n = c->n, N = n + m;
    const bool is_bool = c->kind == 0;
    // 1. the batch alone
    ColumnArrays b;
    {
        DevBuf idk, key;
        idk.alloc(m * 8);
        key.alloc(m * 8);
        CDB_HIP(hipMemcpyAsync(idk.p, ids, m * 8, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(key.p, raw.data(), m * 8, hipMemcpyHostToDevice, s));
        column_sort_rows(c, idk, key, m, 0, "cdb_column_append", b);
    }
    const uint64_t* bk = b.keys_v.as<uint64_t>();
    const int64_t* bi = b.ids_v.as<int64_t>();
    const int64_t* b_id_sorted = b.id_sorted.as<int64_t>();
    const uint32_t* b_vpos = b.vpos.as<uint32_t>();
    const uint64_t* keys = c->keys_v.as<uint64_t>();
    const int64_t* ids_v = c->ids_v.as<int64_t>();
    const int64_t* id_sorted = c->id_sorted.as<int64_t>();
    const uint32_t* vpos = c->vpos.as<uint32_t>();
    // 2. ranks
    DevBuf apos, epos, d_dup;
    apos.alloc(m * 4);
    epos.alloc(m * 4);
    d_dup.alloc(16);
    CDB_HIP(hipMemsetAsync(d_dup.p, 0, 16, s));
    const uint64_t lg = (uint64_t)bit_width64(n);
    int t = prof.begin(s);
    if (is_bool)
        hipLaunchKernelGGL(col_ap_rank_kernel<true>, dim3(grid_for(m)), dim3(256), 0, s, keys, ids_v, id_sorted, n, bk, bi, b_id_sorted, m,
                           apos.as<uint32_t>(), epos.as<uint32_t>(), d_dup.as<unsigned long long>());
    else
        hipLaunchKernelGGL(col_ap_rank_kernel<false>, dim3(grid_for(m)), dim3(256), 0, s, keys, ids_v, id_sorted, n, bk, bi, b_id_sorted, m,
                           apos.as<uint32_t>(), epos.as<uint32_t>(), d_dup.as<unsigned long long>());
    prof.end(t, "col_ap_rank", m * (32 + lg * 24), s);
    CDB_HIP(hipGetLastError());
    unsigned long long dup[2] = {0, 0};
    int64_t ends[2] = {0, 0};  // the smallest new id, the largest old one
    CDB_HIP(hipMemcpyAsync(dup, d_dup.p, 16, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipMemcpyAsync(&ends[0], b_id_sorted, 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipMemcpyAsync(&ends[1], id_sorted + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));  // (the one wait before the merge: duplicates, and whether the id order is a concatenation)
    const bool concat = ends[0] > ends[1];
    if (dup[0]) throw Error("cdb_column_append: duplicate object id " + std::to_string((long long)dup[1]) + " in one column");
    // 3. + 4. value order
    const uint64_t ntiles = ceil_div(N, ST_TILE);
    DevBuf flag, tile_base, newpos_old;
    ColumnArrays a;
    flag.alloc(N);
    CDB_HIP(hipMemsetAsync(flag.p, 0, N, s));
    t = prof.begin(s);
    hipLaunchKernelGGL(col_ap_flag_kernel, dim3(grid_for(m)), dim3(256), 0, s, (const uint32_t*)apos.as<uint32_t>(), m, flag.as<uint8_t>());
    prof.end(t, "col_ap_flag", m * 5, s);
    CDB_HIP(hipGetLastError());
    if (tile_bases(ws, "column append", ByteSet{flag.as<uint8_t>()}, N, tile_base, "col_ap_count", N + ntiles * 8) != m)
        throw InternalError("column append: new rows share an output position (internal)");
    a.keys_v.alloc(N * 8);
    a.ids_v.alloc(N * 8);
    newpos_old.alloc(n * 4);
    t = prof.begin(s);
    hipLaunchKernelGGL(col_ap_value_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, keys, ids_v, bk, bi, N, (const uint8_t*)flag.as<uint8_t>(),
                       (const uint64_t*)tile_base.as<uint64_t>(), a.keys_v.as<uint64_t>(), a.ids_v.as<int64_t>(), newpos_old.as<uint32_t>());
    prof.end(t, "col_ap_value", N * 33 + n * 4 + ntiles * 8, s);
    CDB_HIP(hipGetLastError());
    // 5. id order
    a.id_sorted.alloc(N * 8);
    a.vpos.alloc(N * 4);
    if (concat) {
        t = prof.begin(s);
        hipLaunchKernelGGL(col_ap_id_concat_kernel, dim3(grid_for(N)), dim3(256), 0, s, id_sorted, vpos, n, b_id_sorted, b_vpos,
                           (const uint32_t*)apos.as<uint32_t>(), (const uint32_t*)newpos_old.as<uint32_t>(), N, a.id_sorted.as<int64_t>(),
                           a.vpos.as<uint32_t>());
        prof.end(t, "col_ap_id_concat", N * 28, s);
    } else {
        CDB_HIP(hipMemsetAsync(flag.p, 0, N, s));
        t = prof.begin(s);
        hipLaunchKernelGGL(col_ap_flag_kernel, dim3(grid_for(m)), dim3(256), 0, s, (const uint32_t*)epos.as<uint32_t>(), m, flag.as<uint8_t>());
        prof.end(t, "col_ap_flag", m * 5, s);
        CDB_HIP(hipGetLastError());
        if (tile_bases(ws, "column append", ByteSet{flag.as<uint8_t>()}, N, tile_base, "col_ap_count", N + ntiles * 8) != m)
            throw InternalError("column append: new ids share an id rank (internal)");
        t = prof.begin(s);
        hipLaunchKernelGGL(col_ap_id_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, id_sorted, vpos, b_id_sorted, b_vpos,
                           (const uint32_t*)apos.as<uint32_t>(), (const uint32_t*)newpos_old.as<uint32_t>(), N, (const uint8_t*)flag.as<uint8_t>(),
                           (const uint64_t*)tile_base.as<uint64_t>(), a.id_sorted.as<int64_t>(), a.vpos.as<uint32_t>());
        prof.end(t, "col_ap_id", N * 29 + ntiles * 8, s);
    }
    CDB_HIP(hipGetLastError());
    if (ws.debug_fail_append_prepare) {  // (the new blocks go back with the stream drained; the serving arrays were only read)
        (void)hipStreamSynchronize(s);
        throw DeviceError("debug: append prepare failure requested (test hook)");
    }
    CDB_HIP(hipStreamSynchronize(s));
    prof.resolve();
    a.n = N;
    a.n_false = c->n_false + b.n_false;
    r.a = std::move(a);
    r.concat = concat;
}

// the build of cdb_column_append: the old rows in their key order (none: a column without rows), then the batch, sorted as
// column_build sorts built and staged rows — without staging the batch on the handle
void column_append_build(cdb_column* c, const int64_t* ids, const std::vector<uint64_t>& raw, uint64_t m, ColumnAppendChange& r) {
    hipStream_t s = c->ws.stream;
    r.build_t0 = wall_ms();
    const uint64_t n_old = c->n, n = n_old + m;
    DevBuf idk0, key0;
    idk0.alloc(n * 8);
    key0.alloc(n * 8);
    if (n_old) {
        CDB_HIP(hipMemcpyAsync(idk0.p, c->ids_v.p, n_old * 8, hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipMemcpyAsync(key0.p, c->keys_v.p, n_old * 8, hipMemcpyDeviceToDevice, s));
    }
    CDB_HIP(hipMemcpyAsync(idk0.as<uint64_t>() + n_old, ids, m * 8, hipMemcpyHostToDevice, s));
    CDB_HIP(hipMemcpyAsync(key0.as<uint64_t>() + n_old, raw.data(), m * 8, hipMemcpyHostToDevice, s));
    column_sort_rows(c, idk0, key0, n, n_old, "cdb_column_append", r.a);  // (synchronises)
    if (c->ws.debug_fail_append_prepare) {
        r.a = ColumnArrays{};
        throw DeviceError("debug: append prepare failure requested (test hook)");
    }
}

}  // namespace

void cdb::column_append_prepare(cdb_column* c, const int64_t* ids, const std::vector<uint64_t>& raw, uint64_t m, ColumnAppendChange& r) {
    r.rows = m;
    r.concat = false;
    try {
        if (r.merge) column_append_merge(c, ids, raw, m, r);
        else column_append_build(c, ids, raw, m, r);
    } catch (...) {  // (uploads from ids / raw may still be queued: the caller's arrays are read until the stream is idle)
        (void)hipStreamSynchronize(c->ws.stream);
        throw;
    }
    r.changed = true;
}

void cdb::column_append_commit(cdb_column* c, ColumnAppendChange& r) {
    if (!r.merge) c->id_sort_skipped = r.a.id_sort_skipped;
    column_publish(c, r.a);
    r.changed = false;
    if (r.merge && r.concat) ++c->append_id_concat;
    if (!r.merge) c->build_ms = wall_ms() - r.build_t0;
    ++c->appends;
    ++(r.merge ? c->append_merges : c->append_rebuilds);
    c->append_rows = r.rows;
    c->append_ms = wall_ms() - r.t0;
}

void cdb::column_remove_prepare(cdb_column* c, RowIds ids, uint64_t nids, ColumnRemoval& r) {
    Index& ws = c->ws;
    hipStream_t s = ws.stream;
    Profiler& prof = ws.prof;
    const uint64_t n = c->n;
    r.removed = 0;
    r.missing = nids;
    r.changed = false;
    if (!n) return;  // (never built, or built over nothing: every id is missing)
    const int64_t* id_sorted = c->id_sorted.as<int64_t>();
    const uint32_t* vpos = c->vpos.as<uint32_t>();
    // 1. mark
    DevBuf d_ids, d_out, dead_r, dead_v;
    const int64_t* idp = resident_ids(s, d_ids, ids, nids);
    d_out.alloc(16);
    dead_r.alloc(n);
    dead_v.alloc(n);
    CDB_HIP(hipMemsetAsync(d_out.p, 0, 16, s));
    CDB_HIP(hipMemsetAsync(dead_r.p, 0, n, s));
    CDB_HIP(hipMemsetAsync(dead_v.p, 0, n, s));
    int t = prof.begin(s);
    hipLaunchKernelGGL(col_rm_mark_kernel, dim3(grid_for(nids)), dim3(256), 0, s, idp, nids, id_sorted, vpos, n, dead_r.as<uint8_t>(),
                       dead_v.as<uint8_t>(), d_out.as<unsigned long long>());
    prof.end(t, "col_rm_mark", nids * (8 + 8 * (uint64_t)bit_width64(n) + 6), s);
    CDB_HIP(hipGetLastError());
    // 2. kept positions per tile
    const uint64_t ntiles = ceil_div(n, ST_TILE);
    DevBuf tile_base;
    const uint64_t kept = tile_bases(ws, "column remove", ByteClear{dead_v.as<uint8_t>()}, n, tile_base, "col_rm_count", n + ntiles * 8);
    unsigned long long miss = 0;
    CDB_HIP(hipMemcpyAsync(&miss, d_out.p, 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    r.missing = miss;
    r.removed = n - kept;
    if (kept == n) return;
    // 3. value order
    const uint64_t cap = std::max<uint64_t>(kept, 1);
    ColumnArrays& a = r.a;
    DevBuf newpos;
    try {
        a.keys_v.alloc(cap * 8);
        a.ids_v.alloc(cap * 8);
        a.id_sorted.alloc(cap * 8);
        a.vpos.alloc(cap * 4);
        newpos.alloc(n * 4);
        t = prof.begin(s);
        hipLaunchKernelGGL(col_rm_value_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, (const uint64_t*)c->keys_v.as<uint64_t>(),
                           (const int64_t*)c->ids_v.as<int64_t>(), n, (const uint8_t*)dead_v.as<uint8_t>(), (const uint64_t*)tile_base.as<uint64_t>(),
                           a.keys_v.as<uint64_t>(), a.ids_v.as<int64_t>(), newpos.as<uint32_t>(), c->n_false, d_out.as<uint64_t>() + 1);
        prof.end(t, "col_rm_value", n * 17 + kept * 20 + ntiles * 8, s);
        CDB_HIP(hipGetLastError());
        // 4. id order
        if (tile_bases(ws, "column remove", ByteClear{dead_r.as<uint8_t>()}, n, tile_base, "col_rm_count", n + ntiles * 8) != kept)
            throw InternalError("column remove: kept id ranks and kept positions differ (internal)");
        t = prof.begin(s);
        hipLaunchKernelGGL(col_rm_id_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, id_sorted, vpos, n, (const uint8_t*)dead_r.as<uint8_t>(),
                           (const uint64_t*)tile_base.as<uint64_t>(), (const uint32_t*)newpos.as<uint32_t>(), a.id_sorted.as<int64_t>(),
                           a.vpos.as<uint32_t>());
        prof.end(t, "col_rm_id", n * 13 + kept * 16 + ntiles * 8, s);
        CDB_HIP(hipGetLastError());
        if (ws.debug_fail_prepare) throw DeviceError("debug: prepare failure requested (test hook)");
        uint64_t nf = 0;
        CDB_HIP(hipMemcpyAsync(&nf, d_out.as<uint64_t>() + 1, 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        prof.resolve();
        a.n = kept;
        a.n_false = c->kind != 0 ? 0 : (c->n_false == n ? kept : nf);  // (no slot n_false when every row is false)
    } catch (...) {  // the new blocks go back with the stream drained; the serving arrays were only read
        (void)hipStreamSynchronize(s);
        a = ColumnArrays{};
        throw;
    }
    r.changed = true;
}

void cdb::column_remove_commit(cdb_column* c, ColumnRemoval& r) {
    column_publish(c, r.a);
    r.changed = false;
    ++c->removes;
    ++c->remove_compactions;
    c->remove_rows = r.removed;
    c->remove_ms = wall_ms() - r.t0;
}

extern "C" {

int cdb_column_append(cdb_column* c, const int64_t* ids, const void* values, uint64_t n, uint64_t* appended) {
    if (!c || (n && (!ids || !values))) return CDB_E_INVALID;
    if (appended) *appended = 0;
    return guarded_ix(c->ws, [&] {
        const std::vector<uint64_t> raw = column_raw_values(c->kind, values, n, "cdb_column_append");
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope cs(c->ws);
        if (!n) return;
        if (!c->staged_ids.empty()) throw Error("append: rows were added since the last build");
        if (c->n + n > COLUMN_MAX_ROWS) throw Error("cdb_column_append: a column holds at most 2^32 - 1 rows");
        // a column without rows takes the build of the batch; so does debug_maintain_path = 2 (the build over old rows and batch).
        // The two halves back to back (cdb_insert_objects prepares every field before it commits any)
        ColumnAppendChange r;
        r.t0 = wall_ms();
        r.merge = c->n > 0 && c->debug_maintain_path != 2;
        column_append_prepare(c, ids, raw, n, r);
        column_append_commit(c, r);
        if (appended) *appended = n;
    });
}

int cdb_debug_column_arrays(cdb_column* c, uint64_t* keys_v, int64_t* ids_v, int64_t* id_sorted, uint32_t* vpos) {
    if (!c) return CDB_E_INVALID;
    return guarded_ix(c->ws, [&] {
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope cs(c->ws);
        hipStream_t s = c->ws.stream;
        const uint64_t n = c->n;
        if (!n) return;
        if (keys_v) CDB_HIP(hipMemcpyAsync(keys_v, c->keys_v.p, n * 8, hipMemcpyDeviceToHost, s));
        if (ids_v) CDB_HIP(hipMemcpyAsync(ids_v, c->ids_v.p, n * 8, hipMemcpyDeviceToHost, s));
        if (id_sorted) CDB_HIP(hipMemcpyAsync(id_sorted, c->id_sorted.p, n * 8, hipMemcpyDeviceToHost, s));
        if (vpos) CDB_HIP(hipMemcpyAsync(vpos, c->vpos.p, n * 4, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"
