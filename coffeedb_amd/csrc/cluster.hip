// cluster.hip — `cluster` on the device (include/coffeedb_gpu.h: cdb_column_cluster, cdb_cluster): the rows filter() left over,
// grouped by the value one field holds for them — database.cpp:442-460 (a std::map<std::string, int64_t> filled row by row from
// the host object store), called from interface.cpp:249-273.
//
// Columns.  id -> rank (bisection over id_sorted) -> p = vpos[rank], the row's position in (value, id) order; grouping by value is
// grouping the p by keys_v[p].
//   sparse: radix sort of the 32-bit p (bit_width(n) bits, key only), heads where keys_v differs between neighbours, scan, one
//           group per head; equal keys ascend by id, so the first row of a run carries the group's smallest id.
//   dense:  cnt[p] += 1 per row (u32[n]), an exclusive scan C of cnt, and one pass over the column's runs of equal keys (their
//           starts are made once per build): a run with C[end] > C[start] is a group.  No sort.
//   bool:   two counters and two minima.
// String indexes.  Equal documents are equal suffixes at offset 0 and neighbours in the suffix array — in the reference's order
// too: radix nodes and sorted leaves both partition by the next byte.  Once per built array (ClusterTables, index_impl.h): the
// offset-0 entries compacted in array order, neighbours compared against the text, heads scanned into class numbers; classes
// re-ordered by std::string::operator< on the host when the array is not in plain unsigned order; an (id, document) table when
// the ids do not ascend.  Per call: id -> document -> class, sort of (class, id rank), run lengths.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string_view>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"
#include "scan.h"

using namespace cdb;

namespace {

constexpr uint64_t SIGN = 1ull << 63;
// Columns: dense when nrows * DENSE_DEN > n * DENSE_NUM.  Measured on MI355X over 10^7 rows with 10^3 distinct values and timestamp
// ids, both paths forced at 13 result sizes from 0.01 % to 100 % (tools/bench_cluster.py): sparse still wins at 20 %
// (0.71 vs 0.77 ms per call), dense wins from 30 % on (0.94 vs 0.98 ms; 2.27 vs 2.61 ms at 100 %) — the crossover lies between, 1/4 is
// its middle.  One run on one column shape, rows given ascending by id (the kindest case for the dense path's atomics and for the
// bisection's locality): provisional for other shapes — more distinct values lengthen the dense pass over the runs, shuffled rows
// slow both lookups; not measured.
constexpr uint64_t DENSE_NUM = 1, DENSE_DEN = 4;

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
    for (int off = 32; off; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

// ---- columns -------------------------------------------------------------------------------------------------------------------
// row i -> its position in (value, id) order: key[i] = p (sparse; n for an id the column does not hold, which sorts behind every
// row) and / or cnt[p] += 1 (dense); out[0] += rows missed
__global__ __launch_bounds__(256) void clu_col_lookup_kernel(const int64_t* __restrict__ ids, uint64_t nrows, const int64_t* __restrict__ id_sorted,
                                                             const uint32_t* __restrict__ vpos, uint64_t n, uint32_t* __restrict__ key,
                                                             unsigned int* __restrict__ cnt, unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t miss = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nrows; i += stride) {
        const int64_t id = ids[i];
        const uint64_t r = lower_bound_id(id_sorted, n, id);
        const bool hit = r < n && id_sorted[r] == id;
        const uint32_t p = hit ? vpos[r] : (uint32_t)n;
        miss += hit ? 0 : 1;
        if (key) key[i] = p;
        if (cnt && hit) atomicAdd(cnt + p, 1u);
    }
    miss = wave_sum(miss);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(out, (unsigned long long)miss);
}

// bool: out[0] = rows missed, out[1 + v] = rows with value v, out[3 + v] = their smallest id (sortable form, ~0 = none)
__global__ __launch_bounds__(256) void clu_bool_kernel(const int64_t* __restrict__ ids, uint64_t nrows, const int64_t* __restrict__ id_sorted,
                                                       const uint32_t* __restrict__ vpos, uint64_t n, uint64_t n_false,
                                                       unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t miss = 0, c0 = 0, c1 = 0, m0 = ~0ull, m1 = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nrows; i += stride) {
        const int64_t id = ids[i];
        const uint64_t r = lower_bound_id(id_sorted, n, id);
        const bool hit = r < n && id_sorted[r] == id;
        if (!hit) {
            ++miss;
            continue;
        }
        const uint64_t sid = (uint64_t)id ^ SIGN;
        if (vpos[r] < n_false) {
            ++c0;
            m0 = sid < m0 ? sid : m0;
        } else {
            ++c1;
            m1 = sid < m1 ? sid : m1;
        }
    }
    miss = wave_sum(miss);
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    m0 = wave_min(m0);
    m1 = wave_min(m1);
    if ((threadIdx.x & 63) == 0) {
        if (miss) atomicAdd(out, (unsigned long long)miss);
        if (c0) atomicAdd(out + 1, (unsigned long long)c0);
        if (c1) atomicAdd(out + 2, (unsigned long long)c1);
        if (c0) atomicMin(out + 3, (unsigned long long)m0);
        if (c1) atomicMin(out + 4, (unsigned long long)m1);
    }
}

// sparse: the sorted positions; a head is a position whose key differs from its predecessor's
struct ColHeadIn {
    const uint32_t* key;
    const uint64_t* keys_v;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i == 0 || keys_v[key[i]] != keys_v[key[i - 1]] ? 1ull : 0ull; }
};
struct ColHeadOut {
    const uint32_t* key;
    const uint64_t* keys_v;
    const int64_t* ids_v;
    int kind;
    uint64_t* start;
    uint64_t* values;
    int64_t* rep;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t in) const {
        if (in == ex) return;
        const uint32_t p = key[i];
        start[ex] = i;
        values[ex] = column_key_raw(kind, keys_v[p]);
        rep[ex] = ids_v[p];  // equal keys ascend by id and the positions are sorted: the run's first row has its smallest id
    }
};
// counts[g] = start[g + 1] - start[g], the last group ending at m
__global__ __launch_bounds__(256) void clu_counts_kernel(const uint64_t* __restrict__ start, uint64_t ng, uint64_t m, int64_t* __restrict__ counts) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < ng; g += stride)
        counts[g] = (int64_t)((g + 1 < ng ? start[g + 1] : m) - start[g]);
}

// dense: runs of equal keys of the built column (once per build) ...
struct RunHeadIn {
    const uint64_t* keys_v;
    __device__ __forceinline__ uint64_t operator()(uint64_t p) const { return p == 0 || keys_v[p] != keys_v[p - 1] ? 1ull : 0ull; }
};
struct RunHeadOut {
    uint64_t* run_start;
    __device__ __forceinline__ void operator()(uint64_t p, uint64_t ex, uint64_t in) const {
        if (in != ex) run_start[ex] = p;
    }
};
// ... the exclusive scan C[0 .. n] of the per-position counters ...
struct CntIn {
    const unsigned int* cnt;
    __device__ __forceinline__ uint64_t operator()(uint64_t p) const { return cnt[p]; }
};
struct CntOut {
    uint64_t* C;
    uint64_t n;
    __device__ __forceinline__ void operator()(uint64_t p, uint64_t ex, uint64_t in) const {
        C[p] = ex;
        if (p + 1 == n) C[n] = in;
    }
};
// ... and a group for every run that holds a counted row
struct RunHitIn {
    const uint64_t* run_start;  // [runs + 1]
    const uint64_t* C;
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const { return C[run_start[v + 1]] != C[run_start[v]] ? 1ull : 0ull; }
};
struct RunHitOut {
    const uint64_t* run_start;
    const uint64_t* C;
    const uint64_t* keys_v;
    const int64_t* ids_v;
    int kind;
    int64_t* counts;
    uint64_t* values;
    int64_t* rep;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t ex, uint64_t in) const {
        if (in == ex) return;
        const uint64_t s = run_start[v], e = run_start[v + 1], base = C[s];
        counts[ex] = (int64_t)(C[e] - base);
        values[ex] = column_key_raw(kind, keys_v[s]);
        uint64_t a = s, b = e;  // first position of the run with a counted row: ids ascend inside the run
        while (a < b) {
            const uint64_t m = (a + b) >> 1;
            if (C[m + 1] > base) b = m;
            else a = m + 1;
        }
        rep[ex] = ids_v[a];
    }
};

// ---- string indexes: the class table ---------------------------------------------------------------------------------------------
// entries of offset 0 in array order = the non-empty documents in the order of their whole text
template <typename T>
struct DocEntryIn {
    typename SaOf<T>::ptr sa;
    int bits;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return ((uint64_t)sa[i] >> bits) == 0 ? 1ull : 0ull; }
};
template <typename T>
struct DocEntryOut {
    typename SaOf<T>::ptr sa;
    uint64_t mask;
    uint32_t* list;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t in) const {
        if (in != ex) list[ex] = (uint32_t)((uint64_t)sa[i] & mask);
    }
};
// head[j] = document list[j] differs from list[j - 1]: same length, then bytes — a wavefront per pair, 64 bytes per step
__global__ __launch_bounds__(256) void clu_pair_kernel(const uint32_t* __restrict__ list, uint64_t m, const uint8_t* __restrict__ text,
                                                       const uint64_t* __restrict__ doc_start, uint8_t* __restrict__ head) {
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    const int lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < m; j += waves) {  // (j is uniform in the wavefront)
        bool diff = true;
        if (j > 0) {
            const uint32_t a = list[j - 1], b = list[j];
            const uint64_t sa = doc_start[a], sb = doc_start[b], la = doc_start[a + 1] - sa, lb = doc_start[b + 1] - sb;
            if (la == lb) {
                diff = false;
                for (uint64_t o = 0; o < la; o += 64) {
                    const bool ne = o + lane < la && text[sa + o + lane] != text[sb + o + lane];
                    if (__ballot(ne)) {
                        diff = true;
                        break;
                    }
                }
            }
        }
        if (lane == 0) head[j] = diff ? 1 : 0;
    }
}
struct ClassIn {
    const uint8_t* head;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return head[j]; }
};
struct ClassOut {
    const uint32_t* list;
    uint32_t first;  // 1 when class 0 is the empty document
    uint32_t* class_of_doc;
    uint32_t* class_rep;
    __device__ __forceinline__ void operator()(uint64_t j, uint64_t ex, uint64_t in) const {
        const uint32_t c = (uint32_t)(in - 1) + first, d = list[j];
        class_of_doc[d] = c;
        if (in != ex) class_rep[c] = d;
    }
};
// class 0 of a column with empty documents is represented by one of them (any: they are all alike)
__global__ __launch_bounds__(256) void clu_empty_rep_kernel(const uint64_t* __restrict__ doc_start, uint64_t ndocs, uint32_t* __restrict__ class_rep) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < ndocs; d += stride)
        if (doc_start[d + 1] == doc_start[d]) class_rep[0] = (uint32_t)d;
}
// bytes of document doc[g] to blob[ptr[g] ..): a wavefront per document
__global__ __launch_bounds__(256) void clu_gather_kernel(const uint32_t* __restrict__ doc, uint64_t ng, const uint8_t* __restrict__ text,
                                                         const uint64_t* __restrict__ doc_start, const uint64_t* __restrict__ ptr,
                                                         uint8_t* __restrict__ blob) {
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    const int lane = threadIdx.x & 63;
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < ng; g += waves) {
        const uint32_t d = doc[g];
        const uint64_t s = doc_start[d], len = doc_start[d + 1] - s, o = ptr[g];
        for (uint64_t k = lane; k < len; k += 64) blob[o + k] = text[s + k];
    }
}
__global__ __launch_bounds__(256) void clu_renumber_kernel(uint32_t* __restrict__ class_of_doc, uint64_t ndocs, const uint32_t* __restrict__ new_of_old) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < ndocs; d += stride) class_of_doc[d] = new_of_old[class_of_doc[d]];
}
// flag[0] = 1 unless the ids ascend strictly
__global__ __launch_bounds__(256) void clu_id_order_kernel(const int64_t* __restrict__ ids, uint64_t n, unsigned int* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i + 1 < n; i += stride) bad |= ids[i] >= ids[i + 1];
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
__global__ __launch_bounds__(256) void clu_id_keys_kernel(const int64_t* __restrict__ ids, uint64_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ doc) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        key[i] = (uint64_t)ids[i] ^ SIGN;
        doc[i] = (uint32_t)i;
    }
}
__global__ __launch_bounds__(256) void clu_unflip_kernel(const uint64_t* __restrict__ key, uint64_t n, int64_t* __restrict__ ids) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) ids[i] = (int64_t)(key[i] ^ SIGN);
}

// ---- string indexes: one call ------------------------------------------------------------------------------------------------------
// row i -> key[i] = class << rbits | id rank (the rank orders the rows of a class by id); an id the index does not hold gets class
// `nclasses`, behind every real one.  id_doc == nullptr: id_tab is d_ids itself and the rank is the document.
__global__ __launch_bounds__(256) void clu_str_lookup_kernel(const int64_t* __restrict__ ids, uint64_t nrows, const int64_t* __restrict__ id_tab,
                                                             const uint32_t* __restrict__ id_doc, uint64_t ndocs,
                                                             const uint32_t* __restrict__ class_of_doc, uint64_t nclasses, int rbits,
                                                             uint64_t* __restrict__ key, unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t miss = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nrows; i += stride) {
        const int64_t id = ids[i];
        const uint64_t r = lower_bound_id(id_tab, ndocs, id);
        const bool hit = r < ndocs && id_tab[r] == id;
        uint64_t k = nclasses << rbits;
        if (hit) k = ((uint64_t)class_of_doc[id_doc ? id_doc[r] : (uint32_t)r] << rbits) | r;
        miss += hit ? 0 : 1;
        key[i] = k;
    }
    miss = wave_sum(miss);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(out, (unsigned long long)miss);
}
struct StrHeadIn {
    const uint64_t* key;
    int rbits;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i == 0 || (key[i] >> rbits) != (key[i - 1] >> rbits) ? 1ull : 0ull; }
};
struct StrHeadOut {
    const uint64_t* key;
    int rbits;
    const int64_t* id_tab;
    const uint32_t* class_rep;
    uint64_t* start;
    int64_t* rep;
    uint32_t* rep_doc;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t in) const {
        if (in == ex) return;
        const uint64_t k = key[i];
        start[ex] = i;
        rep[ex] = id_tab[k & ((1ull << rbits) - 1)];  // the rows of a class are sorted by id rank
        rep_doc[ex] = class_rep[k >> rbits];
    }
};
struct LenIn {
    const uint32_t* doc;
    const uint64_t* doc_start;
    __device__ __forceinline__ uint64_t operator()(uint64_t g) const { return doc_start[doc[g] + 1] - doc_start[doc[g]]; }
};
struct PtrOut {
    uint64_t* ptr;
    uint64_t ng;
    __device__ __forceinline__ void operator()(uint64_t g, uint64_t ex, uint64_t in) const {
        ptr[g] = ex;
        if (g + 1 == ng) ptr[ng] = in;
    }
};

// the result arrays: host blocks of the result cache, filled from the device
using Clusters = ResultOwner<cdb_clusters, cdb_clusters_free>;

// ---- columns: host side ------------------------------------------------------------------------------------------------------------
void column_run_starts(cdb_column* c) {
    if (c->clu_generation == c->generation) return;
    Index& ws = c->ws;
    hipStream_t s = ws.stream;
    RunHeadIn in{c->keys_v.as<uint64_t>()};
    const int t = ws.prof.begin(s);
    const uint64_t runs = scan_totals<uint64_t>(s, ws.scan_partials, in, c->n, OpAdd{}, (uint64_t)0);
    DevBuf rs;
    rs.alloc((runs + 1) * 8);
    scan_apply<uint64_t>(s, ws.scan_partials, in, c->n, OpAdd{}, (uint64_t)0, RunHeadOut{rs.as<uint64_t>()});
    ws.prof.end(t, "clu_col_runs", c->n * 16 + runs * 8, s);
    CDB_HIP(hipMemcpyAsync(rs.as<uint64_t>() + runs, &c->n, 8, hipMemcpyHostToDevice, s));
    CDB_HIP(hipGetLastError());
    CDB_HIP(hipStreamSynchronize(s));  // (&c->n is read by the copy)
    c->clu_run_start = std::move(rs);
    c->clu_runs = runs;
    c->clu_generation = c->generation;
}

void column_cluster(cdb_column* c, RowIds ids, uint64_t nrows, Clusters& res) {
    Index& ws = c->ws;
    hipStream_t s = ws.stream;
    const double t0 = wall_ms();
    const uint64_t n = c->n;
    if (n == 0 || nrows == 0) {  // never built (or built empty): no groups, every row missing
        res.r.missing = nrows;
        res.r.counts = (int64_t*)host_alloc(0);
        res.r.rep_ids = (int64_t*)host_alloc(0);
        res.r.values = (uint64_t*)host_alloc(0);
        c->cluster_ms = wall_ms() - t0;
        return;
    }
    DevBuf d_ids, d_out;
    const int64_t* idp = resident_ids(s, d_ids, ids, nrows);
    d_out.alloc(64);
    const uint64_t init[5] = {0, 0, 0, ~0ull, ~0ull};
    CDB_HIP(hipMemcpyAsync(d_out.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    const int64_t* id_sorted = c->id_sorted.as<int64_t>();
    const uint32_t* vpos = c->vpos.as<uint32_t>();
    const uint64_t* keys_v = c->keys_v.as<uint64_t>();
    const int64_t* ids_v = c->ids_v.as<int64_t>();
    const uint64_t lookup_bytes = nrows * (8 + 8 * (uint64_t)bit_width64(n) + 4);
    if (c->kind == 0) {
        int t = ws.prof.begin(s);
        hipLaunchKernelGGL(clu_bool_kernel, dim3(grid_for(nrows)), dim3(256), 0, s, idp, nrows, id_sorted, vpos, n, c->n_false,
                           d_out.as<unsigned long long>());
        ws.prof.end(t, "clu_bool", lookup_bytes, s);
        CDB_HIP(hipGetLastError());
        uint64_t o[5];
        CDB_HIP(hipMemcpyAsync(o, d_out.p, sizeof(o), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        ws.prof.resolve();
        res.r.missing = o[0];
        res.r.counts = (int64_t*)host_alloc(16);
        res.r.rep_ids = (int64_t*)host_alloc(16);
        res.r.values = (uint64_t*)host_alloc(16);
        for (int v = 0; v < 2; ++v)
            if (o[1 + v]) {
                res.r.counts[res.r.ngroups] = (int64_t)o[1 + v];
                res.r.rep_ids[res.r.ngroups] = (int64_t)(o[3 + v] ^ SIGN);
                res.r.values[res.r.ngroups++] = (uint64_t)v;
            }
        c->cluster_ms = wall_ms() - t0;
        return;
    }
    // (the dense path counts rows per position in 32 bits)
    const bool dense = nrows < (1ull << 32) && (c->debug_cluster_path == 2 || (c->debug_cluster_path == 0 && nrows * DENSE_DEN > n * DENSE_NUM));
    DevBuf d_counts, d_rep, d_values;
    uint64_t ng = 0, missing = 0;
    if (dense) {
        ++c->dense_clusters;
        column_run_starts(c);
        DevBuf cnt, C;
        cnt.alloc(n * 4);
        C.alloc((n + 1) * 8);
        CDB_HIP(hipMemsetAsync(cnt.p, 0, n * 4, s));
        int t = ws.prof.begin(s);
        hipLaunchKernelGGL(clu_col_lookup_kernel, dim3(grid_for(nrows)), dim3(256), 0, s, idp, nrows, id_sorted, vpos, n, (uint32_t*)nullptr,
                           cnt.as<unsigned int>(), d_out.as<unsigned long long>());
        ws.prof.end(t, "clu_col_lookup", lookup_bytes + nrows * 4, s);
        t = ws.prof.begin(s);
        CntIn cin{cnt.as<unsigned int>()};
        scan_totals_device<uint64_t>(s, ws.scan_partials, cin, n, OpAdd{}, (uint64_t)0);
        scan_apply<uint64_t>(s, ws.scan_partials, cin, n, OpAdd{}, (uint64_t)0, CntOut{C.as<uint64_t>(), n});
        ws.prof.end(t, "clu_col_cnt_scan", n * 16, s);
        t = ws.prof.begin(s);
        RunHitIn rin{c->clu_run_start.as<uint64_t>(), C.as<uint64_t>()};
        ng = scan_totals<uint64_t>(s, ws.scan_partials, rin, c->clu_runs, OpAdd{}, (uint64_t)0);
        d_counts.alloc(ng * 8);
        d_rep.alloc(ng * 8);
        d_values.alloc(ng * 8);
        scan_apply<uint64_t>(s, ws.scan_partials, rin, c->clu_runs, OpAdd{}, (uint64_t)0,
                             RunHitOut{c->clu_run_start.as<uint64_t>(), C.as<uint64_t>(), keys_v, ids_v, c->kind, d_counts.as<int64_t>(),
                                       d_values.as<uint64_t>(), d_rep.as<int64_t>()});
        ws.prof.end(t, "clu_col_runs_hit", c->clu_runs * 48 + ng * 40, s);
        CDB_HIP(hipGetLastError());
        CDB_HIP(hipMemcpyAsync(&missing, d_out.p, 8, hipMemcpyDeviceToHost, s));
        res.r.counts = res.fetch<int64_t>(d_counts.p, ng);
        res.r.rep_ids = res.fetch<int64_t>(d_rep.p, ng);
        res.r.values = res.fetch<uint64_t>(d_values.p, ng);
        CDB_HIP(hipStreamSynchronize(s));
    } else {
        ++c->sparse_clusters;
        DevBuf k0, k1, start;
        k0.alloc(nrows * 4);
        k1.alloc(nrows * 4);
        int t = ws.prof.begin(s);
        hipLaunchKernelGGL(clu_col_lookup_kernel, dim3(grid_for(nrows)), dim3(256), 0, s, idp, nrows, id_sorted, vpos, n, k0.as<uint32_t>(),
                           (unsigned int*)nullptr, d_out.as<unsigned long long>());
        ws.prof.end(t, "clu_col_lookup", lookup_bytes + nrows * 4, s);
        CDB_HIP(hipGetLastError());
        int sel = 0;
        if (nrows > 1)  // (a missed row's key is n itself: bit_width(n) bits hold every key)
            sel = radix_sort<uint32_t, NoVal>(s, ws.rws, ws.prof, k0.as<uint32_t>(), k1.as<uint32_t>(), (NoVal*)nullptr, (NoVal*)nullptr, nrows, 0,
                                              bit_width64(n), nullptr);
        CDB_HIP(hipMemcpyAsync(&missing, d_out.p, 8, hipMemcpyDeviceToHost, s));
        radix_check_error(s, ws.rws);
        CDB_HIP(hipStreamSynchronize(s));
        const uint64_t m = nrows - missing;  // the rows the column holds come first
        const uint32_t* key = (sel ? k1 : k0).as<uint32_t>();
        t = ws.prof.begin(s);
        ColHeadIn hin{key, keys_v};
        ng = scan_totals<uint64_t>(s, ws.scan_partials, hin, m, OpAdd{}, (uint64_t)0);
        start.alloc(ng * 8);
        d_counts.alloc(ng * 8);
        d_rep.alloc(ng * 8);
        d_values.alloc(ng * 8);
        scan_apply<uint64_t>(s, ws.scan_partials, hin, m, OpAdd{}, (uint64_t)0,
                             ColHeadOut{key, keys_v, ids_v, c->kind, start.as<uint64_t>(), d_values.as<uint64_t>(), d_rep.as<int64_t>()});
        hipLaunchKernelGGL(clu_counts_kernel, dim3(grid_for(ng)), dim3(256), 0, s, (const uint64_t*)start.as<uint64_t>(), ng, m, d_counts.as<int64_t>());
        ws.prof.end(t, "clu_col_heads", m * 48 + ng * 40, s);
        CDB_HIP(hipGetLastError());
        res.r.counts = res.fetch<int64_t>(d_counts.p, ng);
        res.r.rep_ids = res.fetch<int64_t>(d_rep.p, ng);
        res.r.values = res.fetch<uint64_t>(d_values.p, ng);
        CDB_HIP(hipStreamSynchronize(s));
    }
    ws.prof.resolve();
    res.r.ngroups = ng;
    res.r.missing = missing;
    c->cluster_ms = wall_ms() - t0;
}

}  // namespace

// id -> document: the ids are insertion timestamps and usually ascend; otherwise a sorted copy
void cdb::id_table_prepare(Index& ix) {
    Index::IdTable& it = ix.idt;
    if (it.valid) return;
    hipStream_t s = ix.stream;
    const uint64_t ndocs = ix.ndocs;
    it.drop();
    DevBuf flag, id_sorted, id_doc;
    flag.alloc(16);
    CDB_HIP(hipMemsetAsync(flag.p, 0, 16, s));
    hipLaunchKernelGGL(clu_id_order_kernel, dim3(grid_for(ndocs)), dim3(256), 0, s, (const int64_t*)ix.d_ids.as<int64_t>(), ndocs, flag.as<unsigned int>());
    CDB_HIP(hipGetLastError());
    unsigned int unordered = 0;
    CDB_HIP(hipMemcpyAsync(&unordered, flag.p, 4, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    if (unordered) {
        DevBuf k0, k1, v0, v1;
        k0.alloc(ndocs * 8);
        k1.alloc(ndocs * 8);
        v0.alloc(ndocs * 4);
        v1.alloc(ndocs * 4);
        hipLaunchKernelGGL(clu_id_keys_kernel, dim3(grid_for(ndocs)), dim3(256), 0, s, (const int64_t*)ix.d_ids.as<int64_t>(), ndocs, k0.as<uint64_t>(),
                           v0.as<uint32_t>());
        const int sel = radix_sort<uint64_t, uint32_t>(s, ix.rws, ix.prof, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint32_t>(), v1.as<uint32_t>(),
                                                       ndocs, 0, 64, nullptr);
        id_sorted.alloc(ndocs * 8);
        hipLaunchKernelGGL(clu_unflip_kernel, dim3(grid_for(ndocs)), dim3(256), 0, s, (const uint64_t*)(sel ? k1 : k0).as<uint64_t>(), ndocs,
                           id_sorted.as<int64_t>());
        CDB_HIP(hipGetLastError());
        radix_check_error(s, ix.rws);
        CDB_HIP(hipStreamSynchronize(s));
        id_doc = std::move(sel ? v1 : v0);
    }
    it.id_sorted = std::move(id_sorted);
    it.id_doc = std::move(id_doc);
    it.ids_ascend = !unordered;
    it.valid = true;
}

namespace {

// ---- string indexes: host side -----------------------------------------------------------------------------------------------------
void cluster_prepare(Index& ix) {
    Index::ClusterTables& ct = ix.clu;
    if (ct.valid) return;
    const double t0 = wall_ms();
    hipStream_t s = ix.stream;
    const uint64_t ndocs = ix.ndocs, size = ix.size;
    ct.drop();
    DevBuf list, head, class_of_doc, class_rep;
    class_of_doc.alloc(ndocs * 4);
    CDB_HIP(hipMemsetAsync(class_of_doc.p, 0, std::max<uint64_t>(ndocs * 4, 4), s));  // (empty documents stay in class 0)
    // 1. the offset-0 entries in array order
    uint64_t nne = 0;
    sa_dispatch(ix, [&](auto tag) {
        using T = decltype(tag);
        DocEntryIn<T> in{ix.sa_view<T>(), (int)ix.bits};
        // (two brackets, kernels only: the host round trip for the total and the allocation of the list lie between them)
        const uint64_t entry_bytes = size * (ix.sa_packed ? 5 : (uint64_t)ix.width);
        int t = ix.prof.begin(s);
        scan_totals_device<uint64_t>(s, ix.scan_partials, in, size, OpAdd{}, (uint64_t)0);
        ix.prof.end(t, "clu_compact_count", entry_bytes, s);
        CDB_HIP(hipMemcpyAsync(&nne, ix.scan_partials.as<uint64_t>() + ceil_div(size, SC_TILE), 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        list.alloc(nne * 4);
        t = ix.prof.begin(s);
        scan_apply<uint64_t>(s, ix.scan_partials, in, size, OpAdd{}, (uint64_t)0, DocEntryOut<T>{ix.sa_view<T>(), ix.mask, list.as<uint32_t>()});
        ix.prof.end(t, "clu_compact_write", entry_bytes + nne * 4, s);
    });
    CDB_HIP(hipGetLastError());
    if (nne > ndocs) throw InternalError("cdb_cluster: more offset-0 entries than documents (internal)");
    const uint32_t first = nne < ndocs ? 1 : 0;  // empty documents have no suffix: they are class 0
    // 2. neighbours compared against the text, heads scanned into class numbers
    uint64_t nclasses = first;
    if (nne) {
        head.alloc(nne);
        int t = ix.prof.begin(s);
        hipLaunchKernelGGL(clu_pair_kernel, dim3((unsigned)std::min<uint64_t>(ceil_div(nne, 4), 16384)), dim3(256), 0, s,
                           (const uint32_t*)list.as<uint32_t>(), nne, ix.d_text, (const uint64_t*)ix.d_doc_start.as<uint64_t>(), head.as<uint8_t>());
        ix.prof.end(t, "clu_pairs", 2 * size, s);
        CDB_HIP(hipGetLastError());
        ClassIn cin{head.as<uint8_t>()};
        t = ix.prof.begin(s);
        const uint64_t nc = scan_totals<uint64_t>(s, ix.scan_partials, cin, nne, OpAdd{}, (uint64_t)0);
        nclasses += nc;
        class_rep.alloc(nclasses * 4);
        scan_apply<uint64_t>(s, ix.scan_partials, cin, nne, OpAdd{}, (uint64_t)0,
                             ClassOut{list.as<uint32_t>(), first, class_of_doc.as<uint32_t>(), class_rep.as<uint32_t>()});
        ix.prof.end(t, "clu_classes", nne * 10 + nc * 4, s);
    } else {
        class_rep.alloc(4);
    }
    if (first)
        hipLaunchKernelGGL(clu_empty_rep_kernel, dim3(grid_for(ndocs)), dim3(256), 0, s, (const uint64_t*)ix.d_doc_start.as<uint64_t>(), ndocs,
                           class_rep.as<uint32_t>());
    CDB_HIP(hipGetLastError());
    // 3. an array in the reference's order (bytes >= 0x80 under reference_compat) keeps equal documents together but not in
    // std::string order: the classes' representatives are sorted on the host — one download of one document per class
    bool resorted = false;
    if (!ix.sa_sorted && nclasses > 1) {
        std::vector<uint32_t> rep(nclasses);
        CDB_HIP(hipMemcpyAsync(rep.data(), class_rep.p, nclasses * 4, hipMemcpyDeviceToHost, s));
        DevBuf d_ptr, d_blob;
        d_ptr.alloc((nclasses + 1) * 8);
        LenIn lin{class_rep.as<uint32_t>(), ix.d_doc_start.as<uint64_t>()};
        const uint64_t total = scan_totals<uint64_t>(s, ix.scan_partials, lin, nclasses, OpAdd{}, (uint64_t)0);  // (synchronises: rep is here)
        scan_apply<uint64_t>(s, ix.scan_partials, lin, nclasses, OpAdd{}, (uint64_t)0, PtrOut{d_ptr.as<uint64_t>(), nclasses});
        d_blob.alloc(total);
        hipLaunchKernelGGL(clu_gather_kernel, dim3((unsigned)std::min<uint64_t>(ceil_div(nclasses, 4), 16384)), dim3(256), 0, s,
                           (const uint32_t*)class_rep.as<uint32_t>(), nclasses, ix.d_text, (const uint64_t*)ix.d_doc_start.as<uint64_t>(),
                           (const uint64_t*)d_ptr.as<uint64_t>(), d_blob.as<uint8_t>());
        CDB_HIP(hipGetLastError());
        std::vector<uint64_t> ptr(nclasses + 1);
        std::vector<char> blob(std::max<uint64_t>(total, 1));
        CDB_HIP(hipMemcpyAsync(ptr.data(), d_ptr.p, (nclasses + 1) * 8, hipMemcpyDeviceToHost, s));
        if (total) CDB_HIP(hipMemcpyAsync(blob.data(), d_blob.p, total, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        std::vector<uint32_t> order(nclasses), new_of_old(nclasses), new_rep(nclasses);
        std::iota(order.begin(), order.end(), 0u);
        auto text_of = [&](uint32_t c) { return std::string_view(blob.data() + ptr[c], (size_t)(ptr[c + 1] - ptr[c])); };
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return text_of(a) < text_of(b); });  // (char_traits<char>: unsigned bytes)
        for (uint32_t k = 0; k < nclasses; ++k) {
            new_of_old[order[k]] = k;
            new_rep[k] = rep[order[k]];
        }
        DevBuf d_map;
        d_map.alloc(nclasses * 4);
        CDB_HIP(hipMemcpyAsync(d_map.p, new_of_old.data(), nclasses * 4, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(class_rep.p, new_rep.data(), nclasses * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(clu_renumber_kernel, dim3(grid_for(ndocs)), dim3(256), 0, s, class_of_doc.as<uint32_t>(), ndocs,
                           (const uint32_t*)d_map.as<uint32_t>());
        CDB_HIP(hipGetLastError());
        CDB_HIP(hipStreamSynchronize(s));  // (the host vectors are read by the copies)
        resorted = true;
    }
    // 4. id -> document: its own once-per-array piece (cdb_render_rows needs it without the classes)
    id_table_prepare(ix);
    ix.prof.resolve();
    ct.class_of_doc = std::move(class_of_doc);
    ct.class_rep = std::move(class_rep);
    ct.nclasses = nclasses;
    ct.resorted = resorted;
    ct.prepare_ms = wall_ms() - t0;
    ct.valid = true;
}

void index_cluster(Index& ix, RowIds ids, uint64_t nrows, bool with_values, Clusters& res) {
    hipStream_t s = ix.stream;
    auto empty = [&] {
        res.r.missing = nrows;
        res.r.counts = (int64_t*)host_alloc(0);
        res.r.rep_ids = (int64_t*)host_alloc(0);
        if (with_values) {
            res.r.value_ptr = (uint64_t*)host_alloc(8, true);
            res.r.value_blob = (char*)host_alloc(0);
        }
    };
    if (ix.width == 0 || ix.ndocs == 0) {  // never built: no groups, every row missing (cdb_query answers {} there)
        empty();
        return;
    }
    cluster_prepare(ix);
    const double t0 = wall_ms();
    if (nrows == 0) {
        empty();
        ix.clu.last_ms = wall_ms() - t0;
        return;
    }
    const Index::ClusterTables& ct = ix.clu;
    const uint64_t ndocs = ix.ndocs, nclasses = ct.nclasses;
    const int rbits = std::max(1, bit_width64(ndocs - 1)), cbits = bit_width64(nclasses);
    if (rbits + cbits > 64) throw Error("cdb_cluster: too many distinct documents for one sort key");
    const int64_t* id_tab = ix.idt.ids_ascend ? ix.d_ids.as<int64_t>() : ix.idt.id_sorted.as<int64_t>();
    const uint32_t* id_doc = ix.idt.ids_ascend ? nullptr : ix.idt.id_doc.as<uint32_t>();
    DevBuf d_ids, d_out, k0, k1, start, d_counts, d_rep, d_repdoc;
    const int64_t* idp = resident_ids(s, d_ids, ids, nrows);
    d_out.alloc(16);
    CDB_HIP(hipMemsetAsync(d_out.p, 0, 16, s));
    k0.alloc(nrows * 8);
    k1.alloc(nrows * 8);
    int t = ix.prof.begin(s);
    hipLaunchKernelGGL(clu_str_lookup_kernel, dim3(grid_for(nrows)), dim3(256), 0, s, idp, nrows, id_tab, id_doc, ndocs,
                       (const uint32_t*)ct.class_of_doc.as<uint32_t>(), nclasses, rbits, k0.as<uint64_t>(), d_out.as<unsigned long long>());
    ix.prof.end(t, "clu_str_lookup", nrows * (8 + 8 * (uint64_t)bit_width64(ndocs) + 12), s);
    CDB_HIP(hipGetLastError());
    int sel = 0;
    if (nrows > 1)
        sel = radix_sort<uint64_t, NoVal>(s, ix.rws, ix.prof, k0.as<uint64_t>(), k1.as<uint64_t>(), (NoVal*)nullptr, (NoVal*)nullptr, nrows, 0,
                                          rbits + cbits, nullptr);
    uint64_t missing = 0;
    CDB_HIP(hipMemcpyAsync(&missing, d_out.p, 8, hipMemcpyDeviceToHost, s));
    radix_check_error(s, ix.rws);
    CDB_HIP(hipStreamSynchronize(s));
    const uint64_t m = nrows - missing;  // rows of ids the index does not hold carry the largest class: they come last
    const uint64_t* key = (sel ? k1 : k0).as<uint64_t>();
    t = ix.prof.begin(s);
    StrHeadIn hin{key, rbits};
    const uint64_t ng = scan_totals<uint64_t>(s, ix.scan_partials, hin, m, OpAdd{}, (uint64_t)0);
    start.alloc(ng * 8);
    d_counts.alloc(ng * 8);
    d_rep.alloc(ng * 8);
    d_repdoc.alloc(ng * 4);
    scan_apply<uint64_t>(s, ix.scan_partials, hin, m, OpAdd{}, (uint64_t)0,
                         StrHeadOut{key, rbits, id_tab, ct.class_rep.as<uint32_t>(), start.as<uint64_t>(), d_rep.as<int64_t>(), d_repdoc.as<uint32_t>()});
    hipLaunchKernelGGL(clu_counts_kernel, dim3(grid_for(ng)), dim3(256), 0, s, (const uint64_t*)start.as<uint64_t>(), ng, m, d_counts.as<int64_t>());
    ix.prof.end(t, "clu_str_heads", m * 32 + ng * 36, s);
    CDB_HIP(hipGetLastError());
    res.r.counts = res.fetch<int64_t>(d_counts.p, ng);
    res.r.rep_ids = res.fetch<int64_t>(d_rep.p, ng);
    if (with_values) {
        DevBuf d_ptr, d_blob;
        d_ptr.alloc((ng + 1) * 8);
        CDB_HIP(hipMemsetAsync(d_ptr.p, 0, 8, s));  // (no groups: value_ptr = {0})
        LenIn lin{d_repdoc.as<uint32_t>(), ix.d_doc_start.as<uint64_t>()};
        t = ix.prof.begin(s);
        const uint64_t total = scan_totals<uint64_t>(s, ix.scan_partials, lin, ng, OpAdd{}, (uint64_t)0);
        scan_apply<uint64_t>(s, ix.scan_partials, lin, ng, OpAdd{}, (uint64_t)0, PtrOut{d_ptr.as<uint64_t>(), ng});
        d_blob.alloc(total);
        if (ng)
            hipLaunchKernelGGL(clu_gather_kernel, dim3((unsigned)std::min<uint64_t>(ceil_div(ng, 4), 16384)), dim3(256), 0, s,
                               (const uint32_t*)d_repdoc.as<uint32_t>(), ng, ix.d_text, (const uint64_t*)ix.d_doc_start.as<uint64_t>(),
                               (const uint64_t*)d_ptr.as<uint64_t>(), d_blob.as<uint8_t>());
        ix.prof.end(t, "clu_str_values", ng * 28 + 2 * total, s);
        CDB_HIP(hipGetLastError());
        res.r.value_ptr = res.fetch<uint64_t>(d_ptr.p, ng + 1);
        res.r.value_blob = res.fetch<char>(d_blob.p, total);
        CDB_HIP(hipStreamSynchronize(s));  // (the device blocks go back to the pool behind this scope)
    }
    CDB_HIP(hipStreamSynchronize(s));
    ix.prof.resolve();
    res.r.ngroups = ng;
    res.r.missing = missing;
    ix.clu.last_ms = wall_ms() - t0;
}

void run_column_cluster(cdb_column* c, RowIds ids, uint64_t nrows, cdb_clusters* out) {
    std::lock_guard<std::mutex> g(c->ws.mu);
    DeviceScope scope(c->ws);
    Clusters res(c->ws.stream);
    column_cluster(c, ids, nrows, res);
    res.hand_over(out);
}
void run_index_cluster(Index& ix, RowIds ids, uint64_t nrows, bool with_values, cdb_clusters* out) {
    std::lock_guard<std::mutex> g(ix.mu);
    DeviceScope scope(ix);
    Clusters res(ix.stream);
    index_cluster(ix, ids, nrows, with_values, res);
    res.hand_over(out);
}

}  // namespace

void cdb::cluster_index_device_rows(cdb_index* h, const int64_t* d_ids, uint64_t nrows, bool with_values, cdb_clusters* out) {
    run_index_cluster(h->ix, RowIds{nullptr, d_ids}, nrows, with_values, out);
}
void cdb::cluster_column_device_rows(cdb_column* c, const int64_t* d_ids, uint64_t nrows, cdb_clusters* out) {
    run_column_cluster(c, RowIds{nullptr, d_ids}, nrows, out);
}

extern "C" {

int cdb_column_cluster(cdb_column* c, const int64_t* ids, uint64_t nrows, cdb_clusters* out) {
    if (!c || !out || (nrows && !ids)) return CDB_E_INVALID;
    *out = cdb_clusters{};
    return guarded_ix(c->ws, [&] { run_column_cluster(c, RowIds{ids, nullptr}, nrows, out); });
}

int cdb_cluster(cdb_index* h, const int64_t* ids, uint64_t nrows, int with_values, cdb_clusters* out) {
    if (!h || !out || (nrows && !ids)) return CDB_E_INVALID;
    *out = cdb_clusters{};
    return guarded_ix(h->ix, [&] { run_index_cluster(h->ix, RowIds{ids, nullptr}, nrows, with_values != 0, out); });
}

void cdb_clusters_free(cdb_clusters* r) {
    if (!r) return;
    host_free(r->counts);
    host_free(r->rep_ids);
    host_free(r->values);
    host_free(r->value_ptr);
    host_free(r->value_blob);
    std::memset(r, 0, sizeof(*r));
}

}  // extern "C"
