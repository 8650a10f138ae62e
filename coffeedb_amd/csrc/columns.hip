// columns.hip — numeric and bool columns on the device (include/coffeedb_gpu.h: cdb_column_*): the reference's bool_index /
// integer_index / double_index (index.cpp:63-74, 129-173) as sorted device arrays, their range keys resolved by binary search,
// the per-key OR of interface.cpp:78-113 and the AND with string keys (interface.cpp:114-146) without a host round trip.
//
// Layout of a built column of n rows (28 bytes per row):
//   keys_v[p]    u64  order-preserving key of the p-th row in (value, id) order (bool: in (value, insertion) order)
//   ids_v[p]     i64  its object id — what cdb_column_query copies out, a contiguous window per range
//   id_sorted[r] i64  the ids ascending (r = id rank)
//   vpos[r]      u32  position p of id rank r in keys_v / ids_v
// A range is a window [a, b) of positions.  Materialising the union of some windows ascending by id either gathers ids_v over the
// windows and sorts them (sparse), or streams r = 0 .. n-1 and keeps id_sorted[r] when vpos[r] lies in a window (dense: ascending
// and duplicate-free by construction).  A column key of an AND that is broader than the other keys is never materialised: the
// merged rows of the other keys are probed against it (id -> rank by binary search over id_sorted -> vpos -> windows).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"
#include "scan.h"
#include "shim/range_parse.h"  // the one restatement of the reference's range grammar (utility.h:49-86)

using namespace cdb;

namespace {

constexpr uint64_t SIGN = 1ull << 63;
constexpr uint64_t MAX_ROWS = COLUMN_MAX_ROWS;
// Dense when k > n * DENSE_NUM / DENSE_DEN (k = rows inside the windows, overlaps counted).  Measured on MI355X over 10^8 rows with
// timestamp ids, both paths forced at 19 selectivities from 0.2 % to 95 %: sparse still wins at 60 % (1.75 vs
// 1.78 ms), dense wins from 65 % on (1.81 vs 1.84 ms; 2.28 vs 2.59 ms at 95 %) — the crossover lies between, 5/8 is its middle.
constexpr uint64_t DENSE_NUM = 5, DENSE_DEN = 8;

// ---- keys --------------------------------------------------------------------------------------------------------------
// int64: v ^ 2^63; double: sign-flip order with -0.0 folded onto +0.0 (the two zeros compare equal in the reference's pairs and
// then order by id); bool: 0 / 1.  `raw` is the value's bit pattern.
__host__ __device__ __forceinline__ uint64_t order_key(int kind, uint64_t raw) {
    if (kind == 1) return raw ^ SIGN;
    if (kind == 2) {
        if ((raw << 1) == 0) raw = 0;
        return (raw & SIGN) ? ~raw : (raw | SIGN);
    }
    return raw ? 1 : 0;
}
template <int KIND> struct KeyVal;  // the value a key stands for, compared as the reference compares it
template <> struct KeyVal<1> {
    using T = int64_t;
    __device__ __forceinline__ static T get(uint64_t k) { return (int64_t)(k ^ SIGN); }
};
template <> struct KeyVal<2> {
    using T = double;
    __device__ __forceinline__ static T get(uint64_t k) { return __longlong_as_double((long long)((k & SIGN) ? (k ^ SIGN) : ~k)); }
};
template <> struct KeyVal<0> {
    using T = int64_t;
    __device__ __forceinline__ static T get(uint64_t k) { return (int64_t)k; }
};

// rows of this build: ids -> sortable (id ^ 2^63), the new rows' raw values -> keys
__global__ __launch_bounds__(256) void col_prepare_kernel(uint64_t* __restrict__ idk, uint64_t* __restrict__ key, uint64_t n,
                                                          uint64_t first_new, int kind) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        idk[i] ^= SIGN;
        if (i >= first_new) key[i] = order_key(kind, key[i]);
    }
}

// flag[0] = 1 when some id is smaller than its predecessor (the id sort is needed)
__global__ __launch_bounds__(256) void col_order_kernel(const uint64_t* __restrict__ idk, uint64_t n, unsigned int* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i + 1 < n; i += stride) bad |= idk[i] > idk[i + 1];
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void col_iota_kernel(uint32_t* __restrict__ v, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) v[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void col_iota64_kernel(uint64_t* __restrict__ v, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) v[i] = i;
}

// bool columns whose ids needed sorting: rank_of[insertion index] = id rank
__global__ __launch_bounds__(256) void col_rank_of_kernel(const uint64_t* __restrict__ perm, uint64_t n, uint32_t* __restrict__ rank_of) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) rank_of[perm[r]] = (uint32_t)r;
}

// id_sorted[r] = the id of rank r; a duplicate id sets dup[0] and leaves one of the offending ids in dup[1]
__global__ __launch_bounds__(256) void col_id_rank_kernel(const uint64_t* __restrict__ idk, uint64_t n, int64_t* __restrict__ id_sorted,
                                                          unsigned long long* __restrict__ dup) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
        const uint64_t k = idk[r];
        id_sorted[r] = (int64_t)(k ^ SIGN);
        if (r > 0 && idk[r - 1] == k) {
            atomicExch(dup + 1, (unsigned long long)(k ^ SIGN));
            atomicOr(dup, 1ull);
        }
    }
}

// position p of the key order carries c = id rank (numeric) or insertion index (bool, mapped through rank_of when the ids were
// not ascending): ids_v[p] = id of that row, vpos[its rank] = p
__global__ __launch_bounds__(256) void col_finalize_kernel(const uint32_t* __restrict__ carried, uint64_t n,
                                                           const uint32_t* __restrict__ rank_of, const int64_t* __restrict__ id_sorted,
                                                           int64_t* __restrict__ ids_v, uint32_t* __restrict__ vpos) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += stride) {
        const uint32_t c = carried[p];
        const uint32_t r = rank_of ? rank_of[c] : c;
        ids_v[p] = id_sorted[r];
        vpos[r] = (uint32_t)p;
    }
}

// ---- bounds ------------------------------------------------------------------------------------------------------------
// numeric_query (index.cpp:63-74): std::lower_bound over std::pair<T, int64_t> — the very bisection of libstdc++'s lower_bound
// with pair's C++20 operator< (the reference builds as C++20: synth-three-way, so a pair whose values are unordered is never
// less), on the values the keys stand for.  `a.first < b.first || (a.first == b.first && a.second < b.second)` is that order:
// for every non-NaN value (±0 included) it is the plain lexicographic one, and a NaN bound — range_parse.h hands "nan", "-nan"
// through std::from_chars — compares as neither less nor equal, exactly as in the reference.  One thread per bound; bound j =
// (value bits, tag).
template <int KIND>
__global__ __launch_bounds__(64) void col_bounds_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ ids, uint64_t n,
                                                        const uint64_t* __restrict__ bval, const int64_t* __restrict__ btag, uint32_t nb,
                                                        uint64_t* __restrict__ pos) {
    using T = typename KeyVal<KIND>::T;
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nb) return;
    T v;
    const uint64_t raw = bval[j];
    memcpy(&v, &raw, 8);
    const int64_t tag = btag[j];
    uint64_t first = 0, len = n;
    while (len > 0) {
        const uint64_t half = len >> 1, mid = first + half;
        const T mv = KeyVal<KIND>::get(keys[mid]);
        const bool less = mv < v || (mv == v && ids[mid] < tag);
        if (less) {
            first = mid + 1;
            len = len - half - 1;
        } else {
            len = half;
        }
    }
    pos[j] = first;
}

// ---- materialising a union of windows ------------------------------------------------------------------------------------
// disjoint windows [lo[w], hi[w]) ascending: is position p inside one?
__device__ __forceinline__ bool in_windows(uint64_t p, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi, uint32_t nw) {
    uint32_t a = 0, b = nw;  // first window with lo > p
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (lo[m] <= p) a = m + 1;
        else b = m;
    }
    return a > 0 && p < hi[a - 1];
}

// sparse: out[t] = sortable id of the t-th row inside the windows (window w owns t in [off[w], off[w + 1])).  The windows are the
// merged ones, so every position is gathered once and — ids being unique in a column — the sorted keys hold no duplicates: the
// "drop adjacent duplicates" step of a gather over the raw windows is not needed.
__global__ __launch_bounds__(256) void col_gather_kernel(const int64_t* __restrict__ ids_v, const uint64_t* __restrict__ wlo,
                                                         const uint64_t* __restrict__ off, uint32_t nw, uint64_t k,
                                                         uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < k; t += stride) {
        uint32_t a = 0, b = nw;  // last window with off <= t
        while (a < b) {
            const uint32_t m = (a + b) >> 1;
            if (off[m] <= t) a = m + 1;
            else b = m;
        }
        const uint32_t w = a - 1;
        out[t] = (uint64_t)ids_v[wlo[w] + (t - off[w])] ^ SIGN;
    }
}
__global__ __launch_bounds__(256) void col_unflip_kernel(const uint64_t* __restrict__ key, uint64_t k, int64_t* __restrict__ ids) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < k; t += stride) ids[t] = (int64_t)(key[t] ^ SIGN);
}
// dense: id rank r is kept when its position lies in a window
struct DenseIn {
    const uint32_t* vpos;
    const uint64_t* lo;
    const uint64_t* hi;
    uint32_t nw;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return in_windows(vpos[r], lo, hi, nw) ? 1ull : 0ull; }
};
struct DenseOut {
    const int64_t* id_sorted;
    int64_t* ids;
    __device__ __forceinline__ void operator()(uint64_t r, uint64_t ex, uint64_t in) const {
        if (in != ex) ids[ex] = id_sorted[r];
    }
};
// probe filter: merged row i (ascending id) survives when its id is in the column and the id's position lies in a window
struct ProbeIn {
    const int64_t* rows;
    const int64_t* id_sorted;
    uint64_t n;
    const uint32_t* vpos;
    const uint64_t* lo;
    const uint64_t* hi;
    uint32_t nw;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const int64_t id = rows[i];
        uint64_t a = 0, b = n;
        while (a < b) {
            const uint64_t m = (a + b) >> 1;
            if (id_sorted[m] < id) a = m + 1;
            else b = m;
        }
        return a < n && id_sorted[a] == id && in_windows(vpos[a], lo, hi, nw) ? 1ull : 0ull;
    }
};
struct ProbeOut {
    const int64_t* ids;
    const int64_t* counts;
    int64_t* oids;
    int64_t* ocounts;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t in) const {
        if (in != ex) {
            oids[ex] = ids[i];
            ocounts[ex] = counts[i];
        }
    }
};

// windows of one key: [a, b) per range as the reference's loops see them, and their union as disjoint ascending windows
struct Windows {
    std::vector<uint64_t> a, b;      // per range (b >= a)
    std::vector<uint64_t> lo, hi;    // merged
    uint64_t k = 0;                  // sum of b - a (overlaps counted)
};

// ---- build -------------------------------------------------------------------------------------------------------------
// Every row of the column — the previous build's, in its key order (for bool that is insertion order within each value, which the
// stable sort by value keeps ahead of the rows added since), then the staged ones — is sorted twice: by id (skipped when the ids
// already ascend: they are insertion timestamps), then stably by key carrying the id rank (bool: the insertion index), so that
// equal keys ascend by id (bool: keep insertion order).  column_sort_rows is that pair of sorts over rows already on the device
// (cdb_column_append sorts its batch with it), column_build feeds it the old rows and the staged ones and publishes.
}  // namespace

void cdb::column_sort_rows(cdb_column* c, DevBuf& idk0, DevBuf& key0, uint64_t n, uint64_t first_new, const char* who, ColumnArrays& out) {
    Index& ws = c->ws;
    hipStream_t s = ws.stream;
    Profiler& prof = ws.prof;
    const bool is_bool = c->kind == 0;
    const uint64_t cap = std::max<uint64_t>(n, 1);
    DevBuf idk1, key1, car0, car1, v0, v1, rank_of, flags;
    DevBuf ids_v, id_sorted, vpos;
    key1.alloc(cap * 8);
    flags.alloc(32);
    CDB_HIP(hipMemsetAsync(flags.p, 0, 32, s));
    int t = prof.begin(s);
    hipLaunchKernelGGL(col_prepare_kernel, dim3(grid_for(n)), dim3(256), 0, s, idk0.as<uint64_t>(), key0.as<uint64_t>(), n, first_new, c->kind);
    prof.end(t, "col_prepare", n * 16 + (n - first_new) * 8, s);
    t = prof.begin(s);
    hipLaunchKernelGGL(col_order_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)idk0.as<uint64_t>(), n, flags.as<unsigned int>());
    prof.end(t, "col_order", n * 8, s);
    unsigned int unordered = 0;
    CDB_HIP(hipMemcpyAsync(&unordered, flags.p, 4, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));

    const uint64_t* idk = idk0.as<uint64_t>();  // ids ascending (sortable form)
    uint64_t* kcur = key0.as<uint64_t>();       // the key of every carried index: id rank (numeric) / insertion index (bool)
    uint64_t* kspare = key1.as<uint64_t>();
    const uint32_t* rmap = nullptr;             // bool with sorted ids: insertion index -> id rank
    if (unordered && n > 1) {
        idk1.alloc(n * 8);
        if (!is_bool) {
            const int sel = radix_sort<uint64_t, uint64_t>(s, ws.rws, prof, idk0.as<uint64_t>(), idk1.as<uint64_t>(), key0.as<uint64_t>(),
                                                           key1.as<uint64_t>(), n, 0, 64, nullptr);
            idk = (sel ? idk1 : idk0).as<uint64_t>();
            kcur = (sel ? key1 : key0).as<uint64_t>();
            kspare = (sel ? key0 : key1).as<uint64_t>();
        } else {
            car0.alloc(n * 8);
            car1.alloc(n * 8);
            t = prof.begin(s);
            hipLaunchKernelGGL(col_iota64_kernel, dim3(grid_for(n)), dim3(256), 0, s, car0.as<uint64_t>(), n);
            prof.end(t, "col_iota", n * 8, s);
            const int sel = radix_sort<uint64_t, uint64_t>(s, ws.rws, prof, idk0.as<uint64_t>(), idk1.as<uint64_t>(), car0.as<uint64_t>(),
                                                           car1.as<uint64_t>(), n, 0, 64, nullptr);
            idk = (sel ? idk1 : idk0).as<uint64_t>();
            rank_of.alloc(n * 4);
            t = prof.begin(s);
            hipLaunchKernelGGL(col_rank_of_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)(sel ? car1 : car0).as<uint64_t>(), n,
                               rank_of.as<uint32_t>());
            prof.end(t, "col_rank_of", n * 12, s);
            rmap = rank_of.as<uint32_t>();
        }
    }
    out.id_sort_skipped = unordered ? 0 : 1;
    id_sorted.alloc(cap * 8);
    t = prof.begin(s);
    hipLaunchKernelGGL(col_id_rank_kernel, dim3(grid_for(n)), dim3(256), 0, s, idk, n, id_sorted.as<int64_t>(),
                       flags.as<unsigned long long>() + 1);
    prof.end(t, "col_id_rank", n * 16, s);
    unsigned long long dup[2] = {0, 0};
    CDB_HIP(hipMemcpyAsync(dup, flags.as<unsigned long long>() + 1, 16, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    if (dup[0]) throw Error(std::string(who) + ": duplicate object id " + std::to_string((long long)dup[1]) + " in one column");
    // by key, stable, carrying the id rank / insertion index
    v0.alloc(cap * 4);
    v1.alloc(cap * 4);
    t = prof.begin(s);
    hipLaunchKernelGGL(col_iota_kernel, dim3(grid_for(n)), dim3(256), 0, s, v0.as<uint32_t>(), n);
    prof.end(t, "col_iota", n * 4, s);
    int sel = 0;
    if (n > 1)
        sel = radix_sort<uint64_t, uint32_t>(s, ws.rws, prof, kcur, kspare, v0.as<uint32_t>(), v1.as<uint32_t>(), n, 0, is_bool ? 8 : 64,
                                             nullptr);
    const uint32_t* carried = (sel ? v1 : v0).as<uint32_t>();
    ids_v.alloc(cap * 8);
    vpos.alloc(cap * 4);
    t = prof.begin(s);
    hipLaunchKernelGGL(col_finalize_kernel, dim3(grid_for(n)), dim3(256), 0, s, carried, n, rmap, (const int64_t*)id_sorted.as<int64_t>(),
                       ids_v.as<int64_t>(), vpos.as<uint32_t>());
    prof.end(t, "col_finalize", n * 24 + (rmap ? n * 4 : 0), s);
    CDB_HIP(hipGetLastError());
    radix_check_error(s, ws.rws);
    // the sorted keys stay where the sort left them
    DevBuf& kbuf = (sel ? kspare : kcur) == key0.as<uint64_t>() ? key0 : key1;
    DevBuf keys_v = std::move(kbuf);
    // bool: rows with value false = the lower bound of (true, INT64_MIN)
    uint64_t n_false = 0;
    if (is_bool && n) {
        const uint64_t one = 1;
        const int64_t tag = INT64_MIN;
        flags.ensure(32);
        CDB_HIP(hipMemcpyAsync(flags.p, &one, 8, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(flags.as<uint64_t>() + 1, &tag, 8, hipMemcpyHostToDevice, s));
        t = prof.begin(s);
        hipLaunchKernelGGL(col_bounds_kernel<0>, dim3(1), dim3(64), 0, s, (const uint64_t*)keys_v.as<uint64_t>(),
                           (const int64_t*)ids_v.as<int64_t>(), n, (const uint64_t*)flags.as<uint64_t>(),
                           (const int64_t*)(flags.as<int64_t>() + 1), 1u, flags.as<uint64_t>() + 2);
        prof.end(t, "col_bounds", (uint64_t)bit_width64(n) * 16, s);
        CDB_HIP(hipMemcpyAsync(&n_false, flags.as<uint64_t>() + 2, 8, hipMemcpyDeviceToHost, s));
    }
    CDB_HIP(hipStreamSynchronize(s));
    prof.resolve();
    out.keys_v = std::move(keys_v);
    out.ids_v = std::move(ids_v);
    out.id_sorted = std::move(id_sorted);
    out.vpos = std::move(vpos);
    out.n = n;
    out.n_false = n_false;
}

void cdb::column_publish(cdb_column* c, ColumnArrays& a) {
    c->keys_v = std::move(a.keys_v);
    c->ids_v = std::move(a.ids_v);
    c->id_sorted = std::move(a.id_sorted);
    c->vpos = std::move(a.vpos);
    c->n = a.n;
    c->n_false = a.n_false;
    ++c->generation;  // (cluster.hip keeps a table per build)
}

void cdb::column_build(cdb_column* c, const char* who) {
    hipStream_t s = c->ws.stream;
    const double t0 = wall_ms();
    const uint64_t n_old = c->n, n_new = c->staged_ids.size(), n = n_old + n_new;
    if (n > MAX_ROWS) throw Error(std::string(who) + ": a column holds at most 2^32 - 1 rows");
    const uint64_t cap = std::max<uint64_t>(n, 1);
    DevBuf idk0, key0;
    idk0.alloc(cap * 8);
    key0.alloc(cap * 8);
    if (n_old) {
        CDB_HIP(hipMemcpyAsync(idk0.p, c->ids_v.p, n_old * 8, hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipMemcpyAsync(key0.p, c->keys_v.p, n_old * 8, hipMemcpyDeviceToDevice, s));
    }
    if (n_new) {
        CDB_HIP(hipMemcpyAsync(idk0.as<uint64_t>() + n_old, c->staged_ids.data(), n_new * 8, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(key0.as<uint64_t>() + n_old, c->staged_raw.data(), n_new * 8, hipMemcpyHostToDevice, s));
    }
    ColumnArrays a;
    column_sort_rows(c, idk0, key0, n, n_old, who, a);
    c->id_sort_skipped = a.id_sort_skipped;
    column_publish(c, a);
    c->staged_ids.clear();
    c->staged_ids.shrink_to_fit();
    c->staged_raw.clear();
    c->staged_raw.shrink_to_fit();
    c->build_ms = wall_ms() - t0;
}

namespace {

// ---- ranges -> windows -------------------------------------------------------------------------------------------------
std::string range_text(const char* blob, const uint64_t* offsets, uint64_t j) {
    return std::string(blob ? blob + offsets[j] : "", (size_t)(offsets[j + 1] - offsets[j]));
}

// host parse (range_parse.h, the reference's messages), device bounds (one thread per bound), windows back on the host
Windows column_windows(cdb_column* c, const std::vector<std::string>& ranges) {
    if (ranges.empty()) throw Error("The constraint list cannot be empty");  // interface.cpp:75-77
    Windows w;
    const size_t nr = ranges.size();
    w.a.resize(nr);
    w.b.resize(nr);
    if (c->kind == 0) {
        for (size_t j = 0; j < nr; ++j) {
            if (ranges[j] == "false") {
                w.a[j] = 0;
                w.b[j] = c->n_false;
            } else if (ranges[j] == "true") {
                w.a[j] = c->n_false;
                w.b[j] = c->n;
            } else {
                throw Error("Invalid query: \"" + ranges[j] + "\"");  // index.cpp:146
            }
        }
    } else {
        std::vector<uint64_t> val(2 * nr);
        std::vector<int64_t> tag(2 * nr);
        for (size_t j = 0; j < nr; ++j) {
            try {
                if (c->kind == 1) {
                    const auto [lo, hi] = cdb_shim::parse_range<int64_t>(ranges[j]);
                    std::memcpy(&val[2 * j], &lo.first, 8);
                    std::memcpy(&val[2 * j + 1], &hi.first, 8);
                    tag[2 * j] = lo.second;
                    tag[2 * j + 1] = hi.second;
                } else {
                    const auto [lo, hi] = cdb_shim::parse_range<double>(ranges[j]);
                    std::memcpy(&val[2 * j], &lo.first, 8);
                    std::memcpy(&val[2 * j + 1], &hi.first, 8);
                    tag[2 * j] = lo.second;
                    tag[2 * j + 1] = hi.second;
                }
            } catch (const Error&) {
                throw;
            } catch (const std::runtime_error& e) {
                throw Error(e.what());  // "Invalid range: ..." / "Invalid value: ..." verbatim: the caller's mistake, whatever its words
            }
        }
        const uint64_t nb = 2 * nr;
        if (nb > (1ull << 31)) throw Error("cdb_column: too many ranges in one key");
        std::vector<uint64_t> pos(nb, 0);
        if (c->n) {
            hipStream_t s = c->ws.stream;
            c->d_bounds.ensure(nb * 24);
            uint64_t* d_val = c->d_bounds.as<uint64_t>();
            int64_t* d_tag = c->d_bounds.as<int64_t>() + nb;
            uint64_t* d_pos = c->d_bounds.as<uint64_t>() + 2 * nb;
            CDB_HIP(hipMemcpyAsync(d_val, val.data(), nb * 8, hipMemcpyHostToDevice, s));
            CDB_HIP(hipMemcpyAsync(d_tag, tag.data(), nb * 8, hipMemcpyHostToDevice, s));
            const int t = c->ws.prof.begin(s);
            const dim3 grid((unsigned)ceil_div(nb, 64));
            if (c->kind == 1)
                hipLaunchKernelGGL(col_bounds_kernel<1>, grid, dim3(64), 0, s, (const uint64_t*)c->keys_v.as<uint64_t>(),
                                   (const int64_t*)c->ids_v.as<int64_t>(), c->n, (const uint64_t*)d_val, (const int64_t*)d_tag, (uint32_t)nb, d_pos);
            else
                hipLaunchKernelGGL(col_bounds_kernel<2>, grid, dim3(64), 0, s, (const uint64_t*)c->keys_v.as<uint64_t>(),
                                   (const int64_t*)c->ids_v.as<int64_t>(), c->n, (const uint64_t*)d_val, (const int64_t*)d_tag, (uint32_t)nb, d_pos);
            c->ws.prof.end(t, "col_bounds", nb * (uint64_t)bit_width64(c->n) * 16, s);
            CDB_HIP(hipGetLastError());
            CDB_HIP(hipMemcpyAsync(pos.data(), d_pos, nb * 8, hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
            c->ws.prof.resolve();
        }
        for (size_t j = 0; j < nr; ++j) {
            w.a[j] = pos[2 * j];
            w.b[j] = std::max(pos[2 * j], pos[2 * j + 1]);  // first < last or nothing (index.cpp:63-74)
        }
    }
    std::vector<std::pair<uint64_t, uint64_t>> iv;
    for (size_t j = 0; j < nr; ++j) {
        w.k += w.b[j] - w.a[j];
        if (w.b[j] > w.a[j]) iv.emplace_back(w.a[j], w.b[j]);
    }
    std::sort(iv.begin(), iv.end());
    for (const auto& [a, b] : iv) {
        if (!w.lo.empty() && a <= w.hi.back()) {
            w.hi.back() = std::max(w.hi.back(), b);
        } else {
            w.lo.push_back(a);
            w.hi.push_back(b);
        }
    }
    return w;
}

std::vector<std::string> ranges_of(const char* blob, const uint64_t* offsets, uint64_t nranges) {
    std::vector<std::string> r;
    r.reserve(nranges);
    for (uint64_t j = 0; j < nranges; ++j) r.push_back(range_text(blob, offsets, j));
    return r;
}

// merged windows on the device: lo[nw], hi[nw], off[nw + 1] (offsets of the windows' rows)
void upload_windows(hipStream_t s, const Windows& w, DevBuf& d) {
    const uint64_t nw = w.lo.size();
    std::vector<uint64_t> h(3 * nw + 1);
    uint64_t acc = 0;
    for (uint64_t i = 0; i < nw; ++i) {
        h[i] = w.lo[i];
        h[nw + i] = w.hi[i];
        h[2 * nw + i] = acc;
        acc += w.hi[i] - w.lo[i];
    }
    h[3 * nw] = acc;
    d.alloc(h.size() * 8);
    CDB_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, s));
}

// union of the windows ascending by id into `out` (on the column's stream, synchronised); returns the number of ids
uint64_t column_union(cdb_column* c, const Windows& w, DevBuf& out) {
    Index& ws = c->ws;
    hipStream_t s = ws.stream;
    const double t0 = wall_ms();
    out.ensure(16);
    c->last_union_ms = 0;
    if (w.k == 0) return 0;
    uint64_t km = 0;
    for (size_t i = 0; i < w.lo.size(); ++i) km += w.hi[i] - w.lo[i];
    const uint32_t nw = (uint32_t)w.lo.size();
    const bool dense = c->debug_query_path == 2 || (c->debug_query_path == 0 && w.k * DENSE_DEN > c->n * DENSE_NUM);
    DevBuf dw;
    upload_windows(s, w, dw);
    const uint64_t* d_lo = dw.as<uint64_t>();
    const uint64_t* d_hi = d_lo + nw;
    const uint64_t* d_off = d_lo + 2 * nw;
    uint64_t m = 0;
    if (dense) {
        ++c->dense_queries;
        DenseIn in{c->vpos.as<uint32_t>(), d_lo, d_hi, nw};
        const int t = ws.prof.begin(s);
        m = scan_totals<uint64_t>(s, ws.scan_partials, in, c->n, OpAdd{}, (uint64_t)0);
        out.ensure(std::max<uint64_t>(m, 1) * 8);
        scan_apply<uint64_t>(s, ws.scan_partials, in, c->n, OpAdd{}, (uint64_t)0, DenseOut{c->id_sorted.as<int64_t>(), out.as<int64_t>()});
        ws.prof.end(t, "col_dense", c->n * 8 + m * 16, s);
    } else {
        ++c->sparse_queries;
        DevBuf k0, k1;
        k0.alloc(km * 8);
        k1.alloc(km * 8);
        int t = ws.prof.begin(s);
        hipLaunchKernelGGL(col_gather_kernel, dim3(grid_for(km)), dim3(256), 0, s, (const int64_t*)c->ids_v.as<int64_t>(), d_lo, d_off, nw, km,
                           k0.as<uint64_t>());
        ws.prof.end(t, "col_gather", km * 16, s);
        const int sel = radix_sort<uint64_t, NoVal>(s, ws.rws, ws.prof, k0.as<uint64_t>(), k1.as<uint64_t>(), (NoVal*)nullptr, (NoVal*)nullptr,
                                                    km, 0, 64, nullptr);
        out.ensure(km * 8);
        t = ws.prof.begin(s);
        hipLaunchKernelGGL(col_unflip_kernel, dim3(grid_for(km)), dim3(256), 0, s, (const uint64_t*)(sel ? k1 : k0).as<uint64_t>(), km,
                           out.as<int64_t>());
        ws.prof.end(t, "col_unflip", km * 16, s);
        m = km;
    }
    CDB_HIP(hipGetLastError());
    radix_check_error(s, ws.rws);
    CDB_HIP(hipStreamSynchronize(s));
    c->last_union_ms = wall_ms() - t0;
    ws.prof.resolve();
    return m;
}

int64_t* download_ids(hipStream_t s, const int64_t* d, uint64_t n) {
    int64_t* h = (int64_t*)host_alloc(n * 8);
    try {
        if (n) {
            CDB_HIP(hipMemcpyAsync(h, d, n * 8, hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
        }
    } catch (...) {
        host_free(h);
        throw;
    }
    return h;
}

}  // namespace

std::vector<uint64_t> cdb::column_raw_values(int kind, const void* values, uint64_t n, const char* who) {
    std::vector<uint64_t> raw(n);
    if (kind == 0) {
        const uint8_t* v = (const uint8_t*)values;
        for (uint64_t i = 0; i < n; ++i) raw[i] = v[i] ? 1 : 0;
    } else {
        std::memcpy(raw.data(), values, n * 8);
        if (kind == 2)
            for (uint64_t i = 0; i < n; ++i)
                if (std::isnan(((const double*)values)[i]))
                    throw Error(std::string(who) + ": NaN is not a valid value (row " + std::to_string(i) + ")");
    }
    return raw;
}

// The host path of cdb_column_remove: the built rows come back in key order (bool: insertion order within each value, which the
// stable sort by value restores), join the rows staged since, the removed ids are dropped and the column's own build runs over
// the rest.  A failed build leaves the column as it was.
void cdb::column_remove_host(cdb_column* c, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing) {
    hipStream_t s = c->ws.stream;
    const uint64_t n_old = c->n, n_staged = c->staged_ids.size();
    std::vector<int64_t> all_ids(n_old + n_staged);
    std::vector<uint64_t> all_raw(n_old + n_staged);
    if (n_old) {
        CDB_HIP(hipMemcpyAsync(all_ids.data(), c->ids_v.p, n_old * 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(all_raw.data(), c->keys_v.p, n_old * 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < n_old; ++i) all_raw[i] = column_key_raw(c->kind, all_raw[i]);
    }
    std::copy(c->staged_ids.begin(), c->staged_ids.end(), all_ids.begin() + n_old);
    std::copy(c->staged_raw.begin(), c->staged_raw.end(), all_raw.begin() + n_old);
    std::vector<int64_t> held(all_ids), gone(ids, ids + nids);
    std::sort(held.begin(), held.end());
    std::sort(gone.begin(), gone.end());
    uint64_t miss = 0;
    for (int64_t id : gone) miss += std::binary_search(held.begin(), held.end(), id) ? 0 : 1;
    gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
    uint64_t kept = 0;
    for (uint64_t i = 0; i < all_ids.size(); ++i) {
        if (std::binary_search(gone.begin(), gone.end(), all_ids[i])) continue;
        all_ids[kept] = all_ids[i];
        all_raw[kept++] = all_raw[i];
    }
    const uint64_t dropped = all_ids.size() - kept;
    *removed = dropped;
    *missing = miss;
    if (!dropped) return;
    all_ids.resize(kept);
    all_raw.resize(kept);
    c->staged_ids.swap(all_ids);  // (all_ids / all_raw now hold the rows staged before the call)
    c->staged_raw.swap(all_raw);
    c->n = 0;
    try {
        column_build(c);
    } catch (...) {
        c->n = n_old;
        c->staged_ids.swap(all_ids);
        c->staged_raw.swap(all_raw);
        throw;
    }
}

extern "C" {

int cdb_column_create(cdb_column** out, int device, int kind) {
    if (!out) return CDB_E_INVALID;
    *out = nullptr;
    if (kind < 0 || kind > 2) return CDB_E_INVALID;
    if (!usable_device(device)) return CDB_E_DEVICE;
    cdb_column* c = new (std::nothrow) cdb_column();
    if (!c) return CDB_E_DEVICE;
    c->kind = kind;
    c->ws.device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->ws.stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return CDB_E_DEVICE;
    }
    *out = c;
    return CDB_OK;
}

void cdb_column_destroy(cdb_column* c) {
    if (!c) return;
    (void)hipSetDevice(c->ws.device);
    hipStream_t s = c->ws.stream;
    if (s) (void)hipStreamSynchronize(s);
    c->ws.stream = nullptr;
    delete c;  // (device blocks go back to the cache untagged: the stream is idle)
    if (s) {
        DevPool::get().retire_stream(s);
        (void)hipStreamDestroy(s);
    }
}

const char* cdb_column_last_error(const cdb_column* c) {
    static thread_local std::string copy;
    return c ? last_error_copy(c->ws.err_mu, c->ws.err, copy) : "null column";
}

int cdb_column_add_bulk(cdb_column* c, const int64_t* ids, const void* values, uint64_t n) {
    if (!c || (n && (!ids || !values))) return CDB_E_INVALID;
    return guarded_ix(c->ws, [&] {
        const std::vector<uint64_t> raw = column_raw_values(c->kind, values, n, "cdb_column_add_bulk");
        std::lock_guard<std::mutex> g(c->ws.mu);
        if (c->n + c->staged_ids.size() + n > MAX_ROWS) throw Error("cdb_column_add_bulk: a column holds at most 2^32 - 1 rows");
        c->staged_ids.insert(c->staged_ids.end(), ids, ids + n);
        c->staged_raw.insert(c->staged_raw.end(), raw.begin(), raw.end());
    });
}

int cdb_column_build(cdb_column* c) {
    if (!c) return CDB_E_INVALID;
    return guarded_ix(c->ws, [&] {
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope cs(c->ws);
        column_build(c);
    });
}

// Rows leave a column.  With no rows staged since the last build the four arrays are compacted on the device
// (column_maintain.hip); otherwise — and with debug_maintain_path = 2 — the host path below runs.
int cdb_column_remove(cdb_column* c, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing) {
    if (!c || (nids && !ids)) return CDB_E_INVALID;
    if (removed) *removed = 0;
    if (missing) *missing = 0;
    return guarded_ix(c->ws, [&] {
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope cs(c->ws);
        if (!nids) return;
        const double t0 = wall_ms();
        const bool device = c->staged_ids.empty() && c->debug_maintain_path != 2;
        if (device) {  // the two halves back to back (cdb_rowset_remove prepares every field before it commits any)
            ColumnRemoval r;
            r.t0 = t0;
            column_remove_prepare(c, RowIds{ids, nullptr}, nids, r);
            if (removed) *removed = r.removed;
            if (missing) *missing = r.missing;
            if (r.changed) column_remove_commit(c, r);
            return;
        }
        uint64_t rem = 0, miss = 0;
        column_remove_host(c, ids, nids, &rem, &miss);
        if (removed) *removed = rem;
        if (missing) *missing = miss;
        if (!rem) return;
        ++c->removes;
        ++c->remove_rebuilds;
        c->remove_rows = rem;
        c->remove_ms = wall_ms() - t0;
    });
}

int cdb_column_query(cdb_column* c, const char* range, size_t len, int64_t** ids, size_t* nrows) {
    if (!c || !ids || !nrows || (len && !range)) return CDB_E_INVALID;
    *ids = nullptr;
    *nrows = 0;
    return guarded_ix(c->ws, [&] {
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope cs(c->ws);
        const Windows w = column_windows(c, {std::string(range ? range : "", len)});
        const uint64_t a = w.a[0], cnt = w.b[0] - w.a[0];
        c->last_k = cnt;
        *ids = download_ids(c->ws.stream, c->ids_v.as<int64_t>() + a, cnt);
        *nrows = (size_t)cnt;
    });
}

int cdb_column_query_any(cdb_column* c, const char* blob, const uint64_t* offsets, uint64_t nranges, int64_t** ids, size_t* nrows) {
    if (!c || !ids || !nrows || (nranges && !offsets)) return CDB_E_INVALID;
    *ids = nullptr;
    *nrows = 0;
    return guarded_ix(c->ws, [&] {
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope cs(c->ws);
        const Windows w = column_windows(c, ranges_of(blob, offsets, nranges));
        c->last_k = w.k;
        DevBuf out;
        const uint64_t m = column_union(c, w, out);
        *ids = download_ids(c->ws.stream, out.as<int64_t>(), m);
        *nrows = (size_t)m;
    });
}

}  // extern "C"

// ---- the AND of cdb_query_and (capi_query.hip), cdb_query_and_columns and cdb_filter (rowset.hip), up to "rows in ix.q_ids / q_counts"
// The handle that runs the merge and carries the error: the first string key (as in cdb_query_and); without one, the first
// column.  nullptr: the keys are not a valid query (CDB_E_INVALID).
Index* cdb::filter_lead(const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols) {
    if (nkeys < 0 || ncols < 0 || nkeys + ncols < 1 || (nkeys && !keys) || (ncols && !cols)) return nullptr;
    for (int j = 0; j < ncols; ++j)
        if (!cols[j].column) return nullptr;
    Index* lead = nullptr;
    for (int k = 0; k < nkeys && !lead; ++k)
        if (keys[k].index) lead = &keys[k].index->ix;
    if (!lead) {
        if (ncols == 0) return nullptr;  // host rows only: that is cdb_query_and's domain (it needs a string key too)
        lead = &cols[0].column->ws;
    }
    return lead;
}

// Validates the keys, locks every handle and column involved, resolves the keys and merges them on the lead's stream; `consume`
// runs while the locks are held, with the rows in ix.q_ids / q_counts (ascending id, or filtered and ranked when `ranked`).
// `names` = the entry point the refusals speak for (cdb_query_and passes no column keys).
void cdb::filter_rows_on_lead(Index& ix, const FilterNames& names, const cdb_key_query* keys, int nkeys, const cdb_column_key* cols,
                              int ncols, bool ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit,
                              const std::function<void(hipStream_t, DeviceCsr)>& consume) {
    const std::string who = names.who;
    for (int k = 0; k < nkeys; ++k) {
        const cdb_key_query& q = keys[k];
        if (q.index) {
            if (q.index->ix.device != ix.device) throw Error(names.one_gpu);
            check_keywords(KeywordList{q.blob, q.offsets, q.nkw}, names.who, KW_LIST_NOT_EMPTY | KW_OFFSETS | KW_NONE_EMPTY);
        } else if (q.nrows && (!q.ids || !q.counts)) {
            throw Error(who + ": row list missing");
        }
    }
    for (int j = 0; j < ncols; ++j) {
        if (cols[j].column->ws.device != ix.device) throw Error(names.one_gpu);
        if (cols[j].nranges == 0) throw Error("The constraint list cannot be empty");
        if (!cols[j].offsets) throw Error(who + ": range offsets missing");
    }
    // every handle and column involved stays locked until the merge has read its rows (address order: no lock inversion)
    std::vector<std::mutex*> mus;
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].index) mus.push_back(&keys[k].index->ix.mu);
    for (int j = 0; j < ncols; ++j) mus.push_back(&cols[j].column->ws.mu);
    std::sort(mus.begin(), mus.end());
    mus.erase(std::unique(mus.begin(), mus.end()), mus.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    for (std::mutex* m : mus) locks.emplace_back(*m);

    // windows of every column key (the reference's range errors surface here)
    std::vector<Windows> wins(ncols);
    for (int j = 0; j < ncols; ++j) {
        cdb_column* c = cols[j].column;
        DeviceScope cs(c->ws);
        wins[j] = column_windows(c, ranges_of(cols[j].blob, cols[j].offsets, cols[j].nranges));
        c->last_k = wins[j].k;
    }
    DeviceScope lead_scope(ix);
    hipStream_t s = ix.stream;
    std::vector<DeviceRows> lists;
    std::vector<DevBuf> held;  // copies of rows that would be overwritten by a later query on the same handle
    uint64_t m_other = UINT64_MAX;
    for (int k = 0; k < nkeys; ++k) {
        const cdb_key_query& q = keys[k];
        DevBuf di, dc;
        uint64_t n = 0;
        if (q.index) {  // a string key: the OR of its keywords on its own handle and stream, the rows copied on the lead's
            Index& kx = q.index->ix;
            StreamScope kss(kx.stream);
            const Rebased kw = rebase(KeywordList{q.blob, q.offsets, q.nkw});
            const DeviceKeywords d = upload_keywords(kx, kw);
            const DeviceCsr r = query_or_on_device(kx, d.pat, d.offs, q.nkw);  // (synchronises)
            n = r.nrows;
            di.alloc(std::max<uint64_t>(n, 1) * 8);
            dc.alloc(std::max<uint64_t>(n, 1) * 8);
            if (n) {
                CDB_HIP(hipMemcpyAsync(di.p, kx.q_ids.p, n * 8, hipMemcpyDeviceToDevice, s));
                CDB_HIP(hipMemcpyAsync(dc.p, kx.q_counts.p, n * 8, hipMemcpyDeviceToDevice, s));
            }
        } else {  // rows resolved elsewhere (numeric / bool keys: index.cpp:63-74,129-173 return (id, 0) rows)
            n = q.nrows;
            di.alloc(std::max<uint64_t>(n, 1) * 8);
            dc.alloc(std::max<uint64_t>(n, 1) * 8);
            if (n) {
                CDB_HIP(hipMemcpyAsync(di.p, q.ids, n * 8, hipMemcpyHostToDevice, s));
                CDB_HIP(hipMemcpyAsync(dc.p, q.counts, n * 8, hipMemcpyHostToDevice, s));
            }
        }
        m_other = std::min(m_other, n);
        lists.push_back(DeviceRows{di.as<int64_t>(), dc.as<int64_t>(), n});
        held.push_back(std::move(di));
        held.push_back(std::move(dc));
    }
    CDB_HIP(hipStreamSynchronize(s));  // (host rows are pageable)
    // a column key no broader than the smallest other list is materialised and merged; a broader one filters the merge.  Among
    // the column keys only the narrowest can be the smallest list: it is materialised when no other key is smaller, the rest probe
    uint64_t k_min = UINT64_MAX;
    for (int j = 0; j < ncols; ++j) k_min = std::min(k_min, wins[j].k);
    std::vector<int> probes;
    for (int j = 0; j < ncols; ++j) {
        cdb_column* c = cols[j].column;
        if (wins[j].k == k_min && wins[j].k <= m_other) {
            DevBuf di, dc;
            uint64_t n = 0;
            {
                DeviceScope cs(c->ws);
                n = column_union(c, wins[j], di);
                ++c->materialised_keys;
            }
            dc.alloc(std::max<uint64_t>(n, 1) * 8);
            CDB_HIP(hipMemsetAsync(dc.p, 0, std::max<uint64_t>(n, 1) * 8, s));
            lists.push_back(DeviceRows{di.as<int64_t>(), dc.as<int64_t>(), n});
            held.push_back(std::move(di));
            held.push_back(std::move(dc));
        } else {
            probes.push_back(j);
        }
    }
    DeviceCsr r = and_merge_on_device(ix, lists, ranked && probes.empty(), corr_lo, corr_hi, limit);
    if (!probes.empty()) {
        for (int j : probes) {
            cdb_column* c = cols[j].column;
            ++c->probe_filters;
            if (r.nrows == 0) continue;
            DevBuf dw, oi, oc;
            upload_windows(s, wins[j], dw);
            const uint32_t nw = (uint32_t)wins[j].lo.size();
            ProbeIn in{ix.q_ids.as<int64_t>(), c->id_sorted.as<int64_t>(), c->n, c->vpos.as<uint32_t>(), dw.as<uint64_t>(),
                       dw.as<uint64_t>() + nw, nw};
            const int t = ix.prof.begin(s);
            const uint64_t m = scan_totals<uint64_t>(s, ix.scan_partials, in, r.nrows, OpAdd{}, (uint64_t)0);
            oi.alloc(std::max<uint64_t>(m, 1) * 8);
            oc.alloc(std::max<uint64_t>(m, 1) * 8);
            scan_apply<uint64_t>(s, ix.scan_partials, in, r.nrows, OpAdd{}, (uint64_t)0,
                                 ProbeOut{ix.q_ids.as<int64_t>(), ix.q_counts.as<int64_t>(), oi.as<int64_t>(), oc.as<int64_t>()});
            ix.prof.end(t, "col_probe", r.nrows * (16 + 2 * (uint64_t)bit_width64(c->n) * 8 + 8) + m * 16, s);
            if (m) {
                CDB_HIP(hipMemcpyAsync(ix.q_ids.p, oi.p, m * 8, hipMemcpyDeviceToDevice, s));
                CDB_HIP(hipMemcpyAsync(ix.q_counts.p, oc.p, m * 8, hipMemcpyDeviceToDevice, s));
            }
            CDB_HIP(hipGetLastError());
            CDB_HIP(hipStreamSynchronize(s));
            r.nrows = m;
        }
        if (ranked) r = rank_rows_on_device(ix, r, corr_lo, corr_hi, limit);
        else ix.prof.resolve();
    }
    consume(s, r);
}

extern "C" {

int cdb_query_and_columns(const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols, int ranked, int64_t corr_lo,
                          int64_t corr_hi, uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    Index* lead = filter_lead(keys, nkeys, cols, ncols);
    if (!lead) return CDB_E_INVALID;
    Index& ix = *lead;
    return guarded_ix(ix, [&] {
        filter_rows_on_lead(ix, QUERY_AND_COLUMNS_NAMES, keys, nkeys, cols, ncols, ranked != 0, corr_lo, corr_hi, limit,
                            [&](hipStream_t s, DeviceCsr r) {
                                download_rows(s, ix.q_ids.as<int64_t>(), ix.q_counts.as<int64_t>(), r.nrows, ids, counts, nrows);
                            });
    });
}

int cdb_column_get_stat(const cdb_column* c, const char* name, double* value) {
    if (!c || !name || !value) return CDB_E_INVALID;
    std::lock_guard<std::mutex> g(const_cast<cdb_column*>(c)->ws.mu);  // (the counters change under the column's lock)
    struct { const char* n; double v; } tab[] = {
        {"rows", (double)c->n}, {"staged_rows", (double)c->staged_ids.size()}, {"build_ms", c->build_ms},
        {"id_sort_skipped", (double)c->id_sort_skipped}, {"sparse_queries", (double)c->sparse_queries},
        {"dense_queries", (double)c->dense_queries}, {"probe_filters", (double)c->probe_filters},
        {"materialised_keys", (double)c->materialised_keys}, {"last_k", (double)c->last_k}, {"kind", (double)c->kind},
        {"last_union_ms", c->last_union_ms}, {"sparse_clusters", (double)c->sparse_clusters}, {"dense_clusters", (double)c->dense_clusters},
        {"cluster_ms", c->cluster_ms},
        {"appends", (double)c->appends}, {"append_merges", (double)c->append_merges}, {"append_rebuilds", (double)c->append_rebuilds},
        {"append_rows", (double)c->append_rows}, {"append_ms", c->append_ms}, {"append_id_concat", (double)c->append_id_concat},
        {"removes", (double)c->removes}, {"remove_compactions", (double)c->remove_compactions},
        {"remove_rebuilds", (double)c->remove_rebuilds}, {"remove_rows", (double)c->remove_rows}, {"remove_ms", c->remove_ms},
    };
    for (auto& e : tab)
        if (!std::strcmp(e.n, name)) {
            *value = e.v;
            return CDB_OK;
        }
    return CDB_E_INVALID;
}

int cdb_debug_column_set_option(cdb_column* c, const char* name, int64_t value) {
    if (!c || !name) return CDB_E_INVALID;
    std::lock_guard<std::mutex> g(c->ws.mu);
    if (!std::strcmp(name, "profile")) {
        c->ws.prof.enabled = value != 0;
        return CDB_OK;
    }
    if (!std::strcmp(name, "debug_query_path") && value >= 0 && value <= 2) {
        c->debug_query_path = (int)value;
        return CDB_OK;
    }
    if (!std::strcmp(name, "debug_cluster_path") && value >= 0 && value <= 2) {
        c->debug_cluster_path = (int)value;
        return CDB_OK;
    }
    if (!std::strcmp(name, "debug_maintain_path") && value >= 0 && value <= 2) {
        c->debug_maintain_path = (int)value;
        return CDB_OK;
    }
    if (!std::strcmp(name, "debug_fail_prepare")) {
        c->ws.debug_fail_prepare = value != 0;
        return CDB_OK;
    }
    if (!std::strcmp(name, "debug_fail_append_prepare")) {
        c->ws.debug_fail_append_prepare = value != 0;
        return CDB_OK;
    }
    return CDB_E_INVALID;
}

int cdb_debug_column_profile_dump(cdb_column* c, char* buf, size_t cap) {
    if (!c || !buf || cap == 0) return CDB_E_INVALID;
    (void)profile_dump(c->ws, buf, cap);
    return CDB_OK;
}

}  // extern "C"
