// rowset.hip — a filtered row set that stays on the device (include/coffeedb_gpu.h: cdb_filter, cdb_rowset_*): filter() of
// interface.cpp:46-148 runs once, and its consumers — `count`, `query` + `span`, `cluster`, the row list of `remove` — read the rows
// where they lie.  The row set owns copies of (ids, counts), ascending by id, and a work space of its own; nothing of the handles
// that produced it is referenced after cdb_filter has returned.
//
// The page [first, last) of the ranking (descending count compared as signed int64, ties ascending id) sorts only the rows it needs.
// With K = min(last, m): key = ~(count ^ 2^63), so a smaller key is a larger count.  At creation the pass over the counts keeps the
// OR and the AND of all keys: a byte in which the two agree is equal in every row and is never visited.  A radix select then walks
// the differing bytes from the top — per byte one histogram kernel over the rows that still match the prefix found so far (LDS bins,
// flushed with global atomics) and a one-workgroup kernel that picks the bin holding rank K - 1 — without a host round trip.  One
// stable compaction takes the rows with key < T and the first rows (in id order) with key == T that fill up K (two running counts:
// scan.h's U2 over ballot-ranked tiles; stable_tiles.h ranks one flag and synchronises for its total, this take needs two counts
// and no total); those K pairs are sorted and rows [first, K) go out.  K == m, or option debug_page_path = 2: every row is keyed
// and sorted (the sort path).  The page is made in two halves — rowset_page_device leaves ids and counts in device buffers,
// download_rows (host_io.h) fetches them — so that cdb_rowset_select (select.hip) can read the page's fields from the device ids.
#include <cstring>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"
#include "scan.h"

using namespace cdb;

namespace {

constexpr uint64_t SIGN = 1ull << 63;
// the device state, in 64-bit words
constexpr int ST_OR = 0, ST_AND = 1;  // creation: OR / AND of every row's key
constexpr int ST_PREFIX = 2;          // select: the threshold's visited bytes found so far ...
constexpr int ST_MASK = 3;            // ... and which bytes those are
constexpr int ST_SKIP = 4;            // ... and the rank still to skip among the rows that match the prefix
constexpr int ST_HIST = 8;            // 256 digit counters, zeroed by the kernel that reads them
constexpr int ST_WORDS = ST_HIST + 256;

__host__ __device__ __forceinline__ uint64_t page_key(int64_t count) { return ~((uint64_t)count ^ SIGN); }
__host__ __device__ __forceinline__ int64_t page_count(uint64_t key) { return (int64_t)(~key ^ SIGN); }

// ---- creation: the rows into the set's own arrays (src == dst: they are there already) and the key bits -------------------------
__global__ __launch_bounds__(256) void rs_adopt_kernel(const int64_t* __restrict__ src_ids, const int64_t* __restrict__ src_counts,
                                                       int64_t* dst_ids, int64_t* dst_counts, uint64_t n, unsigned long long* st) {
    const bool copy = src_counts != dst_counts;
    unsigned long long o = 0, a = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int64_t c = src_counts[i];
        if (copy) {
            dst_counts[i] = c;
            dst_ids[i] = src_ids[i];
        }
        const uint64_t k = page_key(c);
        o |= k;
        a &= k;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        o |= __shfl_xor(o, off);
        a &= __shfl_xor(a, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&st[ST_OR], o);
        atomicAnd(&st[ST_AND], a);
    }
}

// the $correlation filter (interface.cpp:137-143) as a compaction that keeps the id order
struct CorrKeepIn {
    const int64_t* counts;
    int64_t lo, hi;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return counts[r] >= lo && counts[r] < hi ? 1ull : 0ull; }
};
struct CorrKeepOut {
    const int64_t* ids;
    const int64_t* counts;
    int64_t* out_ids;
    int64_t* out_counts;
    __device__ __forceinline__ void operator()(uint64_t r, uint64_t ex, uint64_t in) const {
        if (in != ex) {
            out_ids[ex] = ids[r];
            out_counts[ex] = counts[r];
        }
    }
};

// ---- select --------------------------------------------------------------------------------------------------------------------
// digit histogram of the rows whose visited bytes equal the prefix; two counts per 16-byte load
__global__ __launch_bounds__(256) void pg_hist_kernel(const int64_t* __restrict__ counts, uint64_t n, int shift, unsigned long long* st) {
    __shared__ unsigned int bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = st[ST_PREFIX], pmask = st[ST_MASK];
    const longlong2* __restrict__ c2 = reinterpret_cast<const longlong2*>(counts);
    const uint64_t npairs = n >> 1;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < npairs; p += (uint64_t)gridDim.x * 256) {
        const longlong2 v = c2[p];
        const uint64_t k0 = page_key(v.x), k1 = page_key(v.y);
        if ((k0 & pmask) == prefix) atomicAdd(&bins[(k0 >> shift) & 255], 1u);
        if ((k1 & pmask) == prefix) atomicAdd(&bins[(k1 >> shift) & 255], 1u);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t k = page_key(counts[n - 1]);
        if ((k & pmask) == prefix) atomicAdd(&bins[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    const unsigned int b = bins[threadIdx.x];
    if (b) atomicAdd(&st[ST_HIST + threadIdx.x], (unsigned long long)b);
}
// one workgroup: the bin that holds the rank still to skip joins the prefix
__global__ __launch_bounds__(256) void pg_pick_kernel(int shift, unsigned long long* st) {
    __shared__ uint64_t s_buf[8];
    const uint64_t h = st[ST_HIST + threadIdx.x];
    st[ST_HIST + threadIdx.x] = 0;
    const uint64_t skip = st[ST_SKIP];
    uint64_t total;
    const uint64_t incl = block_scan_incl<uint64_t>(h, OpAdd{}, s_buf, total);  // (its barriers separate the reads above from the writes below)
    const uint64_t excl = incl - h;
    if (h && excl <= skip && skip < incl) {
        st[ST_PREFIX] |= (uint64_t)threadIdx.x << shift;
        st[ST_MASK] |= 0xFFull << shift;
        st[ST_SKIP] = skip - excl;
    }
}
// The take: rows below the threshold T, and of the rows equal to it the first `quota` in input (= id) order — a stable compaction
// with two running counts (U2: rows below T, rows equal to T).  A workgroup owns TK_TILE consecutive rows, a wave a quarter of
// them in steps of 64: lane = row, so a ballot gives the in-order rank inside a step and every load is one contiguous 512 bytes.
// pg_take_count leaves the tile sums where scan.h's scan of the partials expects them; pg_take_apply places the rows.
constexpr int TK_STEPS = 16;
constexpr int TK_TILE = 4 * TK_STEPS * 64;
__global__ __launch_bounds__(256) void pg_take_count_kernel(const int64_t* __restrict__ counts, uint64_t n, const unsigned long long* __restrict__ st,
                                                            U2* __restrict__ partials) {
    __shared__ unsigned int s_less[4], s_equal[4];
    const uint64_t mask = st[ST_MASK], t = st[ST_PREFIX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * TK_TILE + (uint64_t)wave * (TK_STEPS * 64);
    unsigned int less = 0, equal = 0;
#pragma unroll
    for (int j = 0; j < TK_STEPS; ++j) {
        const uint64_t i = wbase + (uint64_t)j * 64 + lane;
        if (i < n) {
            const uint64_t k = page_key(counts[i]) & mask;
            less += k < t ? 1u : 0u;
            equal += k == t ? 1u : 0u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        less += __shfl_xor(less, off);
        equal += __shfl_xor(equal, off);
    }
    if (lane == 0) {
        s_less[wave] = less;
        s_equal[wave] = equal;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        partials[blockIdx.x] = U2{(uint64_t)s_less[0] + s_less[1] + s_less[2] + s_less[3], (uint64_t)s_equal[0] + s_equal[1] + s_equal[2] + s_equal[3]};
}
__global__ __launch_bounds__(256) void pg_take_apply_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ counts, uint64_t n,
                                                            const unsigned long long* __restrict__ st, const U2* __restrict__ partials, uint64_t K,
                                                            uint64_t* __restrict__ key, uint64_t* __restrict__ val) {
    __shared__ unsigned int s_less[4], s_equal[4];
    const uint64_t mask = st[ST_MASK], t = st[ST_PREFIX], quota = st[ST_SKIP] + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * TK_TILE + (uint64_t)wave * (TK_STEPS * 64);
    const uint64_t below = (1ull << lane) - 1ull;  // the lanes in front of this one
    uint64_t k[TK_STEPS];
    unsigned int less = 0, equal = 0;  // wave totals (uniform)
#pragma unroll
    for (int j = 0; j < TK_STEPS; ++j) {
        const uint64_t i = wbase + (uint64_t)j * 64 + lane;
        const bool in = i < n;
        k[j] = in ? page_key(counts[i]) : 0;
        less += (unsigned int)__popcll(__ballot(in && (k[j] & mask) < t));
        equal += (unsigned int)__popcll(__ballot(in && (k[j] & mask) == t));
    }
    if (lane == 0) {
        s_less[wave] = less;
        s_equal[wave] = equal;
    }
    __syncthreads();
    U2 run = partials[blockIdx.x];  // rows in front of this wave's first row
    for (int w = 0; w < wave; ++w) {
        run.a += s_less[w];
        run.b += s_equal[w];
    }
    if (less == 0 && run.b >= quota) return;  // (uniform) nothing of this wave is taken
#pragma unroll
    for (int j = 0; j < TK_STEPS; ++j) {
        const uint64_t i = wbase + (uint64_t)j * 64 + lane;
        const bool in = i < n;
        const bool is_less = in && (k[j] & mask) < t, is_equal = in && (k[j] & mask) == t;
        const uint64_t bl = __ballot(is_less), be = __ballot(is_equal);
        const uint64_t ex_b = run.b + (uint64_t)__popcll(be & below);
        if (is_less || (is_equal && ex_b < quota)) {
            const uint64_t pos = run.a + (uint64_t)__popcll(bl & below) + (ex_b < quota ? ex_b : quota);
            if (pos < K) {  // (always, while the state is what the picks left)
                key[pos] = k[j];
                val[pos] = (uint64_t)ids[i];
            }
        }
        run.a += (uint64_t)__popcll(bl);
        run.b += (uint64_t)__popcll(be);
    }
}

// ---- sort path: every row keyed; and rows [first, K) of the sorted pairs written out ----------------------------------------------
__global__ __launch_bounds__(256) void pg_key_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ counts, uint64_t n,
                                                     uint64_t* __restrict__ key, uint64_t* __restrict__ val) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    key[r] = page_key(counts[r]);
    val[r] = (uint64_t)ids[r];
}
__global__ __launch_bounds__(256) void pg_out_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val, uint64_t first,
                                                     uint64_t n, int64_t* __restrict__ ids, int64_t* __restrict__ counts) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    ids[r] = (int64_t)val[first + r];
    counts[r] = page_count(key[first + r]);
}

}  // namespace

cdb_rowset* cdb::rowset_new(int device) {
    cdb_rowset* rs = new cdb_rowset();
    rs->ws.device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&rs->ws.stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        delete rs;
        throw DeviceError("cdb_rowset: no stream on the device");
    }
    return rs;
}

void cdb::rowset_delete(cdb_rowset* rs) {  // as cdb_column_destroy
    if (!rs) return;
    (void)hipSetDevice(rs->ws.device);
    hipStream_t s = rs->ws.stream;
    if (s) (void)hipStreamSynchronize(s);
    rs->ws.stream = nullptr;
    delete rs;  // (device blocks go back to the cache untagged: the stream is idle)
    if (s) {
        DevPool::get().retire_stream(s);
        (void)hipStreamDestroy(s);
    }
}

namespace {

// The key bits of the rows in rs->ids / rs->counts (src == nullptr), or of the rows (src_ids, src_counts) on their way into them,
// on stream s; synchronises.
void rowset_adopt(cdb_rowset* rs, hipStream_t s, const int64_t* src_ids, const int64_t* src_counts) {
    rs->state.alloc(ST_WORDS * 8);
    uint64_t init[ST_WORDS] = {};
    init[ST_AND] = ~0ull;
    CDB_HIP(hipMemcpyAsync(rs->state.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    int64_t* di = rs->ids.as<int64_t>();
    int64_t* dc = rs->counts.as<int64_t>();
    if (rs->m)
        hipLaunchKernelGGL(rs_adopt_kernel, dim3(grid_for(rs->m)), dim3(256), 0, s, src_ids ? src_ids : di, src_counts ? src_counts : dc, di, dc,
                           rs->m, rs->state.as<unsigned long long>());
    CDB_HIP(hipGetLastError());
    uint64_t bits[2];
    CDB_HIP(hipMemcpyAsync(bits, rs->state.p, sizeof(bits), hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));  // (init and bits are read / written by the copies)
    rs->key_diff = bits[ST_OR] & ~bits[ST_AND];
}

}  // namespace

void cdb::rowset_adopt_equal_counts(cdb_rowset* rs, hipStream_t s, int64_t count) {
    rs->state.alloc(ST_WORDS * 8);
    uint64_t init[ST_WORDS] = {};
    init[ST_OR] = init[ST_AND] = page_key(count);
    CDB_HIP(hipMemcpyAsync(rs->state.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    CDB_HIP(hipStreamSynchronize(s));  // (init is read by the copy)
    rs->key_diff = 0;
}

namespace {

// The automatic rule (profiles/bench_page.jsonl, one MI355X run over 2^16, 2^20 .. 2^24 rows, three count
// distributions, page ends from 10 to m / 2): below 2^22 rows both paths are bound by their launches and the sort path, which has
// fewer, wins (select / sort 1.00-1.34 at 2^16 and 2^20, 0.94-1.25 at 2^21); at 2^22 select wins every page end up to 1000
// (0.78-0.99) and stays within 7 % above; at 2^23 and 2^24 it takes 0.51-1.02 of the sort path's time.
constexpr uint64_t AUTO_SELECT_MIN_ROWS = 1ull << 22;
bool page_selects(const cdb_rowset* rs, uint64_t K) {
    if (rs->debug_page_path == 2 || K >= rs->m) return false;
    return rs->debug_page_path == 1 || rs->m >= AUTO_SELECT_MIN_ROWS;
}

}  // namespace

void cdb::rowset_page_device(cdb_rowset* rs, uint64_t first, uint64_t last, DevicePage& pg) {
    Index& ws = rs->ws;
    hipStream_t s = ws.stream;
    const uint64_t m = rs->m, K = std::min(last, m);
    pg.n = 0;
    if (first >= K) return;
    DevBuf &k0 = pg.k0, &k1 = pg.k1, &v0 = pg.v0, &v1 = pg.v1, &o_ids = pg.ids, &o_counts = pg.counts;
    const int64_t* d_ids = rs->ids.as<int64_t>();
    const int64_t* d_counts = rs->counts.as<int64_t>();
    unsigned long long* st = rs->state.as<unsigned long long>();
    const bool select = page_selects(rs, K);
    const uint64_t nsort = select ? K : m;
    k0.alloc(nsort * 8); k1.alloc(nsort * 8); v0.alloc(nsort * 8); v1.alloc(nsort * 8);
    if (select) {
        // prefix, mask, rank to skip; and the digit counters cleared (a page that failed between a histogram and its pick left some)
        uint64_t init[ST_WORDS - ST_PREFIX] = {};
        init[ST_SKIP - ST_PREFIX] = K - 1;
        CDB_HIP(hipMemcpyAsync(st + ST_PREFIX, init, sizeof(init), hipMemcpyHostToDevice, s));
        uint64_t passes = 0;
        // (eight workgroups per CU: every workgroup flushes up to 256 global atomics into the same 256 counters)
        const unsigned hist_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(ceil_div(m, 2), 256), 2048));
        for (int b = 7; b >= 0; --b) {
            if (((rs->key_diff >> (8 * b)) & 0xFF) == 0) continue;
            int t = ws.prof.begin(s);
            hipLaunchKernelGGL(pg_hist_kernel, dim3(hist_grid), dim3(256), 0, s, d_counts, m, 8 * b, st);
            ws.prof.end(t, "pg_hist", m * 8, s);
            t = ws.prof.begin(s);
            hipLaunchKernelGGL(pg_pick_kernel, dim3(1), dim3(256), 0, s, 8 * b, st);
            ws.prof.end(t, "pg_pick", 256 * 16 + 32, s);
            ++passes;
        }
        CDB_HIP(hipGetLastError());
        const int t = ws.prof.begin(s);
        const uint64_t nb = ceil_div(m, TK_TILE);
        ws.scan_partials.ensure(scan_partials_slots(nb) * sizeof(U2));
        hipLaunchKernelGGL(pg_take_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, d_counts, m, (const unsigned long long*)st, ws.scan_partials.as<U2>());
        scan_partials_inplace<U2, OpAdd>(s, ws.scan_partials, nb, OpAdd{}, U2{0, 0});
        hipLaunchKernelGGL(pg_take_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, d_ids, d_counts, m, (const unsigned long long*)st,
                           (const U2*)ws.scan_partials.as<U2>(), K, k0.as<uint64_t>(), v0.as<uint64_t>());
        ws.prof.end(t, "pg_take", m * 16 + K * 24, s);
        CDB_HIP(hipGetLastError());
        rs->select_passes = passes;
        ++rs->page_selects;
    } else {
        const int t = ws.prof.begin(s);
        hipLaunchKernelGGL(pg_key_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s, d_ids, d_counts, m, k0.as<uint64_t>(), v0.as<uint64_t>());
        ws.prof.end(t, "pg_key", m * 32, s);
        CDB_HIP(hipGetLastError());
        ++rs->page_sorts;
    }
    int sel = 0;
    if (nsort > 1)
        sel = radix_sort<uint64_t, uint64_t>(s, ws.rws, ws.prof, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint64_t>(), v1.as<uint64_t>(), nsort, 0,
                                             64, nullptr);
    const uint64_t n_out = K - first;
    o_ids.alloc(n_out * 8);
    o_counts.alloc(n_out * 8);
    const int t = ws.prof.begin(s);
    hipLaunchKernelGGL(pg_out_kernel, dim3((unsigned)ceil_div(n_out, 256)), dim3(256), 0, s, (const uint64_t*)(sel ? k1 : k0).as<uint64_t>(),
                       (const uint64_t*)(sel ? v1 : v0).as<uint64_t>(), first, n_out, o_ids.as<int64_t>(), o_counts.as<int64_t>());
    ws.prof.end(t, "pg_out", n_out * 32, s);
    CDB_HIP(hipGetLastError());
    radix_check_error(s, ws.rws);
    pg.n = n_out;
}

namespace {

void rowset_page(cdb_rowset* rs, uint64_t first, uint64_t last, int64_t** ids, int64_t** counts, size_t* nrows) {
    const double t0 = wall_ms();
    DevicePage pg;
    rowset_page_device(rs, first, last, pg);
    download_rows(rs->ws.stream, pg.ids.as<int64_t>(), pg.counts.as<int64_t>(), pg.n, ids, counts, nrows);
    if (pg.n) rs->ws.prof.resolve();
    rs->page_ms = wall_ms() - t0;
}

}  // namespace

extern "C" {

int cdb_filter(const cdb_key_query* keys, int nkeys, const cdb_column_key* cols, int ncols, int has_corr, int64_t corr_lo, int64_t corr_hi,
               cdb_rowset** out) {
    if (!out) return CDB_E_INVALID;
    *out = nullptr;
    Index* lead = filter_lead(keys, nkeys, cols, ncols);
    if (!lead) return CDB_E_INVALID;
    Index& ix = *lead;
    return guarded_ix(ix, [&] {
        cdb_rowset* rs = nullptr;
        try {
            // (the lead's locks are held inside; the row set's own arrays are filled on the lead's stream, which is idle on return)
            filter_rows_on_lead(ix, QUERY_AND_COLUMNS_NAMES, keys, nkeys, cols, ncols, false, 0, 0, 0, [&](hipStream_t s, DeviceCsr r) {
                rs = rowset_new(ix.device);
                const int64_t* q_ids = ix.q_ids.as<int64_t>();
                const int64_t* q_counts = ix.q_counts.as<int64_t>();
                if (has_corr && r.nrows) {
                    CorrKeepIn cin{q_counts, corr_lo, corr_hi};
                    rs->m = scan_totals<uint64_t>(s, ix.scan_partials, cin, r.nrows, OpAdd{}, (uint64_t)0);
                    rs->ids.alloc(rs->m * 8);
                    rs->counts.alloc(rs->m * 8);
                    if (rs->m == r.nrows) {  // every row passes: the copy below does
                        rowset_adopt(rs, s, q_ids, q_counts);
                        return;
                    }
                    scan_apply<uint64_t>(s, ix.scan_partials, cin, r.nrows, OpAdd{}, (uint64_t)0,
                                         CorrKeepOut{q_ids, q_counts, rs->ids.as<int64_t>(), rs->counts.as<int64_t>()});
                    CDB_HIP(hipGetLastError());
                    rowset_adopt(rs, s, nullptr, nullptr);
                } else {
                    rs->m = r.nrows;
                    rs->ids.alloc(rs->m * 8);
                    rs->counts.alloc(rs->m * 8);
                    rowset_adopt(rs, s, q_ids, q_counts);
                }
            });
        } catch (...) {
            (void)hipStreamSynchronize(ix.stream);  // (the row set's arrays were being filled on the lead's stream)
            rowset_delete(rs);
            throw;
        }
        *out = rs;
    });
}

void cdb_rowset_free(cdb_rowset* rs) { rowset_delete(rs); }

const char* cdb_rowset_last_error(const cdb_rowset* rs) {
    static thread_local std::string copy;
    return rs ? last_error_copy(rs->ws.err_mu, rs->ws.err, copy) : "null row set";
}

uint64_t cdb_rowset_size(const cdb_rowset* rs) { return rs ? rs->m : 0; }

int cdb_rowset_rows(cdb_rowset* rs, int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!rs || !ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    return guarded_ix(rs->ws, [&] {
        std::lock_guard<std::mutex> g(rs->ws.mu);
        DeviceScope scope(rs->ws);
        download_rows(rs->ws.stream, rs->ids.as<int64_t>(), rs->counts.as<int64_t>(), rs->m, ids, counts, nrows);
    });
}

int cdb_rowset_page(cdb_rowset* rs, uint64_t first, uint64_t last, int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!rs || !ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    return guarded_ix(rs->ws, [&] {
        std::lock_guard<std::mutex> g(rs->ws.mu);
        DeviceScope scope(rs->ws);
        rowset_page(rs, first, last, ids, counts, nrows);
    });
}

int cdb_rowset_cluster(cdb_rowset* rs, cdb_index* field, int with_values, cdb_clusters* out) {
    if (!rs || !field || !out) return CDB_E_INVALID;
    *out = cdb_clusters{};
    return guarded_ix(rs->ws, [&] {
        std::lock_guard<std::mutex> g(rs->ws.mu);
        if (field->ix.device != rs->ws.device) throw Error("cdb_rowset_cluster: the field lives on another GPU");
        const double t0 = wall_ms();
        cluster_index_device_rows(field, rs->ids.as<int64_t>(), rs->m, with_values != 0, out);
        rs->cluster_ms = wall_ms() - t0;
        ++rs->clusters;
    });
}

int cdb_rowset_cluster_column(cdb_rowset* rs, cdb_column* field, cdb_clusters* out) {
    if (!rs || !field || !out) return CDB_E_INVALID;
    *out = cdb_clusters{};
    return guarded_ix(rs->ws, [&] {
        std::lock_guard<std::mutex> g(rs->ws.mu);
        if (field->ws.device != rs->ws.device) throw Error("cdb_rowset_cluster_column: the field lives on another GPU");
        const double t0 = wall_ms();
        cluster_column_device_rows(field, rs->ids.as<int64_t>(), rs->m, out);
        rs->cluster_ms = wall_ms() - t0;
        ++rs->clusters;
    });
}

int cdb_rowset_get_stat(const cdb_rowset* rs, const char* name, double* value) {
    if (!rs || !name || !value) return CDB_E_INVALID;
    std::lock_guard<std::mutex> g(const_cast<cdb_rowset*>(rs)->ws.mu);  // (the counters change under the row set's lock)
    struct { const char* n; double v; } tab[] = {
        {"rows", (double)rs->m}, {"page_selects", (double)rs->page_selects}, {"page_sorts", (double)rs->page_sorts},
        {"select_passes", (double)rs->select_passes}, {"page_ms", rs->page_ms}, {"clusters", (double)rs->clusters},
        {"cluster_ms", rs->cluster_ms}, {"selects", (double)rs->selects}, {"select_ms", rs->select_ms},
        {"select_rows", (double)rs->select_rows}, {"removes", (double)rs->removes}, {"remove_fields", (double)rs->remove_fields},
        {"remove_ms", rs->remove_ms}, {"all_fields", (double)rs->all_fields}, {"all_input_rows", (double)rs->all_input_rows},
        {"all_ms", rs->all_ms},
    };
    for (auto& e : tab)
        if (!std::strcmp(e.n, name)) {
            *value = e.v;
            return CDB_OK;
        }
    return CDB_E_INVALID;
}

int cdb_debug_rowset_from_rows(int device, const int64_t* ids, const int64_t* counts, uint64_t n, cdb_rowset** out) {
    if (!out) return CDB_E_INVALID;
    *out = nullptr;
    if (n && (!ids || !counts)) return CDB_E_INVALID;
    if (!usable_device(device)) return CDB_E_DEVICE;
    std::mutex err_mu;  // (no handle exists yet to carry the text: the code is all the caller gets)
    std::string err;
    return guarded_call(err_mu, err, [&] {
        cdb_rowset* rs = rowset_new(device);
        try {
            DeviceScope scope(rs->ws);
            hipStream_t s = rs->ws.stream;
            rs->m = n;
            rs->ids.alloc(n * 8);
            rs->counts.alloc(n * 8);
            if (n) {
                CDB_HIP(hipMemcpyAsync(rs->ids.p, ids, n * 8, hipMemcpyHostToDevice, s));
                CDB_HIP(hipMemcpyAsync(rs->counts.p, counts, n * 8, hipMemcpyHostToDevice, s));
            }
            rowset_adopt(rs, s, nullptr, nullptr);
        } catch (...) {
            rowset_delete(rs);
            throw;
        }
        *out = rs;
    });
}

int cdb_debug_rowset_set_option(cdb_rowset* rs, const char* name, int64_t value) {
    if (!rs || !name) return CDB_E_INVALID;
    std::lock_guard<std::mutex> g(rs->ws.mu);
    if (!std::strcmp(name, "profile")) {
        rs->ws.prof.enabled = value != 0;
        return CDB_OK;
    }
    if (!std::strcmp(name, "debug_page_path") && value >= 0 && value <= 2) {
        rs->debug_page_path = (int)value;
        return CDB_OK;
    }
    return CDB_E_INVALID;
}

int cdb_debug_rowset_profile_dump(cdb_rowset* rs, char* buf, size_t cap) {
    if (!rs || !buf || cap == 0) return CDB_E_INVALID;
    return profile_dump(rs->ws, buf, cap) ? CDB_OK : CDB_E_INVALID;  // (a table cut short is an error, not a shorter table)
}

}  // extern "C"
