// debug_scan.hip — test hooks for the device-wide scan (scan.h) and the stable tile ranks built on it (stable_tiles.h), in a
// translation unit of their own like debug_sort.hip.  Nothing here is called by a production path; the hooks call scan_totals /
// scan_apply, scan_partials_inplace and tile_bases / TileRanker exactly as the production call sites do, with the production
// operators (scan.h), on a stream and scan partials of their own.  Host arrays in, host arrays out.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "index_impl.h"
#include "scan.h"
#include "stable_tiles.h"

using namespace cdb;

namespace {

std::mutex g_err_mu;
std::string g_err;

template <typename F>
int guarded_hook(const char* who, F&& f) {
    const int rc = guarded_call(g_err_mu, g_err, std::forward<F>(f));
    if (rc != CDB_OK) {
        std::lock_guard<std::mutex> g(g_err_mu);
        std::fprintf(stderr, "%s: %s\n", who, g_err.c_str());
    }
    return rc;
}

// the stream of one hook call; blocks released while it is current are handed back before it goes
struct CallStream {
    hipStream_t s = nullptr;
    explicit CallStream(int device) {
        if (device >= 0) CDB_HIP(hipSetDevice(device));
        CDB_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    ~CallStream() {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        DevPool::get().retire_stream(s);
        (void)hipStreamDestroy(s);
    }
    CallStream(const CallStream&) = delete;
    CallStream& operator=(const CallStream&) = delete;
};

template <typename T>
struct BothOut {  // what the scan hands its consumer, as it is
    T* ex;
    T* in;
    __device__ __forceinline__ void operator()(uint64_t i, const T& e, const T& c) const {
        ex[i] = e;
        in[i] = c;
    }
};

// scan_totals then scan_apply over `in`, as every two-phase call site runs them
template <typename T, typename In, typename Op>
void scan_both(hipStream_t s, DevBuf& partials, In in, uint64_t n, Op op, T identity, void* out_ex, void* out_in, void* out_total) {
    DevBuf d_ex, d_inc;
    d_ex.alloc(n * sizeof(T));
    d_inc.alloc(n * sizeof(T));
    const T total = scan_totals<T>(s, partials, in, n, op, identity);
    scan_apply<T>(s, partials, in, n, op, identity, BothOut<T>{d_ex.as<T>(), d_inc.as<T>()});
    CDB_HIP(hipGetLastError());
    if (n) {
        CDB_HIP(hipMemcpyAsync(out_ex, d_ex.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(out_in, d_inc.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
    }
    CDB_HIP(hipStreamSynchronize(s));
    if (out_total) std::memcpy(out_total, &total, sizeof(T));
}

template <typename T, typename Op>
void scan_array(hipStream_t s, DevBuf& partials, const void* h_in, uint64_t n, Op op, T identity, void* out_ex, void* out_in,
                void* out_total) {
    DevBuf d_in;
    d_in.alloc(n * sizeof(T));
    if (n) CDB_HIP(hipMemcpyAsync(d_in.p, h_in, n * sizeof(T), hipMemcpyHostToDevice, s));
    scan_both<T>(s, partials, PartialsIn<T>{d_in.as<T>()}, n, op, identity, out_ex, out_in, out_total);
}

constexpr unsigned char GUARD_BYTE = 0xA5;

// scan_partials_inplace over nb raw tile sums in a block of exactly scan_partials_slots(nb) elements (what scan_totals reserves) with
// `guard` poisoned elements behind it; the scratch behind slot nb starts out poisoned too
template <typename T, typename Op>
void partials_inplace(hipStream_t s, void* h_inout, uint64_t nb, uint64_t guard, Op op, T identity, int* guard_ok) {
    const uint64_t slots = scan_partials_slots(nb);
    DevBuf part;
    part.alloc((slots + guard) * sizeof(T));
    CDB_HIP(hipMemsetAsync(part.p, GUARD_BYTE, (slots + guard) * sizeof(T), s));
    if (nb) CDB_HIP(hipMemcpyAsync(part.p, h_inout, nb * sizeof(T), hipMemcpyHostToDevice, s));
    scan_partials_inplace<T, Op>(s, part, nb, op, identity);
    CDB_HIP(hipGetLastError());
    std::vector<unsigned char> g(guard * sizeof(T));
    CDB_HIP(hipMemcpyAsync(h_inout, part.p, (nb + 1) * sizeof(T), hipMemcpyDeviceToHost, s));
    if (guard) CDB_HIP(hipMemcpyAsync(g.data(), part.as<T>() + slots, guard * sizeof(T), hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    int ok = 1;
    for (unsigned char b : g) ok &= b == GUARD_BYTE;
    if (guard_ok) *guard_ok = ok;
}

struct ByteFlagged {
    const uint8_t* flags;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return flags[i] != 0; }
};

// pass B as rm_compact_kernel and the merge of append.hip run it; the rank of every slot is stored, flagged or not
__global__ __launch_bounds__(256) void dbg_ranks_kernel(const uint8_t* __restrict__ flags, uint64_t n, const uint64_t* __restrict__ tile_base,
                                                        uint64_t* __restrict__ out) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t i = tile_slot(k);
        const bool flag = i < n && flags[i] != 0;
        const uint64_t r = ranker.before(k, flag);
        if (i < n) out[i] = r;
    }
}

}  // namespace

extern "C" {

int cdb_debug_scan(int device, int kind, const void* in, uint64_t n, void* out_exclusive, void* out_inclusive, void* out_total) {
    if (kind < CDB_DEBUG_SCAN_U64_ADD || kind > CDB_DEBUG_SCAN_FLAGS_ADD || (n && (!in || !out_exclusive || !out_inclusive)))
        return CDB_E_INVALID;
    return guarded_hook("cdb_debug_scan", [&] {
        CallStream cs(device);
        hipStream_t s = cs.s;
        StreamScope sscope(s);
        DevBuf partials;
        switch (kind) {
        case CDB_DEBUG_SCAN_U64_ADD: scan_array<uint64_t>(s, partials, in, n, OpAdd{}, (uint64_t)0, out_exclusive, out_inclusive, out_total); break;
        case CDB_DEBUG_SCAN_U64_MAX: scan_array<uint64_t>(s, partials, in, n, OpMax{}, (uint64_t)0, out_exclusive, out_inclusive, out_total); break;
        case CDB_DEBUG_SCAN_U2_ADD: scan_array<U2>(s, partials, in, n, OpAdd{}, U2{0, 0}, out_exclusive, out_inclusive, out_total); break;
        case CDB_DEBUG_SCAN_U2_SUMMAX: scan_array<U2>(s, partials, in, n, OpSumMax{}, U2{0, 0}, out_exclusive, out_inclusive, out_total); break;
        case CDB_DEBUG_SCAN_DOCMAX: scan_array<DocMax>(s, partials, in, n, OpDocMax{}, DocMax{~0ull, 0}, out_exclusive, out_inclusive, out_total); break;
        default: {  // the build's group flags, one byte each, fetched by FlagIn::load8 (a library allocation: 16-byte aligned)
            DevBuf d_flags;
            d_flags.alloc(n);
            if (n) CDB_HIP(hipMemcpyAsync(d_flags.p, in, n, hipMemcpyHostToDevice, s));
            scan_both<U2>(s, partials, FlagIn{d_flags.as<uint8_t>()}, n, OpAdd{}, U2{0, 0}, out_exclusive, out_inclusive, out_total);
        }
        }
    });
}

int cdb_debug_scan_partials(int device, int kind, void* partials_inout, uint64_t nb, uint64_t guard_words, int* out_guard_ok) {
    if (out_guard_ok) *out_guard_ok = 0;
    if (kind < CDB_DEBUG_SCAN_U64_ADD || kind > CDB_DEBUG_SCAN_DOCMAX || !partials_inout || nb >= (1ull << 31) || guard_words > (1ull << 24))
        return CDB_E_INVALID;
    return guarded_hook("cdb_debug_scan_partials", [&] {
        CallStream cs(device);
        hipStream_t s = cs.s;
        StreamScope sscope(s);
        switch (kind) {
        case CDB_DEBUG_SCAN_U64_ADD: partials_inplace<uint64_t>(s, partials_inout, nb, guard_words, OpAdd{}, (uint64_t)0, out_guard_ok); break;
        case CDB_DEBUG_SCAN_U64_MAX: partials_inplace<uint64_t>(s, partials_inout, nb, guard_words, OpMax{}, (uint64_t)0, out_guard_ok); break;
        case CDB_DEBUG_SCAN_U2_ADD: partials_inplace<U2>(s, partials_inout, nb, guard_words, OpAdd{}, U2{0, 0}, out_guard_ok); break;
        case CDB_DEBUG_SCAN_U2_SUMMAX: partials_inplace<U2>(s, partials_inout, nb, guard_words, OpSumMax{}, U2{0, 0}, out_guard_ok); break;
        default: partials_inplace<DocMax>(s, partials_inout, nb, guard_words, OpDocMax{}, DocMax{~0ull, 0}, out_guard_ok);
        }
    });
}

int cdb_debug_stable_ranks(int device, const uint8_t* flags, uint64_t n, uint64_t* out_before, uint64_t* out_tile_base, uint64_t* out_total) {
    // (tile_bases would launch an empty grid for an empty array; its callers never pass one)
    if (n == 0 || !flags || !out_before || !out_tile_base) return CDB_E_INVALID;
    return guarded_hook("cdb_debug_stable_ranks", [&] {
        CallStream cs(device);
        hipStream_t s = cs.s;
        StreamScope sscope(s);
        Index ix;  // what tile_bases takes from a handle: its stream, scan partials and (switched off) profiler
        CDB_HIP(hipGetDevice(&ix.device));
        ix.stream = s;
        const uint64_t ntiles = ceil_div(n, ST_TILE);
        DevBuf d_flags, d_out, tile_base;
        d_flags.alloc(n);
        d_out.alloc(n * 8);
        CDB_HIP(hipMemcpyAsync(d_flags.p, flags, n, hipMemcpyHostToDevice, s));
        const uint64_t total = tile_bases(ix, "debug_stable_ranks", ByteFlagged{d_flags.as<uint8_t>()}, n, tile_base, "dbg_count", n + ntiles * 8);
        hipLaunchKernelGGL(dbg_ranks_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, (const uint8_t*)d_flags.as<uint8_t>(), n,
                           (const uint64_t*)tile_base.as<uint64_t>(), d_out.as<uint64_t>());
        CDB_HIP(hipGetLastError());
        CDB_HIP(hipMemcpyAsync(out_before, d_out.p, n * 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(out_tile_base, tile_base.p, ntiles * 8, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        if (out_total) *out_total = total;
    });
}

}  // extern "C"
