// debug_carried.hip — test hook for the in-place carried round (carried_inplace.h: sa_carried_inplace_kernel), in a translation
// unit of its own like debug_scan.hip and debug_sweep.hip.  Nothing here is called by a production path; the hook launches the
// kernel through launch_carried_inplace exactly as refine_groups does, with the production array accessors (Sa40RW, SaRW<V>), on a
// stream of its own, between poisoned guards.  Host arrays in, host arrays out.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "index_impl.h"
#include "scan.h"
#include "carried_inplace.h"

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

constexpr unsigned char GUARD_BYTE = 0xA5;
constexpr uint64_t GUARD = 4096;  // poisoned bytes in front of and behind every array (a multiple of 16: the flag loader's alignment)

// a device array of `bytes` bytes between two poisoned guards
struct Guarded {
    DevBuf buf;
    uint64_t bytes = 0;
    void alloc(hipStream_t s, uint64_t b) {
        bytes = b;
        buf.alloc(b + 2 * GUARD);
        CDB_HIP(hipMemsetAsync(buf.p, GUARD_BYTE, b + 2 * GUARD, s));
    }
    char* data() { return static_cast<char*>(buf.p) + GUARD; }
    void upload(hipStream_t s, const void* h) {
        if (bytes) CDB_HIP(hipMemcpyAsync(data(), h, bytes, hipMemcpyHostToDevice, s));
    }
    void download(hipStream_t s, void* h) {
        if (bytes) CDB_HIP(hipMemcpyAsync(h, data(), bytes, hipMemcpyDeviceToHost, s));
    }
    bool guards_intact(hipStream_t s) {
        std::vector<unsigned char> g(2 * GUARD);
        CDB_HIP(hipMemcpyAsync(g.data(), buf.p, GUARD, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(g.data() + GUARD, data() + bytes, GUARD, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        bool ok = true;
        for (unsigned char b : g) ok &= b == GUARD_BYTE;
        return ok;
    }
};

}  // namespace

extern "C" {

int cdb_debug_carried_inplace(int device, int form, uint64_t* entries_inout, uint8_t* flags_inout, uint64_t n, int xbits,
                              uint64_t* out_partials, uint64_t* out_counts, int* out_guard_ok) {
    if (out_guard_ok) *out_guard_ok = 0;
    if (form < CDB_DEBUG_CARRIED_PACKED40 || form > CDB_DEBUG_CARRIED_U64 || n == 0 || n >= (1ull << 31) || xbits < 1 || xbits > 6 ||
        !entries_inout || !flags_inout || !out_partials || !out_counts)
        return CDB_E_INVALID;
    return guarded_hook("cdb_debug_carried_inplace", [&] {
        CallStream cs(device);
        hipStream_t s = cs.s;
        StreamScope sscope(s);
        const uint64_t nb = ceil_div(n, (uint64_t)SC_TILE);
        Guarded d_flags, d_lo, d_hi, d_part, d_cnt;
        d_flags.alloc(s, n);
        d_flags.upload(s, flags_inout);
        // (the partials block is the one scan_totals_from_partials scans behind the sweep: a slot per tile, the scan's scratch behind)
        d_part.alloc(s, scan_partials_slots(nb) * sizeof(U2));
        d_cnt.alloc(s, CI_COUNT_SLOTS * sizeof(unsigned long long));
        CDB_HIP(hipMemsetAsync(d_cnt.data(), 0, CI_COUNT_SLOTS * sizeof(unsigned long long), s));
        std::vector<uint32_t> lo;
        std::vector<uint8_t> hi;
        if (form == CDB_DEBUG_CARRIED_U64) {
            d_lo.alloc(s, n * 8);
            d_lo.upload(s, entries_inout);
        } else {
            lo.resize(n);
            for (uint64_t i = 0; i < n; ++i) lo[i] = (uint32_t)entries_inout[i];
            d_lo.alloc(s, n * 4);
            d_lo.upload(s, lo.data());
            if (form == CDB_DEBUG_CARRIED_PACKED40) {
                hi.resize(n);
                for (uint64_t i = 0; i < n; ++i) hi[i] = (uint8_t)(entries_inout[i] >> 32);
                d_hi.alloc(s, n);
                d_hi.upload(s, hi.data());
            }
        }
        uint8_t* const fl = reinterpret_cast<uint8_t*>(d_flags.data());
        U2* const part = reinterpret_cast<U2*>(d_part.data());
        unsigned long long* const cnt = reinterpret_cast<unsigned long long*>(d_cnt.data());
        if (form == CDB_DEBUG_CARRIED_PACKED40)
            launch_carried_inplace(s, fl, n, xbits, Sa40RW{reinterpret_cast<uint32_t*>(d_lo.data()), reinterpret_cast<uint8_t*>(d_hi.data())}, part, cnt);
        else if (form == CDB_DEBUG_CARRIED_U32)
            launch_carried_inplace(s, fl, n, xbits, SaRW<uint32_t>{reinterpret_cast<uint32_t*>(d_lo.data())}, part, cnt);
        else
            launch_carried_inplace(s, fl, n, xbits, SaRW<uint64_t>{reinterpret_cast<uint64_t*>(d_lo.data())}, part, cnt);
        CDB_HIP(hipGetLastError());
        d_flags.download(s, flags_inout);
        if (form == CDB_DEBUG_CARRIED_U64) d_lo.download(s, entries_inout);
        else d_lo.download(s, lo.data());
        if (form == CDB_DEBUG_CARRIED_PACKED40) d_hi.download(s, hi.data());
        CDB_HIP(hipMemcpyAsync(out_partials, part, nb * sizeof(U2), hipMemcpyDeviceToHost, s));
        unsigned long long words[CI_COUNT_SLOTS] = {};
        CDB_HIP(hipMemcpyAsync(words, cnt, sizeof(words), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        carried_inplace_totals(words, out_counts[0], out_counts[1]);
        if (form != CDB_DEBUG_CARRIED_U64)
            for (uint64_t i = 0; i < n; ++i) entries_inout[i] = (uint64_t)lo[i] | (form == CDB_DEBUG_CARRIED_PACKED40 ? (uint64_t)hi[i] << 32 : 0ull);
        bool ok = d_flags.guards_intact(s) && d_lo.guards_intact(s) && d_part.guards_intact(s) && d_cnt.guards_intact(s);
        if (form == CDB_DEBUG_CARRIED_PACKED40) ok = ok && d_hi.guards_intact(s);
        if (out_guard_ok) *out_guard_ok = ok ? 1 : 0;
    });
}

}  // extern "C"
