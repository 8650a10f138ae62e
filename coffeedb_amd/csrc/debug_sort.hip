// debug_sort.hip — test hooks for the radix-sort primitive (radix_sort.h), in a translation unit of their own so that the sort's
// kernel configurations they instantiate compile beside the library's other sources instead of inside capi.hip.  Nothing here is
// called by a production path; the hooks call radix_sort() / radix_sort_split() exactly as the production call sites do.
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "index_impl.h"
#include "radix_sort.h"

using namespace cdb;

// A long-lived workspace and the stream it sorts on: what ix.rws / ws.rws are to a handle of the library.
struct cdb_debug_sort_ws {
    int device = 0;
    hipStream_t s = nullptr;
    RadixWorkspace ws;
    Profiler prof;
    std::mutex mu;
};

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

// the stream + workspace of one hook call: the handle's, or a fresh pair that lives for the call
struct CallScope {
    cdb_debug_sort_ws* h;
    cdb_debug_sort_ws local;
    std::unique_lock<std::mutex> lock;
    CallScope(int device, cdb_debug_sort_ws* handle) : h(handle ? handle : &local) {
        if (handle) {
            lock = std::unique_lock<std::mutex>(handle->mu);
            CDB_HIP(hipSetDevice(handle->device));
        } else {
            if (device >= 0) CDB_HIP(hipSetDevice(device));
            CDB_HIP(hipGetDevice(&local.device));
            CDB_HIP(hipStreamCreateWithFlags(&local.s, hipStreamNonBlocking));
        }
    }
    ~CallScope() {
        if (h == &local && local.s) {
            (void)hipStreamSynchronize(local.s);
            {
                StreamScope sscope(local.s);
                local.ws.release();
            }
            DevPool::get().retire_stream(local.s);
            (void)hipStreamDestroy(local.s);
        }
    }
};

struct SortFlags {
    bool device_hist, spare, poison, grouped;
    explicit SortFlags(unsigned f)
        : device_hist(f & CDB_DEBUG_SORT_DEVICE_HIST), spare(f & CDB_DEBUG_SORT_SPARE_VALUES), poison(f & CDB_DEBUG_SORT_POISON),
          grouped(f & CDB_DEBUG_SORT_GROUPED) {}
};

// One attempt (sort + the host's look at the error flag), then — under the grouped flag, as build_suffix_array does after a
// starved pass in XCD-aware tile order — the input restored and one more attempt in plain ticket order.  The device's
// process-wide state (rs_group_order_disable) is left alone, as by the build's debug_starve_group hook.
template <typename Sort, typename Restore>
void sort_with_fallback(hipStream_t s, RadixWorkspace& ws, const SortFlags& fl, void* spare, cdb_debug_sort_result* out, Sort&& sort,
                        Restore&& restore) {
    auto attempt = [&](bool plain, bool poison) {
        ws.allow_group = fl.grouped;
        ws.plain_order = plain;
        ws.debug_poison = poison;
        ws.value_spare = spare;
        SortStats st;
        const int sel = sort(st);
        const int vres = ws.value_result;
        radix_check_error(s, ws);
        out->passes_run = st.passes_run;
        out->passes_skipped = st.passes_skipped;
        out->key_result = sel;
        out->value_result = vres;
    };
    struct Reset {  // (a handle's next call starts from its own flags)
        RadixWorkspace& ws;
        ~Reset() { ws.allow_group = ws.plain_order = ws.debug_poison = false; ws.value_spare = nullptr; }
    } reset{ws};
    try {
        attempt(false, fl.poison);
    } catch (const LookbackTimeout&) {
        if (!fl.grouped) throw;
        restore();
        out->fell_back = 1;
        attempt(true, false);
    }
}

template <typename K, typename V>
void sort_pairs(cdb_debug_sort_ws& h, void* d_keys, void* d_vals, uint64_t n, int begin_bit, int end_bit, int dbits, int variant,
                const SortFlags& fl, cdb_debug_sort_result* out) {
    constexpr bool HAS_V = !std::is_same<V, NoVal>::value;
    constexpr size_t VB = HAS_V ? sizeof(V) : 0;
    hipStream_t s = h.s;
    K* k0 = static_cast<K*>(d_keys);
    V* v0 = HAS_V ? static_cast<V*>(d_vals) : nullptr;
    DevBuf k1, v1, spare, kcopy, vcopy, dhist;
    k1.alloc(n * sizeof(K));
    if (HAS_V) v1.alloc(n * VB);
    if (HAS_V && fl.spare) spare.alloc(n * VB);
    if (fl.grouped) {
        kcopy.alloc(n * sizeof(K));
        CDB_HIP(hipMemcpyAsync(kcopy.p, d_keys, n * sizeof(K), hipMemcpyDeviceToDevice, s));
        if (HAS_V) {
            vcopy.alloc(n * VB);
            CDB_HIP(hipMemcpyAsync(vcopy.p, d_vals, n * VB, hipMemcpyDeviceToDevice, s));
        }
    }
    // device-side histograms, counted as the sort itself counts them (the bucket-wise build derives them from its record kernel).
    // A request for more passes than the sort has is left to the sort to refuse: the histogram kernel has no rows for them.
    const int npass = (int)ceil_div(end_bit - begin_bit, dbits);
    const unsigned long long* d_hist_in = nullptr;
    if (fl.device_hist && npass <= RS_MAX_PASSES) {
        const uint32_t last_mask = (1u << (end_bit - begin_bit - dbits * (npass - 1))) - 1u;
        dhist.alloc((size_t)RS_MAX_PASSES * 256 * sizeof(uint64_t));
        CDB_HIP(hipMemsetAsync(dhist.p, 0, (size_t)RS_MAX_PASSES * 256 * sizeof(uint64_t), s));
        const int grid = (int)std::min<uint64_t>(ceil_div(n, 256 * 16), 256 * 8);
        hipLaunchKernelGGL(rs_hist_kernel<K>, dim3(grid), dim3(256), 0, s, (const K*)k0, n, begin_bit, npass, dbits, last_mask,
                           dhist.as<unsigned long long>());
        d_hist_in = dhist.as<unsigned long long>();
    }
    sort_with_fallback(
        s, h.ws, fl, HAS_V && fl.spare ? spare.p : nullptr, out,
        [&](SortStats& st) {
            return radix_sort<K, V>(s, h.ws, h.prof, k0, k1.as<K>(), v0, HAS_V ? v1.as<V>() : nullptr, n, begin_bit, end_bit, &st,
                                    variant, dbits, (const uint64_t*)nullptr, (const TextGen*)nullptr, d_hist_in);
        },
        [&] {
            CDB_HIP(hipMemcpyAsync(d_keys, kcopy.p, n * sizeof(K), hipMemcpyDeviceToDevice, s));
            if (HAS_V) CDB_HIP(hipMemcpyAsync(d_vals, vcopy.p, n * VB, hipMemcpyDeviceToDevice, s));
        });
    if (out->key_result == 1) CDB_HIP(hipMemcpyAsync(d_keys, k1.p, n * sizeof(K), hipMemcpyDeviceToDevice, s));
    if (HAS_V && out->value_result == 1) CDB_HIP(hipMemcpyAsync(d_vals, v1.p, n * VB, hipMemcpyDeviceToDevice, s));
    CDB_HIP(hipStreamSynchronize(s));
}

// digit histograms of split records, [lead + key passes][256], lowest digit first: the auxiliary word's lead digits, then the
// digits of the key's low hi_bits bits (the last one masked to the bits that are left)
template <typename W>
__global__ __launch_bounds__(256) void dbg_split_hist_kernel(const uint32_t* __restrict__ keys, const W* __restrict__ aux, uint64_t n,
                                                             int lead, int kpass, uint32_t last_mask,
                                                             unsigned long long* __restrict__ hist) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t k = keys[i], a = (uint32_t)aux[i];
        for (int p = 0; p < lead; ++p) atomicAdd(&hist[p * 256 + ((a >> (8 * p)) & 255u)], 1ull);
        for (int p = 0; p < kpass; ++p) {
            uint32_t d = (k >> (8 * p)) & 255u;
            if (p == kpass - 1) d &= last_mask;
            atomicAdd(&hist[(lead + p) * 256 + d], 1ull);
        }
    }
}

template <typename V, typename W>
void sort_split(cdb_debug_sort_ws& h, void* d_keys, void* d_vals, void* d_aux, uint64_t n, int hi_bits, int lead, int variant,
                const SortFlags& fl, cdb_debug_sort_result* out) {
    hipStream_t s = h.s;
    uint32_t* k0 = static_cast<uint32_t*>(d_keys);
    V* v0 = static_cast<V*>(d_vals);
    W* w0 = static_cast<W*>(d_aux);
    DevBuf k1, v1, w1, spare, kcopy, vcopy, wcopy, dhist;
    k1.alloc(n * 4);
    v1.alloc(n * sizeof(V));
    w1.alloc(n * sizeof(W));
    if (fl.spare) spare.alloc(n * sizeof(V));
    if (fl.grouped) {
        kcopy.alloc(n * 4);
        vcopy.alloc(n * sizeof(V));
        wcopy.alloc(n * sizeof(W));
        CDB_HIP(hipMemcpyAsync(kcopy.p, d_keys, n * 4, hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipMemcpyAsync(vcopy.p, d_vals, n * sizeof(V), hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipMemcpyAsync(wcopy.p, d_aux, n * sizeof(W), hipMemcpyDeviceToDevice, s));
    }
    const int kpass = (int)ceil_div(hi_bits, 8), npass = lead + kpass;
    const uint32_t last_mask = (1u << (hi_bits - 8 * (kpass - 1))) - 1u;
    std::vector<uint64_t> h_hist;
    if (fl.device_hist) {
        dhist.alloc((size_t)npass * 256 * sizeof(uint64_t));
        CDB_HIP(hipMemsetAsync(dhist.p, 0, (size_t)npass * 256 * sizeof(uint64_t), s));
        const int grid = (int)std::min<uint64_t>(ceil_div(n, 256 * 16), 256 * 8);
        hipLaunchKernelGGL(dbg_split_hist_kernel<W>, dim3(grid), dim3(256), 0, s, (const uint32_t*)k0, (const W*)w0, n, lead, kpass,
                           last_mask, dhist.as<unsigned long long>());
    } else {
        std::vector<uint32_t> hk(n);
        std::vector<W> hw(n);
        CDB_HIP(hipMemcpyAsync(hk.data(), d_keys, n * 4, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(hw.data(), d_aux, n * sizeof(W), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        h_hist.assign((size_t)npass * 256, 0);
        for (uint64_t i = 0; i < n; ++i) {
            for (int p = 0; p < lead; ++p) h_hist[(size_t)p * 256 + (((uint32_t)hw[i] >> (8 * p)) & 255u)]++;
            for (int p = 0; p < kpass; ++p) {
                uint32_t d = (hk[i] >> (8 * p)) & 255u;
                if (p == kpass - 1) d &= last_mask;
                h_hist[(size_t)(lead + p) * 256 + d]++;
            }
        }
    }
    sort_with_fallback(
        s, h.ws, fl, fl.spare ? spare.p : nullptr, out,
        [&](SortStats& st) {
            return radix_sort_split<V, W>(s, h.ws, h.prof, k0, k1.as<uint32_t>(), v0, v1.as<V>(), w0, w1.as<W>(), n, hi_bits, &st,
                                          variant, 8, fl.device_hist ? nullptr : h_hist.data(), (const TextGen*)nullptr, 0,
                                          fl.device_hist ? dhist.as<unsigned long long>() : nullptr, lead);
        },
        [&] {
            CDB_HIP(hipMemcpyAsync(d_keys, kcopy.p, n * 4, hipMemcpyDeviceToDevice, s));
            CDB_HIP(hipMemcpyAsync(d_vals, vcopy.p, n * sizeof(V), hipMemcpyDeviceToDevice, s));
            CDB_HIP(hipMemcpyAsync(d_aux, wcopy.p, n * sizeof(W), hipMemcpyDeviceToDevice, s));
        });
    if (out->key_result == 1) {
        CDB_HIP(hipMemcpyAsync(d_keys, k1.p, n * 4, hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipMemcpyAsync(d_aux, w1.p, n * sizeof(W), hipMemcpyDeviceToDevice, s));
    }
    if (out->value_result == 1) CDB_HIP(hipMemcpyAsync(d_vals, v1.p, n * sizeof(V), hipMemcpyDeviceToDevice, s));
    CDB_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int cdb_debug_sort_ws_create(int device, cdb_debug_sort_ws** out) {
    if (!out) return CDB_E_INVALID;
    *out = nullptr;
    return guarded_hook("cdb_debug_sort_ws_create", [&] {
        if (device >= 0) CDB_HIP(hipSetDevice(device));
        std::unique_ptr<cdb_debug_sort_ws> h(new cdb_debug_sort_ws);
        CDB_HIP(hipGetDevice(&h->device));
        CDB_HIP(hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking));
        *out = h.release();
    });
}

void cdb_debug_sort_ws_destroy(cdb_debug_sort_ws* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) {
        (void)hipStreamSynchronize(h->s);
        {
            StreamScope sscope(h->s);
            h->ws.release();
        }
        DevPool::get().retire_stream(h->s);
        (void)hipStreamDestroy(h->s);
    }
    delete h;
}

// radix_sort<K, V> as its production callers use it.  Stands in for: the columns' sorts of order-flipped 64-bit keys with 8- and
// 4-byte values and key-only (columns.hip: column build, range queries); the query paths' hit-list and ranked / OR sorts of
// (u64, u64) pairs and key-only batches (query.hip); cluster's key-only u32 and u64 sorts and its (u64, u32) pairs (cluster.hip);
// the suffix-array build's narrow-key sort radix_sort<uint32_t, V> and its 64-bit pair sorts with begin_bit / end_bit inside the
// key and digits of 2..8 bits (sa_initial_direct.hip: the initial sort; sa_build.hip: the per-symbol bucket sort that passes top_shift as end_bit with
// live bits above it); and the bucket-wise build's per-bucket sorts with device-side histograms and the third value buffer
// (sa_build.hip: run_group, radix_sort<K, V> with hb and ix.rws.value_spare).  Under CDB_DEBUG_SORT_GROUPED it follows
// build_suffix_array: allow_group, and after a LookbackTimeout the input restored and the sort redone with plain_order.
int cdb_debug_radix_sort_ex(int device, cdb_debug_sort_ws* ws, void* d_keys, void* d_vals, uint64_t n, int key_bytes, int val_bytes,
                            int begin_bit, int end_bit, int dbits, int variant, unsigned flags, cdb_debug_sort_result* out) {
    cdb_debug_sort_result local = {};
    if (!out) out = &local;
    *out = cdb_debug_sort_result{};
    if (!d_keys || (key_bytes != 4 && key_bytes != 8) || (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) || (val_bytes && !d_vals) ||
        begin_bit < 0 || end_bit <= begin_bit || end_bit > 8 * key_bytes || dbits < 1 || dbits > 8)
        return CDB_E_INVALID;
    // 4 and 41 (kept for A/B measurements) exist for 64-bit keys only, as in production
    if (!(rs_variant_production(variant) || (key_bytes == 8 && (variant == RS_VARIANT_FIRST || variant == RS_VARIANT_DMA)))) return CDB_E_INVALID;
    // radix_sort() passes d_hist_in on to its pair configurations only: for a key-only sort the flag would silently do nothing
    if ((flags & CDB_DEBUG_SORT_DEVICE_HIST) && val_bytes == 0) return CDB_E_INVALID;
    if (n == 0) return CDB_OK;
    return guarded_hook("cdb_debug_radix_sort_ex", [&] {
        CallScope cs(device, ws);
        cdb_debug_sort_ws& h = *cs.h;
        StreamScope sscope(h.s);
        const SortFlags fl(flags);
        const double ms0 = [&] {
            double ms = 0;
            for (auto& kv : h.prof.recs)
                if (kv.first.rfind("rs_onesweep", 0) == 0) ms += kv.second.ms;
            return ms;
        }();
        h.prof.enabled = (flags & CDB_DEBUG_SORT_PROFILE) != 0;
        struct Epoch {  // (reported for a failed sort too)
            cdb_debug_sort_ws& h;
            cdb_debug_sort_result* out;
            ~Epoch() { out->epoch = h.ws.epoch; }
        } epoch{h, out};
        if (key_bytes == 8) {
            if (val_bytes == 4) sort_pairs<uint64_t, uint32_t>(h, d_keys, d_vals, n, begin_bit, end_bit, dbits, variant, fl, out);
            else if (val_bytes == 8) sort_pairs<uint64_t, uint64_t>(h, d_keys, d_vals, n, begin_bit, end_bit, dbits, variant, fl, out);
            else sort_pairs<uint64_t, NoVal>(h, d_keys, d_vals, n, begin_bit, end_bit, dbits, variant, fl, out);
        } else {
            if (val_bytes == 4) sort_pairs<uint32_t, uint32_t>(h, d_keys, d_vals, n, begin_bit, end_bit, dbits, variant, fl, out);
            else if (val_bytes == 8) sort_pairs<uint32_t, uint64_t>(h, d_keys, d_vals, n, begin_bit, end_bit, dbits, variant, fl, out);
            else sort_pairs<uint32_t, NoVal>(h, d_keys, d_vals, n, begin_bit, end_bit, dbits, variant, fl, out);
        }
        if (h.prof.enabled) {
            h.prof.resolve();
            double ms = 0;
            for (auto& kv : h.prof.recs)
                if (kv.first.rfind("rs_onesweep", 0) == 0) ms += kv.second.ms;  // every tile size
            out->onesweep_ms = ms - ms0;
        }
    });
}

// radix_sort_split<V, W> over materialised records (gen == nullptr).  Stands in for the bucket-wise build's per-bucket sorts
// (sa_build.hip): run_group — radix_sort_split<V, W> with W = u8 / u16, every byte of W a sort digit, device histograms, the
// third value buffer — and run_group_packed — radix_sort_split<uint32_t, W> with W = u8 / u16 / u32 whose upper bytes carry
// entry bits 32..39 (lead_digits < sizeof(W)).  Only the (V, W) pairs those two instantiate exist here: no new LDS footprint.
int cdb_debug_radix_sort_split(int device, cdb_debug_sort_ws* ws, void* d_keys, void* d_vals, void* d_aux, uint64_t n, int val_bytes,
                               int aux_bytes, int hi_bits, int lead_digits, int variant, unsigned flags, cdb_debug_sort_result* out) {
    cdb_debug_sort_result local = {};
    if (!out) out = &local;
    *out = cdb_debug_sort_result{};
    // the (value, auxiliary) pairs the bucket-wise build instantiates
    const bool pair_ok = (val_bytes == 4 && (aux_bytes == 1 || aux_bytes == 2 || aux_bytes == 4)) ||
                         (val_bytes == 8 && (aux_bytes == 1 || aux_bytes == 2));
    if (!d_keys || !d_vals || !d_aux || !pair_ok || hi_bits < 1 || hi_bits > 32 || lead_digits < 0 || lead_digits > aux_bytes ||
        !rs_variant_production(variant))
        return CDB_E_INVALID;
    if (n == 0) return CDB_OK;
    return guarded_hook("cdb_debug_radix_sort_split", [&] {
        CallScope cs(device, ws);
        cdb_debug_sort_ws& h = *cs.h;
        StreamScope sscope(h.s);
        const SortFlags fl(flags);
        h.prof.enabled = false;
        struct Epoch {
            cdb_debug_sort_ws& h;
            cdb_debug_sort_result* out;
            ~Epoch() { out->epoch = h.ws.epoch; }
        } epoch{h, out};
        if (val_bytes == 4) {
            if (aux_bytes == 1) sort_split<uint32_t, uint8_t>(h, d_keys, d_vals, d_aux, n, hi_bits, lead_digits, variant, fl, out);
            else if (aux_bytes == 2) sort_split<uint32_t, uint16_t>(h, d_keys, d_vals, d_aux, n, hi_bits, lead_digits, variant, fl, out);
            else sort_split<uint32_t, uint32_t>(h, d_keys, d_vals, d_aux, n, hi_bits, lead_digits, variant, fl, out);
        } else {
            if (aux_bytes == 1) sort_split<uint64_t, uint8_t>(h, d_keys, d_vals, d_aux, n, hi_bits, lead_digits, variant, fl, out);
            else sort_split<uint64_t, uint16_t>(h, d_keys, d_vals, d_aux, n, hi_bits, lead_digits, variant, fl, out);
        }
    });
}

// The first hook (tests/test_gpu_sort.py, tools/sort_bench.py): 64-bit keys, bits [0, key_bits), a fresh workspace, timed.
int cdb_debug_radix_sort(int device, void* d_keys, void* d_vals, uint64_t n, int val_bytes, int key_bits, int variant,
                         double* onesweep_ms, int* passes) {
    if (key_bits < 1 || key_bits > 64) return CDB_E_INVALID;
    cdb_debug_sort_result r = {};
    if (variant != RS_VARIANT_FIRST && variant != RS_VARIANT_DMA && !rs_variant_production(variant)) variant = RS_VARIANT_BIG_BALLOT;  // (rs_dispatch_variant's default)
    const int rc = cdb_debug_radix_sort_ex(device, nullptr, d_keys, val_bytes ? d_vals : nullptr, n, 8, val_bytes, 0, key_bits, 8, variant,
                                           CDB_DEBUG_SORT_PROFILE, &r);
    if (onesweep_ms) *onesweep_ms = r.onesweep_ms;
    if (passes) *passes = r.passes_run;
    return rc;
}

}  // extern "C"
