// sa_initial_direct.hip — the initial sort of builds below 2^32 suffixes (step 3 of sa_build.hip): one radix sort of every
// suffix's key, then the group flags.  The group-flag kernels live here; the bucket-wise build (sa_build.hip) reaches them through
// write_group_flags / write_group_flags32.
#include <cstdlib>

#include "sa_build_phases.h"

namespace cdb {
namespace {

// ---------------------------------------------------------------------------------------------
// group flags: bit0 = first entry of a group of equal prefixes, bit1 = still unresolved
// ---------------------------------------------------------------------------------------------
// k[0] = predecessor, k[1..4] = the four keys of slots i0..i0+3, k[5] = successor -> four flag bytes
__device__ __forceinline__ uint32_t sa_flags_of(const uint64_t (&k)[6], uint64_t i0, uint64_t n, uint32_t kbase,
                                                uint64_t kmagic) {
    uint32_t out = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t i = i0 + q;
        if (i >= n) break;
        const bool head = i == 0 || k[q] != k[q + 1];
        const bool tail = i + 1 == n || k[q + 2] != k[q + 1];
        // an end-of-document code (0) as the last symbol: key = 0 mod base.  kmagic = floor(2^64 / base) + 1
        // makes the quotient one multiply (exact for keys < 2^56); 0 for a power-of-two base
        const uint64_t kq = k[q + 1];
        const bool exhausted = kmagic ? (kq - __umul64hi(kq, kmagic) * kbase) == 0 : (kq & (uint64_t)(kbase - 1u)) == 0;
        out |= (uint32_t)((head ? 1 : 0) | ((!(head && tail) && !exhausted) ? 2 : 0)) << (8 * q);
    }
    return out;
}

__global__ __launch_bounds__(256) void sa_initflags_kernel(const uint64_t* __restrict__ keys, uint64_t n,
                                                           uint32_t kbase, uint64_t kmagic,
                                                           uint8_t* __restrict__ flags, bool flags_aligned) {
    // four consecutive keys per thread (two 16-byte loads), four flag bytes in one store (bytewise when the
    // flag range of a bucket does not start on a 4-byte boundary)
    const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    uint64_t k[6];  // k[0] = predecessor, k[1..4] = own, k[5] = successor
    if (i0 + 4 <= n) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(keys + i0);
        const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(keys + i0 + 2);
        k[1] = a.x; k[2] = a.y; k[3] = b.x; k[4] = b.y;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[1 + q] = i0 + q < n ? keys[i0 + q] : 0;
    }
    k[0] = i0 > 0 ? keys[i0 - 1] : ~k[1];
    k[5] = i0 + 4 < n ? keys[i0 + 4] : 0;
    const uint32_t out = sa_flags_of(k, i0, n, kbase, kmagic);
    if (flags_aligned && i0 + 4 <= n) {
        *reinterpret_cast<uint32_t*>(flags + i0) = out;
    } else {
        for (int q = 0; q < 4 && i0 + q < n; ++q) flags[i0 + q] = (uint8_t)(out >> (8 * q));
    }
}

// the same for 32-bit keys, optionally extended by the separately stored low digit (split sort):
// key = (k32 << low_bits) | low
template <typename W>
__global__ __launch_bounds__(256) void sa_initflags32_kernel(const uint32_t* __restrict__ k32,
                                                             const W* __restrict__ low, int low_bits, uint64_t n,
                                                             uint32_t kbase, uint64_t kmagic, uint8_t* __restrict__ flags,
                                                             bool flags_aligned, U2* __restrict__ tile_sums = nullptr) {
    // tile_sums (optional; `flags` is then the whole array): per scan tile of SC_TILE flags the number of unresolved
    // entries and of unresolved group heads — the sums the first compaction would otherwise re-read every flag for
    __shared__ uint32_t s_sum[2];
    if (tile_sums) {  // (uniform)
        if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
        __syncthreads();
    }
    const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 < n) {
        const uint64_t lmask = (1ull << low_bits) - 1ull;  // (bytes of W above the digits carry other data: packed entries)
        auto full = [&](uint64_t i) -> uint64_t {
            return low ? (((uint64_t)k32[i] << low_bits) | ((uint64_t)low[i] & lmask)) : (uint64_t)k32[i];
        };
        uint64_t k[6];
        if (i0 + 4 <= n) {
            const uint4 a = *reinterpret_cast<const uint4*>(k32 + i0);
            const uint32_t hi[4] = {a.x, a.y, a.z, a.w};
            W l4[4] = {};
            if (low) {
                if constexpr (sizeof(W) == 1) *reinterpret_cast<uint32_t*>(l4) = *reinterpret_cast<const uint32_t*>(low + i0);
                else if constexpr (sizeof(W) == 2) *reinterpret_cast<uint2*>(l4) = *reinterpret_cast<const uint2*>(low + i0);
                else *reinterpret_cast<uint4*>(l4) = *reinterpret_cast<const uint4*>(low + i0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) k[1 + q] = low ? (((uint64_t)hi[q] << low_bits) | ((uint64_t)l4[q] & lmask)) : (uint64_t)hi[q];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) k[1 + q] = i0 + q < n ? full(i0 + q) : 0;
        }
        k[0] = i0 > 0 ? full(i0 - 1) : ~k[1];
        k[5] = i0 + 4 < n ? full(i0 + 4) : 0;
        const uint32_t out = sa_flags_of(k, i0, n, kbase, kmagic);
        if (flags_aligned && i0 + 4 <= n) {
            *reinterpret_cast<uint32_t*>(flags + i0) = out;
        } else {
            for (int q = 0; q < 4 && i0 + q < n; ++q) flags[i0 + q] = (uint8_t)(out >> (8 * q));
        }
        if (tile_sums) {
            const uint32_t unres = (out >> 1) & 0x01010101u;  // (sa_flags_of leaves the bytes behind n zero)
            const uint32_t a = __popc(unres), b = __popc(unres & out);
            if (a) atomicAdd(&s_sum[0], a);
            if (b) atomicAdd(&s_sum[1], b);
        }
    }
    if (tile_sums) {
        __syncthreads();
        if (threadIdx.x == 0 && s_sum[0]) {  // (a workgroup's 1024 flags lie inside one scan tile)
            U2* t = tile_sums + ((uint64_t)blockIdx.x * 1024) / SC_TILE;
            atomicAdd(reinterpret_cast<unsigned long long*>(&t->a), (unsigned long long)s_sum[0]);
            if (s_sum[1]) atomicAdd(reinterpret_cast<unsigned long long*>(&t->b), (unsigned long long)s_sum[1]);
        }
    }
}

}  // namespace

void write_group_flags(hipStream_t s, const uint64_t* keys, uint64_t n, uint32_t kbase, uint64_t kmagic, uint8_t* flags, bool flags_aligned) {
    hipLaunchKernelGGL(sa_initflags_kernel, dim3((unsigned)ceil_div(n, 1024)), dim3(256), 0, s, keys, n, kbase, kmagic, flags, flags_aligned);
}
template <typename W>
void write_group_flags32(hipStream_t s, const uint32_t* k32, const W* low, int low_bits, uint64_t n, uint32_t kbase, uint64_t kmagic,
                         uint8_t* flags, bool flags_aligned, U2* tile_sums) {
    hipLaunchKernelGGL(sa_initflags32_kernel<W>, dim3((unsigned)ceil_div(n, 1024)), dim3(256), 0, s, k32, low, low_bits, n, kbase, kmagic, flags,
                       flags_aligned, tile_sums);
}
template void write_group_flags32<uint8_t>(hipStream_t, const uint32_t*, const uint8_t*, int, uint64_t, uint32_t, uint64_t, uint8_t*, bool, U2*);
template void write_group_flags32<uint16_t>(hipStream_t, const uint32_t*, const uint16_t*, int, uint64_t, uint32_t, uint64_t, uint8_t*, bool, U2*);
template void write_group_flags32<uint32_t>(hipStream_t, const uint32_t*, const uint32_t*, int, uint64_t, uint32_t, uint64_t, uint8_t*, bool, U2*);

// builds below 2^32: one radix sort of every suffix's key, then the group flags
template <typename V>
InitialSort initial_sort_direct(Index& ix, const Alphabet& al, const KeyPlan& kp, const DigitHist& dh, TopCounts& tc, SortStats& ss) {
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size, D = ix.ndocs;
    BuildStats& st = ix.bstats;
    const uint8_t* text = ix.d_text;
    const uint64_t* doc_start = ix.d_doc_start.as<uint64_t>();
    const int nsym = kp.nsym, dbits = kp.dbits, key_bits = kp.key_bits;
    const uint32_t kbase = kp.kbase;
    const uint64_t kmagic = kp.kmagic;
    const bool fused = dh.fused, use_msd = dh.use_msd;
    const uint32_t msd_span = dh.msd_span;
    InitialSort out;
    TextGen gen{text, doc_start, al.d_symmap.as<uint16_t>(), D, (int)ix.bits, kbase, nsym, 0, ix.text_padded};
    double ta = now_ms();
    out.flags.alloc(n);
    // Layout of the sort records.  WIDE: (u64 key, entry).  When the generated first pass can drop the digit it
    // sorts on (it travels as one byte per element) and the rest of the key fits 32 bits, the other passes
    // move 9 instead of 12 bytes per suffix (SPLIT); keys of <= 32 bits need no extra byte at all (NARROW).
    enum { WIDE, NARROW, SPLIT, SPLIT2 } layout = WIDE;
    if (fused && sizeof(V) == 4 && ix.narrow_keys) {
        if (key_bits <= 32) layout = NARROW;
        else if (key_bits - dbits <= 32) layout = SPLIT;
        else if (key_bits - 2 * dbits <= 32) layout = SPLIT2;  // two low digits in a u16: 10 bytes per suffix
    }
    st.key_layout = (int)layout;
    const int low_bits = out.low_bits = layout == SPLIT ? dbits : (layout == SPLIT2 ? 2 * dbits : 0);
    const int low_bytes = out.low_bytes = layout == SPLIT ? 1 : (layout == SPLIT2 ? 2 : 0);
    if (layout != WIDE) {
        if constexpr (sizeof(V) == 4) {
            DevBuf k32[2], vals[2], low[2];
            k32[0].alloc(n * sizeof(uint32_t));
            k32[1].alloc(n * sizeof(uint32_t));
            vals[0].alloc(n * sizeof(V));
            vals[1].alloc(n * sizeof(V));
            if (low_bytes) {
                if (!use_msd) low[0].alloc(n * low_bytes);  // (the MSD-first sort has no travelling byte: only its last pass writes one)
                low[1].alloc(n * low_bytes);
            }
            st.alloc_ms += now_ms() - ta;
            if (getenv("CDB_DEBUG_BUFS"))
                std::fprintf(stderr, "[bufs] k32 %p %p vals %p %p low %p %p flags %p\n", k32[0].p, k32[1].p, vals[0].p, vals[1].p, low[0].p,
                             low[1].p, out.flags.p);
            int sel = 0;
            // The last pass writes the group flags itself (radix_sort.h: SegFinalKeepArgs) where its kernel configuration
            // can (16 Ki tiles, one-atomic ranking): the flag kernel — 5-6 B read per suffix — is then not needed, and the
            // per-tile counts of unresolved entries for the first compaction are counted on the way.
            SegFinalKeepArgs keep;
            DevBuf edges;
            const bool want_keep = ix.flags_in_last_pass && dbits == 8 && rs_variant_maybe_big_atomic(ix.sort_variant, n);  // (16 Ki-tile configurations)
            if (want_keep) {
                const uint64_t nbt = ceil_div(n, (uint64_t)SC_TILE);
                ix.scan_partials.ensure(scan_partials_slots(nbt) * sizeof(U2));
                CDB_HIP(hipMemsetAsync(ix.scan_partials.p, 0, nbt * sizeof(U2), s));
                edges.alloc((ceil_div(n, (uint64_t)RS_SEG_TILE) + 256) * 256 * sizeof(SegEdge));  // (MSD-first: one ragged tile per bucket)
                keep.flags = out.flags.as<uint8_t>();
                keep.edges = edges.as<SegEdge>();
                keep.low_bits = low_bits;
                keep.kbase = kbase;
                keep.kmagic = kmagic;
                keep.tile_sums = ix.scan_partials.as<unsigned long long>();
                keep.sums_tile = SC_TILE;
            }
            if (layout == SPLIT && use_msd && want_keep) {
                // the final pass writes the kept keys in the split layout (u32 = key >> 8, low byte), entries and flags
                if (msd_span) {
                    gen.msd_pair = true;
                    gen.pair_span = dh.pair_consts.pair_span;
                    gen.pair_r = dh.pair_consts.pair_r;
                    gen.pair_s = dh.pair_consts.pair_s;
                } else {
                    gen.msd_shift = 32;
                }
                const bool prebased = tc.counted && msd_span != 0;  // (the counts were made with this span: same rule, same alphabet)
                radix_sort_msd(s, ix.rws, ix.msd_ws, ix.prof, k32[0].as<uint32_t>(), k32[1].as<uint32_t>(), vals[0].as<uint32_t>(),
                               vals[1].as<uint32_t>(), low[1].as<uint8_t>(), n, dh.h_top.data(), gen, dh.msd_m, keep, &ss,
                               prebased ? (const uint32_t*)tc.d_tc.as<uint32_t>() : nullptr, prebased ? &ix.tbw : nullptr, ix.sweep_records);
                st.gen_prebased = prebased ? 1 : 0;
                st.sweep_records = prebased && ix.sweep_records && gen.msd_pair ? 1 : 0;
                tc.d_tc.release();
                ix.tbw.base.release();
                sel = 1;
                out.sorted_low = std::move(low[1]);
                out.flags_by_sort = ix.rws.keep_applied;
            } else if (layout == SPLIT) {
                gen.low_bits = low_bits;
                sel = radix_sort_split<V, uint8_t>(s, ix.rws, ix.prof, k32[0].as<uint32_t>(), k32[1].as<uint32_t>(),
                                                   vals[0].as<V>(), vals[1].as<V>(), low[0].as<uint8_t>(), low[1].as<uint8_t>(), n,
                                                   key_bits - low_bits, &ss, ix.sort_variant, dbits, dh.h_hist.data(), &gen, 0, nullptr, -1,
                                                   want_keep ? &keep : nullptr);
                out.sorted_low = std::move(low[sel]);
                out.flags_by_sort = ix.rws.keep_applied;
            } else if (layout == SPLIT2) {
                gen.low_bits = low_bits;
                sel = radix_sort_split<V, uint16_t>(s, ix.rws, ix.prof, k32[0].as<uint32_t>(), k32[1].as<uint32_t>(),
                                                    vals[0].as<V>(), vals[1].as<V>(), low[0].as<uint16_t>(), low[1].as<uint16_t>(),
                                                    n, key_bits - low_bits, &ss, ix.sort_variant, dbits, dh.h_hist.data(), &gen, 0, nullptr, -1,
                                                    want_keep ? &keep : nullptr);
                out.sorted_low = std::move(low[sel]);
                out.flags_by_sort = ix.rws.keep_applied;
            } else {
                sel = radix_sort<uint32_t, V>(s, ix.rws, ix.prof, k32[0].as<uint32_t>(), k32[1].as<uint32_t>(), vals[0].as<V>(),
                                              vals[1].as<V>(), n, 0, key_bits, &ss, ix.sort_variant, dbits, dh.h_hist.data(), &gen);
            }
            CDB_HIP(hipStreamSynchronize(s));
            out.sorted_k32 = std::move(k32[sel]);
            out.sa_buf = std::move(vals[sel]);
        }
    } else {
        DevBuf keys[2], vals[2];
        keys[0].alloc(n * sizeof(uint64_t));
        keys[1].alloc(n * sizeof(uint64_t));
        vals[0].alloc(n * sizeof(V));
        vals[1].alloc(n * sizeof(V));
        st.alloc_ms += now_ms() - ta;
        int sel;
        if (fused) {
            sel = radix_sort<uint64_t, V>(s, ix.rws, ix.prof, keys[0].as<uint64_t>(), keys[1].as<uint64_t>(), vals[0].as<V>(),
                                          vals[1].as<V>(), n, 0, key_bits, &ss, ix.sort_variant, dbits, dh.h_hist.data(), &gen);
        } else {
            generate_keys<V>(ix, al, kp, keys[0].as<uint64_t>(), vals[0].as<V>());
            sel = radix_sort<uint64_t, V>(s, ix.rws, ix.prof, keys[0].as<uint64_t>(), keys[1].as<uint64_t>(), vals[0].as<V>(),
                                          vals[1].as<V>(), n, 0, key_bits, &ss, ix.sort_variant, dbits);
        }
        CDB_HIP(hipStreamSynchronize(s));
        out.sorted_keys = std::move(keys[sel]);
        out.sa_buf = std::move(vals[sel]);
    }
    out.tile_sums_ready = out.flags_by_sort;
    st.flags_in_last_pass = out.flags_by_sort ? 1 : 0;
    if (!out.flags_by_sort) {
        int t = ix.prof.begin(s);
        if (layout == WIDE)
            hipLaunchKernelGGL(sa_initflags_kernel, dim3((unsigned)ceil_div(n, 1024)), dim3(256), 0, s,
                               (const uint64_t*)out.sorted_keys.as<uint64_t>(), n, kbase, kmagic, out.flags.as<uint8_t>(), true);
        else {
            // (the flag kernel leaves the per-tile counts of unresolved entries for the first compaction: no second sweep
            //  over the flags for them)
            const uint64_t nbt = ceil_div(n, (uint64_t)SC_TILE);
            ix.scan_partials.ensure(scan_partials_slots(nbt) * sizeof(U2));
            CDB_HIP(hipMemsetAsync(ix.scan_partials.p, 0, nbt * sizeof(U2), s));
            out.tile_sums_ready = true;
            if (layout == SPLIT2)
                hipLaunchKernelGGL(sa_initflags32_kernel<uint16_t>, dim3((unsigned)ceil_div(n, 1024)), dim3(256), 0, s,
                                   (const uint32_t*)out.sorted_k32.as<uint32_t>(), (const uint16_t*)out.sorted_low.as<uint16_t>(), low_bits,
                                   n, kbase, kmagic, out.flags.as<uint8_t>(), true, ix.scan_partials.as<U2>());
            else
                hipLaunchKernelGGL(sa_initflags32_kernel<uint8_t>, dim3((unsigned)ceil_div(n, 1024)), dim3(256), 0, s,
                                   (const uint32_t*)out.sorted_k32.as<uint32_t>(),
                                   layout == SPLIT ? (const uint8_t*)out.sorted_low.as<uint8_t>() : (const uint8_t*)nullptr, low_bits,
                                   n, kbase, kmagic, out.flags.as<uint8_t>(), true, ix.scan_partials.as<U2>());
        }
        ix.prof.end(t, "sa_initflags", n * (layout == WIDE ? 9 : 5 + low_bytes), s);
    }
    return out;
}

// the shared sorts of 4-byte entries (sa_build_phases.h): every kernel configuration of these lives in this object — the last pass
// of radix_sort_split<uint32_t, uint8_t> that keeps the keys is also radix_sort_msd's, which only this file calls
template int radix_sort<uint64_t, uint32_t>(CDB_SA_SORT_ARGS(uint64_t, uint32_t));
template int radix_sort<uint32_t, uint32_t>(CDB_SA_SORT_ARGS(uint32_t, uint32_t));
template int radix_sort_split<uint32_t, uint8_t>(CDB_SA_SPLIT_ARGS(uint32_t, uint8_t));
template int radix_sort_split<uint32_t, uint16_t>(CDB_SA_SPLIT_ARGS(uint32_t, uint16_t));

template InitialSort initial_sort_direct<uint32_t>(Index&, const Alphabet&, const KeyPlan&, const DigitHist&, TopCounts&, SortStats&);
template InitialSort initial_sort_direct<uint64_t>(Index&, const Alphabet&, const KeyPlan&, const DigitHist&, TopCounts&, SortStats&);

}  // namespace cdb
