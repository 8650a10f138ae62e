// append.hip — documents join a built index on the device (cdb_append, include/coffeedb_gpu.h; capi.hip holds the entry point,
// the upload and the commit).  Suffixes never cross documents, so the old suffixes keep their mutual order and the new ones get
// theirs from a build over the new documents alone; equal suffixes ascend by document and every new document is numbered behind
// every old one, so a new suffix that equals an old one goes behind it.  The array over "old documents, then new documents" is
// therefore the stable two-way merge of the old array and the new documents' array, ties old first — a merge instead of a sort.
//
//   1. tables    old ids / doc_start copied on the device, the new ones (re-based by the old size) uploaded behind them; the old
//                column's longest document by a reduce; the set of byte values the new text holds
//   2. new array the m new suffixes sorted by the existing build (a throw-away inner Index on this stream), decoded into entries
//                of the NEW layout
//   3. rank      pos_j = #{old suffixes <= new suffix j}: a sparse sample searches the whole old array, the rest between their
//                bracketing samples; a probe is decided by the kept search key where the handle has one and resumes its byte
//                comparison at the prefix both bounds already share (Manber-Myers)
//   4. merge     output slot pos_j + j belongs to new suffix j: one flag per output slot, the flagged slots ranked stably tile by
//                tile (stable_tiles.h: count, scan, ballot ranks), and both kinds of entry re-encoded
// Everything is written into fresh blocks of an AppendPlan while the old index stands.  64-bit indices throughout.
#include <memory>
#include <type_traits>

#include "index_impl.h"
#include "scan.h"
#include "stable_tiles.h"

namespace cdb {
namespace {

constexpr uint64_t AP_SAMPLE = 64;  // every AP_SAMPLE-th new suffix (and the last) searches the whole old array

// ---- 1. tables and text -----------------------------------------------------------------------------------------------------
// out[b >> 5] bit (b & 31) = byte value b occurs in text[0 .. m)
__global__ __launch_bounds__(256) void ap_bytes_kernel(const uint8_t* __restrict__ text, uint64_t m, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_set[8];
    if (threadIdx.x < 8) s_set[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
        const uint32_t b = text[i], w = b >> 5, bit = 1u << (b & 31u);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) mine[k] |= w == k ? bit : 0u;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (mine[k]) atomicOr(&s_set[k], mine[k]);
    __syncthreads();
    if (threadIdx.x < 8 && s_set[threadIdx.x]) atomicOr(out + threadIdx.x, s_set[threadIdx.x]);
}

// dst[d] = src[d] - base (the new documents' starts on the origin of the new text, for the inner build)
__global__ __launch_bounds__(256) void ap_rebase_kernel(const uint64_t* __restrict__ src, uint64_t cnt, uint64_t base, uint64_t* __restrict__ dst) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d < cnt) dst[d] = src[d] - base;
}

// ---- 2. the new documents' array in the new layout --------------------------------------------------------------------------
template <typename Tag>
__global__ __launch_bounds__(256) void ap_decode_kernel(typename SaOf<Tag>::ptr sa, uint64_t m, int in_bits, uint64_t in_mask, int new_bits,
                                                        uint64_t doc_base, uint64_t* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint64_t e = (uint64_t)sa[j];
    out[j] = ((e >> in_bits) << new_bits) | ((e & in_mask) + doc_base);
}

// ---- search keys ------------------------------------------------------------------------------------------------------------
// the key the build keeps for a suffix (sa_build.hip: sa_keygen_kernel): its first nsym symbol codes as a number in base kbase,
// code 0 behind the end of the document.  Reads rem bytes at most.
__device__ __forceinline__ uint64_t suffix_key(const uint8_t* __restrict__ p, uint64_t rem, const uint16_t* map, int nsym, uint32_t kbase) {
    uint64_t key = 0;
    for (int k = 0; k < nsym; ++k) key = key * kbase + ((uint64_t)k < rem ? (uint64_t)map[p[k]] : 0ull);
    return key;
}
// KeptKeys::at with the form known at compile time (ap_rank_kernel: 1 = u64 keys, 2 = u32 keys, 3 / 4 = u32 keys + one / two low bytes)
template <int KF>
__device__ __forceinline__ uint64_t key_at(const KeptKeys& k, uint64_t i) {
    if constexpr (KF == 1) return k.k64[i];
    else if constexpr (KF == 2) return k.k32[i];
    else if constexpr (KF == 3) return ((uint64_t)k.k32[i] << k.low_bits) | (uint64_t)k.low[i];
    else return ((uint64_t)k.k32[i] << k.low_bits) | (uint64_t)reinterpret_cast<const uint16_t*>(k.low)[i];
}
// ---- 3. rank ----------------------------------------------------------------------------------------------------------------
// s <= t ?  (cmp_common's rule: unsigned bytes, shorter first, equal counts as "<=").  The first k bytes of both are known to be
// equal; lcp = the length of their common prefix.  Neither suffix is read past its end.
__device__ __forceinline__ bool suffix_le(const uint8_t* __restrict__ s, uint64_t sl, const uint8_t* __restrict__ t, uint64_t tl, uint64_t k,
                                          uint64_t& lcp) {
    const uint64_t len = sl < tl ? sl : tl;
    uint64_t i = k < len ? k : len;
    for (; i + 8 <= len; i += 8) {
        const uint64_t a = load_be8(s + i), b = load_be8(t + i);
        if (a != b) {
            lcp = i + (uint64_t)(__clzll((long long)(a ^ b)) >> 3);
            return a < b;
        }
    }
    for (; i < len; ++i) {
        const uint8_t a = s[i], b = t[i];
        if (a != b) {
            lcp = i;
            return a < b;
        }
    }
    lcp = len;
    return sl <= tl;
}

// phase 0: the samples (j = 0, AP_SAMPLE, 2 AP_SAMPLE, ... and m - 1) search [0, n]; phase 1: every other j searches
// [pos of the sample in front of it, pos of the sample behind it] — pos is non-decreasing in j.  pos[j] = first slot whose old
// suffix is greater than new suffix j.  Invariant of the bisection: every slot in front of lo holds a suffix <= t and shares at
// least ll bytes with it, every slot from hi on a suffix > t sharing at least rl bytes; a slot between them shares at least
// min(ll, rl) bytes with t, which is where its comparison resumes.  A probe the keys decide leaves ll / rl as they are: the
// bound moves towards t, so what it shared before it still shares.
// KF = the form of the kept keys (0: none, the text decides every probe).  One new suffix per thread, no loop around the
// bisection: wave-uniform switches are template parameters or used in front of it only.
template <typename Tag, int KF>
__global__ __launch_bounds__(256) void ap_rank_kernel(typename SaOf<Tag>::ptr sa, uint64_t n, const uint8_t* __restrict__ otext,
                                                      const uint64_t* __restrict__ ostart, int obits, uint64_t omask,
                                                      const uint64_t* __restrict__ nent, uint64_t m, const uint8_t* __restrict__ ctext,
                                                      const uint64_t* __restrict__ cstart, int nbits, uint64_t nmask, KeptKeys keys,
                                                      const uint16_t* __restrict__ symmap, int nsym, uint32_t kbase, int phase,
                                                      uint64_t* __restrict__ pos, uint64_t* __restrict__ newkey) {
    __shared__ uint16_t s_map[256];
    if constexpr (KF != 0) s_map[threadIdx.x] = symmap[threadIdx.x];
    __syncthreads();
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t j = q, lo = 0, hi = n;
    bool active;
    if (phase == 0) {
        const uint64_t nsamples = (m - 1) / AP_SAMPLE + 1 + ((m - 1) % AP_SAMPLE ? 1 : 0);
        active = q < nsamples;
        j = q * AP_SAMPLE < m ? q * AP_SAMPLE : m - 1;
    } else {
        active = j < m && j % AP_SAMPLE != 0 && j != m - 1;
        if (active) {
            const uint64_t a = j - j % AP_SAMPLE, b = a + AP_SAMPLE < m ? a + AP_SAMPLE : m - 1;
            lo = pos[a];
            hi = pos[b];
        }
    }
    if (!active) return;
    const uint64_t e = nent[j];
    const uint64_t td = e & nmask, tb = cstart[td] + (e >> nbits), tl = cstart[td + 1] - tb;
    const uint8_t* t = ctext + tb;
    uint64_t tkey = 0;
    if constexpr (KF != 0) {
        tkey = suffix_key(t, tl, s_map, nsym, kbase);
        newkey[j] = tkey;
    }
    uint64_t ll = 0, rl = 0;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        bool le = false, decided = false;
        if constexpr (KF != 0) {
            const uint64_t sk = key_at<KF>(keys, mid);
            le = sk < tkey;
            decided = sk != tkey;
        }
        if (!decided) {
            const uint64_t se = (uint64_t)sa[mid];
            const uint64_t sd = se & omask, sb = ostart[sd] + (se >> obits), sl = ostart[sd + 1] - sb;
            uint64_t lcp = 0;
            le = suffix_le(otext + sb, sl, t, tl, ll < rl ? ll : rl, lcp);
            if (le) ll = lcp;
            else rl = lcp;
        }
        if (le) lo = mid + 1;
        else hi = mid;
    }
    pos[j] = lo;
}

// ---- 4. merge ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ap_flag_kernel(const uint64_t* __restrict__ pos, uint64_t m, uint8_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) flag[pos[j] + j] = 1;
}
// the flag of the ranking (stable_tiles.h): output slot o takes a new entry
struct SlotIsNew {
    const uint8_t* flag;
    __device__ __forceinline__ bool operator()(uint64_t o) const { return flag[o] != 0; }
};
// output slot o is new entry number r or old entry number o - r, where r = new entries in front of o
template <typename SrcTag, typename Dst>
__global__ __launch_bounds__(256) void ap_merge_kernel(typename SaOf<SrcTag>::ptr sa, uint64_t N, int old_bits, uint64_t old_mask, int new_bits,
                                                       const uint8_t* __restrict__ flag, const uint64_t* __restrict__ nent,
                                                       const uint64_t* __restrict__ newkey, const uint64_t* __restrict__ tile_base, Dst out,
                                                       KeptKeys kin, KeptKeys kout, bool with_keys) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t o = tile_slot(k);
        const bool valid = o < N;
        const bool isnew = valid && flag[o] != 0;
        const uint64_t r = ranker.before(k, isnew);
        if (valid) {
            if (isnew) {
                out.store(o, (typename Dst::val)nent[r]);
                if (with_keys) kout.put(o, newkey[r]);
            } else {
                const uint64_t i = o - r;
                const uint64_t e = (uint64_t)sa[i];
                out.store(o, (typename Dst::val)(((e >> old_bits) << new_bits) | (e & old_mask)));
                if (with_keys) kout.put(o, kin.at(i));
            }
        }
    }
}

// ---- cdb_debug_verify_keys ----------------------------------------------------------------------------------------------------
template <typename Tag>
__global__ __launch_bounds__(256) void ap_verify_keys_kernel(typename SaOf<Tag>::ptr sa, uint64_t n, const uint8_t* __restrict__ text,
                                                             const uint64_t* __restrict__ doc_start, int bits, uint64_t mask, KeptKeys keys,
                                                             const uint16_t* __restrict__ symmap, int nsym, uint32_t kbase,
                                                             unsigned long long* __restrict__ out) {
    __shared__ uint16_t s_map[256];
    s_map[threadIdx.x] = symmap[threadIdx.x];
    __syncthreads();
    uint64_t bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t e = (uint64_t)sa[i];
        const uint64_t d = e & mask, b = doc_start[d] + (e >> bits), sl = doc_start[d + 1] - b;
        bad += suffix_key(text + b, sl, s_map, nsym, kbase) != keys.at(i) ? 1 : 0;
    }
    for (int off = 32; off; off >>= 1) bad += __shfl_xor(bad, off);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, (unsigned long long)bad);
}

}  // namespace

void append_old_longest(Index& ix, AppendPlan& p) {
    hipStream_t s = ix.stream;
    DevBuf d_out;
    d_out.alloc(8);
    CDB_HIP(hipMemsetAsync(d_out.p, 0, 8, s));
    int t = ix.prof.begin(s);
    longest_document(s, nullptr, ix.d_doc_start.as<uint64_t>(), ix.ndocs, d_out.as<unsigned long long>());
    ix.prof.end(t, "ap_longest", ix.ndocs * 8, s);
    CDB_HIP(hipGetLastError());
    uint64_t out = 0;
    CDB_HIP(hipMemcpyAsync(&out, d_out.p, 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    p.old_longest = out;
}

void append_tables(Index& ix, AppendPlan& p, const int64_t* ids, const uint64_t* new_start) {
    hipStream_t s = ix.stream;
    const uint64_t D = ix.ndocs;
    p.d_start.alloc((D + p.ndocs + 1) * 8);
    p.d_ids.alloc((D + p.ndocs) * 8);
    CDB_HIP(hipMemcpyAsync(p.d_start.p, ix.d_doc_start.p, D * 8, hipMemcpyDeviceToDevice, s));
    CDB_HIP(hipMemcpyAsync(p.d_start.as<uint64_t>() + D, new_start, (p.ndocs + 1) * 8, hipMemcpyHostToDevice, s));
    CDB_HIP(hipMemcpyAsync(p.d_ids.p, ix.d_ids.p, D * 8, hipMemcpyDeviceToDevice, s));
    CDB_HIP(hipMemcpyAsync(p.d_ids.as<int64_t>() + D, ids, p.ndocs * 8, hipMemcpyHostToDevice, s));
}

void append_text_old(Index& ix, AppendPlan& p) {
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size;
    p.text.alloc(n + p.size + TEXT_PAD);
    CDB_HIP(hipMemsetAsync(p.text.as<uint8_t>() + n + p.size, 0, TEXT_PAD, s));
    if (n) CDB_HIP(hipMemcpyAsync(p.text.p, ix.d_text, n, hipMemcpyDeviceToDevice, s));
}

void append_scan_bytes(Index& ix, AppendPlan& p) {
    hipStream_t s = ix.stream;
    uint32_t set[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.size) {
        DevBuf d_set;
        d_set.alloc(32);
        CDB_HIP(hipMemsetAsync(d_set.p, 0, 32, s));
        int t = ix.prof.begin(s);
        hipLaunchKernelGGL(ap_bytes_kernel, dim3(grid_for(ceil_div(p.size, 16))), dim3(256), 0, s, (const uint8_t*)p.text.as<uint8_t>() + ix.size, p.size,
                           d_set.as<uint32_t>());
        ix.prof.end(t, "ap_bytes", p.size, s);
        CDB_HIP(hipGetLastError());
        CDB_HIP(hipMemcpyAsync(set, d_set.p, 32, hipMemcpyDeviceToHost, s));
    }
    CDB_HIP(hipStreamSynchronize(s));
    p.high_bytes = (set[4] | set[5] | set[6] | set[7]) != 0;
    p.unmapped_bytes = false;
    for (int b = 0; b < 256; ++b)
        if (((set[b >> 5] >> (b & 31)) & 1u) && ix.h_symmap_q[b] == 0) p.unmapped_bytes = true;
}

void append_merge(Index& ix, AppendPlan& p, int new_bits, uint64_t new_mask, int new_width, bool new_packed) {
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size, m = p.size, N = n + m, D = ix.ndocs;
    p.arr.alloc(N, new_width, new_packed);
    if (!N) return;
    // ---- the new documents' own array, decoded into entries of the new layout
    DevBuf nent, pos, newkey;
    nent.alloc(std::max<uint64_t>(m, 2) * 8);
    const bool with_keys = keys_recomputable(ix) && !p.unmapped_bytes;
    if (m) {
        auto inner = std::make_unique<Index>();
        Index& in = *inner;
        in.device = ix.device;
        in.stream = s;
        in.aux_stream = ix.aux_stream;  // (lent: the build's second stream and its events belong to the handle)
        in.aux_ev[0] = ix.aux_ev[0];
        in.aux_ev[1] = ix.aux_ev[1];
        struct GiveBack {
            Index& ix;
            Index& in;
            ~GiveBack() {
                ix.aux_stream = in.aux_stream;
                ix.aux_ev[0] = in.aux_ev[0];
                ix.aux_ev[1] = in.aux_ev[1];
            }
        } give_back{ix, in};
        in.reference_compat = ix.reference_compat;
        in.self_check = std::min(ix.self_check, 1);
        in.premap_generation = false;
        in.keep_keys = false;
        in.pack_sa = ix.pack_sa;
        in.force_big_path = ix.force_big_path;
        in.debug_fail_build = ix.debug_fail_build;
        in.rws.plain_order = ix.rws.plain_order;
        in.host_tables_valid = false;
        in.host_text_valid = false;
        in.size = m;
        in.ndocs = p.ndocs;
        in.bits = p.in_bits;
        in.mask = p.in_mask;
        in.width = p.in_width;
        in.off_bits = p.in_off_bits;
        in.d_text_owned.alloc(m + TEXT_PAD);  // (a block of its own: the build wants its text 16-byte aligned)
        CDB_HIP(hipMemcpyAsync(in.d_text_owned.p, p.text.as<uint8_t>() + n, m, hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipMemsetAsync(in.d_text_owned.as<uint8_t>() + m, 0, TEXT_PAD, s));
        in.d_text = in.d_text_owned.as<uint8_t>();
        in.text_padded = true;
        in.d_doc_start.alloc((p.ndocs + 1) * 8);
        in.d_ids.alloc(16);
        hipLaunchKernelGGL(ap_rebase_kernel, dim3((unsigned)ceil_div(p.ndocs + 1, 256)), dim3(256), 0, s,
                           (const uint64_t*)p.d_start.as<uint64_t>() + D, p.ndocs + 1, n, in.d_doc_start.as<uint64_t>());
        CDB_HIP(hipGetLastError());
        build_suffix_array(in);  // (synchronises; a failure here is a failure before the commit)
        if (!in.sa_sorted) throw InternalError("append: the new documents' array is not sorted (internal)");
        const unsigned blocks = (unsigned)ceil_div(m, 256);
        int t = ix.prof.begin(s);
        sa_dispatch(in, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL((ap_decode_kernel<T>), dim3(blocks), dim3(256), 0, s, in.sa_view<T>(), m, (int)in.bits, in.mask, new_bits, D,
                               nent.as<uint64_t>());
        });
        ix.prof.end(t, "ap_decode", m * (8 + (in.sa_packed ? 5 : (uint64_t)in.width)), s);
        CDB_HIP(hipGetLastError());
        CDB_HIP(hipStreamSynchronize(s));  // (the inner index goes: its blocks return to the cache idle)
    }
    // ---- rank
    pos.alloc(std::max<uint64_t>(m, 2) * 8);
    if (with_keys) newkey.alloc(std::max<uint64_t>(m, 2) * 8);
    const KeptKeys kin = with_keys ? keys_of(ix) : KeptKeys{};
    const int nsym = with_keys ? ix.key_nsym : 0;
    const uint16_t* symmap = with_keys ? (const uint16_t*)ix.d_symmap_q.as<uint16_t>() : (const uint16_t*)nullptr;
    if (m) {
        const uint64_t nsamples = (m - 1) / AP_SAMPLE + 2;
        if (ceil_div(m, 256) >= (1ull << 31)) throw InternalError("append: too many new suffixes for one launch (internal)");
        const int kf = !with_keys ? 0 : kin.k64 ? 1 : !kin.low_bits ? 2 : kin.low_bytes == 2 ? 4 : 3;
        for (int phase = 0; phase < 2; ++phase) {
            const unsigned blocks = (unsigned)ceil_div(phase == 0 ? nsamples : m, 256);
            int t = ix.prof.begin(s);
            sa_dispatch(ix, [&](auto tag) {
                using T = decltype(tag);
                auto launch = [&](auto kform) {
                    constexpr int KF = decltype(kform)::value;
                    hipLaunchKernelGGL((ap_rank_kernel<T, KF>), dim3(blocks), dim3(256), 0, s, ix.sa_view<T>(), n, ix.d_text,
                                       (const uint64_t*)ix.d_doc_start.as<uint64_t>(), (int)ix.bits, ix.mask, (const uint64_t*)nent.as<uint64_t>(), m,
                                       (const uint8_t*)p.text.as<uint8_t>(), (const uint64_t*)p.d_start.as<uint64_t>(), new_bits, new_mask, kin,
                                       symmap, nsym, ix.key_base, phase, pos.as<uint64_t>(), newkey.as<uint64_t>());
                };
                if (kf == 0) launch(std::integral_constant<int, 0>{});
                else if (kf == 1) launch(std::integral_constant<int, 1>{});
                else if (kf == 2) launch(std::integral_constant<int, 2>{});
                else if (kf == 3) launch(std::integral_constant<int, 3>{});
                else launch(std::integral_constant<int, 4>{});
            });
            ix.prof.end(t, phase == 0 ? "ap_rank_samples" : "ap_rank", (phase == 0 ? nsamples : m) * (uint64_t)bit_width64(n + 1) * 64, s);
            CDB_HIP(hipGetLastError());
        }
    }
    // ---- merge
    DevBuf flag, tile_base;
    flag.alloc(N);
    CDB_HIP(hipMemsetAsync(flag.p, 0, N, s));
    if (m) {
        int t = ix.prof.begin(s);
        hipLaunchKernelGGL(ap_flag_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s, (const uint64_t*)pos.as<uint64_t>(), m, flag.as<uint8_t>());
        ix.prof.end(t, "ap_flag", m * 9, s);
        CDB_HIP(hipGetLastError());
    }
    const uint64_t ntiles = ceil_div(N, ST_TILE);
    if (tile_bases(ix, "append", SlotIsNew{flag.as<uint8_t>()}, N, tile_base, "ap_count", N + ntiles * 8) != m)
        throw InternalError("append: new entries and new bytes differ (internal)");
    const KeptKeys kout = with_keys ? p.arr.alloc_keys_like(ix, N) : KeptKeys{};
    const int old_bytes = ix.sa_packed ? 5 : ix.width;
    const int t = ix.prof.begin(s);
    sa_dispatch(ix, [&](auto src_tag) {
        using S = decltype(src_tag);
        auto launch = [&](auto dst) {
            using Dd = decltype(dst);
            hipLaunchKernelGGL((ap_merge_kernel<S, Dd>), dim3((unsigned)ntiles), dim3(256), 0, s, ix.sa_view<S>(), N, (int)ix.bits, ix.mask, new_bits,
                               (const uint8_t*)flag.as<uint8_t>(), (const uint64_t*)nent.as<uint64_t>(), (const uint64_t*)newkey.as<uint64_t>(),
                               (const uint64_t*)tile_base.as<uint64_t>(), dst, kin, kout, with_keys);
        };
        if (new_packed) launch(Sa40RW{p.arr.sa.as<uint32_t>(), p.arr.sa_hi.as<uint8_t>()});
        else if (new_width == 8) launch(SaRW<uint64_t>{p.arr.sa.as<uint64_t>()});
        else launch(SaRW<uint32_t>{p.arr.sa.as<uint32_t>()});
    });
    ix.prof.end(t, "ap_merge", n * (uint64_t)old_bytes + m * 8 + N * (1 + (new_packed ? 5 : (uint64_t)new_width) + 2 * kout.bytes_per_slot()) + ntiles * 8, s);
    CDB_HIP(hipGetLastError());
    CDB_HIP(hipStreamSynchronize(s));  // (the scratch blocks above go back to the cache idle)
}

void verify_kept_keys(Index& ix, uint64_t out[2]) {
    out[0] = out[1] = 0;
    if (!ix.size || !keys_recomputable(ix)) return;
    hipStream_t s = ix.stream;
    DevBuf d_out;
    d_out.alloc(8);
    CDB_HIP(hipMemsetAsync(d_out.p, 0, 8, s));
    const KeptKeys kin = keys_of(ix);
    sa_dispatch(ix, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((ap_verify_keys_kernel<T>), dim3(grid_for(ix.size)), dim3(256), 0, s, ix.sa_view<T>(), ix.size, ix.d_text,
                           (const uint64_t*)ix.d_doc_start.as<uint64_t>(), (int)ix.bits, ix.mask, kin, (const uint16_t*)ix.d_symmap_q.as<uint16_t>(),
                           ix.key_nsym, ix.key_base, d_out.as<unsigned long long>());
    });
    CDB_HIP(hipGetLastError());
    CDB_HIP(hipMemcpyAsync(out, d_out.p, 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    out[1] = ix.size;
}

}  // namespace cdb
