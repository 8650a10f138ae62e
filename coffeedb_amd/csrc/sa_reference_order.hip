// sa_reference_order.hip — the last phase of the suffix-array build (step 5 of sa_build.hip): the finished array goes to the
// index, on text with bytes >= 0x80 first into the reference's signed-bucket order (finish_reference_order), out of place where
// a second array fits (apply_reference_order_oop) and by block rotations where none does (apply_reference_order).
#include <algorithm>
#include <cstring>

#include "sa_build_phases.h"

namespace cdb {
namespace {

// ---------------------------------------------------------------------------------------------
// reference-compatible ordering for text with bytes >= 0x80
// ---------------------------------------------------------------------------------------------
// The reference buckets radix nodes by `(int)char - CHAR_MIN + 1` with a SIGNED char (index.h:72), so
// while a bucket holds more than chuck_size suffixes its children are laid out
//     [end of document][bytes 0x80..0xFF][bytes 0x00..0x7F]
// whereas leaves (<= chuck_size, index.cpp:86-95) and both binary searches compare unsigned.  Given the
// plain unsigned order built above, the reference's order is reached by rotating the two byte blocks
// of every "big" bucket, level by level down the trie.  compat_bounds_kernel finds, for one big bucket
// at depth `depth`, where each of the 257 unsigned symbols starts (the bucket is sorted by that symbol).
template <typename V>
__global__ __launch_bounds__(320) void compat_bounds_kernel(typename SaOf<V>::ptr sa,
                                                            const uint8_t* __restrict__ text,
                                                            const uint64_t* __restrict__ doc_start, int bits,
                                                            uint64_t mask, const CompatBucket* __restrict__ buckets,
                                                            uint64_t depth, unsigned long long* __restrict__ bounds) {
    const int c = threadIdx.x;  // symbol 0 = end of document, 1..256 = byte + 1; 257 = one past
    if (c > 257) return;
    const CompatBucket b = buckets[blockIdx.x];
    uint64_t lo = b.lo, hi = b.hi;
    if (c == 257) {
        bounds[(uint64_t)blockIdx.x * 258 + c] = b.hi;
        return;
    }
    while (lo < hi) {  // first slot whose symbol at `depth` is >= c
        const uint64_t mid = lo + (hi - lo) / 2;
        const auto e = sa[mid];
        const uint64_t d = (uint64_t)e & mask, off = (uint64_t)e >> bits;
        const uint64_t p = doc_start[d] + off + depth;
        const uint32_t sym = p == doc_start[d + 1] ? 0u : (uint32_t)text[p] + 1u;
        if (sym < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    bounds[(uint64_t)blockIdx.x * 258 + c] = lo;
}

// in-place reversal of x[0, len): [A|B] -> [B|A] is reverse(A), reverse(B), reverse(A|B) — the same traffic as
// a round trip through a scratch copy, but without the scratch (up to n entries at the root bucket)
template <typename V>
__global__ __launch_bounds__(256) void compat_reverse_kernel(V* __restrict__ x, uint64_t len) {
    // grid-stride: the root bucket of a 16 GiB shard has more than 2^32 pairs, which one launch cannot address
    // with a thread each (found by tests/test_gpu_fullsize.py: the last of the three reversals silently did not run)
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < len / 2; i += stride) {
        const V a = x[i], b = x[len - 1 - i];
        x[i] = b;
        x[len - 1 - i] = a;
    }
}

// roots (optional): the bucket-wise build already laid its first-symbol buckets out in the reference's root order —
// the walk starts one level down, with those buckets as nodes
// (V = storage tag: uint32_t / uint64_t entries in sa_buf, or Packed40 — low words in sa_buf, high bytes in *sa_hi)
template <typename V>
void apply_reference_order(Index& ix, DevBuf& sa_buf, DevBuf* sa_hi, const std::vector<CompatBucket>* roots = nullptr) {
    constexpr bool PK = std::is_same<V, Packed40>::value;
    using EV = typename std::conditional<PK, uint32_t, typename SaOf<V>::val>::type;  // element type of sa_buf
    EV* sa = sa_buf.as<EV>();
    typename SaOf<V>::ptr sa_r;
    if constexpr (PK) sa_r = Sa40{sa_buf.as<uint32_t>(), sa_hi->as<uint8_t>()};
    else sa_r = sa_buf.as<EV>();
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size;
    const uint64_t chuck = std::max<uint64_t>(4096, n / 256);  // index.cpp:218
    std::vector<CompatBucket> level{{0ull, (unsigned long long)n}};
    if (n <= chuck) return;
    DevBuf d_buckets, d_bounds;
    uint64_t depth = 0;
    if (roots) {
        level.clear();
        for (const CompatBucket& b : *roots)
            if (b.hi - b.lo > chuck) level.push_back(b);
        depth = 1;
    }
    uint64_t moved = 0;  // elements reversed (each one read and written)
    const int tprof = ix.prof.begin(s);
    auto reverse = [&](uint64_t at, uint64_t len) {
        if (len > 1) {
            hipLaunchKernelGGL((compat_reverse_kernel<EV>), dim3((unsigned)std::min<uint64_t>(ceil_div(len / 2, 256), 1u << 20)), dim3(256),
                               0, s, sa + at, len);
            if constexpr (PK)
                hipLaunchKernelGGL((compat_reverse_kernel<uint8_t>), dim3((unsigned)std::min<uint64_t>(ceil_div(len / 2, 256), 1u << 20)),
                                   dim3(256), 0, s, sa_hi->as<uint8_t>() + at, len);
            moved += len;
        }
    };
    while (!level.empty()) {
        const size_t nb = level.size();
        d_buckets.ensure(nb * sizeof(CompatBucket));
        d_bounds.ensure(nb * 258 * sizeof(uint64_t));
        CDB_HIP(hipMemcpyAsync(d_buckets.p, level.data(), nb * sizeof(CompatBucket), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL((compat_bounds_kernel<V>), dim3((unsigned)nb), dim3(320), 0, s, sa_r, ix.d_text,
                           (const uint64_t*)ix.d_doc_start.as<uint64_t>(), (int)ix.bits, ix.mask,
                           (const CompatBucket*)d_buckets.as<CompatBucket>(), depth,
                           d_bounds.as<unsigned long long>());
        std::vector<unsigned long long> hb(nb * 258);
        CDB_HIP(hipMemcpyAsync(hb.data(), d_bounds.p, hb.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        std::vector<CompatBucket> next;
        for (size_t b = 0; b < nb; ++b) {
            const unsigned long long* bd = &hb[b * 258];
            const uint64_t a0 = bd[1], b0 = bd[129], end = bd[257];  // [a0,b0) = 0x00..0x7F, [b0,end) = 0x80..0xFF
            const uint64_t lenA = b0 - a0, lenB = end - b0;
            if (lenA && lenB) {
                reverse(a0, lenA);
                reverse(b0, lenB);
                reverse(a0, lenA + lenB);
                ix.bstats.compat_rotations++;
            }
            for (int v = 0; v < 256; ++v) {
                const uint64_t len = bd[v + 2] - bd[v + 1];
                if (len <= chuck) continue;
                const uint64_t start = v >= 128 ? a0 + (bd[v + 1] - b0) : a0 + lenB + (bd[v + 1] - a0);
                next.push_back(CompatBucket{(unsigned long long)start, (unsigned long long)(start + len)});
            }
        }
        level.swap(next);
        ++depth;
    }
    ix.bstats.compat_depth = depth;
    ix.prof.end(tprof, "sa_compat_rotate", 2 * moved * (PK ? 5 : sizeof(EV)), s);
    CDB_HIP(hipStreamSynchronize(s));
}

// The same order reached in ONE out-of-place pass (when a second array fits): the rotations only move whole
// child buckets, so every bucket of the rotated array is still a contiguous range of the plainly sorted one.
// The bucket tree is therefore walked on the UNROTATED array — each bucket carries (its range there, where it
// ends up) — and the leaves become copy segments.  1 read + 1 write per entry instead of 2 + 2 for every
// level of three reversals; the kept search keys can make the same trip.
struct CompatSeg {
    unsigned long long src, dst;
    uint32_t count, pad;
};
constexpr uint32_t CS_ITEM = 16384;
template <typename T>
__global__ __launch_bounds__(256) void compat_segcopy_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                             const CompatSeg* __restrict__ segs) {
    const CompatSeg sg = segs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < sg.count; i += 256) out[sg.dst + i] = in[sg.src + i];
}

struct CompatNode {
    unsigned long long lo, hi, fin;  // range in the sorted array, first slot in the reference order
};

// returns false (nothing done) when the scratch array cannot be had; sa_buf is replaced by the reordered array
template <typename V>
bool apply_reference_order_oop(Index& ix, DevBuf& sa_buf, DevBuf* sa_hi, const std::vector<CompatBucket>* roots = nullptr) {
    constexpr bool PK = std::is_same<V, Packed40>::value;
    using EV = typename std::conditional<PK, uint32_t, typename SaOf<V>::val>::type;  // element type of sa_buf
    constexpr size_t ESZ = PK ? 5 : sizeof(EV);
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size;
    const uint64_t chuck = std::max<uint64_t>(4096, n / 256);  // index.cpp:218
    if (n <= chuck) return true;
    {   // only when the second array fits comfortably: a failed allocation would flush the block cache for nothing
        size_t fre = 0, tot = 0;
        CDB_HIP(hipMemGetInfo(&fre, &tot));
        if ((double)n * ESZ > 0.8 * ((double)fre + (double)DevPool::get().cached_bytes())) return false;
        // ... and only when the pool can hand it out as it stands (a cached block of that size, or untouched VRAM): a hipMalloc
        // that fails first makes the pool return its whole cache to the driver — 2.5-5 s per 16 GiB build when it happened
        if (!DevPool::get().can_serve(n * sizeof(EV), ix.device)) return false;
    }
    DevBuf dst, dst_hi;
    try {
        dst.alloc(n * sizeof(EV));
        if (PK) dst_hi.alloc(n);
    } catch (const Error&) {
        return false;
    }
    typename SaOf<V>::ptr sa;
    if constexpr (PK) sa = Sa40{sa_buf.as<uint32_t>(), sa_hi->as<uint8_t>()};
    else sa = sa_buf.as<EV>();
    std::vector<CompatNode> level{{0ull, (unsigned long long)n, 0ull}};
    std::vector<CompatSeg> segs;
    auto emit = [&](uint64_t src, uint64_t dstpos, uint64_t len) {
        if (!len) return;
        for (uint64_t o = 0; o < len; o += CS_ITEM)
            segs.push_back(CompatSeg{(unsigned long long)(src + o), (unsigned long long)(dstpos + o),
                                     (uint32_t)std::min<uint64_t>(CS_ITEM, len - o), 0u});
    };
    DevBuf d_buckets, d_bounds, d_segs;
    uint64_t depth = 0;
    if (roots) {  // first-symbol buckets already in the reference's root order: they stay where they are
        level.clear();
        for (const CompatBucket& b : *roots) {
            if (b.hi - b.lo > chuck) level.push_back(CompatNode{b.lo, b.hi, b.lo});
            else emit(b.lo, b.lo, b.hi - b.lo);
        }
        depth = 1;
    }
    const uint64_t rotations_before = ix.bstats.compat_rotations;
    std::vector<CompatBucket> cb;
    while (!level.empty()) {
        const size_t nb = level.size();
        cb.resize(nb);
        for (size_t b = 0; b < nb; ++b) cb[b] = CompatBucket{level[b].lo, level[b].hi};
        d_buckets.ensure(nb * sizeof(CompatBucket));
        d_bounds.ensure(nb * 258 * sizeof(uint64_t));
        CDB_HIP(hipMemcpyAsync(d_buckets.p, cb.data(), nb * sizeof(CompatBucket), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL((compat_bounds_kernel<V>), dim3((unsigned)nb), dim3(320), 0, s, sa, ix.d_text,
                           (const uint64_t*)ix.d_doc_start.as<uint64_t>(), (int)ix.bits, ix.mask,
                           (const CompatBucket*)d_buckets.as<CompatBucket>(), depth, d_bounds.as<unsigned long long>());
        std::vector<unsigned long long> hb(nb * 258);
        CDB_HIP(hipMemcpyAsync(hb.data(), d_bounds.p, hb.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        std::vector<CompatNode> next;
        for (size_t b = 0; b < nb; ++b) {
            const unsigned long long* bd = &hb[b * 258];
            const CompatNode nd = level[b];
            const uint64_t a0 = bd[1], b0 = bd[129], end = bd[257];  // [a0,b0) = 0x00..0x7F, [b0,end) = 0x80..0xFF
            const uint64_t lenEnd = a0 - nd.lo, lenA = b0 - a0, lenB = end - b0;
            if (lenA && lenB) ix.bstats.compat_rotations++;
            emit(nd.lo, nd.fin, lenEnd);  // suffixes that end here stay in front
            // children in reference order: 0x80..0xFF first, then 0x00..0x7F; runs of small children are copied
            // as one segment
            uint64_t run_src = 0, run_dst = 0, run_len = 0;
            auto flush = [&] {
                emit(run_src, run_dst, run_len);
                run_len = 0;
            };
            for (int k = 0; k < 256; ++k) {
                const int v = k < 128 ? 128 + k : k - 128;
                const uint64_t lo = bd[v + 1], len = bd[v + 2] - lo;
                if (!len) continue;
                const uint64_t fin = v >= 128 ? nd.fin + lenEnd + (lo - b0) : nd.fin + lenEnd + lenB + (lo - a0);
                if (len > chuck) {
                    flush();
                    next.push_back(CompatNode{(unsigned long long)lo, (unsigned long long)(lo + len), (unsigned long long)fin});
                } else if (run_len && run_src + run_len == lo && run_dst + run_len == fin) {
                    run_len += len;
                } else {
                    flush();
                    run_src = lo;
                    run_dst = fin;
                    run_len = len;
                }
            }
            flush();
        }
        level.swap(next);
        ++depth;
    }
    ix.bstats.compat_depth = depth;
    if (ix.bstats.compat_rotations == rotations_before) return true;  // every node had its children on one side: nothing moves
    if (!segs.empty()) {
        d_segs.alloc(segs.size() * sizeof(CompatSeg));
        CDB_HIP(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(CompatSeg), hipMemcpyHostToDevice, s));
        int t = ix.prof.begin(s);
        hipLaunchKernelGGL((compat_segcopy_kernel<EV>), dim3((unsigned)segs.size()), dim3(256), 0, s, (const EV*)sa_buf.as<EV>(), dst.as<EV>(),
                           (const CompatSeg*)d_segs.as<CompatSeg>());
        if constexpr (PK)
            hipLaunchKernelGGL((compat_segcopy_kernel<uint8_t>), dim3((unsigned)segs.size()), dim3(256), 0, s, (const uint8_t*)sa_hi->as<uint8_t>(),
                               dst_hi.as<uint8_t>(), (const CompatSeg*)d_segs.as<CompatSeg>());
        ix.prof.end(t, "sa_compat_copy", 2 * n * ESZ, s);
    }
    // the kept search keys make the same trip, so that probes on the reordered array can still be decided from
    // one load (query.hip follows the reference's probe sequence there, with the same comparisons)
    if (!segs.empty() && ix.key_nsym) {
        auto permute = [&](DevBuf& buf, size_t esz) {
            if (!buf.p) return;
            DevBuf nb;
            nb.alloc(n * esz);
            const dim3 grid((unsigned)segs.size());
            const CompatSeg* sg = d_segs.as<CompatSeg>();
            if (esz == 8) hipLaunchKernelGGL((compat_segcopy_kernel<uint64_t>), grid, dim3(256), 0, s, (const uint64_t*)buf.as<uint64_t>(), nb.as<uint64_t>(), sg);
            else if (esz == 4) hipLaunchKernelGGL((compat_segcopy_kernel<uint32_t>), grid, dim3(256), 0, s, (const uint32_t*)buf.as<uint32_t>(), nb.as<uint32_t>(), sg);
            else if (esz == 2) hipLaunchKernelGGL((compat_segcopy_kernel<uint16_t>), grid, dim3(256), 0, s, (const uint16_t*)buf.as<uint16_t>(), nb.as<uint16_t>(), sg);
            else hipLaunchKernelGGL((compat_segcopy_kernel<uint8_t>), grid, dim3(256), 0, s, (const uint8_t*)buf.as<uint8_t>(), nb.as<uint8_t>(), sg);
            CDB_HIP(hipStreamSynchronize(s));
            buf = std::move(nb);
        };
        permute(ix.d_keys, 8);
        permute(ix.d_keys32, 4);
        permute(ix.d_keylow, (size_t)std::max(ix.key_low_bytes, 1));
    }
    CDB_HIP(hipStreamSynchronize(s));
    sa_buf = std::move(dst);
    if constexpr (PK) *sa_hi = std::move(dst_hi);
    return true;
}

}  // namespace

// the array goes to the index — on text with bytes >= 0x80 first into the reference's order
template <typename V>
void finish_reference_order(Index& ix, InitialSort& is, Alphabet& al) {
    ix.sa_sorted = !(ix.reference_compat && al.high_bytes);
    ix.pivot_levels = 0;  // the pivot table belongs to the previous suffix array
    if (ix.key_nsym) {  // the code table the kept keys were built with
        ix.d_symmap_q = std::move(al.d_symmap);
        std::memcpy(ix.h_symmap_q, al.h_map, sizeof(al.h_map));
    }
    if (ix.reference_compat && al.high_bytes) {
        std::vector<CompatBucket>& folded_roots = is.folded_roots;
        const std::vector<Depth1Fold>& depth1 = is.depth1;
        // buckets whose two byte blocks were swapped by the sort enter the walk as their two blocks (each sorted by the
        // second symbol and with all children on one side of 0x80: no rotation there, their big children are walked)
        if (!folded_roots.empty() && !depth1.empty()) {
            std::vector<CompatBucket> nodes;
            for (size_t b = 0; b < folded_roots.size(); ++b) {
                const CompatBucket r = folded_roots[b];
                if (depth1[b].done) {
                    const unsigned long long hs = r.lo + depth1[b].nend, ls = hs + depth1[b].nhigh;
                    // (every slot must belong to some entry of the list: the out-of-place form of the walk COPIES the
                    //  array range by range — the fuzz-sized test caught the block of one-symbol suffixes missing here)
                    if (depth1[b].nend) nodes.push_back(CompatBucket{r.lo, hs});
                    nodes.push_back(CompatBucket{hs, ls});
                    nodes.push_back(CompatBucket{ls, r.hi});
                } else {
                    nodes.push_back(r);
                }
            }
            folded_roots.swap(nodes);
        }
        const std::vector<CompatBucket>* roots = folded_roots.empty() ? nullptr : &folded_roots;
        auto reorder = [&](auto tag) {
            using T = decltype(tag);
            if (!apply_reference_order_oop<T>(ix, is.sa_buf, &is.sa_hi_buf, roots)) {
                apply_reference_order<T>(ix, is.sa_buf, &is.sa_hi_buf, roots);  // in place when no second array fits
                ix.drop_keys();                                                 // ... which moves the entries away from their keys
            }
        };
        if (is.packed_out) reorder(Packed40{});
        else reorder(V{});
    }
    ix.d_sa = std::move(is.sa_buf);
    ix.d_sa_hi = std::move(is.sa_hi_buf);
    ix.sa_packed = is.packed_out;
}

template void finish_reference_order<uint32_t>(Index&, InitialSort&, Alphabet&);
template void finish_reference_order<uint64_t>(Index&, InitialSort&, Alphabet&);

}  // namespace cdb
