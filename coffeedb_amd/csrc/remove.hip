// remove.hip — documents leave a built index on the device (cdb_remove, include/coffeedb_gpu.h; capi.hip holds the entry
// point and the commit).  Suffixes never cross documents, equal suffixes ascend by document and the survivors keep their
// relative order, so the suffix array of the surviving documents is the old array with the removed documents' entries
// dropped and the rest re-encoded: a stable stream compaction instead of a sort.
//
//   1. mark      ids -> documents through the id table (cluster.hip: id_table_prepare), one drop flag per document
//   2. tables    a scan over the flags numbers the survivors and sums their lengths: new ids, new doc_start, the old
//                start of every survivor, the old -> new document table (the flag stays separate: no value of it is spent)
//   3. text      gather of the kept documents, cut by OUTPUT bytes (a 3 GiB document spreads over all workgroups)
//   4. array     the kept entries are ranked stably tile by tile (stable_tiles.h: count, scan, ballot ranks) and written with the
//                kept search keys in the new storage form
// Everything is written into fresh blocks of a RemovePlan while the old index stands.  64-bit indices throughout.
#include "index_impl.h"
#include "scan.h"
#include "stable_tiles.h"

namespace cdb {
namespace {

constexpr uint64_t RM_TEXT_RANGE = 64u << 10;  // output bytes per workgroup step of the gather

// ---- 1. mark ----------------------------------------------------------------------------------------------------------------
// out[0] += entries of ids the index does not hold; a held id given twice sets the same flag twice
__global__ __launch_bounds__(256) void rm_mark_kernel(const int64_t* __restrict__ ids, uint64_t nids, const int64_t* __restrict__ id_tab,
                                                      const uint32_t* __restrict__ id_doc, uint64_t ndocs, uint8_t* __restrict__ drop,
                                                      unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t miss = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nids; i += stride) {
        const int64_t id = ids[i];
        const uint64_t r = lower_bound_id(id_tab, ndocs, id);
        const bool hit = r < ndocs && id_tab[r] == id;
        if (hit) drop[id_doc ? (uint64_t)id_doc[r] : r] = 1;
        miss += hit ? 0 : 1;
    }
    for (int off = 32; off; off >>= 1) miss += __shfl_xor(miss, off);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(out, (unsigned long long)miss);
}

// ---- 2. document tables -----------------------------------------------------------------------------------------------------
struct KeptIn {  // (survivor?, its length)
    const uint8_t* drop;
    const uint64_t* doc_start;
    __device__ __forceinline__ U2 operator()(uint64_t d) const {
        return drop[d] ? U2{0, 0} : U2{1, doc_start[d + 1] - doc_start[d]};
    }
};
struct TablesOut {
    const uint8_t* drop;
    const uint64_t* doc_start;
    const int64_t* ids;
    uint64_t ndocs;
    uint32_t* newdoc;     // [ndocs]: meaningful where drop is 0
    int64_t* new_ids;     // [kept]
    uint64_t* new_start;  // [kept + 1]
    uint64_t* src_start;  // [kept]: where the survivor's bytes lie in the old text
    __device__ __forceinline__ void operator()(uint64_t d, const U2& ex, const U2& in) const {
        if (!drop[d]) {
            newdoc[d] = (uint32_t)ex.a;
            new_ids[ex.a] = ids[d];
            new_start[ex.a] = ex.b;
            src_start[ex.a] = doc_start[d];
        }
        if (d + 1 == ndocs) new_start[in.a] = in.b;
    }
};
// the longest document that is not dropped (drop = nullptr: of all; as layout_kernel finds the longest of a resident column)
__global__ __launch_bounds__(256) void longest_document_kernel(const uint8_t* __restrict__ drop, const uint64_t* __restrict__ doc_start,
                                                               uint64_t ndocs, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_max[4];
    uint64_t mx = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < ndocs; d += stride) {
        const uint64_t len = drop && drop[d] ? 0 : doc_start[d + 1] - doc_start[d];
        mx = len > mx ? len : mx;
    }
    for (int off = 32; off; off >>= 1) {
        const uint64_t o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
        if (mx) atomicMax(out, (unsigned long long)mx);
    }
}

// ---- 3. text ----------------------------------------------------------------------------------------------------------------
// last j in [a, b] with start[j] <= pos (start[a] <= pos is given)
__device__ __forceinline__ uint64_t last_start_le(const uint64_t* __restrict__ start, uint64_t a, uint64_t b, uint64_t pos) {
    while (a < b) {
        const uint64_t m = (a + b + 1) >> 1;
        if (start[m] <= pos) a = m;
        else b = m - 1;
    }
    return a;
}
// Every workgroup takes fixed ranges of RM_TEXT_RANGE OUTPUT bytes; two searches in the new doc_start bound the documents of a
// range, every thread then finds the document of its 16 output bytes between them.  A piece that lies inside one document moves
// as one 16-byte store, fed by one aligned 16-byte load or by two and a shift (the source is rarely aligned); pieces that
// cross documents, the last bytes of the text and sources without 32 readable bytes move byte by byte.
__global__ __launch_bounds__(256) void rm_text_kernel(const uint8_t* __restrict__ src, uint64_t src_bytes, const uint64_t* __restrict__ new_start,
                                                      const uint64_t* __restrict__ src_start, uint64_t kept, uint64_t n_new,
                                                      uint8_t* __restrict__ dst) {
    __shared__ uint64_t s_doc[2];
    const bool src_aligned = ((uintptr_t)src & 15u) == 0;
    const uint64_t nranges = (n_new + RM_TEXT_RANGE - 1) / RM_TEXT_RANGE;
    for (uint64_t r = blockIdx.x; r < nranges; r += gridDim.x) {
        const uint64_t r0 = r * RM_TEXT_RANGE, r1 = r0 + RM_TEXT_RANGE < n_new ? r0 + RM_TEXT_RANGE : n_new;
        __syncthreads();  // (s_doc of the previous range is consumed)
        if (threadIdx.x < 2) s_doc[threadIdx.x] = last_start_le(new_start, 0, kept - 1, threadIdx.x ? r1 - 1 : r0);
        __syncthreads();
        const uint64_t j_first = s_doc[0], j_last = s_doc[1];
        for (uint64_t o = r0 + (uint64_t)threadIdx.x * 16; o < r1; o += 256 * 16) {
            uint64_t j = last_start_le(new_start, j_first, j_last, o);
            uint64_t ds = new_start[j], de = new_start[j + 1];
            const uint64_t from = src_start[j] + (o - ds);
            if (src_aligned && o + 16 <= de && o + 16 <= r1 && (from & ~15ull) + 32 <= src_bytes) {
                const uint64_t a = from & ~15ull;
                const unsigned sh = (unsigned)(from & 15u) * 8;
                const uint4 lo4 = *reinterpret_cast<const uint4*>(src + a);
                unsigned __int128 v = ((unsigned __int128)(((uint64_t)lo4.w << 32) | lo4.z) << 64) | (((uint64_t)lo4.y << 32) | lo4.x);
                if (sh) {
                    const uint4 hi4 = *reinterpret_cast<const uint4*>(src + a + 16);
                    const unsigned __int128 w = ((unsigned __int128)(((uint64_t)hi4.w << 32) | hi4.z) << 64) | (((uint64_t)hi4.y << 32) | hi4.x);
                    v = (v >> sh) | (w << (128 - sh));
                }
                const uint64_t v0 = (uint64_t)v, v1 = (uint64_t)(v >> 64);
                *reinterpret_cast<uint4*>(dst + o) = make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32));
            } else {
                const uint64_t end = o + 16 < r1 ? o + 16 : r1;
                for (uint64_t p = o; p < end; ++p) {
                    while (p >= de) {  // (empty documents are stepped over; p < n_new = new_start[kept] ends the walk)
                        ++j;
                        ds = de;
                        de = new_start[j + 1];
                    }
                    dst[p] = src[src_start[j] + (p - ds)];
                }
            }
        }
    }
}

// ---- 4. suffix array --------------------------------------------------------------------------------------------------------
// the flag of the ranking (stable_tiles.h): entry i is kept.  The document field lies below bit 32 in every layout: `lo` + i * stride
// is the entry's low word (stride 1: u32 entries and the packed form's low words; 2: u64 entries)
struct EntryKept {
    const uint32_t* lo;
    int stride;
    uint32_t mask;
    const uint8_t* drop;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return drop[lo[i * (uint64_t)stride] & mask] == 0; }
};

// kept entry number r of the input is entry r of the output, re-encoded; its stored search keys go with it as they are
template <typename SrcTag, typename Dst>
__global__ __launch_bounds__(256) void rm_compact_kernel(typename SaOf<SrcTag>::ptr sa, uint64_t n, int old_bits, uint64_t old_mask, int new_bits,
                                                         const uint8_t* __restrict__ drop, const uint32_t* __restrict__ newdoc,
                                                         const uint64_t* __restrict__ tile_base, Dst out, KeptKeys keys_in, KeptKeys keys_out) {
    TileRanker ranker(tile_base);
    for (int k = 0; k < ST_ROUNDS; ++k) {
        const uint64_t i = tile_slot(k);
        uint64_t e = 0, d = 0;
        bool keep = false;
        if (i < n) {
            e = (uint64_t)sa[i];
            d = e & old_mask;
            keep = drop[d] == 0;
        }
        const uint64_t at = ranker.before(k, keep);
        if (keep) {
            out.store(at, (typename Dst::val)(((e >> old_bits) << new_bits) | (uint64_t)newdoc[d]));
            keys_out.copy(keys_in, i, at);
        }
    }
}

}  // namespace

void longest_document(hipStream_t s, const uint8_t* drop, const uint64_t* doc_start, uint64_t ndocs, unsigned long long* out) {
    hipLaunchKernelGGL(longest_document_kernel, dim3(grid_for(ndocs)), dim3(256), 0, s, drop, doc_start, ndocs, out);
}

void remove_mark(Index& ix, RowIds ids, uint64_t nids, RemovePlan& p) {
    hipStream_t s = ix.stream;
    const uint64_t ndocs = ix.ndocs;
    id_table_prepare(ix);
    const int64_t* id_tab = ix.idt.ids_ascend ? ix.d_ids.as<int64_t>() : ix.idt.id_sorted.as<int64_t>();
    const uint32_t* id_doc = ix.idt.ids_ascend ? nullptr : ix.idt.id_doc.as<uint32_t>();
    const uint64_t* doc_start = ix.d_doc_start.as<uint64_t>();
    DevBuf d_ids, d_out;
    const int64_t* idp = resident_ids(s, d_ids, ids, nids);
    d_out.alloc(16);
    p.drop.alloc(ndocs);
    CDB_HIP(hipMemsetAsync(d_out.p, 0, 16, s));
    CDB_HIP(hipMemsetAsync(p.drop.p, 0, ndocs, s));
    int t = ix.prof.begin(s);
    hipLaunchKernelGGL(rm_mark_kernel, dim3(grid_for(nids)), dim3(256), 0, s, idp, nids, id_tab, id_doc, ndocs,
                       p.drop.as<uint8_t>(), d_out.as<unsigned long long>());
    ix.prof.end(t, "rm_mark", nids * (8 + 8 * (uint64_t)bit_width64(ndocs) + 1), s);
    CDB_HIP(hipGetLastError());
    // survivors and their bytes (the host sizes the new tables from them)
    KeptIn kin{p.drop.as<uint8_t>(), doc_start};
    t = ix.prof.begin(s);
    longest_document(s, p.drop.as<uint8_t>(), doc_start, ndocs, d_out.as<unsigned long long>() + 1);
    uint64_t out[2] = {0, 0};
    CDB_HIP(hipMemcpyAsync(out, d_out.p, 16, hipMemcpyDeviceToHost, s));
    const U2 tot = scan_totals<U2>(s, ix.scan_partials, kin, ndocs, OpAdd{}, U2{0, 0});  // (synchronises: out is here)
    CDB_HIP(hipGetLastError());
    p.missing = out[0];
    p.longest = out[1];
    p.ndocs = tot.a;
    p.size = tot.b;
    p.removed = ndocs - tot.a;
    if (p.removed) {
        p.newdoc.alloc(ndocs * 4);
        p.d_ids.alloc(std::max<uint64_t>(p.ndocs, 1) * 8);
        p.d_start.alloc((p.ndocs + 1) * 8);
        p.src_start.alloc(std::max<uint64_t>(p.ndocs, 1) * 8);
        scan_apply<U2>(s, ix.scan_partials, kin, ndocs, OpAdd{}, U2{0, 0},
                       TablesOut{p.drop.as<uint8_t>(), doc_start, ix.d_ids.as<int64_t>(), ndocs, p.newdoc.as<uint32_t>(), p.d_ids.as<int64_t>(),
                                 p.d_start.as<uint64_t>(), p.src_start.as<uint64_t>()});
        CDB_HIP(hipGetLastError());
    }
    ix.prof.end(t, "rm_tables", ndocs * (2 * 9 + 9) + (p.removed ? ndocs * 4 + p.ndocs * 24 : 0), s);
}

void remove_text(Index& ix, RemovePlan& p) {
    hipStream_t s = ix.stream;
    p.text.alloc(p.size + TEXT_PAD);
    CDB_HIP(hipMemsetAsync((uint8_t*)p.text.p + p.size, 0, TEXT_PAD, s));
    if (!p.size) return;
    const uint64_t nranges = ceil_div(p.size, RM_TEXT_RANGE);
    int t = ix.prof.begin(s);
    hipLaunchKernelGGL(rm_text_kernel, dim3((unsigned)std::min<uint64_t>(nranges, 1u << 16)), dim3(256), 0, s, ix.d_text, ix.size,
                       (const uint64_t*)p.d_start.as<uint64_t>(), (const uint64_t*)p.src_start.as<uint64_t>(), p.ndocs, p.size,
                       p.text.as<uint8_t>());
    ix.prof.end(t, "rm_text", 2 * p.size, s);
    CDB_HIP(hipGetLastError());
}

void remove_compact(Index& ix, RemovePlan& p, int new_bits, int new_width, bool new_packed) {
    hipStream_t s = ix.stream;
    const uint64_t n = ix.size, m = p.size;
    p.arr.alloc(m, new_width, new_packed);
    if (!m) return;  // (what a build leaves for an empty column: a block, no keys)
    const bool with_keys = ix.key_nsym && (ix.d_keys.p || ix.d_keys32.p);
    const KeptKeys keys_in = with_keys ? keys_of(ix) : KeptKeys{}, keys_out = with_keys ? p.arr.alloc_keys_like(ix, m) : KeptKeys{};
    const uint64_t ntiles = ceil_div(n, ST_TILE);
    DevBuf tile_base;
    const EntryKept kept{ix.d_sa.as<uint32_t>(), (!ix.sa_packed && ix.width == 8) ? 2 : 1, (uint32_t)ix.mask, p.drop.as<uint8_t>()};
    if (tile_bases(ix, "remove", kept, n, tile_base, "rm_count", n * (4 + 1) + ntiles * 8) != m)
        throw InternalError("remove: kept entries and kept bytes differ (internal)");
    const int old_bytes = ix.sa_packed ? 5 : ix.width;
    const int t = ix.prof.begin(s);
    sa_dispatch(ix, [&](auto src_tag) {
        using S = decltype(src_tag);
        auto launch = [&](auto dst) {
            using D = decltype(dst);
            hipLaunchKernelGGL((rm_compact_kernel<S, D>), dim3((unsigned)ntiles), dim3(256), 0, s, ix.sa_view<S>(), n, (int)ix.bits, ix.mask, new_bits,
                               (const uint8_t*)p.drop.as<uint8_t>(), (const uint32_t*)p.newdoc.as<uint32_t>(),
                               (const uint64_t*)tile_base.as<uint64_t>(), dst, keys_in, keys_out);
        };
        if (new_packed) launch(Sa40RW{p.arr.sa.as<uint32_t>(), p.arr.sa_hi.as<uint8_t>()});
        else if (new_width == 8) launch(SaRW<uint64_t>{p.arr.sa.as<uint64_t>()});
        else launch(SaRW<uint32_t>{p.arr.sa.as<uint32_t>()});
    });
    ix.prof.end(t, "rm_compact",
                n * ((uint64_t)old_bytes + 1) + m * ((new_packed ? 5 : (uint64_t)new_width) + 4 + 2 * keys_out.bytes_per_slot()) + ntiles * 8, s);
    CDB_HIP(hipGetLastError());
}

}  // namespace cdb
