// render.hip — a page of result rows rendered on the device (include/coffeedb_gpu.h: cdb_render_rows): the tail of select()
// (database.cpp:394-441), which runs ac_automaton::render (database.cpp:58-90) over every returned object's string.
//
// The work is laid over the PAGE: the documents of the found rows end to end, in the caller's row order — P page positions.
//   1. id -> document by bisection over the id table (index_impl.h: IdTable), row lengths scanned into page_ptr[nrows + 1].
//   2. match: a workgroup per tile of SC_TILE page positions stages its bytes (+ a halo) in the LDS, document piece by document
//      piece, and writes for every position the length of the LONGEST keyword that starts there and ends inside the document —
//      shorter occurrences from the same start lie inside it, so the union of occurrences is unchanged.  Keyword lists beyond one
//      LDS chunk run as several launches combined by an elementwise maximum.
//   3. running maximum of reach = p + length over the page positions.  The reference's pop / extend / append rule (database.cpp:
//      62-77) without the list: p begins a span iff its own reach > p and the maximum before it <= p; p ends a span iff the maximum
//      up to and including it == p + 1.  No segment flags are needed: an occurrence ends inside its row and rows lie in page order,
//      so whatever earlier rows reached is <= the first position of this row.
//   4. add-scan of the begin and end marks: every byte's output offset is p + left_len * begins so far + right_len * ends before;
//      the apply step copies the bytes, the owner of a mark writes `left` / `right` and the span's page position.
//   5. per row: span_ptr by bisection over the spans' page positions, text_ptr from it; per span: offsets inside the document.
// No sort, no atomic per occurrence, no loop along a document: one very long document spreads over as many workgroups as it has tiles.
#include <algorithm>
#include <cstring>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"
#include "scan.h"

using namespace cdb;

namespace {

// LDS of the match kernel: 4 KiB + halo of text, 4 bytes per staged position for the end of its row, and one keyword chunk —
// 30.5 KiB, five workgroups per CU (160 KiB).  A keyword's first RN_HEAD bytes sit in the LDS; what lies behind them, and text behind
// the halo, is compared from global memory (only ever reached behind RN_HEAD / RN_HALO equal bytes).
constexpr int RN_HALO = 256;
constexpr int RN_STAGE = SC_TILE + RN_HALO;
constexpr int RN_HEAD = 256;
constexpr int RN_MAX_KW = 256;
constexpr int RN_KW_BYTES = 8192;
constexpr uint32_t RN_NODOC = 0xFFFFFFFFu;
constexpr uint64_t RN_MAX_DOC = 0xFFFF0000ull;  // (row ends relative to a tile are kept in 32 bits)

// row i -> doc[i] (RN_NODOC: the index does not hold ids[i]) and found[i]; out[0] += rows missed, out[1] = longest document met
__global__ __launch_bounds__(256) void rnd_lookup_kernel(const int64_t* __restrict__ ids, uint64_t nrows, const int64_t* __restrict__ id_tab,
                                                         const uint32_t* __restrict__ id_doc, uint64_t ndocs, const uint64_t* __restrict__ doc_start,
                                                         uint32_t* __restrict__ doc, uint8_t* __restrict__ found, unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t miss = 0, longest = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nrows; i += stride) {
        const int64_t id = ids[i];
        const uint64_t r = lower_bound_id(id_tab, ndocs, id);
        const bool hit = r < ndocs && id_tab[r] == id;
        uint32_t d = RN_NODOC;
        if (hit) {
            d = id_doc ? id_doc[r] : (uint32_t)r;
            const uint64_t len = doc_start[d + 1] - doc_start[d];
            longest = len > longest ? len : longest;
        }
        miss += hit ? 0 : 1;
        doc[i] = d;
        found[i] = hit ? 1 : 0;
    }
    for (int off = 32; off; off >>= 1) {
        miss += __shfl_xor(miss, off);
        const uint64_t o = __shfl_xor(longest, off);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63) == 0) {
        if (miss) atomicAdd(out, (unsigned long long)miss);
        if (longest) atomicMax(out + 1, (unsigned long long)longest);
    }
}

struct RowLenIn {
    const uint32_t* doc;
    const uint64_t* doc_start;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const uint32_t d = doc[i];
        return d == RN_NODOC ? 0ull : doc_start[d + 1] - doc_start[d];
    }
};
struct PtrOut {
    uint64_t* ptr;
    uint64_t n;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t in) const {
        ptr[i] = ex;
        if (i + 1 == n) ptr[n] = in;
    }
};

// the row of page position p < page_ptr[nrows]: the largest r with page_ptr[r] <= p (rows before it that end at p are empty)
__device__ __forceinline__ uint64_t row_of(const uint64_t* __restrict__ page_ptr, uint64_t nrows, uint64_t p) {
    uint64_t a = 0, b = nrows;  // page_ptr[a] <= p < page_ptr[b]
    while (b - a > 1) {
        const uint64_t m = (a + b) >> 1;
        if (page_ptr[m] <= p) a = m;
        else b = m;
    }
    return a;
}

// One keyword chunk against every tile of the page.  mlen[p] = longest keyword of the chunk at p (FIRST), or the maximum of that
// and what earlier chunks left.  nk = 0 (first chunk only) stages and copies the text alone.  page_text (first chunk, optional)
// receives the page's bytes in page order for the write-out.
template <bool FIRST>
__global__ __launch_bounds__(256) void rnd_match_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_start,
                                                        const uint32_t* __restrict__ doc, const uint64_t* __restrict__ page_ptr, uint64_t nrows,
                                                        uint64_t P, const uint8_t* __restrict__ heads, const uint64_t* __restrict__ head_off,
                                                        const uint32_t* __restrict__ kw_len, const uint8_t* __restrict__ kw_blob,
                                                        const uint64_t* __restrict__ kw_off, uint32_t nk, uint32_t* __restrict__ mlen,
                                                        uint8_t* __restrict__ page_text) {
    __shared__ uint8_t s_text[RN_STAGE];
    __shared__ uint32_t s_end[RN_STAGE];  // end of the position's row, relative to the tile's first position
    __shared__ uint8_t s_kw[RN_KW_BYTES];
    __shared__ uint32_t s_off[RN_MAX_KW + 1];
    __shared__ uint32_t s_len[RN_MAX_KW];
    __shared__ uint32_t s_first[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 8) s_first[threadIdx.x] = 0;
    if (nk)  // (no keywords: no keyword arrays either)
        for (uint32_t i = threadIdx.x; i <= nk; i += 256) s_off[i] = (uint32_t)(head_off[i] - head_off[0]);
    for (uint32_t i = threadIdx.x; i < nk; i += 256) s_len[i] = kw_len[i];
    __syncthreads();
    const uint32_t head_bytes = nk ? s_off[nk] : 0;
    for (uint32_t i = threadIdx.x; i < head_bytes; i += 256) s_kw[i] = heads[head_off[0] + i];
    for (uint32_t i = threadIdx.x; i < nk; i += 256) {
        const uint8_t c = heads[head_off[i]];
        atomicOr(&s_first[c >> 5], 1u << (c & 31));
    }
    const uint64_t ntiles = (P + SC_TILE - 1) / SC_TILE;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * SC_TILE;
        const uint64_t send = base + RN_STAGE < P ? base + RN_STAGE : P;  // staged page positions: [base, send)
        const uint32_t own = (uint32_t)((base + SC_TILE < P ? base + SC_TILE : P) - base);
        const uint32_t staged = (uint32_t)(send - base);
        __syncthreads();  // (the keyword chunk is in place; the previous tile's text has been read)
        // stage: the wavefronts take the rows that overlap [base, send) in turn; 16-byte loads where the source allows
        const uint64_t r0 = row_of(page_ptr, nrows, base);
        for (uint64_t r = r0 + wave; r < nrows; r += 4) {
            const uint64_t rs = page_ptr[r], re = page_ptr[r + 1];
            if (rs >= send) break;
            if (re == rs) continue;
            const uint64_t lo = rs > base ? rs : base, hi = re < send ? re : send;
            const uint8_t* src = text + doc_start[doc[r]] + (lo - rs);
            const uint32_t j0 = (uint32_t)(lo - base), len = (uint32_t)(hi - lo);
            const uint64_t rel = re - base;
            const uint32_t endrel = rel > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rel;
            uint32_t nh = (uint32_t)((16 - ((uintptr_t)src & 15)) & 15);
            nh = nh < len ? nh : len;
            const uint32_t nvec = (len - nh) >> 4, tail0 = nh + (nvec << 4);
            if ((uint32_t)lane < nh) {
                s_text[j0 + lane] = src[lane];
                s_end[j0 + lane] = endrel;
            }
            for (uint32_t v = lane; v < nvec; v += 64) {
                const uint4 x = *reinterpret_cast<const uint4*>(src + nh + (v << 4));
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
                const uint32_t j = j0 + nh + (v << 4);
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    s_text[j + b] = (uint8_t)(w[b >> 2] >> ((b & 3) * 8));
                    s_end[j + b] = endrel;
                }
            }
            if (tail0 + lane < len) {  // (fewer than 16 bytes)
                s_text[j0 + tail0 + lane] = src[tail0 + lane];
                s_end[j0 + tail0 + lane] = endrel;
            }
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < own; j += 256) {
            const uint64_t p = base + j;
            const uint8_t c = s_text[j];
            if (FIRST && page_text) page_text[p] = c;
            uint32_t best = 0;
            if ((s_first[c >> 5] >> (c & 31)) & 1u) {
                const uint32_t room = s_end[j] - j;  // bytes from p to the end of its document
                uint64_t gsrc = ~0ull;               // text offset of p (looked up only when a compare leaves the LDS)
                for (uint32_t k = 0; k < nk; ++k) {
                    const uint32_t a = s_off[k], m = s_len[k];
                    if (s_kw[a] != c || m <= best || m > room) continue;
                    const uint32_t hl = s_off[k + 1] - a;
                    const uint32_t in_lds = min(min(m, hl), staged - j);
                    uint32_t q = 1;
                    while (q < in_lds && s_text[j + q] == s_kw[a + q]) ++q;
                    if (q < in_lds) continue;
                    if (q < m) {  // the keyword's tail and / or text behind the halo: global memory
                        if (gsrc == ~0ull) {
                            const uint64_t r = row_of(page_ptr, nrows, p);
                            gsrc = doc_start[doc[r]] + (p - page_ptr[r]);
                        }
                        const uint8_t* kb = kw_blob + kw_off[k];
                        while (q < m && (j + q < staged ? s_text[j + q] : text[gsrc + q]) == (q < hl ? s_kw[a + q] : kb[q])) ++q;
                        if (q < m) continue;
                    }
                    best = m;
                }
            }
            if (FIRST) {
                mlen[p] = best;
            } else if (best) {
                const uint32_t old = mlen[p];
                if (best > old) mlen[p] = best;
            }
        }
    }
}

// reach of p: one past the last byte of the longest occurrence starting there (0: none)
struct ReachIn {
    const uint32_t* mlen;
    __device__ __forceinline__ uint64_t operator()(uint64_t p) const {
        const uint32_t m = mlen[p];
        return m ? p + m : 0ull;
    }
};
struct MarkOut {  // bit 0: p begins a span, bit 1: p ends one
    const uint32_t* mlen;
    uint8_t* mark;
    __device__ __forceinline__ void operator()(uint64_t p, uint64_t ex, uint64_t in) const {
        const uint8_t b = (mlen[p] != 0 && ex <= p) ? 1 : 0, e = in == p + 1 ? 2 : 0;
        mark[p] = b | e;
    }
};
struct MarkIn {
    const uint8_t* mark;
    __device__ __forceinline__ U2 operator()(uint64_t p) const {
        const uint8_t f = mark[p];
        return U2{(uint64_t)(f & 1), (uint64_t)(f >> 1)};
    }
};
struct WriteOut {
    const uint8_t* mark;
    const uint8_t* page_text;
    const uint8_t* left;
    const uint8_t* right;
    uint64_t L, R;
    uint8_t* blob;       // nullptr: spans only
    uint64_t* span_beg;  // page positions of the spans' first and last bytes
    uint64_t* span_end;
    __device__ __forceinline__ void operator()(uint64_t p, const U2& ex, const U2& in) const {
        const uint8_t f = mark[p];
        if (f & 1) span_beg[ex.a] = p;
        if (f & 2) span_end[ex.b] = p;
        if (!blob) return;
        const uint64_t o = p + L * in.a + R * ex.b;  // (in.a: a span beginning here has its `left` in front of this byte)
        blob[o] = page_text[p];
        if (f & 1)
            for (uint64_t k = 0; k < L; ++k) blob[o - L + k] = left[k];
        if (f & 2)
            for (uint64_t k = 0; k < R; ++k) blob[o + 1 + k] = right[k];
    }
};
// rows: span_ptr[r] = spans that begin before the row's first position, text_ptr from it; spans: offsets inside their document
__global__ __launch_bounds__(256) void rnd_finish_kernel(const uint64_t* __restrict__ page_ptr, uint64_t nrows, const uint64_t* __restrict__ span_beg,
                                                         const uint64_t* __restrict__ span_end, uint64_t nspans, uint64_t LR,
                                                         uint64_t* __restrict__ span_ptr, uint64_t* __restrict__ text_ptr,
                                                         uint64_t* __restrict__ begin, uint64_t* __restrict__ end) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= nrows || i < nspans; i += stride) {
        if (i <= nrows) {
            const uint64_t p = page_ptr[i];
            uint64_t a = 0, b = nspans;
            while (a < b) {
                const uint64_t m = (a + b) >> 1;
                if (span_beg[m] < p) a = m + 1;
                else b = m;
            }
            span_ptr[i] = a;
            text_ptr[i] = p + LR * a;  // (every span in front of a row is complete)
        }
        if (i < nspans) {
            const uint64_t pb = span_beg[i], rs = page_ptr[row_of(page_ptr, nrows, pb)];
            begin[i] = pb - rs;
            end[i] = span_end[i] - rs;
        }
    }
}

// the result arrays: host blocks of the result cache, filled from the device
using Rendered = ResultOwner<cdb_rendered, cdb_rendered_free>;

// the rows as the caller's host ids, or (d_rows != nullptr) as ids that already lie on the handle's device: only the upload differs;
// the keywords are checked (none is empty)
void render_rows(Index& ix, const int64_t* ids, const int64_t* d_rows, uint64_t nrows, const KeywordList& kws, const char* left, uint64_t L,
                 const char* right, uint64_t R, int what, Rendered& res) {
    hipStream_t s = ix.stream;
    const double t0 = wall_ms();
    const bool want_text = (what & CDB_RENDER_TEXT) != 0, want_spans = (what & CDB_RENDER_SPANS) != 0;
    res.r.nrows = nrows;
    ix.rnd = Index::RenderStats{};
    if (ix.width == 0 || ix.ndocs == 0 || nrows == 0) {  // never built: every row missing (cdb_cluster's choice)
        res.r.missing = nrows;
        res.r.found = (uint8_t*)host_alloc(nrows, true);
        if (want_text) {
            res.r.text_ptr = (uint64_t*)host_alloc((nrows + 1) * 8, true);
            res.r.text_blob = (char*)host_alloc(0);
        }
        if (want_spans) {
            res.r.span_ptr = (uint64_t*)host_alloc((nrows + 1) * 8, true);
            res.r.begin = (uint64_t*)host_alloc(0);
            res.r.end = (uint64_t*)host_alloc(0);
        }
        ix.rnd.last_ms = wall_ms() - t0;
        return;
    }
    id_table_prepare(ix);
    const uint64_t ndocs = ix.ndocs;
    const int64_t* id_tab = ix.idt.ids_ascend ? ix.d_ids.as<int64_t>() : ix.idt.id_sorted.as<int64_t>();
    const uint32_t* id_doc = ix.idt.ids_ascend ? nullptr : ix.idt.id_doc.as<uint32_t>();
    const uint64_t* doc_start = ix.d_doc_start.as<uint64_t>();

    // 1. rows -> documents -> page offsets
    DevBuf d_ids, d_out, d_doc, d_found, d_page;
    if (!d_rows) {
        d_ids.alloc(nrows * 8);
        CDB_HIP(hipMemcpyAsync(d_ids.p, ids, nrows * 8, hipMemcpyHostToDevice, s));
        d_rows = d_ids.as<int64_t>();
    }
    d_out.alloc(16);
    CDB_HIP(hipMemsetAsync(d_out.p, 0, 16, s));
    d_doc.alloc(nrows * 4);
    d_found.alloc(nrows);
    d_page.alloc((nrows + 1) * 8);
    int t = ix.prof.begin(s);
    hipLaunchKernelGGL(rnd_lookup_kernel, dim3(grid_for(nrows)), dim3(256), 0, s, d_rows, nrows, id_tab, id_doc, ndocs,
                       doc_start, d_doc.as<uint32_t>(), d_found.as<uint8_t>(), d_out.as<unsigned long long>());
    CDB_HIP(hipGetLastError());
    RowLenIn lin{d_doc.as<uint32_t>(), doc_start};
    uint64_t stats[2] = {0, 0};
    CDB_HIP(hipMemcpyAsync(stats, d_out.p, 16, hipMemcpyDeviceToHost, s));
    const uint64_t P = scan_totals<uint64_t>(s, ix.scan_partials, lin, nrows, OpAdd{}, (uint64_t)0);  // (synchronises: stats are here)
    scan_apply<uint64_t>(s, ix.scan_partials, lin, nrows, OpAdd{}, (uint64_t)0, PtrOut{d_page.as<uint64_t>(), nrows});
    ix.prof.end(t, "rnd_lookup", nrows * (8 + 8 * (uint64_t)bit_width64(ndocs) + 5 + 2 * 20 + 8), s);  // ids, probes, doc + found, two length passes, page_ptr
    CDB_HIP(hipGetLastError());
    const uint64_t missing = stats[0], longest = stats[1];
    if (longest > RN_MAX_DOC) throw Error("cdb_render_rows: documents of 4 GiB and more cannot be rendered");
    const uint64_t* page_ptr = d_page.as<uint64_t>();

    // 2. keywords that can occur at all (not longer than the page's longest document), cut into LDS chunks
    std::vector<uint64_t> h_off, h_head_off{0};
    std::vector<uint32_t> h_len;
    std::string h_heads;
    struct Chunk {
        uint64_t k0;
        uint32_t nk;
    };
    std::vector<Chunk> chunks;
    bool any_tail = false;
    for (uint64_t j = 0; j < kws.n; ++j) {
        const uint64_t m = kws.off[j + 1] - kws.off[j];
        if (m > longest) continue;
        const uint32_t hl = (uint32_t)std::min<uint64_t>(m, RN_HEAD);
        if (chunks.empty() || chunks.back().nk == RN_MAX_KW || h_heads.size() + hl - h_head_off[chunks.back().k0] > RN_KW_BYTES)
            chunks.push_back(Chunk{(uint64_t)h_len.size(), 0});
        ++chunks.back().nk;
        h_heads.append(kws.blob + kws.off[j], hl);
        h_head_off.push_back(h_heads.size());
        h_len.push_back((uint32_t)m);
        h_off.push_back(kws.off[j]);
        any_tail |= m > hl;
    }
    const uint64_t nk_all = h_len.size();
    DevBuf d_heads, d_head_off, d_len, d_kwoff, d_kwblob;
    if (nk_all) {
        d_heads.alloc(h_heads.size());
        d_head_off.alloc((nk_all + 1) * 8);
        d_len.alloc(nk_all * 4);
        d_kwoff.alloc(nk_all * 8);
        CDB_HIP(hipMemcpyAsync(d_heads.p, h_heads.data(), h_heads.size(), hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(d_head_off.p, h_head_off.data(), (nk_all + 1) * 8, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(d_len.p, h_len.data(), nk_all * 4, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(d_kwoff.p, h_off.data(), nk_all * 8, hipMemcpyHostToDevice, s));
        if (any_tail) {  // (keywords longer than RN_HEAD: their tails are compared from the whole list)
            d_kwblob.alloc(kws.off[kws.n]);
            CDB_HIP(hipMemcpyAsync(d_kwblob.p, kws.blob, kws.off[kws.n], hipMemcpyHostToDevice, s));
        }
    }

    DevBuf d_mlen, d_ptext, d_mark, d_sbeg, d_send, d_blob, d_left, d_right, d_sptr, d_tptr, d_begin, d_end;
    uint64_t nspans = 0;
    d_sptr.alloc((nrows + 1) * 8);
    d_tptr.alloc((nrows + 1) * 8);
    if (P) {
        d_mlen.alloc(P * 4);
        d_mark.alloc(P);
        if (want_text) d_ptext.alloc(P);
        const uint64_t ntiles = ceil_div(P, SC_TILE);
        const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 1u << 20);
        t = ix.prof.begin(s);
        if (chunks.empty()) chunks.push_back(Chunk{0, 0});
        for (size_t c = 0; c < chunks.size(); ++c) {
            const uint64_t k0 = chunks[c].k0;
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, ix.d_text, doc_start, (const uint32_t*)d_doc.as<uint32_t>(), page_ptr, nrows, P,
                                   (const uint8_t*)d_heads.as<uint8_t>(), (const uint64_t*)d_head_off.as<uint64_t>() + k0,
                                   (const uint32_t*)d_len.as<uint32_t>() + k0, (const uint8_t*)d_kwblob.as<uint8_t>(),
                                   (const uint64_t*)d_kwoff.as<uint64_t>() + k0, chunks[c].nk, d_mlen.as<uint32_t>(),
                                   want_text ? d_ptext.as<uint8_t>() : (uint8_t*)nullptr);
            };
            if (c == 0) launch(rnd_match_kernel<true>);
            else launch(rnd_match_kernel<false>);
        }
        ix.prof.end(t, "rnd_match", chunks.size() * P * 5 + (want_text ? P : 0), s);
        CDB_HIP(hipGetLastError());

        // 3. running maximum of the reach -> begin / end marks
        t = ix.prof.begin(s);
        ReachIn rin{d_mlen.as<uint32_t>()};
        scan_totals_device<uint64_t>(s, ix.scan_partials, rin, P, OpMax{}, (uint64_t)0);
        scan_apply<uint64_t>(s, ix.scan_partials, rin, P, OpMax{}, (uint64_t)0, MarkOut{d_mlen.as<uint32_t>(), d_mark.as<uint8_t>()});
        ix.prof.end(t, "rnd_max_scan", P * 13, s);
        CDB_HIP(hipGetLastError());

        // 4. add-scan of the marks, write-out
        t = ix.prof.begin(s);
        MarkIn min_{d_mark.as<uint8_t>()};
        const U2 tot = scan_totals<U2>(s, ix.scan_partials, min_, P, OpAdd{}, U2{0, 0});
        ix.prof.end(t, "rnd_mark_scan", P, s);
        if (tot.a != tot.b) throw InternalError("cdb_render_rows: span begins and ends do not pair up (internal)");
        nspans = tot.a;
        d_sbeg.alloc(nspans * 8);
        d_send.alloc(nspans * 8);
        const uint64_t out_bytes = P + nspans * (L + R);
        if (want_text) {
            d_blob.alloc(out_bytes);
            d_left.alloc(L);
            d_right.alloc(R);
            if (L) CDB_HIP(hipMemcpyAsync(d_left.p, left, L, hipMemcpyHostToDevice, s));
            if (R) CDB_HIP(hipMemcpyAsync(d_right.p, right, R, hipMemcpyHostToDevice, s));
        }
        t = ix.prof.begin(s);
        scan_apply<U2>(s, ix.scan_partials, min_, P, OpAdd{}, U2{0, 0},
                       WriteOut{d_mark.as<uint8_t>(), d_ptext.as<uint8_t>(), d_left.as<uint8_t>(), d_right.as<uint8_t>(), L, R,
                                want_text ? d_blob.as<uint8_t>() : (uint8_t*)nullptr, d_sbeg.as<uint64_t>(), d_send.as<uint64_t>()});
        ix.prof.end(t, "rnd_write", P + nspans * 16 + (want_text ? P + out_bytes : 0), s);
        CDB_HIP(hipGetLastError());
    }
    // 5. per-row offsets, spans relative to their documents
    d_begin.alloc(nspans * 8);
    d_end.alloc(nspans * 8);
    t = ix.prof.begin(s);
    hipLaunchKernelGGL(rnd_finish_kernel, dim3(grid_for(std::max(nrows + 1, nspans))), dim3(256), 0, s, page_ptr, nrows,
                       (const uint64_t*)d_sbeg.as<uint64_t>(), (const uint64_t*)d_send.as<uint64_t>(), nspans, L + R, d_sptr.as<uint64_t>(),
                       d_tptr.as<uint64_t>(), d_begin.as<uint64_t>(), d_end.as<uint64_t>());
    ix.prof.end(t, "rnd_finish", (nrows + 1) * (24 + 8 * (uint64_t)bit_width64(nspans)) + nspans * (32 + 8 * (uint64_t)bit_width64(nrows)), s);
    CDB_HIP(hipGetLastError());

    res.r.missing = missing;
    res.r.nspans = nspans;
    res.r.found = res.fetch<uint8_t>(d_found.p, nrows);
    if (want_text) {
        res.r.text_bytes = P + nspans * (L + R);
        res.r.text_ptr = res.fetch<uint64_t>(d_tptr.p, nrows + 1);
        res.r.text_blob = res.fetch<char>(d_blob.p, res.r.text_bytes);
    }
    if (want_spans) {
        res.r.span_ptr = res.fetch<uint64_t>(d_sptr.p, nrows + 1);
        res.r.begin = res.fetch<uint64_t>(d_begin.p, nspans);
        res.r.end = res.fetch<uint64_t>(d_end.p, nspans);
    }
    CDB_HIP(hipStreamSynchronize(s));  // (the device blocks go back to the pool behind this scope)
    ix.prof.resolve();
    ix.rnd.page_bytes = P;
    ix.rnd.spans = nspans;
    ix.rnd.last_ms = wall_ms() - t0;
}

}  // namespace

void cdb::render_index_device_rows(cdb_index* h, const int64_t* d_ids, uint64_t nrows, const char* blob, const uint64_t* offsets, uint64_t nkw,
                                   const char* left, uint64_t left_len, const char* right, uint64_t right_len, int what, cdb_rendered* out) {
    std::lock_guard<std::mutex> g(h->ix.mu);
    DeviceScope scope(h->ix);
    Rendered res(h->ix.stream);
    render_rows(h->ix, nullptr, d_ids, nrows, KeywordList{blob, offsets, nkw}, left, left_len, right, right_len, what, res);
    res.hand_over(out);
}

extern "C" {

int cdb_render_rows(cdb_index* h, const int64_t* ids, uint64_t nrows, const char* blob, const uint64_t* offsets, uint64_t nkw, const char* left,
                    size_t left_len, const char* right, size_t right_len, int what, cdb_rendered* out) {
    if (!h || !out || (nrows && !ids) || (nkw && !offsets) || (left_len && !left) || (right_len && !right)) return CDB_E_INVALID;
    *out = cdb_rendered{};
    return guarded_ix(h->ix, [&] {
        check_keywords(KeywordList{blob, offsets, nkw}, "cdb_render_rows", KW_NONE_EMPTY | KW_BYTES);
        std::lock_guard<std::mutex> g(h->ix.mu);
        DeviceScope scope(h->ix);
        Rendered res(h->ix.stream);
        render_rows(h->ix, ids, nullptr, nrows, KeywordList{blob, offsets, nkw}, left, left_len, right, right_len, what, res);
        res.hand_over(out);
    });
}

void cdb_rendered_free(cdb_rendered* r) {
    if (!r) return;
    host_free(r->found);
    host_free(r->text_ptr);
    host_free(r->text_blob);
    host_free(r->span_ptr);
    host_free(r->begin);
    host_free(r->end);
    std::memset(r, 0, sizeof(*r));
}

}  // extern "C"
