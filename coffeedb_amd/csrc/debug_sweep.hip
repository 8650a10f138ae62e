// debug_sweep.hip — test hooks for the record sweeps of the bucket-wise build (records_sweep.h: rs_sweep_records_kernel,
// rs_sweep_records_vl_kernel) and the bucket histograms counted from their records (radix_sort.h: rs_seg_hist_kernel), in a
// translation unit of their own like debug_sort.hip and debug_scan.hip.  Nothing here is called by a production path; the hook
// runs what run_segmented and the sweep prologue of sa_build.hip run for ONE bucket group, with the same functions: rs_tile_bases
// over the uploaded per-tile byte counts, rs_tiledoc_kernel over RS_SWEEP_TILE, rs_seg_tilemap_kernel, a TextGen filled like the
// build's, then radix_sweep_records<W> / radix_sweep_records_vl<W>.  Host arrays in, host arrays out, a stream of its own.
//
// The sweeps trust their tables (the build makes them from the text it sweeps); a test hands them over by hand, so the hook
// refuses every combination under which a record could land outside the group's buffers before it launches anything: the
// counts must be the text's, every kept byte must own its slot's column, and the group must hold exactly its slots' records.
// The msd sweep (rs_sweep_msd_kernel) takes its counts from kernels private to sa_build.hip and is not reachable from here.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "index_impl.h"
#define RS_SWEEP_NO_MSD_KERNEL  // (the header's one non-template kernel stays sa_build.hip's)
#include "records_sweep.h"

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

constexpr unsigned char GUARD_BYTE = 0xA5;
constexpr uint64_t GUARD_RECS = 4096;  // poisoned records in front of and behind every record buffer
constexpr uint64_t PAD_BYTES = 128;    // bytes behind the text of a padded buffer (>= RS_GEN_LOOK + 16)

void need(bool ok, const char* what) {
    if (!ok) throw Error(std::string("cdb_debug_sweep_records: ") + what);
}

// everything a record's destination depends on, checked on the host (see the top of the file)
void validate(const cdb_debug_sweep_args& a, uint32_t tiles8, uint32_t& seg_tiles) {
    need(a.text && a.doc_start && a.codeslot && a.slotmap && a.src_col && a.slot_start && a.tile_counts, "null input");
    need(a.seg_begin && a.seg_end && a.seg_tile_begin && a.out_k && a.out_v && a.out_w && a.out_hist && a.out_guard_ok, "null segment or output");
    need(a.n >= 1 && a.n <= (1ull << 26) && a.ndocs >= 1 && a.ndocs <= a.n + (1ull << 20), "size");
    need(a.bits >= 1 && a.bits <= 39 && (a.padded == 0 || a.padded == 1), "bits / padded");
    need(a.aux_bytes == 1 || a.aux_bytes == 2 || a.aux_bytes == 4, "aux_bytes");
    need(a.rec_low_bits >= 0 && a.rec_low_bits <= 24 && a.rec_low_bits % 8 == 0 && a.rec_low_bits <= 8 * a.aux_bytes, "rec_low_bits");
    need(a.npass >= 1 && a.npass <= 8 && a.lead >= 0 && a.lead <= a.npass && a.lead <= a.aux_bytes, "passes");
    need(a.g0 < a.g1 && a.g1 <= (a.vl ? 128u : 255u), "group");
    need(a.doc_start[0] == 0 && a.doc_start[a.ndocs] == a.n, "documents");
    for (uint64_t d = 0; d < a.ndocs; ++d) need(a.doc_start[d] <= a.doc_start[d + 1], "documents unordered");
    if (a.vl) {
        need(a.vl_sym && a.vl_dec, "code tables");
        need(a.end_len >= 1 && a.end_len <= VL_MAX_LEN && a.carry >= 0, "code shape");
    } else {
        need(a.part_m >= 1 && a.part_m < 256, "part_m");
    }
    // the counts are the text's: tile t holds tile_counts[t][b] bytes b
    std::vector<uint64_t> total(256, 0);
    {
        std::vector<uint32_t> c(256);
        for (uint32_t t = 0; t < tiles8; ++t) {
            std::fill(c.begin(), c.end(), 0u);
            const uint64_t p0 = (uint64_t)t * RS_SWEEP_TILE, p1 = std::min<uint64_t>(a.n, p0 + RS_SWEEP_TILE);
            for (uint64_t p = p0; p < p1; ++p) c[a.text[p]]++;
            need(std::memcmp(c.data(), a.tile_counts + (size_t)t * 256, 256 * sizeof(uint32_t)) == 0, "tile_counts are not the text's");
            for (int b = 0; b < 256; ++b) total[b] += c[b];
        }
    }
    // a kept byte is the one column of its slot, names that slot again in phase B, and its slot's records lie inside the group
    std::vector<int> owner(256, -1);
    for (int b = 0; b < 256; ++b) {
        const uint32_t code = a.codeslot[b] & 0xFFu, slot = a.codeslot[b] >> 8;
        if (a.vl) {
            const uint32_t len = a.vl_sym[code & 0x7Fu] >> 8;
            need(len >= 1 && len <= (uint32_t)VL_MAX_LEN, "a byte's code word has no length of 1 .. 7 bits");
        }
        if (slot < a.g0 || slot >= a.g1 || total[b] == 0) continue;  // (a byte the text does not hold keeps code 0, slot 0)
        need(owner[slot] < 0 && a.src_col[slot] == (uint16_t)b, "a kept byte is not the one column of its slot");
        owner[slot] = b;
        if (a.vl) {
            need(code >= 1 && code < 128, "kept code outside the code tables");
            const uint32_t sy = a.vl_sym[code], len = sy >> 8, word = sy & 0xFFu;
            need(word < (1u << len), "code word wider than its length");
            for (uint32_t x = 0; x < (1u << (VL_MAX_LEN - len)); ++x)
                need(a.vl_dec[(word << (VL_MAX_LEN - len)) | x] == (uint16_t)(slot | (len << 8)), "decode table does not name the kept slot");
        } else {
            need(a.slotmap[code] == slot, "slotmap does not name the kept slot");
        }
    }
    for (uint32_t d = a.g0; d < a.g1; ++d) {
        const uint64_t cnt = owner[d] >= 0 ? total[owner[d]] : 0;
        need(owner[d] >= 0 || a.src_col[d] == 0xFFFFu || total[a.src_col[d] & 0xFFu] == 0, "slot column without a kept byte");
        need(a.slot_start[d] >= a.gstart && a.slot_start[d] - a.gstart + cnt <= a.gelems, "slot outside the group");
        // the segment of the slot is its range of records, tiles in running order (run_segmented)
        const uint32_t i = d - a.g0;
        need(a.seg_begin[i] == a.slot_start[d] - a.gstart && a.seg_end[i] == a.seg_begin[i] + cnt, "segment is not its slot's records");
        need(a.seg_tile_begin[i] == seg_tiles, "segment tiles");
        seg_tiles += (uint32_t)ceil_div(cnt, (uint64_t)RS_SEG_TILE);
    }
    need(seg_tiles >= 1 && a.gelems >= 1, "empty group");
}

template <typename W>
void sweep_group(hipStream_t s, const cdb_debug_sweep_args& a) {
    const uint64_t n = a.n, D = a.ndocs;
    const uint32_t tiles8 = (uint32_t)ceil_div(n, (uint64_t)RS_SWEEP_TILE), nseg = a.g1 - a.g0;
    uint32_t seg_tiles = 0;
    validate(a, tiles8, seg_tiles);
    if (!rs_atomic_rank_ok(s)) throw InternalError("cdb_debug_sweep_records: needs the one-atomic ranking (internal)");

    auto upload = [&](DevBuf& d, const void* h, size_t bytes) {
        d.alloc(bytes);
        CDB_HIP(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, s));
    };
    DevBuf d_text, d_docs, d_codeslot, d_slotmap, d_symmap, d_src_col, d_slot_start, d_counts, d_segs, d_tile_seg, d_tile_doc, d_hist, d_vl_sym, d_vl_dec;
    const size_t text_bytes = (size_t)n + (a.padded ? PAD_BYTES : 0);
    d_text.alloc(text_bytes);
    if (a.padded) CDB_HIP(hipMemsetAsync(d_text.p, GUARD_BYTE, text_bytes, s));
    CDB_HIP(hipMemcpyAsync(d_text.p, a.text, n, hipMemcpyHostToDevice, s));
    upload(d_docs, a.doc_start, (size_t)(D + 1) * sizeof(uint64_t));
    upload(d_codeslot, a.codeslot, 256 * sizeof(uint16_t));
    std::vector<uint8_t> slotmap(260, 0);
    std::memcpy(slotmap.data(), a.slotmap, 257);
    upload(d_slotmap, slotmap.data(), slotmap.size());
    std::vector<uint16_t> symmap(256);
    for (int b = 0; b < 256; ++b) symmap[b] = (uint16_t)(a.codeslot[b] & 0xFFu);
    upload(d_symmap, symmap.data(), 256 * sizeof(uint16_t));
    upload(d_src_col, a.src_col, 256 * sizeof(uint16_t));
    upload(d_slot_start, a.slot_start, 256 * sizeof(uint64_t));
    upload(d_counts, a.tile_counts, (size_t)tiles8 * 256 * sizeof(uint32_t));
    std::vector<SegInfo> segs(nseg);
    for (uint32_t i = 0; i < nseg; ++i)
        segs[i] = SegInfo{(unsigned long long)a.seg_begin[i], (unsigned long long)a.seg_end[i], a.seg_tile_begin[i], 0u, 0ull, 0ull};
    upload(d_segs, segs.data(), (size_t)nseg * sizeof(SegInfo));
    d_tile_seg.alloc((size_t)seg_tiles * sizeof(uint32_t));
    d_tile_doc.alloc(((size_t)tiles8 + 1) * sizeof(uint64_t));
    d_hist.alloc((size_t)nseg * 8 * 256 * sizeof(uint64_t));
    if (a.vl) {
        upload(d_vl_sym, a.vl_sym, 256 * sizeof(uint16_t));
        upload(d_vl_dec, a.vl_dec, 128 * sizeof(uint16_t));
    }
    // the record buffers between two poisoned guards
    const uint64_t recs = a.gelems + 2 * GUARD_RECS;
    DevBuf d_k, d_v, d_w;
    d_k.alloc(recs * sizeof(uint32_t));
    d_v.alloc(recs * sizeof(uint32_t));
    d_w.alloc(recs * sizeof(W));
    CDB_HIP(hipMemsetAsync(d_k.p, GUARD_BYTE, recs * sizeof(uint32_t), s));
    CDB_HIP(hipMemsetAsync(d_v.p, GUARD_BYTE, recs * sizeof(uint32_t), s));
    CDB_HIP(hipMemsetAsync(d_w.p, GUARD_BYTE, recs * sizeof(W), s));

    // the sweep prologue of sa_build.hip: tile bases of every bucket slot, the document of every tile's first position
    TileBaseWorkspace tbw;
    const unsigned long long* tile_base = rs_tile_bases(s, tbw, d_counts.as<uint32_t>(), tiles8, d_src_col.as<uint16_t>(),
                                                        (const unsigned long long*)d_slot_start.as<unsigned long long>());
    hipLaunchKernelGGL(rs_tiledoc_kernel, dim3((unsigned)ceil_div((uint64_t)tiles8 + 1, 256)), dim3(256), 0, s, (const uint64_t*)d_docs.as<uint64_t>(),
                       D, n, (uint64_t)RS_SWEEP_TILE, (uint64_t)tiles8, d_tile_doc.as<uint64_t>());
    // one group of run_segmented
    hipLaunchKernelGGL(rs_seg_tilemap_kernel, dim3((unsigned)ceil_div(seg_tiles, 256u)), dim3(256), 0, s, (const SegInfo*)d_segs.as<SegInfo>(), nseg,
                       seg_tiles, d_tile_seg.as<uint32_t>());
    TextGen rg{d_text.as<uint8_t>(), d_docs.as<uint64_t>(), d_symmap.as<uint16_t>(), D, a.bits, a.vl ? 0u : a.base, a.vl ? 0 : a.nsym, 0, a.padded != 0};
    rg.slotmap = d_slotmap.as<uint8_t>();
    rg.rec_low_bits = a.rec_low_bits;
    if (!a.vl && a.part_m > 1) {
        TextGen pg{};
        if (!rs_part_setup(pg, a.base, a.part_m)) throw Error("cdb_debug_sweep_records: no quantiser for (base, part_m)");
        rg.part_m = a.part_m;
        rg.part_r = pg.part_r;
        rg.part_s = pg.part_s;
    }
    rg.tile_doc = d_tile_doc.as<uint64_t>();
    rg.tile_base = tile_base;
    Profiler prof;
    uint32_t* const k = d_k.as<uint32_t>() + GUARD_RECS;
    uint32_t* const v = d_v.as<uint32_t>() + GUARD_RECS;
    W* const w = d_w.as<W>() + GUARD_RECS;
    if (a.vl) {
        VlTables vt;
        vt.sym = d_vl_sym.as<uint16_t>();
        vt.dec = d_vl_dec.as<uint16_t>();
        vt.key_bits = a.key_bits;
        vt.end_len = a.end_len;
        vt.carry = a.carry;
        vt.carry_shift = a.carry_shift;
        radix_sweep_records_vl<W>(s, prof, k, v, w, n, rg, (const uint16_t*)d_codeslot.as<uint16_t>(), vt, a.g0, a.g1, a.gstart, a.gelems,
                                  (const uint32_t*)d_tile_seg.as<uint32_t>(), (const SegInfo*)d_segs.as<SegInfo>(), nseg, seg_tiles, a.lead, a.npass,
                                  d_hist.as<unsigned long long>(), nullptr);
    } else {
        radix_sweep_records<W>(s, prof, k, v, w, n, rg, (const uint16_t*)d_codeslot.as<uint16_t>(), a.g0, a.g1, a.gstart, a.gelems,
                               (const uint32_t*)d_tile_seg.as<uint32_t>(), (const SegInfo*)d_segs.as<SegInfo>(), nseg, seg_tiles, a.lead, a.npass,
                               d_hist.as<unsigned long long>(), nullptr);
    }
    CDB_HIP(hipGetLastError());

    std::vector<unsigned char> gk(2 * GUARD_RECS * 4), gv(2 * GUARD_RECS * 4), gw(2 * GUARD_RECS * sizeof(W));
    auto fetch = [&](const DevBuf& d, size_t esz, void* out, std::vector<unsigned char>& g) {
        const char* p = (const char*)d.p;
        CDB_HIP(hipMemcpyAsync(g.data(), p, GUARD_RECS * esz, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(out, p + GUARD_RECS * esz, a.gelems * esz, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(g.data() + GUARD_RECS * esz, p + (GUARD_RECS + a.gelems) * esz, GUARD_RECS * esz, hipMemcpyDeviceToHost, s));
    };
    fetch(d_k, 4, a.out_k, gk);
    fetch(d_v, 4, a.out_v, gv);
    fetch(d_w, sizeof(W), a.out_w, gw);
    CDB_HIP(hipMemcpyAsync(a.out_hist, d_hist.p, (size_t)nseg * 8 * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (a.out_tile_base) CDB_HIP(hipMemcpyAsync(a.out_tile_base, tile_base, (size_t)tiles8 * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (a.out_tile_doc) CDB_HIP(hipMemcpyAsync(a.out_tile_doc, d_tile_doc.p, ((size_t)tiles8 + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    CDB_HIP(hipStreamSynchronize(s));
    int ok = 1;
    for (const std::vector<unsigned char>* g : {&gk, &gv, &gw})
        for (unsigned char b : *g) ok &= b == GUARD_BYTE;
    *a.out_guard_ok = ok;
}

}  // namespace

extern "C" {

int cdb_debug_sweep_records(int device, const cdb_debug_sweep_args* args) {
    if (!args) return CDB_E_INVALID;
    if (args->out_guard_ok) *args->out_guard_ok = 0;
    return guarded_hook("cdb_debug_sweep_records", [&] {
        const cdb_debug_sweep_args& a = *args;
        need(a.aux_bytes == 1 || a.aux_bytes == 2 || a.aux_bytes == 4, "aux_bytes");
        CallStream cs(device);
        hipStream_t s = cs.s;
        StreamScope sscope(s);
        if (a.aux_bytes == 1) sweep_group<uint8_t>(s, a);
        else if (a.aux_bytes == 2) sweep_group<uint16_t>(s, a);
        else sweep_group<uint32_t>(s, a);
    });
}

int cdb_debug_vl_tables(const uint64_t* counts, int sigma, const uint8_t* slot_of_code, uint16_t* sym_out, uint16_t* dec_out, int* end_len_out) {
    if (!counts || !slot_of_code || !sym_out || !dec_out || !end_len_out || sigma < 2 || sigma > 127) return CDB_E_INVALID;
    return guarded_hook("cdb_debug_vl_tables", [&] {
        VlCode code;
        if (!vl_build(counts, sigma, code)) throw Error("cdb_debug_vl_tables: no code within the length limit");
        vl_fill_tables(code, slot_of_code, sigma, sym_out, dec_out);
        *end_len_out = code.end_len;
    });
}

}  // extern "C"
