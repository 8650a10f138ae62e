// debug_segsort.hip — test hook for the segmented sort of (u32 key, u32 entry, u16 aux) bucket records in its two forms
// (radix_sort.h: radix_sort_segmented over five passes, radix_sort_top_first), in a translation unit of its own like the other
// debug_*.hip.  Nothing here is called by a production path; the hook runs what run_segmented (sa_build.hip) runs for ONE bucket
// group behind the sweep, with the same functions: rs_seg_tilemap_kernel, then either rs_seg_hist_kernel + radix_sort_segmented<u16>
// or radix_sort_top_first<u16> with the SegFinalArgs the build fills in (as SegFinalCellArgs: rs_top_first_fin).  Host arrays in, host arrays out, a stream of its own,
// poisoned guards around every device array a pass writes.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "index_impl.h"
#include "radix_sort.h"

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
constexpr uint64_t GUARD = 4096;  // poisoned elements in front of and behind every guarded array (keeps 256-byte alignment)

void need(bool ok, const char* what) {
    if (!ok) throw Error(std::string("cdb_debug_segsort: ") + what);
}

// n elements of esz bytes between two poisoned guards
struct Guarded {
    DevBuf d;
    size_t esz = 0, n = 0;
    void alloc(size_t n_, size_t esz_, hipStream_t s) {
        n = n_;
        esz = esz_;
        d.alloc((n + 2 * GUARD) * esz);
        CDB_HIP(hipMemsetAsync(d.p, GUARD_BYTE, (n + 2 * GUARD) * esz, s));
    }
    template <typename T> T* ptr() const { return reinterpret_cast<T*>((char*)d.p + GUARD * esz); }
    bool intact(hipStream_t s) const {  // (after the stream was synchronised)
        std::vector<unsigned char> g(2 * GUARD * esz);
        CDB_HIP(hipMemcpyAsync(g.data(), d.p, GUARD * esz, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipMemcpyAsync(g.data() + GUARD * esz, (char*)d.p + (GUARD + n) * esz, GUARD * esz, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        for (unsigned char b : g)
            if (b != GUARD_BYTE) return false;
        return true;
    }
};

}  // namespace

extern "C" {

int cdb_debug_segsort(int device, int form, int packed, uint64_t n, uint32_t nb, const uint64_t* bucket_begin, const uint32_t* k32,
                      const uint32_t* v32, const uint16_t* w16, int ehb, int carry, uint64_t* out_entries, uint8_t* out_flags,
                      uint64_t* out_cells, uint32_t cells_cap, uint32_t* out_ncells, int* out_guard_ok) {
    if (out_guard_ok) *out_guard_ok = 0;
    if (out_ncells) *out_ncells = 0;
    return guarded_hook("cdb_debug_segsort", [&] {
        need(bucket_begin && k32 && v32 && w16 && out_entries && out_flags && out_ncells && out_guard_ok, "null argument");
        need(form == CDB_DEBUG_SEGSORT_FIVE_PASS || form == CDB_DEBUG_SEGSORT_TOP_FIRST, "form");
        need(packed == 0 || packed == 1, "packed");
        need(n >= 1 && n <= (1ull << 22) && nb >= 1 && nb <= 256, "size");
        need(ehb >= 0 && ehb <= 8 && carry >= 0 && carry <= 6 && ehb + carry <= 8, "entry / carried bits");
        need(bucket_begin[0] == 0 && bucket_begin[nb] == n, "buckets do not cover the records");
        std::vector<SegInfo> segs(nb);
        uint32_t tiles = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            need(bucket_begin[b] <= bucket_begin[b + 1], "bucket bounds descend");
            segs[b] = SegInfo{(unsigned long long)bucket_begin[b], (unsigned long long)bucket_begin[b + 1], tiles, 0u, 0ull, 0ull};
            tiles += (uint32_t)ceil_div(bucket_begin[b + 1] - bucket_begin[b], (uint64_t)RS_SEG_TILE);
        }
        need(bucket_begin[nb - 1] < n, "the last bucket is empty");
        for (uint64_t i = 0; i < n; ++i) need(((uint32_t)w16[i] >> 8) >> (ehb + carry) == 0, "aux bits above the entry's and the carried ones");
        need(form == CDB_DEBUG_SEGSORT_FIVE_PASS || (out_cells && cells_cap >= nb * 256u), "cell table");

        CallStream cs(device);
        hipStream_t s = cs.s;
        StreamScope sscope(s);
        if (!rs_atomic_rank_ok(s)) throw InternalError("cdb_debug_segsort: needs the one-atomic ranking (internal)");
        const uint32_t cell_tiles_max = tiles + (form == CDB_DEBUG_SEGSORT_TOP_FIRST ? nb * 256u : 0u);
        Guarded k[2], v[2], w[2], eout, ehi, flags;
        for (int q = 0; q < 2; ++q) {
            k[q].alloc(n, 4, s);
            v[q].alloc(n, 4, s);
            w[q].alloc(n, 2, s);
        }
        eout.alloc(n, packed ? 4 : 8, s);
        ehi.alloc(n, 1, s);
        flags.alloc(n, 1, s);
        CDB_HIP(hipMemcpyAsync(k[0].ptr<uint32_t>(), k32, n * 4, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(v[0].ptr<uint32_t>(), v32, n * 4, hipMemcpyHostToDevice, s));
        CDB_HIP(hipMemcpyAsync(w[0].ptr<uint16_t>(), w16, n * 2, hipMemcpyHostToDevice, s));
        DevBuf d_segs, d_tile_seg, d_hist, d_starts, edges;
        d_segs.alloc((size_t)nb * sizeof(SegInfo));
        CDB_HIP(hipMemcpyAsync(d_segs.p, segs.data(), (size_t)nb * sizeof(SegInfo), hipMemcpyHostToDevice, s));
        d_tile_seg.alloc((size_t)tiles * sizeof(uint32_t));
        d_hist.alloc((size_t)nb * 8 * 256 * sizeof(uint64_t));
        d_starts.alloc((size_t)nb * 8 * 256 * sizeof(uint64_t));
        edges.alloc((size_t)cell_tiles_max * 256 * (form == CDB_DEBUG_SEGSORT_TOP_FIRST ? sizeof(SegCellEdge) : sizeof(SegEdge)));
        hipLaunchKernelGGL(rs_seg_tilemap_kernel, dim3((unsigned)ceil_div(tiles, 256u)), dim3(256), 0, s, (const SegInfo*)d_segs.as<SegInfo>(), nb, tiles,
                           d_tile_seg.as<uint32_t>());
        // the last pass's arguments as run_segmented fills them in (variable-length keys: kbase 2, no magic; blow = 8)
        SegFinalArgs fin;
        if (packed) {
            fin.elo = eout.ptr<uint32_t>();
            fin.ehi = ehi.ptr<uint8_t>();
        } else {
            fin.eout = eout.ptr<uint64_t>();
        }
        fin.flags = flags.ptr<uint8_t>();
        fin.edges = edges.as<SegEdge>();
        fin.hi_shift = 8;
        fin.low_bits = 8;
        fin.kbase = 2;
        fin.kmagic = 0;
        if (carry) {
            fin.hi_mask = (1u << ehb) - 1u;
            fin.carry_mask = (1u << carry) - 1u;
            fin.carry_shift = 8 + ehb;
        }
        RadixWorkspace ws;
        ws.allow_group = true;
        Profiler prof;
        TopFirstWork tfw;
        uint32_t ncell = 0;
        if (form == CDB_DEBUG_SEGSORT_TOP_FIRST) {
            tfw.alloc(nb * 256u, cell_tiles_max);
            const SegFinalCellArgs cfin = rs_top_first_fin(fin, ehb);
            ncell = radix_sort_top_first<uint16_t>(s, ws, prof, k[0].ptr<uint32_t>(), k[1].ptr<uint32_t>(), v[0].ptr<uint32_t>(), v[1].ptr<uint32_t>(),
                                                   w[0].ptr<uint16_t>(), w[1].ptr<uint16_t>(), n, (const SegInfo*)d_segs.as<SegInfo>(), segs.data(),
                                                   (const uint32_t*)d_tile_seg.as<uint32_t>(), nb, tiles, d_hist.as<unsigned long long>(),
                                                   d_starts.as<unsigned long long>(), tfw, cfin, nullptr);
        } else {
            CDB_HIP(hipMemsetAsync(d_hist.p, 0, (size_t)nb * 8 * 256 * sizeof(uint64_t), s));
            hipLaunchKernelGGL((rs_seg_hist_kernel<uint16_t>), dim3((unsigned)ceil_div(tiles, (uint32_t)RS_MSD_HIST_TILES)), dim3(1024), 0, s,
                               (const uint32_t*)k[0].ptr<uint32_t>(), (const uint16_t*)w[0].ptr<uint16_t>(), 1, 5, (const uint32_t*)d_tile_seg.as<uint32_t>(),
                               (const SegInfo*)d_segs.as<SegInfo>(), tiles, d_hist.as<unsigned long long>());
            radix_sort_segmented<uint16_t>(s, ws, prof, k[0].ptr<uint32_t>(), k[1].ptr<uint32_t>(), v[0].ptr<uint32_t>(), v[1].ptr<uint32_t>(),
                                           w[0].ptr<uint16_t>(), w[1].ptr<uint16_t>(), n, (const SegInfo*)d_segs.as<SegInfo>(),
                                           (const uint32_t*)d_tile_seg.as<uint32_t>(), nb, tiles, (const unsigned long long*)d_hist.as<unsigned long long>(),
                                           d_starts.as<unsigned long long>(), 32, 1, fin, nullptr);
        }
        CDB_HIP(hipStreamSynchronize(s));
        radix_check_error(s, ws);
        if (packed) {
            std::vector<uint32_t> lo(n);
            std::vector<uint8_t> hi(n);
            CDB_HIP(hipMemcpyAsync(lo.data(), eout.ptr<uint32_t>(), n * 4, hipMemcpyDeviceToHost, s));
            CDB_HIP(hipMemcpyAsync(hi.data(), ehi.ptr<uint8_t>(), n, hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
            for (uint64_t i = 0; i < n; ++i) out_entries[i] = ((uint64_t)hi[i] << 32) | lo[i];
        } else {
            CDB_HIP(hipMemcpyAsync(out_entries, eout.ptr<uint64_t>(), n * 8, hipMemcpyDeviceToHost, s));
        }
        CDB_HIP(hipMemcpyAsync(out_flags, flags.ptr<uint8_t>(), n, hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        for (uint32_t c = 0; c < ncell; ++c) {
            out_cells[3 * c] = tfw.h_cells[c].begin;
            out_cells[3 * c + 1] = tfw.h_cells[c].end;
            out_cells[3 * c + 2] = tfw.h_cells[c].tile_begin;
        }
        *out_ncells = ncell;
        int ok = 1;
        for (const Guarded* g : {&k[0], &k[1], &v[0], &v[1], &w[0], &w[1], &eout, &flags}) ok &= g->intact(s) ? 1 : 0;
        if (packed) ok &= ehi.intact(s) ? 1 : 0;
        *out_guard_ok = ok;
        ws.release();
    });
}

}  // extern "C"
