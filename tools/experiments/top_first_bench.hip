// top_first_bench.hip — prices the "top key digit first, then 9-byte records inside cells" form of the segmented sort of the
// bucket-wise build (>= 2^32 suffixes, 40-bit variable-length keys) against the five-pass form.  Written before the form was
// built (radix_sort.h: radix_sort_top_first), from the kernels that existed: "present" and "new" below are of that time.
// 2^lg records in 64 Zipf-sized buckets; key bytes Zipf over 64 values (what follows a symbol inside a bucket), the top key
// byte Zipf over `tops` values (256: ~16 K cells; 32: cells of the size a 2^33 build has at 2^30 records).
//   present: rs_seg_hist (u32 key + u16 aux, five digits) + pass on the aux digit + three key passes, 10-byte records, per bucket
//   new:     rs_seg_hist (u16 aux, one digit) + the same aux pass (its shrunk store would save 1 of its 20 bytes: not
//            modelled) + rs_seg_hist (u32 key, four digits, per cell) + three key passes, 9-byte records (u8 aux), per cell
// The last pass (10 + 7 against 9 + 7 bytes) needs the flag / edge machinery and is left to the byte count.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../coffeedb_amd/csrc top_first_bench.hip -o top_first_bench
// run:   ./top_first_bench [log2 n = 30] [tops = 256] [rounds = 3] [uniform key bytes = 0]
#include "radix_sort.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace cdb;

__device__ __forceinline__ uint32_t mix(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
// sym64[256]: Zipf-64 by inverse CDF in 256 steps; symtop[4096]: Zipf over `tops` values in 4096 steps
__global__ void fill_kernel(uint32_t* k, uint32_t* v, uint16_t* w, uint64_t n, const uint8_t* sym64, const uint8_t* symtop, int uniform) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = mix((uint32_t)i * 2654435761u + 12345u), h2 = mix(h + 0x9e3779b9u);
    k[i] = (uint32_t)sym64[h & 255u] | (uint32_t)sym64[(h >> 8) & 255u] << 8 | (uint32_t)sym64[(h >> 16) & 255u] << 16 | (uint32_t)sym64[h >> 24] << 24;
    if (uniform) k[i] = h;
    v[i] = (uint32_t)i;
    w[i] = (uint16_t)(symtop[h2 & 4095u] | ((h2 >> 12) & 0xFFu) << 8);
}
__global__ void shrink_kernel(const uint16_t* w, uint8_t* w8, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w8[i] = (uint8_t)(w[i] >> 8);
}
// after `bits` low key bits were sorted inside every segment: out[0] = inversions, out[1] = aux words that lost their record
__global__ void check_kernel(const uint32_t* k, const uint32_t* v, const uint8_t* w8, const uint16_t* w16, const SegInfo* segs, uint32_t nseg,
                             uint64_t n, uint32_t kmask, unsigned long long* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t lo = 0, hi = nseg - 1;  // segment of i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (segs[mid].begin <= i) lo = mid; else hi = mid - 1;
    }
    if (i + 1 < segs[lo].end) {
        const uint32_t a = k[i] & kmask, b = k[i + 1] & kmask;
        if (a > b || (a == b && w16 == nullptr && v[i] > v[i + 1])) atomicAdd(&out[0], 1ull);
    }
    const uint32_t h2 = mix(mix(v[i] * 2654435761u + 12345u) + 0x9e3779b9u);
    const uint32_t hb = (h2 >> 12) & 0xFFu;
    if ((w8 ? (uint32_t)w8[i] : (uint32_t)(w16[i] >> 8)) != hb) atomicAdd(&out[1], 1ull);
}

static std::vector<uint8_t> zipf_table(int values, int steps) {
    double h = 0;
    for (int r = 1; r <= values; ++r) h += 1.0 / r;
    std::vector<uint8_t> t(steps);
    double acc = 0;
    int pos = 0;
    for (int r = 1; r <= values; ++r) {
        acc += 1.0 / r / h;
        const int upto = r == values ? steps : std::max(pos + 1, (int)std::lround(acc * steps));
        for (; pos < upto && pos < steps; ++pos) t[pos] = (uint8_t)((r * 37) & 255);  // (spread over the byte range; 37 is odd: distinct)
    }
    return t;
}

struct Segs {
    std::vector<SegInfo> h;
    uint32_t tiles = 0;
    SegInfo* d = nullptr;
    uint32_t* tile_seg = nullptr;
    unsigned long long *hist = nullptr, *starts = nullptr;
    void upload(hipStream_t s) {
        const uint32_t nseg = (uint32_t)h.size();
        CDB_HIP(hipMalloc(&d, nseg * sizeof(SegInfo)));
        CDB_HIP(hipMalloc(&tile_seg, (size_t)tiles * 4));
        CDB_HIP(hipMalloc(&hist, (size_t)nseg * 8 * 256 * 8));
        CDB_HIP(hipMalloc(&starts, (size_t)nseg * 8 * 256 * 8));
        CDB_HIP(hipMemcpy(d, h.data(), nseg * sizeof(SegInfo), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(rs_seg_tilemap_kernel, dim3((unsigned)ceil_div(tiles, 256u)), dim3(256), 0, s, d, nseg, tiles, tile_seg);
    }
    void add(uint64_t b, uint64_t e) {
        h.push_back(SegInfo{b, e, tiles, 0u, 0ull, 0ull});
        tiles += (uint32_t)ceil_div(e - b, (uint64_t)RS_SEG_TILE);
    }
    void release() { CDB_HIP(hipFree(d)); CDB_HIP(hipFree(tile_seg)); CDB_HIP(hipFree(hist)); CDB_HIP(hipFree(starts)); }
};

int main(int argc, char** argv) {
    const int lg = argc > 1 ? std::atoi(argv[1]) : 30;
    const int tops = argc > 2 ? std::atoi(argv[2]) : 256;
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 3;
    const int uniform = argc > 4 ? std::atoi(argv[4]) : 0;  // 1: uniform key bytes (bit windows of a code stream) instead of Zipf-64 ones
    if (lg < 20 || lg > 31) { std::printf("log2 n: 20..31 (one thread per record: a grid of 2^32 threads does not launch)\n"); return 1; }
    const uint64_t n = 1ull << lg;
    const uint32_t nb = 64;
    hipStream_t s;
    CDB_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    StreamScope sscope(s);
    uint32_t *k[2], *v[2];
    uint16_t* w[2];
    for (int i = 0; i < 2; ++i) {
        CDB_HIP(hipMalloc(&k[i], n * 4 + 256));
        CDB_HIP(hipMalloc(&v[i], n * 4 + 256));
        CDB_HIP(hipMalloc(&w[i], n * 2 + 256));
    }
    uint8_t* w8[2] = {reinterpret_cast<uint8_t*>(w[0]), reinterpret_cast<uint8_t*>(w[1])};
    unsigned long long* d_out;
    CDB_HIP(hipMalloc(&d_out, 4 * 8));
    uint8_t *d_sym64, *d_symtop;
    {
        const std::vector<uint8_t> a = zipf_table(64, 256), b = zipf_table(tops, 4096);
        CDB_HIP(hipMalloc(&d_sym64, 256));
        CDB_HIP(hipMalloc(&d_symtop, 4096));
        CDB_HIP(hipMemcpy(d_sym64, a.data(), 256, hipMemcpyHostToDevice));
        CDB_HIP(hipMemcpy(d_symtop, b.data(), 4096, hipMemcpyHostToDevice));
    }
    if (!rs_atomic_rank_ok(s)) { std::printf("one-atomic ranking self-test FAILED on this device\n"); return 1; }
    Profiler prof;
    prof.enabled = true;
    RadixWorkspace ws;
    ws.allow_group = true;

    Segs bk;  // the buckets: Zipf-64 sizes
    {
        double hsum = 0;
        for (uint32_t g = 0; g < nb; ++g) hsum += 1.0 / (g + 1);
        uint64_t b = 0;
        for (uint32_t g = 0; g < nb; ++g) {
            const uint64_t e = g + 1 == nb ? n : std::min<uint64_t>(n, b + (uint64_t)((double)n / (g + 1) / hsum));
            bk.add(b, e);
            b = e;
        }
        bk.upload(s);
    }
    auto seg_args = [&](const Segs& sg) {
        SegArgs sa;
        sa.tile_seg = sg.tile_seg; sa.segs = sg.d; sa.tiles = sg.tiles; sa.start_stride = 8 * 256;
        return sa;
    };
    auto fill = [&]() {
        hipLaunchKernelGGL(fill_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, k[0], v[0], w[0], n, (const uint8_t*)d_sym64, (const uint8_t*)d_symtop, uniform);
    };
    auto hist_grid = [](uint32_t tiles) { return dim3((unsigned)ceil_div(tiles, (uint32_t)RS_MSD_HIST_TILES)); };
    auto check = [&](const Segs& sg, int cur, bool is8, uint32_t kmask, const char* what) {
        unsigned long long out[4];
        CDB_HIP(hipMemsetAsync(d_out, 0, 4 * 8, s));
        hipLaunchKernelGGL(check_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, (const uint32_t*)k[cur], (const uint32_t*)v[cur],
                           is8 ? (const uint8_t*)w8[cur] : (const uint8_t*)nullptr, is8 ? (const uint16_t*)nullptr : (const uint16_t*)w[cur],
                           (const SegInfo*)sg.d, (uint32_t)sg.h.size(), n, kmask, d_out);
        CDB_HIP(hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, s));
        CDB_HIP(hipStreamSynchronize(s));
        std::printf("  check %-8s %s (inversions %llu, strayed aux %llu)\n", what, out[0] == 0 && out[1] == 0 ? "ok" : "WRONG", out[0], out[1]);
    };
    std::map<std::string, double> best;
    auto take = [&](bool keep) {
        CDB_HIP(hipStreamSynchronize(s));
        radix_check_error(s, ws);
        prof.resolve();
        if (keep)
            for (auto& kv : prof.recs) {
                const double ms = kv.second.ms / (double)kv.second.launches;
                auto it = best.find(kv.first);
                if (it == best.end() || ms < it->second) best[kv.first] = ms;
            }
        prof.reset();
    };

    // ---- present form: five-digit histogram, aux pass, three key passes over the buckets (10-byte records)
    ws.prepare((uint64_t)bk.tiles * RS_SEG_TILE, RS_SEG_TILE, s);
    for (int r = 0; r <= rounds; ++r) {
        fill();
        CDB_HIP(hipMemsetAsync(bk.hist, 0, (size_t)nb * 8 * 256 * 8, s));
        int t = prof.begin(s);
        hipLaunchKernelGGL((rs_seg_hist_kernel<uint16_t>), hist_grid(bk.tiles), dim3(1024), 0, s, (const uint32_t*)k[0], (const uint16_t*)w[0], 1, 5,
                           (const uint32_t*)bk.tile_seg, (const SegInfo*)bk.d, bk.tiles, bk.hist);
        prof.end(t, "now  hist 6 B, 5 atomics", 0, s);
        hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nb), dim3(256), 0, s, (const unsigned long long*)bk.hist, (const SegInfo*)bk.d, 5, bk.starts);
        const SegArgs sa = seg_args(bk);
        int cur = 0;
        for (int p = 0; p < 4; ++p) {
            t = prof.begin(s);
            rs_launch_pass_ordered<RsBig<>, uint16_t>(s, ws, bk.tiles, k[cur], k[cur ^ 1], v[cur], v[cur ^ 1], n, 8 * (p - 1), 0xFFu,
                                                      (const unsigned long long*)(bk.starts + (size_t)p * 256), NoGen(), w[cur], w[cur ^ 1],
                                                      p == 0 ? 0 : -1, sa);
            prof.end(t, p == 0 ? "now  aux pass, 10 B records, buckets" : "now  key pass, 10 B records, buckets", 0, s);
            cur ^= 1;
        }
        take(r > 0);
        if (r == 0) check(bk, cur, false, 0x00FFFFFFu, "present");
    }

    // ---- control: the same three key passes over the BUCKETS with the aux word shrunk to a byte — what the record width alone
    // buys, without the cells (not a sort anyone needs: the aux digit is dropped unsorted)
    for (int r = 0; r <= rounds; ++r) {
        fill();
        CDB_HIP(hipMemsetAsync(bk.hist, 0, (size_t)nb * 8 * 256 * 8, s));
        hipLaunchKernelGGL((rs_seg_hist_kernel<uint16_t>), hist_grid(bk.tiles), dim3(1024), 0, s, (const uint32_t*)k[0], (const uint16_t*)w[0], 1, 5,
                           (const uint32_t*)bk.tile_seg, (const SegInfo*)bk.d, bk.tiles, bk.hist);
        hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nb), dim3(256), 0, s, (const unsigned long long*)bk.hist, (const SegInfo*)bk.d, 5, bk.starts);
        hipLaunchKernelGGL(shrink_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, (const uint16_t*)w[0], w8[1], n);
        CDB_HIP(hipMemcpyAsync(w8[0], w8[1], n, hipMemcpyDeviceToDevice, s));
        const SegArgs sa = seg_args(bk);
        int cur = 0;
        for (int p = 0; p < 3; ++p) {
            int t = prof.begin(s);
            rs_launch_pass_ordered<RsBig<>, uint8_t>(s, ws, bk.tiles, k[cur], k[cur ^ 1], v[cur], v[cur ^ 1], n, 8 * p, 0xFFu,
                                                     (const unsigned long long*)(bk.starts + (size_t)(p + 1) * 256), NoGen(), w8[cur], w8[cur ^ 1], -1, sa);
            prof.end(t, "ctl  key pass, 9 B records, buckets", 0, s);
            cur ^= 1;
        }
        take(r > 0);
        if (r == 0) check(bk, cur, true, 0x00FFFFFFu, "control");
    }

    // ---- new form
    Segs cells;
    for (int r = 0; r <= rounds; ++r) {
        fill();
        CDB_HIP(hipMemsetAsync(bk.hist, 0, (size_t)nb * 8 * 256 * 8, s));
        int t = prof.begin(s);
        hipLaunchKernelGGL((rs_seg_hist_kernel<uint16_t, false>), hist_grid(bk.tiles), dim3(1024), 0, s, (const uint32_t*)k[0], (const uint16_t*)w[0], 1, 1,
                           (const uint32_t*)bk.tile_seg, (const SegInfo*)bk.d, bk.tiles, bk.hist);
        prof.end(t, "new  hist 2 B, 1 atomic, buckets", 0, s);
        hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nb), dim3(256), 0, s, (const unsigned long long*)bk.hist, (const SegInfo*)bk.d, 1, bk.starts);
        ws.prepare((uint64_t)bk.tiles * RS_SEG_TILE, RS_SEG_TILE, s);
        t = prof.begin(s);
        rs_launch_pass_ordered<RsBig<>, uint16_t>(s, ws, bk.tiles, k[0], k[1], v[0], v[1], n, -8, 0xFFu, (const unsigned long long*)bk.starts, NoGen(),
                                                  w[0], w[1], 0, seg_args(bk));
        prof.end(t, "new  top pass, 10 B records, buckets", 0, s);
        if (r == 0) {  // the cells: non-empty (bucket, top byte) pairs in order
            std::vector<unsigned long long> hh((size_t)nb * 8 * 256);
            CDB_HIP(hipMemcpyAsync(hh.data(), bk.hist, hh.size() * 8, hipMemcpyDeviceToHost, s));
            CDB_HIP(hipStreamSynchronize(s));
            uint64_t maxc = 0, ragged = 0;
            for (uint32_t g = 0; g < nb; ++g) {
                uint64_t b = bk.h[g].begin;
                for (int d = 0; d < 256; ++d) {
                    const uint64_t c = hh[((size_t)g * 8) * 256 + d];
                    if (!c) continue;
                    cells.add(b, b + c);
                    b += c;
                    maxc = std::max(maxc, c);
                }
                if (b != bk.h[g].end) { std::printf("histogram of bucket %u does not add up\n", g); return 1; }
            }
            ragged = (uint64_t)cells.tiles * RS_SEG_TILE - n;
            cells.upload(s);
            std::printf("%zu cells, %u tiles (buckets: %u), largest cell %llu records, padding %.2f %% of the records\n", cells.h.size(), cells.tiles,
                        bk.tiles, (unsigned long long)maxc, 100.0 * (double)ragged / (double)n);
        }
        hipLaunchKernelGGL(shrink_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, (const uint16_t*)w[1], w8[0], n);
        CDB_HIP(hipMemcpyAsync(w8[1], w8[0], n, hipMemcpyDeviceToDevice, s));
        const uint32_t nc = (uint32_t)cells.h.size();
        CDB_HIP(hipMemsetAsync(cells.hist, 0, (size_t)nc * 8 * 256 * 8, s));
        t = prof.begin(s);
        hipLaunchKernelGGL((rs_seg_hist_kernel<uint8_t>), hist_grid(cells.tiles), dim3(1024), 0, s, (const uint32_t*)k[1], (const uint8_t*)w8[1], 0, 4,
                           (const uint32_t*)cells.tile_seg, (const SegInfo*)cells.d, cells.tiles, cells.hist);
        prof.end(t, "new  hist 4 B, 4 atomics, cells", 0, s);
        t = prof.begin(s);
        hipLaunchKernelGGL(rs_seg_digit_start_kernel, dim3(nc), dim3(256), 0, s, (const unsigned long long*)cells.hist, (const SegInfo*)cells.d, 4,
                           cells.starts);
        prof.end(t, "new  digit starts, cells", 0, s);
        ws.prepare((uint64_t)cells.tiles * RS_SEG_TILE, RS_SEG_TILE, s);
        const SegArgs sa = seg_args(cells);
        int cur = 1;
        for (int p = 0; p < 3; ++p) {
            t = prof.begin(s);
            rs_launch_pass_ordered<RsBig<>, uint8_t>(s, ws, cells.tiles, k[cur], k[cur ^ 1], v[cur], v[cur ^ 1], n, 8 * p, 0xFFu,
                                                     (const unsigned long long*)(cells.starts + (size_t)p * 256), NoGen(), w8[cur], w8[cur ^ 1], -1, sa);
            prof.end(t, "new  key pass, 9 B records, cells", 0, s);
            cur ^= 1;
        }
        take(r > 0);
        if (r == 0) check(cells, cur, true, 0x00FFFFFFu, "new");
    }
    std::printf("n = 2^%d, %u buckets, %d top-byte values, %s key bytes; best of %d rounds, ms per launch (x %g for 2^33)\n", lg, nb, tops, uniform ? "uniform" : "Zipf-64", rounds, 8589934592.0 / (double)n);
    for (auto& kv : best) std::printf("  %-40s %8.3f ms  %7.2f B/record at 4.9 TB/s\n", kv.first.c_str(), kv.second, kv.second * 1e-3 * 4.9e12 / (double)n);
    const double now = best["now  hist 6 B, 5 atomics"] + best["now  aux pass, 10 B records, buckets"] + 3 * best["now  key pass, 10 B records, buckets"];
    const double nw = best["new  hist 2 B, 1 atomic, buckets"] + best["new  top pass, 10 B records, buckets"] + best["new  hist 4 B, 4 atomics, cells"] +
                      best["new  digit starts, cells"] + 3 * best["new  key pass, 9 B records, cells"];
    const double sc = 8589934592.0 / (double)n;
    std::printf("  present: hist + aux pass + 3 key passes = %.3f ms (%.1f ms at 2^33)\n", now, now * sc);
    std::printf("  new:     2 hists + top pass + starts + 3 key passes = %.3f ms (%.1f ms at 2^33)\n", nw, nw * sc);
    std::printf("  difference %.3f ms (%.1f ms at 2^33), last pass not included (10 + 7 against 9 + 7 bytes)\n", nw - now, (nw - now) * sc);
    return 0;
}
