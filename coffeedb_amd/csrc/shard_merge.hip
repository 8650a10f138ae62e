// shard_merge.hip — the merge of the shards' answers on the devices, and the cdb_comm_* half of the C ABI.
//
// Suffixes never cross document boundaries (reference src/index.h:61-65) and a result row belongs to exactly one
// document (src/index.cpp:317-321), so a column splits into document-aligned byte ranges with one independent
// suffix array per GPU.  Every shard answers the whole pattern batch for its documents; concatenating the rows of
// a pattern in shard order is already ascending in document index, so the merge is an all-gatherv plus a
// placement — no reduction:
//     1. all-gather of the per-pattern row counts (u32 x patterns),
//     2. one exclusive scan over the (shard, pattern) counts = where every shard's rows of every pattern sit in the
//        gathered stream, and the merged row_ptr,
//     3. all-gatherv of the (id, count) rows — grouped ncclBroadcast, one root per shard (xGMI is point to point
//        and every peer is one hop away: a direct exchange, not a ring),
//     4. a placement kernel moves the rows from shard-major to pattern-major order.
// Two ways in: cdb_shards_* (shards.hip) — ONE process owning G devices (what the CoffeeDB shim uses: database.cpp is a
// single process), one host thread per shard; cdb_comm_* (here) — one process per GPU (bench.py under torchrun), each rank
// merging its own shard.  Both run the same merge over RCCL (loaded at run time: single-GPU users need no RCCL);
// shards that share a device (tests on a one-GPU box) exchange through device-to-device copies instead, because
// RCCL refuses two ranks on one GPU.
#include "shard_merge.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>

#include "index_impl.h"
#include "scan.h"

using namespace cdb;

namespace {

// ---- RCCL, bound at run time ---------------------------------------------------------------------------------
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;

    static RcclApi& get() {
        static RcclApi api;
        static std::once_flag once;
        std::call_once(once, [] {
            // (a process that already loaded an RCCL — PyTorch bundles one — gets that one back by soname)
            for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (api.lib) break;
            }
            if (!api.lib) return;
            auto sym = [&](const char* n) { return dlsym(api.lib, n); };
            api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
            api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
            api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(sym("ncclCommInitAll"));
            api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
            api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
            api.Broadcast = reinterpret_cast<decltype(api.Broadcast)>(sym("ncclBroadcast"));
            api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
            api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
            api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
            if (!api.GetUniqueId || !api.CommInitRank || !api.CommInitAll || !api.CommDestroy || !api.AllGather || !api.Broadcast ||
                !api.GroupStart || !api.GroupEnd) {
                dlclose(api.lib);
                api.lib = nullptr;
            }
        });
        return api;
    }
    bool ok() const { return lib != nullptr; }
};

#define CDB_NCCL(expr)                                                                                    \
    do {                                                                                                  \
        ncclResult_t r_ = (expr);                                                                         \
        if (r_ != ncclSuccess) {                                                                          \
            const RcclApi& a_ = RcclApi::get();                                                           \
            throw ::cdb::DeviceError(std::string("HIP error in " #expr " (RCCL): ") +                           \
                               (a_.GetErrorString ? a_.GetErrorString(r_) : "unknown"));                  \
        }                                                                                                 \
    } while (0)

// ---- the two exchanges --------------------------------------------------------------------------------------------
// one RCCL communicator per rank (ranks may live in one process — cdb_shards — or in one process each — cdb_comm)
struct RcclTransport : Transport {
    int world;
    std::vector<ncclComm_t> comms;  // indexed by LOCAL rank slot
    std::vector<int> local_rank;    // global rank of every local slot
    explicit RcclTransport(int w) : world(w) {}
    ~RcclTransport() override {
        for (ncclComm_t c : comms)
            if (c) (void)RcclApi::get().CommDestroy(c);
    }
    ncclComm_t comm_of(int rank) const {
        for (size_t i = 0; i < local_rank.size(); ++i)
            if (local_rank[i] == rank) return comms[i];
        throw InternalError("internal: rank is not local to this communicator");
    }
    void all_gather(int rank, const void* send, void* recv, size_t bytes, hipStream_t s) override {
        CDB_NCCL(RcclApi::get().AllGather(send, recv, bytes, ncclUint8, comm_of(rank), s));
    }
    void all_gather_v(int rank, const void* send, void* recv, const uint64_t* cnt, const uint64_t* off, hipStream_t s) override {
        // all-gatherv = one broadcast per root inside a group (every rank knows every count, so empty roots are
        // skipped consistently)
        const RcclApi& a = RcclApi::get();
        ncclComm_t c = comm_of(rank);
        CDB_NCCL(a.GroupStart());
        for (int q = 0; q < world; ++q) {
            if (!cnt[q]) continue;
            char* dst = static_cast<char*>(recv) + off[q] * 8;
            ncclResult_t r = a.Broadcast(q == rank ? send : (const void*)dst, dst, cnt[q], ncclUint64, q, c, s);
            if (r != ncclSuccess) {
                (void)a.GroupEnd();
                CDB_NCCL(r);
            }
        }
        CDB_NCCL(a.GroupEnd());
    }
    const char* name() const override { return "rccl"; }
};

// shards of ONE process that share devices: a board of published buffers, device-to-device copies
struct LocalTransport : Transport {
    int world;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    std::vector<const void*> send;
    explicit LocalTransport(int w) : world(w), send(w, nullptr) {}
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t g = gen;
        if (++arrived == world) {
            arrived = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
    void exchange(int rank, const void* snd, void* recv, const uint64_t* bytes, const uint64_t* off_bytes, hipStream_t s) {
        CDB_HIP(hipStreamSynchronize(s));  // this rank's buffer is complete
        {
            std::lock_guard<std::mutex> g(mu);
            send[rank] = snd;
        }
        barrier();  // every buffer is published and complete
        for (int q = 0; q < world; ++q)
            if (bytes[q])
                CDB_HIP(hipMemcpyAsync(static_cast<char*>(recv) + off_bytes[q], send[q], bytes[q], hipMemcpyDeviceToDevice, s));
        CDB_HIP(hipStreamSynchronize(s));
        barrier();  // every rank has read every buffer: they may be reused
    }
    void all_gather(int rank, const void* snd, void* recv, size_t bytes, hipStream_t s) override {
        std::vector<uint64_t> b(world, bytes), o(world);
        for (int q = 0; q < world; ++q) o[q] = (uint64_t)q * bytes;
        exchange(rank, snd, recv, b.data(), o.data(), s);
    }
    void all_gather_v(int rank, const void* snd, void* recv, const uint64_t* cnt, const uint64_t* off, hipStream_t s) override {
        std::vector<uint64_t> b(world), o(world);
        for (int q = 0; q < world; ++q) {
            b[q] = cnt[q] * 8;
            o[q] = off[q] * 8;
        }
        exchange(rank, snd, recv, b.data(), o.data(), s);
    }
    const char* name() const override { return "device copies"; }
};

// ---- merge kernels ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sh_counts_kernel(const uint64_t* __restrict__ row_ptr, uint64_t npat, uint32_t* __restrict__ cnt) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < npat) cnt[j] = (uint32_t)(row_ptr[j + 1] - row_ptr[j]);
}
struct FlatCntIn {  // (shard, pattern) counts in shard-major order = the order of the gathered row stream
    const uint32_t* c;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return c[i]; }
};
struct FlatPtrOut {
    uint64_t* p;
    uint64_t n;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t in) const {
        p[i] = ex;
        if (i + 1 == n) p[n] = in;
    }
};
struct ColSumIn {  // rows of pattern j over all shards
    const uint32_t* c;
    uint64_t npat;
    int world;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const {
        uint64_t t = 0;
        for (int q = 0; q < world; ++q) t += c[(uint64_t)q * npat + j];
        return t;
    }
};
__global__ __launch_bounds__(64) void sh_rank_offsets_kernel(const uint64_t* __restrict__ flat_ptr, uint64_t npat, int world,
                                                             uint64_t* __restrict__ out /*[world + 1]*/) {
    for (int q = threadIdx.x; q <= world; q += 64) out[q] = flat_ptr[(uint64_t)q * npat];  // (any number of ranks)
}
// merged row i: its pattern (search in the merged row_ptr), then the shard whose rows of that pattern cover it
__global__ __launch_bounds__(256) void sh_place_kernel(const uint64_t* __restrict__ g_row_ptr, const uint32_t* __restrict__ all_cnt,
                                                       const uint64_t* __restrict__ flat_ptr, uint64_t npat, int world, uint64_t total,
                                                       const int64_t* __restrict__ in_ids, const int64_t* __restrict__ in_cnt,
                                                       int64_t* __restrict__ out_ids, int64_t* __restrict__ out_cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        uint64_t lo = 0, hi = npat - 1;  // largest j with g_row_ptr[j] <= i
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (g_row_ptr[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const uint64_t j = lo;
        uint64_t k = i - g_row_ptr[j];
        int q = 0;
        for (; q < world - 1; ++q) {
            const uint64_t c = all_cnt[(uint64_t)q * npat + j];
            if (k < c) break;
            k -= c;
        }
        const uint64_t src = flat_ptr[(uint64_t)q * npat + j] + k;
        out_ids[i] = in_ids[src];
        out_cnt[i] = in_cnt[src];
    }
}
// this rank's first row of every pattern in the merged row stream (the counts-only merge)
__global__ __launch_bounds__(256) void sh_base_kernel(const uint64_t* __restrict__ g_row_ptr, const uint32_t* __restrict__ all_cnt,
                                                      uint64_t npat, int rank, uint64_t* __restrict__ base) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= npat) return;
    uint64_t b = g_row_ptr[j];
    for (int q = 0; q < rank; ++q) b += all_cnt[(uint64_t)q * npat + j];
    base[j] = b;
}

// ---- the half both merges share -----------------------------------------------------------------------------------
// Collective.  Every rank's per-pattern row counts on every rank (mr.all_cnt, shard-major) and the merged row_ptr over them
// (mr.g_row_ptr), both queued on s.  False for the empty batch: row_ptr = {0} stands, the stream is idle and nothing was exchanged.
bool gather_counts(MergeRank& mr, const uint64_t* d_row_ptr, uint64_t npat, hipStream_t s) {
    const int G = mr.world;
    mr.g_row_ptr.ensure((npat + 1) * 8);
    if (npat == 0) {
        CDB_HIP(hipMemsetAsync(mr.g_row_ptr.p, 0, 8, s));
        CDB_HIP(hipStreamSynchronize(s));
        return false;
    }
    mr.cnt.ensure(npat * 4);
    mr.all_cnt.ensure((size_t)G * npat * 4);
    hipLaunchKernelGGL(sh_counts_kernel, dim3((unsigned)ceil_div(npat, 256)), dim3(256), 0, s, d_row_ptr, npat, mr.cnt.as<uint32_t>());
    mr.tr->all_gather(mr.rank, mr.cnt.p, mr.all_cnt.p, npat * 4, s);
    ColSumIn cin{mr.all_cnt.as<uint32_t>(), npat, G};
    scan_totals_device<uint64_t>(s, mr.partials, cin, npat, OpAdd{}, (uint64_t)0);
    scan_apply<uint64_t>(s, mr.partials, cin, npat, OpAdd{}, (uint64_t)0, FlatPtrOut{mr.g_row_ptr.as<uint64_t>(), npat});
    return true;
}

// Counts-only merge for host (or rank-local) consumers ("otherwise each GPU D2H's its slice"): the ranks
// exchange nothing but their per-pattern row counts; every rank learns the merged row_ptr and where ITS rows of every
// pattern start in the merged row stream.  No rank ever holds another rank's rows — at C4 (10^7 patterns x 8 shards)
// the full all-gatherv would put ~10^9 rows on every GPU.
void merge_counts_core(MergeRank& mr, const cdb_device_result& local, cdb_shard_slice& out) {
    CDB_HIP(hipSetDevice(mr.device));
    StreamScope ss(mr.stream);
    hipStream_t s = mr.stream;
    const uint64_t npat = local.npat;
    std::memset(&out, 0, sizeof(out));
    out.npat = npat;
    out.nrows_local = local.nrows;
    if (!gather_counts(mr, local.d_row_ptr, npat, s)) {
        out.d_row_ptr = mr.g_row_ptr.as<uint64_t>();
        return;
    }
    mr.flat_ptr.ensure(npat * 8);  // (here: this rank's row bases)
    hipLaunchKernelGGL(sh_base_kernel, dim3((unsigned)ceil_div(npat, 256)), dim3(256), 0, s, (const uint64_t*)mr.g_row_ptr.as<uint64_t>(),
                       (const uint32_t*)mr.all_cnt.as<uint32_t>(), npat, mr.rank, mr.flat_ptr.as<uint64_t>());
    uint64_t total = 0;
    CDB_HIP(hipMemcpyAsync(&total, mr.g_row_ptr.as<uint64_t>() + npat, 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipGetLastError());
    CDB_HIP(hipStreamSynchronize(s));
    out.nrows_total = total;
    out.d_row_ptr = mr.g_row_ptr.as<uint64_t>();
    out.d_row_base = mr.flat_ptr.as<uint64_t>();
}

template <typename F>
int guarded_on(MergeRank* mr, F&& f) {
    return guarded_call(mr->err_mu, mr->err, std::forward<F>(f));
}

}  // namespace

namespace cdb {

MergeRank::~MergeRank() {
    if (own_stream && stream) {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        for (DevBuf* b : {&cnt, &all_cnt, &flat_ptr, &g_row_ptr, &offs, &st_ids, &st_cnt, &out_ids, &out_cnt, &partials}) b->release();
        DevPool::get().retire_stream(stream);
        (void)hipStreamDestroy(stream);
    }
}

std::shared_ptr<Transport> make_group_transport(int G, const std::vector<int>& devices) {
    bool distinct = true;
    for (int i = 0; i < G; ++i)
        for (int j = 0; j < i; ++j)
            if (devices[i] == devices[j]) distinct = false;
    const char* force = std::getenv("CDB_SHARD_TRANSPORT");
    if (G > 1 && distinct && RcclApi::get().ok() && !(force && std::string(force) == "copy")) {
        auto tr = std::make_shared<RcclTransport>(G);
        tr->comms.assign(G, nullptr);
        CDB_NCCL(RcclApi::get().CommInitAll(tr->comms.data(), G, devices.data()));
        for (int i = 0; i < G; ++i) tr->local_rank.push_back(i);
        return tr;
    }
    return std::make_shared<LocalTransport>(G);
}

void merge_core(MergeRank& mr, const cdb_device_result& local, cdb_device_result& merged) {
    CDB_HIP(hipSetDevice(mr.device));
    StreamScope ss(mr.stream);
    hipStream_t s = mr.stream;
    const uint64_t npat = local.npat;
    const int G = mr.world;
    std::memset(&merged, 0, sizeof(merged));
    merged.npat = npat;
    if (!gather_counts(mr, local.d_row_ptr, npat, s)) {
        merged.d_row_ptr = mr.g_row_ptr.as<uint64_t>();
        return;
    }
    // where every (shard, pattern) group starts in the gathered stream
    mr.flat_ptr.ensure(((size_t)G * npat + 1) * 8);
    mr.offs.ensure((G + 2) * 8);
    FlatCntIn fin{mr.all_cnt.as<uint32_t>()};
    scan_totals_device<uint64_t>(s, mr.partials, fin, (uint64_t)G * npat, OpAdd{}, (uint64_t)0);
    scan_apply<uint64_t>(s, mr.partials, fin, (uint64_t)G * npat, OpAdd{}, (uint64_t)0, FlatPtrOut{mr.flat_ptr.as<uint64_t>(), (uint64_t)G * npat});
    hipLaunchKernelGGL(sh_rank_offsets_kernel, dim3(1), dim3(64), 0, s, (const uint64_t*)mr.flat_ptr.as<uint64_t>(), npat, G,
                       mr.offs.as<uint64_t>());
    std::vector<uint64_t> off(G + 1), cntv(G);
    CDB_HIP(hipMemcpyAsync(off.data(), mr.offs.p, (G + 1) * 8, hipMemcpyDeviceToHost, s));
    CDB_HIP(hipGetLastError());
    CDB_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < G; ++q) cntv[q] = off[q + 1] - off[q];
    const uint64_t total = off[G];
    if (cntv[mr.rank] != local.nrows) throw InternalError("internal: shard row count does not match its row_ptr");
    merged.nrows = total;
    merged.d_row_ptr = mr.g_row_ptr.as<uint64_t>();
    if (total == 0) return;
    mr.st_ids.ensure(total * 8);
    mr.st_cnt.ensure(total * 8);
    mr.out_ids.ensure(total * 8);
    mr.out_cnt.ensure(total * 8);
    mr.tr->all_gather_v(mr.rank, local.d_ids, mr.st_ids.p, cntv.data(), off.data(), s);
    mr.tr->all_gather_v(mr.rank, local.d_counts, mr.st_cnt.p, cntv.data(), off.data(), s);
    const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(total, 256), 1u << 20);
    hipLaunchKernelGGL(sh_place_kernel, dim3(grid), dim3(256), 0, s, (const uint64_t*)mr.g_row_ptr.as<uint64_t>(),
                       (const uint32_t*)mr.all_cnt.as<uint32_t>(), (const uint64_t*)mr.flat_ptr.as<uint64_t>(), npat, G, total,
                       (const int64_t*)mr.st_ids.as<int64_t>(), (const int64_t*)mr.st_cnt.as<int64_t>(), mr.out_ids.as<int64_t>(),
                       mr.out_cnt.as<int64_t>());
    CDB_HIP(hipGetLastError());
    CDB_HIP(hipStreamSynchronize(s));
    merged.d_ids = mr.out_ids.as<int64_t>();
    merged.d_counts = mr.out_cnt.as<int64_t>();
}

}  // namespace cdb

// =====================================================================================================================
// one process per GPU
// =====================================================================================================================
struct cdb_comm {
    MergeRank mr;
};

extern "C" {

int cdb_comm_unique_id(void* id128) {
    if (!id128) return CDB_E_INVALID;
    const RcclApi& a = RcclApi::get();
    if (!a.ok()) return CDB_E_DEVICE;
    ncclUniqueId id;
    if (a.GetUniqueId(&id) != ncclSuccess) return CDB_E_DEVICE;
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id128, &id, sizeof(id));
    return CDB_OK;
}

int cdb_comm_create(cdb_comm** out, const void* id128, int rank, int world, int device) {
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return CDB_E_INVALID;
    *out = nullptr;
    const RcclApi& a = RcclApi::get();
    if (!a.ok()) return CDB_E_DEVICE;
    cdb_comm* c = new (std::nothrow) cdb_comm();
    if (!c) return CDB_E_DEVICE;
    try {
        if (device < 0) CDB_HIP(hipGetDevice(&device));
        CDB_HIP(hipSetDevice(device));
        c->mr.rank = rank;
        c->mr.world = world;
        c->mr.device = device;
        CDB_HIP(hipStreamCreateWithFlags(&c->mr.stream, hipStreamNonBlocking));
        c->mr.own_stream = true;
        auto tr = std::make_shared<RcclTransport>(world);
        ncclUniqueId id;
        std::memcpy(&id, id128, sizeof(id));
        ncclComm_t comm = nullptr;
        CDB_NCCL(a.CommInitRank(&comm, world, id, rank));
        tr->comms.push_back(comm);
        tr->local_rank.push_back(rank);
        c->mr.tr = tr;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cdb_comm_create: %s\n", e.what());
        delete c;
        return CDB_E_DEVICE;
    }
    *out = c;
    return CDB_OK;
}

// the ranks of ONE process: e.g. BASELINE config 3's four 8 GiB shards co-resident on one MI355X (tests/test_gpu_fullsize.py)
int cdb_comm_create_group(cdb_comm** out, int world, const int* devices) {
    if (!out || !devices || world < 1) return CDB_E_INVALID;
    for (int i = 0; i < world; ++i) out[i] = nullptr;
    try {
        std::shared_ptr<Transport> tr = make_group_transport(world, std::vector<int>(devices, devices + world));
        for (int i = 0; i < world; ++i) {
            cdb_comm* c = new cdb_comm();
            out[i] = c;
            c->mr.rank = i;
            c->mr.world = world;
            c->mr.device = devices[i];
            c->mr.tr = tr;
            CDB_HIP(hipSetDevice(devices[i]));
            CDB_HIP(hipStreamCreateWithFlags(&c->mr.stream, hipStreamNonBlocking));
            c->mr.own_stream = true;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cdb_comm_create_group: %s\n", e.what());
        for (int i = 0; i < world; ++i) {
            delete out[i];
            out[i] = nullptr;
        }
        return CDB_E_DEVICE;
    }
    return CDB_OK;
}

void cdb_comm_destroy(cdb_comm* c) { delete c; }

const char* cdb_comm_last_error(const cdb_comm* c) {
    static thread_local std::string copy;
    return c ? last_error_copy(c->mr.err_mu, c->mr.err, copy) : "null handle";
}

int cdb_comm_merge(cdb_comm* c, const cdb_device_result* local, cdb_device_result* merged) {
    if (!c || !local || !merged) return CDB_E_INVALID;
    return guarded_on(&c->mr, [&] { merge_core(c->mr, *local, *merged); });
}

int cdb_comm_merge_counts(cdb_comm* c, const cdb_device_result* local, cdb_shard_slice* out) {
    if (!c || !local || !out) return CDB_E_INVALID;
    return guarded_on(&c->mr, [&] { merge_counts_core(c->mr, *local, *out); });
}

int cdb_comm_world(const cdb_comm* c) { return c ? c->mr.world : 0; }
const char* cdb_comm_transport(const cdb_comm* c) { return (c && c->mr.tr) ? c->mr.tr->name() : "none"; }

}  // extern "C"
