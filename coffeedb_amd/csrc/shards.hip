// shards.hip — the string index across several GPUs behind the C ABI: cdb_shards_*, ONE process owning G devices
// (what the CoffeeDB shim uses: database.cpp is a single process), one host thread per shard.
//
// This unit is orchestration only: which shard handles exist (generations), who may touch them (locks), and fanning a call out over
// the shards and joining the parts on the host.  What every shard holds is decided in shard_plan.h (plain host arithmetic); the merge
// of the shards' answers on the devices, its kernels and the cdb_comm_* entry points live in shard_merge.hip.
//
// Locking: `state` guards WHICH shard handles exist — builds and loads replace them under the exclusive
// lock, every query holds it shared for the whole call, so a query never sees a destroyed handle or a half-built set.
// Device work of one shard is serialised by that shard's own ix.mu; code that holds several of them at once (the
// lone-keyword fan-out, the device merge) takes them in ascending shard order.  Writers of the staged column or of what the shards
// hold take staging_mu first.  Lock order everywhere: staging_mu, then state, then the shards' ix.mu in ascending order.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <shared_mutex>
#include <thread>

#include "../../include/coffeedb_gpu.h"
#include "cluster_merge.h"
#include "host_io.h"
#include "shard_merge.h"
#include "shard_plan.h"

using namespace cdb;

// Shared / exclusive lock that PREFERS the writer: glibc's rwlock lets new readers in while a writer waits, so
// two client threads with overlapping queries could keep a finished build from ever taking over.  Here a waiting writer
// closes the door for new readers; the ones inside finish, the generation swap runs, the door opens.  (No thread takes
// the shared side twice: nothing below nests two shared sections.)
class StateLock {
    std::mutex m;
    std::condition_variable cv;
    int readers = 0, writers_waiting = 0;
    bool writer = false;

public:
    void lock_shared() {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !writer && writers_waiting == 0; });
        ++readers;
    }
    void unlock_shared() {
        std::unique_lock<std::mutex> l(m);
        if (--readers == 0) cv.notify_all();
    }
    void lock() {
        std::unique_lock<std::mutex> l(m);
        ++writers_waiting;
        cv.wait(l, [&] { return !writer && readers == 0; });
        --writers_waiting;
        writer = true;
    }
    void unlock() {
        std::unique_lock<std::mutex> l(m);
        writer = false;
        cv.notify_all();
    }
};

// One generation of shards: the handles, which of them hold documents, and the merge state over those.  It owns all of it and lets
// go in the only correct order — the merge ranks borrow their handles' streams, so they go before the handles.
struct Generation {
    std::vector<cdb_index*> shard;                  // one handle per device slot (cdb_shards_append: the slots it opens)
    int used = 0;                                   // shards holding documents
    std::vector<uint64_t> bounds{0};                // docs [bounds[i], bounds[i+1]) live on shard i
    std::vector<std::unique_ptr<MergeRank>> ranks;  // merge state of the shards in use
    std::shared_ptr<Transport> tr;
    size_t options_seen = 0;                        // how many of cdb_shards::options the handles carry (install replays the rest)
    Generation() = default;
    Generation(Generation&& o) noexcept { swap(o); }  // (and so no copies)
    ~Generation() {
        ranks.clear();
        tr.reset();
        for (cdb_index* p : shard) cdb_destroy(p);
    }
    void swap(Generation& o) noexcept {
        shard.swap(o.shard);
        std::swap(used, o.used);
        bounds.swap(o.bounds);
        ranks.swap(o.ranks);
        tr.swap(o.tr);
        std::swap(options_seen, o.options_seen);
    }
};

struct cdb_shards {
    std::vector<int> devices;
    Generation gen;  // the serving generation
    // host staging of the whole column (cdb_shards_add*): the ONE host copy — builds upload views of it (cdb_build_view)
    std::vector<int64_t> ids;
    std::vector<uint64_t> doc_start{0};
    std::string text;
    bool staging_valid = true;               // false after cdb_shards_load until the column is fetched back from the shards
    uint64_t max_shard_bytes = 12ull << 30;  // a shard beyond this is split although fewer devices would do
    bool use_all = false;                    // always spread over every device (bench / tests)
    bool device_merge = false;               // cdb_shards_query_batch merges on the devices (RCCL all-gatherv) instead of the host
    bool replace_in_place = false;           // build: destroy the serving shards FIRST (a column whose old + new arrays do not
                                             // fit together; the reference keeps both, database.cpp:276-280)
    std::vector<std::pair<std::string, int64_t>> options;  // guarded by opt_mu
    std::mutex opt_mu;
    StateLock state;
    std::mutex staging_mu;                   // add* / build read and write the staged column
    mutable std::mutex err_mu;
    std::string err;
};

namespace {

template <typename F>
int guarded_on(cdb_shards* h, F&& f) {
    return guarded_call(h->err_mu, h->err, std::forward<F>(f));
}

// runs f(i) for i in [0, n) on n host threads (each shard has its own device, stream and locks); rethrows the first error
template <typename F>
void parallel_shards(int n, F&& f) {
    if (n == 1) {
        f(0);
        return;
    }
    std::vector<std::thread> th;
    std::mutex emu;
    std::exception_ptr first;
    for (int i = 0; i < n; ++i)
        th.emplace_back([&, i] {
            try {
                f(i);
            } catch (...) {
                std::lock_guard<std::mutex> g(emu);
                if (!first) first = std::current_exception();
            }
        });
    for (auto& t : th) t.join();
    if (first) std::rethrow_exception(first);
}

// a shard's failure becomes this call's: same code, same text
void check_handle(cdb_index* p, int rc) {
    if (rc != CDB_OK) throw Error((Status)rc, cdb_last_error(p));
}
void check_shard(cdb_shards* h, int i, int rc) { check_handle(h->gen.shard[i], rc); }

// G partial results, one per shard, zero-initialised; every one is freed by `free_one` when the scope ends
template <typename T>
struct Parts {
    std::vector<T> v;
    void (*free_one)(T*);
    Parts(int G, void (*f)(T*)) : v(G), free_one(f) {}
    ~Parts() { for (T& x : v) free_one(&x); }
    T& operator[](int i) { return v[i]; }
    const T& operator[](int i) const { return v[i]; }
    int size() const { return (int)v.size(); }
};

// `count` fresh handles on the device slots from `first` on, carrying the options set so far: the one place that makes a shard handle
// after cdb_shards_create.  They are g's at once, so a failure half way lets go of them with g.
void open_handles(cdb_shards* h, int first, int count, Generation& g) {
    std::vector<std::pair<std::string, int64_t>> options;
    {
        std::lock_guard<std::mutex> lk(h->opt_mu);
        options = h->options;  // snapshot: cdb_shards_set_option may append while a build runs (install() replays the rest)
    }
    g.options_seen = options.size();
    for (int i = 0; i < count; ++i) {
        cdb_index* p = nullptr;
        if (cdb_create(&p, h->devices[first + i]) != CDB_OK) throw DeviceError("HIP error: cannot create a shard handle");
        g.shard.push_back(p);
        for (auto& kv : options) (void)cdb_set_option(p, kv.first.c_str(), kv.second);
    }
}

// g's merge ranks and their transport for the first G handles of `shard` (more than one: a lone shard merges nothing)
void make_merge(const std::vector<int>& devices, const std::vector<cdb_index*>& shard, int G, Generation& g) {
    if (G <= 1) return;
    g.tr = make_group_transport(G, devices);
    for (int i = 0; i < G; ++i) {
        auto mr = std::make_unique<MergeRank>();
        mr->rank = i;
        mr->world = G;
        mr->device = devices[i];
        mr->stream = shard[i]->ix.stream;  // the shard's own stream: its query results are complete in stream order
        mr->tr = g.tr;
        g.ranks.push_back(std::move(mr));
    }
}

// A new generation built BESIDE the serving one: fresh handles on every device slot, build_shard(handle, i) for the first `used` of
// them on a host thread each, then the merge state.  Any failure lets go of all of it (~Generation) and the serving generation, its
// bounds and the staging never knew.
template <typename F>
Generation build_generation(cdb_shards* h, int used, const std::vector<uint64_t>& bounds, F&& build_shard) {
    Generation g;
    open_handles(h, 0, (int)h->devices.size(), g);
    g.used = used;
    g.bounds = bounds;
    parallel_shards(used, [&](int i) { build_shard(g.shard[i], i); });
    make_merge(h->devices, g.shard, used, g);
    return g;
}

// `next` takes over (exclusive lock held by the caller); the generation that served is destroyed on the way out, under that lock
void install(cdb_shards* h, Generation next) {
    {   // options set while this generation was being built reached the OLD handles only: replay them on the new ones
        std::lock_guard<std::mutex> g(h->opt_mu);
        for (size_t k = next.options_seen; k < h->options.size(); ++k)
            for (cdb_index* p : next.shard) (void)cdb_set_option(p, h->options[k].first.c_str(), h->options[k].second);
    }
    h->gen.swap(next);
}

// the column back on the host after cdb_shards_load (the shards hold it on their devices)
void fetch_staging(cdb_shards* h) {
    if (h->staging_valid) return;
    std::vector<int64_t> ids;
    std::vector<uint64_t> ds{0};
    std::string text;
    for (int i = 0; i < h->gen.used; ++i) {
        Index& ix = h->gen.shard[i]->ix;
        ensure_host_staging(ix);
        ids.insert(ids.end(), ix.ids.begin(), ix.ids.end());
        const uint64_t base = text.size();
        text.append(ix.host_text);
        for (size_t d = 1; d < ix.doc_start.size(); ++d) ds.push_back(base + ix.doc_start[d]);
        std::string().swap(ix.host_text);  // (one host copy: the shard keeps its device copy)
        ix.host_text_valid = false;
    }
    h->ids.swap(ids);
    h->doc_start.swap(ds);
    h->text.swap(text);
    h->staging_valid = true;
}
void drop_staging(cdb_shards* h) {  // the column lives on the devices (fetch_staging brings it back on demand)
    h->ids.clear();
    h->doc_start.assign(1, 0);
    std::string().swap(h->text);
    h->staging_valid = false;
}
// The staged column, held still and complete, for as long as the scope lives: staging_mu, then — state shared, let go again at once —
// the column fetched back from the shards if a load or a writer left it there.
struct StagedColumn {
    std::lock_guard<std::mutex> held;
    explicit StagedColumn(cdb_shards* h) : held(h->staging_mu) {
        std::shared_lock<StateLock> st(h->state);
        fetch_staging(h);
    }
};

// f(t, j0, j1) over [0, n) split into contiguous ranges, on up to T host threads (small n: one)
template <typename F>
void parallel_ranges(uint64_t n, int T, F&& f) {
    T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)T, n >> 16));
    if (T == 1) {
        f(0, (uint64_t)0, n);
        return;
    }
    parallel_shards(T, [&](int t) { f(t, n * t / T, n * (t + 1) / T); });
}

int out_rows(const std::vector<std::pair<int64_t, int64_t>>& rows, int64_t** ids, int64_t** counts, size_t* nrows) {
    int64_t* oi = (int64_t*)std::malloc(std::max<size_t>(rows.size(), 1) * 8);
    int64_t* oc = (int64_t*)std::malloc(std::max<size_t>(rows.size(), 1) * 8);
    if (!oi || !oc) {
        std::free(oi);
        std::free(oc);
        throw std::bad_alloc();
    }
    for (size_t r = 0; r < rows.size(); ++r) {
        oi[r] = rows[r].first;
        oc[r] = rows[r].second;
    }
    *ids = oi;
    *counts = oc;
    *nrows = rows.size();
    return 0;
}

}  // namespace

extern "C" {

int cdb_shards_create(cdb_shards** out, const int* devices, int ndev) {
    if (!out || ndev < 1 || !devices) return CDB_E_INVALID;
    *out = nullptr;
    cdb_shards* h = new (std::nothrow) cdb_shards();
    if (!h) return CDB_E_DEVICE;
    for (int i = 0; i < ndev; ++i) {
        cdb_index* ix = nullptr;
        const int rc = cdb_create(&ix, devices[i]);
        if (rc != CDB_OK) {
            delete h;
            return rc;
        }
        h->gen.shard.push_back(ix);
        h->devices.push_back(ix->ix.device);
    }
    *out = h;
    return CDB_OK;
}

void cdb_shards_destroy(cdb_shards* h) { delete h; }

const char* cdb_shards_last_error(const cdb_shards* h) {
    static thread_local std::string copy;
    return h ? last_error_copy(h->err_mu, h->err, copy) : "null handle";
}

int cdb_shards_add(cdb_shards* h, int64_t id, const char* value, size_t len) {
    if (!h || (!value && len)) return CDB_E_INVALID;
    return guarded_on(h, [&] {
        StagedColumn staged(h);
        h->text.append(value, len);
        h->ids.push_back(id);
        h->doc_start.push_back(h->text.size());
    });
}

int cdb_shards_add_bulk(cdb_shards* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs) {
    if (!h || (ndocs && (!ids || !doc_start))) return CDB_E_INVALID;
    return guarded_on(h, [&] {
        if (!ndocs) return;
        for (uint64_t d = 0; d < ndocs; ++d)
            if (doc_start[d + 1] < doc_start[d]) throw Error("doc_start must be non-decreasing");
        StagedColumn staged(h);
        h->ids.reserve(h->ids.size() + ndocs);
        h->doc_start.reserve(h->doc_start.size() + ndocs);
        const uint64_t base = h->text.size();
        h->text.append(blob + doc_start[0], doc_start[ndocs] - doc_start[0]);
        for (uint64_t d = 0; d < ndocs; ++d) {
            h->ids.push_back(ids[d]);
            h->doc_start.push_back(base + doc_start[d + 1] - doc_start[0]);
        }
    });
}

// raw-file ingest (database.cpp:170-275) into the sharded column: cdb_add_raw_dir's reader, all or nothing
int cdb_shards_add_raw_dir(cdb_shards* h, const char* dir, const char* key, uint64_t* records, uint64_t* added) {
    if (!h || !dir || !key) return CDB_E_INVALID;
    if (records) *records = 0;
    if (added) *added = 0;
    return guarded_on(h, [&] {
        StagedColumn staged(h);
        uint64_t nrec = 0, nadd = 0;
        read_raw_dir(dir, key, h->ids, h->doc_start, h->text, nrec, nadd);
        if (records) *records = nrec;
        if (added) *added = nadd;
    });
}

int cdb_shards_set_option(cdb_shards* h, const char* name, int64_t value) {
    if (!h || !name) return CDB_E_INVALID;
    if (!std::strcmp(name, "max_shard_bytes")) {
        h->max_shard_bytes = value > 0 ? (uint64_t)value : 1;
        return CDB_OK;
    }
    if (!std::strcmp(name, "use_all_devices")) {
        h->use_all = value != 0;
        return CDB_OK;
    }
    if (!std::strcmp(name, "device_merge")) {
        h->device_merge = value != 0;
        return CDB_OK;
    }
    if (!std::strcmp(name, "replace_in_place")) {
        h->replace_in_place = value != 0;
        return CDB_OK;
    }
    std::shared_lock<StateLock> st(h->state);
    for (cdb_index* p : h->gen.shard) {
        const int rc = cdb_set_option(p, name, value);
        if (rc != CDB_OK) {
            std::lock_guard<std::mutex> g(h->err_mu);
            h->err = cdb_last_error(p);
            return rc;
        }
    }
    {
        std::lock_guard<std::mutex> g(h->opt_mu);
        h->options.emplace_back(name, value);  // (replayed on the fresh handles of every rebuild)
    }
    return CDB_OK;
}

// index.cpp:178-236 over several GPUs.  Transactional: a NEW generation of shard handles is built beside
// the serving one — database.cpp:276-280 keeps the old index answering until the new one is complete — and takes over
// under the exclusive lock only when every shard succeeded; a failure leaves the old generation untouched.  The shards
// upload VIEWS of the one staged column (cdb_build_view): no second host copy per shard.
int cdb_shards_build(cdb_shards* h) {
    if (!h) return CDB_E_INVALID;
    return guarded_on(h, [&] {
        StagedColumn staged(h);  // (the column must not move while the shards upload it)
        const int G = (int)h->devices.size();
        const uint64_t nd = h->ids.size();
        const int used = shard_count(h->doc_start[nd], nd, G, h->max_shard_bytes, h->use_all);
        const std::vector<uint64_t> b = shard_bounds(h->doc_start, used);
        if (h->replace_in_place) {  // the caller accepts an unbuilt window: the old arrays go first — an empty generation takes over
            std::unique_lock<StateLock> st(h->state);
            Generation empty;
            open_handles(h, 0, G, empty);
            install(h, std::move(empty));
        }
        Generation g = build_generation(h, used, b, [&](cdb_index* p, int i) {
            const uint64_t d0 = b[i], d1 = b[i + 1];
            check_handle(p, cdb_build_view(p, h->ids.data() + d0, h->text.data(), h->doc_start.data() + d0, d1 - d0));
        });
        std::unique_lock<StateLock> st(h->state);
        install(h, std::move(g));
    });
}

namespace {
// The same from the caller's own strings (string_index's views): nothing is staged in the handle, every shard gathers its
// documents straight into its pinned upload chunks.  A later cdb_shards_add fetches the column back from the shards.
// With h->staging_mu held (cdb_shards_append to a set that was never built is this build).
void build_views_locked(cdb_shards* h, const int64_t* ids, const char* const* ptrs, const uint64_t* lens, uint64_t ndocs) {
    std::vector<uint64_t> ds(ndocs + 1, 0);
    for (uint64_t d = 0; d < ndocs; ++d) ds[d + 1] = ds[d] + lens[d];
    const int used = shard_count(ds[ndocs], ndocs, (int)h->devices.size(), h->max_shard_bytes, h->use_all);
    const std::vector<uint64_t> b = shard_bounds(ds, used);
    Generation g = build_generation(h, used, b, [&](cdb_index* p, int i) {
        const uint64_t d0 = b[i], d1 = b[i + 1];
        check_handle(p, cdb_build_views(p, ids + d0, ptrs + d0, lens + d0, d1 - d0));
    });
    std::unique_lock<StateLock> st(h->state);
    install(h, std::move(g));
    drop_staging(h);  // (the column lives on the devices and with the caller)
}
constexpr uint64_t SHARDS_MAGIC = 0x3130485344424443ull;  // "CDBDSH01"
}  // namespace
int cdb_shards_build_views(cdb_shards* h, const int64_t* ids, const char* const* ptrs, const uint64_t* lens, uint64_t ndocs) {
    if (!h || (ndocs && (!ids || !ptrs || !lens))) return CDB_E_INVALID;
    return guarded_on(h, [&] {
        std::lock_guard<std::mutex> sg(h->staging_mu);
        build_views_locked(h, ids, ptrs, lens, ndocs);
    });
}

// f4 over shards: `path` holds the shard count and document bounds, `path.<i>` shard i's own file (cdb_save)
int cdb_shards_save(cdb_shards* h, const char* path) {
    if (!h || !path) return CDB_E_INVALID;
    return guarded_on(h, [&] {
        std::shared_lock<StateLock> st(h->state);
        const Generation& gen = h->gen;
        if (gen.used < 1) throw Error("index has not been built");
        for (int i = 0; i < gen.used; ++i) check_shard(h, i, cdb_save(gen.shard[i], (std::string(path) + "." + std::to_string(i)).c_str()));
        FILE* fp = std::fopen(path, "wb");
        if (!fp) throw Error(std::string("Cannot open file: ") + path);
        struct Closer { FILE* f; ~Closer() { std::fclose(f); } } closer{fp};
        const uint64_t hd[2] = {SHARDS_MAGIC, (uint64_t)gen.used};
        bool ok = std::fwrite(hd, 8, 2, fp) == 2;
        ok = ok && std::fwrite(gen.bounds.data(), 8, (size_t)gen.used + 1, fp) == (size_t)gen.used + 1;
        if (!ok) throw Error(std::string("Cannot write file: ") + path);
    });
}

int cdb_shards_load(cdb_shards* h, const char* path) {
    if (!h || !path) return CDB_E_INVALID;
    return guarded_on(h, [&] {
        std::lock_guard<std::mutex> sg(h->staging_mu);
        uint64_t hd[2] = {0, 0};
        std::vector<uint64_t> b;
        {
            FILE* fp = std::fopen(path, "rb");
            if (!fp) throw Error(std::string("Cannot open file: ") + path);
            struct Closer { FILE* f; ~Closer() { std::fclose(f); } } closer{fp};
            if (std::fread(hd, 8, 2, fp) != 2 || hd[0] != SHARDS_MAGIC || hd[1] < 1 || hd[1] > 4096)
                throw Error(std::string("Not a saved sharded index: ") + path);
            b.resize(hd[1] + 1);
            if (std::fread(b.data(), 8, b.size(), fp) != b.size()) throw Error(std::string("Truncated index file: ") + path);
        }
        const int used = (int)hd[1];
        if (used > (int)h->devices.size()) throw Error("saved index has more shards than this handle has devices");
        Generation g = build_generation(h, used, b, [&](cdb_index* p, int i) {
            check_handle(p, cdb_load(p, (std::string(path) + "." + std::to_string(i)).c_str()));
            if (p->ix.ndocs != b[i + 1] - b[i]) throw Error(std::string("Corrupt index file (shard bounds): ") + path);
        });
        std::unique_lock<StateLock> st(h->state);
        install(h, std::move(g));
        drop_staging(h);  // (fetched back by the next add / build)
    });
}

int cdb_shards_count(const cdb_shards* h) { return h ? h->gen.used : 0; }
cdb_index* cdb_shards_get(cdb_shards* h, int i) { return (h && i >= 0 && i < (int)h->gen.shard.size()) ? h->gen.shard[i] : nullptr; }
uint64_t cdb_shards_first_doc(const cdb_shards* h, int i) {
    return (h && i >= 0 && i < (int)h->gen.bounds.size()) ? h->gen.bounds[i] : 0;
}
const char* cdb_shards_transport(const cdb_shards* h) { return (h && h->gen.tr) ? h->gen.tr->name() : "none"; }

// One keyword (database.cpp:392): every shard's lone-keyword kernel is in flight before the first answer is awaited
// (one launch + one poll per shard instead of G complete round trips); shards in order = ascending document index.
int cdb_shards_query(cdb_shards* h, const char* keyword, size_t len, int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!h || !ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    return guarded_on(h, [&] {
        if (len == 0) throw Error("Empty keywords are not allowed");  // index.cpp:239-241
        std::shared_lock<StateLock> st(h->state);
        const std::vector<cdb_index*>& shard = h->gen.shard;
        const int G = std::max(h->gen.used, 1);
        struct Part {
            int64_t *ids = nullptr, *counts = nullptr;
            size_t n = 0;
            SingleLaunch state = SingleLaunch::NotApplicable;
        };
        Parts<Part> part(G, +[](Part* x) { cdb_free(x->ids); cdb_free(x->counts); });
        {
            std::vector<std::unique_lock<std::mutex>> locks;  // ascending shard order
            std::vector<char> in_flight(G, 0);                // launched, answer not collected yet
            try {
                for (int i = 0; i < G; ++i) {
                    Index& ix = shard[i]->ix;
                    locks.emplace_back(ix.mu);
                    DeviceScope scope(ix);
                    part[i].state = query_single_launch(ix, keyword, len);
                    in_flight[i] = part[i].state == SingleLaunch::Launched;
                }
                for (int i = 0; i < G; ++i) {
                    Index& ix = shard[i]->ix;
                    if (part[i].state == SingleLaunch::Absent) query_single_empty(ix, &part[i].ids, &part[i].counts, &part[i].n);
                    else if (part[i].state == SingleLaunch::Launched) {
                        DeviceScope scope(ix);
                        in_flight[i] = 0;  // (collect waits for the answer or throws after the stream was synchronised)
                        if (!query_single_collect(ix, &part[i].ids, &part[i].counts, &part[i].n)) part[i].state = SingleLaunch::NotApplicable;
                    }
                }
            } catch (...) {
                // kernels of the shards already launched would answer LATER into their host-mapped result blocks — over the
                // next query's "not answered yet" mark.  They finish (or the resident workgroup leaves) before the locks go.
                for (int i = 0; i < (int)locks.size(); ++i) {
                    Index& ix = shard[i]->ix;
                    (void)hipSetDevice(ix.device);
                    if (ix.resident_query) query_resident_stop(ix);
                    else if (in_flight[i]) (void)hipStreamSynchronize(ix.stream);
                }
                throw;
            }
        }
        std::vector<std::pair<int64_t, int64_t>> rows;
        for (int i = 0; i < G; ++i) {
            if (part[i].state == SingleLaunch::NotApplicable)  // long hit lists, options: the shard's ordinary path
                check_shard(h, i, cdb_query(shard[i], keyword, len, &part[i].ids, &part[i].counts, &part[i].n));
            for (size_t r = 0; r < part[i].n; ++r) rows.emplace_back(part[i].ids[r], part[i].counts[r]);
        }
        out_rows(rows, ids, counts, nrows);
    });
}

// The per-key operations work shard by shard: documents — hence object ids — are disjoint across shards, so the union over
// shards is a concatenation, ordered afterwards the way the single-GPU call orders it.  The shards work concurrently.
namespace {
void shards_or_rows(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, bool ranked, int64_t lo, int64_t hi,
                    uint64_t limit, std::vector<std::pair<int64_t, int64_t>>& rows) {
    std::shared_lock<StateLock> st(h->state);
    const int G = std::max(h->gen.used, 1);
    std::vector<std::vector<std::pair<int64_t, int64_t>>> part(G);
    parallel_shards(G, [&](int i) {
        int64_t *pi = nullptr, *pc = nullptr;
        size_t n = 0;
        // (every shard's own top `limit` rows contain its share of the global top `limit`)
        check_shard(h, i, ranked ? cdb_query_ranked(h->gen.shard[i], blob, offsets, nkw, lo, hi, limit, &pi, &pc, &n)
                                 : cdb_query_or(h->gen.shard[i], blob, offsets, nkw, &pi, &pc, &n));
        part[i].reserve(n);
        for (size_t r = 0; r < n; ++r) part[i].emplace_back(pi[r], pc[r]);
        cdb_free(pi);
        cdb_free(pc);
    });
    for (int i = 0; i < G; ++i) rows.insert(rows.end(), part[i].begin(), part[i].end());
    if (h->gen.used > 1) {
        if (ranked) {
            std::sort(rows.begin(), rows.end(), [](const auto& a, const auto& b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });
            if (limit && rows.size() > limit) rows.resize(limit);
        } else {
            std::sort(rows.begin(), rows.end());
        }
    }
}
int shards_or_impl(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, bool ranked, int64_t lo, int64_t hi,
                   uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!h || !ids || !counts || !nrows || (nkw && !offsets)) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    return guarded_on(h, [&] {
        std::vector<std::pair<int64_t, int64_t>> rows;
        shards_or_rows(h, blob, offsets, nkw, ranked, lo, hi, limit, rows);
        out_rows(rows, ids, counts, nrows);
    });
}
}  // namespace

int cdb_shards_query_or(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t** ids, int64_t** counts,
                        size_t* nrows) {
    return shards_or_impl(h, blob, offsets, nkw, false, 0, 0, 0, ids, counts, nrows);
}

int cdb_shards_query_ranked(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t corr_lo, int64_t corr_hi,
                            uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows) {
    return shards_or_impl(h, blob, offsets, nkw, true, corr_lo, corr_hi, limit, ids, counts, nrows);
}

// AND across keys (interface.cpp:114-146) when string keys are sharded columns.  Different columns are cut at different
// documents (the cut balances bytes), so the intersection cannot be taken shard by shard: every sharded key is resolved
// with its OR over its own shards (rows ascending by id), then all row lists meet in ONE device merge — the same
// and_merge_on_device as cdb_query_and — on the first shard of the first sharded key.
int cdb_shards_query_and(const cdb_shards_key_query* keys, int nkeys, int ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit,
                         int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!keys || nkeys < 1 || !ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    cdb_shards* lead = nullptr;
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].shards && !lead) lead = keys[k].shards;
    if (!lead) return CDB_E_INVALID;
    return guarded_on(lead, [&] {
        std::vector<std::vector<int64_t>> hi(nkeys), hc(nkeys);
        std::vector<cdb_key_query> flat(nkeys);
        for (int k = 0; k < nkeys; ++k) {
            const cdb_shards_key_query& q = keys[k];
            std::memset(&flat[k], 0, sizeof(cdb_key_query));
            if (q.shards) {
                check_keywords(KeywordList{q.blob, q.offsets, q.nkw}, "cdb_shards_query_and", KW_LIST_NOT_EMPTY | KW_OFFSETS | KW_NONE_EMPTY);
                std::vector<std::pair<int64_t, int64_t>> rows;
                shards_or_rows(q.shards, q.blob, q.offsets, q.nkw, false, 0, 0, 0, rows);
                hi[k].reserve(rows.size());
                hc[k].reserve(rows.size());
                for (auto& r : rows) {
                    hi[k].push_back(r.first);
                    hc[k].push_back(r.second);
                }
                flat[k].ids = hi[k].data();
                flat[k].counts = hc[k].data();
                flat[k].nrows = hi[k].size();
            } else {
                if (q.nrows && (!q.ids || !q.counts)) throw Error("cdb_shards_query_and: row list missing");
                flat[k].ids = q.ids;
                flat[k].counts = q.counts;
                flat[k].nrows = q.nrows;
            }
        }
        std::shared_lock<StateLock> st(lead->state);
        cdb_index* dev = lead->gen.shard[0];
        check_handle(dev, query_and_with_lead(dev, flat.data(), nkeys, ranked, corr_lo, corr_hi, limit, ids, counts, nrows));
    });
}

int cdb_shards_query_spans(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t nkw, cdb_spans* out) {
    if (!h || !out || (nkw && !offsets)) return CDB_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    const int rc = guarded_on(h, [&] {
        std::shared_lock<StateLock> st(h->state);
        Parts<cdb_spans> parts(std::max(h->gen.used, 1), cdb_spans_free);
        parallel_shards(parts.size(), [&](int i) { check_shard(h, i, cdb_query_spans(h->gen.shard[i], blob, offsets, nkw, &parts[i])); });
        uint64_t nd = 0, ns = 0;
        for (const cdb_spans& p : parts.v) {  // shard order = ascending document index
            nd += p.ndocs;
            ns += p.nspans;
        }
        out->ndocs = nd;
        out->nspans = ns;
        out->ids = (int64_t*)host_alloc(nd * 8);
        out->span_ptr = (uint64_t*)host_alloc((nd + 1) * 8, true);
        out->begin = (uint64_t*)host_alloc(ns * 8);
        out->end = (uint64_t*)host_alloc(ns * 8);
        uint64_t d0 = 0, s0 = 0;
        for (const cdb_spans& p : parts.v) {
            for (uint64_t d = 0; d < p.ndocs; ++d) {
                out->ids[d0 + d] = p.ids[d];
                out->span_ptr[d0 + d] = s0 + p.span_ptr[d];
            }
            if (p.nspans) {
                std::memcpy(out->begin + s0, p.begin, p.nspans * 8);
                std::memcpy(out->end + s0, p.end, p.nspans * 8);
            }
            d0 += p.ndocs;
            s0 += p.nspans;
        }
        out->span_ptr[nd] = ns;
    });
    if (rc != CDB_OK) cdb_spans_free(out);
    return rc;
}

// every shard renders the rows it holds (ids are disjoint across shards); the answers go back into the caller's row order
int cdb_shards_render_rows(cdb_shards* h, const int64_t* ids, uint64_t nrows, const char* blob, const uint64_t* offsets, uint64_t nkw, const char* left,
                           size_t left_len, const char* right, size_t right_len, int what, cdb_rendered* out) {
    if (!h || !out || (nrows && !ids) || (nkw && !offsets) || (left_len && !left) || (right_len && !right)) return CDB_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    const int rc = guarded_on(h, [&] {
        std::shared_lock<StateLock> st(h->state);
        Parts<cdb_rendered> parts(std::max(h->gen.used, 1), cdb_rendered_free);
        parallel_shards(parts.size(), [&](int i) {
            check_shard(h, i, cdb_render_rows(h->gen.shard[i], ids, nrows, blob, offsets, nkw, left, left_len, right, right_len, what, &parts[i]));
        });
        const bool want_text = (what & CDB_RENDER_TEXT) != 0, want_spans = (what & CDB_RENDER_SPANS) != 0;
        std::vector<int> owner(nrows, -1);  // the shard that holds row i
        uint64_t ns = 0, tb = 0;
        for (const cdb_rendered& p : parts.v) {
            ns += p.nspans;
            tb += p.text_bytes;
        }
        out->nrows = nrows;
        out->nspans = ns;
        out->text_bytes = tb;
        out->found = (uint8_t*)host_alloc(nrows, true);
        for (uint64_t i = 0; i < nrows; ++i) {
            for (int g = 0; g < parts.size() && owner[i] < 0; ++g)
                if (parts[g].found[i]) owner[i] = g;
            out->found[i] = owner[i] >= 0 ? 1 : 0;
            out->missing += owner[i] < 0 ? 1 : 0;
        }
        if (want_text) {
            out->text_ptr = (uint64_t*)host_alloc((nrows + 1) * 8, true);
            out->text_blob = (char*)host_alloc(tb);
            uint64_t o = 0;
            for (uint64_t i = 0; i < nrows; ++i) {
                out->text_ptr[i] = o;
                if (owner[i] < 0) continue;
                const cdb_rendered& p = parts[owner[i]];
                const uint64_t len = p.text_ptr[i + 1] - p.text_ptr[i];
                if (len) std::memcpy(out->text_blob + o, p.text_blob + p.text_ptr[i], len);
                o += len;
            }
            out->text_ptr[nrows] = o;
        }
        if (want_spans) {
            out->span_ptr = (uint64_t*)host_alloc((nrows + 1) * 8, true);
            out->begin = (uint64_t*)host_alloc(ns * 8);
            out->end = (uint64_t*)host_alloc(ns * 8);
            uint64_t o = 0;
            for (uint64_t i = 0; i < nrows; ++i) {
                out->span_ptr[i] = o;
                if (owner[i] < 0) continue;
                const cdb_rendered& p = parts[owner[i]];
                const uint64_t a = p.span_ptr[i], len = p.span_ptr[i + 1] - a;
                if (len) {
                    std::memcpy(out->begin + o, p.begin + a, len * 8);
                    std::memcpy(out->end + o, p.end + a, len * 8);
                }
                o += len;
            }
            out->span_ptr[nrows] = o;
        }
    });
    if (rc != CDB_OK) cdb_rendered_free(out);
    return rc;
}

namespace {
// Host merge of the shards' CSR answers (the consumer of the C ABI is the host: SURVEY §8e — every GPU hands over its own
// slice, nothing is replicated on the devices).  Every shard answers the whole batch through its own host entry point
// (patterns up and rows down over its own PCIe link, concurrently); the rows of a pattern are then the shards' rows in
// shard order.  The interleave runs over pattern ranges on several host threads.
void shards_batch_host(cdb_shards* h, int G, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out, cdb_hits* hits) {
    Parts<cdb_hits> hpart(G, cdb_hits_free);
    Parts<cdb_result> part(G, cdb_result_free);
    parallel_shards(G, [&](int i) {
        check_shard(h, i, hits ? cdb_query_batch_offsets(h->gen.shard[i], blob, offsets, npat, &part[i], &hpart[i])
                               : cdb_query_batch(h->gen.shard[i], blob, offsets, npat, &part[i]));
    });
    uint64_t nrows = 0, nhits = 0;
    for (int i = 0; i < G; ++i) {
        nrows += part[i].nrows;
        nhits += part[i].nhits;
    }
    out->npat = npat;
    out->nrows = nrows;
    out->nhits = nhits;
    out->row_ptr = (uint64_t*)host_alloc((npat + 1) * 8);
    out->ids = (int64_t*)host_alloc(nrows * 8);
    out->counts = (int64_t*)host_alloc(nrows * 8);
    if (hits) {
        hits->hit_ptr = (uint64_t*)host_alloc((nrows + 1) * 8);
        hits->offsets = (uint64_t*)host_alloc(nhits * 8);
    }
    // first row (and first hit) of every pattern range = the rows (hits) the shards hold in front of it
    const int T = std::max(G, 4);
    parallel_ranges(npat, T, [&](int, uint64_t j0, uint64_t j1) {
        uint64_t row = 0, hit = 0;
        for (int i = 0; i < G; ++i) {
            row += part[i].row_ptr[j0];
            if (hits) hit += hpart[i].hit_ptr[part[i].row_ptr[j0]];
        }
        for (uint64_t j = j0; j < j1; ++j) {
            out->row_ptr[j] = row;
            for (int i = 0; i < G; ++i) {
                const uint64_t a = part[i].row_ptr[j], b = part[i].row_ptr[j + 1];
                if (a == b) continue;
                std::memcpy(out->ids + row, part[i].ids + a, (b - a) * 8);
                std::memcpy(out->counts + row, part[i].counts + a, (b - a) * 8);
                if (hits) {
                    const uint64_t ha = hpart[i].hit_ptr[a], hb = hpart[i].hit_ptr[b];
                    for (uint64_t r = a; r < b; ++r) hits->hit_ptr[row + (r - a)] = hit + (hpart[i].hit_ptr[r] - ha);
                    std::memcpy(hits->offsets + hit, hpart[i].offsets + ha, (hb - ha) * 8);
                    hit += hb - ha;
                }
                row += b - a;
            }
        }
    });
    out->row_ptr[npat] = nrows;
    if (hits) hits->hit_ptr[nrows] = nhits;
}

// ... or merged on the devices (option device_merge: the RCCL all-gatherv path, for consumers that keep the rows in HBM;
// every shard ends up holding the merged CSR, shard 0 hands it to the host)
void shards_batch_device(cdb_shards* h, int G, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out) {
    const std::vector<cdb_index*>& shard = h->gen.shard;
    const Rebased kw = rebase(KeywordList{blob, offsets, npat});  // (once: every shard uploads the same list)
    std::vector<cdb_device_result> local(G), merged(G);
    // every shard stays locked from its query to the end of the merge (the merge reads the shard's result
    // buffers, which a concurrent query on that shard would overwrite); ascending shard order
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < G; ++i) locks.emplace_back(shard[i]->ix.mu);
    parallel_shards(G, [&](int i) {
        Index& ix = shard[i]->ix;
        DeviceScope scope(ix);
        const DeviceKeywords d = upload_keywords(ix, kw);
        const DeviceCsr r = query_batch_on_device(ix, d.pat, d.offs, npat);
        local[i] = cdb_device_result{npat, r.nrows, r.nhits, ix.q_rowptr.as<uint64_t>(), ix.q_ids.as<int64_t>(), ix.q_counts.as<int64_t>()};
    });
    uint64_t hits = 0;
    for (int i = 0; i < G; ++i) hits += local[i].nhits;
    // the collective merge is a phase of its own: a shard that failed above never leaves the others waiting
    parallel_shards(G, [&](int i) { merge_core(*h->gen.ranks[i], local[i], merged[i]); });
    Index& ix0 = shard[0]->ix;
    CDB_HIP(hipSetDevice(ix0.device));
    const cdb_device_result& m = merged[0];
    ResultOwner<cdb_result, cdb_result_free> res(ix0.stream);
    res.r.npat = npat;
    res.r.nrows = m.nrows;
    res.r.nhits = hits;
    res.r.row_ptr = res.fetch<uint64_t>(m.d_row_ptr, npat + 1);
    res.r.ids = res.fetch<int64_t>(m.d_ids, m.nrows);
    res.r.counts = res.fetch<int64_t>(m.d_counts, m.nrows);
    CDB_HIP(hipStreamSynchronize(ix0.stream));
    res.hand_over(out);
}

int shards_batch_impl(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out, cdb_hits* hits) {
    if (!h || !out || (npat && !offsets)) return CDB_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    if (hits) std::memset(hits, 0, sizeof(*hits));
    const int rc = guarded_on(h, [&] {
        check_keywords(KeywordList{blob, offsets, npat}, "cdb_shards_query_batch", KW_NONE_EMPTY);
        std::shared_lock<StateLock> st(h->state);
        const int G = std::max(h->gen.used, 1);
        if (G == 1) {
            check_shard(h, 0, hits ? cdb_query_batch_offsets(h->gen.shard[0], blob, offsets, npat, out, hits)
                                   : cdb_query_batch(h->gen.shard[0], blob, offsets, npat, out));
            return;
        }
        if (h->device_merge && !hits) shards_batch_device(h, G, blob, offsets, npat, out);
        else shards_batch_host(h, G, blob, offsets, npat, out, hits);
    });
    if (rc != CDB_OK) {
        cdb_result_free(out);
        if (hits) cdb_hits_free(hits);
    }
    return rc;
}
}  // namespace

int cdb_shards_query_batch(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out) {
    return shards_batch_impl(h, blob, offsets, npat, out, nullptr);
}

int cdb_shards_query_batch_offsets(cdb_shards* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out,
                                   cdb_hits* hits) {
    if (!hits) return CDB_E_INVALID;
    return shards_batch_impl(h, blob, offsets, npat, out, hits);
}

// ---- remove, append and cluster on a sharded column (include/coffeedb_gpu.h) ---------------------------------------------------
// Remove and append change WHICH documents the shards hold, so they are writers like a build: staging_mu, then the exclusive
// state lock for the whole call (no query runs meanwhile), then the ix.mu of the shards they touch in ascending order.  All or
// nothing: every shard PREPARES its new column beside the serving one (index_impl.h: remove_prepare / append_prepare); one
// failure drops every prepared column and the old ones go on serving; only when all stand does every shard commit.
namespace {
// cdb_remove's / cdb_append's refusal for the set: documents staged with cdb_shards_add* since the last build or load
void refuse_pending(const cdb_shards* h, const char* op) {
    const uint64_t built = h->gen.used ? h->gen.bounds[h->gen.used] : 0;
    if (h->staging_valid && h->ids.size() > built) throw Error(std::string(op) + ": documents were added since the last build");
}
// the bounds follow the documents every shard in use holds now (an emptied or "never built" shard holds none and stays in place)
void recount_bounds(cdb_shards* h) {
    std::vector<uint64_t> b{0};
    for (int i = 0; i < h->gen.used; ++i) {
        const Index& ix = h->gen.shard[i]->ix;
        b.push_back(b.back() + (ix.width ? ix.ndocs : 0));
    }
    h->gen.bounds.swap(b);
}
// ch[i]: shard i's prepared change (null: that shard stays as it is).  Exclusive state lock and the shards' ix.mu held.
void commit_changes(cdb_shards* h, std::vector<ColumnChangePtr>& ch) {
    bool any = false;
    for (const ColumnChangePtr& c : ch) any = any || c;
    if (!any) return;
    std::exception_ptr failed;  // a build over the new text failed on some shard (it is "never built" now); the others committed
    try {
        parallel_shards((int)ch.size(), [&](int i) {
            if (ch[i]) column_commit(h->gen.shard[i]->ix, *ch[i]);
        });
    } catch (...) {
        failed = std::current_exception();
    }
    recount_bounds(h);  // (either way: the shards hold what they hold)
    drop_staging(h);
    if (failed) std::rethrow_exception(failed);
}
}  // namespace

int cdb_shards_remove(cdb_shards* h, const int64_t* ids, uint64_t nids, uint64_t* removed, uint64_t* missing) {
    if (!h || (nids && !ids)) return CDB_E_INVALID;
    if (removed) *removed = 0;
    if (missing) *missing = 0;
    reserve_wait();
    return guarded_on(h, [&] {
        std::lock_guard<std::mutex> sg(h->staging_mu);
        std::unique_lock<StateLock> st(h->state);
        refuse_pending(h, "remove");
        if (!nids) return;
        const int G = h->gen.used;
        if (!G) {  // never built: the set holds no id
            if (missing) *missing = nids;
            return;
        }
        std::vector<std::unique_lock<std::mutex>> locks;  // ascending shard order
        for (int i = 0; i < G; ++i) locks.emplace_back(h->gen.shard[i]->ix.mu);
        std::vector<ColumnChangePtr> ch(G);  // (dropped on a failure, before the locks go)
        std::vector<uint64_t> rem(G, 0), mis(G, 0);
        parallel_shards(G, [&](int i) { ch[i] = remove_prepare(h->gen.shard[i]->ix, RowIds{ids, nullptr}, nids, &rem[i], &mis[i]); });
        uint64_t r = 0, m = 0;
        for (int i = 0; i < G; ++i) {
            r += rem[i];
            m += mis[i];
        }
        if (removed) *removed = r;
        if (missing) *missing = missing_in_all_shards(m, G, nids);
        commit_changes(h, ch);
    });
}

int cdb_shards_append(cdb_shards* h, const int64_t* ids, const char* blob, const uint64_t* doc_start, uint64_t ndocs, uint64_t* appended) {
    if (!h || (ndocs && (!ids || !blob || !doc_start))) return CDB_E_INVALID;
    if (appended) *appended = 0;
    reserve_wait();
    return guarded_on(h, [&] {
        std::lock_guard<std::mutex> sg(h->staging_mu);  // (every writer holds it: h->gen.used and h->ids stand still below)
        refuse_pending(h, "append");
        if (!ndocs) return;
        const uint64_t first = doc_start[0];
        for (uint64_t d = 0; d < ndocs; ++d)
            if (doc_start[d + 1] < doc_start[d]) throw Error("doc_start must be non-decreasing");
        if (doc_start[ndocs] - first >= (1ull << 48)) throw Error("doc_start must be non-decreasing");
        const uint64_t m = doc_start[ndocs] - first;
        if (!h->gen.used) {  // never built: a build of the given documents
            std::vector<const char*> ptrs(ndocs);
            std::vector<uint64_t> lens(ndocs);
            for (uint64_t d = 0; d < ndocs; ++d) {
                ptrs[d] = blob + doc_start[d];
                lens[d] = doc_start[d + 1] - doc_start[d];
            }
            build_views_locked(h, ids, ptrs.data(), lens.data(), ndocs);
            if (appended) *appended = ndocs;
            return;
        }
        std::unique_lock<StateLock> st(h->state);
        Generation& gen = h->gen;
        const int G = (int)h->devices.size(), used = gen.used;
        Index& lx = gen.shard[used - 1]->ix;
        const uint64_t last_bytes = lx.width ? lx.size : 0;
        // The new documents are numbered behind all old ones: they belong at the end of the column.  They join the last shard in use
        // while it stays within max_shard_bytes — or when no idle device slot is left, as the initial build's min(G, ...) lets its
        // last shard grow ...
        if (last_bytes + m <= h->max_shard_bytes || used == G) {
            std::unique_lock<std::mutex> lk(lx.mu);
            std::vector<ColumnChangePtr> ch(used);
            ch[used - 1] = append_prepare(lx, ids, blob, doc_start, ndocs);  // (capacity errors fire here: nothing was touched)
            commit_changes(h, ch);
            if (appended) *appended = ndocs;
            return;
        }
        // ... otherwise the last shard stays as it is and the batch opens new shards on the idle slots (shard_plan.h: append_cuts).
        const std::vector<uint64_t> cut = append_cuts(doc_start, ndocs, h->max_shard_bytes, G - used);
        const int pieces = (int)cut.size() - 1;
        // The new shards are built on fresh handles that carry the options set so far (the state lock keeps cdb_shards_set_option
        // waiting: it then reaches them through gen.shard); a failure destroys them and nothing has changed.  `opened` is no whole
        // generation: it owns what this call makes and, after the commit, what that replaced.
        Generation opened;
        open_handles(h, used, pieces, opened);
        parallel_shards(pieces, [&](int p) {
            check_handle(opened.shard[p], cdb_build_view(opened.shard[p], ids + cut[p], blob, doc_start + cut[p], cut[p + 1] - cut[p]));
        });
        // more shards: the merge ranks and the transport (the LocalTransport's board, the RCCL communicator) are sized by the count
        std::vector<cdb_index*> next(gen.shard);
        for (int p = 0; p < pieces; ++p) next[used + p] = opened.shard[p];
        make_merge(h->devices, next, used + pieces, opened);
        gen.ranks.swap(opened.ranks);  // the commit: nothing below fails.  (~opened: the old ranks, the old transport, the idle handles)
        gen.tr.swap(opened.tr);
        for (int p = 0; p < pieces; ++p) std::swap(gen.shard[used + p], opened.shard[p]);
        gen.used = used + pieces;
        recount_bounds(h);
        drop_staging(h);
        if (appended) *appended = ndocs;
    });
}

// A query: every shard groups the rows it holds and hands over the groups' strings; the lists meet on the host (cluster_merge.h).
// The strings of a with_values result cross PCIe anyway, and a merge that reads every byte once costs less than that download.
int cdb_shards_cluster(cdb_shards* h, const int64_t* ids, uint64_t nrows, int with_values, cdb_clusters* out) {
    if (!h || !out || (nrows && !ids)) return CDB_E_INVALID;
    *out = cdb_clusters{};
    const int rc = guarded_on(h, [&] {
        std::shared_lock<StateLock> st(h->state);
        const int G = std::max(h->gen.used, 1);
        if (G == 1) {
            check_shard(h, 0, cdb_cluster(h->gen.shard[0], ids, nrows, with_values, out));
            return;
        }
        Parts<cdb_clusters> parts(G, cdb_clusters_free);
        parallel_shards(G, [&](int i) { check_shard(h, i, cdb_cluster(h->gen.shard[i], ids, nrows, 1, &parts[i])); });
        std::vector<ClusterList> lists(G);
        uint64_t miss = 0;
        for (int i = 0; i < G; ++i) {
            lists[i] = ClusterList{parts[i].ngroups, parts[i].counts, parts[i].rep_ids, parts[i].value_ptr, parts[i].value_blob};
            miss += parts[i].missing;
        }
        MergedClusters mc;
        merge_cluster_lists(lists.data(), lists.size(), mc);
        const uint64_t ng = mc.ngroups();
        out->ngroups = ng;
        out->missing = missing_in_all_shards(miss, G, nrows);
        out->counts = (int64_t*)host_alloc(ng * 8);
        out->rep_ids = (int64_t*)host_alloc(ng * 8);
        if (ng) {
            std::memcpy(out->counts, mc.counts.data(), ng * 8);
            std::memcpy(out->rep_ids, mc.rep_ids.data(), ng * 8);
        }
        if (with_values) {
            out->value_ptr = (uint64_t*)host_alloc((ng + 1) * 8);
            out->value_blob = (char*)host_alloc(mc.value_blob.size());
            std::memcpy(out->value_ptr, mc.value_ptr.data(), (ng + 1) * 8);
            if (!mc.value_blob.empty()) std::memcpy(out->value_blob, mc.value_blob.data(), mc.value_blob.size());
        }
    });
    if (rc != CDB_OK) cdb_clusters_free(out);
    return rc;
}

}  // extern "C"
