// host_io.h — what the host halves of the entry points share at the boundary: a keyword list into a handle's pattern buffers,
// device arrays into host blocks of the result cache, the owner of a result while it is made, and the profile table as text.
// The caller holds the handle's lock and a DeviceScope on it (index_impl.h).
#pragma once
#include <cstdio>
#include <cstring>

#include "index_impl.h"
#include "keyword_list.h"

namespace cdb {

// a rebased list in ix.q_pat / ix.q_offs, queued on ix.stream (k.rel is read by the copy: it lives until the stream is synchronised)
struct DeviceKeywords {
    const uint8_t* pat;
    const uint64_t* offs;
};
inline DeviceKeywords upload_keywords(Index& ix, const Rebased& k) {
    ix.q_pat.ensure(k.nbytes + 16);
    ix.q_offs.ensure(k.rel.size() * 8);
    if (k.nbytes) CDB_HIP(hipMemcpyAsync(ix.q_pat.p, k.bytes, k.nbytes, hipMemcpyHostToDevice, ix.stream));
    CDB_HIP(hipMemcpyAsync(ix.q_offs.p, k.rel.data(), k.rel.size() * 8, hipMemcpyHostToDevice, ix.stream));
    return DeviceKeywords{ix.q_pat.as<uint8_t>(), ix.q_offs.as<uint64_t>()};
}

// count elements from the device into a fresh host block, queued on s (count = 0: the block alone)
template <typename T> T* fetch(hipStream_t s, const void* d, uint64_t count) {
    T* h = (T*)host_alloc(count * sizeof(T));
    if (count) {
        const hipError_t e = hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) {
            host_free(h);
            CDB_HIP(e);
        }
    }
    return h;
}

// A result struct R while it is made: its arrays are host blocks that `release` (the struct's cdb_*_free) hands back.  Copies
// queued by fetch may still be in flight when an error unwinds: the stream drains before the blocks go.
template <typename R, void (*release)(R*)>
struct ResultOwner {
    R r{};
    hipStream_t stream;
    bool queued = false;
    explicit ResultOwner(hipStream_t s) : stream(s) {}
    ResultOwner(const ResultOwner&) = delete;
    ResultOwner& operator=(const ResultOwner&) = delete;
    ~ResultOwner() {
        if (queued) (void)hipStreamSynchronize(stream);
        release(&r);
    }
    template <typename T> T* fetch(const void* d, uint64_t count) {
        queued = true;
        return cdb::fetch<T>(stream, d, count);
    }
    void hand_over(R* out) {  // (the caller synchronised: the arrays are complete)
        *out = r;
        r = R{};
        queued = false;
    }
};

// n (id, count) rows from the device into result arrays; synchronises s, also when it fails (the blocks go back behind the drain)
inline void download_rows(hipStream_t s, const int64_t* d_ids, const int64_t* d_counts, uint64_t n, int64_t** ids, int64_t** counts,
                          size_t* nrows) {
    int64_t *hi = nullptr, *hc = nullptr;
    try {
        hi = fetch<int64_t>(s, d_ids, n);
        hc = fetch<int64_t>(s, d_counts, n);
        CDB_HIP(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipStreamSynchronize(s);
        host_free(hi);
        host_free(hc);
        throw;
    }
    *ids = hi;
    *counts = hc;
    *nrows = (size_t)n;
}

// the kernel records of ix.prof, one "name ms launches bytes" line each, cut to cap - 1 characters; false: the table was cut short
inline bool profile_dump(Index& ix, char* buf, size_t cap) {
    std::lock_guard<std::mutex> g(ix.mu);
    std::string s;
    for (auto& kv : ix.prof.recs) {
        char line[256];
        std::snprintf(line, sizeof(line), "%s %.6f %llu %llu\n", kv.first.c_str(), kv.second.ms, (unsigned long long)kv.second.launches,
                      (unsigned long long)kv.second.bytes);
        s += line;
    }
    std::strncpy(buf, s.c_str(), cap - 1);
    buf[cap - 1] = 0;
    return s.size() < cap;
}

}  // namespace cdb
