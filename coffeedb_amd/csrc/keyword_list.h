// keyword_list.h — a keyword list as every query entry point receives it (one blob, n + 1 offsets into it), the checks the entry
// points make on it, and its form on the way to the device: the first byte, the byte count and offsets relative to that byte.
//
// Plain host C++ with no HIP and no handle, in the manner of shard_plan.h (tests/cpp/test_keyword_list.cpp runs it on its own,
// against naive restatements).  host_io.h uploads a rebased list; capi_query.hip, columns.hip, render.hip, select.hip and
// shards.hip check and rebase theirs here.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "errors.h"

namespace cdb {

struct KeywordList {  // keyword j = blob[off[j] .. off[j + 1])
    const char* blob;
    const uint64_t* off;
    uint64_t n;
};

// What an entry point refuses, in the order the checks run.  Every entry point names the ones it makes: they differ (a batch
// may be empty, a constraint may not; only render and select look at the blob).
enum KeywordCheck : unsigned {
    KW_LIST_NOT_EMPTY = 1,  // "The constraint list cannot be empty" (interface.cpp:75-77)
    KW_OFFSETS = 2,         // "<who>: keyword offsets missing"
    KW_NONE_EMPTY = 4,      // "Empty keywords are not allowed" (index.cpp:239-241)
    KW_BYTES = 8,           // "<who>: keywords without bytes"
};
inline void check_keywords(const KeywordList& k, const char* who, unsigned checks) {
    if ((checks & KW_LIST_NOT_EMPTY) && k.n == 0) throw Error("The constraint list cannot be empty");
    if ((checks & KW_OFFSETS) && !k.off) throw Error(std::string(who) + ": keyword offsets missing");
    if (checks & KW_NONE_EMPTY)
        for (uint64_t j = 0; j < k.n; ++j)
            if (k.off[j + 1] <= k.off[j]) throw Error("Empty keywords are not allowed");
    if ((checks & KW_BYTES) && k.n && !k.blob) throw Error(std::string(who) + ": keywords without bytes");
}

// The list as it travels: keyword j = bytes[rel[j] .. rel[j + 1]), rel[0] = 0, rel[n] = nbytes.  No keyword: rel = {0}.
struct Rebased {
    const char* bytes = nullptr;
    uint64_t nbytes = 0;
    std::vector<uint64_t> rel{0};
    uint64_t n() const { return rel.size() - 1; }
};
// a checked list (offsets ascending) on its first byte; the bytes stay the caller's
inline Rebased rebase(const KeywordList& k) {
    Rebased r;
    if (!k.n) return r;
    const uint64_t base = k.off[0];
    r.bytes = k.blob + base;
    r.nbytes = k.off[k.n] - base;
    r.rel.resize(k.n + 1);
    for (uint64_t j = 0; j <= k.n; ++j) r.rel[j] = k.off[j] - base;
    return r;
}
// ... of any list, with the empty keywords dropped (cdb_query_spans: an empty highlight keyword never matches,
// ac_automaton::insert); the kept bytes are gathered into `store`, which must outlive the result
inline Rebased rebase_nonempty(const KeywordList& k, std::string& store) {
    Rebased r;
    store.clear();
    for (uint64_t j = 0; j < k.n; ++j) {
        if (k.off[j + 1] <= k.off[j]) continue;
        store.append(k.blob + k.off[j], k.off[j + 1] - k.off[j]);
        r.rel.push_back(store.size());
    }
    r.bytes = store.data();
    r.nbytes = store.size();
    return r;
}

}  // namespace cdb
