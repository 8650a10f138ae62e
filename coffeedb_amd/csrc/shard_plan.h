// shard_plan.h — what every shard of a sharded string column holds: how many shards a column gets, where the document-aligned cuts
// fall, how an appended batch that does not fit the last shard is cut into new ones, and the one identity that turns the shards'
// "missing" counts into the set's.
//
// Plain host C++ with no HIP and no handle, in the manner of cluster_merge.h (tests/cpp/test_shard_plan.cpp runs it on its own,
// against naive restatements).  shards.hip is the only user: cdb_shards_build / _build_views, _append, _remove and _cluster.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace cdb {

// Shard only when the column exceeds what one GPU should hold (north star), unless told to spread anyway (use_all): the fewest shards
// of at most max_shard_bytes, never more than there are device slots — the last shard then grows beyond the limit — or documents,
// and at least one.
inline int shard_count(uint64_t total_bytes, uint64_t ndocs, int slots, uint64_t max_shard_bytes, bool use_all) {
    const uint64_t wanted = (total_bytes + max_shard_bytes - 1) / max_shard_bytes;
    int used = use_all ? slots : (int)std::min<uint64_t>((uint64_t)slots, std::max<uint64_t>(1, wanted));
    return std::max(1, std::min<int>(used, (int)std::max<uint64_t>(ndocs, 1)));
}

// doc-aligned split into `parts` contiguous ranges balanced by bytes: docs [b[r], b[r+1]).  Cut r is the first document boundary at
// or behind byte total * r / parts (the product in 128 bits: a column times its shard count may pass 2^64).
inline std::vector<uint64_t> shard_bounds(const std::vector<uint64_t>& doc_start, int parts) {
    const uint64_t nd = doc_start.size() - 1, total = doc_start[nd];
    std::vector<uint64_t> b{0};
    for (int r = 1; r < parts; ++r) {
        const unsigned __int128 target128 = (unsigned __int128)total * r / parts;
        const uint64_t target = (uint64_t)target128;
        uint64_t d = std::lower_bound(doc_start.begin(), doc_start.end(), target) - doc_start.begin();
        d = std::min<uint64_t>(std::max<uint64_t>(d, b.back()), nd);
        b.push_back(d);
    }
    b.push_back(nd);
    return b;
}

// An appended batch (ndocs documents, doc_start[ndocs + 1] offsets) that opens new shards on `slots` idle device slots: cut at
// document boundaries into pieces of at most max_shard_bytes.  A lone larger document is its own piece; the last slot takes the
// remainder, whatever its size.  Piece p holds docs [cut[p], cut[p + 1]).
inline std::vector<uint64_t> append_cuts(const uint64_t* doc_start, uint64_t ndocs, uint64_t max_shard_bytes, int slots) {
    std::vector<uint64_t> cut{0};
    uint64_t acc = 0;
    for (uint64_t d = 0; d < ndocs; ++d) {
        const uint64_t len = doc_start[d + 1] - doc_start[d];
        if (d > cut.back() && acc + len > max_shard_bytes && (int)cut.size() < slots) {
            cut.push_back(d);
            acc = 0;
        }
        acc += len;
    }
    cut.push_back(ndocs);
    return cut;
}

// Object ids are disjoint across shards: an entry of a list of n ids held by one shard is missing in the other G - 1, an entry held
// by none is missing in all G.  So sum(missing_s) = (G - 1) * held + G * unheld = (G - 1) * n + unheld, and the set misses
inline uint64_t missing_in_all_shards(uint64_t sum_of_shard_missing, int G, uint64_t n) { return sum_of_shard_missing - (uint64_t)(G - 1) * n; }

}  // namespace cdb
