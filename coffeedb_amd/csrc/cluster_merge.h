// cluster_merge.h — the cross-shard half of cdb_shards_cluster: k group lists, each ascending by std::string::operator<, become one.
//
// Every shard of a sharded string column clusters the rows it holds (cdb_cluster with the groups' strings).  A string may
// occur in several shards, so the lists are merged by string: groups with equal strings fuse, their counts add, and the
// representative id is the smallest.  Plain host C++ with no HIP and no handle (tests/cpp/test_cluster_merge.cpp runs it
// on its own).  The merge walks the k heads and picks the smallest by a linear scan: k is the shard count (a handful),
// and every byte of every string is read a small constant number of times — less than the download that brought it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace cdb {

struct ClusterList {  // one shard's answer (the arrays of a cdb_clusters made with with_values = 1)
    uint64_t ngroups = 0;
    const int64_t* counts = nullptr;
    const int64_t* rep_ids = nullptr;
    const uint64_t* value_ptr = nullptr;  // ngroups + 1 offsets into value_blob (may be null when ngroups == 0)
    const char* value_blob = nullptr;
    std::string_view value(uint64_t g) const { return std::string_view(value_blob + value_ptr[g], (size_t)(value_ptr[g + 1] - value_ptr[g])); }
};

struct MergedClusters {
    std::vector<int64_t> counts, rep_ids;
    std::vector<uint64_t> value_ptr{0};  // groups + 1
    std::string value_blob;
    uint64_t ngroups() const { return counts.size(); }
};

// std::string_view compares through char_traits<char>: unsigned bytes, a proper prefix first, the empty string first of all —
// the order every input list is in (include/coffeedb_gpu.h: cdb_cluster)
inline void merge_cluster_lists(const ClusterList* lists, size_t k, MergedClusters& out) {
    out.counts.clear();
    out.rep_ids.clear();
    out.value_ptr.assign(1, 0);
    out.value_blob.clear();
    uint64_t groups = 0, bytes = 0;
    for (size_t q = 0; q < k; ++q) {
        groups += lists[q].ngroups;
        if (lists[q].ngroups) bytes += lists[q].value_ptr[lists[q].ngroups] - lists[q].value_ptr[0];
    }
    out.counts.reserve(groups);
    out.rep_ids.reserve(groups);
    out.value_ptr.reserve(groups + 1);
    out.value_blob.reserve(bytes);
    std::vector<uint64_t> head(k, 0);
    for (;;) {
        size_t best = k;
        for (size_t q = 0; q < k; ++q) {
            if (head[q] == lists[q].ngroups) continue;
            if (best == k || lists[q].value(head[q]) < lists[best].value(head[best])) best = q;
        }
        if (best == k) break;
        const std::string_view v = lists[best].value(head[best]);
        int64_t count = 0, rep = 0;
        bool first = true;
        for (size_t q = best; q < k; ++q) {  // (lists in front of `best` hold a larger head, or none)
            if (head[q] == lists[q].ngroups || lists[q].value(head[q]) != v) continue;
            const uint64_t g = head[q]++;
            count += lists[q].counts[g];
            rep = first ? lists[q].rep_ids[g] : (lists[q].rep_ids[g] < rep ? lists[q].rep_ids[g] : rep);
            first = false;
        }
        out.counts.push_back(count);
        out.rep_ids.push_back(rep);
        out.value_blob.append(v.data(), v.size());
        out.value_ptr.push_back(out.value_blob.size());
    }
}

}  // namespace cdb
