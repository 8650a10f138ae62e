// The cross-shard merge of cluster groups (coffeedb_amd/csrc/cluster_merge.h) on its own: k sorted group lists against a
// std::map<std::string, ...> restatement.  Host code only; tests/test_cluster_merge_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../coffeedb_amd/csrc/cluster_merge.h"

namespace {

struct Group {
    std::string value;
    int64_t count, rep;
};
// one shard's answer, owning its arrays the way a cdb_clusters does (exactly sized: the sanitizer sees every overrun)
struct Owned {
    std::vector<int64_t> counts, reps;
    std::vector<uint64_t> ptr;
    std::vector<char> blob;
    cdb::ClusterList view;
    explicit Owned(std::vector<Group> g, bool null_when_empty = false) {
        std::sort(g.begin(), g.end(), [](const Group& a, const Group& b) { return a.value < b.value; });  // std::string order
        ptr.push_back(0);
        for (const Group& x : g) {
            counts.push_back(x.count);
            reps.push_back(x.rep);
            blob.insert(blob.end(), x.value.begin(), x.value.end());
            ptr.push_back(blob.size());
        }
        view.ngroups = g.size();
        if (g.empty() && null_when_empty) return;  // (an empty list may come without arrays)
        view.counts = counts.data();
        view.rep_ids = reps.data();
        view.value_ptr = ptr.data();
        view.value_blob = blob.data();
    }
};

int failures = 0;
void check(const char* name, const std::vector<std::vector<Group>>& lists, bool null_when_empty = false) {
    std::map<std::string, std::pair<int64_t, int64_t>> want;  // value -> (count, smallest rep)
    for (const auto& l : lists)
        for (const Group& g : l) {
            auto it = want.find(g.value);
            if (it == want.end()) want.emplace(g.value, std::make_pair(g.count, g.rep));
            else {
                it->second.first += g.count;
                it->second.second = std::min(it->second.second, g.rep);
            }
        }
    std::vector<Owned> owned;
    owned.reserve(lists.size());
    for (const auto& l : lists) owned.emplace_back(l, null_when_empty);
    std::vector<cdb::ClusterList> views;
    for (const Owned& o : owned) views.push_back(o.view);
    cdb::MergedClusters m;
    m.counts.assign(3, 7);  // (stale contents of a reused result must not survive)
    cdb::merge_cluster_lists(views.data(), views.size(), m);
    bool ok = m.ngroups() == want.size() && m.rep_ids.size() == want.size() && m.value_ptr.size() == want.size() + 1 && m.value_ptr[0] == 0 &&
              m.value_ptr.back() == m.value_blob.size();
    size_t g = 0;
    for (auto it = want.begin(); ok && it != want.end(); ++it, ++g) {
        const std::string got = m.value_blob.substr(m.value_ptr[g], m.value_ptr[g + 1] - m.value_ptr[g]);
        ok = got == it->first && m.counts[g] == it->second.first && m.rep_ids[g] == it->second.second;
    }
    if (!ok) {
        std::printf("FAIL %s (k = %zu): %zu groups, expected %zu\n", name, lists.size(), (size_t)m.ngroups(), want.size());
        ++failures;
    }
}

std::vector<Group> random_list(std::mt19937_64& rng, int n, int alphabet, int maxlen, bool high) {
    std::map<std::string, Group> g;  // (a list holds every string once)
    for (int i = 0; i < n; ++i) {
        std::string v((size_t)(rng() % (uint64_t)(maxlen + 1)), 'a');
        for (char& c : v) c = (char)((high ? 0x7E : 'a') + (int)(rng() % (uint64_t)alphabet));
        g[v] = Group{v, (int64_t)(rng() % 9 + 1), (int64_t)(rng() % 1000) - 500};
    }
    std::vector<Group> out;
    for (auto& kv : g) out.push_back(kv.second);
    return out;
}

}  // namespace

int main() {
    const std::vector<Group> A = {{"", 2, 40}, {"a", 1, 7}, {"ab", 3, 9}, {"abc", 1, 1}, {"b", 5, 12}};
    const std::vector<Group> B = {{"", 1, 3}, {"ab", 1, 2}, {"abd", 2, 60}, {"c", 1, 61}};
    const std::vector<Group> H = {{"\x7f", 1, 5}, {"\x80", 2, 6}, {"\xff", 1, 8}, {"a\x80", 1, 10}, {"a\x7f", 4, 11}, {std::string("a\0b", 3), 1, 13}, {"a", 1, 14}};
    const std::vector<Group> none;
    for (const bool nulls : {false, true}) {
        check("no lists", {}, nulls);
        check("one empty list", {none}, nulls);
        check("all lists empty", {none, none, none}, nulls);
        check("empty lists among full ones", {none, A, none, B, none, none, H, none}, nulls);
    }
    check("k = 1", {A});
    check("k = 2", {A, B});
    check("k = 3", {A, B, H});
    check("k = 8", {A, B, H, A, none, B, H, A});
    check("entirely equal lists", {A, A});
    check("entirely equal lists, k = 3", {B, B, B});
    check("entirely equal lists, k = 8", {A, A, A, A, A, A, A, A});
    check("a proper prefix in another list", {{{"ab", 1, 1}}, {{"a", 1, 2}}, {{"abc", 1, 3}}});
    check("the empty string in two lists", {{{"", 4, 9}}, {{"", 1, 2}, {"x", 1, 3}}});
    check("the empty string only", {{{"", 4, 9}}, {{"", 1, 2}}, {{"", 3, -2}}});
    check("bytes >= 0x80 sort behind ASCII (unsigned order)", {H, {{"\x80", 1, 1}, {"z", 1, 2}}});
    check("bytes >= 0x80, k = 8", {H, H, A, H, B, H, none, H});
    {
        std::vector<std::vector<Group>> same(8, std::vector<Group>{{"same", 2, 0}});
        for (size_t q = 0; q < same.size(); ++q) same[q][0].rep = 100 - (int64_t)q;  // (the smallest rep sits in the last list)
        check("one string in all 8 lists", same);
        same.resize(3);
        check("one string in all 3 lists", same);
        same.resize(2);
        check("one string in both lists", same);
    }
    std::mt19937_64 rng(12345);
    for (const int k : {1, 2, 3, 8})
        for (int round = 0; round < 40; ++round) {
            std::vector<std::vector<Group>> lists;
            for (int q = 0; q < k; ++q) lists.push_back(random_list(rng, (int)(rng() % 40), 2 + round % 3, 1 + round % 5, round % 4 == 3));
            check("random lists", lists);
        }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
