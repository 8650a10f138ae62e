// string_index::cluster / remove / append on a SHARDED string column through the reference-side binding (coffeedb_amd/csrc/shim/index.h).
// Run with COFFEEDB_GPUS="0,0" COFFEEDB_SHARD_ALL="1": every column is split over two shards.  cluster() is checked against the literal
// std::map loop of database.cpp:442-460; after remove() and append() the index must answer like one freshly built over the same documents.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "index.h"

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                            \
        }                                                          \
    } while (0)

using C = index::cluster_type;
using R = index::result_type;
static std::map<int64_t, std::map<std::string, std::string>> data;  // database.cpp's object store, string fields only

// database.cpp:442-460 for a string field
static C reference_cluster(const R& results, const std::string& field) {
    std::map<std::string, int64_t> times;
    for (auto [id, correlation] : results) {
        auto iter = data[id].find(field);
        times[iter->second] += 1;
    }
    return C(times.begin(), times.end());
}

// the documents of `data` in id order, in a fresh index
static void fill(string_index& ix) {
    for (auto& [id, obj] : data) ix.add(id, obj["name"]);
    ix.build();
}
static R rows_of_store() {
    R rows;
    for (auto& [id, obj] : data) rows.emplace_back(id, 0);
    return rows;
}
static void same_answers(const string_index& got, const string_index& fresh) {
    const std::vector<std::string> kws = {"coffee", "sun", "a", "fe", "\xc3\xa9", "db", "zzz", "kafei", "e"};
    for (const std::string& kw : kws) CHECK(got.query(kw) == fresh.query(kw));
    CHECK(got.query_batch(kws) == fresh.query_batch(kws));
    CHECK(got.query_any(kws) == fresh.query_any(kws));
    CHECK(got.query_ranked(kws, 1, 1000, 5) == fresh.query_ranked(kws, 1, 1000, 5));
    CHECK(got.highlight_spans(kws) == fresh.highlight_spans(kws));
    const R rows = rows_of_store();
    CHECK(got.render_rows(rows, kws, "<", ">") == fresh.render_rows(rows, kws, "<", ">"));
    CHECK(got.cluster(rows) == fresh.cluster(rows));
    CHECK(got.cluster(rows) == reference_cluster(rows, "name"));
}

int main() {
    const char* e = std::getenv("COFFEEDB_GPUS");
    if (!e || !*e) {
        std::printf("set COFFEEDB_GPUS=\"0,0\" COFFEEDB_SHARD_ALL=\"1\"\n");
        return 2;
    }
    try {
        const char* names[] = {"sunkafei", "coffee", "sunkafei", "", "coffeedb", "coffee", "caf\xc3\xa9", "sunkafei", "", "db", "coffee", "caf\xc3\xa9"};
        const int n = 12;
        for (int i = 0; i < n; ++i) data[1000 + 7 * i]["name"] = names[i];
        string_index name;
        fill(name);
        {   // cluster: equal strings (and the empty string) live in both shards and must form one group each
            const R all = rows_of_store();
            const R some(all.begin() + 2, all.begin() + 9), none;
            for (const R* rows : {&all, &some, &none}) CHECK(name.cluster(*rows) == reference_cluster(*rows, "name"));
            CHECK((name.cluster(all) == C{{"", 2}, {"caf\xc3\xa9", 2}, {"coffee", 3}, {"coffeedb", 1}, {"db", 1}, {"sunkafei", 3}}));
            const R hits = name.query("coffee");
            CHECK(hits.size() == 4);
            CHECK((name.cluster(hits) == C{{"coffee", 3}, {"coffeedb", 1}}));
        }
        {   // remove: documents of both shards leave, an id nobody holds is ignored
            const std::vector<int64_t> gone = {1000, 1000 + 7 * 5, 1000 + 7 * 11, 424242};
            CHECK(name.remove(gone));
            for (int64_t id : gone) data.erase(id);
            string_index fresh;
            fill(fresh);
            same_answers(name, fresh);
        }
        std::vector<std::string> keep = {"coffee", "", "sunkafei and coffee", "caf\xc3\xa9"};
        {   // append: the documents added since build() join the end of the sharded column
            CHECK(!name.append());  // nothing pending
            for (size_t k = 0; k < keep.size(); ++k) {
                data[5000 + (int64_t)k]["name"] = keep[k];
                name.add(5000 + (int64_t)k, keep[k]);
            }
            CHECK(!name.remove({1007}));  // documents were added since the last build: refused, nothing changes
            CHECK(name.append());
            string_index fresh;
            fill(fresh);
            same_answers(name, fresh);
        }
        {   // ... and the next removal works on the grown column, down to nothing
            CHECK(name.remove({5000, 1007}));
            data.erase(5000);
            data.erase(1007);
            string_index fresh;
            fill(fresh);
            same_answers(name, fresh);
            std::vector<int64_t> rest;
            for (auto& [id, obj] : data) rest.push_back(id);
            CHECK(name.remove(rest));
            CHECK(name.query("coffee").empty());
            CHECK(name.cluster(rows_of_store()).empty());
        }
    } catch (const std::exception& ex) {
        std::printf("FAIL exception: %s\n", ex.what());
        ++failures;
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
