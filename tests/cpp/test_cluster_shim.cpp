// `cluster` through the reference-side binding (coffeedb_amd/csrc/shim/cluster.h, index.h).
//  * host part (-DCLUSTER_SHIM_HOST_ONLY: no library, no GPU): cdb_shim::cluster_rows fed with hand-made cdb_clusters — the
//    strings std::to_string makes, their merging and their order.
//  * device part (COFFEEDB_GPU_NUMERIC=1 test_cluster_shim): a handful of objects in a std::map store, cluster() over an integer,
//    a double, a bool and a string field against a literal restatement of database.cpp:442-460 over that store.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <string>
#include <variant>
#include <vector>

#include "cluster.h"
#ifndef CLUSTER_SHIM_HOST_ONLY
#include "index.h"
#endif

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                            \
        }                                                          \
    } while (0)

using C = std::vector<std::pair<const std::string, int64_t>>;

static uint64_t bits_of(double v) {
    uint64_t r;
    std::memcpy(&r, &v, 8);
    return r;
}

static void host_part() {
    {  // int64: printed in full, ordered as strings
        const int64_t mn = std::numeric_limits<int64_t>::min(), mx = std::numeric_limits<int64_t>::max();
        uint64_t values[] = {(uint64_t)mn, (uint64_t)-10, (uint64_t)-1, 9, 10, (uint64_t)mx};
        int64_t counts[] = {1, 2, 3, 4, 5, 6}, reps[] = {0, 0, 0, 0, 0, 0};
        cdb_clusters c{6, 0, counts, reps, values, nullptr, nullptr};
        const C got = cdb_shim::cluster_rows(c, 1);
        CHECK((got == C{{"-1", 3}, {"-10", 2}, {"-9223372036854775808", 1}, {"10", 5}, {"9", 4}, {"9223372036854775807", 6}}));
    }
    {  // double: "%f"; values that print alike share an entry; inf prints inf
        const double inf = std::numeric_limits<double>::infinity();
        uint64_t values[] = {bits_of(-inf), bits_of(-2.5), bits_of(0.0), bits_of(1e-7), bits_of(2e-7), bits_of(1.5), bits_of(1234567.125), bits_of(inf)};
        int64_t counts[] = {1, 2, 4, 8, 16, 32, 64, 128}, reps[8] = {};
        cdb_clusters c{8, 0, counts, reps, values, nullptr, nullptr};
        const C got = cdb_shim::cluster_rows(c, 2);
        CHECK((got == C{{"-2.500000", 2}, {"-inf", 1}, {"0.000000", 28}, {"1.500000", 32}, {"1234567.125000", 64}, {"inf", 128}}));
    }
    {  // bool: promoted to int
        uint64_t values[] = {0, 1};
        int64_t counts[] = {7, 5}, reps[] = {1, 2};
        cdb_clusters c{2, 3, counts, reps, values, nullptr, nullptr};
        CHECK((cdb_shim::cluster_rows(c, 0) == C{{"0", 7}, {"1", 5}}));
        cdb_clusters one{1, 0, counts, reps, values + 1, nullptr, nullptr};
        CHECK((cdb_shim::cluster_rows(one, 0) == C{{"1", 7}}));
    }
    {  // strings: slices of the blob, already in order; the empty string first
        char blob[] = "ababc\xffz";
        uint64_t ptr[] = {0, 0, 2, 5, 7};
        int64_t counts[] = {1, 2, 3, 4}, reps[4] = {};
        cdb_clusters c{4, 0, counts, reps, nullptr, ptr, blob};
        CHECK((cdb_shim::cluster_rows(c) == C{{"", 1}, {"ab", 2}, {"abc", 3}, {"\xffz", 4}}));
    }
    {  // nothing
        cdb_clusters c{};
        CHECK(cdb_shim::cluster_rows(c, 1).empty() && cdb_shim::cluster_rows(c).empty());
    }
}

#ifndef CLUSTER_SHIM_HOST_ONLY
using value = std::variant<bool, int64_t, double, std::string>;
using R = index::result_type;
static std::map<int64_t, std::map<std::string, value>> data;

// database.cpp:442-460, restated over the store above
static C reference_cluster(const R& results, const std::string& field) {
    std::map<std::string, int64_t> times;
    for (auto [id, correlation] : results) {
        auto iter = data[id].find(field);
        std::visit([&times](auto&& val) {
            using type = std::decay_t<decltype(val)>;
            if constexpr (std::is_same_v<type, std::string>) {
                times[val] += 1;
            } else {
                times[std::to_string(val)] += 1;
            }
        }, iter->second);
    }
    return C(times.begin(), times.end());
}

static void device_part() {
    // the README's two objects, then a few more
    const char* names[] = {"sunkafei", "coffee", "sunkafei", "", "coffeedb", "coffee", "caf\xc3\xa9", "sunkafei", ""};
    const int64_t numbers[] = {1234, 999, -10, -1, 10, 9, 999, 1234, -10};
    const double ratios[] = {1e-7, 2e-7, 1.5, -2.5, 1.5, 3.0, 0.0, 1e-7, 1.5};
    const bool flags[] = {true, false, true, true, false, true, true, false, true};
    const int n = 9;
    string_index name;
    integer_index number;
    double_index ratio;
    bool_index flag;
    std::vector<std::string> keep(names, names + n);
    R all;
    for (int i = 0; i < n; ++i) {
        const int64_t id = 1000 + 7 * ((i * 5) % n);  // (not ascending)
        data[id]["name"] = keep[i];
        data[id]["number"] = numbers[i];
        data[id]["ratio"] = ratios[i];
        data[id]["flag"] = flags[i];
        name.add(id, keep[i]);
        number.add(id, numbers[i]);
        ratio.add(id, ratios[i]);
        flag.add(id, flags[i]);
        all.emplace_back(id, 0);
    }
    name.build();
    number.build();
    ratio.build();
    flag.build();
    const R whole = all, some(all.begin() + 2, all.begin() + 7), none;
    for (const R* rows : {&whole, &some, &none}) {
        CHECK(number.cluster(*rows) == reference_cluster(*rows, "number"));
        CHECK(ratio.cluster(*rows) == reference_cluster(*rows, "ratio"));
        CHECK(flag.cluster(*rows) == reference_cluster(*rows, "flag"));
        CHECK(name.cluster(*rows) == reference_cluster(*rows, "name"));
    }
    CHECK((number.cluster(all) == C{{"-1", 1}, {"-10", 2}, {"10", 1}, {"1234", 2}, {"9", 1}, {"999", 2}}));
    CHECK((ratio.cluster(all) == C{{"-2.500000", 1}, {"0.000000", 4}, {"1.500000", 3}, {"3.000000", 1}}));
    // the rows string_index::query returns are clustered like any others
    const R hits = name.query("coffee");
    CHECK(hits.size() == 3);
    CHECK(name.cluster(hits) == reference_cluster(hits, "name"));
    CHECK((name.cluster(hits) == C{{"coffee", 2}, {"coffeedb", 1}}));
}
#endif

int main() {
    try {
        host_part();
#ifndef CLUSTER_SHIM_HOST_ONLY
        const char* e = std::getenv("COFFEEDB_GPU_NUMERIC");
        if (!e || *e != '1') {
            std::printf("set COFFEEDB_GPU_NUMERIC=1\n");
            return 2;
        }
        device_part();
#endif
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
