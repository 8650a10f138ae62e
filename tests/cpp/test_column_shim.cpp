// The drop-in index.h / index.cpp with COFFEEDB_GPU_NUMERIC=1: bool / integer / double indexes backed by GPU columns
// (cdb_column_*), driven the way database.cpp drives them, and a whole filter() — a string key, an integer range key and a
// bool key — answered by one cdb_query_and_columns call.  usage: COFFEEDB_GPU_NUMERIC=1 test_column_shim
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "index.h"
#include "../../include/coffeedb_gpu.h"

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                            \
        }                                                          \
    } while (0)

using R = std::vector<std::pair<int64_t, int64_t>>;

// the expectations of test_index_shim.cpp's numeric(), now answered by the device
static void numeric_on_gpu() {
    std::map<std::string, std::unique_ptr<index>> indices;
    indices["n"] = std::make_unique<integer_index>();
    auto* ip = dynamic_cast<integer_index*>(indices["n"].get());
    CHECK(ip != nullptr && ip->column() != nullptr);
    const int64_t vals[] = {123, 234, 999, 100, 200};
    for (int i = 0; i < 5; ++i) ip->add(10 + i, vals[i]);
    indices["n"]->build();
    bool threw = false;
    CHECK((indices["n"]->query("[100,200]") == R{{13, 0}, {10, 0}, {14, 0}}));
    CHECK((indices["n"]->query("(100,200)") == R{{10, 0}}));
    CHECK((indices["n"]->query(" [ 100, 200) ") == R{{13, 0}, {10, 0}}));
    try { indices["n"]->query("[100 ,200]"); } catch (const std::runtime_error& e) { threw = std::string(e.what()) == "Invalid value: 100 "; }
    CHECK(threw);
    CHECK((indices["n"]->query("[-inf,inf]").size() == 5));
    threw = false;
    try { indices["n"]->query("100..200"); } catch (const std::runtime_error& e) { threw = std::string(e.what()) == "Invalid range: 100..200"; }
    CHECK(threw);
    // database.cpp adds after a build and builds again (the `build` operation): every row is indexed
    ip->add(20, 150);
    indices["n"]->build();
    CHECK((indices["n"]->query("[100,200]") == R{{13, 0}, {10, 0}, {20, 0}, {14, 0}}));

    double_index di;
    CHECK(di.column() != nullptr);
    di.add(1, 1.7724); di.add(2, -3.5); di.add(3, 2.0);
    di.build();
    CHECK((di.query("[1.5,2.0]") == R{{1, 0}, {3, 0}}));
    CHECK((di.query("[1.5,2.0)") == R{{1, 0}}));
    CHECK((di.query("[-inf,0]") == R{}));  // -inf = the smallest positive double (utility.h:54-56)

    bool_index bi;
    CHECK(bi.column() != nullptr);
    bi.add(7, true); bi.add(8, false); bi.add(9, true);
    bi.build();
    CHECK((bi.query("true") == R{{7, 0}, {9, 0}}));
    CHECK((bi.query("false") == R{{8, 0}}));
    threw = false;
    try { bi.query("maybe"); } catch (const std::runtime_error& e) { threw = std::string(e.what()) == "Invalid query: \"maybe\""; }
    CHECK(threw);
    threw = false;  // the caller's words do not decide the error's class: the reference's wording, no "GPU column: " in front
    try { bi.query("internal"); } catch (const std::runtime_error& e) { threw = std::string(e.what()) == "Invalid query: \"internal\""; }
    CHECK(threw);
    CHECK(string_index::number == 3 && double_index::number == 2 && integer_index::number == 1 && bool_index::number == 0);
}

// filter({"secret": ["010"], "age": ["[10,20]", "[30,40]"], "active": "true"}) on the device
static void device_filter() {
    const char* docs[] = {"3010103", "301022", "01011010", "xx010", "none", "0101"};
    const int64_t ids[] = {100, 101, 102, 103, 104, 105};
    const int64_t ages[] = {15, 35, 50, 12, 18, 40};
    const bool act[] = {true, true, true, false, true, true};
    string_index s;
    integer_index age;
    bool_index active;
    std::vector<std::string> keep(docs, docs + 6);
    for (int i = 0; i < 6; ++i) {
        s.add(ids[i], keep[i]);
        age.add(ids[i], ages[i]);
        active.add(ids[i], act[i]);
    }
    s.build();
    age.build();
    active.build();
    // string_index keeps its cdb_index* private; its rows enter as a host list (what query_any returns) beside the columns,
    // and once more through a device string key built here directly
    const R srows = s.query_any({"010"});
    std::vector<int64_t> si, sc;
    for (auto& [i, c] : srows) { si.push_back(i); sc.push_back(c); }
    cdb_key_query kq{};
    kq.ids = si.data();
    kq.counts = sc.data();
    kq.nrows = si.size();
    const std::string ablob = "[10,20][30,40]", bblob = "true";
    const uint64_t aoff[] = {0, 7, 14}, boff[] = {0, 4};
    cdb_column_key cols[2] = {{age.column(), ablob.data(), aoff, 2}, {active.column(), bblob.data(), boff, 1}};
    int64_t *oi = nullptr, *oc = nullptr;
    size_t n = 0;
    CHECK(cdb_query_and_columns(&kq, 1, cols, 2, 0, 0, 0, 0, &oi, &oc, &n) == CDB_OK);
    // "010" in 100 (x2), 101, 102 (x2), 103, 105; ages in [10,20] u [30,40]: 100, 101, 103, 104, 105; active: all but 103
    R got;
    for (size_t r = 0; r < n; ++r) got.emplace_back(oi[r], oc[r]);
    CHECK((got == R{{100, 2}, {101, 1}, {105, 1}}));
    cdb_free(oi);
    cdb_free(oc);
    // the same with a device string key, ranked
    cdb_index* h = nullptr;
    CHECK(cdb_create(&h, -1) == CDB_OK);
    for (int i = 0; i < 6; ++i) cdb_add(h, ids[i], docs[i], std::string(docs[i]).size());
    CHECK(cdb_build(h) == CDB_OK);
    const std::string kw = "010";
    const uint64_t koff[] = {0, 3};
    cdb_key_query sk{};
    sk.index = h;
    sk.blob = kw.data();
    sk.offsets = koff;
    sk.nkw = 1;
    CHECK(cdb_query_and_columns(&sk, 1, cols, 2, 1, 1, 100, 0, &oi, &oc, &n) == CDB_OK);
    got.clear();
    for (size_t r = 0; r < n; ++r) got.emplace_back(oi[r], oc[r]);
    CHECK((got == R{{100, 2}, {101, 1}, {105, 1}}));
    cdb_free(oi);
    cdb_free(oc);
    // an invalid range reaches the caller in the reference's words, through the string key's handle
    const std::string bad = "[1,2";
    const uint64_t bad_off[] = {0, 4};
    cdb_column_key badk{age.column(), bad.data(), bad_off, 1};
    CHECK(cdb_query_and_columns(&sk, 1, &badk, 1, 0, 0, 0, 0, &oi, &oc, &n) == CDB_E_INVALID);
    CHECK(std::string(cdb_last_error(h)) == "Invalid range: [1,2");
    cdb_destroy(h);
}

int main() {
    const char* e = std::getenv("COFFEEDB_GPU_NUMERIC");
    if (!e || *e != '1') {
        std::printf("set COFFEEDB_GPU_NUMERIC=1\n");
        return 2;
    }
    try {
        numeric_on_gpu();
        device_filter();
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
