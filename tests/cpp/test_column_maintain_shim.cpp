// append() of the drop-in bool / integer / double indexes.  "gpu" (COFFEEDB_GPU_NUMERIC=1): add + build, then add + append();
// the queries must equal those of indexes built over everything; append() without pending rows is false.  "cpu" (variable
// unset): append() is false and changes nothing.  usage: [COFFEEDB_GPU_NUMERIC=1] test_column_maintain_shim gpu|cpu
#include <cstdio>
#include <cstdlib>
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

static const int N = 9000, FIRST = 6000;  // rows in all, rows of the first build
static int64_t id_of(int i) { return (int64_t)((i * 7919) % N) * 3 - 5000; }  // shuffled, negative ones among them
static int64_t ival(int i) { return (i * 31) % 97 - 40; }
static double dval(int i) { return ((i * 17) % 101 - 50) * 0.25; }
static bool bval(int i) { return (i * 13) % 5 < 2; }

template <typename Ix, typename F>
static void fill(Ix& ix, int from, int to, F value) {
    for (int i = from; i < to; ++i) ix.add(id_of(i), value(i));
}

static void on_gpu() {
    integer_index ia, ib;
    double_index da, db;
    bool_index ba, bb;
    CHECK(ia.column() && da.column() && ba.column());
    fill(ia, 0, FIRST, ival);
    fill(da, 0, FIRST, dval);
    fill(ba, 0, FIRST, bval);
    ia.build();
    da.build();
    ba.build();
    CHECK(!ia.append() && !da.append() && !ba.append());  // nothing pending
    fill(ia, FIRST, N, ival);
    fill(da, FIRST, N, dval);
    fill(ba, FIRST, N, bval);
    CHECK(ia.append() && da.append() && ba.append());
    CHECK(!ia.append() && !da.append() && !ba.append());  // the rows were handed over once
    fill(ib, 0, N, ival);
    fill(db, 0, N, dval);
    fill(bb, 0, N, bval);
    ib.build();
    db.build();
    bb.build();
    for (const char* r : {"[-40,56]", "[0,10)", "(5,5]", "[-inf,inf]", "[12,12]"}) CHECK(ia.query(r) == ib.query(r));
    for (const char* r : {"[-12.5,12.5]", "[0,2.5)", "[0.25,0.25]", "[-1000,1000]"}) CHECK(da.query(r) == db.query(r));
    for (const char* r : {"true", "false"}) CHECK(ba.query(r) == bb.query(r));
    CHECK(ia.query("[-inf,inf]").size() == (size_t)N && ba.query("true").size() + ba.query("false").size() == (size_t)N);
    // a refused batch (an id the column holds) stays pending and reaches the caller in the library's words
    ia.add(id_of(3), 1);
    bool threw = false;
    try {
        ia.append();
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()) == "cdb_column_append: duplicate object id " + std::to_string(id_of(3)) + " in one column";
    }
    CHECK(threw);
    CHECK(ia.query("[-inf,inf]").size() == (size_t)N);
}

static void on_cpu() {
    integer_index ia;
    double_index da;
    bool_index ba;
    CHECK(!ia.column() && !da.column() && !ba.column());
    fill(ia, 0, 100, ival);
    fill(da, 0, 100, dval);
    fill(ba, 0, 100, bval);
    ia.build();
    da.build();
    ba.build();
    const auto qi = ia.query("[-inf,inf]");
    const auto qd = da.query("[-1000,1000]");
    const auto qb = ba.query("true");
    CHECK(!ia.append() && !da.append() && !ba.append());
    CHECK(ia.query("[-inf,inf]") == qi && da.query("[-1000,1000]") == qd && ba.query("true") == qb);
    // rows added to a CPU class are the class's own business (the reference's add()); append() stays false and takes nothing
    // away from the build() the caller falls back to
    fill(ia, 100, 120, ival);
    fill(da, 100, 120, dval);
    fill(ba, 100, 120, bval);
    CHECK(!ia.append() && !da.append() && !ba.append());
    ia.build();
    da.build();
    ba.build();
    integer_index ib;
    double_index db;
    bool_index bb;
    fill(ib, 0, 120, ival);
    fill(db, 0, 120, dval);
    fill(bb, 0, 120, bval);
    ib.build();
    db.build();
    bb.build();
    CHECK(ia.query("[-inf,inf]") == ib.query("[-inf,inf]") && da.query("[-1000,1000]") == db.query("[-1000,1000]"));
    CHECK(ba.query("true") == bb.query("true") && ba.query("false") == bb.query("false"));
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const char* e = std::getenv("COFFEEDB_GPU_NUMERIC");
    const bool gpu = e && *e == '1';
    if ((mode != "gpu" && mode != "cpu") || gpu != (mode == "gpu")) {
        std::printf("usage: COFFEEDB_GPU_NUMERIC=1 test_column_maintain_shim gpu | test_column_maintain_shim cpu\n");
        return 2;
    }
    try {
        if (gpu) on_gpu();
        else on_cpu();
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
