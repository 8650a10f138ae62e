// cdb_shim::insert as a database.cpp-style caller uses it: objects with two string fields, an integer, a double and a bool field (not
// every object has every field) are inserted in one call over fields that already serve older objects, and read back by select.
//   errors   the reference's three messages (database.cpp:284-290, :329) before anything reaches the library; the library's text for
//            an id a field already holds and for a failing field, after which nothing has changed
//   insert   every field answers like the model with the new objects; select over everything returns them
// usage: COFFEEDB_GPU_NUMERIC=1 test_insert_shim
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "index.h"
#include "insert.h"
#include "rowset.h"
#include "select.h"

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                            \
        }                                                          \
    } while (0)

using cdb_shim::var;
using object = std::vector<std::pair<std::string, var>>;

template <typename F>
static std::string thrown(F&& f) {
    try {
        f();
    } catch (const std::exception& e) {
        return e.what();
    }
    return "(nothing thrown)";
}

int main() {
    string_index title, body;
    integer_index year;
    double_index score;
    bool_index fresh;
    CHECK(title.gpu_index() && body.gpu_index() && year.column() && score.column() && fresh.column());
    if (failures) return 1;
    // the older objects: ids 100 .. 139 (the strings live until the program ends: the indexes keep views)
    std::vector<std::string> titles, bodies;
    for (int i = 0; i < 40; ++i) {
        titles.push_back("old coffee #" + std::to_string(i));
        bodies.push_back("about beans " + std::to_string(i % 7));
    }
    for (int i = 0; i < 40; ++i) {
        title.add(100 + i, titles[i]);
        if (i % 2) body.add(100 + i, bodies[i]);
        year.add(100 + i, 1990 + i);
        if (i % 3) score.add(100 + i, 0.5 * i);
        fresh.add(100 + i, i % 4 == 0);
    }
    title.build();
    body.build();
    year.build();
    score.build();
    fresh.build();
    const cdb_shim::field_map fields{{"title", &title}, {"body", &body}, {"year", &year}, {"score", &score}, {"fresh", &fresh}};
    const std::vector<cdb_index*> strings{title.gpu_index(), body.gpu_index()};
    const std::vector<cdb_column*> columns{year.column(), score.column(), fresh.column()};
    const auto count_all = [&] { return cdb_shim::rowset::everything(strings, columns).size(); };
    CHECK(count_all() == 40);

    // ---- the reference's three messages ----------------------------------------------------------------------------------------
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"title", var(std::string("x"))}}}, {8, object{}}}, fields); }) == "Empty objects are not allowed");
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"", var(std::string("x"))}}}}, fields); }) == "Empty keys are not allowed");
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"year", var(std::string("1999"))}}}}, fields); }) == "Mismatched type for \"year\"");
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"title", var(int64_t(3))}}}}, fields); }) == "Mismatched type for \"title\"");
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"score", var(int64_t(3))}}}}, fields); }) == "Mismatched type for \"score\"");
    // the two refusals of this header's own: a key no field of the map has (the reference would create its index), a key named twice
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"title", var(std::string("x"))}, {"price", var(int64_t(3))}}}}, fields); }) ==
          "insert: field \"price\" is not in the field map");
    CHECK(thrown([&] { cdb_shim::insert({{7, object{{"year", var(int64_t(1))}, {"title", var(std::string("x"))}, {"year", var(int64_t(2))}}}}, fields); }) ==
          "Duplicate key \"year\" in one object");
    CHECK(count_all() == 40);

    // ---- the batch: ids descending, below, between and above the old ones ---------------------------------------------------------
    std::vector<cdb_shim::insert_object> batch;
    std::map<int64_t, object> model;
    const int64_t ids[] = {500, 141, 99, -3};
    for (int k = 0; k < 4; ++k) {
        object o;
        o.emplace_back("title", var(std::string("new roast #") + std::to_string(k)));
        if (k != 1) o.emplace_back("body", var(std::string(k == 2 ? "" : "about crema")));
        if (k != 2) o.emplace_back("year", var(int64_t(2020 + k)));
        if (k == 0) o.emplace_back("score", var(2.75));
        o.emplace_back("fresh", var(k % 2 == 0));
        batch.emplace_back(ids[k], o);
        model.emplace(ids[k], o);
    }

    // an id a field of the call already holds: the library's text, nothing changed
    {
        auto held = batch;
        held[2].first = 116;  // (body holds the odd ids only; std::map order of the names: body, fresh, ...)
        CHECK(thrown([&] { cdb_shim::insert(held, fields); }) == "cdb_insert_objects: object id 116 is already held by field 1");
        held[2].first = 500;
        CHECK(thrown([&] { cdb_shim::insert(held, fields); }) == "cdb_insert_objects: object id 500 twice in the batch");
    }
    // a failing field: "field <i>: ..." in std::map order of the names (body, fresh, score, title, year), and every field as before
    const auto before_title = title.query("coffee");
    const auto before_year = year.query("[-inf,inf]");
    CHECK(cdb_debug_column_set_option(score.column(), "debug_fail_append_prepare", 1) == CDB_OK);
    CHECK(thrown([&] { cdb_shim::insert(batch, fields); }) == "field 2: debug: append prepare failure requested (test hook)");
    CHECK(cdb_debug_column_set_option(score.column(), "debug_fail_append_prepare", 0) == CDB_OK);
    CHECK(title.query("coffee") == before_title && year.query("[-inf,inf]") == before_year && title.query("roast").empty());
    CHECK(count_all() == 40);

    // ---- the insert ------------------------------------------------------------------------------------------------------------
    const auto res = cdb_shim::insert(batch, fields);
    CHECK(res.size() == 5);
    const char* names[] = {"body", "fresh", "score", "title", "year"};
    const uint64_t joined[] = {3, 4, 1, 4, 3};
    for (size_t k = 0; k < res.size() && k < 5; ++k)
        CHECK(res[k].first == names[k] && res[k].second.appended == joined[k] && res[k].second.status == CDB_OK && res[k].second.committed == 1);
    CHECK(count_all() == 44);
    CHECK(title.query("roast").size() == 4 && title.query("coffee") == before_title);
    CHECK(body.query("crema").size() == 2);
    CHECK(year.query("[2020,2030]").size() == 10 + 3 && year.query("[2030,2100]").empty() &&year.query("[-inf,inf]").size() == before_year.size() + 3);
    CHECK(score.query("[2.75,2.75]").size() == 1 && fresh.query("true").size() == 10 + 2);

    // read back by select: every inserted object comes out with the fields it was given, in std::map order of the names
    cdb_shim::rowset all = cdb_shim::rowset::everything(strings, columns);
    const auto objects = cdb_shim::select(all, 0, UINT64_MAX, fields, {}, {}, "", "");
    CHECK(objects.size() == 44);
    // rows ascend by id: -3, 99, then the old ones, 141, 500
    const size_t at[] = {43, 42, 1, 0};  // where batch[k] stands
    for (int k = 0; k < 4 && objects.size() == 44; ++k) {
        std::map<std::string, var> want(model.at(ids[k]).begin(), model.at(ids[k]).end());
        std::map<std::string, var> got(objects[at[k]].begin(), objects[at[k]].end());
        CHECK(got == want);
    }

    std::printf(failures ? "FAILED %d\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
