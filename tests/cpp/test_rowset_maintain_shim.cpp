// cdb_shim::rowset::remove and rowset::everything as a database.cpp-style caller uses them: objects with two string fields and an
// integer field (not every object has every field) live in std::map objects here and in GPU indexes there.
//   remove   by constraints (interface.cpp:274-285): filter() over title keyword AND year range -> a row set -> remove from all three
//            fields in one call; every field must then answer like the model without those objects
//   count    without constraints (interface.cpp:289-301 over query(), database.cpp:380-386): everything(...).size()
//   query    without constraints, with `span` and fields: cdb_shim::select over everything(...)
//   failure  a failing field is rethrown as std::runtime_error with the library's text, and nothing has changed
// usage: COFFEEDB_GPU_NUMERIC=1 test_rowset_maintain_shim
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "index.h"
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

struct Object {
    bool has_title = false, has_body = false, has_year = false;
    std::string title, body;
    int64_t year = 0;
};

static const int N = 600;
static const char* WORDS[] = {"coffee", "bean", "roast", "grinder", "filter", "crema", "arabica"};

static std::map<int64_t, Object> make_objects() {
    std::map<int64_t, Object> data;
    for (int i = 0; i < N; ++i) {
        Object o;
        const int64_t id = (int64_t)((i * 389) % N) * 5 - 700;  // shuffled insertion order is up to the caller; negative ids among them
        o.has_title = i % 7 != 0;
        o.has_body = i % 3 != 1;
        o.has_year = i % 5 != 2;
        o.title = std::string(WORDS[i % 7]) + " " + WORDS[(i / 7) % 7] + " #" + std::to_string(i);
        o.body = std::string("about ") + WORDS[(i * 3) % 7] + " and " + WORDS[(i * 5 + 1) % 7];
        o.year = 1990 + (i * 13) % 40;
        if (!o.has_title && !o.has_body && !o.has_year) o.has_year = true;
        data.emplace(id, o);
    }
    return data;
}

static index::result_type model_query(const std::map<int64_t, Object>& data, bool title, const std::string& kw) {
    index::result_type out;
    for (const auto& [id, o] : data) {
        if (title ? !o.has_title : !o.has_body) continue;
        const std::string& text = title ? o.title : o.body;
        int64_t count = 0;
        for (size_t p = text.find(kw); p != std::string::npos; p = text.find(kw, p + 1)) ++count;
        if (count) out.emplace_back(id, count);
    }
    return out;
}
static index::result_type sorted_by_id(index::result_type r) {
    std::sort(r.begin(), r.end());
    return r;
}

int main() {
    std::map<int64_t, Object> data = make_objects();
    string_index title, body;
    integer_index year;
    CHECK(title.gpu_index() && body.gpu_index() && year.column());
    if (failures) return 1;
    for (const auto& [id, o] : data) {  // (the strings live in `data` until the program ends: the indexes keep views)
        if (o.has_title) title.add(id, o.title);
        if (o.has_body) body.add(id, o.body);
        if (o.has_year) year.add(id, o.year);
    }
    title.build();
    body.build();
    year.build();
    const std::vector<cdb_index*> strings{title.gpu_index(), body.gpu_index()};
    const std::vector<cdb_column*> columns{year.column()};

    // ---- count and query without constraints ---------------------------------------------------------------------------------
    {
        cdb_shim::rowset all = cdb_shim::rowset::everything(strings, columns);
        CHECK(all.size() == data.size());
        const auto page = all.page(10, 25);
        CHECK(page.size() == 15);
        auto it = data.begin();
        std::advance(it, 10);
        for (size_t r = 0; r < page.size(); ++r, ++it) CHECK(page[r].first == it->first && page[r].second == 0);
        const cdb_shim::field_map fields{{"title", &title}, {"body", &body}, {"year", &year}};
        const auto objects = cdb_shim::select(all, 10, 25, fields, {"year", "title"}, {}, "", "");
        it = data.begin();
        std::advance(it, 10);
        size_t k = 0;
        for (int r = 0; r < 15; ++r, ++it) {
            const Object& o = it->second;
            if (!o.has_year && !o.has_title) continue;  // (a row whose object comes out empty is dropped)
            CHECK(k < objects.size());
            if (k >= objects.size()) break;
            const cdb_shim::object_type& got = objects[k++];
            size_t f = 0;
            if (o.has_year) {
                CHECK(f < got.size() && got[f].first == "year" && std::get<int64_t>(got[f].second) == o.year);
                ++f;
            }
            if (o.has_title) {
                CHECK(f < got.size() && got[f].first == "title" && std::get<std::string>(got[f].second) == o.title);
                ++f;
            }
            CHECK(f == got.size());  // (count 0: no $correlation)
        }
        CHECK(k == objects.size());
        // one field alone is the ids that field holds
        cdb_shim::rowset years = cdb_shim::rowset::everything({}, columns);
        size_t with_year = 0;
        for (const auto& kv : data) with_year += kv.second.has_year;
        CHECK(years.size() == with_year);
    }

    // ---- remove by constraints -----------------------------------------------------------------------------------------------
    const std::string kw = "coffee", range = "[1995,2015]";
    const uint64_t kw_offsets[2] = {0, kw.size()}, range_offsets[2] = {0, range.size()};
    cdb_key_query key{};
    key.index = title.gpu_index();
    key.blob = kw.data();
    key.offsets = kw_offsets;
    key.nkw = 1;
    cdb_column_key ckey{};
    ckey.column = year.column();
    ckey.blob = range.data();
    ckey.offsets = range_offsets;
    ckey.nranges = 1;
    std::set<int64_t> doomed;
    for (const auto& [id, o] : data)
        if (o.has_title && o.title.find(kw) != std::string::npos && o.has_year && o.year >= 1995 && o.year <= 2015) doomed.insert(id);
    CHECK(!doomed.empty() && doomed.size() < data.size());
    cdb_rowset* raw = nullptr;
    CHECK(cdb_filter(&key, 1, &ckey, 1, 0, 0, 0, &raw) == CDB_OK);
    cdb_shim::rowset hit(raw);
    CHECK(hit.size() == doomed.size());
    const std::vector<cdb_remove_field> fields{cdb_shim::rowset::field_of(title.gpu_index()), cdb_shim::rowset::field_of(body.gpu_index()),
                                               cdb_shim::rowset::field_of(year.column())};

    // a failing field: the library's text, and every field as before
    const auto before_title = title.query("bean");
    const auto before_year = year.query("[-inf,inf]");
    CHECK(cdb_set_option(body.gpu_index(), "debug_fail_prepare", 1) == CDB_OK);
    bool threw = false;
    try {
        hit.remove(fields);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()) == "field 1: debug: prepare failure requested (test hook)";
        if (!threw) std::printf("unexpected text: %s\n", e.what());
    }
    CHECK(threw);
    CHECK(cdb_set_option(body.gpu_index(), "debug_fail_prepare", 0) == CDB_OK);
    CHECK(title.query("bean") == before_title && year.query("[-inf,inf]") == before_year);
    CHECK(sorted_by_id(body.query("about")) == model_query(data, false, "about"));

    // the same call again: every field loses the objects
    uint64_t rows = 0;
    const auto res = hit.remove(fields, &rows);
    CHECK(rows == doomed.size() && res.size() == 3);
    size_t in_body = 0;
    for (int64_t id : doomed) in_body += data.at(id).has_body;
    CHECK(res[0].removed == doomed.size() && res[0].missing == 0 && res[0].committed == 1 && res[0].status == CDB_OK);
    CHECK(res[1].removed == in_body && res[1].removed + res[1].missing == rows);
    CHECK(res[2].removed == doomed.size() && res[2].missing == 0 && res[2].committed == 1);
    for (int64_t id : doomed) data.erase(id);
    for (const char* w : WORDS) {
        CHECK(sorted_by_id(title.query(w)) == model_query(data, true, w));
        CHECK(sorted_by_id(body.query(w)) == model_query(data, false, w));
    }
    size_t with_year = 0;
    for (const auto& kv : data) with_year += kv.second.has_year;
    CHECK(year.query("[-inf,inf]").size() == with_year);
    for (const auto& row : year.query("[1995,2015]")) CHECK(!doomed.count(row.first));
    CHECK(cdb_shim::rowset::everything(strings, columns).size() == data.size());

    // no field at all is refused with a text
    threw = false;
    try {
        cdb_shim::rowset::everything({}, {});
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).rfind("cdb_rowset_all: ", 0) == 0;
    }
    CHECK(threw);

    std::printf(failures ? "FAILED %d\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
