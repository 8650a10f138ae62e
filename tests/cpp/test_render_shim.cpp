// string_index::render_rows through the reference-side binding (coffeedb_amd/csrc/shim/index.h), driven the way select()
// (database.cpp:394-441) would: a page in rank order, one id the index lacks, a repeated id — every string equal to
// cdb_shim::render_spans (highlight.h) applied to highlight_spans, the whole-column path.
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "highlight.h"
#include "index.h"

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                             \
        }                                                           \
    } while (0)

int main() {
    std::map<int64_t, std::string> store = {{100, "3010103"}, {101, "xx3010"}, {102, "01011010"}, {103, ""}, {104, "no digits here"},
                                            {105, "0101010101 and 3 and 010"}, {106, std::string(9000, '0') + "1" + std::string(50, '0')}};
    auto sp = std::make_unique<string_index>();
    for (const auto& [id, text] : store) sp->add(id, text);
    sp->build();
    const std::vector<std::string> keywords = {"010", "3", "00"};
    std::map<int64_t, cdb_shim::spans_t> spans_of;
    for (auto& [id, spans] : sp->highlight_spans(keywords)) spans_of[id] = spans;
    // the page: rank order (not id order), an id the index lacks, a repeat
    const index::result_type page = {{105, 9}, {102, 4}, {999, 1}, {100, 3}, {106, 2}, {104, 0}, {103, 0}, {102, 4}, {101, 1}};
    for (const auto& [left, right] : std::vector<std::pair<std::string, std::string>>{{"<b>", "</b>"}, {"", "]"}, {"[", ""}}) {
        const auto got = sp->render_rows(page, keywords, left, right);
        CHECK(got.size() == page.size());
        for (size_t i = 0; i < page.size() && i < got.size(); ++i) {
            const int64_t id = page[i].first;
            if (!store.count(id)) {
                CHECK(!got[i].has_value());
                continue;
            }
            CHECK(got[i].has_value());
            if (got[i]) CHECK(*got[i] == cdb_shim::render_spans(store[id], spans_of[id], left, right));
        }
    }
    {  // README.md:107-110, and select without highlight
        const auto one = sp->render_rows({{100, 1}}, {"010"}, "<b>", "</b>");
        CHECK(one.size() == 1 && one[0] && *one[0] == "3<b>01010</b>3");
        const auto plain = sp->render_rows(page, {}, "<b>", "</b>");
        for (size_t i = 0; i < page.size(); ++i) CHECK(store.count(page[i].first) ? (plain[i] && *plain[i] == store[page[i].first]) : !plain[i]);
        CHECK(sp->render_rows({}, keywords, "<", ">").empty());
    }
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
