// cdb_shim::select (coffeedb_amd/csrc/shim/select.h) driven the way interface.cpp:181-248 drives select(): a database.cpp-style
// caller keeps its objects in std::map, builds one index per field — two string fields, an int64 field, a bool field; the numeric
// ones on the GPU (COFFEEDB_GPU_NUMERIC=1) — filters once into a row set and runs the README's query shapes.  Every answer is compared
// with database.cpp:394-441 restated here over the caller's own objects.
#include <algorithm>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <variant>
#include <vector>

#include "index.h"
#include "select.h"

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                             \
        }                                                           \
    } while (0)

using cdb_shim::constraint_list;
using cdb_shim::object_type;
using cdb_shim::var;
using rows_t = std::vector<std::pair<int64_t, int64_t>>;
using store_t = std::map<int64_t, std::map<std::string, var>>;

// ac_automaton::render (database.cpp:58-90): at every end position the longest keyword that ends there
static std::string render(const std::string& text, const std::vector<std::string>& keywords, const std::string& left, const std::string& right) {
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    for (uint64_t i = 0; i < text.size(); ++i) {
        uint64_t length = 0;
        for (const auto& k : keywords)
            if (k.size() <= i + 1 && k.size() > length && text.compare(i + 1 - k.size(), k.size(), k) == 0) length = k.size();
        if (!length) continue;
        const uint64_t begin = i - length + 1;
        while (spans.size() && begin <= spans.back().first) spans.pop_back();
        if (spans.size() && begin <= spans.back().second) spans.back().second = i;
        else spans.emplace_back(begin, i);
    }
    std::string ret;
    auto iter = spans.begin();
    for (uint64_t i = 0; i < text.size(); ++i) {
        if (iter != spans.end() && i == iter->first) ret += left;
        ret += text[i];
        if (iter != spans.end() && i == iter->second) {
            ret += right;
            ++iter;
        }
    }
    return ret;
}

// database.cpp:394-441 over the caller's objects; string_keys: the fields that are string indexes (renderer, :145-151)
static std::vector<object_type> model_select(const store_t& data, const rows_t& results, const std::vector<std::string>& keys,
                                             const constraint_list& constraints, const std::string& left, const std::string& right) {
    std::map<std::string, std::vector<std::string>> automatons;
    for (const auto& [key, keywords] : constraints) automatons.emplace(key, keywords);
    auto transform = [&](const std::string& key, const var& v) -> var {
        if (const auto* s = std::get_if<std::string>(&v); s && automatons.count(key)) return render(*s, automatons.at(key), left, right);
        return v;
    };
    const bool flag = keys.empty() || std::find(keys.begin(), keys.end(), "$correlation") != keys.end();
    std::vector<object_type> ret;
    static const std::map<std::string, var> none;
    for (auto [id, correlation] : results) {
        const auto found = data.find(id);
        const auto& obj = found == data.end() ? none : found->second;
        object_type object;
        auto put = [&](const std::string& key, const var& v) { object.emplace_back(key, constraints.size() ? transform(key, v) : v); };
        if (keys.size()) {
            for (const auto& key : keys)
                if (auto it = obj.find(key); it != obj.end()) put(key, it->second);
        } else {
            for (const auto& kv : obj) put(kv.first, kv.second);
        }
        if (correlation && flag) object.emplace_back("$correlation", var((int64_t)correlation));
        if (object.size()) ret.push_back(std::move(object));
    }
    return ret;
}

// interface.cpp:144-146 with the project's tie rule (ascending id), then `span` (:228-241)
static rows_t model_page(rows_t rows, uint64_t first, uint64_t last) {
    std::stable_sort(rows.begin(), rows.end(), [](const auto& a, const auto& b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });
    if (first >= rows.size()) return {};
    return rows_t(rows.begin() + first, rows.begin() + std::min<uint64_t>(last, rows.size()));
}

int main() {
    // some twenty objects with differing field sets; ids are not in insertion order for the indexes (descending adds below)
    store_t data;
    const char* secrets[] = {"3010103", "301022", "0101010", "", "no digits", "010 and 010", "33", "x010x", "0100", "10101"};
    for (int i = 0; i < 21; ++i) {
        const int64_t id = 5000 + 37 * i;
        auto& obj = data[id];
        if (i % 7 != 6) obj["secret"] = std::string(secrets[i % 10]);
        if (i % 3 != 1) obj["name"] = std::string(i % 2 ? "yulemao" : "sunkafei") + std::to_string(i);
        if (i % 5 != 4) obj["number"] = (int64_t)(i % 4 == 0 ? -100 * i : 100 + 11 * i);
        if (i % 4 != 3) obj["flag"] = i % 3 == 0;
    }
    data[9000]["position"] = 1.7724;  // an object none of the four fields holds
    auto secret = std::make_unique<string_index>();
    auto name = std::make_unique<string_index>();
    auto number = std::make_unique<integer_index>();
    auto flag = std::make_unique<bool_index>();
    if (!number->column() || !flag->column()) {
        std::printf("FAILED: the numeric indexes are not on the GPU (COFFEEDB_GPU_NUMERIC=1)\n");
        return 1;
    }
    for (auto it = data.rbegin(); it != data.rend(); ++it) {
        const auto& [id, obj] = *it;
        if (auto f = obj.find("secret"); f != obj.end()) secret->add(id, std::get<std::string>(f->second));
        if (auto f = obj.find("name"); f != obj.end()) name->add(id, std::get<std::string>(f->second));
        if (auto f = obj.find("number"); f != obj.end()) number->add(id, std::get<int64_t>(f->second));
        if (auto f = obj.find("flag"); f != obj.end()) flag->add(id, std::get<bool>(f->second));
    }
    secret->build();
    name->build();
    number->build();
    flag->build();
    const cdb_shim::field_map fields = {{"secret", secret.get()}, {"name", name.get()}, {"number", number.get()}, {"flag", flag.get()}};

    // filter() for {"secret": "010", "number": "[-5000,900]"}: the string key resolved as the shim resolves it on one GPU and on
    // several (query_any), the column joined on the device
    const std::vector<std::string> kw = {"010"};
    const rows_t string_rows = secret->query_any(kw);
    std::vector<int64_t> r_ids, r_counts;
    for (auto [id, c] : string_rows) {
        r_ids.push_back(id);
        r_counts.push_back(c);
    }
    cdb_key_query key{};
    key.ids = r_ids.data();
    key.counts = r_counts.data();
    key.nrows = r_ids.size();
    const std::string range = "[-5000,900]";
    const uint64_t range_off[2] = {0, range.size()};
    cdb_column_key col{number->column(), range.data(), range_off, 1};
    cdb_rowset* h = nullptr;
    CHECK(cdb_filter(&key, 1, &col, 1, 0, 0, 0, &h) == CDB_OK && h);
    if (!h) {
        std::printf("FAILED\n");
        return 1;
    }
    cdb_shim::rowset rs(h);
    const rows_t all = rs.all();
    CHECK(all.size() >= 5);
    {  // the rows themselves, against the objects
        rows_t want;
        for (const auto& [id, obj] : data) {
            auto s = obj.find("secret");
            auto n = obj.find("number");
            if (s == obj.end() || n == obj.end()) continue;
            const std::string& t = std::get<std::string>(s->second);
            int64_t occ = 0;
            for (size_t p = 0; p + 3 <= t.size(); ++p) occ += t.compare(p, 3, "010") == 0;
            const int64_t v = std::get<int64_t>(n->second);
            if (occ && v >= -5000 && v <= 900) want.emplace_back(id, occ);
        }
        CHECK(all == want);
    }
    const constraint_list constraints = {{"secret", kw}, {"number", {range}}};
    const uint64_t m = all.size();
    struct Span { uint64_t first, last; };
    const std::vector<Span> spans = {{0, UINT64_MAX}, {0, 1}, {m - 1, m}, {1, 3}, {m, m + 4}, {0, m + 9}};
    const std::vector<std::vector<std::string>> key_lists = {{}, {"name", "secret"}, {"name"}, {"secret", "$correlation", "number"}, {"flag", "nowhere", "flag"},
                                                             {"$correlation"}, {"position"}};
    for (const Span& sp : spans)
        for (const auto& keys : key_lists) {
            const rows_t page = model_page(all, sp.first, sp.last);
            // README.md:93-110: with highlight the constraints reach select()
            CHECK(cdb_shim::select(rs, sp.first, sp.last, fields, keys, constraints, "<b>", "</b>") == model_select(data, page, keys, constraints, "<b>", "</b>"));
            // README.md:53-92: without highlight interface.cpp:225-227 clears them
            CHECK(cdb_shim::select(rs, sp.first, sp.last, fields, keys, {}, "", "") == model_select(data, page, keys, {}, "", ""));
        }
    {  // README.md:107-110 literally: object 5000 holds "3010103" and is ranked first (two occurrences)
        const auto got = cdb_shim::select(rs, 0, UINT64_MAX, fields, {"secret"}, constraints, "<b>", "</b>");
        bool seen = false;
        for (const auto& object : got) seen |= object.size() == 1 && object[0].second == var(std::string("3<b>01010</b>3"));
        CHECK(seen);
    }
    {  // a constraint on a field that is no string index renders nothing; two string fields with their own keyword lists
        const constraint_list two = {{"name", {"sun", "mao1"}}, {"secret", {"0", "10"}}, {"flag", {"true"}}};
        CHECK(cdb_shim::select(rs, 0, UINT64_MAX, fields, {}, two, "[", "]") == model_select(data, model_page(all, 0, UINT64_MAX), {}, two, "[", "]"));
    }
    {  // an empty keyword is refused with the reference's words
        bool threw = false;
        try {
            (void)cdb_shim::select(rs, 0, 5, fields, {}, {{"secret", {""}}}, "<", ">");
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()) == "Empty keywords are not allowed";
        }
        CHECK(threw);
    }
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
