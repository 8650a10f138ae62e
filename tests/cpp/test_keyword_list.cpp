// The keyword-list pieces every query entry point shares (coffeedb_amd/csrc/keyword_list.h) on their own: the checks, the rebase
// onto the first byte and the rebase that drops empty keywords, each against a naive restatement written here.  Host code only;
// tests/test_keyword_list_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../coffeedb_amd/csrc/keyword_list.h"

namespace {

using Offs = std::vector<uint64_t>;
int failures = 0;
int checks = 0;

void fail(const std::string& name, const std::string& what) {
    std::printf("FAIL %s: %s\n", name.c_str(), what.c_str());
    ++failures;
}

// ---- the travelling form, restated: cut every keyword out as a string, then lay the strings end to end -------------------------
std::vector<std::string> cut(const std::string& blob, const Offs& off, bool drop_empty) {
    std::vector<std::string> kws;
    for (size_t j = 0; j + 1 < off.size(); ++j) {
        if (off[j + 1] <= off[j]) {
            if (!drop_empty) kws.emplace_back();
            continue;
        }
        kws.push_back(blob.substr(off[j], off[j + 1] - off[j]));
    }
    return kws;
}
void expect_travels(const std::string& name, const cdb::Rebased& r, const std::vector<std::string>& want) {
    ++checks;
    std::string all;
    Offs rel{0};
    for (const std::string& k : want) {
        all += k;
        rel.push_back(all.size());
    }
    if (r.rel != rel) return fail(name, "relative offsets differ");
    if (r.n() != want.size()) return fail(name, "n() = " + std::to_string(r.n()));
    if (r.nbytes != all.size()) return fail(name, "nbytes = " + std::to_string(r.nbytes));
    if (r.nbytes && std::string(r.bytes, r.nbytes) != all) return fail(name, "bytes differ");
}
void check_rebase(const std::string& name, const std::string& blob, const Offs& off) {
    const cdb::KeywordList k{blob.data(), off.data(), off.size() - 1};
    expect_travels(name, cdb::rebase(k), cut(blob, off, false));
    if (off.size() > 1 && cdb::rebase(k).bytes != blob.data() + off[0]) fail(name, "the bytes were copied or moved");
}
void check_nonempty(const std::string& name, const std::string& blob, const Offs& off) {
    const cdb::KeywordList k{blob.data(), off.data(), off.size() - 1};
    std::string store = "left over from an earlier call";
    const cdb::Rebased r = cdb::rebase_nonempty(k, store);
    expect_travels(name, r, cut(blob, off, true));
    if (r.bytes != store.data() || r.nbytes != store.size()) fail(name, "the bytes do not live in the store");
}

// ---- the checks, restated: the first of the four conditions, in their fixed order, that the entry point asked for ----------------
std::string refusal_referee(const cdb::KeywordList& k, const std::string& who, unsigned checks_) {
    if ((checks_ & cdb::KW_LIST_NOT_EMPTY) && k.n == 0) return "The constraint list cannot be empty";
    if ((checks_ & cdb::KW_OFFSETS) && k.off == nullptr) return who + ": keyword offsets missing";
    if (checks_ & cdb::KW_NONE_EMPTY) {
        bool empty = false;
        for (uint64_t j = 0; j < k.n; ++j) empty = empty || !(k.off[j] < k.off[j + 1]);
        if (empty) return "Empty keywords are not allowed";
    }
    if ((checks_ & cdb::KW_BYTES) && k.n != 0 && k.blob == nullptr) return who + ": keywords without bytes";
    return "";
}
std::string refusal(const cdb::KeywordList& k, const char* who, unsigned checks_) {
    try {
        cdb::check_keywords(k, who, checks_);
    } catch (const cdb::Error& e) {
        if (e.status != cdb::Status::Invalid) return std::string("(status ") + std::to_string((int)e.status) + ") " + e.what();
        return e.what();
    }
    return "";
}
// the flag combinations the entry points use: batch (+ shards batch); OR / ranked; the three ANDs; render and select
const unsigned USED[] = {cdb::KW_NONE_EMPTY, cdb::KW_LIST_NOT_EMPTY | cdb::KW_NONE_EMPTY,
                         cdb::KW_LIST_NOT_EMPTY | cdb::KW_OFFSETS | cdb::KW_NONE_EMPTY, cdb::KW_NONE_EMPTY | cdb::KW_BYTES};
void check_refusals(const std::string& name, const cdb::KeywordList& k) {
    for (unsigned c : USED)
        for (const char* who : {"cdb_query_and", "cdb_render_rows"}) {
            ++checks;
            const std::string got = refusal(k, who, c), want = refusal_referee(k, who, c);
            if (got != want) fail(name + " checks=" + std::to_string(c) + " who=" + who, "got '" + got + "', want '" + want + "'");
        }
}
void expect_refusal(const std::string& name, const cdb::KeywordList& k, const char* who, unsigned c, const std::string& want) {
    ++checks;
    const std::string got = refusal(k, who, c);
    if (got != want) fail(name, "got '" + got + "', want '" + want + "'");
}

}  // namespace

int main() {
    const std::string blob = "junk...coffeeteamilk!!tail";
    // ---- rebase: base 0 and a base behind junk, one keyword, no keyword
    check_rebase("base 0", "coffeeteamilk", Offs{0, 6, 9, 13});
    check_rebase("base 7", blob, Offs{7, 13, 16, 20});
    check_rebase("one keyword", blob, Offs{16, 20});
    check_rebase("one keyword at 0", "x", Offs{0, 1});
    {
        ++checks;
        const cdb::Rebased none = cdb::rebase(cdb::KeywordList{nullptr, nullptr, 0});
        if (none.rel != Offs{0} || none.n() != 0 || none.nbytes != 0) fail("no keyword", "not {0}");
        const Offs lone{5};  // (a batch of no patterns may still come with an offset array)
        const cdb::Rebased none2 = cdb::rebase(cdb::KeywordList{blob.data(), lone.data(), 0});
        if (none2.rel != Offs{0} || none2.nbytes != 0) fail("no keyword, offsets given", "not {0}");
    }
    // ---- the dropping rebase: nothing to drop, first and last empty, an empty one between, decreasing offsets, all empty, none
    check_nonempty("nothing empty", blob, Offs{7, 13, 16, 20});
    check_nonempty("first and last empty", blob, Offs{7, 7, 13, 16, 16});
    check_nonempty("middle empty", blob, Offs{7, 13, 13, 16});
    check_nonempty("decreasing", blob, Offs{7, 13, 9, 16});
    check_nonempty("all empty", blob, Offs{7, 7, 7});
    check_nonempty("no keyword", blob, Offs{7});
    {
        ++checks;
        std::string store;
        const cdb::Rebased none = cdb::rebase_nonempty(cdb::KeywordList{nullptr, nullptr, 0}, store);
        if (none.rel != Offs{0} || none.nbytes != 0) fail("dropping, null list", "not {0}");
    }
    // ---- the checks against the restatement: sound lists, equal and decreasing offsets, no list, no offsets, no bytes
    const Offs good{7, 13, 16, 20}, equal{7, 13, 13, 20}, equal_first{7, 7, 13}, equal_last{7, 13, 13}, decreasing{7, 13, 9, 20}, lone{7};
    check_refusals("good", cdb::KeywordList{blob.data(), good.data(), 3});
    check_refusals("equal offsets", cdb::KeywordList{blob.data(), equal.data(), 3});
    check_refusals("first empty", cdb::KeywordList{blob.data(), equal_first.data(), 2});
    check_refusals("last empty", cdb::KeywordList{blob.data(), equal_last.data(), 2});
    check_refusals("decreasing offsets", cdb::KeywordList{blob.data(), decreasing.data(), 3});
    check_refusals("empty list", cdb::KeywordList{blob.data(), lone.data(), 0});
    check_refusals("empty list, nothing given", cdb::KeywordList{nullptr, nullptr, 0});
    check_refusals("no bytes", cdb::KeywordList{nullptr, good.data(), 3});
    check_refusals("no bytes, an empty keyword", cdb::KeywordList{nullptr, equal.data(), 3});
    // (offsets missing with keywords announced is only ever asked together with KW_OFFSETS in front of the walk over them)
    for (const char* who : {"cdb_query_and", "cdb_shards_query_and"}) {
        const cdb::KeywordList k{blob.data(), nullptr, 3};
        const unsigned c = cdb::KW_LIST_NOT_EMPTY | cdb::KW_OFFSETS | cdb::KW_NONE_EMPTY;
        expect_refusal(std::string("no offsets ") + who, k, who, c, refusal_referee(k, who, c));
    }
    // ---- every message, literally, under two names; and where two checks fire on one input, the order the entry points have
    const unsigned AND = cdb::KW_LIST_NOT_EMPTY | cdb::KW_OFFSETS | cdb::KW_NONE_EMPTY, RENDER = cdb::KW_NONE_EMPTY | cdb::KW_BYTES;
    expect_refusal("literal: empty list", cdb::KeywordList{blob.data(), lone.data(), 0}, "a", AND, "The constraint list cannot be empty");
    expect_refusal("literal: offsets a", cdb::KeywordList{blob.data(), nullptr, 2}, "cdb_query_and", AND, "cdb_query_and: keyword offsets missing");
    expect_refusal("literal: offsets b", cdb::KeywordList{blob.data(), nullptr, 2}, "cdb_query_and_columns", AND,
                   "cdb_query_and_columns: keyword offsets missing");
    expect_refusal("literal: empty keyword", cdb::KeywordList{blob.data(), equal.data(), 3}, "a", AND, "Empty keywords are not allowed");
    expect_refusal("literal: bytes a", cdb::KeywordList{nullptr, good.data(), 3}, "cdb_render_rows", RENDER, "cdb_render_rows: keywords without bytes");
    expect_refusal("literal: bytes b", cdb::KeywordList{nullptr, good.data(), 3}, "cdb_rowset_select", RENDER,
                   "cdb_rowset_select: keywords without bytes");
    expect_refusal("order: empty list before missing offsets", cdb::KeywordList{nullptr, nullptr, 0}, "a", AND, "The constraint list cannot be empty");
    expect_refusal("order: empty keyword before missing bytes", cdb::KeywordList{nullptr, equal.data(), 3}, "a", RENDER,
                   "Empty keywords are not allowed");
    // a check that was not asked for does not fire: a batch may be empty, and only render and select look at the blob
    expect_refusal("batch: empty list passes", cdb::KeywordList{nullptr, nullptr, 0}, "a", cdb::KW_NONE_EMPTY, "");
    expect_refusal("batch: null blob passes", cdb::KeywordList{nullptr, good.data(), 3}, "a", cdb::KW_NONE_EMPTY, "");
    expect_refusal("and: null blob passes", cdb::KeywordList{nullptr, good.data(), 3}, "a", AND, "");
    expect_refusal("render: empty list passes", cdb::KeywordList{nullptr, nullptr, 0}, "a", RENDER, "");

    if (failures) {
        std::printf("%d of %d checks failed\n", failures, checks);
        return 1;
    }
    std::printf("OK %d checks\n", checks);
    return 0;
}
