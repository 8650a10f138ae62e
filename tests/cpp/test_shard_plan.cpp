// The planning arithmetic of a sharded column (coffeedb_amd/csrc/shard_plan.h) on its own: the shard count, the document-aligned
// bounds and the cuts of an appended batch, each against a naive restatement written here.  Host code only;
// tests/test_shard_plan_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../coffeedb_amd/csrc/shard_plan.h"

namespace {

using Vec = std::vector<uint64_t>;
int failures = 0;
int checks = 0;

std::string show(const Vec& v) {
    std::string s = "{";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "}";
}
void fail(const std::string& name, const std::string& what) {
    std::printf("FAIL %s: %s\n", name.c_str(), what.c_str());
    ++failures;
}
Vec starts_of(const Vec& lens) {
    Vec ds{0};
    for (uint64_t l : lens) ds.push_back(ds.back() + l);
    return ds;
}

// ---- bounds: a linear scan for the first document boundary >= floor(total * r / parts), clamped to be non-decreasing -------------
// floor(total * r / parts) without a wide product: total = q * parts + rem, so total * r / parts = q * r + rem * r / parts
uint64_t target_of(uint64_t total, uint64_t r, uint64_t parts) { return (total / parts) * r + (total % parts) * r / parts; }
Vec bounds_referee(const Vec& ds, int parts) {
    const uint64_t nd = ds.size() - 1;
    Vec b{0};
    for (int r = 1; r < parts; ++r) {
        const uint64_t t = target_of(ds[nd], (uint64_t)r, (uint64_t)parts);
        uint64_t d = 0;
        while (d < nd && ds[d] < t) ++d;
        b.push_back(std::max(d, b.back()));
    }
    b.push_back(nd);
    return b;
}
void check_bounds(const std::string& name, const Vec& ds, int parts) {
    ++checks;
    const Vec got = cdb::shard_bounds(ds, parts), want = bounds_referee(ds, parts);
    const uint64_t nd = ds.size() - 1;
    bool ok = got.size() == (size_t)parts + 1 && got.front() == 0 && got.back() == nd && std::is_sorted(got.begin(), got.end());
    if (!ok || got != want) fail(name + " parts=" + std::to_string(parts), "got " + show(got) + ", want " + show(want));
}

// ---- shard count ----------------------------------------------------------------------------------------------------------------
int count_referee(uint64_t total, uint64_t ndocs, int G, uint64_t limit, bool use_all) {
    uint64_t used = G;
    if (!use_all) {
        used = total / limit + (total % limit ? 1 : 0);  // the fewest shards of at most `limit` bytes
        if (used < 1) used = 1;
        if (used > (uint64_t)G) used = G;
    }
    if (ndocs >= 1 && used > ndocs) used = ndocs;  // a shard holds at least one document ...
    if (ndocs == 0) used = 1;                      // ... and a column without documents is one empty shard
    return (int)used;
}
void check_count(uint64_t total, uint64_t ndocs, int G, uint64_t limit, bool use_all, int want_literal = -1) {
    ++checks;
    const int got = cdb::shard_count(total, ndocs, G, limit, use_all), want = count_referee(total, ndocs, G, limit, use_all);
    if (got != want || got < 1 || got > G || (want_literal >= 0 && got != want_literal))
        fail("shard_count", "total=" + std::to_string(total) + " ndocs=" + std::to_string(ndocs) + " G=" + std::to_string(G) + " limit=" +
                                std::to_string(limit) + " use_all=" + std::to_string(use_all) + ": got " + std::to_string(got) + ", want " +
                                std::to_string(want_literal >= 0 ? want_literal : want));
}

// ---- append cuts: piece by piece — a piece takes its first document whatever its size, then every further one that keeps it within
// the limit; the last slot takes all that is left -------------------------------------------------------------------------------------
Vec cuts_referee(const Vec& ds, uint64_t limit, int slots) {
    const uint64_t nd = ds.size() - 1;
    Vec cut{0};
    uint64_t start = 0;
    for (int piece = 1; start < nd; ++piece) {
        uint64_t end = nd;
        if (piece < slots) {
            end = start + 1;
            while (end < nd && ds[end + 1] - ds[start] <= limit) ++end;
        }
        cut.push_back(end);
        start = end;
    }
    return cut;
}
void check_cuts(const std::string& name, const Vec& lens, uint64_t limit, int slots, const Vec* want_literal = nullptr) {
    ++checks;
    Vec ds = starts_of(lens);
    for (uint64_t& x : ds) x += 1000;  // (a batch's offsets need not start at 0)
    const uint64_t nd = lens.size();
    const Vec got = cdb::append_cuts(ds.data(), nd, limit, slots), want = cuts_referee(ds, limit, slots);
    bool ok = got.size() >= 2 && got.front() == 0 && got.back() == nd && got.size() - 1 <= (size_t)slots;
    for (size_t p = 0; ok && p + 1 < got.size(); ++p) {
        ok = got[p] < got[p + 1];                                                                      // strictly increasing
        if (ok && p + 2 < got.size()) ok = ds[got[p + 1]] - ds[got[p]] <= limit || got[p + 1] - got[p] == 1;  // all but the last piece
    }
    if (!ok || got != want || (want_literal && got != *want_literal))
        fail(name + " limit=" + std::to_string(limit) + " slots=" + std::to_string(slots),
             "got " + show(got) + ", want " + show(want_literal ? *want_literal : want));
}

}  // namespace

int main() {
    // ---- bounds ----
    for (int parts : {1, 2, 3, 8}) {
        check_bounds("no documents", Vec{0}, parts);
        check_bounds("only empty documents", Vec{0, 0, 0, 0, 0}, parts);
        check_bounds("one document", Vec{0, 17}, parts);
        check_bounds("more parts than documents", starts_of({5, 1, 9}), parts);
        check_bounds("even", starts_of(Vec(64, 10)), parts);
        check_bounds("giant at the front", starts_of({100000, 1, 2, 3, 1, 2, 3, 4}), parts);
        check_bounds("giant in the middle", starts_of({1, 2, 3, 100000, 1, 2, 3, 4}), parts);
        check_bounds("giant at the end", starts_of({1, 2, 3, 1, 2, 3, 4, 100000}), parts);
        check_bounds("empty documents at the targets", starts_of({4, 0, 0, 4, 0, 0, 4, 0, 0, 4}), parts);
    }
    {   // total * r around and beyond 2^64: synthetic offsets, nothing of that size exists.  With parts = 4, 2^64 / parts = 2^62, and the
        // product for the last cut (r = 3) wraps 64 bits from total = 2^64 / 3 on
        const uint64_t Q = 1ull << 62, T = ~0ull / 3;
        for (uint64_t total : Vec{Q - 1, Q + 1, T, T + 1, 3 * Q + 12345, ~0ull}) {
            const Vec ds{0, total / 7, total / 4, total / 4 + 1, total / 2 - 1, total / 2, total / 4 * 3 + 1, total - 1, total};
            for (int parts : {2, 3, 4, 7}) check_bounds("total " + std::to_string(total), ds, parts);
        }
        if ((uint64_t)((T + 1) * 3) >= T) fail("wide product", "the case does not wrap 64 bits");
    }
    std::mt19937_64 rng(20240611);
    for (int it = 0; it < 400; ++it) {
        const int nd = (int)(rng() % 60);
        Vec lens(nd);
        for (uint64_t& l : lens) {
            const uint64_t k = rng() % 10;
            l = k == 0 ? 0 : k == 1 ? rng() % 5000 : rng() % 40;  // ragged: empty documents, short ones, now and then a long one
        }
        check_bounds("random " + std::to_string(it), starts_of(lens), 1 + (int)(rng() % 9));
    }

    // ---- shard count ----
    for (bool use_all : {false, true})
        for (int G : {1, 3, 8})
            for (uint64_t limit : {1ull, 7ull, 100ull, 12ull << 30})
                for (uint64_t ndocs : {0ull, 1ull, 2ull, 5ull, 1000ull})
                    for (uint64_t total : Vec{0, 1, limit - 1, limit, limit + 1, 3 * limit, 3 * limit + 1, 100 * limit})
                        check_count(total, ndocs, G, limit, use_all);
    check_count(0, 0, 8, 100, false, 1);         // nothing at all: one empty shard
    check_count(0, 0, 8, 100, true, 1);
    check_count(0, 50, 8, 100, false, 1);        // only empty documents
    check_count(300, 50, 8, 100, false, 3);      // an exact multiple of the limit ...
    check_count(301, 50, 8, 100, false, 4);      // ... and one byte more
    check_count(5000, 50, 8, 100, false, 8);     // more wanted than there are slots
    check_count(5000, 3, 8, 100, false, 3);      // fewer documents than slots
    check_count(5000, 3, 8, 100, true, 3);
    check_count(10, 50, 8, 100, true, 8);        // use_all spreads a column that would fit one shard
    check_count(5, 50, 8, 1, false, 5);          // a limit of one byte

    // ---- append cuts ----
    const Vec one_piece{0, 5}, three{0, 2, 4, 6}, capped{0, 2, 4, 10}, four_empty{0, 4};
    check_cuts("everything fits in one piece", {10, 20, 30, 5, 5}, 100, 4, &one_piece);
    check_cuts("everything fits exactly", {10, 20, 30, 40}, 100, 4);
    check_cuts("exactly `slots` pieces", {50, 50, 50, 50, 50, 50}, 100, 3, &three);
    check_cuts("more pieces wanted than slots", {50, 50, 50, 50, 50, 50, 50, 50, 50, 50}, 100, 3, &capped);
    check_cuts("a large document at the front", {500, 10, 10, 10}, 100, 4);
    check_cuts("a large document in the middle", {10, 10, 500, 10, 10}, 100, 4);
    check_cuts("a large document at the end", {10, 10, 10, 500}, 100, 4);
    check_cuts("only large documents", {500, 600, 700, 800, 900}, 100, 4);
    check_cuts("empty documents at a cut", {60, 40, 0, 0, 1, 0, 99, 0, 0, 1}, 100, 5);
    check_cuts("only empty documents", {0, 0, 0, 0}, 100, 3, &four_empty);
    check_cuts("one document", {7}, 100, 3);
    for (int slots : {1, 2, 3, 7, 100}) {
        check_cuts("a limit of one byte", {1, 1, 0, 1, 2, 0, 0, 1}, 1, slots);
        check_cuts("ragged", {30, 30, 30, 30, 0, 100, 101, 1, 1, 98, 1, 50, 50, 50}, 100, slots);
    }
    for (int it = 0; it < 400; ++it) {
        Vec lens(1 + rng() % 40);
        for (uint64_t& l : lens) l = rng() % 8 == 0 ? 0 : rng() % 150;
        check_cuts("random " + std::to_string(it), lens, 1 + rng() % 200, 1 + (int)(rng() % 8));
    }

    // ---- the "missing" identity: ids are disjoint across shards, so every shard but the holder misses a held id ----
    for (int G : {1, 2, 5})
        for (uint64_t n : {0ull, 1ull, 1000ull})
            for (uint64_t held : Vec{0, n / 3, n}) {
                ++checks;
                const uint64_t sum = (uint64_t)(G - 1) * held + (uint64_t)G * (n - held);
                if (cdb::missing_in_all_shards(sum, G, n) != n - held) fail("missing", "G=" + std::to_string(G) + " n=" + std::to_string(n));
            }

    if (failures) {
        std::printf("%d of %d checks FAILED\n", failures, checks);
        return 1;
    }
    std::printf("OK: %d checks\n", checks);
    return 0;
}
