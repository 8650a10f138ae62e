// test_vl_code.cpp — the alphabetic code of the bucket-wise build's sort keys (vl_code.h) on the host alone: every code vl_build
// returns must be order-preserving, prefix-free and complete within VL_MAX_LEN bits, the tables made from it must decode every
// window to the one symbol whose word starts it, and its weighted length is judged against an O(n^3) dynamic program for the optimal
// alphabetic tree.  Plain C++, no HIP: g++ -std=c++17 -I coffeedb_amd/csrc tests/cpp/test_vl_code.cpp.
#include "vl_code.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

using namespace cdb;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d %s — ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            if (++g_failures > 20) std::exit(1);           \
        }                                                  \
    } while (0)

using Counts = std::vector<uint64_t>;  // [0] = END (documents), [1 .. sigma] = the symbols

// ---- the weight families ------------------------------------------------------------------------------------------------------------
const char* const FAMILY[] = {"uniform", "powers_of_two", "many_zeros", "harmonic", "doubling"};
constexpr int NFAMILY = 5;

Counts make_counts(int family, int sigma, std::mt19937_64& rng) {
    Counts c(sigma + 1);
    for (int i = 0; i <= sigma; ++i) {
        switch (family) {
        case 0: c[i] = 1 + rng() % 1000000; break;
        case 1: c[i] = 1ull << (rng() % 41); break;
        case 2: c[i] = rng() % 5 == 0 ? 1 + rng() % 1000 : 0; break;
        case 3: c[i] = 1000000000ull / (uint64_t)(i + 1); break;
        default: c[i] = 1ull << std::min(i, 50);
        }
    }
    if (family == 2) {
        // vl_build's collision rate is positive only when two symbols occur (one symbol alone collides with certainty, whatever its
        // word); the build passes the counts of symbols the text holds.  Two of them stay non-zero; END's count may be zero.
        const int a = 1 + (int)(rng() % sigma), b = 1 + (a + (int)(rng() % (sigma - 1))) % sigma;
        c[a] = 1 + rng() % 1000;
        c[b] = 1 + rng() % 1000;
    }
    return c;
}

// ---- the code itself ----------------------------------------------------------------------------------------------------------------
unsigned aligned(const VlCode& v, int i) { return (unsigned)v.bits[i] << (VL_MAX_LEN - v.len[i]); }

void check_code(const VlCode& v, const Counts& cnt, int sigma, const std::string& what) {
    const int n = sigma + 1;
    CHECK(v.nsyms == n, "%s: nsyms %d", what.c_str(), v.nsyms);
    unsigned kraft = 0;
    int mn = VL_MAX_LEN + 1, mx = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(v.len[i] >= 1 && v.len[i] <= VL_MAX_LEN, "%s: len[%d] = %d", what.c_str(), i, v.len[i]);
        if (v.len[i] < 1 || v.len[i] > VL_MAX_LEN) return;
        CHECK(v.bits[i] < (1u << v.len[i]), "%s: bits[%d] = %u does not fit %d bits", what.c_str(), i, v.bits[i], v.len[i]);
        kraft += 1u << (VL_MAX_LEN - v.len[i]);
        mx = std::max(mx, (int)v.len[i]);
        if (i > 0) mn = std::min(mn, (int)v.len[i]);
    }
    CHECK(v.bits[0] == 0, "%s: END's word is %u", what.c_str(), v.bits[0]);
    for (int i = 0; i + 1 < n; ++i) {
        CHECK(aligned(v, i) < aligned(v, i + 1), "%s: words %d and %d are not in order", what.c_str(), i, i + 1);
        CHECK((aligned(v, i + 1) >> (VL_MAX_LEN - v.len[i])) != v.bits[i], "%s: word %d is a prefix of word %d", what.c_str(), i, i + 1);
    }
    for (int i = 0; i < n; ++i)  // (prefix-free among all pairs, not neighbours only)
        for (int j = 0; j < n; ++j)
            if (i != j && v.len[i] <= v.len[j])
                CHECK((v.bits[j] >> (v.len[j] - v.len[i])) != v.bits[i], "%s: word %d is a prefix of word %d", what.c_str(), i, j);
    CHECK(kraft == (1u << VL_MAX_LEN), "%s: Kraft sum %u / %u", what.c_str(), kraft, 1u << VL_MAX_LEN);
    CHECK(v.end_len == v.len[0], "%s: end_len %d, len[0] %d", what.c_str(), v.end_len, v.len[0]);
    CHECK(v.max_len == mx, "%s: max_len %d, table %d", what.c_str(), v.max_len, mx);
    CHECK(v.min_len == mn, "%s: min_len %d, table %d", what.c_str(), v.min_len, mn);
    CHECK(v.rate > 0, "%s: rate %g", what.c_str(), v.rate);
    (void)cnt;
}

void check_tables(const VlCode& v, int sigma, const std::string& what) {
    uint8_t slot[260] = {0};
    for (int c = 1; c <= sigma; ++c) slot[c] = (uint8_t)(sigma - c);  // some permutation of the bucket slots 0 .. sigma - 1
    uint16_t sym[256], dec[1 << VL_MAX_LEN];
    for (auto& x : sym) x = 0xDEAD;
    for (auto& x : dec) x = 0xDEAD;
    vl_fill_tables(v, slot, sigma, sym, dec);
    for (unsigned w = 0; w < (1u << VL_MAX_LEN); ++w) {
        int owner = -1, owners = 0;
        for (int c = 0; c <= sigma; ++c)
            if ((w >> (VL_MAX_LEN - v.len[c])) == v.bits[c]) {
                owner = c;
                ++owners;
            }
        CHECK(owners == 1, "%s: window %u starts with %d words", what.c_str(), w, owners);
        if (owners != 1) return;
        const unsigned want = owner == 0 ? (0xFFu | ((unsigned)v.end_len << 8)) : ((unsigned)slot[owner] | ((unsigned)v.len[owner] << 8));
        CHECK(dec[w] == want, "%s: dec[%u] = %04x, symbol %d wants %04x", what.c_str(), w, dec[w], owner, want);
    }
    for (int c = 0; c < 256; ++c) {
        if (c > sigma) {
            CHECK(sym[c] == 0, "%s: sym[%d] = %04x beyond the alphabet", what.c_str(), c, sym[c]);
            continue;
        }
        CHECK((sym[c] & 0xFF) == v.bits[c] && (sym[c] >> 8) == v.len[c], "%s: sym[%d] = %04x", what.c_str(), c, sym[c]);
        if (c == 0) continue;
        // round trip: the symbol's own word, padded with zeros or with ones, decodes to its slot and its length
        const unsigned l = sym[c] >> 8, lo = (sym[c] & 0xFFu) << (VL_MAX_LEN - l), hi = lo | ((1u << (VL_MAX_LEN - l)) - 1u);
        CHECK((dec[lo] & 0xFF) == slot[c] && (dec[lo] >> 8) == l && dec[hi] == dec[lo], "%s: symbol %d does not round-trip", what.c_str(), c);
    }
}

// ---- optimality: dynamic programs over doubled integer weights (vl_build floors a zero count at one half), exact in 64 bits --------
constexpr uint64_t INF = ~0ull;
std::vector<uint64_t> doubled(const Counts& c) {
    std::vector<uint64_t> w(c.size());
    for (size_t i = 0; i < c.size(); ++i) w[i] = std::max<uint64_t>(2 * c[i], 1);
    return w;
}
// least weighted path length of an alphabetic tree over w whose leaves lie at most `limit` levels deep (INF: none)
uint64_t optimal_alphabetic(const std::vector<uint64_t>& w, int limit) {
    const int n = (int)w.size();
    std::vector<uint64_t> pre(n + 1, 0);
    for (int i = 0; i < n; ++i) pre[i + 1] = pre[i] + w[i];
    std::vector<std::vector<uint64_t>> prev(n, std::vector<uint64_t>(n, INF)), cur;
    for (int i = 0; i < n; ++i) prev[i][i] = 0;  // depth 0: single leaves only
    for (int d = 1; d <= limit; ++d) {
        cur.assign(n, std::vector<uint64_t>(n, INF));
        for (int i = 0; i < n; ++i) cur[i][i] = 0;
        for (int len = 2; len <= n; ++len)
            for (int i = 0; i + len <= n; ++i) {
                const int j = i + len - 1;
                uint64_t best = INF;
                for (int k = i; k < j; ++k)
                    if (prev[i][k] != INF && prev[k + 1][j] != INF) best = std::min(best, prev[i][k] + prev[k + 1][j]);
                if (best != INF) cur[i][j] = best + (pre[j + 1] - pre[i]);
            }
        if (cur == prev) break;  // deeper trees gain nothing any more
        prev.swap(cur);
    }
    return prev[0][n - 1];
}

struct Optimality {
    int judged = 0, fits = 0, limited = 0;
    double worst_ratio = 1.0;
    std::string worst_case;
};

void check_optimal(const VlCode& v, const Counts& cnt, const std::string& what, Optimality& o) {
    const std::vector<uint64_t> w = doubled(cnt);
    const int n = (int)w.size();
    uint64_t got = 0;
    for (int i = 0; i < n; ++i) got += w[i] * v.len[i];
    const uint64_t unlimited = optimal_alphabetic(w, n), limited = optimal_alphabetic(w, VL_MAX_LEN);
    CHECK(limited != INF && unlimited <= limited, "%s: the dynamic programs disagree", what.c_str());
    CHECK(got >= limited, "%s: weighted length %llu beats the depth-%d optimum %llu", what.c_str(), (unsigned long long)got, VL_MAX_LEN,
          (unsigned long long)limited);
    ++o.judged;
    if (limited == unlimited) {  // the unlimited optimum already fits: Garsia-Wachs must find it
        ++o.fits;
        const double diff = (double)(got - std::min(got, unlimited));
        CHECK(diff <= 1e-9 * (double)unlimited, "%s: weighted length %llu, optimum %llu", what.c_str(), (unsigned long long)got,
              (unsigned long long)unlimited);
    } else {  // the weight floor is a heuristic: reported, not asserted
        ++o.limited;
        const double ratio = (double)got / (double)limited;
        if (ratio > o.worst_ratio) {
            o.worst_ratio = ratio;
            o.worst_case = what;
        }
    }
}

}  // namespace

int main() {
    std::mt19937_64 rng(20260519);
    int built = 0, refused = 0;
    Optimality opt;
    auto run = [&](int family, int sigma, int trial) {
        const Counts cnt = make_counts(family, sigma, rng);
        const std::string what = std::string(FAMILY[family]) + " sigma " + std::to_string(sigma) + " trial " + std::to_string(trial);
        VlCode v;
        if (!vl_build(cnt.data(), sigma, v)) {
            ++refused;
            return;
        }
        ++built;
        check_code(v, cnt, sigma, what);
        check_tables(v, sigma, what);
        if (sigma <= 47) check_optimal(v, cnt, what, opt);
    };
    for (int family = 0; family < NFAMILY; ++family) {
        for (int sigma : {2, 3, 7, 64, 126, 127})
            for (int trial = 0; trial < 20; ++trial) run(family, sigma, trial);
        for (int trial = 0; trial < 600; ++trial) run(family, 2 + (int)(rng() % 39), trial);
    }
    CHECK(built > 0 && opt.fits > 0 && opt.limited > 0, "built %d, optimum fits %d, depth-limited %d", built, opt.fits, opt.limited);

    // what vl_build must refuse: one symbol, more symbols than VL_MAX_LEN bits can tell apart, nothing counted at all
    {
        VlCode v;
        Counts ones(130, 1), zeros(130, 0);
        CHECK(!vl_build(ones.data(), 1, v), "sigma = 1 was accepted");
        CHECK(!vl_build(ones.data(), 0, v), "sigma = 0 was accepted");
        CHECK(!vl_build(ones.data(), 128, v), "sigma = 128 was accepted");
        CHECK(vl_build(ones.data(), 127, v), "sigma = 127, flat counts, was refused");
        for (int sigma : {2, 7, 127}) CHECK(!vl_build(zeros.data(), sigma, v), "all-zero counts were accepted (sigma %d)", sigma);
    }

    std::printf("codes built %d, refused %d; judged against the optimum %d: unlimited optimum fits %d, depth-limited %d, worst ratio over the "
                "depth-%d optimum %.4f (%s)\n",
                built, refused, opt.judged, opt.fits, opt.limited, VL_MAX_LEN, opt.worst_ratio, opt.worst_case.c_str());
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
