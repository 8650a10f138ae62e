// test_seg_cell_edge.cpp — the 16-byte edge record of the last pass over cells (seg_cell_edge.h) on the host alone: what is packed
// comes back out at the ends of every field, the fields do not reach into each other, and the two limit checks refuse exactly
// what the record cannot hold.  Plain C++, no HIP: g++ -std=c++17 -I coffeedb_amd/csrc tests/cpp/test_seg_cell_edge.cpp.
#include "seg_cell_edge.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

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

void round_trip(uint32_t first, uint32_t last, unsigned long long pos, uint32_t cnt) {
    const SegCellEdge e = seg_cell_edge_pack(first, last, pos, cnt);
    CHECK(e.first == first && e.last == last, "keys %08x %08x", first, last);
    CHECK(seg_cell_edge_pos(e.pos_cnt) == pos, "pos %llx cnt %u -> %llx", pos, cnt, seg_cell_edge_pos(e.pos_cnt));
    CHECK(seg_cell_edge_cnt(e.pos_cnt) == cnt, "pos %llx cnt %u -> %u", pos, cnt, seg_cell_edge_cnt(e.pos_cnt));
}

// 0 = accepted, 3 = refused as an internal error, -1 = anything else
int limits(unsigned long long slots, unsigned long long tile) {
    try {
        seg_cell_edge_check_limits(slots, tile);
        return 0;
    } catch (const InternalError& e) {
        return (int)e.status;
    } catch (...) {
        return -1;
    }
}

}  // namespace

int main() {
    static_assert(sizeof(SegCellEdge) == 16 && alignof(SegCellEdge) == 8, "one 16-byte store per record");
    const unsigned long long top = (1ull << 48) - 1ull;
    const uint32_t keys[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const unsigned long long poss[] = {0ull, 1ull, (1ull << 32) - 1ull, 1ull << 32, (1ull << 47) + 12345ull, top - 1ull, top};
    const uint32_t cnts[] = {0u, 1u, 16383u, 16384u};
    for (uint32_t f : keys)
        for (uint32_t l : keys)
            for (unsigned long long p : poss)
                for (uint32_t c : cnts) round_trip(f, l, p, c);
    std::mt19937_64 rng(99);
    for (int i = 0; i < 100000; ++i) round_trip((uint32_t)rng(), (uint32_t)rng(), rng() & top, (uint32_t)(rng() % 16385u));
    // a full count leaves the slot alone, and a full slot the count
    CHECK(seg_cell_edge_pack(0, 0, top, 0).pos_cnt == top, "slot bits");
    CHECK(seg_cell_edge_pack(0, 0, 0, 16384).pos_cnt == (16384ull << 48), "count bits");
    // the record in memory: keys in the first eight bytes, slot | count in the second eight
    {
        const SegCellEdge e = seg_cell_edge_pack(0x11223344u, 0xAABBCCDDu, 5, 7);
        uint32_t w[4];
        std::memcpy(w, &e, 16);
        CHECK(w[0] == 0x11223344u && w[1] == 0xAABBCCDDu, "key words %08x %08x", w[0], w[1]);
        unsigned long long q;
        std::memcpy(&q, (const char*)&e + 8, 8);
        CHECK(q == (5ull | (7ull << 48)), "slot word %llx", q);
    }
    // limits: slots are [0, slots), so 2^48 of them still fit; a run is at most one tile of 16384
    CHECK(limits(0, 16384) == 0, "empty group");
    CHECK(limits(1ull << 33, 16384) == 0, "2^33 slots");
    CHECK(limits(1ull << 48, 16384) == 0, "2^48 slots: the largest is 2^48 - 1");
    CHECK(limits((1ull << 48) + 1, 16384) == 3, "2^48 + 1 slots");
    CHECK(limits(~0ull, 16384) == 3, "2^64 - 1 slots");
    CHECK(limits(1000, 1) == 0, "tile of one");
    CHECK(limits(1000, 16385) == 3, "tile of 16385");
    CHECK(limits(1000, 1ull << 20) == 3, "tile of 2^20");
    CHECK(limits((1ull << 48) + 1, 16385) == 3, "both");
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
