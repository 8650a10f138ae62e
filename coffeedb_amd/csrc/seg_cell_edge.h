// seg_cell_edge.h — the 16-byte edge record of the last pass over cells (radix_pass.h: SegFinalCellArgs) and its limits.
// A cell's keys are 32 bits wide and a (tile, digit) run has at most one tile of elements, so the run's first and last key, its
// output slot and its length fit 16 bytes where the general record (SegEdge: 64-bit keys) takes 32.
// Standard headers only: a plain host program can include it (tests/cpp/test_seg_cell_edge.cpp).
#pragma once
#include <cstdint>
#include <string>

#include "errors.h"

#if defined(__HIPCC__)
#define CDB_CELL_EDGE_HD __host__ __device__ __forceinline__
#else
#define CDB_CELL_EDGE_HD inline
#endif

namespace cdb {

constexpr int SEG_CELL_POS_BITS = 48;                          // output slot of the run's first element, inside the bucket group
constexpr uint32_t SEG_CELL_CNT_MAX = 16384;                   // elements of a run in the 16 bits above it: at most one tile
constexpr unsigned long long SEG_CELL_POS_MASK = (1ull << SEG_CELL_POS_BITS) - 1ull;

struct SegCellEdge {
    uint32_t first, last;        // keys of the run's first and last element
    unsigned long long pos_cnt;  // pos | cnt << 48 (cnt = 0: the tile has no element of the digit; pos still says where one would go)
};
static_assert(sizeof(SegCellEdge) == 16, "cell edge record: 16 bytes");

CDB_CELL_EDGE_HD SegCellEdge seg_cell_edge_pack(uint32_t first, uint32_t last, unsigned long long pos, uint32_t cnt) {
    SegCellEdge e;
    e.first = first;
    e.last = last;
    e.pos_cnt = pos | ((unsigned long long)cnt << SEG_CELL_POS_BITS);
    return e;
}
CDB_CELL_EDGE_HD unsigned long long seg_cell_edge_pos(unsigned long long pos_cnt) { return pos_cnt & SEG_CELL_POS_MASK; }
CDB_CELL_EDGE_HD uint32_t seg_cell_edge_cnt(unsigned long long pos_cnt) { return (uint32_t)(pos_cnt >> SEG_CELL_POS_BITS); }

// what a pass may write into such records: every output slot below 2^48 (`slots` = one past the largest) and no run longer
// than the count field holds (`tile` = elements per tile, the most one run can have)
inline void seg_cell_edge_check_limits(unsigned long long slots, unsigned long long tile) {
    if (slots > (1ull << SEG_CELL_POS_BITS)) throw InternalError("cell edge record: output slot beyond 2^48 (internal)");
    if (tile > (unsigned long long)SEG_CELL_CNT_MAX)
        throw InternalError("cell edge record: a run of more than 16384 elements (internal)");
}

}  // namespace cdb
