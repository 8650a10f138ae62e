// sa_sorts.hip — the sorts of 8-byte entries that more than one phase of the suffix-array build calls (sa_build_phases.h), instantiated
// once.  (Those of 4-byte entries: sa_initial_direct.hip, beside the MSD-first sort they share two kernel configurations with.)
#include "sa_build_phases.h"

namespace cdb {

template int radix_sort<uint64_t, uint64_t>(CDB_SA_SORT_ARGS(uint64_t, uint64_t));
template int radix_sort<uint32_t, uint64_t>(CDB_SA_SORT_ARGS(uint32_t, uint64_t));
template int radix_sort_split<uint64_t, uint8_t>(CDB_SA_SPLIT_ARGS(uint64_t, uint8_t));
template int radix_sort_split<uint64_t, uint16_t>(CDB_SA_SPLIT_ARGS(uint64_t, uint16_t));

}  // namespace cdb
