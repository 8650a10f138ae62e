// cluster.h — the reference-side half of `cluster` (database.cpp:442-460, called from interface.cpp:249-273): turns the groups
// the device made (include/coffeedb_gpu.h: cdb_clusters) into exactly what cluster() returns — the field's values as the
// reference prints them, each with the number of result rows that hold it, ordered as std::map<std::string, int64_t> orders.
// Host only, header only; needs no GPU and no library symbol (the caller frees the cdb_clusters).
//
// The reference keys its map with std::to_string(val) for everything that is not a string (database.cpp:453-455):
//   int64_t -> "%lld";  double -> "%f" (six decimals: 1e-7 and 2e-7 both print "0.000000" and share one map entry);
//   bool -> promoted to int: "0" / "1".
// The device groups by VALUE, so groups that print alike are merged here, and the order becomes that of the printed strings
// ("-1" < "-10" < "10" < "9").  One divergence is inherited from the column: -0.0 was folded onto +0.0 when it was built, so the
// reference's separate "-0.000000" entry is counted under "0.000000" (coffeedb_gpu.h).
#ifndef CDB_SHIM_CLUSTER_H
#define CDB_SHIM_CLUSTER_H
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/coffeedb_gpu.h"

namespace cdb_shim {

using cluster_result = std::vector<std::pair<const std::string, int64_t>>;

// std::to_string of the value behind a column's raw group value (kind = the reference's `number` tag: 0 bool, 1 int64, 2 double)
inline std::string cluster_value_string(int kind, uint64_t raw) {
    if (kind == 1) {
        int64_t v;
        std::memcpy(&v, &raw, 8);
        return std::to_string(v);
    }
    if (kind == 2) {
        double v;
        std::memcpy(&v, &raw, 8);
        return std::to_string(v);
    }
    return std::to_string(raw != 0);  // (bool promotes to int: "0" / "1")
}

// groups of a numeric / bool column (cdb_column_cluster) -> cluster()'s return value
inline cluster_result cluster_rows(const cdb_clusters& c, int kind) {
    std::map<std::string, int64_t> times;
    for (uint64_t g = 0; g < c.ngroups; ++g) times[cluster_value_string(kind, c.values[g])] += c.counts[g];
    return cluster_result(times.begin(), times.end());
}

// groups of a string index (cdb_cluster with with_values != 0) -> cluster()'s return value; the groups already arrive in
// std::string order
inline cluster_result cluster_rows(const cdb_clusters& c) {
    cluster_result out;
    out.reserve(c.ngroups);
    for (uint64_t g = 0; g < c.ngroups; ++g)
        out.emplace_back(std::string(c.value_blob + c.value_ptr[g], (size_t)(c.value_ptr[g + 1] - c.value_ptr[g])), c.counts[g]);
    return out;
}

}  // namespace cdb_shim
#endif
