// rowset.h — filter() once, then count, page and cluster (include/coffeedb_gpu.h: cdb_filter, cdb_rowset_*): a move-only owner of
// a row set for the reference-side code.  interface.cpp runs the same filter() (interface.cpp:46-148) in front of `count`, `query`
// with `span`, `cluster` and `remove`; with this class filter() is one cdb_filter call and the four operations read the rows on
// the device.  Header only; a failed call throws std::runtime_error with the library's message, as the shim's indexes do.
#ifndef CDB_SHIM_ROWSET_H
#define CDB_SHIM_ROWSET_H
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/coffeedb_gpu.h"

namespace cdb_shim {

class rowset {
public:
    using rows = std::vector<std::pair<int64_t, int64_t>>;  // (object id, $correlation): filter()'s own element type

    rowset() = default;
    // takes a row set that cdb_filter made
    explicit rowset(cdb_rowset* h) : h_(h) {}
    rowset(rowset&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    rowset& operator=(rowset&& o) noexcept {
        if (this != &o) {
            cdb_rowset_free(h_);
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    rowset(const rowset&) = delete;
    rowset& operator=(const rowset&) = delete;
    ~rowset() { cdb_rowset_free(h_); }

    cdb_rowset* get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

    // `count` (interface.cpp:289-301): no row leaves the device
    uint64_t size() const { return cdb_rowset_size(h_); }
    // every row ascending by id: the list `remove` walks (interface.cpp:274-285)
    rows all() const {
        int64_t *ids = nullptr, *counts = nullptr;
        size_t n = 0;
        check(cdb_rowset_rows(h_, &ids, &counts, &n));
        return take(ids, counts, n);
    }
    // `query` with `span` [first, last) (interface.cpp:144-146, :228-241): descending $correlation, ties ascending id
    rows page(uint64_t first, uint64_t last) const {
        int64_t *ids = nullptr, *counts = nullptr;
        size_t n = 0;
        check(cdb_rowset_page(h_, first, last, &ids, &counts, &n));
        return take(ids, counts, n);
    }
    // `cluster` (database.cpp:442-460) by a string index / a column: the caller prints the groups with shim/cluster.h and frees them
    // with cdb_clusters_free
    cdb_clusters cluster(cdb_index* field, bool with_values = true) const {
        cdb_clusters out{};
        check(cdb_rowset_cluster(h_, field, with_values ? 1 : 0, &out));
        return out;
    }
    cdb_clusters cluster(cdb_column* field) const {
        cdb_clusters out{};
        check(cdb_rowset_cluster_column(h_, field, &out));
        return out;
    }

    // `remove` (interface.cpp:274-285): the rows of the set leave every field given, all or none; ids stay on the device.  A field is
    // a cdb_remove_field with `index` or `column` set (field_of below); the per-field results come back in the caller's order.  A
    // failure throws with the library's text ("field <i>: ..."); after a failed prepare nothing has changed in any field.
    static cdb_remove_field field_of(cdb_index* h) { return cdb_remove_field{h, nullptr, 0, 0, 0, 0}; }
    static cdb_remove_field field_of(cdb_column* c) { return cdb_remove_field{nullptr, c, 0, 0, 0, 0}; }
    std::vector<cdb_remove_field> remove(std::vector<cdb_remove_field> fields, uint64_t* removed_rows = nullptr) const {
        uint64_t n = 0;
        check(cdb_rowset_remove(h_, fields.data(), (int)fields.size(), &n));
        if (removed_rows) *removed_rows = n;
        return fields;
    }
    // filter() without constraints (interface.cpp:51-53 -> query(), database.cpp:380-386): every object the given fields hold, count 0.
    // `count` without constraints is everything(...).size(); a `query` with `span` is everything(...).page(first, last)
    static rowset everything(const std::vector<cdb_index*>& indexes, const std::vector<cdb_column*>& columns) {
        cdb_rowset* h = nullptr;
        const int rc = cdb_rowset_all(indexes.empty() ? nullptr : indexes.data(), (int)indexes.size(), columns.empty() ? nullptr : columns.data(),
                                      (int)columns.size(), &h);
        if (rc != CDB_OK) {
            const char* why = !indexes.empty() && indexes[0] ? cdb_last_error(indexes[0])
                              : !columns.empty() && columns[0] ? cdb_column_last_error(columns[0]) : "";
            throw std::runtime_error(std::string("cdb_rowset_all: ") + (*why ? why : "invalid arguments"));
        }
        return rowset(h);
    }

private:
    void check(int rc) const {
        if (rc != CDB_OK) throw std::runtime_error(h_ ? cdb_rowset_last_error(h_) : "cdb_shim::rowset: empty");
    }
    static rows take(int64_t* ids, int64_t* counts, size_t n) {
        rows out;
        out.reserve(n);
        for (size_t r = 0; r < n; ++r) out.emplace_back(ids[r], counts[r]);
        cdb_free(ids);
        cdb_free(counts);
        return out;
    }
    cdb_rowset* h_ = nullptr;
};

}  // namespace cdb_shim
#endif
