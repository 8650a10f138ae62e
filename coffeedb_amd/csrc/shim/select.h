// select.h — the reference-side select() (database.cpp:394-441, called from interface.cpp:242) over a row set that stayed on the
// device: one cdb_rowset_select call (include/coffeedb_gpu.h) cuts the page and reads every field, and this header puts the objects
// together by the reference's rules.  Header only; a failed call throws std::runtime_error with the library's message.  It returns
// what select() returns; printing JSON stays with the caller (interface.cpp:243-247).
//
// The reference reads the objects from its host store, `data[id]` (database.cpp:22).  Here a field is read from the index that holds
// it, so "the object has the field" becomes "the field's index holds the id".  The two agree: build() (database.cpp:170-282) is the
// only writer of `data`, and each of its four branches stores data[id][key] = value and calls ptr->add(id, value) on indices[key] side
// by side (:211-212, :226-227, :241-242, :263-264) — a type mismatch throws and fails the whole build; insert() (:283-379) touches
// neither, it checks the types, creates an EMPTY index for a new key and writes the record file.  Two records can make them differ,
// and neither comes from insert(): a record that names one key twice (data keeps the last value, the index is given the id twice: a
// GPU column refuses that build), and a NaN double (a GPU column refuses it).  A key that insert() announced but no build() has seen
// yet has an empty index and no data: no object shows it, here as there.
//
// Rules (database.cpp:394-441):
//   fields      in `keys` order — a key the object lacks is skipped, a key named twice appears twice — or, with no keys, every field
//               of `fields` in std::map order (which is the order of data[id], a std::map over the same names);
//   rendering   with constraints: a STRING field named in them is rendered with that key's keyword list (the first entry of that
//               name, as std::map::emplace keeps it; database.cpp:145-151), every other field is plain; without constraints
//               everything is plain — interface.cpp:225-227 clears them when the query has no `highlight`;
//   correlation "$correlation" is appended last when the row's count is not 0 and keys is empty or names it;
//   dropped     a row whose object comes out empty is dropped;
//   order       the page is cdb_rowset_page's: descending count, TIES ASCENDING ID (the reference's std::sort leaves ties open).
// KNOWN DIVERGENCE, inherited from the column: a double stored as -0.0 reads +0.0 (coffeedb_gpu.h).
#ifndef CDB_SHIM_SELECT_H
#define CDB_SHIM_SELECT_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../../include/coffeedb_gpu.h"
#include "index.h"
#include "rowset.h"

namespace cdb_shim {

using var = std::variant<bool, int64_t, double, std::string>;  // config.h:7
using object_type = std::vector<std::pair<const std::string, var>>;
using constraint_list = std::vector<std::pair<std::string, std::vector<std::string>>>;
// the named fields, as `indices` (database.cpp:21) holds them: a string_index, or a bool / integer / double index that lives on
// the GPU (COFFEEDB_GPU_NUMERIC=1: column() is set)
// (`class index`: <strings.h> declares a function of that name)
using field_map = std::map<std::string, const class index*>;
inline const std::string select_key_correlation = "$correlation";  // config.h:8

namespace detail {
struct selected_guard {
    cdb_selected r{};
    ~selected_guard() { cdb_selected_free(&r); }
};
inline var column_var(int kind, uint64_t raw) {
    if (kind == 1) {
        int64_t v;
        std::memcpy(&v, &raw, 8);
        return var(v);
    }
    if (kind == 2) {
        double v;
        std::memcpy(&v, &raw, 8);
        return var(v);
    }
    return var(raw != 0);
}
}  // namespace detail

// rows [first, last) of rs's ranking (`span`; no span: first = 0, last = UINT64_MAX) as select() returns them
inline std::vector<object_type> select(const rowset& rs, uint64_t first, uint64_t last, const field_map& fields,
                                       const std::vector<std::string>& keys, const constraint_list& constraints, const std::string& left,
                                       const std::string& right) {
    // 1. the fields to read, each once, and where every output position finds its field
    std::vector<std::pair<std::string, int>> wanted;  // (name, slot) in output order
    std::vector<const std::string*> slot_name;
    std::map<std::string, int> slot_of;
    auto want = [&](const std::string& name) {
        auto [it, fresh] = slot_of.emplace(name, (int)slot_name.size());
        if (fresh) slot_name.push_back(&it->first);
        wanted.emplace_back(name, it->second);
    };
    if (keys.empty()) {
        for (const auto& kv : fields) want(kv.first);
    } else {
        for (const auto& k : keys)
            if (fields.count(k)) want(k);
    }
    // 2. their device objects and keyword lists
    const int nslots = (int)slot_name.size();
    std::vector<cdb_select_field> q(std::max(nslots, 1));
    std::vector<std::string> kw_blob(nslots);
    std::vector<std::vector<uint64_t>> kw_off(nslots);
    for (int s = 0; s < nslots; ++s) {
        const std::string& name = *slot_name[s];
        const class index* ix = fields.at(name);
        cdb_select_field& f = q[s];
        f = cdb_select_field{};
        if (auto* sp = dynamic_cast<const string_index*>(ix)) {
            f.index = sp->gpu_index();
            f.shards = sp->gpu_shards();
            kw_off[s].push_back(0);
            const auto c = std::find_if(constraints.begin(), constraints.end(), [&](const auto& kv) { return kv.first == name; });
            if (c != constraints.end())
                for (const auto& k : c->second) {
                    kw_blob[s] += k;
                    kw_off[s].push_back(kw_blob[s].size());
                }
            f.kw_blob = kw_blob[s].data();
            f.kw_offsets = kw_off[s].data();
            f.nkw = kw_off[s].size() - 1;
        } else if (auto* bp = dynamic_cast<const bool_index*>(ix)) {
            f.column = bp->column();
        } else if (auto* ip = dynamic_cast<const integer_index*>(ix)) {
            f.column = ip->column();
        } else if (auto* dp = dynamic_cast<const double_index*>(ix)) {
            f.column = dp->column();
        }
        if (!f.index && !f.shards && !f.column)
            throw std::logic_error("select: field \"" + name + "\" is not on the GPU (COFFEEDB_GPU_NUMERIC=1)");
    }
    // 3. one call: the page and every field of it
    detail::selected_guard g;
    if (cdb_rowset_select(rs.get(), first, last, q.data(), nslots, left.data(), left.size(), right.data(), right.size(), &g.r) != CDB_OK)
        throw std::runtime_error(rs ? cdb_rowset_last_error(rs.get()) : "cdb_shim::select: empty row set");
    // 4. the objects
    const bool flag = keys.empty() || std::find(keys.begin(), keys.end(), select_key_correlation) != keys.end();
    std::vector<object_type> ret;
    for (uint64_t i = 0; i < g.r.nrows; ++i) {
        object_type object;
        for (const auto& [name, s] : wanted) {
            const cdb_selected_field& f = g.r.fields[s];
            if (!f.found[i]) continue;
            if (f.kind == 3)
                object.emplace_back(name, var(std::string(f.text_blob + f.text_ptr[i], (size_t)(f.text_ptr[i + 1] - f.text_ptr[i]))));
            else
                object.emplace_back(name, detail::column_var(f.kind, f.values[i]));
        }
        if (g.r.counts[i] && flag) object.emplace_back(select_key_correlation, var((int64_t)g.r.counts[i]));
        if (!object.empty()) ret.push_back(std::move(object));
    }
    return ret;
}

}  // namespace cdb_shim
#endif
