// insert.h — the reference-side insert() (database.cpp:283-379) followed by the build that makes the objects visible (:170-282), for a
// batch of objects over fields that live on the GPU: one cdb_insert_objects call (include/coffeedb_gpu.h), all fields or none.
// Header only; a failed call throws std::runtime_error with the library's message, as the shim's indexes do.
//
// The reference checks an object key by key (empty object, empty key, the type of the value against the index of that name) and
// writes raw/<id>; the next build() reads every record into every index.  Here the objects are grouped by key: every field gets the
// strictly ascending list of the batch's objects that hold it and their values in that order, and the library checks the ids (none
// twice in the batch, none already held by a field of the call) before any field changes.
// STATED DIVERGENCE (coffeedb_gpu.h): inserting an id again does not replace the object, it is refused; remove it first.
// A key that one object names twice is refused here with `Duplicate key "<key>" in one object` (std::runtime_error): the reference
// writes both values into raw/<id> and its build() keeps the last in `data` while the index is given the id twice; a GPU column refuses
// that build, and the library would see the field's rows not ascending and say so in terms a caller of this header never wrote.
// A key the field map does not name is a std::logic_error here: the reference creates an index of the value's type for it, which
// the caller of this header does (an empty string_index / integer_index / ... in its map) before it calls.
// The shim's string_index keeps views of the documents add() collected for its own build(); objects inserted here reach the device
// only.  A caller that later REBUILDS such a field through add() + build() hands those documents over again, as the reference's
// build() reads them again from raw/<id>.
#ifndef CDB_SHIM_INSERT_H
#define CDB_SHIM_INSERT_H
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
#include "select.h"

namespace cdb_shim {

using insert_object = std::pair<int64_t, std::vector<std::pair<std::string, var>>>;  // (id, object): insert()'s own arguments

namespace detail {
struct insert_column {  // what one field of the batch receives
    const class index* ix = nullptr;
    int kind = 3;  // 0 bool, 1 int64, 2 double, 3 string: the reference's `number` tags
    std::vector<uint64_t> rows;
    std::string blob;                    // string field
    std::vector<uint64_t> doc_start{0};  // ...
    std::vector<uint8_t> bools;          // bool column
    std::vector<uint64_t> raw;           // int64 / double column: the values' bit patterns
};
inline int kind_of(const var& v) { return (int)v.index(); }  // bool, int64_t, double, std::string in config.h's order
}  // namespace detail

// Every object joins every field it names, all or none.  Returns the per-field results in std::map order of the names the batch uses
// (name, cdb_insert_field with appended / status / committed).  Throws the reference's messages for an empty object, an empty key and a
// value of the wrong type, std::logic_error for a field that is not on one GPU, and std::runtime_error with the library's text for
// everything cdb_insert_objects refuses or fails at ("field <i>: ..." names the i-th field in that order).
inline std::vector<std::pair<std::string, cdb_insert_field>> insert(const std::vector<insert_object>& objects, const field_map& fields) {
    std::map<std::string, detail::insert_column> cols;
    std::vector<int64_t> ids;
    ids.reserve(objects.size());
    for (uint64_t i = 0; i < objects.size(); ++i) {
        const auto& [id, object] = objects[i];
        if (object.empty()) throw std::runtime_error("Empty objects are not allowed");  // database.cpp:284-286
        ids.push_back(id);
        for (const auto& [key, value] : object) {
            if (key.empty()) throw std::runtime_error("Empty keys are not allowed");  // database.cpp:288-290
            const auto f = fields.find(key);
            if (f == fields.end() || !f->second) throw std::logic_error("insert: field \"" + key + "\" is not in the field map");
            detail::insert_column& c = cols[key];
            if (!c.ix) {
                c.ix = f->second;
                if (dynamic_cast<const bool_index*>(c.ix)) c.kind = 0;
                else if (dynamic_cast<const integer_index*>(c.ix)) c.kind = 1;
                else if (dynamic_cast<const double_index*>(c.ix)) c.kind = 2;
                else c.kind = 3;
            }
            if (detail::kind_of(value) != c.kind || (c.kind == 3 && !dynamic_cast<const string_index*>(c.ix)))
                throw std::runtime_error("Mismatched type for \"" + key + "\"");  // database.cpp:329
            if (!c.rows.empty() && c.rows.back() == i) throw std::runtime_error("Duplicate key \"" + key + "\" in one object");
            c.rows.push_back(i);
            if (c.kind == 3) {
                c.blob += std::get<std::string>(value);
                c.doc_start.push_back(c.blob.size());
            } else if (c.kind == 0) {
                c.bools.push_back(std::get<bool>(value) ? 1 : 0);
            } else {
                uint64_t bits = 0;
                if (c.kind == 1) {
                    const int64_t v = std::get<int64_t>(value);
                    std::memcpy(&bits, &v, 8);
                } else {
                    const double v = std::get<double>(value);
                    std::memcpy(&bits, &v, 8);
                }
                c.raw.push_back(bits);
            }
        }
    }
    std::vector<cdb_insert_field> q;
    std::vector<std::string> names;
    for (auto& [name, c] : cols) {
        cdb_insert_field f{};
        if (c.kind == 3) {
            const auto* sp = static_cast<const string_index*>(c.ix);
            f.index = sp->gpu_index();
            if (c.blob.empty()) c.blob.push_back('\0');  // (empty documents only: the C ABI still wants a pointer)
            f.blob = c.blob.data();
            f.doc_start = c.doc_start.data();
        } else if (c.kind == 0) {
            f.column = static_cast<const bool_index*>(c.ix)->column();
            f.values = c.bools.data();
        } else {
            f.column = c.kind == 1 ? static_cast<const integer_index*>(c.ix)->column() : static_cast<const double_index*>(c.ix)->column();
            f.values = c.raw.data();
        }
        if (!f.index && !f.column) throw std::logic_error("insert: field \"" + name + "\" is not on one GPU (COFFEEDB_GPU_NUMERIC=1, no COFFEEDB_GPUS)");
        f.rows = c.rows.data();
        f.nrows = c.rows.size();
        q.push_back(f);
        names.push_back(name);
    }
    std::vector<std::pair<std::string, cdb_insert_field>> out;
    if (q.empty()) return out;  // no object at all
    const int rc = cdb_insert_objects(ids.data(), ids.size(), q.data(), (int)q.size(), nullptr);
    if (rc != CDB_OK) {
        const char* why = q[0].index ? cdb_last_error(q[0].index) : cdb_column_last_error(q[0].column);
        throw std::runtime_error(*why ? why : "cdb_insert_objects: invalid arguments");
    }
    for (size_t k = 0; k < q.size(); ++k) out.emplace_back(names[k], q[k]);
    return out;
}

}  // namespace cdb_shim
#endif
