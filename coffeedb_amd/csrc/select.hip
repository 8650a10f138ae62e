// select.hip — the tail of the reference's `query` operation (interface.cpp:181-248: filter() -> rank -> span -> select(fields,
// highlight), database.cpp:394-441) in one call on a row set: cdb_rowset_select cuts the page as cdb_rowset_page does, keeps the
// page's ids in device memory and reads every requested field where it lies — string fields through render.hip's device-ids form,
// numeric and bool fields through the per-row direction of a column (id -> value), which cdb_column_values also offers on its own.
//
// sel_values_kernel: a lane is a row, blockIdx.y a column.  The lane finds its id's rank with the bisection of columns.hip's ProbeIn
// (lower bound over id_sorted, then a < n && id_sorted[a] == id), follows vpos to the row's place in value order and turns the order
// key back into the value.  One launch serves every column field of a select; values, miss counters and found bytes of all columns
// lie in one block — [ncols x nrows values | ncols counters | ncols x nrows found bytes] — that comes back in one copy.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"

using namespace cdb;

namespace {

struct SelColumn {
    const int64_t* id_sorted;
    const uint32_t* vpos;
    const uint64_t* keys_v;
    uint64_t n;
    int kind;
};

__global__ __launch_bounds__(256) void sel_values_kernel(const int64_t* __restrict__ ids, uint64_t nrows, const SelColumn* __restrict__ cols,
                                                         uint64_t* __restrict__ values, unsigned long long* missing, uint8_t* __restrict__ found) {
    const SelColumn c = cols[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < nrows;
    bool hit = false;
    if (in) {
        const int64_t id = ids[i];
        uint64_t a = 0, b = c.n;
        while (a < b) {
            const uint64_t m = (a + b) >> 1;
            if (c.id_sorted[m] < id) a = m + 1;
            else b = m;
        }
        hit = a < c.n && c.id_sorted[a] == id;
        const uint64_t o = (uint64_t)blockIdx.y * nrows + i;
        values[o] = hit ? column_key_raw(c.kind, c.keys_v[c.vpos[a]]) : 0;
        found[o] = hit ? 1 : 0;
    }
    const uint64_t miss = __ballot(in && !hit);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(&missing[blockIdx.y], (unsigned long long)__popcll(miss));
}

// where the three parts of the block lie, on the device and on the host alike
struct ValuesLayout {
    uint64_t ncols, nrows;
    uint64_t missing_at() const { return ncols * nrows * 8; }
    uint64_t found_at() const { return missing_at() + ncols * 8; }
    uint64_t bytes() const { return found_at() + ncols * nrows; }
};

// The values of the rows d_ids[nrows] (device memory, complete) in every column of `cols`, on stream s; the caller holds the columns'
// locks.  Returns the host block (host_free), filled: the stream has been synchronised.
uint8_t* select_values(hipStream_t s, Profiler& prof, const int64_t* d_ids, const ValuesLayout& lay, cdb_column* const* cols) {
    std::vector<SelColumn> desc(lay.ncols);
    uint64_t levels = 0;
    for (uint64_t j = 0; j < lay.ncols; ++j) {
        const cdb_column* c = cols[j];
        desc[j] = SelColumn{c->id_sorted.as<int64_t>(), c->vpos.as<uint32_t>(), c->keys_v.as<uint64_t>(), c->n, c->kind};
        levels += (uint64_t)bit_width64(c->n);
    }
    DevBuf d_desc, d_block;
    d_desc.alloc(lay.ncols * sizeof(SelColumn));
    d_block.alloc(lay.bytes());
    uint8_t* block = (uint8_t*)host_alloc(lay.bytes(), true);
    try {
        if (lay.nrows) {
            uint8_t* d = d_block.as<uint8_t>();
            CDB_HIP(hipMemcpyAsync(d_desc.p, desc.data(), lay.ncols * sizeof(SelColumn), hipMemcpyHostToDevice, s));
            CDB_HIP(hipMemsetAsync(d + lay.missing_at(), 0, lay.ncols * 8, s));
            const int t = prof.begin(s);
            hipLaunchKernelGGL(sel_values_kernel, dim3((unsigned)ceil_div(lay.nrows, 256), (unsigned)lay.ncols), dim3(256), 0, s, d_ids, lay.nrows,
                               (const SelColumn*)d_desc.as<SelColumn>(), (uint64_t*)d, (unsigned long long*)(d + lay.missing_at()), d + lay.found_at());
            prof.end(t, "sel_values", lay.nrows * (lay.ncols * (8 + 4 + 8 + 9) + 8 * levels), s);  // id, vpos, key, value + found; the probes
            CDB_HIP(hipGetLastError());
            CDB_HIP(hipMemcpyAsync(block, d, lay.bytes(), hipMemcpyDeviceToHost, s));
        }
        CDB_HIP(hipStreamSynchronize(s));  // (desc is read by its copy; the device blocks go back to the pool behind this scope)
    } catch (...) {
        (void)hipStreamSynchronize(s);
        host_free(block);
        throw;
    }
    return block;
}

constexpr unsigned SEL_MAX_COLUMNS = 65535;  // gridDim.y

// the result while it is made (every piece of it arrives behind a synchronise of its own: download_rows, select_values, the renders)
using Selected = ResultOwner<cdb_selected, cdb_selected_free>;

bool field_is_valid(const cdb_select_field& f) {
    if ((f.index != nullptr) + (f.shards != nullptr) + (f.column != nullptr) != 1) return false;
    if (f.column && f.nkw) return false;  // a column has no keywords to highlight
    return !f.nkw || f.kw_offsets;
}

void rowset_select(cdb_rowset* rs, uint64_t first, uint64_t last, const cdb_select_field* fields, int nfields, const char* left, size_t L,
                   const char* right, size_t R, Selected& res) {
    Index& ws = rs->ws;
    hipStream_t s = ws.stream;
    const double t0 = wall_ms();
    // 1. the page, as cdb_rowset_page makes it; the download synchronises: everything below reads finished device ids
    DevicePage pg;
    rowset_page_device(rs, first, last, pg);
    size_t n = 0;
    download_rows(s, pg.ids.as<int64_t>(), pg.counts.as<int64_t>(), pg.n, &res.r.ids, &res.r.counts, &n);
    rs->page_ms = wall_ms() - t0;
    res.r.nrows = n;
    res.r.nfields = nfields;
    res.r.fields = (cdb_selected_field*)host_alloc(std::max(nfields, 1) * sizeof(cdb_selected_field), true);
    std::vector<cdb_column*> cols;
    for (int k = 0; k < nfields; ++k) {
        res.r.fields[k].kind = fields[k].column ? fields[k].column->kind : 3;
        if (fields[k].column) cols.push_back(fields[k].column);
    }
    const int64_t* d_page = pg.ids.as<int64_t>();
    // 2. every column field in one launch on the row set's stream, under the columns' locks (address order: columns.hip's rule)
    if (!cols.empty()) {
        std::vector<std::mutex*> mus;
        for (cdb_column* c : cols) mus.push_back(&c->ws.mu);
        std::sort(mus.begin(), mus.end());
        mus.erase(std::unique(mus.begin(), mus.end()), mus.end());
        std::vector<std::unique_lock<std::mutex>> locks;
        for (std::mutex* m : mus) locks.emplace_back(*m);
        const ValuesLayout lay{(uint64_t)cols.size(), (uint64_t)n};
        uint8_t* block = select_values(s, ws.prof, d_page, lay, cols.data());
        uint64_t j = 0;
        for (int k = 0; k < nfields; ++k) {
            if (!fields[k].column) continue;
            cdb_selected_field& f = res.r.fields[k];
            f.values = (uint64_t*)block + j * n;  // (the first column field's `values` is the block: cdb_selected_free)
            f.missing = ((const uint64_t*)(block + lay.missing_at()))[j];
            f.found = block + lay.found_at() + j * n;
            ++j;
        }
    }
    if (pg.n) ws.prof.resolve();
    // 3. the string fields, one at a time: each under its own handle's lock and on its own stream, no two index locks together
    for (int k = 0; k < nfields; ++k) {
        const cdb_select_field& q = fields[k];
        if (q.column) continue;
        cdb_selected_field& f = res.r.fields[k];
        cdb_rendered rr{};
        if (q.index) {
            render_index_device_rows(q.index, d_page, n, q.kw_blob, q.kw_offsets, q.nkw, left, L, right, R, CDB_RENDER_TEXT, &rr);
        } else {
            const int rc = cdb_shards_render_rows(q.shards, res.r.ids, n, q.kw_blob, q.kw_offsets, q.nkw, left, L, right, R, CDB_RENDER_TEXT, &rr);
            if (rc != CDB_OK) throw Error((Status)rc, std::string(cdb_shards_last_error(q.shards)));
        }
        f.missing = rr.missing;
        f.found = rr.found;
        f.text_ptr = rr.text_ptr;
        f.text_blob = rr.text_blob;
    }
    ++rs->selects;
    rs->select_rows = n;
    rs->select_ms = wall_ms() - t0;
}

}  // namespace

extern "C" {

int cdb_column_values(cdb_column* c, const int64_t* ids, uint64_t nrows, uint64_t* values, uint8_t* found, uint64_t* missing) {
    if (!c || (nrows && (!ids || !values || !found))) return CDB_E_INVALID;
    if (missing) *missing = 0;
    return guarded_ix(c->ws, [&] {
        std::lock_guard<std::mutex> g(c->ws.mu);
        DeviceScope scope(c->ws);
        if (nrows == 0) return;
        hipStream_t s = c->ws.stream;
        DevBuf d_ids;
        d_ids.alloc(nrows * 8);
        CDB_HIP(hipMemcpyAsync(d_ids.p, ids, nrows * 8, hipMemcpyHostToDevice, s));
        const ValuesLayout lay{1, nrows};
        cdb_column* cols[1] = {c};
        uint8_t* block = select_values(s, c->ws.prof, d_ids.as<int64_t>(), lay, cols);
        c->ws.prof.resolve();
        std::memcpy(values, block, nrows * 8);
        std::memcpy(found, block + lay.found_at(), nrows);
        if (missing) std::memcpy(missing, block + lay.missing_at(), 8);
        host_free(block);
    });
}

int cdb_rowset_select(cdb_rowset* rs, uint64_t first, uint64_t last, const cdb_select_field* fields, int nfields, const char* left,
                      size_t left_len, const char* right, size_t right_len, cdb_selected* out) {
    if (out) *out = cdb_selected{};
    if (!rs || !out) return CDB_E_INVALID;
    if (nfields < 0 || (nfields && !fields) || (left_len && !left) || (right_len && !right)) return CDB_E_INVALID;
    for (int k = 0; k < nfields; ++k)
        if (!field_is_valid(fields[k])) return CDB_E_INVALID;
    return guarded_ix(rs->ws, [&] {
        size_t ncols = 0;
        for (int k = 0; k < nfields; ++k) {
            const cdb_select_field& q = fields[k];
            check_keywords(KeywordList{q.kw_blob, q.kw_offsets, q.nkw}, "cdb_rowset_select", KW_NONE_EMPTY | KW_BYTES);
            ncols += q.column != nullptr;
        }
        if (ncols > SEL_MAX_COLUMNS) throw Error("cdb_rowset_select: more than 65535 column fields");
        std::lock_guard<std::mutex> g(rs->ws.mu);
        for (int k = 0; k < nfields; ++k) {
            const cdb_select_field& q = fields[k];
            if ((q.index && q.index->ix.device != rs->ws.device) || (q.column && q.column->ws.device != rs->ws.device))
                throw Error("cdb_rowset_select: a field lives on another GPU");
        }
        DeviceScope scope(rs->ws);
        Selected res(rs->ws.stream);
        rowset_select(rs, first, last, fields, nfields, left, left_len, right, right_len, res);
        res.hand_over(out);
    });
}

void cdb_selected_free(cdb_selected* r) {
    if (!r) return;
    host_free(r->ids);
    host_free(r->counts);
    bool block_freed = false;
    for (int k = 0; r->fields && k < r->nfields; ++k) {
        cdb_selected_field& f = r->fields[k];
        if (f.kind == 3) {
            host_free(f.found);
            host_free(f.text_ptr);
            host_free(f.text_blob);
        } else if (f.values && !block_freed) {  // one block holds every column field's values and found bytes
            host_free(f.values);
            block_freed = true;
        }
    }
    host_free(r->fields);
    std::memset(r, 0, sizeof(*r));
}

}  // extern "C"
