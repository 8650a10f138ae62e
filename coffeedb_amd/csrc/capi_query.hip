// capi_query.hip — the query entry points of the C ABI on one string index (include/coffeedb_gpu.h): every cdb_query*, the
// frees of their results, the coalescing of concurrent single-keyword queries, and the two device-batch calls.  Host logic
// only: keyword lists in (keyword_list.h, host_io.h), results out, error translation.  All device work is in query.hip;
// the AND's key resolution is columns.hip's (filter_rows_on_lead).  Handle lifecycle, builds and the rest are capi.hip's.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>

#include "../../include/coffeedb_gpu.h"
#include "host_io.h"

using namespace cdb;

namespace {
using BatchResult = ResultOwner<cdb_result, cdb_result_free>;
using BatchHits = ResultOwner<cdb_hits, cdb_hits_free>;
using Spans = ResultOwner<cdb_spans, cdb_spans_free>;

int query_batch_impl(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out, cdb_hits* hits) {
    if (!h || !out || (npat && !offsets)) return CDB_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    if (hits) std::memset(hits, 0, sizeof(*hits));
    return guarded_ix(h->ix, [&] {
        Index& ix = h->ix;
        const KeywordList kws{blob, offsets, npat};
        check_keywords(kws, "cdb_query_batch", KW_NONE_EMPTY);
        std::lock_guard<std::mutex> g(ix.mu);
        DeviceScope dscope(ix);
        const double t0 = wall_ms();
        hipStream_t s = ix.stream;
        const Rebased kw = rebase(kws);
        const DeviceKeywords d = upload_keywords(ix, kw);
        CDB_HIP(hipStreamSynchronize(s));
        const double t1 = wall_ms();
        const DeviceCsr r = query_batch_on_device(ix, d.pat, d.offs, npat, hits != nullptr);
        CDB_HIP(hipStreamSynchronize(s));
        const double t2 = wall_ms();
        BatchResult res(s);  // (a failed allocation or copy: nothing half-filled leaves the library)
        BatchHits hres(s);
        res.r.npat = npat;
        res.r.nrows = r.nrows;
        res.r.nhits = r.nhits;
        res.r.row_ptr = res.fetch<uint64_t>(ix.q_rowptr.p, npat + 1);
        res.r.ids = res.fetch<int64_t>(ix.q_ids.p, r.nrows);
        res.r.counts = res.fetch<int64_t>(ix.q_counts.p, r.nrows);
        if (hits) {  // (no row: hit_ptr = {0})
            hres.r.hit_ptr = r.nrows ? hres.fetch<uint64_t>(ix.q_hitptr.p, r.nrows + 1) : (uint64_t*)host_alloc(8, true);
            hres.r.offsets = hres.fetch<uint64_t>(ix.q_hitoff.p, r.nhits);
        }
        CDB_HIP(hipStreamSynchronize(s));
        res.hand_over(out);
        if (hits) hres.hand_over(hits);
        ix.qstats.query_ms = wall_ms() - t0;
        ix.qstats.upload_ms = t1 - t0;
        ix.qstats.device_ms = t2 - t1;
        ix.qstats.download_ms = wall_ms() - t2;
        ix.qstats.nhits = r.nhits;
        ix.qstats.nrows = r.nrows;
    });
}

int query_or_impl(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t** ids, int64_t** counts,
                  size_t* nrows, bool ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit) {
    if (!h || !ids || !counts || !nrows || (nkw && !offsets)) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    return guarded_ix(h->ix, [&] {
        Index& ix = h->ix;
        const KeywordList kws{blob, offsets, nkw};
        check_keywords(kws, "cdb_query_or", KW_LIST_NOT_EMPTY | KW_NONE_EMPTY);
        std::lock_guard<std::mutex> g(ix.mu);
        DeviceScope dscope(ix);
        const Rebased kw = rebase(kws);
        const DeviceKeywords d = upload_keywords(ix, kw);
        const DeviceCsr r = ranked ? query_ranked_on_device(ix, d.pat, d.offs, nkw, corr_lo, corr_hi, limit) : query_or_on_device(ix, d.pat, d.offs, nkw);
        download_rows(ix.stream, ix.q_ids.as<int64_t>(), ix.q_counts.as<int64_t>(), r.nrows, ids, counts, nrows);
    });
}
}  // namespace

int cdb::query_and_with_lead(cdb_index* lead, const cdb_key_query* keys, int nkeys, int ranked, int64_t corr_lo, int64_t corr_hi,
                             uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows) {
    Index& ix = lead->ix;
    return guarded_ix(ix, [&] {
        filter_rows_on_lead(ix, QUERY_AND_NAMES, keys, nkeys, nullptr, 0, ranked != 0, corr_lo, corr_hi, limit, [&](hipStream_t s, DeviceCsr r) {
            download_rows(s, ix.q_ids.as<int64_t>(), ix.q_counts.as<int64_t>(), r.nrows, ids, counts, nrows);
        });
    });
}

extern "C" {

int cdb_query_batch(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out) {
    return query_batch_impl(h, blob, offsets, npat, out, nullptr);
}

int cdb_query_batch_offsets(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t npat, cdb_result* out,
                            cdb_hits* hits) {
    if (!hits) return CDB_E_INVALID;
    return query_batch_impl(h, blob, offsets, npat, out, hits);
}

int cdb_query_or(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t** ids, int64_t** counts,
                 size_t* nrows) {
    return query_or_impl(h, blob, offsets, nkw, ids, counts, nrows, false, 0, 0, 0);
}

int cdb_query_ranked(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, int64_t corr_lo, int64_t corr_hi,
                     uint64_t limit, int64_t** ids, int64_t** counts, size_t* nrows) {
    return query_or_impl(h, blob, offsets, nkw, ids, counts, nrows, true, corr_lo, corr_hi, limit);
}

int cdb_query_and(const cdb_key_query* keys, int nkeys, int ranked, int64_t corr_lo, int64_t corr_hi, uint64_t limit, int64_t** ids,
                  int64_t** counts, size_t* nrows) {
    if (!keys || nkeys < 1 || !ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    cdb_index* lead = nullptr;  // the first string key: its stream runs the merge, its handle carries the error
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].index && !lead) lead = keys[k].index;
    if (!lead) return CDB_E_INVALID;
    return cdb::query_and_with_lead(lead, keys, nkeys, ranked, corr_lo, corr_hi, limit, ids, counts, nrows);
}

int cdb_query_spans(cdb_index* h, const char* blob, const uint64_t* offsets, uint64_t nkw, cdb_spans* out) {
    if (!h || !out || (nkw && !offsets)) return CDB_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    return guarded_ix(h->ix, [&] {
        Index& ix = h->ix;
        std::string pat;
        const Rebased kw = rebase_nonempty(KeywordList{blob, offsets, nkw}, pat);
        std::lock_guard<std::mutex> g(ix.mu);
        DeviceScope dscope(ix);
        hipStream_t s = ix.stream;
        SpanResult r;
        if (kw.n()) {
            const DeviceKeywords d = upload_keywords(ix, kw);
            r = query_spans_on_device(ix, d.pat, d.offs, kw.n(), kw.nbytes);
        }
        Spans res(s);
        res.r.ndocs = r.ndocs;
        res.r.nspans = r.nspans;
        res.r.ids = res.fetch<int64_t>(ix.q_ids.p, r.ndocs);  // (no span: no document, span_ptr = {0}, nothing is copied)
        res.r.span_ptr = r.nspans ? res.fetch<uint64_t>(ix.q_rowptr.p, r.ndocs + 1) : (uint64_t*)host_alloc(8, true);
        res.r.begin = res.fetch<uint64_t>(ix.q_keys0.p, r.nspans);
        res.r.end = res.fetch<uint64_t>(ix.q_keys1.p, r.nspans);
        if (r.nspans) CDB_HIP(hipStreamSynchronize(s));
        res.hand_over(out);
    });
}

void cdb_hits_free(cdb_hits* x) {
    if (!x) return;
    host_free(x->hit_ptr);
    host_free(x->offsets);
    std::memset(x, 0, sizeof(*x));
}

void cdb_spans_free(cdb_spans* r) {
    if (!r) return;
    host_free(r->ids);
    host_free(r->span_ptr);
    host_free(r->begin);
    host_free(r->end);
    std::memset(r, 0, sizeof(*r));
}

void cdb_result_free(cdb_result* r) {
    if (!r) return;
    host_free(r->row_ptr);
    host_free(r->ids);
    host_free(r->counts);
    std::memset(r, 0, sizeof(*r));
}

// Single-keyword queries arrive from many host threads at once (the reference serves them from an
// httplib pool under a shared lock, database.cpp:388) and one GPU round trip costs ~100 us, so
// concurrent callers are coalesced: the first caller becomes the leader and resolves everything that
// queued up as ONE batched GPU query, then the next batch, until the queue is empty; the others wait
// for their slice of the result.  No artificial delay is added for a lone caller.
namespace {
struct PendingQuery {
    const char* kw;
    size_t len;
    int64_t *ids = nullptr, *counts = nullptr;
    size_t rows = 0;
    int rc = CDB_OK;
    bool done = false;
};

void run_coalesced(cdb_index* h, std::vector<PendingQuery*>& batch) {
    if (batch.size() == 1) {  // a lone keyword: one wavefront, one launch (query.hip: q_single_kernel)
        PendingQuery* q = batch[0];
        int64_t *ids = nullptr, *counts = nullptr;
        size_t rows = 0;
        bool answered = false;
        const int rc1 = guarded_ix(h->ix, [&] {
            Index& ix = h->ix;
            std::lock_guard<std::mutex> g(ix.mu);
            DeviceScope dscope(ix);
            const double t0 = wall_ms();
            answered = query_single_on_device(ix, q->kw, q->len, &ids, &counts, &rows);
            if (answered) ix.qstats.query_ms = wall_ms() - t0;
        });
        if (rc1 != CDB_OK) {
            q->rc = rc1;
            return;
        }
        if (answered) {
            q->rows = rows;
            q->ids = ids;
            q->counts = counts;
            q->rc = CDB_OK;
            return;
        }
    }
    std::string blob;
    std::vector<uint64_t> offs{0};
    for (auto* q : batch) {
        blob.append(q->kw, q->len);
        offs.push_back(blob.size());
    }
    cdb_result r;
    const int rc = cdb_query_batch(h, blob.data(), offs.data(), batch.size(), &r);
    for (size_t j = 0; j < batch.size(); ++j) {
        PendingQuery* q = batch[j];
        q->rc = rc;
        if (rc != CDB_OK) continue;
        const uint64_t a = r.row_ptr[j], b = r.row_ptr[j + 1];
        q->rows = (size_t)(b - a);
        q->ids = (int64_t*)std::malloc(std::max<size_t>(q->rows, 1) * 8);
        q->counts = (int64_t*)std::malloc(std::max<size_t>(q->rows, 1) * 8);
        if (!q->ids || !q->counts) {
            q->rc = CDB_E_DEVICE;
            continue;
        }
        std::memcpy(q->ids, r.ids + a, q->rows * 8);
        std::memcpy(q->counts, r.counts + a, q->rows * 8);
    }
    if (rc == CDB_OK) cdb_result_free(&r);
}
}  // namespace

int cdb_query(cdb_index* h, const char* keyword, size_t len, int64_t** ids, int64_t** counts, size_t* nrows) {
    if (!h || !ids || !counts || !nrows) return CDB_E_INVALID;
    *ids = nullptr;
    *counts = nullptr;
    *nrows = 0;
    Index& ix = h->ix;
    if (len == 0) {  // index.cpp:239-241
        set_error(ix, "Empty keywords are not allowed");
        return CDB_E_INVALID;
    }
    PendingQuery me{keyword, len};
    if (!ix.coalesce_queries) {
        std::vector<PendingQuery*> one{&me};
        run_coalesced(h, one);
    } else {
        // Leader / follower: whoever finds no leader takes everything queued so far (its own query included),
        // resolves it as ONE batched GPU query and then gives the leadership up — a waiter whose query arrived
        // meanwhile takes over.  A leader therefore never serves more than the batch holding its own query (under
        // sustained load it would otherwise never return), and leadership cannot be stranded by an exception.
        std::unique_lock<std::mutex> lk(ix.qmu);
        ix.qpending.push_back(&me);
        while (!me.done) {
            if (ix.qleader) {
                ix.qcv.wait(lk, [&] { return me.done || !ix.qleader; });
                continue;
            }
            ix.qleader = true;
            std::vector<void*> taken;
            taken.swap(ix.qpending);
            lk.unlock();
            try {
                std::vector<PendingQuery*> batch;
                batch.reserve(taken.size());
                for (void* p : taken) batch.push_back(static_cast<PendingQuery*>(p));
                run_coalesced(h, batch);
            } catch (...) {  // (host allocation failure while assembling the batch)
                const Failure fail = classify_current_exception();
                for (void* p : taken) {
                    PendingQuery* q = static_cast<PendingQuery*>(p);
                    std::free(q->ids);
                    std::free(q->counts);
                    q->ids = q->counts = nullptr;
                    q->rc = fail.code;
                }
                set_error(ix, fail.message);
            }
            lk.lock();
            for (void* p : taken) static_cast<PendingQuery*>(p)->done = true;
            ix.qleader = false;
            ix.qcv.notify_all();
        }
    }
    if (me.rc != CDB_OK) {
        std::free(me.ids);
        std::free(me.counts);
        return me.rc;
    }
    *ids = me.ids;
    *counts = me.counts;
    *nrows = me.rows;
    return CDB_OK;
}

namespace {
int query_batch_device_impl(cdb_index* h, const void* d_blob, const uint64_t* d_offsets, uint64_t npat, cdb_device_result* out,
                            cdb_device_hits* hits) {
    if (!h || !out) return CDB_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    if (hits) std::memset(hits, 0, sizeof(*hits));
    return guarded_ix(h->ix, [&] {
        Index& ix = h->ix;
        std::lock_guard<std::mutex> g(ix.mu);
        DeviceScope dscope(ix);
        const double t0 = wall_ms();
        const DeviceCsr r = query_batch_on_device(ix, static_cast<const uint8_t*>(d_blob), d_offsets, npat, hits != nullptr);
        out->npat = npat;
        out->nrows = r.nrows;
        out->nhits = r.nhits;
        out->d_row_ptr = ix.q_rowptr.as<uint64_t>();
        out->d_ids = ix.q_ids.as<int64_t>();
        out->d_counts = ix.q_counts.as<int64_t>();
        if (hits) {
            hits->d_hit_ptr = ix.q_hitptr.as<uint64_t>();
            hits->d_offsets = ix.q_hitoff.as<uint64_t>();
        }
        ix.qstats.query_ms = wall_ms() - t0;
        ix.qstats.nhits = r.nhits;
        ix.qstats.nrows = r.nrows;
    });
}
}  // namespace

int cdb_query_batch_device(cdb_index* h, const void* d_blob, const uint64_t* d_offsets, uint64_t npat,
                           uint64_t blob_bytes, cdb_device_result* out) {
    (void)blob_bytes;
    return query_batch_device_impl(h, d_blob, d_offsets, npat, out, nullptr);
}

int cdb_query_batch_offsets_device(cdb_index* h, const void* d_blob, const uint64_t* d_offsets, uint64_t npat,
                                   uint64_t blob_bytes, cdb_device_result* out, cdb_device_hits* hits) {
    (void)blob_bytes;
    if (!hits) return CDB_E_INVALID;
    return query_batch_device_impl(h, d_blob, d_offsets, npat, out, hits);
}

}  // extern "C"
