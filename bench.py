#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X string index (BASELINE.json metric:
"SA build GiB/s + batched substring matches/sec").

One step = one pass of the hot path over one batch of synthetic input, per GPU:
    cdb_build_resident : suffix-array construction over the rank's corpus shard (text + document table resident in HBM)
    cdb_query_batch(_offsets)_device : the whole pattern batch against that suffix array (patterns resident in HBM)
    (N > 1) merge of the per-shard match lists into one CSR result over RCCL (cdb_shard_* of the C ABI).
Default workload = BASELINE.json configs[2] ("c2"), the largest single-GPU configuration: 2^23 docs x 1024 B over a Zipf
alphabet of 64 symbols = 8 GiB of text per GPU (8-byte entries), 1 000 000 patterns of length 6..16 with occurrence
offsets (weak scaling: the corpus grows with N).

A plain run sets up, warms up, times --steps steps, writes the last step's results if --dump-outputs DIR is given (the arrays
the caller of the timed path receives, float64 .npy; long ones as a fixed, seeded sample of their positions) and prints its
lines.  Everything else it can measure or check (the legs below marked --full) runs only with --full.

Rank 0 prints TWO stdout lines.  The LAST one is the contract's line and is bounded (< 6 KB, scalar values only):
  "roofline"     — the dominant kernel of the timed region, timed live with HIP events on the library's stream
  "cpu_baseline" — (--full) the CPU restatement of the reference (oracle/, kind "port") timed on this host on a bounded,
                   doc-aligned slice of the SAME corpus (rank 0, N = 1 only)
  "configs"      — (--full) a digest of the other single-GPU configurations of BASELINE.json: c1 (1 GiB ASCII, 100 k patterns; with the
                   literal bit-exact check of the whole array against the CPU oracle: "c1_sa_bit_exact"), c0, utf8_4g
                   (north_star target: 4 GiB UTF-8, reference-compatible order), c4shard (16 GiB UTF-8 = one GPU's share of
                   C4, 10 M patterns, $correlation ranking); at N = 4 / 8 the per-GPU shapes of C3 / C4 run on every rank
The line BEFORE it ({"bench_detail": ...}, also written to bench_detail.json beside this file) carries everything else:
per-kernel times, build statistics, query rooflines and, with --full, PCIe-inclusive legs, cold start, lone-keyword latency,
the whole-corpus CPU baseline of C1.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # BASELINE.json configs[0]: the reference's own CPU-runnable case
    "c0": dict(kind="ascii", docs=10_000, doclen=256, npat=1_000, mmin=4, mmax=16),
    # configs[1] — the configuration the metric is quoted on (default)
    "c1": dict(kind="ascii", docs=1 << 20, doclen=1024, npat=100_000, mmin=4, mmax=16),
    "mid": dict(kind="ascii", docs=1 << 16, doclen=1024, npat=100_000, mmin=4, mmax=16),
    # configs[2]: 8 GiB, Zipf alphabet of 64 symbols, 1 M patterns with occurrence offsets.  The million patterns are
    # 6..16 bytes: on this text a sampled 2..5-byte keyword matches 10^4..4 x 10^8 suffixes, so a million of them would
    # return more rows than any memory holds — the short keywords run as a separate tail of `short` patterns (len 2..5,
    # ~3 x 10^9 hits together, resolved in chunks under the hit budget)
    "c2": dict(kind="zipf", docs=1 << 23, doclen=1024, npat=1_000_000, mmin=6, mmax=16, offsets=True, short=200),
    # north_star target: SA build on 4 GiB of valid UTF-8 (reference_compat order, 8-byte entries)
    "utf8_4g": dict(kind="utf8", bytes=4 << 30, npat=100_000, mmin=4, mmax=16),
    # configs[3] per GPU: 8 GiB ASCII (4 of these = 32 GiB)
    "c3shard": dict(kind="ascii", docs=1 << 23, doclen=1024, npat=100_000, mmin=4, mmax=16),
    # configs[4] per GPU: 16 GiB UTF-8 (8 of these = 128 GiB), 10 M patterns, $correlation ranking
    "c4shard": dict(kind="utf8", bytes=16 << 30, npat=10_000_000, mmin=4, mmax=16, ranked=True),
    # configs[3] / configs[4] as BASELINE.json words them — a FIXED corpus split across the ranks (--scaling strong):
    # 32 GiB ASCII over 4 GPUs, 128 GiB UTF-8 over 8 GPUs with 10 M patterns and $correlation ranking
    # configs[4] in miniature (the 8-rank dress rehearsal on one GPU, tests/test_bench_launch.py): 256 MiB UTF-8 per rank,
    # 10^6 patterns, counts merge + $correlation ranking
    "c4mini": dict(kind="utf8", bytes=256 << 20, npat=1_000_000, mmin=4, mmax=16, ranked=True),
    "c3": dict(kind="ascii", docs=1 << 25, doclen=1024, npat=100_000, mmin=4, mmax=16, total=True),
    "c4": dict(kind="utf8", bytes=128 << 30, npat=10_000_000, mmin=4, mmax=16, ranked=True, total=True),
}
MAX_SHARD_BYTES = 16 << 30  # the largest corpus one MI355X builds (8-byte entries: 128 GiB of suffix array + scratch)


def per_rank_cfg(cfg, world, scaling):
    """This rank's share.  weak: the workload as written, per GPU.  strong: a fixed total cut into `world` doc-aligned
    shards; a share that does not fit one GPU is clamped (and says so: the run is then not the whole corpus)."""
    if scaling != "strong":
        return dict(cfg), None
    c = dict(cfg)
    note = None
    if c["kind"] == "utf8":
        share = c["bytes"] // world
        if share > MAX_SHARD_BYTES:
            note = f"clamped: {share / 2**30:.0f} GiB per GPU does not fit, {MAX_SHARD_BYTES / 2**30:.0f} GiB built"
            share = MAX_SHARD_BYTES
        c["bytes"] = share
    else:
        docs = c["docs"] // world
        if docs * c["doclen"] > MAX_SHARD_BYTES:
            note = f"clamped: {docs * c['doclen'] / 2**30:.0f} GiB per GPU does not fit, {MAX_SHARD_BYTES / 2**30:.0f} GiB built"
            docs = MAX_SHARD_BYTES // c["doclen"]
        c["docs"] = docs
    return c, note

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


class _DevArr:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001 - the GPU box has no .git
        return None


def pmc_traffic(workload=None):
    """HBM bytes per launch from the committed rocprofv3 PMC passes of this same command
    (profiles/traffic_latest.json for the C1 step, profiles/traffic_latest_<workload>.json for the configurations;
    written by tools/summarize_profile.py; FETCH_SIZE x2-corrected as MI355X_MICROARCH.md prescribes).  bench.py cannot
    collect PMC counters itself: the figures are tagged with the profile and commit they were measured at — NOT measured
    in this run."""
    path = os.path.join(ROOT, "profiles", "traffic_latest.json" if workload in (None, "c1") else f"traffic_latest_{workload}.json")
    try:
        return json.load(open(path))
    except (OSError, ValueError):
        return None


def make_corpus(torch, W, cfg, rank, device):
    """Synthetic shard of this rank, generated in HBM.  Returns (text, doc_start numpy u64, n)."""
    if cfg["kind"] == "ascii":
        n = cfg["docs"] * cfg["doclen"]
        return W.random_bytes_torch(n, 12345, 0x20, 0x7E, stream=rank, device=device), W.uniform_docs(cfg["docs"], cfg["doclen"]), n
    if cfg["kind"] == "zipf":
        n = cfg["docs"] * cfg["doclen"]
        return W.zipf_bytes_torch(n, seed=2 + rank, device=device), W.uniform_docs(cfg["docs"], cfg["doclen"]), n
    text, ds = W.utf8_bytes_torch(cfg["bytes"], seed=4 + rank, device=device)
    return text, ds, int(ds[-1])


def describe(cfg, n, ndocs):
    kind = {"ascii": "printable ASCII", "zipf": "Zipf alphabet of 64 symbols", "utf8": "valid UTF-8 (1/2/3-byte code points)"}[cfg["kind"]]
    return (f"{ndocs} docs, {n / 2**30:.3f} GiB of {kind}; {cfg['npat']} patterns len {cfg['mmin']}-{cfg['mmax']}"
            + (" with occurrence offsets" if cfg.get("offsets") else "") + (" + $correlation ranking" if cfg.get("ranked") else ""))


def dominant(prof, builds=None):
    """The kernel with the largest share of the HIP-event time, with its algorithmic bytes per launch.  `builds` = builds the
    profile covers: the per-build figures are what stays comparable when two profilers cut a pass into launches differently."""
    if not prof:
        return None
    name = max(prof, key=lambda k: prof[k]["ms"])
    k = prof[name]
    avg_ms = k["ms"] / max(k["launches"], 1)
    gbs = k["bytes"] / (k["ms"] * 1e-3) / 1e9 if k["ms"] else 0.0
    out = {"bound": "hbm", "kernel": name, "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(gbs / HBM_PEAK_GBS, 4), "avg_launch_ms": round(avg_ms, 4), "launches": k["launches"],
           "algorithmic_bytes_per_launch": k["bytes"] // max(k["launches"], 1),
           "share_of_kernel_time": round(k["ms"] / sum(v["ms"] for v in prof.values()), 3)}
    if builds:
        out["launches_per_build"] = round(k["launches"] / builds, 2)
        out["algorithmic_bytes_per_build"] = int(k["bytes"] // builds)
        out["ms_per_build"] = round(k["ms"] / builds, 3)
    return out


def attach_traffic(roof, tr, note):
    """PMC traffic of the dominant kernel from a committed rocprofv3 profile, in THIS run's launch definition: rocprofv3 counts
    every kernel launch, the library's profiler may merge or split the launches of one pass (bucket groups), so the profile's
    bytes are carried over per BUILD and divided by this run's launches per build — `traffic` and
    `algorithmic_bytes_per_launch` then describe the same launch (85.5 GB measured beside 103.1 GB algorithmic)."""
    if not roof:
        return
    ent = (tr or {}).get("kernels", {}).get(roof["kernel"])
    if not ent:
        roof["traffic"] = None
        return
    per_build = ent["hbm_bytes_per_launch"] * ent.get("launches", 1)
    lpb = roof.get("launches_per_build") or ent.get("launches", 1)
    roof["traffic"] = round(per_build / lpb)
    roof["traffic_per_build"] = round(per_build)
    roof["traffic_over_algorithmic"] = round(per_build / roof["algorithmic_bytes_per_build"], 3) if roof.get("algorithmic_bytes_per_build") else None
    roof["traffic_profile_launches_per_build"] = ent.get("launches", 1)
    roof["traffic_source"] = {k: tr.get(k) for k in ("profile", "commit", "source") if tr.get(k)}
    roof["traffic_note"] = note


def build_stats(g):
    keys = ("rounds", "ext_rounds", "dbl_rounds", "unresolved_after_initial", "sort_passes", "sort_passes_skipped",
            "key_symbols", "symbol_bits", "alphabet", "isa_built", "bucketed", "bucket_groups", "segmented", "key_layout", "root_folded", "compat_rotations", "group_fallbacks", "self_check_fallbacks", "dense_key_retries", "bucket_low_digits",
            "fused_records", "sweep_records", "gen_prebased", "vl_key_bits", "partial_levels", "list_rounds", "pairclass_fused", "group_sorts", "group_sort_fallbacks", "vl_avg_len", "vl_rate", "vl_est_unresolved")
    out = {}
    for k in keys:
        try:
            out[k] = g.stat(k)
        except KeyError:
            pass
    return out


def query_traffic():
    """Committed counters of the query kernels and the measured random-sector ceiling (profiles/query_traffic_latest.json, written
    by tools/query_pmc.sh: memory-side read requests of the L2 per batch from rocprofv3 PMC passes of this same command, and
    tools/experiments/gather_ceiling.hip).  Like roofline.traffic: tagged with its profile, NOT measured in this run."""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "query_traffic_latest.json")))
    except (OSError, ValueError):
        return None


def query_roofline(torch, r, npat, n, width, query_s, device, prof=None, workload=None, stored_entry_bytes=None):
    """The batched search (index.cpp:260-287) against the roofline that bounds it: the RANDOM-SECTOR rate of the memory system, not
    its streaming bandwidth.  peak = the best rate tools/experiments/gather_ceiling.hip reaches on a working set of this size
    (dependent or independent random 64-byte-sector reads, 1-32 waves per CU); achieved = memory-side read requests of q_search per
    batch (committed PMC profile of this workload: TCC_EA0_RDREQ, one per random sector read — calibrated on the same program) ÷ the
    kernel's duration by HIP events in THIS run.  The probes that never leave the LDS pivot table or the L2 are not in it."""
    levels = max(1, math.ceil(math.log2(max(n, 2))))
    out = {"bound": "hbm-random-sector", "patterns_per_s": round(npat / query_s, 1), "probes_per_s": round(npat * 2 * levels / query_s, 1),
           "levels": levels, "hits": int(r.nhits), "rows": int(r.nrows), "achieved": None, "peak": None, "unit": "G sectors/s", "frac": None}
    qt = query_traffic()
    ent = ((qt or {}).get("batches", {}).get(workload) or {})
    k = (ent.get("kernels") or {}).get("q_search_fast_kernel")
    ps = (prof or {}).get("q_search")
    if k and ps and ps["launches"] and ent.get("patterns") == npat:
        ms = ps["ms"] / ps["launches"]
        ws_gb = n * (1 + (stored_entry_bytes or width)) / 1e9
        tab = {float(g_): v for g_, v in qt["ceiling"]["G_sectors_per_s_by_working_set_GB"].items()}
        near = min(tab, key=lambda g_: abs(math.log(max(g_, 1e-3) / max(ws_gb, 1e-3))))
        req = k["TCC_EA0_RDREQ_sum"]
        out.update({"kernel": "q_search", "achieved": round(req / (ms * 1e-3) / 1e9, 2), "peak": tab[near], "frac": round(req / (ms * 1e-3) / 1e9 / tab[near], 4),
                    "kernel_ms": round(ms, 4), "memory_requests_per_batch": req, "memory_requests_per_pattern": round(req / npat, 1),
                    "l2_hit_share_of_l1_misses": round(1 - req / max(k.get("TCP_TCC_READ_REQ_sum", req), 1), 3),
                    "working_set_GB": round(ws_gb, 1), "peak_measured_at_working_set_GB": near,
                    "traffic_source": f"{qt.get('profile')} (committed rocprofv3 PMC pass of this workload + gather_ceiling.hip; not measured in this run)"})
    else:
        out["note"] = "no committed counters for this workload / batch size: rates only"
    return out


def run_config(torch, capi, W, name, rank, device, local_rank, reps=2, make_merger=None, agree=None, merge_mode="counts",
               dist=None, world=1, extras=None, in_turn=None):
    """One of the non-default configurations: build (1 warm-up + reps) and query (1 warm-up + reps), HBM-resident."""
    cfg = WORKLOADS[name]
    clamp_note = None
    if cfg.get("total"):  # BASELINE configs[3] / [4] as worded: a FIXED corpus cut into `world` doc-aligned shards
        total_bytes = cfg["bytes"] if cfg["kind"] == "utf8" else cfg["docs"] * cfg["doclen"]
        cfg, clamp_note = per_rank_cfg(cfg, world, "strong")
    if make_merger is not None and merge_mode == "full" and cfg["npat"] > 1_000_000:
        # full all-gatherv merge: every rank ends up holding the merged rows of ALL shards; 10^7 patterns x N shards would
        # be ~10^9 rows per rank — the batch is cut to 10^6 patterns (the counts-only merge runs the whole batch)
        cfg = dict(cfg, npat=1_000_000)
    t_gen = time.perf_counter()
    text, ds, n = (in_turn or (lambda f: f()))(lambda: make_corpus(torch, W, cfg, rank, device))
    ndocs = len(ds) - 1
    d_ds = torch.from_numpy(ds.astype(np.int64)).to(device)
    d_ids = torch.arange(ndocs, dtype=torch.int64, device=device) + rank * ndocs
    miss = 0xFF if cfg["kind"] == "utf8" else 0x7F
    d_blob, d_offs, nbytes = (in_turn or (lambda f: f()))(lambda: W.sample_patterns_torch(
        text, d_ds, cfg["npat"], cfg["mmin"], cfg["mmax"], seed=99, miss_byte=miss, utf8=cfg["kind"] == "utf8"))
    torch.cuda.synchronize()
    # (by now this process has released VRAM — the main run's tensors and block cache — so the first build of a configuration
    #  is served recycled pages, which the driver scrubs when they are allocated again: 53 ms per GiB against 7.5 ms per GiB for
    #  untouched VRAM, tools/experiments/alloc_cost.hip.  A process that builds on untouched VRAM — server.cpp:44's start-up
    #  build — pays 1.1 x a warm build: tools/big_one.py)
    torch.cuda.empty_cache()
    t_gen = time.perf_counter() - t_gen
    capi.load_library().cdb_release_cached_memory()
    capi.memory_reset_peak()
    g = capi.GpuStringIndex(device=local_rank)
    g.set_option("profile", 1)
    out = {"workload": f"{name}: " + describe(cfg, n, ndocs), "generate_s": round(t_gen, 2)}
    if cfg.get("total"):
        out["workload"] += (f" per GPU; fixed corpus of {total_bytes / 2**30:.0f} GiB split into {world} doc-aligned shards (--scaling strong)"
                            + (f" ({clamp_note})" if clamp_note else ""))
        out["scaling"] = "strong"
    try:
        bms = []
        for i in range(reps + 1):
            if i == 1:
                g.profile_reset()
            t = time.perf_counter()
            g.build_resident(text.data_ptr(), d_ds.data_ptr(), d_ids.data_ptr(), ndocs)
            bms.append((time.perf_counter() - t) * 1e3)
        prof_build = g.profile()
        out["sa_width"] = g.sa_width
        out["dtype"] = "u64" if g.sa_width == 8 else "u32"
        out["build_ms"] = [round(x, 2) for x in bms[1:]]
        out["first_build_ms_incl_allocation"] = round(bms[0], 1)
        out["first_build_vram"] = "recycled: released by this process just before, scrubbed by the driver on re-allocation (untouched VRAM: ~1.1 x a warm build, DESIGN.md §5)"
        out["sa_build_GiB_per_s"] = round(n / 2**30 / (min(bms[1:]) * 1e-3), 3)
        out["build_stats"] = build_stats(g)
        out["roofline"] = dominant(prof_build, builds=reps)
        attach_traffic(out["roofline"], pmc_traffic(name), "committed PMC profile of this configuration (not measured in this run)")
        mem_in_use, mem_peak, _ = capi.memory_stats()
        out["peak_hbm_bytes"] = int(mem_peak + n)   # library allocations at their peak + the caller's resident text
        out["index_hbm_bytes"] = int(mem_in_use + n)
        out["hbm_note"] = ("peak = most device memory the library held during a build (index + scratch) + the resident text; index = what "
                           "stays after it.  A rebuild beside a serving index (database.cpp:276-280) needs index + peak <= 288 GB")
        kern_ms = sum(v["ms"] for v in prof_build.values()) / reps
        kern_bytes = sum(v["bytes"] for v in prof_build.values()) / reps
        out["build_kernels_ms"] = round(kern_ms, 2)
        out["build_algorithmic_bytes_per_suffix"] = round(kern_bytes / n, 1)
        out["build_algorithmic_GBps_over_kernel_time"] = round(kern_bytes / (kern_ms * 1e-3) / 1e9, 1) if kern_ms else None
        wall_ms = min(bms[1:])
        out["build_algorithmic_GBps_over_wall_time"] = round(kern_bytes / (wall_ms * 1e-3) / 1e9, 1)
        out["build_frac_of_hbm_peak_over_wall_time"] = round(kern_bytes / (wall_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        out["kernel_time_share_of_wall"] = round(kern_ms / wall_ms, 3)
        out["kernels_ms"] = {k: round(v["ms"] / reps, 3) for k, v in sorted(prof_build.items(), key=lambda kv: -kv[1]["ms"])[:8]}
        qms = []
        r = None
        for i in range(reps + 1):
            t = time.perf_counter()
            if cfg.get("offsets"):
                r, _hx = g.query_batch_offsets_device(d_blob.data_ptr(), d_offs.data_ptr(), cfg["npat"], nbytes)
            else:
                r = g.query_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), cfg["npat"], nbytes)
            qms.append((time.perf_counter() - t) * 1e3)
        if make_merger is not None and agree(True):  # N > 1: the shards' match lists merged over RCCL (cdb_comm_merge);
            merger = make_merger(g)                  # collective — entered only when every rank got this far
            out["merge_ms"] = None
            mms = []
            for i in range(reps + 1):
                t = time.perf_counter()
                mres = merger.merge(r, cfg["npat"])
                mms.append((time.perf_counter() - t) * 1e3)
            out["merge_ms"] = [round(x, 3) for x in mms[1:]]
            out["merge"] = merger.note
            if hasattr(mres, "nrows_total"):
                out["merged_rows"] = int(mres.nrows_total)
            else:
                out["merged_rows"] = int(getattr(mres, "nrows", 0)) if not isinstance(mres, tuple) else int(mres[0][-1].item())
            if dist is not None and world > 1:  # rows every rank contributes (its slice of the merged CSR)
                mine = torch.tensor([int(r.nrows)], dtype=torch.int64, device=device if dist.get_backend() == "nccl" else "cpu")
                allr = [torch.zeros_like(mine) for _ in range(world)]
                dist.all_gather(allr, mine)
                out["rows_per_rank"] = [int(x.item()) for x in allr]
            merger.close()
        out["query_ms"] = [round(x, 3) for x in qms[1:]]
        out["query_patterns_per_s"] = round(cfg["npat"] / (min(qms[1:]) * 1e-3), 1)
        out["query_hits_per_batch"] = int(r.nhits)
        out["query_rows_per_batch"] = int(r.nrows)
        out["query_roofline"] = query_roofline(torch, r, cfg["npat"], n, g.sa_width, min(qms[1:]) * 1e-3, device, prof=g.profile(), workload=name,
                                               stored_entry_bytes=g.stat("sa_bytes_per_entry"))
        if cfg.get("short"):
            out["short_patterns"] = short_tail(torch, W, g, text, d_ds, cfg, miss)
        if cfg.get("ranked"):
            # full $correlation ranking (interface.cpp:78-146) of the union over a keyword list: OR-merge, filter, rank
            nkw = 100_000
            hb = d_blob[: int(d_offs[nkw].item())].cpu().numpy()
            ho = d_offs[: nkw + 1].cpu().numpy().astype(np.uint64)
            kws_blob, kws_offs = hb, ho
            t = time.perf_counter()
            rids, rcnt = g.query_ranked_arrays(kws_blob, kws_offs, 1, 1 << 62, 1000, rows=True)
            out["ranked"] = {"keywords": nkw, "limit": 1000, "rows": len(rids), "ms": round((time.perf_counter() - t) * 1e3, 2),
                             "note": "cdb_query_ranked: host keyword list in, top rows out (PCIe-inclusive)"}
            if dist is not None and world > 1:
                # global $correlation ranking over the shards (object ids are disjoint: every shard's own top `limit` rows
                # hold its share of the global top `limit`): gather the shard lists, rank once more
                t = time.perf_counter()
                pad = torch.full((2, 1000), -1, dtype=torch.int64)
                pad[0, :len(rids)] = torch.from_numpy(rids)
                pad[1, :len(rcnt)] = torch.from_numpy(rcnt)
                pad = pad.to(device if dist.get_backend() == "nccl" else "cpu")
                allp = [torch.empty_like(pad) for _ in range(world)]
                dist.all_gather(allp, pad)
                cat = torch.cat(allp, 1).cpu().numpy()
                keep = cat[1] >= 0
                order = np.lexsort((cat[0][keep], -cat[1][keep]))[:1000]
                out["ranked"]["global"] = {"rows": int(len(order)), "top_count": int(cat[1][keep][order[0]]) if len(order) else 0,
                                           "ms": round((time.perf_counter() - t) * 1e3, 2),
                                           "note": "per-shard top lists all-gathered and ranked (descending count, ties ascending id)"}
        out["order_proof"] = proof_block(g)   # (of the last build; it ran beside the queries above)
        out["verify"] = verify_block(g)
        if extras is not None:
            try:
                extras.before_close(g, text, ds, np.arange(ndocs, dtype=np.int64) + rank * ndocs, d_blob, d_offs, nbytes,
                                    cfg["npat"], n, out)
            except Exception as e:  # noqa: BLE001
                out["c1_extras_error"] = repr(e)[:300]
    except Exception:
        if agree is not None and "merge_ms" not in out and "query_ms" not in out:
            agree(False)  # (the other ranks must not wait for this one in the merge)
        raise
    finally:
        g.close()
        del text, d_blob, d_offs, d_ds, d_ids
        torch.cuda.empty_cache()
        capi.load_library().cdb_release_cached_memory()
    if extras is not None:
        extras.after_close(out, ndocs, cfg.get("doclen", 1024))
    return out


def short_tail(torch, W, g, text, d_ds, cfg, miss):
    """The short-pattern tail of SURVEY §8(d)'s C2 (m from 2): keywords of 2..5 bytes match 10^4..10^8 suffixes each here; the
    batch is resolved in chunks of patterns under the hit budget, results (rows and occurrence offsets) stay in HBM."""
    ns = cfg["short"]
    sb_, so_, snb = W.sample_patterns_torch(text, d_ds, ns, 2, 5, seed=5, miss_byte=miss)
    torch.cuda.synchronize()
    sms = []
    for i in range(2):
        t = time.perf_counter()
        rs, _hs = g.query_batch_offsets_device(sb_.data_ptr(), so_.data_ptr(), ns, snb)
        sms.append((time.perf_counter() - t) * 1e3)
    return {"patterns": ns, "len": "2-5", "ms": [round(x, 2) for x in sms], "hits": int(rs.nhits), "rows": int(rs.nrows),
            "hits_per_s": round(int(rs.nhits) / (min(sms) * 1e-3), 1),
            "note": "with occurrence offsets, device-resident; chunked under query_hit_budget (2^31 hits)"}


def proof_block(g, timeout_ms=180_000):
    """The order proof behind the last build (option self_check = 3, default: every adjacent pair against the text on a helper
    thread, AFTER the build returned — verify.hip: proof_start): waits for it and reports what it found."""
    st = g.proof_wait(timeout_ms)
    return {"state": {0: "not started", 1: "still running", 2: "proved", 3: "damage found and repaired", 4: "repair failed",
                      5: "cancelled", 6: "could not run"}.get(st, str(st)),
            "order_proved": bool(g.stat("order_proved")), "proof_ms": round(g.stat("proof_ms"), 2), "pairs": int(g.stat("proof_pairs")),
            "bad_pairs": int(g.stat("proof_bad_pairs")), "self_check_fallbacks": int(g.stat("self_check_fallbacks")),
            # pairs whose first differing bytes lie on both sides of 0x80 (reference-compat order: judged by the size of their bucket,
            # the proof's second stage) / pairs left unjudged
            "mixed_pairs": int(g.stat("proof_mixed_pairs")), "skipped_pairs": int(g.stat("proof_skipped_pairs"))}


def verify_block(g):
    """cdb_verify: the GPU's own adjacent-pair sweep over the whole published array (verify.hip)."""
    v = g.verify()
    return {"invalid_entries": int(v["invalid_entries"]), "inversions": int(v["inversions"]),
            "tie_violations": int(v["tie_violations"]), "entry_sum_ok": bool(v["entry_sum"] == v["expected_entry_sum"])}


def c0_sweep(W):
    """C0 in full on the CPU port with the build's thread count swept (the reference spawns hardware_concurrency() spinning
    workers, index.cpp:225 — oversubscription is visible in the sweep).  Returns (MiB/s by threads, best count, 1-thread q/s)."""
    from oracle import OracleIndex
    cores = os.cpu_count() or 1
    c0 = WORKLOADS["c0"]
    blob0, ds0 = W.ascii_corpus(c0["docs"], c0["doclen"], seed=12345)
    ids0 = np.arange(c0["docs"], dtype=np.int64)
    sweep = {}
    for th in sorted({min(8, cores), min(32, cores), cores}):
        o = OracleIndex()
        o.add_bulk(ids0, blob0, ds0)
        t = time.perf_counter()
        o.build(th)
        sweep[str(th)] = round(len(blob0) / 2**20 / (time.perf_counter() - t), 3)
    pb0, po0 = W.sample_patterns(blob0, ds0, c0["npat"], c0["mmin"], c0["mmax"], seed=99)
    t = time.perf_counter()
    o.query_batch(pb0, po0, nthreads=1, want_rows=False)
    return sweep, int(max(sweep, key=lambda k: sweep[k])), c0["npat"] / (time.perf_counter() - t)


def cpu_baseline(W, host_text, doclen, budget_s=32.0, full_budget_s=300.0, gpu_check=None, corpus="bench corpus", c0=None,
                 mmin=4, mmax=16, whole_bytes=None):
    """CPU restatement of the reference (oracle/cpu_ref.cpp, kind "port") on this host, as BASELINE.md §3 plans:
    C0 in full with the thread count swept (c0_sweep), then the largest prefix of `host_text` (documents of `doclen` bytes)
    that builds within the budget, with the query leg on that same index — and, when `full_budget_s` allows, the whole of
    `host_text` with the literal bit-exact check against the GPU's array (`gpu_check`).  `whole_bytes`: size of the
    configuration `host_text` is a slice of (C2: 8 GiB) — the rate is then the slice's, labelled as such."""
    from oracle import OracleIndex
    cores = os.cpu_count() or 1
    sweep, best_th, c0_q1 = c0 if c0 is not None else c0_sweep(W)
    c0 = WORKLOADS["c0"]
    # ---- prefix of the bench corpus: x4 until the next step would leave the budget
    out = {"unit": "GiB/s", "kind": "port", "c0_build_MiB_per_s_by_threads": sweep,
           "c0_query_patterns_per_s_1thread": round(c0_q1, 1)}
    if host_text is None:
        out.update({"value": round(max(sweep.values()) / 1024, 6), "cores": best_th, "sample": "C0 in full (10k docs x 256 B)"})
        return out
    nd = 1 << 13
    spent = 0.0
    tb = None
    while True:
        ds = W.uniform_docs(nd, doclen)
        blob = host_text[: nd * doclen]
        if nd * doclen == (32 << 20) and cores > 8:
            # the thread count that is best on 10 k tiny documents (C0) is not the best on a real slice: sweep it once here, at
            # 32 MiB (about 2 s per build), and keep the winner for the larger prefixes and the whole corpus
            by_th = {}
            for th in sorted({8, 16, 32, 64} & set(range(1, cores + 1))):
                o = OracleIndex()
                o.add_bulk(np.arange(nd, dtype=np.int64), blob, ds)
                t = time.perf_counter()
                o.build(th)
                by_th[th] = time.perf_counter() - t
                spent += by_th[th]
            best_th = min(by_th, key=by_th.get)
            out["slice_32MiB_build_MiB_per_s_by_threads"] = {str(k): round(32 / v, 3) for k, v in by_th.items()}
            tb = by_th[best_th]
        else:
            o = OracleIndex()
            o.add_bulk(np.arange(nd, dtype=np.int64), blob, ds)
            t = time.perf_counter()
            o.build(best_th)
            tb = time.perf_counter() - t
            spent += tb
        if spent + 4.5 * tb > budget_s or (nd * 4) * doclen > len(host_text):
            break
        nd *= 4
    npat = 100_000

    def query_leg(o, blob, ds):
        spb, spo = W.sample_patterns(blob, ds, npat, mmin, mmax, seed=99)
        t = time.perf_counter()
        o.query_batch(spb, spo, nthreads=1, want_rows=False)
        tq1 = time.perf_counter() - t
        t = time.perf_counter()
        o.query_batch(spb, spo, nthreads=cores, want_rows=False)
        return tq1, time.perf_counter() - t

    tq1, tqa = query_leg(o, blob, ds)
    prefix = {
        "value": round(nd * doclen / 2**30 / tb, 6),
        "cores": best_th,
        "host_threads_available": cores,
        "sample": f"first {nd} docs ({nd * doclen / 2**20:.0f} MiB) of the {corpus}, SA build with {best_th} threads (the best of "
                  f"the sweeps); {npat} patterns len {mmin}-{mmax} sampled from that prefix, queried on that same index"
                  + (f"; the rate of this slice stands for the {whole_bytes / 2**30:.0f} GiB corpus (linear extrapolation, SURVEY §8(d): an "
                     f"upper bound for the CPU, whose comparison sort is n log n)" if whole_bytes else ""),
        "build_s": round(tb, 3),
        "query_patterns_per_s_1thread": round(npat / tq1, 1),
        "query_patterns_per_s_allcores": round(npat / tqa, 1),
    }
    out.update(prefix)
    # ---- the whole bench corpus once per run when the prefix predicts it finishes in bounded time (the
    # reference's sort is n log n: x (full / prefix) x 1.3), with the query leg on that same index — the index the GPU's
    # matches/s are measured on.  The prefix figures stay in the line as the fast fallback.
    full_docs = len(host_text) // doclen
    predicted = tb * (full_docs / nd) * 1.3
    if full_docs > nd and full_budget_s > 0 and predicted <= full_budget_s:
        del o
        ds = W.uniform_docs(full_docs, doclen)
        o = OracleIndex()
        o.add_bulk(np.arange(full_docs, dtype=np.int64), host_text[: full_docs * doclen], ds)
        t = time.perf_counter()
        o.build(best_th)
        tbf = time.perf_counter() - t
        tq1, tqa = query_leg(o, host_text[: full_docs * doclen], ds)
        if gpu_check is not None:
            # BASELINE config 1's "bit-exact SA check" taken literally (index.cpp:209-231 vs cdb_sa_copy): the oracle's complete array,
            # ties in the canonical order of SURVEY §8(c), against the array the GPU built in the timed region — and the rows of the
            # whole pattern batch.  The oracle is the checker here, outside the timed region.
            try:
                t = time.perf_counter()
                o.canonicalize(cores)
                gs = gpu_check["sa"]
                osa = o.sa_view()
                same = bool(osa.dtype == gs.dtype and osa.shape == gs.shape and np.array_equal(osa, gs))
                orp, oi, oc, ohits = o.query_batch(gpu_check["pb"], gpu_check["po"], nthreads=cores)
                grp, gi, gc, ghits = gpu_check["rows"]
                rows_same = bool(ohits == ghits and np.array_equal(orp, grp) and np.array_equal(oi, gi) and np.array_equal(oc, gc))
                out["sa_bit_exact"] = same
                out["rows_bit_exact"] = rows_same
                out["bit_exact_check"] = {"entries": int(len(gs)), "entry_bytes": int(gs.dtype.itemsize), "patterns": int(len(orp) - 1),
                                             "rows": int(len(oi)), "hits": int(ohits), "seconds": round(time.perf_counter() - t, 2),
                                             "note": "oracle array (ties canonicalised) == cdb_sa_copy of the GPU build, element for element; "
                                                     "oracle rows == cdb_query_batch rows for the whole batch"}
            except Exception as e:  # noqa: BLE001
                out["sa_bit_exact"] = None
                out["bit_exact_check"] = {"error": repr(e)[:300]}
        out.update({
            "value": round(full_docs * doclen / 2**30 / tbf, 6),
            "sample": f"the WHOLE {corpus} ({full_docs} docs, {full_docs * doclen / 2**20:.0f} MiB), SA build with {best_th} threads (the "
                      f"best of the sweeps); {npat} patterns len {mmin}-{mmax} sampled from it, queried on that same index",
            "build_s": round(tbf, 3),
            "query_patterns_per_s_1thread": round(npat / tq1, 1),
            "query_patterns_per_s_allcores": round(npat / tqa, 1),
            "prefix_sample": {k: prefix[k] for k in ("value", "sample", "build_s", "query_patterns_per_s_1thread", "query_patterns_per_s_allcores")},
        })
    else:
        if not whole_bytes:
            out["full_corpus_skipped"] = f"predicted {predicted:.0f} s > budget {full_budget_s:.0f} s" if full_docs > nd else "prefix is the corpus"
    return out


CPU_SLICE_BYTES = 256 << 20   # the headline's CPU leg sees at most this much of the corpus (it stops earlier on its time budget)
SHORT_LINE_LIMIT = 6000       # bytes; the driver keeps the last ~8 KB of stdout — the final line must fit with room to spare


class C1Extras:
    """What only BASELINE config 1 carries (1 GiB of text, 4-byte entries: small enough to hold on the host): the lone-keyword
    latency of database.cpp:392's call, the PCIe-inclusive legs through the host entry points, and the literal bit-exact check
    of the whole array against the CPU oracle.  Runs on the index of the c1 block (or on the timed one under --workload c1)."""

    def __init__(self, torch, capi, W, args):
        self.torch, self.capi, self.W, self.args = torch, capi, W, args
        self.host_text = self.gpu_check = None

    def before_close(self, g, text, doc_start, ids, d_blob, d_offs, nbytes, npat, n, out):
        args, capi, W = self.args, self.capi, self.W
        self.host_text = host_text = text.cpu().numpy()
        pb = d_blob[:nbytes].cpu().numpy()
        po = d_offs.cpu().numpy().astype(np.uint64)
        # the call database.cpp:392 makes: ONE keyword through cdb_query (one wavefront, host-mapped result)
        try:
            kws = [bytes(host_text[p:p + 8]) for p in range(1000, 1000 + 97 * 64, 97)]
            for kw in kws[:8]:
                g.query(kw)
            lat = []
            for kw in kws:
                t = time.perf_counter()
                g.query(kw)
                lat.append((time.perf_counter() - t) * 1e6)
            lat.sort()

            def pct(a):
                return {"median": round(float(a[len(a) // 2]), 2), "p10": round(float(a[len(a) // 10]), 2), "p90": round(float(a[(len(a) * 9) // 10]), 2)}

            sq = dict(pct(lat), keywords=len(kws), note="cdb_query through the Python ctypes binding, 8-byte keywords, one caller")
            sq["c_caller"] = dict(pct(np.sort(g.query_latency_us(kws, reps=32))),
                                  note="timed inside the library (cdb_debug_query_latency): what a C++ caller such as database.cpp:392 sees; "
                                       "median over 32 calls per keyword; DEFAULT options (resident_query = 2: keywords arriving back to back "
                                       "go to the resident workgroup after 6 calls less than 1 ms apart)")
            for mode, key in ((1, "resident"), (0, "launched")):   # the resident workgroup forced on / off (one launch per keyword)
                g.set_option("resident_query", mode)
                for kw in kws[:8]:
                    g.query(kw)
                sq[key] = dict(pct(np.sort(g.query_latency_us(kws, reps=32))), note=f"option resident_query = {mode}, timed like c_caller")
            g.set_option("resident_query", 2)
            out["single_query_us"] = sq
        except Exception as e:  # noqa: BLE001
            out["single_query_us"] = {"error": repr(e)[:200]}
        if not args.no_pcie:
            try:
                out["pcie_inclusive"] = pcie_inclusive(capi, W, host_text, doc_start, ids, pb, po, n, npat)
                # SURVEY §8(d) defines the metric INCLUDING the transfers: host column in, index built (cdb_build_view), and host
                # patterns in, host rows out (cdb_query_batch)
                out["sa_build_GiB_per_s_incl_h2d"] = out["pcie_inclusive"]["build_view_GiB_per_s"]
                out["pcie_inclusive_query_patterns_per_s"] = out["pcie_inclusive"]["query_patterns_per_s"]
            except Exception as e:  # noqa: BLE001 - reported, the block stands
                out["pcie_inclusive"] = {"error": repr(e)[:300]}
        if not args.no_cpu_baseline and args.cpu_full_budget > 0:
            try:  # the array and rows of the index just built, for the literal bit-exact check in the CPU leg
                self.gpu_check = {"sa": g.sa(), "rows": g.query_batch(pb, po), "pb": pb, "po": po}
            except Exception as e:  # noqa: BLE001
                out["bit_exact_check"] = {"error": "fetching the GPU array: " + repr(e)[:200]}

    def after_close(self, out, ndocs, doclen):
        if self.args.no_pcie or not isinstance(out.get("pcie_inclusive"), dict) or "error" in out["pcie_inclusive"]:
            return
        # what the SHIM's build() really calls (shim/index.cpp: cdb_build_views over one std::string per document,
        # database.cpp:262-264): the C++ caller of tests/cpp at this shape, in a process of its own
        out["pcie_inclusive"]["build_views"] = host_caller("views", ndocs, doclen, 3)
        # ... and at the north-star size: 4 M separately allocated strings of valid UTF-8 (4 GiB), warm (repetitions 1-2)
        out["pcie_inclusive"]["build_views_4g"] = host_caller("views", 4 << 20, 1024, 2, "utf8")

    def cpu_leg(self, out, W, c0, args, doclen, top):
        """The CPU port over the WHOLE C1 corpus (when its prefix predicts it fits the budget) + the bit-exact check."""
        cb = cpu_baseline(W, self.host_text, doclen, full_budget_s=args.cpu_full_budget, gpu_check=self.gpu_check, c0=c0, corpus="C1 corpus")
        for k in ("sa_bit_exact", "rows_bit_exact", "bit_exact_check"):
            if k in cb:
                out[("c1_" if top else "") + k] = cb.pop(k)
        out["cpu_baseline"] = cb
        self.host_text = self.gpu_check = None


def _clip(x, limit):
    x = str(x)
    return x if len(x) <= limit else x[: limit - 3] + "..."


def short_line(out):
    """The FINAL stdout line: the contract's keys with scalar values only, a digest of the other configurations, and nothing
    else — everything else lives in bench_detail.json (and in the stdout line before this one).  Bounded: the driver keeps
    the last ~8 KB of stdout, and a line it cannot parse is an unmeasured round."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "commit", "rccl_ranks", "rows_per_rank", "merged_rows", "sa_build_only_GiB_per_s", "sa_build_GiB_per_s_incl_h2d",
            "query_patterns_per_s", "query_hits_per_batch", "query_rows_per_batch", "build_ms_per_step",
            "build_algorithmic_bytes_per_suffix", "build_frac_of_hbm_peak_over_wall_time", "kernel_time_share_of_wall",
            "peak_hbm_bytes", "order_proved", "proof_ms", "c1_sa_bit_exact", "c1_rows_bit_exact", "utf8_256m_sa_bit_exact", "utf8_256m_rows_bit_exact",
            "zipf_256m_sa_bit_exact", "zipf_256m_rows_bit_exact")
    s = {k: out[k] for k in keep if k in out}
    cfg = out.get("config") or {}
    s["config"] = {"workload": _clip(cfg.get("workload", ""), 420), **{k: v for k, v in cfg.items() if k != "workload" and not isinstance(v, (dict, list, str))}}
    roof = out.get("roofline")
    if isinstance(roof, dict):
        r = {k: roof[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "launches",
                                  "algorithmic_bytes_per_launch", "share_of_kernel_time", "traffic_over_algorithmic") if k in roof}
        src = roof.get("traffic_source")
        if isinstance(src, dict):
            r["traffic_source"] = _clip(f"{src.get('profile')} @ {src.get('commit')} (committed rocprofv3 PMC passes of this command; not measured in this run)", 160)
        s["roofline"] = r
    else:
        s["roofline"] = None
    qr = out.get("query_roofline")
    if isinstance(qr, dict):
        s["query_roofline"] = {k: qr[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "patterns_per_s", "probes_per_s", "levels",
                                                  "memory_requests_per_pattern", "kernel_ms") if k in qr}
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = {k: cb[k] for k in ("value", "unit", "cores", "kind", "host_threads_available", "build_s", "query_patterns_per_s_1thread",
                                "query_patterns_per_s_allcores", "error") if k in cb}
        if "sample" in cb:
            c["sample"] = _clip(cb["sample"], 420)
        s["cpu_baseline"] = c
        qa = cb.get("query_patterns_per_s_allcores")
        if qa and out.get("query_patterns_per_s"):
            s["query_vs_cpu_allcores"] = round(out["query_patterns_per_s"] / qa, 1)
    else:
        s["cpu_baseline"] = None
    sc = out.get("mg_selfcheck")
    if isinstance(sc, dict):
        s["mg_selfcheck"] = {k: (_clip(v, 200) if isinstance(v, str) else v) for k, v in sc.items()
                             if k in ("ok", "world", "transport", "cdb_comm_world", "devices_distinct", "share_gpu", "bus_ids",
                                      "merged_rows", "sum_of_local_rows", "error")}
    else:
        s["mg_selfcheck"] = None
    if out.get("merge"):
        s["merge"] = _clip(out["merge"], 200)
    dig = {}
    for name, b in (out.get("configs") or {}).items():
        if not isinstance(b, dict):
            continue
        if "error" in b:
            dig[name] = {"error": _clip(b["error"], 120)}
            continue
        d = {"build_ms": min(b["build_ms"]) if b.get("build_ms") else None, "sa_build_GiB_per_s": b.get("sa_build_GiB_per_s"),
             "frac_over_wall": b.get("build_frac_of_hbm_peak_over_wall_time"),
             "dominant_frac": (b.get("roofline") or {}).get("frac"), "query_patterns_per_s": b.get("query_patterns_per_s"),
             "query_frac": (b.get("query_roofline") or {}).get("frac"),
             "peak_hbm_bytes": b.get("peak_hbm_bytes"), "dtype": b.get("dtype")}
        if isinstance(b.get("order_proof"), dict) and "order_proved" in b["order_proof"]:
            d["order_proved"] = b["order_proof"]["order_proved"]
        v = b.get("verify")
        if isinstance(v, dict):
            d["verify_ok"] = bool(v["invalid_entries"] == 0 and v["tie_violations"] == 0 and v["entry_sum_ok"])
            d["inversions"] = v["inversions"]
        if isinstance(b.get("cpu_baseline"), dict) and "value" in b["cpu_baseline"]:
            d["cpu_GiB_per_s"] = b["cpu_baseline"]["value"]
            d["cpu_query_allcores"] = b["cpu_baseline"].get("query_patterns_per_s_allcores")
        if b.get("sa_build_GiB_per_s_incl_h2d") is not None:
            d["incl_h2d_GiB_per_s"] = b["sa_build_GiB_per_s_incl_h2d"]
        if isinstance(b.get("all_ranks"), dict):
            d["aggregate_GiB_per_s"] = b["all_ranks"].get("sa_build_GiB_per_s_aggregate")
        dig[name] = {k: v for k, v in d.items() if v is not None}
    s["configs"] = dig
    c1 = dig.get("c1") or {}
    if c1.get("cpu_query_allcores") and c1.get("query_patterns_per_s"):
        # north_star: ">= 10 x the CPU reference's matches/sec on 100k batched patterns" = BASELINE config 1, CPU port on all host threads
        s["c1_query_vs_cpu_allcores"] = round(c1["query_patterns_per_s"] / c1["cpu_query_allcores"], 1)
    s["detail"] = "bench_detail.json (written beside bench.py; also the stdout line before this one)"
    # the guard: drop the optional parts, least important first, until the line fits
    for victim in ("build_ms_per_step", "merge", "query_roofline", "rows_per_rank", "configs"):
        if len(json.dumps(s)) <= SHORT_LINE_LIMIT:
            break
        if victim == "configs":
            s["configs"] = {k: {kk: vv for kk, vv in v.items() if kk in ("build_ms", "sa_build_GiB_per_s", "error")} for k, v in dig.items()}
        else:
            s.pop(victim, None)
    return s


def emit(out):
    """Rank 0's output: the whole record to bench_detail.json and to an EARLIER stdout line, then the bounded final line."""
    short = short_line(out)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_detail.json"), "w") as f:
                    json.dump(out, f, indent=1)
            except OSError:
                pass
    print(json.dumps({"bench_detail": out}), flush=True)
    line = json.dumps(short, allow_nan=False)
    assert len(line) <= 8000, len(line)
    print(line, flush=True)


DUMP_SAMPLE = 1 << 19   # positions kept of a longer output array (5 arrays x 2 files x 4 MiB at most: 40 MiB in all)
DUMP_SEED = 20261016


def dump_outputs(torch, out_dir, r, hx, device):
    """--dump-outputs: the arrays the last timed step handed its caller (cdb_query_batch[_offsets]_device: row_ptr, ids, counts
    [, hit_ptr, offsets]) as float64 .npy files (every value is an integer below 2^53: exact).  An array of more than
    DUMP_SAMPLE entries is written at DUMP_SAMPLE positions drawn with a fixed seed from its length, and <name>_index.npy holds
    those positions, so that two builds of the project can be compared output for output."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"row_ptr": (r.d_row_ptr, int(r.npat) + 1), "ids": (r.d_ids, int(r.nrows)), "counts": (r.d_counts, int(r.nrows))}
    if hx is not None:
        arrays.update({"hit_ptr": (hx.d_hit_ptr, int(r.nrows) + 1), "offsets": (hx.d_offsets, int(r.nhits))})
    for name, (ptr, n) in arrays.items():
        vals = np.empty(0, dtype=np.int64)
        if n:
            t = torch.as_tensor(_DevArr(ptr, n, "<i8"), device=device)
            if n > DUMP_SAMPLE:
                idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_SAMPLE, replace=False))
                np.save(os.path.join(out_dir, f"{name}_index.npy"), idx.astype(np.float64))
                t = t[torch.from_numpy(idx).to(device)]
            vals = t.cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), vals.astype(np.float64))


def midsize_bit_exact(torch, capi, W, nbytes=256 << 20):
    """Literal oracle parity on the bucket-wise (>= 2^32-style) build path at a size with real tiles — the siblings of
    `c1_sa_bit_exact` (the same check runs as tests/test_gpu_midsize_oracle.py with more option sets): 256 MiB of
    valid UTF-8 and 256 MiB of Zipf-64 text in documents of ~1 KiB + one long one (8-byte entries), force_big_path, two uneven
    bucket groups, reference_compat = 1 (index.h:66-73, index.cpp:86-126); cdb_sa_copy == oracle array (ties canonicalised),
    element for element, and the rows of 10 000 patterns.  The oracle is the checker, outside every timed region."""
    from oracle import OracleIndex
    out = {}
    threads = min(32, os.cpu_count() or 1)
    for kind in ("utf8", "zipf"):
        key = f"{kind}_{nbytes >> 20}m"
        t0 = time.perf_counter()
        try:
            if kind == "utf8":
                text, ds = W.utf8_bytes_torch(nbytes, seed=41, device="cuda")
                blob = text.cpu().numpy()
                del text
            else:
                blob = W.zipf_bytes_torch(nbytes, seed=43, device="cuda").cpu().numpy()
                ds = W.uniform_docs(nbytes // 1024, 1024)
            torch.cuda.empty_cache()
            mid = len(ds) // 3   # one long document (64 merged: ~64 KiB), so that the entries need more than 32 bits
            ds = np.concatenate([ds[:mid + 1], ds[mid + 64:]]).astype(np.uint64)
            nd, n = len(ds) - 1, int(ds[-1])
            ids = (np.arange(nd, dtype=np.int64) * 5 + 3)[::-1].copy()
            g = capi.GpuStringIndex()
            for k, v in {"force_big_path": 1, "bucket_group_limit": int(n * 0.62), **({"vl_keys": 40} if kind == "zipf" else {})}.items():
                g.set_option(k, v)
            g.add_bulk(ids, blob, ds)
            g.build()
            gsa = g.sa()
            pb, po = W.sample_patterns(blob, ds, 10_000, 2, 14, seed=7, miss_frac=0.1, miss_byte=0xFF if kind == "utf8" else 0x7F)
            grows = g.query_batch(pb, po)
            info = {k: g.stat(k) for k in ("bucketed", "bucket_groups", "sweep_records", "vl_key_bits", "partial_levels", "self_check_fallbacks")}
            proved = g.proof_wait(60_000)
            g.close()
            o = OracleIndex()
            o.add_bulk(ids, blob, ds)
            o.build(threads)
            o.canonicalize(threads)
            osa = o.sa_view()
            same = bool(osa.dtype == gsa.dtype and osa.shape == gsa.shape and np.array_equal(osa, gsa))
            orows = o.query_batch(pb, po, nthreads=threads)
            rows_same = bool(orows[3] == grows[3] and all(np.array_equal(a, b) for a, b in zip(orows[:3], grows[:3])))
            out[key + "_sa_bit_exact"] = same
            out[key + "_rows_bit_exact"] = rows_same
            out[key] = dict(info, entries=int(len(gsa)), entry_bytes=int(gsa.dtype.itemsize), order_proof_state=proved,
                            seconds=round(time.perf_counter() - t0, 1))
            del o, osa, gsa
        except Exception as e:  # noqa: BLE001
            out[key + "_sa_bit_exact"] = None
            out[key] = {"error": repr(e)[:300]}
    return out


def host_caller(*argv, timeout=600):
    """tests/cpp/test_index_shim (the database.cpp-style C++ caller over shim/index.{h,cpp}) in one of its timing modes; returns
    its JSON line.  A process of its own: no torch, no warm block cache."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_index_shim")
    try:
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-C", os.path.dirname(exe), "test_index_shim"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, text=True, timeout=timeout)
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not lines:
            return {"error": (p.stdout + p.stderr)[-300:], "rc": p.returncode}
        return json.loads(lines[-1])
    except Exception as e:  # noqa: BLE001 - reported in the line
        return {"error": repr(e)[:300]}


def pcie_inclusive(capi, W, host_text, doc_start, ids, pb, po, n, npat, reps=3):
    """The same work through the host entry points: cdb_add_bulk (host staging) + cdb_build (H2D of text and tables
    inside the timed call) and cdb_query_batch (patterns up, CSR rows down)."""
    tb, ta = [], []
    g = None
    for _ in range(reps):
        if g is not None:
            g.close()
        g = capi.GpuStringIndex()
        t = time.perf_counter()
        g.add_bulk(ids, host_text, doc_start)
        ta.append(time.perf_counter() - t)
        t = time.perf_counter()
        g.build()
        tb.append(time.perf_counter() - t)
    v = g.verify()  # (the column went through the chunked pinned staging path: the index must be the same sorted permutation)
    verify_ok = bool(v["inversions"] == 0 and v["tie_violations"] == 0 and v["invalid_entries"] == 0 and v["entry_sum"] == v["expected_entry_sum"])
    # the same from the caller's own buffer (cdb_build_view: what string_index's string_views are — no staging memcpy)
    tv = []
    for _ in range(reps):
        g.close()
        g = capi.GpuStringIndex()
        t = time.perf_counter()
        g.build_view(ids, host_text, doc_start)
        tv.append(time.perf_counter() - t)
    v = g.verify()
    verify_ok = verify_ok and bool(v["inversions"] == 0 and v["tie_violations"] == 0 and v["invalid_entries"] == 0 and v["entry_sum"] == v["expected_entry_sum"])
    tq = []
    for _ in range(reps + 1):
        t = time.perf_counter()
        res = g.query_batch(pb, po)
        tq.append(time.perf_counter() - t)
        del res
    out = {"build_view_GiB_per_s": round(n / 2**30 / min(tv), 3), "build_view_ms": [round(x * 1e3, 2) for x in tv],
           "add_bulk_plus_build_GiB_per_s": round(n / 2**30 / (min(ta) + min(tb)), 3),
           "build_GiB_per_s": round(n / 2**30 / min(tb), 3), "build_ms": [round(x * 1e3, 2) for x in tb],
           "add_bulk_ms_host_memcpy": round(min(ta) * 1e3, 1), "build_device_part_ms": round(g.stat("build_ms"), 2), "build_upload_ms": round(g.stat("host_upload_ms"), 2), "build_free_staging_ms": round(g.stat("host_free_ms"), 2), "verify_ok": verify_ok,
           "query_patterns_per_s": round(npat / min(tq[1:]), 1), "query_ms": [round(x * 1e3, 3) for x in tq[1:]],
           "query_split_ms": {"upload": round(g.stat("query_upload_ms"), 3), "device": round(g.stat("query_device_ms"), 3),
                              "download": round(g.stat("query_download_ms"), 3)}}
    g.close()
    return out


def mg_selfcheck(torch, dist, capi, g, merger, rank, world, local_rank, device, coll_device, args, build, d_blob, d_offs, npat):
    """The N > 1 plumbing checked before anything is timed: communicator size, one device per rank, and a small merge whose
    merged row_ptr[-1] equals the all-reduced sum of the ranks' local row counts.  Every rank returns the same verdict
    (`ok` is all-reduced), so a failure ends ALL ranks with a non-zero exit instead of a hang in the timed region."""
    out = {"world": world, "transport": merger.comm.transport if merger.comm is not None else f"torch.distributed/{args.backend}",
           "cdb_comm_world": int(merger.comm.world) if merger.comm is not None else None, "patterns": int(npat)}
    ok = True
    try:
        if merger.comm is not None and int(merger.comm.world) != world:
            ok = False
            out["error"] = f"cdb_comm_world {merger.comm.world} != {world}"
        # one device per rank (PCI bus ids; --share-gpu is the one-GPU stand-in and says so)
        prop = torch.cuda.get_device_properties(device)
        bus = int(getattr(prop, "pci_bus_id", local_rank)) * 256 + int(getattr(prop, "pci_device_id", 0))
        mine = torch.tensor([bus if not args.share_gpu else rank], dtype=torch.int64, device=coll_device)
        alld = [torch.zeros_like(mine) for _ in range(world)]
        if world > 1:
            dist.all_gather(alld, mine)
        else:
            alld = [mine]
        devs = [int(x.item()) for x in alld]
        out["bus_ids"] = [f"{d >> 8:02x}:{d & 255:02x}" for d in devs] if not args.share_gpu else ["shared cuda:0"] * world
        out["devices_distinct"] = len(set(devs)) == world
        out["share_gpu"] = bool(args.share_gpu)
        if not out["devices_distinct"]:
            ok = False
            out["error"] = f"ranks share a device: {devs}"
        r = None
        try:
            build()
            nb = int(d_offs[npat].item())
            r = g.query_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), npat, nb)
        except Exception as e:  # noqa: BLE001
            ok = False
            out["error"] = repr(e)[:300]
        ready = torch.tensor([1 if (ok and r is not None) else 0], dtype=torch.int32, device=coll_device)
        if world > 1:  # (the merge is collective: nobody enters it unless everybody can)
            dist.all_reduce(ready, op=dist.ReduceOp.MIN)
        if not bool(ready.item()):
            raise RuntimeError(out.get("error", "another rank failed before the merge"))
        local_rows = int(r.nrows)
        m = merger.merge(r, npat)
        if merger.comm is not None:
            merged_rows = int(m.nrows_total) if merger.mode == "counts" else int(m.nrows)
        else:
            merged_rows = int(m[0][-1].item())
        t = torch.tensor([local_rows], dtype=torch.int64, device=coll_device)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        out["local_rows"] = local_rows
        out["sum_of_local_rows"] = int(t.item())
        out["merged_rows"] = merged_rows
        if merged_rows != int(t.item()):
            ok = False
            out["error"] = f"merged row_ptr[-1] {merged_rows} != sum of local rows {int(t.item())}"
    except Exception as e:  # noqa: BLE001 - a rank that throws must still reach the all-reduce below
        ok = False
        out["error"] = repr(e)[:300]
    v = torch.tensor([1 if ok else 0], dtype=torch.int32, device=coll_device)
    if world > 1:
        dist.all_reduce(v, op=dist.ReduceOp.MIN)
    out["ok"] = bool(v.item())
    return out


def launch_plan(gpus, env, argv, share_gpu=False, device_count=None):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (WORLD_SIZE unset) must still run N ranks — a
    line that says "n_gpus": 1 for a --gpus 8 command would void a scaling curve.  Returns the command that re-runs this
    script under torch.distributed.run with one rank per GPU, or None when the process is already a rank (or N = 1).
    Exits non-zero when the box has fewer than N GPUs (unless --share-gpu: the one-GPU test of the N > 1 code path)."""
    if gpus < 1:
        raise SystemExit(f"--gpus {gpus}: need at least one GPU")
    if gpus == 1 or "WORLD_SIZE" in env:
        return None
    if not share_gpu:
        if device_count is None:
            import torch
            device_count = torch.cuda.device_count()
        if device_count < gpus:
            raise SystemExit(f"bench.py --gpus {gpus}: only {device_count} GPU(s) visible on this node — refusing to "
                             f"print a line for fewer GPUs than asked for")
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the timed steps: cold start, order-proof leg, verify, short-pattern tail, "
                         "PCIe-inclusive legs, the \"configs\" block, the 256 MiB oracle-parity check and the CPU baseline (the "
                         "--configs and --no-* options below select among these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's query results (rank 0) as DIR/<name>.npy (float64)")
    ap.add_argument("--configs", default="auto",
                    help="comma-separated extra configurations for the \"configs\" block (auto: c2,utf8_4g,c4shard at N = 1 on "
                         "the default workload, c3 at N = 4, c4 at N = 8 — the fixed 32 / 128 GiB corpora split across the ranks; none: skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-full-budget", type=float, default=300.0,
                    help="seconds the CPU baseline may spend on the WHOLE bench corpus (0: prefix only); it runs when the "
                         "128 MiB prefix predicts it fits")
    ap.add_argument("--no-pcie", action="store_true")
    ap.add_argument("--no-proof-leg", action="store_true",
                    help="skip the order-proof leg behind the timed region (one more build + three batches; the rocprofv3 passes of "
                         "tools/profile_round.sh use it so that a profiled run holds exactly --steps builds)")
    ap.add_argument("--no-midsize-check", action="store_true",
                    help="skip the 256 MiB UTF-8 / Zipf oracle-parity check of the bucket-wise path (about a minute of CPU oracle)")
    ap.add_argument("--no-cold-start", action="store_true",
                    help="skip the cold-start leg (a fresh C++ process builds a 4 GiB UTF-8 column from host memory once, before "
                         "this process touches the GPU; N = 1, default workload only)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="rendezvous backend for N > 1 (nccl = RCCL over xGMI; gloo + --share-gpu only exists to "
                         "exercise the N > 1 code path on a one-GPU box)")
    ap.add_argument("--share-gpu", action="store_true", help="all ranks use cuda:0 (testing only)")
    ap.add_argument("--print-launch", action="store_true",
                    help="print the self-launch decision for --gpus N (the torch.distributed.run command, or null) and exit")
    ap.add_argument("--force-merge", action="store_true",
                    help="run the RCCL merge of the N > 1 step with a one-rank communicator (testing the plumbing on one GPU)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: the workload per GPU (default; what the driver's --gpus N runs measure).  strong: a FIXED corpus "
                         "(--workload c3 = 32 GiB, c4 = 128 GiB) generated shard-wise on the devices and split across the ranks")
    ap.add_argument("--merge", default="counts", choices=["counts", "full"],
                    help="N > 1: counts = all-gather of the per-pattern row counts only, every rank keeps its own rows "
                         "(cdb_comm_merge_counts; host / rank-local consumers); full = all-gatherv of all rows to every rank")
    args = ap.parse_args()

    plan = launch_plan(args.gpus, os.environ, sys.argv[1:], share_gpu=args.share_gpu)
    if args.print_launch:
        print(json.dumps({"launch": plan}))
        return
    if plan is not None:
        # `python bench.py --gpus N` without a launcher: become N ranks (one per GPU) and hand rank 0's line through.
        # The child ranks inherit stdout / stderr, the exit code is the job's.
        raise SystemExit(subprocess.call(plan))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the line would report the wrong GPU count")

    cold = None
    if args.full and world == 1 and args.workload == "c2" and args.configs == "auto" and not args.no_cold_start:
        # server.cpp:44: the start-up build of a fresh process — measured FIRST, while this process has not touched the GPU
        # (VRAM a process released just before is scrubbed by the driver on re-allocation: the recycled case the configs
        # blocks measure)
        cold = host_caller("cold", 4 << 30)  # (with string_index::reserve running beside the "ingest": the product path)
        if isinstance(cold, dict) and "error" not in cold:
            # the same start-up without the reservation, for the record (SECOND: its pages are recycled ones)
            cold["without_reserve"] = host_caller("cold", 4 << 30, "noreserve")

    import torch
    import torch.distributed as dist
    from coffeedb_amd import capi, shard, workloads as W

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a MI355X GPU (the HIP path has no CPU fallback)")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    coll_device = device if args.backend == "nccl" else torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group("gloo")

    trace = (lambda m: print(f"[bench rank {rank}] {m}", file=sys.stderr, flush=True)) if os.environ.get("CDB_BENCH_TRACE") else (lambda m: None)
    if os.environ.get("CDB_BENCH_TRACE"):   # (where every thread of a rank that got stuck is: after 45 s, then every 45 s)
        import faulthandler
        faulthandler.dump_traceback_later(45, repeat=True, file=sys.stderr)
    cfg, clamp_note = per_rank_cfg(WORKLOADS[args.workload], world, args.scaling)
    if cfg.get("total") and args.scaling != "strong":
        raise SystemExit(f"--workload {args.workload} is a fixed-size corpus: run it with --scaling strong")
    trace("process group up")

    def in_turn(fn):
        """--share-gpu (several ranks on ONE device, testing only): torch's generation kernels of four or more processes at once
        on one GPU never finish (every rank stuck in its first .item(); two processes are fine) — the ranks take turns."""
        if not (args.share_gpu and world > 1):
            return fn()
        res = None
        for r_ in range(world):
            if r_ == rank:
                res = fn()
                torch.cuda.synchronize()
            dist.barrier()
        return res

    text, doc_start, n = in_turn(lambda: make_corpus(torch, W, cfg, rank, device))
    trace("corpus generated")
    ndocs = len(doc_start) - 1
    npat, mmin, mmax = cfg["npat"], cfg["mmin"], cfg["mmax"]
    ids = np.arange(ndocs, dtype=np.int64) + rank * ndocs
    d_doc_start = torch.from_numpy(doc_start.astype(np.int64)).to(device)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(device)
    small = n <= (2 << 30) and cfg["kind"] == "ascii"
    host_text = text.cpu().numpy() if (rank == 0 and small) else None

    # ---- one pattern batch for every shard (rank 0 samples it from its own text, then broadcast)
    pb = po = None
    if rank == 0:
        if small:
            pb, po = W.sample_patterns(host_text, doc_start, npat, mmin, mmax, seed=99)
            nbytes = len(pb)
        else:
            miss = 0xFF if cfg["kind"] == "utf8" else 0x7F
            b_, o_, nbytes = W.sample_patterns_torch(text, d_doc_start, npat, mmin, mmax, seed=99, miss_byte=miss,
                                                     utf8=cfg["kind"] == "utf8")
        meta = torch.tensor([nbytes], dtype=torch.int64, device=device)
    else:
        meta = torch.zeros(1, dtype=torch.int64, device=device)

    def bcast(t):
        if world == 1:
            return
        if coll_device == t.device:
            dist.broadcast(t, 0)
        else:
            c = t.to(coll_device)
            dist.broadcast(c, 0)
            t.copy_(c)

    trace("patterns sampled")
    bcast(meta)
    nbytes = int(meta.item())
    d_blob = torch.zeros(nbytes + 16, dtype=torch.uint8, device=device)
    d_offs = torch.zeros(npat + 1, dtype=torch.int64, device=device)
    if rank == 0:
        if small:
            d_blob[:nbytes] = torch.from_numpy(pb).to(device)
            d_offs.copy_(torch.from_numpy(po.astype(np.int64)).to(device))
        else:
            d_blob[:nbytes] = b_[:nbytes]
            d_offs.copy_(o_)
            del b_, o_
    bcast(d_blob)
    bcast(d_offs)
    trace("patterns broadcast")

    g = capi.GpuStringIndex(device=local_rank)
    g.set_option("profile", 1)
    merger = shard.ShardMerger(capi, g, dist, rank, world, coll_device, device, mode=args.merge) if (world > 1 or args.force_merge) else None

    merged_rows = [None]   # row_ptr[-1] of the last step's merged CSR (N > 1)
    last_hits = [None]     # occurrence offsets of the last step's query (workloads with offsets)
    call_wall = []         # (build call, query call) wall ms per step, as the caller sees them

    def step():
        # the document table is resident like the text (cdb_build_resident): nothing but scalars crosses PCIe in a step
        trace("build")
        tw0 = time.perf_counter()
        g.build_resident(text.data_ptr(), d_doc_start.data_ptr(), d_ids.data_ptr(), ndocs)
        tw1 = time.perf_counter()
        trace(f"query (build {g.stat('build_ms'):.1f} ms, group_fallbacks {g.stat('group_fallbacks'):.0f})")
        tb = g.stat("build_ms")
        if cfg.get("offsets"):
            r, last_hits[0] = g.query_batch_offsets_device(d_blob.data_ptr(), d_offs.data_ptr(), npat, nbytes)
        else:
            r = g.query_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), npat, nbytes)
        tq = g.stat("query_ms")
        call_wall.append((round((tw1 - tw0) * 1e3, 3), round((time.perf_counter() - tw1) * 1e3, 3)))
        if merger is not None:
            trace("merge")
            m = merger.merge(r, npat)
            if merger.comm is not None:
                merged_rows[0] = int(m.nrows_total) if merger.mode == "counts" else int(m.nrows)
            else:
                merged_rows[0] = int(m[0][-1].item())
        trace("step done")
        return tb, tq, r

    torch.cuda.synchronize()  # inputs complete before the library's own stream touches them
    capi.memory_reset_peak()
    trace("inputs ready")
    selfcheck = None
    if merger is not None:
        # first contact with several GPUs is the driver's run: fail loudly and cheaply BEFORE the timed region
        selfcheck = mg_selfcheck(torch, dist, capi, g, merger, rank, world, local_rank, device, coll_device, args,
                                 lambda: g.build_resident(text.data_ptr(), d_doc_start.data_ptr(), d_ids.data_ptr(), ndocs),
                                 d_blob, d_offs, min(npat, 1000))
        if rank == 0:
            print(json.dumps({"mg_selfcheck": selfcheck}), file=sys.stderr, flush=True)
        if not selfcheck["ok"]:
            raise SystemExit(f"mg_selfcheck failed on rank {rank}: {selfcheck}")
    for _ in range(args.warmup):
        step()
    g.profile_reset()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    build_ms = query_ms = 0.0
    step_build_ms = []
    r = None
    del call_wall[:]
    for _ in range(args.steps):
        tb, tq, r = step()
        build_ms += tb
        query_ms += tq
        step_build_ms.append(round(tb, 3))
    # The order proof of a step's build runs BEHIND it, in the gaps between library calls, and is cancelled by the next step's build;
    # the last step's proof would go on into the closing synchronize (which waits for every stream: 1.9 s measured with a 16 GiB
    # UTF-8 column) — it is cancelled the same way, here.  Proofs are measured in the order_proof leg behind the timed region.
    g.set_option("proof_cancel", 1)
    t_sync = time.perf_counter()
    torch.cuda.synchronize()
    t_sync = (time.perf_counter() - t_sync) * 1e3
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed, build_ms, query_ms], dtype=torch.float64, device=coll_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, build_ms, query_ms = (float(x) for x in t.tolist())
    trace("timed region done")
    hits, rows = int(r.nhits), int(r.nrows)
    rows_per_rank = [rows]
    if world > 1:  # rows every rank contributed to the merged result of the last step
        mine = torch.tensor([rows], dtype=torch.int64, device=coll_device)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rows_per_rank = [int(x.item()) for x in allr]
    if args.dump_outputs and rank == 0:   # (before any other query on this handle: the device arrays live until the next one)
        dump_outputs(torch, args.dump_outputs, r, last_hits[0], device)

    prof = g.profile()
    steps = args.steps
    out = None
    if rank == 0:
        gib_total = world * n * steps / 2**30
        roof = dominant(prof, builds=steps)
        traffic = pmc_traffic(args.workload)
        attach_traffic(roof, traffic if (traffic and traffic.get("suffixes") in (None, n)) else None,
                       "committed PMC profile of this same command (not measured in this run)")
        build_kernels = {k: v for k, v in prof.items() if not k.startswith("q_")}
        kern_ms = sum(v["ms"] for v in build_kernels.values()) / steps
        kern_bytes = sum(v["bytes"] for v in build_kernels.values()) / steps
        out = {
            "metric": "sa_build_GiB_per_s",
            "value": round(gib_total / elapsed, 4),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1e3 / steps, 3),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "u64" if g.sa_width == 8 else "u32",  # suffix-array entries and sort keys of this configuration (text is u8)
            "data": "synthetic",
            "config": {
                "workload": f"{args.workload}: " + describe(cfg, n, ndocs) + " per GPU; step = SA build + batched query"
                            + (" + RCCL merge of the shards' match lists" if world > 1 else "")
                            + (f"; fixed corpus of {world * n / 2**30:.0f} GiB split into {world} doc-aligned shards" if args.scaling == "strong" else "")
                            + (f" ({clamp_note})" if clamp_note else ""),
                "docs_per_gpu": ndocs, "bytes_per_gpu": n, "patterns": npat,
            },
            "commit": git_head(),
            "merge": merger.note if merger is not None else None,
            "rccl_ranks": int(merger.comm.world) if (merger is not None and merger.comm is not None) else None,
            "rows_per_rank": rows_per_rank,
            "merged_rows": merged_rows[0],
            "mg_selfcheck": selfcheck,
            "sa_build_only_GiB_per_s": round(world * n * steps / 2**30 / (build_ms * 1e-3), 4),
            "query_patterns_per_s": round(world * npat * steps / (query_ms * 1e-3), 1),
            "query_hits_per_batch": hits,
            "query_rows_per_batch": rows,
            "build_ms_per_step": step_build_ms,
            "call_wall_ms_per_step": list(call_wall),       # (build call, query call) as the caller's clock sees them
            "closing_synchronize_ms": round(t_sync, 3),     # torch.cuda.synchronize() behind the last step (waits for every stream)
            "build_stats": build_stats(g),
            "roofline": roof,
            "build_kernels_ms_per_step": round(kern_ms, 3),
            "build_algorithmic_bytes_per_suffix": round(kern_bytes / n, 1),
            # every build kernel's algorithmic bytes over the WALL time of the builds (launch gaps and host work included)
            "build_frac_of_hbm_peak_over_wall_time": round(kern_bytes / (build_ms * 1e-3 / steps) / 1e9 / HBM_PEAK_GBS, 4),
            "kernel_time_share_of_wall": round(kern_ms / (build_ms / steps), 3),
            "peak_hbm_bytes": int(capi.memory_stats()[1] + n),
            "kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:14]},
        }
        if traffic and "kernels" in traffic and traffic.get("suffixes") in (None, n):
            tot = sum(k["hbm_bytes_per_launch"] * k.get("launches", 1) for k in traffic["kernels"].values()
                      if not str(k.get("phase", "")).startswith("q"))
            out["build_hbm_traffic_per_suffix_profiled"] = {"bytes": round(tot / traffic.get("suffixes", n), 1),
                                                            "profile": traffic.get("profile"), "commit": traffic.get("commit")}
        out["query_roofline"] = query_roofline(torch, r, npat, n, g.sa_width, query_ms * 1e-3 / steps, device, prof=prof, workload=args.workload,
                                               stored_entry_bytes=g.stat("sa_bytes_per_entry"))
    if merger is not None:
        merger.close()

    # ---- everything below is outside the timed region and runs with --full only; whatever fails there is reported, the headline stands
    c0 = None
    cpu_slice = None
    if args.full and rank == 0 and world == 1:
        try:
            if args.no_proof_leg:
                raise RuntimeError("skipped (--no-proof-leg)")
            # the order proof and what it costs the queries it runs beside: a fresh build, the batch at once (the proof of that build
            # is sweeping the array meanwhile), the proof awaited, the batch again
            def one_batch():
                t = time.perf_counter()
                if cfg.get("offsets"):
                    g.query_batch_offsets_device(d_blob.data_ptr(), d_offs.data_ptr(), npat, nbytes)
                else:
                    g.query_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), npat, nbytes)
                return (time.perf_counter() - t) * 1e3
            g.build_resident(text.data_ptr(), d_doc_start.data_ptr(), d_ids.data_ptr(), ndocs)
            q_during = one_batch()
            state_then = g.proof_wait(0)
            out["order_proof"] = proof_block(g)
            q_after = min(one_batch(), one_batch())
            out["order_proof"].update({"query_ms_while_proving": round(q_during, 3), "query_ms_after": round(q_after, 3),
                                       "proof_was_running_during_that_query": state_then == 1})
            out["order_proved"] = out["order_proof"]["order_proved"]
            out["proof_ms"] = out["order_proof"]["proof_ms"]
        except Exception as e:  # noqa: BLE001
            out["order_proof"] = {"error": repr(e)[:300]}
        out["verify"] = verify_block(g)
        if cfg.get("short"):
            try:
                out["short_patterns"] = short_tail(torch, W, g, text, d_doc_start, cfg, 0x7F)
            except Exception as e:  # noqa: BLE001
                out["short_patterns"] = {"error": repr(e)[:300]}
        if not args.no_cpu_baseline and cfg["kind"] != "utf8":
            # a doc-aligned slice of the headline corpus for the CPU leg at the end (documents of cfg["doclen"] bytes)
            take = min(n, CPU_SLICE_BYTES) // cfg["doclen"] * cfg["doclen"]
            cpu_slice = text[:take].cpu().numpy()
    extras = None
    if args.full and rank == 0 and world == 1 and small:   # the headline IS C1 (--workload c1): its extras run on the timed index
        extras = C1Extras(torch, capi, W, args)
        try:
            extras.before_close(g, text, doc_start, ids, d_blob, d_offs, nbytes, npat, n, out)
        except Exception as e:  # noqa: BLE001
            out["c1_extras_error"] = repr(e)[:300]
    g.close()
    if extras is not None:
        extras.after_close(out, ndocs, cfg.get("doclen", 1024))
    if args.full and rank == 0 and world == 1 and not small and not args.no_pcie and cfg["kind"] != "utf8":
        # SURVEY §8(d) defines t_build INCLUDING the H2D of the text: the same corpus from host memory through
        # cdb_build_view (the caller's buffer, chunked pinned staging inside the timed call) — beside `value`, never in it
        try:
            host_full = text.cpu().numpy()
            gv = capi.GpuStringIndex(device=local_rank)
            tv = []
            for _ in range(2):
                t = time.perf_counter()
                gv.build_view(ids, host_full, doc_start)
                tv.append(time.perf_counter() - t)
            out["sa_build_GiB_per_s_incl_h2d"] = round(n / 2**30 / min(tv), 3)
            out["pcie_inclusive"] = {"build_view_ms": [round(x * 1e3, 1) for x in tv], "build_device_part_ms": round(gv.stat("build_ms"), 2),
                                     "build_upload_ms": round(gv.stat("host_upload_ms"), 2), "verify": verify_block(gv),
                                     "note": "cdb_build_view over the whole host column (pageable numpy buffer), H2D inside the timed call"}
            gv.close()
            del host_full
        except Exception as e:  # noqa: BLE001
            out["pcie_inclusive"] = {"error": repr(e)[:300]}
    if cold is not None:
        out["cold_start"] = cold
    del text, d_blob, d_offs
    torch.cuda.empty_cache()
    capi.load_library().cdb_release_cached_memory()
    extra = args.configs if args.full else "none"
    if extra == "auto":
        extra = ("c1,c0,utf8_4g,c4shard" if world == 1 and args.workload == "c2" else
                 "c3" if world == 4 else "c4" if world == 8 else "none")  # C3 / C4 as BASELINE.json words them
    c1x = None
    if extra != "none":
        blocks = {}
        for name in [x for x in extra.split(",") if x]:
            try:
                mk = (lambda gi: shard.ShardMerger(capi, gi, dist, rank, world, coll_device, device, mode=args.merge)) if world > 1 else None

                def agree(ok):
                    t_ = torch.tensor([1 if ok else 0], dtype=torch.int32, device=coll_device)
                    dist.all_reduce(t_, op=dist.ReduceOp.MIN)
                    return bool(t_.item())

                ex = None
                if name == "c1" and rank == 0 and world == 1:
                    ex = c1x = C1Extras(torch, capi, W, args)
                res = run_config(torch, capi, W, name, rank, device, local_rank, make_merger=mk, agree=agree if world > 1 else None,
                                 merge_mode=args.merge, dist=dist if world > 1 else None, world=world, extras=ex, in_turn=in_turn)
            except Exception as e:  # noqa: BLE001
                res = {"workload": name, "error": repr(e)[:300]}
            if world > 1:  # per-GPU shapes of C3 / C4 on every rank: report the slowest rank's rate x N
                v = torch.tensor([res.get("sa_build_GiB_per_s", 0.0), res.get("query_patterns_per_s", 0.0)],
                                 dtype=torch.float64, device=coll_device)
                dist.all_reduce(v, op=dist.ReduceOp.MIN)
                res["all_ranks"] = {"sa_build_GiB_per_s_aggregate": round(float(v[0]) * world, 3),
                                    "query_patterns_per_s_slowest_rank": round(float(v[1]), 1), "n_gpus": world,
                                    "note": "independent per-shard builds (no data-path collective); every shard answers "
                                            "the whole pattern batch"}
            blocks[name] = res
        if rank == 0:
            out["configs"] = blocks
    # (RCCL announces its version through C stdio, flushed at exit: every rank pushes that out now, so that rank 0's JSON
    #  line is the last thing on the job's stdout)
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass
    sys.stdout.flush()
    if world > 1:
        dist.barrier()
    if rank == 0:
        out["cpu_baseline"] = None
        if args.full and world == 1 and not args.no_cpu_baseline and not args.no_midsize_check and args.configs == "auto":
            try:
                out["midsize_bit_exact"] = midsize_bit_exact(torch, capi, W)
                for k, v in out["midsize_bit_exact"].items():
                    if k.endswith("_bit_exact"):
                        out[k] = v
            except Exception as e:  # noqa: BLE001
                out["midsize_bit_exact"] = {"error": repr(e)[:300]}
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                c0 = c0_sweep(W)
                # the headline's CPU leg: a bounded slice of the SAME corpus (C2: the first 256 MiB of the 8 GiB, doc-aligned)
                if small:
                    extras.cpu_leg(out, W, c0, args, cfg.get("doclen", 1024), top=True)
                else:
                    out["cpu_baseline"] = cpu_baseline(W, cpu_slice, cfg.get("doclen", 1024), full_budget_s=0, c0=c0,
                                                       corpus=f"{args.workload} corpus", mmin=mmin, mmax=mmax,
                                                       whole_bytes=n if cpu_slice is not None and n > len(cpu_slice) else None)
            except Exception as e:  # noqa: BLE001
                out["cpu_baseline"] = {"error": repr(e)[:300]}
            if c1x is not None and isinstance(out.get("configs", {}).get("c1"), dict) and "error" not in out["configs"]["c1"]:
                # BASELINE config 1's "bit-exact SA check", literally: the oracle over the WHOLE C1 corpus against the array
                # the GPU built in the c1 block (and the whole-corpus CPU rate)
                try:
                    c1x.cpu_leg(out["configs"]["c1"], W, c0, args, 1024, top=False)
                    for k in ("sa_bit_exact", "rows_bit_exact"):
                        if k in out["configs"]["c1"]:
                            out["c1_" + k] = out["configs"]["c1"][k]
                except Exception as e:  # noqa: BLE001
                    out["configs"]["c1"]["cpu_baseline"] = {"error": repr(e)[:300]}
        emit(out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
