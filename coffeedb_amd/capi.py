"""ctypes binding of libcoffeedb_gpu.so (include/coffeedb_gpu.h).

`GpuStringIndex` mirrors the reference's string_index surface (add / build / query,
/root/reference/src/index.h:54-86) plus the batched query.  There is no CPU fallback: loading fails
loudly when the HIP library is missing, and cdb_create fails when no gfx950 device is present.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libcoffeedb_gpu.so")
if os.environ.get("CDB_LIB_PATH"):   # (timing experiments with ablated builds of the library: tools/experiments/abl/)
    LIB_PATH = os.environ["CDB_LIB_PATH"]
_LIB = None

EXPORTS = [
    "cdb_create", "cdb_destroy", "cdb_last_error", "cdb_add", "cdb_add_bulk", "cdb_build", "cdb_build_view", "cdb_build_views", "cdb_build_device", "cdb_build_resident", "cdb_raw_record_find_string", "cdb_add_raw_record", "cdb_add_raw_dir", "cdb_save", "cdb_load",
    "cdb_query", "cdb_query_or", "cdb_query_ranked", "cdb_query_and", "cdb_query_spans", "cdb_spans_free", "cdb_free", "cdb_query_batch", "cdb_query_batch_offsets", "cdb_hits_free", "cdb_result_free", "cdb_query_batch_device", "cdb_query_batch_offsets_device", "cdb_size", "cdb_bits",
    "cdb_mask", "cdb_sa_width", "cdb_sa_copy", "cdb_set_option", "cdb_get_stat", "cdb_profile_get",
    "cdb_profile_dump", "cdb_profile_reset", "cdb_release_cached_memory", "cdb_cached_memory_bytes", "cdb_set_cache_limit", "cdb_memory_stats", "cdb_memory_reset_peak",
    "cdb_debug_radix_sort", "cdb_debug_verify", "cdb_debug_verify_reference", "cdb_debug_self_check", "cdb_proof_wait", "cdb_layout_rule", "cdb_debug_query_latency",
    "cdb_shards_create", "cdb_shards_destroy", "cdb_shards_last_error", "cdb_shards_add", "cdb_shards_add_bulk", "cdb_shards_set_option",
    "cdb_shards_build", "cdb_shards_query", "cdb_shards_query_batch", "cdb_shards_query_or", "cdb_shards_query_ranked", "cdb_shards_query_spans", "cdb_shards_count", "cdb_shards_get", "cdb_shards_first_doc",
    "cdb_shards_transport", "cdb_shards_build_views", "cdb_shards_query_batch_offsets", "cdb_shards_query_and", "cdb_shards_add_raw_dir", "cdb_shards_save", "cdb_shards_load",
    "cdb_comm_unique_id", "cdb_comm_create", "cdb_comm_create_group", "cdb_comm_destroy", "cdb_comm_last_error", "cdb_comm_merge", "cdb_comm_merge_counts",
    "cdb_comm_world", "cdb_comm_transport", "cdb_reserve", "cdb_reserve_wait",
    "cdb_column_create", "cdb_column_destroy", "cdb_column_last_error", "cdb_column_add_bulk", "cdb_column_build", "cdb_column_query",
    "cdb_column_query_any", "cdb_query_and_columns", "cdb_column_get_stat", "cdb_debug_column_set_option", "cdb_debug_column_profile_dump",
    "cdb_column_cluster", "cdb_cluster", "cdb_clusters_free",
    "cdb_render_rows", "cdb_shards_render_rows", "cdb_rendered_free",
    "cdb_remove", "cdb_column_remove", "cdb_column_append", "cdb_debug_column_arrays",
    "cdb_append", "cdb_debug_verify_keys",
    "cdb_shards_remove", "cdb_shards_append", "cdb_shards_cluster",
    "cdb_debug_sort_ws_create", "cdb_debug_sort_ws_destroy", "cdb_debug_radix_sort_ex", "cdb_debug_radix_sort_split",
    "cdb_filter", "cdb_rowset_free", "cdb_rowset_last_error", "cdb_rowset_size", "cdb_rowset_rows", "cdb_rowset_page", "cdb_rowset_cluster",
    "cdb_rowset_cluster_column", "cdb_rowset_get_stat", "cdb_debug_rowset_from_rows", "cdb_debug_rowset_set_option",
    "cdb_debug_rowset_profile_dump",
    "cdb_column_values", "cdb_rowset_select", "cdb_selected_free",
    "cdb_rowset_remove", "cdb_rowset_all",
    "cdb_insert_objects", "cdb_insert_get_stat",
    "cdb_debug_scan", "cdb_debug_scan_partials", "cdb_debug_stable_ranks",
    "cdb_debug_sweep_records", "cdb_debug_vl_tables",
    "cdb_debug_carried_inplace", "cdb_debug_segsort",
]


class CdbResult(C.Structure):
    _fields_ = [("npat", C.c_uint64), ("nrows", C.c_uint64), ("nhits", C.c_uint64),
                ("row_ptr", C.POINTER(C.c_uint64)), ("ids", C.POINTER(C.c_int64)), ("counts", C.POINTER(C.c_int64))]


class CdbSpans(C.Structure):
    _fields_ = [("ndocs", C.c_uint64), ("nspans", C.c_uint64), ("ids", C.POINTER(C.c_int64)),
                ("span_ptr", C.POINTER(C.c_uint64)), ("begin", C.POINTER(C.c_uint64)), ("end", C.POINTER(C.c_uint64))]


class CdbHits(C.Structure):
    _fields_ = [("hit_ptr", C.POINTER(C.c_uint64)), ("offsets", C.POINTER(C.c_uint64))]


class CdbDeviceResult(C.Structure):
    _fields_ = [("npat", C.c_uint64), ("nrows", C.c_uint64), ("nhits", C.c_uint64),
                ("d_row_ptr", C.c_void_p), ("d_ids", C.c_void_p), ("d_counts", C.c_void_p)]


class CdbShardSlice(C.Structure):
    _fields_ = [("npat", C.c_uint64), ("nrows_total", C.c_uint64), ("nrows_local", C.c_uint64),
                ("d_row_ptr", C.c_void_p), ("d_row_base", C.c_void_p)]


class CdbKeyQuery(C.Structure):
    _fields_ = [("index", C.c_void_p), ("blob", C.c_void_p), ("offsets", C.c_void_p), ("nkw", C.c_uint64),
                ("ids", C.c_void_p), ("counts", C.c_void_p), ("nrows", C.c_size_t)]


class CdbColumnKey(C.Structure):
    _fields_ = [("column", C.c_void_p), ("blob", C.c_void_p), ("offsets", C.c_void_p), ("nranges", C.c_uint64)]


class CdbClusters(C.Structure):
    _fields_ = [("ngroups", C.c_uint64), ("missing", C.c_uint64), ("counts", C.POINTER(C.c_int64)), ("rep_ids", C.POINTER(C.c_int64)),
                ("values", C.POINTER(C.c_uint64)), ("value_ptr", C.POINTER(C.c_uint64)), ("value_blob", C.POINTER(C.c_char))]


class CdbRendered(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("missing", C.c_uint64), ("nspans", C.c_uint64), ("text_bytes", C.c_uint64),
                ("found", C.POINTER(C.c_uint8)), ("text_ptr", C.POINTER(C.c_uint64)), ("text_blob", C.POINTER(C.c_char)),
                ("span_ptr", C.POINTER(C.c_uint64)), ("begin", C.POINTER(C.c_uint64)), ("end", C.POINTER(C.c_uint64))]


RENDER_TEXT, RENDER_SPANS = 1, 2


class CdbSelectField(C.Structure):
    _fields_ = [("index", C.c_void_p), ("shards", C.c_void_p), ("column", C.c_void_p),
                ("kw_blob", C.c_void_p), ("kw_offsets", C.c_void_p), ("nkw", C.c_uint64)]


class CdbSelectedField(C.Structure):
    _fields_ = [("kind", C.c_int), ("missing", C.c_uint64), ("found", C.POINTER(C.c_uint8)), ("values", C.POINTER(C.c_uint64)),
                ("text_ptr", C.POINTER(C.c_uint64)), ("text_blob", C.POINTER(C.c_char))]


class CdbSelected(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("nfields", C.c_int), ("ids", C.POINTER(C.c_int64)), ("counts", C.POINTER(C.c_int64)),
                ("fields", C.POINTER(CdbSelectedField))]


class CdbRemoveField(C.Structure):
    _fields_ = [("index", C.c_void_p), ("column", C.c_void_p), ("removed", C.c_uint64), ("missing", C.c_uint64),
                ("status", C.c_int32), ("committed", C.c_int32)]


class CdbInsertField(C.Structure):
    _fields_ = [("index", C.c_void_p), ("column", C.c_void_p), ("rows", C.c_void_p), ("nrows", C.c_uint64), ("blob", C.c_void_p),
                ("doc_start", C.c_void_p), ("values", C.c_void_p), ("appended", C.c_uint64), ("status", C.c_int32),
                ("committed", C.c_int32)]


SELECT_STRING = 3   # cdb_selected_field.kind of a string field (the reference's tag)


class CdbDeviceHits(C.Structure):
    _fields_ = [("d_hit_ptr", C.c_void_p), ("d_offsets", C.c_void_p)]


def build_library(force=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    try:
        # PyTorch wheels bundle their own libamdhip64; two HIP runtimes in one process do not see each
        # other's devices.  Loading torch first makes this library bind to the runtime torch uses
        # (tests and bench.py share device pointers with torch).  C/C++ hosts simply use /opt/rocm's.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing — build it with `make -C {CSRC}` (there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    vp, u64, i64, cp = C.c_void_p, C.c_uint64, C.c_int64, C.c_char_p
    lib.cdb_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.cdb_destroy.argtypes = [vp]
    lib.cdb_destroy.restype = None
    lib.cdb_last_error.argtypes = [vp]
    lib.cdb_last_error.restype = cp
    lib.cdb_add.argtypes = [vp, i64, cp, C.c_size_t]
    lib.cdb_add_bulk.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_raw_record_find_string.argtypes = [vp, C.c_size_t, cp, C.POINTER(i64), C.POINTER(cp), C.POINTER(C.c_size_t)]
    lib.cdb_add_raw_record.argtypes = [vp, cp, vp, C.c_size_t]
    lib.cdb_add_raw_dir.argtypes = [vp, cp, cp, C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_save.argtypes = [vp, cp]
    lib.cdb_load.argtypes = [vp, cp]
    lib.cdb_build.argtypes = [vp]
    lib.cdb_build_device.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_build_resident.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_query.argtypes = [vp, cp, C.c_size_t, C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)),
                              C.POINTER(C.c_size_t)]
    lib.cdb_query_ranked.argtypes = [vp, vp, vp, u64, i64, i64, u64, C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)),
                                     C.POINTER(C.c_size_t)]
    lib.cdb_query_or.argtypes = [vp, vp, vp, u64, C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)),
                                 C.POINTER(C.c_size_t)]
    lib.cdb_query_and.argtypes = [C.POINTER(CdbKeyQuery), C.c_int, C.c_int, i64, i64, u64, C.POINTER(C.POINTER(i64)),
                                  C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_query_spans.argtypes = [vp, vp, vp, u64, C.POINTER(CdbSpans)]
    lib.cdb_spans_free.argtypes = [C.POINTER(CdbSpans)]
    lib.cdb_spans_free.restype = None
    lib.cdb_free.argtypes = [vp]
    lib.cdb_free.restype = None
    lib.cdb_query_batch.argtypes = [vp, vp, vp, u64, C.POINTER(CdbResult)]
    lib.cdb_query_batch_offsets.argtypes = [vp, vp, vp, u64, C.POINTER(CdbResult), C.POINTER(CdbHits)]
    lib.cdb_hits_free.argtypes = [C.POINTER(CdbHits)]
    lib.cdb_hits_free.restype = None
    lib.cdb_result_free.argtypes = [C.POINTER(CdbResult)]
    lib.cdb_result_free.restype = None
    lib.cdb_query_batch_device.argtypes = [vp, vp, vp, u64, u64, C.POINTER(CdbDeviceResult)]
    lib.cdb_query_batch_offsets_device.argtypes = [vp, vp, vp, u64, u64, C.POINTER(CdbDeviceResult), C.POINTER(CdbDeviceHits)]
    for f in ("cdb_size", "cdb_bits", "cdb_mask"):
        getattr(lib, f).argtypes = [vp]
        getattr(lib, f).restype = u64
    lib.cdb_sa_width.argtypes = [vp]
    lib.cdb_sa_copy.argtypes = [vp, vp, u64]
    lib.cdb_set_option.argtypes = [vp, cp, i64]
    lib.cdb_get_stat.argtypes = [vp, cp, C.POINTER(C.c_double)]
    lib.cdb_profile_get.argtypes = [vp, cp, C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_profile_dump.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.cdb_profile_reset.argtypes = [vp]
    lib.cdb_profile_reset.restype = None
    lib.cdb_release_cached_memory.argtypes = []
    lib.cdb_release_cached_memory.restype = None
    lib.cdb_set_cache_limit.argtypes = [u64]
    lib.cdb_set_cache_limit.restype = None
    lib.cdb_memory_stats.argtypes = [C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_memory_stats.restype = None
    lib.cdb_memory_reset_peak.argtypes = []
    lib.cdb_memory_reset_peak.restype = None
    lib.cdb_cached_memory_bytes.argtypes = []
    lib.cdb_cached_memory_bytes.restype = u64
    lib.cdb_debug_verify.argtypes = [vp, C.POINTER(u64)]
    lib.cdb_debug_verify_reference.argtypes = [vp, C.POINTER(u64)]
    lib.cdb_debug_self_check.argtypes = [vp, C.c_int, C.POINTER(u64)]
    lib.cdb_proof_wait.argtypes = [vp, C.c_double]
    lib.cdb_proof_wait.restype = C.c_int
    lib.cdb_debug_radix_sort.argtypes = [C.c_int, vp, vp, u64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                         C.POINTER(C.c_int)]
    lib.cdb_shards_create.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
    lib.cdb_shards_destroy.argtypes = [vp]
    lib.cdb_shards_destroy.restype = None
    lib.cdb_shards_last_error.argtypes = [vp]
    lib.cdb_shards_last_error.restype = cp
    lib.cdb_shards_add.argtypes = [vp, i64, cp, C.c_size_t]
    lib.cdb_shards_add_bulk.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_shards_set_option.argtypes = [vp, cp, i64]
    lib.cdb_shards_build.argtypes = [vp]
    lib.cdb_shards_query.argtypes = [vp, cp, C.c_size_t, C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_shards_query_batch.argtypes = [vp, vp, vp, u64, C.POINTER(CdbResult)]
    lib.cdb_shards_query_or.argtypes = [vp, vp, vp, u64, C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_shards_query_ranked.argtypes = [vp, vp, vp, u64, i64, i64, u64, C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)),
                                            C.POINTER(C.c_size_t)]
    lib.cdb_shards_query_spans.argtypes = [vp, vp, vp, u64, C.POINTER(CdbSpans)]
    lib.cdb_shards_count.argtypes = [vp]
    lib.cdb_shards_get.argtypes = [vp, C.c_int]
    lib.cdb_shards_get.restype = vp
    lib.cdb_shards_first_doc.argtypes = [vp, C.c_int]
    lib.cdb_shards_first_doc.restype = u64
    lib.cdb_shards_transport.argtypes = [vp]
    lib.cdb_shards_transport.restype = cp
    lib.cdb_comm_unique_id.argtypes = [vp]
    lib.cdb_comm_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int]
    lib.cdb_reserve.argtypes = [C.c_int, u64, u64, C.c_char_p, C.c_size_t]
    lib.cdb_reserve_wait.restype = None
    lib.cdb_comm_create_group.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
    lib.cdb_comm_destroy.argtypes = [vp]
    lib.cdb_comm_destroy.restype = None
    lib.cdb_comm_last_error.argtypes = [vp]
    lib.cdb_comm_last_error.restype = cp
    lib.cdb_comm_merge.argtypes = [vp, C.POINTER(CdbDeviceResult), C.POINTER(CdbDeviceResult)]
    lib.cdb_comm_merge_counts.argtypes = [vp, C.POINTER(CdbDeviceResult), C.POINTER(CdbShardSlice)]
    lib.cdb_comm_world.argtypes = [vp]
    lib.cdb_comm_transport.argtypes = [vp]
    lib.cdb_comm_transport.restype = cp
    lib.cdb_build_view.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_build_views.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_shards_build_views.argtypes = [vp, vp, vp, vp, u64]
    lib.cdb_shards_query_batch_offsets.argtypes = [vp, vp, vp, u64, C.POINTER(CdbResult), C.POINTER(CdbHits)]
    lib.cdb_shards_query_and.argtypes = [C.POINTER(CdbKeyQuery), C.c_int, C.c_int, i64, i64, u64, C.POINTER(C.POINTER(i64)),
                                         C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_shards_add_raw_dir.argtypes = [vp, cp, cp, C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_shards_save.argtypes = [vp, cp]
    lib.cdb_shards_load.argtypes = [vp, cp]
    lib.cdb_column_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.cdb_column_destroy.argtypes = [vp]
    lib.cdb_column_destroy.restype = None
    lib.cdb_column_last_error.argtypes = [vp]
    lib.cdb_column_last_error.restype = cp
    lib.cdb_column_add_bulk.argtypes = [vp, vp, vp, u64]
    lib.cdb_column_build.argtypes = [vp]
    lib.cdb_column_query.argtypes = [vp, cp, C.c_size_t, C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_column_query_any.argtypes = [vp, vp, vp, u64, C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_query_and_columns.argtypes = [C.POINTER(CdbKeyQuery), C.c_int, C.POINTER(CdbColumnKey), C.c_int, C.c_int, i64, i64, u64,
                                          C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_column_get_stat.argtypes = [vp, cp, C.POINTER(C.c_double)]
    lib.cdb_debug_column_set_option.argtypes = [vp, cp, i64]
    lib.cdb_debug_column_profile_dump.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.cdb_column_cluster.argtypes = [vp, vp, u64, C.POINTER(CdbClusters)]
    lib.cdb_cluster.argtypes = [vp, vp, u64, C.c_int, C.POINTER(CdbClusters)]
    lib.cdb_clusters_free.argtypes = [C.POINTER(CdbClusters)]
    lib.cdb_clusters_free.restype = None
    render_args = [vp, vp, u64, vp, vp, u64, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.POINTER(CdbRendered)]
    lib.cdb_render_rows.argtypes = render_args
    lib.cdb_shards_render_rows.argtypes = render_args
    lib.cdb_rendered_free.argtypes = [C.POINTER(CdbRendered)]
    lib.cdb_rendered_free.restype = None
    lib.cdb_remove.argtypes = [vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_column_remove.argtypes = [vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_column_append.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    lib.cdb_debug_column_arrays.argtypes = [vp, vp, vp, vp, vp]
    lib.cdb_append.argtypes = [vp, vp, vp, vp, u64, C.POINTER(u64)]
    lib.cdb_debug_verify_keys.argtypes = [vp, C.POINTER(u64)]
    lib.cdb_shards_remove.argtypes = lib.cdb_remove.argtypes
    lib.cdb_shards_append.argtypes = lib.cdb_append.argtypes
    lib.cdb_shards_cluster.argtypes = lib.cdb_cluster.argtypes
    rows_out = [C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(i64)), C.POINTER(C.c_size_t)]
    lib.cdb_filter.argtypes = [C.POINTER(CdbKeyQuery), C.c_int, C.POINTER(CdbColumnKey), C.c_int, C.c_int, i64, i64, C.POINTER(vp)]
    lib.cdb_rowset_free.argtypes = [vp]
    lib.cdb_rowset_free.restype = None
    lib.cdb_rowset_last_error.argtypes = [vp]
    lib.cdb_rowset_last_error.restype = cp
    lib.cdb_rowset_size.argtypes = [vp]
    lib.cdb_rowset_size.restype = u64
    lib.cdb_rowset_rows.argtypes = [vp] + rows_out
    lib.cdb_rowset_page.argtypes = [vp, u64, u64] + rows_out
    lib.cdb_rowset_cluster.argtypes = [vp, vp, C.c_int, C.POINTER(CdbClusters)]
    lib.cdb_rowset_cluster_column.argtypes = [vp, vp, C.POINTER(CdbClusters)]
    lib.cdb_rowset_get_stat.argtypes = [vp, cp, C.POINTER(C.c_double)]
    lib.cdb_debug_rowset_from_rows.argtypes = [C.c_int, vp, vp, u64, C.POINTER(vp)]
    lib.cdb_debug_rowset_set_option.argtypes = [vp, cp, i64]
    lib.cdb_debug_rowset_profile_dump.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.cdb_column_values.argtypes = [vp, vp, u64, vp, vp, C.POINTER(u64)]
    lib.cdb_rowset_remove.argtypes = [vp, C.POINTER(CdbRemoveField), C.c_int, C.POINTER(u64)]
    lib.cdb_rowset_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.POINTER(vp)]
    lib.cdb_insert_objects.argtypes = [vp, u64, C.POINTER(CdbInsertField), C.c_int, C.POINTER(u64)]
    lib.cdb_insert_get_stat.argtypes = [vp, vp, cp, C.POINTER(C.c_double)]
    lib.cdb_rowset_select.argtypes = [vp, u64, u64, C.POINTER(CdbSelectField), C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(CdbSelected)]
    lib.cdb_selected_free.argtypes = [C.POINTER(CdbSelected)]
    lib.cdb_selected_free.restype = None
    _LIB = lib
    return lib


def _array(ptr, n, dtype):
    """copy of a C result array of n elements"""
    n = int(n)
    if n == 0:
        return np.empty(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).copy()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _render_rows(self, fn, ids, keywords, left, right, text, spans, raw):
    """cdb_render_rows / cdb_shards_render_rows behind GpuStringIndex.render_rows and GpuShards.render_rows"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
    offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in keywords], out=offs[1:])
    left, right = bytes(left), bytes(right)
    r = CdbRendered()
    self._check(fn(self._h, _ptr(ids) if len(ids) else None, len(ids), _ptr(blob) if len(blob) else None, _ptr(offs), len(keywords),
                   left if left else None, len(left), right if right else None, len(right),
                   (RENDER_TEXT if text else 0) | (RENDER_SPANS if spans else 0), C.byref(r)))
    try:
        n = int(r.nrows)
        found = _array(r.found, n, np.uint8).astype(bool)
        tp = tb = sp = sb = se = None
        if r.text_ptr:
            tp = _array(r.text_ptr, n + 1, np.uint64)
            tb = C.string_at(r.text_blob, int(r.text_bytes))
        if r.span_ptr:
            sp = _array(r.span_ptr, n + 1, np.uint64)
            sb = _array(r.begin, int(r.nspans), np.uint64)
            se = _array(r.end, int(r.nspans), np.uint64)
        if raw:
            return {"found": found, "missing": int(r.missing), "nspans": int(r.nspans), "text_bytes": int(r.text_bytes), "text_ptr": tp,
                    "text_blob": tb, "span_ptr": sp, "begin": sb, "end": se}
        texts = None if tp is None else [tb[int(tp[i]):int(tp[i + 1])] for i in range(n)]
        spans_ = None if sp is None else [[(int(sb[k]), int(se[k])) for k in range(int(sp[i]), int(sp[i + 1]))] for i in range(n)]
        return found, texts, spans_, int(r.missing)
    finally:
        self._lib.cdb_rendered_free(C.byref(r))


def _cluster_strings(self, fn, ids, with_values):
    """cdb_cluster / cdb_shards_cluster behind GpuStringIndex.cluster and GpuShards.cluster"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    r = CdbClusters()
    self._check(fn(self._h, _ptr(ids) if len(ids) else None, len(ids), 1 if with_values else 0, C.byref(r)))
    try:
        ng = int(r.ngroups)
        values = None
        if with_values:
            vp_ = _array(r.value_ptr, ng + 1, np.uint64)
            blob = C.string_at(r.value_blob, int(vp_[ng])) if ng else b""
            values = [blob[int(vp_[g]):int(vp_[g + 1])] for g in range(ng)]
        return values, _array(r.counts, ng, np.int64), _array(r.rep_ids, ng, np.int64), int(r.missing)
    finally:
        self._lib.cdb_clusters_free(C.byref(r))


def _remove_ids(self, fn, ids):
    """cdb_remove / cdb_shards_remove behind GpuStringIndex.remove and GpuShards.remove"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    removed, missing = C.c_uint64(0), C.c_uint64(0)
    self._check(fn(self._h, _ptr(ids) if len(ids) else None, len(ids), C.byref(removed), C.byref(missing)))
    return int(removed.value), int(missing.value)


def _append_docs(self, fn, ids, blob, doc_start):
    """cdb_append / cdb_shards_append behind GpuStringIndex.append and GpuShards.append"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
    assert len(doc_start) == len(ids) + 1
    if len(doc_start) and int(doc_start[-1]) > len(blob):   # (the C ABI takes plain pointers: a short blob would be read past its end)
        raise ValueError(f"blob holds {len(blob)} bytes, doc_start[-1] = {int(doc_start[-1])}")
    if not len(blob):
        blob = np.zeros(1, dtype=np.uint8)   # (empty documents only: the C ABI still wants a pointer)
    appended = C.c_uint64(0)
    self._check(fn(self._h, _ptr(ids) if len(ids) else None, _ptr(blob), _ptr(doc_start), len(ids), C.byref(appended)))
    return int(appended.value)


class GpuStringIndex:
    """string_index on the GPU: add() / build() / query() as in the reference, plus query_batch()."""

    def __init__(self, device=-1):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.cdb_create(C.byref(h), device)
        if rc != 0:
            raise RuntimeError(f"cdb_create failed (code {rc}): no usable gfx950 device — there is no CPU fallback")
        self._h = h
        # measurement plumbing of THIS binding (tools/, bench.py A/B runs): CDB_OPTIONS="name=value,..." is applied through
        # cdb_set_option; the library itself reads no option from the environment
        for kv in filter(None, os.environ.get("CDB_OPTIONS", "").split(",")):
            name, _, val = kv.partition("=")
            self._lib.cdb_set_option(self._h, name.strip().encode(), int(val))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cdb_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.cdb_last_error(self._h).decode(errors="replace"))

    # ---- reference surface
    def add(self, id_, value: bytes):
        self._check(self._lib.cdb_add(self._h, int(id_), value, len(value)))

    def add_bulk(self, ids, blob, doc_start):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
        assert len(doc_start) == len(ids) + 1
        if len(doc_start) and int(doc_start[-1]) > len(blob):   # (the C ABI takes plain pointers: a short blob would be read past its end)
            raise ValueError(f"blob holds {len(blob)} bytes, doc_start[-1] = {int(doc_start[-1])}")
        self._check(self._lib.cdb_add_bulk(self._h, _ptr(ids), _ptr(blob), _ptr(doc_start), len(ids)))

    def build(self):
        self._check(self._lib.cdb_build(self._h))

    def build_view(self, ids, blob, doc_start):
        """cdb_build_view: build straight from the caller's host column (no staging copy inside the handle)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
        assert len(doc_start) == len(ids) + 1
        if len(doc_start) and int(doc_start[-1]) > len(blob):   # (the C ABI takes plain pointers: a short blob would be read past its end)
            raise ValueError(f"blob holds {len(blob)} bytes, doc_start[-1] = {int(doc_start[-1])}")
        self._check(self._lib.cdb_build_view(self._h, _ptr(ids), _ptr(blob) if len(blob) else None, _ptr(doc_start), len(ids)))

    def build_views(self, ids, docs):
        """cdb_build_views: documents as separate bytes objects (string_index's views), gathered by the library."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        ptrs = (C.c_char_p * len(docs))(*docs)
        lens = np.array([len(d) for d in docs], dtype=np.uint64)
        self._check(self._lib.cdb_build_views(self._h, _ptr(ids), C.cast(ptrs, C.c_void_p), _ptr(lens), len(docs)))

    def add_raw_record(self, key: bytes, record: bytes):
        self._check(self._lib.cdb_add_raw_record(self._h, key, record, len(record)))

    def add_raw_dir(self, directory, key: bytes):
        """Every record file of `directory` (ascending name order); returns (records parsed, documents added)."""
        nrec, nadd = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.cdb_add_raw_dir(self._h, os.fsencode(directory), key, C.byref(nrec), C.byref(nadd)))
        return nrec.value, nadd.value

    def save(self, path):
        self._check(self._lib.cdb_save(self._h, os.fsencode(path)))

    def load(self, path):
        self._check(self._lib.cdb_load(self._h, os.fsencode(path)))

    def build_device(self, d_text_ptr, doc_start, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
        self._check(self._lib.cdb_build_device(self._h, C.c_void_p(d_text_ptr), _ptr(doc_start), _ptr(ids), len(ids)))

    def build_resident(self, d_text_ptr, d_doc_start_ptr, d_ids_ptr, ndocs):
        """Build over text AND document tables that already live in device memory (u64[ndocs+1], i64[ndocs])."""
        self._check(self._lib.cdb_build_resident(self._h, C.c_void_p(d_text_ptr), C.c_void_p(d_doc_start_ptr),
                                                 C.c_void_p(d_ids_ptr), int(ndocs)))

    def query(self, kw: bytes):
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_query(self._h, kw, len(kw), C.byref(ids), C.byref(cnt), C.byref(n)))
        out = [(ids[i], cnt[i]) for i in range(n.value)]
        self._lib.cdb_free(ids)
        self._lib.cdb_free(cnt)
        return out

    def query_or(self, keywords):
        """Union over `keywords` by object id with summed counts, ascending id (interface.cpp:78-113)."""
        blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
        offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
        np.cumsum([len(k) for k in keywords], out=offs[1:])
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_query_or(self._h, _ptr(blob) if len(blob) else None, _ptr(offs), len(keywords),
                                           C.byref(ids), C.byref(cnt), C.byref(n)))
        out = [(ids[i], cnt[i]) for i in range(n.value)]
        self._lib.cdb_free(ids)
        self._lib.cdb_free(cnt)
        return out

    def query_ranked(self, keywords, lo=1, hi=(1 << 62), limit=0):
        """query_or, filtered to lo <= count < hi, ranked by descending count (ties: ascending id), first `limit` rows."""
        blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
        offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
        np.cumsum([len(k) for k in keywords], out=offs[1:])
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_query_ranked(self._h, _ptr(blob) if len(blob) else None, _ptr(offs), len(keywords),
                                               int(lo), int(hi), int(limit), C.byref(ids), C.byref(cnt), C.byref(n)))
        out = [(ids[i], cnt[i]) for i in range(n.value)]
        self._lib.cdb_free(ids)
        self._lib.cdb_free(cnt)
        return out

    def query_ranked_arrays(self, blob, offsets, lo=1, hi=(1 << 62), limit=0, rows=False):
        """cdb_query_ranked over an already packed keyword list (bench: 10^5 keywords); returns the number of rows
        (rows=True: the (ids, counts) arrays)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_query_ranked(self._h, _ptr(blob), _ptr(offsets), len(offsets) - 1, int(lo), int(hi), int(limit),
                                               C.byref(ids), C.byref(cnt), C.byref(n)))
        out = int(n.value)
        if rows:
            out = (np.array(ids[:n.value], dtype=np.int64), np.array(cnt[:n.value], dtype=np.int64))
        self._lib.cdb_free(ids)
        self._lib.cdb_free(cnt)
        return out

    def query_spans(self, keywords):
        """{object id: [(begin, end_inclusive), ...]} — merged highlight spans (database.cpp:58-76)."""
        blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
        offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
        np.cumsum([len(k) for k in keywords], out=offs[1:])
        r = CdbSpans()
        self._check(self._lib.cdb_query_spans(self._h, _ptr(blob) if len(blob) else None, _ptr(offs), len(keywords),
                                              C.byref(r)))
        try:
            out = []
            for d in range(r.ndocs):
                a, b = r.span_ptr[d], r.span_ptr[d + 1]
                out.append((r.ids[d], [(r.begin[k], r.end[k]) for k in range(a, b)]))
            return out
        finally:
            self._lib.cdb_spans_free(C.byref(r))

    # ---- batched
    @staticmethod
    def _adopt(ptr, n, dtype, owner):
        """numpy view of a C result array of n elements; large arrays are adopted without a copy (the view
        keeps `owner` alive, whose finaliser hands the pinned blocks back to the library)."""
        n = int(n)
        if n == 0:
            return np.empty(0, dtype=dtype)
        nbytes = n * np.dtype(dtype).itemsize
        buf = (C.c_uint8 * nbytes).from_address(C.addressof(ptr.contents))
        if nbytes < (1 << 20):
            return np.frombuffer(buf, dtype=dtype).copy()
        buf._owner = owner
        return np.frombuffer(buf, dtype=dtype)

    class _Owner:
        def __init__(self, lib, *frees):
            self._frees = [(getattr(lib, fn), C.byref(obj), obj) for fn, obj in frees]

        def __del__(self):
            for fn, ref, _obj in self._frees:
                fn(ref)

    def query_batch(self, blob, offsets):
        """Returns (row_ptr uint64[npat+1], ids int64[nrows], counts int64[nrows], nhits)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        npat = len(offsets) - 1
        r = CdbResult()
        self._check(self._lib.cdb_query_batch(self._h, _ptr(blob), _ptr(offsets), npat, C.byref(r)))
        own = self._Owner(self._lib, ("cdb_result_free", r))
        nrows = int(r.nrows)
        return (self._adopt(r.row_ptr, npat + 1, np.uint64, own), self._adopt(r.ids, nrows, np.int64, own),
                self._adopt(r.counts, nrows, np.int64, own), int(r.nhits))

    def query_batch_offsets(self, blob, offsets):
        """query_batch plus (hit_ptr uint64[nrows+1], occurrence offsets uint64[nhits])."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        npat = len(offsets) - 1
        r, hx = CdbResult(), CdbHits()
        self._check(self._lib.cdb_query_batch_offsets(self._h, _ptr(blob), _ptr(offsets), npat, C.byref(r), C.byref(hx)))
        own = self._Owner(self._lib, ("cdb_result_free", r), ("cdb_hits_free", hx))
        nrows, nhits = int(r.nrows), int(r.nhits)
        return (self._adopt(r.row_ptr, npat + 1, np.uint64, own), self._adopt(r.ids, nrows, np.int64, own),
                self._adopt(r.counts, nrows, np.int64, own), self._adopt(hx.hit_ptr, nrows + 1, np.uint64, own),
                self._adopt(hx.offsets, nhits, np.uint64, own))

    def query_batch_device(self, d_blob_ptr, d_offsets_ptr, npat, blob_bytes):
        r = CdbDeviceResult()
        self._check(self._lib.cdb_query_batch_device(self._h, C.c_void_p(d_blob_ptr), C.c_void_p(d_offsets_ptr), npat,
                                                     blob_bytes, C.byref(r)))
        return r

    def query_batch_offsets_device(self, d_blob_ptr, d_offsets_ptr, npat, blob_bytes):
        r, hx = CdbDeviceResult(), CdbDeviceHits()
        self._check(self._lib.cdb_query_batch_offsets_device(self._h, C.c_void_p(d_blob_ptr), C.c_void_p(d_offsets_ptr), npat,
                                                             blob_bytes, C.byref(r), C.byref(hx)))
        return r, hx

    # ---- introspection / options / measurements
    size = property(lambda s: s._lib.cdb_size(s._h))
    bits = property(lambda s: s._lib.cdb_bits(s._h))
    mask = property(lambda s: s._lib.cdb_mask(s._h))
    sa_width = property(lambda s: s._lib.cdb_sa_width(s._h))

    def sa(self):
        n, w = self.size, self.sa_width
        out = np.empty(n, dtype=np.uint32 if w == 4 else np.uint64)
        if n:
            self._check(self._lib.cdb_sa_copy(self._h, _ptr(out), out.nbytes))
        return out

    def verify(self):
        """GPU-side structural check of the suffix array (see cdb_debug_verify)."""
        out = (C.c_uint64 * 5)()
        self._check(self._lib.cdb_debug_verify(self._h, out))
        return {"inversions": out[0], "tie_violations": out[1], "entry_sum": out[2], "invalid_entries": out[3],
                "expected_entry_sum": out[4]}

    def verify_reference(self):
        """GPU-side check of the REFERENCE's order (signed child order inside radix nodes; cdb_debug_verify_reference)."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.cdb_debug_verify_reference(self._h, out))
        return {"violations": out[0], "mixed_pairs": out[1], "radix_node_pairs": out[2], "tie_violations": out[3]}

    def proof_wait(self, timeout_ms=-1.0):
        """State of the order proof behind the last build / load (cdb_proof_wait): 2 proved, 3 damage found and repaired, ..."""
        return int(self._lib.cdb_proof_wait(self._h, float(timeout_ms)))

    def self_check(self, full=False):
        """(pairs out of order, invalid entries) among 2^15 random adjacent pairs, or among all of them (cdb_debug_self_check)."""
        out = (C.c_uint64 * 2)()
        self._check(self._lib.cdb_debug_self_check(self._h, 1 if full else 0, out))
        return int(out[0]), int(out[1])

    def query_latency_us(self, keywords, reps=32):
        """median microseconds per cdb_query call of every keyword, measured inside the library (no binding overhead)"""
        blob = b"".join(keywords)
        offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(k) for k in keywords])
        out = np.zeros(len(keywords), dtype=np.float64)
        self._lib.cdb_debug_query_latency.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self._check(self._lib.cdb_debug_query_latency(self._h, blob, _ptr(offs), len(keywords), reps, _ptr(out)))
        return out

    def cluster(self, ids, with_values=True):
        """cdb_cluster (database.cpp:442-460 for this string field): the rows `ids` grouped by their document, groups in
        std::string order.  Returns (values: list of bytes, or None without with_values; counts int64; rep_ids int64: the smallest
        id of each group among the rows; missing: rows whose id the index does not hold)."""
        return _cluster_strings(self, self._lib.cdb_cluster, ids, with_values)

    def render_rows(self, ids, keywords, left=b"", right=b"", text=True, spans=True, raw=False):
        """cdb_render_rows (the tail of select(), database.cpp:394-441): the rows `ids` in the caller's order, each rendered as
        ac_automaton::render does for this key's keyword list.  Returns (found bool[nrows]; texts: list of bytes, None without
        `text`; spans: per row a list of (begin, end_inclusive) inside the original document, None without `spans`; missing).
        raw=True returns the C arrays (text_ptr, text_blob, span_ptr, begin, end, ...) in a dict instead."""
        return _render_rows(self, self._lib.cdb_render_rows, ids, keywords, left, right, text, spans, raw)

    def remove(self, ids):
        """cdb_remove: the documents `ids` leave the built index on the device (no rebuild, nothing uploaded but the ids); the handle
        then equals a fresh one built over the survivors.  Returns (removed: distinct documents dropped, missing: entries of `ids`
        the index does not hold)."""
        return _remove_ids(self, self._lib.cdb_remove, ids)

    def append(self, ids, blob, doc_start):
        """cdb_append: the documents (ids, blob, doc_start as for build_view) join the built index on the device — only they are
        uploaded and sorted; the handle then equals a fresh one built over the old documents followed by the new ones.  Returns the
        number of documents that joined."""
        return _append_docs(self, self._lib.cdb_append, ids, blob, doc_start)

    def verify_keys(self):
        """GPU-side check of the kept search keys against the text (cdb_debug_verify_keys); checked = 0: no keys are kept."""
        out = (C.c_uint64 * 2)()
        self._check(self._lib.cdb_debug_verify_keys(self._h, out))
        return {"mismatches": int(out[0]), "checked": int(out[1])}

    def set_option(self, name, value):
        self._check(self._lib.cdb_set_option(self._h, name.encode(), int(value)))

    def stat(self, name):
        v = C.c_double(0)
        if self._lib.cdb_get_stat(self._h, name.encode(), C.byref(v)) != 0:
            raise KeyError(name)
        return v.value

    def profile(self):
        buf = C.create_string_buffer(1 << 16)
        self._lib.cdb_profile_dump(self._h, buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, launches, nbytes = line.split()
            out[name] = {"ms": float(ms), "launches": int(launches), "bytes": int(nbytes)}
        return out

    def profile_reset(self):
        self._lib.cdb_profile_reset(self._h)


class _BorrowedIndex(GpuStringIndex):
    """A shard handle owned by its cdb_shards object: never destroyed from here."""

    def close(self):
        self._h = None

    __del__ = close


class GpuShards:
    """cdb_shards: the string index spread over several GPUs of one process (devices may repeat on a one-GPU box)."""

    def __init__(self, devices):
        self._lib = load_library()
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        rc = self._lib.cdb_shards_create(C.byref(h), arr, len(devices))
        if rc != 0:
            raise RuntimeError(f"cdb_shards_create failed (code {rc}): no usable gfx950 device — there is no CPU fallback")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cdb_shards_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.cdb_shards_last_error(self._h).decode(errors="replace"))

    def add(self, id_, value: bytes):
        self._check(self._lib.cdb_shards_add(self._h, int(id_), value, len(value)))

    def add_bulk(self, ids, blob, doc_start):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
        assert len(doc_start) == len(ids) + 1
        if len(doc_start) and int(doc_start[-1]) > len(blob):   # (the C ABI takes plain pointers: a short blob would be read past its end)
            raise ValueError(f"blob holds {len(blob)} bytes, doc_start[-1] = {int(doc_start[-1])}")
        self._check(self._lib.cdb_shards_add_bulk(self._h, _ptr(ids), _ptr(blob), _ptr(doc_start), len(ids)))

    def set_option(self, name, value):
        self._check(self._lib.cdb_shards_set_option(self._h, name.encode(), int(value)))

    def build(self):
        self._check(self._lib.cdb_shards_build(self._h))

    def build_views(self, ids, docs):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        ptrs = (C.c_char_p * len(docs))(*docs)
        lens = np.array([len(d) for d in docs], dtype=np.uint64)
        self._check(self._lib.cdb_shards_build_views(self._h, _ptr(ids), C.cast(ptrs, C.c_void_p), _ptr(lens), len(docs)))

    count = property(lambda s: s._lib.cdb_shards_count(s._h))
    transport = property(lambda s: s._lib.cdb_shards_transport(s._h).decode())

    def first_doc(self, i):
        return int(self._lib.cdb_shards_first_doc(self._h, i))

    def shard(self, i):
        """Borrowed GpuStringIndex view of shard i (do not close it)."""
        g = _BorrowedIndex.__new__(_BorrowedIndex)
        g._lib = self._lib
        g._h = C.c_void_p(self._lib.cdb_shards_get(self._h, i))
        return g

    def query(self, kw: bytes):
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_shards_query(self._h, kw, len(kw), C.byref(ids), C.byref(cnt), C.byref(n)))
        out = [(ids[i], cnt[i]) for i in range(n.value)]
        self._lib.cdb_free(ids)
        self._lib.cdb_free(cnt)
        return out

    @staticmethod
    def _pack(keywords):
        blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
        offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
        np.cumsum([len(k) for k in keywords], out=offs[1:])
        return blob, offs

    def query_or(self, keywords, ranked=False, lo=1, hi=(1 << 62), limit=0):
        blob, offs = self._pack(keywords)
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        bp = _ptr(blob) if len(blob) else None
        if ranked:
            self._check(self._lib.cdb_shards_query_ranked(self._h, bp, _ptr(offs), len(keywords), int(lo), int(hi), int(limit),
                                                          C.byref(ids), C.byref(cnt), C.byref(n)))
        else:
            self._check(self._lib.cdb_shards_query_or(self._h, bp, _ptr(offs), len(keywords), C.byref(ids), C.byref(cnt), C.byref(n)))
        out = [(ids[i], cnt[i]) for i in range(n.value)]
        self._lib.cdb_free(ids)
        self._lib.cdb_free(cnt)
        return out

    def query_spans(self, keywords):
        blob, offs = self._pack(keywords)
        r = CdbSpans()
        self._check(self._lib.cdb_shards_query_spans(self._h, _ptr(blob) if len(blob) else None, _ptr(offs), len(keywords), C.byref(r)))
        try:
            return [(r.ids[d], [(r.begin[k], r.end[k]) for k in range(r.span_ptr[d], r.span_ptr[d + 1])]) for d in range(r.ndocs)]
        finally:
            self._lib.cdb_spans_free(C.byref(r))

    def render_rows(self, ids, keywords, left=b"", right=b"", text=True, spans=True, raw=False):
        """GpuStringIndex.render_rows over all shards"""
        return _render_rows(self, self._lib.cdb_shards_render_rows, ids, keywords, left, right, text, spans, raw)

    def query_batch(self, blob, offsets):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        npat = len(offsets) - 1
        r = CdbResult()
        self._check(self._lib.cdb_shards_query_batch(self._h, _ptr(blob), _ptr(offsets), npat, C.byref(r)))
        own = GpuStringIndex._Owner(self._lib, ("cdb_result_free", r))
        nrows = int(r.nrows)
        ad = GpuStringIndex._adopt
        return (ad(r.row_ptr, npat + 1, np.uint64, own), ad(r.ids, nrows, np.int64, own), ad(r.counts, nrows, np.int64, own),
                int(r.nhits))

    def query_batch_offsets(self, blob, offsets):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        npat = len(offsets) - 1
        r, hx = CdbResult(), CdbHits()
        self._check(self._lib.cdb_shards_query_batch_offsets(self._h, _ptr(blob), _ptr(offsets), npat, C.byref(r), C.byref(hx)))
        own = GpuStringIndex._Owner(self._lib, ("cdb_result_free", r), ("cdb_hits_free", hx))
        nrows, nhits = int(r.nrows), int(r.nhits)
        ad = GpuStringIndex._adopt
        return (ad(r.row_ptr, npat + 1, np.uint64, own), ad(r.ids, nrows, np.int64, own), ad(r.counts, nrows, np.int64, own),
                ad(hx.hit_ptr, nrows + 1, np.uint64, own), ad(hx.offsets, nhits, np.uint64, own))

    def add_raw_dir(self, directory, key: bytes):
        nrec, nadd = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.cdb_shards_add_raw_dir(self._h, os.fsencode(directory), key, C.byref(nrec), C.byref(nadd)))
        return nrec.value, nadd.value

    def save(self, path):
        self._check(self._lib.cdb_shards_save(self._h, os.fsencode(path)))

    def load(self, path):
        self._check(self._lib.cdb_shards_load(self._h, os.fsencode(path)))

    def remove(self, ids):
        """cdb_shards_remove: GpuStringIndex.remove over all shards, all or nothing.  Returns (removed, missing); an emptied shard
        stays in place."""
        return _remove_ids(self, self._lib.cdb_shards_remove, ids)

    def append(self, ids, blob, doc_start):
        """cdb_shards_append: GpuStringIndex.append at the end of the sharded column — into the last shard while it stays within
        max_shard_bytes, else onto the idle device slots (`count` grows).  Returns the number of documents that joined."""
        return _append_docs(self, self._lib.cdb_shards_append, ids, blob, doc_start)

    def cluster(self, ids, with_values=True):
        """cdb_shards_cluster: GpuStringIndex.cluster over all shards (equal strings of different shards form one group)."""
        return _cluster_strings(self, self._lib.cdb_shards_cluster, ids, with_values)


class GpuColumn:
    """bool_index / integer_index / double_index on the GPU (cdb_column_*).  kind: 0 / "bool", 1 / "int64", 2 / "double" (the
    reference's `number` tags).  add_bulk() rows become visible at the next build(); query(range) returns [(id, 0), ...] in the
    reference's order ((value, id), bool: insertion order); query_any(ranges) the union's ids ascending (numpy int64)."""

    KINDS = {"bool": 0, "int64": 1, "double": 2}
    DTYPES = {0: np.uint8, 1: np.int64, 2: np.float64}

    def __init__(self, kind, device=-1):
        self._lib = load_library()
        self.kind = self.KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
        if self.kind not in (0, 1, 2):
            raise ValueError(f"GpuColumn: unknown kind {kind!r}")
        h = C.c_void_p()
        rc = self._lib.cdb_column_create(C.byref(h), device, self.kind)
        if rc != 0:
            raise RuntimeError(f"cdb_column_create failed (code {rc}): no usable gfx950 device — there is no CPU fallback")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cdb_column_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.cdb_column_last_error(self._h).decode(errors="replace"))

    def add_bulk(self, ids, values):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        vals = np.asarray(values)
        vals = np.ascontiguousarray(vals != 0 if self.kind == 0 else vals, dtype=self.DTYPES[self.kind])
        if len(ids) != len(vals):
            raise ValueError("add_bulk: ids and values differ in length")
        self._check(self._lib.cdb_column_add_bulk(self._h, _ptr(ids), _ptr(vals), len(ids)))

    def build(self):
        self._check(self._lib.cdb_column_build(self._h))

    def query_ids(self, range_):
        """query() as a numpy array of ids (same order)."""
        r = range_.encode() if isinstance(range_, str) else bytes(range_)
        ids, n = C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_column_query(self._h, r, len(r), C.byref(ids), C.byref(n)))
        try:
            return np.ctypeslib.as_array(ids, shape=(n.value,)).copy() if n.value else np.empty(0, dtype=np.int64)
        finally:
            self._lib.cdb_free(ids)

    def query(self, range_):
        return [(int(i), 0) for i in self.query_ids(range_)]

    @staticmethod
    def _pack(ranges):
        enc = [r.encode() if isinstance(r, str) else bytes(r) for r in ranges]
        blob = np.frombuffer(b"".join(enc), dtype=np.uint8)
        offs = np.zeros(len(enc) + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in enc], out=offs[1:])
        return blob, offs

    def query_any(self, ranges):
        blob, offs = self._pack(ranges)
        ids, n = C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(self._lib.cdb_column_query_any(self._h, _ptr(blob) if len(blob) else None, _ptr(offs), len(ranges),
                                                   C.byref(ids), C.byref(n)))
        try:
            return np.ctypeslib.as_array(ids, shape=(n.value,)).copy() if n.value else np.empty(0, dtype=np.int64)
        finally:
            self._lib.cdb_free(ids)

    def _values(self, values):
        vals = np.asarray(values)
        return np.ascontiguousarray(vals != 0 if self.kind == 0 else vals, dtype=self.DTYPES[self.kind])

    def append(self, ids, values):
        """cdb_column_append: the rows join the built column on the device (only they are uploaded and sorted); the column then
        equals one that got them by add_bulk() + build().  Returns the number of rows appended."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        vals = self._values(values)
        if len(ids) != len(vals):
            raise ValueError("append: ids and values differ in length")
        appended = C.c_uint64(0)
        self._check(self._lib.cdb_column_append(self._h, _ptr(ids) if len(ids) else None, _ptr(vals) if len(ids) else None, len(ids),
                                                C.byref(appended)))
        return int(appended.value)

    def arrays(self):
        """Test hook (cdb_debug_column_arrays): the device arrays (keys_v uint64, ids_v int64, id_sorted int64, vpos uint32)."""
        n = int(self.stat("rows"))
        out = (np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint32))
        self._check(self._lib.cdb_debug_column_arrays(self._h, *[_ptr(a) if n else None for a in out]))
        return out

    def remove(self, ids):
        """cdb_column_remove: the rows `ids` leave the column (built and staged rows alike) — compacted on the device, or, with
        staged rows, filtered on the host and rebuilt.  Returns (removed, missing) as GpuStringIndex.remove does."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        removed, missing = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.cdb_column_remove(self._h, _ptr(ids) if len(ids) else None, len(ids), C.byref(removed), C.byref(missing)))
        return int(removed.value), int(missing.value)

    def cluster(self, ids):
        """cdb_column_cluster (database.cpp:442-460 for this field): the rows `ids` grouped by value, ascending.  Returns
        (values: int64 / float64 / bool array, counts int64, rep_ids int64: the smallest id of each group among the rows,
        missing: rows whose id the column does not hold)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        r = CdbClusters()
        self._check(self._lib.cdb_column_cluster(self._h, _ptr(ids) if len(ids) else None, len(ids), C.byref(r)))
        try:
            ng = int(r.ngroups)
            raw = _array(r.values, ng, np.uint64)
            values = raw.astype(np.bool_) if self.kind == 0 else raw.view(np.int64 if self.kind == 1 else np.float64)
            return values, _array(r.counts, ng, np.int64), _array(r.rep_ids, ng, np.int64), int(r.missing)
        finally:
            self._lib.cdb_clusters_free(C.byref(r))

    def _typed(self, raw):
        """raw uint64 values (cdb_clusters.values, cdb_column_values) as the column's dtype"""
        return raw.astype(np.bool_) if self.kind == 0 else raw.view(np.int64 if self.kind == 1 else np.float64)

    def values(self, ids, with_missing=False, raw=False):
        """cdb_column_values (data[id][field] of database.cpp:406-415): the value of every row of `ids`, in the caller's order.  Returns
        (values as the column's dtype, found bool array); a row the column does not hold has found False and value 0.  raw=True
        leaves the values as the uint64 the C side returns; with_missing=True appends the count of rows not found."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = len(ids)
        vals, found, missing = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8), C.c_uint64(0)
        self._check(self._lib.cdb_column_values(self._h, _ptr(ids) if n else None, n, _ptr(vals) if n else None, _ptr(found) if n else None,
                                                C.byref(missing)))
        out = (vals if raw else self._typed(vals), found.astype(bool))
        return out + (int(missing.value),) if with_missing else out

    def stat(self, name):
        v = C.c_double(0)
        if self._lib.cdb_column_get_stat(self._h, name.encode(), C.byref(v)) != 0:
            raise KeyError(name)
        return v.value

    def set_option(self, name, value):
        """Test / measurement hook (cdb_debug_column_set_option): "profile", "debug_query_path", "debug_cluster_path",
        "debug_maintain_path", "debug_fail_prepare", "debug_fail_append_prepare"."""
        self._check(self._lib.cdb_debug_column_set_option(self._h, name.encode(), int(value)))

    def profile(self):
        buf = C.create_string_buffer(1 << 16)
        self._lib.cdb_debug_column_profile_dump(self._h, buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, launches, nbytes = line.split()
            out[name] = {"ms": float(ms), "launches": int(launches), "bytes": int(nbytes)}
        return out


class ShardComm:
    """cdb_comm: one rank of a one-process-per-GPU group; merge() is collective."""

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = np.zeros(128, dtype=np.uint8)
        if lib.cdb_comm_unique_id(_ptr(buf)) != 0:
            raise RuntimeError("cdb_comm_unique_id failed: RCCL is not available")
        return buf

    def __init__(self, uid, rank, world, device):
        self._lib = load_library()
        uid = np.ascontiguousarray(uid, dtype=np.uint8)
        h = C.c_void_p()
        rc = self._lib.cdb_comm_create(C.byref(h), _ptr(uid), rank, world, device)
        if rc != 0:
            raise RuntimeError(f"cdb_comm_create failed (code {rc})")
        self._h = h

    @classmethod
    def group(cls, devices):
        """The ranks of ONE process (cdb_comm_create_group): one ShardComm per entry of `devices`; a host thread per rank
        calls the collectives.  Ranks sharing a device exchange through device copies."""
        lib = load_library()
        devs = (C.c_int * len(devices))(*devices)
        hs = (C.c_void_p * len(devices))()
        rc = lib.cdb_comm_create_group(hs, len(devices), devs)
        if rc != 0:
            raise RuntimeError(f"cdb_comm_create_group failed (code {rc})")
        out = []
        for h in hs:
            c = cls.__new__(cls)
            c._lib, c._h = lib, C.c_void_p(h)
            out.append(c)
        return out

    def merge(self, local: "CdbDeviceResult"):
        out = CdbDeviceResult()
        if self._lib.cdb_comm_merge(self._h, C.byref(local), C.byref(out)) != 0:
            raise RuntimeError(self._lib.cdb_comm_last_error(self._h).decode(errors="replace"))
        return out

    def merge_counts(self, local: "CdbDeviceResult"):
        """Counts-only collective: merged row_ptr + this rank's first merged row per pattern (device arrays)."""
        out = CdbShardSlice()
        if self._lib.cdb_comm_merge_counts(self._h, C.byref(local), C.byref(out)) != 0:
            raise RuntimeError(self._lib.cdb_comm_last_error(self._h).decode(errors="replace"))
        return out

    world = property(lambda s: s._lib.cdb_comm_world(s._h))
    transport = property(lambda s: s._lib.cdb_comm_transport(s._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cdb_comm_destroy(self._h)
            self._h = None

    __del__ = close


def memory_stats():
    """(in_use, peak, cached) bytes of device memory as the library's allocator sees the process (cdb_memory_stats)."""
    lib = load_library()
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lib.cdb_memory_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def memory_reset_peak():
    load_library().cdb_memory_reset_peak()


def _pack_column_keys(keys):
    """The keys of query_and() as the arrays cdb_query_and_columns / cdb_filter take: (cdb_key_query array or None, its length,
    cdb_column_key array, its length, the handle that carries an error, the buffers to keep alive during the call)."""
    plain = [(ix, data) for ix, data in keys if not isinstance(ix, GpuColumn)]
    colk = [(ix, data) for ix, data in keys if isinstance(ix, GpuColumn)]
    arr = (CdbKeyQuery * max(len(plain), 1))()
    carr = (CdbColumnKey * len(colk))()
    keep = []
    lead = None
    for k, (ix, data) in enumerate(plain):
        if isinstance(ix, GpuStringIndex):
            lead = lead or ix
            blob = np.frombuffer(b"".join(data), dtype=np.uint8)
            offs = np.zeros(len(data) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in data], out=offs[1:])
            keep += [blob, offs]
            arr[k].index = ix._h
            arr[k].blob = blob.ctypes.data if len(blob) else None
            arr[k].offsets = offs.ctypes.data
            arr[k].nkw = len(data)
        elif ix is None:
            ri = np.ascontiguousarray([r[0] for r in data], dtype=np.int64)
            rc = np.ascontiguousarray([r[1] for r in data], dtype=np.int64)
            keep += [ri, rc]
            arr[k].ids = ri.ctypes.data if len(ri) else None
            arr[k].counts = rc.ctypes.data if len(rc) else None
            arr[k].nrows = len(ri)
        else:
            raise TypeError(f"query_and: column keys combine with GpuStringIndex keys and host rows only, not {type(ix).__name__}")
    for j, (col, ranges) in enumerate(colk):
        ranges = [ranges] if isinstance(ranges, (str, bytes)) else list(ranges)
        blob, offs = GpuColumn._pack(ranges)
        keep += [blob, offs]
        carr[j].column = col._h
        carr[j].blob = blob.ctypes.data if len(blob) else None
        carr[j].offsets = offs.ctypes.data
        carr[j].nranges = len(ranges)
    if lead is None and colk:
        lead = colk[0][0]
    return (arr if plain else None), len(plain), carr, len(colk), lead, keep


def _raise_lead_error(lib, lead, what):
    if isinstance(lead, GpuColumn):
        raise RuntimeError(lib.cdb_column_last_error(lead._h).decode(errors="replace"))
    if lead is not None:
        raise RuntimeError(lib.cdb_last_error(lead._h).decode(errors="replace"))
    raise RuntimeError(f"{what}: no string key and no column")


def _query_and_columns(keys, ranked, lo, hi, limit):
    """cdb_query_and_columns: the keys of query_and() with (GpuColumn, [ranges]) among them."""
    lib = load_library()
    arr, nk, carr, nc, lead, keep = _pack_column_keys(keys)
    ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
    rc_ = lib.cdb_query_and_columns(arr, nk, carr, nc, 1 if ranked else 0, int(lo), int(hi), int(limit),
                                    C.byref(ids), C.byref(cnt), C.byref(n))
    if rc_ != 0:
        _raise_lead_error(lib, lead, "cdb_query_and_columns")
    out = [(ids[i], cnt[i]) for i in range(n.value)]
    lib.cdb_free(ids)
    lib.cdb_free(cnt)
    return out


def query_and(keys, ranked=False, lo=1, hi=(1 << 62), limit=0):
    """AND across keys on the device (cdb_query_and / cdb_shards_query_and / cdb_query_and_columns).  keys: (GpuStringIndex or
    GpuShards, [keywords]) for a string column, (GpuColumn, [ranges]) for a numeric / bool column or (None, [(id, count), ...])
    for rows resolved elsewhere (ascending id).  Returns [(id, summed count), ...]."""
    if any(isinstance(ix, GpuColumn) for ix, _ in keys):
        return _query_and_columns(keys, ranked, lo, hi, limit)
    lib = load_library()
    sharded = any(isinstance(ix, GpuShards) for ix, _ in keys)
    arr = (CdbKeyQuery * len(keys))()
    keep = []
    lead = None
    for k, (ix, data) in enumerate(keys):
        if ix is not None and not isinstance(ix, (GpuShards, GpuStringIndex)):
            raise TypeError(f"query_and: key {k} is neither a GpuStringIndex, a GpuShards nor None")
        if sharded and isinstance(ix, GpuStringIndex):
            # a plain index beside sharded keys: cdb_shards_key_query.shards must be a cdb_shards* — handing it a cdb_index*
            # would be reinterpreted.  Resolve the key with its own OR (ascending id) and pass the rows.
            if not data:
                raise RuntimeError("The constraint list cannot be empty")
            ix, data = None, ix.query_or(list(data))
        if ix is not None:
            if lead is None or (sharded and not isinstance(lead, GpuShards)):
                lead = ix
            blob = np.frombuffer(b"".join(data), dtype=np.uint8)
            offs = np.zeros(len(data) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in data], out=offs[1:])
            keep += [blob, offs]
            arr[k].index = ix._h
            arr[k].blob = blob.ctypes.data if len(blob) else None
            arr[k].offsets = offs.ctypes.data
            arr[k].nkw = len(data)
        else:
            ri = np.ascontiguousarray([r[0] for r in data], dtype=np.int64)
            rc = np.ascontiguousarray([r[1] for r in data], dtype=np.int64)
            keep += [ri, rc]
            arr[k].ids = ri.ctypes.data if len(ri) else None
            arr[k].counts = rc.ctypes.data if len(rc) else None
            arr[k].nrows = len(ri)
    ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
    fn = lib.cdb_shards_query_and if sharded else lib.cdb_query_and  # (cdb_shards_key_query has cdb_key_query's layout)
    rc_ = fn(arr, len(keys), 1 if ranked else 0, int(lo), int(hi), int(limit), C.byref(ids), C.byref(cnt), C.byref(n))
    if rc_ != 0:
        err = lib.cdb_shards_last_error if isinstance(lead, GpuShards) else lib.cdb_last_error
        raise RuntimeError(err(lead._h).decode(errors="replace") if lead is not None else "cdb_query_and: no string key")
    out = [(ids[i], cnt[i]) for i in range(n.value)]
    lib.cdb_free(ids)
    lib.cdb_free(cnt)
    return out


class GpuRowSet:
    """A filtered row set that stays on the device (cdb_rowset_*): made by filter_rows() or debug_rowset_from_rows().  `size` is the
    `count` operation; rows() all rows ascending by id; page(first, last) rows [first, last) of the ranking (descending count as
    signed int64, ties ascending id); cluster(field) groups the rows by a GpuStringIndex or GpuColumn without uploading them;
    select(first, last, fields) is page() plus the fields of its rows, read on the device in the same call.
    rows() and page() return (ids, counts) as numpy int64 arrays."""

    def __init__(self, handle):
        self._lib = load_library()
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cdb_rowset_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.cdb_rowset_last_error(self._h).decode(errors="replace"))

    @property
    def size(self):
        return int(self._lib.cdb_rowset_size(self._h))

    def __len__(self):
        return self.size

    def _rows(self, fn, *args):
        ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        self._check(fn(self._h, *args, C.byref(ids), C.byref(cnt), C.byref(n)))
        try:
            return _array(ids, n.value, np.int64), _array(cnt, n.value, np.int64)
        finally:
            self._lib.cdb_free(ids)
            self._lib.cdb_free(cnt)

    def rows(self):
        return self._rows(self._lib.cdb_rowset_rows)

    def page(self, first, last):
        return self._rows(self._lib.cdb_rowset_page, int(first), int(last))

    def cluster(self, field, with_values=True):
        """GpuStringIndex.cluster / GpuColumn.cluster of this set's ids, with their return values."""
        r = CdbClusters()
        if isinstance(field, GpuColumn):
            self._check(self._lib.cdb_rowset_cluster_column(self._h, field._h, C.byref(r)))
        elif isinstance(field, GpuStringIndex):
            self._check(self._lib.cdb_rowset_cluster(self._h, field._h, 1 if with_values else 0, C.byref(r)))
        else:
            raise TypeError(f"GpuRowSet.cluster: {type(field).__name__} is neither a GpuStringIndex nor a GpuColumn")
        try:
            ng = int(r.ngroups)
            counts, reps = _array(r.counts, ng, np.int64), _array(r.rep_ids, ng, np.int64)
            if isinstance(field, GpuColumn):
                raw = _array(r.values, ng, np.uint64)
                values = raw.astype(np.bool_) if field.kind == 0 else raw.view(np.int64 if field.kind == 1 else np.float64)
                return values, counts, reps, int(r.missing)
            values = None
            if with_values:
                ptr = _array(r.value_ptr, ng + 1, np.uint64)
                blob = C.string_at(r.value_blob, int(ptr[ng])) if ng else b""
                values = [blob[int(ptr[g]):int(ptr[g + 1])] for g in range(ng)]
            return values, counts, reps, int(r.missing)
        finally:
            self._lib.cdb_clusters_free(C.byref(r))

    def select(self, first, last, fields, left=b"", right=b"", raw=False):
        """cdb_rowset_select: rows [first, last) of the ranking (page()'s rules) with their fields, read on the device in one call.
        `fields` is a list of (GpuStringIndex | GpuShards, keywords) pairs — keywords may be empty: the plain document — and
        GpuColumn objects.  Returns (ids, counts, per-field results in the caller's order): a string field gives
        (texts: list of bytes, found bool array, missing), a column (values as its dtype, found, missing).  raw=True leaves every
        field as a dict of the C arrays ("kind", "found", "missing", and "values" uint64 or "text_ptr" / "text_blob")."""
        packed, keep = (CdbSelectField * max(len(fields), 1))(), []
        for k, f in enumerate(fields):
            q = packed[k]
            if isinstance(f, GpuColumn):
                q.column = f._h
                continue
            handle, keywords = f
            if isinstance(handle, GpuShards):
                q.shards = handle._h
            elif isinstance(handle, GpuStringIndex):
                q.index = handle._h
            else:
                raise TypeError(f"GpuRowSet.select: field {k}: {type(handle).__name__} is neither a GpuStringIndex nor a GpuShards")
            keywords = [bytes(x) for x in keywords]
            blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
            offs = np.zeros(len(keywords) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in keywords], out=offs[1:])
            keep += [blob, offs]
            q.kw_blob, q.kw_offsets, q.nkw = (blob.ctypes.data if len(blob) else None), offs.ctypes.data, len(keywords)
        left, right = bytes(left), bytes(right)
        r = CdbSelected()
        self._check(self._lib.cdb_rowset_select(self._h, int(first), int(last), packed, len(fields), left if left else None, len(left),
                                                right if right else None, len(right), C.byref(r)))
        try:
            n = int(r.nrows)
            out = []
            for k, f in enumerate(fields):
                g = r.fields[k]
                found = _array(g.found, n, np.uint8).astype(bool)
                if g.kind == SELECT_STRING:
                    tp = _array(g.text_ptr, n + 1, np.uint64)
                    tb = C.string_at(g.text_blob, int(tp[n]))
                    if raw:
                        out.append({"kind": g.kind, "found": found, "missing": int(g.missing), "text_ptr": tp, "text_blob": tb})
                    else:
                        out.append(([tb[int(tp[i]):int(tp[i + 1])] for i in range(n)], found, int(g.missing)))
                else:
                    vals = _array(g.values, n, np.uint64)
                    if raw:
                        out.append({"kind": g.kind, "found": found, "missing": int(g.missing), "values": vals})
                    else:
                        out.append((f._typed(vals), found, int(g.missing)))
            return _array(r.ids, n, np.int64), _array(r.counts, n, np.int64), out
        finally:
            self._lib.cdb_selected_free(C.byref(r))

    def remove(self, fields):
        """cdb_rowset_remove: the rows of this set leave every field of `fields` (GpuStringIndex and GpuColumn objects), all or none;
        the ids stay on the device.  Returns (rows, per-field dicts "removed", "missing", "status", "committed" in the caller's
        order).  A failure raises RowSetRemoveError, a RuntimeError that carries the return code as `.code` and the per-field dicts as
        `.fields`."""
        packed = (CdbRemoveField * max(len(fields), 1))()
        for k, f in enumerate(fields):
            if isinstance(f, GpuColumn):
                packed[k].column = f._h
            elif isinstance(f, GpuStringIndex):
                packed[k].index = f._h
            else:
                raise TypeError(f"GpuRowSet.remove: field {k}: {type(f).__name__} is neither a GpuStringIndex nor a GpuColumn")
        rows = C.c_uint64(0)
        rc_ = self._lib.cdb_rowset_remove(self._h, packed, len(fields), C.byref(rows))
        out = [{"removed": int(q.removed), "missing": int(q.missing), "status": int(q.status), "committed": int(q.committed)}
               for q in packed[:len(fields)]]
        if rc_ != 0:
            e = RowSetRemoveError(self._lib.cdb_rowset_last_error(self._h).decode(errors="replace"))
            e.code, e.fields, e.rows = rc_, out, int(rows.value)
            raise e
        return int(rows.value), out

    def stat(self, name):
        v = C.c_double(0)
        if self._lib.cdb_rowset_get_stat(self._h, name.encode(), C.byref(v)) != 0:
            raise KeyError(name)
        return v.value

    def set_option(self, name, value):
        """Test / measurement hook (cdb_debug_rowset_set_option): "debug_page_path" (0 automatic, 1 select, 2 sort), "profile"."""
        if self._lib.cdb_debug_rowset_set_option(self._h, name.encode(), int(value)) != 0:
            raise ValueError(f"GpuRowSet.set_option: {name} = {value}")

    def profile(self):
        buf = C.create_string_buffer(1 << 16)
        self._lib.cdb_debug_rowset_profile_dump(self._h, buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, launches, nbytes = line.split()
            out[name] = {"ms": float(ms), "launches": int(launches), "bytes": int(nbytes)}
        return out


class RowSetRemoveError(RuntimeError):
    """GpuRowSet.remove failed: `.code` is the library's return code, `.fields` the per-field results, `.rows` the set's size."""
    code, fields, rows = 0, (), 0


def rowset_all(fields):
    """cdb_rowset_all: the GpuRowSet of every object the given fields (GpuStringIndex and GpuColumn objects) hold — the union of their
    ids, ascending as signed int64, every count 0.  filter() without constraints."""
    lib = load_library()
    idx = [f for f in fields if isinstance(f, GpuStringIndex)]
    cols = [f for f in fields if isinstance(f, GpuColumn)]
    if len(idx) + len(cols) != len(fields):
        raise TypeError("rowset_all: fields are GpuStringIndex and GpuColumn objects")
    ai = (C.c_void_p * max(len(idx), 1))(*[f._h for f in idx])
    ac = (C.c_void_p * max(len(cols), 1))(*[f._h for f in cols])
    h = C.c_void_p()
    rc_ = lib.cdb_rowset_all(ai if idx else None, len(idx), ac if cols else None, len(cols), C.byref(h))
    if rc_ != 0:
        lead = idx[0] if idx else (cols[0] if cols else None)
        if lead is None:
            raise RuntimeError(f"cdb_rowset_all failed (code {rc_}): no field given")
        err = lib.cdb_last_error if idx else lib.cdb_column_last_error
        raise RuntimeError(err(lead._h).decode(errors="replace"))
    return GpuRowSet(h)


class InsertObjectsError(RuntimeError):
    """insert_objects failed: `.code` is the library's return code, `.fields` the per-field results."""
    code, fields = 0, ()


def insert_objects(ids, fields):
    """cdb_insert_objects: the objects `ids` join every field of `fields`, all or none.  A field is a tuple (handle, rows, payload):
    handle a GpuStringIndex or a GpuColumn; rows the strictly ascending indices into `ids` of the objects that hold the field, or
    None for every object; payload (blob, doc_start) for a string field — as GpuStringIndex.append takes them — and the values for a
    column.  Returns (inserted, per-field dicts "appended", "status", "committed" in the caller's order).  A failure raises
    InsertObjectsError, a RuntimeError with the first field's error text that carries the return code as `.code` and the per-field
    dicts as `.fields`."""
    lib = load_library()
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    packed = (CdbInsertField * max(len(fields), 1))()
    keep = []   # the arrays the packed pointers refer to
    for k, (f, rows, payload) in enumerate(fields):
        q = packed[k]
        if rows is None:
            q.nrows = len(ids)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.uint64)
            q.nrows = len(rows)
            if not len(rows):
                rows = np.zeros(1, dtype=np.uint64)   # (no row: the C ABI still wants a pointer, NULL means every object)
            keep.append(rows)
            q.rows = _ptr(rows)
        n = int(q.nrows)
        if isinstance(f, GpuColumn):
            q.column = f._h
            vals = f._values(payload if payload is not None else [])
            if len(vals) != n:
                raise ValueError(f"insert_objects: field {k}: {len(vals)} values for {n} rows")
            keep.append(vals)
            q.values = _ptr(vals) if n else None
        elif isinstance(f, GpuStringIndex):
            q.index = f._h
            blob, doc_start = payload if payload is not None else (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
            if len(doc_start) != n + 1:
                raise ValueError(f"insert_objects: field {k}: doc_start holds {len(doc_start)} entries for {n} rows")
            if int(doc_start[-1]) > len(blob):   # (the C ABI takes plain pointers: a short blob would be read past its end)
                raise ValueError(f"insert_objects: field {k}: blob holds {len(blob)} bytes, doc_start[-1] = {int(doc_start[-1])}")
            if not len(blob):
                blob = np.zeros(1, dtype=np.uint8)   # (empty documents only: the C ABI still wants a pointer)
            keep += [blob, doc_start]
            q.blob, q.doc_start = _ptr(blob), _ptr(doc_start)
        else:
            raise TypeError(f"insert_objects: field {k}: {type(f).__name__} is neither a GpuStringIndex nor a GpuColumn")
    inserted = C.c_uint64(0)
    rc_ = lib.cdb_insert_objects(_ptr(ids) if len(ids) else None, len(ids), packed, len(fields), C.byref(inserted))
    out = [{"appended": int(q.appended), "status": int(q.status), "committed": int(q.committed)} for q in packed[:len(fields)]]
    if rc_ != 0:
        lead = fields[0][0] if fields else None
        if lead is None:
            raise RuntimeError(f"cdb_insert_objects failed (code {rc_}): no field given")
        err = lib.cdb_last_error if isinstance(lead, GpuStringIndex) else lib.cdb_column_last_error
        e = InsertObjectsError(err(lead._h).decode(errors="replace"))
        e.code, e.fields = rc_, out
        raise e
    return int(inserted.value), out


def insert_stat(lead, name):
    """cdb_insert_get_stat on the handle that led insert_objects calls (their first field): "inserts", "insert_fields",
    "insert_objects", "insert_ms"."""
    lib = load_library()
    v = C.c_double(0)
    col = isinstance(lead, GpuColumn)
    if lib.cdb_insert_get_stat(None if col else lead._h, lead._h if col else None, name.encode(), C.byref(v)) != 0:
        raise KeyError(name)
    return v.value


def filter_rows(keys, corr=None):
    """cdb_filter: the keys of query_and() (GpuStringIndex, GpuColumn and host-row keys; resolve a GpuShards key with its query_or
    first) merged on the device into a GpuRowSet.  corr = (lo, hi) keeps rows with lo <= count < hi."""
    lib = load_library()
    arr, nk, carr, nc, lead, keep = _pack_column_keys(keys)
    lo, hi = (0, 0) if corr is None else corr
    h = C.c_void_p()
    rc_ = lib.cdb_filter(arr, nk, carr if nc else None, nc, 0 if corr is None else 1, int(lo), int(hi), C.byref(h))
    if rc_ != 0:
        _raise_lead_error(lib, lead, "cdb_filter")
    return GpuRowSet(h)


def debug_rowset_from_rows(ids, counts, device=-1):
    """Test hook (cdb_debug_rowset_from_rows): a GpuRowSet over the given rows, ids ascending."""
    lib = load_library()
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if len(ids) != len(counts):
        raise ValueError("debug_rowset_from_rows: ids and counts differ in length")
    h = C.c_void_p()
    rc_ = lib.cdb_debug_rowset_from_rows(device, _ptr(ids) if len(ids) else None, _ptr(counts) if len(counts) else None, len(ids), C.byref(h))
    if rc_ != 0:
        raise RuntimeError(f"cdb_debug_rowset_from_rows failed (code {rc_})" + (": no usable gfx950 device" if rc_ == 2 else ""))
    return GpuRowSet(h)


def debug_radix_sort(d_keys_ptr, d_vals_ptr, n, val_bytes, key_bits, variant=0, device=-1):
    """In-place device sort through the library's radix primitive; returns (onesweep_ms, passes)."""
    lib = load_library()
    ms, passes = C.c_double(0), C.c_int(0)
    rc = lib.cdb_debug_radix_sort(device, C.c_void_p(d_keys_ptr), C.c_void_p(d_vals_ptr) if d_vals_ptr else None, n,
                                  val_bytes, key_bits, variant, C.byref(ms), C.byref(passes))
    if rc != 0:
        raise RuntimeError(f"cdb_debug_radix_sort failed ({rc})")
    return ms.value, passes.value


SORT_DEVICE_HIST, SORT_SPARE_VALUES, SORT_POISON, SORT_GROUPED, SORT_PROFILE = 1, 2, 4, 8, 16


class CdbDebugSortResult(C.Structure):
    _fields_ = [("passes_run", C.c_int), ("passes_skipped", C.c_int), ("key_result", C.c_int), ("value_result", C.c_int),
                ("fell_back", C.c_int), ("epoch", C.c_uint32), ("onesweep_ms", C.c_double)]


class SortError(RuntimeError):
    """A sort hook failed; `status` is the CDB_E_* code of the error thrown inside the library."""

    def __init__(self, what, status):
        super().__init__(f"{what} failed ({status})")
        self.status = status


class DebugSortWorkspace:
    """A RadixWorkspace and its stream that outlive one sort (cdb_debug_sort_ws_*): pass it as `ws` to the sort hooks."""

    def __init__(self, device=-1):
        lib = load_library()
        lib.cdb_debug_sort_ws_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.cdb_debug_sort_ws_destroy.argtypes = [C.c_void_p]
        lib.cdb_debug_sort_ws_destroy.restype = None
        self._h = C.c_void_p()
        rc = lib.cdb_debug_sort_ws_create(device, C.byref(self._h))
        if rc != 0:
            raise SortError("cdb_debug_sort_ws_create", rc)

    def close(self):
        if self._h:
            load_library().cdb_debug_sort_ws_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _sort_result(r):
    return {name: getattr(r, name) for name, _ in CdbDebugSortResult._fields_}


def debug_radix_sort_ex(d_keys_ptr, d_vals_ptr, n, key_bytes, val_bytes, begin_bit, end_bit, dbits=8, variant=0, flags=0, ws=None,
                        device=-1):
    """radix_sort<K, V> as the library calls it, in place on device memory; returns the hook's result record as a dict.
    Raises SortError with the status of the error thrown."""
    lib = load_library()
    lib.cdb_debug_radix_sort_ex.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_uint, C.POINTER(CdbDebugSortResult)]
    r = CdbDebugSortResult()
    rc = lib.cdb_debug_radix_sort_ex(device, ws._h if ws is not None else None, C.c_void_p(d_keys_ptr),
                                     C.c_void_p(d_vals_ptr) if d_vals_ptr else None, n, key_bytes, val_bytes, begin_bit, end_bit,
                                     dbits, variant, flags, C.byref(r))
    if rc != 0:
        raise SortError("cdb_debug_radix_sort_ex", rc)
    return _sort_result(r)


def debug_radix_sort_split(d_keys_ptr, d_vals_ptr, d_aux_ptr, n, val_bytes, aux_bytes, hi_bits, lead_digits, variant=0, flags=0,
                           ws=None, device=-1):
    """radix_sort_split over materialised (u32 key, value, auxiliary word) records, in place on device memory."""
    lib = load_library()
    lib.cdb_debug_radix_sort_split.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(CdbDebugSortResult)]
    r = CdbDebugSortResult()
    rc = lib.cdb_debug_radix_sort_split(device, ws._h if ws is not None else None, C.c_void_p(d_keys_ptr), C.c_void_p(d_vals_ptr),
                                        C.c_void_p(d_aux_ptr), n, val_bytes, aux_bytes, hi_bits, lead_digits, variant, flags,
                                        C.byref(r))
    if rc != 0:
        raise SortError("cdb_debug_radix_sort_split", rc)
    return _sort_result(r)


SCAN_U64_ADD, SCAN_U64_MAX, SCAN_U2_ADD, SCAN_U2_SUMMAX, SCAN_DOCMAX, SCAN_FLAGS_ADD = range(6)


class ScanError(RuntimeError):
    """A scan hook failed; `status` is the CDB_E_* code of the error thrown inside the library."""

    def __init__(self, what, status):
        super().__init__(f"{what} failed ({status})")
        self.status = status


def _scan_item_shape(kind, n):
    return (n,) if kind in (SCAN_U64_ADD, SCAN_U64_MAX) else (n, 2)


def debug_scan(kind, items, device=-1):
    """scan_totals + scan_apply as the library calls them (cdb_debug_scan).  items: uint64[n] for the two uint64 kinds, uint64[n, 2]
    for the pair kinds, uint8[n] flag bytes for SCAN_FLAGS_ADD.  Returns (exclusive, inclusive, total) as uint64 arrays."""
    lib = load_library()
    lib.cdb_debug_scan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    items = np.ascontiguousarray(items, dtype=np.uint8 if kind == SCAN_FLAGS_ADD else np.uint64)
    n = items.shape[0]
    if items.shape != ((n,) if kind == SCAN_FLAGS_ADD else _scan_item_shape(kind, n)):
        raise ValueError(f"scan kind {kind}: items of shape {items.shape}")
    ex = np.zeros(_scan_item_shape(kind, n), dtype=np.uint64)
    inc = np.zeros_like(ex)
    total = np.zeros(_scan_item_shape(kind, 1)[1:], dtype=np.uint64)
    rc = lib.cdb_debug_scan(device, kind, items.ctypes.data if n else None, n, ex.ctypes.data if n else None,
                            inc.ctypes.data if n else None, total.ctypes.data)
    if rc != 0:
        raise ScanError("cdb_debug_scan", rc)
    return ex, inc, total


def debug_scan_partials(kind, sums, guard_words=64, device=-1):
    """scan_partials_inplace over raw tile sums (cdb_debug_scan_partials; kinds 0..4, items as for debug_scan).  Returns
    (exclusive prefixes [nb], grand total, guard intact)."""
    lib = load_library()
    lib.cdb_debug_scan_partials.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]
    sums = np.ascontiguousarray(sums, dtype=np.uint64)
    nb = sums.shape[0]
    if kind == SCAN_FLAGS_ADD or sums.shape != _scan_item_shape(kind, nb):
        raise ValueError(f"scan kind {kind}: sums of shape {sums.shape}")
    buf = np.zeros(_scan_item_shape(kind, nb + 1), dtype=np.uint64)
    buf[:nb] = sums
    ok = C.c_int(0)
    rc = lib.cdb_debug_scan_partials(device, kind, buf.ctypes.data, nb, guard_words, C.byref(ok))
    if rc != 0:
        raise ScanError("cdb_debug_scan_partials", rc)
    return buf[:nb], buf[nb], bool(ok.value)


def debug_stable_ranks(flags, device=-1):
    """tile_bases + TileRanker over flag bytes (cdb_debug_stable_ranks).  Returns (flagged slots in front of every slot [n], in
    front of every tile of 4096 slots, the total tile_bases returned)."""
    lib = load_library()
    lib.cdb_debug_stable_ranks.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    n = flags.shape[0]
    before = np.zeros(n, dtype=np.uint64)
    tile_base = np.zeros(max((n + 4095) // 4096, 1), dtype=np.uint64)
    total = C.c_uint64(0)
    rc = lib.cdb_debug_stable_ranks(device, flags.ctypes.data, n, before.ctypes.data, tile_base.ctypes.data, C.byref(total))
    if rc != 0:
        raise ScanError("cdb_debug_stable_ranks", rc)
    return before, tile_base[:(n + 4095) // 4096], total.value


CARRIED_PACKED40, CARRIED_U32, CARRIED_U64 = range(3)


class CarriedError(RuntimeError):
    """The carried-round hook failed; `status` is the CDB_E_* code of the error thrown inside the library."""

    def __init__(self, what, status):
        super().__init__(f"{what} failed ({status})")
        self.status = status


def debug_carried_inplace(entries, flags, xbits, form=CARRIED_PACKED40, device=-1):
    """The in-place carried round over (entries, flag bytes) as the build launches it (cdb_debug_carried_inplace).  Returns
    (entries uint64[n], flags uint8[n], partials uint64[tiles, 2], open entries met, entries moved, guards intact)."""
    lib = load_library()
    lib.cdb_debug_carried_inplace.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int)]
    entries = np.array(entries, dtype=np.uint64)   # (copies: the hook works in place)
    flags = np.array(flags, dtype=np.uint8)
    n = entries.shape[0]
    if entries.shape != (n,) or flags.shape != (n,):
        raise ValueError(f"entries of shape {entries.shape}, flags of shape {flags.shape}")
    partials = np.zeros(((n + 4095) // 4096, 2), dtype=np.uint64)
    counts = np.zeros(2, dtype=np.uint64)
    ok = C.c_int(0)
    rc = lib.cdb_debug_carried_inplace(device, form, entries.ctypes.data if n else None, flags.ctypes.data if n else None, n, xbits,
                                       partials.ctypes.data, counts.ctypes.data, C.byref(ok))
    if rc != 0:
        raise CarriedError("cdb_debug_carried_inplace", rc)
    return entries, flags, partials, int(counts[0]), int(counts[1]), bool(ok.value)


SEGSORT_FIVE_PASS, SEGSORT_TOP_FIRST = range(2)


class SegsortError(RuntimeError):
    """The segmented-sort hook failed; `status` is the CDB_E_* code of the error thrown inside the library."""

    def __init__(self, what, status):
        super().__init__(f"{what} failed ({status})")
        self.status = status


def debug_segsort(form, bucket_begin, k32, v32, w16, ehb, carry, packed=True, device=-1):
    """One bucket group through the segmented sort in the given form (cdb_debug_segsort).  Returns (entries uint64[n],
    flags uint8[n], cells uint64[ncells, 3] = (begin, end, tile_begin) — empty for the five-pass form —, guards intact)."""
    lib = load_library()
    lib.cdb_debug_segsort.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_int)]
    bb = np.ascontiguousarray(bucket_begin, dtype=np.uint64)
    k32 = np.ascontiguousarray(k32, dtype=np.uint32)
    v32 = np.ascontiguousarray(v32, dtype=np.uint32)
    w16 = np.ascontiguousarray(w16, dtype=np.uint16)
    n, nb = k32.shape[0], bb.shape[0] - 1
    if v32.shape != (n,) or w16.shape != (n,) or nb < 1:
        raise ValueError("record arrays of different lengths, or no bucket")
    entries = np.zeros(max(n, 1), dtype=np.uint64)
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    cells = np.zeros((nb * 256, 3), dtype=np.uint64)
    ncells, ok = C.c_uint32(0), C.c_int(0)
    rc = lib.cdb_debug_segsort(device, form, 1 if packed else 0, n, nb, bb.ctypes.data, k32.ctypes.data, v32.ctypes.data, w16.ctypes.data,
                               ehb, carry, entries.ctypes.data, flags.ctypes.data, cells.ctypes.data, nb * 256, C.byref(ncells), C.byref(ok))
    if rc != 0:
        raise SegsortError("cdb_debug_segsort", rc)
    return entries[:n], flags[:n], cells[:ncells.value].copy(), bool(ok.value)


class CdbDebugSweepArgs(C.Structure):
    _fields_ = [("text", C.c_void_p), ("n", C.c_uint64), ("doc_start", C.c_void_p), ("ndocs", C.c_uint64), ("bits", C.c_int),
                ("padded", C.c_int), ("codeslot", C.c_void_p), ("slotmap", C.c_void_p), ("src_col", C.c_void_p),
                ("slot_start", C.c_void_p), ("vl", C.c_int), ("base", C.c_uint32), ("nsym", C.c_int), ("part_m", C.c_uint32),
                ("vl_sym", C.c_void_p), ("vl_dec", C.c_void_p), ("key_bits", C.c_int), ("end_len", C.c_int), ("carry", C.c_int),
                ("carry_shift", C.c_int), ("rec_low_bits", C.c_int), ("aux_bytes", C.c_int), ("g0", C.c_uint32), ("g1", C.c_uint32),
                ("gstart", C.c_uint64), ("gelems", C.c_uint64), ("seg_begin", C.c_void_p), ("seg_end", C.c_void_p),
                ("seg_tile_begin", C.c_void_p), ("lead", C.c_int), ("npass", C.c_int), ("tile_counts", C.c_void_p),
                ("out_k", C.c_void_p), ("out_v", C.c_void_p), ("out_w", C.c_void_p), ("out_hist", C.c_void_p),
                ("out_tile_base", C.c_void_p), ("out_tile_doc", C.c_void_p), ("out_guard_ok", C.POINTER(C.c_int))]


class SweepError(RuntimeError):
    """A sweep hook failed; `status` is the CDB_E_* code of the error thrown inside the library."""

    def __init__(self, what, status):
        super().__init__(f"{what} failed ({status})")
        self.status = status


def debug_sweep_records(text, doc_start, bits, padded, codeslot, slotmap, src_col, slot_start, rec_low_bits, aux_bytes, g0, g1, gstart,
                        gelems, seg_begin, seg_end, seg_tile_begin, lead, npass, tile_counts, dense=None, vl=None, device=-1):
    """One bucket group through the build's record sweep and histogram sweep (cdb_debug_sweep_records).  dense = (base, nsym,
    part_m) or vl = (vl_sym[256], vl_dec[128], key_bits, end_len, carry, carry_shift).  Returns a dict: k, v (uint32[gelems]), w
    (uint8 / uint16 / uint32 [gelems]), hist (uint64[g1 - g0, 8, 256]), tile_base (uint64[tiles, 256]), tile_doc (uint64[tiles + 1]),
    guard_ok."""
    if (dense is None) == (vl is None):
        raise ValueError("exactly one of dense / vl")
    lib = load_library()
    lib.cdb_debug_sweep_records.argtypes = [C.c_int, C.POINTER(CdbDebugSweepArgs)]
    keep = []

    def arr(x, dtype, shape=None):
        x = np.ascontiguousarray(x, dtype=dtype)
        if shape is not None and x.shape != shape:
            raise ValueError(f"array of shape {x.shape}, expected {shape}")
        keep.append(x)
        return x.ctypes.data

    text = np.ascontiguousarray(text, dtype=np.uint8)
    n = int(text.shape[0])
    doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
    tiles, nseg = (n + 8191) // 8192, int(g1) - int(g0)
    a = CdbDebugSweepArgs()
    a.text, a.n = arr(text, np.uint8), n
    a.doc_start, a.ndocs = arr(doc_start, np.uint64), doc_start.shape[0] - 1
    a.bits, a.padded = int(bits), int(padded)
    a.codeslot = arr(codeslot, np.uint16, (256,))
    a.slotmap = arr(slotmap, np.uint8, (257,))
    a.src_col = arr(src_col, np.uint16, (256,))
    a.slot_start = arr(slot_start, np.uint64, (256,))
    if dense is not None:
        a.vl, (a.base, a.nsym, a.part_m) = 0, (int(x) for x in dense)
    else:
        a.vl = 1
        a.vl_sym, a.vl_dec = arr(vl[0], np.uint16, (256,)), arr(vl[1], np.uint16, (128,))
        a.key_bits, a.end_len, a.carry, a.carry_shift = (int(x) for x in vl[2:])
    a.rec_low_bits, a.aux_bytes = int(rec_low_bits), int(aux_bytes)
    a.g0, a.g1, a.gstart, a.gelems = int(g0), int(g1), int(gstart), int(gelems)
    a.seg_begin, a.seg_end = arr(seg_begin, np.uint64, (nseg,)), arr(seg_end, np.uint64, (nseg,))
    a.seg_tile_begin = arr(seg_tile_begin, np.uint32, (nseg,))
    a.lead, a.npass = int(lead), int(npass)
    a.tile_counts = arr(tile_counts, np.uint32, (tiles, 256))
    wtype = {1: np.uint8, 2: np.uint16, 4: np.uint32}[int(aux_bytes)]
    out = {"k": np.zeros(int(gelems), np.uint32), "v": np.zeros(int(gelems), np.uint32), "w": np.zeros(int(gelems), wtype),
           "hist": np.zeros((max(nseg, 0), 8, 256), np.uint64), "tile_base": np.zeros((tiles, 256), np.uint64),
           "tile_doc": np.zeros(tiles + 1, np.uint64)}
    a.out_k, a.out_v, a.out_w, a.out_hist = (out[x].ctypes.data for x in ("k", "v", "w", "hist"))
    a.out_tile_base, a.out_tile_doc = out["tile_base"].ctypes.data, out["tile_doc"].ctypes.data
    ok = C.c_int(0)
    a.out_guard_ok = C.pointer(ok)
    rc = lib.cdb_debug_sweep_records(device, C.byref(a))
    if rc != 0:
        raise SweepError("cdb_debug_sweep_records", rc)
    out["guard_ok"] = bool(ok.value)
    return out


def debug_vl_tables(counts, slot_of_code):
    """The variable-length code the build would choose (cdb_debug_vl_tables; host only).  counts[0] = documents, counts[c] =
    occurrences of symbol code c; slot_of_code[c] = bucket slot of code c.  Returns (sym uint16[256], dec uint16[128], end_len)."""
    lib = load_library()
    lib.cdb_debug_vl_tables.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    sigma = counts.shape[0] - 1
    slot_of_code = np.ascontiguousarray(slot_of_code, dtype=np.uint8)
    if slot_of_code.shape != (sigma + 1,):
        raise ValueError("slot_of_code: one entry per symbol code, END included")
    sym, dec, end_len = np.zeros(256, np.uint16), np.zeros(128, np.uint16), C.c_int(0)
    rc = lib.cdb_debug_vl_tables(counts.ctypes.data, sigma, slot_of_code.ctypes.data, sym.ctypes.data, dec.ctypes.data, C.byref(end_len))
    if rc != 0:
        raise SweepError("cdb_debug_vl_tables", rc)
    return sym, dec, end_len.value


def layout_rule(ndocs, longest):
    """(bits, mask, width, off_bits) of the reference's entry layout, or RuntimeError with the reference's message."""
    lib = load_library()
    lib.cdb_layout_rule.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    bits, mask, width, off = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(256)
    if lib.cdb_layout_rule(ndocs, longest, C.byref(bits), C.byref(mask), C.byref(width), C.byref(off), err, 256) != 0:
        raise RuntimeError(err.value.decode())
    return bits.value, mask.value, width.value, off.value


def raw_record_find_string(record: bytes, key: bytes):
    """(id, value) of the string stored under `key` in one CoffeeDB raw record, or None."""
    lib = load_library()
    id_, val, n = C.c_int64(0), C.c_char_p(), C.c_size_t(0)
    buf = C.create_string_buffer(record, len(record))
    r = lib.cdb_raw_record_find_string(buf, len(record), key, C.byref(id_), C.byref(val), C.byref(n))
    if r < 0:
        raise ValueError("malformed raw record")
    if r == 0:
        return None
    off = C.cast(val, C.c_void_p).value - C.addressof(buf)
    return id_.value, record[off:off + n.value]
