"""The numpy referee of a row set's page (tests/test_gpu_rowset.py, tests/test_rowset_cpu.py): rows ascending by id are ranked by
descending count compared as signed int64, ties ascending id — key = ~(count ^ 2^63) as an unsigned number, stable argsort, slice."""
import numpy as np

SIGN = np.uint64(1 << 63)


def page_key(counts):
    return ~(np.ascontiguousarray(counts, dtype=np.int64).view(np.uint64) ^ SIGN)


def ranking(ids, counts):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    order = np.argsort(page_key(counts), kind="stable")
    return ids[order], counts[order]


def page(ids, counts, first, last):
    """rows [first, min(last, m)) of the ranking; no rows when first >= min(last, m)"""
    ri, rc = ranking(ids, counts)
    k = min(int(last), len(ri))
    if first >= k:
        return ri[:0], rc[:0]
    return ri[first:k], rc[first:k]


def differing_bytes(counts):
    """bytes of the key in which the rows differ: what a select has to visit"""
    keys = page_key(counts)
    if len(keys) == 0:
        return 0
    diff = int(np.bitwise_or.reduce(keys ^ keys[0]))
    return sum(1 for b in range(8) if (diff >> (8 * b)) & 0xFF)
