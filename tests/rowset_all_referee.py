"""What cdb_rowset_all returns, stated in numpy: the union of the fields' id lists ascending as signed int64, each id once, every
count 0 — and a page of it, which is a plain slice because all counts are equal and ties ascend by id.  Pinned against Python's
own sorted(set(...)) by tests/test_rowset_maintain_cpu.py."""
import numpy as np


def union(lists):
    lists = [np.asarray(l, dtype=np.int64) for l in lists]
    if not lists:
        return np.empty(0, dtype=np.int64)
    return np.unique(np.concatenate(lists))


def page(ids, first, last):
    ids = np.asarray(ids, dtype=np.int64)[first:min(last, len(ids))] if first < min(last, len(ids)) else np.empty(0, dtype=np.int64)
    return ids, np.zeros(len(ids), dtype=np.int64)
