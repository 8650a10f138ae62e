"""What cdb_insert_objects (coffeedb_amd/csrc/insert.hip) does to a database, stated over a dict model {field: {id: value}} — the
referee of tests/test_gpu_insert.py, pinned on the CPU by tests/test_insert_referee.py — and the named cases both files walk through.

A batch is (ids, [(field, rows or None, values), ...]): field k receives the pairs (ids[rows[j]], values[j]); rows None = every object.
insert() returns the new dicts, or a Refusal by the rules of include/coffeedb_gpu.h, checked in the library's order:

    rows    a field's rows do not ascend strictly, or one is >= len(ids)          (field = that field's index in the batch)
    empty   an object that no field lists                                        (id = the object's INDEX in the batch)
    twice   an id stands twice in the batch                                      (id = the smallest such id)
    held    an id of the batch is held by a field of the call, listed or not     (id = the smallest such id as a signed number,
                                                                                  field = the first field of the call that holds it)

The rule is stated twice, once in Python integers (insert) and once in numpy as the device states it — keys id ^ 2^63 compared
unsigned, a sort and a head count for `twice`, a lower bound per (id, field) and a minimum per field for `held` (insert_np)."""
from collections import namedtuple

import numpy as np

Refusal = namedtuple("Refusal", "kind id field")
SIGN = np.uint64(1 << 63)
LO, HI = -(1 << 63), (1 << 63) - 1


def _rows_of(rows, nobjects):
    return list(range(nobjects)) if rows is None else [int(r) for r in rows]


def insert(db, ids, fields):
    """db: {name: {id: value}} (left unchanged); fields: [(name, rows or None, values)].  Python integers only."""
    ids = [int(x) for x in ids]
    n = len(ids)
    listed = [False] * n
    for k, (name, rows, values) in enumerate(fields):
        r = _rows_of(rows, n)
        if any(x >= n for x in r) or any(b <= a for a, b in zip(r, r[1:])):
            return Refusal("rows", None, k)
        assert len(values) == len(r), "a field's values and rows differ in length"
        for x in r:
            listed[x] = True
    for i in range(n):
        if not listed[i]:
            return Refusal("empty", i, None)
    seen, twice = set(), []
    for x in ids:
        if x in seen:
            twice.append(x)
        seen.add(x)
    if twice:
        return Refusal("twice", min(twice), None)
    held = [x for x in ids if any(x in db[name] for name, _, _ in fields)]
    if held:
        x = min(held)
        return Refusal("held", x, next(k for k, (name, _, _) in enumerate(fields) if x in db[name]))
    out = {name: dict(rows) for name, rows in db.items()}
    for name, rows, values in fields:
        for j, x in enumerate(_rows_of(rows, n)):
            out[name][ids[x]] = values[j]
    return out


def _id_of_key(key):
    u = int(key) ^ (1 << 63)
    return u - (1 << 64) if u >= (1 << 63) else u


def check_ids_np(lists, ids):
    """The device's id check: lists = the ascending int64 ids every field of the call holds.  None, or Refusal twice / held."""
    ids = np.asarray(ids, dtype=np.int64)
    key = np.sort(ids.view(np.uint64) ^ SIGN)
    heads = 1 + int((key[1:] != key[:-1]).sum()) if len(key) else 0
    if heads != len(key):
        rep = key[1:][key[1:] == key[:-1]].min()
        return Refusal("twice", _id_of_key(rep), None)
    hits, least = [], []
    for l in lists:
        l = np.asarray(l, dtype=np.int64)
        a = np.searchsorted(l, ids, side="left")
        hit = (a < len(l)) & (l[np.minimum(a, max(len(l) - 1, 0))] == ids) if len(l) else np.zeros(len(ids), dtype=bool)
        hits.append(int(hit.sum()))
        least.append((ids[hit].view(np.uint64) ^ SIGN).min() if hit.any() else np.uint64(0xFFFFFFFFFFFFFFFF))
    who, best = None, np.uint64(0xFFFFFFFFFFFFFFFF)
    for k in range(len(lists)):
        if hits[k] and (who is None or least[k] < best):   # (the key of INT64_MAX is all ones)
            who, best = k, least[k]
    if who is None:
        return None
    return Refusal("held", _id_of_key(best), who)


def insert_np(db, ids, fields):
    """insert() with the id check in the device's terms; the host-side rules (rows, empty) as the library's loop states them."""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    listed = np.zeros(n, dtype=bool)
    for k, (name, rows, values) in enumerate(fields):
        if rows is None:
            listed[:] = True
            continue
        r = np.asarray(rows, dtype=np.uint64)
        if (r >= n).any() or (np.diff(r.astype(object)) <= 0).any():
            return Refusal("rows", None, k)
        listed[r.astype(np.int64)] = True
    if not listed.all():
        return Refusal("empty", int(np.argmin(listed)), None)
    lists = [np.sort(np.fromiter(db[name].keys(), dtype=np.int64, count=len(db[name]))) for name, _, _ in fields]
    refusal = check_ids_np(lists, ids)
    if refusal is not None:
        return refusal
    out = {name: dict(rows) for name, rows in db.items()}
    for name, rows, values in fields:
        r = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
        out[name].update(zip(ids[r].tolist(), list(values)))
    return out


# ---- the named cases of the id check ------------------------------------------------------------------------------------------
# name -> (lists: the ids every field of the call holds before it, in the caller's order; ids: the batch; want: None or a Refusal;
#          edge: what test_insert_referee.py asserts the case reaches, as a dict of facts)
def _held(n, base=10**6, step=3):
    return base + step * np.arange(n, dtype=np.int64)


def _batch(n, base=2000):
    """n fresh ids (base .. base + n - 1: none that a list of the cases holds), shuffled so that the batch does not ascend"""
    rng = np.random.default_rng(n + 17)
    return (base + rng.permutation(n)).astype(np.int64)


def fresh_cases():
    out = {}
    # batch sizes around the wave and the workgroup, all ids fresh; field lists of n = 0, 1, 2 and a non-power of two
    for n in (1, 63, 64, 65, 255, 256, 257):
        out[f"fresh_{n}"] = ([_held(0), _held(1), _held(2), _held(11)], _batch(n), None, {"nobjects": n})

    def one(name, n, lane, lists, field, offender, **edge):
        ids = _batch(n)
        ids[lane] = offender
        out[name] = (lists, ids, Refusal("held", int(offender), field), dict(edge, lane=lane, nobjects=n))

    L = _held(11)
    one("first_lane", 300, 0, [L], 0, L[4])
    one("lane_63", 300, 63, [L], 0, L[4])
    one("lane_64", 300, 64, [L], 0, L[4])
    one("last_lane_of_a_ragged_block", 300, 299, [L], 0, L[4], ragged=True)
    one("first_entry_of_the_list", 100, 50, [L], 0, L[0], entry=0)
    one("last_entry_of_the_list", 100, 50, [L], 0, L[-1], entry=10)
    for name, x in (("int64_min", LO), ("minus_one", -1), ("zero", 0), ("int64_max", HI)):
        one("offender_" + name, 70, 69, [np.array(sorted([LO, -1, 0, HI, 5, -7]), dtype=np.int64)], 0, x)
    one("held_by_two_fields", 100, 10, [_held(5, base=500000), L, L.copy()], 1, L[3], holders=(1, 2))
    one("only_in_the_last_list", 260, 258, [_held(3), _held(0), _held(2), np.array([-50, 7000], dtype=np.int64)], 3, -50, last_y=True)
    one("list_of_one", 65, 64, [_held(0), np.array([-9], dtype=np.int64)], 1, -9)
    # two offenders: the smaller SIGNED id is named, though its key-less bit pattern is the larger
    ids = _batch(130)
    ids[5], ids[129] = 4, -3
    out["two_offenders_smaller_signed_id"] = ([np.array([-3, 4], dtype=np.int64)], ids, Refusal("held", -3, 0), {"offenders": (-3, 4)})
    # ... in two fields: field 1 holds the smaller one, so field 1 is named although field 0 holds an offender too
    out["two_offenders_in_two_fields"] = ([np.array([4], dtype=np.int64), np.array([-3], dtype=np.int64)], ids.copy(),
                                          Refusal("held", -3, 1), {"offenders": (-3, 4)})
    # batch duplicates
    ids = _batch(300)
    ids[41] = ids[40]
    out["twice_adjacent"] = ([L], ids, Refusal("twice", int(ids[40]), None), {"distance": 1})
    ids = _batch(300)
    ids[260] = ids[4]
    out["twice_at_distance_256"] = ([L], ids, Refusal("twice", int(ids[4]), None), {"distance": 256})
    ids = _batch(64)
    ids[0], ids[1], ids[2], ids[3] = 1000, LO + 1000, -1, HI   # pairs that differ in the sign bit only
    out["sign_bit_is_no_duplicate"] = ([L], ids, None, {"sign_pairs": ((1000, LO + 1000), (-1, HI))})
    ids = _batch(10)
    ids[7] = ids[1] = -2
    ids[9] = ids[3] = -1
    out["twice_two_ids_smaller_named"] = ([L], ids, Refusal("twice", -2, None), {})
    # a duplicate that a field also holds: the batch check comes first
    ids = _batch(10)
    ids[2] = ids[8] = L[1]
    out["twice_beats_held"] = ([L], ids, Refusal("twice", int(L[1]), None), {})
    return out
