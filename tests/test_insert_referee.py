"""tests/insert_referee.py on the CPU: the two statements of cdb_insert_objects' rules (Python integers, numpy in the device's terms)
agree on every named case and on random batches, every named case gives the refusal it was written for, and every named case reaches
the edge it is named for."""
import numpy as np
import pytest

from . import insert_referee as R

CASES = R.fresh_cases()


def _db_and_fields(lists, ids):
    """every field of a case holds its list (value = -id) and is offered every object of the batch"""
    db = {f"f{k}": {int(x): -int(x) for x in l} for k, l in enumerate(lists)}
    fields = [(f"f{k}", None, [7 * int(x) for x in ids]) for k in range(len(lists))]
    return db, fields


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case_gives_its_refusal_in_both_forms(name):
    lists, ids, want, _ = CASES[name]
    assert all((np.diff(np.asarray(l, dtype=object)) > 0).all() for l in lists), "a field's list ascends strictly"
    assert R.check_ids_np(lists, ids) == want
    db, fields = _db_and_fields(lists, ids)
    got, got_np = R.insert(db, ids, fields), R.insert_np(db, ids, fields)
    if want is None:
        assert got == got_np and not isinstance(got, R.Refusal)
        for k, l in enumerate(lists):
            assert sorted(got[f"f{k}"]) == sorted(set(l.tolist()) | set(ids.tolist()))
            assert all(got[f"f{k}"][int(x)] == 7 * int(x) for x in ids)
    else:
        assert got == got_np == want
    assert db == _db_and_fields(lists, ids)[0], "the model is left unchanged"


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case_reaches_its_edge(name):
    lists, ids, want, edge = CASES[name]
    n = len(ids)
    if "nobjects" in edge:
        assert n == edge["nobjects"]
    if "lane" in edge:   # the one offender, where the name says
        held = set(x for l in lists for x in l.tolist())
        assert [i for i, x in enumerate(ids.tolist()) if x in held] == [edge["lane"]] and ids[edge["lane"]] == want.id
    if edge.get("ragged"):
        assert n % 256 and edge["lane"] == n - 1 and n > 256
    if "entry" in edge:
        assert lists[want.field].tolist().index(want.id) == edge["entry"] and edge["entry"] in (0, len(lists[want.field]) - 1)
    if "holders" in edge:
        assert [k for k, l in enumerate(lists) if want.id in l.tolist()] == list(edge["holders"]) and want.field == edge["holders"][0]
    if edge.get("last_y"):
        assert want.field == len(lists) - 1 and len(lists) > 1 and edge["lane"] >= 256
    if "offenders" in edge:
        lo, hi = edge["offenders"]
        assert lo < hi and want.id == lo and {lo, hi} <= set(ids.tolist())
        assert (lo & (2**64 - 1)) > (hi & (2**64 - 1)), "as raw bit patterns the order is the other way round"
    if "distance" in edge:
        i, j = [k for k, x in enumerate(ids.tolist()) if x == want.id]
        assert j - i == edge["distance"]
    if "sign_pairs" in edge:
        for a, b in edge["sign_pairs"]:
            assert (a ^ b) & (2**64 - 1) == 1 << 63 and a in ids.tolist() and b in ids.tolist()
        assert want is None


def test_case_names_cover_the_list():
    sizes = {len(c[1]) for name, c in CASES.items() if name.startswith("fresh_")}
    assert sizes == {1, 63, 64, 65, 255, 256, 257}
    lens = {len(l) for c in CASES.values() for l in c[0]}
    assert {0, 1, 2} <= lens and any(n > 2 and n & (n - 1) for n in lens)
    assert {c[2].id for name, c in CASES.items() if name.startswith("offender_")} == {R.LO, -1, 0, R.HI}


def test_host_side_rules():
    db = {"a": {1: "x"}, "b": {}}
    assert R.insert(db, [5, 6], [("a", [0], ["p"]), ("b", [0], [1])]) == R.insert_np(db, [5, 6], [("a", [0], ["p"]), ("b", [0], [1])]) \
        == R.Refusal("empty", 1, None)
    for rows in ([1, 0], [0, 0], [0, 2]):
        f = [("a", None, ["p", "q"]), ("b", rows, [1, 2])]
        assert R.insert(db, [5, 6], f) == R.insert_np(db, [5, 6], f) == R.Refusal("rows", None, 1)
    f = [("a", [1], ["q"]), ("b", None, [1, 2])]
    want = {"a": {1: "x", 6: "q"}, "b": {5: 1, 6: 2}}
    assert R.insert(db, [5, 6], f) == R.insert_np(db, [5, 6], f) == want
    f = [("a", [], []), ("b", None, [1])]   # a field without rows still takes part in the id check
    assert R.insert(db, [1], f) == R.insert_np(db, [1], f) == R.Refusal("held", 1, 0)
    assert R.insert(db, [], [("a", None, [])]) == R.insert_np(db, [], [("a", None, [])]) == db


def test_both_forms_agree_on_random_batches():
    rng = np.random.default_rng(20261021)
    pool = np.concatenate([rng.integers(-30, 30, 40), [R.LO, R.HI, R.LO + 1, R.HI - 1]]).astype(np.int64)
    kinds = set()
    for _ in range(400):
        nf = int(rng.integers(1, 4))
        db = {f"f{k}": {int(x): 0 for x in rng.choice(pool, int(rng.integers(0, 6)), replace=False)} for k in range(nf)}
        n = int(rng.integers(0, 7))
        ids = rng.choice(pool, n, replace=bool(rng.integers(0, 4) == 0)) if n else np.empty(0, dtype=np.int64)
        fields = []
        for k in range(nf):
            rows = None if rng.integers(0, 2) else np.flatnonzero(rng.integers(0, 2, n)).astype(np.uint64)
            m = n if rows is None else len(rows)
            fields.append((f"f{k}", rows, list(range(m))))
        a, b = R.insert(db, ids, fields), R.insert_np(db, ids, fields)
        assert a == b, (db, ids, fields)
        kinds.add(a.kind if isinstance(a, R.Refusal) else "ok")
    assert kinds == {"ok", "empty", "twice", "held"}
