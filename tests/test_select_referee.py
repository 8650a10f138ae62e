"""The referee of select (tests/select_referee.py) pinned to the answers the reference publishes in its README (README.md:80-110)
and to the rules of database.cpp:394-441 on hand-made cases.  No GPU, no library."""
from . import select_referee as S

# the two objects of README.md:22-46; ids are insertion timestamps, so the first object has the smaller one
DATA = {
    1001: {"number": 123, "name": b"sunkafei", "secret": b"3010103"},
    1002: {"number": 234, "name": b"yulemao", "position": 1.7724, "secret": b"301022"},
}
# filter() for "secret": "010" (README.md:80-92): "3010103" holds 010 twice (overlapping), "301022" once; the number key adds 0
ROWS = [(1001, 2), (1002, 1)]


def test_readme_highlight_fields_span():
    """README.md:93-110"""
    got = S.query(DATA, ROWS, keys=["name", "secret"], constraints=[("secret", [b"010"]), ("number", [b"[0,900]"])],
                  highlight=(b"<b>", b"</b>"), span=(0, 1))
    assert got == [[("name", b"sunkafei"), ("secret", b"3<b>01010</b>3")]]


def test_readme_correlation_appended_last():
    """README.md:80-92: $correlation 2 and 1; select() appends it behind the object's own fields (database.cpp:433-435), which come in
    std::map order"""
    got = S.query(DATA, ROWS, constraints=[("secret", [b"010"])])
    assert got == [
        [("name", b"sunkafei"), ("number", 123), ("secret", b"3010103"), ("$correlation", 2)],
        [("name", b"yulemao"), ("number", 234), ("position", 1.7724), ("secret", b"301022"), ("$correlation", 1)],
    ]


def test_readme_fields_without_correlation():
    """README.md:66-79: numeric constraint only, correlation 0 -> nothing appended"""
    assert S.query(DATA, [(1001, 0), (1002, 0)], keys=["name"], constraints=[("number", [b"[100,900]"])]) == \
        [[("name", b"sunkafei")], [("name", b"yulemao")]]


def test_without_highlight_nothing_is_rendered():
    """interface.cpp:225-227 clears the constraints"""
    got = S.query(DATA, ROWS, keys=["secret"], constraints=[("secret", [b"010"])])
    assert got == [[("secret", b"3010103")], [("secret", b"301022")]]


def test_key_order_and_absent_fields():
    got = S.select(DATA, [(1002, 0), (1001, 0)], ["secret", "position", "nowhere", "name"], [])
    assert got == [[("secret", b"301022"), ("position", 1.7724), ("name", b"yulemao")], [("secret", b"3010103"), ("name", b"sunkafei")]]
    # std::map order is by bytes: upper case before lower case, a prefix before the longer key
    data = {5: {"b": 1, "B": 2, "ab": 3, "a": 4}}
    assert [k for k, _ in S.select(data, [(5, 0)], [], [])[0]] == ["B", "a", "ab", "b"]


def test_empty_objects_are_dropped():
    rows = [(1001, 0), (1002, 0), (7, 0)]
    assert S.select(DATA, rows, ["position"], []) == [[("position", 1.7724)]]            # 1001 lacks it, 7 is no object at all
    assert S.select(DATA, [(7, 3)], ["position"], []) == []                             # keys do not name $correlation
    assert S.select(DATA, [(7, 3)], ["position", "$correlation"], []) == [[("$correlation", 3)]]   # ... now the object is not empty
    assert S.select(DATA, [(7, 3)], [], []) == [[("$correlation", 3)]]


def test_only_constrained_string_fields_are_rendered():
    got = S.select(DATA, [(1001, 1)], [], [("secret", [b"01"]), ("number", [b"123"])], b"[", b"]")
    assert got == [[("name", b"sunkafei"), ("number", 123), ("secret", b"3[01][01]03"), ("$correlation", 1)]]


def test_span_and_ties():
    rows = [(1, 5), (2, 9), (3, 5), (4, -1), (5, 9)]
    assert S.query_rows(rows) == [(2, 9), (5, 9), (1, 5), (3, 5), (4, -1)]    # ties ascending id; counts compared as signed
    assert S.query_rows(rows, (1, 3)) == [(5, 9), (1, 5)]
    assert S.query_rows(rows, (5, 9)) == [] and S.query_rows(rows, (4, 99)) == [(4, -1)]


def test_field_views():
    texts, found, missing = S.field_text({1: b"3010103", 3: b""}, [3, 2, 1, 1], [b"010"], b"<b>", b"</b>")
    assert texts == [b"", b"", b"3<b>01010</b>3", b"3<b>01010</b>3"] and found == [True, False, True, True] and missing == 1
    assert S.field_text({1: b"3010103"}, [1], [])[0] == [b"3010103"]
    assert S.field_values({1: 10, 2: -3}, [2, 9, 1]) == ([-3, 0, 10], [True, False, True], 1)
