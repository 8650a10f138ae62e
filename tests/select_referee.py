"""The referee of `select` (tests/test_select_referee.py, tests/test_gpu_select.py): the tail of the reference's `query` operation
restated over a plain model — objects as {id: {field: value}} (str field names; values bytes / int / float / bool) and a ranked row
list [(id, correlation)].

  render()      ac_automaton::render, database.cpp:58-90: at every end position the longest keyword that ends there joins the span
                list by the pop / extend / append rule; `left` goes before a span's first byte, `right` behind its last.
  Renderer      database.cpp:139-165: one automaton per constraint key; a string value of such a key is rendered, every other value
                goes through as it is.
  select()      database.cpp:394-441: fields in `keys` order (absent fields skipped) or, with no keys, all fields in std::map order
                (ascending by the key's bytes); rendered when `constraints` is not empty; "$correlation" appended LAST when it is
                not 0 and keys is empty or names it; a row whose object comes out empty is dropped.
  query_rows()  interface.cpp:144-146 and 228-241: the ranking and the span.
  TIES.  The reference ranks with std::sort and a comparator that looks at the counts only (interface.cpp:144-146), so rows of equal
  count come in no defined order there.  The project's rule — descending count as signed int64, ties ascending id — is what
  rowset_referee.ranking computes, and what every comparison here uses.

The device-side entry points answer per field, not per object; field_text() / field_values() restate one field of a page that way."""
import functools

from . import rowset_referee

KEY_CORRELATION = "$correlation"


def render(text, keywords, left, right):
    """database.cpp:58-90.  Returns the rendered bytes."""
    return _render(bytes(text), tuple(keywords), bytes(left), bytes(right))


@functools.lru_cache(maxsize=None)   # (a page of a test asks for the same documents again and again)
def _render(text, keywords, left, right):
    lens = sorted({len(k) for k in keywords}, reverse=True)
    kws = set(keywords)
    spans = []
    for i in range(len(text)):
        length = 0   # length[node]: the longest keyword that ends at i
        for m in lens:
            if m <= i + 1 and text[i + 1 - m:i + 1] in kws:
                length = m
                break
        if length:
            begin = i - length + 1
            while spans and begin <= spans[-1][0]:
                spans.pop()
            if spans and begin <= spans[-1][1]:
                spans[-1][1] = i
            else:
                spans.append([begin, i])
    ret, it = bytearray(), 0
    for i in range(len(text)):
        if it < len(spans) and i == spans[it][0]:
            ret += left
        ret.append(text[i])
        if it < len(spans) and i == spans[it][1]:
            ret += right
            it += 1
    return bytes(ret)


class Renderer:
    """database.cpp:139-165.  constraints: [(key, [keyword bytes, ...]), ...]"""

    def __init__(self, constraints, left, right):
        self.automatons = {key: list(kws) for key, kws in constraints}
        self.left, self.right = left, right

    def __call__(self, key, value):
        if isinstance(value, bytes) and key in self.automatons:
            return render(value, self.automatons[key], self.left, self.right)
        return value


def select(data, results, keys, constraints, left=b"", right=b""):
    """database.cpp:394-441.  Returns [[(field, value), ...], ...]"""
    transformer = Renderer(constraints, left, right)
    flag = not keys or KEY_CORRELATION in keys
    ret = []
    for id_, correlation in results:
        obj = data.get(id_, {})
        names = [k for k in keys if k in obj] if keys else sorted(obj, key=lambda k: k.encode())
        if constraints:
            out = [(k, transformer(k, obj[k])) for k in names]
        else:
            out = [(k, obj[k]) for k in names]
        if correlation and flag:
            out.append((KEY_CORRELATION, correlation))
        if out:
            ret.append(out)
    return ret


def query_rows(rows, span=None):
    """rows [(id, count)] ascending by id (what filter() leaves) -> ranked (ties ascending id), then `span` = (first, last)"""
    ri, rc = rowset_referee.ranking([r[0] for r in rows], [r[1] for r in rows])
    ranked = list(zip(ri.tolist(), rc.tolist()))
    if span is not None:
        first, last = span
        ranked = [] if first >= len(ranked) else ranked[first:min(last, len(ranked))]
    return ranked


def query(data, rows, keys=(), constraints=(), highlight=None, span=None):
    """interface.cpp:181-248 behind filter(): without `highlight` the constraints do not reach select() (:225-227)"""
    left, right = highlight if highlight is not None else (b"", b"")
    return select(data, query_rows(rows, span), list(keys), list(constraints) if highlight is not None else [], left, right)


# ---- one field of a page, as the device answers it ---------------------------------------------------------------------------
def field_text(store, page, keywords, left=b"", right=b""):
    """store: {id: document bytes}.  Returns (texts, found, missing): a row the field does not hold is b"" and not found."""
    texts, found, cache = [], [], {}
    for i in page:
        i = int(i)
        if i in store and i not in cache:
            cache[i] = render(store[i], keywords, left, right) if keywords else store[i]
        texts.append(cache.get(i, b""))
        found.append(i in store)
    return texts, found, found.count(False)


def field_values(store, page):
    """store: {id: value}.  Returns (values, found, missing): a row the field does not hold is 0 and not found."""
    values = [store.get(int(i), 0) for i in page]
    found = [int(i) in store for i in page]
    return values, found, found.count(False)
