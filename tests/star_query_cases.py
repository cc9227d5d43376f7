"""Case builders and the expectation of the star query tests (hj.h "Star
query").  Pure numpy: no GPU and no library call, so test_star_query_cases.py
checks the expectation against a nested loop and the shared cases' coverage
conditions on a CPU-only machine.

A query over star_cases' dict(wide, n, dims) is a dict(where, val, expr,
gshift, gbase, fact_group): where a list of (column, lo, hi, "in" | "out"),
expr None or (op, column) with op in "add" | "sub" | "mul", fact_group a list
of (column, shift, base); every column in the case's dtype.  expect() restricts
star_cases.Expect to the rows the predicates admit -- built over a case whose
fact columns are cut to those rows, the row ids mapped back -- then applies the
extended key formula in uint64 arithmetic and aggregate_cases.expect."""
import functools

import numpy as np

import aggregate_cases as GC
import star_agg_cases as AG
import star_cases as SC

I64_MIN, I64_MAX = GC.I64_MIN, GC.I64_MAX
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
TILE = SC.TILE
COLS = GC.COLS
M64 = (1 << 64) - 1


def dtype_of(wide):
    return np.int64 if wide else np.int32


def extremes(wide):
    return (I64_MIN, I64_MAX) if wide else (I32_MIN, I32_MAX)


def query(where=(), val=None, expr=None, gshift=(), gbase=None, fact_group=()):
    return dict(where=[tuple(w) if len(w) == 4 else tuple(w) + ("in",) for w in where], val=val, expr=expr,
                gshift=list(gshift), gbase=None if gbase is None else list(gbase), fact_group=list(fact_group))


# ------------------------------------------------------------------ the expectation
def admits(c, where):
    """Per fact row: every predicate admits it (signed int64 compares of the sign-extended column)."""
    ok = np.ones(c["n"], bool)
    for col, lo, hi, kind in where:
        assert kind in ("in", "out") and len(col) == c["n"] and I64_MIN <= lo <= I64_MAX and I64_MIN <= hi <= I64_MAX
        x = np.asarray(col).astype(np.int64)
        inside = (x >= np.int64(lo)) & (x <= np.int64(hi))
        ok &= inside if kind == "in" else ~inside
    return ok


def restrict(c, ok):
    """Case c with its fact columns cut to the rows in ok, and those rows' ids."""
    ids = np.flatnonzero(ok).astype(np.int64)
    return dict(wide=c["wide"], n=len(ids), dims=[dict(d, sk=d["sk"][ids]) for d in c["dims"]]), ids


class Expect:
    """star_cases.Expect over the admitted rows: rows are positions in the uncut
    fact table, pays per dimension the payloads of those rows, ok the
    predicates' verdict per fact row, keep the qualifying rows' mask."""

    def __init__(self, c, where):
        self.ok = admits(c, where)
        cut, ids = restrict(c, self.ok)
        e = SC.Expect(cut)
        self.rows = ids[e.rows]
        self.pays = e.pays
        self.m = e.m
        self.keep = np.zeros(c["n"], bool)
        self.keep[self.rows] = True


def value(c, val, expr):
    """v(j) of every fact row as int64 words: sign-extended, the operation in uint64 arithmetic."""
    a = np.zeros(c["n"], np.int64) if val is None else np.asarray(val).astype(np.int64)
    if expr is None:
        return a
    op, vb = expr
    a, b = a.view(np.uint64), np.asarray(vb).astype(np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        v = {"add": lambda: a + b, "sub": lambda: a - b, "mul": lambda: a * b}[op]()
    return v.view(np.int64)


def group_keys(e, q):
    """g(j) of the qualifying rows: the star aggregate's formula plus the fact fields."""
    g = AG.group_keys(e, q["gshift"], q["gbase"]).view(np.uint64).copy()
    for col, shift, base in q["fact_group"]:
        assert 0 <= shift <= 63
        x = np.asarray(col).astype(np.int64)[e.rows].view(np.uint64)
        with np.errstate(over="ignore"):
            g += (x - np.uint64(base & M64)) << np.uint64(shift)
    return g.view(np.int64)


def expect(c, q, e=None):
    """The five expected columns as int64 arrays sorted by key."""
    e = Expect(c, q["where"]) if e is None else e
    return GC.expect(group_keys(e, q), value(c, q["val"], q["expr"])[e.rows])


def brute(c, q):
    """The same by nested loops over Python integers (tiny inputs)."""
    wrap = lambda s: (s + (1 << 63)) % (1 << 64) - (1 << 63)  # noqa: E731
    acc = {}
    for j in range(c["n"]):
        ok = True
        for col, lo, hi, kind in q["where"]:
            ok &= (lo <= int(col[j]) <= hi) == (kind == "in")
        g = 0
        for d, dm in enumerate(c["dims"]):
            ps = [int(dm["rp"][i]) for i in range(len(dm["rk"])) if int(dm["rk"][i]) == int(dm["sk"][j])]
            if dm["how"] == "inner":
                ok &= len(ps) > 0
            elif dm["how"] == "anti":
                ok &= len(ps) == 0
            if q["gshift"][d] >= 0:
                p = min(ps) if ps else int(dm["null"])
                g += ((p - (q["gbase"][d] if q["gbase"] is not None else 0)) % (1 << 64)) << q["gshift"][d]
        if not ok:
            continue
        for col, shift, base in q["fact_group"]:
            g += ((int(col[j]) - base) % (1 << 64)) << shift
        g = wrap(g % (1 << 64))
        v = 0 if q["val"] is None else int(q["val"][j])
        if q["expr"] is not None:
            b = int(q["expr"][1][j])
            v = wrap({"add": v + b, "sub": v - b, "mul": v * b}[q["expr"][0]])
        a = acc.setdefault(g, [0, 0, v, v])
        a[0] += 1
        a[1] += v
        a[2], a[3] = min(a[2], v), max(a[3], v)
    keys = sorted(acc)
    cols = [keys, [acc[k][0] for k in keys], [wrap(acc[k][1]) for k in keys], [acc[k][2] for k in keys],
            [acc[k][3] for k in keys]]
    return {n: np.array(col, np.int64) for n, col in zip(COLS, cols)}


def groups_per_tile(c, e, q):
    """Distinct group keys among each tile's qualifying rows."""
    g, tile = group_keys(e, q), e.rows // TILE
    return [len(np.unique(g[tile == t])) for t in range(-(-c["n"] // TILE))]


# ------------------------------------------------------------------ builders
def fact_column(c, lo, hi, seed, plant=()):
    """A fact column of the case's dtype, uniform in [lo, hi]; plant: values written at rows 0, 1, ... and at the
    last rows (when the case has room), so that they meet the first and the ragged last tile."""
    n = c["n"]
    col = np.random.default_rng(1000 + seed).integers(lo, hi, n, dtype=np.int64, endpoint=True)
    for i, v in enumerate(plant):
        if n > 2 * len(plant):
            col[i] = col[n - 1 - i] = v
    return col.astype(dtype_of(c["wide"]))


def layout(c, grouped, fcols):
    """One key over the grouped dimensions' payload fields (star_agg_cases.plan's
    ranges) followed by the fact columns' fields, each as wide as the column's
    observed minimum and maximum need, the first field highest; a 0-bit field
    is left out.  Returns (gshift, gbase, [(col, shift, base), ...])."""
    nd = len(c["dims"])
    _, lo = AG.plan(c, grouped) if nd else ([], [])
    bits = [0] * nd
    for i in grouped:
        d = c["dims"][i]
        vals = [int(v) for v in (d["rp"].min(), d["rp"].max())] if len(d["rp"]) else []
        if d["how"] == "left":
            vals.append(int(d["null"]))
        bits[i] = (max(vals) - min(vals)).bit_length() if vals else 0
    fl = [int(f.min()) if len(f) else 0 for f in fcols]
    fb = [(int(f.max()) - int(f.min())).bit_length() if len(f) else 0 for f in fcols]
    assert sum(bits) + sum(fb) <= 64
    at = sum(bits) + sum(fb)
    gshift = [-1] * nd
    for i in range(nd):
        at -= bits[i]
        if bits[i]:
            gshift[i] = at
    fg = []
    for f, l, b in zip(fcols, fl, fb):
        at -= b
        if b:
            fg.append((f, at, l))
    assert at == 0
    return gshift, lo, fg


# ------------------------------------------------------------------ the shared cases
@functools.lru_cache(maxsize=None)
def sizes_case(wide):
    """Two dimensions (inner, left), one IN predicate at about one half, one
    7-value fact group and a MUL operand over 2049 rows; sizes_at cuts it."""
    c = SC.small_case(wide, 2049, hows=("inner", "left"), seed=20, p=(0.6, 0.5))
    return c, dict(pred=fact_column(c, 0, 99, 1), fg=fact_column(c, -3, 3, 2), val=AG.values(c, 7), vb=AG.values(c, 8))


def sizes_at(wide, n):
    full, f = sizes_case(wide)
    c = dict(wide=wide, n=n, dims=[dict(d, sk=d["sk"][:n]) for d in full["dims"]])
    gshift, gbase, fg = layout(full, (0, 1), [f["fg"]])
    fg = [(col[:n], s, b) for col, s, b in fg]
    return c, query([(f["pred"][:n], 0, 49, "in")], f["val"][:n], ("mul", f["vb"][:n]), gshift, gbase, fg)


EDGE_N = 2 * TILE + 77


@functools.lru_cache(maxsize=None)
def edge_case(wide):
    """2 * TILE + 77 rows over (inner, left), both grouped, with a plain
    predicate column in [0, 99] and one holding both extremes of its dtype."""
    c = SC.small_case(wide, EDGE_N, hows=("inner", "left"), seed=21, p=(0.6, 0.5))
    lo, hi = extremes(wide)
    planted = [0, 1, 2, 3, EDGE_N - 1, EDGE_N - 2, EDGE_N - 3, EDGE_N - 4]
    c["dims"][0]["sk"][planted] = c["dims"][0]["rk"][:len(planted)]      # the extremes' rows pass the inner dimension
    ext = fact_column(c, -50, 50, 4, plant=(lo, hi, lo + 1, hi - 1))
    cols = dict(p=fact_column(c, 0, 99, 3), ext=ext, q=fact_column(c, -1000, 1000, 5), r=fact_column(c, 0, 9, 6))
    return c, cols


def edge_predicates(wide):
    """name -> (where, edge): edge is None for an ordinary predicate (0 <
    admitted < n is asserted), "all" / "none" for one that admits every / no row."""
    _, f = edge_case(wide)
    lo, hi = extremes(wide)
    out = {
        "in": ([(f["p"], 10, 59, "in")], None),
        "out": ([(f["p"], 10, 59, "out")], None),
        "lo == hi": ([(f["p"], 42, 42, "in")], None),
        "lo == hi out": ([(f["p"], 42, 42, "out")], None),
        "lo > hi in": ([(f["p"], 60, 10, "in")], "none"),
        "lo > hi out": ([(f["p"], 60, 10, "out")], "all"),
        "full in": ([(f["ext"], I64_MIN, I64_MAX, "in")], "all"),
        "full out": ([(f["ext"], I64_MIN, I64_MAX, "out")], "none"),
        "the minimum alone": ([(f["ext"], lo, lo, "in")], None),
        "the maximum alone": ([(f["ext"], hi, hi, "in")], None),
        "both extremes": ([(f["ext"], lo + 1, hi - 1, "out")], None),
        "all but the extremes": ([(f["ext"], lo + 1, hi - 1, "in")], None),
        "up to the maximum": ([(f["ext"], 0, hi, "in")], None),
        "down to the minimum": ([(f["ext"], lo, -1, "in")], None),
        "four at once": ([(f["p"], 5, 94, "in"), (f["ext"], -40, 45, "in"), (f["q"], -100, 100, "out"),
                          (f["r"], 3, 3, "out")], None),
    }
    if not wide:   # bounds outside int32: "always" and "never"
        out["past int32 in"] = ([(f["ext"], I32_MIN - 1, I32_MAX + 1, "in")], "all")
        out["below int32 in"] = ([(f["ext"], I64_MIN, I32_MIN - 1, "in")], "none")
        out["above int32 out"] = ([(f["ext"], I32_MAX + 1, I64_MAX, "out")], "all")
    return out


def edge_query(wide, where, expr="mul"):
    c, f = edge_case(wide)
    gshift, gbase, fg = layout(c, (0, 1), [f["r"]])
    return c, query(where, AG.values(c, 9), None if expr is None else (expr, AG.values(c, 10)), gshift, gbase, fg)


@functools.lru_cache(maxsize=None)
def dead_tile_case(wide):
    """Three full tiles over (inner, inner).  step: 1 outside the middle tile, 0
    inside it (a step function of the row index).  doomed: 1 exactly where some
    dimension fails the row, so a predicate on it admits only rows that then
    all fail."""
    c = SC.small_case(wide, 3 * TILE, hows=("inner", "inner"), seed=22, p=(0.7, 0.8))
    dt = dtype_of(wide)
    step = (np.arange(c["n"]) // TILE != 1).astype(dt)
    doomed = (~SC.Expect(c).keep).astype(dt)
    return c, dict(step=step, doomed=doomed, fg=fact_column(c, 0, 4, 11))


def dead_tile_queries(wide):
    c, f = dead_tile_case(wide)
    gshift, gbase, fg = layout(c, (0, 1), [f["fg"]])
    val, vb = AG.values(c, 12), AG.values(c, 13)
    return c, {"step": query([(f["step"], 1, 1, "in")], val, ("add", vb), gshift, gbase, fg),
               "doomed": query([(f["doomed"], 1, 1, "in")], val, ("add", vb), gshift, gbase, fg)}


@functools.lru_cache(maxsize=None)
def vop_case(wide):
    """TILE + 500 rows over one inner dimension; both value columns hold both extremes, at the same rows."""
    c = SC.small_case(wide, TILE + 500, hows=("inner",), rows=(400,), seed=23, p=(0.8,))
    c["dims"][0]["sk"][[0, 1, c["n"] // 2, c["n"] - 1]] = c["dims"][0]["rk"][0]   # the extremes' rows are kept
    return c, dict(val=AG.values(c, 14), vb=AG.values(c, 14), pred=fact_column(c, 0, 9, 15))


@functools.lru_cache(maxsize=None)
def fact_group_case(wide):
    """2 * TILE + 300 rows over (inner, left) with three fact columns: seven
    values around zero (a negative base), two values (a one-bit field, fshift
    63 its home) and three thousand values (more than 512 groups in a tile from
    the fact column alone)."""
    c = SC.small_case(wide, 2 * TILE + 300, hows=("inner", "left"), seed=24, p=(0.7, 0.5))
    return c, dict(seven=fact_column(c, -3, 3, 16), bit=fact_column(c, 10, 11, 17), many=fact_column(c, 0, 2999, 18),
                   pred=fact_column(c, 0, 9, 19), val=AG.values(c, 20), vb=AG.values(c, 21))


def no_dims(c):
    """Case c without its dimensions: the ndims == 0 shape."""
    return dict(wide=c["wide"], n=c["n"], dims=[])


@functools.lru_cache(maxsize=None)
def strided_query(wide):
    """star_cases.strided_case (1026 tiles, two LDS-resident tables) with one
    predicate admitting seven rows in ten and one five-value fact group, grouped
    by the first dimension too."""
    c = SC.unpadded(SC.strided_case(wide))
    pred, fg = fact_column(c, 0, 9, 30), fact_column(c, 0, 4, 31)
    gshift, gbase, fgl = layout(c, (0,), [fg])
    q = query([(pred, 0, 6, "in")], AG.values(c, 32), ("sub", AG.values(c, 33)), gshift, gbase, fgl)
    e = Expect(c, q["where"])
    return c, q, e, expect(c, q, e)


OVERFLOW_GROUPS = AG.OVERFLOW_GROUPS


@functools.lru_cache(maxsize=None)
def overflow_case(wide):
    """No dimension; a fact column of OVERFLOW_GROUPS distinct values, each in some row."""
    n = 2 * TILE
    c = dict(wide=wide, n=n, dims=[])
    return c, dict(fg=(np.arange(n) % OVERFLOW_GROUPS).astype(dtype_of(wide)), val=AG.values(c, 40))
