"""Case builders and the expectation of the star probe tests (hj.h "Star
probe").  Pure numpy: no GPU and no library call, so test_star_cases.py checks
the expectation against a nested loop and the shared cases' coverage conditions
on a CPU-only machine.

A case is dict(wide, n, dims): dims a list of dict(rk, rp, sk, how, null) --
the dimension's build columns (i32: rp the row ids), its key column of the
probe rows, its kind and its LEFT null.  expect() composes
positional_cases.lookup_expect per dimension with the kind rules.  int64
payloads are asof_cases.payloads' (never a multiple of three), NULL and
SENTINEL are multiples of three, i32 payloads are row ids >= 0."""
import functools

import numpy as np

import asof_cases as AC
import positional_cases as PC

I64_MIN = PC.I64_MIN
TILE = PC.TILE
NULL, SENTINEL, EXTRA = PC.NULL, PC.SENTINEL, PC.EXTRA
KINDS = ("inner", "left", "anti")


class Expect:
    """What numpy says the star probe of case c gives: keep (per probe row),
    rows (the positions kept), pays (per dimension the payload column of the
    kept rows, None for anti), cnt (per dimension the partner counts of every
    probe row), m."""

    def __init__(self, c):
        n = c["n"]
        self.keep = np.ones(n, bool)
        self.cnt, full = [], []
        for d in c["dims"]:
            assert d["how"] in KINDS and len(d["sk"]) == n
            p, k = PC.lookup_expect(d["rk"].astype(np.int64), d["rp"], d["sk"].astype(np.int64), d["null"])
            if d["how"] == "inner":
                self.keep &= k > 0
            elif d["how"] == "anti":
                self.keep &= k == 0
            self.cnt.append(k)
            full.append(None if d["how"] == "anti" else p)
        self.rows = np.flatnonzero(self.keep).astype(np.int64)
        self.pays = [None if p is None else p[self.rows] for p in full]
        self.m = len(self.rows)


def brute(c):
    """The same by a nested loop (tiny inputs): (rows, pays)."""
    rows, pays = [], [[] for _ in c["dims"]]
    for j in range(c["n"]):
        vals, ok = [], True
        for d in c["dims"]:
            ps = [int(d["rp"][i]) for i in range(len(d["rk"])) if int(d["rk"][i]) == int(d["sk"][j])]
            if d["how"] == "inner":
                ok &= len(ps) > 0
            elif d["how"] == "anti":
                ok &= len(ps) == 0
            vals.append(min(ps) if ps else d["null"])
        if ok:
            rows.append(j)
            for q, v in zip(pays, vals):
                q.append(v)
    return (np.array(rows, np.int64),
            [None if d["how"] == "anti" else np.array(q, np.int64) for d, q in zip(c["dims"], pays)])


# ------------------------------------------------------------------ builders
def _top(wide):
    return 1 << 40 if wide else 1 << 29


def relation(seed, nr, wide, repeats=0, null_row=None, pad=0):
    """A build side: nr distinct keys in [1, top) -- `repeats` of them then
    taken by the last `repeats` rows again, wide: row null_row holding
    INT64_MIN -- followed by `pad` rows of negative keys no probe column holds.
    Payloads: int64 distinct values around zero, i32 the row ids."""
    rng = np.random.default_rng(seed)
    dt = np.int64 if wide else np.int32
    rk = rng.permutation(np.unique(rng.integers(1, _top(wide), 2 * nr + 8)))[:nr].astype(dt)
    assert len(rk) == nr
    if repeats:
        rk[nr - repeats:] = rk[:repeats]
    if wide and null_row is not None:
        rk[null_row] = I64_MIN
    if pad:
        rk = np.concatenate([rk, -np.arange(1, pad + 1, dtype=dt) * 7])
    return rk, AC.payloads(rk, seed + 1)


def column(seed, rk, n, hit):
    """A probe key column: row j holds a key of rk (never INT64_MIN, never a
    negative pad key) where hit[j], else a key no build side holds."""
    rng = np.random.default_rng(seed)
    wide = rk.dtype == np.int64
    top = _top(wide)
    sk = rng.integers(2 * top, 4 * top - 1, n).astype(rk.dtype)
    pool = rk[rk > 0]
    hit = np.asarray(hit, bool)
    if len(pool) and hit.any():
        sk[hit] = pool[rng.integers(0, len(pool), int(hit.sum()))]
    return sk


def dim(rk, rp, sk, how, null=NULL):
    return dict(rk=rk, rp=rp, sk=sk, how=how, null=null)


# ------------------------------------------------------------------ the shared cases
MIXED_N = 2 * TILE + 77
MIXED_ROWS = (300, 1000, 5000)
# wide: probe rows whose dimension-0 key is INT64_MIN -- the first tile (kept), the middle one (dimension 1 drops
# it), the ragged last (kept) -- and a kept row whose LEFT key is INT64_MIN (dimension 2's side list is empty)
MIXED_NULL_ROWS = (5, TILE + 10, 2 * TILE + 70)
MIXED_LEFT_NULL_ROW = 40


@functools.lru_cache(maxsize=None)
def mixed_case(wide):
    """Three dimensions (inner, inner, left) of 300, 1000 and 5000 build rows,
    the last with repeated keys: tile 0 keeps all 2048 rows, tile 1 none (half
    fail dimension 0, the others pass it and fail dimension 1), the ragged
    tile 2 some; a quarter of the LEFT keys have no partner."""
    n = MIXED_N
    rng = np.random.default_rng(11 + wide)
    r0 = relation(100 + wide, MIXED_ROWS[0], wide, null_row=7)
    r1 = relation(110 + wide, MIXED_ROWS[1], wide)
    r2 = relation(120 + wide, MIXED_ROWS[2], wide, repeats=50)
    tile = np.arange(n) // TILE
    h0 = (tile == 0) | ((tile == 1) & (np.arange(n) % 2 == 0)) | ((tile == 2) & (rng.random(n) < 0.6))
    h1 = (tile == 0) | ((tile == 1) & (np.arange(n) % 2 == 1)) | ((tile == 2) & (rng.random(n) < 0.7))
    h2 = rng.random(n) < 0.75
    s0, s1, s2 = column(130, r0[0], n, h0), column(131, r1[0], n, h1), column(132, r2[0], n, h2)
    s2[rng.permutation(n)[:200]] = r2[0][0]            # a repeated build key: the smallest of two payloads
    if wide:
        s0[list(MIXED_NULL_ROWS)] = I64_MIN
        s1[MIXED_NULL_ROWS[2]] = r1[0][3]              # the ragged tile's INT64_MIN row is kept
        s2[MIXED_LEFT_NULL_ROW] = I64_MIN
    return dict(wide=wide, n=n, dims=[dim(*r0, s0, "inner"), dim(*r1, s1, "inner"), dim(*r2, s2, "left")])


@functools.lru_cache(maxsize=None)
def four_case(wide):
    """Four dimensions (inner, left, anti, inner) over 3 * 2048 + 500 rows:
    rows that fail only the last one, only the anti one, and a LEFT null."""
    n = 3 * TILE + 500
    rng = np.random.default_rng(21 + wide)
    r = [relation(200 + 10 * i + wide, nr, wide, null_row=3 if i == 2 else None)
         for i, nr in enumerate((400, 900, 200, 1500))]
    hits = [rng.random(n) < p for p in (0.8, 0.5, 0.1, 0.7)]
    s = [column(240 + i, r[i][0], n, hits[i]) for i in range(4)]
    if wide:
        s[2][[17, TILE + 3]] = I64_MIN                 # the anti dimension holds INT64_MIN: these rows are dropped
    hows = ("inner", "left", "anti", "inner")
    return dict(wide=wide, n=n, dims=[dim(*r[i], s[i], hows[i]) for i in range(4)])


STRIDED_PAD = 3000   # rows that take the second dimension's table past 64 KiB


STRIDED_HOWS = (("inner", "inner"), ("left", "left"))


@functools.lru_cache(maxsize=None)
def strided_case(wide, hows=STRIDED_HOWS[0]):
    """positional_cases.SEVERAL_NS probe rows (1026 tiles) over two dimensions
    of kinds `hows` whose tables are exactly 64 KiB each: both LDS-resident,
    one workgroup per CU, so every workgroup of the probe launch strides.  A
    quarter of the rows have a partner in the first dimension, six in ten in
    the second (five of its keys twice); wide: the first build holds INT64_MIN
    and the probe rows positional_cases.NULL_ROWS ask for it (and have a
    partner in the second).  The second dimension's build carries STRIDED_PAD
    more rows of keys no probe row holds: built with them its table is read
    from global memory and the result is the same."""
    n = PC.SEVERAL_NS
    nr = 2048 if wide else 4096
    rng = np.random.default_rng(31 + wide)
    r0 = relation(300 + wide, nr, wide, null_row=PC.SIDE_ROW)
    r1 = relation(310 + wide, nr, wide, repeats=5, pad=STRIDED_PAD)
    s0 = column(320, r0[0], n, rng.random(n) < 0.25)
    s1 = column(321, r1[0], n, rng.random(n) < 0.6)
    if wide:
        s0[list(PC.NULL_ROWS)] = I64_MIN
        s1[list(PC.NULL_ROWS)] = r1[0][7]
    return dict(wide=wide, n=n, nr=nr, dims=[dim(*r0, s0, hows[0]), dim(*r1, s1, hows[1])])


def unpadded(c):
    """strided_case without the second dimension's pad rows."""
    d1 = c["dims"][1]
    return dict(c, dims=[c["dims"][0], dict(d1, rk=d1["rk"][:c["nr"]], rp=d1["rp"][:c["nr"]])])


@functools.lru_cache(maxsize=None)
def expect_of(name, wide, *args):
    """The shared cases' expectations, computed once per process and never written."""
    return Expect({"mixed": mixed_case, "four": four_case, "strided": strided_case}[name](wide, *args))


def small_case(wide, n, hows=("inner", "left"), rows=(300, 1000), seed=0, p=(0.5, 0.6), **kw):
    """len(hows) dimensions of `rows` build rows over n probe rows, dimension i
    hit with probability p[i]; kw goes to the first dimension's relation()."""
    rng = np.random.default_rng(41 + seed)
    dims = []
    for i, how in enumerate(hows):
        rk, rp = relation(400 + 10 * i + seed, rows[i], wide, **(kw if i == 0 else {}))
        dims.append(dim(rk, rp, column(440 + i + seed, rk, n, rng.random(n) < p[i]), how))
    return dict(wide=wide, n=n, dims=dims)
