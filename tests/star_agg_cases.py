"""Case builders and the expectation of the star aggregate tests (hj.h "Star
aggregate").  Pure numpy: no GPU and no library call, so test_star_agg_cases.py
checks the expectation against a nested loop and the shared cases' coverage
conditions on a CPU-only machine.

A case is star_cases' dict(wide, n, dims) plus, per call, a value column and
per dimension gshift / gbase.  expect() composes star_cases.Expect (which rows
are kept, each dimension's payload of them) with the group-key formula in
uint64 arithmetic and aggregate_cases.expect's sort-based group-by."""
import functools
import itertools

import numpy as np

import aggregate_cases as GC
import star_cases as SC

I64_MIN, I64_MAX = GC.I64_MIN, GC.I64_MAX
TILE = SC.TILE
COLS = GC.COLS


def values(c, seed=5):
    """The fact column to aggregate, in the key columns' dtype: the whole range
    of it, the extremes among them -- int64 sums wrap."""
    if c["wide"]:
        return GC.values(c["n"], seed)
    n = c["n"]
    v = np.random.default_rng(seed).integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int64, endpoint=True).astype(np.int32)
    if n >= 4:
        v[[0, n // 2]] = -(1 << 31)
        v[[1, n - 1]] = (1 << 31) - 1
    return v


def plan(c, grouped):
    """KeyCodec's sealed plan over the payloads the grouped dimensions can give
    (their build payloads and a LEFT null): (gshift, gbase) per dimension,
    gshift -1 for a dimension outside `grouped` or of one value only."""
    nd = len(c["dims"])
    lo, bits = [0] * nd, [0] * nd
    for i in grouped:
        d = c["dims"][i]
        assert d["how"] != "anti"
        vals = [int(v) for v in (d["rp"].min(), d["rp"].max())] if len(d["rp"]) else []
        if d["how"] == "left":
            vals.append(int(d["null"]))
        if vals:
            lo[i], bits[i] = min(vals), (max(vals) - min(vals)).bit_length()
    assert sum(bits) <= 64
    gshift = [-1] * nd
    for i in grouped:
        if bits[i]:
            gshift[i] = sum(bits[j] for j in grouped if j > i)
    return gshift, lo


def group_keys(e, gshift, gbase=None):
    """g(j) of the kept rows, as int64 words: the formula in uint64 arithmetic."""
    g = np.zeros(e.m, np.uint64)
    for d, sh in enumerate(gshift):
        if sh < 0:
            continue
        base = np.uint64((gbase[d] if gbase is not None else 0) & ((1 << 64) - 1))
        with np.errstate(over="ignore"):
            g += (e.pays[d].astype(np.int64).view(np.uint64) - base) << np.uint64(sh)
    return g.view(np.int64)


def expect(c, e, val, gshift, gbase=None):
    """The five expected columns as int64 arrays sorted by key; val None: zeros are summed."""
    v = np.zeros(c["n"], np.int64) if val is None else np.asarray(val).astype(np.int64)
    return GC.expect(group_keys(e, gshift, gbase), v[e.rows])


def brute(c, val, gshift, gbase=None):
    """The same by nested loops over Python integers (tiny inputs)."""
    rows, pays = SC.brute(c)
    acc = {}
    for o, j in enumerate(rows):
        g = 0
        for d, sh in enumerate(gshift):
            if sh >= 0:
                g += ((int(pays[d][o]) - (gbase[d] if gbase is not None else 0)) % (1 << 64)) << sh
        g %= 1 << 64
        g -= (1 << 64) if g >= (1 << 63) else 0
        v = int(val[j])
        a = acc.setdefault(g, [0, 0, v, v])
        a[0] += 1
        a[1] += v
        a[2], a[3] = min(a[2], v), max(a[3], v)
    keys = sorted(acc)
    wrap = lambda s: (s + (1 << 63)) % (1 << 64) - (1 << 63)  # noqa: E731
    cols = [keys, [acc[k][0] for k in keys], [wrap(acc[k][1]) for k in keys], [acc[k][2] for k in keys],
            [acc[k][3] for k in keys]]
    return {n: np.array(col, np.int64) for n, col in zip(COLS, cols)}


def subsets(c):
    """Every subset of the dimensions that have a payload (the non-ANTI ones), the empty one first."""
    can = [i for i, d in enumerate(c["dims"]) if d["how"] != "anti"]
    return [s for k in range(len(can) + 1) for s in itertools.combinations(can, k)]


def groups_per_tile(c, e, gshift, gbase=None):
    """Distinct group keys among each tile's kept rows (0 for a tile with no survivor)."""
    g, tile = group_keys(e, gshift, gbase), e.rows // TILE
    return [len(np.unique(g[tile == t])) for t in range(-(-c["n"] // TILE))]


# ------------------------------------------------------------------ the shared cases
MANY_ROWS = (300, 1000)


@functools.lru_cache(maxsize=None)
def many_case(wide):
    """Two grouped inner dimensions of 300 and 1000 build rows over three
    tiles, nine rows in ten kept: far more than 512 distinct groups in every
    tile, so most rows pass the LDS table by and reach the global one directly."""
    return SC.small_case(wide, 2 * TILE + 900, hows=("inner", "inner"), rows=MANY_ROWS, seed=70, p=(0.95, 0.95))


@functools.lru_cache(maxsize=None)
def min_word_case(wide):
    """One grouped inner dimension whose payloads have both parities: under
    gshift 63 the group keys are exactly 0 and the INT64_MIN word."""
    return SC.small_case(wide, TILE + 321, hows=("inner",), rows=(400,), seed=71, p=(0.8,))


OVERFLOW_RESERVE = 8
OVERFLOW_CAPACITY = 2048          # what reserve_groups(8) gives: max(2 * 8, 2048)
OVERFLOW_GROUPS = OVERFLOW_CAPACITY + 1000


@functools.lru_cache(maxsize=None)
def overflow_case(wide):
    """One grouped left dimension of OVERFLOW_GROUPS build rows, each asked for
    by one probe row and more: that many distinct groups in one call."""
    nr = OVERFLOW_GROUPS
    rk, rp = SC.relation(80 + wide, nr, wide)
    n = 2 * TILE
    sk = rk[np.arange(n) % nr].copy()
    return dict(wide=wide, n=n, dims=[SC.dim(rk, rp, sk, "left")])
