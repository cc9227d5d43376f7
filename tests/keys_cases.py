"""Host restatement of the composite-key codec (hj.h "Composite keys"): the
plan with Python integers, pack and unpack once with Python integers
(pack_py / unpack_py: the definition, row by row) and once with wrapping numpy
uint64 arithmetic (pack / unpack: the same formula over whole columns, for the
large cases).  Nothing here touches the library."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
M64 = (1 << 64) - 1


def plan(relations, ncols=None):
    """The sealed plan after observing `relations` (each a list of equally long
    numpy columns): lo / hi per column over every observed row, bits = the bit
    length of hi - lo, shift = the widths of the columns after it, total."""
    ncols = len(relations[0]) if ncols is None else ncols
    rows = sum(len(r[0]) for r in relations)
    lo, hi = [0] * ncols, [0] * ncols
    if rows:
        for c in range(ncols):
            lo[c] = min(int(r[c].min()) for r in relations if len(r[c]))
            hi[c] = max(int(r[c].max()) for r in relations if len(r[c]))
    bits = [(h - l).bit_length() for l, h in zip(lo, hi)]   # 64 - clz(span), 0 for span == 0
    shift = [sum(bits[c + 1:]) for c in range(ncols)]
    total = sum(bits)
    return {"lo": lo, "hi": hi, "bits": bits, "shift": shift, "total_bits": total, "fits": total <= 64,
            "rows_observed": rows}


def pack_py(pl, cols):
    """Row by row with Python integers: OR over the columns with bits > 0 of (v - lo) << shift."""
    assert pl["fits"]
    out = []
    for row in zip(*[c.tolist() for c in cols]):
        k = 0
        for v, lo, b, s in zip(row, pl["lo"], pl["bits"], pl["shift"]):
            if b > 0:
                k |= ((v - lo) & M64) << s
        assert k <= M64
        out.append(k)
    return np.array(out, dtype=np.uint64).view(np.int64)


def unpack_py(pl, keys, dtypes):
    ks = [int(k) & M64 for k in keys.tolist()]
    cols = []
    for lo, b, s, dt in zip(pl["lo"], pl["bits"], pl["shift"], dtypes):
        cols.append(np.array([lo + (((k >> s) & ((1 << b) - 1)) if b else 0) for k in ks], dtype=dt))
    return cols


def pack(pl, cols):
    """pack_py over whole columns (wrapping uint64 arithmetic); int64 words."""
    assert pl["fits"]
    key = np.zeros(len(cols[0]), np.uint64)
    with np.errstate(over="ignore"):
        for col, lo, b, s in zip(cols, pl["lo"], pl["bits"], pl["shift"]):
            if b > 0:
                d = col.astype(np.int64).view(np.uint64) - np.uint64(lo & M64)
                key |= d << np.uint64(s)
    return key.view(np.int64)


def unpack(pl, keys, dtypes):
    k = np.ascontiguousarray(keys, np.int64).view(np.uint64)
    cols = []
    with np.errstate(over="ignore"):
        for lo, b, s, dt in zip(pl["lo"], pl["bits"], pl["shift"], dtypes):
            f = (k >> np.uint64(s)) & np.uint64((1 << b) - 1) if b else np.zeros(len(k), np.uint64)
            cols.append((f + np.uint64(lo & M64)).view(np.int64).astype(dt))
    return cols


def outside(pl, cols):
    """Per row: some column's value lies outside the plan's [lo, hi]."""
    bad = np.zeros(len(cols[0]), bool)
    for col, lo, hi in zip(cols, pl["lo"], pl["hi"]):
        c = col.astype(np.int64)
        if lo > I64_MIN:
            bad |= c < lo
        if hi < I64_MAX:
            bad |= c > hi
    return bad


def lex_order(cols):
    """argsort of the rows as tuples, column 0 most significant."""
    return np.lexsort(tuple(c.astype(np.int64) for c in reversed(cols)))


def column(rng, dtype, lo, hi, n, plant=True):
    """n values of dtype uniform in [lo, hi], both ends planted (n >= 2)."""
    c = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True).astype(dtype)
    if plant and n >= 2:
        at = rng.permutation(n)[:2]
        c[at[0]], c[at[1]] = lo, hi
    return c


# name -> (dtypes, [(lo, hi) per column]); every joint range fits 64 bits
SHAPES = {
    "i64x2": ((np.int64, np.int64), ((-(1 << 40), 1 << 40), (-5000, 5000))),                      # 42 + 14
    "i32-i64-i32": ((np.int32, np.int64, np.int32), ((I32_MIN, I32_MAX), (-(1 << 20), 1 << 20), (-100, 100))),   # 32 + 22 + 8
    "i32x4": ((np.int32,) * 4, ((0, 65535), (-7, 8), (3, 3), (-(1 << 30), 1 << 30))),             # 16 + 4 + 0 + 31
}


def relation(name, n, seed):
    dtypes, ranges = SHAPES[name]
    rng = np.random.default_rng(seed)
    return [column(rng, dt, lo, hi, n) for dt, (lo, hi) in zip(dtypes, ranges)]
