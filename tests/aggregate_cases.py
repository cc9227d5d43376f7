"""Expectations and value columns of the hash aggregate tests (hj_dev_aggregate_*).
Pure numpy: no GPU, so the helpers and their own checks run on a CPU-only machine.

The aggregate returns one row (key, count, sum, min, max) per distinct key of
one relation.  Here the relation is sorted by key once and reduced per distinct
key with np.unique(return_index, return_counts) and np.add / np.minimum /
np.maximum.reduceat (int64 add wraps, as the kernels' does)."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN = -(1 << 31)
COLS = ("key", "cnt", "sum", "min", "max")


def values(n, seed):
    """n int64 values over the whole range, so that sums wrap, INT64_MIN and INT64_MAX among them."""
    v = np.random.default_rng(seed).integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    if n >= 4:
        v[[0, n // 2]] = I64_MIN
        v[[1, n - 1]] = I64_MAX
    return v


def values_of(key, seed=5, row_base=0):
    """The value column of a key column: int64 the whole range, i32 the row ids."""
    if key.dtype == np.int32:
        return np.arange(len(key), dtype=np.int64) + row_base
    return values(len(key), seed)


def expect(key, val):
    """The five expected columns as int64 arrays, sorted by key."""
    key, val = np.asarray(key).astype(np.int64), np.asarray(val, np.int64)
    if len(key) == 0:
        return {c: np.zeros(0, np.int64) for c in COLS}
    o = np.argsort(key, kind="stable")
    ks, vs = key[o], val[o]
    uk, start, c = np.unique(ks, return_index=True, return_counts=True)
    with np.errstate(over="ignore"):
        s = np.add.reduceat(vs, start)
    return dict(zip(COLS, (uk, c.astype(np.int64), s, np.minimum.reduceat(vs, start), np.maximum.reduceat(vs, start))))


def keys_over(n, distinct, seed, dtype=np.int64, plant=()):
    """n keys drawn from `distinct` distinct values (each present at least once
    when n >= distinct), the values of `plant` among them."""
    if n == 0:
        return np.zeros(0, dtype)
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    pool = set(int(x) for x in plant)
    while len(pool) < distinct:
        pool.update(int(x) for x in rng.integers(info.min, info.max, distinct - len(pool), dtype=dtype, endpoint=True))
    pool = np.array(sorted(pool), dtype=dtype)
    k = pool[rng.integers(0, distinct, n)]
    if n >= distinct:
        k[rng.permutation(n)[:distinct]] = pool
    return k


def _self_check():
    k = np.array([5, 5, 7, 8, I64_MIN, 5, 0, -1], np.int64)
    v = np.array([I64_MAX, 1, -4, 99, I64_MIN, 2, 3, I64_MAX], np.int64)
    e = expect(k, v)
    assert e["key"].tolist() == [I64_MIN, -1, 0, 5, 7, 8]
    assert e["cnt"].tolist() == [1, 1, 1, 3, 1, 1]
    assert e["sum"].tolist() == [I64_MIN, I64_MAX, 3, I64_MIN + 2, -4, 99]   # I64_MAX + 1 + 2 wraps
    assert e["min"].tolist() == [I64_MIN, I64_MAX, 3, 1, -4, 99]
    assert e["max"].tolist() == [I64_MIN, I64_MAX, 3, I64_MAX, -4, 99]
    assert all(len(a) == 0 and a.dtype == np.int64 for a in expect(k[:0], v[:0]).values())
    k32 = np.array([-1, I32_MIN, 0, -1, 0, -1], np.int32)
    e = expect(k32, values_of(k32, row_base=10))
    assert e["key"].tolist() == [I32_MIN, -1, 0] and e["cnt"].tolist() == [1, 3, 2]
    assert e["min"].tolist() == [11, 10, 12] and e["max"].tolist() == [11, 15, 14] and e["sum"].tolist() == [11, 38, 26]
    kk = keys_over(50, 20, 1, np.int32, plant=(-1, 0, I32_MIN))
    assert len(np.unique(kk)) == 20 and {-1, 0, I32_MIN} <= set(kk.tolist())


_self_check()
