"""Expectations and value columns of the group probe tests (hj_dev_group_*).
Pure numpy: no GPU, so the helpers and their own checks run on a CPU-only machine.

The group probe returns one row (R payload, count, sum, min, max) per build
row: the aggregates of the probe side's values over the rows with the build
row's key.  Here S is sorted by key once and reduced per distinct key with
np.add / np.minimum / np.maximum.reduceat (int64 add wraps, as the kernels'
does); every R row then takes its key's aggregates by searchsorted."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
COLS = ("r", "cnt", "sum", "min", "max")


def values(n, seed):
    """n int64 values over the whole range, so that sums wrap, INT64_MIN and INT64_MAX among them."""
    v = np.random.default_rng(seed).integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    if n >= 4:
        v[[0, n // 2]] = I64_MIN
        v[[1, n - 1]] = I64_MAX
    return v


def payloads(rk, seed=1):
    """R's payloads, distinct: int64 a permutation around zero, i32 the row ids."""
    n = len(rk)
    if rk.dtype == np.int32:
        return np.arange(n, dtype=np.int64)
    return (np.random.default_rng(seed).permutation(n).astype(np.int64) - n // 2) * 3 + 1


def expect(rk, rp, sk, sv, how="matched", null=0):
    """The five expected columns as int64 arrays, sorted by R payload."""
    rk, sk = np.asarray(rk).astype(np.int64), np.asarray(sk).astype(np.int64)
    rp, sv = np.asarray(rp, np.int64), np.asarray(sv, np.int64)
    nr = len(rk)
    cnt = np.zeros(nr, np.int64)
    tot = np.zeros(nr, np.int64)
    lo = np.full(nr, null, np.int64)
    hi = np.full(nr, null, np.int64)
    if len(sk) and nr:
        o = np.argsort(sk, kind="stable")
        ks, vs = sk[o], sv[o]
        uk, start, c = np.unique(ks, return_index=True, return_counts=True)
        with np.errstate(over="ignore"):
            s_sum = np.add.reduceat(vs, start)
        s_min, s_max = np.minimum.reduceat(vs, start), np.maximum.reduceat(vs, start)
        at = np.minimum(np.searchsorted(uk, rk), len(uk) - 1)
        hit = uk[at] == rk
        cnt = np.where(hit, c[at], 0).astype(np.int64)
        tot = np.where(hit, s_sum[at], 0).astype(np.int64)
        lo = np.where(hit, s_min[at], null).astype(np.int64)
        hi = np.where(hit, s_max[at], null).astype(np.int64)
    keep = np.ones(nr, bool) if how == "all" else cnt > 0
    o = np.argsort(rp[keep], kind="stable")
    return {k: a[keep][o] for k, a in zip(COLS, (rp, cnt, tot, lo, hi))}


def _self_check():
    rk = np.array([5, 7, 5, 9, I64_MIN], np.int64)
    rp = np.array([10, 11, 12, 13, 14], np.int64)
    sk = np.array([5, 5, 7, 8, I64_MIN, 5], np.int64)
    sv = np.array([I64_MAX, 1, -4, 99, I64_MIN, 2], np.int64)
    e = expect(rk, rp, sk, sv, "all", null=-7)
    assert e["r"].tolist() == [10, 11, 12, 13, 14]
    assert e["cnt"].tolist() == [3, 1, 3, 0, 1]
    assert e["sum"].tolist() == [I64_MIN + 2, -4, I64_MIN + 2, 0, I64_MIN]   # I64_MAX + 1 + 2 wraps
    assert e["min"].tolist() == [1, -4, 1, -7, I64_MIN] and e["max"].tolist() == [I64_MAX, -4, I64_MAX, -7, I64_MIN]
    m = expect(rk, rp, sk, sv, "matched")
    assert m["r"].tolist() == [10, 11, 12, 14] and m["cnt"].tolist() == [3, 1, 3, 1]
    assert all(len(expect(rk[:0], rp[:0], sk, sv, h)["r"]) == 0 for h in ("all", "matched"))
    assert expect(rk, rp, sk[:0], sv[:0], "all", 3)["min"].tolist() == [3] * 5


_self_check()
