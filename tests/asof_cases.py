"""Case builders and expectations of the as-of probe tests.  Pure numpy: no
GPU and no library call, so test_asof_abi.py checks these helpers on hand
cases on a CPU-only machine.

The expectation sorts R by (key, payload) and bisects per S row: keys and
payloads / bounds are replaced by their ranks, which order as the values do,
so that (key rank, payload rank) packs into one int64 a single np.searchsorted
bisects.  Signed int64 order throughout -- i32 relations are passed widened,
row ids as payloads -- so INT64_MIN and INT64_MAX are ordinary values."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KINDS = (0, 1, 2, 3)   # HJ_ASOF_BACKWARD, _FORWARD, and each | HJ_ASOF_STRICT
KIND_ARGS = {0: ("backward", False), 1: ("forward", False), 2: ("backward", True), 3: ("forward", True)}


def expect(rk, rp, sk, sb, kind, null):
    """(out_r, found) the as-of probe of (sk, sb) in (rk, rp) gives under `kind`."""
    rk, rp, sk, sb = (np.asarray(a).astype(np.int64) for a in (rk, rp, sk, sb))
    nr, ns = len(rk), len(sk)
    if nr == 0 or ns == 0:
        return np.full(ns, null, np.int64), np.zeros(ns, bool)
    kr = np.unique(np.concatenate([rk, sk]), return_inverse=True)[1].astype(np.int64)
    vr = np.unique(np.concatenate([rp, sb]), return_inverse=True)[1].astype(np.int64)
    assert kr.max() < (1 << 31) and vr.max() < (1 << 31)
    rc, sc = (kr[:nr] << 32) | vr[:nr], (kr[nr:] << 32) | vr[nr:]
    o = np.argsort(rc, kind="stable")
    rc = rc[o]
    fwd, strict = bool(kind & 1), bool(kind & 2)
    if not fwd:   # the last R row at or before (strict: before) the bound
        at = np.searchsorted(rc, sc, "left" if strict else "right") - 1
    else:         # the first R row at or after (strict: after) it
        at = np.searchsorted(rc, sc, "right" if strict else "left")
    inside = (at >= 0) & (at < nr)
    at = np.clip(at, 0, nr - 1)
    found = inside & ((rc[at] >> 32) == kr[nr:])
    return np.where(found, rp[o][at], null).astype(np.int64), found


def versions(keys, seed):
    """`keys` (distinct) with 1-4 copies of each, as many rows as `keys` has:
    the row count is what the table sizes go by.  Shuffled."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    ends = np.cumsum(rng.integers(1, 5, n))
    group = np.searchsorted(ends, np.arange(n), "right")   # row -> its group
    return keys[group][rng.permutation(n)]


def payloads(rk, seed=1):
    """R's payloads: int64 distinct values around zero (negative ones among
    them), i32 the row ids."""
    n = len(rk)
    if rk.dtype == np.int32:
        return np.arange(n, dtype=np.int64)
    return (np.random.default_rng(seed).permutation(n).astype(np.int64) - n // 2) * 3 + 1


def bounds(rk, rp, sk, seed, exact=0.4):
    """S's bound column, in sk's dtype: drawn from the payloads' range and an
    eighth of it beyond either end; `exact` of the rows with a partner get the
    payload of one of their partners (exact matches)."""
    rng = np.random.default_rng(seed)
    ns = len(sk)
    if len(rk) == 0:
        return rng.integers(-50, 50, ns).astype(sk.dtype)
    rp = np.asarray(rp, np.int64)
    lo, hi = int(rp.min()), int(rp.max())
    m = max(2, (hi - lo) // 8)
    sb = rng.integers(lo - m, hi + m + 1, ns, dtype=np.int64)
    o = np.lexsort((rp, rk))
    a, b = np.searchsorted(rk[o], sk, "left"), np.searchsorted(rk[o], sk, "right")
    pick = np.minimum(a + (rng.random(ns) * (b - a)).astype(np.int64), len(rk) - 1)
    take = (b > a) & (rng.random(ns) < exact)
    sb[take] = rp[o][pick][take]
    return sb.astype(sk.dtype)


def repeated_keys_case(dtype):
    """Distinct keys, some three times, one 502 times (probed by 301 rows), shuffled."""
    rng = np.random.default_rng(17)
    base = rng.permutation(1 << 20)[:1500].astype(np.int64) * 5 + 3
    rk = np.concatenate([base, base[:100], base[:100], np.full(499, base[7])])
    rk = rk[rng.permutation(len(rk))].astype(dtype)
    sk = np.concatenate([base[::2], base[:100], [base[7]] * 300, rng.integers(1 << 25, 1 << 26, 3000)]).astype(dtype)
    return rk, sk[rng.permutation(len(sk))]


def asof_join_loop(rkey, rtime, skey, stime, direction="backward", exact=True, tolerance=None):
    """pandas merge_asof(by=key, on=time) as a plain loop: per S row the index
    of the matched R row or -1.  Among equal times backward takes the last R
    row and forward the first; nearest prefers backward on a distance tie."""
    out = np.full(len(skey), -1, np.int64)
    rows = np.arange(len(rkey))
    for j in range(len(skey)):
        same = rkey == skey[j]
        t = int(stime[j])
        back = rows[same & ((rtime <= t) if exact else (rtime < t))]
        forw = rows[same & ((rtime >= t) if exact else (rtime > t))]
        b = f = -1
        if len(back):
            tb = rtime[back].max()
            b = int(back[rtime[back] == tb].max())
        if len(forw):
            tf = rtime[forw].min()
            f = int(forw[rtime[forw] == tf].min())
        if direction == "backward":
            r = b
        elif direction == "forward":
            r = f
        elif b >= 0 and (f < 0 or t - int(rtime[b]) <= int(rtime[f]) - t):
            r = b
        else:
            r = f
        if r >= 0 and tolerance is not None and abs(int(rtime[r]) - t) > tolerance:
            r = -1
        out[j] = r
    return out
