"""Case builders and expectations of the outer / full / build probe tests that
are shared between test modules.  Pure numpy (and the CPU oracle's generators
for the radix shapes): no GPU, so every builder and its structural asserts
can be run on a CPU-only machine.

An expectation is held as row indices -- the pairs (ri, si), the S rows
without a partner (s_un) and the R rows without one (r_un) -- so one case
serves the int64 types (payload columns) and the i32 types (row ids)."""
import functools

import numpy as np

I64_MIN = -(1 << 63)
TILE = 2048   # rows of a probe tile, slots of a slot-scan tile
KINDS = ("outer", "full", "build")


class Expect:
    """What numpy says R and S join to: sort + searchsorted for the pairs, np.isin for the null rows."""

    def __init__(self, rk, sk):
        o = np.argsort(rk, kind="stable")
        rs = rk[o]
        lo, hi = np.searchsorted(rs, sk, "left"), np.searchsorted(rs, sk, "right")
        self.cnt = hi - lo                                   # partners of every S row
        off = np.arange(int(self.cnt.sum())) - np.repeat(np.cumsum(self.cnt) - self.cnt, self.cnt)
        self.ri = o[np.repeat(lo, self.cnt) + off]
        self.si = np.repeat(np.arange(len(sk)), self.cnt)
        self.s_un = np.flatnonzero(self.cnt == 0)
        self.r_un = np.flatnonzero(~np.isin(rk, sk))
        self.pairs, self.n_s, self.n_r = len(self.ri), len(self.s_un), len(self.r_un)

    def m(self, kind):
        return self.pairs + (self.n_s if kind in ("outer", "full") else 0) + (self.n_r if kind in ("full", "build") else 0)

    def rows(self, kind, rp, sp, null_r, null_s):
        """The expected columns (r, s) of `kind`: the pairs, then S's null rows, then R's."""
        r, s = [rp[self.ri]], [sp[self.si]]
        if kind in ("outer", "full"):
            r.append(np.full(self.n_s, null_r, np.int64))
            s.append(sp[self.s_un])
        if kind in ("full", "build"):
            r.append(rp[self.r_un])
            s.append(np.full(self.n_r, null_s, np.int64))
        return np.concatenate(r).astype(np.int64), np.concatenate(s).astype(np.int64)


def sorted_pairs(r, s):
    o = np.lexsort((s, r))
    return np.stack([r[o], s[o]])


def same_rows(gr, gs, er, es, null_r, null_s):
    """Exact multiset equality of the rows (gr, gs) and (er, es).  Neither
    null value is a payload, so the rows fall into three classes -- (null_r,
    s), (r, null_s) and pairs -- that are compared class by class: one
    column sort for each kind of null row, a two-column sort for the pairs."""
    if len(gr) != len(er):
        return False
    g_s, g_r = gr == null_r, gs == null_s
    e_s, e_r = er == null_r, es == null_s
    assert not (e_s & e_r).any()
    if (g_s & g_r).any():
        return False
    g_p, e_p = ~(g_s | g_r), ~(e_s | e_r)
    return (np.array_equal(np.sort(gs[g_s]), np.sort(es[e_s])) and np.array_equal(np.sort(gr[g_r]), np.sort(er[e_r]))
            and np.array_equal(sorted_pairs(gr[g_p], gs[g_p]), sorted_pairs(er[e_p], es[e_p])))


# ------------------------------------------------------------------ strided general path and slot scan
R_OFF, S_OFF = 1 << 33, 1 << 40   # int64 payloads: the row index plus these


@functools.lru_cache(maxsize=None)
def strided_general_case(cus):
    """The smallest global-table shape at which the three persistent loops of
    8 x CUs workgroups take a second tile: 8 x CUs + 60 probe tiles, every
    one handed to the general path (k_probe_slow, k_probe_mark), and a build
    side past 2^21 rows, whose table is more than 8 x CUs x 2048 slots
    (k_emit_unmatched).  Keys fit int32, so the case serves both row widths.
    Built once per process and shared between test modules: its arrays are never written."""
    tiles = 8 * cus + 60
    ns = tiles * TILE - 1000
    nr = (1 << 21) + 5
    rng = np.random.default_rng(8 * cus + 60)
    rk = rng.permutation(1 << 23)[:nr].astype(np.int64) * 3 + 1   # distinct
    rk[-3:] = rk[:3]                                              # three keys twice
    sk = rng.integers(0, 1 << 25, ns, dtype=np.int64)
    # one row of every tile (the last holds 1048) meets a repeated key: the tile is handed over
    at = np.arange(tiles) * TILE + rng.integers(0, TILE - 1000, tiles)
    sk[at] = rk[0]
    e = Expect(rk, sk)
    slots = 1 << int(2 * nr - 1).bit_length()                     # 2 * nr rounded up to a power of two
    assert len(np.unique(rk)) == nr - 3
    assert int((e.cnt > 1).sum()) == tiles, int((e.cnt > 1).sum())   # the slow list is filled to exactly its tile count
    assert np.array_equal(np.unique(np.flatnonzero(e.cnt > 1) // TILE), np.arange(tiles))
    assert tiles > 8 * cus and slots > 8 * cus * TILE
    assert e.pairs > 0 and e.n_r > 0 and e.n_s > 0
    assert int(rk.max()) < (1 << 31) and int(sk.max()) < (1 << 31)
    return dict(rk=rk, sk=sk, exp=e, tiles=tiles, slots=slots)


# ------------------------------------------------------------------ radix join paths
RADIX_SHAPES = ("stream-pkfk", "stream-dups", "grp-wide", "grp-i32", "b-some", "stream-null", "grp-wide-null",
                "b-oversized")


def radix_path_case(oracle, name):
    """Build keys, probe keys, radix bits and the join kernel the shape is
    chosen for (None: whichever the inner probe reports), for the shapes
    whose kernel choice test_gpu_radix.py pins, shifted so that R and S both
    hold rows without a partner."""
    kernel, wide = None, True
    if name in ("stream-pkfk", "stream-null"):
        rk, _, sk, _ = oracle.gen_pkfk_i64(11, 6000, 90000, 0.8)
        rk = np.concatenate([rk, (1 << 45) + np.arange(3000, dtype=np.int64)])   # keys S does not hold
        sk = sk.copy()
        if name == "stream-null":   # INT64_MIN build keys: items deferred to k_join
            rk[::500] = I64_MIN
            sk[::1777] = I64_MIN
        bits, kernel = 3, "k_join_u_stream"
    elif name == "stream-dups":
        rk = oracle.gen_uniform_i64(11, 1, -999, 3000, 9000)[0]
        sk = oracle.gen_uniform_i64(11, 2, 1, 4000, 90000)[0]
        bits, kernel = 3, "k_join_u_stream"
    elif name in ("grp-wide", "grp-wide-null"):
        rk = oracle.gen_uniform_i64(10, 1, 1, 2000, 20000)[0].copy()
        sk = oracle.gen_uniform_i64(10, 2, 500, 2500, 6000)[0]
        if name == "grp-wide-null":   # INT64_MIN build keys: the grouped kernel defers through list 2
            rk[::97] = I64_MIN
        bits, kernel = 6, "k_join_grp"
    elif name == "grp-i32":
        rk = oracle.gen_uniform_i64(7, 1, 1, 400, 16000)[0].astype(np.int32)
        sk = oracle.gen_uniform_i64(7, 2, 100, 500, 12000)[0].astype(np.int32)
        bits, kernel, wide = 6, "k_join_grp", False
    elif name == "b-some":        # every tenth build key repeated: the bucketed table's marked-slot path
        rk = oracle.gen_uniform_i64(8, 1, 1, 1 << 40, 20000)[0].copy()
        rk[::10] = rk[1::10]
        sk = oracle.gen_uniform_i64(8, 2, 1, 1 << 40, 20000)[0].copy()
        sk[:5000] = rk[:5000]
        bits, kernel = 6, "k_join_b"
    elif name == "b-oversized":   # 20000 copies of one key: several LDS build rounds of one partition
        rk = np.concatenate([np.full(20000, 42, np.int64), np.arange(1000, 3000, dtype=np.int64)])
        sk = oracle.gen_uniform_i64(12, 2, 1, 6000, 9000)[0].copy()
        sk[[10, 4000, 8999]] = 42
        bits = 4
    else:
        raise KeyError(name)
    e = Expect(rk, sk)
    assert e.pairs > 0 and e.n_r > 0 and e.n_s > 0, (name, e.pairs, e.n_r, e.n_s)
    if name.endswith("-null"):
        assert (rk == I64_MIN).any() and (sk == I64_MIN).any() == (name == "stream-null")
    if kernel == "k_join_u_stream":
        assert len(sk) >= 8 * len(rk)   # the probe-heavy shape
    if name == "b-oversized":
        assert 3 <= int((sk == 42).sum()) < 20
    return dict(name=name, rk=rk, sk=sk, exp=e, bits=bits, kernel=kernel, wide=wide)


def replay_sets_other_kernels(oracle, n, cap):
    """Two (R keys, S keys) sets of n rows a side that move a captured int64
    radix join off k_join_b with empty deferral lists: keys uniform in
    [1, n / 4] on both sides (most build keys repeat: k_join_grp takes every
    item), and PK-FK keys with INT64_MIN on both sides (the deferral lists
    fill).  Neither result reaches `cap` rows."""
    grp = (oracle.gen_uniform_i64(71, 1, 1, n // 4, n)[0], oracle.gen_uniform_i64(71, 2, 1, n // 4, n)[0])
    rk, _, sk, _ = oracle.gen_pkfk_i64(75, n, n, 0.5)
    rk, sk = rk.copy(), sk.copy()
    rk[::97] = sk[::131] = I64_MIN
    assert len(np.unique(grp[0])) < n // 2          # more than half of the build rows repeat a key
    for r, s in (grp, (rk, sk)):
        e = Expect(r, s)
        assert e.n_r > 0 and e.n_s > 0 and e.m("full") < cap, (e.pairs, e.n_r, e.n_s, cap)
    return grp, (rk, sk)


def fresh_context_case():
    """2^10 partitions, 30000 build rows, 50 probe rows (most partitions hold
    build rows only), and a 200000-row probe side for the same build."""
    rng = np.random.default_rng(5)
    rk = rng.permutation(1 << 20)[:30000].astype(np.int64) * 1000003 + 17
    sk = np.concatenate([rk[rng.integers(0, 30000, 25)], rng.integers(1 << 50, 1 << 51, 25, dtype=np.int64)])
    big = rng.integers(1 << 50, 1 << 51, 200000, dtype=np.int64)
    hit = rng.random(200000) < 0.4
    big[hit] = rk[rng.integers(0, 30000, int(hit.sum()))]
    e, eb = Expect(rk, sk), Expect(rk, big)
    assert e.n_r >= 30000 - 25 and e.n_s == 25 and e.pairs == 25
    assert eb.pairs > 0 and eb.n_r > 0 and eb.n_s > 0
    return dict(rk=rk, sk=sk, exp=e, big=big, exp_big=eb, bits=10)
