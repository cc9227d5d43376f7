"""Expand probe (hj_dev_expand_*: every partner of every probe row, as a CSR in
input order) on both strategies and both row widths.

Expected results come from numpy on the host (expand_cases), never from the
library.  Offsets are compared exactly, element by element; values after
sorting within segments, and unsorted too when the build repeats no key.
Outputs are sentinel-filled and EXTRA elements longer than needed: everything
past the n + 1 offsets and past min(M, cap) values must stay untouched.  int64
payloads are a seeded permutation around zero, times three plus one: NULL and
SENTINEL are multiples of three, so neither is a payload."""
import numpy as np
import pytest
import torch

import expand_cases as XC
import outer_cases as OC
from hashjoin import HashJoin, _lib, lib
from join_gpu import assert_radix_kernel, build, dev, glob_hj, hj, sentinels, timing_reports  # noqa: F401
from test_gpu_lookup import payloads, repeated_keys_case

pytestmark = pytest.mark.gpu

I64_MIN = OC.I64_MIN
NULL, SENTINEL, EXTRA = -9, -12345, 64   # i32 payloads are row ids (>= 0)
TILE, FAN = _lib.EXPAND_SCAN_TILE, _lib.EXPAND_SCAN_FAN   # the scan's tile, and tile sums per step of their scan


def probe(hj, sk, how, cap, d_sk=None):
    """One expand of the current build into sentinel-filled outputs: (M,
    offsets, values) as int64 host arrays; cap None is the count form."""
    n = len(sk)
    dt = torch.int64 if sk.dtype == np.int64 else torch.int32
    off = sentinels(n + 1 + EXTRA, SENTINEL, torch.int64)
    buf = sentinels(cap + EXTRA, SENTINEL, dt) if cap is not None else None
    out = buf[:cap] if cap else None
    m = int(hj.probe_expand(dev(sk) if d_sk is None else d_sk, off, out, how=how, null=NULL).item())
    return m, off.cpu().numpy(), None if buf is None else buf.cpu().numpy().astype(np.int64)


def check(hj, rk, rp, sk, how, cap="exact", d_sk=None):
    """The full call at `cap` ('exact': M) against numpy; returns the expectation."""
    e = XC.ExpandExpect(rk, rp, sk, how, NULL)
    n = len(sk)
    cap = e.m if cap == "exact" else cap
    m, off, vals = probe(hj, sk, how, cap, d_sk)
    assert m == e.m, (m, e.m)
    assert np.array_equal(off[:n + 1], e.off), np.flatnonzero(off[:n + 1] != e.off)[:8]
    assert (off[n + 1:] == SENTINEL).all()
    upto = min(e.m, cap)
    assert e.same_values(vals, upto)
    assert (vals[upto:] == SENTINEL).all()      # nothing at or past cap, nothing past M
    return e


def both_kinds(hj, rk, rp, sk):
    return [check(hj, rk, rp, sk, how) for how in XC.KINDS]


def assert_radix(hj):
    assert _lib.HJ_JOIN_KERNEL_EXPAND == 10
    assert_radix_kernel(hj, _lib.HJ_JOIN_KERNEL_EXPAND, "k_join_expand")


class radix:
    """with radix(hj, bits): the strategy for the block, AUTO afterwards."""

    def __init__(self, hj, bits, strategy="radix"):
        self.hj, self.bits, self.strategy = hj, bits, strategy

    def __enter__(self):
        self.hj.set_strategy(self.strategy, radix_bits=self.bits if self.strategy == "radix" else 0)

    def __exit__(self, *a):
        self.hj.set_strategy("auto")


# ------------------------------------------------------------------ global
# (ns = 2 * 2048 + 77 is three tiles, one per workgroup: k_probe_lookup's count
# stage and k_probe_expand never stride here.  The shape with more tiles than
# workgroups, and a cap that cuts a later tile, is test_gpu_positional_tiles.py's.)
@pytest.mark.parametrize("nr", [1, 2048, 3000])   # 2048: the last LDS-resident table
def test_global_i64(glob_hj, oracle, nr):
    ns = 2 * 2048 + 77   # a ragged third tile
    rk, _, sk, _ = oracle.gen_pkfk_i64(300 + nr, nr, ns, 0.6)
    rp = payloads(rk, nr)
    build(glob_hj, rk, rp)
    ei, eo = both_kinds(glob_hj, rk, rp, sk)
    assert ei.unique and 0 < ei.m < ns and eo.m == ns
    assert glob_hj.strategy_used == "global" and glob_hj.join_kernel is None


@pytest.mark.parametrize("nr", [4000, 5000])   # either side of a 64-KiB table
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 2 * 2048 + 77 - len(r[::3]))])
    build(glob_hj, r, None)
    ei, _ = both_kinds(glob_hj, r, payloads(r), s)
    assert ei.m >= len(r[::3])


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_repeated_build_keys(hj, strategy, dtype):
    rk, sk = repeated_keys_case(dtype)
    rp = payloads(rk, 3)
    with radix(hj, 2, strategy):
        build(hj, rk, rp)
        assert hj.has_duplicates()
        ei, _ = both_kinds(hj, rk, rp, sk)
        assert set(np.unique(ei.cnt).tolist()) == {0, 1, 3, 502}
        assert hj.has_duplicates() and hj.strategy_used == strategy


@pytest.mark.parametrize("where", ["probe", "build", "both"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_int64_min(hj, oracle, strategy, where):
    rk = oracle.gen_uniform_i64(12, 1, -2000, 2000, 1500)[0].copy()
    sk = oracle.gen_uniform_i64(12, 2, -3000, 3000, 2 * 2048 + 77)[0].copy()
    if where in ("both", "build"):
        rk[::500] = I64_MIN
    if where in ("both", "probe"):
        sk[::1777] = I64_MIN
    rp = payloads(rk, 5)
    with radix(hj, 3, strategy):
        build(hj, rk, rp)
        ei, eo = both_kinds(hj, rk, rp, sk)
        if where == "both":
            assert (ei.cnt[::1777] == 3).all()
        if where == "probe":
            assert (ei.cnt[::1777] == 0).all() and (eo.r[eo.off[:-1][::1777]] == NULL).all()


# ------------------------------------------------------------------ radix
@pytest.mark.parametrize("bits", [1, 9, 17])   # 1, 1 and 2 partition passes
def test_radix_pkfk(hj, oracle, bits):
    rk, _, sk, _ = oracle.gen_pkfk_i64(bits, 20000, 50000, 0.8)
    rp = payloads(rk, bits)
    with radix(hj, bits):
        build(hj, rk, rp)
        assert hj.radix_passes == {1: 1, 9: 1, 17: 2}[bits]
        both_kinds(hj, rk, rp, sk)
        assert_radix(hj)


@pytest.mark.parametrize("name", OC.RADIX_SHAPES)
def test_radix_shapes(hj, oracle, name):
    c = OC.radix_path_case(oracle, name)
    rk, sk = c["rk"], c["sk"]
    rp = payloads(rk, 7)
    with radix(hj, c["bits"]):
        build(hj, rk, rp)
        ei, _ = both_kinds(hj, rk, rp, sk)
        assert_radix(hj)
        if name == "b-oversized":   # one segment filled across several build rounds
            assert (ei.cnt[[10, 4000, 8999]] == 20000).all()


def test_radix_fresh_context():
    c = OC.fresh_context_case()
    rp = payloads(c["rk"], 9)
    h = HashJoin(0)
    try:
        h.set_strategy("radix", radix_bits=c["bits"])
        build(h, c["rk"], rp)
        for sk in (c["sk"], c["big"]):
            both_kinds(h, c["rk"], rp, sk)
            assert_radix(h)
    finally:
        h.close()


@pytest.mark.parametrize("how", XC.KINDS)
def test_radix_partitions_without_build_rows(hj, how):
    """2^10 partitions, 50 build rows: most S rows lie in items without build
    rows -- their null under OUTER, nothing under INNER."""
    rk = np.arange(50, dtype=np.int64) * 1000003 + 17
    rng = np.random.default_rng(5)
    sk = rng.integers(1 << 40, 1 << 41, 30000, dtype=np.int64)
    hit = rng.random(30000) < 0.5
    sk[hit] = rk[rng.integers(0, 50, int(hit.sum()))]
    rp = payloads(rk, 2)
    with radix(hj, 10):
        build(hj, rk, rp)
        check(hj, rk, rp, sk, how)
        assert_radix(hj)


def test_radix_hot_probe_key_many_chunks(hj):
    rk = np.arange(3000, dtype=np.int64) * 7
    sk = np.concatenate([np.full(50000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    sk = sk[np.random.default_rng(3).permutation(len(sk))]
    rp = payloads(rk, 4)
    with radix(hj, 6):
        build(hj, rk, rp)
        both_kinds(hj, rk, rp, sk)
        assert_radix(hj)


def test_radix_distinct_keys_over_one_round(hj, oracle):
    """30000 distinct build keys per partition: several build rounds, the sub-chunks-outermost path."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(77, 60000, 40000, 0.5)
    rp = payloads(rk, 6)
    with radix(hj, 1):
        build(hj, rk, rp)
        both_kinds(hj, rk, rp, sk)
        assert_radix(hj)


def test_radix_partition_of_int64_min_rows_only(hj):
    """6000 build rows, all INT64_MIN: one partition whose every build round is
    nothing but the key the LDS table cannot hold."""
    rk = np.full(6000, I64_MIN, np.int64)
    sk = np.arange(1, 4001, dtype=np.int64) * 11
    sk[[5, 1700, 3999]] = I64_MIN
    rp = payloads(rk, 8)
    with radix(hj, 1):
        build(hj, rk, rp)
        ei, eo = both_kinds(hj, rk, rp, sk)
        assert ei.m == 3 * 6000 and eo.m == 3 * 6000 + 3997
        assert_radix(hj)


@pytest.mark.parametrize("bits", [1, 9])
def test_radix_i32(hj, oracle, bits):
    r = oracle.gen_uniform_i32(bits, 1, -(1 << 31), (1 << 31) - 1, 30000)
    r[1000:1300] = r[:300]   # some keys twice
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(bits, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    with radix(hj, bits):
        build(hj, r, None)
        ei, _ = both_kinds(hj, r, payloads(r), s)
        assert ei.cnt.max() >= 2
        assert_radix(hj)


# ------------------------------------------------------------------ both strategies
@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_empty_and_tiny(hj, strategy, wide):
    dt = np.int64 if wide else np.int32
    e = np.empty(0, dt)
    k = np.array([5, 9, 5, 3], dt)
    one, other = np.array([4], dt), np.array([6], dt)
    with radix(hj, 3, strategy):
        for rk, sk in [(e, k), (k, e), (one, one), (one, other), (k, one), (k, k[:1])]:
            rp = payloads(rk, 8)
            build(hj, rk, rp)
            ei, eo = both_kinds(hj, rk, rp, sk)
            assert hj.strategy_used == strategy
            if len(rk) == 0:
                assert ei.m == 0 and (ei.off == 0).all()
                assert np.array_equal(eo.off, np.arange(len(sk) + 1)) and (eo.r == NULL).all()
            if len(sk) == 0:
                assert ei.off.tolist() == [0] and eo.off.tolist() == [0]


def mixed_case(oracle, wide):
    """Repeated and missing keys on both sides, in a dtype's range."""
    rk = oracle.gen_uniform_i64(41, 1, 1, 4000, 9000)[0].copy()
    sk = oracle.gen_uniform_i64(41, 2, 1, 6000, 7000)[0].copy()
    if wide:
        rk[::97] = I64_MIN
        sk[::131] = I64_MIN
        return rk, sk
    return rk.astype(np.int32), sk.astype(np.int32)


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_count_form_truncation_and_counts(hj, oracle, strategy, wide):
    """The count form equals the full call's offsets and M; truncation at cap
    in {1, M // 2 inside a segment, M - 1, M}; cap == 0 with an output is
    rejected; OUTER's M is the outer join's, INNER's the inner join's count."""
    rk, sk = mixed_case(oracle, wide)
    rp = payloads(rk, 13)
    d_sk = dev(sk)
    with radix(hj, 4, strategy):
        build(hj, rk, rp)
        for how in XC.KINDS:
            e = XC.ExpandExpect(rk, rp, sk, how, NULL)
            m, off, none = probe(hj, sk, how, None)
            assert none is None and m == e.m and np.array_equal(off[:len(sk) + 1], e.off)
            assert (off[len(sk) + 1:] == SENTINEL).all()
            off_t, m_t = hj.count_expand(d_sk, how=how)
            assert m_t == e.m and np.array_equal(off_t.cpu().numpy(), e.off)
            # a cap that lands inside a segment of more than one entry
            inside = int(e.off[np.flatnonzero((e.w > 1) & (e.off[:-1] >= e.m // 2))[0]]) + 1
            for cap in (1, inside, e.m - 1, e.m):
                check(hj, rk, rp, sk, how, cap, d_sk)
            assert hj.strategy_used == strategy
        ox = OC.Expect(rk, sk)
        assert XC.ExpandExpect(rk, rp, sk, "outer", NULL).m == ox.m("outer")
        assert hj.count_expand(d_sk, how="outer")[1] == ox.m("outer")
        assert hj.count_expand(d_sk, how="inner")[1] == hj.count_rows(d_sk) == ox.pairs
        # cap == 0 with a non-null output, and cap > 0 without one
        f = lib.hj_dev_expand_i64 if wide else lib.hj_dev_expand_i32
        off = torch.zeros(len(sk) + 1, dtype=torch.int64, device="cuda")
        o = torch.zeros(8, dtype=d_sk.dtype, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        P = lambda t: t.data_ptr()   # noqa: E731
        assert f(hj._ctx, 0, P(d_sk), len(sk), NULL, P(off), P(o), 0, P(cnt), None) == _lib.HJ_ERR_ARG
        assert b"bad output" in lib.hj_last_error()
        assert f(hj._ctx, 0, P(d_sk), len(sk), NULL, P(off), None, 8, P(cnt), None) == _lib.HJ_ERR_ARG
        assert b"bad output" in lib.hj_last_error()


# ------------------------------------------------------------------ the scan's boundaries
R3 = np.array([7, 8, 7], np.int64)   # key 7 twice, key 8 once


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, TILE * FAN + 1],
                         ids=["1", "tile-1", "tile", "tile+1", "fan*tile+1"])
def test_scan_boundaries(glob_hj, n):
    """All-hit probe sides against a 3-row build: around one scan tile, and one
    row past what a single step of the tile sums' scan takes."""
    sk = np.where(np.arange(n) % 3 == 1, 8, 7).astype(np.int64)
    rp = np.array([1, 4, 7], np.int64)
    build(glob_hj, R3, rp)
    e = check(glob_hj, R3, rp, sk, "inner")
    assert e.m == n + int((sk == 7).sum())


def test_scan_boundaries_radix(hj):
    n = TILE * 3 + 1
    sk = np.where(np.arange(n) % 3 == 1, 8, 7).astype(np.int64)
    rp = np.array([1, 4, 7], np.int64)
    with radix(hj, 2):
        build(hj, R3, rp)
        check(hj, R3, rp, sk, "outer")
        assert_radix(hj)


def test_m_past_2_to_32(hj):
    """2^16 probe rows of one key against 2^17 copies of it: M = 2^33, the
    count form only.  The scan is the same code under both strategies; the
    radix count stage keeps each key once per build round, where the global
    table would chain 2^17 equal keys behind one slot (a quadratic build)."""
    nr, ns = 1 << 17, 1 << 16
    rk = torch.full((nr,), 5, dtype=torch.int64, device="cuda")
    sk = torch.full((ns,), 5, dtype=torch.int64, device="cuda")
    with radix(hj, 2):
        hj.build_table(rk, torch.arange(nr, dtype=torch.int64, device="cuda"))
        off, m = hj.count_expand(sk, how="inner")
        assert m == nr * ns == 1 << 33
        assert torch.equal(off, torch.arange(ns + 1, dtype=torch.int64, device="cuda") * nr)
        assert_radix(hj)


# ------------------------------------------------------------------ state
def _sorted(cnt, *cols):
    m = int(cnt.item())
    a = [c[:m].cpu().numpy() for c in cols]
    o = np.lexsort(tuple(reversed(a)))
    return [c[o] for c in a]


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_one_build_serves_every_probe(hj, oracle, strategy):
    """inner -> expand -> lookup -> full -> expand -> inner of one build: each
    result equals its first occurrence and the repeat flag keeps its answer."""
    rk, sk = mixed_case(oracle, True)
    rp = payloads(rk, 41)
    n = len(sk)
    d_sk, d_sp = dev(sk), dev(np.arange(n, dtype=np.int64))
    cap = int(OC.Expect(rk, sk).m("full")) + 8
    o_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    o_s = torch.empty_like(o_r)
    l_r = torch.empty(n, dtype=torch.int64, device="cuda")
    l_c = torch.empty(n, dtype=torch.int32, device="cuda")

    def inner():
        return _sorted(hj.probe_relation(d_sk, d_sp, o_r, o_s), o_r, o_s)

    def full():
        return _sorted(hj.probe_full(d_sk, d_sp, o_r, o_s, kind="full", null_r=NULL, null_s=NULL), o_r, o_s)

    def lookup():
        hj.probe_lookup(d_sk, l_r, l_c, null=NULL)
        return [l_r.cpu().numpy(), l_c.cpu().numpy()]

    def expand():
        e = check(hj, rk, rp, sk, "outer", d_sk=d_sk)
        m, off, vals = probe(hj, sk, "outer", e.m, d_sk)
        return [off[:n + 1], e.sorted_within(vals)]

    with radix(hj, 10, strategy):
        build(hj, rk, rp)
        first = {"inner": inner()}
        dups = hj.has_duplicates()
        assert dups
        first["expand"] = expand()
        first["lookup"] = lookup()
        first["full"] = full()
        assert hj.join_kernel != "k_join_expand"
        for name, f in (("expand", expand), ("inner", inner), ("lookup", lookup), ("full", full)):
            again = f()
            assert all(np.array_equal(a, b) for a, b in zip(first[name], again)), name
        assert np.array_equal(first["lookup"][1], XC.ExpandExpect(rk, rp, sk, "inner", NULL).cnt)
        assert len(first["inner"][0]) == OC.Expect(rk, sk).pairs
        assert hj.has_duplicates() == dups
        # and a build without repeats keeps saying so after an expand
        uk = np.arange(12000, dtype=np.int64) * 5
        up = payloads(uk, 42)
        build(hj, uk, up)
        check(hj, uk, up, sk, "inner")
        assert not hj.has_duplicates()


# ------------------------------------------------------------------ graph
@pytest.mark.parametrize("n", [5000, 70000])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_graph_replay(hj, oracle, strategy, n):
    """A captured expand (a linear graph of kernels), replayed twice over new probe keys."""
    rk = oracle.gen_pkfk_i64(61, n, n, 1.0)[0].copy()
    rk[::97] = rk[1::97]   # some build keys twice
    sets = [oracle.gen_pkfk_i64(61, n, n, f)[2] for f in (1.0, 0.5, 0.1)]
    rp = payloads(rk, 61)
    cap = 2 * n + 16
    sk = torch.empty(n, dtype=torch.int64, device="cuda")

    def load(keys):
        sk.copy_(torch.from_numpy(np.ascontiguousarray(keys)))
        torch.cuda.synchronize()

    g = None
    with radix(hj, 0, strategy):
        try:
            hj.allocate_hash_table(n, 64)
            build(hj, rk, rp)
            hj.reserve_probe(n, 64)
            hj.reserve_expand(n, 64)
            off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            o_r = torch.empty(cap, dtype=torch.int64, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            load(sets[0])
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):   # one eager step on the capture stream first
                hj.probe_expand(sk, off, o_r, how="outer", null=NULL, count=cnt)
            torch.cuda.synchronize()
            eager = (int(cnt.item()), off.cpu().numpy(), o_r.cpu().numpy())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                hj.probe_expand(sk, off, o_r, how="outer", null=NULL, count=cnt)
            torch.cuda.synchronize()
            assert hj.strategy_used == strategy
            for keys in sets[1:] + sets[:1]:
                load(keys)
                off.fill_(SENTINEL)
                o_r.fill_(SENTINEL)
                cnt.fill_(SENTINEL)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                e = XC.ExpandExpect(rk, rp, keys, "outer", NULL)
                assert int(cnt.item()) == e.m
                assert np.array_equal(off.cpu().numpy(), e.off)
                vals = o_r.cpu().numpy()
                assert e.same_values(vals) and (vals[e.m:] == SENTINEL).all()
            # the last replay ran over the first set again: the eager result, offsets exactly
            assert eager[0] == e.m and np.array_equal(eager[1], e.off)
            assert np.array_equal(e.sorted_within(eager[2]), e.sorted_within(vals))
        finally:
            del g
            torch.cuda.synchronize()


# ------------------------------------------------------------------ python
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_ordered_join_is_the_pandas_order_merge(hj, oracle, strategy):
    """ordered_join(how='left') over a unique-key build equals numpy with no sorting at all."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(31, 3000, 9000, 0.4)
    rp = payloads(rk, 31)
    sp = np.arange(len(sk), dtype=np.int64) * 2 + 5
    e = XC.ExpandExpect(rk, rp, sk, "outer", NULL)
    assert e.unique and 0 < (e.cnt == 0).sum() < len(sk)
    with radix(hj, 5, strategy):
        g_r, g_s = hj.ordered_join(dev(rk), dev(rp), dev(sk), dev(sp), how="left", null=NULL)
        assert hj.strategy_used == strategy
        assert np.array_equal(g_r.cpu().numpy(), e.r) and np.array_equal(g_s.cpu().numpy(), sp[e.seg])
        ei = XC.ExpandExpect(rk, rp, sk, "inner", NULL)
        g_r, g_s = hj.ordered_join(dev(rk), dev(rp), dev(sk), how="inner")
        assert np.array_equal(g_r.cpu().numpy(), ei.r) and np.array_equal(g_s.cpu().numpy(), ei.seg)
        off, vals = hj.expand(dev(rk), dev(rp), dev(sk), how="outer", null=NULL)
        assert np.array_equal(off.cpu().numpy(), e.off) and np.array_equal(vals.cpu().numpy(), e.r)
        # i32: R's row ids
        r32, s32 = rk.astype(np.int32), sk.astype(np.int32)
        e32 = XC.ExpandExpect(r32, payloads(r32), s32, "outer", -1)
        g_r, g_s = hj.ordered_join(dev(r32), None, dev(s32), how="left")
        assert g_r.dtype == torch.int32 and np.array_equal(g_r.cpu().numpy().astype(np.int64), e32.r)
        assert np.array_equal(g_s.cpu().numpy(), e32.seg)


def test_errors_in_order():
    """null context; kind; no build of that layout; null count pointer, bad
    relation, null offsets, bad outputs; (a build past INT32_MAX rows: not
    reachable at test sizes;) i32: n > INT32_MAX."""
    h = HashJoin(0)
    try:
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = torch.zeros(4, dtype=torch.int64, device="cuda")
        k32 = k.to(torch.int32)
        off = torch.zeros(5, dtype=torch.int64, device="cuda")
        o32 = torch.zeros(4, dtype=torch.int32, device="cuda")
        P = lambda t: t.data_ptr()   # noqa: E731
        ARG, STATE = _lib.HJ_ERR_ARG, _lib.HJ_ERR_STATE
        f64, f32 = lib.hj_dev_expand_i64, lib.hj_dev_expand_i32
        assert f64(None, 7, None, -1, -1, None, None, -1, None, None) == ARG
        assert b"null context" in lib.hj_last_error()
        assert f64(h._ctx, 7, None, -1, -1, None, None, -1, None, None) == ARG
        assert b"kind" in lib.hj_last_error()
        assert f64(h._ctx, 1, None, -1, -1, None, None, -1, None, None) == STATE
        h.build_table(k32)
        assert f64(h._ctx, 0, P(k), 4, -1, P(off), None, 0, P(cnt), None) == STATE   # an i32 build
        assert f32(h._ctx, 0, None, 4, -1, None, None, -1, None, None) == ARG
        assert b"count pointer" in lib.hj_last_error()
        assert f32(h._ctx, 0, None, 4, -1, None, None, -1, P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert f32(h._ctx, 0, P(k32), 4, -1, None, None, -1, P(cnt), None) == ARG
        assert b"offsets" in lib.hj_last_error()
        assert f32(h._ctx, 0, P(k32), 4, -1, P(off), None, -1, P(cnt), None) == ARG
        assert b"bad output" in lib.hj_last_error()
        # (refused before any row is read: the buffers hold 4 rows)
        assert f32(h._ctx, 0, P(k32), 1 << 31, -1, P(off), P(o32), 4, P(cnt), None) == ARG
        assert b"2^31" in lib.hj_last_error()
        with pytest.raises(ValueError):
            h.probe_expand(k32, off[:4])                   # n + 1 offsets
        with pytest.raises(ValueError):
            h.probe_expand(k32, off, out_r=k)              # the key's dtype
        with pytest.raises(KeyError):
            h.probe_expand(k32, off, how="left")           # the raw call's kinds are inner / outer
        with pytest.raises(ValueError):
            h.ordered_join(k, k, k, how="outer")
    finally:
        h.close()


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_reports_expand(hj, oracle, strategy):
    rk, _, sk, _ = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    rp = payloads(rk, 51)
    timing_reports(hj, strategy, lambda: build(hj, rk, rp), [lambda: check(hj, rk, rp, sk, "inner")])
