"""Probe-side outer join (LEFT OUTER, hj_dev_probe_outer_*) on both strategies
and both row widths.

Expected results never come from the library: the pairs from the oracle's
chained join (int64) or a numpy sort-merge (i32, empty sides), plus
(null, S.pay[~np.isin(S.key, R.key)]), compared as sorted multisets; M is
also held against count_outer."""
from collections import Counter

import numpy as np
import pytest
import torch

import outer_cases as OC
import routed_layout as RL
from join_gpu import dev, glob_hj, graph_replay, hj, host, radix, timing_reports  # noqa: F401

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
RADIX_KERNELS = ("k_join_b", "k_join_u_stream", "k_join_grp")


def assert_radix(hj):
    assert hj.strategy_used == "radix"
    assert hj.join_kernel in RADIX_KERNELS


def build(hj, rk, rp=None):
    if rk.dtype == np.int32:
        hj.build_table(dev(rk))
    else:
        hj.build_table(dev(rk), dev(np.arange(len(rk), dtype=np.int64) if rp is None else rp))


def np_join(rk, rp, sk, sp):
    """Every (rp[i], sp[j]) with rk[i] == sk[j], by sorting R (numpy only)."""
    o = np.argsort(rk, kind="stable")
    rs = rk[o]
    lo, hi = np.searchsorted(rs, sk, "left"), np.searchsorted(rs, sk, "right")
    c = hi - lo
    si = np.repeat(np.arange(len(sk)), c)
    off = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
    ri = o[np.repeat(lo, c) + off]
    return rp[ri].astype(np.int64), sp[si].astype(np.int64)


def expected(oracle, rk, rp, sk, sp, null):
    """(R.pay or null, S.pay) of the outer join and its unmatched-row count."""
    if rk.dtype == np.int64 and len(rk) and len(sk):
        er, es = oracle.chained_join_i64(rk, rp, sk, sp)
    else:
        er, es = np_join(rk, rp, sk, sp)
    un = ~np.isin(sk, rk)
    n_un = int(un.sum())
    return (np.concatenate([er, np.full(n_un, null, np.int64)]),
            np.concatenate([es, sp[un].astype(np.int64)]), n_un)


def probe(hj, sk, sp, null, row_base=0, cap=None):
    """One outer probe of the current build into outputs of `cap` rows (default: found by counting)."""
    wide = sk.dtype == np.int64
    d_sk = dev(sk)
    if cap is None:
        cap = max(1, hj.count_outer(d_sk))
    dt = torch.int64 if wide else torch.int32
    out_r = torch.full((cap,), -7, dtype=dt, device="cuda")
    out_s = torch.full_like(out_r, -7)
    cnt = hj.probe_outer(d_sk, dev(sp) if wide else None, out_r, out_s, null=null, row_base=row_base)
    m = int(cnt.item())
    assert len(sk) <= m <= cap, (m, len(sk), cap)
    return out_r[:m].cpu().numpy().astype(np.int64), out_s[:m].cpu().numpy().astype(np.int64)


def check_outer(hj, oracle, rk, sk, rp=None, sp=None, null=-1, row_base=0):
    """The outer probe of the current build (of rk, rp) against the expected multiset."""
    if rp is None:
        rp = np.arange(len(rk), dtype=np.int64)
    if sp is None:
        sp = row_base + np.arange(len(sk), dtype=np.int64)
    er, es, n_un = expected(oracle, rk, rp, sk, sp, null)
    assert len(er) >= len(sk)
    assert hj.count_outer(dev(sk)) == len(er)
    gr, gs = probe(hj, sk, sp, null, row_base)
    assert len(gr) == len(er), (len(gr), len(er))
    assert oracle.same_multiset(gr, gs, er, es)
    assert int((gr == null).sum()) >= n_un
    return n_un


# ------------------------------------------------------------------ global
@pytest.mark.parametrize("nr", [1, 1000, 2048, 3000])   # 2048: the last LDS-resident table
def test_global_pkfk_i64(glob_hj, oracle, nr):
    ns = (1 << 16) + 37   # a ragged last 2048-row tile
    rk, rp, sk, sp = oracle.gen_pkfk_i64(100 + nr, nr, ns, 0.6)
    build(glob_hj, rk, rp)
    n_un = check_outer(glob_hj, oracle, rk, sk, rp, sp)
    assert 0 < n_un < ns
    assert glob_hj.strategy_used == "global"
    assert glob_hj.join_kernel is None


@pytest.mark.parametrize("nr", [4000, 5000])   # either side of a 64-KiB table
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    build(glob_hj, r)
    assert check_outer(glob_hj, oracle, r, s, row_base=7, null=-1) > 0


def test_global_repeated_build_keys(glob_hj, oracle):
    """The general path: tiles with multi-match rows, and rows without a match inside them."""
    rk, rp = oracle.gen_uniform_i64(11, 1, 1, 300, 1000)
    sk, sp = oracle.gen_uniform_i64(11, 2, 1, 400, 1 << 16)
    build(glob_hj, rk, rp)
    assert glob_hj.has_duplicates()
    assert check_outer(glob_hj, oracle, rk, sk, rp, sp) > 0
    assert glob_hj.has_duplicates()


@pytest.mark.parametrize("where", ["probe", "both", "build"])
def test_global_int64_min(glob_hj, oracle, where):
    rk, rp = oracle.gen_uniform_i64(12, 1, -2000, 2000, 1500)
    sk, sp = oracle.gen_uniform_i64(12, 2, -3000, 3000, 1 << 15)
    if where in ("both", "build"):
        rk[::500] = I64_MIN
    if where in ("both", "probe"):
        sk[::1777] = I64_MIN
    build(glob_hj, rk, rp)
    null = -77
    assert not (rp == null).any()
    check_outer(glob_hj, oracle, rk, sk, rp, sp, null=null)
    if where == "probe":   # no INT64_MIN build row: each such probe row is one null row
        gr, gs = probe(glob_hj, sk, sp, null)
        rows = gr[np.isin(gs, sp[::1777])]
        assert len(rows) == len(sp[::1777]) and (rows == null).all()


def test_global_null_value_is_passed_through(glob_hj, oracle):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(14, 3000, 20000, 0.5)
    build(glob_hj, rk, rp)
    null = I64_MIN + 5
    n_un = check_outer(glob_hj, oracle, rk, sk, rp, sp, null=null)
    gr, _ = probe(glob_hj, sk, sp, null)
    assert int((gr == null).sum()) == n_un > 0 and not (gr == -1).any()


@pytest.mark.parametrize("kind", ["outer", "outer-count"])
def test_global_general_path_strides(glob_hj, kind):
    """Every probe tile is handed to the general path, 60 more of them than
    k_probe_slow's persistent workgroups, the slow list filled to its exact
    tile count: the OUTER general path takes a second tile -- exact M, exact rows."""
    c = OC.strided_general_case(torch.cuda.get_device_properties(0).multi_processor_count)
    e, nr, ns = c["exp"], len(c["rk"]), len(c["sk"])
    rp, sp = np.arange(nr, dtype=np.int64) + OC.R_OFF, np.arange(ns, dtype=np.int64) + OC.S_OFF
    glob_hj.build_table(dev(c["rk"]), dev(rp))
    d_sk, m = dev(c["sk"]), e.m("outer")
    if kind == "outer-count":
        assert glob_hj.count_outer(d_sk) == m
        assert glob_hj.strategy_used == "global"
        return
    out_r = torch.full((m + 64,), -7, dtype=torch.int64, device="cuda")
    out_s = torch.full_like(out_r, -7)
    got = int(glob_hj.probe_outer(d_sk, dev(sp), out_r, out_s, null=-1).item())
    assert glob_hj.strategy_used == "global"
    assert got == m
    g_r, g_s = out_r.cpu().numpy(), out_s.cpu().numpy()
    assert (g_r[m:] == -7).all() and (g_s[m:] == -7).all()
    assert OC.same_rows(g_r[:m], g_s[:m], *e.rows("outer", rp, sp, -1, -2), -1, -2)


# ------------------------------------------------------------------ radix
@pytest.mark.parametrize("bits", [1, 3, 9, 12, 17])   # 1-, 2- and 3-pass plans
def test_radix_pkfk(hj, oracle, bits):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(bits, 20000, 30000, 0.7)
    radix(hj, bits)
    try:
        build(hj, rk, rp)
        assert check_outer(hj, oracle, rk, sk, rp, sp, null=I64_MIN + 5) > 0
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_partitions_without_build_rows(hj, oracle):
    """2^10 partitions, 50 build rows: most partitions hold probe rows only --
    exactly the null rows (the second stage's work map must keep them)."""
    rk = np.arange(50, dtype=np.int64) * 1000003 + 17
    rng = np.random.default_rng(5)
    sk = rng.integers(1 << 40, 1 << 41, 30000, dtype=np.int64)
    hit = rng.random(30000) < 0.5
    sk[hit] = rk[rng.integers(0, 50, int(hit.sum()))]
    sp = np.arange(30000, dtype=np.int64) * 3
    radix(hj, 10)
    try:
        build(hj, rk)
        n_un = check_outer(hj, oracle, rk, sk, sp=sp)
        assert 0.4 < n_un / 30000 < 0.6
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_build_key_rounds(hj, oracle):
    """20000 copies of one build key: a matching probe row comes out 20000
    times and never as a null row; an unmatched one exactly once."""
    rk = np.concatenate([np.full(20000, 42, np.int64), np.arange(1000, 3000, dtype=np.int64)])
    sk = np.array([42, 7, 42, 2500, 99999], np.int64)
    sp = np.arange(5, dtype=np.int64)
    radix(hj, 4)
    try:
        build(hj, rk)
        check_outer(hj, oracle, rk, sk, sp=sp)
        gr, gs = probe(hj, sk, sp, -1)
        assert np.bincount(gs, minlength=5).tolist() == [20000, 1, 20000, 1, 1]
        assert sorted(gs[gr == -1].tolist()) == [1, 4]
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_distinct_keys_over_one_round(hj, oracle):
    """60000 distinct build keys in 2 partitions: multi-round items, where an S
    row unmatched in round 1 must not be emitted before the last round."""
    rk, rp, sk, sp = oracle.gen_pkfk_i64(77, 60000, 40000, 0.5)
    assert len(np.unique(rk)) == 60000
    radix(hj, 1)
    try:
        build(hj, rk, rp)
        check_outer(hj, oracle, rk, sk, rp, sp)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_probe_key_many_chunks(hj, oracle):
    rk = np.arange(3000, dtype=np.int64) * 7
    sk = np.concatenate([np.full(50000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    radix(hj, 6)
    try:
        build(hj, rk)
        check_outer(hj, oracle, rk, sk)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_int64_min_both_sides(hj, oracle):
    rk, rp = oracle.gen_uniform_i64(3, 1, -100, 100, 5000)
    sk, sp = oracle.gen_uniform_i64(3, 2, -100, 100, 4000)
    rk[::97] = I64_MIN
    sk[::131] = I64_MIN
    sp = np.arange(4000, dtype=np.int64)
    null = -9
    radix(hj, 5)
    try:
        build(hj, rk, rp)
        check_outer(hj, oracle, rk, sk, rp, sp, null=null)
        assert_radix(hj)
        # and with no INT64_MIN on the build side those probe rows are null rows
        keep = rk != I64_MIN
        build(hj, rk[keep], rp[keep])
        check_outer(hj, oracle, rk[keep], sk, rp[keep], sp, null=null)
        gr, gs = probe(hj, sk, sp, null)
        rows = gr[np.isin(gs, sp[::131])]
        assert len(rows) == len(sp[::131]) and (rows == null).all()
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_empty_and_tiny(hj, oracle):
    e = np.empty(0, np.int64)
    k = np.array([5, 9, 5, 3], np.int64)
    one, other = np.array([4], np.int64), np.array([6], np.int64)
    radix(hj, 3)
    try:
        for rk, sk in [(e, k), (k, e), (one, one), (one, other)]:
            build(hj, rk)
            n_un = check_outer(hj, oracle, rk, sk, sp=np.arange(len(sk), dtype=np.int64) + 100)
            if len(rk) == 0:
                assert n_un == len(sk)   # R empty: every S row is a null row
            assert_radix(hj)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("bits", [1, 9])
def test_radix_i32(hj, oracle, bits):
    r = oracle.gen_uniform_i32(bits, 1, -(1 << 31), (1 << 31) - 1, 30000)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(bits, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    radix(hj, bits)
    try:
        build(hj, r)
        assert check_outer(hj, oracle, r, s, row_base=7, null=-1) > 0
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


# ------------------------------------------------------------------ both strategies
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_tuples_form_equals_columns(hj, oracle, strategy):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(21, 5000, 20011, 0.5)
    hj.set_strategy(strategy, radix_bits=7 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        cr, cs = probe(hj, sk, sp, -3)
        out_r = torch.empty(len(cr), dtype=torch.int64, device="cuda")
        out_s = torch.empty_like(out_r)
        m = int(hj.probe_outer_tuples(dev(np.stack([sk, sp], axis=1)), out_r, out_s, null=-3).item())
        assert m == len(cr) == len(expected(oracle, rk, rp, sk, sp, -3)[0])
        assert oracle.same_multiset(out_r.cpu().numpy(), out_s.cpu().numpy(), cr, cs)
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


# (strategy, S rows, hit fraction): global; radix with the pairs alone past the
# capacity; radix with pairs < capacity < M, so the boundary falls inside the
# unmatched-rows stage
@pytest.mark.parametrize("strategy,ns,frac", [("global", 1 << 16, 0.6), ("radix", 30000, 0.7), ("radix", 30000, 0.02)],
                         ids=["global", "radix-pairs-over-cap", "radix-cap-in-second-stage"])
def test_capacity(hj, oracle, strategy, ns, frac):
    cap, sentinel, null = 1000, -12345, -1
    rk, rp, sk, sp = oracle.gen_pkfk_i64(13, 3000 if strategy == "global" else 20000, ns, frac)
    er, es, n_un = expected(oracle, rk, rp, sk, sp, null)
    pairs = len(er) - n_un
    assert len(er) > cap and (pairs > cap if frac > 0.1 else 0 < pairs < cap)
    hj.set_strategy(strategy, radix_bits=6 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        back_r = torch.full((cap + 4096,), sentinel, dtype=torch.int64, device="cuda")
        back_s = torch.full_like(back_r, sentinel)
        m = int(hj.probe_outer(dev(sk), dev(sp), back_r[:cap], back_s[:cap], null=null).item())
        assert m == len(er)
        got_r, got_s = back_r.cpu().numpy(), back_s.cpu().numpy()
        assert (got_r[cap:] == sentinel).all() and (got_s[cap:] == sentinel).all()
        extra = Counter(zip(got_r[:cap].tolist(), got_s[:cap].tolist())) - Counter(zip(er.tolist(), es.tolist()))
        assert not extra, list(extra.items())[:5]
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


def _fuzz_cases():
    rng = np.random.default_rng(0x0A7E2)
    units = [1, 63, 64, 65, 511, 513, 2047, 2049, 3071, 3073, 4097, 8193, 12289, 40000]
    cases = []
    for i in range(12):
        nr = min(40000, int(rng.choice(units)) + int(rng.integers(0, 3)))
        ns = min(40000, int(rng.choice(units)) * int(rng.integers(1, 4)))
        span = int(rng.choice([64, 1000, 1 << 20, 1 << 40]))
        bits = int(rng.choice([1, 4, 7, 9, 12, 17]))
        cases.append((i, nr, ns, span, bits))
    return cases


@pytest.mark.parametrize("i,nr,ns,span,bits", _fuzz_cases())
def test_fuzz_ragged(hj, oracle, i, nr, ns, span, bits):
    rng = np.random.default_rng(3000 + i)
    try:
        for wide in (True, False):
            sp_ = span if wide else min(span, 1 << 30)
            lo = -sp_ // 2
            rk = rng.integers(lo, lo + sp_, nr, dtype=np.int64)
            sk = rng.integers(lo, lo + sp_, ns, dtype=np.int64)
            hit = rng.random(ns) < 0.5
            sk[hit] = rk[rng.integers(0, nr, int(hit.sum()))]
            if wide:
                sp, base, null = rng.integers(-(1 << 62), 1 << 62, ns, dtype=np.int64), 0, I64_MIN + 5
            else:
                rk, sk, sp, base, null = rk.astype(np.int32), sk.astype(np.int32), None, i, -1
            radix(hj, bits)
            build(hj, rk)
            check_outer(hj, oracle, rk, sk, sp=sp, null=null, row_base=base)
            assert_radix(hj)
            hj.set_strategy("global")
            build(hj, rk)
            check_outer(hj, oracle, rk, sk, sp=sp, null=null, row_base=base)
            assert hj.strategy_used == "global"
    finally:
        hj.set_strategy("auto")


# ------------------------------------------------------------------ interaction
def _sorted(r, s):
    o = np.lexsort((s, r))
    return r[o], s[o]


def _inner(hj, sk, sp, cap):
    out_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    out_s = torch.empty_like(out_r)
    m = int(hj.probe_relation(dev(sk), dev(sp), out_r, out_s).item())
    assert m <= cap
    return _sorted(out_r[:m].cpu().numpy(), out_s[:m].cpu().numpy())


def _exists(hj, sk, sp, kind):
    out_s = torch.empty(len(sk), dtype=torch.int64, device="cuda")
    m = int(hj.probe_exists(dev(sk), dev(sp), kind, out_s).item())
    return np.sort(out_s[:m].cpu().numpy())


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_one_build_serves_inner_outer_semi_anti(hj, oracle, strategy):
    rk, rp = oracle.gen_uniform_i64(41, 1, 1, 500, 12000)
    sk, _ = oracle.gen_uniform_i64(41, 2, 1, 600, 9000)
    sp = np.arange(9000, dtype=np.int64)
    er, es, n_un = expected(oracle, rk, rp, sk, sp, -1)
    mask = np.isin(sk, rk)
    hj.set_strategy(strategy, radix_bits=10 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        inner1 = _inner(hj, sk, sp, len(er))
        dups = hj.has_duplicates()
        assert dups
        outer1 = _sorted(*probe(hj, sk, sp, -1))
        if strategy == "radix":
            assert_radix(hj)   # (not k_join_exists: the kernel that produced the pairs)
        assert np.array_equal(_exists(hj, sk, sp, "semi"), sp[mask])
        assert np.array_equal(_exists(hj, sk, sp, "anti"), sp[~mask])
        outer2 = _sorted(*probe(hj, sk, sp, -1))
        inner2 = _inner(hj, sk, sp, len(er))
        assert np.array_equal(inner1[0], inner2[0]) and np.array_equal(inner1[1], inner2[1])
        assert np.array_equal(outer1[0], outer2[0]) and np.array_equal(outer1[1], outer2[1])
        assert len(inner1[0]) == len(er) - n_un and n_un > 0
        assert oracle.same_multiset(outer1[0], outer1[1], er, es)
        assert hj.has_duplicates() == dups
        assert hj.strategy_used == strategy
        # a duplicate-free build keeps saying so after an outer probe
        uk = np.arange(12000, dtype=np.int64) * 5
        build(hj, uk)
        check_outer(hj, oracle, uk, sk, sp=sp)
        assert not hj.has_duplicates()
    finally:
        hj.set_strategy("auto")


def test_auto_dual_build_picks_strategy_by_probe_size(hj):
    hj.set_strategy("auto")
    hj.probe_hint(None)
    nr, ns, null = 1 << 18, 1 << 24, -1
    rk = torch.arange(nr, dtype=torch.int64, device="cuda") * 2
    rp = torch.arange(nr, dtype=torch.int64, device="cuda") * 5 + 2
    hj.build_table(rk, rp)
    sk = torch.arange(ns, dtype=torch.int64, device="cuda") % (1 << 19)
    sp = torch.arange(ns, dtype=torch.int64, device="cuda") * 3 + 1
    mask = (sk % 2) == 0   # (R holds the even keys below 2^19, each once)
    want_r = torch.where(mask, (sk // 2) * 5 + 2, torch.full_like(sk, null))

    def digest(t):
        return int(t.sum().item()), int((t ^ (t >> 7)).sum().item())

    out_r = torch.empty(ns, dtype=torch.int64, device="cuda")
    out_s = torch.empty_like(out_r)
    m = int(hj.probe_outer(sk, sp, out_r, out_s, null=null).item())
    assert hj.strategy_used == "radix"
    assert m == ns and int(mask.sum().item()) == ns // 2
    assert digest(out_s) == digest(sp) and digest(out_r) == digest(want_r)
    # each pair is the right one, not only each column: R.pay + 7 * S.pay
    assert digest(out_r + 7 * out_s) == digest(want_r + 7 * sp)
    small = 1 << 12
    m = int(hj.probe_outer(sk[:small], sp[:small], out_r[:small], out_s[:small], null=null).item())
    assert hj.strategy_used == "global"
    assert hj.join_kernel is None
    assert m == small
    o = torch.argsort(out_s[:small])
    assert torch.equal(out_s[:small][o], sp[:small]) and torch.equal(out_r[:small][o], want_r[:small])


def test_outer_probe_after_routed_build(hj, oracle):
    """After a routed build an outer probe over unrouted rows is valid, like hj_dev_probe_i64."""
    N, sub, q = 4, 3, 1
    rk, rp, sk, sp = oracle.gen_pkfk_i64(360, 40000, 60000, 0.6)
    R = RL.Routed(hj, dev(rk), dev(rp), N, sub)
    t, c = R.received(q)
    hj.build_routed(t, c, N, sub)
    g = N.bit_length() - 1
    own_r, own_s = RL.rparts(rk, g) == q, RL.rparts(sk, g) == q
    mk, mp = sk[own_s], sp[own_s]
    n_un = check_outer(hj, oracle, rk[own_r], mk, rp[own_r], mp, null=-5)
    assert 0 < n_un < len(mk)
    assert_radix(hj)


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_reports_outer_probes(hj, oracle, strategy):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    timing_reports(hj, strategy, lambda: build(hj, rk, rp), [lambda: probe(hj, sk, sp, -1, cap=len(sk))])


@pytest.mark.parametrize("n,strategy,wide", [(1 << 16, "radix", True), (1 << 12, "global", False)],
                         ids=["i64-2^16-radix", "i32-2^12-global"])
def test_graph_replay(hj, oracle, n, strategy, wide):
    kt = torch.int64 if wide else torch.int32
    rk = torch.empty(n, dtype=kt, device="cuda")
    sk = torch.empty(n, dtype=kt, device="cuda")
    rp = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 2 if wide else None
    sp = torch.arange(n, dtype=torch.int64, device="cuda") * 2 + 1 if wide else None
    grp = None
    if wide:
        sets = [oracle.gen_pkfk_i64(61 + j, n, n, f)[0::2] for j, f in enumerate((1.0, 0.5, 0.1, 0.8))]
        if strategy == "radix":   # the replays also leave k_join_b and fill the deferral lists
            grp, with_nulls = OC.replay_sets_other_kernels(oracle, n, 8 * n)
            sets += [grp, with_nulls]
    else:
        sets = [(oracle.gen_uniform_i32(65 + j, 1, 1, hi, n), oracle.gen_uniform_i32(65 + j, 2, 1, hi, n))
                for j, hi in enumerate((4 * n, n // 4, 1 << 30, 2 * n))]

    def load(data):
        rk.copy_(torch.from_numpy(np.ascontiguousarray(data[0])))
        sk.copy_(torch.from_numpy(np.ascontiguousarray(data[1])))
        torch.cuda.synchronize()

    bits, cap = 64 if wide else 32, 8 * n
    out_r = torch.empty(cap, dtype=kt, device="cuda")
    out_s = torch.empty_like(out_r)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    pay_r = np.arange(n, dtype=np.int64) * 3 + 2 if wide else np.arange(n, dtype=np.int64)
    pay_s = np.arange(n, dtype=np.int64) * 2 + 1 if wide else np.arange(n, dtype=np.int64)

    def setup():
        load(sets[0])
        hj.allocate_hash_table(n, bits)
        hj.build_table(rk, rp)
        hj.reserve_probe(n, bits)

    def step():
        hj.build_table(rk, rp)
        hj.probe_outer(sk, sp, out_r, out_s, null=-1, count=cnt)

    def reload(data):
        load(data)
        out_r.fill_(-9)
        cnt.zero_()

    def verify(data):
        m = int(cnt.item())
        er, es = np_join(data[0], pay_r, data[1], pay_s)
        un = ~np.isin(data[1], data[0])
        er, es = np.concatenate([er, np.full(int(un.sum()), -1, np.int64)]), np.concatenate([es, pay_s[un]])
        assert m == len(er) <= cap
        assert oracle.same_multiset(host(out_r[:m]), host(out_s[:m]), er, es)
        if data is grp:   # the replay chose its kernel from this data, on the device
            assert m < cap and hj.join_kernel == "k_join_grp"

    graph_replay(hj, strategy, setup, step, sets[1:], reload, verify)


def test_outer_join_method(hj, oracle):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(31, 3000, 9000, 0.3)
    er, es, n_un = expected(oracle, rk, rp, sk, sp, -1)
    r, s = hj.outer_join(dev(rk), dev(rp), dev(sk), dev(sp), capacity=10)   # one re-probe at the exact M
    assert oracle.same_multiset(r.cpu().numpy(), s.cpu().numpy(), er, es)
    r, s = hj.outer_join(dev(rk), dev(rp), dev(sk), dev(sp), null=I64_MIN + 5)
    assert int((r == I64_MIN + 5).sum().item()) == n_un
    r32, s32 = rk.astype(np.int32), sk.astype(np.int32)
    r, s = hj.outer_join(dev(r32), None, dev(s32))
    assert r.dtype == torch.int32 and s.dtype == torch.int32
    e32 = expected(oracle, r32, np.arange(3000, dtype=np.int64), s32, np.arange(9000, dtype=np.int64), -1)
    assert oracle.same_multiset(r.cpu().numpy().astype(np.int64), s.cpu().numpy().astype(np.int64), e32[0], e32[1])
