"""Build-side and full outer join (RIGHT / FULL OUTER, hj_dev_probe_full_*) on
both strategies and both row widths.

Expected results never come from the library: the pairs from the oracle's
chained join (int64) or a numpy sort-merge (i32, empty sides), R's null rows
(R.pay[~np.isin(R.key, S.key)], null_s) and, for the full kind, S's null rows
(null_r, S.pay[~np.isin(S.key, R.key)]), compared as sorted multisets; M is
also held against count_full."""
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
KINDS = ("full", "build")


def assert_radix(hj):
    assert hj.strategy_used == "radix"
    assert hj.join_kernel in RADIX_KERNELS   # the kernel that produced the pairs


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


class Exp:
    """The expected rows of one (R, S, kind): columns r, s and the three sizes."""

    def __init__(self, oracle, rk, rp, sk, sp, kind, null_r, null_s):
        if rk.dtype == np.int64 and len(rk) and len(sk):
            pr, ps = oracle.chained_join_i64(rk, rp, sk, sp)
        else:
            pr, ps = np_join(rk, rp, sk, sp)
        r_un = ~np.isin(rk, sk)
        s_un = ~np.isin(sk, rk) if kind == "full" else np.zeros(len(sk), bool)
        self.pairs, self.n_r, self.n_s = len(pr), int(r_un.sum()), int(s_un.sum())
        self.r = np.concatenate([pr, rp[r_un].astype(np.int64), np.full(self.n_s, null_r, np.int64)])
        self.s = np.concatenate([ps, np.full(self.n_r, null_s, np.int64), sp[s_un].astype(np.int64)])
        self.m = len(self.r)


def probe(hj, sk, sp, kind, null_r, null_s, row_base=0, cap=None):
    """One full probe of the current build into outputs of `cap` rows (default: found by counting)."""
    wide = sk.dtype == np.int64
    d_sk = dev(sk)
    if cap is None:
        cap = max(1, hj.count_full(d_sk, kind=kind))
    dt = torch.int64 if wide else torch.int32
    out_r = torch.full((cap,), -7, dtype=dt, device="cuda")
    out_s = torch.full_like(out_r, -7)
    cnt = hj.probe_full(d_sk, dev(sp) if wide else None, out_r, out_s, kind=kind, null_r=null_r, null_s=null_s,
                        row_base=row_base)
    m = int(cnt.item())
    assert 0 <= m <= cap, (m, cap)
    return out_r[:m].cpu().numpy().astype(np.int64), out_s[:m].cpu().numpy().astype(np.int64)


def check_full(hj, oracle, rk, sk, rp=None, sp=None, null_r=-1, null_s=-2, row_base=0, kinds=KINDS):
    """Both kinds of the full probe of the current build (of rk, rp) against
    the expected multisets; returns the full kind's Exp."""
    if rp is None:
        rp = np.arange(len(rk), dtype=np.int64)
    if sp is None:
        sp = row_base + np.arange(len(sk), dtype=np.int64)
    first = None
    for kind in kinds:
        e = Exp(oracle, rk, rp, sk, sp, kind, null_r, null_s)
        assert hj.count_full(dev(sk), kind=kind) == e.m
        gr, gs = probe(hj, sk, sp, kind, null_r, null_s, row_base)
        assert len(gr) == e.m, (kind, len(gr), e.m)
        assert oracle.same_multiset(gr, gs, e.r, e.s), kind
        first = first or e
    return first


# ------------------------------------------------------------------ global
@pytest.mark.parametrize("nr", [1, 1000, 2048, 3000])   # 2048: the last LDS-resident table
def test_global_pkfk_i64(glob_hj, oracle, nr):
    ns = 8 * nr + 37
    rk, rp, sk, sp = oracle.gen_pkfk_i64(200 + nr, nr, ns, 0.6)
    build(glob_hj, rk, rp)
    e = check_full(glob_hj, oracle, rk, sk, rp, sp)
    if nr > 1:
        assert 0 < e.n_r < nr and 0 < e.n_s < ns and e.pairs > nr - e.n_r   # some R rows unmatched, some matched twice
    assert glob_hj.strategy_used == "global"
    assert glob_hj.join_kernel is None


@pytest.mark.parametrize("nr", [4000, 5000])   # either side of a 64-KiB table
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    build(glob_hj, r)
    e = check_full(glob_hj, oracle, r, s, row_base=7)
    assert e.n_r > 0 and e.n_s > 0


def test_global_repeated_build_keys(glob_hj, oracle):
    """Every copy of a matched key is absent from R's null rows, every copy of
    an unmatched key present once; one key is repeated 200 times, so its
    copies are spread along a chain between other keys' slots."""
    rk, rp = oracle.gen_uniform_i64(11, 1, 1, 300, 1000)
    rk = np.concatenate([rk, np.full(200, 150, np.int64), np.full(200, 5000, np.int64)])
    rp = np.arange(len(rk), dtype=np.int64) + 10
    sk, _ = oracle.gen_uniform_i64(11, 2, 100, 400, 9000)   # keys 1..99 and 5000 of R stay unmatched
    sp = np.arange(9000, dtype=np.int64) + 50000
    assert (sk == 150).any()
    build(glob_hj, rk, rp)
    assert glob_hj.has_duplicates()
    e = check_full(glob_hj, oracle, rk, sk, rp, sp)
    assert e.n_r >= 200 and e.n_s > 0
    gr, gs = probe(glob_hj, sk, sp, "build", -1, -2)
    got = np.sort(gr[gs == -2])
    assert np.array_equal(got, np.sort(rp[~np.isin(rk, sk)]))   # each unmatched copy once, no matched copy
    assert not np.isin(rp[rk == 150], got).any() and np.isin(rp[rk == 5000], got).all()
    assert glob_hj.has_duplicates()


@pytest.mark.parametrize("where", ["build", "probe", "both"])
def test_global_int64_min(glob_hj, oracle, where):
    rk, rp = oracle.gen_uniform_i64(12, 1, -2000, 2000, 1500)
    sk, sp = oracle.gen_uniform_i64(12, 2, -3000, 3000, 1 << 14)
    if where in ("both", "build"):
        rk[::500] = I64_MIN
    if where in ("both", "probe"):
        sk[::1777] = I64_MIN
    build(glob_hj, rk, rp)
    null_r, null_s = -77, -78
    assert not (rp == null_r).any() and not (sp == null_s).any()
    check_full(glob_hj, oracle, rk, sk, rp, sp, null_r=null_r, null_s=null_s)
    gr, gs = probe(glob_hj, sk, sp, "full", null_r, null_s)
    side = rp[rk == I64_MIN]
    if where == "build":   # the side-list rows come out with null_s, once each
        rows = gs[np.isin(gr, side)]
        assert len(rows) == len(side) == 3 and (rows == null_s).all()
    if where == "both":    # matched: never with null_s
        assert not (gs[np.isin(gr, side)] == null_s).any()
    if where == "probe":   # no INT64_MIN build row: each such probe row is one null row
        rows = gr[np.isin(gs, sp[::1777])]
        assert len(rows) == len(sp[::1777]) and (rows == null_r).all()


def test_global_null_values_are_passed_through(glob_hj, oracle):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(14, 3000, 20000, 0.5)
    build(glob_hj, rk, rp)
    null_r, null_s = I64_MIN + 5, I64_MIN + 6
    e = check_full(glob_hj, oracle, rk, sk, rp, sp, null_r=null_r, null_s=null_s)
    gr, gs = probe(glob_hj, sk, sp, "full", null_r, null_s)
    assert int((gr == null_r).sum()) == e.n_s > 0 and int((gs == null_s).sum()) == e.n_r > 0
    gr, gs = probe(glob_hj, sk, sp, "build", null_r, null_s)   # null_r is ignored
    assert not (gr == null_r).any() and int((gs == null_s).sum()) == e.n_r


@pytest.fixture(scope="module")
def strided():
    """outer_cases.strided_general_case on the device: more handed-over tiles
    and more slot tiles than the general path's 8 x CUs persistent workgroups."""
    c = dict(OC.strided_general_case(torch.cuda.get_device_properties(0).multi_processor_count))
    nr, ns = len(c["rk"]), len(c["sk"])
    c["rp"], c["sp"] = np.arange(nr, dtype=np.int64) + OC.R_OFF, np.arange(ns, dtype=np.int64) + OC.S_OFF
    c["row_r"], c["row_s"] = np.arange(nr, dtype=np.int64), np.arange(ns, dtype=np.int64)   # i32: row ids
    c["d_rk"], c["d_rp"], c["d_sk"], c["d_sp"] = dev(c["rk"]), dev(c["rp"]), dev(c["sk"]), dev(c["sp"])
    return c


@pytest.mark.parametrize("kind", ["full", "build", "full-count", "build-count"])
def test_global_general_path_and_slot_scan_stride(glob_hj, strided, kind):
    """Every probe tile is handed to the general path, 60 more of them than
    k_probe_slow's / k_probe_mark's persistent workgroups, the slow list filled
    to its exact tile count; the table is more slot tiles than
    k_emit_unmatched's workgroups: each loop takes a second tile -- exact M, exact rows."""
    c, e = strided, strided["exp"]
    base = kind.split("-")[0]
    glob_hj.build_table(c["d_rk"], c["d_rp"])
    assert glob_hj.capacity == c["slots"]
    m = e.m(base)
    if kind.endswith("-count"):
        assert glob_hj.count_full(c["d_sk"], kind=base) == m
        assert glob_hj.strategy_used == "global"
        return
    out_r = torch.full((m + 64,), -7, dtype=torch.int64, device="cuda")
    out_s = torch.full_like(out_r, -7)
    got = int(glob_hj.probe_full(c["d_sk"], c["d_sp"], out_r, out_s, kind=base, null_r=-1, null_s=-2).item())
    assert glob_hj.strategy_used == "global"
    assert got == m
    g_r, g_s = out_r.cpu().numpy(), out_s.cpu().numpy()
    assert (g_r[m:] == -7).all() and (g_s[m:] == -7).all()
    assert OC.same_rows(g_r[:m], g_s[:m], *e.rows(base, c["rp"], c["sp"], -1, -2), -1, -2)


def test_global_general_path_and_slot_scan_stride_i32(glob_hj, strided):
    """The same shape for the i32 types (row ids for payloads), full kind."""
    c, e = strided, strided["exp"]
    glob_hj.build_table(dev(c["rk"].astype(np.int32)))
    assert glob_hj.capacity == c["slots"]
    m = e.m("full")
    d_sk = dev(c["sk"].astype(np.int32))
    out_r = torch.full((m + 64,), -7, dtype=torch.int32, device="cuda")
    out_s = torch.full_like(out_r, -7)
    got = int(glob_hj.probe_full(d_sk, None, out_r, out_s, kind="full", null_r=-1, null_s=-2).item())
    assert glob_hj.strategy_used == "global"
    assert got == m
    g_r, g_s = out_r.cpu().numpy().astype(np.int64), out_s.cpu().numpy().astype(np.int64)
    assert (g_r[m:] == -7).all() and (g_s[m:] == -7).all()
    assert OC.same_rows(g_r[:m], g_s[:m], *e.rows("full", c["row_r"], c["row_s"], -1, -2), -1, -2)


# ------------------------------------------------------------------ radix
@pytest.mark.parametrize("bits", [1, 3, 9, 12, 17])   # 1-, 2- and 3-pass plans
def test_radix_pkfk(hj, oracle, bits):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(bits, 20000, 30000, 0.7)
    radix(hj, bits)
    try:
        build(hj, rk, rp)
        e = check_full(hj, oracle, rk, sk, rp, sp, null_r=I64_MIN + 5, null_s=I64_MIN + 6)
        assert e.n_r > 0 and e.n_s > 0
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_partitions_without_probe_rows(hj, oracle):
    """2^10 partitions, 30000 build rows, 50 probe rows: most partitions hold
    build rows only -- exactly R's null rows (the new stage's work map must keep them)."""
    rng = np.random.default_rng(5)
    rk = rng.permutation(1 << 20)[:30000].astype(np.int64) * 1000003 + 17
    sk = np.concatenate([rk[rng.integers(0, 30000, 25)], rng.integers(1 << 50, 1 << 51, 25, dtype=np.int64)])
    sp = np.arange(50, dtype=np.int64) * 3
    radix(hj, 10)
    try:
        build(hj, rk)
        e = check_full(hj, oracle, rk, sk, sp=sp)
        assert e.n_r >= 30000 - 25 and e.n_s == 25
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_rounds_sub_chunks_and_items(hj, oracle):
    """Two partitions: 40000 distinct probe keys are several 5120-row build
    rounds of the exchanged stage (a build row unmatched in round 1 must not be
    emitted before the last round), and 60000 build rows are several
    sub-chunks and several work items per partition."""
    rk, rp, sk, sp = oracle.gen_pkfk_i64(77, 60000, 40000, 0.5)
    sk, i = np.unique(sk, return_index=True)
    sp = sp[i]
    extra = np.arange(40000 - len(sk), dtype=np.int64) + (1 << 45)   # distinct keys R does not hold
    sk, sp = np.concatenate([sk, extra]), np.concatenate([sp, extra])
    assert len(np.unique(sk)) == 40000 and len(np.unique(rk)) == 60000
    radix(hj, 1)
    try:
        build(hj, rk, rp)
        e = check_full(hj, oracle, rk, sk, rp, sp)
        assert e.n_r > 20000 and e.n_s > 0
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_probe_key(hj, oracle):
    """50000 copies of one probe key: one slot of the exchanged stage's table."""
    rk = np.arange(3000, dtype=np.int64) * 7
    sk = np.concatenate([np.full(50000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    radix(hj, 6)
    try:
        build(hj, rk)
        e = check_full(hj, oracle, rk, sk)
        assert e.n_r > 0
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_build_key(hj, oracle):
    """20000 copies of one build key matched by one S row: none is emitted as a
    null row; with that S row removed all 20000 are, once each."""
    rk = np.concatenate([np.full(20000, 42, np.int64), np.arange(1000, 3000, dtype=np.int64)])
    rp = np.arange(len(rk), dtype=np.int64)
    sk = np.array([7, 42, 2500, 99999], np.int64)
    sp = np.arange(4, dtype=np.int64) + 100000
    radix(hj, 4)
    try:
        build(hj, rk, rp)
        check_full(hj, oracle, rk, sk, rp, sp)
        gr, gs = probe(hj, sk, sp, "build", -1, -2)
        assert int((gs == 100001).sum()) == 20000
        assert not np.isin(gr[gs == -2], rp[:20000]).any()
        sk2, sp2 = np.delete(sk, 1), np.delete(sp, 1)
        check_full(hj, oracle, rk, sk2, rp, sp2)
        gr, gs = probe(hj, sk2, sp2, "build", -1, -2)
        assert np.array_equal(np.sort(gr[gs == -2])[:20000], rp[:20000])
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_int64_min(hj, oracle):
    rk, _ = oracle.gen_uniform_i64(3, 1, -100, 100, 5000)
    sk, _ = oracle.gen_uniform_i64(3, 2, -150, 50, 4000)
    rk[::97] = I64_MIN
    sk[::131] = I64_MIN
    rp = np.arange(5000, dtype=np.int64) + 1000000
    sp = np.arange(4000, dtype=np.int64) + 50000
    radix(hj, 5)
    try:
        build(hj, rk, rp)
        check_full(hj, oracle, rk, sk, rp, sp, null_r=-9, null_s=-10)   # on both sides
        assert_radix(hj)
        keep = sk != I64_MIN                                            # on the build side only
        e = check_full(hj, oracle, rk, sk[keep], rp, sp[keep], null_r=-9, null_s=-10)
        gr, gs = probe(hj, sk[keep], sp[keep], "full", -9, -10)
        rows = gs[np.isin(gr, rp[::97])]   # each INT64_MIN build row once, as a null row
        assert len(rows) == len(rp[::97]) and (rows == -10).all()
        assert e.n_r >= len(rp[::97])
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
            x = check_full(hj, oracle, rk, sk, sp=np.arange(len(sk), dtype=np.int64) + 100)
            if len(rk) == 0:
                assert x.m == len(sk) == x.n_s   # R empty: FULL gives every S row as a null row
                assert hj.count_full(dev(sk), kind="build") == 0
            if len(sk) == 0:
                assert x.m == len(rk) == x.n_r   # S empty: every R row comes out
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
        e = check_full(hj, oracle, r, s, row_base=7)
        assert e.n_r > 0 and e.n_s > 0
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
        for kind in KINDS:
            cr, cs = probe(hj, sk, sp, kind, -3, -4)
            out_r = torch.empty(len(cr), dtype=torch.int64, device="cuda")
            out_s = torch.empty_like(out_r)
            m = int(hj.probe_full_tuples(dev(np.stack([sk, sp], axis=1)), out_r, out_s, kind=kind, null_r=-3,
                                         null_s=-4).item())
            assert m == len(cr) == Exp(oracle, rk, rp, sk, sp, kind, -3, -4).m
            assert oracle.same_multiset(out_r.cpu().numpy(), out_s.cpu().numpy(), cr, cs)
            assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("where", ["pairs", "s-null-rows", "r-null-rows"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_capacity(hj, oracle, strategy, where):
    """out_cap inside the pairs, inside S's null rows and inside R's null rows
    (the stages' order): M stays exact, nothing at or past out_cap is touched,
    and what is written is a sub-multiset of the expected rows."""
    sentinel = -12345
    rk, rp, sk, sp = oracle.gen_pkfk_i64(13, 4000, 6000, 0.5)
    e = Exp(oracle, rk, rp, sk, sp, "full", -1, -2)
    assert min(e.pairs, e.n_s, e.n_r) > 600
    cap = {"pairs": e.pairs - 500, "s-null-rows": e.pairs + e.n_s - 500, "r-null-rows": e.m - 500}[where]
    hj.set_strategy(strategy, radix_bits=6 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        for kind in KINDS:
            x = e if kind == "full" else Exp(oracle, rk, rp, sk, sp, kind, -1, -2)
            c = cap if kind == "full" or where == "pairs" else x.m - 500   # build: no S null rows to fall inside
            back_r = torch.full((c + 4096,), sentinel, dtype=torch.int64, device="cuda")
            back_s = torch.full_like(back_r, sentinel)
            m = int(hj.probe_full(dev(sk), dev(sp), back_r[:c], back_s[:c], kind=kind, null_r=-1, null_s=-2).item())
            assert m == x.m > c
            got_r, got_s = back_r.cpu().numpy(), back_s.cpu().numpy()
            assert (got_r[c:] == sentinel).all() and (got_s[c:] == sentinel).all()
            extra = Counter(zip(got_r[:c].tolist(), got_s[:c].tolist())) - Counter(zip(x.r.tolist(), x.s.tolist()))
            assert not extra, list(extra.items())[:5]
            assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


def _fuzz_cases():
    rng = np.random.default_rng(0xF011)
    units = [0, 1, 63, 65, 511, 513, 2047, 2049, 3071, 3073, 4097, 5000]
    cases = []
    for i in range(12):
        nr = min(5000, int(rng.choice(units)) + int(rng.integers(0, 3)))
        ns = min(5000, int(rng.choice(units)) * int(rng.integers(1, 3)))
        span = int(rng.choice([64, 1000, 1 << 20, 1 << 40]))
        bits = int(rng.choice([1, 4, 7, 9, 12, 17]))
        cases.append((i, nr, ns, span, bits))
    return cases


@pytest.mark.parametrize("i,nr,ns,span,bits", _fuzz_cases())
def test_fuzz_ragged(hj, oracle, i, nr, ns, span, bits):
    rng = np.random.default_rng(7000 + i)
    try:
        for wide in (True, False):
            sp_ = span if wide else min(span, 1 << 30)
            lo = -sp_ // 2
            rk = rng.integers(lo, lo + sp_, nr, dtype=np.int64)
            sk = rng.integers(lo, lo + 2 * sp_, ns, dtype=np.int64)
            if nr:
                hit = rng.random(ns) < 0.4
                sk[hit] = rk[rng.integers(0, nr, int(hit.sum()))]
            if wide:
                sp, base, nulls = rng.integers(-(1 << 62), 1 << 62, ns, dtype=np.int64), 0, (I64_MIN + 5, I64_MIN + 6)
            else:
                rk, sk, sp, base, nulls = rk.astype(np.int32), sk.astype(np.int32), None, i, (-1, -2)
            radix(hj, bits)
            build(hj, rk)
            check_full(hj, oracle, rk, sk, sp=sp, null_r=nulls[0], null_s=nulls[1], row_base=base)
            assert_radix(hj)
            hj.set_strategy("global")
            build(hj, rk)
            check_full(hj, oracle, rk, sk, sp=sp, null_r=nulls[0], null_s=nulls[1], row_base=base)
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


def _outer(hj, sk, sp, cap):
    out_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    out_s = torch.empty_like(out_r)
    m = int(hj.probe_outer(dev(sk), dev(sp), out_r, out_s, null=-1).item())
    assert m <= cap
    return _sorted(out_r[:m].cpu().numpy(), out_s[:m].cpu().numpy())


def _exists(hj, sk, sp, kind):
    out_s = torch.empty(len(sk), dtype=torch.int64, device="cuda")
    m = int(hj.probe_exists(dev(sk), dev(sp), kind, out_s).item())
    s = np.sort(out_s[:m].cpu().numpy())
    return s, s


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_one_build_serves_every_probe_kind(hj, oracle, strategy):
    rk, rp = oracle.gen_uniform_i64(41, 1, 1, 500, 12000)
    sk, _ = oracle.gen_uniform_i64(41, 2, 100, 600, 9000)
    sp = np.arange(9000, dtype=np.int64)
    full = Exp(oracle, rk, rp, sk, sp, "full", -1, -2)
    bld = Exp(oracle, rk, rp, sk, sp, "build", -1, -2)
    assert full.n_r > 0 and full.n_s > 0
    cap = full.m
    runs = {
        "inner": lambda: _inner(hj, sk, sp, cap),
        "outer": lambda: _outer(hj, sk, sp, cap),
        "semi": lambda: _exists(hj, sk, sp, "semi"),
        "anti": lambda: _exists(hj, sk, sp, "anti"),
        "full": lambda: _sorted(*probe(hj, sk, sp, "full", -1, -2, cap=cap)),
        "build": lambda: _sorted(*probe(hj, sk, sp, "build", -1, -2, cap=cap)),
    }
    hj.set_strategy(strategy, radix_bits=10 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        first = {}
        for name in ("inner", "outer", "semi", "anti", "full", "build"):
            first[name] = runs[name]()
        dups = hj.has_duplicates()
        assert dups
        assert oracle.same_multiset(*first["full"], full.r, full.s)
        assert oracle.same_multiset(*first["build"], bld.r, bld.s)
        assert len(first["inner"][0]) == full.pairs
        assert np.array_equal(first["semi"][0], sp[np.isin(sk, rk)])
        for name in ("build", "anti", "full", "inner", "semi", "outer", "full", "build"):   # another order
            again = runs[name]()
            assert np.array_equal(again[0], first[name][0]) and np.array_equal(again[1], first[name][1]), name
            if strategy == "radix" and name in ("full", "build"):
                assert_radix(hj)
        assert hj.has_duplicates() == dups
        assert hj.strategy_used == strategy
        # a duplicate-free build keeps saying so after full probes
        uk = np.arange(12000, dtype=np.int64) * 5
        build(hj, uk)
        check_full(hj, oracle, uk, sk, sp=sp)
        assert not hj.has_duplicates()
    finally:
        hj.set_strategy("auto")


def test_auto_dual_build_picks_strategy_by_probe_size(hj):
    hj.set_strategy("auto")
    hj.probe_hint(None)
    nr, ns, null_r, null_s = 1 << 18, 1 << 24, -1, -2
    rk = torch.arange(nr, dtype=torch.int64, device="cuda") * 2
    rp = torch.arange(nr, dtype=torch.int64, device="cuda") * 5 + 2
    hj.build_table(rk, rp)
    sk = torch.arange(ns, dtype=torch.int64, device="cuda") % (1 << 18)
    sp = torch.arange(ns, dtype=torch.int64, device="cuda") * 3 + 1

    def digest(t):
        return int(t.sum().item()), int((t ^ (t >> 7)).sum().item())

    def want(n):
        """Expected columns for S = the first n rows (R holds the even keys below 2^19, each once)."""
        k, p = sk[:n], sp[:n]
        wr = torch.where((k % 2) == 0, (k // 2) * 5 + 2, torch.full_like(k, null_r))
        un = rp[(rk >= min(n, 1 << 18))]   # S's keys are 0 .. min(n, 2^18) - 1
        return torch.cat([wr, un]), torch.cat([p, torch.full_like(un, null_s)])

    out_r = torch.empty(ns + nr, dtype=torch.int64, device="cuda")
    out_s = torch.empty_like(out_r)
    for n, strategy in ((ns, "radix"), (1 << 12, "global")):
        wr, ws = want(n)
        m = int(hj.probe_full(sk[:n], sp[:n], out_r, out_s, kind="full", null_r=null_r, null_s=null_s).item())
        assert hj.strategy_used == strategy
        if strategy == "global":
            assert hj.join_kernel is None
        assert m == len(wr) and m > n
        assert digest(out_s[:m]) == digest(ws) and digest(out_r[:m]) == digest(wr)
        # each row is the right one, not only each column: R.pay + 7 * S.pay
        assert digest(out_r[:m] + 7 * out_s[:m]) == digest(wr + 7 * ws)
        assert hj.count_full(sk[:n], kind="build") == m - int(((sk[:n] % 2) == 1).sum().item())


def test_full_probe_after_routed_build(hj, oracle):
    """After a routed build a full probe over unrouted rows is valid, like hj_dev_probe_i64."""
    N, sub, q = 4, 3, 1
    rk, rp, sk, sp = oracle.gen_pkfk_i64(360, 40000, 60000, 0.6)
    R = RL.Routed(hj, dev(rk), dev(rp), N, sub)
    t, c = R.received(q)
    hj.build_routed(t, c, N, sub)
    g = N.bit_length() - 1
    own_r, own_s = RL.rparts(rk, g) == q, RL.rparts(sk, g) == q
    mk, mp = sk[own_s], sp[own_s]
    e = check_full(hj, oracle, rk[own_r], mk, rp[own_r], mp, null_r=-5, null_s=-6)
    assert 0 < e.n_s < len(mk) and 0 < e.n_r < int(own_r.sum())
    assert_radix(hj)


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_reports_full_probes(hj, oracle, strategy):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    timing_reports(hj, strategy, lambda: build(hj, rk, rp),
                   [lambda kind=kind: probe(hj, sk, sp, kind, -1, -2, cap=len(sk) + len(rk)) for kind in KINDS])


@pytest.mark.parametrize("n,strategy,wide", [(1 << 16, "radix", True), (1 << 12, "global", False)],
                         ids=["i64-2^16-radix", "i32-2^12-global"])
def test_graph_replay(hj, oracle, n, strategy, wide):
    """Build + full probe captured once, replayed over inputs rewritten in
    place: the mark bitmap (global) and the work maps (radix) are clean per replay."""
    kt = torch.int64 if wide else torch.int32
    rk = torch.empty(n, dtype=kt, device="cuda")
    sk = torch.empty(n, dtype=kt, device="cuda")
    rp = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 2 if wide else None
    sp = torch.arange(n, dtype=torch.int64, device="cuda") * 2 + 1 if wide else None
    grp = None
    if wide:
        sets = [oracle.gen_pkfk_i64(61 + j, n, n, f)[0::2] for j, f in enumerate((1.0, 0.5, 0.1))]
        if strategy == "radix":   # the replays also leave k_join_b and fill the deferral lists
            grp, with_nulls = OC.replay_sets_other_kernels(oracle, n, 10 * n)
            sets += [grp, with_nulls]
    else:
        sets = [(oracle.gen_uniform_i32(65 + j, 1, 1, hi, n), oracle.gen_uniform_i32(65 + j, 2, 1, hi, n))
                for j, hi in enumerate((4 * n, n // 4, 1 << 30))]

    def load(data):
        rk.copy_(torch.from_numpy(np.ascontiguousarray(data[0])))
        sk.copy_(torch.from_numpy(np.ascontiguousarray(data[1])))
        torch.cuda.synchronize()

    bits, cap = 64 if wide else 32, 10 * n
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
        hj.probe_full(sk, sp, out_r, out_s, kind="full", null_r=-1, null_s=-2, count=cnt)

    def reload(data):
        load(data)
        out_r.fill_(-9)
        cnt.zero_()

    def verify(data):
        m = int(cnt.item())
        e = Exp(oracle, np.ascontiguousarray(data[0]), pay_r, np.ascontiguousarray(data[1]), pay_s, "full", -1, -2)
        assert m == e.m <= cap
        assert oracle.same_multiset(host(out_r[:m]), host(out_s[:m]), e.r, e.s)
        if data is grp:   # the replay chose its kernel from this data, on the device
            assert e.m < cap and hj.join_kernel == "k_join_grp"

    graph_replay(hj, strategy, setup, step, sets[1:], reload, verify)


def test_full_join_method(hj, oracle):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(31, 3000, 9000, 0.3)
    e = Exp(oracle, rk, rp, sk, sp, "full", -1, -1)
    r, s = hj.full_join(dev(rk), dev(rp), dev(sk), dev(sp), capacity=10)   # one re-probe at the exact M
    assert oracle.same_multiset(r.cpu().numpy(), s.cpu().numpy(), e.r, e.s)
    r, s = hj.full_join(dev(rk), dev(rp), dev(sk), dev(sp), null_r=I64_MIN + 5, null_s=I64_MIN + 6)
    assert int((r == I64_MIN + 5).sum().item()) == e.n_s and int((s == I64_MIN + 6).sum().item()) == e.n_r
    b = Exp(oracle, rk, rp, sk, sp, "build", -1, -2)
    r, s = hj.full_join(dev(rk), dev(rp), dev(sk), dev(sp), how="build", null_s=-2)
    assert oracle.same_multiset(r.cpu().numpy(), s.cpu().numpy(), b.r, b.s)
    r32, s32 = rk.astype(np.int32), sk.astype(np.int32)
    r, s = hj.full_join(dev(r32), None, dev(s32))
    assert r.dtype == torch.int32 and s.dtype == torch.int32
    e32 = Exp(oracle, r32, np.arange(3000, dtype=np.int64), s32, np.arange(9000, dtype=np.int64), "full", -1, -1)
    assert oracle.same_multiset(r.cpu().numpy().astype(np.int64), s.cpu().numpy().astype(np.int64), e32.r, e32.s)
    with pytest.raises(ValueError):
        hj.full_join(dev(rk), dev(rp), dev(sk), dev(sp), how="left")
