"""Semi- and anti-join probes (EXISTS / NOT EXISTS, hj_dev_exists_*) on both
strategies and both row widths.

Expected results come from numpy on the host, never from the library:
mask = np.isin(S.key, R.key); semi = S.pay[mask], anti = S.pay[~mask],
compared after sorting (with out_key: as (key, payload) pairs)."""
import numpy as np
import pytest
import torch

from hashjoin import HashJoin, lib
from join_gpu import assert_radix_kernel, dev, glob_hj, graph_replay, hj, host, radix, timing_reports  # noqa: F401

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
KINDS = ("semi", "anti")


def build(hj, rk, rp=None):
    if rk.dtype == np.int32:
        hj.build_table(dev(rk))
    else:
        hj.build_table(dev(rk), dev(np.zeros_like(rk) if rp is None else rp))


def probe(hj, sk, sp, kind, row_base=0):
    """(keys, payloads) of one exists probe of the current build, output sized |S|."""
    wide = sk.dtype == np.int64
    n = max(1, len(sk))
    out_s = torch.full((n,), -7, dtype=torch.int64 if wide else torch.int32, device="cuda")
    out_k = torch.full_like(out_s, -7)
    cnt = hj.probe_exists(dev(sk), dev(sp) if wide else None, kind, out_s, out_k, row_base=row_base)
    m = int(cnt.item())
    assert 0 <= m <= len(sk), (kind, m, len(sk))
    return out_k[:m].cpu().numpy().astype(np.int64), out_s[:m].cpu().numpy().astype(np.int64)


def same_pairs(gk, gp, ek, ep):
    if len(gk) != len(ek):
        return False
    a, b = np.lexsort((gp, gk)), np.lexsort((ep, ek))
    return np.array_equal(gk[a], ek[b]) and np.array_equal(gp[a], ep[b])


def check_both(hj, rk, sk, sp=None, row_base=0):
    """Both kinds of the current build against numpy; semi and anti partition S."""
    if sp is None:
        sp = row_base + np.arange(len(sk), dtype=np.int64)
    mask = np.isin(sk, rk)
    got = {}
    for kind, sel in (("semi", mask), ("anti", ~mask)):
        gk, gp = probe(hj, sk, sp, kind, row_base)
        assert len(gp) == int(sel.sum()), (kind, len(gp), int(sel.sum()))
        assert same_pairs(gk, gp, sk[sel].astype(np.int64), sp[sel].astype(np.int64)), kind
        assert hj.count_exists(dev(sk), kind) == int(sel.sum()), kind
        got[kind] = gp
    assert len(got["semi"]) + len(got["anti"]) == len(sk)
    if len(np.unique(sp)) == len(sp):
        assert len(np.intersect1d(got["semi"], got["anti"])) == 0
    return mask


def assert_radix(hj):
    assert_radix_kernel(hj, 6, "k_join_exists")


def test_errors_kind_and_state():
    from hashjoin import _lib
    h = HashJoin(0)
    try:
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = torch.zeros(4, dtype=torch.int64, device="cuda")
        args = (k.data_ptr(), k.data_ptr(), 4, None, None, 0, cnt.data_ptr(), None)
        assert lib.hj_dev_exists_i64(h._ctx, 2, *args) == _lib.HJ_ERR_ARG
        assert lib.hj_dev_exists_i64(h._ctx, -1, *args) == _lib.HJ_ERR_ARG
        assert lib.hj_dev_exists_i64(h._ctx, 0, *args) == _lib.HJ_ERR_STATE   # no build yet
        h.build_table(k.to(torch.int32))
        assert lib.hj_dev_exists_i64(h._ctx, 1, *args) == _lib.HJ_ERR_STATE   # an i32 build: layout mismatch
        assert lib.hj_dev_exists_i32(h._ctx, 1, k.data_ptr(), 4, 0, None, None, 5, cnt.data_ptr(), None) == _lib.HJ_ERR_ARG
        with pytest.raises(KeyError):
            h.probe_exists(k.to(torch.int32), kind="outer")
    finally:
        h.close()


# ------------------------------------------------------------------ global
@pytest.mark.parametrize("nr", [1, 1000, 2048, 3000])   # 2048: the last LDS-resident table
def test_global_pkfk_i64(glob_hj, oracle, nr):
    ns = (1 << 16) + 37   # a ragged last 2048-row tile
    rk, rp, sk, sp = oracle.gen_pkfk_i64(100 + nr, nr, ns, 0.6)
    build(glob_hj, rk, rp)
    check_both(glob_hj, rk, sk, sp)
    assert glob_hj.strategy_used == "global"
    assert glob_hj.join_kernel is None


def test_global_repeated_build_keys(glob_hj, oracle):
    rk, rp = oracle.gen_uniform_i64(11, 1, 1, 300, 1000)
    sk, sp = oracle.gen_uniform_i64(11, 2, 1, 400, 1 << 16)
    build(glob_hj, rk, rp)
    assert glob_hj.has_duplicates()
    check_both(glob_hj, rk, sk, sp)
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
    mask = check_both(glob_hj, rk, sk, sp)
    if where == "both":
        assert mask[::1777].all()
    if where == "probe":
        assert not mask[::1777].any()


@pytest.mark.parametrize("nr", [4000, 5000])   # either side of a 64-KiB table
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    build(glob_hj, r)
    check_both(glob_hj, r, s, row_base=7)


@pytest.mark.parametrize("kind", KINDS)
def test_global_capacity(glob_hj, oracle, kind):
    ns, cap, sentinel = 1 << 16, 1000, -12345
    rk, rp, sk, sp = oracle.gen_pkfk_i64(13, 3000, ns, 0.6 if kind == "semi" else 0.4)
    mask = np.isin(sk, rk)
    sel = mask if kind == "semi" else ~mask
    build(glob_hj, rk, rp)
    back_s = torch.full((cap + 4096,), sentinel, dtype=torch.int64, device="cuda")
    back_k = torch.full_like(back_s, sentinel)
    m = int(glob_hj.probe_exists(dev(sk), dev(sp), kind, back_s[:cap], back_k[:cap]).item())
    assert m == int(sel.sum()) and m > cap
    got_s, got_k = back_s.cpu().numpy(), back_k.cpu().numpy()
    assert (got_s[cap:] == sentinel).all() and (got_k[cap:] == sentinel).all()
    assert len(np.unique(got_s[:cap])) == cap
    key_of = dict(zip(sp[sel].tolist(), sk[sel].tolist()))
    assert all(key_of.get(p) == k for p, k in zip(got_s[:cap].tolist(), got_k[:cap].tolist()))


# ------------------------------------------------------------------ radix
@pytest.mark.parametrize("bits", [1, 3, 9, 12, 17])   # 1-, 2- and 3-pass plans
def test_radix_pkfk(hj, oracle, bits):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(bits, 20000, 30000, 0.7)
    radix(hj, bits)
    try:
        build(hj, rk, rp)
        check_both(hj, rk, sk, sp)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_partitions_without_build_rows(hj, oracle):
    """2^10 partitions, 50 build rows: ~970 partitions hold probe rows only --
    exactly the rows an anti-join returns (the work map must keep them)."""
    rk = np.arange(50, dtype=np.int64) * 1000003 + 17
    rng = np.random.default_rng(5)
    sk = rng.integers(1 << 40, 1 << 41, 30000, dtype=np.int64)
    hit = rng.random(30000) < 0.5
    sk[hit] = rk[rng.integers(0, 50, int(hit.sum()))]
    sp = np.arange(30000, dtype=np.int64) * 3
    radix(hj, 10)
    try:
        build(hj, rk)
        mask = check_both(hj, rk, sk, sp)
        assert 0.4 < mask.mean() < 0.6
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_build_key_rounds(hj):
    """20000 copies of one build key: its partition spans several build
    rounds, and a probe row matching it is still emitted exactly once."""
    rk = np.concatenate([np.full(20000, 42, np.int64), np.arange(1000, 3000, dtype=np.int64)])
    sk = np.array([42, 7, 42, 2500, 99999], np.int64)
    sp = np.arange(5, dtype=np.int64)
    radix(hj, 4)
    try:
        build(hj, rk)
        _, semi = probe(hj, sk, sp, "semi")
        _, anti = probe(hj, sk, sp, "anti")
        assert sorted(semi.tolist()) == [0, 2, 3]
        assert sorted(anti.tolist()) == [1, 4]
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_distinct_keys_over_one_round(hj, oracle):
    """30000 DISTINCT build keys per partition: more than any one-round table
    of 8-B slots in 64 KiB holds, so rounds cannot be avoided by deduplication."""
    rk, rp, sk, sp = oracle.gen_pkfk_i64(77, 60000, 40000, 0.5)
    assert len(np.unique(rk)) == 60000
    radix(hj, 1)
    try:
        build(hj, rk, rp)
        check_both(hj, rk, sk, sp)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_probe_key_many_chunks(hj):
    rk = np.arange(3000, dtype=np.int64) * 7
    sk = np.concatenate([np.full(50000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    sp = np.arange(len(sk), dtype=np.int64)
    radix(hj, 6)
    try:
        build(hj, rk)
        check_both(hj, rk, sk, sp)
    finally:
        hj.set_strategy("auto")


def test_radix_int64_min_both_sides(hj, oracle):
    rk, rp = oracle.gen_uniform_i64(3, 1, -100, 100, 5000)
    sk, sp = oracle.gen_uniform_i64(3, 2, -100, 100, 4000)
    rk[::97] = I64_MIN
    sk[::131] = I64_MIN
    sp = np.arange(4000, dtype=np.int64)
    radix(hj, 5)
    try:
        build(hj, rk, rp)
        mask = check_both(hj, rk, sk, sp)
        assert mask[::131].all()
        # and with no INT64_MIN on the build side those probe rows are anti rows
        rk2 = rk[rk != I64_MIN]
        build(hj, rk2)
        mask = check_both(hj, rk2, sk, sp)
        assert not mask[::131].any()
    finally:
        hj.set_strategy("auto")


def test_radix_empty_and_tiny(hj):
    e = np.empty(0, np.int64)
    k = np.array([5, 9, 5, 3], np.int64)
    one, other = np.array([4], np.int64), np.array([6], np.int64)
    radix(hj, 3)
    try:
        for rk, sk in [(e, k), (k, e), (one, one), (one, other)]:
            build(hj, rk)
            check_both(hj, rk, sk, np.arange(len(sk), dtype=np.int64) + 100)
            assert hj.strategy_used == "radix"
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("bits", [1, 9])
def test_radix_i32(hj, oracle, bits):
    r = oracle.gen_uniform_i32(bits, 1, -(1 << 31), (1 << 31) - 1, 30000)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(bits, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    radix(hj, bits)
    try:
        build(hj, r)
        check_both(hj, r, s, row_base=7)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_tuples_form_equals_columns(hj, oracle, strategy):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(21, 5000, 20011, 0.5)
    hj.set_strategy(strategy, radix_bits=7 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        tup = dev(np.stack([sk, sp], axis=1))
        for kind in KINDS:
            ck, cp = probe(hj, sk, sp, kind)
            out_s = torch.empty(len(sk), dtype=torch.int64, device="cuda")
            out_k = torch.empty_like(out_s)
            m = int(hj.probe_exists_tuples(tup, kind, out_s, out_k).item())
            assert same_pairs(out_k[:m].cpu().numpy(), out_s[:m].cpu().numpy(), ck, cp), kind
            sel = np.isin(sk, rk) if kind == "semi" else ~np.isin(sk, rk)
            assert m == int(sel.sum())
    finally:
        hj.set_strategy("auto")


def _fuzz_cases():
    rng = np.random.default_rng(0xE15)
    units = [1, 63, 64, 65, 511, 513, 2047, 2049, 3071, 3073, 4097, 8193, 12289, 40000]
    cases = []
    for i in range(12):
        nr = min(40000, int(rng.choice(units)) + int(rng.integers(0, 3)))
        ns = min(40000, int(rng.choice(units)) * int(rng.integers(1, 4)))
        span = int(rng.choice([3, 64, 1000, 1 << 20, 1 << 40]))
        bits = int(rng.choice([1, 4, 7, 9, 12, 17]))
        cases.append((i, nr, ns, span, bits, bool(i % 3)))
    return cases


@pytest.mark.parametrize("i,nr,ns,span,bits,wide", _fuzz_cases())
def test_fuzz_ragged(hj, i, nr, ns, span, bits, wide):
    rng = np.random.default_rng(2000 + i)
    if not wide:
        span = min(span, 1 << 30)
    lo = -span // 2
    rk = rng.integers(lo, lo + span, nr, dtype=np.int64)
    sk = rng.integers(lo, lo + span, ns, dtype=np.int64)
    hit = rng.random(ns) < 0.5
    sk[hit] = rk[rng.integers(0, nr, int(hit.sum()))]
    if wide:
        sp = rng.integers(-(1 << 62), 1 << 62, ns, dtype=np.int64)
        base = 0
    else:
        rk, sk, sp, base = rk.astype(np.int32), sk.astype(np.int32), None, i
    try:
        radix(hj, bits)
        build(hj, rk)
        check_both(hj, rk, sk, sp, row_base=base)
        assert_radix(hj)
        hj.set_strategy("global")
        build(hj, rk)
        check_both(hj, rk, sk, sp, row_base=base)
        assert hj.strategy_used == "global"
    finally:
        hj.set_strategy("auto")


def test_semi_and_anti_join_methods(hj, oracle):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(31, 3000, 9000, 0.3)
    mask = np.isin(sk, rk)
    k, p = hj.semi_join(dev(rk), dev(sk), dev(sp), with_keys=True, capacity=10)   # one re-probe at the exact M
    assert same_pairs(k.cpu().numpy(), p.cpu().numpy(), sk[mask], sp[mask])
    p = hj.anti_join(dev(rk), dev(sk), dev(sp), rpay=dev(rp))
    assert np.array_equal(np.sort(p.cpu().numpy()), np.sort(sp[~mask]))
    r32, s32 = rk.astype(np.int32), sk.astype(np.int32)
    rows = hj.semi_join(dev(r32), dev(s32))
    assert rows.dtype == torch.int32
    assert np.array_equal(np.sort(rows.cpu().numpy()), np.flatnonzero(np.isin(s32, r32)))


# ------------------------------------------------------------------ interaction
def _inner(hj, sk, sp, cap):
    out_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    out_s = torch.empty_like(out_r)
    m = int(hj.probe_relation(dev(sk), dev(sp), out_r, out_s).item())
    assert m <= cap
    r, s = out_r[:m].cpu().numpy(), out_s[:m].cpu().numpy()
    o = np.lexsort((s, r))
    return r[o], s[o]


def test_one_build_serves_inner_semi_anti(hj, oracle):
    rk, rp = oracle.gen_uniform_i64(41, 1, 1, 500, 12000)
    sk, sp = oracle.gen_uniform_i64(41, 2, 1, 500, 9000)
    sp = np.arange(9000, dtype=np.int64)
    cap = 12000 * 9000 // 500 * 2
    radix(hj, 10)
    try:
        build(hj, rk, rp)
        first = _inner(hj, sk, sp, cap)
        assert hj.join_kernel != "k_join_exists"
        check_both(hj, rk, sk, sp)
        assert_radix(hj)
        second = _inner(hj, sk, sp, cap)
        assert hj.join_kernel != "k_join_exists"
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
        assert len(first[0]) == int(np.bincount(rk, minlength=501)[sk].sum())
        check_both(hj, rk, sk, sp)
        assert hj.has_duplicates()
        uk = np.arange(12000, dtype=np.int64) * 5
        build(hj, uk)
        check_both(hj, uk, sk, sp)
        assert not hj.has_duplicates()
    finally:
        hj.set_strategy("auto")


def test_auto_dual_build_picks_strategy_by_probe_size(hj):
    hj.set_strategy("auto")
    hj.probe_hint(None)
    rk = torch.arange(1 << 18, dtype=torch.int64, device="cuda") * 2
    hj.build_table(rk, torch.zeros_like(rk))
    sk = torch.arange(1 << 24, dtype=torch.int64, device="cuda") % (1 << 19)
    sp = torch.arange(1 << 24, dtype=torch.int64, device="cuda") * 3 + 1
    mask = torch.isin(sk, rk)
    out_s = torch.empty(1 << 24, dtype=torch.int64, device="cuda")
    for kind, sel in (("semi", mask), ("anti", ~mask)):
        m = int(hj.probe_exists(sk, sp, kind, out_s).item())
        assert hj.strategy_used == "radix"
        assert m == int(sel.sum().item()) == 1 << 23
        assert int(out_s[:m].sum().item()) == int(sp[sel].sum().item())
        assert int((out_s[:m] ^ (out_s[:m] >> 7)).sum().item()) == int((sp[sel] ^ (sp[sel] >> 7)).sum().item())
    small = 1 << 12
    m = int(hj.probe_exists(sk[:small], sp[:small], "semi", out_s[:small]).item())
    assert hj.strategy_used == "global"
    assert hj.join_kernel is None
    assert m == int(mask[:small].sum().item())
    assert np.array_equal(np.sort(out_s[:m].cpu().numpy()), sp[:small][mask[:small]].cpu().numpy())


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_reports_exists_probes(hj, oracle, strategy):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    timing_reports(hj, strategy, lambda: build(hj, rk, rp), [lambda: probe(hj, sk, sp, "anti")])


@pytest.mark.parametrize("n,strategy,wide", [(1 << 16, "radix", True), (1 << 12, "global", False)],
                         ids=["i64-2^16-radix", "i32-2^12-global"])
def test_graph_replay(hj, oracle, n, strategy, wide):
    kt = torch.int64 if wide else torch.int32
    rk = torch.empty(n, dtype=kt, device="cuda")
    sk = torch.empty(n, dtype=kt, device="cuda")
    rp = torch.zeros(n, dtype=torch.int64, device="cuda") if wide else None
    sp = torch.arange(n, dtype=torch.int64, device="cuda") * 2 + 1 if wide else None
    if wide:
        sets = [oracle.gen_pkfk_i64(61 + j, n, n, f)[0::2] for j, f in enumerate((1.0, 0.5, 0.1, 0.8))]
    else:
        sets = [(oracle.gen_uniform_i32(65 + j, 1, 1, hi, n), oracle.gen_uniform_i32(65 + j, 2, 1, hi, n))
                for j, hi in enumerate((4 * n, n // 4, 1 << 30, 2 * n))]

    def load(data):
        rk.copy_(torch.from_numpy(np.ascontiguousarray(data[0])))
        sk.copy_(torch.from_numpy(np.ascontiguousarray(data[1])))
        torch.cuda.synchronize()

    bits = 64 if wide else 32
    out_s = torch.empty(n, dtype=kt, device="cuda")
    out_k = torch.empty_like(out_s)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def setup():
        load(sets[0])
        hj.allocate_hash_table(n, bits)
        hj.build_table(rk, rp)
        hj.reserve_probe(n, bits)

    def step():
        hj.build_table(rk, rp)
        hj.probe_exists(sk, sp, "anti", out_s, out_k, count=cnt)

    def reload(data):
        load(data)
        out_s.fill_(-1)
        cnt.zero_()

    def verify(data):
        m = int(cnt.item())
        sel = ~np.isin(data[1], data[0])
        pay = (np.arange(n, dtype=np.int64) * 2 + 1) if wide else np.arange(n, dtype=np.int64)
        assert m == int(sel.sum())
        assert same_pairs(host(out_k[:m]), host(out_s[:m]), data[1][sel].astype(np.int64), pay[sel])

    graph_replay(hj, strategy, setup, step, sets[1:], reload, verify)
