"""Positional lookup probe (SINGLE / MARK join, hj_dev_lookup_*) on both
strategies and both row widths.

Expected results come from numpy on the host, never from the library: the
count column is outer_cases.Expect(rk, sk).cnt, the payload column the minimum
of R's payloads over each key (sort by (key, payload), then searchsorted).
Results are compared element by element at the probe row's own position, with
no sorting.  int64 payloads are a seeded permutation around zero, times three
plus one: NULL and SENTINEL are multiples of three, so neither is a payload."""
import numpy as np
import pytest
import torch

import outer_cases as OC
from hashjoin import HashJoin, _lib, lib
from join_gpu import (assert_radix_kernel, build, dev, glob_hj, graph_replay, hj, host, sentinels,  # noqa: F401
                      timing_reports)
from positional_cases import EXTRA, NULL, SENTINEL   # -9, -12345, 64: i32 payloads are row ids (>= 0)
from positional_cases import lookup_expect as expect

pytestmark = pytest.mark.gpu

I64_MIN = OC.I64_MIN


def payloads(rk, seed=1):
    """R's payloads: int64 a permutation with negative values, i32 the row ids."""
    n = len(rk)
    if rk.dtype == np.int32:
        return np.arange(n, dtype=np.int64)
    return (np.random.default_rng(seed).permutation(n).astype(np.int64) - n // 2) * 3 + 1


def probe(hj, sk, want_r=True, want_cnt=True):
    """One lookup of the current build into sentinel-filled outputs EXTRA rows
    longer than S: (d_count, out_r, out_cnt) as int64 host arrays (None if not asked for)."""
    n = len(sk)
    dt = torch.int64 if sk.dtype == np.int64 else torch.int32
    o_r = sentinels(n + EXTRA, SENTINEL, dt) if want_r else None
    o_c = sentinels(n + EXTRA, SENTINEL, torch.int32) if want_cnt else None
    m = int(hj.probe_lookup(dev(sk), o_r, o_c, null=NULL).item())
    host = lambda t: None if t is None else t.cpu().numpy().astype(np.int64)   # noqa: E731
    return m, host(o_r), host(o_c)


def check(hj, rk, rp, sk, want_r=True, want_cnt=True):
    er, ec = expect(rk, rp, sk)
    n = len(sk)
    m, g_r, g_c = probe(hj, sk, want_r, want_cnt)
    assert m == int((ec > 0).sum()), (m, int((ec > 0).sum()))
    if want_cnt:
        assert np.array_equal(g_c[:n], ec), np.flatnonzero(g_c[:n] != ec)[:8]
        assert (g_c[n:] == SENTINEL).all()
    if want_r:
        assert np.array_equal(g_r[:n], er), np.flatnonzero(g_r[:n] != er)[:8]
        assert (g_r[n:] == SENTINEL).all()
    return er, ec


def assert_radix(hj):
    assert _lib.HJ_JOIN_KERNEL_LOOKUP == 7
    assert_radix_kernel(hj, _lib.HJ_JOIN_KERNEL_LOOKUP, "k_join_lookup")


# ------------------------------------------------------------------ global
# (ns = 2 * 2048 + 77 is three tiles, one per workgroup: k_probe_lookup never
# strides here, so its load-ahead and hand-over stay idle.  The shape with
# more tiles than workgroups is test_gpu_positional_tiles.py's.)
@pytest.mark.parametrize("nr", [1, 2048, 3000])   # 2048: the last LDS-resident table
def test_global_i64(glob_hj, oracle, nr):
    ns = 2 * 2048 + 77   # a ragged third tile
    rk, _, sk, _ = oracle.gen_pkfk_i64(300 + nr, nr, ns, 0.6)
    rp = payloads(rk, nr)
    build(glob_hj, rk, rp)
    _, ec = check(glob_hj, rk, rp, sk)
    assert 0 < (ec > 0).sum() < ns and ec.max() == 1
    assert glob_hj.strategy_used == "global" and glob_hj.join_kernel is None


@pytest.mark.parametrize("nr", [4000, 5000])   # either side of a 64-KiB table
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 2 * 2048 + 77 - len(r[::3]))])
    build(glob_hj, r, None)
    _, ec = check(glob_hj, r, payloads(r), s)
    assert (ec > 0).sum() >= len(r[::3])


def repeated_keys_case(dtype):
    """Distinct keys, some three times, one 500 times, shuffled."""
    rng = np.random.default_rng(17)
    base = rng.permutation(1 << 20)[:1500].astype(np.int64) * 5 + 3
    rk = np.concatenate([base, base[:100], base[:100], np.full(499, base[7])])
    rk = rk[rng.permutation(len(rk))].astype(dtype)
    sk = np.concatenate([base[::2], base[:100], [base[7]] * 5, rng.integers(1 << 25, 1 << 26, 3000)]).astype(dtype)
    return rk, sk[rng.permutation(len(sk))]


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
def test_global_repeated_build_keys(glob_hj, dtype):
    rk, sk = repeated_keys_case(dtype)
    rp = payloads(rk, 3)
    build(glob_hj, rk, rp)
    assert glob_hj.has_duplicates()
    _, ec = check(glob_hj, rk, rp, sk)
    assert set(np.unique(ec).tolist()) == {0, 1, 3, 502}
    assert glob_hj.has_duplicates()


@pytest.mark.parametrize("where", ["probe", "build", "both"])
def test_global_int64_min(glob_hj, oracle, where):
    rk = oracle.gen_uniform_i64(12, 1, -2000, 2000, 1500)[0].copy()
    sk = oracle.gen_uniform_i64(12, 2, -3000, 3000, 2 * 2048 + 77)[0].copy()
    if where in ("both", "build"):
        rk[::500] = I64_MIN
    if where in ("both", "probe"):
        sk[::1777] = I64_MIN
    rp = payloads(rk, 5)
    build(glob_hj, rk, rp)
    er, ec = check(glob_hj, rk, rp, sk)
    if where == "both":
        assert (ec[::1777] == 3).all() and (er[::1777] == rp[::500].min()).all()
    if where == "probe":
        assert (ec[::1777] == 0).all() and (er[::1777] == NULL).all()


@pytest.mark.parametrize("which", ["payload-only", "count-only"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_single_output(hj, oracle, strategy, which):
    rk, _, sk, _ = oracle.gen_pkfk_i64(23, 3000, 9001, 0.5)
    rp = payloads(rk, 23)
    hj.set_strategy(strategy, radix_bits=5 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk, want_r=which == "payload-only", want_cnt=which == "count-only")
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


# ------------------------------------------------------------------ radix
# one pass of the half-size workgroups, one of the full-size ones (S's row
# index enters in the first pass: both of its variants), and a two-pass plan
@pytest.mark.parametrize("bits", [1, 9, 17])
def test_radix_pkfk(hj, oracle, bits):
    rk, _, sk, _ = oracle.gen_pkfk_i64(bits, 20000, 50000, 0.8)
    rp = payloads(rk, bits)
    hj.set_strategy("radix", radix_bits=bits)
    try:
        build(hj, rk, rp)
        assert hj.radix_passes == {1: 1, 9: 1, 17: 2}[bits]
        check(hj, rk, rp, sk)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("name", OC.RADIX_SHAPES)
def test_radix_shapes(hj, oracle, name):
    c = OC.radix_path_case(oracle, name)
    rk, sk = c["rk"], c["sk"]
    rp = payloads(rk, 7)
    hj.set_strategy("radix", radix_bits=c["bits"])
    try:
        build(hj, rk, rp)
        _, ec = check(hj, rk, rp, sk)
        assert_radix(hj)
        if name == "b-oversized":   # the count and the minimum are taken across build rounds
            assert (ec[[10, 4000, 8999]] == 20000).all()
    finally:
        hj.set_strategy("auto")


def test_radix_fresh_context():
    """A new context, 2^10 partitions: most hold build rows only (50 probe
    rows), then most hold probe rows of both kinds (200000 probe rows)."""
    c = OC.fresh_context_case()
    rp = payloads(c["rk"], 9)
    h = HashJoin(0)
    try:
        h.set_strategy("radix", radix_bits=c["bits"])
        build(h, c["rk"], rp)
        for sk in (c["sk"], c["big"]):
            check(h, c["rk"], rp, sk)
            assert_radix(h)
    finally:
        h.close()


def test_radix_partitions_without_build_rows(hj):
    """2^10 partitions, 50 build rows: most S rows lie in partitions without
    any -- the kernel itself writes their (null, 0), nothing prefills."""
    rk = np.arange(50, dtype=np.int64) * 1000003 + 17
    rng = np.random.default_rng(5)
    sk = rng.integers(1 << 40, 1 << 41, 30000, dtype=np.int64)
    hit = rng.random(30000) < 0.5
    sk[hit] = rk[rng.integers(0, 50, int(hit.sum()))]
    rp = payloads(rk, 2)
    hj.set_strategy("radix", radix_bits=10)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_probe_key_many_chunks(hj):
    rk = np.arange(3000, dtype=np.int64) * 7
    sk = np.concatenate([np.full(50000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    sk = sk[np.random.default_rng(3).permutation(len(sk))]
    rp = payloads(rk, 4)
    hj.set_strategy("radix", radix_bits=6)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_distinct_keys_over_one_round(hj, oracle):
    """30000 distinct build keys per partition: several build rounds whose
    tables hold different keys, the sub-chunks-outermost path."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(77, 60000, 40000, 0.5)
    rp = payloads(rk, 6)
    hj.set_strategy("radix", radix_bits=1)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("bits", [1, 9])
def test_radix_i32(hj, oracle, bits):
    r = oracle.gen_uniform_i32(bits, 1, -(1 << 31), (1 << 31) - 1, 30000)
    r[1000:1300] = r[:300]   # some keys twice: the smaller row id wins
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(bits, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    hj.set_strategy("radix", radix_bits=bits)
    try:
        build(hj, r, None)
        _, ec = check(hj, r, payloads(r), s)
        assert ec.max() >= 2
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


# ------------------------------------------------------------------ both strategies
@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_empty_and_tiny(hj, strategy, wide):
    dt = np.int64 if wide else np.int32
    e = np.empty(0, dt)
    k = np.array([5, 9, 5, 3], dt)
    one, other = np.array([4], dt), np.array([6], dt)
    hj.set_strategy(strategy, radix_bits=3 if strategy == "radix" else 0)
    try:
        for rk, sk in [(e, k), (k, e), (one, one), (one, other), (k, one), (k, k[:1])]:
            rp = payloads(rk, 8)
            build(hj, rk, rp)
            er, ec = check(hj, rk, rp, sk)
            assert hj.strategy_used == strategy
            if len(rk) == 0:
                assert (er == NULL).all() and (ec == 0).all()
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_int64_min_build_rows_and_the_repeat_flag(hj, oracle, strategy, copies):
    """INT64_MIN is a key like any other to has_duplicates() too: two build rows
    that hold it (they sit beside the table, in no slot) are a repeated key,
    one is not -- with no other key twice."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(5, 3000, 9001, 0.5)
    rk, sk = rk.copy(), sk.copy()
    rk[[7, 2900][:copies]] = I64_MIN
    sk[::1777] = I64_MIN
    assert len(np.unique(rk)) == 3000 - (copies - 1)
    rp = payloads(rk, 5)
    hj.set_strategy(strategy, radix_bits=5 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        _, ec = check(hj, rk, rp, sk)
        assert (ec[::1777] == copies).all() and ec.max() == copies
        assert hj.strategy_used == strategy
        assert hj.has_duplicates() == (copies == 2)
        check(hj, rk, rp, sk)
    finally:
        hj.set_strategy("auto")


def _sorted(cnt, *cols):
    m = int(cnt.item())
    a = [c[:m].cpu().numpy() for c in cols]
    o = np.lexsort(tuple(reversed(a)))
    return [c[o] for c in a]


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_one_build_serves_every_probe(hj, oracle, strategy):
    """inner -> lookup -> semi -> full -> lookup -> inner, semi, full of one
    build: each result equals its first, and the repeat flag keeps its answer."""
    rk = oracle.gen_uniform_i64(41, 1, 1, 500, 12000)[0].copy()
    sk = oracle.gen_uniform_i64(41, 2, 1, 700, 9000)[0].copy()
    rk[::97] = I64_MIN
    sk[::131] = I64_MIN
    rp = payloads(rk, 41)
    d_sk, d_sp = dev(sk), dev(np.arange(9000, dtype=np.int64))
    cap = int(OC.Expect(rk, sk).m("full")) + 8
    o_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    o_s = torch.empty_like(o_r)

    def inner():
        return _sorted(hj.probe_relation(d_sk, d_sp, o_r, o_s), o_r, o_s)

    def semi():
        return _sorted(hj.probe_exists(d_sk, d_sp, "semi", o_s), o_s)

    def full():
        return _sorted(hj.probe_full(d_sk, d_sp, o_r, o_s, kind="full", null_r=NULL, null_s=NULL), o_r, o_s)

    hj.set_strategy(strategy, radix_bits=10 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        first = {"inner": inner()}
        dups = hj.has_duplicates()
        assert dups
        check(hj, rk, rp, sk)
        first["semi"] = semi()
        first["full"] = full()
        assert hj.join_kernel != "k_join_lookup"
        check(hj, rk, rp, sk)
        if strategy == "radix":
            assert_radix(hj)
        for name, f in (("inner", inner), ("semi", semi), ("full", full)):
            again = f()
            assert all(np.array_equal(a, b) for a, b in zip(first[name], again)), name
        assert len(first["inner"][0]) == OC.Expect(rk, sk).pairs
        assert hj.has_duplicates() == dups
        check(hj, rk, rp, sk)
        # and a build without repeats keeps saying so after a lookup
        uk = np.arange(12000, dtype=np.int64) * 5
        up = payloads(uk, 42)
        build(hj, uk, up)
        check(hj, uk, up, sk)
        assert not hj.has_duplicates()
        check(hj, uk, up, sk)
    finally:
        hj.set_strategy("auto")


def test_lookup_method(hj, oracle):
    rk, _, sk, _ = oracle.gen_pkfk_i64(31, 3000, 9000, 0.3)
    rp = payloads(rk, 31)
    er, ec = expect(rk, rp, sk)
    got = hj.lookup(dev(rk), dev(rp), dev(sk), null=NULL)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), er)
    g_r, g_c = hj.lookup(dev(rk), dev(rp), dev(sk), null=NULL, with_counts=True)
    assert g_c.dtype == torch.int32
    assert np.array_equal(g_r.cpu().numpy(), er) and np.array_equal(g_c.cpu().numpy(), ec)
    # rpay None: the id -> index mapping
    idx = hj.lookup(dev(rk), None, dev(sk))
    ei, _ = expect(rk, np.arange(len(rk), dtype=np.int64), sk)
    ei[ec == 0] = -1
    assert np.array_equal(idx.cpu().numpy(), ei)
    assert np.array_equal(rk[ei[ec > 0]], sk[ec > 0])
    r32, s32 = rk.astype(np.int32), sk.astype(np.int32)
    rows, c32 = hj.lookup(dev(r32), None, dev(s32), with_counts=True)
    e32, ec32 = expect(r32, payloads(r32), s32)
    e32[ec32 == 0] = -1
    assert rows.dtype == torch.int32 and c32.dtype == torch.int32
    assert np.array_equal(rows.cpu().numpy(), e32) and np.array_equal(c32.cpu().numpy(), ec32)


def test_errors_in_order():
    """null context; no build of that layout; null count pointer, bad relation,
    both outputs null; (a build past INT32_MAX rows: not reachable at test
    sizes;) i32: n > INT32_MAX."""
    h = HashJoin(0)
    try:
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = torch.zeros(4, dtype=torch.int64, device="cuda")
        k32 = k.to(torch.int32)
        o = torch.zeros(4, dtype=torch.int64, device="cuda")
        c = torch.zeros(4, dtype=torch.int32, device="cuda")
        P = lambda t: t.data_ptr()   # noqa: E731
        ARG, STATE = _lib.HJ_ERR_ARG, _lib.HJ_ERR_STATE
        # everything else wrong too: the context comes first, then the state
        assert lib.hj_dev_lookup_i64(None, None, -1, -1, None, None, None, None) == ARG
        assert b"null context" in lib.hj_last_error()
        assert lib.hj_dev_lookup_i64(h._ctx, None, -1, -1, None, None, None, None) == STATE
        h.build_table(k32)
        assert lib.hj_dev_lookup_i64(h._ctx, P(k), 4, -1, P(o), P(c), P(cnt), None) == STATE   # an i32 build
        assert lib.hj_dev_lookup_i32(h._ctx, None, 4, -1, None, None, None, None) == ARG
        assert b"count pointer" in lib.hj_last_error()
        assert lib.hj_dev_lookup_i32(h._ctx, None, 4, -1, None, None, P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert lib.hj_dev_lookup_i32(h._ctx, P(k32), -1, -1, None, None, P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert lib.hj_dev_lookup_i32(h._ctx, P(k32), 4, -1, None, None, P(cnt), None) == ARG
        assert b"both outputs null" in lib.hj_last_error()
        # (refused before any row is read: the buffers hold 4 rows)
        assert lib.hj_dev_lookup_i32(h._ctx, P(k32), 1 << 31, -1, P(c), P(c), P(cnt), None) == ARG
        assert b"2^31" in lib.hj_last_error()
        assert lib.hj_dev_lookup_i32(h._ctx, P(k32), 1 << 31, -1, None, None, P(cnt), None) == ARG
        assert b"both outputs null" in lib.hj_last_error()
        # both outputs null is fine for an empty S
        assert lib.hj_dev_lookup_i32(h._ctx, None, 0, -1, None, None, P(cnt), None) == _lib.HJ_OK
        torch.cuda.synchronize()
        assert int(cnt.item()) == 0
        with pytest.raises(ValueError):
            h.probe_lookup(k32)
        with pytest.raises(ValueError):
            h.probe_lookup(k32, out_r=o)                   # the key's dtype
        with pytest.raises(ValueError):
            h.probe_lookup(k32, out_cnt=c[:3])             # too short
        with pytest.raises(ValueError):
            h.probe_lookup(k32, out_cnt=o)                 # int32 counts
    finally:
        h.close()


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_reports_lookup(hj, oracle, strategy):
    rk, _, sk, _ = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    rp = payloads(rk, 51)
    timing_reports(hj, strategy, lambda: build(hj, rk, rp), [lambda: check(hj, rk, rp, sk)])


@pytest.mark.parametrize("n,strategy,wide", [(1 << 16, "radix", True), (1 << 12, "global", False)],
                         ids=["i64-2^16-radix", "i32-2^12-global"])
def test_graph_replay(hj, oracle, n, strategy, wide):
    """A captured lookup, replayed after S's keys were overwritten in place."""
    kt = torch.int64 if wide else torch.int32
    if wide:
        rk = oracle.gen_pkfk_i64(61, n, n, 1.0)[0].copy()
        rk[::97] = rk[1::97]   # some build keys twice
        sets = [oracle.gen_pkfk_i64(61, n, n, f)[2] for f in (1.0, 0.5, 0.1)]
    else:
        rk = oracle.gen_uniform_i32(65, 1, 1, 2 * n, n)
        sets = [oracle.gen_uniform_i32(65 + j, 2, 1, hi, n) for j, hi in enumerate((4 * n, n // 4, 2 * n))]
    rp = payloads(rk, 61)
    sk = torch.empty(n, dtype=kt, device="cuda")

    def load(keys):
        sk.copy_(torch.from_numpy(np.ascontiguousarray(keys)))
        torch.cuda.synchronize()

    bits = 64 if wide else 32
    o_r = torch.empty(n, dtype=kt, device="cuda")
    o_c = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def setup():
        hj.allocate_hash_table(n, bits)
        build(hj, rk, rp)
        hj.reserve_probe(n, bits)
        load(sets[0])

    def reload(keys):
        load(keys)
        for t in (o_r, o_c, cnt):
            t.fill_(SENTINEL)

    def verify(keys):
        er, ec = expect(rk, rp, keys)
        assert int(cnt.item()) == int((ec > 0).sum())
        assert np.array_equal(host(o_r), er)
        assert np.array_equal(host(o_c), ec)

    graph_replay(hj, strategy, setup, lambda: hj.probe_lookup(sk, o_r, o_c, null=NULL, count=cnt),
                 sets[1:] + sets[:1], reload, verify)
