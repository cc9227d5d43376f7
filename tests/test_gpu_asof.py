"""As-of probe (hj_dev_asof_*, merge_asof(by=key, on=time)) on both strategies
and both row widths.

Expected results come from numpy on the host, never from the library:
asof_cases.expect sorts R by (key, payload) and bisects per S row.  Results
are compared element by element at the probe row's own position, with no
sorting, and d_count against the numpy count.  int64 payloads are a seeded
permutation around zero, times three plus one: NULL and SENTINEL are
multiples of three, so neither is a payload.  Most builds hold 1-4 copies of
a key, so the bound selects among them; bounds come from the payloads' range
and slightly outside it, a share of them equal to a partner's payload.  Every
case runs all four kinds unless it says otherwise."""
import numpy as np
import pytest
import torch

import asof_cases as AC
import outer_cases as OC
from hashjoin import HashJoin, _lib, lib
from join_gpu import (assert_radix_kernel, build, dev, glob_hj, graph_replay, hj, host, sentinels,  # noqa: F401
                      timing_reports)

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = AC.I64_MIN, AC.I64_MAX
NULL, SENTINEL, EXTRA = -9, -12345, 64   # i32 payloads are row ids (>= 0)


def probe(hj, sk, sb, kind, null=NULL):
    """One as-of probe of the current build into a sentinel-filled output EXTRA
    rows longer than S: (d_count, out_r as an int64 host array)."""
    n = len(sk)
    dt = torch.int64 if sk.dtype == np.int64 else torch.int32
    o_r = sentinels(n + EXTRA, SENTINEL, dt)
    direction, strict = AC.KIND_ARGS[kind]
    m = int(hj.probe_asof(dev(sk), dev(sb), o_r, direction=direction, strict=strict, null=null).item())
    return m, o_r.cpu().numpy().astype(np.int64)


def check(hj, rk, rp, sk, sb, kinds=AC.KINDS, null=NULL):
    """Every kind of `kinds` against numpy; returns {kind: (expected column, found mask)}."""
    n, out = len(sk), {}
    for kind in kinds:
        er, found = AC.expect(rk, rp, sk, sb, kind, null)
        m, g = probe(hj, sk, sb, kind, null)
        assert m == int(found.sum()), (kind, m, int(found.sum()))
        assert np.array_equal(g[:n], er), (kind, np.flatnonzero(g[:n] != er)[:8])
        assert (g[n:] == SENTINEL).all(), kind
        out[kind] = (er, found)
    return out


def selects(res, sk_has_partner):
    """The bound really selects: under each non-strict kind some rows with a
    partner find a candidate and some do not."""
    for kind in (0, 1):
        f = res[kind][1]
        assert 0 < int(f.sum()) < int(sk_has_partner.sum()), kind


def assert_radix(hj):
    assert _lib.HJ_JOIN_KERNEL_ASOF == 11
    assert_radix_kernel(hj, _lib.HJ_JOIN_KERNEL_ASOF, "k_join_asof")


# ------------------------------------------------------------------ global
# (ns = 2 * 2048 + 77 is three tiles, one per workgroup: k_probe_asof never
# strides here, so its load-ahead and hand-over stay idle.  The shape with
# more tiles than workgroups is test_gpu_positional_tiles.py's.)
@pytest.mark.parametrize("nr", [1, 2048, 3000])   # 2048: the last LDS-resident table
def test_global_i64(glob_hj, oracle, nr):
    ns = 2 * 2048 + 77   # a ragged third tile
    rk, _, sk, _ = oracle.gen_pkfk_i64(300 + nr, nr, ns, 0.9)
    rk = AC.versions(rk, nr)
    rp = AC.payloads(rk, nr)
    sb = AC.bounds(rk, rp, sk, nr)
    build(glob_hj, rk, rp)
    res = check(glob_hj, rk, rp, sk, sb)
    if nr > 1:
        assert glob_hj.has_duplicates()
        selects(res, OC.Expect(rk, sk).cnt > 0)
    assert glob_hj.strategy_used == "global" and glob_hj.join_kernel is None


@pytest.mark.parametrize("nr", [4000, 5000])   # either side of a 64-KiB table
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    r[1000:1300] = r[:300]    # some keys twice
    r[2000:2300] = r[:300]    # and three times
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 2 * 2048 + 77 - len(r[::3]))])
    rp = AC.payloads(r)
    sb = AC.bounds(r, rp, s, nr)
    assert (sb < 0).any() and (sb > nr).any()   # bounds before the first row and past the last
    build(glob_hj, r, None)
    res = check(glob_hj, r, rp, s, sb)
    selects(res, OC.Expect(r, s).cnt > 0)


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
def test_global_repeated_build_keys(glob_hj, dtype):
    """One key 502 times: its chain is walked to EMPTY, and each of its 301
    probe rows picks its own partner."""
    rk, sk = AC.repeated_keys_case(dtype)
    rp = AC.payloads(rk, 3)
    sb = AC.bounds(rk, rp, sk, 3, exact=0.3)
    build(glob_hj, rk, rp)
    assert glob_hj.has_duplicates()
    res = check(glob_hj, rk, rp, sk, sb)
    vals, copies = np.unique(rk, return_counts=True)
    hot = sk == vals[copies.argmax()]
    assert copies.max() == 502 and hot.sum() == 301 and len(np.unique(res[0][0][hot])) > 100
    assert glob_hj.has_duplicates()


def test_global_unique_build_keys(glob_hj, oracle):
    """No repeated build key: the walk stops at the first equal key whether or
    not its payload qualifies."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(19, 3000, 2 * 2048 + 77, 0.8)
    rp = AC.payloads(rk, 19)
    sb = AC.bounds(rk, rp, sk, 19)
    build(glob_hj, rk, rp)
    assert not glob_hj.has_duplicates()
    res = check(glob_hj, rk, rp, sk, sb)
    selects(res, OC.Expect(rk, sk).cnt > 0)
    assert not glob_hj.has_duplicates()


def int64_min_case(oracle, where, nr=1500, ns=2 * 2048 + 77, seed=12):
    """Keys with INT64_MIN on either side; the INT64_MIN build rows' payloads
    straddle the bounds of the INT64_MIN probe rows."""
    rk = AC.versions(oracle.gen_uniform_i64(seed, 1, -2000, 2000, nr)[0].copy(), seed)
    sk = oracle.gen_uniform_i64(seed, 2, -3000, 3000, ns)[0].copy()
    if where in ("both", "build"):
        rk[::nr // 5] = I64_MIN
    if where in ("both", "probe"):
        sk[::ns // 9] = I64_MIN
    rp = AC.payloads(rk, seed)
    sb = AC.bounds(rk, rp, sk, seed)
    if where == "both":
        side = np.sort(rp[rk == I64_MIN])
        at = np.flatnonzero(sk == I64_MIN)
        assert len(side) >= 5 and len(at) >= 9
        # below all, between each pair, on one, above all
        sb[at[:7]] = [side[0] - 1, side[0], side[0] + 1, side[2], side[2] + 1, side[-1], side[-1] + 1]
    return rk, rp, sk, sb


@pytest.mark.parametrize("where", ["probe", "build", "both"])
def test_global_int64_min(glob_hj, oracle, where):
    rk, rp, sk, sb = int64_min_case(oracle, where)
    build(glob_hj, rk, rp)
    res = check(glob_hj, rk, rp, sk, sb)
    nul = sk == I64_MIN
    if where == "both":
        assert 0 < res[0][1][nul].sum() < nul.sum() and len(np.unique(res[0][0][nul])) >= 4
    if where == "probe":
        assert not res[0][1][nul].any() and nul.any()


# ------------------------------------------------------------------ radix
# one pass of the half-size workgroups, one of the full-size ones (S's row
# index enters in the first pass: both of its variants), and a two-pass plan
@pytest.mark.parametrize("bits", [1, 9, 17])
def test_radix_pkfk(hj, oracle, bits):
    rk, _, sk, _ = oracle.gen_pkfk_i64(bits, 20000, 50000, 0.9)
    rk = AC.versions(rk, bits)
    rp = AC.payloads(rk, bits)
    sb = AC.bounds(rk, rp, sk, bits)
    hj.set_strategy("radix", radix_bits=bits)
    try:
        build(hj, rk, rp)
        assert hj.radix_passes == {1: 1, 9: 1, 17: 2}[bits]
        res = check(hj, rk, rp, sk, sb)
        selects(res, OC.Expect(rk, sk).cnt > 0)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("hot", [False, True], ids=["distinct", "hot-key"])
def test_radix_over_one_round(hj, oracle, hot):
    """30000 build rows per partition: several build rounds whose tables hold
    different keys, the sub-chunks-outermost path.  hot-key: one key's 20000
    copies span the rounds -- the best is carried across them and must be the
    global one."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(77, 60000, 40000, 0.7)
    rk = AC.versions(rk, 77)
    sk = sk.copy()
    if hot:
        rk[np.random.default_rng(1).permutation(60000)[:20000]] = 42
        sk[::40] = 42
    rp = AC.payloads(rk, 6)
    sb = AC.bounds(rk, rp, sk, 6)
    hj.set_strategy("radix", radix_bits=1)
    try:
        build(hj, rk, rp)
        res = check(hj, rk, rp, sk, sb)
        if hot:
            at = sk == 42
            assert at.sum() == 1000 and res[0][1][at].sum() > 800 and len(np.unique(res[0][0][at])) > 500
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_partitions_without_build_rows(hj):
    """2^10 partitions, 50 build rows: most S rows lie in partitions without
    any -- the kernel itself writes their null, nothing prefills."""
    rk = np.repeat(np.arange(25, dtype=np.int64) * 1000003 + 17, 2)
    rng = np.random.default_rng(5)
    sk = rng.integers(1 << 40, 1 << 41, 30000, dtype=np.int64)
    hit = rng.random(30000) < 0.5
    sk[hit] = rk[rng.integers(0, 50, int(hit.sum()))]
    rp = AC.payloads(rk, 2)
    sb = AC.bounds(rk, rp, sk, 2)
    hj.set_strategy("radix", radix_bits=10)
    try:
        build(hj, rk, rp)
        res = check(hj, rk, rp, sk, sb)
        selects(res, hit)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_hot_probe_key_many_chunks(hj):
    """One probe key 50000 times over many sub-chunks, each row its own bound."""
    rk = np.concatenate([np.arange(3000, dtype=np.int64) * 7, np.full(3, 21, np.int64)])
    sk = np.concatenate([np.full(50000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    sk = sk[np.random.default_rng(3).permutation(len(sk))]
    rp = AC.payloads(rk, 4)
    sb = AC.bounds(rk, rp, sk, 4, exact=0.1)
    assert len(np.unique(sb[sk == 21])) > 2000
    hj.set_strategy("radix", radix_bits=6)
    try:
        build(hj, rk, rp)
        res = check(hj, rk, rp, sk, sb)
        assert len(np.unique(res[0][0][sk == 21])) == 5   # the four copies and the null
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


def test_radix_int64_min_inside_rounds(hj, oracle):
    """INT64_MIN build rows inside a multi-round partition and INT64_MIN probe
    rows in several sub-chunks: the list in the payload words and the rebuild
    per sub-chunk."""
    rk, rp, sk, sb = int64_min_case(oracle, "both", nr=30000, ns=20000, seed=14)
    assert (rk == I64_MIN).sum() >= 5
    hj.set_strategy("radix", radix_bits=1)
    try:
        build(hj, rk, rp)
        res = check(hj, rk, rp, sk, sb)
        nul = sk == I64_MIN
        assert 0 < res[0][1][nul].sum() < nul.sum()
        assert_radix(hj)
        # and in a single-round partition of two sub-chunks, whose table is rebuilt only because of the list
        hj.set_strategy("radix", radix_bits=2)
        rk2, rp2, sk2, sb2 = int64_min_case(oracle, "both", nr=3000, ns=20000, seed=15)
        build(hj, rk2, rp2)
        check(hj, rk2, rp2, sk2, sb2)
        assert_radix(hj)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("bits", [1, 9])
def test_radix_i32(hj, oracle, bits):
    r = oracle.gen_uniform_i32(bits, 1, -(1 << 31), (1 << 31) - 1, 30000)
    r[1000:1300] = r[:300]   # some keys twice
    r[2000:2300] = r[:300]   # and three times
    s = np.concatenate([r[::3], oracle.gen_uniform_i32(bits, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    rp = AC.payloads(r)
    sb = AC.bounds(r, rp, s, bits)
    hj.set_strategy("radix", radix_bits=bits)
    try:
        build(hj, r, None)
        res = check(hj, r, rp, s, sb)
        selects(res, OC.Expect(r, s).cnt > 0)
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
            rp = AC.payloads(rk, 8)
            for sb in (np.full(len(sk), 1, dt), np.full(len(sk), -2, dt), np.arange(len(sk)).astype(dt)):
                build(hj, rk, rp)
                res = check(hj, rk, rp, sk, sb)
                assert hj.strategy_used == strategy
                if len(rk) == 0:
                    assert all((er == NULL).all() and not f.any() for er, f in res.values())
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_extremes_i64(hj, strategy):
    """Bounds INT64_MIN and INT64_MAX under all four kinds, payloads INT64_MIN
    and INT64_MAX in R, and a null value that equals a real payload: validity
    is the found bit, never a sentinel, and strict is no bound +- 1."""
    rk = np.array([1, 1, 1, 2, 2, 3, 4, 4, 4, 5], np.int64)
    rp = np.array([I64_MIN, 0, I64_MAX, I64_MIN, I64_MAX, I64_MIN, -7, 7, I64_MAX, I64_MAX], np.int64)
    keys = np.array([1, 2, 3, 4, 5, 6], np.int64)
    vals = np.array([I64_MIN, I64_MIN + 1, -7, 0, 7, I64_MAX - 1, I64_MAX], np.int64)
    sk, sb = np.repeat(keys, len(vals)), np.tile(vals, len(keys))
    hj.set_strategy(strategy, radix_bits=2 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        for null in (NULL, 0, I64_MIN, I64_MAX):   # 0, INT64_MIN, INT64_MAX are payloads
            res = check(hj, rk, rp, sk, sb, null=null)
        lo, hi = sb == I64_MIN, sb == I64_MAX
        assert not res[2][1][lo].any() and not res[3][1][hi].any()   # strict: nothing below the least, above the greatest
        assert res[0][1][lo & (sk <= 3)].all() and res[1][1][hi & np.isin(sk, (1, 2, 4, 5))].all()
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_extremes_i32(hj, strategy):
    """i32: row ids zero-extended, bounds sign-extended -- INT32_MIN is below
    every row and INT32_MAX above it; a null row that is a real row id."""
    rk = np.array([1, 1, 2, 3, 1], np.int32)
    keys = np.array([1, 2, 3, 4], np.int32)
    vals = np.array([-(1 << 31), -1, 0, 1, 3, 4, 5, (1 << 31) - 1], np.int32)
    sk, sb = np.repeat(keys, len(vals)), np.tile(vals, len(keys))
    hj.set_strategy(strategy, radix_bits=2 if strategy == "radix" else 0)
    try:
        build(hj, rk, None)
        for null in (-1, 0, 4):
            res = check(hj, rk, AC.payloads(rk), sk, sb, null=null)
        assert not res[0][1][sb < 0].any() and res[1][1][(sb < 0) & (sk < 4)].all()
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
def test_strategies_agree_bit_for_bit(hj, oracle, wide):
    if wide:
        rk = AC.versions(oracle.gen_uniform_i64(33, 1, 1, 1 << 40, 9000)[0].copy(), 33)
        sk = np.concatenate([rk[::2], oracle.gen_uniform_i64(33, 2, 1, 1 << 40, 4501)[0]])
        rk[::1000] = sk[::900] = I64_MIN
    else:
        rk = AC.versions(oracle.gen_uniform_i32(33, 1, 1, 1 << 30, 9000), 33)
        sk = np.concatenate([rk[::2], oracle.gen_uniform_i32(33, 2, 1, 1 << 30, 4501)])
    rp = AC.payloads(rk, 33)
    sb = AC.bounds(rk, rp, sk, 33)
    got = {}
    try:
        for strategy in ("global", "radix"):
            hj.set_strategy(strategy, radix_bits=4 if strategy == "radix" else 0)
            build(hj, rk, rp)
            got[strategy] = [probe(hj, sk, sb, kind) for kind in AC.KINDS]
            assert hj.strategy_used == strategy
        check(hj, rk, rp, sk, sb)   # (and the last build's against numpy)
    finally:
        hj.set_strategy("auto")
    for (mg, g), (mr, r) in zip(got["global"], got["radix"]):
        assert mg == mr and np.array_equal(g, r)


def _sorted(cnt, *cols):
    m = int(cnt.item())
    a = [c[:m].cpu().numpy() for c in cols]
    o = np.lexsort(tuple(reversed(a)))
    return [c[o] for c in a]


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_one_build_serves_every_probe(hj, oracle, strategy):
    """inner -> as-of -> lookup -> full -> as-of of one build: each result
    equals its first, and the repeat flag keeps its answer."""
    rk = oracle.gen_uniform_i64(41, 1, 1, 4000, 12000)[0].copy()
    sk = oracle.gen_uniform_i64(41, 2, 1, 6000, 9000)[0].copy()
    rk[::97] = I64_MIN
    sk[::131] = I64_MIN
    rp = AC.payloads(rk, 41)
    sb = AC.bounds(rk, rp, sk, 41)
    d_sk, d_sp = dev(sk), dev(np.arange(9000, dtype=np.int64))
    cap = int(OC.Expect(rk, sk).m("full")) + 8
    o_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    o_s = torch.empty_like(o_r)
    l_r = torch.empty(9000, dtype=torch.int64, device="cuda")

    def inner():
        return _sorted(hj.probe_relation(d_sk, d_sp, o_r, o_s), o_r, o_s)

    def lookup():
        m = int(hj.probe_lookup(d_sk, l_r, None, null=NULL).item())
        return [np.array([m]), l_r.cpu().numpy()]

    def full():
        return _sorted(hj.probe_full(d_sk, d_sp, o_r, o_s, kind="full", null_r=NULL, null_s=NULL), o_r, o_s)

    hj.set_strategy(strategy, radix_bits=10 if strategy == "radix" else 0)
    try:
        build(hj, rk, rp)
        first = {"inner": inner()}
        dups = hj.has_duplicates()
        assert dups
        check(hj, rk, rp, sk, sb)
        first["lookup"] = lookup()
        first["full"] = full()
        assert hj.join_kernel != "k_join_asof"
        check(hj, rk, rp, sk, sb)
        if strategy == "radix":
            assert_radix(hj)
        for name, f in (("inner", inner), ("lookup", lookup), ("full", full)):
            again = f()
            assert all(np.array_equal(a, b) for a, b in zip(first[name], again)), name
        assert len(first["inner"][0]) == OC.Expect(rk, sk).pairs
        assert hj.has_duplicates() == dups
        # and a build without repeats keeps saying so after an as-of probe
        uk = np.arange(12000, dtype=np.int64) * 5
        up = AC.payloads(uk, 42)
        build(hj, uk, up)
        check(hj, uk, up, sk, sb, kinds=(0, 3))
        assert not hj.has_duplicates()
    finally:
        hj.set_strategy("auto")


def test_asof_method(hj, oracle):
    rk, _, sk, _ = oracle.gen_pkfk_i64(31, 3000, 9000, 0.6)
    rk = AC.versions(rk, 31)
    rp = AC.payloads(rk, 31)
    sb = AC.bounds(rk, rp, sk, 31)
    got = hj.asof(dev(rk), dev(rp), dev(sk), dev(sb), direction="forward", strict=True, null=NULL)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), AC.expect(rk, rp, sk, sb, 3, NULL)[0])
    # rpay None: "the last R row with this key at or before row b"
    rows = np.arange(len(rk), dtype=np.int64)
    b = AC.bounds(rk, rows, sk, 32)
    idx = hj.asof(dev(rk), None, dev(sk), dev(b))
    ei, found = AC.expect(rk, rows, sk, b, 0, -1)
    assert np.array_equal(idx.cpu().numpy(), ei)
    assert np.array_equal(rk[ei[found]], sk[found]) and (ei[found] <= b[found]).all()
    r32, s32, b32 = rk.astype(np.int32), sk.astype(np.int32), b.astype(np.int32)   # (the keys' low words)
    i32 = hj.asof(dev(r32), None, dev(s32), dev(b32))
    e32, f32 = AC.expect(r32, rows, s32, b32, 0, -1)
    assert i32.dtype == torch.int32 and np.array_equal(i32.cpu().numpy().astype(np.int64), e32)
    # out_r None: probe_asof allocates the column
    cnt = hj.probe_asof(dev(s32), dev(b32))
    assert int(cnt.item()) == int(f32.sum())
    assert np.array_equal(hj.asof_out.cpu().numpy().astype(np.int64), e32)


def test_errors_in_order():
    """null context; a bad kind; no build of that layout; null count pointer,
    null skey / sbound / out_r with n > 0, n < 0; i32: n > INT32_MAX."""
    h = HashJoin(0)
    try:
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = torch.zeros(4, dtype=torch.int64, device="cuda")
        k32 = k.to(torch.int32)
        o = torch.zeros(4, dtype=torch.int64, device="cuda")
        o32 = o.to(torch.int32)
        P = lambda t: t.data_ptr()   # noqa: E731
        ARG, STATE = _lib.HJ_ERR_ARG, _lib.HJ_ERR_STATE
        f64, f32 = lib.hj_dev_asof_i64, lib.hj_dev_asof_i32
        # everything else wrong too: the context comes first, then the kind, then the state
        assert f64(None, 4, None, None, -1, -1, None, None, None) == ARG
        assert b"null context" in lib.hj_last_error()
        for kind in (4, -1, 8):
            assert f64(h._ctx, kind, None, None, -1, -1, None, None, None) == ARG
            assert b"kind" in lib.hj_last_error()
        assert f64(h._ctx, 3, None, None, -1, -1, None, None, None) == STATE   # a probe before a build
        h.build_table(k32)
        assert f64(h._ctx, 0, P(k), P(k), 4, -1, P(o), P(cnt), None) == STATE   # an i32 build
        assert f32(h._ctx, 0, None, None, 4, -1, None, None, None) == ARG
        assert b"count pointer" in lib.hj_last_error()
        assert f32(h._ctx, 0, None, P(k32), 4, -1, P(o32), P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert f32(h._ctx, 0, P(k32), P(k32), -1, -1, P(o32), P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert f32(h._ctx, 1, P(k32), None, 4, -1, P(o32), P(cnt), None) == ARG
        assert b"bound" in lib.hj_last_error()
        assert f32(h._ctx, 2, P(k32), P(k32), 4, -1, None, P(cnt), None) == ARG
        assert b"output" in lib.hj_last_error()
        # (refused before any row is read: the buffers hold 4 rows)
        assert f32(h._ctx, 0, P(k32), P(k32), 1 << 31, -1, P(o32), P(cnt), None) == ARG
        assert b"2^31" in lib.hj_last_error()
        # every pointer null is fine for an empty S
        assert f32(h._ctx, 3, None, None, 0, -1, None, P(cnt), None) == _lib.HJ_OK
        torch.cuda.synchronize()
        assert int(cnt.item()) == 0
        with pytest.raises(ValueError):
            h.probe_asof(k32, k)                           # the key's dtype
        with pytest.raises(ValueError):
            h.probe_asof(k32, k32[:3])                     # and its length
        with pytest.raises(ValueError):
            h.probe_asof(k32, k32, out_r=o32[:3])          # too short
        with pytest.raises(KeyError):
            h.probe_asof(k32, k32, direction="nearest")    # asof_join's
    finally:
        h.close()


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_reports_asof(hj, oracle, strategy):
    rk, _, sk, _ = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    rp = AC.payloads(rk, 51)
    sb = AC.bounds(rk, rp, sk, 51)
    timing_reports(hj, strategy, lambda: build(hj, rk, rp), [lambda: check(hj, rk, rp, sk, sb, kinds=(0,))])


@pytest.mark.parametrize("strategy,wide", [("radix", True), ("global", False)], ids=["i64-radix", "i32-global"])
def test_graph_replay(hj, oracle, strategy, wide):
    """Build + as-of probe captured as one linear graph on one stream, replayed
    over new data in the same buffers."""
    n = 9001
    kt = torch.int64 if wide else torch.int32
    sets = []
    for seed in (61, 62, 63):
        if wide:
            rk, _, sk, _ = oracle.gen_pkfk_i64(seed, n, n, 0.8)
            rk, sk = AC.versions(rk, seed), sk.copy()
            rk[::977] = sk[::1009] = I64_MIN
        else:
            rk = AC.versions(oracle.gen_uniform_i32(seed, 1, 1, 4 * n, n), seed)
            sk = np.concatenate([rk[::2], oracle.gen_uniform_i32(seed, 2, 1, 4 * n, n - len(rk[::2]))])
        rp = AC.payloads(rk, seed)
        sets.append((rk, rp, sk, AC.bounds(rk, rp, sk, seed)))
    d_rk, d_sk, d_sb = (torch.empty(n, dtype=kt, device="cuda") for _ in range(3))
    d_rp = torch.empty(n, dtype=torch.int64, device="cuda") if wide else None

    def load(rk, rp, sk, sb):
        for t, x in ((d_rk, rk), (d_rp, rp), (d_sk, sk), (d_sb, sb)):
            if t is not None:
                t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        torch.cuda.synchronize()

    bits = 64 if wide else 32
    o_r = torch.empty(n, dtype=kt, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def setup():
        load(*sets[0])
        hj.allocate_hash_table(n, bits)
        hj.build_table(d_rk, d_rp)
        hj.reserve_probe(n, bits)

    def step():
        hj.build_table(d_rk, d_rp)
        hj.probe_asof(d_sk, d_sb, o_r, null=NULL, count=cnt)

    def reload(data):
        load(*data)
        o_r.fill_(SENTINEL)
        cnt.fill_(SENTINEL)

    def verify(data):
        er, found = AC.expect(*data, 0, NULL)
        assert int(cnt.item()) == int(found.sum())
        assert np.array_equal(host(o_r), er)

    graph_replay(hj, strategy, setup, step, sets[1:] + sets[:1], reload, verify)


# ------------------------------------------------------------------ asof_join
def join_case(nr, ns, seed, span=60):
    """Unsorted relations of few keys and few distinct times: duplicate (key,
    time) rows in R, S times below and above every R time."""
    rng = np.random.default_rng(seed)
    rk = rng.integers(0, 12, nr, dtype=np.int64) * 1000003 - 5
    rt = rng.integers(-span, span, nr, dtype=np.int64) * 10
    sk = rng.integers(0, 14, ns, dtype=np.int64) * 1000003 - 5
    st = rng.integers(-span - 20, span + 20, ns, dtype=np.int64) * 10 + rng.integers(0, 2, ns) * 5
    return rk, rt, sk, st


@pytest.mark.parametrize("nr", [256, 257], ids=["pow2", "pow2+1"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_asof_join(hj, strategy, nr):
    rk, rt, sk, st = join_case(nr, 700, nr)
    key_time = rk * 100000 + rt
    assert len(np.unique(key_time)) < nr                      # duplicate (key, time) rows
    assert st.min() < rt.min() and st.max() > rt.max()
    assert ((st[:, None] == rt[None, :]) & (sk[:, None] == rk[None, :])).any()   # exact matches
    hj.set_strategy(strategy, radix_bits=3 if strategy == "radix" else 0)
    try:
        for direction in ("backward", "forward", "nearest"):
            for exact in (True, False):
                for tol in (None, 25):
                    got = hj.asof_join(dev(rk), dev(rt), dev(sk), dev(st), direction=direction,
                                       allow_exact_matches=exact, tolerance=tol).cpu().numpy()
                    want = AC.asof_join_loop(rk, rt, sk, st, direction, exact, tol)
                    assert np.array_equal(got, want), (direction, exact, tol, np.flatnonzero(got != want)[:8])
                    assert (want >= 0).any() and (want < 0).any()
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


def test_asof_join_nearest_tie_and_duplicates(hj):
    rk = np.array([1, 1, 1, 1, 2], np.int64)
    rt = np.array([20, 10, 10, 20, 15], np.int64)
    sk = np.array([1, 1, 1, 1, 2, 3], np.int64)
    st = np.array([15, 10, 20, 30, 15, 15], np.int64)
    d = lambda *a: [dev(x) for x in a]   # noqa: E731
    assert hj.asof_join(*d(rk, rt, sk, st)).cpu().tolist() == [2, 2, 3, 3, 4, -1]                          # the last of equals
    assert hj.asof_join(*d(rk, rt, sk, st), direction="forward").cpu().tolist() == [0, 1, 0, -1, 4, -1]   # the first
    assert hj.asof_join(*d(rk, rt, sk, st), direction="nearest").cpu().tolist() == [2, 2, 3, 3, 4, -1]    # 15: a tie, backward
    for direction in ("backward", "forward", "nearest"):
        want = AC.asof_join_loop(rk, rt, sk, st, direction)
        assert hj.asof_join(*d(rk, rt, sk, st), direction=direction).cpu().tolist() == want.tolist()
    e = np.empty(0, np.int64)
    assert hj.asof_join(*d(e, e, sk, st)).cpu().tolist() == [-1] * 6
    assert hj.asof_join(*d(rk, rt, e, e)).numel() == 0


def test_asof_join_refuses_what_does_not_pack(hj):
    rk = np.array([1, 1, 2, 2], np.int64)
    rt = np.array([0, 1 << 62, 5, 6], np.int64)
    with pytest.raises(ValueError):
        hj.asof_join(dev(rk), dev(rt), dev(rk), dev(rt))
    # 2^60 with 2 row bits packs: 61 + 2 = 63
    rt = np.array([-(1 << 59), 1 << 59, 5, 6], np.int64)
    got = hj.asof_join(dev(rk), dev(rt), dev(rk), dev(rt)).cpu().tolist()
    assert got == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        hj.asof_join(dev(rk), dev(rt), dev(rk), dev(rt), direction="sideways")
