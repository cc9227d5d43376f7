"""Group probe (join, then aggregate per build row; hj_dev_group_*) on both
strategies and both row widths.

Expected results come from numpy on the host (group_cases.expect: S sorted by
key, np.add / np.minimum / np.maximum.reduceat per distinct key), never from
the library.  Every case compares all five columns after sorting by R payload
(R payloads are distinct), for both kinds unless noted.  int64 values span the
whole range, so sums wrap, and include INT64_MIN / INT64_MAX; i32 values are
the S row ids.  Outputs are SENTINEL-filled and EXTRA rows longer than the
capacity passed: nothing may be written at or past it."""
import numpy as np
import pytest
import torch

import group_cases as GC
import outer_cases as OC
import routed_layout as RL
from hashjoin import HashJoin, _lib, lib
from join_gpu import assert_radix_kernel, build, dev, glob_hj, graph_replay, hj, host, sentinels  # noqa: F401

pytestmark = pytest.mark.gpu

I64_MIN = OC.I64_MIN
NULL, SENTINEL, EXTRA = -9, -12345, 64
COLS = GC.COLS
HOWS = ("matched", "all")


def s_values(sk, seed=5, row_base=0):
    """S's value column: int64 the whole range, i32 the row ids."""
    if sk.dtype == np.int32:
        return np.arange(len(sk), dtype=np.int64) + row_base
    return GC.values(len(sk), seed)


def run(hj, sk, sv, how, cap, cols=COLS, tuples=False, row_base=0):
    """One group probe of the current build with out_cap = cap: (M, {col: the
    whole SENTINEL-filled buffer of cap + EXTRA elements as int64})."""
    wide = sk.dtype == np.int64
    dt = torch.int64 if wide else torch.int32
    bufs = {c: sentinels(cap + EXTRA, SENTINEL, torch.int64 if c == "sum" else dt)
            for c in cols}
    o = {c: (bufs[c][:cap] if c in bufs else None) for c in COLS}
    kw = dict(how=how, out_r=o["r"], out_cnt=o["cnt"], out_sum=o["sum"], out_min=o["min"], out_max=o["max"], null=NULL)
    if tuples:
        m = hj.probe_group_tuples(dev(np.stack([sk, sv], axis=1)), **kw)
    elif wide:
        needs_val = any(c in cols for c in ("sum", "min", "max"))
        m = hj.probe_group(dev(sk), dev(sv) if needs_val else None, **kw)
    else:
        m = hj.probe_group(dev(sk), None, row_base=row_base, **kw)
    return int(m.item()), {c: b.cpu().numpy().astype(np.int64) for c, b in bufs.items()}


def check(hj, rk, rp, sk, sv, hows=HOWS, cols=COLS, tuples=False, row_base=0):
    """Both kinds against numpy, all rows; returns the expectations by kind."""
    out = {}
    for how in hows:
        e = GC.expect(rk, rp, sk, sv, how, NULL)
        m_exp = len(e["r"])
        cap = max(1, len(rk))
        m, got = run(hj, sk, sv, how, cap, cols, tuples, row_base)
        assert m == m_exp, (how, m, m_exp)
        o = np.argsort(got["r"][:m], kind="stable") if "r" in cols else None
        for c in cols:
            g = got[c][:m]
            # without the payload column the rows have no name: the column's multiset
            g, want = (g[o], e[c]) if o is not None else (np.sort(g), np.sort(e[c]))
            assert np.array_equal(g, want), (how, c, np.flatnonzero(g != want)[:8])
            assert (got[c][m:] == SENTINEL).all(), (how, c)
        out[how] = e
    return out


def assert_radix(hj):
    assert _lib.HJ_JOIN_KERNEL_GROUP == 8
    assert_radix_kernel(hj, _lib.HJ_JOIN_KERNEL_GROUP, "k_join_group")


def radix_case(hj, bits, rk, sk, seed=3, **kw):
    rp, sv = GC.payloads(rk, seed), s_values(sk, seed)
    hj.set_strategy("radix", radix_bits=bits)
    try:
        build(hj, rk, rp)
        e = check(hj, rk, rp, sk, sv, **kw)
        assert_radix(hj)
        return e
    finally:
        hj.set_strategy("auto")


# ------------------------------------------------------------------ global
@pytest.mark.parametrize("nr", [1, 2048, 3000])
def test_global_i64(glob_hj, oracle, nr):
    ns = 9 * 2048 + 77   # a ragged last tile
    rk, _, sk, _ = oracle.gen_pkfk_i64(300 + nr, nr, ns, 0.6)
    rp, sv = GC.payloads(rk, nr), s_values(sk, nr)
    build(glob_hj, rk, rp)
    e = check(glob_hj, rk, rp, sk, sv)
    assert 0 < len(e["matched"]["r"]) <= nr == len(e["all"]["r"])
    assert glob_hj.strategy_used == "global" and glob_hj.join_kernel is None


@pytest.mark.parametrize("nr", [4000, 5000])
def test_global_i32(glob_hj, oracle, nr):
    r = oracle.gen_uniform_i32(nr, 1, -(1 << 31), (1 << 31) - 1, nr)
    s = np.concatenate([r[::3], r[::6], oracle.gen_uniform_i32(nr, 2, -(1 << 31), (1 << 31) - 1, 15000)])
    build(glob_hj, r, None)
    e = check(glob_hj, r, GC.payloads(r), s, s_values(s))
    assert e["all"]["cnt"].max() >= 2 and (e["all"]["cnt"] == 0).any()


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
    """Every copy of a repeated build key is a row of its own with the whole group."""
    rk, sk = repeated_keys_case(dtype)
    rp, sv = GC.payloads(rk, 3), s_values(sk, 3)
    build(glob_hj, rk, rp)
    assert glob_hj.has_duplicates()
    e = check(glob_hj, rk, rp, sk, sv)
    assert len(e["all"]["r"]) == len(rk)
    assert int((e["all"]["cnt"] == 6).sum()) == 502   # base[7]: 502 copies, 1 + 5 S rows
    assert glob_hj.has_duplicates()


@pytest.mark.parametrize("where", ["probe", "build", "both"])
def test_global_int64_min(glob_hj, oracle, where):
    rk = oracle.gen_uniform_i64(12, 1, -2000, 2000, 1500)[0].copy()
    sk = oracle.gen_uniform_i64(12, 2, -2000, 2000, 20000)[0].copy()
    if where in ("build", "both"):
        rk[::500] = I64_MIN
    if where in ("probe", "both"):
        sk[::1777] = I64_MIN
    rp, sv = GC.payloads(rk, 12), s_values(sk, 12)
    build(glob_hj, rk, rp)
    e = check(glob_hj, rk, rp, sk, sv)["all"]
    side = np.isin(e["r"], rp[rk == I64_MIN])
    assert int(side.sum()) == (3 if where != "probe" else 0)
    if where == "both":
        assert (e["cnt"][side] == len(sk[::1777])).all()
    if where == "build":
        assert (e["cnt"][side] == 0).all() and (e["min"][side] == NULL).all()


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
def test_global_strided_tiles(glob_hj, wide):
    """The slot scan's persistent loop takes a second tile (|R| = 2^21 + 5) over 8 x CUs + 60 probe tiles."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = OC.strided_general_case(cus)
    dt = np.int64 if wide else np.int32
    rk, sk = c["rk"].astype(dt), c["sk"].astype(dt)
    rp, sv = GC.payloads(rk, 2), s_values(sk, 2)
    build(glob_hj, rk, rp)
    assert glob_hj.capacity == c["slots"]
    e = check(glob_hj, rk, rp, sk, sv)
    assert e["all"]["cnt"].max() >= c["tiles"]   # the key every tile holds


# ------------------------------------------------------------------ radix, int64
@pytest.mark.parametrize("bits", [1, 9, 17])
def test_radix_pkfk(hj, oracle, bits):
    rk, _, sk, _ = oracle.gen_pkfk_i64(bits, 20000, 50000, 0.8)
    e = radix_case(hj, bits, rk, sk, seed=bits)
    assert 0 < len(e["matched"]["r"]) < 20000


@pytest.mark.parametrize("name", [n for n in OC.RADIX_SHAPES if n != "grp-i32"])
def test_radix_shapes(hj, oracle, name):
    c = OC.radix_path_case(oracle, name)
    e = radix_case(hj, c["bits"], c["rk"], c["sk"], seed=7)
    assert (e["all"]["cnt"] == 0).any() and (e["all"]["cnt"] > 0).any()


def test_radix_fresh_context():
    """A new context, 2^10 partitions: most hold build rows only (50 probe
    rows: ALL's empty groups), then a 200000-row probe side."""
    c = OC.fresh_context_case()
    rp = GC.payloads(c["rk"], 9)
    h = HashJoin(0)
    try:
        h.set_strategy("radix", radix_bits=c["bits"])
        build(h, c["rk"], rp)
        for sk in (c["sk"], c["big"]):
            e = check(h, c["rk"], rp, sk, s_values(sk, 9))
            assert_radix(h)
            assert len(e["all"]["r"]) == 30000
    finally:
        h.close()


def test_radix_partitions_without_build_rows(hj):
    """2^10 partitions, 50 build rows: most S rows lie in partitions without any, and nothing is emitted for them."""
    rk = np.arange(50, dtype=np.int64) * 1000003 + 17
    rng = np.random.default_rng(5)
    sk = rng.integers(1 << 40, 1 << 41, 30000, dtype=np.int64)
    hit = rng.random(30000) < 0.5
    sk[hit] = rk[rng.integers(0, 50, int(hit.sum()))]
    e = radix_case(hj, 10, rk, sk)
    assert len(e["matched"]["r"]) == 50


def test_radix_hot_probe_key(hj):
    """One S key 70,000 times with values of both signs, two partitions: many
    rounds, a slot's count of 2560 in a round, a running count past 16 bits."""
    rk = np.arange(3000, dtype=np.int64) * 7
    sk = np.concatenate([np.full(70000, 21, np.int64), np.arange(0, 30000, 3, dtype=np.int64)])
    sk = sk[np.random.default_rng(3).permutation(len(sk))]
    e = radix_case(hj, 1, rk, sk)["all"]
    assert e["cnt"].max() == 70001 > 65535


def test_radix_distinct_keys_over_one_round(hj, oracle):
    """20000 distinct S keys per partition: several rounds whose tables hold different keys."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(77, 3000, 3000, 1.0)
    sk = np.concatenate([sk, (1 << 44) + np.arange(40000, dtype=np.int64)])
    assert len(np.unique(sk)) > 2 * 5120 + 3000
    radix_case(hj, 1, rk, sk)


def test_radix_many_build_rows_and_probe_rounds(hj, oracle):
    """10000 R rows and 15000 S rows per partition: S is read again for every R sub-chunk, nothing twice."""
    rk, _, sk, _ = oracle.gen_pkfk_i64(78, 20000, 30000, 0.7)
    e = radix_case(hj, 1, rk, sk)
    assert int(e["all"]["cnt"].sum()) == OC.Expect(rk, sk).pairs


# ------------------------------------------------------------------ radix, i32
@pytest.mark.parametrize("bits", [1, 9])
def test_radix_i32(hj, oracle, bits):
    r = oracle.gen_uniform_i32(bits, 1, -(1 << 31), (1 << 31) - 1, 30000)
    r[1000:1300] = r[:300]   # some build keys twice
    s = np.concatenate([r[::3], r[::7], oracle.gen_uniform_i32(bits, 2, -(1 << 31), (1 << 31) - 1, 10000)])
    e = radix_case(hj, bits, r, s)
    assert e["all"]["cnt"].max() >= 2


def test_radix_i32_grouped_shape(hj, oracle):
    c = OC.radix_path_case(oracle, "grp-i32")
    radix_case(hj, c["bits"], c["rk"], c["sk"])


# ------------------------------------------------------------------ both strategies
def small_case(oracle, wide, seed=23):
    if wide:
        rk, _, sk, _ = oracle.gen_pkfk_i64(seed, 3000, 9001, 0.5)
        rk, sk = rk.copy(), sk.copy()
        rk[::400] = I64_MIN
        sk[::900] = I64_MIN
        return rk, sk
    r = oracle.gen_uniform_i32(seed, 1, 1, 6000, 3000)
    return r, oracle.gen_uniform_i32(seed, 2, 1, 9000, 9001)


def with_strategy(hj, strategy, bits=5):
    hj.set_strategy(strategy, radix_bits=bits if strategy == "radix" else 0)


@pytest.mark.parametrize("cols", [("r",), ("cnt",), ("sum",), ("min",), ("max",), ("cnt", "sum")],
                         ids=lambda c: "+".join(c))
@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_output_subsets(hj, oracle, strategy, wide, cols):
    rk, sk = small_case(oracle, wide)
    rp, sv = GC.payloads(rk, 23), s_values(sk, 23)
    with_strategy(hj, strategy)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk, sv, cols=cols)
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_count_only(hj, oracle, strategy, wide):
    rk, sk = small_case(oracle, wide)
    rp = GC.payloads(rk, 23)
    with_strategy(hj, strategy)
    try:
        build(hj, rk, rp)
        for how in HOWS:
            e = GC.expect(rk, rp, sk, s_values(sk), how, NULL)
            assert hj.count_group(dev(sk), how) == len(e["r"])
        assert hj.count_group(dev(sk), "all") == len(rk)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_capacity_below_m(hj, oracle, strategy, wide):
    """out_cap < M: d_count is exact, the rows written are rows of the result, nothing at or past out_cap."""
    rk, sk = small_case(oracle, wide)
    rp, sv = GC.payloads(rk, 23), s_values(sk, 23)
    with_strategy(hj, strategy)
    try:
        build(hj, rk, rp)
        for how in HOWS:
            e = GC.expect(rk, rp, sk, sv, how, NULL)
            cap = len(e["r"]) // 3
            assert 0 < cap < len(e["r"])
            m, got = run(hj, sk, sv, how, cap)
            assert m == len(e["r"])
            at = np.searchsorted(e["r"], got["r"][:cap])
            assert len(np.unique(got["r"][:cap])) == cap
            for c in COLS:
                assert np.array_equal(got[c][:cap], e[c][at]), (how, c)
                assert (got[c][cap:] == SENTINEL).all(), (how, c)
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_empty_and_tiny(hj, strategy, wide):
    dt = np.int64 if wide else np.int32
    e = np.empty(0, dt)
    k = np.array([5, 9, 5, 3], dt)
    one, other = np.array([4], dt), np.array([6], dt)
    with_strategy(hj, strategy, bits=3)
    try:
        for rk, sk in [(e, k), (k, e), (one, one), (one, other), (k, one), (k, k[:1]), (e, e)]:
            rp = GC.payloads(rk, 8)
            build(hj, rk, rp)
            got = check(hj, rk, rp, sk, s_values(sk, 8))
            assert hj.strategy_used == strategy
            assert len(got["all"]["r"]) == len(rk)
            if len(sk) == 0:
                assert len(got["matched"]["r"]) == 0 and (got["all"]["min"] == NULL).all()
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_tuples_form_equals_columns(hj, oracle, strategy):
    rk, sk = small_case(oracle, True)
    rp, sv = GC.payloads(rk, 23), s_values(sk, 23)
    with_strategy(hj, strategy)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk, sv, tuples=True)
        assert hj.strategy_used == strategy
    finally:
        hj.set_strategy("auto")


def _sorted(cnt, *cols):
    m = int(cnt.item())
    a = [c[:m].cpu().numpy() for c in cols]
    o = np.lexsort(tuple(reversed(a)))
    return [c[o] for c in a]


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_one_build_serves_every_probe(hj, oracle, strategy):
    """inner, lookup, semi, full -> group -> the same four: each result equals
    its first, the group probe equals numpy each time, the repeat flag keeps its answer."""
    rk = oracle.gen_uniform_i64(41, 1, 1, 500, 12000)[0].copy()
    sk = oracle.gen_uniform_i64(41, 2, 1, 700, 9000)[0].copy()
    rk[::97] = I64_MIN
    sk[::131] = I64_MIN
    rp, sv = GC.payloads(rk, 41), s_values(sk, 41)
    d_sk, d_sp = dev(sk), dev(np.arange(9000, dtype=np.int64))
    cap = int(OC.Expect(rk, sk).m("full")) + 8
    o_r = torch.empty(cap, dtype=torch.int64, device="cuda")
    o_s = torch.empty_like(o_r)
    l_r = torch.empty(9000, dtype=torch.int64, device="cuda")
    l_c = torch.empty(9000, dtype=torch.int32, device="cuda")

    def lookup():
        hj.probe_lookup(d_sk, l_r, l_c, null=NULL)
        return [l_r.cpu().numpy(), l_c.cpu().numpy()]

    probes = {
        "inner": lambda: _sorted(hj.probe_relation(d_sk, d_sp, o_r, o_s), o_r, o_s),
        "lookup": lookup,
        "semi": lambda: _sorted(hj.probe_exists(d_sk, d_sp, "semi", o_s), o_s),
        "full": lambda: _sorted(hj.probe_full(d_sk, d_sp, o_r, o_s, kind="full", null_r=NULL, null_s=NULL), o_r, o_s),
    }
    with_strategy(hj, strategy, bits=10)
    try:
        build(hj, rk, rp)
        first = {n: f() for n, f in probes.items()}
        dups = hj.has_duplicates()
        assert dups
        check(hj, rk, rp, sk, sv)
        if strategy == "radix":
            assert_radix(hj)
        for n, f in probes.items():
            again = f()
            assert all(np.array_equal(a, b) for a, b in zip(first[n], again)), n
            assert hj.join_kernel != "k_join_group"
            check(hj, rk, rp, sk, sv)
        assert len(first["inner"][0]) == OC.Expect(rk, sk).pairs
        assert hj.has_duplicates() == dups
        # and a build without repeats keeps saying so after a group probe
        uk = np.arange(12000, dtype=np.int64) * 5
        up = GC.payloads(uk, 42)
        build(hj, uk, up)
        check(hj, uk, up, sk, sv)
        assert not hj.has_duplicates()
        check(hj, uk, up, sk, sv)
    finally:
        hj.set_strategy("auto")


def test_after_routed_build(hj, oracle):
    """After a routed build the group probe is valid over this owner's S rows, unrouted."""
    N, sub, q = 4, 3, 1
    rk, rp, sk, _ = oracle.gen_pkfk_i64(360, 40000, 60000, 0.6)
    rk, sk = rk.copy(), sk.copy()
    rk[3] = rk[30000]
    sk[::700] = rk[3]
    rp = GC.payloads(rk, 36)
    R = RL.Routed(hj, dev(rk), dev(rp), N, sub)
    t, c = R.received(q)
    hj.build_routed(t, c, N, sub)
    g = N.bit_length() - 1
    own_r, own_s = RL.rparts(rk, g) == q, RL.rparts(sk, g) == q
    mine = sk[own_s]
    assert 0 < own_r.sum() < len(rk) and 0 < len(mine) < len(sk)
    e = check(hj, rk[own_r], rp[own_r], mine, s_values(mine, 36))
    assert_radix(hj)
    assert 0 < len(e["matched"]["r"]) < len(e["all"]["r"]) == int(own_r.sum())
    check(hj, rk[own_r], rp[own_r], mine, s_values(mine, 36), tuples=True)


def test_errors_in_order():
    """null context; bad kind; no build of that layout; null count pointer, bad relation, bad outputs."""
    h = HashJoin(0)
    try:
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = torch.zeros(4, dtype=torch.int64, device="cuda")
        k32 = k.to(torch.int32)
        o = torch.zeros(4, dtype=torch.int64, device="cuda")
        o32 = torch.zeros(4, dtype=torch.int32, device="cuda")
        P = lambda t: t.data_ptr()   # noqa: E731
        ARG, STATE, OK = _lib.HJ_ERR_ARG, _lib.HJ_ERR_STATE, _lib.HJ_OK
        g64, g32, gt = lib.hj_dev_group_i64, lib.hj_dev_group_i32, lib.hj_dev_group_tuples_i64
        none5 = (None,) * 5
        # everything else wrong too: the context comes first, then the kind, then the state
        assert g64(None, 7, None, None, -1, 0, *none5, -1, None, None) == ARG
        assert b"null context" in lib.hj_last_error()
        assert g64(h._ctx, 7, None, None, -1, 0, *none5, -1, None, None) == ARG
        assert b"kind" in lib.hj_last_error()
        assert g64(h._ctx, 0, None, None, -1, 0, *none5, -1, None, None) == STATE
        assert gt(h._ctx, 1, None, -1, 0, *none5, -1, None, None) == STATE
        h.build_table(k32)
        assert g64(h._ctx, 0, P(k), P(k), 4, 0, P(o), *none5[1:], 4, P(cnt), None) == STATE   # an i32 build
        assert g32(h._ctx, 2, P(k32), 4, 0, 0, P(o32), *none5[1:], 4, P(cnt), None) == ARG
        assert b"kind" in lib.hj_last_error()
        assert g32(h._ctx, 0, None, 4, 0, 0, *none5, -1, None, None) == ARG
        assert b"count pointer" in lib.hj_last_error()
        assert g32(h._ctx, 0, None, 4, 0, 0, *none5, -1, P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert g32(h._ctx, 0, P(k32), -1, 0, 0, *none5, -1, P(cnt), None) == ARG
        assert b"relation" in lib.hj_last_error()
        assert g32(h._ctx, 0, P(k32), 1 << 31, 0, 0, P(o32), *none5[1:], 4, P(cnt), None) == ARG   # before any row is read
        assert b"row ids" in lib.hj_last_error()
        assert g32(h._ctx, 0, P(k32), 4, -1, 0, P(o32), *none5[1:], 4, P(cnt), None) == ARG
        assert b"row ids" in lib.hj_last_error()
        for cap, first in ((-1, None), (4, None), (0, P(o32))):
            assert g32(h._ctx, 0, P(k32), 4, 0, 0, first, *none5[1:], cap, P(cnt), None) == ARG
            assert b"output" in lib.hj_last_error()
        assert g32(h._ctx, 1, P(k32), 4, 0, 0, *none5, 0, P(cnt), None) == OK   # the count-only form
        torch.cuda.synchronize()
        assert int(cnt.item()) == 4
        h.build_table(k, k)
        # a value column is needed only by the aggregates that read it
        assert g64(h._ctx, 0, P(k), None, 4, 0, None, None, P(o), None, None, 4, P(cnt), None) == ARG
        assert b"value column" in lib.hj_last_error()
        assert g64(h._ctx, 0, P(k), None, 4, 0, P(o), P(o), None, None, None, 4, P(cnt), None) == OK
        torch.cuda.synchronize()
        with pytest.raises(KeyError):
            h.probe_group(k, k, how="left")
        with pytest.raises(ValueError):
            h.probe_group(k, None, out_sum=o)             # no value column
        with pytest.raises(ValueError):
            h.probe_group(k, k, out_r=o, out_cnt=o[:3])   # lengths differ
        with pytest.raises(ValueError):
            h.probe_group(k, k, out_cnt=o32)              # the key's dtype
        with pytest.raises(ValueError):
            h.probe_group(k, k, out_sum=o32)              # int64 sums
    finally:
        h.close()


@pytest.mark.parametrize("strategy", ["global", "radix"])
def test_timing_and_join_kernel_report_the_call(hj, oracle, strategy):
    rk, _, sk, _ = oracle.gen_pkfk_i64(51, 4000, 20000, 0.5)
    rp, sv = GC.payloads(rk, 51), s_values(sk, 51)
    with_strategy(hj, strategy, bits=6)
    hj.set_timing(True)
    try:
        build(hj, rk, rp)
        check(hj, rk, rp, sk, sv, hows=("all",))
        t = hj.last_timing()
        assert t["probe"] > 0
        if strategy == "radix":
            assert t["probe_partition"] > 0 and t["probe_join"] > 0
            assert_radix(hj)
        else:
            assert hj.strategy_used == "global" and hj.join_kernel is None
    finally:
        hj.set_timing(False)
        hj.set_strategy("auto")


def test_group_join_method(hj, oracle):
    rk, _, sk, _ = oracle.gen_pkfk_i64(31, 3000, 9000, 0.3)
    rp, sv = GC.payloads(rk, 31), s_values(sk, 31)
    for how in HOWS:
        e = GC.expect(rk, rp, sk, sv, how, NULL)
        r, a = hj.group_join(dev(rk), dev(rp), dev(sk), dev(sv), how=how, aggs=("count", "sum", "min", "max"), null=NULL)
        assert set(a) == {"count", "sum", "min", "max"} and r.dtype == torch.int64
        o = np.argsort(r.cpu().numpy())
        assert np.array_equal(r.cpu().numpy()[o], e["r"])
        for name, col in (("count", "cnt"), ("sum", "sum"), ("min", "min"), ("max", "max")):
            assert np.array_equal(a[name].cpu().numpy()[o], e[col]), (how, name)
    # the default aggregates, a capacity below M (one re-probe), and the i32 types
    e = GC.expect(rk, rp, sk, sv, "matched", NULL)
    r, a = hj.group_join(dev(rk), dev(rp), dev(sk), dev(sv), capacity=5)
    o = np.argsort(r.cpu().numpy())
    assert sorted(a) == ["count", "sum"] and np.array_equal(a["sum"].cpu().numpy()[o], e["sum"])
    r32, s32 = rk.astype(np.int32), sk.astype(np.int32)
    e32 = GC.expect(r32, GC.payloads(r32), s32, s_values(s32), "all", NULL)
    r, a = hj.group_join(dev(r32), None, dev(s32), None, how="all", aggs=("count", "min", "sum"), null=NULL)
    o = np.argsort(r.cpu().numpy())
    assert r.dtype == torch.int32 and a["count"].dtype == torch.int32 and a["sum"].dtype == torch.int64
    for name, col in (("count", "cnt"), ("min", "min"), ("sum", "sum")):
        assert np.array_equal(a[name].cpu().numpy().astype(np.int64)[o], e32[col]), name
    with pytest.raises(ValueError):
        hj.group_join(dev(rk), dev(rp), dev(sk), dev(sv), aggs=("mean",))


@pytest.mark.parametrize("n,strategy,wide", [(1 << 16, "radix", True), (1 << 12, "global", False)],
                         ids=["i64-2^16-radix", "i32-2^12-global"])
def test_graph_replay(hj, oracle, n, strategy, wide):
    """A captured group probe, replayed after S's keys and values were
    overwritten in place: each replay equals numpy for its inputs (a stale
    reset of the per-call state would carry the last replay's aggregates over)."""
    kt = torch.int64 if wide else torch.int32
    if wide:
        rk = oracle.gen_pkfk_i64(61, n, n, 1.0)[0].copy()
        rk[::97] = rk[1::97]   # some build keys twice
        sets = [oracle.gen_pkfk_i64(61, n, n, f)[2] for f in (1.0, 0.5, 0.1)]
    else:
        rk = oracle.gen_uniform_i32(65, 1, 1, 2 * n, n)
        sets = [oracle.gen_uniform_i32(65 + j, 2, 1, hi, n) for j, hi in enumerate((4 * n, n // 4, 2 * n))]
    rp = GC.payloads(rk, 61)
    sk = torch.empty(n, dtype=kt, device="cuda")
    sv = torch.empty(n, dtype=torch.int64, device="cuda") if wide else None

    def load(keys, vals):
        sk.copy_(torch.from_numpy(np.ascontiguousarray(keys)))
        if wide:
            sv.copy_(torch.from_numpy(vals))
        torch.cuda.synchronize()

    bits = 64 if wide else 32
    outs = {c: torch.empty(n, dtype=torch.int64 if c == "sum" else kt, device="cuda") for c in COLS}
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def setup():
        hj.allocate_hash_table(n, bits)
        hj.reserve_group(n, bits)
        build(hj, rk, rp)
        hj.reserve_probe(n, bits)
        load(sets[0], s_values(sets[0], 0))

    def probe():
        hj.probe_group(sk, sv, "all", outs["r"], outs["cnt"], outs["sum"], outs["min"], outs["max"], null=NULL,
                       count=cnt)

    def reload(entry):
        load(*entry[1:])
        for t in (*outs.values(), cnt):
            t.fill_(SENTINEL)

    def verify(entry):
        j, keys, vals = entry
        e = GC.expect(rk, rp, keys, vals, "all", NULL)
        assert int(cnt.item()) == n
        o = np.argsort(outs["r"].cpu().numpy(), kind="stable")
        for c in COLS:
            assert np.array_equal(host(outs[c])[o], e[c]), (j, c)

    graph_replay(hj, strategy, setup, probe, [(j, keys, s_values(keys, 100 + j))
                                              for j, keys in enumerate(sets[1:] + sets[:1])], reload, verify)
