"""The star probe (hj.h "Star probe") on the GPU, i64 and i32: n probe rows
over up to four built dimensions in one kernel, the rows every dimension admits
kept in input order.  Expected results come from numpy (star_cases.Expect:
positional_cases.lookup_expect per dimension under the kind rules), never from
the library; outputs are sentinel-filled and EXTRA rows longer than the
capacity passed, and every position is compared with no sorting: the defined
values below min(M, cap), the sentinel from there on."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import positional_cases as PC
import star_cases as SC
from hashjoin import HashJoin, HJError, _lib, lib, star_join
from star_gpu import (EXTRA, IDS, NULL, SENTINEL, TILE, WIDTHS, assert_same_state, build, context_state, ctxs, dev,
                      dim_arrays, host, ptr, sentinels, star, strided_keys)

pytestmark = pytest.mark.gpu


def check(star, dims, c, e, cap=None, want_row=True, want=None, row_base=0, plan=None):
    """One probe at `cap` (None: M + 5) with the outputs asked for (want: per
    dimension; None: every dimension that has a column) against e.  plan: called
    with last_plan after the call, before anything is compared."""
    dt = torch.int64 if c["wide"] else torch.int32
    cap = e.m + 5 if cap is None else cap
    want = [p is not None for p in e.pays] if want is None else want
    bufs = [sentinels(cap + EXTRA, dt) if w else None for w in want]
    rbuf = sentinels(cap + EXTRA, dt) if want_row else None
    m = int(star.probe_into(dims, [None if b is None else b[:cap] for b in bufs],
                            None if rbuf is None else rbuf[:cap], row_base=row_base).item())
    if plan is not None:
        plan(star.last_plan)
    assert m == e.m, (m, e.m)
    upto = min(m, cap)
    for i, b in enumerate(bufs):
        if b is None:
            continue
        g = host(b)
        assert np.array_equal(g[:upto], e.pays[i][:upto]), (i, np.flatnonzero(g[:upto] != e.pays[i][:upto])[:8])
        assert (g[upto:] == SENTINEL).all(), i
    if rbuf is not None:
        g = host(rbuf)
        assert np.array_equal(g[:upto], e.rows[:upto] + row_base), np.flatnonzero(g[:upto] != e.rows[:upto] + row_base)[:8]
        assert (g[upto:] == SENTINEL).all()
    return m


def table_bytes(h, wide):
    return h.capacity * (16 if wide else 8)


# ------------------------------------------------------------------ mixed placement
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_mixed_placement(ctxs, star, wide):
    """(inner, inner, left) of 300, 1000 and 5000 build rows over 2 * 2048 + 77
    rows: the first two tables in LDS, the third in global memory, three launches."""
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    dims = build(ctxs, c)
    check(star, dims, c, e)
    p = star.last_plan
    assert p["lds_dims"] == [True, True, False, False], p
    assert p["launches"] == 3 and p["tiles"] == 3 and 1 <= p["grid"] <= 3, p
    assert p["lds_bytes"] == table_bytes(ctxs[0], wide) + table_bytes(ctxs[1], wide), p
    assert table_bytes(ctxs[2], wide) > _lib.STAR_LDS_TABLE_BYTES
    assert ctxs[2].has_duplicates() and not ctxs[0].has_duplicates()
    # bit-equal across runs: the same call into fresh buffers
    check(star, dims, c, e)


# ------------------------------------------------------------------ kinds and dimension counts
@pytest.mark.parametrize("how", SC.KINDS)
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_one_dimension_of_each_kind(ctxs, star, wide, how):
    c = SC.small_case(wide, 2 * TILE + 333, hows=(how,), rows=(700,), seed=SC.KINDS.index(how), null_row=2)
    if wide:
        c["dims"][0]["sk"][[0, TILE + 1, 2 * TILE + 300]] = SC.I64_MIN
    e = SC.Expect(c)
    assert (how == "left" and e.m == c["n"]) or 0 < e.m < c["n"]
    check(star, build(ctxs, c), c, e)
    assert star.last_plan["launches"] == (1 if how == "left" else 3)


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_four_dimensions(ctxs, star, wide):
    c, e = SC.four_case(wide), SC.expect_of("four", wide)
    check(star, build(ctxs, c), c, e)
    assert star.last_plan["lds_dims"] == [True, False, True, True]   # the decision walks no LEFT dimension


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_anti_with_inner(ctxs, star, wide):
    c = SC.small_case(wide, TILE + 900, hows=("anti", "inner"), seed=5, p=(0.4, 0.7))
    e = SC.Expect(c)
    assert 0 < e.m < c["n"] and e.pays[0] is None
    check(star, build(ctxs, c), c, e)


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_same_context_twice(ctxs, star, wide):
    """One build probed by two key columns: inner on the first, left on the second."""
    n = TILE + 123
    rk, rp = SC.relation(77, 500, wide, null_row=1)
    rng = np.random.default_rng(78)
    sa, sb = SC.column(79, rk, n, rng.random(n) < 0.5), SC.column(80, rk, n, rng.random(n) < 0.5)
    c = dict(wide=wide, n=n, dims=[SC.dim(rk, rp, sa, "inner"), SC.dim(rk, rp, sb, "left", NULL - 3)])
    e = SC.Expect(c)
    ctxs[0].build_table(dev(rk), dev(rp) if wide else None)
    dims = [(ctxs[0], dev(sa), "inner", NULL), (ctxs[0], dev(sb), "left", NULL - 3)]
    assert 0 < e.m < n and (e.pays[1] == NULL - 3).any()
    check(star, dims, c, e)


@pytest.mark.parametrize("how", SC.KINDS)
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_empty_dimension(ctxs, star, wide, how):
    """An empty build side behind an ordinary inner dimension: inner gives M =
    0, left all nulls, anti admits every row the first dimension kept."""
    c = SC.small_case(wide, TILE + 50, hows=("inner", how), seed=9)
    dt = np.int64 if wide else np.int32
    c["dims"][1].update(rk=np.zeros(0, dt), rp=np.zeros(0, np.int64))
    if wide:
        c["dims"][1]["sk"][3] = SC.I64_MIN
    e = SC.Expect(c)
    first = int((e.cnt[0] > 0).sum())
    assert e.m == (0 if how == "inner" else first) and first > 0
    if how == "left":
        assert (e.pays[1] == NULL).all()
    check(star, build(ctxs, c), c, e)


# ------------------------------------------------------------------ every kind LEFT
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_all_left_is_one_positional_launch(ctxs, star, wide):
    c = SC.small_case(wide, 2 * TILE + 100, hows=("left", "left"), seed=3, null_row=0)
    if wide:
        c["dims"][0]["sk"][[7, 2 * TILE + 99]] = SC.I64_MIN
    e = SC.Expect(c)
    n = c["n"]
    assert e.m == n and np.array_equal(e.rows, np.arange(n)) and (e.pays[0] == NULL).any()
    dims = build(ctxs, c)
    for cap in (None, n, n - 100, TILE, 1):     # roomy, exact, cut inside the last tile, at a tile edge, one row
        check(star, dims, c, e, cap=cap)
        assert star.last_plan["launches"] == 1, cap
    check(star, dims, c, e, want=[False, True], want_row=False)
    assert star.count(dims) == n and star.last_plan["launches"] == 1


# ------------------------------------------------------------------ repeated build keys, INT64_MIN
@pytest.mark.parametrize("repeats", [20, 0], ids=["repeats", "unique"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_repeated_build_keys(ctxs, star, wide, repeats):
    """With repeats the smallest payload of the key's rows comes back; with
    unique keys the walk ends at the first equal key (the repeat flag is clear)."""
    n = TILE + 700
    c = SC.small_case(wide, n, hows=("inner", "left"), rows=(600, 900), seed=12, p=(0.7, 0.6), repeats=repeats)
    if repeats:
        c["dims"][0]["sk"][::9] = c["dims"][0]["rk"][4]     # a key two build rows hold
    e = SC.Expect(c)
    dims = build(ctxs, c)
    assert ctxs[0].has_duplicates() == bool(repeats) and not ctxs[1].has_duplicates()
    assert int(e.cnt[0].max()) == (2 if repeats else 1)
    check(star, dims, c, e)
    assert ctxs[0].has_duplicates() == bool(repeats)


@pytest.mark.parametrize("where", ["build", "probe", "both"])
def test_wide_int64_min(ctxs, star, where):
    n = TILE + 300
    c = SC.small_case(True, n, hows=("inner", "left"), seed=15, null_row=5 if where != "probe" else None)
    rows = [1, TILE - 1, TILE, n - 1]
    if where != "build":
        c["dims"][0]["sk"][rows] = SC.I64_MIN
        c["dims"][1]["sk"][rows[0]] = SC.I64_MIN            # dimension 1 never holds it: a LEFT null where row 1 is kept
    e = SC.Expect(c)
    if where == "both":
        assert e.keep[rows].all() and (e.pays[0][np.searchsorted(e.rows, rows)] == c["dims"][0]["rp"][5]).all()
        assert e.pays[1][np.searchsorted(e.rows, rows[0])] == NULL
    if where == "probe":
        assert not e.keep[rows].any()
    check(star, build(ctxs, c), c, e)


# ------------------------------------------------------------------ sizes
@functools.lru_cache(maxsize=None)
def sizes_relations(wide):
    return SC.small_case(wide, 2049 + 1, hows=("inner", "left"), seed=20, p=(0.6, 0.5))


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_sizes(ctxs, star, wide, n, aligned):
    """n around the wave and the tile; key columns that start at element 1 of
    their tensor are not 16-byte aligned."""
    full = sizes_relations(wide)
    off = 0 if aligned else 1
    c = dict(wide=wide, n=n, dims=[dict(d, sk=d["sk"][off:off + n]) for d in full["dims"]])
    e = SC.Expect(c)
    keys = [dev(d["sk"])[off:off + n] for d in full["dims"]]
    assert all((k.data_ptr() % 16 == 0) == aligned for k in keys if n)
    dims = build(ctxs, c, keys)
    check(star, dims, c, e)
    assert star.count(dims) == e.m
    if n == 0:
        assert star.last_plan["launches"] == 1


# ------------------------------------------------------------------ capacity and optional outputs
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_capacity_and_optional_outputs(ctxs, star, wide):
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    dims = build(ctxs, c)
    assert e.m > TILE + 10
    for cap in (1000, TILE, TILE + 7, e.m, e.m - 1):   # inside tile 0, at its edge, inside the last tile, exact, one short
        check(star, dims, c, e, cap=cap)
    assert star.count(dims) == e.m and star.last_plan["launches"] == 3   # decision, scan, the counter
    check(star, dims, c, e, want=[False] * 3)                             # out_row only: the write launch walks no table
    check(star, dims, c, e, want=[False, True, False], want_row=False)    # one payload column only
    check(star, dims, c, e, want_row=False)                               # payloads without out_row
    check(star, dims, c, e, want=[True, False, True], cap=TILE + 7)
    if not wide:
        check(star, dims, c, e, row_base=1000)


# ------------------------------------------------------------------ more tiles than workgroups
@pytest.mark.parametrize("forced_global", [False, True], ids=["all-lds", "one-global"])
@pytest.mark.parametrize("hows", SC.STRIDED_HOWS, ids=["inner", "left"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_strided_tiles(ctxs, star, wide, hows, forced_global):
    """1026 tiles over two 64-KiB tables (one workgroup per CU): every
    workgroup of the probe launch -- the decision of two inner dimensions, the
    keep-all launch of two left ones -- strides, loads the next tile's keys
    ahead, and meets INT64_MIN in a first, a later and the ragged last tile.
    forced_global: the second dimension built with its pad rows, so its table
    is read from global memory."""
    padded = SC.strided_case(wide, hows)
    c = padded if forced_global else SC.unpadded(padded)
    e = SC.expect_of("strided", wide, hows)
    dims = build(ctxs, c, strided_keys(wide))
    star.reserve(c["n"])

    def strides(p):
        assert p["tiles"] == 1026 and p["grid"] < p["tiles"], p   # on a part with more CUs this must fail, not pass unstrided
        assert p["lds_dims"] == [True, not forced_global, False, False], p
        assert p["lds_bytes"] == (64 if forced_global else 128) * 1024, p
        assert p["launches"] == (3 if hows[0] == "inner" else 1), p

    check(star, dims, c, e, plan=strides)
    check(star, dims, c, e, cap=int(e.keep[:600 * TILE].sum()) + 3)   # cut in a tile no workgroup takes first


# ------------------------------------------------------------------ the contexts are only read
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_contexts_untouched(ctxs, star, wide):
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    dims = build(ctxs, c)
    before = context_state(dims, c["n"], wide)
    used = [h.strategy_used for h, *_ in dims]
    check(star, dims, c, e)
    star.count(dims)
    assert [h.strategy_used for h, *_ in dims] == used
    after = context_state(dims, c["n"], wide)
    assert_same_state(before, after)
    for i in range(3):   # and the lookups say what the expectation's dimension columns say
        assert np.array_equal(before[i][3], e.cnt[i])


# ------------------------------------------------------------------ error paths
def raw_call(star, wide, hs, kinds, keys, n, outs, out_row, cap, count):
    nd = len(hs)
    f = lib.hj_dev_star_i64 if wide else lib.hj_dev_star_i32
    args = [star._s, nd, *dim_arrays(wide, hs, kinds, keys), n]
    if not wide:
        args.append(0)
    args += [(C.c_void_p * nd)(*[None if o is None else o.data_ptr() for o in outs]),
             ptr(out_row), cap, ptr(count), None]
    return f(*args), lib.hj_last_error().decode()


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_error_paths(ctxs, star, wide):
    c = SC.small_case(wide, 1000, hows=("inner", "left"), seed=30)
    e = SC.Expect(c)
    dims = build(ctxs, c)
    dt = torch.int64 if wide else torch.int32
    col = torch.full((e.m + 5,), SENTINEL, dtype=dt, device="cuda")
    # a radix-only build has no global table: HJ_ERR_STATE naming the dimension
    other = HashJoin(0)
    try:
        other.set_strategy("radix")
        d1 = c["dims"][1]
        other.build_table(dev(d1["rk"]), dev(d1["rp"]) if wide else None)
        with pytest.raises(HJError, match=r"failed with -4: .*dimension 1.*HJ_STRATEGY_GLOBAL"):
            star.probe_into([dims[0], (other, dims[1][1], "left", NULL)], [None, None], col)
        # a build of the other layout
        o = SC.small_case(not wide, 10, hows=("inner",), seed=31)["dims"][0]
        other.set_strategy("global")
        other.build_table(dev(o["rk"]), dev(o["rp"]) if not wide else None)
        with pytest.raises(HJError, match=r"failed with -4: .*dimension 0"):
            star.probe_into([(other, dims[0][1], "inner", NULL)], [None], col)
    finally:
        other.close()
    # ANTI has no payload column
    with pytest.raises(HJError, match=r"failed with -1: .*dimension 1.*ANTI"):
        star.probe_into([dims[0], (dims[1][0], dims[1][1], "anti", NULL)], [None, col], None)
    # both bad-cap forms, and a null count pointer
    hs, keys, cnt = [d[0] for d in dims], [d[1] for d in dims], torch.zeros(1, dtype=torch.int64, device="cuda")
    rc, msg = raw_call(star, wide, hs, [0, 1], keys, c["n"], [None, None], None, 7, cnt)
    assert rc == _lib.HJ_ERR_ARG and "out_cap > 0 with every output null" in msg
    rc, msg = raw_call(star, wide, hs, [0, 1], keys, c["n"], [None, col], None, 0, cnt)
    assert rc == _lib.HJ_ERR_ARG and "out_cap == 0 with an output" in msg
    rc, msg = raw_call(star, wide, hs, [0, 3], keys, c["n"], [None, None], None, 0, cnt)
    assert rc == _lib.HJ_ERR_ARG and "dimension 1" in msg and "kind" in msg
    rc, msg = raw_call(star, wide, hs, [0, 1], keys, -1, [None, None], None, 0, cnt)
    assert rc == _lib.HJ_ERR_ARG and "negative row count" in msg
    with pytest.raises(ValueError):
        star.probe_into(dims + dims + dims)                 # six dimensions
    if not wide:
        with pytest.raises(HJError, match=r"failed with -1: .*row ids past"):
            star.probe_into(dims, [None, None], col, row_base=(1 << 31) - 10)
    # none of it disturbed the object: the plain call still answers
    check(star, dims, c, e)


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_auto_dual_build_is_accepted(star, wide):
    """AUTO's build of 2^18 rows keeps a global table beside its radix partitions: a valid dimension."""
    nr, n = 1 << 18, 3 * TILE + 11
    rk, rp = SC.relation(50 + wide, nr, wide, null_row=9)
    rng = np.random.default_rng(51)
    sk = SC.column(52, rk, n, rng.random(n) < 0.5)
    if wide:
        sk[[4, n - 2]] = SC.I64_MIN
    c = dict(wide=wide, n=n, dims=[SC.dim(rk, rp, sk, "inner")])
    e = SC.Expect(c)
    h = HashJoin(0)
    try:
        h.set_strategy("auto")
        h.build_table(dev(rk), dev(rp) if wide else None)
        assert h.strategy_used == "global" and h.radix_passes >= 1     # the dual build
        check(star, [(h, dev(sk), "inner", NULL)], c, e)
        assert star.last_plan["lds_dims"] == [False] * 4 and star.last_plan["grid"] == star.last_plan["tiles"] == 4
        assert h.strategy_used == "global"
    finally:
        h.close()


# ------------------------------------------------------------------ one linear graph
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_graph_replay_over_new_inputs(ctxs, star, wide):
    """The dimensions' builds and the star probe captured once after reserve,
    replayed over new contents of the same buffers."""
    n, rows = 2 * TILE + 500, (300, 5000)
    sets = [SC.small_case(wide, n, hows=("inner", "left"), rows=rows, seed=60 + i, p=(0.3 + 0.2 * i, 0.6),
                          repeats=(0, 30, 0)[i], null_row=(None, 8, 2)[i]) for i in range(3)]
    if wide:
        sets[1]["dims"][0]["sk"][[3, n - 1]] = SC.I64_MIN
    kt = torch.int64 if wide else torch.int32
    rk = [torch.empty(r, dtype=kt, device="cuda") for r in rows]
    rp = [torch.empty(r, dtype=torch.int64, device="cuda") if wide else None for r in rows]
    sk = [torch.empty(n, dtype=kt, device="cuda") for _ in rows]

    def load(c):
        for i, d in enumerate(c["dims"]):
            rk[i].copy_(torch.from_numpy(d["rk"]))
            sk[i].copy_(torch.from_numpy(d["sk"]))
            if wide:
                rp[i].copy_(torch.from_numpy(d["rp"]))
        torch.cuda.synchronize()

    hs = ctxs[:2]
    for h, r in zip(hs, rows):
        h.allocate_hash_table(r, 64 if wide else 32)
    star.reserve(n)
    dims = [(hs[0], sk[0], "inner", NULL), (hs[1], sk[1], "left", NULL)]
    cap = n
    out_pay = [torch.empty(cap, dtype=kt, device="cuda") for _ in rows]
    out_row = torch.empty(cap, dtype=kt, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def step():
        for i, h in enumerate(hs):
            h.build_table(rk[i], rp[i])
        star.probe_into(dims, out_pay, out_row, count=cnt)

    load(sets[0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # one eager step on the capture stream first
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    torch.cuda.synchronize()
    try:
        for c in sets:
            e = SC.Expect(c)
            load(c)
            for t in out_pay + [out_row]:
                t.fill_(SENTINEL)
            cnt.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert int(cnt.item()) == e.m and 0 < e.m < n
            assert np.array_equal(host(out_row)[:e.m], e.rows) and (host(out_row)[e.m:] == SENTINEL).all()
            for i in range(2):
                assert np.array_equal(host(out_pay[i])[:e.m], e.pays[i]), i
                assert (host(out_pay[i])[e.m:] == SENTINEL).all(), i
    finally:
        del g
        torch.cuda.synchronize()


# ------------------------------------------------------------------ star_join
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_star_join(ctxs, wide):
    """Against numpy, and against the library's own chain: one probe_lookup per
    dimension, a mask, nonzero and gathers."""
    c, e = SC.four_case(wide), SC.expect_of("four", wide)
    d_in = [(dev(d["rk"]), dev(d["rp"]) if wide else None, dev(d["sk"]), d["how"], d["null"]) for d in c["dims"]]
    rows, pays = star_join(d_in)
    assert np.array_equal(host(rows), e.rows)
    for got, want in zip(pays, e.pays):
        assert (got is None) == (want is None)
        if got is not None:
            assert np.array_equal(host(got), want)
    dt = torch.int64 if wide else torch.int32
    keep, cols = torch.ones(c["n"], dtype=torch.bool, device="cuda"), []
    for h, (rk, rp, sk, how, null) in zip(ctxs, d_in):
        h.build_table(rk, rp)
        o_r = torch.empty(c["n"], dtype=dt, device="cuda")
        o_c = torch.empty(c["n"], dtype=torch.int32, device="cuda")
        h.probe_lookup(sk, o_r, o_c, null=null)
        if how != "left":
            keep &= (o_c > 0) if how == "inner" else (o_c == 0)
        cols.append(None if how == "anti" else o_r)
    idx = keep.nonzero().flatten()
    assert torch.equal(idx.to(dt), rows)
    for got, col in zip(pays, cols):
        if col is not None:
            assert torch.equal(col[idx], got)
