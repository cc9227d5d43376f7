"""The star aggregate (hj.h "Star aggregate") on the GPU, i64 and i32: GROUP BY
over a star probe's qualifying rows in one fused pass.  Expected results come
from numpy (star_agg_cases.expect: star_cases.Expect, the group-key formula in
uint64 arithmetic, a sort-based group-by), never from the library; outputs are
sentinel-filled and EXTRA rows longer than the capacity passed.  Row order is
unspecified, so rows are matched to the expectation by their key; the guard
region past the capacity must hold the sentinel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import star_agg_cases as AG
import star_cases as SC
from hashjoin import HashJoin, HJError, KeyCodec, StarProbe, _lib, lib, star_aggregate
from star_gpu import (ARG, EXTRA, GROUP_AGGS, IDS, NULL, SENTINEL, TILE, WIDTHS, assert_same_state, build, check_groups,
                      compare, context_state, ctxs, dev, dim_arrays, host, ptr, sentinels, star, strided_keys)

pytestmark = pytest.mark.gpu
STAR_GROUPS = 1 << 13   # the shared star fixture reserves them

COLS = AG.COLS


def run(star, dims, c, e, val, gshift, gbase=None, want=COLS, cap=None, dval=None, plan=None):
    """One call at `cap` (None: G + 5) writing the columns in `want` against the expectation."""
    x = AG.expect(c, e, val, gshift, gbase)
    cap = len(x["key"]) + 5 if cap is None else cap
    bufs = {col: sentinels(cap + EXTRA) for col in want}
    needs_val = any(col in want for col in ("sum", "min", "max"))
    if dval is None and needs_val:
        dval = dev(val)
    cnt = star.aggregate_into(dims, dval if needs_val else None, group=gshift, base=gbase,
                              **{ARG[col]: b[:cap] for col, b in bufs.items()})
    if plan is not None:
        plan(star.last_plan)
    check_groups(cnt, bufs, x, cap)
    return x


# ------------------------------------------------------------------ the shared cases, every grouped subset
@pytest.mark.parametrize("name", ["mixed", "four"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_every_grouped_subset(ctxs, star, wide, name):
    """All of count / sum / min / max over values that hold both extremes (int64:
    sums wrap), grouped by every subset of the dimensions with a payload."""
    c = (SC.mixed_case if name == "mixed" else SC.four_case)(wide)
    e = SC.expect_of(name, wide)
    dims = build(ctxs, c)
    val = AG.values(c)
    dval = dev(val)
    for grouped in AG.subsets(c):
        gshift, gbase = AG.plan(c, grouped)
        x = run(star, dims, c, e, val, gshift, gbase, dval=dval)
        assert (len(x["key"]) == 1) == (not grouped)
        p = star.last_plan
        assert p["launches"] == 4 and p["tiles"] == -(-c["n"] // TILE), p
        if name == "mixed":   # the two inner tables in LDS; the 5000-row LEFT one is global when walked, unread when not
            assert p["lds_dims"] == [True, True, False, False], p
    run(star, dims, c, e, val, gshift, gbase, dval=dval)   # bit-equal across runs


# ------------------------------------------------------------------ sizes
@functools.lru_cache(maxsize=None)
def sizes_relations(wide):
    return SC.small_case(wide, 2049, hows=("inner", "left"), seed=20, p=(0.6, 0.5))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_sizes(ctxs, star, wide, n):
    full = sizes_relations(wide)
    c = dict(wide=wide, n=n, dims=[dict(d, sk=d["sk"][:n]) for d in full["dims"]])
    e = SC.Expect(c)
    dims = build(ctxs, c)
    gshift, gbase = AG.plan(c, (0, 1))
    run(star, dims, c, e, AG.values(c), gshift, gbase)
    assert star.last_plan["launches"] == (4 if n else 3)
    run(star, dims, c, e, None, gshift, gbase, want=())   # the count form


# ------------------------------------------------------------------ kinds
@pytest.mark.parametrize("how", SC.KINDS)
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_one_dimension_of_each_kind(ctxs, star, wide, how):
    c = SC.small_case(wide, 2 * TILE + 333, hows=(how,), rows=(700,), seed=SC.KINDS.index(how), null_row=2)
    if wide:
        c["dims"][0]["sk"][[0, TILE + 1, 2 * TILE + 300]] = SC.I64_MIN
    e = SC.Expect(c)
    assert (how == "left" and e.m == c["n"]) or 0 < e.m < c["n"]
    dims = build(ctxs, c)
    gshift, gbase = AG.plan(c, () if how == "anti" else (0,))
    x = run(star, dims, c, e, AG.values(c), gshift, gbase)
    assert len(x["key"]) == (1 if how == "anti" else len(np.unique(e.pays[0])))
    if how == "left":   # outside the key a LEFT dimension is never read: one group of every row
        x = run(star, dims, c, e, AG.values(c), [-1])
        assert x["cnt"].tolist() == [c["n"]] and star.last_plan["lds_dims"] == [False] * 4


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_anti_with_a_grouped_second_dimension(ctxs, star, wide):
    c = SC.small_case(wide, TILE + 900, hows=("anti", "inner"), seed=5, p=(0.4, 0.7))
    e = SC.Expect(c)
    assert 0 < e.m < c["n"] and e.pays[0] is None
    gshift, gbase = AG.plan(c, (1,))
    run(star, build(ctxs, c), c, e, AG.values(c), gshift, gbase)


@pytest.mark.parametrize("how", SC.KINDS)
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_empty_dimension(ctxs, star, wide, how):
    """An empty build side behind an ordinary inner dimension: inner gives no
    group at all, left the null's group, anti what the first dimension kept."""
    c = SC.small_case(wide, TILE + 50, hows=("inner", how), seed=9)
    dt = np.int64 if wide else np.int32
    c["dims"][1].update(rk=np.zeros(0, dt), rp=np.zeros(0, np.int64))
    if wide:
        c["dims"][1]["sk"][3] = SC.I64_MIN
    e = SC.Expect(c)
    dims = build(ctxs, c)
    grouped = (0,) if how == "anti" else (0, 1)
    gshift, gbase = AG.plan(c, grouped)
    x = run(star, dims, c, e, AG.values(c), gshift, gbase)
    assert (len(x["key"]) == 0) == (how == "inner")
    if how == "left":   # the null alone, at a shift of its own: every key carries it
        x = run(star, dims, c, e, AG.values(c), [-1, 3], [0, 0])
        assert x["key"].tolist() == [NULL * 8]


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_no_dimension_walked(ctxs, star, wide):
    """Every kind LEFT and every gshift -1: one hot group of all n rows, no table read."""
    c = SC.small_case(wide, 2 * TILE + 100, hows=("left", "left"), seed=3)
    e = SC.Expect(c)
    val = AG.values(c)
    x = run(star, build(ctxs, c), c, e, val, [-1, -1])
    assert x["key"].tolist() == [0] and x["cnt"].tolist() == [c["n"]]
    assert star.last_plan["lds_bytes"] == 0 and star.last_plan["launches"] == 4


# ------------------------------------------------------------------ many groups, one group, the INT64_MIN word
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_many_groups(ctxs, star, wide):
    """More than 512 distinct groups in every tile: rows the LDS table does not admit go to the global one directly."""
    c = AG.many_case(wide)
    e = SC.Expect(c)
    gshift, gbase = AG.plan(c, (0, 1))
    star.reserve_groups(e.m)
    x = run(star, build(ctxs, c), c, e, AG.values(c), gshift, gbase)
    assert len(x["key"]) > 3 * 512


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_one_hot_group(ctxs, star, wide):
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    x = run(star, build(ctxs, c), c, e, AG.values(c), [-1, -1, -1])
    assert x["key"].tolist() == [0] and x["cnt"].tolist() == [e.m]


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_int64_min_group_word(ctxs, star, wide):
    """gshift 63 over payloads of both parities: exactly the keys 0 and INT64_MIN."""
    c = AG.min_word_case(wide)
    e = SC.Expect(c)
    dims = build(ctxs, c)
    x = run(star, dims, c, e, AG.values(c), [63])
    assert x["key"].tolist() == [AG.I64_MIN, 0]
    run(star, dims, c, e, AG.values(c), [63], cap=1)        # whichever comes first is a true group
    run(star, dims, c, e, None, [63], want=("key", "cnt"))


# ------------------------------------------------------------------ repeated build keys, wide INT64_MIN keys
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_repeated_build_key_in_a_grouped_dimension(ctxs, star, wide):
    """The smallest payload of the key's rows decides the group, in a dropping and in a LEFT dimension."""
    n = TILE + 700
    for hows in (("inner", "left"), ("left", "inner")):
        c = SC.small_case(wide, n, hows=hows, rows=(600, 900), seed=12, p=(0.7, 0.6), repeats=20)
        c["dims"][0]["sk"][::9] = c["dims"][0]["rk"][4]     # a key two build rows hold
        e = SC.Expect(c)
        dims = build(ctxs, c)
        assert ctxs[0].has_duplicates() and not ctxs[1].has_duplicates() and int(e.cnt[0].max()) == 2
        gshift, gbase = AG.plan(c, (0, 1))
        run(star, dims, c, e, AG.values(c), gshift, gbase)
        assert ctxs[0].has_duplicates()


@pytest.mark.parametrize("where", ["build", "probe", "both"])
def test_wide_int64_min_keys(ctxs, star, where):
    """A grouped dimension's payload from the side list."""
    n = TILE + 300
    c = SC.small_case(True, n, hows=("inner", "left"), seed=15, null_row=5 if where != "probe" else None)
    rows = [1, TILE - 1, TILE, n - 1]
    if where != "build":
        c["dims"][0]["sk"][rows] = SC.I64_MIN
        c["dims"][1]["sk"][rows[0]] = SC.I64_MIN            # dimension 1 never holds it: a LEFT null where row 1 is kept
    e = SC.Expect(c)
    if where == "both":
        assert e.keep[rows].all() and (e.pays[0][np.searchsorted(e.rows, rows)] == c["dims"][0]["rp"][5]).all()
    gshift, gbase = AG.plan(c, (0, 1))
    run(star, build(ctxs, c), c, e, AG.values(c), gshift, gbase)
    # two build rows under INT64_MIN: the side list's minimum decides
    if where == "both":
        c["dims"][0]["rk"][9] = SC.I64_MIN
        e = SC.Expect(c)
        lo = min(int(c["dims"][0]["rp"][5]), int(c["dims"][0]["rp"][9]))
        assert (e.pays[0][np.searchsorted(e.rows, rows)] == lo).all()
        run(star, build(ctxs, c), c, e, AG.values(c), gshift, gbase)


# ------------------------------------------------------------------ more tiles than workgroups
@functools.lru_cache(maxsize=None)
def strided_expect(wide, hows):
    c = SC.strided_case(wide, hows)
    val = AG.values(c)
    gshift, gbase = AG.plan(c, (0, 1))
    return val, gshift, gbase, AG.expect(c, SC.expect_of("strided", wide, hows), val, gshift, gbase)


@pytest.mark.parametrize("forced_global", [False, True], ids=["all-lds", "one-global"])
@pytest.mark.parametrize("hows", SC.STRIDED_HOWS, ids=["inner", "left"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_strided_tiles(ctxs, star, wide, hows, forced_global):
    """1026 tiles over two 64-KiB tables beside the collapse table: every
    persistent workgroup strides and loads the next tile's keys ahead.
    forced_global: the second dimension built with its pad rows, so its table is
    read from global memory -- and the groups are the same."""
    padded = SC.strided_case(wide, hows)
    c = padded if forced_global else SC.unpadded(padded)
    e = SC.expect_of("strided", wide, hows)
    val, gshift, gbase, x = strided_expect(wide, hows)
    dims = build(ctxs, c, strided_keys(wide))
    G = len(x["key"])
    star.reserve_groups(G)
    bufs = {col: sentinels(G + EXTRA) for col in COLS}
    cnt = star.aggregate_into(dims, dev(val), group=gshift, base=gbase, **{ARG[col]: b[:G] for col, b in bufs.items()})
    p = star.last_plan
    assert p["tiles"] == 1026 and p["grid"] < p["tiles"], p   # on a part with more CUs this must fail, not pass unstrided
    assert p["lds_dims"] == [True, not forced_global, False, False], p
    assert p["lds_bytes"] == (64 if forced_global else 128) * 1024 and p["launches"] == 4, p
    assert G > 512
    check_groups(cnt, bufs, x, G)
    assert int(x["cnt"].sum()) == e.m


# ------------------------------------------------------------------ capacity, the count form, optional outputs
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_capacity_below_the_groups(ctxs, star, wide):
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    dims = build(ctxs, c)
    val = AG.values(c)
    gshift, gbase = AG.plan(c, (0, 2))
    G = len(AG.expect(c, e, val, gshift, gbase)["key"])
    assert G > 600
    for cap in (1, 255, 600, G - 1, G):
        run(star, dims, c, e, val, gshift, gbase, cap=cap)


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_count_form_and_optional_outputs(ctxs, star, wide):
    c, e = SC.four_case(wide), SC.expect_of("four", wide)
    dims = build(ctxs, c)
    val = AG.values(c)
    gshift, gbase = AG.plan(c, (0, 1))
    run(star, dims, c, e, val, gshift, gbase, want=())                     # the count form, sval NULL
    run(star, dims, c, e, val, gshift, gbase, want=("key", "cnt"))         # sval NULL with the count only
    run(star, dims, c, e, val, gshift, gbase, want=("cnt",))
    for leave in COLS:                                                     # each output NULL in turn
        run(star, dims, c, e, val, gshift, gbase, want=tuple(col for col in COLS if col != leave))
    for only in ("sum", "min", "max"):
        run(star, dims, c, e, val, gshift, gbase, want=("key", only))
    # a null gbase is all zeros
    x = AG.expect(c, e, val, gshift, None)
    out = star.aggregate(dims, dev(val), aggs=GROUP_AGGS, group=gshift)
    compare({col: host(out[k]) for col, k in zip(COLS, ("key",) + GROUP_AGGS)}, x, len(x["key"]), True)


# ------------------------------------------------------------------ the contexts are only read
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_contexts_untouched(ctxs, star, wide):
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    dims = build(ctxs, c)
    before = context_state(dims, c["n"], wide)
    used = [h.strategy_used for h, *_ in dims]
    gshift, gbase = AG.plan(c, (0, 1, 2))
    run(star, dims, c, e, AG.values(c), gshift, gbase)
    run(star, dims, c, e, None, gshift, gbase, want=())
    assert [h.strategy_used for h, *_ in dims] == used
    assert_same_state(before, context_state(dims, c["n"], wide))
    for i in range(3):   # and the lookups say what the expectation's dimension columns say
        assert np.array_equal(before[i][3], e.cnt[i])


# ------------------------------------------------------------------ the composed path, star_aggregate
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_equals_the_composed_path(ctxs, star, wide):
    """StarProbe.probe, a gather of the value, KeyCodec.pack and
    HashJoin.aggregate over the same builds give the same groups."""
    c, e = SC.four_case(wide), SC.expect_of("four", wide)
    dims = build(ctxs, c)
    val = AG.values(c)
    dval = dev(val)
    dt = torch.int64 if wide else torch.int32
    rows, pays = star.probe(dims)
    cols = [pays[0], pays[1]]
    kc, agg = KeyCodec([dt, dt]), HashJoin(0)
    try:
        kc.observe(cols)
        kc.seal()
        info = kc.info()
        assert info["fits"] and all(b > 0 for b in info["bits"])
        a = agg.aggregate(kc.pack(cols), dval[rows.long()].to(torch.int64), aggs=GROUP_AGGS)
        gshift, gbase = [info["bits"][1], 0, -1, -1], [info["lo"][0], info["lo"][1], 0, 0]
        f = star.aggregate(dims, dval, aggs=GROUP_AGGS, group=gshift, base=gbase)
        o_a, o_f = torch.argsort(a["key"]), torch.argsort(f["key"])
        for k in ("key",) + GROUP_AGGS:
            assert torch.equal(a[k][o_a].to(torch.int64), f[k][o_f]), k
        x = AG.expect(c, e, val, gshift, gbase)
        assert np.array_equal(host(f["key"][o_f]), x["key"]) and np.array_equal(host(f["sum"][o_f]), x["sum"])
        # the codec turns the keys back into the payload columns
        back = kc.unpack(f["key"].contiguous())
        pairs = set(zip(e.pays[0].tolist(), e.pays[1].tolist()))
        assert set(zip(host(back[0]).tolist(), host(back[1]).tolist())) == pairs
    finally:
        kc.close()
        agg.close()


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_star_aggregate(wide):
    """Against numpy, the unpacked group columns and a LEFT null group included."""
    c, e = SC.four_case(wide), SC.expect_of("four", wide)
    val = AG.values(c)
    d_in = [(dev(d["rk"]), dev(d["rp"]) if wide else None, dev(d["sk"]), d["how"], d["null"]) for d in c["dims"]]
    out = star_aggregate(d_in, dev(val), group_by=[True, True, False, False], aggs=GROUP_AGGS)
    assert out["keys"][2] is None and out["keys"][3] is None
    k0, k1 = host(out["keys"][0]), host(out["keys"][1])
    assert (k1 == NULL).any()                                       # the LEFT null is a group value
    # numpy: group the kept rows by the payload pair
    pair = e.pays[0] * (1 << 32) + (e.pays[1] - NULL)                # (both well inside 31 bits)
    x = AG.GC.expect(pair, val.astype(np.int64)[e.rows])
    got = k0 * (1 << 32) + (k1 - NULL)
    o = np.argsort(got)
    assert np.array_equal(got[o], x["key"])
    for col, k in zip(COLS[1:], GROUP_AGGS):
        assert np.array_equal(host(out[k])[o], x[col]), k
    # grouped by nothing: one group; count alone needs no value column
    out = star_aggregate(d_in, None, aggs=("count",))
    assert out["keys"] == [None] * 4 and host(out["count"]).tolist() == [e.m]
    with pytest.raises(ValueError):
        star_aggregate(d_in, dev(val), group_by=[False, False, True, False])   # the anti dimension


def test_star_aggregate_range_error():
    """Grouped payload ranges that need more than 64 bits together: HJ_ERR_RANGE, raised."""
    rk = np.array([1, 2, 3], np.int64)
    rp = np.array([AG.I64_MIN, 0, AG.I64_MAX], np.int64)
    sk = np.array([1, 2, 3, 1], np.int64)
    d = (dev(rk), dev(rp), dev(sk), "inner")
    with pytest.raises(HJError, match=str(_lib.HJ_ERR_RANGE)):
        star_aggregate([d, d], dev(sk), group_by=[True, True])
    out = star_aggregate([d, d], dev(sk), group_by=[True, False], aggs=("count", "min"))   # 64 bits exactly fit
    o = np.argsort(host(out["keys"][0]))
    assert host(out["keys"][0])[o].tolist() == [AG.I64_MIN, 0, AG.I64_MAX] and host(out["count"])[o].tolist() == [2, 1, 1]


# ------------------------------------------------------------------ error paths
def raw_call(s, wide, hs, kinds, keys, gshift, val, n, outs, cap, count, nulls=True):
    nd = len(hs)
    f = lib.hj_dev_star_aggregate_i64 if wide else lib.hj_dev_star_aggregate_i32
    rc = f(s, nd, *dim_arrays(wide, hs, kinds, keys, nulls), None if gshift is None else (C.c_int * nd)(*gshift), None,
           ptr(val), n, *[ptr(o) for o in outs], cap, ptr(count), None)
    return rc, lib.hj_last_error().decode()


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_error_order(ctxs, star, wide):
    """One call per rung of hj.h's error order, each with the later rungs broken too."""
    c = SC.small_case(wide, 1000, hows=("inner", "left"), seed=30)
    e = SC.Expect(c)
    dims = build(ctxs, c)
    hs, keys = [d[0] for d in dims], [d[1] for d in dims]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    col = sentinels(e.m + 5)
    no, ARGE, STATE = [None] * 5, _lib.HJ_ERR_ARG, _lib.HJ_ERR_STATE
    fresh = StarProbe(0)                # no group reserve
    other = HashJoin(0)
    try:
        s = fresh._s
        rc, msg = raw_call(None, wide, hs, [0, 1], keys, [0, 0], None, -1, no, 7, None)
        assert rc == ARGE and "null star" in msg
        for nd_bad in ([], hs + hs + hs[:1]):
            k = len(nd_bad)
            rc, msg = raw_call(s, wide, nd_bad, [9] * k, [None] * k, [99] * k, None, -1, no, 7, None)
            assert rc == ARGE and "ndims" in msg
        rc, msg = raw_call(s, wide, [None, None], [9, 9], keys, None, None, -1, no, 7, None)
        assert rc == ARGE and "gshift array" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, -1, no, 7, None, nulls=False)
        assert rc == ARGE and "null-value" in msg
        # per dimension, in index order
        rc, msg = raw_call(s, wide, [hs[0], None], [0, 9], keys, [0, 99], None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "null context" in msg
        rc, msg = raw_call(s, wide, hs, [0, 3], keys, [0, 99], None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "kind" in msg
        for bad in (64, -2):
            rc, msg = raw_call(s, wide, hs, [0, 2], keys, [0, bad], None, -1, no, 7, None)
            assert rc == ARGE and "dimension 1" in msg and "gshift" in msg
        rc, msg = raw_call(s, wide, hs, [0, 2], keys, [0, 0], None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "ANTI" in msg
        # no build of that layout, a radix-only build: HJ_ERR_STATE naming the dimension, behind its argument errors
        o = SC.small_case(not wide, 10, hows=("inner",), seed=31)["dims"][0]
        other.set_strategy("global")
        other.build_table(dev(o["rk"]), dev(o["rp"]) if not wide else None)
        rc, msg = raw_call(s, wide, [hs[0], other], [0, 1], keys, [0, 0], None, -1, no, 7, None)
        assert rc == STATE and "dimension 1" in msg and "layout" in msg
        rc, msg = raw_call(s, wide, [hs[0], other], [0, 1], keys, [0, 64], None, -1, no, 7, None)
        assert rc == ARGE and "gshift" in msg
        other.set_strategy("radix")
        d1 = c["dims"][1]
        other.build_table(dev(d1["rk"]), dev(d1["rp"]) if wide else None)
        rc, msg = raw_call(s, wide, [hs[0], other], [0, 1], keys, [0, 0], None, -1, no, 7, None)
        assert rc == STATE and "dimension 1" in msg and "HJ_STRATEGY_GLOBAL" in msg
        # no group reserve
        assert fresh.group_capacity == 0
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, -1, no, 7, None)
        assert rc == STATE and "hj_star_reserve_groups" in msg
        with pytest.raises(HJError, match=r"failed with -4"):
            fresh.aggregate_into(dims)
        # from here on the module's star, which has its table
        s = star._s
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, -1, no, 7, None)
        assert rc == ARGE and "null count pointer" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, -1, [None, None, col, None, None], 0, cnt)
        assert rc == ARGE and "negative row count" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], [keys[0], None], [0, 0], None, c["n"], [None, None, col, None, None], 0, cnt)
        assert rc == ARGE and "dimension 1 has null keys" in msg
        for k in (2, 3, 4):   # the sval rule, ahead of the output rules
            outs = [col if i == k else None for i in range(5)]
            rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, c["n"], outs, 0, cnt)
            assert rc == ARGE and "without a value column" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, c["n"], no, 7, cnt)
        assert rc == ARGE and "out_cap > 0 with every output null" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, c["n"], [col, None, None, None, None], 0, cnt)
        assert rc == ARGE and "out_cap == 0 with an output" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], None, c["n"], [col, None, None, None, None], -1, cnt)
        assert rc == ARGE and "negative output capacity" in msg
        # n == 0 takes null columns
        rc, msg = raw_call(s, wide, hs, [0, 1], [None, None], [0, 0], None, 0, no, 0, cnt)
        assert rc == 0 and int(cnt.item()) == 0
        with pytest.raises(ValueError):
            star.aggregate_into(dims + dims + dims)                 # six dimensions
    finally:
        fresh.close()
        other.close()
    # none of it disturbed the object: the plain call still answers
    gshift, gbase = AG.plan(c, (0, 1))
    run(star, dims, c, e, AG.values(c), gshift, gbase)


def test_group_capacity():
    s = StarProbe(0)
    try:
        assert s.group_capacity == 0
        for want, cap in ((0, 2048), (8, 2048), (1024, 2048), (1025, 4096), (100, 4096), (5000, 16384)):   # grow-only
            s.reserve_groups(want)
            assert s.group_capacity == cap, (want, cap)
        assert _lib.STAR_GROUP_MIN_CAPACITY == 2048
    finally:
        s.close()


# ------------------------------------------------------------------ one linear graph
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_graph_replay_over_new_inputs(ctxs, star, wide):
    """The dimensions' builds and the star aggregate captured once after
    reserve_groups, replayed over new contents of the same buffers."""
    n, rows = 2 * TILE + 500, (300, 5000)
    sets = [SC.small_case(wide, n, hows=("inner", "left"), rows=rows, seed=60 + i, p=(0.3 + 0.2 * i, 0.6),
                          repeats=(0, 30, 0)[i], null_row=(None, 8, 2)[i]) for i in range(3)]
    if wide:
        sets[1]["dims"][0]["sk"][[3, n - 1]] = SC.I64_MIN
    kt = torch.int64 if wide else torch.int32
    rk = [torch.empty(r, dtype=kt, device="cuda") for r in rows]
    rp = [torch.empty(r, dtype=torch.int64, device="cuda") if wide else None for r in rows]
    sk = [torch.empty(n, dtype=kt, device="cuda") for _ in rows]
    dval = torch.empty(n, dtype=kt, device="cuda")
    # the kernel arguments travel in the graph: one field layout wide enough for every set
    gshift, gbase = [24, 0], [-(1 << 20), -(1 << 20)]

    def load(c, val):
        for i, d in enumerate(c["dims"]):
            rk[i].copy_(torch.from_numpy(d["rk"]))
            sk[i].copy_(torch.from_numpy(d["sk"]))
            if wide:
                rp[i].copy_(torch.from_numpy(d["rp"]))
        dval.copy_(torch.from_numpy(val))
        torch.cuda.synchronize()

    hs = ctxs[:2]
    for h, r in zip(hs, rows):
        h.allocate_hash_table(r, 64 if wide else 32)
    star.reserve_groups(n)
    dims = [(hs[0], sk[0], "inner", NULL), (hs[1], sk[1], "left", NULL)]
    cap = n
    outs = {col: torch.empty(cap, dtype=torch.int64, device="cuda") for col in COLS}
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def step():
        for i, h in enumerate(hs):
            h.build_table(rk[i], rp[i])
        star.aggregate_into(dims, dval, count=cnt, group=gshift, base=gbase, **{ARG[col]: b for col, b in outs.items()})

    load(sets[0], AG.values(sets[0], 90))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # one eager step on the capture stream first
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    torch.cuda.synchronize()
    try:
        for i, c in enumerate(sets):
            e = SC.Expect(c)
            val = AG.values(c, 90 + i)
            x = AG.expect(c, e, val, gshift, gbase)
            G = len(x["key"])
            load(c, val)
            for t in outs.values():
                t.fill_(SENTINEL)
            cnt.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert 1 < G < n
            check_groups(cnt, outs, x, cap)
    finally:
        del g
        torch.cuda.synchronize()


# ------------------------------------------------------------------ overflow (the last test of the file)
def test_group_table_overflow(ctxs):
    """reserve_groups(8) gives 2048 slots; 2048 + 1000 distinct groups in one
    call cannot fit: the call returns with bit 63 of the count set and nothing
    stored, the wrapper raises, and an in-range call on the same star is exact.
    The insert is a counted loop: this test needs no time limit of its own."""
    c = AG.overflow_case(True)
    e = SC.Expect(c)
    s = StarProbe(0)
    try:
        s.reserve_groups(AG.OVERFLOW_RESERVE)
        assert s.group_capacity == AG.OVERFLOW_CAPACITY == _lib.STAR_GROUP_MIN_CAPACITY
        dims = build(ctxs, c)
        cap = AG.OVERFLOW_GROUPS + 5
        key, num = sentinels(cap), sentinels(cap)
        m = int(s.aggregate_into(dims, None, key, num, group=[0]).item())
        torch.cuda.synchronize()
        assert m < 0, m                                              # bit 63
        assert (host(key) == SENTINEL).all() and (host(num) == SENTINEL).all()
        with pytest.raises(HJError, match="group table"):
            s.aggregate(dims, None, aggs=("count",), group=[0])
        # in range again on the same star: grouped by nothing, then by the payload's low bits (8 values)
        x = run(s, dims, c, e, AG.values(c), [-1])
        assert x["cnt"].tolist() == [c["n"]]
        x = run(s, dims, c, e, AG.values(c), [61])
        assert len(x["key"]) == 8
        # and with room for them all the same rows are exact
        s.reserve_groups(AG.OVERFLOW_GROUPS)
        x = run(s, dims, c, e, AG.values(c), [0])
        assert len(x["key"]) == AG.OVERFLOW_GROUPS
    finally:
        s.close()
