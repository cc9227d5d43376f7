"""The star query (hj.h "Star query") on the GPU, i64 and i32: the star
aggregate with fact-side predicates, a two-column value expression and
fact-side group fields in one fused pass.  Expected results come from numpy
(star_query_cases.expect), never from the library; outputs are sentinel-filled
and EXTRA rows longer than the capacity passed, rows are matched to the
expectation by their key, and the guard region must hold the sentinel.  The
tile is 2048 rows throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

import star_agg_cases as AG
import star_cases as SC
import star_query_cases as QC
from hashjoin import HJError, StarProbe, _lib, lib, star_query
from star_gpu import (ARG, EXTRA, GROUP_AGGS, IDS, NULL, SENTINEL, TILE, WIDTHS, assert_same_state, build, check_groups,
                      compare, context_state, ctxs, dev, dim_arrays, host, ptr, sentinels, star)

pytestmark = pytest.mark.gpu
STAR_GROUPS = 1 << 13   # the shared star fixture reserves them

COLS = QC.COLS
OPS = {"add": _lib.HJ_VALUE_ADD, "sub": _lib.HJ_VALUE_SUB, "mul": _lib.HJ_VALUE_MUL}
assert TILE == 2048


def qargs(q):
    """The query's device-side keyword arguments of query_into / query."""
    return dict(where=[(dev(col), lo, hi, kind) for col, lo, hi, kind in q["where"]],
                expr=None if q["expr"] is None else (q["expr"][0], dev(q["expr"][1])),
                fact_group=[(dev(col), s, b) for col, s, b in q["fact_group"]], group=q["gshift"], base=q["gbase"])


def run(star, dims, c, q, want=COLS, cap=None, x=None, kw=None):
    """One query_into at `cap` (None: G + 5) writing the columns in `want` against the expectation."""
    x = QC.expect(c, q) if x is None else x
    cap = len(x["key"]) + 5 if cap is None else cap
    bufs = {col: sentinels(cap + EXTRA) for col in want}
    needs_val = any(col in want for col in ("sum", "min", "max"))
    cnt = star.query_into(dims, dev(q["val"]) if needs_val else None, **(qargs(q) if kw is None else kw),
                          **{ARG[col]: b[:cap] for col, b in bufs.items()})
    check_groups(cnt, bufs, x, cap)
    return x


def make_fact(where=(), vop=0, vb=None, fact_group=(), npreds=None, nfact=None):
    """An hj_star_fact over device tensors (None: a null column); npreds / nfact override the counts."""
    f = _lib.StarFact()
    f.npreds = len(where) if npreds is None else npreds
    for p, (col, lo, hi, kind) in enumerate(where):
        f.pcol[p], f.plo[p], f.phi[p], f.pkind[p] = None if col is None else col.data_ptr(), lo, hi, kind
    f.vop, f.vb = vop, None if vb is None else vb.data_ptr()
    f.nfact = len(fact_group) if nfact is None else nfact
    for i, (col, shift, base) in enumerate(fact_group):
        f.fcol[i], f.fshift[i], f.fbase[i] = None if col is None else col.data_ptr(), shift, base
    return f


def raw_call(s, wide, hs, kinds, keys, gshift, fact, val, n, outs, cap, count, nulls=True, nd=None, gbase=None):
    nd = len(hs) if nd is None else nd
    k = len(hs)
    f = lib.hj_dev_star_query_i64 if wide else lib.hj_dev_star_query_i32
    rc = f(s, nd, *dim_arrays(wide, hs, kinds, keys, nulls),
           None if gshift is None or not k else (C.c_int * k)(*gshift),
           None if gbase is None or not k else (C.c_int64 * k)(*gbase),
           None if fact is None else C.byref(fact), ptr(val), n, *[ptr(o) for o in outs], cap, ptr(count), None)
    return rc, lib.hj_last_error().decode()


# ------------------------------------------------------------------ 1. fact == NULL equals aggregate_into
@pytest.mark.parametrize("name", ["mixed", "four"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_null_fact_equals_aggregate_into(ctxs, star, wide, name):
    c = (SC.mixed_case if name == "mixed" else SC.four_case)(wide)
    e = SC.expect_of(name, wide)
    dims = build(ctxs, c)
    val = AG.values(c)
    dval = dev(val)
    grouped = (0, 2) if name == "mixed" else (0, 1)
    gshift, gbase = AG.plan(c, grouped)
    x = AG.expect(c, e, val, gshift, gbase)
    G = len(x["key"])
    a = {col: torch.full((G + EXTRA,), SENTINEL, dtype=torch.int64, device="cuda") for col in COLS}
    cnt = star.aggregate_into(dims, dval, group=gshift, base=gbase, **{ARG[col]: b[:G] for col, b in a.items()})
    assert int(cnt.item()) == G
    plan_a = star.last_plan
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for fact in (None, make_fact()):   # a null descriptor, and one that asks for nothing
        b = {col: torch.full((G + EXTRA,), SENTINEL, dtype=torch.int64, device="cuda") for col in COLS}
        rc, msg = raw_call(star._s, wide, [d[0] for d in dims], [SC.KINDS.index(d[2]) for d in dims],
                           [d[1] for d in dims], gshift, fact, dval, c["n"], [b[col][:G] for col in COLS], G, count,
                           gbase=gbase)
        assert rc == 0, msg
        assert int(count.item()) == G and star.last_plan == plan_a
        oa, ob = torch.argsort(a["key"][:G]), torch.argsort(b["key"][:G])
        for col in COLS:
            assert torch.equal(a[col][:G][oa], b[col][:G][ob]), col
            assert (host(b[col])[G:] == SENTINEL).all()
        compare({col: host(t) for col, t in b.items()}, x, G, True)


# ------------------------------------------------------------------ 2. sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_sizes(ctxs, star, wide, n):
    c, q = QC.sizes_at(wide, n)
    dims = build(ctxs, c)
    run(star, dims, c, q)
    assert star.last_plan["launches"] == (4 if n else 3)
    run(star, dims, c, q, want=())   # the count form
    assert star.last_plan["launches"] == (4 if n else 3)


# ------------------------------------------------------------------ 3. predicate kinds and edges
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_predicate_kinds_and_edges(ctxs, star, wide):
    c, _ = QC.edge_case(wide)
    dims = build(ctxs, c)
    for name, (where, edge) in QC.edge_predicates(wide).items():
        _, q = QC.edge_query(wide, where)
        x = run(star, dims, c, q)
        assert (len(x["key"]) == 0) == (edge == "none"), name
    # full range under IN is the query without the predicate
    _, q0 = QC.edge_query(wide, [])
    _, q1 = QC.edge_query(wide, QC.edge_predicates(wide)["full in"][0])
    x0, x1 = QC.expect(c, q0), QC.expect(c, q1)
    assert all(np.array_equal(x0[col], x1[col]) for col in COLS)
    run(star, dims, c, q0)


# ------------------------------------------------------------------ 4. a tile with no survivor
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_tile_without_a_survivor(ctxs, star, wide):
    c, qs = QC.dead_tile_queries(wide)
    dims = build(ctxs, c)
    x = run(star, dims, c, qs["step"])
    assert len(x["key"]) > 1
    x = run(star, dims, c, qs["doomed"])      # every admitted row fails a dimension: G == 0, nothing stored
    assert len(x["key"]) == 0
    run(star, dims, c, qs["doomed"], want=())
    run(star, dims, c, qs["step"])            # and the object answers as before


# ------------------------------------------------------------------ 5. the value expression
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_value_operations(ctxs, star, wide):
    c, f = QC.vop_case(wide)
    dims = build(ctxs, c)
    gshift, gbase, _ = QC.layout(c, (0,), [])
    vb2 = AG.values(c, 33)
    for expr in (None, ("add", f["vb"]), ("sub", f["vb"]), ("mul", f["vb"]), ("sub", vb2), ("mul", vb2)):
        q = QC.query([(f["pred"], 0, 7, "in")], f["val"], expr, gshift, gbase)
        run(star, dims, c, q)
        run(star, dims, c, q, want=("key", "min", "max"))
        run(star, dims, c, QC.query([], f["val"], expr, [-1]), want=("sum", "min", "max"))   # one group of them all
    # vop set with only the count asked for: vb is not read and may be NULL
    q = QC.query([(f["pred"], 0, 7, "in")], f["val"], None, gshift, gbase)
    kw = dict(qargs(q), expr=("mul", None))
    run(star, dims, c, q, want=("key", "cnt"), kw=kw)
    run(star, dims, c, q, want=(), kw=kw)
    # the operand may alias the value column and a key column
    dval = dev(f["val"])
    x = QC.expect(c, QC.query([], f["val"], ("mul", f["val"]), gshift, gbase))
    out = star.query(dims, dval, aggs=GROUP_AGGS, expr=("mul", dval), group=gshift, base=gbase)
    compare({col: host(out[k]) for col, k in zip(COLS, ("key",) + GROUP_AGGS)}, x, len(x["key"]), True)


# ------------------------------------------------------------------ 6. fact groups
@pytest.mark.parametrize("with_dims", [True, False], ids=["dims", "nodims"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_fact_groups(ctxs, star, wide, with_dims):
    full, f = QC.fact_group_case(wide)
    c = full if with_dims else QC.no_dims(full)
    dims = build(ctxs, c)
    nd = len(c["dims"])
    where = [(f["pred"], 0, 7, "in")]
    # one fact group (a negative base), two fact groups; the dimensions grouped and not
    for grouped in (((0, 1), ()) if with_dims else ((),)):
        for fcols in ([f["seven"]], [f["seven"], f["bit"]]):
            gshift, gbase, fg = QC.layout(c, grouped, fcols)
            assert fg[0][2] == -3 and len(fg) == len(fcols)
            run(star, dims, c, QC.query(where, f["val"], ("mul", f["vb"]), gshift, gbase, fg))
    # fshift 63: without another field the keys are 0 and the INT64_MIN word
    q = QC.query(where, f["val"], ("add", f["vb"]), [-1] * nd, None, [(f["bit"], 63, 10)])
    x = run(star, dims, c, q)
    assert x["key"].tolist() == [QC.I64_MIN, 0]
    run(star, dims, c, q, cap=1)
    q = QC.query(where, f["val"], None, [-1] * nd, None, [(f["bit"], 63, 10), (f["seven"], 0, -3)])
    assert len(run(star, dims, c, q)["key"]) == 14
    # more than 512 groups per tile from the fact column alone: rows go to the global table directly
    q = QC.query(where, f["val"], ("mul", f["vb"]), [-1] * nd, None, [(f["many"], 0, 0)])
    x = run(star, dims, c, q)
    assert len(x["key"]) > 512
    assert star.last_plan["launches"] == 4 and (with_dims or star.last_plan["lds_bytes"] == 0)


# ------------------------------------------------------------------ 7. no dimension
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_no_dimension(star, wide):
    full, f = QC.fact_group_case(wide)
    c = QC.no_dims(full)
    three = [(f["pred"], 1, 8, "in"), (f["seven"], 0, 0, "out"), (f["many"], 100, 2500, "in")]
    q = QC.query(three, f["val"], ("mul", f["vb"]))
    x = run(star, [], c, q)                   # nothing grouped: one row
    assert x["key"].tolist() == [0] and 0 < int(x["cnt"][0]) < c["n"]
    p = star.last_plan
    assert p["lds_bytes"] == 0 and p["lds_dims"] == [False] * 4 and p["launches"] == 4 and p["tiles"] == 3, p
    run(star, [], c, q, want=())
    q = QC.query(three + [(f["pred"], 9, 9, "in")], f["val"], ("mul", f["vb"]))
    assert len(run(star, [], c, q)["key"]) == 0                                 # no qualifying row: M = 0
    gshift, gbase, fg = QC.layout(c, (), [f["seven"], f["bit"]])
    x = run(star, [], c, QC.query(three, f["val"], ("mul", f["vb"]), gshift, gbase, fg))
    assert 6 < len(x["key"]) <= 12 and star.last_plan["lds_bytes"] == 0
    # no predicate either: a GROUP BY of the fact column; a null descriptor: one group of every row
    x = run(star, [], c, QC.query([], f["val"], None, [], None, fg))
    assert len(x["key"]) == 14
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.full((2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    rc, msg = raw_call(star._s, wide, [], [], [], None, None, dev(f["val"]), c["n"], [None, out[0], out[1], None, None],
                       4, cnt)
    assert rc == 0, msg
    v = f["val"].astype(np.int64)
    with np.errstate(over="ignore"):
        assert int(cnt.item()) == 1 and host(out[:, 0]).tolist() == [c["n"], int(v.sum())]
    assert (host(out[:, 1:]) == SENTINEL).all() and star.last_plan["lds_bytes"] == 0
    with pytest.raises(ValueError):
        star.query_into([])                                                     # nothing to take n from


# ------------------------------------------------------------------ 8. more tiles than workgroups
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_strided_tiles(ctxs, star, wide):
    """1026 tiles over two 64-KiB tables: every persistent workgroup strides, and
    the column loaded ahead for the next tile is the predicate's."""
    c, q, e, x = QC.strided_query(wide)
    dims = build(ctxs, c)
    G = len(x["key"])
    star.reserve_groups(G)
    bufs = {col: sentinels(G + EXTRA) for col in COLS}
    cnt = star.query_into(dims, dev(q["val"]), **qargs(q), **{ARG[col]: b[:G] for col, b in bufs.items()})
    p = star.last_plan
    assert p["tiles"] == 1026 and p["grid"] < p["tiles"], p   # on a part with more CUs this must fail, not pass unstrided
    assert p["lds_dims"] == [True, True, False, False] and p["lds_bytes"] == 128 * 1024 and p["launches"] == 4, p
    check_groups(cnt, bufs, x, G)


# ------------------------------------------------------------------ 9. the composed path
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_equals_the_composed_path(ctxs, star, wide):
    """Torch masks, nonzero, every column indexed through it, the torch
    expression and StarProbe.aggregate over the same builds give the same groups."""
    c, f = QC.edge_case(wide)
    dims = build(ctxs, c)
    gshift, gbase = AG.plan(c, (0, 1))
    dt = torch.int64 if wide else torch.int32
    # i32: aggregate takes an int32 value column, so the composed expression has to fit one
    va = AG.values(c, 50) if wide else QC.fact_column(c, -30000, 30000, 50)
    vb = AG.values(c, 51) if wide else QC.fact_column(c, -30000, 30000, 51)
    dva, dvb = dev(va), dev(vb)
    for name in ("in", "out", "four at once", "both extremes", "lo > hi in"):
        where = QC.edge_predicates(wide)[name][0]
        dwhere = [(dev(col), lo, hi, kind) for col, lo, hi, kind in where]
        mask = torch.ones(c["n"], dtype=torch.bool, device="cuda")
        for col, lo, hi, kind in dwhere:
            inside = (col >= lo) & (col <= hi)
            mask &= inside if kind == "in" else ~inside
        idx = mask.nonzero().squeeze(1)
        cut = [(h, sk[idx], how, null) for h, sk, how, null in dims]
        for op in ("add", "sub", "mul"):
            a, b = dva[idx], dvb[idx]
            v = (a + b if op == "add" else a - b if op == "sub" else a * b).to(dt)
            fused = star.query(dims, dva, aggs=GROUP_AGGS, where=dwhere, expr=(op, dvb), group=gshift, base=gbase)
            if idx.numel() == 0:
                assert fused["key"].numel() == 0
                continue
            comp = star.aggregate(cut, v, aggs=GROUP_AGGS, group=gshift, base=gbase)
            o_c, o_f = torch.argsort(comp["key"]), torch.argsort(fused["key"])
            for k in ("key",) + GROUP_AGGS:
                assert torch.equal(comp[k][o_c], fused[k][o_f]), (name, op, k)
            x = QC.expect(c, QC.query(where, va, (op, vb), gshift, gbase))
            assert np.array_equal(host(fused["sum"][o_f]), x["sum"])


# ------------------------------------------------------------------ 10. star_query
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_star_query(wide):
    """Against numpy: the unpacked group columns, a LEFT null group and a fact key column included."""
    c = SC.four_case(wide)
    p, fk = QC.fact_column(c, 0, 9, 60), QC.fact_column(c, -3, 3, 61)
    val, vb = AG.values(c, 62), AG.values(c, 63)
    where = [(p, 2, 7, "in")]
    e = QC.Expect(c, where)
    d_in = [(dev(d["rk"]), dev(d["rp"]) if wide else None, dev(d["sk"]), d["how"], d["null"]) for d in c["dims"]]
    out = star_query(d_in, dev(val), where=[(dev(p), 2, 7)], expr=("sub", dev(vb)), group_by=[True, True, False, False],
                     fact_group_by=[dev(fk)], aggs=GROUP_AGGS)
    assert out["keys"][2] is None and out["keys"][3] is None and len(out["fact_keys"]) == 1
    got = np.stack([host(out["keys"][0]), host(out["keys"][1]), host(out["fact_keys"][0])], 1)
    assert (got[:, 1] == NULL).any()                                 # the LEFT null is a group value
    assert out["fact_keys"][0].dtype == (torch.int64 if wide else torch.int32)
    trip = np.stack([e.pays[0].astype(np.int64), e.pays[1].astype(np.int64), fk.astype(np.int64)[e.rows]], 1)
    u, inv = np.unique(trip, axis=0, return_inverse=True)
    x = AG.GC.expect(inv.reshape(-1), QC.value(c, val, ("sub", vb))[e.rows])
    at = {tuple(r): i for i, r in enumerate(u.tolist())}
    idx = np.array([at[tuple(r)] for r in got.tolist()])
    assert len(got) == len(u) and len(set(idx.tolist())) == len(u)
    for col, k in zip(COLS[1:], GROUP_AGGS):
        assert np.array_equal(host(out[k]), x[col][idx]), k
    # no dimension, grouped by nothing: the scalar aggregate's one row
    out = star_query([], dev(val), where=[(dev(p), 2, 7)], expr=("mul", dev(vb)), aggs=("count", "sum"))
    ok = (p >= 2) & (p <= 7)
    with np.errstate(over="ignore"):
        want = int(QC.value(c, val, ("mul", vb))[ok].sum())
    assert out["keys"] == [] and out["fact_keys"] == []
    assert host(out["count"]).tolist() == [int(ok.sum())] and host(out["sum"]).tolist() == [want]


def test_star_query_range_error():
    """Fields that need more than 64 bits together: HJ_ERR_RANGE, raised; exactly 64 fit."""
    wide_col = np.array([QC.I64_MIN, 0, QC.I64_MAX, 0], np.int64)
    bit = np.array([0, 1, 0, 1], np.int64)
    with pytest.raises(HJError, match=str(_lib.HJ_ERR_RANGE)):
        star_query([], dev(bit), fact_group_by=[dev(wide_col), dev(bit)])
    out = star_query([], dev(bit), fact_group_by=[dev(wide_col)], aggs=("count", "max"))
    o = np.argsort(host(out["fact_keys"][0]))
    assert host(out["fact_keys"][0])[o].tolist() == [QC.I64_MIN, 0, QC.I64_MAX]
    assert host(out["count"])[o].tolist() == [1, 2, 1] and host(out["max"])[o].tolist() == [0, 1, 0]
    # a 0-bit field is left out
    out = star_query([], dev(bit), fact_group_by=[dev(np.full(4, 7, np.int64)), dev(bit)], aggs=("count",))
    assert host(out["fact_keys"][0]).tolist() == [7, 7] and sorted(host(out["fact_keys"][1]).tolist()) == [0, 1]


# ------------------------------------------------------------------ 11. the contexts are only read
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_contexts_untouched(ctxs, star, wide):
    c, _ = QC.edge_case(wide)
    dims = build(ctxs, c)
    before = context_state(dims, c["n"], wide)
    _, q = QC.edge_query(wide, QC.edge_predicates(wide)["four at once"][0])
    run(star, dims, c, q)
    run(star, dims, c, q, want=())
    assert_same_state(before, context_state(dims, c["n"], wide))


# ------------------------------------------------------------------ 12. error order
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_error_order(ctxs, star, wide):
    """One call per rung of hj.h's error order, each with the later rungs broken too."""
    c = SC.small_case(wide, 1000, hows=("inner", "left"), seed=30)
    dims = build(ctxs, c)
    hs, keys = [d[0] for d in dims], [d[1] for d in dims]
    n = c["n"]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    col = torch.full((n + 5,), SENTINEL, dtype=torch.int64, device="cuda")
    fc = dev(QC.fact_column(c, 0, 9, 1))
    no, ARGE, STATE = [None] * 5, _lib.HJ_ERR_ARG, _lib.HJ_ERR_STATE
    IN = _lib.HJ_PRED_IN
    # a descriptor with every field wrong; each rung mends the fields in front of its own
    def fact(npreds=9, pkind=7, vop=9, nfact=9, fshift=64, pcol=None, fcol=None, vb=None):
        return make_fact([(fc, 0, 5, IN), (pcol, 0, 5, pkind)], vop, vb, [(fc, 0, 0), (fcol, fshift, 0)], npreds, nfact)

    good = dict(npreds=2, pkind=IN, vop=_lib.HJ_VALUE_MUL, nfact=2, fshift=3)
    fresh = StarProbe(0)                # no group reserve
    try:
        s = fresh._s
        rc, msg = raw_call(None, wide, hs, [0, 1], keys, [0, 0], fact(), None, -1, no, 7, None)
        assert rc == ARGE and "null star" in msg
        for nd_bad in (-1, 5):
            rc, msg = raw_call(s, wide, hs, [9, 9], [None, None], [99, 99], fact(), None, -1, no, 7, None, nd=nd_bad)
            assert rc == ARGE and "ndims" in msg and "0..4" in msg
        rc, msg = raw_call(s, wide, [None, None], [9, 9], keys, None, fact(), None, -1, no, 7, None)
        assert rc == ARGE and "gshift array" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(), None, -1, no, 7, None, nulls=False)
        assert rc == ARGE and "null-value" in msg
        # per dimension, as the star aggregate, ahead of the descriptor
        rc, msg = raw_call(s, wide, [hs[0], None], [0, 9], keys, [0, 99], fact(), None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "null context" in msg
        rc, msg = raw_call(s, wide, hs, [0, 3], keys, [0, 99], fact(), None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "kind" in msg
        rc, msg = raw_call(s, wide, hs, [0, 2], keys, [0, 64], fact(), None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "gshift" in msg
        rc, msg = raw_call(s, wide, hs, [0, 2], keys, [0, 0], fact(), None, -1, no, 7, None)
        assert rc == ARGE and "dimension 1" in msg and "ANTI" in msg
        # the descriptor, field by field -- with dimensions, and with none (every array null)
        for k, who in ((2, hs), (0, [])):
            call = lambda f: raw_call(s, wide, who, [0, 1][:k], keys[:k], [0, 0][:k], f, None, -1, no, 7, None)  # noqa: E731
            for bad in (-1, 5, 9):
                rc, msg = call(fact(npreds=bad))
                assert rc == ARGE and "npreds" in msg
            for bad in (-1, 2):
                rc, msg = call(fact(npreds=2, pkind=bad))
                assert rc == ARGE and "pkind[1]" in msg
            for bad in (-1, 4):
                rc, msg = call(fact(npreds=2, pkind=IN, vop=bad))
                assert rc == ARGE and "vop" in msg
            for bad in (-1, 3):
                rc, msg = call(fact(npreds=2, pkind=IN, vop=3, nfact=bad))
                assert rc == ARGE and "nfact" in msg
            for bad in (-1, 64):
                rc, msg = call(fact(npreds=2, pkind=IN, vop=3, nfact=2, fshift=bad))
                assert rc == ARGE and "fshift[1]" in msg
            # no group reserve
            assert fresh.group_capacity == 0
            rc, msg = call(fact(**good))
            assert rc == STATE and "hj_star_reserve_groups" in msg
        with pytest.raises(HJError, match=r"failed with -4"):
            fresh.query_into(dims)
        # from here on the module's star, which has its table
        s = star._s
        val = keys[0]
        some = [None, None, col, None, None]
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good), None, -1, no, 7, None)
        assert rc == ARGE and "null count pointer" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good), None, -1, some, 0, cnt)
        assert rc == ARGE and "negative row count" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], [keys[0], None], [0, 0], fact(**good), None, n, some, 0, cnt)
        assert rc == ARGE and "dimension 1 has null keys" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good), None, n, some, 0, cnt)
        assert rc == ARGE and "pcol[1]" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good, pcol=fc), None, n, some, 0, cnt)
        assert rc == ARGE and "fcol[1]" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good, pcol=fc, fcol=fc), None, n, some, 0, cnt)
        assert rc == ARGE and "without a value column" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good, pcol=fc, fcol=fc), val, n, some, 0, cnt)
        assert rc == ARGE and "fact.vb" in msg
        ok = fact(**good, pcol=fc, fcol=fc, vb=fc)
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], ok, val, n, some, 0, cnt)
        assert rc == ARGE and "out_cap == 0 with an output" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], ok, val, n, no, 7, cnt)
        assert rc == ARGE and "out_cap > 0 with every output null" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], ok, val, n, some, -1, cnt)
        assert rc == ARGE and "negative output capacity" in msg
        # vb NULL is accepted with the count alone; n == 0 takes null columns everywhere
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good, pcol=fc, fcol=fc), None, n,
                           [col, col, None, None, None], 0, cnt)
        assert rc == ARGE and "out_cap == 0 with an output" in msg
        rc, msg = raw_call(s, wide, hs, [0, 1], keys, [0, 0], fact(**good, pcol=fc, fcol=fc), None, n, no, 0, cnt)
        assert rc == 0, msg
        for k, who in ((2, hs), (0, [])):
            rc, msg = raw_call(s, wide, who, [0, 1][:k], [None, None][:k], [0, 0][:k], fact(**good), None, 0, some,
                               col.numel(), cnt)
            assert rc == 0 and int(cnt.item()) == 0, msg
        assert (host(col) == SENTINEL).all()
        with pytest.raises(ValueError):
            star.query_into(dims, where=[(fc, 0, 1)] * 5)
        with pytest.raises(ValueError):
            star.query_into(dims, fact_group=[(fc, 0, 0)] * 3)
        with pytest.raises(ValueError):
            star.query_into(dims, expr=("div", fc))
    finally:
        fresh.close()
    # none of it disturbed the object: the plain call still answers
    gshift, gbase, fg = QC.layout(c, (0, 1), [])
    run(star, dims, c, QC.query([(QC.fact_column(c, 0, 9, 1), 0, 5, "in")], AG.values(c), None, gshift, gbase))


# ------------------------------------------------------------------ 13. one linear graph
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_graph_replay_over_new_inputs(ctxs, star, wide):
    """The dimensions' builds and the star query captured once after
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
    dval, dvb, dpred, dfg = (torch.empty(n, dtype=kt, device="cuda") for _ in range(4))
    # the kernel arguments travel in the graph: bounds, and one field layout wide enough for every set
    gshift, gbase = [24, 0], [-(1 << 20), -(1 << 20)]
    where_of = lambda p: [(p, 20, 79, "in")]  # noqa: E731
    fg_of = lambda f: [(f, 48, -3)]  # noqa: E731

    def facts(c, i):
        return (AG.values(c, 90 + i), AG.values(c, 95 + i), QC.fact_column(c, 0, 99, 70 + i),
                QC.fact_column(c, -3 + (i == 1), 3 - (i == 2), 80 + i))

    def load(c, cols):
        for i, d in enumerate(c["dims"]):
            rk[i].copy_(torch.from_numpy(d["rk"]))
            sk[i].copy_(torch.from_numpy(d["sk"]))
            if wide:
                rp[i].copy_(torch.from_numpy(d["rp"]))
        for t, a in zip((dval, dvb, dpred, dfg), cols):
            t.copy_(torch.from_numpy(a))
        torch.cuda.synchronize()

    hs = ctxs[:2]
    for h, r in zip(hs, rows):
        h.allocate_hash_table(r, 64 if wide else 32)
    star.reserve_groups(n)
    dims = [(hs[0], sk[0], "inner", NULL), (hs[1], sk[1], "left", NULL)]
    outs = {col: torch.empty(n, dtype=torch.int64, device="cuda") for col in COLS}
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def step():
        for i, h in enumerate(hs):
            h.build_table(rk[i], rp[i])
        star.query_into(dims, dval, count=cnt, where=where_of(dpred), expr=("mul", dvb), fact_group=fg_of(dfg),
                        group=gshift, base=gbase, **{ARG[col]: b for col, b in outs.items()})

    load(sets[0], facts(sets[0], 0))
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
            val, vb, pred, fcol = facts(c, i)
            x = QC.expect(c, QC.query(where_of(pred), val, ("mul", vb), gshift, gbase, fg_of(fcol)))
            G = len(x["key"])
            load(c, (val, vb, pred, fcol))
            for t in outs.values():
                t.fill_(SENTINEL)
            cnt.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert 1 < G < n
            check_groups(cnt, outs, x, n)
    finally:
        del g
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 14. overflow (the last test of the file)
def test_group_table_overflow():
    """reserve_groups(8) gives 2048 slots; a fact column of 2048 + 1000 distinct
    values cannot fit: bit 63 of the count, nothing stored, the wrapper raises,
    and an in-range call on the same star is exact.  The insert is the star
    aggregate's counted loop: this test needs no time limit of its own."""
    c, f = QC.overflow_case(True)
    s = StarProbe(0)
    try:
        s.reserve_groups(AG.OVERFLOW_RESERVE)
        assert s.group_capacity == AG.OVERFLOW_CAPACITY == _lib.STAR_GROUP_MIN_CAPACITY
        cap = QC.OVERFLOW_GROUPS + 5
        key, num = sentinels(cap), sentinels(cap)
        dfg = dev(f["fg"])
        m = int(s.query_into([], None, key, num, fact_group=[(dfg, 0, 0)]).item())
        torch.cuda.synchronize()
        assert m < 0, m                                              # bit 63
        assert (host(key) == SENTINEL).all() and (host(num) == SENTINEL).all()
        with pytest.raises(HJError, match="group table"):
            s.query([], None, aggs=("count",), fact_group=[(dfg, 0, 0)])
        # in range again on the same star: a predicate leaves 100 groups; then the low three bits' eight
        x = run(s, [], c, QC.query([(f["fg"], 0, 99, "in")], f["val"], ("mul", f["val"]), [], None, [(f["fg"], 0, 0)]))
        assert len(x["key"]) == 100
        x = run(s, [], c, QC.query([], f["val"], None, [], None, [(f["fg"], 61, 0)]))
        assert len(x["key"]) == 8
        s.reserve_groups(QC.OVERFLOW_GROUPS)
        x = run(s, [], c, QC.query([], f["val"], None, [], None, [(f["fg"], 0, 0)]))
        assert len(x["key"]) == QC.OVERFLOW_GROUPS
    finally:
        s.close()
