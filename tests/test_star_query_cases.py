"""CPU checks of the star query tests' expectation (star_query_cases.py): the
numpy expectation against a nested loop over Python integers on tiny inputs,
and the coverage conditions of the shared cases the GPU tests run, so that none
of them can silently become vacuous."""
import numpy as np
import pytest

import star_agg_cases as AG
import star_cases as SC
import star_query_cases as QC

TILE = QC.TILE
WIDTHS = [True, False]
IDS = ["i64", "i32"]


def same(a, b):
    return all(np.array_equal(a[col], b[col]) for col in QC.COLS)


# ------------------------------------------------------------------ the expectation against the nested loop
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_expectation_equals_the_nested_loop(wide):
    lo, hi = QC.extremes(wide)
    for seed, hows in enumerate([("inner",), ("inner", "left"), ("anti", "inner"), ()]):
        c = SC.small_case(wide, 90, hows=hows, rows=(12, 20)[:len(hows)], seed=seed, p=(0.7, 0.6)[:len(hows)])
        p = QC.fact_column(c, 0, 9, seed, plant=(lo, hi))
        f1, f2 = QC.fact_column(c, -3, 3, seed + 50), QC.fact_column(c, 0, 1, seed + 60)
        val, vb = AG.values(c, seed + 70), AG.values(c, seed + 80)
        grouped = tuple(i for i, h in enumerate(hows) if h != "anti")
        gshift, gbase, fg = QC.layout(c, grouped, [f1, f2])
        wheres = [[], [(p, 2, 6, "in")], [(p, 2, 6, "out")], [(p, 0, hi, "in"), (f1, 0, 0, "out")],
                  [(p, lo, lo, "in")], [(p, 5, 4, "in")], [(p, 5, 4, "out")], [(p, QC.I64_MIN, QC.I64_MAX, "out")]]
        for where in wheres:
            for expr in (None, ("add", vb), ("sub", vb), ("mul", vb)):
                q = QC.query(where, val, expr, gshift, gbase, fg)
                assert same(QC.expect(c, q), QC.brute(c, q)), (hows, len(where), expr and expr[0])
        # fshift 63 over a two-valued column, alone: the keys 0 and INT64_MIN
        q = QC.query([(p, 0, 9, "in")], val, ("mul", vb), [-1] * len(hows), None, [(f2, 63, 0)])
        x = QC.expect(c, q)
        assert same(x, QC.brute(c, q)) and x["key"].tolist() == [QC.I64_MIN, 0]
        # nothing grouped: one group, or none
        q = QC.query([(p, 0, 9, "in")], val, None, [-1] * len(hows))
        assert QC.expect(c, q)["key"].tolist() == [0] and same(QC.expect(c, q), QC.brute(c, q))
        q = QC.query([(p, 20, 30, "in")], val, None, [-1] * len(hows))
        assert len(QC.expect(c, q)["key"]) == 0 and same(QC.expect(c, q), QC.brute(c, q))


def test_value_wraps():
    c = dict(wide=True, n=4, dims=[])
    a = np.array([QC.I64_MIN, QC.I64_MAX, -1, 3], np.int64)
    b = np.array([QC.I64_MIN, QC.I64_MAX, QC.I64_MIN, -7], np.int64)
    assert QC.value(c, a, ("mul", b)).tolist() == [0, 1, QC.I64_MIN, -21]
    assert QC.value(c, a, ("add", b)).tolist() == [0, -2, QC.I64_MAX, -4]
    assert QC.value(c, a, ("sub", b)).tolist() == [0, 0, QC.I64_MAX, 10]
    a32, b32 = np.array([QC.I32_MIN, QC.I32_MAX], np.int32), np.array([QC.I32_MIN, QC.I32_MIN], np.int32)
    c32 = dict(wide=False, n=2, dims=[])
    assert QC.value(c32, a32, ("mul", b32)).tolist() == [1 << 62, QC.I32_MAX * QC.I32_MIN]   # i32 never wraps


def test_rows_are_mapped_back():
    c = SC.small_case(True, 500, hows=("inner", "left"), seed=2)
    p = QC.fact_column(c, 0, 9, 1)
    e, full = QC.Expect(c, [(p, 3, 7, "in")]), SC.Expect(c)
    ok = (p >= 3) & (p <= 7)
    assert np.array_equal(e.keep, full.keep & ok) and np.array_equal(e.rows, np.flatnonzero(full.keep & ok))
    for d in range(2):
        assert np.array_equal(e.pays[d], full.pays[d][ok[full.rows]])


# ------------------------------------------------------------------ coverage conditions of the shared cases
def coverage(c, where):
    """(admitted, qualifying, n) and the two cross conditions: a row a predicate
    admits fails a dimension; a row a predicate drops would have passed every dimension."""
    e, full = QC.Expect(c, where), SC.Expect(c)
    return int(e.ok.sum()), e.m, bool((e.ok & ~full.keep).any()), bool((~e.ok & full.keep).any())


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_sizes_case_coverage(wide):
    for n in (63, 64, 65, 2047, 2048, 2049):
        c, q = QC.sizes_at(wide, n)
        adm, m, a, b = coverage(c, q["where"])
        assert 0 < m < adm < n and a and b, (n, adm, m)
        assert 0.35 < adm / n < 0.65                       # about one half
        assert len(q["fact_group"]) == 1 and q["expr"][0] == "mul"
    c, q = QC.sizes_at(wide, 1)
    assert c["n"] == 1 and len(q["where"][0][0]) == 1
    c, q = QC.sizes_at(wide, 0)
    assert len(QC.expect(c, q)["key"]) == 0


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_edge_predicates_coverage(wide):
    c, f = QC.edge_case(wide)
    lo, hi = QC.extremes(wide)
    assert c["n"] == 2 * TILE + 77
    assert (f["ext"] == lo).any() and (f["ext"] == hi).any() and f["ext"].dtype == QC.dtype_of(wide)
    names = set()
    for name, (where, edge) in QC.edge_predicates(wide).items():
        adm, m, a, b = coverage(c, where)
        names.add(name)
        if edge is None:
            assert 0 < m <= adm < c["n"], (name, adm, m)
            assert 0 < m < c["n"]
        elif edge == "all":
            assert adm == c["n"] and 0 < m < c["n"] and a, name
        else:
            assert adm == 0 and m == 0, name
    # every predicate of more than a handful of rows meets both cross conditions
    for name in ("in", "out", "lo == hi out", "all but the extremes", "up to the maximum", "down to the minimum",
                 "four at once"):
        adm, m, a, b = coverage(c, QC.edge_predicates(wide)[name][0])
        assert a and b and m < adm, name
    assert {"in", "out", "lo == hi", "lo > hi in", "lo > hi out", "full in", "full out", "both extremes",
            "four at once"} <= names
    assert len(QC.edge_predicates(wide)["four at once"][0]) == 4
    # the extremes: exactly the planted rows
    e = QC.Expect(c, QC.edge_predicates(wide)["both extremes"][0])
    assert int(e.ok.sum()) == 4 and set(f["ext"][e.ok].tolist()) == {lo, hi}


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_dead_tile_coverage(wide):
    c, qs = QC.dead_tile_queries(wide)
    assert c["n"] == 3 * TILE
    e = QC.Expect(c, qs["step"]["where"])
    tile = np.arange(c["n"]) // TILE
    assert not e.ok[tile == 1].any() and e.ok[tile != 1].all()      # the middle tile has no survivor
    assert not e.keep[tile == 1].any() and e.keep[tile == 0].any() and e.keep[tile == 2].any()
    assert SC.Expect(c).keep[tile == 1].any()                       # and would have had some
    e = QC.Expect(c, qs["doomed"]["where"])
    assert 0 < int(e.ok.sum()) < c["n"] and e.m == 0                # admitted rows, all failed by the dimensions
    assert len(QC.expect(c, qs["doomed"])["key"]) == 0


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_vop_case_coverage(wide):
    c, f = QC.vop_case(wide)
    lo, hi = QC.extremes(wide)
    e = SC.Expect(c)
    for r in (0, 1, c["n"] // 2, c["n"] - 1):
        assert e.keep[r] and int(f["val"][r]) in (lo, hi) and int(f["vb"][r]) in (lo, hi)
    assert 0 < e.m < c["n"]
    if wide:   # sums and products wrap
        exact = sum(int(a) * int(b) for a, b in zip(f["val"][e.rows], f["vb"][e.rows]))
        assert not QC.I64_MIN <= exact <= QC.I64_MAX
        assert int(f["val"][0]) * int(f["vb"][0]) > QC.I64_MAX


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_fact_group_case_coverage(wide):
    c, f = QC.fact_group_case(wide)
    assert len(np.unique(f["seven"])) == 7 and int(f["seven"].min()) < 0
    assert sorted(np.unique(f["bit"]).tolist()) == [10, 11]
    # more than 512 distinct groups per tile from the fact column alone, with and without dimensions
    for cc in (c, QC.no_dims(c)):
        nd = len(cc["dims"])
        q = QC.query([(f["pred"], 0, 7, "in")], f["val"], ("mul", f["vb"]), [-1] * nd, None, [(f["many"], 0, 0)])
        e = QC.Expect(cc, q["where"])
        per = QC.groups_per_tile(cc, e, q)
        assert min(per[:2]) > 512, per
    # fshift 63 alone: the INT64_MIN group word
    q = QC.query([], f["val"], None, [], None, [(f["bit"], 63, 10)])
    assert QC.expect(QC.no_dims(c), q)["key"].tolist() == [QC.I64_MIN, 0]


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_strided_query_coverage(wide):
    c, q, e, x = QC.strided_query(wide)
    adm, full = int(e.ok.sum()), SC.expect_of("strided", wide)
    assert -(-c["n"] // TILE) == 1026 and 0 < e.m < adm < c["n"]
    assert (e.ok & ~full.keep).any() and (~e.ok & full.keep).any()
    assert len(q["fact_group"]) == 1 and len(q["where"]) == 1 and len(x["key"]) > 512
    assert int(x["cnt"].sum()) == e.m


def test_overflow_case_coverage():
    c, f = QC.overflow_case(True)
    assert len(np.unique(f["fg"])) == QC.OVERFLOW_GROUPS > AG.OVERFLOW_CAPACITY and c["dims"] == []
