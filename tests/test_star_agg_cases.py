"""CPU checks of the star aggregate's case builders (star_agg_cases): the
expectation against nested loops on tiny inputs of every kind mix, and the
coverage conditions the GPU tests rely on in the shared cases -- a tile with
more than 512 distinct groups, a tile with exactly one group, a group key equal
to the INT64_MIN word, a tile with no survivor and a wrapped sum -- so that the
GPU tests cannot pass vacuously."""
import numpy as np
import pytest

import star_agg_cases as AG
import star_cases as SC

WIDTHS = [True, False]
IDS = ["i64", "i32"]


def tiny(wide, hows, seed):
    rng = np.random.default_rng(seed + 2 * wide)
    dt = np.int64 if wide else np.int32
    n, dims = 70, []
    for i, how in enumerate(hows):
        nr = (0, 7, 12, 5)[(i + len(hows)) % 4]           # an empty build side among them
        rk = rng.integers(1, 6, nr).astype(dt)              # few values: repeats, hits and misses
        if wide and nr:
            rk[0] = SC.I64_MIN
        rp = (rng.permutation(nr).astype(np.int64) - 3) * 3 + 1 if wide else np.arange(nr, dtype=np.int64)
        sk = rng.integers(1, 9, n).astype(dt)
        if wide:
            sk[rng.integers(0, n, 4)] = SC.I64_MIN
        dims.append(SC.dim(rk, rp, sk, how, SC.NULL - 3 * i))
    return dict(wide=wide, n=n, dims=dims)


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
@pytest.mark.parametrize("hows", [("inner",), ("left",), ("anti",), ("inner", "left", "anti"), ("left", "left"),
                                  ("anti", "inner", "left", "inner")])
def test_expect_equals_the_nested_loop(wide, hows):
    c = tiny(wide, hows, len(hows))
    e = SC.Expect(c)
    val = AG.values(c, 3)
    for grouped in AG.subsets(c):
        gshift, gbase = AG.plan(c, grouped)
        for sh, base in ((gshift, gbase), (gshift, None), ([63 if i in grouped else -1 for i in range(len(hows))], gbase)):
            want, got = AG.brute(c, val, sh, base), AG.expect(c, e, val, sh, base)
            for col in AG.COLS:
                assert np.array_equal(got[col], want[col]), (grouped, sh, col)
            assert int(got["cnt"].sum()) == e.m and (e.m > 0) == (len(got["key"]) > 0)


def test_no_qualifying_row_is_no_group():
    for wide in WIDTHS:
        c = SC.small_case(wide, 0)
        e = SC.Expect(c)
        assert all(len(a) == 0 for a in AG.expect(c, e, AG.values(c), [-1, -1]).values())
        dt = np.int64 if wide else np.int32
        c = dict(wide=wide, n=10, dims=[SC.dim(np.zeros(0, dt), np.zeros(0, np.int64), np.arange(1, 11).astype(dt), "inner")])
        assert len(AG.expect(c, SC.Expect(c), AG.values(c), [0])["key"]) == 0


def test_plan_is_the_codecs():
    """Column 0 is the highest field, a one-value column takes no bits and no shift."""
    c = SC.mixed_case(True)
    gshift, gbase = AG.plan(c, (0, 2))
    d0, d2 = c["dims"][0], c["dims"][2]
    lo2 = min(int(d2["rp"].min()), SC.NULL)
    bits2 = (max(int(d2["rp"].max()), SC.NULL) - lo2).bit_length()
    assert gshift == [bits2, -1, 0] and gbase == [int(d0["rp"].min()), 0, lo2]
    one = dict(wide=True, n=4, dims=[SC.dim(np.array([5], np.int64), np.array([7], np.int64), np.full(4, 5, np.int64), "inner")])
    assert AG.plan(one, (0,)) == ([-1], [7])
    # the fields stay apart: as many groups as distinct payload pairs
    e = SC.expect_of("mixed", True)
    pairs = len(set(zip(e.pays[0].tolist(), e.pays[2].tolist())))
    assert len(AG.expect(c, e, AG.values(c), gshift, gbase)["key"]) == pairs


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_shared_cases_coverage(wide):
    # mixed: tile 0 keeps every row, tile 1 none; grouped by nothing tile 0 is one group
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    per_tile = AG.groups_per_tile(c, e, [-1, -1, -1])
    assert per_tile[0] == 1 and per_tile[1] == 0 and per_tile[2] == 1
    assert np.bincount(e.rows // SC.TILE, minlength=3)[1] == 0
    val = AG.values(c)
    x = AG.expect(c, e, val, [-1, -1, -1])
    assert len(x["key"]) == 1 and x["key"][0] == 0 and x["cnt"][0] == e.m
    if wide:   # a wrapped sum, and both extremes among the values of the kept rows
        exact = int(sum(int(v) for v in val[e.rows]))
        assert not -(1 << 63) <= exact < (1 << 63) and int(x["sum"][0]) == (exact + (1 << 63)) % (1 << 64) - (1 << 63)
        assert x["min"][0] == AG.I64_MIN and x["max"][0] == AG.I64_MAX
    else:
        assert x["min"][0] == -(1 << 31) and x["max"][0] == (1 << 31) - 1
    # every subset of the dimensions with a payload, for mixed and four
    assert len(AG.subsets(c)) == 8 and len(AG.subsets(SC.four_case(wide))) == 8
    # many: more than 512 distinct groups in every tile
    c = AG.many_case(wide)
    e = SC.Expect(c)
    gshift, gbase = AG.plan(c, (0, 1))
    assert c["n"] > 2 * SC.TILE and min(AG.groups_per_tile(c, e, gshift, gbase)) > 512
    assert all(s >= 0 for s in gshift)
    # the INT64_MIN word: exactly the keys 0 and INT64_MIN, both with rows
    c = AG.min_word_case(wide)
    e = SC.Expect(c)
    x = AG.expect(c, e, AG.values(c), [63])
    assert x["key"].tolist() == [AG.I64_MIN, 0] and (x["cnt"] > 100).all()
    # overflow: more distinct groups than the smallest table holds
    c = AG.overflow_case(wide)
    e = SC.Expect(c)
    assert e.m == c["n"] and len(AG.expect(c, e, None, [0])["key"]) == AG.OVERFLOW_GROUPS
    assert AG.OVERFLOW_GROUPS == AG.OVERFLOW_CAPACITY + 1000 and AG.OVERFLOW_CAPACITY == max(2 * AG.OVERFLOW_RESERVE, 2048)
