"""CPU checks of the star probe's case builders (star_cases): the expectation
against a nested loop on tiny inputs, and the coverage conditions the GPU tests
rely on in the shared cases -- 0 < M < n, a tile with no survivor and one with
all 2048, a row that fails only the last dimension, a LEFT null, an INT64_MIN
probe key in a first, a middle and the ragged last tile, and the table sizes
that put the dimensions where the tests assert them."""
import numpy as np
import pytest

import positional_cases as PC
import star_cases as SC

WIDTHS = [True, False]
IDS = ["i64", "i32"]


def slots(nr):
    return max(16, 1 << int(2 * max(nr, 1) - 1).bit_length())


def table_bytes(d, wide):
    return slots(len(d["rk"])) * (16 if wide else 8)


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
@pytest.mark.parametrize("hows", [("inner",), ("left",), ("anti",), ("inner", "left", "anti"),
                                  ("anti", "inner", "left", "inner")])
def test_expect_equals_the_nested_loop(wide, hows):
    rng = np.random.default_rng(len(hows) + 2 * wide)
    dt = np.int64 if wide else np.int32
    n = 60
    dims = []
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
    c = dict(wide=wide, n=n, dims=dims)
    e = SC.Expect(c)
    rows, pays = SC.brute(c)
    assert np.array_equal(e.rows, rows) and e.m == len(rows)
    for got, want, how in zip(e.pays, pays, hows):
        assert (got is None) == (how == "anti") == (want is None)
        if got is not None:
            assert np.array_equal(got, want)


def test_expect_of_no_rows_and_of_an_empty_dimension():
    for wide in WIDTHS:
        c = SC.small_case(wide, 0)
        e = SC.Expect(c)
        assert e.m == 0 and all(len(p) == 0 for p in e.pays)
        dt = np.int64 if wide else np.int32
        empty = (np.zeros(0, dt), np.zeros(0, np.int64))
        sk = np.arange(1, 11).astype(dt)
        assert SC.Expect(dict(wide=wide, n=10, dims=[SC.dim(*empty, sk, "inner")])).m == 0
        assert SC.Expect(dict(wide=wide, n=10, dims=[SC.dim(*empty, sk, "anti")])).m == 10
        e = SC.Expect(dict(wide=wide, n=10, dims=[SC.dim(*empty, sk, "left")]))
        assert e.m == 10 and (e.pays[0] == SC.NULL).all()


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_mixed_case_coverage(wide):
    c, e = SC.mixed_case(wide), SC.expect_of("mixed", wide)
    n = c["n"]
    assert n == 2 * SC.TILE + 77 and [d["how"] for d in c["dims"]] == ["inner", "inner", "left"]
    assert [len(d["rk"]) for d in c["dims"]] == list(SC.MIXED_ROWS)
    assert 0 < e.m < n
    per_tile = np.bincount(e.rows // SC.TILE, minlength=3)
    assert per_tile[0] == SC.TILE and per_tile[1] == 0 and 0 < per_tile[2] < 77
    # rows that pass dimension 0 and fail dimension 1 (the last one that can drop a row), in the tile nothing survives
    only_last = (e.cnt[0] > 0) & (e.cnt[1] == 0)
    assert only_last[SC.TILE:2 * SC.TILE].sum() > 100
    # a LEFT null among the kept rows, and a repeated build key answered with the smaller payload
    left = e.cnt[2][e.rows]
    assert (left == 0).any() and (left == 2).any() and (e.pays[2][left == 0] == SC.NULL).all()
    assert not (e.pays[2][left > 0] == SC.NULL).any() and not (e.pays[0] == SC.NULL).any()
    # placement: the first two tables fit LDS, the third does not, in both layouts
    b = [table_bytes(d, wide) for d in c["dims"]]
    assert b[0] <= 64 * 1024 and b[1] <= 64 * 1024 and b[0] + b[1] <= 128 * 1024 and b[2] > 64 * 1024
    if wide:
        s0 = c["dims"][0]["sk"]
        rows = list(SC.MIXED_NULL_ROWS)
        assert (s0[rows] == SC.I64_MIN).all() and [r // SC.TILE for r in rows] == [0, 1, 2]
        assert rows[2] >= 2 * SC.TILE and list(e.keep[rows]) == [True, False, True] and (e.cnt[0][rows] == 1).all()
        j = SC.MIXED_LEFT_NULL_ROW
        assert c["dims"][2]["sk"][j] == SC.I64_MIN and e.keep[j] and e.cnt[2][j] == 0
        assert not (c["dims"][2]["rk"] == SC.I64_MIN).any()


@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_four_case_coverage(wide):
    c, e = SC.four_case(wide), SC.expect_of("four", wide)
    assert [d["how"] for d in c["dims"]] == ["inner", "left", "anti", "inner"] and 0 < e.m < c["n"]
    ok = [e.cnt[0] > 0, np.ones(c["n"], bool), e.cnt[2] == 0, e.cnt[3] > 0]
    assert (ok[0] & ok[2] & ~ok[3]).sum() > 100      # fails only the last dimension
    assert (ok[0] & ~ok[2] & ok[3]).sum() > 100      # fails only the anti dimension
    assert (e.cnt[1][e.rows] == 0).any() and (e.cnt[1][e.rows] > 0).any() and e.pays[2] is None
    if wide:
        assert not e.keep[[17, SC.TILE + 3]].any() and (e.cnt[2][[17, SC.TILE + 3]] == 1).all()


@pytest.mark.parametrize("hows", SC.STRIDED_HOWS, ids=["inner", "left"])
@pytest.mark.parametrize("wide", WIDTHS, ids=IDS)
def test_strided_case_coverage(wide, hows):
    c, e = SC.strided_case(wide, hows), SC.expect_of("strided", wide, hows)
    u = SC.unpadded(c)
    assert c["n"] == PC.SEVERAL_NS and -(-c["n"] // SC.TILE) == 1026
    assert e.m == c["n"] if hows[0] == "left" else 0 < e.m < c["n"]
    # both tables exactly 64 KiB without the pad rows, the second past it with them
    assert [table_bytes(d, wide) for d in u["dims"]] == [64 * 1024, 64 * 1024]
    assert table_bytes(c["dims"][1], wide) > 64 * 1024 and len(c["dims"][1]["rk"]) == c["nr"] + SC.STRIDED_PAD
    # the pad rows change nothing: no probe row holds their keys
    assert not np.isin(c["dims"][1]["sk"], c["dims"][1]["rk"][c["nr"]:]).any()
    second = e.cnt[1][e.rows]
    assert (second == 2).any() and (second == 0).any() == (hows[1] == "left")
    if wide:
        rows = list(PC.NULL_ROWS)
        assert (c["dims"][0]["sk"][rows] == SC.I64_MIN).all() and e.keep[rows].all() and (e.cnt[0][rows] == 1).all()
        assert sorted(r // SC.TILE for r in rows) == sorted(PC.NULL_TILES)


def test_payloads_never_collide_with_null_or_sentinel():
    for wide in WIDTHS:
        for c in (SC.mixed_case(wide), SC.four_case(wide)):
            for d in c["dims"]:
                assert not np.isin(d["rp"], [SC.NULL, SC.SENTINEL]).any()
