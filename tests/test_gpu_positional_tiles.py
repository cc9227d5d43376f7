"""The positional probes of the global strategy (k_probe_lookup, k_probe_asof,
k_probe_expand) with more tiles than workgroups: a table of exactly 64 KiB
runs two workgroups per CU, and positional_cases.strided_positional_case's
probe side has 1026 tiles, the last ragged, so every workgroup takes a second
tile at least -- the grid-stride loop, the LDS variants' load-ahead and
hand-over, INT64_MIN probe keys in a workgroup's first, second and third
tile, a cap that cuts a later tile, and the counter add over several tiles.

Every test first asserts that the shape strides on this device (on a part
with more CUs it must fail, not pass unstrided), then that the build is the
64-KiB table of the global strategy.  Expected results come from numpy
(positional_cases, asof_cases, expand_cases), computed once per case and
shared; every position is compared, with no sorting but inside expand's
segments.  repeats=False: no build key twice, the chain walks' early exit."""
import functools

import numpy as np
import pytest
import torch

import asof_cases as AC
import expand_cases as XC
import positional_cases as PC
from hashjoin import HashJoin
from join_gpu import dev, sentinels

pytestmark = pytest.mark.gpu

NULL, SENTINEL, EXTRA = PC.NULL, PC.SENTINEL, PC.EXTRA
NULL_ROWS = list(PC.NULL_ROWS)
SHAPES = [(True, True), (True, False), (False, True), (False, False)]
SHAPE_IDS = ["i64-repeats", "i64-unique", "i32-repeats", "i32-unique"]


@pytest.fixture(scope="module")
def hj():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    h = HashJoin(0)
    h.set_strategy("global")
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def case(wide, repeats):
    """The strided relation with its columns on the device as well (once per module)."""
    c = PC.strided_positional_case(wide, repeats)
    return dict(c, d_rk=dev(c["rk"]), d_rp=dev(c["rp"]) if wide else None, d_sk=dev(c["sk"]), d_sb=dev(c["sb"]))


@functools.lru_cache(maxsize=None)
def lookup_expected(wide, repeats):
    c = PC.strided_positional_case(wide, repeats)
    return PC.lookup_expect(c["rk"], c["rp"], c["sk"], NULL)


@functools.lru_cache(maxsize=None)
def expand_expected(wide, repeats, how):
    c = PC.strided_positional_case(wide, repeats)
    return XC.ExpandExpect(c["rk"], c["rp"], c["sk"], how, NULL)


def assert_strides(c):
    """More tiles than two workgroups per CU: every workgroup of the LDS-table
    probes takes a second tile (on a part with more CUs this must fail, not pass unstrided)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-len(c["sk"]) // PC.TILE) > 2 * cus, (len(c["sk"]), cus)


def built(hj, wide, repeats):
    """The case, striding asserted, built: the 64-KiB table of the global strategy."""
    c = case(wide, repeats)
    assert_strides(c)
    hj.build_table(c["d_rk"], c["d_rp"])
    assert hj.capacity == c["slots"] and hj.capacity * (16 if wide else 8) == 64 * 1024
    assert hj.has_duplicates() == repeats
    return c


def host(t):
    return None if t is None else t.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------ lookup
@pytest.mark.parametrize("wide,repeats", SHAPES, ids=SHAPE_IDS)
def test_lookup_strided(hj, wide, repeats):
    """Both outputs, the payload alone, the count alone: every position, d_count, nothing past n."""
    c = built(hj, wide, repeats)
    er, ec = lookup_expected(wide, repeats)
    n = len(c["sk"])
    dt = torch.int64 if wide else torch.int32
    assert 0 < int((ec > 0).sum()) < n and int(ec.max()) == (2 if repeats else 1)
    if wide:   # the INT64_MIN probe rows answer from the side list
        assert (ec[NULL_ROWS] == 1).all() and (er[NULL_ROWS] == c["rp"][PC.SIDE_ROW]).all()
    for want_r, want_cnt in ((True, True), (True, False), (False, True)):
        o_r = sentinels(n + EXTRA, SENTINEL, dt) if want_r else None
        o_c = sentinels(n + EXTRA, SENTINEL, torch.int32) if want_cnt else None
        m = int(hj.probe_lookup(c["d_sk"], o_r, o_c, null=NULL).item())
        assert hj.strategy_used == "global"
        g_r, g_c = host(o_r), host(o_c)
        if want_r:
            assert np.array_equal(g_r[:n], er), (want_cnt, np.flatnonzero(g_r[:n] != er)[:8])
            assert (g_r[n:] == SENTINEL).all()
        if want_cnt:
            assert np.array_equal(g_c[:n], ec), (want_r, np.flatnonzero(g_c[:n] != ec)[:8])
            assert (g_c[n:] == SENTINEL).all()
        assert m == int((ec > 0).sum()), (want_r, want_cnt, m, int((ec > 0).sum()))
    assert hj.has_duplicates() == repeats


# ------------------------------------------------------------------ as-of
@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("wide,repeats", SHAPES, ids=SHAPE_IDS)
def test_asof_strided(hj, wide, repeats, kind):
    c = built(hj, wide, repeats)
    er, found = AC.expect(c["rk"], c["rp"], c["sk"], c["sb"], kind, NULL)
    n = len(c["sk"])
    if kind in (0, 1):   # the bound really chooses, among all rows and among the side list's
        assert 0 < int(found.sum()) < int((c["cnt"] > 0).sum())
        if wide:
            assert 0 < int(found[NULL_ROWS].sum()) < len(NULL_ROWS)
    o_r = sentinels(n + EXTRA, SENTINEL, torch.int64 if wide else torch.int32)
    direction, strict = AC.KIND_ARGS[kind]
    m = int(hj.probe_asof(c["d_sk"], c["d_sb"], o_r, direction=direction, strict=strict, null=NULL).item())
    assert hj.strategy_used == "global"
    g = host(o_r)
    assert np.array_equal(g[:n], er), np.flatnonzero(g[:n] != er)[:8]
    assert m == int(found.sum()), (m, int(found.sum()))
    assert (g[n:] == SENTINEL).all()


# ------------------------------------------------------------------ expand
def expand(hj, c, e, how, cap):
    """One expand at `cap` (None: the count form) against e: M, every offset,
    the values below min(M, cap) segment by segment, nothing at or past it."""
    n = len(c["sk"])
    dt = torch.int64 if c["wide"] else torch.int32
    off = sentinels(n + 1 + EXTRA, SENTINEL, torch.int64)
    buf = sentinels(cap + EXTRA, SENTINEL, dt) if cap is not None else None
    m = int(hj.probe_expand(c["d_sk"], off, None if buf is None else buf[:cap], how=how, null=NULL).item())
    assert hj.strategy_used == "global"
    assert m == e.m, (m, e.m)
    off = off.cpu().numpy()
    assert np.array_equal(off[:n + 1], e.off), np.flatnonzero(off[:n + 1] != e.off)[:8]
    assert (off[n + 1:] == SENTINEL).all()
    if buf is not None:
        vals, upto = host(buf), min(e.m, cap)
        assert e.same_values(vals, upto)
        assert (vals[upto:] == SENTINEL).all()


@pytest.mark.parametrize("how", XC.KINDS)
@pytest.mark.parametrize("wide,repeats", SHAPES, ids=SHAPE_IDS)
def test_expand_strided(hj, wide, repeats, how):
    """The count form, cap = M, and a cap that cuts the segment of a row in a
    tile its workgroup reaches in a later iteration (repeats: in the middle of
    its two partners; else right behind its one)."""
    c = built(hj, wide, repeats)
    e = expand_expected(wide, repeats, how)
    assert e.unique == (not repeats)
    row = c["cut_row"]
    cap = int(e.off[row]) + 1
    assert row // PC.TILE >= PC.CUT_TILE and e.off[row] < cap <= e.off[row + 1] and cap < e.m
    expand(hj, c, e, how, None)
    expand(hj, c, e, how, e.m)
    expand(hj, c, e, how, cap)
    assert hj.has_duplicates() == repeats
