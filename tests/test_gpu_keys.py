"""Composite keys on the GPU (hj.h "Composite keys"): the plan, pack and unpack
of the key codec, and join_on / aggregate_on / distinct_on on both strategies.

Every expectation comes from the host (keys_cases: the plan with Python
integers, pack and unpack in numpy; joins and aggregates from numpy over dense
tuple ids), never from the library.  Outputs are SENTINEL-filled and EXTRA
elements longer than what may be written: nothing may be written past it."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import keys_cases as KC
from hashjoin import HashJoin, HJError, KeyCodec, _lib, lib

pytestmark = pytest.mark.gpu

SENTINEL, EXTRA = -12345, 64
I64_MIN, I64_MAX, I32_MIN, I32_MAX = KC.I64_MIN, KC.I64_MAX, KC.I32_MIN, KC.I32_MAX
TDT = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}
STRATEGIES = ["global", "radix"]


@pytest.fixture(scope="module")
def hj():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    h = HashJoin(0)
    yield h
    h.close()


@contextlib.contextmanager
def strategy(hj, name, bits=0):
    hj.set_strategy(name, radix_bits=bits if name == "radix" else 0)
    try:
        yield hj
    finally:
        hj.set_strategy("auto")


@contextlib.contextmanager
def codec_for(cols):
    kc = KeyCodec([TDT[c.dtype] for c in cols])
    try:
        yield kc
    finally:
        kc.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def devs(cols):
    return [dev(c) for c in cols]


def wrap_rows():
    """A row count at which the observe, pack and unpack loops all take a second
    step: more tiles than the capped grid has workgroups, and a ragged tail."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * _lib.KEYS_GRID_PER_CU * _lib.KEYS_TILE + _lib.KEYS_TILE + 77


def same_plan(info, pl):
    for k in ("total_bits", "bits", "lo", "hi", "rows_observed", "fits"):
        assert info[k] == pl[k], (k, info[k], pl[k])
    assert info["rows_out_of_range"] == 0


def sealed(kc, relations):
    kc.reset()
    for r in relations:
        kc.observe(devs(r))
    kc.seal()
    return kc.info()


# ------------------------------------------------------------------ the plan
def plan_cases():
    rng = np.random.default_rng(1)
    i64, i32 = np.int64, np.int32
    col = KC.column
    full = np.array([I64_MIN, -1, 0, I64_MAX, 12], i64)
    return {
        "one-column": [[col(rng, i64, -1000, 5000, 3000)]],
        "negative": [[col(rng, i64, -10**12, -10**12 + 9999, 700), col(rng, i32, -500, -3, 700)]],
        "mixed": [[col(rng, i32, -9, 100000, 4097), col(rng, i64, 1 << 40, (1 << 40) + 5, 4097), col(rng, i32, 7, 7, 4097)]],
        "const-full": [[np.full(5, 77, i64), full]],
        "i32-extremes": [[np.array([I32_MIN, 3, I32_MAX], i32), np.array([I32_MAX, I32_MIN, 0], i32)]],
        "two-observes": [[col(rng, i64, -50, -10, 999), col(rng, i32, 0, 9, 999)],
                         [col(rng, i64, 1000, 2000, 1500), col(rng, i32, 100, 200, 1500)]],
        "empty-then-rows": [[np.zeros(0, i32), np.zeros(0, i64)], [col(rng, i32, 5, 6, 64), col(rng, i64, -3, 3, 64)]],
        "only-empty": [[np.zeros(0, i64), np.zeros(0, i32)]],
    }


@pytest.mark.parametrize("name", list(plan_cases()))
def test_plan_matches_the_model(name):
    relations = plan_cases()[name]
    with codec_for(relations[0]) as kc:
        same_plan(sealed(kc, relations), KC.plan(relations))


def test_plan_without_any_observation_and_after_reset():
    big = [KC.column(np.random.default_rng(2), np.int64, -(1 << 50), 1 << 50, 5000),
           KC.column(np.random.default_rng(3), np.int32, I32_MIN, I32_MAX, 5000)]
    small = [np.array([4, 9], np.int64), np.array([-1, -1], np.int32)]
    with codec_for(big) as kc:
        kc.seal()   # a fresh codec is in the reset state
        same_plan(kc.info(), KC.plan([[big[0][:0], big[1][:0]]]))
        same_plan(sealed(kc, [big]), KC.plan([big]))
        same_plan(sealed(kc, [small]), KC.plan([small]))   # reset forgot the wide range
        assert kc.info()["bits"] == [3, 0]


def test_call_order_is_checked_on_the_host():
    cols = [np.array([1, 2, 3], np.int64)]
    with codec_for(cols) as kc:
        d = devs(cols)
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            kc.pack(d)
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            kc.unpack(d[0])
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            kc.info()
        kc.observe(d)
        kc.seal()
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            kc.observe(d)
        kc.reset()
        kc.observe(d)
        # arguments come before the call order: a null column, a null output, n < 0
        ptrs = (C.c_void_p * 1)(None)
        assert lib.hj_dev_keycodec_observe(kc._kc, ptrs, 3, None) == _lib.HJ_ERR_ARG
        assert b"column" in lib.hj_last_error()
        ptrs = (C.c_void_p * 1)(d[0].data_ptr())
        assert lib.hj_dev_keycodec_pack(kc._kc, ptrs, 3, None, None) == _lib.HJ_ERR_ARG
        assert b"null output" in lib.hj_last_error()
        assert lib.hj_dev_keycodec_pack(kc._kc, ptrs, -1, d[0].data_ptr(), None) == _lib.HJ_ERR_ARG
        assert lib.hj_dev_keycodec_observe(kc._kc, None, 0, None) == _lib.HJ_OK   # n == 0 takes null pointers


# ------------------------------------------------------------------ more than 64 bits
def test_65_bits_is_an_error_and_nothing_is_written():
    full = np.array([I64_MIN, 5, I64_MAX, -9], np.int64)
    two = np.array([0, 1, 1, 0], np.int64)
    pl = KC.plan([[full, two]])
    assert pl["total_bits"] == 65
    with codec_for([full, two]) as kc:
        info = sealed(kc, [[full, two]])
        same_plan(info, pl)
        assert not info["fits"]
        assert lib.hj_keycodec_info(kc._kc, None, None, None, None, None, None) == _lib.HJ_ERR_RANGE
        assert b"64 + 1 = 65" in lib.hj_last_error()
        out = torch.full((4 + EXTRA,), SENTINEL, dtype=torch.int64, device="cuda")
        tup = torch.full((8 + EXTRA,), SENTINEL, dtype=torch.int64, device="cuda")
        kc.pack(devs([full, two]), out=out)
        kc.pack_tuples(devs([full, two]), dev(two), out=tup)
        back = [torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2)]
        kc.unpack(dev(full), outs=back)
        torch.cuda.synchronize()
        for t in (out, tup, *back):
            assert (t == SENTINEL).all()
    h = HashJoin(0)
    try:
        for how in HashJoin.JOIN_ON_KINDS:
            with pytest.raises(HJError, match="65 bits"):
                h.join_on(devs([full, two]), None, devs([full, two]), None, how=how)
        with pytest.raises(HJError, match="65 bits"):
            h.aggregate_on(devs([full, two]))
        assert h.strategy_used is None   # nothing was built
        assert lib.hj_ctx_build_has_duplicates(h._ctx) == _lib.HJ_ERR_STATE
    finally:
        h.close()


# ------------------------------------------------------------------ pack and unpack
def pack_sizes():
    t = _lib.KEYS_TILE
    return [1, 63, 64, 65, t - 1, t, t + 1, "wrap"]


@pytest.mark.parametrize("shape", list(KC.SHAPES))
@pytest.mark.parametrize("n", pack_sizes())
def test_pack_and_unpack_match_the_model(shape, n):
    n = wrap_rows() if n == "wrap" else n
    dtypes = KC.SHAPES[shape][0]
    cols = KC.relation(shape, n, n % 1000 + 5)
    pay = np.arange(n, dtype=np.int64) * 3 - 7
    pl = KC.plan([cols])
    want = KC.pack(pl, cols)
    with codec_for(cols) as kc:
        d = devs(cols)
        same_plan(sealed(kc, [cols]), pl)
        out = torch.full((n + EXTRA,), SENTINEL, dtype=torch.int64, device="cuda")
        assert kc.pack(d, out=out) is out
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want), np.flatnonzero(got[:n] != want)[:8]
        assert (got[n:] == SENTINEL).all()
        tup = torch.full((2 * n + EXTRA,), SENTINEL, dtype=torch.int64, device="cuda")
        kc.pack_tuples(d, dev(pay), out=tup)
        got = tup.cpu().numpy()
        assert np.array_equal(got[:2 * n:2], want) and np.array_equal(got[1:2 * n:2], pay)
        assert (got[2 * n:] == SENTINEL).all()
        outs = [torch.full((n + EXTRA,), SENTINEL, dtype=TDT[np.dtype(dt)], device="cuda") for dt in dtypes]
        kc.unpack(out[:n], outs=outs)
        for o, c in zip(outs, cols):
            g = o.cpu().numpy()
            assert np.array_equal(g[:n], c) and (g[n:] == SENTINEL).all()
        # a skipped column stays untouched, the others are written
        outs = [None] + [torch.full((n,), SENTINEL, dtype=TDT[np.dtype(dt)], device="cuda") for dt in dtypes[1:]]
        back = kc.unpack(out[:n], outs=outs)
        assert back[0] is None
        for o, c in zip(back[1:], cols[1:]):
            assert np.array_equal(o.cpu().numpy(), c)
        assert kc.info()["rows_out_of_range"] == 0
        assert kc.pack([t[:0] for t in d]).numel() == 0   # n == 0 writes nothing


def test_totals_of_exactly_64_bits():
    """(constant, full-range int64): bits {0, 64} -- the constant column must not
    be shifted by 64 -- and two full-range int32 columns: {32, 32}.  Every word
    occurs, INT64_MIN included."""
    rng = np.random.default_rng(64)
    n = 3001
    full = KC.column(rng, np.int64, I64_MIN, I64_MAX, n)
    a, b = KC.column(rng, np.int32, I32_MIN, I32_MAX, n), KC.column(rng, np.int32, I32_MIN, I32_MAX, n)
    a[:2], b[:2] = (I32_MIN, I32_MAX), (I32_MAX, I32_MIN)
    a[7], b[7] = 0, I32_MIN   # (0 - INT32_MIN) << 32 = the INT64_MIN word
    for cols, bits in (([np.full(n, -3, np.int64), full], [0, 64]), ([full, np.full(n, 9, np.int32)], [64, 0]),
                       ([a, b], [32, 32])):
        pl = KC.plan([cols])
        assert pl["bits"] == bits and pl["total_bits"] == 64
        want = KC.pack(pl, cols)
        with codec_for(cols) as kc:
            same_plan(sealed(kc, [cols]), pl)
            k = kc.pack(devs(cols))
            assert np.array_equal(k.cpu().numpy(), want)
            for o, c in zip(kc.unpack(k), cols):
                assert np.array_equal(o.cpu().numpy(), c)
    assert want[7] == I64_MIN


@pytest.mark.parametrize("shape", ["i64x2", "i32-i64-i32"])
def test_misaligned_views_give_the_same_keys(shape):
    """Columns, payload and outputs that start 1 or 3 elements into their
    allocation (4 / 8 / 12 / 24 bytes off a 16-byte boundary) take the element path."""
    n = 5001
    dtypes = KC.SHAPES[shape][0]
    cols = KC.relation(shape, n, 21)
    pay = np.arange(n, dtype=np.int64)
    pl = KC.plan([cols])
    want = KC.pack(pl, cols)

    def view(a, off):
        t = torch.empty(len(a) + off, dtype=TDT[a.dtype], device="cuda")[off:]
        t.copy_(torch.from_numpy(a))
        return t

    with codec_for(cols) as kc:
        for offs in ((1,) * len(cols), (3,) * len(cols), (0, 1, 3)[:len(cols)], (3, 0, 1)[:len(cols)]):
            d = [view(c, o) for c, o in zip(cols, offs)]
            assert any(t.data_ptr() % 16 for t in d)
            kc.reset()
            kc.observe(d)
            kc.seal()
            same_plan(kc.info(), pl)
            for ooff in (0, 1):
                out = torch.full((n + EXTRA + ooff,), SENTINEL, dtype=torch.int64, device="cuda")[ooff:]
                kc.pack(d, out=out)
                got = out.cpu().numpy()
                assert np.array_equal(got[:n], want) and (got[n:] == SENTINEL).all(), (offs, ooff)
                tup = torch.full((2 * n + EXTRA + ooff,), SENTINEL, dtype=torch.int64, device="cuda")[ooff:]
                kc.pack_tuples(d, view(pay, offs[0]), out=tup)
                got = tup.cpu().numpy()
                assert np.array_equal(got[:2 * n:2], want) and np.array_equal(got[1:2 * n:2], pay), (offs, ooff)
                assert (got[2 * n:] == SENTINEL).all()
            outs = [torch.full((n + EXTRA + o,), SENTINEL, dtype=TDT[np.dtype(dt)], device="cuda")[o:]
                    for dt, o in zip(dtypes, offs)]
            kc.unpack(view(want, offs[-1]), outs=outs)
            for o, c in zip(outs, cols):
                g = o.cpu().numpy()
                assert np.array_equal(g[:n], c) and (g[n:] == SENTINEL).all(), offs
        # what is no 1-D contiguous device tensor of the codec's dtypes raises
        d = devs(cols)
        with pytest.raises(ValueError):
            kc.observe([torch.stack([d[0], d[0]], dim=1)[:, 0]] + d[1:])   # strided
        with pytest.raises(ValueError):
            kc.observe([d[0][:-1]] + d[1:])                                # lengths differ
        with pytest.raises(ValueError):
            kc.observe([d[0].cpu()] + d[1:])                               # not on the device
        with pytest.raises(TypeError):
            kc.observe([d[0].to(torch.int16)] + d[1:])
        with pytest.raises(ValueError):
            kc.observe(d[:-1])


def test_rows_outside_the_observed_range_are_counted():
    n, k = 6000, 37
    R = KC.relation("i32-i64-i32", 4000, 31)
    S = KC.relation("i32-i64-i32", n, 32)
    S[0] = np.clip(S[0], -1000, 1000).astype(np.int32)   # column 0 of R spans all of int32: keep S inside anyway
    pl = KC.plan([R])
    rng = np.random.default_rng(33)
    at = rng.permutation(n)[:k]
    S[1][at[:20]] = pl["hi"][1] + 1 + np.arange(20)      # above the range
    S[2][at[10:]] = pl["lo"][2] - 1 - np.arange(k - 10)  # below it; rows at[10:20] are outside in two columns
    bad = KC.outside(pl, S)
    assert bad.sum() == k
    want = KC.pack(pl, S)
    with codec_for(R) as kc:
        same_plan(sealed(kc, [R]), pl)
        got = kc.pack(devs(S)).cpu().numpy()
        info = kc.info()
        assert info["rows_out_of_range"] == k
        assert np.array_equal(got[~bad], want[~bad])
        kc.pack(devs(S))   # the count accumulates until the next reset
        assert kc.info()["rows_out_of_range"] == 2 * k
        assert sealed(kc, [R])["rows_out_of_range"] == 0


@pytest.mark.parametrize("shape", list(KC.SHAPES))
def test_unsigned_key_order_is_the_lexicographic_order(shape):
    cols = KC.relation(shape, 20000, 41)
    with codec_for(cols) as kc:
        sealed(kc, [cols])
        ku = kc.pack(devs(cols)).cpu().numpy().view(np.uint64)
    order = KC.lex_order(cols)
    assert np.array_equal(np.sort(ku), ku[order])
    # and tuples are equal exactly where keys are
    rows = np.stack([c.astype(np.int64) for c in cols], axis=1)[order]
    assert np.array_equal((np.diff(ku[order]) == 0), (np.diff(rows, axis=0) == 0).all(axis=1))


# ------------------------------------------------------------------ join_on
def join_case(seed=51, nr=3000, ns=5000):
    """R and S over three key columns (int32, int64, int32) drawn from one pool
    of tuples, with duplicates and misses on both sides, one pair of tuples that
    differs only in the first column and one that differs only in the last."""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.integers(-40, 40, 1500), rng.integers(-(1 << 25), 1 << 25, 1500), rng.integers(0, 6, 1500)],
                    axis=1)
    pool[0] = (I32_MIN, -5, 3)
    pool[1] = (I32_MAX, -5, 3)          # differs from pool[0] in the first column only
    pool[2] = (11, 1 << 25, 0)
    pool[3] = (11, 1 << 25, 5)          # differs from pool[2] in the last column only
    special, pool = pool[:4].copy(), np.unique(pool[4:], axis=0)
    rng.shuffle(pool)
    pool = np.concatenate([pool[:len(pool) // 2], special, pool[len(pool) // 2:]])   # the middle third is in both relations
    p = len(pool)
    rrows = pool[np.concatenate([np.arange(p * 2 // 3), rng.integers(0, p * 2 // 3, nr - p * 2 // 3)])]
    srows = pool[np.concatenate([np.arange(p // 3, p), rng.integers(p // 3, p, ns - (p - p // 3))])]
    split = lambda rows: [rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int32)]  # noqa: E731
    rp = np.arange(nr, dtype=np.int64) * 2 + 1000
    sp = np.arange(ns, dtype=np.int64) * 2 + 1000001
    return split(rrows), rp, split(srows), sp


def numpy_join(rcols, rp, scols, sp, how, null=-1):
    """The join over dense tuple ids (np.unique over both relations' rows): sorted (r, s) pairs, or sorted S payloads."""
    rows = np.concatenate([np.stack([c.astype(np.int64) for c in rcols], axis=1),
                           np.stack([c.astype(np.int64) for c in scols], axis=1)])
    inv = np.unique(rows, axis=0, return_inverse=True)[1].reshape(-1)
    rid, sid = inv[:len(rp)], inv[len(rp):]
    by_id = {}
    for i, t in enumerate(rid.tolist()):
        by_id.setdefault(t, []).append(i)
    pairs, s_hit, r_hit = [], np.zeros(len(sp), bool), np.zeros(len(rp), bool)
    for j, t in enumerate(sid.tolist()):
        for i in by_id.get(t, ()):
            pairs.append((rp[i], sp[j]))
            s_hit[j] = r_hit[i] = True
    if how == "semi":
        return np.sort(sp[s_hit])
    if how == "anti":
        return np.sort(sp[~s_hit])
    if how in ("left", "full"):
        pairs += [(null, v) for v in sp[~s_hit]]
    if how in ("right", "full"):
        pairs += [(v, null) for v in rp[~r_hit]]
    a = np.array(pairs, np.int64).reshape(-1, 2)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


@pytest.fixture(scope="module")
def join_data():
    rcols, rp, scols, sp = join_case()
    want = {how: numpy_join(rcols, rp, scols, sp, how) for how in HashJoin.JOIN_ON_KINDS}
    assert len(want["inner"]) > len(sp) and len(want["anti"]) > 0 and len(want["right"]) > len(want["inner"])
    return rcols, rp, scols, sp, want


@pytest.mark.parametrize("how", HashJoin.JOIN_ON_KINDS)
@pytest.mark.parametrize("name", STRATEGIES)
def test_join_on_matches_numpy(hj, join_data, name, how):
    rcols, rp, scols, sp, want = join_data
    with strategy(hj, name, 4):
        got = hj.join_on(devs(rcols), dev(rp), devs(scols), dev(sp), how=how)
        assert hj.strategy_used == name
        if name == "radix":
            assert sum(hj.radix_plan) == 4   # 2^4 real partitions
    if how in ("semi", "anti"):
        assert np.array_equal(np.sort(got.cpu().numpy()), want[how])
    else:
        a = np.stack([got[0].cpu().numpy(), got[1].cpu().numpy()], axis=1)
        assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], want[how])


def test_join_on_default_payloads_and_bad_arguments(hj, join_data):
    rcols, rp, scols, sp, _ = join_data
    o_r, o_s = hj.join_on(devs(rcols), None, devs(scols), None)   # payloads: the row indices
    want = numpy_join(rcols, np.arange(len(rp)), scols, np.arange(len(sp)), "inner")
    a = np.stack([o_r.cpu().numpy(), o_s.cpu().numpy()], axis=1)
    assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], want)
    with pytest.raises(ValueError):
        hj.join_on(devs(rcols), None, devs(scols), None, how="cross")
    with pytest.raises(TypeError):
        hj.join_on(devs(rcols), None, [t.to(torch.int64) for t in devs(scols)], None)   # dtypes differ between the sides
    with pytest.raises(ValueError):
        hj.join_on(devs(rcols), None, devs(scols)[:2], None)


# ------------------------------------------------------------------ aggregate_on / distinct_on
@pytest.mark.parametrize("name", STRATEGIES)
def test_aggregate_on_and_distinct_on_match_numpy(hj, name):
    rng = np.random.default_rng(61)
    n = 30000
    a = rng.integers(-20, 20, n).astype(np.int32)
    b = (rng.integers(0, 50, n) * (1 << 33) - (1 << 38)).astype(np.int64)
    a[:2], b[:2] = (-(1 << 20), 1 << 20), (5, 5)   # 22 + 39 bits
    val = rng.integers(-(1 << 62), 1 << 62, n)
    rows = np.stack([a.astype(np.int64), b], axis=1)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    o = np.argsort(inv, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(inv[o]) != 0])
    with np.errstate(over="ignore"):
        want = {"count": np.diff(np.r_[starts, n]), "sum": np.add.reduceat(val[o], starts),
                "min": np.minimum.reduceat(val[o], starts), "max": np.maximum.reduceat(val[o], starts)}
    with strategy(hj, name, 4):
        got = hj.aggregate_on([dev(a), dev(b)], dev(val), aggs=("count", "sum", "min", "max"))
        assert hj.strategy_used == name
        keys = got["keys"]
        assert keys[0].dtype == torch.int32 and keys[1].dtype == torch.int64 and len(keys[0]) == len(uniq)
        ka, kb = keys[0].cpu().numpy(), keys[1].cpu().numpy()
        order = KC.lex_order([ka, kb])
        assert np.array_equal(np.stack([ka.astype(np.int64), kb], axis=1)[order], uniq)
        for c, w in want.items():
            assert np.array_equal(got[c].cpu().numpy()[order], w), c
        d = hj.distinct_on([dev(a), dev(b)])
        da, db = d[0].cpu().numpy(), d[1].cpu().numpy()
        assert d[0].dtype == torch.int32 and d[1].dtype == torch.int64
        assert np.array_equal(np.stack([da.astype(np.int64), db], axis=1)[KC.lex_order([da, db])], uniq)


# ------------------------------------------------------------------ graph
def test_linear_graph_replays_over_new_data():
    """reset, observe R, observe S, seal, pack R, pack S captured once; replayed
    after the input buffers were overwritten with data of another range, the plan
    and the keys are the new data's."""
    nr, ns = 5000, 9001
    dt = (np.int32, np.int64)

    def data(seed, lo0, hi0, lo1, hi1):
        rng = np.random.default_rng(seed)
        mk = lambda n: [KC.column(rng, dt[0], lo0, hi0, n), KC.column(rng, dt[1], lo1, hi1, n)]  # noqa: E731
        return mk(nr), mk(ns)

    sets = [data(71, -5, 1000, 0, 1 << 30), data(72, I32_MIN, -(1 << 30), -(1 << 30), -7), data(73, 4, 4, I64_MIN, I64_MAX)]
    kc = KeyCodec([torch.int32, torch.int64])
    g = None
    try:
        tr = [torch.empty(nr, dtype=TDT[np.dtype(d)], device="cuda") for d in dt]
        ts = [torch.empty(ns, dtype=TDT[np.dtype(d)], device="cuda") for d in dt]
        kr = torch.empty(nr + EXTRA, dtype=torch.int64, device="cuda")
        ks = torch.empty(ns + EXTRA, dtype=torch.int64, device="cuda")

        def load(R, S):
            for t, c in zip(tr + ts, R + S):
                t.copy_(torch.from_numpy(c))
            kr.fill_(SENTINEL)
            ks.fill_(SENTINEL)
            torch.cuda.synchronize()

        def call():
            kc.reset()
            kc.observe(tr)
            kc.observe(ts)
            kc.seal()
            kc.pack(tr, out=kr)
            kc.pack(ts, out=ks)

        load(*sets[0])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):   # one eager step on the capture stream first
            call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        torch.cuda.synchronize()
        for R, S in sets[1:] + sets[:1]:
            load(R, S)
            g.replay()
            torch.cuda.synchronize()
            pl = KC.plan([R, S])
            same_plan(kc.info(), pl)
            for got, cols in ((kr, R), (ks, S)):
                a = got.cpu().numpy()
                n = len(cols[0])
                assert np.array_equal(a[:n], KC.pack(pl, cols)) and (a[n:] == SENTINEL).all()
    finally:
        del g
        torch.cuda.synchronize()
        kc.close()
