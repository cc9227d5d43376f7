"""Hash aggregate (GROUP BY key over one relation, DISTINCT; hj_dev_aggregate_*)
on both strategies and both row widths.

Expected results come from numpy on the host (aggregate_cases.expect: the
relation sorted by key, np.unique and np.add / np.minimum / np.maximum.reduceat
per distinct key), never from the library.  Every case compares all five
columns, sorted by key, bit for bit.  int64 values span the whole range, so
sums wrap, and include INT64_MIN / INT64_MAX; i32 values are the row ids.
Outputs are SENTINEL-filled and EXTRA rows longer than the capacity passed:
nothing may be written at or past it."""
import numpy as np
import pytest
import torch

import aggregate_cases as AC
from hashjoin import HashJoin, HJError, _lib, lib
from join_gpu import dev, hj, sentinels, strategy  # noqa: F401

pytestmark = pytest.mark.gpu

I64_MIN, I32_MIN = AC.I64_MIN, AC.I32_MIN
SENTINEL, EXTRA = -12345, 64
COLS = AC.COLS
DTYPES = [np.int64, np.int32]
DT_IDS = ["i64", "i32"]
STRATEGIES = ["global", "radix"]
AGGS = ("count", "sum", "min", "max")


def planted(dtype):
    return (I64_MIN, 0, -1) if dtype == np.int64 else (-1, I32_MIN, 0)


def run(hj, key, val, cap, cols=COLS, tuples=False, row_base=0, tensors=None):
    """One aggregate with out_cap = cap: (M, {col: the whole SENTINEL-filled
    buffer of cap + EXTRA elements as int64}).  tensors: (key, val) device
    tensors to pass instead of fresh copies."""
    wide = key.dtype == np.int64
    dt = torch.int64 if wide else torch.int32
    bufs = {c: sentinels(cap + EXTRA, SENTINEL, torch.int64 if c == "sum" else dt)
            for c in cols}
    o = {c: (bufs[c][:cap] if c in bufs else None) for c in COLS}
    kw = dict(out_key=o["key"], out_cnt=o["cnt"], out_sum=o["sum"], out_min=o["min"], out_max=o["max"])
    if tuples:
        m = hj.aggregate_tuples_into(dev(np.stack([key, val], axis=1)), **kw)
    elif wide:
        needs_val = any(c in cols for c in ("sum", "min", "max"))
        tk, tv = tensors if tensors else (dev(key), dev(val))
        m = hj.aggregate_into(tk, tv if needs_val else None, **kw)
    else:
        m = hj.aggregate_into(tensors[0] if tensors else dev(key), None, row_base=row_base, **kw)
    return int(m.item()), {c: b.cpu().numpy().astype(np.int64) for c, b in bufs.items()}


def compare(m, got, e, cols=COLS):
    assert m == len(e["key"]), (m, len(e["key"]))
    o = np.argsort(got["key"][:m], kind="stable") if "key" in cols else None
    for c in cols:
        g = got[c][:m]
        # without the key column the rows have no name: the column's multiset
        g, want = (g[o], e[c]) if o is not None else (np.sort(g), np.sort(e[c]))
        assert np.array_equal(g, want), (c, np.flatnonzero(g != want)[:8])
        assert (got[c][m:] == SENTINEL).all(), c


def check(hj, key, val=None, cols=COLS, tuples=False, row_base=0, tensors=None):
    """The aggregate against numpy, all rows; returns the expectation."""
    val = AC.values_of(key, 5, row_base) if val is None else val
    e = AC.expect(key, val)
    m, got = run(hj, key, val, max(1, len(e["key"])), cols, tuples, row_base, tensors)
    compare(m, got, e, cols)
    return e


def assert_reports(hj, name):
    assert hj.strategy_used == name
    if name == "radix":
        assert lib.hj_ctx_join_kernel(hj._ctx) == _lib.HJ_JOIN_KERNEL_AGGREGATE == 9
        assert hj.join_kernel == "aggregate" and len(hj.radix_plan) >= 1
    else:
        assert hj.join_kernel is None and hj.radix_plan == []


# ------------------------------------------------------------------ global
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049])
def test_global_tile_edge(hj, n, dtype):
    with strategy(hj, "global"):
        e = check(hj, AC.keys_over(n, min(n, 37), n + 1, dtype))
        assert len(e["key"]) == min(n, 37)
        assert_reports(hj, "global")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_global_planted_keys(hj, dtype):
    key = AC.keys_over(5000, 700, 11, dtype, plant=planted(dtype))
    with strategy(hj, "global"):
        e = check(hj, key)
        assert len(e["key"]) == 700 and set(planted(dtype)) <= set(e["key"].tolist())
        if dtype == np.int64:
            check(hj, key, tuples=True)


def test_global_int64_min_is_the_only_key(hj):
    with strategy(hj, "global"):
        e = check(hj, np.full(3000, I64_MIN, np.int64))
        assert e["key"].tolist() == [I64_MIN] and e["cnt"].tolist() == [3000]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_global_one_key(hj, dtype):
    """One group with count = n: every tile's flush carries a partial count above 1."""
    with strategy(hj, "global"):
        e = check(hj, np.full(4099, 77, dtype))
        assert e["cnt"].tolist() == [4099]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_global_all_distinct(hj, dtype):
    """Each tile holds more distinct keys than its LDS table: the direct-to-global path."""
    key = (np.random.default_rng(6).permutation(1 << 20)[:6000] * 3 - 7000).astype(dtype)
    with strategy(hj, "global"):
        e = check(hj, key)
        assert len(e["key"]) == 6000 and (e["cnt"] == 1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_global_strided_tiles_and_offset_views(hj, dtype):
    """The persistent loops take a second tile (8 x CUs + 60 input tiles, a
    table of more than 8 x CUs x 2048 slots), and the inputs are views that
    start off a 16-byte boundary."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus + 60) * 2048 - 1000
    rng = np.random.default_rng(cus)
    key = rng.integers(0, 1 << 21, n).astype(dtype)
    key[::2048] = 5   # a key every tile holds
    val = AC.values_of(key, 9)
    tk = torch.empty(n + 3, dtype=torch.int64 if dtype == np.int64 else torch.int32, device="cuda")[3:]
    tv = torch.empty(n + 1, dtype=torch.int64, device="cuda")[1:]
    tk.copy_(torch.from_numpy(key))
    tv.copy_(torch.from_numpy(val))
    with strategy(hj, "global"):
        e = check(hj, key, val, tensors=(tk, tv))
        assert hj.capacity > 8 * cus * 2048 and e["cnt"].max() >= 8 * cus + 60


# ------------------------------------------------------------------ radix
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("bits", [5, 10, 19])
def test_radix_passes(hj, bits, dtype):
    key = AC.keys_over(200000, 50000, bits, dtype, plant=planted(dtype))
    with strategy(hj, "radix", bits):
        e = check(hj, key)
        assert len(e["key"]) == 50000 and hj.radix_passes == (bits + 8) // 9
        assert_reports(hj, "radix")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_radix_overflowing_partitions(hj, dtype):
    """Two partitions of ~50 000 distinct keys each, far more than an LDS
    table admits: the items are re-run in sub-splits and stay exact."""
    key = AC.keys_over(150000, 100000, 21, dtype, plant=planted(dtype))
    with strategy(hj, "radix", 1):
        e = check(hj, key)
        assert len(e["key"]) == 100000
        assert hj.count_distinct(dev(key)) == 100000   # the count-only form through the same splits


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("hot,dtype", [(12345, np.int64), (I64_MIN, np.int64), (12345, np.int32)],
                         ids=["i64", "i64-min", "i32"])
def test_radix_hot_key(hj, hot, dtype, bits):
    """299 000 of 300 000 rows share one key: its count exceeds 16 bits and its
    partition streams through one slot."""
    rng = np.random.default_rng(4)
    key = np.full(300000, hot, dtype)
    at = rng.permutation(300000)[:1000]
    key[at] = (np.arange(1000) * 7 + 100).astype(dtype)
    with strategy(hj, "radix", bits):
        e = check(hj, key)
        assert len(e["key"]) == 1001 and e["cnt"].max() == 299000
        assert_reports(hj, "radix")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_radix_all_distinct(hj, dtype):
    key = (np.random.default_rng(8).permutation(1 << 22)[:1 << 18] - (1 << 20)).astype(dtype)
    with strategy(hj, "radix"):
        e = check(hj, key)
        assert len(e["key"]) == 1 << 18


def test_radix_fresh_context_and_tuples():
    """A new context with no reserve call; then the packed-tuples form."""
    h = HashJoin(0)
    try:
        h.set_strategy("radix", radix_bits=7)
        key = AC.keys_over(60000, 9000, 31, plant=planted(np.int64))
        check(h, key)
        assert_reports(h, "radix")
        check(h, key, tuples=True)
        check(h, key[:0])
        check(h, key.astype(np.int32))
    finally:
        h.close()


# ------------------------------------------------------------------ both strategies
SUBSETS = [("key",), ("cnt",), ("sum",), ("min",), ("max",), ("cnt", "sum"), COLS]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", STRATEGIES)
def test_column_subsets_and_count_only(hj, name, dtype):
    key = AC.keys_over(20000, 3000, 41, dtype, plant=planted(dtype))
    val = AC.values_of(key, 41)
    with strategy(hj, name, 3):
        for cols in SUBSETS:
            check(hj, key, val, cols=cols)
        m, _ = run(hj, key, val, 0, cols=())
        assert m == 3000 == hj.count_distinct(dev(key))
        assert_reports(hj, name)


@pytest.mark.parametrize("name", STRATEGIES)
def test_error_paths(hj, name):
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    k = dev(np.array([3, 3, 4, I64_MIN], np.int64))
    k32 = k.to(torch.int32)
    o = torch.zeros(4, dtype=torch.int64, device="cuda")
    o32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    P = lambda t: t.data_ptr()   # noqa: E731
    ARG, OK = _lib.HJ_ERR_ARG, _lib.HJ_OK
    a64, a32, at = lib.hj_dev_aggregate_i64, lib.hj_dev_aggregate_i32, lib.hj_dev_aggregate_tuples_i64
    none5 = (None,) * 5
    with strategy(hj, name, 2):
        c = hj._ctx
        # the context first, then the count pointer, the relation, the outputs
        assert a64(None, None, None, -1, *none5, -1, None, None) == ARG and b"null context" in lib.hj_last_error()
        assert a64(c, None, None, -1, *none5, -1, None, None) == ARG and b"count pointer" in lib.hj_last_error()
        assert a64(c, None, None, 4, *none5, -1, P(cnt), None) == ARG and b"relation" in lib.hj_last_error()
        assert at(c, P(k), -1, *none5, -1, P(cnt), None) == ARG and b"relation" in lib.hj_last_error()
        assert a32(c, P(k32), 1 << 31, 0, P(o32), *none5[1:], 4, P(cnt), None) == ARG and b"row ids" in lib.hj_last_error()
        assert a32(c, P(k32), 4, -1, P(o32), *none5[1:], 4, P(cnt), None) == ARG and b"row ids" in lib.hj_last_error()
        for cap, first in ((-1, None), (4, None), (0, P(o))):
            assert a64(c, P(k), P(k), 4, first, *none5[1:], cap, P(cnt), None) == ARG
            assert b"output" in lib.hj_last_error()
        assert a32(c, P(k32), 4, 0, P(o32), *none5[1:], 0, P(cnt), None) == ARG and b"output" in lib.hj_last_error()
        # a value column is needed only by the aggregates that read it
        assert a64(c, P(k), None, 4, None, None, P(o), None, None, 4, P(cnt), None) == ARG
        assert b"value column" in lib.hj_last_error()
        assert a64(c, P(k), None, 4, P(o), P(o), None, None, None, 4, P(cnt), None) == OK
        torch.cuda.synchronize()
        assert int(cnt.item()) == 3
        assert a64(c, P(k), None, 4, *none5, 0, P(cnt), None) == OK   # the count-only form
        torch.cuda.synchronize()
        assert int(cnt.item()) == 3
        with pytest.raises(ValueError):
            hj.aggregate_into(k, k, out_key=o, out_cnt=o[:3])   # lengths differ
        with pytest.raises(ValueError):
            hj.aggregate_into(k, k, out_cnt=o32)                # the key's dtype
        with pytest.raises(ValueError):
            hj.aggregate_into(k32, k, out_key=o32)              # i32 rows carry row ids
        with pytest.raises(HJError):
            hj.aggregate_into(k, None, out_sum=o)               # no value column


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", STRATEGIES)
def test_capacity_below_m(hj, name, dtype):
    key = AC.keys_over(30000, 5000, 51, dtype, plant=planted(dtype))
    val = AC.values_of(key, 51)
    e = AC.expect(key, val)
    with strategy(hj, name, 4):
        for cap in (1, 777, 4999):
            m, got = run(hj, key, val, cap)
            assert m == 5000
            for c in COLS:
                assert (got[c][cap:] == SENTINEL).all(), (cap, c)
            k = got["key"][:cap]
            assert len(np.unique(k)) == cap
            at = np.searchsorted(e["key"], k)
            assert (e["key"][at] == k).all()
            for c in COLS:
                assert np.array_equal(got[c][:cap], e[c][at]), (cap, c)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_strategies_agree_and_match_the_group_probe(hj, dtype):
    """GLOBAL and RADIX give bit-equal rows, and both equal group_join(R = the
    distinct keys of S, S, how="matched"): the oracle-proven group probe."""
    key = AC.keys_over(40000, 6000, 61, dtype, plant=planted(dtype))
    val = AC.values_of(key, 61)
    wide = dtype == np.int64
    res = {}
    for name in STRATEGIES:
        with strategy(hj, name, 5):
            a = hj.aggregate(dev(key), dev(val) if wide else None, aggs=AGGS)
            o = np.argsort(a["key"].cpu().numpy(), kind="stable")
            res[name] = {c: t.cpu().numpy().astype(np.int64)[o] for c, t in a.items()}
    for c in res["global"]:
        assert np.array_equal(res["global"][c], res["radix"][c]), c
    rk = np.unique(key)
    r, g = hj.group_join(dev(rk), dev(rk) if wide else None, dev(key), dev(val) if wide else None, how="matched",
                         aggs=AGGS)
    r = r.cpu().numpy().astype(np.int64)
    gk = r if wide else rk[r].astype(np.int64)   # i32: the payload is R's row id
    o = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[o], res["global"]["key"])
    for c in AGGS:
        assert np.array_equal(g[c].cpu().numpy().astype(np.int64)[o], res["global"][c]), c



@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_auto_goes_by_rows(hj, dtype):
    hj.set_strategy("auto")
    check(hj, AC.keys_over(1000, 300, 71, dtype))
    assert_reports(hj, "global")
    n = (1 << 21) + 5
    key = np.random.default_rng(72).integers(-(1 << 19), 1 << 19, n).astype(dtype)
    e = check(hj, key)
    assert_reports(hj, "radix")
    assert len(e["key"]) > 1 << 19


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", STRATEGIES)
def test_state_after_an_aggregate(hj, oracle, name, dtype):
    """No build is left behind, and a build + probe after it works as before it."""
    rk, rp, sk, sp = oracle.gen_pkfk_i64(81, 30000, 50000, 0.7)
    wide = dtype == np.int64
    dt = torch.int64 if wide else torch.int32
    if not wide:   # the keys' low words (the join is compared with itself); i32 rows carry row ids, no payloads
        rk, sk, rp, sp = rk.astype(np.int32), sk.astype(np.int32), None, None

    def pay(p):
        return dev(p) if wide else None

    def join():
        hj.build_table(dev(rk), pay(rp))
        m = hj.count_rows(dev(sk))
        out_r = torch.empty(m, dtype=dt, device="cuda")
        out_s = torch.empty(m, dtype=dt, device="cuda")
        hj.probe_relation(dev(sk), pay(sp), out_r, out_s)
        pairs = np.stack([out_r.cpu().numpy(), out_s.cpu().numpy()], axis=1)
        return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]

    with strategy(hj, name, 5):
        first = join()
        assert len(first) > 0
        check(hj, sk, sp)
        assert_reports(hj, name)
        out = torch.empty(8, dtype=dt, device="cuda")
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            hj.probe_relation(dev(sk), pay(sp), out, out.clone())
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            hj.count_rows(dev(sk))
        with pytest.raises(HJError, match=str(_lib.HJ_ERR_STATE)):
            hj.count_group(dev(sk))
        assert lib.hj_ctx_build_has_duplicates(hj._ctx) == _lib.HJ_ERR_STATE
        assert np.array_equal(join(), first)
        assert hj.join_kernel != "aggregate"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", STRATEGIES)
def test_timing_reports_the_call(hj, name, dtype):
    key = AC.keys_over(50000, 8000, 91, dtype)
    hj.set_timing(True)
    try:
        with strategy(hj, name, 6):
            check(hj, key)
            t = hj.last_timing()
            assert t["probe"] > 0
            if name == "radix":
                assert t["probe_partition"] > 0 and t["probe_join"] > 0
                # the split sums to the whole within the events' resolution (three
                # float differences of microsecond stamps: 20 us + 2 % is generous)
                assert abs(t["probe_partition"] + t["probe_join"] - t["probe"]) <= 0.02 + 0.02 * t["probe"]
            else:
                assert t["probe_partition"] == 0 and t["probe_join"] == t["probe"]
            assert_reports(hj, name)
    finally:
        hj.set_timing(False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [5000, 70000])
@pytest.mark.parametrize("name", STRATEGIES)
def test_graph_replay(name, n, dtype):
    """A captured aggregate, replayed after the inputs were overwritten in
    place: each replay equals numpy for its inputs (a stale table, counter or
    accumulator would carry the last replay's groups over).  i32: the value is
    the row id, so no value tensor is passed."""
    wide = dtype == np.int64
    dt = torch.int64 if wide else torch.int32
    h = HashJoin(0)
    g = None
    try:
        h.set_strategy(name, radix_bits=6 if name == "radix" else 0)
        h.reserve_aggregate(n, 64 if wide else 32)
        tk = torch.empty(n, dtype=dt, device="cuda")
        tv = torch.empty(n, dtype=torch.int64, device="cuda") if wide else None
        outs = {c: torch.empty(n, dtype=torch.int64 if c == "sum" else dt, device="cuda") for c in COLS}
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        sets = [AC.keys_over(n, d, 100 + d, dtype, plant=p)
                for d, p in ((n // 3, ()), (n // 50, planted(dtype)[:2]), (n, planted(dtype)[2:]))]

        def load(keys, vals):
            tk.copy_(torch.from_numpy(keys))
            if wide:
                tv.copy_(torch.from_numpy(vals))
            torch.cuda.synchronize()

        def call():
            h.aggregate_into(tk, tv, outs["key"], outs["cnt"], outs["sum"], outs["min"], outs["max"], count=cnt)

        load(sets[0], AC.values_of(sets[0], 0))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):   # one eager step on the capture stream first
            call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        torch.cuda.synchronize()
        assert h.strategy_used == name
        for j, keys in enumerate(sets[1:]):
            vals = AC.values_of(keys, 200 + j)
            load(keys, vals)
            for t in outs.values():
                t.fill_(SENTINEL)
            cnt.fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            e = AC.expect(keys, vals)
            m = int(cnt.item())
            got = {c: outs[c].cpu().numpy().astype(np.int64) for c in COLS}
            for c in COLS:
                assert (got[c][m:] == SENTINEL).all(), (j, c)
            compare(m, {c: a[:m] for c, a in got.items()}, e)
    finally:
        del g
        torch.cuda.synchronize()
        h.close()


def test_aggregate_and_distinct_methods(hj):
    key = AC.keys_over(9000, 1200, 95, plant=planted(np.int64))
    val = AC.values(9000, 95)
    e = AC.expect(key, val)
    a = hj.aggregate(dev(key), dev(val))
    assert sorted(a) == ["count", "key", "sum"] and all(len(t) == 1200 for t in a.values())
    o = np.argsort(a["key"].cpu().numpy())
    assert np.array_equal(a["key"].cpu().numpy()[o], e["key"]) and np.array_equal(a["sum"].cpu().numpy()[o], e["sum"])
    # a capacity below M: one more call at M
    a = hj.aggregate(dev(key), dev(val), aggs=("min", "max", "count"), capacity=5)
    o = np.argsort(a["key"].cpu().numpy())
    for name, col in (("min", "min"), ("max", "max"), ("count", "cnt")):
        assert np.array_equal(a[name].cpu().numpy()[o], e[col]), name
    d = hj.distinct(dev(key))
    assert d.dtype == torch.int64 and np.array_equal(np.sort(d.cpu().numpy()), e["key"])
    k32 = key.astype(np.int32)
    e32 = AC.expect(k32, AC.values_of(k32))
    a = hj.aggregate(dev(k32), aggs=("count", "min", "sum"))
    o = np.argsort(a["key"].cpu().numpy())
    assert a["key"].dtype == torch.int32 and a["count"].dtype == torch.int32 and a["sum"].dtype == torch.int64
    for name, col in (("key", "key"), ("count", "cnt"), ("min", "min"), ("sum", "sum")):
        assert np.array_equal(a[name].cpu().numpy().astype(np.int64)[o], e32[col]), name
    assert np.array_equal(np.sort(hj.distinct(dev(k32), capacity=3).cpu().numpy()), e32["key"])
    assert hj.count_distinct(dev(key[:0])) == 0 and len(hj.distinct(dev(key[:0]))) == 0
    with pytest.raises(ValueError):
        hj.aggregate(dev(key), dev(val), aggs=("mean",))
