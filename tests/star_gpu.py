"""What the star family's GPU tests (test_gpu_star, test_gpu_star_agg,
test_gpu_star_query) share: the contexts and the StarProbe they run on, the
host <-> device helpers, sentinel-filled outputs, the comparison of group rows
by key, the snapshot that shows a context was only read, and the ctypes arrays
of the raw calls."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import star_cases as SC
from hashjoin import HashJoin, StarProbe

NULL, SENTINEL, EXTRA, TILE = SC.NULL, SC.SENTINEL, SC.EXTRA, SC.TILE
WIDTHS = [True, False]
IDS = ["i64", "i32"]
GROUP_AGGS = ("count", "sum", "min", "max")
ARG = {"key": "out_key", "cnt": "out_cnt", "sum": "out_sum", "min": "out_min", "max": "out_max"}


@pytest.fixture(scope="module")
def ctxs():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    hs = [HashJoin(0) for _ in range(4)]
    for h in hs:
        h.set_strategy("global")
    yield hs
    for h in hs:
        h.close()


@pytest.fixture(scope="module")
def star(request):
    """The module's StarProbe, with a group table of the module's STAR_GROUPS groups where it names some."""
    s = StarProbe(0)
    if getattr(request.module, "STAR_GROUPS", 0):
        s.reserve_groups(request.module.STAR_GROUPS)
    yield s
    s.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.int64)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def sentinels(n, dtype=torch.int64):
    return torch.full((n,), SENTINEL, dtype=dtype, device="cuda")


def build(ctxs, c, keys=None):
    """Every dimension of case c built in its own context: the call's dimension list.
    keys: the probe key columns already on the device."""
    dims = []
    for i, (h, d) in enumerate(zip(ctxs, c["dims"])):
        h.build_table(dev(d["rk"]), dev(d["rp"]) if c["wide"] else None)
        assert h.strategy_used == "global"
        dims.append((h, dev(d["sk"]) if keys is None else keys[i], d["how"], d["null"]))
    return dims


@functools.lru_cache(maxsize=None)
def strided_keys(wide):
    return [dev(d["sk"]) for d in SC.strided_case(wide)["dims"]]


def compare(got, x, upto, full):
    """got: the host columns written (a dict by column name), x the expectation
    sorted by key.  Every row below `upto` is a true group row with its own
    aggregates; full: they are all the groups."""
    if "key" in got:
        k = got["key"][:upto]
        idx = np.searchsorted(x["key"], k)
        assert (idx < len(x["key"])).all() and np.array_equal(x["key"][idx], k), "a key that is no group"
        assert len(np.unique(k)) == upto, "a group twice"
        for col, g in got.items():
            assert np.array_equal(g[:upto], x[col][idx]), (col, np.flatnonzero(g[:upto] != x[col][idx])[:8])
    elif full:   # no key column to match rows by: each column as a multiset
        for col, g in got.items():
            assert np.array_equal(np.sort(g[:upto]), np.sort(x[col])), col
    if full:
        assert upto == len(x["key"])


def check_groups(cnt, bufs, x, cap):
    """A grouped call's count and the columns it wrote (a dict by column name,
    sentinel-filled before, `cap` of each passed) against x: true group rows
    below min(G, cap), the sentinel from there on."""
    g, G = int(cnt.item()), len(x["key"])
    assert g == G, (g, G)
    upto = min(g, cap)
    got = {col: host(b) for col, b in bufs.items()}
    for col, a in got.items():
        assert (a[upto:] == SENTINEL).all(), col
    compare(got, x, upto, upto == G)


def context_state(dims, n, wide):
    """What each dimension's context answers to a lookup and a join of its key column, and its host facts."""
    out = []
    for h, sk, _, _ in dims:
        o_r = sentinels(n, torch.int64 if wide else torch.int32)
        o_c = sentinels(n, torch.int32)
        hits = int(h.probe_lookup(sk, o_r, o_c, null=NULL).item())
        pairs = int(h.probe_relation(sk, sk if wide else None).item())
        out.append((hits, pairs, host(o_r), host(o_c), h.has_duplicates(), h.strategy_used, h.capacity))
    return out


def assert_same_state(before, after):
    for b, a in zip(before, after):
        assert b[:2] == a[:2] and b[4:] == a[4:]
        assert np.array_equal(b[2], a[2]) and np.array_equal(b[3], a[3])


def dim_arrays(wide, hs, kinds, keys, nulls=True):
    """A raw call's (contexts, kinds, key columns, nulls) as ctypes arrays; a None entry is a null pointer,
    nulls=False a null array, no dimension four null arrays."""
    k = len(hs)
    if not k:
        return None, None, None, None
    return ((C.c_void_p * k)(*[None if h is None else h._ctx for h in hs]), (C.c_int * k)(*kinds),
            (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in keys]),
            ((C.c_int64 if wide else C.c_int32) * k)(*[NULL] * k) if nulls else None)
