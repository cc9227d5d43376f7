"""CPU checks of the group probe entry points (hj_dev_group_*,
hj_ctx_reserve_group): they are exported and bound, the constants are
declared, and a null context is reported before anything touches a device."""
import numpy as np

import group_cases as GC
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
ARGC = {"hj_dev_group_i64": 14, "hj_dev_group_tuples_i64": 13, "hj_dev_group_i32": 14, "hj_ctx_reserve_group": 3}


def test_group_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n, argc in ARGC.items():
        assert n in names
        assert len(getattr(L, n).argtypes) == argc
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_JOIN_KERNEL_GROUP 8" in text
    assert "#define HJ_GROUP_MATCHED 0" in text and "#define HJ_GROUP_ALL 1" in text
    assert "#define HJ_ABI_VERSION 1" in text
    assert (_lib.HJ_JOIN_KERNEL_GROUP, _lib.HJ_GROUP_MATCHED, _lib.HJ_GROUP_ALL) == (8, 0, 1)
    assert L.hj_abi_version() == 1


def test_python_side_names_the_kernel_and_the_methods():
    H = hashjoin.HashJoin
    assert H.JOIN_KERNELS[8] == "k_join_group"
    for m in ("reserve_group", "probe_group", "probe_group_tuples", "count_group", "group_join"):
        assert callable(getattr(H, m))


def test_null_context_is_an_argument_error():
    # everything else wrong too (the kind, the relation, the outputs): the context comes first
    calls = {"hj_dev_group_i64": (None, 7, None, None, -1, 0, None, None, None, None, None, -1, None, None),
             "hj_dev_group_tuples_i64": (None, 7, None, -1, 0, None, None, None, None, None, -1, None, None),
             "hj_dev_group_i32": (None, 7, None, -1, -1, 0, None, None, None, None, None, -1, None, None),
             "hj_ctx_reserve_group": (None, -1, 7)}
    for n, args in calls.items():
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()


def test_numpy_expectation_wraps_and_keeps_extremes():
    v = GC.values(1000, 3)
    assert v.min() == GC.I64_MIN and v.max() == GC.I64_MAX
    e = GC.expect(np.array([1], np.int64), np.array([0], np.int64), np.ones(1000, np.int64), v)
    with np.errstate(over="ignore"):
        assert e["sum"][0] == v.sum() and e["cnt"][0] == 1000
    assert e["min"][0] == GC.I64_MIN and e["max"][0] == GC.I64_MAX
