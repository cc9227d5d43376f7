"""CPU checks of the hash aggregate entry points (hj_dev_aggregate_*,
hj_ctx_reserve_aggregate): they are exported and bound, the constant is
declared, a null context is reported before anything touches a device, and
the numpy expectation answers its own known cases."""
import numpy as np

import aggregate_cases as AC
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
ARGC = {"hj_dev_aggregate_i64": 12, "hj_dev_aggregate_tuples_i64": 11, "hj_dev_aggregate_i32": 12,
        "hj_ctx_reserve_aggregate": 3}


def test_aggregate_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n, argc in ARGC.items():
        assert n in names
        assert len(getattr(L, n).argtypes) == argc
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_JOIN_KERNEL_AGGREGATE 9" in text
    assert "#define HJ_ABI_VERSION 1" in text
    assert _lib.HJ_JOIN_KERNEL_AGGREGATE == 9
    assert L.hj_abi_version() == 1


def test_python_side_names_the_kernel_and_the_methods():
    H = hashjoin.HashJoin
    assert H.JOIN_KERNELS[9] == "aggregate" and "aggregate" in H.JOIN_KERNELS.values()
    for m in ("reserve_aggregate", "aggregate_into", "aggregate_tuples_into", "count_distinct", "aggregate",
              "distinct"):
        assert callable(getattr(H, m))


def test_null_context_is_an_argument_error():
    # everything else wrong too (the relation, the outputs, the count pointer): the context comes first
    calls = {"hj_dev_aggregate_i64": (None, None, None, -1, None, None, None, None, None, -1, None, None),
             "hj_dev_aggregate_tuples_i64": (None, None, -1, None, None, None, None, None, -1, None, None),
             "hj_dev_aggregate_i32": (None, None, -1, -1, None, None, None, None, None, -1, None, None),
             "hj_ctx_reserve_aggregate": (None, -1, 7)}
    for n, args in calls.items():
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()


def test_numpy_expectation_wraps_and_keeps_extremes():
    v = AC.values(1000, 3)
    assert v.min() == AC.I64_MIN and v.max() == AC.I64_MAX
    e = AC.expect(np.full(1000, AC.I64_MIN, np.int64), v)
    with np.errstate(over="ignore"):
        assert e["sum"].tolist() == [int(v.sum())] and e["cnt"].tolist() == [1000]
    assert e["key"].tolist() == [AC.I64_MIN] and e["min"].tolist() == [AC.I64_MIN] and e["max"].tolist() == [AC.I64_MAX]
    # a sum that wraps: INT64_MAX + 1 is INT64_MIN
    w = AC.expect(np.array([3, 3], np.int64), np.array([AC.I64_MAX, 1], np.int64))
    assert w["sum"].tolist() == [AC.I64_MIN] and w["min"].tolist() == [1] and w["max"].tolist() == [AC.I64_MAX]
    # n == 0: no rows, five empty int64 columns
    z = AC.expect(np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert set(z) == set(AC.COLS) and all(len(a) == 0 for a in z.values())
    # i32: min / max are the key's first and last row, as np.unique(return_index) gives the first
    k = np.array([4, -1, 4, 4, -1], np.int32)
    e = AC.expect(k, AC.values_of(k))
    first = np.unique(k, return_index=True)[1]
    assert e["min"].tolist() == first.tolist() == [1, 0] and e["max"].tolist() == [4, 3]
