"""CPU checks of the as-of probe's entry points (hj_dev_asof_*): they are
exported and bound, the constants are declared, a null context is reported
before anything touches a device -- and the numpy expectation the GPU tests
compare against answers hand-made cases."""
import numpy as np

import asof_cases as AC
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
ASOF = ("hj_dev_asof_i64", "hj_dev_asof_i32")


def test_asof_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n in ASOF:
        assert n in names
        assert len(getattr(L, n).argtypes) == 9
    text = open(_lib.HEADER_PATH).read()
    for line in ("#define HJ_ASOF_BACKWARD 0", "#define HJ_ASOF_FORWARD  1", "#define HJ_ASOF_STRICT   2",
                 "#define HJ_JOIN_KERNEL_ASOF 11", "#define HJ_ABI_VERSION 1"):
        assert line in text, line
    assert (_lib.HJ_ASOF_BACKWARD, _lib.HJ_ASOF_FORWARD, _lib.HJ_ASOF_STRICT) == (0, 1, 2)
    assert _lib.HJ_JOIN_KERNEL_ASOF == 11
    assert L.hj_abi_version() == 1


def test_python_side_names_the_kernel_and_the_methods():
    H = hashjoin.HashJoin
    assert H.JOIN_KERNELS[11] == "k_join_asof"
    assert callable(H.probe_asof) and callable(H.asof) and callable(H.asof_join)


def test_null_context_is_an_argument_error():
    for n in ASOF:
        # everything else wrong too (the kind among it): the context comes first
        assert getattr(L, n)(None, 7, None, None, -1, -1, None, None, None) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()


def test_expectation_on_hand_cases():
    rk = np.array([5, 5, 5, 9, 7], np.int64)
    rp = np.array([10, -4, 30, 10, AC.I64_MIN], np.int64)
    sk = np.array([5, 5, 5, 5, 9, 9, 3, 7, 7], np.int64)
    sb = np.array([10, 9, -5, 31, 10, 11, 10, AC.I64_MIN, AC.I64_MAX], np.int64)
    N = -99
    want = {0: [10, -4, N, 30, 10, 10, N, AC.I64_MIN, AC.I64_MIN],
            1: [10, 10, -4, N, 10, N, N, AC.I64_MIN, N],
            2: [-4, -4, N, 30, N, 10, N, N, AC.I64_MIN],
            3: [30, 10, -4, N, N, N, N, N, N]}
    for kind in AC.KINDS:
        got, found = AC.expect(rk, rp, sk, sb, kind, N)
        assert got.tolist() == want[kind], kind
        assert found.tolist() == [v != N for v in want[kind]]
    got, found = AC.expect(rk[:0], rp[:0], sk, sb, 0, N)
    assert (got == N).all() and not found.any()


def test_join_loop_on_hand_cases():
    rk = np.array([1, 1, 1, 2], np.int64)
    rt = np.array([10, 10, 20, 15], np.int64)
    sk = np.array([1, 1, 1, 2, 3, 1], np.int64)
    st = np.array([10, 15, 5, 15, 15, 30], np.int64)
    assert AC.asof_join_loop(rk, rt, sk, st).tolist() == [1, 1, -1, 3, -1, 2]
    assert AC.asof_join_loop(rk, rt, sk, st, "forward").tolist() == [0, 2, 0, 3, -1, -1]
    assert AC.asof_join_loop(rk, rt, sk, st, "nearest").tolist() == [1, 1, 0, 3, -1, 2]   # 15: a tie, backward
    assert AC.asof_join_loop(rk, rt, sk, st, exact=False).tolist() == [-1, 1, -1, -1, -1, 2]
    assert AC.asof_join_loop(rk, rt, sk, st, tolerance=4).tolist() == [1, -1, -1, 3, -1, -1]
