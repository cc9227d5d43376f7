"""CPU checks of the expand probe's entry points (hj_dev_expand_*): they are
exported and bound, the kernel constant is declared, the ABI version did not
move, and a null context is reported before anything touches a device."""
import numpy as np

import expand_cases as XC
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
EXPAND = ("hj_dev_expand_i64", "hj_dev_expand_i32")


def test_expand_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n in EXPAND:
        assert n in names
        assert len(getattr(L, n).argtypes) == 10
    assert "hj_ctx_reserve_expand" in names and len(L.hj_ctx_reserve_expand.argtypes) == 3
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_JOIN_KERNEL_EXPAND 10" in text
    assert "#define HJ_EXPAND_INNER 0" in text and "#define HJ_EXPAND_OUTER 1" in text
    assert "#define HJ_ABI_VERSION 1" in text
    assert _lib.HJ_JOIN_KERNEL_EXPAND == 10
    assert (_lib.HJ_EXPAND_INNER, _lib.HJ_EXPAND_OUTER) == (0, 1)
    assert L.hj_abi_version() == 1


def test_python_side_names_the_kernel_and_the_methods():
    H = hashjoin.HashJoin
    assert H.JOIN_KERNELS[10] == "k_join_expand"
    for m in ("reserve_expand", "probe_expand", "count_expand", "expand", "ordered_join"):
        assert callable(getattr(H, m)), m


def test_null_context_is_an_argument_error():
    for n in EXPAND:
        assert getattr(L, n)(None, 0, None, 0, -1, None, None, 0, None, None) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()
    assert L.hj_ctx_reserve_expand(None, 0, 64) == _lib.HJ_ERR_ARG
    assert b"null context" in L.hj_last_error()


def test_expectation_builder_on_a_hand_made_case():
    """expand_cases against a result written out by hand."""
    rk = np.array([5, 9, 5, 3], np.int64)
    rp = np.array([10, 20, 30, 40], np.int64)
    sk = np.array([5, 7, 3, 5], np.int64)
    e = XC.ExpandExpect(rk, rp, sk, "inner", -9)
    assert e.off.tolist() == [0, 2, 2, 3, 5] and e.m == 5 and not e.unique
    assert e.sorted_within(e.r).tolist() == [10, 30, 40, 10, 30]
    assert e.same_values(np.array([30, 10, 40, 10, 30])) and not e.same_values(np.array([30, 30, 40, 10, 30]))
    assert e.same_values(np.array([30, 10, 40, 30]), 4) and not e.same_values(np.array([30, 10, 40, 40]), 4)
    o = XC.ExpandExpect(rk, rp, sk, "outer", -9)
    assert o.off.tolist() == [0, 2, 3, 4, 6] and o.r[2] == -9
    z = XC.ExpandExpect(rk[:0], rp[:0], sk, "outer", -9)
    assert z.off.tolist() == [0, 1, 2, 3, 4] and (z.r == -9).all()
