"""CPU checks of the positional lookup entry points (hj_dev_lookup_*): they
are exported and bound, the kernel constant is declared, and a null context
is reported before anything touches a device."""
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
LOOKUP = ("hj_dev_lookup_i64", "hj_dev_lookup_i32")


def _call(name, ctx):
    return getattr(L, name)(ctx, None, 0, -1, None, None, None, None)


def test_lookup_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n in LOOKUP:
        assert n in names
        assert len(getattr(L, n).argtypes) == 8
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_JOIN_KERNEL_LOOKUP 7" in text
    assert "#define HJ_ABI_VERSION 1" in text
    assert _lib.HJ_JOIN_KERNEL_LOOKUP == 7
    assert L.hj_abi_version() == 1


def test_python_side_names_the_kernel_and_the_methods():
    assert hashjoin.HashJoin.JOIN_KERNELS[7] == "k_join_lookup"
    assert callable(hashjoin.HashJoin.probe_lookup) and callable(hashjoin.HashJoin.lookup)


def test_null_context_is_an_argument_error():
    for n in LOOKUP:
        assert _call(n, None) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()
