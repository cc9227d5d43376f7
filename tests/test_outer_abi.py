"""CPU checks of the probe-side outer join entry points (hj_dev_probe_outer_*):
they are declared, exported and bound, and their argument errors are reported
before anything touches a device."""
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
OUTER = ("hj_dev_probe_outer_i64", "hj_dev_probe_outer_tuples_i64", "hj_dev_probe_outer_i32")


def _call(name, ctx):
    """The count-only form over an empty relation, with no count pointer."""
    if name == "hj_dev_probe_outer_i64":
        return L.hj_dev_probe_outer_i64(ctx, None, None, 0, -1, None, None, 0, None, None)
    if name == "hj_dev_probe_outer_tuples_i64":
        return L.hj_dev_probe_outer_tuples_i64(ctx, None, 0, -1, None, None, 0, None, None)
    return L.hj_dev_probe_outer_i32(ctx, None, 0, 0, -1, None, None, 0, None, None)


def test_outer_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n in OUTER:
        assert n in names
        f = getattr(L, n)
        assert f.argtypes is not None and f.restype is _lib._int
    # (context, relation ..., null value, two outputs, capacity, count, stream)
    assert len(L.hj_dev_probe_outer_i64.argtypes) == 10
    assert len(L.hj_dev_probe_outer_tuples_i64.argtypes) == 9
    assert len(L.hj_dev_probe_outer_i32.argtypes) == 10
    assert L.hj_abi_version() == 1
    assert "#define HJ_ABI_VERSION 1" in open(_lib.HEADER_PATH).read()


def test_null_context_is_an_argument_error():
    for n in OUTER:
        assert _call(n, None) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()
    # the context is looked at first: an i32 row-id range that is itself an error
    assert L.hj_dev_probe_outer_i32(None, None, 5, -3, -1, None, None, 0, None, None) == _lib.HJ_ERR_ARG
    assert b"null context" in L.hj_last_error()


def _ctx_without_build():
    """As test_exists_abi's: a context no build has run on, where a device lets
    hj_ctx_create make one; (None, False) on a machine without a device."""
    import torch
    if torch.cuda.is_available():
        ctx = L.hj_ctx_create(0)
        assert ctx
        return ctx, True
    return None, False


def test_missing_build_is_a_state_error():
    ctx, real = _ctx_without_build()
    if not real:
        return   # (no device: the null-context order above is all that can be checked)
    try:
        for n in OUTER:
            assert _call(n, ctx) == _lib.HJ_ERR_STATE
            assert b"build" in L.hj_last_error()
    finally:
        L.hj_ctx_destroy(ctx)
