"""CPU checks of the build-side / full outer join entry points
(hj_dev_probe_full_*): they are declared, exported and bound, and their
argument errors are reported in the documented order before anything touches
a device."""
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
FULL = ("hj_dev_probe_full_i64", "hj_dev_probe_full_tuples_i64", "hj_dev_probe_full_i32")


def _call(name, ctx, kind=_lib.HJ_OUTER_FULL):
    """The count-only form over an empty relation, with no count pointer."""
    if name == "hj_dev_probe_full_i64":
        return L.hj_dev_probe_full_i64(ctx, kind, None, None, 0, -1, -1, None, None, 0, None, None)
    if name == "hj_dev_probe_full_tuples_i64":
        return L.hj_dev_probe_full_tuples_i64(ctx, kind, None, 0, -1, -1, None, None, 0, None, None)
    return L.hj_dev_probe_full_i32(ctx, kind, None, 0, 0, -1, -1, None, None, 0, None, None)


def test_full_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n in FULL:
        assert n in names
        f = getattr(L, n)
        assert f.argtypes is not None and f.restype is _lib._int
    # (context, kind, relation ..., two null values, two outputs, capacity, count, stream)
    assert len(L.hj_dev_probe_full_i64.argtypes) == 12
    assert len(L.hj_dev_probe_full_tuples_i64.argtypes) == 11
    assert len(L.hj_dev_probe_full_i32.argtypes) == 12
    assert (_lib.HJ_OUTER_BUILD, _lib.HJ_OUTER_FULL) == (1, 2)
    header = open(_lib.HEADER_PATH).read()
    assert "#define HJ_OUTER_BUILD 1" in header and "#define HJ_OUTER_FULL 2" in header
    assert L.hj_abi_version() == 1
    assert "#define HJ_ABI_VERSION 1" in header


def test_null_context_is_reported_first():
    for n in FULL:
        for kind in (_lib.HJ_OUTER_BUILD, _lib.HJ_OUTER_FULL, 0, 3):   # ahead of a bad kind too
            assert _call(n, None, kind) == _lib.HJ_ERR_ARG
            assert b"null context" in L.hj_last_error()
    # and ahead of an i32 row-id range that is itself an error
    assert L.hj_dev_probe_full_i32(None, 2, None, 5, -3, -1, -1, None, None, 0, None, None) == _lib.HJ_ERR_ARG
    assert b"null context" in L.hj_last_error()


def _ctx_without_build():
    """A context no build has run on, where a device lets hj_ctx_create make
    one; (None, False) on a machine without a device."""
    import torch
    if torch.cuda.is_available():
        ctx = L.hj_ctx_create(0)
        assert ctx
        return ctx, True
    return None, False


def test_bad_kind_then_missing_build():
    ctx, real = _ctx_without_build()
    if not real:
        return   # (no device: the null-context order above is all that can be checked)
    try:
        for n in FULL:
            for kind in (0, 3):
                assert _call(n, ctx, kind) == _lib.HJ_ERR_ARG
                assert b"kind" in L.hj_last_error()
            for kind in (_lib.HJ_OUTER_BUILD, _lib.HJ_OUTER_FULL):
                assert _call(n, ctx, kind) == _lib.HJ_ERR_STATE
                assert b"build" in L.hj_last_error()
    finally:
        L.hj_ctx_destroy(ctx)
