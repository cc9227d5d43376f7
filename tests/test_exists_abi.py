"""CPU checks of the semi- / anti-join entry points (hj_dev_exists_*): they are
exported and bound, and their argument errors are reported before anything
touches a device."""
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
EXISTS = ("hj_dev_exists_i64", "hj_dev_exists_tuples_i64", "hj_dev_exists_i32")


def _call(name, ctx, kind):
    if name == "hj_dev_exists_i64":
        return L.hj_dev_exists_i64(ctx, kind, None, None, 0, None, None, 0, None, None)
    if name == "hj_dev_exists_tuples_i64":
        return L.hj_dev_exists_tuples_i64(ctx, kind, None, 0, None, None, 0, None, None)
    return L.hj_dev_exists_i32(ctx, kind, None, 0, 0, None, None, 0, None, None)


def test_exists_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n in EXISTS:
        assert n in names
        assert getattr(L, n).argtypes is not None
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_EXISTS_SEMI 0" in text and "#define HJ_EXISTS_ANTI 1" in text
    assert "#define HJ_JOIN_KERNEL_EXISTS 6" in text
    assert (_lib.HJ_EXISTS_SEMI, _lib.HJ_EXISTS_ANTI, _lib.HJ_JOIN_KERNEL_EXISTS) == (0, 1, 6)
    assert L.hj_abi_version() == 1


def test_null_context_is_an_argument_error():
    for n in EXISTS:
        for kind in (_lib.HJ_EXISTS_SEMI, _lib.HJ_EXISTS_ANTI):
            assert _call(n, None, kind) == _lib.HJ_ERR_ARG
        assert b"null context" in L.hj_last_error()


def _ctx_without_build():
    """A context no build has run on, where a device lets hj_ctx_create make
    one (it launches nothing); (None, False) on a machine without a device."""
    import torch
    if torch.cuda.is_available():
        ctx = L.hj_ctx_create(0)
        assert ctx
        return ctx, True
    return None, False


def test_unknown_kind_and_missing_build():
    ctx, real = _ctx_without_build()
    if not real:
        # no device: only the null-context order can be checked -- the kind is
        # looked at after the context, so a bad kind on a null context is
        # still the context's error
        for n in EXISTS:
            assert _call(n, None, 2) == _lib.HJ_ERR_ARG
            assert _call(n, None, -1) == _lib.HJ_ERR_ARG
        return
    try:
        for n in EXISTS:
            for kind in (2, -1):
                assert _call(n, ctx, kind) == _lib.HJ_ERR_ARG
                assert b"kind" in L.hj_last_error()
            assert _call(n, ctx, _lib.HJ_EXISTS_SEMI) == _lib.HJ_ERR_STATE
            assert _call(n, ctx, _lib.HJ_EXISTS_ANTI) == _lib.HJ_ERR_STATE
    finally:
        L.hj_ctx_destroy(ctx)
