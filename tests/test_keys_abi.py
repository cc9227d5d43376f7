"""CPU checks of the composite-key codec (hj.h "Composite keys"): every symbol
is exported and bound, HJ_ERR_RANGE is declared, a null codec and a bad column
set are reported before anything touches a device, the Python side has its
names, and the host model (keys_cases) answers its own known cases."""
import ctypes as C

import numpy as np

import hashjoin
import keys_cases as KC
from hashjoin import _lib

L = hashjoin.lib
ARGC = {"hj_keycodec_create": 3, "hj_keycodec_destroy": 1, "hj_dev_keycodec_reset": 2, "hj_dev_keycodec_observe": 4,
        "hj_dev_keycodec_seal": 2, "hj_dev_keycodec_pack": 5, "hj_dev_keycodec_pack_tuples": 6,
        "hj_dev_keycodec_unpack": 5, "hj_keycodec_info": 7}


def test_keys_symbols_declared_and_bound():
    names = hashjoin.declared_symbols()
    for n, argc in ARGC.items():
        assert n in names
        assert len(getattr(L, n).argtypes) == argc
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_ERR_RANGE (-6)" in text
    assert "#define HJ_KEYS_MAX_COLS 4" in text
    assert "#define HJ_ABI_VERSION 1" in text
    assert _lib.HJ_ERR_RANGE == -6 and _lib.HJ_KEYS_MAX_COLS == 4
    assert L.hj_abi_version() == 1
    # the loop-wrap sizes the GPU tests take from here
    assert _lib.KEYS_TILE % _lib.KEYS_BLOCK == 0 and _lib.KEYS_GRID_PER_CU >= 1


def test_null_codec_is_an_argument_error():
    # everything else wrong too: the codec comes first
    calls = {"hj_dev_keycodec_reset": (None, None),
             "hj_dev_keycodec_observe": (None, None, -1, None),
             "hj_dev_keycodec_seal": (None, None),
             "hj_dev_keycodec_pack": (None, None, -1, None, None),
             "hj_dev_keycodec_pack_tuples": (None, None, None, -1, None, None),
             "hj_dev_keycodec_unpack": (None, None, -1, None, None),
             "hj_keycodec_info": (None, None, None, None, None, None, None)}
    for n, args in calls.items():
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG, n
        assert b"null codec" in L.hj_last_error(), n
    L.hj_keycodec_destroy(None)   # a no-op


def test_create_checks_its_arguments_before_any_device():
    four = (C.c_int * 5)(64, 32, 64, 32, 64)
    for ncols in (0, 5, -1):
        assert not L.hj_keycodec_create(0, ncols, four)
        assert b"ncols" in L.hj_last_error()
    assert not L.hj_keycodec_create(0, 2, (C.c_int * 2)(64, 16))
    assert b"col_bits" in L.hj_last_error()
    assert not L.hj_keycodec_create(0, 1, None)
    assert b"col_bits" in L.hj_last_error()


def test_python_side_has_the_names():
    assert hashjoin.KeyCodec is hashjoin.join.KeyCodec
    for m in ("observe", "seal", "pack", "pack_tuples", "unpack", "reset", "info", "close"):
        assert callable(getattr(hashjoin.KeyCodec, m))
    for m in ("join_on", "aggregate_on", "distinct_on"):
        assert callable(getattr(hashjoin.HashJoin, m))
    assert hashjoin.HashJoin.JOIN_ON_KINDS == ("inner", "semi", "anti", "left", "right", "full")


# ------------------------------------------------------------------ the model's own known cases
def test_model_small_ranges():
    a = np.array([3, 12, 7], np.int32)            # span 9: 4 bits
    b = np.array([5, 5, 5], np.int64)             # constant: 0 bits
    c = np.array([-1000, 0, 1047], np.int64)      # span 2047: 11 bits
    pl = KC.plan([[a, b, c]])
    assert pl["bits"] == [4, 0, 11] and pl["shift"] == [11, 11, 0] and pl["total_bits"] == 15 and pl["fits"]
    assert pl["lo"] == [3, 5, -1000] and pl["hi"] == [12, 5, 1047] and pl["rows_observed"] == 3
    k = KC.pack_py(pl, [a, b, c])
    assert k.tolist() == [0 << 11 | 0, 9 << 11 | 1000, 4 << 11 | 2047]
    assert np.array_equal(KC.pack(pl, [a, b, c]), k)
    # a span of exactly a power of two takes one bit more
    assert KC.plan([[np.array([0, 8], np.int64)]])["bits"] == [4]
    assert KC.plan([[np.array([0, 7], np.int64)]])["bits"] == [3]
    # two relations: the union of the ranges; an empty relation changes nothing
    e = [a[:0], b[:0], c[:0]]
    p2 = KC.plan([[a, b, c], e, [a + 100, b, c]])
    assert p2["lo"][0] == 3 and p2["hi"][0] == 112 and p2["rows_observed"] == 6
    # nothing observed: all widths 0, lo = hi = 0
    p0 = KC.plan([e])
    assert p0["bits"] == [0, 0, 0] and p0["lo"] == p0["hi"] == [0, 0, 0] and p0["total_bits"] == 0


def test_model_totals_of_exactly_64():
    const = np.array([7, 7, 7], np.int64)
    full = np.array([KC.I64_MIN, -1, KC.I64_MAX], np.int64)
    pl = KC.plan([[const, full]])
    assert pl["bits"] == [0, 64] and pl["shift"] == [64, 0] and pl["total_bits"] == 64 and pl["fits"]
    k = KC.pack_py(pl, [const, full])             # the 0-bit column is never shifted
    assert k.view(np.uint64).tolist() == [0, (1 << 63) - 1, (1 << 64) - 1]
    assert np.array_equal(KC.pack(pl, [const, full]), k)
    x = np.array([KC.I32_MIN, 0, KC.I32_MAX], np.int32)
    y = np.array([KC.I32_MAX, KC.I32_MIN, -1], np.int32)
    pl = KC.plan([[x, y]])
    assert pl["bits"] == [32, 32] and pl["shift"] == [32, 0] and pl["total_bits"] == 64 and pl["fits"]
    k = KC.pack_py(pl, [x, y])
    assert k.view(np.uint64).tolist() == [0xFFFFFFFF, 1 << 63, (0xFFFFFFFF << 32) | 0x7FFFFFFF]
    assert k[1] == KC.I64_MIN                     # the INT64_MIN word is an ordinary key
    assert np.array_equal(KC.pack(pl, [x, y]), k)


def test_model_flags_65_bits():
    full = np.array([KC.I64_MIN, KC.I64_MAX], np.int64)
    two = np.array([0, 1], np.int64)
    pl = KC.plan([[full, two]])
    assert pl["bits"] == [64, 1] and pl["total_bits"] == 65 and not pl["fits"]


def test_model_round_trip_and_order():
    for name, (dtypes, _) in KC.SHAPES.items():
        cols = KC.relation(name, 500, 11)
        pl = KC.plan([cols])
        assert pl["fits"], name
        k = KC.pack_py(pl, cols)
        assert np.array_equal(KC.pack(pl, cols), k), name
        for back in (KC.unpack_py(pl, k, dtypes), KC.unpack(pl, k, dtypes)):
            assert all(np.array_equal(b, c) and b.dtype == c.dtype for b, c in zip(back, cols)), name
        # injective on the observed box, and the UNSIGNED key order is the tuples' lexicographic order
        rows = np.stack([c.astype(np.int64) for c in cols], axis=1)
        assert len(np.unique(k)) == len(np.unique(rows, axis=0)), name
        ku = k.view(np.uint64)
        assert np.array_equal(np.sort(ku), ku[KC.lex_order(cols)]), name
        assert not KC.outside(pl, cols).any()
