"""CPU checks of the key filter (hj.h "Key filter"): every symbol is declared,
bound and exported, the Python side has its names, hj_filter_place is the
format's function (the known answers and the numpy model), hj_filter_blocks_for
sizes as documented, a null filter and bad create arguments are reported before
anything touches a device, and the host model (filter_cases) passes its own
checks."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import hashjoin
from hashjoin import _lib

L = hashjoin.lib
ARGC = {"hj_filter_blocks_for": 2, "hj_filter_place": 4, "hj_filter_create": 3, "hj_filter_destroy": 1,
        "hj_filter_words": 3, "hj_filter_reserve": 2, "hj_dev_filter_clear": 2, "hj_dev_filter_insert_i64": 4,
        "hj_dev_filter_insert_tuples_i64": 4, "hj_dev_filter_insert_i32": 4, "hj_dev_filter_merge": 3,
        "hj_dev_filter_apply_i64": 11, "hj_dev_filter_apply_tuples_i64": 9, "hj_dev_filter_apply_i32": 10}


def place(key, nblocks):
    b, m = C.c_int64(-1), (C.c_uint32 * 8)()
    assert L.hj_filter_place(key, nblocks, C.byref(b), m) == _lib.HJ_OK
    return b.value, list(m)


def test_filter_symbols_declared_bound_and_exported():
    names = hashjoin.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n, argc in ARGC.items():
        assert n in names, n
        assert len(getattr(L, n).argtypes) == argc, n
        assert n in exported, n
    text = open(_lib.HEADER_PATH).read()
    assert "#define HJ_FILTER_PASS 0" in text and "#define HJ_FILTER_REJECT 1" in text
    assert "#define HJ_ABI_VERSION 1" in text and L.hj_abi_version() == 1
    assert _lib.HJ_FILTER_PASS == 0 and _lib.HJ_FILTER_REJECT == 1
    # the loop-wrap sizes the GPU tests take from here
    assert _lib.FILTER_TILE % _lib.FILTER_BLOCK == 0 and _lib.FILTER_GRID_PER_CU >= 1


def test_python_side_has_the_names():
    assert hashjoin.KeyFilter is hashjoin.join.KeyFilter
    for m in ("clear", "insert", "merge", "apply", "count", "reserve", "close"):
        assert callable(getattr(hashjoin.KeyFilter, m)), m
    for m in ("key_filter", "filtered_join"):
        assert callable(getattr(hashjoin.HashJoin, m)), m
    import inspect

    from hashjoin import dist
    p = inspect.signature(dist.distributed_join).parameters
    assert "prefilter" in p and p["prefilter"].default is None
    sig = inspect.signature(hashjoin.KeyFilter.__init__).parameters
    assert sig["bits_per_key"].default == 16


def test_place_known_answers():
    for key, nblocks, block, mask in FC.KNOWN:
        assert place(key, nblocks) == (block, mask), (key, nblocks)
        b, m = FC.place([key], nblocks)   # and the model restates the same table
        assert (int(b[0]), m[0].tolist()) == (block, mask), (key, nblocks)
    assert int(FC.fmix64(np.uint64(5 ^ FC.XOR))) == 0xf9a60599c02adcdd


@pytest.mark.parametrize("nblocks", FC.PLACE_NBLOCKS)
def test_place_equals_the_model(nblocks):
    keys = FC.keys(nblocks % 1000 + 3, 10**4)
    keys[:6] = (FC.I64_MIN, -1, 0, 1, FC.I64_MAX, 1 << 32)
    wb, wm = FC.place(keys, nblocks)
    assert wb.min() >= 0 and wb.max() < nblocks
    b, m = C.c_int64(), (C.c_uint32 * 8)()
    for i, k in enumerate(keys.tolist()):
        assert L.hj_filter_place(k, nblocks, C.byref(b), m) == _lib.HJ_OK
        assert b.value == wb[i] and list(m) == wm[i].tolist(), (k, nblocks)


def test_place_takes_null_outputs_and_rejects_bad_nblocks():
    assert L.hj_filter_place(7, 10, None, None) == _lib.HJ_OK
    for nb in (0, -1, 1 << 31, 1 << 40):
        assert L.hj_filter_place(7, nb, None, None) == _lib.HJ_ERR_ARG
        assert b"nblocks" in L.hj_last_error()


def test_blocks_for():
    for n, bits in ((0, 16), (1, 4), (15, 16), (16, 16), (17, 16), (1 << 16, 16), (1 << 20, 8), (1000, 12), (3, 64),
                    (1 << 28, 24), ((1 << 31) - 1, 64)):
        assert L.hj_filter_blocks_for(n, bits) == FC.blocks_for(n, bits), (n, bits)
    assert L.hj_filter_blocks_for(1 << 16, 16) == 4096 and L.hj_filter_blocks_for(0, 16) == 1
    assert L.hj_filter_blocks_for(17, 16) == 2 and L.hj_filter_blocks_for(1000, 12) == 47
    for n, bits in ((-1, 16), (10, 3), (10, 65), (10, 0), (1 << 62, 64), (1 << 37, 16)):   # the last two: past 2^31 - 1 blocks
        assert L.hj_filter_blocks_for(n, bits) < 0, (n, bits)


def test_null_filter_is_an_argument_error():
    # everything else wrong too: the filter comes first
    calls = {"hj_filter_words": (None, None, None),
             "hj_filter_reserve": (None, -1),
             "hj_dev_filter_clear": (None, None),
             "hj_dev_filter_insert_i64": (None, None, -1, None),
             "hj_dev_filter_insert_tuples_i64": (None, None, -1, None),
             "hj_dev_filter_insert_i32": (None, None, -1, None),
             "hj_dev_filter_merge": (None, None, None),
             "hj_dev_filter_apply_i64": (None, 7, None, None, -1, None, None, None, -1, None, None),
             "hj_dev_filter_apply_tuples_i64": (None, 7, None, -1, None, None, -1, None, None),
             "hj_dev_filter_apply_i32": (None, 7, None, -1, -1, None, None, -1, None, None)}
    for n, args in calls.items():
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG, n
        assert b"null filter" in L.hj_last_error(), n
    L.hj_filter_destroy(None)   # a no-op


def test_create_checks_its_arguments_before_any_device():
    for nb in (0, -5, 1 << 31, 1 << 35):
        assert not L.hj_filter_create(0, nb, None)
        assert b"nblocks" in L.hj_last_error()
    for off in (8, 16, 4, 31):
        assert not L.hj_filter_create(0, 4, C.c_void_p(0x10000 + off))
        assert b"32-byte aligned" in L.hj_last_error()
    with pytest.raises(ValueError):
        hashjoin.KeyFilter()                      # neither n_keys nor nblocks
    with pytest.raises(ValueError):
        hashjoin.KeyFilter(100, bits_per_key=3)   # before any device is asked for


# ------------------------------------------------------------------ the model's own checks
def test_model_has_no_false_negatives_and_is_a_function_of_the_set():
    ins, _ = FC.disjoint(5, 1 << 12, 16)
    ins[:4] = (FC.I64_MIN, -1, 0, FC.I64_MAX)
    for nb in (1, 7, FC.blocks_for(len(ins), 16)):
        w = FC.build(ins, nb)
        assert FC.test(w, ins).all()
        assert np.array_equal(FC.build(ins, nb, dense=True), w) and np.array_equal(FC.build(ins, nb, dense=False), w)
        rng = np.random.default_rng(6)
        again = np.concatenate([ins, ins[rng.integers(0, len(ins), 500)]])[rng.permutation(len(ins) + 500)]
        assert np.array_equal(FC.build(again, nb), w)                         # order and repeats do not matter
        assert np.array_equal(FC.build(ins[:1000], nb) | FC.build(ins[1000:], nb), w)   # a union is an OR
    assert not FC.test(np.zeros((5, 8), np.uint32), ins).any()               # a cleared filter passes nothing
    small = np.array([-7, 0, 7, 1 << 31, -(1 << 31)], np.int64)
    assert np.array_equal(FC.build(small[:3].astype(np.int32), 9), FC.build(small[:3], 9))   # i32 = its sign extension
    # one key sets exactly one bit in each word of one block
    w = FC.build([42], 5)
    assert (w != 0).any(axis=1).sum() == 1 and all(bin(int(x)).count("1") == 1 for x in w[(w != 0).any(axis=1)][0])


@pytest.mark.parametrize("bits, cap", [(16, 0.005), (8, 0.06)])
def test_model_false_positive_caps(bits, cap):
    """2^16 inserted, 2^20 disjoint absent random keys.  The caps keep a broken
    model (one that sets every bit, say) from passing: the format itself gives
    0.13 % at 16 bits per key and 3.3 % at 8."""
    ins, absent = FC.disjoint(7, 1 << 16, 1 << 20)
    w = FC.build(ins, FC.blocks_for(len(ins), bits))
    assert FC.test(w, ins).all()
    fp = int(FC.test(w, absent).sum())
    print(f"bits per key {bits}: {fp} of {len(absent)} false positives ({100.0 * fp / len(absent):.3f} %)")
    assert fp <= cap * len(absent)
