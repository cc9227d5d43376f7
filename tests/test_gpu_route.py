"""hj_dev_route_i64 (the folded routing's send side) against a numpy
restatement: part = the top log2(nranks) + sub_bits bits of key *
0x9E3779B97F4A7C15 mod 2^64 (radix_hash, csrc/hj_internal.h).  The counts are
the restatement's bincount, part p's rows are exactly the input rows of part
p, and nothing is written outside the n output rows: the output is a view
into a sentinel-filled buffer with 64 guard rows on either side (the exact
pass writes partial first and last lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

from hashjoin import HashJoin
from hashjoin._lib import check, lib
from routed_layout import rparts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (2, 4), (8, 6), (64, 3), (256, 1)]   # small and full-size pass variants, the 9-bit limit
SIZES = [0, 1, 4095, 4096, 4097, 8193, 100003]
NMAX = max(SIZES)
GUARD = 64
SENTINEL = 0x5A5A5A5A5A5A5A5A
INT64_MIN = -(1 << 63)
# (key column offset, payload column offset, output row offset), in elements / rows:
# cols_aligned is false whenever a column is 8 B off; k_slot_hist looks at the key pointer alone
LAYOUTS = {"aligned": (0, 0, 0), "both_off": (1, 1, 0), "key_off": (1, 0, 0), "pay_off": (0, 1, 0),
           "out_off": (0, 0, 1)}


@pytest.fixture(scope="module")
def hj():
    h = HashJoin(0)
    yield h
    h.close()


def _host_data(kind):
    rng = np.random.default_rng(20260 + len(kind))
    key = rng.integers(INT64_MIN, (1 << 63) - 1, NMAX, dtype=np.int64, endpoint=True)
    key[::997] = INT64_MIN            # INT64_MIN keys present (row 0 among them)
    key[5::1013] = key[5]             # and a repeated ordinary key
    if kind == "hot":                 # 40 % of the rows on one key, spread over the tiles
        key[rng.random(NMAX) < 0.4] = key[11]
    pay = rng.integers(INT64_MIN, (1 << 63) - 1, NMAX, dtype=np.int64, endpoint=True)
    return key, pay


@pytest.fixture(scope="module")
def data():
    """kind -> host (key, pay) and device copies at element offsets 0 and 1
    (a torch allocation is at least 256-B aligned; one int64 further is not
    16-B aligned)."""
    out = {}
    for kind in ("uniform", "hot"):
        key, pay = _host_data(kind)
        dev = {}
        for name, col in (("key", key), ("pay", pay)):
            for off in (0, 1):
                buf = torch.zeros(NMAX + 2, dtype=torch.int64, device="cuda")
                buf[off:off + NMAX] = torch.from_numpy(col).cuda()
                assert buf.data_ptr() % 256 == 0
                dev[name, off] = buf
        out[kind] = (key, pay, dev)
    return out


def _route_guarded(hj, key, pay, n, nranks, sub, out_off):
    """Route into rows [GUARD + out_off, + n) of a sentinel-filled buffer;
    returns (rows, counts) on the host after checking the guards."""
    parts = nranks << sub
    buf = torch.full((GUARD + out_off + n + GUARD, 2), SENTINEL, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 128 == 0
    lo = GUARD + out_off
    out = buf[lo:lo + n]
    counts = torch.full((parts + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    cview = counts[GUARD:GUARD + parts]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    check(lib.hj_dev_route_i64(hj._ctx, vp(key), vp(pay), n, nranks, sub, vp(out), vp(cview),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hj_dev_route_i64")
    b, c = buf.cpu().numpy(), counts.cpu().numpy()
    assert (b[:lo] == SENTINEL).all() and (b[lo + n:] == SENTINEL).all(), "rows written outside the output"
    assert (c[:GUARD] == SENTINEL).all() and (c[GUARD + parts:] == SENTINEL).all(), "counts written outside"
    return b[lo:lo + n], c[GUARD:GUARD + parts]


def _assert_routed(rows, counts, key, pay, bits):
    n = len(key)
    part = rparts(key, bits)
    assert np.array_equal(counts, np.bincount(part, minlength=1 << bits))
    # part p's rows sorted by (key, payload) == the input rows of part p sorted the same way
    got_part = np.repeat(np.arange(1 << bits), counts)
    assert len(got_part) == n
    og = np.lexsort((rows[:, 1], rows[:, 0], got_part))
    oi = np.lexsort((pay, key, part))
    assert np.array_equal(got_part[og], part[oi])
    assert np.array_equal(rows[og, 0], key[oi]) and np.array_equal(rows[og, 1], pay[oi])
    # (and each row sits in the part its own key hashes to)
    assert np.array_equal(rparts(rows[:, 0], bits), got_part)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nranks,sub", SHAPES)
def test_route_vs_restatement(hj, data, nranks, sub, n, layout):
    key, pay, dev = data["uniform"]
    ko, po, oo = LAYOUTS[layout]
    dk, dp = dev["key", ko][ko:ko + n], dev["pay", po][po:po + n]
    if n:
        assert dk.data_ptr() % 16 == 8 * ko and dp.data_ptr() % 16 == 8 * po
    rows, counts = _route_guarded(hj, dk, dp, n, nranks, sub, oo)
    _assert_routed(rows, counts, key[:n], pay[:n], (nranks.bit_length() - 1) + sub)


@pytest.mark.parametrize("layout", ["aligned", "key_off", "out_off"])
@pytest.mark.parametrize("n", [4097, 100003])
@pytest.mark.parametrize("nranks,sub", SHAPES)
def test_route_hot_key_vs_restatement(hj, data, nranks, sub, n, layout):
    """40 % of the rows on one key: a tile's largest bin holds more than an
    eighth of it, the pass's hot-bin counting."""
    key, pay, dev = data["hot"]
    assert 0.35 < (key[:n] == key[11]).mean() < 0.45
    ko, po, oo = LAYOUTS[layout]
    rows, counts = _route_guarded(hj, dev["key", ko][ko:ko + n], dev["pay", po][po:po + n], n, nranks, sub, oo)
    _assert_routed(rows, counts, key[:n], pay[:n], (nranks.bit_length() - 1) + sub)
