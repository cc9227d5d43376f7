"""The key filter on the GPU (hj.h "Key filter"): the words after clear /
insert / merge, apply's compaction, the linear graph, filtered_join on both
strategies and distributed_join(prefilter=...) over RCCL at world size 1.

Every expectation comes from the host model (filter_cases, numpy), never from
the library: the words are compared bit for bit, apply's rows element by
element in input order.  Outputs are SENTINEL-filled and EXTRA rows longer than
what may be written: nothing may be written past the capacity."""
import contextlib
import ctypes as C
import itertools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import filter_cases as FC
from hashjoin import KeyFilter, _lib, gen_pkfk, lib
from join_gpu import dev, hj, sentinels, strategy  # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SENTINEL, EXTRA = -12345, 64
I64_MIN, I64_MAX = FC.I64_MIN, FC.I64_MAX
STRATEGIES = ["global", "radix"]
KINDS = ["pass", "reject"]
FORMS = ["i64", "tuples", "i32"]


@contextlib.contextmanager
def new_filter(nblocks):
    """A filter whose words start as garbage (they are undefined until the first clear)."""
    f = KeyFilter(nblocks=nblocks)
    f.words.fill_(0x5A5A5A5A5A5A5A5A)
    try:
        yield f
    finally:
        f.close()


def words_of(f):
    return f.words.cpu().numpy().view(np.uint32).reshape(-1, 8)


def same_words(f, want):
    got = words_of(f)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:4], got[bad[:2]], want[bad[:2]])


def wrap_rows():
    """A row count at which the insert and apply loops take a second step: more
    tiles than the capped grid has workgroups, and a ragged tail."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * _lib.FILTER_GRID_PER_CU * _lib.FILTER_TILE + _lib.FILTER_TILE + 77


# ------------------------------------------------------------------ words after insert
def insert_cases():
    return {
        "one-key": (lambda: np.array([42], np.int64), 1),
        # ~30 keys per block: many lanes of one wave OR into the same block (about 60 % of its bits end up set)
        "crowded-7-blocks": (lambda: FC.keys(101, 210), 7),
        "one-key-5000-times": (lambda: np.full(5000, -987654321, np.int64), 3),
        "extremes": (lambda: np.array([I64_MIN, -1, 0, I64_MAX], np.int64), 5),
        "4099-blocks": (lambda: FC.keys(102, 30000), 4099),
        "2^20+7-blocks": (lambda: FC.keys(103, 50000), (1 << 20) + 7),
        "small-values": (lambda: np.arange(-3000, 3001, dtype=np.int64), 400),
    }


@pytest.mark.parametrize("name", list(insert_cases()))
def test_words_after_insert_match_the_model(name):
    make, nb = insert_cases()[name]
    keys = make()
    want = FC.build(keys, nb)
    assert not (want == 0xFFFFFFFF).all(axis=1).any()   # no saturated block: an all-ones filter hides errors
    with new_filter(nb) as f:
        f.clear()
        f.insert(dev(keys))
        same_words(f, want)
        # the tuples form and (where the values fit) the i32 form give the same filter
        f.clear()
        f.insert(dev(np.stack([keys, keys * 3 + 1], axis=1)))
        same_words(f, want)
        if np.abs(keys).max() < (1 << 31):
            f.clear()
            f.insert(dev(keys.astype(np.int32)))
            same_words(f, want)


def test_i32_insert_is_the_insert_of_the_sign_extended_values():
    k32 = np.random.default_rng(104).integers(-(1 << 31), (1 << 31) - 1, 9001, dtype=np.int64, endpoint=True)
    k32[:4] = (-(1 << 31), -1, 0, (1 << 31) - 1)
    k32 = k32.astype(np.int32)
    nb = FC.blocks_for(len(k32), 16)
    want = FC.build(k32.astype(np.int64), nb)
    with new_filter(nb) as f, new_filter(nb) as g:
        f.clear()
        f.insert(dev(k32))
        g.clear()
        g.insert(dev(k32.astype(np.int64)))
        same_words(f, want)
        same_words(g, want)
        f.clear()
        f.insert(dev(np.concatenate([[7], k32]).astype(np.int32))[1:])   # 4 bytes off a 16-byte boundary
        same_words(f, want)


def test_unaligned_columns_and_two_inserts():
    keys = FC.keys(105, 6001)
    nb = FC.blocks_for(6000, 12)
    with new_filter(nb) as f:
        d = dev(keys)
        assert d[1:].data_ptr() % 16 == 8
        f.clear()
        f.insert(d[1:])                                     # the element path
        same_words(f, FC.build(keys[1:], nb))
        t = dev(np.stack([keys, keys], axis=1).reshape(-1))[1:-1].view(-1, 2)   # tuples 8 bytes off: rows {k[i], k[i+1]}
        assert t.data_ptr() % 16 == 8
        f.clear()
        f.insert(t)
        same_words(f, FC.build(keys[:-1], nb))
        # two inserts (and an empty one, with a null pointer) against their union
        f.clear()
        f.insert(d[:2500])
        f.insert(d[:0])
        assert lib.hj_dev_filter_insert_i64(f._f, None, 0, None) == _lib.HJ_OK
        f.insert(d[2000:])
        same_words(f, FC.build(keys, nb))
        assert lib.hj_dev_filter_insert_i64(f._f, None, 5, None) == _lib.HJ_ERR_ARG
        assert lib.hj_dev_filter_insert_i64(f._f, d.data_ptr(), -1, None) == _lib.HJ_ERR_ARG


def test_insert_past_the_capped_grid():
    n = wrap_rows()
    keys = FC.keys(106, n)
    nb = FC.blocks_for(n, 16)
    with new_filter(nb) as f:
        f.clear()
        f.insert(dev(keys))
        same_words(f, FC.build(keys, nb))


def test_caller_owned_words_with_guards_and_clear():
    """The library works in the caller's buffer, touches nothing past its end,
    and a filter it allocates itself behaves the same."""
    nb, guard = 37, 8
    keys = FC.keys(107, 300)
    want = FC.build(keys, nb)
    buf = sentinels(nb * 4 + guard, SENTINEL, torch.int64)
    f = KeyFilter(words=buf[:nb * 4])
    try:
        assert f.nblocks == nb and f.words.data_ptr() == buf.data_ptr()
        p, n = C.c_void_p(), C.c_int64()
        assert lib.hj_filter_words(f._f, C.byref(p), C.byref(n)) == _lib.HJ_OK
        assert p.value == buf.data_ptr() and n.value == nb
        f.clear()
        assert (buf[:nb * 4] == 0).all() and (buf[nb * 4:] == SENTINEL).all()
        f.insert(dev(keys))
        same_words(f, want)
        assert (buf[nb * 4:] == SENTINEL).all()
        assert f.count(dev(keys)) == len(keys)
        f.clear()                                           # clear after insert: all zeros, passes nothing
        assert (buf[:nb * 4] == 0).all() and (buf[nb * 4:] == SENTINEL).all()
        assert f.count(dev(keys)) == 0 and f.count(dev(keys), "reject") == len(keys)
    finally:
        f.close()
    own = lib.hj_filter_create(0, nb, None)                 # the filter allocates and owns its words
    assert own
    try:
        assert lib.hj_dev_filter_clear(own, None) == _lib.HJ_OK
        d = dev(keys)
        assert lib.hj_dev_filter_insert_i64(own, d.data_ptr(), len(keys), None) == _lib.HJ_OK
        p, n = C.c_void_p(), C.c_int64()
        assert lib.hj_filter_words(own, C.byref(p), C.byref(n)) == _lib.HJ_OK and n.value == nb and p.value % 32 == 0
        with new_filter(nb) as g:                            # its words, read by merging them into a cleared filter
            g.clear()
            assert lib.hj_dev_filter_merge(g._f, own, None) == _lib.HJ_OK
            same_words(g, want)
    finally:
        lib.hj_filter_destroy(own)


def test_merge_is_the_or_of_two_filters():
    a, b = FC.keys(108, 4000), FC.keys(109, 2500)
    nb = FC.blocks_for(6500, 16)
    with new_filter(nb) as f, new_filter(nb) as g, new_filter(nb + 1) as other:
        f.clear()
        f.insert(dev(a))
        g.clear()
        g.insert(dev(b))
        f.merge(g)
        same_words(f, FC.build(a, nb) | FC.build(b, nb))
        same_words(f, FC.build(np.concatenate([a, b]), nb))
        same_words(g, FC.build(b, nb))                       # the other side is only read
        assert f.count(dev(np.concatenate([a, b]))) == 6500  # a key merged in always passes
        # a words tensor (another rank's words, gathered) merges the same way
        f.clear()
        f.insert(dev(a))
        f.merge_words(dev(FC.as_i64(FC.build(b, nb))))
        same_words(f, FC.build(np.concatenate([a, b]), nb))
        before = words_of(f).copy()
        assert lib.hj_dev_filter_merge(f._f, other._f, None) == _lib.HJ_ERR_ARG
        assert b"geometry" in lib.hj_last_error()
        assert lib.hj_dev_filter_merge(f._f, None, None) == _lib.HJ_ERR_ARG
        same_words(f, before)


# ------------------------------------------------------------------ apply
@pytest.fixture(scope="module")
def probe_data():
    """One build side (2^12 keys at 8 bits per key: a few per cent of the
    absent keys pass, so the model decides every row) and one probe relation
    of wrap_rows() rows that every apply test takes a prefix of."""
    build = FC.keys(110, 1 << 12)
    build[:4] = (I64_MIN, -1, 0, I64_MAX)
    nb = FC.blocks_for(len(build), 8)
    words = FC.build(build, nb)
    n = wrap_rows()
    skey = FC.relation(111, n, build, hit=0.4)
    spay = np.arange(n, dtype=np.int64) * 5 - 11
    passes = FC.test(words, skey)
    assert 0.4 < passes.mean() < 0.5 and passes[:70].any() and not passes[:70].all()
    # the i32 relation: its own build side and filter
    b32 = np.random.default_rng(112).integers(-(1 << 31), (1 << 31) - 1, 1 << 12, dtype=np.int64, endpoint=True)
    w32 = FC.build(b32, nb)
    s32 = np.random.default_rng(113).integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int64, endpoint=True)
    hit = np.random.default_rng(114).random(n) < 0.4
    s32[hit] = b32[np.random.default_rng(115).integers(0, len(b32), int(hit.sum()))]
    return dict(nb=nb, build=build, words=words, skey=skey, spay=spay, passes=passes, b32=b32, w32=w32,
                s32=s32.astype(np.int32), passes32=FC.test(w32, s32))


@pytest.fixture(scope="module")
def filters(probe_data):
    f, f32 = KeyFilter(nblocks=probe_data["nb"]), KeyFilter(nblocks=probe_data["nb"])
    for flt, b in ((f, probe_data["build"]), (f32, probe_data["b32"])):
        flt.clear()
        flt.insert(dev(b))
    same_words(f, probe_data["words"])
    same_words(f32, probe_data["w32"])
    yield {"i64": f, "tuples": f, "i32": f32}
    f.close()
    f32.close()


ROW_BASE = 1000


def run_apply(f, form, kind, pd, n, outs, cap, skey_dev=None):
    """One apply of the first n rows into SENTINEL-filled outputs of cap rows
    (+ EXTRA guard rows); checks the count, the rows in input order and that
    nothing is written at or past cap.  outs: a subset of key / pay / row."""
    if form == "i32":
        sk, mask, dt = pd["s32"][:n], pd["passes32"][:n], torch.int32
    else:
        sk, mask, dt = pd["skey"][:n], pd["passes"][:n], torch.int64
    sp = pd["spay"][:n]
    idx = np.flatnonzero(mask if kind == "pass" else ~mask)
    M = len(idx)
    want = {"key": np.stack([sk[idx], sp[idx]], axis=1) if form == "tuples" else sk[idx], "pay": sp[idx],
            "row": (idx + ROW_BASE).astype(np.int32) if form == "i32" else idx}
    if cap == "M-1":
        cap = max(M - 1, 1)
    elif cap == "M":
        cap = max(M, 1)
    elif cap == "M+5":
        cap = M + 5
    bufs = {}
    for o in outs:
        shape = (cap + EXTRA, 2) if (o == "key" and form == "tuples") else (cap + EXTRA,)
        bufs[o] = torch.full(shape, SENTINEL, dtype=torch.int64 if o == "pay" else dt, device="cuda")
    views = {o: b[:cap] for o, b in bufs.items()}
    if skey_dev is None:
        skey_dev = dev(np.stack([sk, sp], axis=1)) if form == "tuples" else dev(sk)
    cnt = sentinels(1, SENTINEL, torch.int64)
    f.apply_into(skey_dev, dev(sp) if (form == "i64" and "pay" in outs) else None, kind, views.get("key"),
                 views.get("pay"), views.get("row"), count=cnt, row_base=ROW_BASE)
    assert int(cnt.item()) == M, (form, kind, n, int(cnt.item()), M)
    k = min(M, cap)
    for o, b in bufs.items():
        got = b.cpu().numpy()
        assert np.array_equal(got[:k], want[o][:k]), (form, kind, n, o, np.flatnonzero(got[:k] != want[o][:k])[:8])
        assert (got[k:] == SENTINEL).all(), (form, kind, n, o, "written past the capacity")
    return M


def apply_sizes():
    t = _lib.FILTER_TILE
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, "wrap"]


@pytest.mark.parametrize("n", apply_sizes())
@pytest.mark.parametrize("kind", KINDS)
def test_apply_matches_the_model_in_input_order(filters, probe_data, kind, n):
    n = wrap_rows() if n == "wrap" else n
    all_outs = {"i64": ("key", "pay", "row"), "tuples": ("key", "row"), "i32": ("key", "row")}
    total = 0
    for form in FORMS:
        total += run_apply(filters[form], form, kind, probe_data, n, all_outs[form], max(n, 1))
        run_apply(filters[form], form, kind, probe_data, n, (), 0)            # the count form
    assert n < 64 or total > 0


@pytest.mark.parametrize("kind", KINDS)
def test_apply_every_subset_of_the_outputs_and_every_capacity(filters, probe_data, kind):
    n = _lib.FILTER_TILE * 2 + 77
    for form, names in (("i64", ("key", "pay", "row")), ("tuples", ("key", "row")), ("i32", ("key", "row"))):
        subsets = [s for r in range(1, len(names) + 1) for s in itertools.combinations(names, r)]
        for outs in subsets:
            run_apply(filters[form], form, kind, probe_data, n, outs, n)
        for cap in ("M-1", "M", "M+5"):
            for outs in (names, names[-1:]):
                run_apply(filters[form], form, kind, probe_data, n, outs, cap)


def test_apply_unaligned_relations(filters, probe_data):
    n = 5001
    pd = probe_data
    for kind in KINDS:
        k = dev(np.concatenate([[9], pd["skey"][:n]]))[1:]
        assert k.data_ptr() % 16 == 8
        run_apply(filters["i64"], "i64", kind, pd, n, ("key", "pay", "row"), n, skey_dev=k)
        t = dev(np.concatenate([[9], np.stack([pd["skey"][:n], pd["spay"][:n]], axis=1).reshape(-1)]))[1:].view(-1, 2)
        assert t.data_ptr() % 16 == 8
        run_apply(filters["tuples"], "tuples", kind, pd, n, ("key", "row"), n, skey_dev=t)
        k32 = dev(np.concatenate([[9], pd["s32"][:n]]).astype(np.int32))[1:]
        assert k32.data_ptr() % 16 == 4
        run_apply(filters["i32"], "i32", kind, pd, n, ("key", "row"), n, skey_dev=k32)


def test_apply_argument_errors(filters, probe_data):
    f = filters["i64"]._f
    k = dev(probe_data["skey"][:100])
    o = sentinels(100, SENTINEL, torch.int64)
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    A = lib.hj_dev_filter_apply_i64
    kp, op, cp = k.data_ptr(), o.data_ptr(), c.data_ptr()
    assert A(f, 2, kp, None, 100, op, None, None, 100, cp, None) == _lib.HJ_ERR_ARG and b"kind" in lib.hj_last_error()
    assert A(f, 2, kp, None, 100, op, None, None, 100, None, None) == _lib.HJ_ERR_ARG and b"kind" in lib.hj_last_error()
    assert A(f, 0, kp, None, 100, op, None, None, 100, None, None) == _lib.HJ_ERR_ARG and b"count" in lib.hj_last_error()
    assert A(f, 0, None, None, 100, op, None, None, 100, cp, None) == _lib.HJ_ERR_ARG
    assert A(f, 0, kp, None, -1, op, None, None, 100, cp, None) == _lib.HJ_ERR_ARG
    assert A(f, 0, kp, None, 100, None, op, None, 100, cp, None) == _lib.HJ_ERR_ARG      # out_pay without spay
    assert A(f, 0, kp, None, 100, None, None, None, 100, cp, None) == _lib.HJ_ERR_ARG    # a capacity, no output
    assert A(f, 0, kp, None, 100, op, None, None, 0, cp, None) == _lib.HJ_ERR_ARG        # an output, no capacity
    assert A(f, 0, kp, None, 100, op, None, None, -1, cp, None) == _lib.HJ_ERR_ARG
    k32 = dev(probe_data["s32"][:100])
    assert lib.hj_dev_filter_apply_i32(filters["i32"]._f, 0, k32.data_ptr(), 100, (1 << 31) - 50, None, None, 0, cp,
                                       None) == _lib.HJ_ERR_ARG                           # row ids past 2^31 - 1
    torch.cuda.synchronize()
    assert (o == SENTINEL).all() and int(c.item()) == 0                                   # nothing ran


def test_cleared_filter_passes_nothing_and_inserted_keys_all_pass():
    keys = FC.keys(116, 1 << 16)
    absent = FC.disjoint(117, 16, 1 << 16)[1]
    nb = FC.blocks_for(len(keys), 16)
    with new_filter(nb) as f:
        f.clear()
        assert f.count(dev(keys)) == 0 and f.count(dev(keys), "reject") == len(keys)
        assert f.apply(dev(keys)).numel() == 0
        f.insert(dev(keys))
        assert f.count(dev(keys)) == len(keys) and f.count(dev(keys), "reject") == 0
        got, rows = f.apply(dev(keys), with_rows=True)
        assert np.array_equal(got.cpu().numpy(), keys) and np.array_equal(rows.cpu().numpy(), np.arange(len(keys)))
        want = FC.test(FC.build(keys, nb), absent)
        assert f.count(dev(absent)) == int(want.sum()) < len(absent) // 100
        # apply(): the undersized output is resized at the exact M
        k, p = f.apply(dev(keys[:5000]), dev(keys[:5000] + 1), capacity=7)
        assert np.array_equal(k.cpu().numpy(), keys[:5000]) and np.array_equal(p.cpu().numpy(), keys[:5000] + 1)


# ------------------------------------------------------------------ graph
def test_linear_graph_replays_over_new_data():
    """clear, insert R, insert R2, apply S captured once on a side stream;
    replayed after the buffers were overwritten, the words and the rows are the
    new data's."""
    nr, nr2, ns = 3000, 1001, 9001
    nb = FC.blocks_for(nr + nr2, 8)

    def data(seed):
        r, r2 = FC.keys(seed, nr), FC.keys(seed + 50, nr2)
        return r, r2, FC.relation(seed + 100, ns, np.concatenate([r, r2]), hit=0.3), FC.keys(seed + 150, ns)

    sets = [data(201), data(202), data(203)]
    f = KeyFilter(nblocks=nb)
    g = None
    try:
        tr, tr2 = (torch.empty(n, dtype=torch.int64, device="cuda") for n in (nr, nr2))
        tk, tp = (torch.empty(ns, dtype=torch.int64, device="cuda") for _ in range(2))
        ok, op, orow = (torch.empty(ns + EXTRA, dtype=torch.int64, device="cuda") for _ in range(3))
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        f.reserve(ns)

        def load(r, r2, sk, sp):
            for t, a in ((tr, r), (tr2, r2), (tk, sk), (tp, sp)):
                t.copy_(torch.from_numpy(a))
            for o in (ok, op, orow, cnt):
                o.fill_(SENTINEL)
            f.words.fill_(-1)
            torch.cuda.synchronize()

        def call(s):
            f.clear(stream=s)
            f.insert(tr, stream=s)
            f.insert(tr2, stream=s)
            f.apply_into(tk, tp, "pass", ok[:ns], op[:ns], orow[:ns], count=cnt, stream=s)

        load(*sets[0])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):   # one eager step on the capture stream first
            call(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(s)
        torch.cuda.synchronize()
        for r, r2, sk, sp in sets[1:] + sets[:1]:
            load(r, r2, sk, sp)
            g.replay()
            torch.cuda.synchronize()
            want = FC.build(np.concatenate([r, r2]), nb)
            same_words(f, want)
            idx = np.flatnonzero(FC.test(want, sk))
            m = len(idx)
            assert int(cnt.item()) == m and 0 < m < ns
            for got, w in ((ok, sk[idx]), (op, sp[idx]), (orow, idx)):
                a = got.cpu().numpy()
                assert np.array_equal(a[:m], w) and (a[m:] == SENTINEL).all()
    finally:
        del g
        torch.cuda.synchronize()
        f.close()


# ------------------------------------------------------------------ filtered_join
@pytest.fixture(scope="module")
def join_data():
    rng = np.random.default_rng(301)
    rk = FC.keys(302, 3000)
    rk[:3] = (I64_MIN, 0, I64_MAX)
    rk[100:200] = rk[:100]                                  # repeated build keys
    rp = np.arange(len(rk), dtype=np.int64) * 2 + 1000
    sk = FC.relation(303, 20000, rk, hit=0.3)
    sk[:2] = (I64_MIN, 5)
    sp = rng.permutation(len(sk)).astype(np.int64) + 500000
    return rk, rp, sk, sp


def sorted_pairs(a, b):
    x = np.stack([a.cpu().numpy(), b.cpu().numpy()], axis=1)
    return x[np.lexsort((x[:, 1], x[:, 0]))]


@pytest.mark.parametrize("how", ["inner", "semi", "anti"])
@pytest.mark.parametrize("name", STRATEGIES)
def test_filtered_join_equals_the_unfiltered_join(hj, join_data, name, how):
    rk, rp, sk, sp = join_data
    d = [dev(x) for x in join_data]
    hit = np.isin(sk, rk)
    with strategy(hj, name, 4):
        if how == "inner":
            want = sorted_pairs(*hj.join(d[0], d[1], d[2], d[3]))
            got = sorted_pairs(*hj.filtered_join(d[0], d[1], d[2], d[3]))
            by_key = {}
            for k, p in zip(rk.tolist(), rp.tolist()):
                by_key.setdefault(k, []).append(p)
            host = sorted((p, s) for k, s in zip(sk.tolist(), sp.tolist()) for p in by_key.get(k, ()))
            assert got.tolist() == [list(t) for t in host]
        else:
            f = hj.semi_join if how == "semi" else hj.anti_join
            want = np.sort(f(d[0], d[2], d[3], d[1]).cpu().numpy())
            got = np.sort(hj.filtered_join(d[0], d[1], d[2], d[3], how=how).cpu().numpy())
            assert np.array_equal(got, np.sort(sp[hit if how == "semi" else ~hit]))
            wk = hj.filtered_join(d[0], d[1], d[2], d[3], how=how, with_keys=True)
            assert np.array_equal(sorted_pairs(*wk), sorted_pairs(dev(sk[hit if how == "semi" else ~hit]),
                                                                  dev(sp[hit if how == "semi" else ~hit])))
        assert hj.strategy_used == name
        assert np.array_equal(got, want)
    words = FC.build(rk, FC.blocks_for(len(rk), 16))
    assert hj.last_filtered == (len(sk), int(FC.test(words, sk).sum()))


def test_filtered_join_drops_rows_on_a_selective_join(hj):
    nr, ns = 1 << 14, 1 << 16
    rk, rp, sk, sp = gen_pkfk(0x5EED, nr, ns, frac=0.25)
    want = sorted_pairs(*hj.join(rk, rp, sk, sp))
    got = sorted_pairs(*hj.filtered_join(rk, rp, sk, sp))
    assert np.array_equal(got, want) and 0.2 * ns < len(got) < 0.3 * ns
    words = FC.build(rk.cpu().numpy(), FC.blocks_for(nr, 16))
    kept = int(FC.test(words, sk.cpu().numpy()).sum())
    assert hj.last_filtered == (ns, kept) and len(got) <= kept < ns // 3
    with pytest.raises(ValueError):
        hj.filtered_join(rk, rp, sk, sp, how="left")
    with pytest.raises(TypeError):
        hj.filtered_join(rk.to(torch.int32), None, sk.to(torch.int32))


# ------------------------------------------------------------------ distributed
def test_rccl_distributed_join_prefilter_world1():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "rccl_filter_worker.py"), str(port)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "RCCL_FILTER_WORKER_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
