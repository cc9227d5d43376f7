"""positional_cases on a CPU-only machine: the fuzz list's size caps and what
it covers, the four expectation helpers against plain nested loops over the
definitions of include/hj.h, and the strided relation's structure."""
import hashlib

import numpy as np
import pytest

import asof_cases as AC
import expand_cases as XC
import group_cases as GC
import outer_cases as OC
import positional_cases as PC

I64_MIN, I64_MAX = AC.I64_MIN, AC.I64_MAX
NULL = PC.NULL
CASES = PC.fuzz_cases()


def repeating_rows(rk):
    """How many build rows hold a key that another row holds too."""
    c = np.unique(rk, return_counts=True)[1]
    return int(c[c > 1].sum())


# ------------------------------------------------------------------ the fuzz list
@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_fuzz_case_size_caps(case):
    i, nr, ns, span, bits, wide = case
    d = PC.fuzz_relations(case)
    rk, rp, sk, sb, sv = d["rk"], d["rp"], d["sk"], d["sb"], d["sv"]
    assert len(rk) == len(rp) == nr and len(sk) == len(sb) == len(sv) == ns
    assert rk.dtype == sk.dtype == sb.dtype == (np.int64 if wide else np.int32)
    assert OC.Expect(rk, sk).m("outer") <= 2_500_000            # expand outer's M
    assert len(GC.expect(rk, rp, sk, sv, "all", NULL)["r"]) <= nr
    # the rank packing of asof_cases.expect: (key rank, value rank) in 32 bits each
    kr = np.unique(np.concatenate([rk, sk]).astype(np.int64), return_inverse=True)[1]
    vr = np.unique(np.concatenate([rp, sb.astype(np.int64)]), return_inverse=True)[1]
    assert kr.max() < (1 << 31) and vr.max() < (1 << 31)
    # neither the null value nor the sentinel is a payload
    assert not np.isin([NULL, PC.SENTINEL], rp).any()
    assert ((rk == I64_MIN).any(), (sk == I64_MIN).any()) == {
        None: (False, False), "both": (True, True), "probe": (False, True), "build": (True, False)}[d["null"]]


def test_fuzz_list_coverage():
    assert len(CASES) == 24 and [c[0] for c in CASES] == list(range(24))
    rel = [PC.fuzz_relations(c) for c in CASES]
    rep = [repeating_rows(d["rk"]) for d in rel]
    assert sum(r == 0 for r in rep) >= 3
    assert sum(r > c[1] // 2 for r, c in zip(rep, CASES)) >= 3
    modes = [d["null"] for d, c in zip(rel, CASES) if c[5]]
    assert all(d["null"] is None for d, c in zip(rel, CASES) if not c[5])
    assert modes.count("both") >= 2 and modes.count("probe") >= 1 and modes.count("build") >= 1
    for unit in (64, 1024, 4096, 8192):
        assert any(c[2] < unit for c in CASES) and any(c[2] > unit for c in CASES), unit
    for wide in (True, False):
        assert {PC.passes(c[4]) for c in CASES if c[5] == wide} == {1, 2, 3}, wide
    assert all(1 <= c[4] <= 24 for c in CASES)


# ------------------------------------------------------------------ the helpers against a nested loop
def tiny_relations():
    """Three relations of at most 200 rows: (rk, rp, sk, sb, sv), one with
    INT64_MIN on both sides, one with a key 20 times, one i32."""
    rng = np.random.default_rng(11)
    out = []
    rk = rng.integers(-40, 40, 150, dtype=np.int64)
    sk = rng.integers(-50, 50, 200, dtype=np.int64)
    rk[[3, 77, 149]] = I64_MIN
    sk[[0, 50, 199]] = I64_MIN
    out.append((rk, sk))
    rk = np.concatenate([rng.permutation(1000)[:100].astype(np.int64), np.full(20, 4242, np.int64)])
    rk = rk[rng.permutation(120)]
    sk = np.concatenate([rk[::3], np.full(7, 4242, np.int64), rng.integers(2000, 3000, 60, dtype=np.int64)])
    out.append((rk, sk[rng.permutation(len(sk))]))
    rk = rng.integers(-(1 << 31), -(1 << 31) + 60, 90, dtype=np.int64).astype(np.int32)
    sk = rng.integers(-(1 << 31), -(1 << 31) + 80, 130, dtype=np.int64).astype(np.int32)
    out.append((rk, sk))
    rels = []
    for n, (rk, sk) in enumerate(out):
        rp = AC.payloads(rk, n)
        sb = AC.bounds(rk, rp, sk, n)
        sv = GC.values(len(sk), n) if rk.dtype == np.int64 else np.arange(len(sk), dtype=np.int64)
        rels.append((rk, rp, sk, sb, sv))
    return rels


TINY = tiny_relations()


def partners(rk, rp, key):
    return [int(rp[i]) for i in range(len(rk)) if int(rk[i]) == int(key)]


def test_tiny_relations_shape():
    assert all(len(t[0]) <= 200 and len(t[2]) <= 200 for t in TINY)
    assert (TINY[0][0] == I64_MIN).sum() == 3 and (TINY[0][2] == I64_MIN).sum() == 3
    assert np.unique(TINY[1][0], return_counts=True)[1].max() == 20
    assert TINY[2][0].dtype == np.int32


@pytest.mark.parametrize("t", range(3))
def test_lookup_expect_is_the_definition(t):
    """out_r[j] = the smallest payload among the R rows with S's key, or null; cnt[j] = how many."""
    rk, rp, sk, _, _ = TINY[t]
    er, ec = PC.lookup_expect(rk, rp, sk)
    for j in range(len(sk)):
        p = partners(rk, rp, sk[j])
        assert int(ec[j]) == len(p), j
        assert int(er[j]) == (min(p) if p else NULL), j
    assert 0 < int((ec > 0).sum()) < len(sk) and int(ec.max()) > 1


@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("t", range(3))
def test_asof_expect_is_the_definition(t, kind):
    """BACKWARD: max {p in P(j): p <= b}; FORWARD: min {p: p >= b}; STRICT: < / >."""
    rk, rp, sk, sb, _ = TINY[t]
    er, found = AC.expect(rk, rp, sk, sb, kind, NULL)
    for j in range(len(sk)):
        b = int(sb[j])
        p = partners(rk, rp, sk[j])
        if kind == 0:
            q = [x for x in p if x <= b]
        elif kind == 1:
            q = [x for x in p if x >= b]
        elif kind == 2:
            q = [x for x in p if x < b]
        else:
            q = [x for x in p if x > b]
        assert bool(found[j]) == bool(q), j
        assert int(er[j]) == ((min(q) if kind & 1 else max(q)) if q else NULL), j
    assert 0 < int(found.sum()) < len(sk)


@pytest.mark.parametrize("how", XC.KINDS)
@pytest.mark.parametrize("t", range(3))
def test_expand_expect_is_the_definition(t, how):
    """w(j) = c(j) (outer: max(1, c(j))), off = its exclusive scan and M, the
    segment holds each partner's payload once (outer, no partner: the null)."""
    rk, rp, sk, _, _ = TINY[t]
    e = XC.ExpandExpect(rk, rp, sk, how, NULL)
    run = 0
    for j in range(len(sk)):
        p = partners(rk, rp, sk[j])
        seg = p if p or how == "inner" else [NULL]
        assert int(e.off[j]) == run and int(e.cnt[j]) == len(p), j
        assert sorted(e.r[run:run + len(seg)].tolist()) == sorted(seg), j
        assert (e.seg[run:run + len(seg)] == j).all()
        run += len(seg)
    assert int(e.off[len(sk)]) == run == e.m == len(e.r)
    assert e.unique == (len(set(rk.tolist())) == len(rk))
    # same_values: the expectation itself, in another order inside the segments, passes; a foreign value does not
    assert e.same_values(e.r)
    if not e.unique:
        assert e.same_values(e.r[np.lexsort((-e.r, e.seg))])
    bad = e.r.copy()
    bad[e.m // 2] += 1
    assert not e.same_values(bad)


@pytest.mark.parametrize("how", ["matched", "all"])
@pytest.mark.parametrize("t", range(3))
def test_group_expect_is_the_definition(t, how):
    """Per R row: count, wrapping sum, min and max of S's values over the rows with its key; sorted by payload."""
    rk, rp, sk, _, sv = TINY[t]
    e = GC.expect(rk, rp, sk, sv, how, NULL)
    rows = []
    for i in range(len(rk)):
        v = [int(sv[j]) for j in range(len(sk)) if int(sk[j]) == int(rk[i])]
        if not v and how == "matched":
            continue
        s = (sum(v) + (1 << 63)) % (1 << 64) - (1 << 63)   # two's-complement wrap
        rows.append((int(rp[i]), len(v), s, min(v) if v else NULL, max(v) if v else NULL))
    rows.sort()
    assert len(e["r"]) == len(rows)
    for c, col in enumerate(GC.COLS):
        assert e[col].tolist() == [r[c] for r in rows], col
    assert any(r[1] == 0 for r in rows) == (how == "all") and any(r[1] > 1 for r in rows)


# ------------------------------------------------------------------ the strided relation
@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("repeats", [True, False], ids=["repeats", "unique"])
def test_strided_positional_case(wide, repeats):
    c = PC.strided_positional_case(wide, repeats)
    rk, rp, sk, sb = c["rk"], c["rp"], c["sk"], c["sb"]
    ns = len(sk)
    # a table of exactly 64 KiB: rows x 2 rounded up to a power of two, 16 B (wide) or 8 B a slot
    assert c["slots"] == (4096 if wide else 8192) and c["slots"] * (16 if wide else 8) == 64 * 1024
    assert c["slots"] // 2 < 2 * len(rk) <= c["slots"]
    assert ns == PC.SEVERAL_NS == (1 << 21) + 2048 + 77 and -(-ns // PC.TILE) == 1026 and ns % PC.TILE == 77
    assert (repeating_rows(rk) > 0) == repeats and repeating_rows(rk) == (10 if repeats else 0)
    e = OC.Expect(rk, sk)
    assert np.array_equal(e.cnt, c["cnt"])
    assert int((e.cnt > 0).sum()) >= ns // 4 and int((e.cnt == 0).sum()) > ns // 2
    assert int((e.cnt > 1).sum()) == (40 if repeats else 0)
    assert not np.isin([NULL, PC.SENTINEL], rp).any() and len(np.unique(rp)) == len(rp)
    assert sb.dtype == sk.dtype
    # the truncating expand cap: inside a tile that every workgroup reaches in a later iteration only
    row = c["cut_row"]
    assert row // PC.TILE >= PC.CUT_TILE and e.cnt[row] == (2 if repeats else 1)
    x = XC.ExpandExpect(rk, rp, sk, "inner", NULL)
    cap = int(x.off[row]) + 1
    assert x.off[row] < cap <= x.off[row + 1] and cap < x.m and (cap < x.off[row + 1]) == repeats
    # under each non-strict kind the bound chooses: some rows with a partner find a candidate, some do not
    for kind in (0, 1):
        found = AC.expect(rk, rp, sk, sb, kind, NULL)[1]
        assert 0 < int(found.sum()) < int((e.cnt > 0).sum())
    if not wide:
        assert not (rk == np.iinfo(np.int32).min).any()
        return
    assert tuple(r // PC.TILE for r in PC.NULL_ROWS) == PC.NULL_TILES == (3, 519, 0, 512, 1025)
    assert np.flatnonzero(rk == I64_MIN).tolist() == [PC.SIDE_ROW]
    assert np.flatnonzero(sk == I64_MIN).tolist() == sorted(PC.NULL_ROWS)
    assert (e.cnt[list(PC.NULL_ROWS)] == 1).all()
    side = int(rp[PC.SIDE_ROW])
    at = sb[list(PC.NULL_ROWS)]
    assert (at < side).any() and (at == side).any() and (at > side).any()
    for kind in (0, 1):
        found = AC.expect(rk, rp, sk, sb, kind, NULL)[1][list(PC.NULL_ROWS)]
        assert 0 < int(found.sum()) < len(PC.NULL_ROWS), kind


# sha256 over the dtype names and bytes of several_tiles_case's nine host
# arrays, as the commit before the relation moved into positional_cases built them
PARENT_DIGESTS = {
    (True, None, True): "e72c60fd5f06550f1ace167ca2709ffa28633716770ae08c4a654b98ef85234d",
    (False, None, True): "8a015a83063d8f9889a6294dc4dfc1a6b58976fbc9c6a79399346fac79db207b",
    (True, 2, True): "3b4c4e891d148bb117cebcd5c01aa4408c1ad55dff22aff6e3ede9e8eddae477",
    (True, 2, False): "6fe3c583f2cb9200a0aa04a8f3fcc0cb617b53742fe171798adf8634851fb82a",
    (False, 2, True): "f78e894ab1050d7d9299b273fb4c9cd2292025ced8da36d39f991753b9d3fb11",
}


@pytest.mark.parametrize("wide,step,s_nulls", list(PARENT_DIGESTS))
def test_several_tiles_arrays_unchanged(wide, step, s_nulls):
    """The arrays test_gpu_small_table.py's users see (every argument set they
    pass) are byte for byte what they were before the move."""
    c = PC.several_tiles_arrays(wide, slice(None, None, step), s_nulls)
    h = hashlib.sha256()
    for k in ("rk", "rp", "sk", "sp", "cnt", "exp_r", "exp_s", "null_s_rows", "null_r_rows"):
        a = np.ascontiguousarray(c[k])
        h.update(str(a.dtype).encode())
        h.update(a.tobytes())
    assert h.hexdigest() == PARENT_DIGESTS[(wide, step, s_nulls)]
