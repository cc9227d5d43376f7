"""Case builders shared by the positional probes' strided-tile and ragged-fuzz
tests (lookup, as-of, expand; the fuzz adds group).  Pure numpy: no GPU and no
library call, so test_positional_cases.py checks every builder, and the
expectation helpers against a nested loop, on a CPU-only machine.

Expectations are asof_cases.expect, expand_cases.ExpandExpect,
group_cases.expect and lookup_expect below (the count column is
outer_cases.Expect(rk, sk).cnt, the payload column the minimum of R's payloads
over each key: sort by (key, payload), then searchsorted).  int64 payloads are
a seeded permutation around zero, times three plus one: NULL and SENTINEL are
multiples of three, so neither is a payload; i32 payloads are row ids."""
import functools

import numpy as np

import asof_cases as AC
import group_cases as GC
import outer_cases as OC

I64_MIN = OC.I64_MIN
TILE = OC.TILE
NULL, SENTINEL, EXTRA = -9, -12345, 64


def lookup_expect(rk, rp, sk, null=NULL):
    """(payload column, count column) numpy says the lookup of sk in (rk, rp) gives."""
    cnt = OC.Expect(rk, sk).cnt
    if len(rk) == 0:
        return np.full(len(sk), null, np.int64), cnt
    o = np.lexsort((rp, rk))
    lo = np.minimum(np.searchsorted(rk[o], sk, "left"), len(rk) - 1)
    return np.where(cnt > 0, rp[o][lo], null).astype(np.int64), cnt


# ------------------------------------------------------------------ strided LDS-table tiles
# 1026 tiles of 2048 rows, the last with 77: a 64-KiB table runs two
# workgroups per CU (512 on 256 CUs), so every workgroup strides over two
# tiles at least, workgroups 0 and 1 over three
SEVERAL_NS = (1 << 21) + 2048 + 77
# INT64_MIN probe keys: tile 3 (workgroup 3 hands on its first tile and keeps
# its second), tile 512 + 7 (workgroup 7: the reverse), tiles 0 and 512
# (workgroup 0 keeps only its third) and the ragged last tile
NULL_ROWS = (3 * 2048 + 5, (512 + 7) * 2048 + 100, 1, 512 * 2048 + 2047, 1025 * 2048 + 10)
NULL_TILES = (3, 512 + 7, 0, 512, 1025)
SIDE_ROW = 100   # the build row that holds INT64_MIN (wide)
CUT_TILE = 600   # the truncating expand cap lies in a tile no workgroup takes first


def several_tiles_arrays(wide, hits=slice(None), s_nulls=True, repeats=True):
    """Build and probe columns, and what numpy says they join to: a table of
    exactly 64 KiB with five repeated keys (wide: and one INT64_MIN key), a
    probe side a quarter of which hits it, forty rows of it a repeated key.
    hits: the slice of the plain build rows that the hits are drawn from (the
    rest, like four of the repeated keys, then have no partner in S);
    s_nulls=False leaves NULL_ROWS as misses, so S holds no INT64_MIN key;
    repeats=False: no build key twice (the forty rows then meet a plain key),
    as many rows, so the table keeps its slots."""
    nr, ns = (2048, SEVERAL_NS) if wide else (4096, SEVERAL_NS)
    dt, top = (np.int64, 1 << 40) if wide else (np.int32, 1 << 29)
    rng = np.random.default_rng(2048 if wide else 4096)
    rk = rng.permutation(np.unique(rng.integers(1, top, 2 * nr)))[:nr].astype(dt)
    assert len(rk) == nr
    if repeats:
        rk[nr - 5:] = rk[:5]                                # five keys twice
    plain = np.arange(5, nr - 5)                            # build rows whose key is neither repeated nor null
    if wide:
        rk[SIDE_ROW] = I64_MIN
        plain = plain[plain != SIDE_ROW]
    rp = np.arange(nr, dtype=np.int64) + (7000 if wide else 0)   # (i32: the row id)
    sk = rng.integers(2 * top, 4 * top - 1, ns).astype(dt)       # misses
    hit = rng.permutation(ns)[:ns // 4]
    sk[hit] = rk[rng.choice(plain[hits], len(hit))]         # a quarter of S hits R once
    sk[rng.permutation(ns)[:40]] = rk[0]                    # forty rows meet a repeated key
    if wide and s_nulls:
        sk[list(NULL_ROWS)] = I64_MIN
    sp = np.arange(ns, dtype=np.int64) + (1 << 32 if wide else 0)
    # sort + searchsorted: build rows lo[j] .. hi[j] of the sorted side match probe row j
    order = np.argsort(rk, kind="stable")
    lo, hi = np.searchsorted(rk[order], sk, "left"), np.searchsorted(rk[order], sk, "right")
    cnt = hi - lo
    first = np.cumsum(cnt) - cnt
    within = np.arange(int(cnt.sum())) - np.repeat(first, cnt)
    exp_r = rp[order[np.repeat(lo, cnt) + within]]
    exp_s = np.repeat(sp, cnt)
    assert int((cnt == 2).sum()) >= (40 if repeats else 0) and int((cnt > 0).sum()) >= ns // 4
    assert (len(np.unique(rk)) == nr) == (not repeats)
    # the rows without a partner: S's by the counts, R's by np.isin (every copy of a key no S row holds)
    r_un = ~np.isin(rk, sk)
    pairs, n_s, n_r = len(exp_r), int((cnt == 0).sum()), int(r_un.sum())
    assert pairs > 0 and n_s > 0 and n_r > (0 if hits == slice(None) else 1000)
    assert r_un[[1, 2, 3, 4]].all() and r_un[nr - 4:].all() and not r_un[0] and (not r_un[nr - 5]) == repeats
    return dict(rk=rk, rp=rp, sk=sk, sp=sp, cnt=cnt, exp_r=exp_r, exp_s=exp_s, null_s_rows=sp[cnt == 0],
                null_r_rows=rp[r_un])


@functools.lru_cache(maxsize=None)
def strided_positional_case(wide, repeats):
    """The relation of the strided-tile tests of lookup, as-of and expand:
    several_tiles_arrays' keys (a 64-KiB table, 1026 probe tiles, a quarter of
    S hits; wide: build row SIDE_ROW and the probe rows NULL_ROWS hold
    INT64_MIN), payloads as the positional tests make them, and an as-of bound
    column whose values at NULL_ROWS straddle the side row's payload.  cut_row
    is a probe row in a tile >= CUT_TILE with more than one partner (repeats=
    False: with one).  Built once per process; its arrays are never written."""
    c = several_tiles_arrays(wide, repeats=repeats)
    rk, sk = c["rk"], c["sk"]
    rp = AC.payloads(rk, 2048)
    sb = AC.bounds(rk, rp, sk, 4096 + repeats)
    if wide:
        side = int(rp[SIDE_ROW])
        # backward (p <= b) finds the side row from the second on but the fourth, forward (p >= b) the first, second and fourth
        sb[list(NULL_ROWS)] = [side - 1, side, side + 1, side - 2, side + 3]
    cnt = c["cnt"]
    rows = np.flatnonzero((np.arange(len(sk)) // TILE >= CUT_TILE) & (cnt > 1 if repeats else cnt == 1))
    assert len(rows) > 0
    slots = 1 << int(2 * len(rk) - 1).bit_length()          # 2 * rows rounded up to a power of two
    return dict(wide=wide, repeats=repeats, rk=rk, rp=rp, sk=sk, sb=sb, cnt=cnt, cut_row=int(rows[0]), slots=slots)


# ------------------------------------------------------------------ ragged fuzz
FUZZ_SEED = 0x90de   # chosen so that test_positional_cases.py's size caps and coverage conditions hold
FUZZ_UNITS = [1, 63, 64, 65, 511, 513, 1023, 1025, 4095, 4096, 4097, 8191, 8193, 12289, 40961]
FUZZ_BITS = [1, 4, 9, 12, 17, 19]           # 1, 1, 1, 2, 2 and 3 partition passes
NULL_MODES = ("both", "probe", "build")     # where every third wide case plants INT64_MIN


def passes(bits):
    return (bits + 8) // 9   # <= 9 bits per partition pass


def fuzz_cases():
    """Seeded sizes just around the kernels' units (64-row runs, 512/1024-row
    buckets, 4096-row pass tiles, 8192-row probe chunks), key ranges from
    every-key-repeats to nearly unique, both row widths, 1-3 pass plans:
    (i, nr, ns, span, bits, wide)."""
    rng = np.random.default_rng(FUZZ_SEED)
    cases = []
    for i in range(24):
        nr = int(rng.choice(FUZZ_UNITS)) + int(rng.integers(0, 3))
        ns = int(rng.choice(FUZZ_UNITS)) * int(rng.integers(1, 4))
        span = int(rng.choice([3, 64, 1000, 1 << 20, 1 << 40]))
        span = max(span, nr * ns // 2_000_000 + 1)   # at most ~2M result rows
        bits = int(rng.choice(FUZZ_BITS))
        wide = bool(i % 3)
        cases.append((i, nr, ns, span if wide else min(span, 1 << 30), bits, wide))
    return cases


def null_mode(case):
    """Where the case holds INT64_MIN: 'both', 'probe' (S only: the side list
    is empty), 'build', or None -- every third wide case, the modes in turn."""
    i, wide = case[0], case[5]
    j = i - i // 3 - 1   # the case's place among the wide ones (i % 3 != 0)
    return NULL_MODES[(j // 3) % 3] if wide and j % 3 == 0 else None


def _fuzz_keys(rng, lo, span, nr, ns):
    # ~70 % of S rows take a key drawn from R (sparse spans still match)
    rk = rng.integers(lo, lo + span, nr, dtype=np.int64)
    sk = rng.integers(lo, lo + span, ns, dtype=np.int64)
    hit = rng.random(ns) < 0.7
    sk[hit] = rk[rng.integers(0, nr, int(hit.sum()))]
    return rk, sk


def fuzz_relations(case):
    """The case's columns: rk, rp (R's keys and payloads), sk (S's keys), sb
    (as-of bounds, in sk's dtype), sv (group values: int64 the whole range,
    i32 the row ids), and null: null_mode(case)."""
    i, nr, ns, span, bits, wide = case
    rng = np.random.default_rng(7000 + i)
    rk, sk = _fuzz_keys(rng, -span // 2, span, nr, ns)
    mode = null_mode(case)
    if mode in ("both", "build"):
        rk[rng.integers(0, nr, 3)] = I64_MIN
    if mode in ("both", "probe"):
        sk[rng.integers(0, ns, 9)] = I64_MIN
    if not wide:
        rk, sk = rk.astype(np.int32), sk.astype(np.int32)
    rp = AC.payloads(rk, 100 + i)
    sb = AC.bounds(rk, rp, sk, 200 + i)
    sv = GC.values(ns, 300 + i) if wide else np.arange(ns, dtype=np.int64)
    return dict(rk=rk, rp=rp, sk=sk, sb=sb, sv=sv, null=mode)
