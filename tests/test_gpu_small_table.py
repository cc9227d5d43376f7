"""Global tables small enough to live in LDS (k_probe<..., LDS>, tables of
<= 64 KiB: int64 builds of <= 2048 rows, i32 builds of <= 4096 rows) against
the oracle: unique and repeated build keys, INT64_MIN probe keys (their
tiles take the general path), count-only, i32 reference types, and the sizes
either side of the LDS limit.  The inner, exists, outer and full probes also
run with more tiles than workgroups (several_tiles_case); the positional
probes (lookup, as-of, expand) do so in test_gpu_positional_tiles.py."""
import numpy as np
import pytest
import torch

import positional_cases as PC
from hashjoin import HashJoin
from join_gpu import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hj():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    h = HashJoin(0)
    h.set_strategy("global")
    yield h
    h.close()


def join(hj, rk, rp, sk, sp):
    if rk.dtype == np.int32:
        o_r, o_s = hj.join(dev(rk), None, dev(sk), None)
    else:
        o_r, o_s = hj.join(dev(rk), dev(rp), dev(sk), dev(sp))
    torch.cuda.synchronize()
    assert hj.strategy_used == "global"
    return o_r.cpu().numpy().astype(np.int64), o_s.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("nr", [1, 100, 1000, 1024, 2048, 3000])   # 3000: 8192 slots, past the LDS limit
def test_small_table_pkfk(hj, oracle, nr):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(nr, nr, 1 << 20, 0.8)
    o = join(hj, rk, rp, sk, sp)
    assert oracle.same_multiset(*o, *oracle.chained_join_i64(rk, rp, sk, sp, H=max(1, nr // 4)))


def test_small_table_repeated_build_keys(hj, oracle):
    rk, rp = oracle.gen_uniform_i64(61, 1, 1, 300, 1000)
    sk, sp = oracle.gen_uniform_i64(61, 2, 1, 400, 1 << 18)
    o = join(hj, rk, rp, sk, sp)
    assert oracle.same_multiset(*o, *oracle.chained_join_i64(rk, rp, sk, sp, H=100))


def test_small_table_int64_min_probe_keys(hj, oracle):
    I64_MIN = -(1 << 63)
    rk, rp, sk, sp = oracle.gen_pkfk_i64(62, 1500, 1 << 19, 0.9)
    rk[::211] = I64_MIN
    sk[::1777] = I64_MIN
    o = join(hj, rk, rp, sk, sp)
    assert oracle.same_multiset(*o, *oracle.nested_loop_i64(rk, rp, sk[:1 << 19], sp[:1 << 19]))


def test_small_table_count_only(hj, oracle):
    rk, rp, sk, sp = oracle.gen_pkfk_i64(63, 700, 1 << 20, 0.6)
    hj.build_table(dev(rk), dev(rp))
    er, _ = oracle.chained_join_i64(rk, rp, sk, sp, H=100)
    assert hj.count_rows(dev(sk)) == len(er)


@pytest.mark.parametrize("nr", [1000, 4000, 5000])   # i32: 8192 slots x 8 B = 64 KiB; 5000: past it
def test_small_table_i32(hj, oracle, nr):
    r = oracle.gen_uniform_i32(64, 1, 1, 1 << 20, nr)
    s = oracle.gen_uniform_i32(64, 2, 1, 1 << 20, 1 << 20)
    o = join(hj, r, None, s, None)
    assert oracle.same_multiset(*o, *oracle.chained_join_i32(r, s, H=max(1, nr // 4)))


I64_MIN = PC.I64_MIN
# 1026 tiles of 2048 rows, the last with 77, and the rows of S that hold
# INT64_MIN: see positional_cases, which builds the relation
SEVERAL_NS, NULL_ROWS = PC.SEVERAL_NS, PC.NULL_ROWS


def several_tiles_case(wide, hits=slice(None), s_nulls=True):
    """positional_cases.several_tiles_arrays (a table of exactly 64 KiB, a
    probe side of 1026 tiles a quarter of which hits it, and what numpy says
    they join to) with its four columns on the device as well."""
    c = PC.several_tiles_arrays(wide, hits, s_nulls)
    return dict(c, d_rk=dev(c["rk"]), d_rp=dev(c["rp"]) if wide else None, d_sk=dev(c["sk"]),
                d_sp=dev(c["sp"]) if wide else None)


@pytest.fixture(scope="module")
def several_i64():
    return several_tiles_case(True)


def sorted_pairs(a, b):
    o = np.lexsort((b, a))
    return np.stack([a[o], b[o]])


def inner_pairs(hj, c):
    """The join of case c through probe_relation, outputs sized M + 64."""
    wide = c["rk"].dtype == np.int64
    hj.build_table(c["d_rk"], c["d_rp"])
    m = len(c["exp_r"])
    o_r = torch.full((m + 64,), -7, dtype=torch.int64 if wide else torch.int32, device="cuda")
    o_s = torch.full_like(o_r, -7)
    got = int(hj.probe_relation(c["d_sk"], c["d_sp"], o_r, o_s).item())
    assert hj.strategy_used == "global"
    assert got == m
    return o_r[:m].cpu().numpy().astype(np.int64), o_s[:m].cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("kind", ["inner", "count", "semi", "anti"])
def test_workgroups_take_several_tiles(hj, several_i64, kind):
    """k_probe's / k_probe_exists's grid-stride loop with more than one tile
    per workgroup, some of them handed to the general path (NULL_ROWS, the
    forty rows that meet a repeated key): exact count, exact rows."""
    c = several_i64
    if kind == "inner":
        g_r, g_s = inner_pairs(hj, c)
        assert np.array_equal(sorted_pairs(g_r, g_s), sorted_pairs(c["exp_r"], c["exp_s"]))
        return
    hj.build_table(c["d_rk"], c["d_rp"])
    if kind == "count":
        assert hj.count_rows(c["d_sk"]) == len(c["exp_r"])
        assert hj.strategy_used == "global"
        return
    keep = c["cnt"] > 0 if kind == "semi" else c["cnt"] == 0
    m = int(keep.sum())
    o_s = torch.full((len(c["sk"]),), -7, dtype=torch.int64, device="cuda")
    o_k = torch.full_like(o_s, -7)
    got = int(hj.probe_exists(c["d_sk"], c["d_sp"], kind, o_s, o_k).item())
    assert hj.strategy_used == "global"
    assert got == m
    assert np.array_equal(sorted_pairs(o_k[:m].cpu().numpy(), o_s[:m].cpu().numpy()),
                          sorted_pairs(c["sk"][keep], c["sp"][keep]))
    assert hj.count_exists(c["d_sk"], kind) == m


def test_workgroups_take_several_tiles_i32(hj):
    """The same shape for the i32 types: 4096 build rows, 8192 slots x 8 B = 64 KiB."""
    c = several_tiles_case(False)
    g_r, g_s = inner_pairs(hj, c)
    assert np.array_equal(sorted_pairs(g_r, g_s), sorted_pairs(c["exp_r"], c["exp_s"]))


HALF = slice(None, None, 2)   # hits drawn from every second plain build row: a thousand R rows keep no partner
NULL_R, NULL_S, SENTINEL = -1, -2, -7   # payloads are >= 0 (i32: row ids)
OUTER_KINDS = ["outer", "outer-count", "full", "build", "full-count", "build-count"]


@pytest.fixture(scope="module")
def several_i64_half():
    return several_tiles_case(True, HALF)


def assert_strides(c):
    """More tiles than two workgroups per CU: every workgroup of the LDS-table
    probes takes a second tile (on a part with more CUs this must fail, not pass unstrided)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-len(c["sk"]) // 2048) > 2 * cus, (len(c["sk"]), cus)


def outer_expected(c, kind):
    """The rows of kind outer / full / build: the pairs, (NULL_R, S.pay) of the
    S rows without a partner, (R.pay, NULL_S) of the R rows without one."""
    r, s = [c["exp_r"]], [c["exp_s"]]
    if kind in ("outer", "full"):
        r.append(np.full(len(c["null_s_rows"]), NULL_R, np.int64))
        s.append(c["null_s_rows"])
    if kind in ("full", "build"):
        r.append(c["null_r_rows"])
        s.append(np.full(len(c["null_r_rows"]), NULL_S, np.int64))
    return np.concatenate(r), np.concatenate(s)


def outer_probe(hj, c, kind, m):
    """Probe kind of the current build into outputs of m + 64 sentinel rows:
    exact M, and the 64 rows past it untouched."""
    dt = torch.int64 if c["rk"].dtype == np.int64 else torch.int32
    o_r = torch.full((m + 64,), SENTINEL, dtype=dt, device="cuda")
    o_s = torch.full_like(o_r, SENTINEL)
    if kind == "outer":
        cnt = hj.probe_outer(c["d_sk"], c["d_sp"], o_r, o_s, null=NULL_R)
    else:
        cnt = hj.probe_full(c["d_sk"], c["d_sp"], o_r, o_s, kind=kind, null_r=NULL_R, null_s=NULL_S)
    got = int(cnt.item())
    assert hj.strategy_used == "global"
    assert got == m
    g_r, g_s = o_r.cpu().numpy().astype(np.int64), o_s.cpu().numpy().astype(np.int64)
    assert (g_r[m:] == SENTINEL).all() and (g_s[m:] == SENTINEL).all()
    return g_r[:m], g_s[:m]


def check_outer_kind(hj, c, kind):
    assert_strides(c)
    assert min(c["rp"].min(), c["sp"].min()) >= 0   # no payload is a null value or the sentinel
    hj.build_table(c["d_rk"], c["d_rp"])
    base = kind.split("-")[0]
    e_r, e_s = outer_expected(c, base)
    if kind.endswith("-count"):
        got = hj.count_outer(c["d_sk"]) if base == "outer" else hj.count_full(c["d_sk"], kind=base)
        assert hj.strategy_used == "global"
        assert got == len(e_r)
        return None
    g_r, g_s = outer_probe(hj, c, base, len(e_r))
    assert np.array_equal(sorted_pairs(g_r, g_s), sorted_pairs(e_r, e_s))
    return g_r, g_s


@pytest.mark.parametrize("kind", OUTER_KINDS)
@pytest.mark.parametrize("hits", ["all", "half"])
def test_workgroups_take_several_tiles_outer(hj, several_i64, several_i64_half, hits, kind):
    """k_probe_outer<LDS> (outer, full) and k_probe<LDS, MARKS> (build) with
    more than one tile per workgroup, some tiles handed to the general path
    between tiles that stay, then k_probe_mark and k_emit_unmatched: exact M,
    exact rows, nothing written past M.  half: a thousand build rows, and both
    copies of four repeated keys, come out as R's null rows."""
    check_outer_kind(hj, several_i64 if hits == "all" else several_i64_half, kind)


def test_side_list_row_without_partner(hj):
    """S holds no INT64_MIN key: build row 100 (INT64_MIN, the side list's only
    row) comes out once, as (rp[100], NULL_S), behind workgroup 0's tiles."""
    c = several_tiles_case(True, HALF, s_nulls=False)
    assert c["rk"][100] == I64_MIN and not (c["sk"] == I64_MIN).any()
    assert np.isin(c["rp"][100], c["null_r_rows"])
    g_r, g_s = check_outer_kind(hj, c, "full")
    assert g_s[g_r == c["rp"][100]].tolist() == [NULL_S]


@pytest.mark.parametrize("kind", ["outer", "full"])
def test_workgroups_take_several_tiles_outer_i32(hj, kind):
    """The same for the i32 types (4096 build rows, row ids for payloads)."""
    check_outer_kind(hj, several_tiles_case(False, HALF), kind)


@pytest.mark.parametrize("nr,wide", [(1500, True), (4000, True), (3000, False), (20000, False)])
def test_few_repeated_build_keys(hj, oracle, nr, wide):
    """A handful of repeated build keys: only the tiles whose rows meet one go
    to the general path (every other tile keeps the fast path) -- exact."""
    rng = np.random.default_rng(nr)
    if wide:
        rk, rp = oracle.gen_uniform_i64(nr, 1, 1, 1 << 40, nr)
        rk[nr - 5:] = rk[:5]                      # five keys twice
        sk, sp = oracle.gen_uniform_i64(nr, 2, 1, 1 << 40, 1 << 20)
        idx = rng.integers(0, nr, 1 << 18)
        sk[:1 << 18] = rk[idx]                    # a quarter of S hits R
        sk[rng.integers(0, 1 << 20, 40)] = rk[0]  # forty rows meet a repeated key
        o = join(hj, rk, rp, sk, sp)
        assert oracle.same_multiset(*o, *oracle.chained_join_i64(rk, rp, sk, sp, H=max(1, nr // 4)))
    else:
        r = oracle.gen_uniform_i32(nr, 1, 1, 1 << 30, nr)
        r[nr - 5:] = r[:5]
        s = oracle.gen_uniform_i32(nr, 2, 1, 1 << 30, 1 << 20)
        s[:1 << 18] = r[rng.integers(0, nr, 1 << 18)]
        s[rng.integers(0, 1 << 20, 40)] = r[0]
        o = join(hj, r, None, s, None)
        assert oracle.same_multiset(*o, *oracle.chained_join_i32(r, s, H=max(1, nr // 4)))
