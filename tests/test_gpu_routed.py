"""The multi-source routed build and probe (hj_dev_build_routed_i64 /
hj_dev_probe_routed_i64 with nsrc > 1) on one GPU.

routed_layout.folded_join emulates N ranks' folded exchange: N sender slices
of uneven sizes (one empty, one of a single row) are routed with
hj_dev_route_i64, every owner's receive buffers are assembled source by
source with their (N, bins) count matrices -- the layout
hashjoin/dist.py::RoutedExchange delivers and include/hj.h documents -- and
joined with the routed build / probe.  The union over all owners and parts
must be the oracle's join of the global relations, exactly.  Every buffer is
first held against routed_layout.check_layout, the statement the CPU stand-in
asserts on the product's exchange (test_routed_layout.py, test_dist_gloo.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import routed_layout as RL
from hashjoin import HashJoin
from hashjoin._lib import HJ_ERR_ARG, HJ_JOIN_KERNEL_EXISTS, lib

pytestmark = pytest.mark.gpu

INT64_MIN = -(1 << 63)
SENTINEL = 0x5A5A5A5A5A5A5A5A
# (senders = owners, bin bits per owner, S bin ranges); (8, 6, 2) is the N = 8 product plan
SHAPES = [(2, 4, 1), (4, 3, 3), (8, 1, 1), (16, 5, 4), (64, 3, 2), (8, 6, 2)]
RUN_UNITS = [0, 1, 63, 64, 65, 129]   # rows of one (sender, part): around the 64-row run unit
EXISTS = HashJoin.JOIN_KERNELS[HJ_JOIN_KERNEL_EXISTS]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def hj():
    h = HashJoin(0)
    yield h
    h.close()


def _make(oracle, kind):
    if kind == "grouped":   # keys in [1, 900] on both sides: most build keys repeat
        rk, rp = oracle.gen_uniform_i64(301, 1, 1, 900, 40000)
        sk, sp = oracle.gen_uniform_i64(301, 2, 1, 900, 60000)
        return rk, rp, sk, sp
    rk, rp, sk, sp = oracle.gen_pkfk_i64(300, 40000, 60000, 0.85)
    if kind == "skew":      # 30 % of S on one key: one (owner, bin) is huge from every sender
        sk = sk.copy()
        sk[np.random.default_rng(302).random(len(sk)) < 0.3] = rk[123]
    if kind == "int64_min":
        rk, sk = rk.copy(), sk.copy()
        rk[[5, 17000, 39999]] = INT64_MIN   # from three different senders
        sk[::500] = INT64_MIN
    return rk, rp, sk, sp


@pytest.fixture(scope="module")
def relations(oracle):
    """kind -> (host columns, device columns, expected pairs): generated and
    joined by the oracle once, shared by every shape, never modified."""
    out = {}
    for kind in ("pkfk", "grouped", "skew", "int64_min"):
        cols = _make(oracle, kind)
        dev = tuple(_dev(a) for a in cols)
        for a in cols:
            a.setflags(write=False)
        out[kind] = (cols, dev, oracle.chained_join_i64(*cols))
    return out


@pytest.mark.parametrize("kind", ["pkfk", "grouped", "skew", "int64_min"])
@pytest.mark.parametrize("N,sub,s_parts", SHAPES)
def test_multi_source_vs_oracle(hj, oracle, relations, N, sub, s_parts, kind):
    (rk, rp, sk, sp), dev, exp = relations[kind]
    if kind == "skew":
        assert 0.28 < (sk == rk[123]).mean() < 0.33
    outs = RL.folded_join(hj, *dev, N, sub, s_parts)
    got_r, got_s = RL.union(outs)
    print(f"{kind} N={N} sub={sub} parts={s_parts}: M = {len(got_r)}, oracle {len(exp[0])}")
    assert oracle.same_multiset(got_r, got_s, *exp)
    # every pair came out of the owner of its key (payloads are global row ids)
    g = N.bit_length() - 1
    for q, (o_r, o_s) in enumerate(outs):
        assert (RL.rparts(sk[o_s.cpu().numpy()], g) == q).all()
        assert (RL.rparts(rk[o_r.cpu().numpy()], g) == q).all()


def _keys_by_part(bits, per_part, seed):
    """per_part distinct keys of every one of the 2^bits parts (the numpy
    restatement classifies a pool of random keys)."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(INT64_MIN, (1 << 63) - 1, (per_part << bits) * 4, dtype=np.int64))
    rng.shuffle(pool)
    part = RL.rparts(pool, bits)
    by = [pool[part == p][:per_part] for p in range(1 << bits)]
    assert all(len(k) == per_part for k in by)
    return by


def _planned(N, sub, rows_of, seed, hit=0.5):
    """Global R and S in which sender s holds exactly rows_of(s, p) rows of
    part p, on both sides; S keys are partly R keys of the same part (any
    sender's), partly keys R does not hold.  Returns the columns, the sender
    bounds and the (N, parts) plan."""
    g = N.bit_length() - 1
    P = N << sub
    plan = np.array([[rows_of(s, p) for p in range(P)] for s in range(N)], np.int64)
    per = int(plan.sum(0).max())
    by = _keys_by_part(g + sub, 2 * per + 2, seed)
    rng = np.random.default_rng(seed + 1)
    r_rows, s_rows = [], []
    used = np.zeros(P, np.int64)
    for s in range(N):
        rs, ss = [], []
        for p in range(P):
            c = int(plan[s, p])
            rs.append(by[p][used[p]:used[p] + c])
            used[p] += c
        r_rows.append(rng.permutation(np.concatenate(rs)))
        s_rows.append(ss)
    for s in range(N):
        for p in range(P):
            c = int(plan[s, p])
            nr = int(plan[:, p].sum())
            h = int(round(c * hit)) if nr else 0
            hits = rng.choice(by[p][:nr], h) if h else np.zeros(0, np.int64)
            misses = rng.choice(by[p][nr:], c - h)
            s_rows[s].append(np.concatenate([hits, misses]))
        s_rows[s] = rng.permutation(np.concatenate(s_rows[s]))
    bounds = np.concatenate([[0], np.cumsum(plan.sum(1))]).tolist()
    rk, sk = np.concatenate(r_rows), np.concatenate(s_rows)
    return rk, np.arange(len(rk), dtype=np.int64), sk, np.arange(len(sk), dtype=np.int64), bounds, plan


def _assert_plan(hj, key, pay, N, sub, bounds, plan):
    """hj_dev_route_i64 counted every sender's parts as planned."""
    R = RL.Routed(hj, _dev(key), _dev(pay), N, sub, bounds)
    for s in range(N):
        assert R.counts[s].cpu().tolist() == plan[s].tolist()


def test_run_unit_counts(hj, oracle):
    """(sender s, part p) holds exactly [0, 1, 63, 64, 65, 129][(s + p) % 6]
    rows on both sides: every run count around the 64-row unit in every
    position of the source loop."""
    N, sub = 8, 2
    rk, rp, sk, sp, bounds, plan = _planned(N, sub, lambda s, p: RUN_UNITS[(s + p) % 6], 310)
    _assert_plan(hj, rk, rp, N, sub, bounds, plan)
    _assert_plan(hj, sk, sp, N, sub, bounds, plan)
    for s_parts in (1, 3):
        outs = RL.folded_join(hj, _dev(rk), _dev(rp), _dev(sk), _dev(sp), N, sub, s_parts, bounds, bounds)
        assert oracle.same_multiset(*RL.union(outs), *oracle.nested_loop_i64(rk, rp, sk, sp))


def test_sparse_even_64_sources(oracle):
    """64 sources x 8 bins with 8 rows in each of one owner's 512 (source,
    bin) pairs, 4096 R x 4096 S rows, on a fresh context (the workspace is
    sized by these calls alone): 512 runs of 8 rows, where rows / 64 is 64.

    Before the run lists were sized for rows / 64 + nsrc * bins runs the
    listing dropped the runs past the ping set's 391 entries: d_count came
    back 2309 for the oracle's 3072, with bit 63 clear."""
    N, sub, q = 64, 3, 37
    F = 1 << sub
    rows_of = lambda s, p: 8 if p // F == q else 0  # noqa: E731
    rk, rp, sk, sp, bounds, plan = _planned(N, sub, rows_of, 320, hit=0.75)
    assert len(rk) == 4096 and len(sk) == 4096
    exp = oracle.nested_loop_i64(rk, rp, sk, sp)
    assert len(exp[0]) == 4096 * 3 // 4
    h = HashJoin(0)
    try:
        R = RL.Routed(h, _dev(rk), _dev(rp), N, sub, bounds)
        S = RL.Routed(h, _dev(sk), _dev(sp), N, sub, bounds)
        t, c = R.received(q)
        assert t.shape[0] == 4096 and (c == 8).all() and c.shape == (64, 8)
        RL.check_layout(t.cpu().numpy(), c.cpu().numpy(), 0, N, sub, q)
        h.build_routed(t, c, N, sub)
        ts, cs = S.received(q)
        RL.check_layout(ts.cpu().numpy(), cs.cpu().numpy(), 0, N, sub, q)
        o_r = torch.empty(4096, dtype=torch.int64, device="cuda"); o_s = torch.empty_like(o_r)
        m = int(h.probe_routed(ts, cs, 0, o_r, o_s).item())
        print(f"sparse 64 x 8 x 8: d_count = {m} ({m & ((1 << 63) - 1)} rows, bit 63 {'set' if m < 0 else 'clear'})"
              f", oracle M = {len(exp[0])}")
        assert m == len(exp[0])
        assert oracle.same_multiset(o_r[:m].cpu().numpy(), o_s[:m].cpu().numpy(), *exp)
    finally:
        h.close()


def test_sparse_300_by_500(oracle):
    """300 R x 500 S rows over 64 senders and 512 parts, on a fresh context:
    most (source, bin) counts are 0 or 1 and some owners receive nothing."""
    rk, rp, sk, sp = oracle.gen_pkfk_i64(330, 300, 500, 0.85)
    h = HashJoin(0)
    try:
        outs = RL.folded_join(h, _dev(rk), _dev(rp), _dev(sk), _dev(sp), 64, 3, 2)
    finally:
        h.close()
    assert oracle.same_multiset(*RL.union(outs), *oracle.nested_loop_i64(rk, rp, sk, sp))


def _one_owner(hj, rk, rp, sk, sp, N, sub, q):
    """Owner q's routed build; returns the routed S and the owner's rows of
    the global relations (host masks)."""
    R = RL.Routed(hj, _dev(rk), _dev(rp), N, sub)
    S = RL.Routed(hj, _dev(sk), _dev(sp), N, sub)
    t, c = R.received(q)
    RL.check_layout(t.cpu().numpy(), c.cpu().numpy(), 0, N, sub, q)
    hj.build_routed(t, c, N, sub)
    g = N.bit_length() - 1
    return S, RL.rparts(rk, g) == q, RL.rparts(sk, g) == q


@pytest.mark.parametrize("dups", [False, True])
def test_repeat_across_sources(hj, oracle, dups):
    """One build key whose two copies arrive from different senders, met by
    no probe row: has_duplicates() after routed probes in 2 bin ranges is
    true, and false without the repeat (test_folded_duplicates_after_parts
    with nsrc = 4)."""
    N, sub = 4, 3
    rk, rp, sk, sp = oracle.gen_pkfk_i64(340, 40000, 30000, 0.9)
    b = RL.slice_bounds(len(rk), N)
    i, j = b[0] + 7, b[2] + 11          # rows of senders 0 and 2
    assert b[0] <= i < b[1] and b[2] <= j < b[3]
    if dups:
        rk = rk.copy()
        rk[j] = rk[i]
    keep = sk != rk[i]
    sk, sp = sk[keep], sp[keep]
    q = int(RL.rparts(rk[i:i + 1], N.bit_length() - 1)[0])
    S, own_r, own_s = _one_owner(hj, rk, rp, sk, sp, N, sub, q)
    F = 1 << sub
    rs, ss = [], []
    for b0, b1 in ((0, F // 2), (F // 2, F)):
        ts, cs = S.received(q, b0, b1)
        o = RL.probe_exact(lambda o_r, o_s: hj.probe_routed(ts, cs, b0, o_r, o_s), ts.shape[0], ts.device)
        rs.append(o[0].cpu().numpy()); ss.append(o[1].cpu().numpy())
    exp = oracle.chained_join_i64(rk[own_r], rp[own_r], sk[own_s], sp[own_s])
    assert oracle.same_multiset(np.concatenate(rs), np.concatenate(ss), *exp)
    assert hj.has_duplicates() == dups


def test_capacity_below_m(hj, oracle):
    """out_cap below M through views of a sentinel-filled buffer: d_count is
    M exactly, nothing is written at or past out_cap (nor before the view),
    and the rows written are distinct true pairs."""
    N, sub, q = 4, 3, 2
    rk, rp, sk, sp = oracle.gen_pkfk_i64(350, 40000, 60000, 0.85)
    S, own_r, own_s = _one_owner(hj, rk, rp, sk, sp, N, sub, q)
    exp = oracle.chained_join_i64(rk[own_r], rp[own_r], sk[own_s], sp[own_s])
    M = len(exp[0])
    cap, G = M // 2 + 1, 64        # (odd row offset below: the views are 8 B off a 16-B boundary)
    ts, cs = S.received(q)
    bufs = [torch.full((G + 1 + M + G,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2)]
    views = [b[G + 1:G + 1 + cap] for b in bufs]
    m = int(hj.probe_routed(ts, cs, 0, views[0], views[1]).item())
    assert m == M
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert (h[:G + 1] == SENTINEL).all() and (h[G + 1 + cap:] == SENTINEL).all()
    got = oracle.sorted_pairs(host[0][G + 1:G + 1 + cap], host[1][G + 1:G + 1 + cap])
    want = oracle.sorted_pairs(*exp)
    # payloads are row ids, so true pairs are distinct: got is a duplicate-free subset of want
    assert len(np.unique(got, axis=0)) == cap
    both = np.concatenate([got, want])
    assert len(np.unique(both, axis=0)) == M


def _reported(h):
    """What the context says of its last probe: (join kernel, strategy)."""
    return h.join_kernel, h.strategy_used


def _alone(build, probe):
    """_reported of a fresh context after build(h) followed directly by probe(h)."""
    h = HashJoin(0)
    try:
        build(h)
        probe(h)
        return _reported(h)
    finally:
        h.close()


def test_unrouted_probes_after_routed_build(hj, oracle):
    """After a routed build the ordinary probes are valid too (hj.h): this
    owner's S rows, unrouted, through hj_dev_probe_tuples_i64 and the semi-
    and anti-join hj_dev_exists_tuples_i64 give the oracle's join / np.isin.
    hj_ctx_join_kernel names the last probe's kernel throughout: the exists
    kernel after each exists probe, and after the closing routed probe what a
    fresh context reports for that build and probe alone."""
    N, sub, q = 4, 3, 1
    rk, rp, sk, sp = oracle.gen_pkfk_i64(360, 40000, 60000, 0.6)
    rk = rk.copy(); sk = sk.copy()
    rk[3] = rk[30000]                       # a repeated build key, from two senders
    sk[::700] = rk[3]
    _, own_r, own_s = _one_owner(hj, rk, rp, sk, sp, N, sub, q)
    if not own_r[3]:                        # (keep the repeat on this owner)
        q = int(RL.rparts(rk[3:4], N.bit_length() - 1)[0])
        _, own_r, own_s = _one_owner(hj, rk, rp, sk, sp, N, sub, q)
    mine = np.stack([sk[own_s], sp[own_s]], axis=1)
    t = _dev(mine)
    o_r, o_s = RL.probe_exact(lambda a, b: hj.probe_tuples(t, a, b), t.shape[0], t.device)
    exp = oracle.chained_join_i64(rk[own_r], rp[own_r], mine[:, 0], mine[:, 1])
    assert oracle.same_multiset(o_r.cpu().numpy(), o_s.cpu().numpy(), *exp)
    assert hj.count_rows(_dev(mine[:, 0])) == len(exp[0])      # (hj_dev_count_i64: the column form)
    hit = np.isin(mine[:, 0], rk[own_r])
    assert 0 < hit.sum() < len(hit)
    for kind, want in (("semi", mine[hit]), ("anti", mine[~hit])):
        out_s = torch.empty(max(1, len(mine)), dtype=torch.int64, device="cuda")
        out_k = torch.empty_like(out_s)
        m = int(hj.probe_exists_tuples(t, kind, out_s, out_k).item())
        assert m == len(want)
        assert hj.join_kernel == EXISTS
        got = oracle.sorted_pairs(out_k[:m].cpu().numpy(), out_s[:m].cpu().numpy())
        assert np.array_equal(got, oracle.sorted_pairs(want[:, 0], want[:, 1]))
    # and the routed probe still joins after them
    S = RL.Routed(hj, _dev(sk), _dev(sp), N, sub)
    ts, cs = S.received(q)
    o = RL.probe_exact(lambda a, b: hj.probe_routed(ts, cs, 0, a, b), ts.shape[0], ts.device)
    assert oracle.same_multiset(o[0].cpu().numpy(), o[1].cpu().numpy(), *exp)
    last = _reported(hj)
    assert last[0] != EXISTS
    tr, cr = RL.Routed(hj, _dev(rk), _dev(rp), N, sub).received(q)
    fresh = _alone(lambda h: h.build_routed(tr, cr, N, sub),
                   lambda h: RL.probe_exact(lambda a, b: h.probe_routed(ts, cs, 0, a, b), ts.shape[0], ts.device))
    assert fresh[0] is not None
    assert last == fresh


def test_last_probe_is_reported_through_mixed_probes(hj, oracle, relations):
    """One routed build, then routed inner, semi, tuple, anti, count and routed
    inner probes in that order, then a semi probe with a routed inner probe
    directly behind it (the one order in which no other entry point runs
    between an exists probe and a routed one): every call returns the oracle's
    count (np.isin for semi / anti), and join_kernel / strategy_used name that
    call's kernel: the exists kernel for semi / anti, for an inner probe what
    a fresh context reports after the same build followed by that probe alone."""
    N, sub, q = 4, 3, 1
    (rk, rp, sk, sp), dev, _ = relations["pkfk"]
    tr, cr = RL.Routed(hj, dev[0], dev[1], N, sub).received(q)
    ts, cs = RL.Routed(hj, dev[2], dev[3], N, sub).received(q)
    g = N.bit_length() - 1
    own_r, own_s = RL.rparts(rk, g) == q, RL.rparts(sk, g) == q
    mine = np.stack([sk[own_s], sp[own_s]], axis=1)
    t, col = _dev(mine), _dev(mine[:, 0])
    M = len(oracle.chained_join_i64(rk[own_r], rp[own_r], mine[:, 0], mine[:, 1])[0])
    hit = int(np.isin(mine[:, 0], rk[own_r]).sum())
    assert 0 < hit < len(mine) and ts.shape[0] == len(mine)

    def build(h):
        h.build_routed(tr, cr, N, sub)

    def routed(h):
        return RL.probe_exact(lambda a, b: h.probe_routed(ts, cs, 0, a, b), len(mine), t.device)[0].shape[0]

    def tuples(h):
        return RL.probe_exact(lambda a, b: h.probe_tuples(t, a, b), len(mine), t.device)[0].shape[0]

    def count(h):
        return h.count_rows(col)

    def exists(kind):
        return lambda h: int(h.probe_exists_tuples(t, kind, torch.empty(len(mine), dtype=torch.int64, device="cuda")).item())

    alone = {f: _alone(build, f) for f in (routed, tuples, count)}
    for f in alone:
        assert alone[f] == (alone[f][0], "radix") and alone[f][0] not in (None, EXISTS)
    steps = [(routed, M, alone[routed]), (exists("semi"), hit, (EXISTS, "radix")), (tuples, M, alone[tuples]),
             (exists("anti"), len(mine) - hit, (EXISTS, "radix")), (count, M, alone[count]),
             (routed, M, alone[routed]), (exists("semi"), hit, (EXISTS, "radix")), (routed, M, alone[routed])]
    build(hj)
    for i, (probe, want, reported) in enumerate(steps):
        got = probe(hj)
        print(f"step {i}: count {got} (want {want}), reports {_reported(hj)} (want {reported})")
        assert got == want
        assert _reported(hj) == reported


def test_routed_build_rejects_more_than_nine_routing_bits(hj):
    """log2(nranks) + sub_bits > 9 cannot have come out of hj_dev_route_i64
    (<= 512 parts): the routed build refuses it, as the routing does."""
    t = torch.zeros((16, 2), dtype=torch.int64, device="cuda")
    c = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    c[0, 0] = 16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.hj_dev_build_routed_i64(hj._ctx, vp(t), 16, vp(c), 1, 256, 2, st) == HJ_ERR_ARG
    assert lib.hj_dev_build_routed_i64(hj._ctx, vp(t), 16, vp(c), 1, 128, 2, st) == 0
