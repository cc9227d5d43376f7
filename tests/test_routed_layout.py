"""The one-device emulation of N ranks' folded exchange (routed_layout.py),
proved on the CPU: with the numpy stand-in for the kernels
(test_dist_gloo._CpuJoin) the union of the per-owner pairs is the oracle's
join, every assembled buffer satisfies check_layout, and check_layout rejects
a buffer whose count matrix does not describe it.  The GPU tests
(test_gpu_routed.py, test_gpu_route.py) run the same helper and the same
statement over the real kernels."""
import numpy as np
import pytest
import torch

import routed_layout as RL
from test_dist_gloo import _CpuJoin


def _relations(oracle, kind, seed):
    if kind == "pkfk":
        return oracle.gen_pkfk_i64(seed, 3000, 5000, 0.85)
    if kind == "dups":
        rk, rp = oracle.gen_uniform_i64(seed, 1, 1, 300, 2000)
        sk, sp = oracle.gen_uniform_i64(seed, 2, 1, 300, 2600)
        return rk, rp, sk, sp
    lo = -(1 << 63)   # INT64_MIN keys on both sides
    rk, rp = oracle.gen_uniform_i64(seed, 1, lo, lo + 40, 1500)
    sk, sp = oracle.gen_uniform_i64(seed, 2, lo, lo + 40, 1800)
    return rk, rp, sk, sp


@pytest.mark.parametrize("N", [1, 2, 3, 8, 64])
def test_slice_bounds_are_uneven(N):
    for n in (0, 1, 5, 4096, 60000):
        b = RL.slice_bounds(n, N)
        sizes = np.diff(b)
        assert len(b) == N + 1 and b[0] == 0 and b[-1] == n and (sizes >= 0).all()
        if N >= 3 and n >= N * N:
            assert sizes[1] == 0 and sizes[-1] == 1           # one empty sender, one with a single row
            rest = np.delete(sizes, [1, N - 1])
            assert len(set(rest.tolist())) == len(rest)        # no two of the others alike
        if N == 2 and n >= 2:
            assert sizes.tolist() == [1, n - 1]


def test_rparts_is_the_radix_hash():
    keys = np.array([0, 1, -1, -(1 << 63), (1 << 63) - 1, 12345678901234567], np.int64)
    for bits in (1, 3, 9):
        want = [((int(k) & ((1 << 64) - 1)) * 0x9E3779B97F4A7C15 % (1 << 64)) >> (64 - bits) for k in keys]
        assert RL.rparts(keys, bits).tolist() == want
    assert RL.rparts(keys, 0).tolist() == [0] * len(keys)
    assert np.array_equal(RL.rparts(keys, 7), _CpuJoin._rparts(keys, 7))


@pytest.mark.parametrize("N,sub,s_parts", [(1, 5, 2), (2, 4, 1), (4, 3, 3), (8, 1, 1), (8, 6, 2), (64, 3, 2)])
@pytest.mark.parametrize("kind", ["pkfk", "dups", "int64_min"])
def test_folded_join_cpu_vs_oracle(oracle, N, sub, s_parts, kind):
    rk, rp, sk, sp = _relations(oracle, kind, 100 + N + sub)
    hj = _CpuJoin()
    t = torch.from_numpy
    outs = RL.folded_join(hj, t(rk), t(rp), t(sk), t(sp), N, sub, s_parts)
    assert len(outs) == N
    assert hj.calls["build"] == N and hj.calls["probe"] >= N * min(s_parts, 1 << sub)   # (+ re-probes at the exact M)
    assert oracle.same_multiset(*RL.union(outs), *oracle.nested_loop_i64(rk, rp, sk, sp))
    # every pair came from the owner of its key (S.pay of the generators is the row id)
    g = N.bit_length() - 1
    for q, (_, o_s) in enumerate(outs):
        assert (RL.rparts(sk[o_s.numpy()], g) == q).all()


def test_received_buffers_are_the_exchange_layout(oracle):
    """Routed.received against a direct statement: source by source, each
    source's rows of the owner's bins in bin order, counts stacked (N, nbins)."""
    N, sub = 4, 3
    F = 1 << sub
    rk, rp = oracle.gen_uniform_i64(7, 1, -(1 << 40), 1 << 40, 5000)
    hj = _CpuJoin()
    R = RL.Routed(hj, torch.from_numpy(rk), torch.from_numpy(rp), N, sub)
    sizes = np.diff(R.bounds)
    assert sizes[1] == 0 and sizes[-1] == 1
    part = RL.rparts(rk, 2 + sub)
    seen = 0
    for q in range(N):
        for b0, b1 in ((0, F), (2, 5)):
            t, c = R.received(q, b0, b1)
            assert c.shape == (N, b1 - b0) and c.is_contiguous()
            RL.check_layout(t.numpy(), c.numpy(), b0, N, sub, q)
            for s in range(N):
                sl = slice(R.bounds[s], R.bounds[s + 1])
                want = [int(((part[sl] == q * F + b)).sum()) for b in range(b0, b1)]
                assert c[s].tolist() == want
            if (b0, b1) == (0, F):
                seen += t.shape[0]
                # the buffer is a permutation of the owner's rows
                mine = part >> sub == q
                assert sorted(zip(t[:, 0].tolist(), t[:, 1].tolist())) == sorted(zip(rk[mine].tolist(), rp[mine].tolist()))
    assert seen == len(rk)


def test_check_layout_rejects_a_wrong_count_matrix(oracle):
    """Two sources' count rows swapped (bin counts differ, totals kept): the
    statement the GPU tests rely on must notice."""
    N, sub = 4, 2
    rk, rp = oracle.gen_uniform_i64(9, 1, -(1 << 40), 1 << 40, 3000)
    R = RL.Routed(_CpuJoin(), torch.from_numpy(rk), torch.from_numpy(rp), N, sub)
    t, c = R.received(1)
    RL.check_layout(t.numpy(), c.numpy(), 0, N, sub, 1)
    c = c.numpy()
    assert not np.array_equal(c[0], c[2])
    swapped = c.copy()
    swapped[[0, 2]] = swapped[[2, 0]]
    with pytest.raises(AssertionError):
        RL.check_layout(t.numpy(), swapped, 0, N, sub, 1)
    with pytest.raises(AssertionError):
        RL.check_layout(t.numpy(), c, 0, N, sub, 2)        # another owner's bits
    with pytest.raises(AssertionError):
        RL.check_layout(t.numpy()[:-1], c, 0, N, sub, 1)   # a row short
