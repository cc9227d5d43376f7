"""distributed_join(prefilter=...) over gloo on CPU tensors (worlds 2 and 3).

The device kernels are replaced by test_dist_gloo's _CpuJoin, unchanged, plus a
key_filter backed by the numpy model (filter_cases): every rank inserts its R
slice, the words are OR-reduced by the product's own code (torch.distributed,
ReduceOp.BOR on the int64 words tensor), S is filtered before it is routed.
Checked: the pairs equal the unfiltered call's, the reduced words equal the
model's words for the union of every rank's R, phases["filtered"] equals the
model's survivor count, fewer S rows cross when most have no partner, the
replicate mode ignores the keyword, and an hj without the factory raises."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import filter_cases as FC
from test_dist_gloo import _CpuJoin, _init, _rdzv, _relations

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.timeout(300, method="thread")


class _ModelFilter:
    """KeyFilter's clear / insert / apply on CPU tensors, by the numpy model."""

    def __init__(self, n_keys, bits_per_key):
        self.nblocks = FC.blocks_for(int(n_keys), int(bits_per_key))
        self.words = torch.full((self.nblocks * 4,), -1, dtype=torch.int64)   # undefined until the first clear

    def _w(self):
        return self.words.numpy().view(np.uint32).reshape(-1, 8)

    def clear(self):
        self.words.zero_()

    def insert(self, keys):
        self.words |= torch.from_numpy(FC.as_i64(FC.build(keys.numpy(), self.nblocks)).copy())

    def apply(self, skey, spay):
        m = torch.from_numpy(FC.test(self._w(), skey.numpy()))
        return skey[m].contiguous(), spay[m].contiguous()


class _FilteredCpuJoin(_CpuJoin):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.filters = []

    def key_filter(self, n_keys, bits_per_key=16):
        self.filters.append(_ModelFilter(n_keys, bits_per_key))
        return self.filters[-1]


def _worker(rank, world, rdzv, case, outdir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mlir-hashjoin_amd"))
    _init(rank, world, rdzv)
    from hashjoin.dist import distributed_join
    rk, rp, sk, sp = (torch.from_numpy(x) for x in _relations(case, rank, world))
    kw = dict(replicate_max_rows=case.get("replicate", 0), route_bits=case.get("route_bits"),
              s_parts=case.get("s_parts"), max_rows=case.get("max_rows"))
    bits = case.get("bits", 16)
    with pytest.raises(ValueError, match="key_filter"):   # an hj without the factory
        distributed_join(_CpuJoin(), rk, rp, sk, sp, prefilter=bits, **kw)
    ph0, ph1 = {}, {}
    base = distributed_join(_CpuJoin(), rk, rp, sk, sp, phases=ph0, **kw)
    hj = _FilteredCpuJoin()
    got = distributed_join(hj, rk, rp, sk, sp, phases=ph1, prefilter=bits, **kw)
    assert ph1["mode"] == ph0["mode"]
    if ph1["mode"] == "replicate":
        # S never crosses a link: the keyword is ignored
        assert not hj.filters and "filtered" not in ph1 and "s_filter" not in ph1
        assert ph1["rows"] == ph0["rows"]
    else:
        all_r = _relations(case, 0, 1)[0]
        want = FC.build(all_r, FC.blocks_for(case["NR"], bits))
        assert len(hj.filters) == 1
        assert np.array_equal(hj.filters[0]._w(), want)                 # the OR over every rank's R
        keep = int(FC.test(want, sk.numpy()).sum())
        assert ph1["filtered"] == (sk.numel(), keep)
        assert ph1["start"].elapsed_time(ph1["s_filter"]) >= 0.0 and ph1["s_filter"].elapsed_time(ph1["routed"]) >= 0.0
        assert ph1["rows"][0] == ph0["rows"][0]                         # R is routed as before
    np.savez(os.path.join(outdir, f"f{rank}.npz"), r0=base[0].numpy(), s0=base[1].numpy(), r1=got[0].numpy(),
             s1=got[1].numpy(), ns0=np.array([ph0["rows"][1]]), ns1=np.array([ph1["rows"][1]]),
             shuffle=np.array([ph1["mode"] == "shuffle"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", [
    dict(dist="pkfk", NR=3000, NS=6000, frac=0.25, seed=61),
    dict(dist="pkfk", NR=3001, NS=5999, frac=0.25, seed=62, world=3, s_parts=3, max_rows=113),
    dict(dist="pkfk", NR=3000, NS=6000, frac=0.25, seed=63, route_bits=3),               # folded
    dict(dist="uniform", NR=2000, NS=2500, hi=300, seed=64, world=3, bits=8),           # duplicates, every S row hits
    dict(dist="uniform", NR=600, NS=1500, lo=-(1 << 63), hi=-(1 << 63) + 4000, seed=65),  # INT64_MIN keys, misses
    dict(dist="pkfk", NR=700, NS=4000, frac=0.25, seed=66, replicate=1 << 21),          # replicated: ignored
    dict(dist="pkfk", NR=5, NS=3, frac=1.0, seed=67, world=3),                          # ranks without rows
], ids=["pkfk_quarter", "three_ranks_parts", "folded", "dups_3ranks_8bits", "int64_min", "replicate", "tiny"])
def test_distributed_join_prefilter_gloo(case, tmp_path, oracle):
    world = case.get("world", 2)
    mp.spawn(_worker, args=(world, _rdzv(tmp_path), case, str(tmp_path)), nprocs=world, join=True)
    z = [dict(np.load(tmp_path / f"f{k}.npz", allow_pickle=False)) for k in range(world)]
    cat = lambda name: np.concatenate([d[name] for d in z])  # noqa: E731
    parts = [_relations(case, k, world) for k in range(world)]
    rk, rp, sk, sp = (np.concatenate([p[i] for p in parts]) for i in range(4))
    er, es = oracle.nested_loop_i64(rk, rp, sk, sp)
    assert oracle.same_multiset(cat("r0"), cat("s0"), er, es)
    assert oracle.same_multiset(cat("r1"), cat("s1"), er, es)       # the same pairs with the prefilter
    ns0, ns1 = int(cat("ns0").sum()), int(cat("ns1").sum())
    assert ns0 == case["NS"]
    if not z[0]["shuffle"][0]:
        assert ns1 == ns0
        return
    want = FC.build(rk, FC.blocks_for(case["NR"], case.get("bits", 16)))
    assert ns1 == int(FC.test(want, sk).sum())                      # the S rows that crossed
    if case.get("frac") == 0.25:
        assert ns1 < ns0 // 2                                       # three quarters have no partner
