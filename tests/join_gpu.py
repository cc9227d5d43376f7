"""What the join kinds' GPU tests (test_gpu_exists, _lookup, _expand, _asof,
_group, _aggregate, _outer, _full and the modules beside them) share: the
module's context, the strategy helpers, host <-> device helpers, and the
skeletons of the timing-report and captured-graph tests.  What differs per
kind -- its payloads, its probe and check -- stays in its module."""
import contextlib

import numpy as np
import pytest
import torch

from hashjoin import HashJoin, lib


@pytest.fixture(scope="module")
def hj():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    h = HashJoin(0)
    yield h
    h.close()


@pytest.fixture
def glob_hj(hj):
    hj.set_strategy("global")
    yield hj
    hj.set_strategy("auto")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.int64)


def sentinels(n, value, dtype=torch.int64):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def build(hj, rk, rp):
    """Build R: int64 keys with their payload column, i32 keys alone (row ids)."""
    hj.build_table(dev(rk), dev(rp) if rk.dtype == np.int64 else None)


def radix(hj, bits):
    hj.set_strategy("radix", radix_bits=bits)


@contextlib.contextmanager
def strategy(hj, name, bits=0):
    """with strategy(hj, name, bits): the strategy for the block (bits: a radix plan's), AUTO afterwards."""
    hj.set_strategy(name, radix_bits=bits if name == "radix" else 0)
    try:
        yield hj
    finally:
        hj.set_strategy("auto")


def assert_radix_kernel(hj, kernel_id, kernel_name):
    """The last probe ran under the radix strategy in the kernel the ABI numbers kernel_id."""
    assert hj.strategy_used == "radix"
    assert lib.hj_ctx_join_kernel(hj._ctx) == kernel_id
    assert hj.join_kernel == kernel_name


def timing_reports(hj, strategy, build, probes):
    """With timing on under `strategy` (radix: 2^6 partitions): build(), then behind each call of `probes` the
    context reports a probe time and, for radix, its split into partitioning and join."""
    hj.set_strategy(strategy, radix_bits=6 if strategy == "radix" else 0)
    hj.set_timing(True)
    try:
        build()
        for probe in probes:
            probe()
            t = hj.last_timing()
            assert t["probe"] > 0
            if strategy == "radix":
                assert t["probe_partition"] > 0 and t["probe_join"] > 0
    finally:
        hj.set_timing(False)
        hj.set_strategy("auto")


def graph_replay(hj, strategy, setup, step, replays, reload, verify):
    """A captured call replayed over inputs rewritten in place, under `strategy`: setup() loads the first inputs,
    builds and reserves; step() -- the call, into tensors that stay -- runs once eagerly on a fresh stream and is
    then captured there; per entry of `replays`, reload(entry) overwrites the inputs and refills the outputs, the
    graph is replayed, and verify(entry) holds the outputs against the caller's expectation."""
    hj.set_strategy(strategy)
    g = None
    try:
        setup()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):   # one eager step on the capture stream first
            step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
        torch.cuda.synchronize()
        assert hj.strategy_used == strategy
        for entry in replays:
            reload(entry)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            verify(entry)
    finally:
        del g
        torch.cuda.synchronize()
        hj.set_strategy("auto")
