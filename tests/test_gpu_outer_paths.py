"""The outer, full and build probes behind every radix join path.

The unmatched-rows stages (radix_unmatched, radix_unmatched_build) build a
second work map in the work area the join's kernels have just used and append
behind the join's cursor.  That has to hold behind the stream kernel, the
grouped kernel (int64 and i32 rows), the bucketed kernel with repeated keys
and the deferral chains (list 1 -> list 2 -> k_join) alike, so each shape
here first pins the kernel its inner probe runs (outer_cases.radix_path_case)
and then runs every kind on that one build; and on a context whose buffers no
earlier join has grown.

Expected rows come from numpy alone (outer_cases.Expect) and are compared as
exact multisets."""
from collections import Counter

import numpy as np
import pytest
import torch

import outer_cases as OC
from hashjoin import HashJoin
from join_gpu import dev, hj, sentinels  # noqa: F401

pytestmark = pytest.mark.gpu

RADIX_KERNELS = ("k_join_b", "k_join_u_stream", "k_join_grp")
NULL_R, NULL_S, SENTINEL = -9, -10, -12345   # payloads are >= 0


class Case:
    """One shape on the device: keys, payloads (int64: the row index plus an
    offset; i32: the row id itself) and what numpy expects."""

    def __init__(self, rk, sk, exp, wide):
        self.wide, self.exp = wide, exp
        self.rp = np.arange(len(rk), dtype=np.int64) + (1000000 if wide else 0)
        self.sp = np.arange(len(sk), dtype=np.int64) + (50000000 if wide else 0)
        self.d_rk, self.d_sk = dev(rk), dev(sk)
        self.d_rp, self.d_sp = (dev(self.rp), dev(self.sp)) if wide else (None, None)
        self.dt = torch.int64 if wide else torch.int32

    def build(self, hj):
        hj.build_table(self.d_rk, self.d_rp)

    def rows(self, kind):
        return self.exp.rows(kind, self.rp, self.sp, NULL_R, NULL_S)

    def probe(self, hj, kind, cap, extra=64):
        """Probe `kind` ("inner" too) into outputs of `cap` rows followed by
        `extra` sentinel rows the probe is not told about: (M, r, s), all cap + extra rows."""
        back_r = sentinels(cap + extra, SENTINEL, self.dt)
        back_s = torch.full_like(back_r, SENTINEL)
        o_r, o_s = back_r[:cap], back_s[:cap]
        if kind == "inner":
            cnt = hj.probe_relation(self.d_sk, self.d_sp, o_r, o_s)
        elif kind == "outer":
            cnt = hj.probe_outer(self.d_sk, self.d_sp, o_r, o_s, null=NULL_R)
        else:
            cnt = hj.probe_full(self.d_sk, self.d_sp, o_r, o_s, kind=kind, null_r=NULL_R, null_s=NULL_S)
        m = int(cnt.item())
        return m, back_r.cpu().numpy().astype(np.int64), back_s.cpu().numpy().astype(np.int64)

    def count(self, hj, kind):
        return hj.count_outer(self.d_sk) if kind == "outer" else hj.count_full(self.d_sk, kind=kind)

    def check(self, hj, kind):
        """The probe of `kind`, then its count form: exact M, exact rows, nothing past M."""
        m = self.exp.m(kind)
        got, g_r, g_s = self.probe(hj, kind, m)
        assert got == m, kind
        assert (g_r[m:] == SENTINEL).all() and (g_s[m:] == SENTINEL).all(), kind
        assert OC.same_rows(g_r[:m], g_s[:m], *self.rows(kind), NULL_R, NULL_S), kind
        assert self.count(hj, kind) == m, kind


@pytest.mark.parametrize("name", OC.RADIX_SHAPES)
def test_every_kind_behind_each_join_kernel(hj, oracle, name):
    c = OC.radix_path_case(oracle, name)
    case, e = Case(c["rk"], c["sk"], c["exp"], c["wide"]), c["exp"]
    hj.set_strategy("radix", radix_bits=c["bits"])
    try:
        case.build(hj)
        m, r1, s1 = case.probe(hj, "inner", e.pairs)
        assert hj.strategy_used == "radix"
        kernel = hj.join_kernel
        if c["kernel"] is None:
            assert kernel in RADIX_KERNELS
        else:
            assert kernel == c["kernel"]   # (a shape that does not choose its kernel is the shape's fault)
        dups = hj.has_duplicates()
        assert m == e.pairs
        first = OC.sorted_pairs(r1[:m], s1[:m])
        assert np.array_equal(first, OC.sorted_pairs(case.rp[e.ri], case.sp[e.si]))
        for kind in OC.KINDS:
            case.check(hj, kind)
            assert hj.strategy_used == "radix"
            assert hj.join_kernel == kernel, kind
            assert hj.has_duplicates() == dups, kind
        m, r2, s2 = case.probe(hj, "inner", e.pairs)
        assert m == e.pairs and np.array_equal(OC.sorted_pairs(r2[:m], s2[:m]), first)
        assert hj.join_kernel == kernel
    finally:
        hj.set_strategy("auto")


@pytest.mark.parametrize("where", ["pairs", "s-null-rows", "r-null-rows"])
@pytest.mark.parametrize("name", ["stream-pkfk", "grp-wide", "grp-i32"])
def test_capacity_behind_each_join_kernel(hj, oracle, name, where):
    """out_cap inside the pairs, inside S's null rows and inside R's null rows
    (the stages' order) of the full kind: M stays exact, nothing at or past
    out_cap is touched, and what was written is a sub-multiset of the expected rows."""
    c = OC.radix_path_case(oracle, name)
    case, e = Case(c["rk"], c["sk"], c["exp"], c["wide"]), c["exp"]
    assert min(e.pairs, e.n_s, e.n_r) > 600
    cap = {"pairs": e.pairs - 500, "s-null-rows": e.pairs + e.n_s - 500, "r-null-rows": e.m("full") - 500}[where]
    hj.set_strategy("radix", radix_bits=c["bits"])
    try:
        case.build(hj)
        m, g_r, g_s = case.probe(hj, "full", cap, extra=4096)
        assert m == e.m("full") > cap
        assert hj.strategy_used == "radix" and hj.join_kernel == c["kernel"]
        assert (g_r[cap:] == SENTINEL).all() and (g_s[cap:] == SENTINEL).all()
        e_r, e_s = case.rows("full")
        extra = Counter(zip(g_r[:cap].tolist(), g_s[:cap].tolist())) - Counter(zip(e_r.tolist(), e_s.tolist()))
        assert not extra, list(extra.items())[:5]
    finally:
        hj.set_strategy("auto")


def test_fresh_context_runs_build_side_probes_first():
    """radix_unmatched_build cuts R's runs into work items in an area that the
    build sized: on a new context, whose buffers no earlier join has grown, the
    first probes are build, full and outer (50 probe rows against 30000 build
    rows in 2^10 partitions), then a 200000-row probe side of the same build."""
    c = OC.fresh_context_case()
    h = HashJoin(0)
    try:
        h.set_strategy("radix", radix_bits=c["bits"])
        small = Case(c["rk"], c["sk"], c["exp"], True)
        small.build(h)
        for kind in ("build", "full", "outer"):
            small.check(h, kind)
            assert h.strategy_used == "radix" and h.join_kernel in RADIX_KERNELS
        big = Case(c["rk"], c["big"], c["exp_big"], True)
        for kind in ("build", "full", "outer"):
            big.check(h, kind)
            assert h.strategy_used == "radix" and h.join_kernel in RADIX_KERNELS
    finally:
        h.close()
