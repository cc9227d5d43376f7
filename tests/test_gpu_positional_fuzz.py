"""Ragged fuzz of the probes that share the rounded-table skeleton (lookup,
expand, group) and as-of on top of it: positional_cases.fuzz_cases' sizes
around the kernels' units, every case under RADIX with its own bits and then
under GLOBAL.

One build per strategy serves all the probes, in an order shuffled by the
case's seed: lookup (both columns), as-of (all four kinds), expand inner and
outer at cap = M and one cap that cuts a segment, group MATCHED and ALL (all
five columns).  Each is compared with numpy (never the library): position by
position for lookup and as-of, offsets exactly and values inside segments for
expand, rows sorted by payload for group; d_count of each, and the sentinels
past the end.  After the last probe an inner count and has_duplicates() must
give numpy's answers -- no probe wrote what the build left.  Lookup's and
as-of's columns under RADIX and GLOBAL are compared with each other too."""
import numpy as np
import pytest
import torch

import asof_cases as AC
import expand_cases as XC
import group_cases as GC
import outer_cases as OC
import positional_cases as PC
from hashjoin import _lib, lib
from join_gpu import dev, hj, host, sentinels  # noqa: F401

pytestmark = pytest.mark.gpu

NULL, SENTINEL, EXTRA = PC.NULL, PC.SENTINEL, PC.EXTRA
CASES = PC.fuzz_cases()
PROBES = ("lookup", "asof-0", "asof-1", "asof-2", "asof-3", "expand-inner", "expand-outer", "expand-cut",
          "group-matched", "group-all")
KERNEL = {"lookup": _lib.HJ_JOIN_KERNEL_LOOKUP, "asof": _lib.HJ_JOIN_KERNEL_ASOF,
          "expand": _lib.HJ_JOIN_KERNEL_EXPAND, "group": _lib.HJ_JOIN_KERNEL_GROUP}


def expectations(case, d):
    """What numpy says every probe of the case gives, and the cap of expand-cut."""
    rk, rp, sk, sb, sv = d["rk"], d["rp"], d["sk"], d["sb"], d["sv"]
    e = {"lookup": PC.lookup_expect(rk, rp, sk, NULL)}
    for kind in AC.KINDS:
        e[f"asof-{kind}"] = AC.expect(rk, rp, sk, sb, kind, NULL)
    for how in XC.KINDS:
        e[f"expand-{how}"] = XC.ExpandExpect(rk, rp, sk, how, NULL)
    for how in ("matched", "all"):
        e[f"group-{how}"] = GC.expect(rk, rp, sk, sv, how, NULL)
    # expand-cut: the case's kind, cut one element into the segment of a seeded
    # row with several partners (none: in the middle of the result)
    how = XC.KINDS[case[0] % 2]
    x = e[f"expand-{how}"]
    many = np.flatnonzero(x.w > 1)
    rng = np.random.default_rng(500 + case[0])
    cap = int(x.off[many[rng.integers(0, len(many))]]) + 1 if len(many) else x.m // 2
    e["expand-cut"] = (how, x, cap) if 0 < cap < x.m else None
    return e


def run_probe(hj, name, d, dv, e):
    """Probe `name` of the current build against its expectation; returns the
    columns that are a function of the data alone (lookup, as-of), else None."""
    sk = d["sk"]
    n, wide = len(sk), sk.dtype == np.int64
    dt = torch.int64 if wide else torch.int32
    if name == "lookup":
        er, ec = e[name]
        o_r = sentinels(n + EXTRA, SENTINEL, dt)
        o_c = sentinels(n + EXTRA, SENTINEL, torch.int32)
        m = int(hj.probe_lookup(dv["sk"], o_r, o_c, null=NULL).item())
        g_r, g_c = host(o_r), host(o_c)
        assert np.array_equal(g_r[:n], er), np.flatnonzero(g_r[:n] != er)[:8]
        assert np.array_equal(g_c[:n], ec), np.flatnonzero(g_c[:n] != ec)[:8]
        assert (g_r[n:] == SENTINEL).all() and (g_c[n:] == SENTINEL).all()
        assert m == int((ec > 0).sum()), (m, int((ec > 0).sum()))
        return g_r, g_c
    if name.startswith("asof"):
        er, found = e[name]
        direction, strict = AC.KIND_ARGS[int(name[-1])]
        o_r = sentinels(n + EXTRA, SENTINEL, dt)
        m = int(hj.probe_asof(dv["sk"], dv["sb"], o_r, direction=direction, strict=strict, null=NULL).item())
        g = host(o_r)
        assert np.array_equal(g[:n], er), np.flatnonzero(g[:n] != er)[:8]
        assert (g[n:] == SENTINEL).all()
        assert m == int(found.sum()), (m, int(found.sum()))
        return (g,)
    if name.startswith("expand"):
        if e[name] is None:   # a result of fewer than two elements has no cap inside it
            return None
        how, x, cap = e[name] if name == "expand-cut" else (name[7:], e[name], e[name].m)
        off = sentinels(n + 1 + EXTRA, SENTINEL, torch.int64)
        buf = sentinels(cap + EXTRA, SENTINEL, dt)
        m = int(hj.probe_expand(dv["sk"], off, buf[:cap] if cap else None, how=how, null=NULL).item())
        off, vals = off.cpu().numpy(), host(buf)
        assert m == x.m, (m, x.m)
        assert np.array_equal(off[:n + 1], x.off), np.flatnonzero(off[:n + 1] != x.off)[:8]
        assert (off[n + 1:] == SENTINEL).all()
        assert x.same_values(vals, min(x.m, cap))
        assert (vals[min(x.m, cap):] == SENTINEL).all()
        return None
    how = name[6:]
    x = e[name]
    cap = max(1, len(d["rk"]))
    bufs = {c: sentinels(cap + EXTRA, SENTINEL, torch.int64 if c == "sum" else dt)
            for c in GC.COLS}
    kw = {f"out_{c}": bufs[c][:cap] for c in GC.COLS}
    if wide:
        m = int(hj.probe_group(dv["sk"], dv["sv"], how=how, null=NULL, **kw).item())
    else:   # the value is the S row id
        m = int(hj.probe_group(dv["sk"], None, how=how, null=NULL, row_base=0, **kw).item())
    assert m == len(x["r"]), (m, len(x["r"]))
    got = {c: host(b) for c, b in bufs.items()}
    o = np.argsort(got["r"][:m], kind="stable")
    for c in GC.COLS:
        assert np.array_equal(got[c][:m][o], x[c]), (c, np.flatnonzero(got[c][:m][o] != x[c])[:8])
        assert (got[c][m:] == SENTINEL).all(), c
    return None


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[4]}-{'i64' if c[5] else 'i32'}" for c in CASES])
def test_fuzz_ragged_positional(hj, case):
    i, nr, ns, span, bits, wide = case
    d = PC.fuzz_relations(case)
    e = expectations(case, d)
    pairs = OC.Expect(d["rk"], d["sk"]).pairs
    repeats = len(np.unique(d["rk"])) < nr
    dv = {k: dev(d[k]) for k in ("rk", "sk", "sb")}
    dv["rp"] = dev(d["rp"]) if wide else None
    dv["sv"] = dev(d["sv"]) if wide else None
    same = {}
    for s, strategy in enumerate(("radix", "global")):
        order = np.random.default_rng(10 * i + s).permutation(len(PROBES))
        hj.set_strategy(strategy, radix_bits=bits if strategy == "radix" else 0)
        try:
            hj.build_table(dv["rk"], dv["rp"])
            name = None
            for name in (PROBES[j] for j in order):
                cols = run_probe(hj, name, d, dv, e)
                assert hj.strategy_used == strategy, name
                if cols is not None:
                    same.setdefault(name, []).append(cols)
            if strategy == "radix":
                assert hj.radix_passes == PC.passes(bits)
                if e[name] is not None:   # (an expand-cut that did not run leaves the probe before it)
                    assert lib.hj_ctx_join_kernel(hj._ctx) == KERNEL[name.split("-")[0]], name
            assert hj.count_rows(dv["sk"]) == pairs, strategy
            assert hj.strategy_used == strategy
            assert hj.has_duplicates() == repeats, strategy
        finally:
            hj.set_strategy("auto")
    for name, (a, b) in same.items():   # RADIX and GLOBAL, bit for bit
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    assert set(same) == {"lookup", "asof-0", "asof-1", "asof-2", "asof-3"}
