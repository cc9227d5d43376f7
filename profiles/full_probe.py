#!/usr/bin/env python3
"""Probe-phase time of the build-side (RIGHT) and full outer probes against the
inner and outer probes of the SAME build, box and process, and against the
only route to a full outer join before hj_dev_probe_full_*: build R + outer
probe of S, then build S + anti probe of R (DESIGN "Full / build-side outer
probe").  Device events (set_timing), 2 warm-up rounds, then REPS alternating
rounds; median and [min, max] in ms.

  stage_build = build probe_join - inner probe_join   (radix: the exchanged
  stage_full  = full  probe_join - outer probe_join    anti stage over R)
  global: the same differences of the probe phase = marking + emit scan;
          emit_ms is the build probe of an EMPTY S (memset + scan alone, every
          R row emitted), mark_ms the rest (stage 1's marking and the pass
          over the tiles it handed to the general path)
  two_build   = build(R) + outer(S) + build(S) + anti(R), events around the lot
  one_build   = build(R) + full(S), likewise

  python profiles/full_probe.py radix 28 28 0.5     # 2^28 x 2^28 PK-FK, half the probe rows match
  python profiles/full_probe.py global 20 26 1.0
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402

strategy, lr, ls = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
frac = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
REPS = int(os.environ.get("REPS", "7"))
nr, ns = 1 << lr, 1 << ls
rk, rp, sk, sp = hashjoin.gen_pkfk(0x5EED, nr, ns, frac)
hj = hashjoin.HashJoin(0)
hj.set_strategy(strategy)
hj.set_timing(True)
out_r = torch.empty(ns + nr, dtype=torch.int64, device="cuda")   # (PK-FK: M <= |S| + |R|)
out_s = torch.empty_like(out_r)
empty = torch.empty(0, dtype=torch.int64, device="cuda")
res, counts = {}, {}
KINDS = ("inner", "outer", "build", "full") + (("emit",) if strategy == "global" else ())
PHASES = ("probe", "probe_partition", "probe_join")


def one(kind):
    if kind == "inner":
        cnt = hj.probe_relation(sk, sp, out_r, out_s)
    elif kind == "outer":
        cnt = hj.probe_outer(sk, sp, out_r, out_s, null=-1)
    elif kind == "emit":
        cnt = hj.probe_full(empty, empty, out_r, out_s, kind="build")
    else:
        cnt = hj.probe_full(sk, sp, out_r, out_s, kind=kind)
    t = hj.last_timing()
    counts[kind] = int(cnt.item())
    return t


def med(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def one_build():
    hj.build_table(rk, rp)
    hj.probe_full(sk, sp, out_r, out_s, kind="full")


def two_build():
    hj.build_table(rk, rp)
    hj.probe_outer(sk, sp, out_r, out_s, null=-1)
    hj.build_table(sk, sp)
    hj.probe_exists(rk, rp, "anti", out_s)


hj.probe_hint(ns)
hj.build_table(rk, rp)
build_ms = hj.last_timing()["build"]
for it in range(2 + REPS):
    for kind in KINDS:
        t = one(kind)
        if it >= 2:
            for k in PHASES:
                res.setdefault(kind + ":" + k, []).append(t[k])
unmatched_r = counts["build"] - counts["inner"]
assert counts["full"] == counts["outer"] + unmatched_r and counts["outer"] == ns, counts
out = {"strategy": hj.strategy_used, "build_rows": nr, "probe_rows": ns, "frac": frac, "reps": REPS,
       "build_ms": round(build_ms, 3), "rows": counts}
for k, v in res.items():
    out[k] = med(v)
m = {k: out[k + ":probe"]["median"] for k in KINDS}
phase = "probe_join" if hj.strategy_used == "radix" else "probe"
out["stage_build_ms"] = round(out["build:" + phase]["median"] - out["inner:" + phase]["median"], 3)
out["stage_full_ms"] = round(out["full:" + phase]["median"] - out["outer:" + phase]["median"], 3)
out["build_over_inner"] = round(m["build"] / m["inner"], 3)
out["full_over_outer"] = round(m["full"] / m["outer"], 3)
if strategy == "global":
    out["emit_ms"] = m["emit"]
    out["mark_ms"] = round(out["stage_build_ms"] - m["emit"], 3)
# the two routes to a full outer join, end to end, alternating (the probe hint covers both builds' sizes)
one_b, two_b = [], []
hj.probe_hint(max(nr, ns))
for it in range(1 + REPS):
    a, b = timed(one_build), timed(two_build)
    if it >= 1:
        one_b.append(a)
        two_b.append(b)
hj.probe_hint(None)
out["one_build"] = med(one_b)
out["two_build"] = med(two_b)
out["route_saving_ms"] = round(out["two_build"]["median"] - out["one_build"]["median"], 3)
print(json.dumps(out))
