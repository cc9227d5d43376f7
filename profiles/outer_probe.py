#!/usr/bin/env python3
"""Probe-phase time of the outer probe against inner + anti of the SAME build,
box and process -- what a caller had to run for an outer join before
hj_dev_probe_outer_* (DESIGN "Outer probe"): device events (set_timing), 2
warm-up rounds, then REPS alternating rounds of inner, anti, outer; median and
[min, max] of probe / probe_partition / probe_join in ms, then the yardstick:

  saving      = inner + anti - outer            (medians of the probe phase)
  spread      = (max - min) of inner + (max - min) of anti
  passes      = saving > spread
  stage2      = outer probe_join - inner probe_join   (radix: the unmatched-rows
                stage, the cost a fused radix kernel would remove)

  python profiles/outer_probe.py radix 28 28 0.5     # 2^28 x 2^28 PK-FK, half the probe rows match
  python profiles/outer_probe.py global 20 26 1.0
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
out_r = torch.empty(ns, dtype=torch.int64, device="cuda")   # (PK-FK: M = |S| for the outer probe)
out_s = torch.empty_like(out_r)
hj.build_table(rk, rp)
build_ms = hj.last_timing()["build"]
res, counts = {}, {}
KINDS = ("inner", "anti", "outer")
PHASES = ("probe", "probe_partition", "probe_join")


def one(kind):
    if kind == "inner":
        cnt = hj.probe_relation(sk, sp, out_r, out_s)
    elif kind == "anti":
        cnt = hj.probe_exists(sk, sp, "anti", out_s)
    else:
        cnt = hj.probe_outer(sk, sp, out_r, out_s, null=-1)
    t = hj.last_timing()
    counts[kind] = int(cnt.item())
    return t


for it in range(2 + REPS):
    for kind in KINDS:
        t = one(kind)
        if it >= 2:
            for k in PHASES:
                res.setdefault(kind + ":" + k, []).append(t[k])
assert counts["outer"] == counts["inner"] + counts["anti"] == ns, counts
out = {"strategy": hj.strategy_used, "build_rows": nr, "probe_rows": ns, "frac": frac, "reps": REPS,
       "build_ms": round(build_ms, 3), "rows": counts}
for k, v in res.items():
    out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
med = {k: out[k + ":probe"]["median"] for k in KINDS}
spread = sum(out[k + ":probe"]["max"] - out[k + ":probe"]["min"] for k in ("inner", "anti"))
out["saving_ms"] = round(med["inner"] + med["anti"] - med["outer"], 3)
out["spread_ms"] = round(spread, 3)
out["passes"] = out["saving_ms"] > out["spread_ms"]
out["outer_over_inner"] = round(med["outer"] / med["inner"], 3) if med["inner"] > 0 else None
out["stage2_ms"] = round(out["outer:probe_join"]["median"] - out["inner:probe_join"]["median"], 3)
print(json.dumps(out))
