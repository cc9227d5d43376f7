#!/usr/bin/env python3
"""Probe-phase time of the semi- / anti-join probes against the inner probe of
the SAME build, box and process (DESIGN §5 "exists probes"): device events
(set_timing), 2 warm-up rounds, then REPS alternating rounds of inner, semi,
anti; median and [min, max] of probe / probe_partition / probe_join in ms.

  python profiles/exists_probe.py radix 28 28     # 2^28 x 2^28 PK-FK (C3's inputs)
  python profiles/exists_probe.py global 20 26
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
out_r = torch.empty(ns, dtype=torch.int64, device="cuda")
out_s = torch.empty_like(out_r)
hj.build_table(rk, rp)
build_ms = hj.last_timing()["build"]
res, counts = {}, {}


def one(kind):
    if kind == "inner":
        cnt = hj.probe_relation(sk, sp, out_r, out_s)
    else:
        cnt = hj.probe_exists(sk, sp, kind, out_s)
    t = hj.last_timing()
    counts[kind] = int(cnt.item())
    return t


for it in range(2 + REPS):
    for kind in ("inner", "semi", "anti"):
        t = one(kind)
        if it >= 2:
            for k in ("probe", "probe_partition", "probe_join"):
                res.setdefault(kind + ":" + k, []).append(t[k])
out = {"strategy": hj.strategy_used, "build_rows": nr, "probe_rows": ns, "frac": frac, "reps": REPS,
       "build_ms": round(build_ms, 3), "rows": counts, "join_kernel": hj.join_kernel}
for k, v in res.items():
    out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(out))
