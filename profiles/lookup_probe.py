#!/usr/bin/env python3
"""Probe-phase time of the positional lookup probe against the inner probe of
the SAME build, box and process, and against what a caller composed before it
existed: probe_outer with spay = arange(|S|) followed by the torch scatter
dst[out_s] = out_r, timed together (DESIGN §5 "Lookup probe against inner and
outer + scatter").  Device events, 2 warm-up rounds, then REPS alternating
rounds of inner, lookup, lookup without the count column, outer + scatter; median and [min, max] in ms.
`probe*` keys are the library's own events (set_timing), `wall` a pair of
stream events around the whole row (the only figure the composition has).

  python profiles/lookup_probe.py radix 28 28        # 2^28 x 2^28 PK-FK (C3's inputs)
  python profiles/lookup_probe.py radix 28 28 0.5
  python profiles/lookup_probe.py global 20 26
  python profiles/lookup_probe.py global 11 26       # the LDS-resident table
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
look_r = torch.empty_like(out_r)
look_c = torch.empty(ns, dtype=torch.int32, device="cuda")
dst = torch.empty_like(out_r)
rows = torch.arange(ns, dtype=torch.int64, device="cuda")
hj.build_table(rk, rp)
build_ms = hj.last_timing()["build"]
res, counts = {}, {}


def one(kind):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if kind == "inner":
        cnt = hj.probe_relation(sk, sp, out_r, out_s)
    elif kind == "lookup":
        cnt = hj.probe_lookup(sk, look_r, look_c)
    elif kind == "lookup-payload-only":   # what the composition below produces: no count column
        cnt = hj.probe_lookup(sk, look_r)
    else:
        # (a unique build key: the outer probe returns exactly |S| rows, so the
        # scatter needs no count from the device)
        cnt = hj.probe_outer(sk, rows, out_r, out_s, null=-1)
        dst[out_s] = out_r
    e1.record()
    e1.synchronize()
    t = hj.last_timing()
    t["wall"] = e0.elapsed_time(e1)
    counts[kind] = int(cnt.item())
    return t


for it in range(2 + REPS):
    for kind in ("inner", "lookup", "lookup-payload-only", "outer+scatter"):
        t = one(kind)
        if it >= 2:
            for k in ("wall", "probe", "probe_partition", "probe_join"):
                res.setdefault(kind + ":" + k, []).append(t[k])
assert counts["outer+scatter"] == ns and torch.equal(dst, look_r), "the composition and the lookup differ"
out = {"strategy": hj.strategy_used, "build_rows": nr, "probe_rows": ns, "frac": frac, "reps": REPS,
       "build_ms": round(build_ms, 3), "rows": counts}
for k, v in res.items():
    out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(out))
