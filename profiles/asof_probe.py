#!/usr/bin/env python3
"""Probe-phase time of the as-of probe (backward) against the positional lookup
with the payload column alone, on the SAME build, box and process (DESIGN §5
"As-of probe against the lookup").  PK-FK inputs of gen_pkfk, a unique build
key; the bound column is S's payload column (any int64 column: with one
partner per row the bound decides found / not found, not the walk's length).
The library's own events (set_timing), one warm-up round, then REPS alternating
rounds; median and [min, max] in ms.  `copy` is the flat copy of |S| 16-B rows
(hj_dev_stream_copy) between stream events, the box's yardstick.

  python profiles/asof_probe.py global 24 26
  python profiles/asof_probe.py radix 24 26
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
REPS = int(os.environ.get("REPS", "5"))
nr, ns = 1 << lr, 1 << ls
rk, rp, sk, sp = hashjoin.gen_pkfk(0x5EED, nr, ns, 1.0)
hj = hashjoin.HashJoin(0)
hj.set_strategy(strategy)
hj.set_timing(True)
look_r = torch.empty(ns, dtype=torch.int64, device="cuda")
asof_r = torch.empty_like(look_r)
hj.build_table(rk, rp)
build_ms = hj.last_timing()["build"]
res, counts = {}, {}


def one(kind):
    if kind == "lookup-payload-only":
        cnt = hj.probe_lookup(sk, look_r)
    else:
        cnt = hj.probe_asof(sk, sp, asof_r, direction="backward")
    torch.cuda.synchronize()
    counts[kind] = int(cnt.item())
    return hj.last_timing()


def copy_ms():
    src = torch.empty((ns, 2), dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    src.fill_(1)
    ts = []
    for _ in range(1 + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hashjoin.stream_copy(src, dst, shape="flat")
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts[1:]


for it in range(1 + REPS):
    for kind in ("lookup-payload-only", "asof-backward"):
        t = one(kind)
        if it >= 1:
            for k in ("probe", "probe_partition", "probe_join"):
                res.setdefault(kind + ":" + k, []).append(t[k])
# (the same rows qualify where the bound admits the one partner: the as-of result is the lookup's or null)
agree = bool(((asof_r == look_r) | (asof_r == -1)).all().item())
out = {"strategy": hj.strategy_used, "join_kernel": hj.join_kernel, "build_rows": nr, "probe_rows": ns, "reps": REPS,
       "build_ms": round(build_ms, 3), "rows": counts, "asof_is_lookup_or_null": agree}
for k, v in res.items():
    out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
c = copy_ms()
out["copy_flat_ms"] = {"median": round(statistics.median(c), 3), "min": round(min(c), 3), "max": round(max(c), 3)}
out["asof_over_lookup"] = round(out["asof-backward:probe"]["median"] / out["lookup-payload-only:probe"]["median"], 3)
print(json.dumps(out))
