#!/usr/bin/env python3
"""Whole-row time of the star probe against what a caller composed before it
existed, over the SAME builds, box and process: one probe_lookup (payload only)
per dimension, a torch mask over the payload columns, nonzero and one gather
per column (DESIGN §5 "Star probe against the lookup chain").  A fact table of
2^LOG_N rows over dimensions of 2^11, 2^11, 2^15 and 2^20 build rows, all built
under the global strategy.  Settings:

  sel-first   every kind inner, one 2^11 dimension keeps ~3 % of the rows and
              comes first; the others keep ~90 % each
  sel-last    the same dimensions, the selective one last
  keep-all    every kind left (no row dropped): payload columns only, ~90 % hits

Stream events around the whole row, 2 warm-up rounds, then REPS alternating
rounds of star and chain; median and [min, max] in ms.  The script asserts that
both give the same rows and payload columns.

  python profiles/star_probe.py i64 sel-first
  python profiles/star_probe.py i32 keep-all 26
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402

width, setting = sys.argv[1], sys.argv[2]
log_n = int(sys.argv[3]) if len(sys.argv) > 3 else 26
REPS = int(os.environ.get("REPS", "7"))
assert width in ("i64", "i32") and setting in ("sel-first", "sel-last", "keep-all")
wide = width == "i64"
dt = torch.int64 if wide else torch.int32
n = 1 << log_n
NULL = -9
gen = torch.Generator(device="cuda")
gen.manual_seed(0x57A2)

# (log2 build rows, share of the fact rows with a partner); the first is the selective one
spec = [(11, 0.03 if setting != "keep-all" else 0.9), (11, 0.9), (15, 0.9), (20, 0.9)]
if setting == "sel-last":
    spec = spec[1:] + spec[:1]
how = "left" if setting == "keep-all" else "inner"

hjs, dims, keys = [], [], []
for lr, share in spec:
    nr = 1 << lr
    rk = (torch.arange(nr, dtype=torch.int64, device="cuda") * 7 + 3).to(dt)    # distinct, int32-safe
    rp = torch.arange(nr, dtype=torch.int64, device="cuda") * 3 + 1 if wide else None   # never NULL
    sk = rk[torch.randint(0, nr, (n,), device="cuda", generator=gen)]
    miss = torch.rand(n, device="cuda", generator=gen) >= share
    sk[miss] = -1 - torch.randint(0, 1 << 30, (int(miss.sum()),), device="cuda", generator=gen).to(dt)
    del miss
    h = hashjoin.HashJoin(0)
    h.set_strategy("global")
    h.build_table(rk, rp)
    assert h.strategy_used == "global"
    hjs.append(h)
    keys.append(sk)
    dims.append((h, sk, how, NULL))

star = hashjoin.StarProbe(0)
star.reserve(n)
cap = n if setting == "keep-all" else n // 8
s_pay = [torch.empty(cap, dtype=dt, device="cuda") for _ in dims]
s_row = None if setting == "keep-all" else torch.empty(cap, dtype=dt, device="cuda")
s_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
c_col = [torch.empty(n, dtype=dt, device="cuda") for _ in dims]
last = {}


def run_star():
    star.probe_into(dims, s_pay, s_row, count=s_cnt)
    last["star"] = None


def run_chain():
    for (h, sk, _, _), col in zip(dims, c_col):
        h.probe_lookup(sk, col, None, null=NULL)
    if setting == "keep-all":
        last["chain"] = (None, c_col)
        return
    keep = c_col[0] != NULL
    for col in c_col[1:]:
        keep &= col != NULL
    idx = keep.nonzero().flatten()
    last["chain"] = (idx, [col[idx] for col in c_col])


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


res = {"star": [], "chain": []}
for it in range(2 + REPS):
    for kind, f in (("star", run_star), ("chain", run_chain)):
        t = timed(f)
        if it >= 2:
            res[kind].append(t)

m = int(s_cnt.item())
idx, cols = last["chain"]
assert m <= cap, (m, cap)
if idx is None:
    assert m == n
else:
    assert m == idx.numel() and torch.equal(s_row[:m], idx.to(dt)), "the star probe and the chain keep different rows"
for a, b in zip(s_pay, cols):
    assert torch.equal(a[:m], b[:m]), "the star probe and the chain differ in a payload column"
plan = star.last_plan
out = {"width": width, "setting": setting, "probe_rows": n, "build_rows": [1 << lr for lr, _ in spec],
       "shares": [s for _, s in spec], "kept_rows": m, "kept_share": round(m / n, 4), "reps": REPS,
       "plan": {k: plan[k] for k in ("launches", "grid", "tiles", "lds_mask", "lds_bytes")}}
for k, v in res.items():
    out[k + ":wall"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(out))
