#!/usr/bin/env python3
"""Probe-phase time of the group probe against the inner probe of the SAME
build, box and process, and against what a caller composed before it existed:
probe_relation with rpay = arange(|R|) followed by torch index_add_ /
scatter_reduce_ over out_r, timed together (DESIGN §5 "Group probe against
inner + reduction").  Device events, 2 warm-up rounds, then REPS alternating
rounds of inner, group (count + sum), group (all four), inner + reduction;
median and [min, max] in ms.  `probe*` keys are the library's own events
(set_timing), `wall` a pair of stream events around the whole row (the only
figure the composition has).  The composition's count and sum per R row must
equal the group probe's.

  python profiles/group_probe.py pkfk radix 28 28        # 2^28 x 2^28 PK-FK (C3's inputs)
  python profiles/group_probe.py pkfk radix 28 28 0.5
  python profiles/group_probe.py pkfk global 20 26
  python profiles/group_probe.py ref                     # 10M x 10M i32, keys in [1, 100k]
  python profiles/group_probe.py zipf radix 26 26 0.9    # a Zipf probe side
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402

shape = sys.argv[1]
REPS = int(os.environ.get("REPS", "7"))
frac = theta = None
if shape == "ref":
    strategy, nr, ns = "auto", 10_000_000, 10_000_000
    rk = hashjoin.gen_uniform_i32(0x5EED, 1, 1, 100_000, nr)
    sk = hashjoin.gen_uniform_i32(0x5EED, 2, 1, 100_000, ns)
    rp = sp = None
    pairs = 1_020_000_000   # ~ nr * ns / 100k: every S row meets ~100 build rows
else:
    strategy, nr, ns = sys.argv[2], 1 << int(sys.argv[3]), 1 << int(sys.argv[4])
    if shape == "zipf":
        theta = float(sys.argv[5]) if len(sys.argv) > 5 else 0.9
        rk = hashjoin.gen_pkfk(0x5EED, nr, 1, 1.0)[0]
        sk, sp = hashjoin.gen_zipf(0x5EED, nr, ns, theta)
    else:
        frac = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
        rk, _, sk, sp = hashjoin.gen_pkfk(0x5EED, nr, ns, frac)
    rp = torch.arange(nr, dtype=torch.int64, device="cuda")   # the payload is R's row index
    pairs = ns
wide = rk.dtype == torch.int64
kt = rk.dtype
hj = hashjoin.HashJoin(0)
hj.set_strategy(strategy)
hj.set_timing(True)
out_r = torch.empty(pairs, dtype=kt, device="cuda")
out_s = torch.empty_like(out_r)
g = {c: torch.empty(nr, dtype=torch.int64 if c == "sum" else kt, device="cuda") for c in ("r", "cnt", "sum", "min", "max")}
c_cnt = torch.empty(nr, dtype=torch.int64, device="cuda")
c_sum = torch.empty_like(c_cnt)
c_min = torch.empty_like(c_cnt)
c_max = torch.empty_like(c_cnt)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
hj.build_table(rk, rp)
build_ms = hj.last_timing()["build"]
res, counts, kernels = {}, {}, {}


def one(kind):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if kind == "inner":
        cnt = hj.probe_relation(sk, sp, out_r, out_s)
    elif kind == "group-count-sum":
        cnt = hj.probe_group(sk, sp, "all", g["r"], g["cnt"], g["sum"])
    elif kind == "group-all-four":
        cnt = hj.probe_group(sk, sp, "all", g["r"], g["cnt"], g["sum"], g["min"], g["max"])
    else:
        # what a caller does today: every pair, then a reduction over R's row index
        cnt = hj.probe_relation(sk, sp, out_r, out_s)
        m = int(cnt.item())
        assert m <= pairs, (m, pairs)
        idx, val = out_r[:m].long(), out_s[:m].long()
        c_cnt.zero_().index_add_(0, idx, torch.ones_like(val))
        c_sum.zero_().index_add_(0, idx, val)
        if kind == "inner+reduce-all-four":
            c_min.fill_(I64_MAX).scatter_reduce_(0, idx, val, "amin")
            c_max.fill_(I64_MIN).scatter_reduce_(0, idx, val, "amax")
    e1.record()
    e1.synchronize()
    t = hj.last_timing()
    t["wall"] = e0.elapsed_time(e1)
    counts[kind] = int(cnt.item())
    kernels[kind] = hj.join_kernel
    return t


KINDS = ("inner", "group-count-sum", "group-all-four", "inner+reduce-count-sum", "inner+reduce-all-four")
for it in range(2 + REPS):
    for kind in KINDS:
        t = one(kind)
        if it >= 2:
            for k in ("wall", "probe", "probe_partition", "probe_join"):
                res.setdefault(kind + ":" + k, []).append(t[k])
# the last rounds left the composition's and the group probe's results: they must agree row for row
assert counts["group-all-four"] == nr, counts
row = g["r"].long()
some = g["cnt"].long() > 0
assert torch.equal(c_cnt[row], g["cnt"].long()) and torch.equal(c_sum[row], g["sum"]), "count / sum differ"
assert torch.equal(c_min[row][some], g["min"].long()[some]) and torch.equal(c_max[row][some], g["max"].long()[some]), \
    "min / max differ"
out = {"shape": shape, "strategy": hj.strategy_used, "join_kernel": kernels["group-all-four"], "build_rows": nr, "probe_rows": ns,
       "frac": frac, "theta": theta, "reps": REPS, "build_ms": round(build_ms, 3), "rows": counts}
for k, v in res.items():
    out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(out))
