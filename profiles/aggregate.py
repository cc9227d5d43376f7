#!/usr/bin/env python3
"""Time of the hash aggregate (HashJoin.aggregate_into: GROUP BY key over one
relation) against what a caller composed before it existed:
torch.unique(key, return_inverse=True) followed by index_add_ (count, sum) and
scatter_reduce_ (amin, amax) over the inverse, timed together between two
stream events (DESIGN §5 "Hash aggregate against torch.unique + reduction").
One process, one box: 2 warm-up rounds, then REPS rounds that alternate the
aggregate under GLOBAL forced, RADIX forced and AUTO (count + sum, and all
four) with the composition (the same two); median and [min, max] in ms.
`radix_plan` is the bits of each partition pass the call ran under ([] under
GLOBAL).  `probe*` keys are the library's own events (set_timing: the whole call, and
under RADIX its partition / aggregate split), `wall` a pair of stream events
around the call (the only figure the composition has).  `copy` is one flat
hj_dev_stream_copy of the input's bytes (read + write) on the same box.  The
composition's columns must equal the aggregate's, key for key.

  python profiles/aggregate.py distinct 26     # 2^26 rows, all distinct (gen_pkfk's build side)
  python profiles/aggregate.py uniform 26 16   # 2^26 rows uniform over 2^16 keys
  python profiles/aggregate.py zipf 26 0.9     # 2^26 rows Zipf(0.9) over 2^26 keys
  python profiles/aggregate.py ref             # 10M i32 keys in [1, 100k]
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
param = None
if shape == "ref":
    n = 10_000_000
    key, val = hashjoin.gen_uniform_i32(0x5EED, 1, 1, 100_000, n), None
else:
    n = 1 << int(sys.argv[2])
    if shape == "distinct":
        key, val = hashjoin.gen_pkfk(0x5EED, n, 1, 1.0)[:2]
    elif shape == "uniform":
        param = int(sys.argv[3])
        key, val = hashjoin.gen_uniform_i64(0x5EED, 1, 1, 1 << param, n)
    else:
        param = float(sys.argv[3]) if len(sys.argv) > 3 else 0.9
        key, val = hashjoin.gen_zipf(0x5EED, n, n, param)
kt = key.dtype
tval = val if val is not None else torch.arange(n, dtype=torch.int64, device="cuda")   # i32: the row ids
hj = hashjoin.HashJoin(0)
hj.set_timing(True)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
m_exp = hj.count_distinct(key)
cap = max(1, m_exp)
out = {c: torch.empty(cap, dtype=torch.int64 if c == "sum" else kt, device="cuda") for c in ("key", "cnt", "sum", "min", "max")}
torch_res = {}
res, rows, kernels, used, plans = {}, {}, {}, {}, {}


def one(kind):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    who, what = kind.split(":")
    if who != "torch":
        hj.set_strategy(who)
    e0.record()
    if who == "torch":
        # what a caller did before: sort-based unique, then reductions over the inverse
        uk, inv = torch.unique(key, return_inverse=True)
        c_cnt = torch.zeros(uk.numel(), dtype=torch.int64, device="cuda").index_add_(0, inv, torch.ones_like(tval))
        c_sum = torch.zeros(uk.numel(), dtype=torch.int64, device="cuda").index_add_(0, inv, tval)
        torch_res.update(key=uk, cnt=c_cnt, sum=c_sum)
        if what == "all-four":
            torch_res["min"] = torch.full((uk.numel(),), I64_MAX, dtype=torch.int64, device="cuda").scatter_reduce_(
                0, inv, tval, "amin")
            torch_res["max"] = torch.full((uk.numel(),), I64_MIN, dtype=torch.int64, device="cuda").scatter_reduce_(
                0, inv, tval, "amax")
        m = uk.numel()
    elif what == "count-sum":
        m = hj.aggregate_into(key, val, out["key"], out["cnt"], out["sum"])
    else:
        m = hj.aggregate_into(key, val, out["key"], out["cnt"], out["sum"], out["min"], out["max"])
    e1.record()
    e1.synchronize()
    t = hj.last_timing() if who != "torch" else {}
    t["wall"] = e0.elapsed_time(e1)
    rows[kind] = int(m) if who == "torch" else int(m.item())
    if who != "torch":
        kernels[kind], used[kind], plans[kind] = hj.join_kernel, hj.strategy_used, hj.radix_plan
    return t


def agree():
    """The aggregate's last result (all four) against the composition's, key for key."""
    o = torch.argsort(out["key"][:m_exp].long())
    assert torch.equal(out["key"][:m_exp].long()[o], torch_res["key"].long()), "keys differ"
    for c in ("cnt", "sum", "min", "max"):
        assert torch.equal(out[c][:m_exp].long()[o], torch_res[c]), c + " differs"


KINDS = [w + ":" + a for w in ("global", "radix", "auto", "torch") for a in ("count-sum", "all-four")]
for it in range(2 + REPS):
    for kind in KINDS:
        t = one(kind)
        if it >= 2:
            for k in ("wall", "probe", "probe_partition", "probe_join"):
                if k in t:
                    res.setdefault(kind + ":" + k, []).append(t[k])
    if it == 0:
        # each strategy's all-four result against the composition's, once
        one("torch:all-four")
        for w in ("global", "radix", "auto"):
            one(w + ":all-four")
            agree()
assert all(r == m_exp for r in rows.values()), (rows, m_exp)
# one flat streamed copy of the input's bytes on this box
src = torch.empty(n * (16 if val is not None else 4) // 8 + 2, dtype=torch.int64, device="cuda")
src = src[: src.numel() // 2 * 2]
dst = torch.empty_like(src)
copy = []
for it in range(2 + REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hashjoin.stream_copy(src, dst, "flat")
    e1.record()
    e1.synchronize()
    if it >= 2:
        copy.append(e0.elapsed_time(e1))
line = {"shape": shape, "param": param, "rows": n, "groups": m_exp, "key": str(kt).replace("torch.", ""), "reps": REPS,
        "strategy_used": used, "join_kernel": kernels, "radix_plan": plans,
        "copy": {"median": round(statistics.median(copy), 3), "min": round(min(copy), 3), "max": round(max(copy), 3)}}
for k, v in res.items():
    line[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(line))
