#!/usr/bin/env python3
"""Whole-row time of the star query against what a caller composed on the
previous API over the SAME builds, box and process: one torch mask per
predicate, nonzero, a gather of every needed column through it, the torch
expression into a temporary and StarProbe.aggregate_into over the cut columns
(DESIGN section 5 "Star query against mask + gather + star aggregate").  The
star aggregate section's protocol: a fact table of 2^LOG_N rows over
dimensions of 2^11, 2^11, 2^15 and 2^20 build rows built under the global
strategy, stream events around the whole row, 2 warm-up rounds, then REPS
alternating rounds of the fused call and the composed path; median and
[min, max] in ms.  The script asserts that both give the same result.

  q1   one INNER 2^11 dimension (90 % hits); discount BETWEEN 1 AND 3 (3/11 of
       the rows) AND quantity < 25 (24/50); sum(price * discount); one group
  q4   four INNER dimensions (90 % hits each), no predicate;
       sum(revenue - cost); grouped by the two 2^11 dimensions (int64: 32
       payload values each; int32: row ids, so up to 2^22 groups)
  q6   no dimension; the two predicates of q1 and a date range (1/7);
       sum(price * discount); one group.  The previous API has no aggregate
       without a dimension: the composed path ends in torch's sum
  fg   q1 grouped by a 7-value fact column.  The previous API has no fact-side
       group field: the composed path runs the star probe over the cut key
       column for the surviving positions, gathers the value and the group
       column through them and ends in HashJoin.aggregate_into

  python profiles/star_query.py i64 q1
  python profiles/star_query.py i32 q6 24
  python profiles/star_query.py all        # every row, each in a child process under its own timeout,
                                           # appended to profiles/star_query.jsonl
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

if sys.argv[1] == "all":
    log_n = sys.argv[2:3]
    with open(os.path.join(HERE, "star_query.jsonl"), "a") as out:
        for width in ("i64", "i32"):
            for shape in ("q1", "q4", "q6", "fg"):
                cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), width, shape] + log_n
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if r.returncode != 0:   # a fault, an abort or a time limit: nothing more is started
                    sys.exit(f"{' '.join(cmd[4:])}: exit status {r.returncode}")
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402

width, shape = sys.argv[1], sys.argv[2]
log_n = int(sys.argv[3]) if len(sys.argv) > 3 else 26
REPS = int(os.environ.get("REPS", "7"))
assert width in ("i64", "i32") and shape in ("q1", "q4", "q6", "fg")
wide = width == "i64"
dt = torch.int64 if wide else torch.int32
n = 1 << log_n
gen = torch.Generator(device="cuda")
gen.manual_seed(0x57A4)


def column(lo, hi):
    return torch.randint(lo, hi + 1, (n,), device="cuda", generator=gen).to(dt)


# (log2 build rows, payload = row >> this): the star aggregate section's four dimensions
spec = {"q1": [(11, 6)], "fg": [(11, 6)], "q6": [], "q4": [(11, 6), (11, 6), (15, 6), (20, 0)]}[shape]
hjs, dims = [], []
for lr, shr in spec:
    nr = 1 << lr
    rk = (torch.arange(nr, dtype=torch.int64, device="cuda") * 7 + 3).to(dt)    # distinct, int32-safe
    rp = (torch.arange(nr, dtype=torch.int64, device="cuda") >> shr) * 3 + 1 if wide else None
    sk = rk[torch.randint(0, nr, (n,), device="cuda", generator=gen)]
    miss = torch.rand(n, device="cuda", generator=gen) >= 0.9
    sk[miss] = -1 - torch.randint(0, 1 << 30, (int(miss.sum()),), device="cuda", generator=gen).to(dt)
    del miss
    h = hashjoin.HashJoin(0)
    h.set_strategy("global")
    h.build_table(rk, rp)
    assert h.strategy_used == "global"
    hjs.append(h)
    dims.append((h, sk, "inner", -9))

va = column(1, 9999)                          # price / revenue
if shape == "q4":
    where, vb, op = [], column(1, 999), "sub"
else:
    vb, op = column(0, 10), "mul"             # discount
    where = [(vb, 1, 3), (column(1, 50), 1, 24)]
    if shape == "q6":
        where.append((column(0, 2554), 365, 729))
fcol = column(-3, 3) if shape == "fg" else None
fact_group = [(fcol, 0, -3)] if shape == "fg" else []
group = base = None
gcap = 8
if shape == "q4":   # the two 2^11 dimensions' payloads: int64 32 values each (times 3, plus 1), int32 the row ids
    group, base = ([7, 0, -1, -1], [1, 1, 0, 0]) if wide else ([11, 0, -1, -1], [0, 0, 0, 0])
    gcap = (1 << 14) if wide else (1 << 22)

star = hashjoin.StarProbe(0)
star.reserve(n)
star.reserve_groups(gcap)
f_key, f_cnt, f_sum = (torch.empty(gcap, dtype=torch.int64, device="cuda") for _ in range(3))
c_key, c_cnt, c_sum = (torch.empty(gcap, dtype=torch.int64, device="cuda") for _ in range(3))
f_num, c_num, s_cnt = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3))
agg = hashjoin.HashJoin(0)
s_row = torch.empty(n // 4, dtype=dt, device="cuda") if shape == "fg" else None
seen = {}


def run_fused():
    star.query_into(dims, va, f_key, f_cnt, f_sum, count=f_num, where=where, expr=(op, vb), fact_group=fact_group,
                    group=group, base=base)


def expression(a, b):
    return a * b if op == "mul" else a - b


def run_composed():
    if where:
        mask = None
        for col, lo, hi in where:
            m = (col >= lo) & (col <= hi)
            mask = m if mask is None else mask & m
        idx = mask.nonzero().squeeze(1)
        cut = [(h, sk[idx], how, null) for h, sk, how, null in dims]
        v = expression(va[idx], vb[idx])
    else:
        idx, cut, v = None, dims, expression(va, vb)
    if shape == "q6":   # no dimension: no aggregate of the previous API takes it; torch's sum and the row count
        c_key[0], c_cnt[0], c_sum[0] = 0, idx.numel(), v.sum()
        c_num.fill_(1 if idx.numel() else 0)
    elif shape == "fg":   # no fact-side group field: the star probe's positions, two gathers, the aggregate
        star.probe_into(cut, None, s_row, count=s_cnt)
        if "m" not in seen:   # (the caller reads M once to size the views; the data stays the same)
            seen["m"] = int(s_cnt.item())
        rows = s_row[:seen["m"]].long()
        agg.aggregate_into((fcol[idx][rows] + 3).to(torch.int64), v[rows].to(torch.int64), c_key, c_cnt, c_sum,
                           count=c_num)
    else:
        star.aggregate_into(cut, v, c_key, c_cnt, c_sum, count=c_num, group=group, base=base)
    seen["admitted"] = n if idx is None else idx.numel()


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


res = {"fused": [], "composed": []}
for it in range(2 + REPS):
    for kind, f in (("fused", run_fused), ("composed", run_composed)):
        t = timed(f)
        if it >= 2:
            res[kind].append(t)

g = int(f_num.item())
assert 0 < g <= gcap and g == int(c_num.item()), (g, int(c_num.item()), gcap)
of, oc = torch.argsort(f_key[:g]), torch.argsort(c_key[:g])
assert torch.equal(f_key[:g][of], c_key[:g][oc]), "the fused call and the composed path differ in the groups"
assert torch.equal(f_cnt[:g][of], c_cnt[:g][oc]) and torch.equal(f_sum[:g][of], c_sum[:g][oc]), "they differ in an aggregate"
run_fused()
torch.cuda.synchronize()
plan = star.last_plan
kept = int(f_cnt[:g].sum().item())
out = {"width": width, "shape": shape, "probe_rows": n, "build_rows": [1 << s[0] for s in spec],
       "predicates": len(where), "op": op, "fact_groups": len(fact_group), "admitted_rows": seen["admitted"],
       "kept_rows": kept, "kept_share": round(kept / n, 4), "groups": g, "group_capacity": star.group_capacity,
       "reps": REPS, "plan": {k: plan[k] for k in ("launches", "grid", "tiles", "lds_mask", "lds_bytes")}}
for k, v in res.items():
    out[k + ":wall"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(out))
