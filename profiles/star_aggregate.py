#!/usr/bin/env python3
"""Whole-row time of the star aggregate against what a caller composed on the
previous API over the SAME builds, box and process: StarProbe.probe_into (the
grouped payload columns and out_row), a torch gather of the value column
through out_row, KeyCodec.pack of the payload columns and HashJoin.aggregate
(DESIGN section 5 "Star aggregate against probe + gather + pack + aggregate").
The star probe section's shapes: a fact table of 2^LOG_N rows over dimensions
of 2^11, 2^11, 2^15 and 2^20 build rows, all built under the global strategy.

  sel-first   every kind inner, one 2^11 dimension keeps ~3 % of the rows and
              comes first; the others keep ~90 % each
  sel-last    the same dimensions, the selective one last
  keep-all    every kind left (no row dropped), ~90 % hits

Two dimensions are grouped, count + sum taken:

  few    int64: the two 2^11 dimensions, whose payloads take 32 values each
         (about 10^3 groups).  int32 payloads are row ids, so two grouped
         dimensions cannot give fewer than 2^22 combinations: there ONE 2^11
         dimension is grouped (2048 groups).
  many   int64: a 2^11 dimension with distinct payloads and the 2^15 one with
         512 payload values (2^20 combinations); int32: the two 2^11
         dimensions (2^22 combinations).  About 10^6 groups where the selective
         dimension leaves 1.5 M rows.

Stream events around the whole row, 2 warm-up rounds, then REPS alternating
rounds of the fused call and the composed path; median and [min, max] in ms.
The script asserts that both give the same groups, counts and sums.

  python profiles/star_aggregate.py i64 sel-first few
  python profiles/star_aggregate.py i32 keep-all many 26
  python profiles/star_aggregate.py all        # every row, each in a child process under its own timeout,
                                               # appended to profiles/star_aggregate.jsonl
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
    with open(os.path.join(HERE, "star_aggregate.jsonl"), "a") as out:
        for width in ("i64", "i32"):
            for setting in ("sel-first", "sel-last", "keep-all"):
                for groups in ("few", "many"):
                    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), width, setting, groups] + log_n
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

width, setting, groups = sys.argv[1], sys.argv[2], sys.argv[3]
log_n = int(sys.argv[4]) if len(sys.argv) > 4 else 26
REPS = int(os.environ.get("REPS", "7"))
assert width in ("i64", "i32") and setting in ("sel-first", "sel-last", "keep-all") and groups in ("few", "many")
wide = width == "i64"
dt = torch.int64 if wide else torch.int32
n = 1 << log_n
NULL = -9
gen = torch.Generator(device="cuda")
gen.manual_seed(0x57A3)

# (log2 build rows, share of the fact rows with a partner, payload = row >> this, name); the first is the selective one
spec = [(11, 0.03 if setting != "keep-all" else 0.9, 6 if groups == "few" else 0, "a"), (11, 0.9, 6 if groups == "few" else 0, "b"),
        (15, 0.9, 6, "c"), (20, 0.9, 0, "d")]
if setting == "sel-last":
    spec = spec[1:] + spec[:1]
if wide:
    by = ("a", "b") if groups == "few" else ("b", "c")
else:
    by = ("b",) if groups == "few" else ("a", "b")
how = "left" if setting == "keep-all" else "inner"

hjs, dims, pay_cols, rows = [], [], [], []
for lr, share, shr, name in spec:
    nr = 1 << lr
    rk = (torch.arange(nr, dtype=torch.int64, device="cuda") * 7 + 3).to(dt)    # distinct, int32-safe
    rp = (torch.arange(nr, dtype=torch.int64, device="cuda") >> shr) * 3 + 1 if wide else None   # never NULL
    sk = rk[torch.randint(0, nr, (n,), device="cuda", generator=gen)]
    miss = torch.rand(n, device="cuda", generator=gen) >= share
    sk[miss] = -1 - torch.randint(0, 1 << 30, (int(miss.sum()),), device="cuda", generator=gen).to(dt)
    del miss
    h = hashjoin.HashJoin(0)
    h.set_strategy("global")
    h.build_table(rk, rp)
    assert h.strategy_used == "global"
    hjs.append(h)
    dims.append((h, sk, how, NULL))
    pay_cols.append(rp if wide else torch.arange(nr, dtype=torch.int32, device="cuda"))
val = torch.randint(-1000, 1000, (n,), device="cuda", generator=gen).to(dt)
grouped = [i for i, s in enumerate(spec) if s[3] in by]

# the codec's plan over the grouped payload columns (and the LEFT null), sealed once: both paths pack by it
kc = hashjoin.KeyCodec([dt] * len(grouped))
cols = [torch.cat([pay_cols[i], torch.tensor([NULL], dtype=dt, device="cuda")]) if how == "left" else pay_cols[i] for i in grouped]
for j, c in enumerate(cols):
    kc.observe([c if k == j else cols[k][:1].expand(c.numel()).contiguous() for k in range(len(cols))])
kc.seal()
info = kc.info()
assert info["fits"]
gshift, gbase = [-1] * 4, [0] * 4
for j, i in enumerate(grouped):
    if info["bits"][j]:
        gshift[i], gbase[i] = sum(info["bits"][j + 1:]), info["lo"][j]

star = hashjoin.StarProbe(0)
star.reserve(n)
cap = n if setting == "keep-all" else n // 8
combos = 1
for c in cols:   # the groups there can be: the product of the grouped columns' distinct values
    combos *= int(torch.unique(c).numel())
gcap = min(combos, cap)
star.reserve_groups(gcap)
f_key, f_cnt, f_sum = (torch.empty(gcap, dtype=torch.int64, device="cuda") for _ in range(3))
f_num = torch.zeros(1, dtype=torch.int64, device="cuda")
s_pay = [torch.empty(cap, dtype=dt, device="cuda") if i in grouped else None for i in range(4)]
s_row = torch.empty(cap, dtype=dt, device="cuda")
s_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
agg = hashjoin.HashJoin(0)
c_key, c_cnt, c_sum = (torch.empty(gcap, dtype=torch.int64, device="cuda") for _ in range(3))
c_num = torch.zeros(1, dtype=torch.int64, device="cuda")
m_known = {}


def run_fused():
    star.aggregate_into(dims, val, f_key, f_cnt, f_sum, count=f_num, group=gshift, base=gbase)


def run_composed():
    star.probe_into(dims, s_pay, s_row, count=s_cnt)
    if "m" not in m_known:   # (the caller reads M once to size the views; later rounds reuse it, the data being the same)
        m_known["m"] = int(s_cnt.item())
    m = m_known["m"]
    v = val[s_row[:m].long()].to(torch.int64)
    key = kc.pack([s_pay[i][:m] for i in grouped])
    agg.aggregate_into(key, v, c_key, c_cnt, c_sum, count=c_num)


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
assert int(f_cnt[:g].sum().item()) == m_known["m"]
plan = star.last_plan   # (of the composed path's probe; the fused call's is taken below)
run_fused()
torch.cuda.synchronize()
plan = star.last_plan
out = {"width": width, "setting": setting, "groups_setting": groups, "probe_rows": n,
       "build_rows": [1 << s[0] for s in spec], "shares": [s[1] for s in spec], "grouped": grouped, "gshift": gshift,
       "kept_rows": m_known["m"], "kept_share": round(m_known["m"] / n, 4), "groups": g,
       "group_capacity": star.group_capacity, "composed_aggregate": agg.strategy_used, "reps": REPS,
       "plan": {k: plan[k] for k in ("launches", "grid", "tiles", "lds_mask", "lds_bytes")}}
for k, v in res.items():
    out[k + ":wall"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
print(json.dumps(out))
