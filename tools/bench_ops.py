"""Throughput of the secondary operators: selection and the
nested-loop.mlir row join, on one MI355X, inputs resident in HBM.  One JSON
line per case (HIP-event timing on the current stream, median of 10 after 2
warm-ups); algorithmic bytes as stated in DESIGN.md.

usage: python tools/bench_ops.py  [> profiles/r01_ops_bench.jsonl]
       python tools/bench_ops.py expand [a] [b] [c]  [> profiles/expand_probe.jsonl]

The `expand` op ("Expand probe") times hj_dev_expand_* on
  a: 2^26 x 2^26 int64 PK-FK, hit fraction 1.0, AUTO (radix);
  b: 2^20 x 2^24 int64 PK-FK on the global table;
  c: 10M x 10M i32 keys uniform in [1, 100k] (~1e9 entries, ~100 per row)
against two yardsticks on the same inputs in the same process: the payload-only
positional lookup (the one-partner floor) and what a caller composes without
it -- the inner probe with S.pay = the row index, torch.sort on the S column
and a gather of the R column.  Rounds alternate the variants; median [min,
max] of the timed rounds in ms, device events (`wall`) and the library's own
phase events (`partition`, `rest`: RADIX's [4] and [5]).  The count form
(partition, counts, scan) is timed as a variant of its own, so the fill is
full - count form.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402
from hashjoin._lib import check, lib  # noqa: E402

HBM = 8000.0


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def expand_op(shape, reps, warm):
    if shape == "a":
        nr, ns, strategy, wide = 1 << 26, 1 << 26, "auto", True
    elif shape == "b":
        nr, ns, strategy, wide = 1 << 20, 1 << 24, "global", True
    else:
        nr, ns, strategy, wide = 10_000_000, 10_000_000, "auto", False
    if wide:
        rk, rp, sk, _ = hashjoin.gen_pkfk(0x5EED, nr, ns, 1.0)
    else:
        rk, rp = hashjoin.gen_uniform_i32(0x5EED, 1, 1, 100_000, nr), None
        sk = hashjoin.gen_uniform_i32(0x5EED, 2, 1, 100_000, ns)
    dt = sk.dtype
    hj = hashjoin.HashJoin(0)
    hj.set_strategy(strategy)
    hj.set_timing(True)
    hj.probe_hint(ns)
    hj.build_table(rk, rp)
    build_ms = hj.last_timing()["build"]
    off, m = hj.count_expand(sk)
    hj.reserve_expand(ns, 64 if wide else 32)
    out_r = torch.empty(m, dtype=dt, device="cuda")
    look_r = torch.empty(ns, dtype=dt, device="cuda")
    in_r, in_s = torch.empty(m, dtype=dt, device="cuda"), torch.empty(m, dtype=dt, device="cuda")
    rows = torch.arange(ns, dtype=torch.int64, device="cuda") if wide else None
    res, keep = {}, {}

    def one(kind):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if kind == "expand":
            hj.probe_expand(sk, off, out_r)
        elif kind == "expand-count-form":
            hj.probe_expand(sk, off, None)
        elif kind == "lookup-payload-only":
            hj.probe_lookup(sk, look_r)
        else:   # inner probe carrying the row index, sort by it, gather the R column
            hj.probe_relation(sk, rows, in_r, in_s)
            order = torch.sort(in_s, stable=False).indices
            keep["composed"] = in_r[order]
        e1.record()
        e1.synchronize()
        t = hj.last_timing()
        if kind == "expand":
            keep["kernel"] = hj.join_kernel
        return {"wall": e0.elapsed_time(e1), "partition": t["probe_partition"], "rest": t["probe_join"],
                "probe": t["probe"]}

    kinds = ("expand", "expand-count-form", "lookup-payload-only", "inner+sort+gather")
    for it in range(warm + reps):
        for kind in kinds:
            t = one(kind)
            if it >= warm:
                for k, v in t.items():
                    res.setdefault(kind + ":" + k, []).append(v)
    # the composition and the expand hold the same partners per probe row (the same array when the build is unique)
    seg = torch.repeat_interleave(torch.arange(ns, device="cuda"), off[1:] - off[:-1], output_size=m)
    same = bool(torch.equal(keep["composed"], out_r)) if wide else None
    sums = bool(torch.equal(torch.zeros(ns, dtype=torch.int64, device="cuda").index_add_(0, seg, out_r.long()),
                            torch.zeros(ns, dtype=torch.int64, device="cuda").index_add_(
                                0, seg, keep["composed"].long())))
    out = {"op": "expand", "shape": shape, "dtype": str(dt).replace("torch.", ""), "strategy": hj.strategy_used,
           "join_kernel": keep["kernel"], "build_rows": nr, "probe_rows": ns, "entries": m, "reps": reps, "warm": warm,
           "build_ms": round(build_ms, 3), "equals_composition": same, "segment_sums_equal": sums,
           "device": torch.cuda.get_device_name(0)}
    for k, v in res.items():
        out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(out), flush=True)
    hj.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "expand":
        reps, warm = int(os.environ.get("REPS", "7")), int(os.environ.get("WARM", "2"))
        for shape in (sys.argv[2:] or ["a", "b", "c"]):
            expand_op(shape, reps, warm)
            torch.cuda.empty_cache()
        return
    hj = hashjoin.HashJoin(0)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    # selection: 2^28 f32, keep ~50 %
    n = 1 << 28
    x = torch.rand(n, device="cuda", dtype=torch.float32)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    for sel in (0.01, 0.5, 0.99):
        ms = timed(lambda: check(lib.hj_dev_select_f32(hj._ctx, x.data_ptr(), n, 0, sel, out.data_ptr(), None, n,
                                                       cnt.data_ptr(), st), "select"))
        m = int(cnt.item())
        byts = n * 4 * 2 + m * 4   # count pass + write pass read the input; survivors written once
        print(json.dumps({"op": "select_f32 lt", "n": n, "selectivity": round(m / n, 4), "ms": round(ms, 4),
                          "elements_per_s": round(n / ms * 1e3, 1), "algorithmic_GBps": round(byts / ms / 1e6, 1),
                          "frac_hbm": round(byts / ms / 1e6 / HBM, 4)}), flush=True)
    del x, out
    # nested-loop rows: X 2^24 x 4 cols, Y 2^20 x 3 cols, keys in [0, 2^20): ~16 matches... keep PK-FK-like
    rx, ry = 1 << 24, 1 << 20
    X = torch.randint(-(1 << 30), 1 << 30, (rx, 4), dtype=torch.int32, device="cuda")
    Y = torch.randint(-(1 << 30), 1 << 30, (ry, 3), dtype=torch.int32, device="cuda")
    Y[:, 0] = torch.randperm(ry, device="cuda", dtype=torch.int32)   # unique inner keys
    X[:, 0] = torch.randint(0, ry, (rx,), dtype=torch.int32, device="cuda")
    oc = 4 + 3 - 1
    outr = torch.empty((rx, oc), dtype=torch.int32, device="cuda")
    args = (X.data_ptr(), rx, 4, 4, Y.data_ptr(), ry, 3, 3)
    ms = timed(lambda: check(lib.hj_dev_join_rows_i32(hj._ctx, *args, outr.data_ptr(), oc, rx, cnt.data_ptr(), st),
                             "rows"))
    m = int(cnt.item())
    byts = rx * 16 + ry * 12 + m * oc * 4 + m * (16 + 12)   # tables read + rows written + row gathers
    print(json.dumps({"op": "join_rows_i32 (nested-loop.mlir)", "X": [rx, 4], "Y": [ry, 3], "rows": m,
                      "ms": round(ms, 4), "rows_per_s": round(m / ms * 1e3, 1),
                      "algorithmic_GBps": round(byts / ms / 1e6, 1)}), flush=True)
    del X, Y, outr
    # out-of-core: host-resident 2^28 x 2^28 PK-FK, PCIe Gen5 x16 between
    import time
    NR = NS = 1 << 28
    rk, rp, sk, sp = hashjoin.gen_pkfk(0x5EED, NR, NS)
    h = [t.cpu().numpy() for t in (rk, rp, sk, sp)]
    del rk, rp, sk, sp
    torch.cuda.empty_cache()
    for budget, name in ((0, "R resident, S streamed"), (8 << 30, "8 GiB budget: routed into groups")):
        hj.join_host(*h, device_budget=budget)   # warm-up (page-locking, workspaces)
        t0 = time.perf_counter()
        o_r, o_s = hj.join_host(*h, device_budget=budget)
        dt = time.perf_counter() - t0
        m = len(o_r)
        assert m == NS
        print(json.dumps({"op": "join_host_ooc_i64", "mode": name, "R_rows": NR, "S_rows": NS, "s": round(dt, 4),
                          "probe_tuples_per_s": round(NS / dt, 1),
                          "pcie_bytes_min": (NR + NS) * 16 + m * 16,
                          "pcie_GBps_min": round(((NR + NS) * 16 + m * 16) / dt / 1e9, 1)}), flush=True)
    hj.close()


if __name__ == "__main__":
    main()
