#!/usr/bin/env python3
"""Times of the key filter (hj.h "Key filter") on one box, one process, inputs
resident: 2 warm-up rounds, then REPS (default 7) timed between stream events;
one JSON line per measurement with the median and [min, max] in ms.

  python tools/bench_filter.py insert            # insert at 2^20 and 2^24 keys (the library's form)
  python tools/bench_filter.py apply [26 28]     # apply (PASS, all outputs) against a flat stream copy of the
                                                 # same bytes and against hj_dev_select_i64, filters of 2 / 32 / 512 MiB
  python tools/bench_filter.py join [24 28]      # filtered_join against join at 2^a x 2^b, frac 1.0 / 0.5 / 0.1 / 0.01

The two forms of the insert and of the apply are timed by
mlir-hashjoin_amd/micro/filter_micro.hip."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402
from hashjoin import _lib  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))


def timed(run, before=None):
    ms = []
    for it in range(2 + REPS):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_insert():
    for lg in (20, 24):
        n = 1 << lg
        rk = hashjoin.gen_pkfk(0x5EED, n, 1)[0]
        f = hashjoin.KeyFilter(n)
        emit(op="clear", filter_bytes=f.nblocks * 32, ms=timed(f.clear))
        emit(op="insert", keys=n, filter_bytes=f.nblocks * 32, ms=timed(lambda: f.insert(rk), f.clear))
        f.close()


def bench_apply(lgs):
    hj = hashjoin.HashJoin(0)
    for lg in lgs:
        n = 1 << lg
        outs = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3)]
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        for mib in (2, 32, 512):
            f = hashjoin.KeyFilter(nblocks=(mib << 20) // 32)
            nr = f.nblocks * 16                                   # 16 bits per key
            rk, _, sk, sp = hashjoin.gen_pkfk(0x5EED, nr, n, 0.5)
            f.clear()
            f.insert(rk)
            f.reserve(n)
            t = timed(lambda: f.apply_into(sk, sp, "pass", outs[0], outs[1], outs[2], count=cnt))
            kept = int(cnt.item())
            emit(op="apply", rows=n, filter_bytes=f.nblocks * 32, build_keys=nr, kept=kept, ms=t)
            emit(op="apply-count", rows=n, filter_bytes=f.nblocks * 32, ms=timed(lambda: f.apply_into(sk, count=cnt)))
            f.close()
            if mib == 32:
                # the same bytes through one flat copy: 16 B read per row, 24 B written per row kept
                words = (16 * n + 24 * kept) // 2 // 16 * 2
                src, dst = (torch.empty(words, dtype=torch.int64, device="cuda") for _ in range(2))
                emit(op="stream-copy-flat", rows=n, bytes_each_way=words * 8,
                     ms=timed(lambda: hashjoin.stream_copy(src, dst, "flat")))
                del src, dst
                # hj_dev_select_i64 keeping as many rows (values and row indices out): the payloads are the row ids
                thr = kept
                sel = lambda: _lib.check(_lib.lib.hj_dev_select_i64(  # noqa: E731
                    hj._ctx, sp.data_ptr(), n, 0, thr, outs[0].data_ptr(), outs[1].data_ptr(), n, cnt.data_ptr(),
                    torch.cuda.current_stream().cuda_stream))
                t = timed(sel)
                emit(op="select_i64", rows=n, kept=int(cnt.item()), ms=t)
            del rk, sk, sp
    hj.close()


def bench_join(lr, ls):
    nr, ns = 1 << lr, 1 << ls
    hj = hashjoin.HashJoin(0)
    for frac in (1.0, 0.5, 0.1, 0.01):
        rk, rp, sk, sp = hashjoin.gen_pkfk(0x5EED, nr, ns, frac)
        res = {}
        a = hj.join(rk, rp, sk, sp)
        b = hj.filtered_join(rk, rp, sk, sp)
        assert a[0].numel() == b[0].numel()
        m, kept = a[0].numel(), hj.last_filtered[1]
        del a, b
        res["join"] = timed(lambda: hj.join(rk, rp, sk, sp, capacity=max(m, 1)))
        res["filtered_join"] = timed(lambda: hj.filtered_join(rk, rp, sk, sp, capacity=max(m, 1)))
        emit(op="join", build=nr, probe=ns, frac=frac, pairs=m, kept=kept, strategy=hj.strategy_used, ms=res)
        del rk, rp, sk, sp
    hj.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "insert"
    args = [int(a) for a in sys.argv[2:]]
    if what == "insert":
        bench_insert()
    elif what == "apply":
        bench_apply(args or [26, 28])
    elif what == "join":
        bench_join(*(args or [24, 28]))
    else:
        sys.exit(__doc__)
