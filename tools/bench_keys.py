"""Key packing against the flat copy on one MI355X ("Key
packing against the flat copy"): observe, pack and pack_tuples of two int64
columns, each beside hj_dev_stream_copy(HJ_COPY_FLAT) moving the same number
of bytes (read + written) on the same box, and join_on beside join on keys
packed beforehand.  Rounds alternate an operation and its copy; one JSON line
per case with the median [min, max] of the timed rounds in ms (device events
for the kernels; a host clock around the synchronising join calls).

usage: python tools/bench_keys.py [log2_rows=28] [log2_join_rows=26] [rounds=9]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlir-hashjoin_amd"))
import torch  # noqa: E402

import hashjoin  # noqa: E402


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def rounds_of(variants, rounds, warm, clock):
    """{name: [ms per timed round]}: every round runs each variant once, in order."""
    ts = {k: [] for k in variants}
    for r in range(warm + rounds):
        for k, fn in variants.items():
            t = clock(fn)
            if r >= warm:
                ts[k].append(t)
    return ts


def stat(ts):
    return {"ms": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def kernels(lg, rounds):
    n = 1 << lg
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(0, 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g)
    b = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g)
    pay = torch.arange(n, dtype=torch.int64, device="cuda")
    out = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    # the copies' buffers: up to 5n words each way (pack_tuples moves 3n in + 2n out)
    src = torch.randint(0, 1 << 62, (5 * n // 2,), dtype=torch.int64, device="cuda", generator=g)
    dst = torch.empty_like(src)
    kc = hashjoin.KeyCodec([torch.int64, torch.int64])
    kc.observe([a, b])
    kc.seal()
    info = kc.info()
    assert info["fits"], info

    ko = hashjoin.KeyCodec([torch.int64, torch.int64])   # a codec of its own: observing again needs a reset

    def observe():
        ko.reset()
        ko.observe([a, b])

    # the other paths: unpack; int32 / int64 / int32 columns (4 rows per lane); columns 8 bytes off a 16-byte
    # boundary (the element path)
    keys = kc.pack([a, b])
    ua, ub = torch.empty_like(a), torch.empty_like(b)
    a32 = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int32, device="cuda", generator=g)
    c32 = torch.randint(0, 256, (n,), dtype=torch.int32, device="cuda", generator=g)
    k3 = hashjoin.KeyCodec([torch.int32, torch.int64, torch.int32])
    k3.observe([a32, b, c32])
    k3.seal()
    assert k3.info()["fits"]
    am, bm = (torch.empty(n + 1, dtype=torch.int64, device="cuda")[1:] for _ in range(2))
    am.copy_(a)
    bm.copy_(b)

    cases = {"observe": (observe, 16 * n), "pack": (lambda: kc.pack([a, b], out=out), 24 * n),
             "pack_tuples": (lambda: kc.pack_tuples([a, b], pay, out=out), 40 * n),
             "unpack": (lambda: kc.unpack(keys, outs=[ua, ub]), 24 * n),
             "pack_i32_i64_i32": (lambda: k3.pack([a32, b, c32], out=out), 24 * n),
             "pack_misaligned": (lambda: kc.pack([am, bm], out=out), 24 * n)}
    for name, (fn, nbytes) in cases.items():
        words = nbytes // 16   # the copy reads and writes half of the bytes each
        ts = rounds_of({name: fn, "copy": lambda: hashjoin.stream_copy(src[:words], dst[:words], "flat")}, rounds, 2,
                       ev_ms)
        op, cp = stat(ts[name]), stat(ts["copy"])
        print(json.dumps({"case": name, "rows": n, "bytes": nbytes, **op, "tb_per_s": round(nbytes / op["ms"] / 1e9, 3),
                          "copy": cp, "copy_tb_per_s": round(nbytes / cp["ms"] / 1e9, 3),
                          "ratio_to_copy": round(op["ms"] / cp["ms"], 3)}), flush=True)
    for c in (kc, ko, k3):
        c.close()


def join(lg, rounds):
    n = 1 << lg
    rk, rp, sk, sp = hashjoin.gen_pkfk(0x5EED, n, n, 1.0)
    split = lambda k: [k >> 32, k & 0xFFFFFFFF]   # noqa: E731  (two int64 columns, 32 + 32 bits)
    rcols, scols = split(rk), split(sk)
    del rk, sk
    hj = hashjoin.HashJoin(0)
    kc = hashjoin.KeyCodec([torch.int64, torch.int64])
    kc.observe(rcols); kc.observe(scols); kc.seal()
    prk, psk = kc.pack(rcols), kc.pack(scols)
    info = kc.info()
    kc.close()
    m = {}

    def on():
        m["on"] = hj.join_on(rcols, rp, scols, sp)[0].numel()

    def packed():
        m["packed"] = hj.join(prk, rp, psk, sp)[0].numel()

    ts = rounds_of({"join_on": on, "join_packed": packed}, rounds, 2, host_ms)
    assert m["on"] == m["packed"] == n, m
    a, b = stat(ts["join_on"]), stat(ts["join_packed"])
    print(json.dumps({"case": "join_on", "rows": [n, n], "result_rows": m["on"], "join_on": a, "join_packed": b,
                      "difference_ms": round(a["ms"] - b["ms"], 3), "plan_bits": info["bits"]}), flush=True)
    hj.close()


if __name__ == "__main__":
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    lgj = int(sys.argv[2]) if len(sys.argv) > 2 else 26
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    assert torch.cuda.is_available(), "needs a HIP device"
    kernels(lg, rounds)
    torch.cuda.empty_cache()
    join(lgj, rounds)
