"""Single-rank RCCL worker for tests/test_gpu_filter.py (run as its own
process: the process group is created before anything touches the GPU).

distributed_join(prefilter=16, replicate_max_rows=0) over a world-size-1 "nccl"
(= RCCL) group against the unfiltered call and the oracle, plain and folded;
phases["filtered"] against the numpy model's survivor count."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "mlir-hashjoin_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", sys.argv[1] if len(sys.argv) > 1 else "29643")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    import numpy as np
    import filter_cases as FC
    import hashjoin
    from hashjoin.dist import distributed_join
    from oracle import pyoracle as O

    hj = hashjoin.HashJoin(0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rk, rp, sk, sp = O.gen_pkfk_i64(45, 30000, 50000, 0.25)
    er, es = O.nested_loop_i64(rk, rp, sk, sp)
    keep = int(FC.test(FC.build(rk, FC.blocks_for(len(rk), 16)), sk).sum())
    ok = 0
    for mode, kw in (("shuffle", dict(replicate_max_rows=0)),
                     ("shuffle_p2p_parts", dict(replicate_max_rows=0, max_rows=4093, self_p2p=True, s_parts=2)),
                     ("folded", dict(replicate_max_rows=0, route_bits=4, self_p2p=True))):
        base = distributed_join(hj, d(rk), d(rp), d(sk), d(sp), **kw)
        ph = {}
        got = distributed_join(hj, d(rk), d(rp), d(sk), d(sp), phases=ph, prefilter=16, **kw)
        torch.cuda.synchronize()
        for o_r, o_s in (base, got):
            assert O.same_multiset(o_r.cpu().numpy(), o_s.cpu().numpy(), er, es), (mode, o_r.numel(), len(er))
        assert ph["mode"] == "shuffle" and ph["filtered"] == (len(sk), keep) and ph["rows"] == (len(rk), keep)
        assert len(er) <= keep < len(sk) // 3
        assert ph["s_route"].elapsed_time(ph["s_filter"]) >= 0.0 and ph["s_filter"].elapsed_time(ph["routed"]) >= 0.0
        ok += 1
        print(f"ok {mode} M={len(er)} kept={keep} of {len(sk)}", flush=True)
    ph = {}
    got = distributed_join(hj, d(rk), d(rp), d(sk), d(sp), phases=ph, prefilter=16, replicate_max_rows=1 << 21)
    assert ph["mode"] == "replicate" and "filtered" not in ph
    assert O.same_multiset(got[0].cpu().numpy(), got[1].cpu().numpy(), er, es)
    hj.close()
    dist.destroy_process_group()
    print(f"RCCL_FILTER_WORKER_OK {ok + 1}", flush=True)


if __name__ == "__main__":
    main()
