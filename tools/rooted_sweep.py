#!/usr/bin/env python3
"""Rooted-collective sweep: ncclBroadcast and ncclReduce (f32 sum) from / to
rank 0 for 8 B - 128 KiB (x4 steps) at 2, 4 and 8 ranks, the ring and the
one-hop LL path alternating on ONE communicator (vcclCommSetAlgo), every row
checked.  Per row: min and median us per call over --steps calls (default 50)
after warm-up, each call timed by its own event pair, the max over ranks.

    python tools/rooted_sweep.py [--min-bytes N] [--max-bytes N] [--steps K] [--ranks 2,4,8] [--direct]

--direct: the ring against the two-hop direct path instead,
128 KiB - 64 MiB by default, 20 calls per row, VCCL_DIRECT_ROOTED_THRESHOLD set
to --max-bytes and VCCL_LL_ROOTED_THRESHOLD left unset.

The parent spawns the rank processes (bench.py's launcher; ranks share a GPU
when the box has fewer than ranks — then the rows are rehearsal rows: LL
latency between processes time-slicing one GPU is bimodal)
with VCCL_LL_ROOTED_THRESHOLD set to --max-bytes, and prints one JSON line per
row.  Measurement tool, not product code."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    for i, a in enumerate(sys.argv):
        if a == name and i + 1 < len(sys.argv):
            return sys.argv[i + 1]
    return default


DIRECT = "--direct" in sys.argv
MIN_BYTES = int(arg("--min-bytes", 128 << 10 if DIRECT else 8))
MAX_BYTES = int(arg("--max-bytes", 64 << 20 if DIRECT else 128 << 10))
STEPS = max(20, int(arg("--steps", 20))) if DIRECT else max(50, int(arg("--steps", 50)))
RANKS = [int(x) for x in arg("--ranks", "2,4,8").split(",")]
WARMUP = 5


def sizes(lo, hi):
    out, s = [], lo
    while s <= hi:
        out.append(s)
        s *= 4
    if out[-1] != hi and hi >= lo:
        out.append(hi)
    return out


def parent():
    import bench
    rc = 0
    for n in RANKS:
        env = dict(os.environ)
        env.pop("WORLD_SIZE", None)
        env.pop("VCCL_LL_ROOTED_THRESHOLD", None)
        env.pop("VCCL_DIRECT_ROOTED_THRESHOLD", None)
        env["VCCL_DIRECT_ROOTED_THRESHOLD" if DIRECT else "VCCL_LL_ROOTED_THRESHOLD"] = str(MAX_BYTES)
        env["ROOTED_SWEEP_CHILD"] = "1"
        env.setdefault("VCCL_SPIN_TIMEOUT_S", "30")
        plan = bench.rank_launch_plan(["--gpus", str(n)] + sys.argv[1:], env, script=os.path.abspath(__file__))
        rc = rc or bench._spawn_ranks(plan)
    sys.exit(rc)


def timed(fn, sync):
    """us of each of STEPS calls after WARMUP, one event pair per call."""
    import torch
    for _ in range(WARMUP):
        fn()
    sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    sync()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)


def child():
    import torch
    import torch.distributed as dist

    from vccl_amd import nccl
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(rank % torch.cuda.device_count())
    shared = world > torch.cuda.device_count()
    if shared:
        os.environ["VCCL_ALLOW_SHARED_DEVICE"] = "1"
    dist.init_process_group("gloo")
    obj = [nccl.unique_id_to_bytes(nccl.get_unique_id()) if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    comm = nccl.Comm.init_rank(world, nccl.unique_id_from_bytes(obj[0]), rank)
    sp = torch.cuda.current_stream().cuda_stream
    U8, F32 = nccl.ncclUint8, nccl.ncclFloat32

    def row(**kw):
        t = torch.tensor([kw["min_us"], kw["median_us"]], dtype=torch.float64)
        ok = torch.tensor([1 if kw["ok"] else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        kw.update(min_us=round(t[0].item(), 2), median_us=round(t[1].item(), 2), ok=bool(ok.item()))
        if rank == 0:
            print(json.dumps(kw), flush=True)
        return kw["ok"]

    good = True
    for nb in sizes(MIN_BYTES, MAX_BYTES):
        cnt = nb // 4
        g = torch.Generator(device="cpu").manual_seed(nb)
        pay = torch.randint(0, 256, (nb,), dtype=torch.uint8, generator=g).cuda()
        x = ((torch.arange(cnt) * 7 + 13 * rank) % 11 + rank).float().cuda()  # small integers: any fold order is exact
        want = sum(((torch.arange(cnt) * 7 + 13 * r) % 11 + r).float() for r in range(world)).cuda()
        for op in ("broadcast", "reduce"):
            for path in ("ring", "direct" if DIRECT else "ll"):  # alternating on the one comm
                comm.set_algo(path)
                coll, count, dt = (3, nb, U8) if op == "broadcast" else (4, cnt, F32)
                algo = comm.coll_algo(coll, count, dt)
                if op == "broadcast":
                    out = torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda")
                    fn = lambda: comm.broadcast(pay.data_ptr() if rank == 0 else 0, out.data_ptr(), nb, U8, 0, sp)  # noqa: E731
                else:
                    out = torch.full((cnt,), float("nan"), device="cuda")
                    fn = lambda: comm.reduce(x.data_ptr(), out.data_ptr() if rank == 0 else 0, cnt, F32, nccl.ncclSum, 0, sp)  # noqa: E731
                us = timed(fn, torch.cuda.synchronize)
                ok = algo == path and (torch.equal(out, pay) if op == "broadcast" else rank != 0 or torch.equal(out, want))
                good &= row(op=op, ranks=world, shared_gpu=shared, path=algo, bytes=nb, calls=STEPS, min_us=us[0],
                            median_us=us[len(us) // 2], ok=ok)
    comm.set_algo(None)
    err = comm.async_error()
    comm.destroy()
    dist.destroy_process_group()
    sys.exit(0 if good and not err else 1)


if __name__ == "__main__":
    if "RANK" in os.environ and "ROOTED_SWEEP_CHILD" in os.environ:
        child()
    else:
        parent()
