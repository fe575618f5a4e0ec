#!/usr/bin/env python3
"""Point-to-point sweep: one-way ncclSend / ncclRecv at 2 ranks for 8 B - 256
MiB (x4 steps) with 1, 2, 4 and 8 parts per peer, the same sizes as
ncclBroadcast from rank 0 on as many ring channels as the send has parts
(five repeats: their min-max spread is the margin a send row is read
against), and ncclAllToAll at 4 and 8 ranks.  Every row is byte-checked.

    python tools/p2p_sweep.py [--min-bytes N] [--max-bytes N] [--steps K] [--skip send,sendparts,bcast,a2a]

(--skip sendparts drops the 1 / 2 / 4-part send rows and keeps the comparison
run.)  The P2P knobs of the environment (NCCL_P2P_NVL_CHUNKSIZE, ...) reach the
ranks unchanged.

The parent spawns the rank processes (bench.py's launcher; ranks share a GPU
when the box has fewer than ranks) and prints one JSON line per row: us per
call (max over ranks) and GB/s of payload.  Measurement tool, not product
code."""
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


MIN_BYTES = int(arg("--min-bytes", 8))
MAX_BYTES = int(arg("--max-bytes", 256 << 20))
STEPS = int(arg("--steps", 10))
SKIP = set(arg("--skip", "").split(","))
BCAST_PARTS = 8


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
    jobs = []
    if "send" not in SKIP and "sendparts" not in SKIP:
        jobs += [(2, "send", {"VCCL_P2P_PARTS": str(p)}) for p in (1, 2, 4)]
    # parts = broadcast channels, one comm, one run: the comparison rows
    if "send" not in SKIP or "bcast" not in SKIP:
        jobs.append((2, "send+bcast" if "bcast" not in SKIP else "send",
                     {"VCCL_P2P_PARTS": str(BCAST_PARTS), "VCCL_NCHANNELS": str(BCAST_PARTS)}))
    if "a2a" not in SKIP:
        jobs += [(n, "a2a", {}) for n in (4, 8)]
    rc = 0
    for n, mode, extra in jobs:
        env = dict(os.environ)
        env.pop("WORLD_SIZE", None)
        env.update(extra)
        env["P2P_SWEEP_MODE"] = mode
        env.setdefault("VCCL_SPIN_TIMEOUT_S", "30")
        plan = bench.rank_launch_plan(["--gpus", str(n)] + sys.argv[1:], env, script=os.path.abspath(__file__))
        rc = rc or bench._spawn_ranks(plan)
    sys.exit(rc)


def timed(fn, steps, sync):
    import torch
    for _ in range(2):
        fn()
    sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    sync()
    return a.elapsed_time(b) * 1e3 / steps


def child():
    import torch
    import torch.distributed as dist

    from vccl_amd import nccl
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(rank % torch.cuda.device_count())
    if world > torch.cuda.device_count():
        os.environ["VCCL_ALLOW_SHARED_DEVICE"] = "1"
    dist.init_process_group("gloo")
    obj = [nccl.unique_id_to_bytes(nccl.get_unique_id()) if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    comm = nccl.Comm.init_rank(world, nccl.unique_id_from_bytes(obj[0]), rank)
    sp = torch.cuda.current_stream().cuda_stream
    mode = os.environ["P2P_SWEEP_MODE"]
    parts = int(os.environ.get("VCCL_P2P_PARTS", 4))
    U8 = nccl.ncclUint8

    def pay(nb, src, dst):
        g = torch.Generator(device="cpu").manual_seed(nb % 65521 + 131 * src + dst)
        head = torch.randint(0, 256, (min(nb, 1 << 20),), dtype=torch.uint8, generator=g).cuda()
        return head.repeat(-(-nb // head.numel()))[:nb].contiguous()

    def row(**kw):
        us = torch.tensor([kw["us"]], dtype=torch.float64)
        ok = torch.tensor([1 if kw["ok"] else 0])
        dist.all_reduce(us, op=dist.ReduceOp.MAX)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        kw.update(us=round(us.item(), 2), ok=bool(ok.item()))
        kw["gbs"] = round(kw["bytes"] / (kw["us"] * 1e3), 3) if kw["us"] > 0 else 0.0
        if rank == 0:
            print(json.dumps(kw), flush=True)
        return kw["ok"]

    good = True
    if mode.startswith("send"):
        for nb in sizes(MIN_BYTES, MAX_BYTES):
            src = pay(nb, 0, 1)
            dst = torch.full((nb,), 0xA5, dtype=torch.uint8, device="cuda")
            if rank == 0:
                fn = lambda: comm.send(src.data_ptr(), nb, U8, 1, sp)  # noqa: E731
            else:
                fn = lambda: comm.recv(dst.data_ptr(), nb, U8, 0, sp)  # noqa: E731
            us = timed(fn, STEPS, torch.cuda.synchronize)
            ok = rank == 0 or torch.equal(dst, src)
            good &= row(op="send", ranks=world, parts=parts, bytes=nb, us=us, ok=ok)
            if mode.endswith("bcast"):
                for rep in range(5):
                    out = torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda")
                    fn = lambda: comm.broadcast(src.data_ptr(), out.data_ptr(), nb, U8, 0, sp)  # noqa: E731
                    us = timed(fn, STEPS, torch.cuda.synchronize)
                    good &= row(op="broadcast", ranks=world, channels=comm.n_channels(), rep=rep, bytes=nb, us=us,
                                ok=torch.equal(out, src))
            del src, dst
    else:
        for nb in sizes(max(MIN_BYTES, 1 << 10), min(MAX_BYTES, 16 << 20)):
            send = torch.cat([pay(nb, rank, p) for p in range(world)])
            out = torch.full((nb * world,), 0xA5, dtype=torch.uint8, device="cuda")
            fn = lambda: comm.all_to_all(send.data_ptr(), out.data_ptr(), nb, U8, sp)  # noqa: E731
            us = timed(fn, STEPS, torch.cuda.synchronize)
            ok = torch.equal(out, torch.cat([pay(nb, p, rank) for p in range(world)]))
            good &= row(op="all_to_all", ranks=world, parts=parts, bytes=nb * (world - 1), bytes_per_pair=nb, us=us,
                        ok=ok)
            del send, out
    err = comm.async_error()
    comm.destroy()
    dist.destroy_process_group()
    sys.exit(0 if good and not err else 1)


if __name__ == "__main__":
    if "RANK" in os.environ and "P2P_SWEEP_MODE" in os.environ:
        child()
    else:
        parent()
