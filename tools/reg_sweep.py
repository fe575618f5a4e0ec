#!/usr/bin/env python3
"""Zero-copy sweep: ncclAllReduce / ncclReduceScatter / ncclAllGather (f32 sum;
bytes) for 64 KiB - 1 GiB of bucket (x4 steps) at 4 and 8 ranks, on ONE
communicator created with VCCL_REG_THRESHOLD set, three ways per row:

  zero_copy   registered buffers: the zero-copy kernel (device/direct_reg.hpp)
  fallback    unregistered buffers: the same kernel's fallback, the staged
              direct path behind one negotiation epoch
  off         the threshold switched off (vcclCommSetRegThreshold 0): the
              comm's own choice for the size, which is the behaviour without
              the feature

Every timed output is checked against the exact value, and the path of every
row is confirmed by vcclCommRegStats.  Per row: min and median us per call over
--steps calls (default 20) after warm-up, each call timed by its own event
pair, the max over ranks.

    python tools/reg_sweep.py [--min-bytes N] [--max-bytes N] [--steps K] [--ranks 4,8]

With --a2a the sweep is ncclAllToAll (u8) instead, on a communicator created
with VCCL_REG_A2A_THRESHOLD set: 64 KiB - 64 MiB per pair (x4 steps), 10 timed
calls after 2 warm-ups, the same three modes (fallback: the per-peer FIFOs
behind one negotiation launch; off: vcclCommSetRegA2aThreshold 0), every row
checked and its path confirmed by vcclCommRegA2aStats
(profiles/reg_sweep/reg_a2a_sweep.jsonl).

With --rooted the sweep is ncclBroadcast (u8) and ncclReduce (f32 sum) from / to
rank 0, on a communicator created with VCCL_REG_ROOTED_THRESHOLD set: 64 KiB -
256 MiB (x4 steps), the same three modes (fallback: the staged direct rooted
part behind one negotiation epoch; off: vcclCommSetRegRootedThreshold 0), every
row checked and its path confirmed by vcclCommRegRootedStats
(profiles/reg_sweep/reg_rooted_sweep.jsonl).

The parent spawns the rank processes (bench.py's launcher; ranks share a GPU
when the box has fewer than ranks — then the rows are rehearsal rows: they show
HBM traffic and phase count, and nothing about xGMI) and prints one JSON line
per row.  Measurement tool, not product code."""
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


A2A = "--a2a" in sys.argv
ROOTED = "--rooted" in sys.argv
MIN_BYTES = int(arg("--min-bytes", 64 << 10))
MAX_BYTES = int(arg("--max-bytes", 64 << 20 if A2A else 256 << 20 if ROOTED else 1 << 30))
STEPS = max(5, int(arg("--steps", 10 if A2A else 20)))
RANKS = [int(x) for x in arg("--ranks", "4,8").split(",")]
WARMUP = 2 if A2A else 3
THRESH = 32 << 10


def sizes(lo, hi):
    out, s = [], lo
    while s <= hi:
        out.append(s)
        s *= 4
    return out


def parent():
    import bench
    rc = 0
    for n in RANKS:
        env = dict(os.environ)
        env.pop("WORLD_SIZE", None)
        env["REG_SWEEP_CHILD"] = "1"
        env["VCCL_REG_A2A_THRESHOLD" if A2A else "VCCL_REG_ROOTED_THRESHOLD" if ROOTED else "VCCL_REG_THRESHOLD"] = \
            str(THRESH)
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
    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(rank % torch.cuda.device_count())
    shared = n > torch.cuda.device_count()
    if shared:
        os.environ["VCCL_ALLOW_SHARED_DEVICE"] = "1"
    dist.init_process_group("gloo")
    obj = [nccl.unique_id_to_bytes(nccl.get_unique_id()) if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(obj[0]), rank)
    sp = torch.cuda.current_stream().cuda_stream
    F32, U8 = nccl.ncclFloat32, nccl.ncclUint8
    if (comm.set_reg_a2a_threshold(THRESH) if A2A else comm.set_reg_rooted_threshold(THRESH) if ROOTED
            else comm.set_reg_threshold(THRESH)) != THRESH:
        raise SystemExit("this communicator has no buffer registry (the threshold did not take effect)")

    def row(**kw):
        t = torch.tensor([kw["min_us"], kw["median_us"]], dtype=torch.float64)
        ok = torch.tensor([1 if kw["ok"] else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        kw.update(min_us=round(t[0].item(), 2), median_us=round(t[1].item(), 2), ok=bool(ok.item()))
        if rank == 0:
            print(json.dumps(kw), flush=True)
        return kw["ok"]

    def buffers(coll, nbytes):
        """(send, recv, call, check) for a bucket of nbytes on fresh tensors."""
        if coll == "allreduce":
            cnt = nbytes // 4
            i = torch.arange(cnt, device="cuda", dtype=torch.int32)
            x = (i % 13 + rank).float()
            y = torch.empty_like(x)
            want = ((i % 13) * n + n * (n - 1) // 2).float()
            return x, y, lambda: comm.all_reduce(x.data_ptr(), y.data_ptr(), cnt, F32, nccl.ncclSum, sp), \
                lambda: torch.equal(y, want)
        if coll == "reducescatter":
            per = nbytes // 4 // n
            i = torch.arange(per * n, device="cuda", dtype=torch.int32)
            x = (i % 13 + rank).float()
            y = torch.empty(per, device="cuda")
            want = ((i[rank * per:(rank + 1) * per] % 13) * n + n * (n - 1) // 2).float()
            return x, y, lambda: comm.reduce_scatter(x.data_ptr(), y.data_ptr(), per, F32, nccl.ncclSum, sp), \
                lambda: torch.equal(y, want)
        per = nbytes // n
        i = torch.arange(per, device="cuda", dtype=torch.int32)
        x = ((i + rank) % 251).to(torch.uint8)
        y = torch.empty(per * n, device="cuda", dtype=torch.uint8)
        want = torch.cat([((i + p) % 251).to(torch.uint8) for p in range(n)])
        return x, y, lambda: comm.all_gather(x.data_ptr(), y.data_ptr(), per, U8, sp), lambda: torch.equal(y, want)

    def a2a_rows():
        """--a2a: ncclAllToAll (u8) at MIN_BYTES .. MAX_BYTES per pair, the three
        modes per row; only sendbuff is registered (nobody reads a peer's recvbuff)."""
        good = True
        for pair in sizes(MIN_BYTES, MAX_BYTES):
            for mode in ("zero_copy", "fallback", "off"):
                i = torch.arange(pair * n, device="cuda", dtype=torch.int32)
                x = ((i + 7 * rank) % 251).to(torch.uint8)
                y = torch.empty(pair * n, device="cuda", dtype=torch.uint8)
                j = i % pair + rank * pair  # block p of my output is block `rank` of rank p's input
                want = ((j + 7 * (i // pair)) % 251).to(torch.uint8)
                del i, j
                handle = comm.register(x.data_ptr(), x.numel()) if mode == "zero_copy" else None
                comm.set_reg_a2a_threshold(0 if mode == "off" else THRESH)
                torch.cuda.synchronize()
                dist.barrier()  # every rank's registrations precede every import
                base = comm.reg_a2a_stats()
                y.zero_()
                us = timed(lambda: comm.all_to_all(x.data_ptr(), y.data_ptr(), pair, U8, sp), torch.cuda.synchronize)
                d = [a - b for a, b in zip(comm.reg_a2a_stats(), base)]
                calls = WARMUP + STEPS
                path_ok = d == {"zero_copy": [calls, calls, 0], "fallback": [calls, 0, calls], "off": [0, 0, 0]}[mode]
                good &= row(coll="alltoall", ranks=n, pair_bytes=pair, mode=mode, min_us=us[0],
                            median_us=us[len(us) // 2], steps=STEPS, shared_gpu=shared,
                            ok=bool(torch.equal(y, want)) and path_ok and comm.async_error() == 0)
                if handle is not None:
                    comm.deregister(handle)
                del x, y, want
        comm.set_reg_a2a_threshold(THRESH)
        return good

    def rooted_rows():
        """--rooted: ncclBroadcast (u8) from and ncclReduce (f32 sum) to rank 0.  Only
        what a peer reads is registered: the root's sendbuff and the non-roots'
        recvbuffs of a broadcast, every sendbuff of a reduce."""
        good = True
        for coll in ("broadcast", "reduce"):
            for nbytes in sizes(MIN_BYTES, MAX_BYTES):
                for mode in ("zero_copy", "fallback", "off"):
                    if coll == "broadcast":
                        i = torch.arange(nbytes, device="cuda", dtype=torch.int32)
                        want = (i % 251).to(torch.uint8)
                        x = want.clone() if rank == 0 else None
                        y = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
                        del i
                        mine = x if rank == 0 else y

                        def call():
                            comm.broadcast(x.data_ptr() if rank == 0 else 0, y.data_ptr(), nbytes, U8, 0, sp)
                    else:
                        cnt = nbytes // 4
                        i = torch.arange(cnt, device="cuda", dtype=torch.int32)
                        x = (i % 13 + rank).float()
                        y = torch.empty_like(x) if rank == 0 else None
                        want = ((i % 13) * n + n * (n - 1) // 2).float() if rank == 0 else None
                        del i
                        mine = x

                        def call():
                            comm.reduce(x.data_ptr(), y.data_ptr() if rank == 0 else 0, cnt, F32, nccl.ncclSum, 0, sp)
                    handle = comm.register(mine.data_ptr(), mine.numel() * mine.element_size()) \
                        if mode == "zero_copy" else None
                    comm.set_reg_rooted_threshold(0 if mode == "off" else THRESH)
                    torch.cuda.synchronize()
                    dist.barrier()  # every rank's registrations precede every import
                    base = comm.reg_rooted_stats()
                    if y is not None:
                        y.zero_()
                    us = timed(call, torch.cuda.synchronize)
                    d = [a - b for a, b in zip(comm.reg_rooted_stats(), base)]
                    calls = WARMUP + STEPS
                    path_ok = d == {"zero_copy": [calls, calls, 0], "fallback": [calls, 0, calls],
                                    "off": [0, 0, 0]}[mode]
                    value_ok = y is None or bool(torch.equal(y, want))
                    good &= row(coll=coll, ranks=n, bytes=nbytes, mode=mode, min_us=us[0], median_us=us[len(us) // 2],
                                steps=STEPS, shared_gpu=shared, ok=value_ok and path_ok and comm.async_error() == 0)
                    if handle is not None:
                        comm.deregister(handle)
                    del x, y, want, mine
        comm.set_reg_rooted_threshold(THRESH)
        return good

    good = True
    for coll in () if A2A or ROOTED else ("allreduce", "reducescatter", "allgather"):
        for nbytes in sizes(MIN_BYTES, MAX_BYTES):
            for mode in ("zero_copy", "fallback", "off"):
                x, y, call, check = buffers(coll, nbytes)
                handles = []
                if mode == "zero_copy":
                    handles = [comm.register(t.data_ptr(), t.numel() * t.element_size()) for t in (x, y)]
                comm.set_reg_threshold(0 if mode == "off" else THRESH)
                torch.cuda.synchronize()
                dist.barrier()  # every rank's registrations precede every import
                base = comm.reg_stats()
                y.zero_()
                us = timed(call, torch.cuda.synchronize)
                d = [a - b for a, b in zip(comm.reg_stats()[:3], base[:3])]
                calls = WARMUP + STEPS
                path_ok = d == {"zero_copy": [calls, calls, 0], "fallback": [calls, 0, calls], "off": [0, 0, 0]}[mode]
                good &= row(coll=coll, ranks=n, bytes=nbytes, mode=mode, min_us=us[0], median_us=us[len(us) // 2],
                            steps=STEPS, shared_gpu=shared, ok=bool(check()) and path_ok and comm.async_error() == 0)
                for h in handles:
                    comm.deregister(h)
                del x, y
    if A2A:
        good = a2a_rows()
    elif ROOTED:
        good = rooted_rows()
    else:
        comm.set_reg_threshold(THRESH)
    torch.cuda.synchronize()
    dist.barrier()
    comm.destroy()
    dist.destroy_process_group()
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    child() if os.environ.get("REG_SWEEP_CHILD") else parent()
