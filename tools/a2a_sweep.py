#!/usr/bin/env python3
"""All-to-all sweep: ncclAllToAll for 8 B - 256 KiB per pair (x4 steps) and two
ncclAllToAllv rows from a seeded random matrix — every pair under the per-pair
limit, and about a quarter of the pairs over it — at 2, 4 and 8 ranks, the p2p
FIFO path and the one-hop LL path alternating on ONE communicator
(vcclCommSetA2aThreshold), every row byte-checked and its path confirmed by
vcclCommA2aStats.  Per row: min and median us per call over --steps calls
(default 50) after warm-up, each call timed by its own event pair, the max over
ranks.

    python tools/a2a_sweep.py [--min-bytes N] [--max-bytes N] [--steps K] [--ranks 2,4,8] [--direct]

--direct sweeps the one-hop direct path instead (vcclCommSetDirectA2aThreshold,
vcclCommA2aStatsEx): ncclAllToAll for 16 KiB up to the per-pair limit (what one
inbox region holds, at most --max-bytes, default 2 MiB) and two ncclAllToAllv
rows under the limit, one balanced and one skewed (a quarter of the pairs 16x
the others), FIFO and direct alternating on the one communicator.

The parent spawns the rank processes (bench.py's launcher; ranks share a GPU
when the box has fewer than ranks — then the rows are rehearsal rows: LL
latency between processes time-slicing one GPU is bimodal) and
prints one JSON line per row.  Measurement tool, not product code."""
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
MIN_BYTES = int(arg("--min-bytes", 16 << 10 if DIRECT else 8))
MAX_BYTES = int(arg("--max-bytes", 2 << 20 if DIRECT else 256 << 10))
STEPS = max(50, int(arg("--steps", 50)))
RANKS = [int(x) for x in arg("--ranks", "2,4,8").split(",")]
WARMUP = 5
V_LIMIT = 64 << 10  # the per-pair limit of the all-to-allv rows
V_OVER = 96 << 10   # ... and the size of the pairs over it


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
        env["A2A_SWEEP_CHILD"] = "1"
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
    import numpy as np
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
    U8 = nccl.ncclUint8
    n = world

    def pay(nb, src, dst, tag):
        return np.random.default_rng((tag * 64 + src) * 64 + dst + 1).integers(0, 256, nb, dtype=np.uint8)

    def row(**kw):
        t = torch.tensor([kw["min_us"], kw["median_us"]], dtype=torch.float64)
        ok = torch.tensor([1 if kw["ok"] else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        kw.update(min_us=round(t[0].item(), 2), median_us=round(t[1].item(), 2), ok=bool(ok.item()))
        if rank == 0:
            print(json.dumps(kw), flush=True)
        return kw["ok"]

    def measure(op, m, label, limit):
        """m[a][b] bytes from a to b; both paths in turn on the one comm."""
        good = True
        sc, rc = [int(m[rank][p]) for p in range(n)], [int(m[p][rank]) for p in range(n)]
        sd, rd = [int(x) for x in np.cumsum([0] + sc[:-1])], [int(x) for x in np.cumsum([0] + rc[:-1])]
        send = torch.from_numpy(np.concatenate([pay(sc[p], rank, p, label) for p in range(n)] +
                                               [np.zeros(1, np.uint8)])).cuda()
        want = torch.from_numpy(np.concatenate([pay(rc[p], p, rank, label) for p in range(n)] +
                                               [np.full(1, 0x5A, np.uint8)])).cuda()
        for path, thr in (("fifo", 0), ("direct" if DIRECT else "ll", limit)):
            eff = comm.set_direct_a2a_threshold(thr) if DIRECT else comm.set_a2a_threshold(thr)
            out = torch.full_like(want, 0x5A)
            if op == "alltoall":
                fn = lambda: comm.all_to_all(send.data_ptr(), out.data_ptr(), sc[0], U8, sp)  # noqa: E731
            else:
                fn = lambda: comm.all_to_allv(send.data_ptr(), sc, sd, out.data_ptr(), rc, rd, U8, sp)  # noqa: E731
            s0 = comm.a2a_stats_ex() if DIRECT else comm.a2a_stats()
            us = timed(fn, torch.cuda.synchronize)
            s1 = comm.a2a_stats_ex() if DIRECT else comm.a2a_stats()
            calls = STEPS + WARMUP
            if DIRECT:
                pl = nccl.direct_a2a_plan(n, rank, sc, rc, op == "alltoall", 0, eff, 1)
                fifo = len(pl["res_sends"]) + len(pl["res_recvs"])
                ok = eff == thr and torch.equal(out, want) and [a - b for a, b in zip(s1, s0)] == \
                    [0, 0, calls * int(pl["direct_launch"]), calls * (2 * n - fifo), calls * fifo]
                good &= row(op=op, ranks=world, shared_gpu=shared, path=path,
                            bytes_per_pair=label if op == "alltoall" else None,
                            variant=None if op == "alltoall" else label_name[label], direct_pairs=2 * n - fifo,
                            fifo_pairs=fifo, calls=STEPS, min_us=us[0], median_us=us[len(us) // 2], ok=ok)
                continue
            pl = nccl.ll_a2a_plan(n, rank, sc, rc, op == "alltoall", eff, max(1, (1 << 20) // 8))
            fifo = len(pl["res_sends"]) + len(pl["res_recvs"])
            ok = eff == thr and torch.equal(out, want) and \
                [a - b for a, b in zip(s1, s0)] == [calls * int(pl["launch"]), calls * (2 * n - fifo), calls * fifo]
            good &= row(op=op, ranks=world, shared_gpu=shared, path=path, bytes_per_pair=label if op == "alltoall" else None,
                        variant=None if op == "alltoall" else label_name[label], ll_pairs=2 * n - fifo, fifo_pairs=fifo,
                        calls=STEPS, min_us=us[0], median_us=us[len(us) // 2], ok=ok)
        comm.set_direct_a2a_threshold(0) if DIRECT else comm.set_a2a_threshold(0)
        return good

    label_name = {1: "all_under_limit", 2: "quarter_over_limit", 3: "balanced", 4: "skewed"}
    good = True
    if DIRECT:
        limit = min(MAX_BYTES, comm.set_direct_a2a_threshold(1 << 40))  # what one region holds
        comm.set_direct_a2a_threshold(0)
        for nb in sizes(MIN_BYTES, limit):
            good &= measure("alltoall", [[nb] * n for _ in range(n)], nb, limit)
        rng = np.random.default_rng(2027 + n)
        balanced = rng.integers(limit // 16, limit // 8 + 1, size=(n, n))
        skewed = rng.integers(limit // 32, limit // 16 + 1, size=(n, n))
        hot = rng.random((n, n)) < 0.25
        hot[0, n - 1] = True
        skewed[hot] *= 16
        good &= measure("alltoallv", balanced, 3, limit)
        good &= measure("alltoallv", skewed, 4, limit)
        err = comm.async_error()
        comm.destroy()
        dist.destroy_process_group()
        sys.exit(0 if good and not err else 1)
    for nb in sizes(MIN_BYTES, MAX_BYTES):
        good &= measure("alltoall", [[nb] * n for _ in range(n)], nb, MAX_BYTES)
    rng = np.random.default_rng(2026 + n)
    under = rng.integers(0, 4097, size=(n, n))
    over = under.copy()
    over[rng.random((n, n)) < 0.25] = V_OVER
    if not (over > V_LIMIT).any():
        over[0, n - 1] = V_OVER
    good &= measure("alltoallv", under, 1, V_LIMIT)
    good &= measure("alltoallv", over, 2, V_LIMIT)
    err = comm.async_error()
    comm.destroy()
    dist.destroy_process_group()
    sys.exit(0 if good and not err else 1)


if __name__ == "__main__":
    if "RANK" in os.environ and "A2A_SWEEP_CHILD" in os.environ:
        child()
    else:
        parent()
