#!/usr/bin/env python3
"""MXFP8 sweep: the bf16 ncclSum all-reduce, 1 MiB - 256 MiB (x4 steps), on ONE communicator created with
NCCL_ALGO=Direct, two ways per row:

  native   the threshold off (vcclCommSetArMxfp8Threshold 0): the forced-Direct two-shot kernel, 2 bytes per
           element and hop
  mxfp8    the threshold at 1 byte: device/direct_mx.hpp, 33/32 bytes per element and hop

Inputs are k / 4 for |k| <= 31, so the native sum is exact in any order; every row carries a correctness flag:
native against that exact sum, mxfp8 bit for bit against the CPU model of the format
(tests/mp_ar_mxfp8_worker.py) on the first and the last 64 Ki elements rounded to whole tiles — the format is local
to a 32-element block, so a span of whole blocks is modelled from its own inputs.  The path of every row is
confirmed by vcclCommArMxfp8Stats.  Per row: min and median us per call over --steps calls after warm-up, each timed
by its own event pair, the max over ranks.

    python tools/mxfp8_sweep.py [--min-bytes N] [--max-bytes N] [--steps K] [--ranks 2,4,8]

Ranks share a GPU when the box has fewer GPUs than ranks: such rows are rehearsal rows (shared_gpu true) and say
nothing about xGMI, where the format's saving is.  Measurement tool, not product code."""
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


MIN_BYTES = int(arg("--min-bytes", 1 << 20))
MAX_BYTES = int(arg("--max-bytes", 256 << 20))
STEPS = max(5, int(arg("--steps", 20)))
RANKS = [int(x) for x in arg("--ranks", "2,4,8").split(",")]
WARMUP, SPAN = 3, 64 << 10


def parent():
    import bench
    rc = 0
    for n in RANKS:
        env = dict(os.environ)
        env.pop("WORLD_SIZE", None)
        env.update(MXFP8_SWEEP_CHILD="1", NCCL_ALGO="Direct")
        env.setdefault("VCCL_SPIN_TIMEOUT_S", "30")
        plan = bench.rank_launch_plan(["--gpus", str(n)] + sys.argv[1:], env, script=os.path.abspath(__file__))
        rc = rc or bench._spawn_ranks(plan)
    sys.exit(rc)


def child():
    import torch
    import torch.distributed as dist

    from tests.mp_ar_mxfp8_worker import model_allreduce
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
    if comm.set_ar_mxfp8_threshold(1) != 1:
        raise SystemExit("the MXFP8 threshold did not take effect on this communicator")

    def values(i, r):  # k / 4, |k| <= 31, of element indices i on rank r
        return ((i * 7 + r * 13) % 63 - 31).float() * 0.25

    good, size = True, MIN_BYTES
    while size <= MAX_BYTES:
        cnt = size // 2
        spans = sorted({(0, min(cnt, SPAN)), (max(0, (cnt - SPAN) // 512 * 512), cnt)})
        for mode in ("native", "mxfp8"):
            comm.set_ar_mxfp8_threshold(0 if mode == "native" else 1)
            i = torch.arange(cnt, device="cuda", dtype=torch.int32)
            x = values(i, rank).to(torch.bfloat16)
            del i
            y = torch.zeros_like(x)
            base = comm.ar_mxfp8_stats()
            for _ in range(WARMUP):
                comm.all_reduce(x.data_ptr(), y.data_ptr(), cnt, nccl.ncclBfloat16, nccl.ncclSum, sp)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
            for a, b in ev:
                a.record()
                comm.all_reduce(x.data_ptr(), y.data_ptr(), cnt, nccl.ncclBfloat16, nccl.ncclSum, sp)
                b.record()
            torch.cuda.synchronize()
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
            ok = comm.ar_mxfp8_stats() - base == (0 if mode == "native" else WARMUP + STEPS)
            for lo, hi in spans:
                xs = [values(torch.arange(lo, hi, dtype=torch.int32), r) for r in range(n)]
                want = torch.stack(xs).sum(0).to(torch.bfloat16) if mode == "native" \
                    else model_allreduce(xs, torch.bfloat16)
                ok = ok and torch.equal(y[lo:hi].cpu().view(torch.int16), want.view(torch.int16))
            t = torch.tensor([us[0], us[len(us) // 2]], dtype=torch.float64)
            flag = torch.tensor([1 if ok and comm.async_error() == 0 else 0])
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            good &= bool(flag.item())
            if rank == 0:
                print(json.dumps(dict(coll="allreduce_bf16", ranks=n, bytes=size, mode=mode,
                                      algo=comm.coll_algo(0, cnt, 9), min_us=round(t[0].item(), 2),
                                      median_us=round(t[1].item(), 2), steps=STEPS, shared_gpu=shared,
                                      ok=bool(flag.item()))), flush=True)
            del x, y
        size *= 4
    torch.cuda.synchronize()
    dist.barrier()
    comm.destroy()
    dist.destroy_process_group()
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    child() if os.environ.get("MXFP8_SWEEP_CHILD") else parent()
