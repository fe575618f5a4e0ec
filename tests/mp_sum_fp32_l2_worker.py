"""One rank of tests/test_gpu_sum_fp32_l2.py (which says what the inputs are).  argv: rank nranks uid_hex case.
Every rank derives all ranks' inputs from the seed and checks its own output; exit 0 when it is right."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests import _mp  # noqa: E402
from tests.mp_sum_fp32_worker import AR, RS, TYPES, expected, run, three_chunk_count, values  # noqa: E402
from vccl_amd import nccl  # noqa: E402

RED, SENTINEL = 4, 0x5a
# per rank; at n = 8 the largest bucket, bf16, is 8 * 4099 * 2 = 65 584 bytes, below GEOM's LL reduce-scatter
# threshold of n * 1 MiB; a block of 8198 bytes ends in a partial line
RS_COUNT = 4099


def types_ops(n):  # avg premultiplies by 1 / 4: exact at n = 4
    return [(dt, op) for dt in (9, 10) + ((6, 11) if n == 4 else ())
            for op in (nccl.ncclSum,) + ((nccl.ncclAvg,) if n == 4 else ())]


def case_ll(comm, rank, n, sp):
    want = "direct" if os.environ.get("VCCL_LL_THRESHOLD") == "0" else "ll"
    bad = [(coll, dt, op, count, ip) for dt, op in types_ops(n) for coll, count in ((AR, 1), (AR, 4099), (RS, RS_COUNT))
           for ip in (False, True)
           if comm.coll_algo(coll, count, dt) != want or not run(comm, rank, n, sp, coll, dt, op, count, ip)]
    if n == 4:  # buffers one element past alignment
        bad += [(c, "misaligned") for c in (AR, RS) if not run(comm, rank, n, sp, c, 9, nccl.ncclSum, 4099, False, 1)]
    return bad


def call(comm, rank, n, sp, coll, dt, op, count, root=0, registered=None):
    """One out-of-place call on buffers of its own; True when the output is the exact sum cast once (a reduce's
    non-root: the untouched sentinel).  registered True / False: on registered buffers or not, after a small f32
    all-reduce and a synchronise (every peer's registrations precede my enqueue), and counted by the comm as
    zero-copy / as a fallback."""
    t, total = TYPES[dt][0], n * count if coll == RS else count
    xs = [values(dt, 2000 * count + 17 * dt + 5 * coll + r, total) for r in range(n)]
    exp = expected(dt, xs, 0.25 if op == nccl.ncclAvg else 1.0)
    exp = exp[rank * count:(rank + 1) * count] if coll == RS else exp
    send = xs[rank].to(t).cuda()
    recv = torch.full((len(exp) * t.itemsize,), SENTINEL, dtype=torch.uint8).cuda()
    hs = [comm.register(b.data_ptr(), b.numel() * b.element_size()) for b in (send, recv)] if registered else []
    stats = comm.reg_rooted_stats if coll == RED else comm.reg_stats
    if registered is not None:
        one = torch.ones(64, device="cuda")
        comm.all_reduce(one.data_ptr(), one.data_ptr(), 64, nccl.ncclFloat32, nccl.ncclSum, sp)
        base = stats()  # synchronises
    if coll == RED:
        comm.reduce(send.data_ptr(), recv.data_ptr(), count, dt, op, root, sp)
    else:
        (comm.all_reduce if coll == AR else comm.reduce_scatter)(send.data_ptr(), recv.data_ptr(), count, dt, op, sp)
    torch.cuda.synchronize()
    ok = registered is None or [a - b for a, b in zip(stats()[:3], base[:3])] == [1, registered, not registered]
    for h in hs:
        comm.deregister(h)
    want = torch.full_like(recv, SENTINEL) if coll == RED and rank != root else exp.view(torch.uint8).cuda()
    return ok and torch.equal(recv, want)


def case_reg(comm, rank, n, sp):
    bad = [(coll, dt, op, reg) for dt, op in types_ops(n) for coll in (AR, RS) for reg in (True, False)
           if not call(comm, rank, n, sp, coll, dt, op, 4099, registered=reg)]
    return bad + [(RED, reg) for reg in (True, False)
                  if not call(comm, rank, n, sp, RED, 9, nccl.ncclSum, 4099, n - 1, registered=reg)]


def case_reduce(comm, rank, n, sp):
    return [(dt, op, count, root) for dt, op in types_ops(n) for root in (0, n - 1)
            for count in (1, 4099, three_chunk_count(AR, n, TYPES[dt][0].itemsize))
            if comm.coll_algo(RED, count, dt) != "direct" or not call(comm, rank, n, sp, RED, dt, op, count, root)]


def case_levels(comm, rank, n, sp):
    """On a comm created without the variable: each request reports its level; level 1 leaves a bf16 ncclReduce as
    it is; level 2 makes it exact (other bits) and leaves an f32 sum and a bf16 max all-reduce as they are."""
    got = {}
    for level in (0, 1, 2):
        if comm.set_sum_fp32(level) != level:
            return [("level", level)]
        for name, dt, op in (("reduce", 9, nccl.ncclSum), ("f32", 7, nccl.ncclSum), ("max", 9, nccl.ncclMax)):
            x = values(9, 30 + rank, 4099).to(torch.float32 if dt == 7 else torch.bfloat16).cuda()
            y = torch.zeros_like(x)
            if name == "reduce":
                comm.reduce(x.data_ptr(), y.data_ptr(), 4099, dt, op, 0, sp)
            else:
                comm.all_reduce(x.data_ptr(), y.data_ptr(), 4099, dt, op, sp)
            torch.cuda.synchronize()
            got[name, level] = y.cpu().view(torch.uint8)
    exact = expected(9, [values(9, 30 + r, 4099) for r in range(n)]).view(torch.uint8)
    same = [("reduce", 1, got["reduce", 0]), ("f32", 2, got["f32", 0]), ("max", 2, got["max", 0])]
    same += [("reduce", 2, exact)] * (rank == 0)
    return [(k, lv) for k, lv, want in same if not torch.equal(got[k, lv], want)] + \
        [("reduce unchanged",)] * (rank == 0 and torch.equal(got["reduce", 0], exact))


def main():
    rank, n, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3])), rank)
    bad = {"ll": case_ll, "reg": case_reg, "reduce": case_reduce, "levels": case_levels}[case](
        comm, rank, n, torch.cuda.current_stream().cuda_stream)
    err = comm.async_error()
    comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
