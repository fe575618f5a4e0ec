"""One rank of tests/test_gpu_allreduce_bias.py.  argv: rank nranks uid_hex case; exit 0 when its outputs are right."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _mp  # noqa: E402
from tests.mp_sum_fp32_worker import AR, three_chunk_count  # noqa: E402
from vccl_amd import nccl  # noqa: E402

F32, BF16, E4M3, I32 = nccl.ncclFloat32, nccl.ncclBfloat16, 10, nccl.ncclInt32
SUM, PROD, MAX = nccl.ncclSum, nccl.ncclProd, nccl.ncclMax
TORCH = {F32: torch.float32, BF16: torch.bfloat16, E4M3: torch.float8_e4m3fn, I32: torch.int32}
OPS = {SUM: torch.sum, PROD: torch.prod, MAX: torch.amax}
# largest |k| of the inputs k / 4 (i32: k): 5 k for the sums and k^5 for the product fit the type's significand
KMAX = {(F32, SUM): 1000, (BF16, SUM): 51, (E4M3, SUM): 3, (I32, MAX): 1000, (F32, PROD): 15}
# (type, op, count, placement); recv_off / acc_off: that buffer alone one element off 16 bytes; acc_send: acc = sendbuff
ROWS = [(F32, SUM, 1, "out"), (F32, SUM, 3, "in"), (F32, SUM, 1027, "recv_off"), (F32, SUM, 1027, "acc_off"),
        (F32, SUM, 1027, "acc_send"), (BF16, SUM, 3, "acc_off"), (BF16, SUM, 1027, "recv_off"), (BF16, SUM, 1027, "in"),
        (E4M3, SUM, 3, "recv_off"), (E4M3, SUM, 1027, "acc_off"), (I32, MAX, 1, "in"), (I32, MAX, 1027, "acc_off"),
        (F32, PROD, 3, "out"), (F32, PROD, 1027, "acc_off")]
CHUNKS = [(F32, SUM, "chunks", "out"), (BF16, SUM, "chunks", "acc_off"), (E4M3, SUM, "chunks", "in")]  # on Direct only


def inputs(dt, op, count, n, same):  # n inputs and the bias, float64; `same`: every input is the bias
    k = np.random.default_rng(1000 * count + 17 * dt + op).integers(-KMAX[dt, op], KMAX[dt, op] + 1, (n + 1, count))
    x = torch.from_numpy(k.astype(np.float64)) * (1.0 if dt == I32 else 0.25)
    return x[n:].expand(n + 1, count) if same else x


def call(comm, sp, dt, op, xs, mine, bias, place, null_bias=False):  # one all-reduce; the output's bytes
    t, count, a0, r0 = TORCH[dt], xs.shape[1], int(place == "acc_off"), int(place == "recv_off")
    send = xs[mine].float().to(t).cuda()
    acc = send if place == "acc_send" else torch.cat([torch.zeros(a0, dtype=torch.float64), bias]).float().to(t).cuda()
    recv = send if place == "in" else torch.zeros(count + 1).to(t).cuda()
    s, r = send.data_ptr(), recv[r0:].data_ptr()
    if null_bias:  # the C entry point itself with acc = NULL (the binding would call ncclAllReduce)
        nccl.check(nccl.lib().ncclAllReduceWithBias(s, r, count, dt, op, comm.handle, sp, 0))
    else:
        comm.all_reduce(s, r, count, dt, op, sp, acc=acc[a0:].data_ptr())
    torch.cuda.synchronize()
    return recv[r0:r0 + count].cpu().view(torch.uint8)


def run_rows(comm, rank, n, sp, rows):  # the rows that differ from op over inputs and bias in float64, cast once
    bad = []
    for dt, op, count, place in rows:
        count = three_chunk_count(AR, n, TORCH[dt].itemsize) if count == "chunks" else count
        x = inputs(dt, op, count, n, place == "acc_send")
        exp = OPS[op](x, 0).float().to(TORCH[dt]).view(torch.uint8)
        bad += [(dt, op, count, place)] * (not torch.equal(call(comm, sp, dt, op, x[:n], rank, x[n], place), exp))
    return bad


def main():
    rank, n, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3])), rank)
    sp, S = torch.cuda.current_stream().cuda_stream, SUM
    path, _, extra = case.partition("+")  # ll2 / direct1: that path under VCCL_SUM_FP32 at that level
    algo, wide = {"ll2": "ll", "direct1": "direct"}.get(path, path), path in ("ll2", "direct1")
    bad = [("path", comm.coll_algo(AR, 1027, BF16))] * (comm.coll_algo(AR, 1027, BF16) != algo)
    if extra == "order":  # inputs big and 1, bias 1: big natively, big + 2 with the bias inside the binary32 fold
        for dt, big in ((BF16, 256.0), (E4M3, 16.0)):
            x = torch.tensor([[big], [1.0], [1.0]], dtype=torch.float64)
            exp = (x[0] + 2 * wide).float().to(TORCH[dt]).view(torch.uint8)
            bad += [(dt, "order")] * (not torch.equal(call(comm, sp, dt, S, x[:2], rank, x[2], "out"), exp))
        bad += run_rows(comm, rank, n, sp, [r for r in ROWS if r[0] in (BF16, E4M3)] * wide)  # wide packs and tails
    else:
        if path == "ll":  # ncclAvg, a PreMulSum op and acc == recvbuff are refused, and the comm stays usable
            x, y, half = torch.ones(8).cuda(), torch.zeros(8).cuda(), ctypes.c_float(0.5)
            pre = comm.create_premulsum(ctypes.addressof(half), F32, 1)  # ncclScalarHostImmediate
            codes = [nccl.lib().ncclAllReduceWithBias(x.data_ptr(), y.data_ptr(), 8, F32, op, comm.handle, sp, a)
                     for op, a in ((nccl.ncclAvg, x.data_ptr()), (pre, x.data_ptr()), (S, y.data_ptr()))]
            bad += [("refusals", codes)] * (codes != [nccl.ncclInvalidArgument] * 3)
        bad += run_rows(comm, rank, n, sp, ROWS + (CHUNKS if path == "direct" else []))
        xs = [inputs(F32, S, c, n, False) for c in (1027, 515, 259)]
        if path == "direct":  # one group: two bias calls and, in the middle, a plain all-reduce of the same type
            send, acc = [x[rank].float().cuda() for x in xs], [x[n].float().cuda() for x in xs]
            recv = [torch.zeros_like(t) for t in send]
            nccl.group_start()
            for i, x in enumerate(xs):
                comm.all_reduce(send[i].data_ptr(), recv[i].data_ptr(), x.shape[1], F32, S, sp,
                                acc=acc[i].data_ptr() if i != 1 else None)
            nccl.group_end()
            torch.cuda.synchronize()
            exp = [x[:n + (i != 1)].sum(0).float() for i, x in enumerate(xs)]
            bad += [("group", i) for i in range(3) if not torch.equal(recv[i].cpu(), exp[i])]
        got = call(comm, sp, F32, S, xs[0][:n], rank, xs[0][n], "out", True)  # a NULL bias: the bits of ncclAllReduce
        bad += [("null",)] * (not torch.equal(got, xs[0][:n].sum(0).float().view(torch.uint8)))
    bad += [("async error", comm.async_error())] * (comm.async_error() != 0)
    comm.destroy()
    sys.exit(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad)" if bad else 0)


if __name__ == "__main__":
    main()
