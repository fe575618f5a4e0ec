"""One rank of tests/test_gpu_sum_fp32.py (which says what the inputs are).  argv: rank nranks uid_hex case outdir.
Every rank derives all ranks' inputs from the seed and checks its own output; exit 0 when it is right."""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _mp  # noqa: E402
from vccl_amd import nccl  # noqa: E402

AR, RS = 0, 1
# nccl type code -> (torch dtype, largest |k|: k exact in the type and 8 k / 4 far below its largest finite value)
TYPES = {6: (torch.float16, 2047), 9: (torch.bfloat16, 255), 10: (torch.float8_e4m3fn, 15), 11: (torch.float8_e5m2, 7)}


def values(dt, seed, n_elts):  # binary32 values k / 4, exact in type dt
    k = np.random.default_rng(seed).integers(-TYPES[dt][1], TYPES[dt][1] + 1, n_elts)
    return torch.from_numpy(k.astype(np.float32)) * 0.25


def expected(dt, xs, scale=1.0):  # the exact binary32 sum of the (premultiplied) inputs, narrowed once
    return (torch.stack(xs) * scale).sum(0).to(TYPES[dt][0])


def native_fold(dt, xs, scale=1.0):  # the inputs folded in the given order, one rounding to the type per step
    ys = [(x * scale).to(TYPES[dt][0]) for x in xs]
    return functools.reduce(lambda acc, y: (acc.float() + y.float()).to(y.dtype), ys)


def three_chunk_count(coll, n, esz):
    """A count that moves through the inbox in three chunks (host/setup.cc's region, host/plan.cc direct_plan)."""
    region = (max(int(os.environ["VCCL_DIRECT_CHUNK_BYTES"]), 64 << 10) + n - 1) // n // 256 * 256 + 256
    relts, align = (region - 16) // esz, 16 // esz
    return 2 * (relts * n // (n * align) * (n * align) if coll == AR else relts // align * align) + 1031


def run(comm, rank, n, sp, coll, dt, op, count, inplace, off=0):
    """An all-reduce (count elements) or reduce-scatter (count per rank), buffers `off` elements past alignment."""
    t, total = TYPES[dt][0], count if coll == AR else n * count
    xs = [values(dt, 1000 * count + 17 * dt + r, total) for r in range(n)]
    exp = expected(dt, xs, 0.25 if op == nccl.ncclAvg else 1.0)  # avg runs at n = 4: premultiplied by 1 / 4
    exp = exp[rank * count:(rank + 1) * count] if coll == RS else exp
    send = torch.zeros(total + off, dtype=t).cuda()
    send[off:] = xs[rank].to(t).cuda()
    recv = send if inplace else torch.zeros(len(exp) + off, dtype=t).cuda()
    r0 = off + (rank * count if inplace and coll == RS else 0)
    call = comm.all_reduce if coll == AR else comm.reduce_scatter
    call(send[off:].data_ptr(), recv[r0:].data_ptr(), count, dt, op, sp)
    torch.cuda.synchronize()
    return torch.equal(recv[r0:r0 + len(exp)].cpu().view(torch.uint8), exp.view(torch.uint8))


def case_colls(comm, rank, n, sp, res):
    bad = []
    for dt in (9, 10) + ((6, 11) if n == 4 else ()):
        for op in (nccl.ncclSum,) + ((nccl.ncclAvg,) if n == 4 else ()):
            for coll, count, ip in ((AR, 1, 0), (AR, 1, 1), (AR, 4099, 0), (AR, 4099, 1), (RS, 4099, 0), (RS, 4099, 1)):
                bad += [(coll, dt, op, count, ip)] * (not run(comm, rank, n, sp, coll, dt, op, count, bool(ip)))
    if n == 4:  # buffers one element past alignment; the reported path of an 8-byte call; the calls left alone
        bad += [(c, "misaligned") for c in (AR, RS) if not run(comm, rank, n, sp, c, 9, nccl.ncclSum, 4099, False, 1)]
        bad += [("algo",)] * (comm.coll_algo(AR, 4, 9) != "direct")
        case_plain(comm, rank, n, sp, res)
    return bad


def case_chunks(comm, rank, n, sp, res):
    return [(c, dt) for dt in (9, 10) for c in (AR, RS)
            if not run(comm, rank, n, sp, c, dt, nccl.ncclSum, three_chunk_count(c, n, TYPES[dt][0].itemsize), c == RS)]


def case_plain(comm, rank, n, sp, res):
    for name, dt, op in (("f32_sum", 7, nccl.ncclSum), ("bf16_max", 9, nccl.ncclMax), ("bf16_sum", 9, nccl.ncclSum)):
        x = values(9, 30 + rank, 4099).to(torch.bfloat16 if dt == 9 else torch.float32).cuda()
        y = torch.zeros_like(x)
        comm.all_reduce(x.data_ptr(), y.data_ptr(), 4099, dt, op, sp)
        torch.cuda.synchronize()
        res[name] = y.cpu().view(torch.uint8).numpy()
        res[name + "_algo"] = np.array(comm.coll_algo(AR, 4099, dt))


def main():
    rank, n, case, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4], sys.argv[5]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3])), rank)
    res = {}
    bad = {"colls": case_colls, "chunks": case_chunks, "plain": case_plain}[case](
        comm, rank, n, torch.cuda.current_stream().cuda_stream, res) or []
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    err = comm.async_error()
    comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
