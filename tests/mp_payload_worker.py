#!/usr/bin/env python3
"""One rank of the payload tests (tests/test_gpu_payloads.py).

argv: rank nranks uid_hex outdir
One comm; the path is switched between calls (vcclCommSetAlgo: the one-hop
LL kernels, the staged direct path, the SIMPLE ring with the workgroup and
with the per-wave slot hand-off, the LL128 ring) and vcclCommCollAlgo must
report the forced path for every call.  Per path: an all-reduce of 8 209
elements, a reduce-scatter of 2 053 per rank and (LL and ring) an ncclReduce
of 8 209 to root n - 1, for f16, bf16, f32, f64, both fp8, i8, i32, u64 and
every op, on tests/_payloads.py hard_input streams.  On the LL path also: two
all-reduces into a receive pointer 2 bytes past alignment (guard bytes
checked here) and, at n = 2, every byte pair through u8, i8, E4M3 and E5M2.
In the per-wave pass the per-wave launch counter must rise for the f32 / f16
/ bf16 sums and for nothing else.  Outputs go to outdir/rank<r>.npz for the
parent's oracle check.  Exit 0 when the local checks pass."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tests import _mp  # noqa: E402
from tests import _payloads as P  # noqa: E402
from vccl_amd import nccl  # noqa: E402

AR, RS, RED = 0, 1, 4
# (pass name, vcclCommSetAlgo path, per-wave hand-off, runs ncclReduce)
PASSES = (("ll", "ll", False, True), ("direct", "direct", False, False), ("ring", "ring", False, True),
          ("wave", "ring", True, True), ("ll128", "ll128", False, False))
PAIR_TYPES = (1, 0, 10, 11)  # u8, i8, E4M3, E5M2
MIS = ((6, P.AR_COUNT), (9, 4099))  # (type, count) of the all-reduces 2 bytes past alignment
GUARD, FILL = 64, 0xA5


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()


def out_buf(nbytes):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def run_matrix(comm, rank, n, sp, name, path, wave, reduce_too, res, bad):
    """The (type, op) matrix on the comm's current path.  Every call's step of
    the per-wave launch counter is checked: one for an f32 / f16 / bf16 sum
    in the per-wave pass, zero for every other call."""
    for dt in P.MATRIX_TYPES:
        esz = nccl.TYPE_SIZE[dt]
        for op in P.MATRIX_OPS:
            colls = [(AR, "ar", P.AR_COUNT, P.AR_COUNT), (RS, "rs", P.RS_COUNT, n * P.RS_COUNT)]
            if reduce_too:
                colls.append((RED, "red", P.AR_COUNT, P.AR_COUNT))
            for code, cname, count, n_in in colls:
                algo = comm.coll_algo(code, count, dt)
                if algo != path:
                    bad.append((name, cname, dt, op, "path", algo))
                    continue
                x = P.hard_input(dt, op, n_in, rank, n, P.SEED)
                xb, yb = to_dev(x), out_buf(count * esz)
                launches = comm.set_ring_wave(None)
                if code == AR:
                    comm.all_reduce(xb.data_ptr(), yb.data_ptr(), count, dt, op, sp)
                elif code == RS:
                    comm.reduce_scatter(xb.data_ptr(), yb.data_ptr(), count, dt, op, sp)
                else:
                    comm.reduce(xb.data_ptr(), yb.data_ptr(), count, dt, op, n - 1, sp)
                torch.cuda.synchronize()
                if code != RED or rank == n - 1:
                    res[f"{name}_{cname}_{dt}_{op}"] = yb.cpu().numpy().view(x.dtype)
                elif not bool((yb == FILL).all()):
                    bad.append((name, cname, dt, op, "non-root output written"))
                if not np.array_equal(xb.cpu().numpy(), x.view(np.uint8)):
                    bad.append((name, cname, dt, op, "input written"))
                per_wave = wave and op == nccl.ncclSum and dt in (nccl.ncclFloat32, nccl.ncclFloat16, nccl.ncclBfloat16)
                if comm.set_ring_wave(None) - launches != int(per_wave):
                    bad.append((name, cname, dt, op, "per-wave launches", comm.set_ring_wave(None) - launches))


def run_ll_extras(comm, rank, n, sp, res, bad):
    # the zero-padded last line: a receive pointer 2 bytes past alignment, guards around the output
    for dt, count in MIS:
        x = P.hard_input(dt, 0, count, rank, n, P.SEED + 1)
        xb = to_dev(x)
        yb = out_buf(GUARD + 2 + x.nbytes + GUARD)
        assert yb.data_ptr() % 16 == 0
        if comm.coll_algo(AR, count, dt) != "ll":
            bad.append(("mis", dt, "path"))
        comm.all_reduce(xb.data_ptr(), yb.data_ptr() + GUARD + 2, count, dt, nccl.ncclSum, sp)
        torch.cuda.synchronize()
        raw = yb.cpu().numpy()
        if not ((raw[:GUARD + 2] == FILL).all() and (raw[GUARD + 2 + x.nbytes:] == FILL).all()):
            bad.append(("mis", dt, "guard bytes written"))
        res[f"ll_mis_{dt}"] = raw[GUARD + 2:GUARD + 2 + x.nbytes].copy().view(x.dtype)
    if n != 2:
        return
    # every byte pair through the per-element functors: rank 0 holds a, rank 1 holds b
    mine = P.all_pairs_u8()[rank]
    half = mine.size // 2
    for dt in PAIR_TYPES:
        x = mine.view(O.NP_DTYPE[dt])
        for op in P.MATRIX_OPS:
            for code, cname, count in ((AR, "ar", mine.size), (RS, "rs", half)):
                if comm.coll_algo(code, count, dt) != "ll":
                    bad.append(("pairs", cname, dt, op, "path"))
                    continue
                xb, yb = to_dev(x), out_buf(count)
                if code == AR:
                    comm.all_reduce(xb.data_ptr(), yb.data_ptr(), count, dt, op, sp)
                else:
                    comm.reduce_scatter(xb.data_ptr(), yb.data_ptr(), count, dt, op, sp)
                torch.cuda.synchronize()
                res[f"pairs_{cname}_{dt}_{op}"] = yb.cpu().numpy().view(x.dtype)


def main():
    rank, n = int(sys.argv[1]), int(sys.argv[2])
    uid = nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3]))
    outdir = sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, uid, rank)
    sp = torch.cuda.current_stream().cuda_stream
    res, bad = {}, []
    for name, path, wave, reduce_too in PASSES:
        comm.set_algo(path)
        comm.set_ring_wave(wave)
        run_matrix(comm, rank, n, sp, name, path, wave, reduce_too, res, bad)
        comm.set_ring_wave(False)
        if name == "ll":
            run_ll_extras(comm, rank, n, sp, res, bad)
    comm.set_algo(None)
    torch.cuda.synchronize()
    err = comm.async_error()
    comm.destroy()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
    if bad or err:
        print(f"rank {rank}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
