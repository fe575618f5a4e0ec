"""One rank of tests/test_gpu_sum_fp32_ring.py (which says what the inputs are).  argv: rank nranks uid_hex case.
Every rank derives all ranks' inputs from the seed and checks its own output; exit 0 when it is right."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _mp  # noqa: E402
from tests.mp_sum_fp32_worker import AR, RS, TYPES, run, values  # noqa: E402
from vccl_amd import nccl  # noqa: E402

NCH, SLOT, KSTEPS = 14, 4096, 8  # the test's geometry (VCCL_NCHANNELS, VCCL_SLOT_BYTES) and the FIFO depth


def multi_slice_count(coll, n, dt):
    """The smallest count (all-reduce: elements, reduce-scatter: per rank) of the form 4096 k + 3 at which a
    channel's part is more than 2048 elements per chunk and per rank and more than KSTEPS binary32 slots long."""
    need = max(2048, KSTEPS * SLOT // 4) + 1
    for count in range(4099, 1 << 22, 4096):
        p = nccl.ring_partition(coll, count, dt, n, NCH, SLOT)
        part = max(p[2:5]) // (n if coll == AR else 1)
        if part >= need and min(p[5:8]) > 2048:
            return count
    raise AssertionError("no such count")


def types_ops(n):  # the exactness of avg needs a power-of-two 1 / n, and `run` premultiplies by 1 / 4
    return [(dt, op) for dt in (9, 10) + ((6, 11) if n == 2 else ())
            for op in (nccl.ncclSum,) + ((nccl.ncclAvg,) if n == 4 else ())]


def case_exact(comm, rank, n, sp):
    bad = []
    for dt, op in types_ops(n):
        for coll in (AR, RS):
            for count in (1, 4099, multi_slice_count(coll, n, dt)):
                for ip in (False, True):
                    if comm.coll_algo(coll, count, dt) != "ring" or not run(comm, rank, n, sp, coll, dt, op, count, ip):
                        bad.append((coll, dt, op, count, ip))
    if n == 3:  # buffers one element past alignment
        bad += [(c, "misaligned") for c in (AR, RS) if not run(comm, rank, n, sp, c, 9, nccl.ncclSum, 4099, False, 1)]
    return bad


def mixed(dt, seed, n_elts):  # normals scaled by 2^k, k uniform in [-6, 6], rounded to the type: order-sensitive
    g = np.random.default_rng(seed)
    x = g.standard_normal(n_elts) * np.exp2(g.integers(-6, 7, n_elts))
    return torch.from_numpy(x.astype(np.float32)).to(TYPES[dt][0])


def case_order(comm, rank, n, sp):
    """The wide ring against the staged direct wide kernel on the same call: the same fold order, the same bits."""
    bad = []
    for dt in (9, 10):
        for coll in (AR, RS):
            count = multi_slice_count(coll, n, dt)
            send = mixed(dt, 77 * dt + rank, count * (n if coll == RS else 1)).cuda()
            out = []
            for threshold, want in ((1, "ring"), (0, "direct")):
                comm.set_sum_fp32_ring_threshold(threshold)
                recv = torch.zeros(count, dtype=send.dtype).cuda()
                (comm.all_reduce if coll == AR else comm.reduce_scatter)(send.data_ptr(), recv.data_ptr(), count, dt,
                                                                         nccl.ncclSum, sp)
                torch.cuda.synchronize()
                out.append(recv.cpu().view(torch.uint8))
                bad += [(coll, dt, "algo", want)] * (comm.coll_algo(coll, count, dt) != want)
            bad += [(coll, dt, int((out[0] != out[1]).sum()))] * (not torch.equal(out[0], out[1]))
    return bad


def case_switch(comm, rank, n, sp):
    """On a comm created without the variables: the path follows the two setters, native calls keep their bits."""
    def ar(dt):
        x = values(9, 30 + rank, 4099).to(torch.float32 if dt == 7 else torch.bfloat16).cuda()
        y = torch.zeros_like(x)
        comm.all_reduce(x.data_ptr(), y.data_ptr(), 4099, dt, nccl.ncclSum, sp)
        torch.cuda.synchronize()
        return comm.coll_algo(AR, 4099, dt), y.cpu().view(torch.uint8)

    bf0, f0 = ar(9), ar(7)
    comm.set_sum_fp32(1)
    wide = ar(9)
    eff = comm.set_sum_fp32_ring_threshold(1)
    ring = ar(9)
    comm.set_sum_fp32(0)  # the threshold stays set
    off = ar(9)
    comm.set_sum_fp32(1)
    f1 = ar(7)
    bad = [("level 1", wide[0])] * (wide[0] != "direct") + [("effective", eff)] * (eff != 1)
    bad += [("threshold", ring[0])] * (ring[0] != "ring" or not torch.equal(ring[1], wide[1]))
    bad += [("level 0", off[0])] * (off[0] != bf0[0] or not torch.equal(off[1], bf0[1]))
    return bad + [("f32", f1[0])] * (f1[0] != f0[0] or not torch.equal(f1[1], f0[1]))


def main():
    rank, n, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3])), rank)
    bad = {"exact": case_exact, "order": case_order, "switch": case_switch}[case](
        comm, rank, n, torch.cuda.current_stream().cuda_stream)
    err = comm.async_error()
    comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
