#!/usr/bin/env python3
"""One rank of the LL send / recv tests (tests/test_gpu_p2p_ll.py): argv rank nranks uid_hex case.
Payloads, guarded destinations and the grouped exchange are mp_p2p_worker's; every comparison is byte-exact."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests import _mp  # noqa: E402
from tests.mp_p2p_worker import SENTINEL, U8, Dest, Src, exchange_sizes, payload  # noqa: E402
from vccl_amd import nccl  # noqa: E402

# threshold 4096, LL step 1024: around a line, a step and the threshold; 0 and 4097 are not LL
SIZES = (0, 1, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097)
N_LL = sum(0 < s <= 4096 for s in SIZES)


def stats(comm, before, n_ll, n_all, what):  # vcclCommP2pStats since `before`: n_ll LL messages of n_all sends and recvs
    got = tuple(a - b for a, b in zip(comm.p2p_stats(), before))
    return [] if got == (n_ll, n_all - n_ll) else [(what, "stats", got, "want", (n_ll, n_all - n_ll))]


def case_sizes(comm, rank, n, sp):
    before = comm.p2p_stats()
    bad = exchange_sizes(comm, rank, n, sp, 0, SIZES, (U8,), (0, 1, 3), (0, 2, 5))
    return bad + stats(comm, before, 18 * N_LL, 18 * len(SIZES), "sizes")


def case_once(comm, rank, n, sp):
    """The size list once; a comm initialised without the threshold has no LL FIFOs and stays at 0."""
    before = comm.p2p_stats()
    on = comm.set_p2p_ll_threshold(4096) > 0
    bad = exchange_sizes(comm, rank, n, sp, 2000, SIZES, (U8,), (1,), (2,))
    return bad + stats(comm, before, 2 * N_LL if on else 0, 2 * len(SIZES), "once")


def back_to_back(comm, rank, sp, tag0):
    """40 ungrouped Send / Recv, the direction and 8 B / 4096 B alternating: 50 steps each way, the short
    message on the long one's stale lines."""
    bad, peer = [], 1 - rank
    for it in range(40):
        nb, tag, sender = (8, 4096)[(it // 2) % 2], tag0 + it, rank == it % 2
        src, dst = Src(payload(nb, rank, peer, tag), it % 3), Dest(nb, it % 5)
        comm.send(src.ptr, nb, U8, peer, sp) if sender else comm.recv(dst.ptr, nb, U8, peer, sp)
        torch.cuda.synchronize()
        bad += [] if sender or dst.ok(payload(nb, peer, rank, tag)) else [("back_to_back", tag0, it, nb)]
    return bad


def case_counters(comm, rank, n, sp):
    before = comm.p2p_stats()
    return back_to_back(comm, rank, sp, 3000) + stats(comm, before, 40, 40, "counters")


def case_wrap(comm, rank, n, sp):
    bad = []
    for step in (0x7FFFFFF0, 0xFFFFFFF0):  # across bit 31, then across bit 32 of the step
        torch.cuda.synchronize()
        comm.debug_set_p2p_ll_steps(step)
        bad += back_to_back(comm, rank, sp, 4000 + (step >> 28))
    return bad


def case_mixed(comm, rank, n, sp):
    nxt, prv, sizes = (rank + 1) % n, (rank - 1) % n, (64, 300 << 10, 2048)
    before = comm.p2p_stats()
    srcs = [Src(payload(nb, rank, nxt, 5000 + k), k) for k, nb in enumerate(sizes)]
    dsts = [Dest(nb, 2 * k) for k, nb in enumerate(sizes)]
    torch.cuda.synchronize()
    nccl.group_start()
    for k, nb in enumerate(sizes):
        comm.send(srcs[k].ptr, nb, U8, nxt, sp)
        comm.recv(dsts[k].ptr, nb, U8, prv, sp)
    nccl.group_end()
    torch.cuda.synchronize()
    bad = [("shift", k) for k, nb in enumerate(sizes) if not dsts[k].ok(payload(nb, prv, rank, 5000 + k))]
    bad += stats(comm, before, 4, 6, "shift")

    def nb_of(a, b):  # pair a -> b of the all-to-allv: one empty, LL sizes where a + b is odd, FIFO sizes else
        return 0 if (a, b) == (2, 0) else 100 + 900 * a + 31 * b if (a + b) % 2 else 5000 + 4001 * a + 911 * b
    sc, rc = [nb_of(rank, p) for p in range(n)], [nb_of(p, rank) for p in range(n)]
    sd, rd = [list(itertools.accumulate([0] + c[:-1])) for c in (sc, rc)]
    send = torch.cat([payload(c, rank, p, 5100) for p, c in enumerate(sc)])
    dst = Dest(sum(rc), 3)
    before = comm.p2p_stats()
    torch.cuda.synchronize()
    comm.all_to_allv(send.data_ptr(), sc, sd, dst.ptr, rc, rd, U8, sp)
    torch.cuda.synchronize()
    bad += [] if dst.ok(torch.cat([payload(c, p, rank, 5100) for p, c in enumerate(rc)])) else [("alltoallv",)]
    n_ll = sum(0 < c <= 4096 for cs in (sc, rc) for p, c in enumerate(cs) if p != rank)
    return bad + stats(comm, before, n_ll, 2 * n, "alltoallv")


def case_capture(comm, rank, n, sp):
    nb, peer = 2048, 1 - rank
    bad = exchange_sizes(comm, rank, n, sp, 6000, (nb, 8), (U8,), (0,), (0,))
    src, dst = torch.zeros(nb, dtype=torch.uint8, device="cuda"), Dest(nb)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        nccl.group_start()
        comm.send(src.data_ptr(), nb, U8, peer, s.cuda_stream)
        comm.recv(dst.ptr, nb, U8, peer, s.cuda_stream)
        nccl.group_end()
        g.capture_end()
    for it in range(3):  # the device-resident steps: every replay moves on
        src.copy_(payload(nb, rank, peer, 6010 + it))
        dst.buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        bad += [] if dst.ok(payload(nb, peer, rank, 6010 + it)) else [("replay", it)]
    return bad + exchange_sizes(comm, rank, n, sp, 6020, (nb, 4096), (U8,), (3,), (5,))


if __name__ == "__main__":
    rank, n, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3])), rank)
    bad = globals()["case_" + case](comm, rank, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = comm.async_error()
    comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)
