#!/usr/bin/env python3
"""One rank of the point-to-point tests (tests/test_gpu_p2p.py).

argv: rank nranks uid_hex case
ncclSend / ncclRecv / ncclAllToAll / ncclAllToAllv over the per-peer FIFOs.
Every received byte is compared with a seeded payload both ends can compute;
destinations are pre-filled with a sentinel and carry 64 guard bytes on each
side that must stay untouched.  Exit 0 on success."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import _mp  # noqa: E402
from vccl_amd import nccl  # noqa: E402

GUARD = 64
SENTINEL = 0xA5
U8, BF16, F32 = nccl.ncclUint8, nccl.ncclBfloat16, nccl.ncclFloat32
ESZ = {U8: 1, BF16: 2, F32: 4}
# the size list of case 1 under the test geometry (step 16 KiB, 2 parts, a
# second part from 4 KiB): none, sub-pack, one part, a step and one byte more,
# a FIFO wrap (8 slots) and 300 KiB = two wraps on both parts
SIZES = (0, 1, 17, 4095, 16384, 16385, 8 * 16384 + 3, 300 << 10)


def payload(nbytes, src, dst, tag):
    g = torch.Generator(device="cpu").manual_seed((tag * 64 + src) * 64 + dst + 1)
    return torch.randint(0, 256, (max(nbytes, 1),), dtype=torch.uint8, generator=g)[:nbytes].cuda()


class Dest:
    """A destination of nbytes at byte offset `off` past a 16-byte boundary,
    sentinel-filled, with GUARD bytes on each side."""

    def __init__(self, nbytes, off=0):
        self.nbytes, self.lo = nbytes, GUARD + off
        self.buf = torch.full((nbytes + off + 2 * GUARD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def data(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    def ok(self, want):
        """The payload exact, every byte around it still the sentinel."""
        return (torch.equal(self.data(), want) and bool((self.buf[:self.lo] == SENTINEL).all())
                and bool((self.buf[self.lo + self.nbytes:] == SENTINEL).all()))

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


class Src:
    def __init__(self, data, off=0):
        self.buf = torch.zeros(data.numel() + off + 16, dtype=torch.uint8, device="cuda")
        self.buf[off:off + data.numel()] = data
        self.ptr = self.buf.data_ptr() + off


def elems(nbytes, dtype):
    return -(-nbytes // ESZ[dtype])


def exchange_sizes(comm, rank, n, sp, tag0, sizes, dtypes, soffs, doffs):
    """n = 2: a grouped exchange both ways per (size, offsets, type)."""
    bad = []
    peer = 1 - rank
    tag = tag0
    for dt in dtypes:
        for size in sizes:
            cnt = elems(size, dt)
            nb = cnt * ESZ[dt]
            for so in soffs:
                for do in doffs:
                    tag += 1
                    src = Src(payload(nb, rank, peer, tag), so)
                    dst = Dest(nb, do)
                    torch.cuda.synchronize()
                    nccl.group_start()
                    comm.send(src.ptr, cnt, dt, peer, sp)
                    comm.recv(dst.ptr, cnt, dt, peer, sp)
                    nccl.group_end()
                    torch.cuda.synchronize()
                    if not dst.ok(payload(nb, peer, rank, tag)):
                        bad.append(("exchange", dt, size, so, do))
    return bad


def case_exchange(comm, rank, n, sp):
    return exchange_sizes(comm, rank, n, sp, 0, SIZES, (U8, BF16, F32), (0, 1, 3), (0, 2, 5))


def case_fences(comm, rank, n, sp):
    return exchange_sizes(comm, rank, n, sp, 5000, SIZES, (U8,), (0,), (0,))


def case_ungrouped(comm, rank, n, sp):
    """Rank 0 Send, rank 1 Recv, then the reverse; 20 iterations back to back
    (the persistent step counters)."""
    bad = []
    peer = 1 - rank
    for it in range(20):
        for sender in (0, 1):
            for k, nb in enumerate((1 << 10, 300 << 10)):
                tag = 100 + it * 4 + sender * 2 + k
                if rank == sender:
                    src = Src(payload(nb, rank, peer, tag))
                    comm.send(src.ptr, nb, U8, peer, sp)
                    torch.cuda.synchronize()
                else:
                    dst = Dest(nb)
                    comm.recv(dst.ptr, nb, U8, peer, sp)
                    torch.cuda.synchronize()
                    if not dst.ok(payload(nb, peer, rank, tag)):
                        bad.append(("ungrouped", it, sender, nb))
    return bad


def case_ring_shift(comm, rank, n, sp):
    """Send to r + 1, recv from r - 1 in a group; then two and three messages
    to the same peer in one group (sweep order: matched in call order)."""
    bad = []
    nxt, prv = (rank + 1) % n, (rank - 1) % n
    for m, sizes in enumerate(((70_001,), (5, 200 << 10), (140_000, 0, 4097))):
        srcs = [Src(payload(nb, rank, nxt, 300 + 8 * m + k)) for k, nb in enumerate(sizes)]
        dsts = [Dest(nb, k) for k, nb in enumerate(sizes)]
        torch.cuda.synchronize()
        nccl.group_start()
        for k, nb in enumerate(sizes):  # recvs first on odd ranks: call order across kinds is free
            if rank % 2:
                comm.recv(dsts[k].ptr, nb, U8, prv, sp)
                comm.send(srcs[k].ptr, nb, U8, nxt, sp)
            else:
                comm.send(srcs[k].ptr, nb, U8, nxt, sp)
                comm.recv(dsts[k].ptr, nb, U8, prv, sp)
        nccl.group_end()
        torch.cuda.synchronize()
        for k, nb in enumerate(sizes):
            if not dsts[k].ok(payload(nb, prv, rank, 300 + 8 * m + k)):
                bad.append(("shift", m, k))
    return bad


def pair_size(a, b, n):
    """A distinct size per ordered pair, one of them zero."""
    return 0 if (a, b) == (1, 2) else 1000 * (a * n + b) + 17 * a + b + (200 << 10 if (a + b) % 3 == 0 else 0)


def case_full_exchange(comm, rank, n, sp):
    bad = []
    # self pairs: ranks 0 and 1 out of place, rank 2 in place, rank 3 none
    peers = [p for p in range(n) if p != rank]
    srcs = {p: Src(payload(pair_size(rank, p, n), rank, p, 400), p % 3) for p in range(n)}
    dsts = {p: Dest(pair_size(p, rank, n), p % 2) for p in range(n)}
    inplace = Src(payload(5000, rank, rank, 401))
    torch.cuda.synchronize()
    nccl.group_start()
    for p in peers:
        comm.send(srcs[p].ptr, pair_size(rank, p, n), U8, p, sp)
    if rank in (0, 1):
        comm.send(srcs[rank].ptr, pair_size(rank, rank, n), U8, rank, sp)
        comm.recv(dsts[rank].ptr, pair_size(rank, rank, n), U8, rank, sp)
    elif rank == 2:
        comm.send(inplace.ptr, 5000, U8, rank, sp)
        comm.recv(inplace.ptr, 5000, U8, rank, sp)
    for p in reversed(peers):
        comm.recv(dsts[p].ptr, pair_size(p, rank, n), U8, p, sp)
    nccl.group_end()
    torch.cuda.synchronize()
    for p in range(n):
        if p == rank and rank not in (0, 1):
            if not dsts[p].untouched():
                bad.append(("full: unused self destination written", p))
        elif not dsts[p].ok(payload(pair_size(p, rank, n), p, rank, 400)):
            bad.append(("full", p))
    if not torch.equal(inplace.buf[:5000], payload(5000, rank, rank, 401)):
        bad.append(("full: in-place self pair changed",))
    # an unmatched self send: ncclGroupEnd fails, nothing of the group runs
    dsts = {p: Dest(3000, 1) for p in peers}
    src = Src(payload(3000, rank, rank, 402))
    torch.cuda.synchronize()
    nccl.group_start()
    for p in peers:
        comm.send(src.ptr, 3000, U8, p, sp)
        comm.recv(dsts[p].ptr, 3000, U8, p, sp)
    comm.send(src.ptr, 3000, U8, rank, sp)
    rc = nccl.lib().ncclGroupEnd()
    torch.cuda.synchronize()
    if rc != nccl.ncclInvalidUsage:
        bad.append(("unmatched self send: ncclGroupEnd returned", rc))
    if not all(d.untouched() for d in dsts.values()):
        bad.append(("unmatched self send: a buffer was written",))
    # ... and the comm still works
    bad += case_ring_shift(comm, rank, n, sp)
    return bad


def case_all_to_all(comm, rank, n, sp):
    bad = []
    for i, cnt in enumerate((1, 1000, 70_001)):
        nb = cnt * 4
        send = torch.cat([payload(nb, rank, p, 500 + i) for p in range(n)])
        dst = Dest(nb * n)
        torch.cuda.synchronize()
        comm.all_to_all(send.data_ptr(), dst.ptr, cnt, F32, sp)
        torch.cuda.synchronize()
        if not dst.ok(torch.cat([payload(nb, p, rank, 500 + i) for p in range(n)])):
            bad.append(("alltoall", cnt))
    # all-to-allv: uneven counts, a zero, gaps between the blocks (bf16 elements)
    def cnt_of(a, b):
        return 0 if (a, b) == (2, 0) else 37 + 4001 * a + 911 * b + (90_000 if a == b else 0)
    scounts = [cnt_of(rank, p) for p in range(n)]
    rcounts = [cnt_of(p, rank) for p in range(n)]
    sdispls, rdispls, so, ro = [], [], 3, 5
    for p in range(n):
        sdispls.append(so)
        rdispls.append(ro)
        so += scounts[p] + 7 * (p + 1)
        ro += rcounts[p] + 3 * (p + 2)
    send = torch.zeros(so * 2, dtype=torch.uint8, device="cuda")
    for p in range(n):
        send[sdispls[p] * 2:(sdispls[p] + scounts[p]) * 2] = payload(scounts[p] * 2, rank, p, 510)
    dst = Dest(ro * 2)
    want = torch.full((ro * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    for p in range(n):
        want[rdispls[p] * 2:(rdispls[p] + rcounts[p]) * 2] = payload(rcounts[p] * 2, p, rank, 510)
    torch.cuda.synchronize()
    comm.all_to_allv(send.data_ptr(), scounts, sdispls, dst.ptr, rcounts, rdispls, BF16, sp)
    torch.cuda.synchronize()
    if not dst.ok(want):
        bad.append(("alltoallv",))
    # in place is refused
    rc = nccl.lib().ncclAllToAll(dst.ptr, dst.ptr, 4, F32, comm.handle, sp)
    if rc != nccl.ncclInvalidArgument:
        bad.append(("alltoall in place returned", rc))
    return bad


def case_mixed(comm, rank, n, sp):
    """All-reduce, a grouped exchange, all-reduce on one comm and two streams,
    no host wait in between: results as if sequential."""
    bad = []
    cnt = 300_001
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    nxt, prv = (rank + 1) % n, (rank - 1) % n
    for it in range(3):
        base = (torch.arange(cnt, device="cuda") % 7 + it).float()
        x = base * (rank + 1)
        y = torch.full((cnt,), float("nan"), device="cuda")
        z = torch.full((cnt,), float("nan"), device="cuda")
        w = torch.full((cnt,), float("nan"), device="cuda")
        torch.cuda.synchronize()
        comm.all_reduce(x.data_ptr(), y.data_ptr(), cnt, F32, nccl.ncclSum, s1.cuda_stream)
        nccl.group_start()
        comm.send(y.data_ptr(), cnt, F32, nxt, s2.cuda_stream)
        comm.recv(z.data_ptr(), cnt, F32, prv, s2.cuda_stream)
        nccl.group_end()
        comm.all_reduce(z.data_ptr(), w.data_ptr(), cnt, F32, nccl.ncclSum, s1.cuda_stream)
        torch.cuda.synchronize()
        tot = n * (n + 1) // 2
        if not (torch.equal(y, base * tot) and torch.equal(z, base * tot) and torch.equal(w, base * (tot * n))):
            bad.append(("mixed", it))
    return bad


def case_arg_errors(comm, rank, n, sp):
    bad = []
    L = nccl.lib()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p, h = buf.data_ptr(), comm.handle
    inv = nccl.ncclInvalidArgument
    checks = {
        "send peer -1": L.ncclSend(p, 4, U8, -1, h, sp), "send peer n": L.ncclSend(p, 4, U8, n, h, sp),
        "recv peer -1": L.ncclRecv(p, 4, U8, -1, h, sp), "recv peer n": L.ncclRecv(p, 4, U8, n, h, sp),
        "send type": L.ncclSend(p, 4, nccl.ncclNumTypes, 1 - rank, h, sp),
        "recv type": L.ncclRecv(p, 4, -1, 1 - rank, h, sp),
        "send NULL": L.ncclSend(None, 4, U8, 1 - rank, h, sp), "recv NULL": L.ncclRecv(None, 4, U8, 1 - rank, h, sp),
        "alltoall type": L.ncclAllToAll(p, p + 32, 1, 99, h, sp),
    }
    bad += [(k, v) for k, v in checks.items() if v != inv]
    if L.ncclSend(None, 0, U8, 1 - rank, h, sp) != 0 or L.ncclRecv(None, 0, U8, 1 - rank, h, sp) != 0:
        bad.append(("NULL buffer with count 0 refused",))
    # a group containing one bad call fails at End and launches nothing
    dst = Dest(32)
    nccl.group_start()
    comm.send(p, 32, U8, 1 - rank, sp)
    comm.recv(dst.ptr, 32, U8, 1 - rank, sp)
    if L.ncclSend(p, 4, U8, n, h, sp) != inv:
        bad.append(("bad call in group",))
    if L.ncclGroupEnd() != inv:
        bad.append(("group with a bad call did not fail",))
    torch.cuda.synchronize()
    if not dst.untouched():
        bad.append(("group with a bad call wrote a buffer",))
    bad += exchange_sizes(comm, rank, n, sp, 700, (4097,), (U8,), (1,), (2,))
    return bad


def case_defaults(comm, rank, n, sp):
    """Library defaults, n = 8 on a shared GPU: the co-residency caps."""
    bad = []
    for i, nb in enumerate((64 << 10, 2 << 20)):
        send = torch.cat([payload(nb, rank, p, 800 + i) for p in range(n)])
        dst = Dest(nb * n)
        torch.cuda.synchronize()
        comm.all_to_all(send.data_ptr(), dst.ptr, nb, U8, sp)
        torch.cuda.synchronize()
        if not dst.ok(torch.cat([payload(nb, p, rank, 800 + i) for p in range(n)])):
            bad.append(("defaults", nb))
    return bad


def case_capture(comm, rank, n, sp):
    """One stream captures a grouped exchange of 40 KiB (no fork inside the
    capture); three replays with fresh payloads, eager exchanges around."""
    nb = 40 << 10
    peer = 1 - rank
    bad = exchange_sizes(comm, rank, n, sp, 900, (nb,), (U8,), (0,), (0,))
    src = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    dst = Dest(nb)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        nccl.group_start()
        comm.send(src.data_ptr(), nb, U8, peer, s.cuda_stream)
        comm.recv(dst.ptr, nb, U8, peer, s.cuda_stream)
        nccl.group_end()
        g.capture_end()
    for it in range(3):
        src.copy_(payload(nb, rank, peer, 910 + it))
        dst.buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if not dst.ok(payload(nb, peer, rank, 910 + it)):
            bad.append(("replay", it))
    bad += exchange_sizes(comm, rank, n, sp, 920, (nb, 300 << 10), (U8,), (3,), (5,))
    return bad


CASES = {"exchange": case_exchange, "ungrouped": case_ungrouped, "ring_shift": case_ring_shift,
         "full_exchange": case_full_exchange, "all_to_all": case_all_to_all, "mixed": case_mixed,
         "arg_errors": case_arg_errors, "defaults": case_defaults, "capture": case_capture, "fences": case_fences}


def main():
    rank, n = int(sys.argv[1]), int(sys.argv[2])
    uid = nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3]))
    case = sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, uid, rank)
    sp = torch.cuda.current_stream().cuda_stream
    bad = CASES[case](comm, rank, n, sp)
    torch.cuda.synchronize()
    err = comm.async_error()
    comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
