#!/usr/bin/env python3
"""One rank of the zero-copy all-to-all tests (tests/test_gpu_reg_a2a.py).

argv: rank nranks uid_hex case        (case "single": one process, ncclCommInitAll)
The parent sets the shared-GPU geometry of the all-to-all tests plus
VCCL_REG_A2A_THRESHOLD=32768 (or leaves it out, the "off" cases).  A call is
run twice: with its sendbuff registered (the zero-copy path) and on
unregistered copies of the same layout (the fallback through the FIFOs); the
two outputs are compared byte for byte, guard bytes included, and both with
the value computed on the host.  After registering, a case runs one small
warm-up collective and synchronises, so every peer's registry write is ordered
before every import and the expected path is deterministic.  Every case ends by
comparing vcclCommRegA2aStats with what it expects, on every rank.  Exit 0 on
success."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _mp  # noqa: E402
from tests.mp_direct_reg_worker import AR, Buf, Call, SENTINEL, warmup  # noqa: E402
from vccl_amd import nccl  # noqa: E402

U8, F32, BF16 = nccl.ncclUint8, nccl.ncclFloat32, nccl.ncclBfloat16
THRESH = 32768


def payload(tag, rank, nbytes):
    return np.random.default_rng((tag * 16 + rank) * 4 + 3).integers(0, 256, nbytes, dtype=np.uint8)


def uniform_matrix(n, nbytes):
    """(send bytes, send offsets, receive offsets) of ncclAllToAll, all n x n."""
    return ([[nbytes] * n for _ in range(n)], [[p * nbytes for p in range(n)] for _ in range(n)],
            [[p * nbytes for p in range(n)] for _ in range(n)])


def v_matrix(n, seed, small_rank=None):
    """Random counts with zero pairs, a zero row and a zero column, blocks laid
    out in shuffled (non-monotonic) order with gaps; at least one pair of every
    rank reaches the threshold, except small_rank's: all of its pairs, sent and
    received, stay below it."""
    rng = np.random.default_rng(seed)
    sizes = [0, 0, 1, 17, 40, 4096, 16385, THRESH - 1, THRESH, THRESH + 1, 100_003, 300_001]
    sb = [[int(rng.choice(sizes)) for _ in range(n)] for _ in range(n)]
    zr = int(rng.integers(n))  # rank zr sends nothing, rank zc receives nothing
    if zr == small_rank:
        zr = (zr + 1) % n
    zc = (zr + 1) % n
    for p in range(n):
        sb[zr][p] = 0
        sb[p][zc] = 0
    for r in range(n):  # every rank has one big pair: what it sends to zr (zr: what it receives)
        if r != zr:
            sb[r][zr] = 70_001 + 16 * r
    if small_rank is not None:
        for p in range(n):
            sb[small_rank][p] = min(sb[small_rank][p], 1000 + p)
            sb[p][small_rank] = min(sb[p][small_rank], 2000 + p)

    def offsets(lengths):
        order = rng.permutation(n)
        off, pos = [0] * n, int(rng.choice([0, 1, 4]))
        for p in order:
            off[p] = pos
            pos += lengths[p] + int(rng.choice([0, 3, 16]))
        return off
    so = [offsets(sb[r]) for r in range(n)]
    ro = [offsets([sb[p][r] for p in range(n)]) for r in range(n)]
    return sb, so, ro


class A2a:
    """One all-to-all on buffers of its own.  mat = (sb, so, ro) in bytes;
    esz: the element size the call is issued with (every entry a multiple);
    soff / roff: the user pointers' distance from the registered / allocated base."""

    def __init__(self, rank, n, mat, tag, uniform, esz=1, soff=0, roff=0):
        self.rank, self.n, self.uniform, self.esz, self.tag = rank, n, uniform, esz, tag
        self.sb, self.so, self.ro = mat
        self.send = Buf(self.extent(rank, True), soff)
        self.recv = Buf(self.extent(rank, False), roff)
        self.fill(tag)

    def extent(self, r, send):
        if send:
            return max([self.so[r][p] + self.sb[r][p] for p in range(self.n)] + [1])
        return max([self.ro[r][p] + self.sb[p][r] for p in range(self.n)] + [1])

    def fill(self, tag):
        """Fresh input, a cleared output, and the value the host computes."""
        n, r = self.n, self.rank
        self.send.put(payload(tag, r, self.send.n))
        self.recv.put(np.full(self.recv.n, SENTINEL, np.uint8))
        self.want = np.full(self.recv.n, SENTINEL, np.uint8)
        for p in range(n):
            src = payload(tag, p, self.extent(p, True))
            self.want[self.ro[r][p]:self.ro[r][p] + self.sb[p][r]] = src[self.so[p][r]:self.so[p][r] + self.sb[p][r]]

    def pair_bytes(self):
        return self.sb[0][0]

    def largest(self):
        r = self.rank
        return max([max(self.sb[r][p], self.sb[p][r]) for p in range(self.n) if p != r] + [0])

    def issue(self, comm, sp):
        e, r, n = self.esz, self.rank, self.n
        if self.uniform:
            comm.all_to_all(self.send.ptr, self.recv.ptr, self.pair_bytes() // e, U8 if e == 1 else BF16, sp)
        else:
            comm.all_to_allv(self.send.ptr, [self.sb[r][p] // e for p in range(n)], [self.so[r][p] // e for p in range(n)],
                             self.recv.ptr, [self.sb[p][r] // e for p in range(n)], [self.ro[r][p] // e for p in range(n)],
                             U8 if e == 1 else BF16, sp)

    def check(self, other=None):
        out = []
        if not self.recv.guards_ok() or not self.send.guards_ok():
            out.append("guards")
        if not np.array_equal(self.recv.data(), self.want):
            out.append("value")
        if not np.array_equal(self.send.data(), payload(self.tag, self.rank, self.send.n)):
            out.append("sendbuff written")
        if other is not None and not torch.equal(self.recv.t, other.recv.t):
            out.append("differs from the FIFO path")
        return out


class Stats:
    def __init__(self, comm, thresh=THRESH):
        self.comm, self.thresh = comm, thresh
        self.base = comm.reg_a2a_stats()
        self.want = [0, 0, 0]  # eligible launches, zero-copy, fallback

    def expect(self, call, zero_copy, times=1, index=0):
        if nccl.reg_a2a_eligible(call.uniform, call.pair_bytes(), self.thresh, index):
            self.want[0] += times
            self.want[1 if zero_copy else 2] += times

    def bad(self):
        d = [a - b for a, b in zip(self.comm.reg_a2a_stats(), self.base)]
        return [] if d == self.want else [("reg a2a stats", d, self.want)]


def run_pairs(comm, sp, calls, st, zero_copy=True):
    """calls = [(registered twin, unregistered twin)]: both issued, then
    compared with each other and the host's value; at most 32 registrations."""
    bad = []
    for lo in range(0, len(calls), 24):
        part = calls[lo:lo + 24]
        for a, _ in part:
            a.send.register(comm)
        warmup(comm, sp)
        for a, b in part:
            a.issue(comm, sp)
            b.issue(comm, sp)
            st.expect(a, zero_copy)
            st.expect(b, False)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(part):
            bad += [(lo + i, w) for w in a.check(b)] + [(lo + i, "fifo: " + w) for w in b.check()]
        for a, _ in part:
            a.send.deregister(comm)
    return bad


def twins(rank, n, mat, tag, uniform, **kw):
    return A2a(rank, n, mat, tag, uniform, **kw), A2a(rank, n, mat, tag, uniform, **kw)


# -------------------------------------------------------------------- cases
def case_uniform(comm, rank, n, sp):
    """u8 at 32 767 (no eligible launch), 32 768, 32 769 and 1 MiB + 3 bytes per
    pair; bf16 at the same edge in elements; the send and receive pointers 0, 1
    and 4 bytes past the registered base, independently."""
    st = Stats(comm)
    calls = [twins(rank, n, uniform_matrix(n, b), 100 + i, True)
             for i, b in enumerate((THRESH - 1, THRESH, THRESH + 1, (1 << 20) + 3))]
    calls += [twins(rank, n, uniform_matrix(n, 2 * c), 110 + i, True, esz=2)
              for i, c in enumerate((THRESH // 2 - 1, THRESH // 2, THRESH // 2 + 1))]
    calls += [twins(rank, n, uniform_matrix(n, THRESH + 1), 120 + 3 * i + j, True, soff=so, roff=ro)
              for i, so in enumerate((0, 1, 4)) for j, ro in enumerate((0, 1, 4)) if so or ro]
    bad = run_pairs(comm, sp, calls, st)
    if st.want != [26, 13, 13]:  # 3 + 2 + 8 eligible specs, each on both paths
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_small(comm, rank, n, sp):
    """The threshold at 16, 40 bytes per pair: one short slice per block, every
    other workgroup of a v-call's grid owns an empty one."""
    if comm.set_reg_a2a_threshold(16) != 16:
        return [("threshold",)]
    st = Stats(comm, 16)
    sb, so, ro = uniform_matrix(n, 40)
    calls = [twins(rank, n, (sb, so, ro), 200, True), twins(rank, n, (sb, so, ro), 201, False),
             twins(rank, n, uniform_matrix(n, 15), 202, True)]  # below 16: today's path
    bad = run_pairs(comm, sp, calls, st)
    if st.want != [4, 2, 2]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_v(comm, rank, n, sp):
    """Random v-calls, zero-copy; then one whose rank-1 pairs all stay below the
    threshold: rank 1 votes no, fallback is counted on all ranks."""
    st = Stats(comm)
    calls = [twins(rank, n, v_matrix(n, 300 + i), 300 + i, False, soff=(0, 1, 4)[i % 3], roff=(4, 0, 1)[i % 3])
             for i in range(4)]
    bad = run_pairs(comm, sp, calls, st)
    small = [twins(rank, n, v_matrix(n, 350, small_rank=1), 350, False)]
    if (small[0][0].largest() >= THRESH) != (rank != 1):
        bad.append(("the small-rank matrix", rank, small[0][0].largest()))
    bad += run_pairs(comm, sp, small, st, zero_copy=False)
    if st.want != [10, 4, 6]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_mixed(comm, rank, n, sp):
    """n = 4.  Rank 1 unregistered; rank 1 registered 16 bytes short of its last
    block: fallback on all four ranks.  Only the recvbuffs unregistered (they
    never are registered here) with every sendbuff registered: zero-copy; and
    again after another warm-up."""
    bad = []
    st = Stats(comm)
    for step, (reg, short, zc) in enumerate(((False, 0, False), (True, 16, False), (True, 0, True), (True, 0, True))):
        c = A2a(rank, n, uniform_matrix(n, 40_000), 400 + step, True)
        if rank != 1 or reg:
            c.send.register(comm, short if rank == 1 else 0)
        warmup(comm, sp)
        c.issue(comm, sp)
        st.expect(c, zc)
        torch.cuda.synchronize()
        bad += [(step, w) for w in c.check()]
        c.send.deregister(comm)
    if st.want != [4, 2, 2]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def ring_bufs(rank, n, tag, nbytes=50_000):
    s, r = Buf(nbytes), Buf(nbytes)
    s.put(payload(tag, rank, nbytes))
    return s, r, payload(tag, (rank - 1) % n, nbytes)


def case_group(comm, rank, n, sp):
    """Two eligible all-to-alls and a plain send / recv ring in one group,
    registered (zero-copy) and not (fallback); then nine all-to-alls in one
    group: the ninth takes today's path."""
    bad = []
    st = Stats(comm)
    for reg in (True, False):
        a = A2a(rank, n, uniform_matrix(n, 40_001), 500, True)
        b = A2a(rank, n, v_matrix(n, 501), 501, False)
        s, r, want = ring_bufs(rank, n, 502)
        if reg:
            a.send.register(comm)
            b.send.register(comm)
        warmup(comm, sp)
        nccl.group_start()
        a.issue(comm, sp)
        comm.send(s.ptr, s.n, U8, (rank + 1) % n, sp)  # per peer, sends and recvs keep one order on both ends
        comm.recv(r.ptr, r.n, U8, (rank - 1) % n, sp)
        b.issue(comm, sp)
        nccl.group_end()
        st.expect(a, reg, index=0)
        st.expect(b, reg, index=1)
        torch.cuda.synchronize()
        bad += [(reg, "a", w) for w in a.check()] + [(reg, "b", w) for w in b.check()]
        if not np.array_equal(r.data(), want) or not r.guards_ok():
            bad.append((reg, "ring"))
        a.send.deregister(comm)
        b.send.deregister(comm)
    nine = [A2a(rank, n, uniform_matrix(n, THRESH + 16 * i), 510 + i, True) for i in range(9)]
    for c in nine:
        c.send.register(comm)
    warmup(comm, sp)
    before = comm.a2a_stats_ex()
    nccl.group_start()
    for c in nine:
        c.issue(comm, sp)
    nccl.group_end()
    for i, c in enumerate(nine):
        st.expect(c, True, index=i)
    torch.cuda.synchronize()
    bad += [("nine", i, w) for i, c in enumerate(nine) for w in c.check()]
    d = [x - y for x, y in zip(comm.a2a_stats_ex(), before)]
    if d != [0, 0, 0, 0, 2 * n]:  # the ninth alone is counted: every pair on the FIFOs, as today
        bad.append(("a2a stats", d))
    if st.want != [12, 10, 2]:
        bad.append(("planned", st.want))
    return bad + st.bad()


B2B = ("zc", "fb", "ar", "ll", "direct", "p2p")


def case_b2b(comm, rank, n, sp):
    """40 calls with no host synchronisation cycling this path zero-copy, its
    fallback, a zero-copy all-reduce, an LL all-to-all, a direct all-to-all and
    a plain send / recv ring; one synchronise at the end."""
    bad = []
    st = Stats(comm)
    ar_base = comm.reg_stats()
    plan = [(B2B[i % len(B2B)], 600 + i) for i in range(40)]
    calls = []
    for kind, tag in plan:
        if kind in ("zc", "fb"):
            mat, uni = (uniform_matrix(n, 50_001), True) if tag % 4 < 2 else (v_matrix(n, tag), False)
            calls.append(A2a(rank, n, mat, tag, uni))
            if kind == "zc":
                calls[-1].send.register(comm)
        elif kind == "ar":
            calls.append(Call(rank, n, (AR, F32, nccl.ncclSum, 12_001, False, 0), tag))
            for b in calls[-1].bufs():
                b.register(comm)
        elif kind in ("ll", "direct"):
            calls.append(A2a(rank, n, uniform_matrix(n, 2048 if kind == "ll" else 12_288), tag, True))
        else:
            calls.append(ring_bufs(rank, n, tag))
    warmup(comm, sp)
    before = comm.a2a_stats_ex()
    for (kind, tag), c in zip(plan, calls):
        if kind == "p2p":
            nccl.group_start()
            comm.send(c[0].ptr, c[0].n, U8, (rank + 1) % n, sp)
            comm.recv(c[1].ptr, c[1].n, U8, (rank - 1) % n, sp)
            nccl.group_end()
            continue
        c.issue(comm, sp)
        if kind in ("zc", "fb"):
            st.expect(c, kind == "zc")
    torch.cuda.synchronize()
    for i, ((kind, tag), c) in enumerate(zip(plan, calls)):
        if kind == "p2p":
            if not np.array_equal(c[1].data(), c[2]) or not c[1].guards_ok():
                bad.append((i, kind))
        elif c.check():
            bad.append((i, kind, c.check()))
    d = [x - y for x, y in zip(comm.a2a_stats_ex(), before)]
    n_ll, n_direct = sum(k == "ll" for k, _ in plan), sum(k == "direct" for k, _ in plan)
    if d != [n_ll, 2 * n * n_ll, n_direct, 2 * n * n_direct, 0]:
        bad.append(("a2a stats", d))
    ar = [x - y for x, y in zip(comm.reg_stats()[:3], ar_base[:3])]
    n_ar = sum(k == "ar" for k, _ in plan)
    if ar != [n_ar, n_ar, 0]:
        bad.append(("reg stats", ar))
    if st.want != [14, 7, 7]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_capture(comm, rank, n, sp):
    """[zero-copy, fallback] captured, replayed three times with fresh inputs;
    the counters grow with every replay.  Imports happen at eager enqueues only,
    so one eager eligible call precedes the capture."""
    bad = []
    st = Stats(comm)
    zc = A2a(rank, n, v_matrix(n, 700), 700, False, soff=1)
    fb = A2a(rank, n, uniform_matrix(n, 40_001), 701, True)
    zc.send.register(comm)
    warmup(comm, sp)
    zc.issue(comm, sp)
    st.expect(zc, True)
    torch.cuda.synchronize()
    bad += [("eager", w) for w in zc.check()]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        zc.issue(comm, s.cuda_stream)
        fb.issue(comm, s.cuda_stream)
        g.capture_end()
    for it in range(3):
        zc.fill(710 + 2 * it)
        zc.tag = 710 + 2 * it
        fb.fill(711 + 2 * it)
        fb.tag = 711 + 2 * it
        st.expect(zc, True)
        st.expect(fb, False)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        bad += [(it, "zc", w) for w in zc.check()] + [(it, "fb", w) for w in fb.check()] + st.bad()
    if st.want != [7, 4, 3]:
        bad.append(("planned", st.want))
    return bad


def case_wrap(comm, rank, n, sp):
    """The direct epoch seeded at 0xfffffffd, then four calls across the wrap:
    zero-copy (two positions), fallback (one), zero-copy, zero-copy."""
    bad = []
    st = Stats(comm)
    calls = [A2a(rank, n, uniform_matrix(n, 40_001) if i % 2 else v_matrix(n, 800 + i), 800 + i, bool(i % 2))
             for i in range(4)]
    for i, c in enumerate(calls):
        if i != 1:
            c.send.register(comm)
    comm.set_algo("ring")  # the warm-up leaves no inbox flag behind
    warmup(comm, sp)
    comm.set_algo(None)
    comm.debug_set_epochs(0xFFFFFFFD, 0xFFFFFFFD)
    for i, c in enumerate(calls):
        c.issue(comm, sp)
        st.expect(c, i != 1)
        torch.cuda.synchronize()
        if comm.async_error() or c.check():
            bad.append((i, c.check()))
    if st.want != [4, 3, 1]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_fences(comm, rank, n, sp):
    st = Stats(comm)
    calls = [twins(rank, n, uniform_matrix(n, THRESH + 1), 900, True, soff=1),
             twins(rank, n, v_matrix(n, 901), 901, False, roff=4)]
    bad = run_pairs(comm, sp, calls, st)
    if os.environ.get("VCCL_FENCES") != "1" or st.want != [4, 2, 2]:
        bad.append(("setup", st.want))
    return bad + st.bad()


def case_reregister(comm, rank, n, sp):
    """Deregister, then register another allocation that lands in the same
    entry: zero-copy, exact; the allocation is freed in between."""
    bad = []
    st = Stats(comm)
    for step in range(3):
        c = A2a(rank, n, uniform_matrix(n, 40_001 + step), 1000 + step, True)
        c.send.register(comm)
        if comm.reg_stats()[3] != 1:
            bad.append(("live", step))
        warmup(comm, sp)
        c.issue(comm, sp)
        st.expect(c, True)
        torch.cuda.synchronize()
        bad += [(step, w) for w in c.check()]
        c.send.deregister(comm)
        if step == 1:  # give the allocation back to the runtime before the next registration
            del c
            torch.cuda.empty_cache()
    if st.want != [3, 3, 0]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_off(comm, rank, n, sp):
    """The path is off: the stats stay zero, vcclCommSetRegA2aThreshold has no
    registry to switch on, and the call behaves as today — exact over the FIFOs,
    or refused as before on a comm without point-to-point connections."""
    bad = []
    c = A2a(rank, n, uniform_matrix(n, 40_001), 1100, True)
    c.send.register(comm)
    if comm.set_reg_a2a_threshold(THRESH) != 0:
        bad.append(("effective",))
    warmup(comm, sp)
    before = comm.a2a_stats_ex()
    no_p2p = os.environ.get("VCCL_P2P_BUFFERS") == "0" or os.environ.get("VCCL_NET_FORCE") == "1"
    try:
        c.issue(comm, sp)
        torch.cuda.synchronize()
        if no_p2p:
            bad.append(("not refused",))
        bad += c.check()
        d = [x - y for x, y in zip(comm.a2a_stats_ex(), before)]
        if d != [0, 0, 0, 0, 2 * n]:
            bad.append(("a2a stats", d))
    except nccl.VcclError as e:
        if not no_p2p or e.code != nccl.ncclInvalidUsage:
            bad.append(("refused", e.code))
    c.send.deregister(comm)
    if comm.reg_a2a_stats() != (0, 0, 0):
        bad.append(("stats", comm.reg_a2a_stats()))
    return bad


CASES = {"uniform": case_uniform, "small": case_small, "v": case_v, "mixed": case_mixed, "group": case_group,
         "b2b": case_b2b, "capture": case_capture, "wrap": case_wrap, "fences": case_fences,
         "reregister": case_reregister, "off": case_off}


def single_process(n):
    """ncclCommInitAll ranks in one process (the peers' buffers are addressed by
    raw pointer): each round one group holding every comm's all-to-all."""
    dev_of = [r % _mp.device_count() for r in range(n)]
    if _mp.shares_device(n):
        os.environ["VCCL_ALLOW_SHARED_DEVICE"] = "1"
    comms = nccl.Comm.init_all(dev_of)
    streams = []
    for r in range(n):
        torch.cuda.set_device(dev_of[r])
        streams.append(torch.cuda.Stream())
    bad = []

    def each(f):
        out = []
        for r in range(n):
            torch.cuda.set_device(dev_of[r])
            out.append(f(r))
        return out

    def grouped(calls):
        nccl.group_start()
        for r in range(n):
            calls[r].issue(comms[r], streams[r].cuda_stream)
        nccl.group_end()
        each(lambda r: torch.cuda.synchronize())

    base = [c.reg_a2a_stats() for c in comms]
    rounds = ((uniform_matrix(n, 40_001), True), (v_matrix(n, 1201), False))
    for i, (mat, uni) in enumerate(rounds):
        zc = each(lambda r: A2a(r, n, mat, 1200 + i, uni))
        fb = each(lambda r: A2a(r, n, mat, 1200 + i, uni))
        each(lambda r: zc[r].send.register(comms[r]))
        grouped(each(lambda r: Call(r, n, (AR, F32, nccl.ncclSum, 64, True, 0), 0)))  # the warm-up
        grouped(zc)
        grouped(fb)
        for r in range(n):
            torch.cuda.set_device(dev_of[r])
            bad += [(i, r, w) for w in zc[r].check(fb[r])] + [(i, r, "fifo: " + w) for w in fb[r].check()]
        each(lambda r: zc[r].send.deregister(comms[r]))
    for r in range(n):
        torch.cuda.set_device(dev_of[r])
        d = [a - b for a, b in zip(comms[r].reg_a2a_stats(), base[r])]
        if d != [2 * len(rounds), len(rounds), len(rounds)]:
            bad.append(("reg a2a stats", r, d))
    err = [c.async_error() for c in comms]
    for c in comms:
        c.destroy()
    return bad, any(err)


def main():
    rank, n = int(sys.argv[1]), int(sys.argv[2])
    case = sys.argv[4]
    if case == "single":
        bad, err = single_process(n)
    else:
        uid = nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3]))
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
