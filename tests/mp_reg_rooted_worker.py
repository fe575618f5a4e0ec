#!/usr/bin/env python3
"""One rank of the zero-copy broadcast / reduce tests (tests/test_gpu_reg_rooted.py).

argv: rank nranks uid_hex case outdir     (case "single": one process, ncclCommInitAll)
The parent sets the shared-GPU geometry plus VCCL_REG_ROOTED_THRESHOLD=32768 (or
leaves it out, case "off").  A call runs on registered buffers (the zero-copy
path) and, where the case says so, on unregistered copies of the same layout
(the same kernel's fallback: the staged direct rooted part).  After registering,
a case runs one small warm-up collective and synchronises, so every peer's
registry write is ordered before every import and the expected path is
deterministic.  Reduce outputs go to outdir/rank<r>.npz for the parent's oracle
check.  Every case ends by comparing vcclCommRegRootedStats with what it
expects and by checking that vcclCommRegStats did not move, on every rank.
Exit 0 on success."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _mp  # noqa: E402
from tests import ring_cases as RC  # noqa: E402
from tests.mp_direct_reg_worker import AR, SENTINEL, Buf, warmup  # noqa: E402
from tests.mp_direct_reg_worker import Call as RegCall  # noqa: E402
from tests.mp_direct_rooted_worker import region_bytes  # noqa: E402
from tests.mp_ll_rooted_worker import ints_f32, ints_sum, payload  # noqa: E402
from vccl_amd import nccl  # noqa: E402

U8, F32 = nccl.ncclUint8, nccl.ncclFloat32
SUM = nccl.ncclSum
BC, RED = 3, 4
THRESH = 32768
OFFS = (0, 4, 3)  # user pointers past the registered base


def bcast_sizes(n):
    return [32767, 32768, 32769, 32768 + 16 * (n - 1) - 1, 32768 + 16 * (n - 1) + 1, 65541, (1 << 20) + 3]


def roots_of(n, reduce=False):
    return list(range(n)) if n <= 4 else ([0, n - 1] if reduce else [0, 3, 7])


class Stats:
    """The rooted counters' expected movement; vcclCommRegStats must stand still
    (but for `ar`: the zero-copy all-reduces of the back-to-back case)."""

    def __init__(self, comm):
        self.comm = comm
        self.base = comm.reg_rooted_stats()
        self.reg = comm.reg_stats()[:3]
        self.want = [0, 0, 0]
        self.ar = 0

    def expect(self, nbytes, zero_copy, times=1):
        if nbytes >= THRESH:
            self.want[0] += times
            self.want[1 if zero_copy else 2] += times

    def bad(self):
        d = [a - b for a, b in zip(self.comm.reg_rooted_stats(), self.base)]
        out = [] if d == self.want else [("rooted stats", d, self.want)]
        r = [a - b for a, b in zip(self.comm.reg_stats()[:3], self.reg)]
        return out + ([] if r == [self.ar, self.ar, 0] else [("reg stats moved", r)])


class Bcast:
    """One broadcast: ncclBroadcast out of place (a non-root's sendbuff NULL) or
    ncclBcast in place.  Offsets differ between the root and the non-roots."""

    def __init__(self, rank, n, root, nbytes, inplace, tag, i=0):
        self.rank, self.root, self.nbytes, self.inplace = rank, root, nbytes, inplace
        self.want = payload(nbytes, tag)
        self.recv = Buf(nbytes, OFFS[(i + (rank - root) % n) % 3])
        self.send = None
        if rank == root:
            self.send = self.recv if inplace else Buf(nbytes, OFFS[(i + 1) % 3])
            self.send.put(self.want)

    def bufs(self):
        """What a peer reads: the root's sendbuff, a non-root's recvbuff."""
        return [self.send if self.rank == self.root else self.recv]

    def issue(self, comm, sp):
        if self.inplace:
            nccl.check(nccl.lib().ncclBcast(ctypes.c_void_p(self.recv.ptr), ctypes.c_size_t(self.nbytes), U8, self.root,
                                            comm.handle, ctypes.c_void_p(sp)), "ncclBcast")
        else:
            comm.broadcast(self.send.ptr if self.send else 0, self.recv.ptr, self.nbytes, U8, self.root, sp)

    def check(self):
        out = []
        if not np.array_equal(self.recv.data(), self.want):
            out.append("value")
        if not self.recv.guards_ok() or (self.send is not None and not self.send.guards_ok()):
            out.append("guards")
        if self.send is not None and not np.array_equal(self.send.data(), self.want):
            out.append("root input written")
        return out


class Reduce:
    """One reduce of `x` (numpy, this rank's input).  A non-root's recvbuff is
    NULL or a sentinel buffer that must stay untouched; only sendbuff is ever
    registered."""

    def __init__(self, rank, n, root, x, dt, op, inplace, off=0):
        self.rank, self.root, self.dt, self.op, self.inplace = rank, root, dt, op, inplace
        self.x = np.ascontiguousarray(x).view(np.uint8)
        self.count = self.x.size // nccl.TYPE_SIZE[dt]
        self.send = Buf(self.x.size, off)
        self.send.put(self.x)
        self.null = not inplace and rank != root and (rank + root) % 2 == 1
        self.recv = self.send if inplace else None if self.null else Buf(self.x.size, off)

    def bufs(self):
        return [self.send]

    def refill(self, x):
        self.x = np.ascontiguousarray(x).view(np.uint8)
        self.send.t.fill_(SENTINEL)
        self.send.put(self.x)
        if self.recv is not None and self.recv is not self.send:
            self.recv.t.fill_(SENTINEL)

    def issue(self, comm, sp):
        comm.reduce(self.send.ptr, self.recv.ptr if self.recv is not None else 0, self.count, self.dt, self.op,
                    self.root, sp)

    def out(self):
        return self.recv.data().copy()

    def check(self, want=None):
        out = []
        if not self.send.guards_ok() or (self.recv is not None and not self.recv.guards_ok()):
            out.append("guards")
        if not (self.inplace and self.rank == self.root) and not np.array_equal(self.send.data(), self.x):
            out.append("input written")
        if self.rank != self.root and self.recv is not None and not self.inplace and \
                not bool((self.recv.t == SENTINEL).all()):
            out.append("non-root output written")
        if want is not None and self.rank == self.root and not np.array_equal(self.out(), want.view(np.uint8)):
            out.append("value")
        return out


def reg_all(comm, calls):
    for c in calls:
        for b in c.bufs():
            b.register(comm)


def dereg_all(comm, calls):
    for c in calls:
        for b in c.bufs():
            b.deregister(comm)


# -------------------------------------------------------------------- cases
def case_bcast(comm, rank, n, sp, res):
    bad = []
    st = Stats(comm)
    specs = [(nb, root, inplace) for nb in bcast_sizes(n) for root in roots_of(n) for inplace in (False, True)]
    for lo in range(0, len(specs), 24):
        part = specs[lo:lo + 24]
        calls = [Bcast(rank, n, root, nb, inplace, 100 + lo + i, lo + i) for i, (nb, root, inplace) in enumerate(part)]
        reg_all(comm, calls)
        warmup(comm, sp)
        for c in calls:
            c.issue(comm, sp)
            st.expect(c.nbytes, True)
        torch.cuda.synchronize()
        bad += [(part[i], w) for i, c in enumerate(calls) for w in c.check()]
        dereg_all(comm, calls)
    if st.want[2] != 0 or st.want[0] != 6 * len(roots_of(n)) * 2:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_reduce(comm, rank, n, sp, res):
    bad = []
    st = Stats(comm)
    for root in roots_of(n, True):
        zc, fb = [], []
        for ri, (name, op, dt, count, inplace) in enumerate(RC.REDUCE_CASES):
            x = RC.gen_reduce_input(ri, rank)
            zc.append(Reduce(rank, n, root, x, dt, op, inplace))
            fb.append(Reduce(rank, n, root, x, dt, op, inplace))
        reg_all(comm, zc)
        warmup(comm, sp)
        for a, b in zip(zc, fb):
            a.issue(comm, sp)
            b.issue(comm, sp)
            st.expect(a.x.size, True)
            st.expect(b.x.size, False)
        torch.cuda.synchronize()
        for (name, *_), a, b in zip(RC.REDUCE_CASES, zc, fb):
            bad += [(name, root, w) for w in a.check() + ["staged: " + w for w in b.check()]]
            if rank == root:
                if not np.array_equal(a.out(), b.out()):
                    bad.append((name, root, "differs from the staged path"))
                res[f"{name}_r{root}"] = a.out()  # bytes: the parent views them in the row's type
        dereg_all(comm, zc)
    big = sum(1 for ri in range(len(RC.REDUCE_CASES)) if RC.gen_reduce_input(ri, 0).nbytes >= THRESH)
    if st.want != [2 * big * len(roots_of(n, True)), big * len(roots_of(n, True)), big * len(roots_of(n, True))]:
        bad.append(("planned", st.want))
    nch = nccl.reg_rooted_plan(RED, 1 << 21, nccl.ncclInt64, n, rank, 0, region_bytes(n), 16)["n_chunks"]
    if nch < 16:
        bad.append(("chunks of the 16 MiB row", nch))
    return bad + st.bad()


def case_mixed(comm, rank, n, sp, res):
    """n = 4.  The root's sendbuff unregistered; non-root 1's recvbuff
    unregistered; rank 1's reduce input 16 bytes past the end of its
    registration: fallback on all four ranks, exact.  After rank 1 registers and
    one warm-up call: zero-copy on all."""
    bad = []
    st = Stats(comm)
    nb, cnt = 65_541, 16_391
    for step in range(5):
        if step < 2 or step == 4:
            root = 0 if step != 1 else 2
            c = Bcast(rank, n, root, nb, False, 500 + step, step)
            skip = (step == 0 and rank == root) or (step == 1 and rank == 1)
            short, size, want = 0, nb, None
        else:
            c = Reduce(rank, n, 3, ints_f32(cnt, rank, 500 + step), F32, SUM, False, 4)
            skip, short, size = False, (16 if step == 2 and rank == 1 else 0), 4 * cnt
            want = ints_sum(cnt, n, 500 + step)
        if not skip:
            for b in c.bufs():
                b.register(comm, short)
        warmup(comm, sp)
        c.issue(comm, sp)
        st.expect(size, step >= 3)
        torch.cuda.synchronize()
        bad += [(step, w) for w in (c.check(want) if want is not None else c.check())]
        dereg_all(comm, [c])
    if st.want != [5, 2, 3]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_mixed2(comm, rank, n, sp, res):
    """n = 2: nobody reads the non-root's recvbuff, so the root's registration alone is zero-copy."""
    st = Stats(comm)
    c = Bcast(rank, n, 1, 65_541, False, 520)
    if rank == 1:
        reg_all(comm, [c])
    warmup(comm, sp)
    c.issue(comm, sp)
    st.expect(c.nbytes, True)
    torch.cuda.synchronize()
    bad = c.check()
    dereg_all(comm, [c])
    return bad + st.bad()


B2B = ("zc_bc", "zc_red1", "zc_red3", "fb_bc", "fb_red1", "fb_red3", "zc_ar", "st_bc", "st_red", "ll")
RED1, RED3 = 12_001, 75_000


def case_b2b(comm, rank, n, sp, res):
    """48 calls with no host synchronisation on a 128 KiB inbox, roots rotating."""
    bad = []
    st = Stats(comm)
    chunks = [nccl.reg_rooted_plan(RED, c, F32, n, rank, 0, region_bytes(n), 4)["n_chunks"] for c in (RED1, RED3)]
    if chunks != [1, 3]:
        bad.append(("chunks", chunks))
    plan = [(B2B[i % len(B2B)], 700 + i, i % n) for i in range(48)]
    calls = []
    for kind, tag, root in plan:
        if kind.endswith("bc"):
            calls.append(Bcast(rank, n, root, 5000 if kind == "st_bc" else 100_003, tag % 2 == 1, tag, tag))
        elif kind == "zc_ar":
            calls.append(RegCall(rank, n, (AR, F32, SUM, RED1, False, 0), tag))
        elif kind == "ll":
            calls.append(RegCall(rank, n, (AR, F32, SUM, 256, False, 0), tag))
        else:
            cnt = RED3 if kind.endswith("3") else 1500 if kind == "st_red" else RED1
            calls.append(Reduce(rank, n, root, ints_f32(cnt, rank, tag), F32, SUM, tag % 3 == 0))
        if kind.startswith("zc"):
            reg_all(comm, [calls[-1]])
    warmup(comm, sp)
    for (kind, tag, root), c in zip(plan, calls):
        if kind.startswith("st"):
            comm.set_algo("direct")
        c.issue(comm, sp)
        comm.set_algo(None)
        if kind == "zc_ar":
            st.ar += 1
        elif kind[:2] in ("zc", "fb"):
            st.expect(THRESH, kind.startswith("zc"))
    torch.cuda.synchronize()
    for i, ((kind, tag, root), c) in enumerate(zip(plan, calls)):
        if isinstance(c, Reduce):
            w = c.check(ints_sum(c.count, n, tag))
        else:
            w = c.check()
        if w:
            bad.append((i, kind, root, w))
    if st.want[1] < 12 or st.want[2] < 12:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_capture(comm, rank, n, sp, res):
    """[broadcast root 0, reduce root 1, broadcast root 1] captured after an eager
    warm-up that imported the buffers, replayed three times with fresh inputs."""
    bad = []
    st = Stats(comm)
    nb, cnt = 65_541, 16_391
    calls = [Bcast(rank, n, 0, nb, False, 800, 0), Reduce(rank, n, 1, ints_f32(cnt, rank, 801), F32, SUM, False),
             Bcast(rank, n, 1, nb, True, 802, 1)]
    reg_all(comm, calls)
    warmup(comm, sp)
    for c in calls:  # the eager calls import the peers' ranges
        c.issue(comm, sp)
        st.expect(nb, True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        for c in calls:
            c.issue(comm, s.cuda_stream)
        g.capture_end()
    for it in range(3):
        before = comm.reg_rooted_stats()
        for i in (0, 2):
            c = calls[i]
            c.want = payload(nb, 810 + 3 * it + i)
            c.recv.t.fill_(SENTINEL)
            if c.send is not None:
                c.send.t.fill_(SENTINEL)
                c.send.put(c.want)
        calls[1].refill(ints_f32(cnt, rank, 811 + 3 * it))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        st.expect(nb, True, 3)
        after = comm.reg_rooted_stats()
        if [a - b for a, b in zip(after, before)] != [3, 3, 0]:
            bad.append(("replay counters", it, after, before))
        bad += [(it, 0, w) for w in calls[0].check()] + [(it, 2, w) for w in calls[2].check()]
        bad += [(it, 1, w) for w in calls[1].check(ints_sum(cnt, n, 811 + 3 * it))]
    return bad + st.bad()


def case_wrap(comm, rank, n, sp, res):
    """The direct epoch seeded at 0xfffffffd, then two broadcasts and two reduces across the wrap."""
    bad = []
    st = Stats(comm)
    nb, cnt = 65_541, 16_391
    calls = [Bcast(rank, n, 0, nb, False, 900, 0), Reduce(rank, n, 1, ints_f32(cnt, rank, 901), F32, SUM, False),
             Bcast(rank, n, 1, nb, True, 902, 2), Reduce(rank, n, 0, ints_f32(cnt, rank, 903), F32, SUM, True, 4)]
    reg_all(comm, calls)
    comm.set_algo("ring")  # the warm-up leaves no inbox flag behind
    warmup(comm, sp)
    comm.set_algo(None)
    comm.debug_set_epochs(0xFFFFFFFD, 0xFFFFFFFD)
    for i, c in enumerate(calls):
        c.issue(comm, sp)
        st.expect(nb, True)
        torch.cuda.synchronize()
        w = c.check(ints_sum(cnt, n, 900 + i)) if isinstance(c, Reduce) else c.check()
        if comm.async_error() or w:
            bad.append((i, w))
    return bad + st.bad()


def case_fences(comm, rank, n, sp, res):
    bad = []
    st = Stats(comm)
    nb, cnt = 65_541, 70_001
    zc = [Bcast(rank, n, 1, nb, False, 1000, 1), Reduce(rank, n, 2, ints_f32(cnt, rank, 1001), F32, SUM, False, 4)]
    fb = [Bcast(rank, n, 1, nb, False, 1000, 1), Reduce(rank, n, 2, ints_f32(cnt, rank, 1001), F32, SUM, False, 4)]
    reg_all(comm, zc)
    warmup(comm, sp)
    for a, b in zip(zc, fb):
        a.issue(comm, sp)
        b.issue(comm, sp)
        st.expect(nb, True)
        st.expect(nb, False)
    torch.cuda.synchronize()
    for c in zc + fb:
        bad += c.check(ints_sum(cnt, n, 1001)) if isinstance(c, Reduce) else c.check()
    if os.environ.get("VCCL_FENCES") != "1" or st.want != [4, 2, 2]:
        bad.append(("setup", st.want))
    return bad + st.bad()


def case_off(comm, rank, n, sp, res):
    """The path is off (threshold unset, a net peer, or Direct excluded): the new
    stats stay zero, vcclCommSetRegRootedThreshold has nothing to switch on
    (without a registry) and the calls take today's path.  Without any registry
    *handle == buff still holds."""
    bad = []
    nb, cnt = 65_541, 16_391
    algos = (comm.coll_algo(BC, nb, U8), comm.coll_algo(RED, cnt, F32))
    has_registry = os.environ.get("VCCL_REG_THRESHOLD") is not None and comm.set_reg_threshold(THRESH) > 0
    calls = [Bcast(rank, n, 0, nb, False, 1100), Reduce(rank, n, 1, ints_f32(cnt, rank, 1101), F32, SUM, False)]
    reg_all(comm, calls)
    if not has_registry:
        for c in calls:
            for b in c.bufs():
                if b.handle != b.base:
                    bad.append(("handle", b.handle, b.base))
        if comm.set_reg_rooted_threshold(THRESH) != 0:
            bad.append(("effective",))
    reg0 = comm.reg_stats()[:3]
    warmup(comm, sp)
    for c in calls:
        c.issue(comm, sp)
    torch.cuda.synchronize()
    bad += calls[0].check() + calls[1].check(ints_sum(cnt, n, 1101))
    dereg_all(comm, calls)
    if comm.reg_rooted_stats() != (0, 0, 0) or comm.reg_stats()[:3] != reg0:
        bad.append(("stats", comm.reg_rooted_stats(), comm.reg_stats()))
    if (comm.coll_algo(BC, nb, U8), comm.coll_algo(RED, cnt, F32)) != algos:
        bad.append(("algo",))
    return bad


CASES = {"bcast": case_bcast, "reduce": case_reduce, "mixed": case_mixed, "mixed2": case_mixed2, "b2b": case_b2b,
         "capture": case_capture, "wrap": case_wrap, "fences": case_fences, "off": case_off}


def single_process(n):
    """ncclCommInitAll ranks in one process (peers by raw pointer): each call
    inside ncclGroupStart / End, one collective per comm."""
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

    base = [c.reg_rooted_stats() for c in comms]
    reg0 = [c.reg_stats()[:3] for c in comms]
    nb, cnt, want = 65_541, 16_391, 0
    for i in range(4):
        def make(r):
            if i % 2 == 0:
                return Bcast(r, n, i // 2, nb, i == 2, 1200 + i, i)
            return Reduce(r, n, i // 2, ints_f32(cnt, r, 1200 + i), F32, SUM, i == 3)
        zc, fb = each(make), each(make)
        each(lambda r: reg_all(comms[r], [zc[r]]))
        grouped(each(lambda r: RegCall(r, n, (AR, F32, SUM, 64, True, 0), 0)))  # the warm-up
        grouped(zc)
        grouped(fb)
        want += 1
        for r in range(n):
            torch.cuda.set_device(dev_of[r])
            for c in (zc[r], fb[r]):
                bad += [(i, r, w) for w in (c.check(ints_sum(cnt, n, 1200 + i)) if i % 2 else c.check())]
        each(lambda r: dereg_all(comms[r], [zc[r]]))
    for r in range(n):
        torch.cuda.set_device(dev_of[r])
        d = [a - b for a, b in zip(comms[r].reg_rooted_stats(), base[r])]
        if d != [2 * want, want, want] or comms[r].reg_stats()[:3] != reg0[r]:
            bad.append(("stats", r, d))
    err = [c.async_error() for c in comms]
    for c in comms:
        c.destroy()
    return bad, any(err)


def main():
    rank, n = int(sys.argv[1]), int(sys.argv[2])
    case, outdir = sys.argv[4], sys.argv[5]
    if case == "single":
        bad, err = single_process(n)
    else:
        uid = nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3]))
        _mp.bind(rank, n)
        comm = nccl.Comm.init_rank(n, uid, rank)
        sp = torch.cuda.current_stream().cuda_stream
        res = {}
        bad = CASES[case](comm, rank, n, sp, res)
        torch.cuda.synchronize()
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **res)
        err = comm.async_error()
        comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
