#!/usr/bin/env python3
"""One rank of the zero-copy direct tests (tests/test_gpu_direct_reg.py).

argv: rank nranks uid_hex case        (case "single": one process, ncclCommInitAll)
The parent sets the shared-GPU geometry of the all-to-all tests plus
VCCL_REG_THRESHOLD=32768 (or leaves it out, case "off").  A call is run twice:
on registered buffers (the zero-copy path) and on unregistered copies of the
same layout (the same kernel's fallback: the staged direct path); the two
outputs are compared bit for bit, guard bytes included, integer and
integer-valued results also with the exact value.  After registering, a case
runs one small warm-up collective and synchronises, so every peer's registry
write is ordered before every import and the expected path is deterministic.
Every case ends by comparing vcclCommRegStats with what it expects, on every
rank.  Exit 0 on success."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _mp  # noqa: E402
from vccl_amd import nccl  # noqa: E402

U8, I32, F32, BF16 = nccl.ncclUint8, nccl.ncclInt32, nccl.ncclFloat32, nccl.ncclBfloat16
SUM, PROD, MAX, AVG = nccl.ncclSum, nccl.ncclProd, nccl.ncclMax, nccl.ncclAvg
AR, RS, AG, BC = 0, 1, 2, 3
THRESH = 32768
SENTINEL, GUARD = 0xB7, 64


# ------------------------------------------------------------------- payloads
def bf16_bits(x):
    """Small integers / halves as bf16 bit patterns (exact: 8 significant bits)."""
    return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def make_input(dt, op, count, rank, tag):
    """Rank `rank`'s input of `count` elements as bytes: values whose sum /
    product / maximum over up to 8 ranks is exact in the type."""
    rng = np.random.default_rng((tag * 16 + rank) * 4 + 1)
    if dt == U8:
        return rng.integers(0, 256, count, dtype=np.uint8)
    if dt == I32:
        return rng.integers(-1 << 30, 1 << 30, count, dtype=np.int32).view(np.uint8)
    if op == PROD:
        v = rng.choice(np.array([1.0, 2.0, 0.5], np.float32), count)
    else:
        v = rng.integers(0, 12, count).astype(np.float32)
    return (v if dt == F32 else bf16_bits(v)).view(np.uint8)


def exact(dt, op, rows):
    """The exact reduction of the ranks' inputs (bytes), or None (bf16 avg:
    only the bitwise comparison with the staged path)."""
    if dt == U8:
        return np.sum(np.stack(rows), axis=0, dtype=np.uint8)
    if dt == I32:
        return np.max(np.stack([r.view(np.int32) for r in rows]), axis=0).view(np.uint8)
    if op == AVG:
        return None
    if dt == BF16:
        f = [(r.view(np.uint16).astype(np.uint32) << 16).view(np.float32) for r in rows]
    else:
        f = [r.view(np.float32) for r in rows]
    acc = f[0].copy()
    for x in f[1:]:
        acc = acc * x if op == PROD else acc + x
    return (acc if dt == F32 else bf16_bits(acc)).view(np.uint8)


class Buf:
    """[GUARD | off | nbytes | GUARD], sentinel-filled.  The registered range
    starts at the 16-byte-aligned `base`; the user pointer is `off` bytes past it."""

    def __init__(self, nbytes, off=0):
        self.n, self.off = nbytes, off
        self.t = torch.full((2 * GUARD + off + nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.base = self.t.data_ptr() + GUARD
        self.ptr = self.base + off
        self.handle = None

    def put(self, data, at=0):
        lo = GUARD + self.off + at
        self.t[lo:lo + data.size] = torch.from_numpy(np.ascontiguousarray(data)).cuda()

    def data(self):
        return self.t.cpu().numpy()[GUARD + self.off:GUARD + self.off + self.n]

    def guards_ok(self):
        b = self.t.cpu().numpy()
        return bool((b[:GUARD + self.off] == SENTINEL).all() and (b[GUARD + self.off + self.n:] == SENTINEL).all())

    def register(self, comm, short=0):
        self.handle = comm.register(self.base, self.off + self.n - short)

    def deregister(self, comm):
        if self.handle is not None:
            comm.deregister(self.handle)
        self.handle = None


class Call:
    """One collective on buffers of its own.  spec = (coll, dt, op, count,
    in_place, off): count as the API takes it (RS recvcount, AG sendcount)."""

    def __init__(self, rank, n, spec, tag):
        self.rank, self.n, self.spec = rank, n, spec
        coll, dt, op, count, inplace, off = spec
        esz = nccl.TYPE_SIZE[dt]
        rows = [make_input(dt, op, count * (n if coll == RS else 1), r, tag) for r in range(n)]
        mine = rows[rank]
        if coll == AR:
            self.recv = Buf(count * esz, off)
            self.send = self.recv if inplace else Buf(count * esz, off)
            self.send.put(mine)
            self.sptr, self.rptr = self.send.ptr, self.recv.ptr
            self.want, self.at = exact(dt, op, rows), 0
        elif coll == RS:
            blk = count * esz
            self.send = Buf(n * blk, off)
            self.send.put(mine)
            self.recv = self.send if inplace else Buf(blk, off)
            self.sptr = self.send.ptr
            self.rptr = self.send.ptr + rank * blk if inplace else self.recv.ptr
            w = exact(dt, op, rows)
            self.want, self.at = (None if w is None else w[rank * blk:(rank + 1) * blk]), (rank * blk if inplace else 0)
        else:
            blk = count * esz
            self.recv = Buf(n * blk, off)
            if inplace:
                self.send = self.recv
                self.recv.put(mine, rank * blk)
                self.sptr = self.recv.ptr + rank * blk
            else:
                self.send = Buf(blk, off)
                self.send.put(mine)
                self.sptr = self.send.ptr
            self.rptr = self.recv.ptr
            self.want, self.at = np.concatenate(rows), 0

    def bufs(self):
        return [self.send] if self.send is self.recv else [self.send, self.recv]

    def refill(self, tag):
        """Fresh input in the same buffers (graph replays)."""
        fresh = Call.__new__(Call)
        Call.__init__(fresh, self.rank, self.n, self.spec, tag)
        self.recv.t.copy_(fresh.recv.t)
        if self.send is not self.recv:
            self.send.t.copy_(fresh.send.t)
        self.want = fresh.want

    def issue(self, comm, sp):
        coll, dt, op, count, _, _ = self.spec
        if coll == AR:
            comm.all_reduce(self.sptr, self.rptr, count, dt, op, sp)
        elif coll == RS:
            comm.reduce_scatter(self.sptr, self.rptr, count, dt, op, sp)
        else:
            comm.all_gather(self.sptr, self.rptr, count, dt, sp)

    def eligible(self, thresh=THRESH):
        coll, dt, _, count, _, _ = self.spec
        return nccl.reg_eligible(coll, count, dt, self.n, thresh)

    def check(self, other=None):
        """Guards intact, the exact value where known, and bit-identical to
        `other` (the same call on the other path)."""
        out = []
        if not self.recv.guards_ok() or not self.send.guards_ok():
            out.append("guards")
        if self.want is not None and not np.array_equal(self.recv.data()[self.at:self.at + self.want.size], self.want):
            out.append("value")
        if other is not None and not torch.equal(self.recv.t, other.recv.t):
            out.append("differs from the staged path")
        return out


class Stats:
    def __init__(self, comm):
        self.comm = comm
        self.base = comm.reg_stats()
        self.want = [0, 0, 0]  # eligible launches, zero-copy, fallback

    def expect(self, call, zero_copy, times=1):
        if call.eligible():
            self.want[0] += times
            self.want[1 if zero_copy else 2] += times

    def bad(self, live=0):
        got = self.comm.reg_stats()
        d = [a - b for a, b in zip(got[:3], self.base[:3])]
        out = [] if d == self.want else [("reg stats", d, self.want)]
        return out + ([] if got[3] == live else [("live entries", got[3], live)])


def warmup(comm, sp):
    """A small collective (below the threshold) and a synchronise: every
    peer's registrations so far are ordered before my next enqueue."""
    x = torch.ones(64, device="cuda")
    comm.all_reduce(x.data_ptr(), x.data_ptr(), 64, F32, SUM, sp)
    torch.cuda.synchronize()


def run_batch(comm, rank, n, sp, specs, st, tag0):
    """Every spec on registered buffers and on unregistered copies; at most 32
    registrations at a time."""
    bad = []
    for lo in range(0, len(specs), 14):
        part = specs[lo:lo + 14]
        zc = [Call(rank, n, s, tag0 + lo + i) for i, s in enumerate(part)]
        fb = [Call(rank, n, s, tag0 + lo + i) for i, s in enumerate(part)]
        for c in zc:
            for b in c.bufs():
                b.register(comm)
        warmup(comm, sp)
        for a, b in zip(zc, fb):
            a.issue(comm, sp)
            b.issue(comm, sp)
            st.expect(a, True)
            st.expect(b, False)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(zc, fb)):
            for what in a.check(b) + ["staged: " + w for w in b.check()]:
                bad.append((part[i], what))
        for c in zc:
            for b in c.bufs():
                b.deregister(comm)
    return bad


# -------------------------------------------------------------------- cases
def case_allreduce(comm, rank, n, sp):
    st = Stats(comm)
    specs = []
    for dt, op, offs in ((F32, SUM, (0, 4)), (BF16, AVG, (0, 2)), (I32, MAX, (0, 4))):
        counts = (8191, 8192, 8193, 16391, 1_048_579)
        if dt == BF16:  # also at twice the count: the same bytes, so the same threshold edge as the 4-byte types
            counts += tuple(2 * c for c in counts)
        for count in counts:
            for inplace in (False, True):
                for off in offs:
                    specs.append((AR, dt, op, count, inplace, off))
    bad = run_batch(comm, rank, n, sp, specs, st, 100)
    # eligible: 4 counts x 4 layouts for f32, i32 and the doubled bf16 counts, 2 x 4 for the plain bf16 counts
    # (16391 and 1048579 elements); every other spec is below the threshold: no eligible launch
    if st.want != [112, 56, 56]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_reducescatter(comm, rank, n, sp):
    st = Stats(comm)
    specs = [(RS, dt, op, count, inplace, off)
             for dt, op, count in ((BF16, SUM, 8195), (F32, PROD, 4099), (U8, SUM, 65_537))
             for inplace in (False, True) for off in (0,)]
    bad = run_batch(comm, rank, n, sp, specs, st, 300)
    if st.want[1] != sum(1 for s in specs if nccl.reg_eligible(RS, s[3], s[1], n, THRESH)):
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_allgather(comm, rank, n, sp):
    st = Stats(comm)
    specs = [(AG, U8, SUM, count, inplace, 0) for count in ((1 << 20) + 1, 16_385) for inplace in (False, True)]
    bad = run_batch(comm, rank, n, sp, specs, st, 400)
    if st.want != [8, 4, 4]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_mixed(comm, rank, n, sp):
    """n = 4.  Rank 1 unregistered; only its recvbuff unregistered; its call 16
    bytes past the end of its registration: fallback on all four ranks, exact.
    Then rank 1 registers: zero-copy on all."""
    bad = []
    st = Stats(comm)
    spec = (AR, F32, SUM, 16_391, False, 0)
    for step, (reg_send, reg_recv, short) in enumerate(((False, False, 0), (True, False, 0), (True, True, 16),
                                                        (True, True, 0))):
        c = Call(rank, n, spec, 500 + step)
        mine = (reg_send, reg_recv, short) if rank == 1 else (True, True, 0)
        if mine[0]:
            c.send.register(comm, mine[2])
        if mine[1]:
            c.recv.register(comm, mine[2])
        warmup(comm, sp)
        c.issue(comm, sp)
        st.expect(c, step == 3)
        torch.cuda.synchronize()
        bad += [(step, w) for w in c.check()]
        for b in c.bufs():
            b.deregister(comm)
    if st.want != [4, 1, 3]:
        bad.append(("planned", st.want))
    return bad + st.bad()


def case_reregister(comm, rank, n, sp):
    """Deregister, register another allocation that lands in the same entries,
    call: zero-copy, exact.  Free the allocation after deregistering, call on a
    new one: exact."""
    bad = []
    st = Stats(comm)
    spec = (AR, I32, MAX, 20_000, False, 0)
    for step in range(3):
        c = Call(rank, n, spec, 600 + step)
        for b in c.bufs():
            b.register(comm)
        if comm.reg_stats()[3] != 2:
            bad.append(("live", step))
        warmup(comm, sp)
        c.issue(comm, sp)
        st.expect(c, True)
        torch.cuda.synchronize()
        bad += [(step, w) for w in c.check()]
        for b in c.bufs():
            b.deregister(comm)
        if step == 1:  # give the allocation back to the runtime before the next registration
            del c, b
            torch.cuda.empty_cache()
    rc = nccl.lib().ncclCommDeregister(comm.handle, 0x1234)
    if rc != nccl.ncclInvalidArgument:
        bad.append(("bad handle", rc))
    if st.want != [3, 3, 0]:
        bad.append(("planned", st.want))
    return bad + st.bad()


B2B = ("zc_ar", "zc_rs", "zc_ag", "fb_ar", "fb_rs", "fb_ag", "st_ar", "st_rs", "st_ag", "bc", "ll")


def case_b2b(comm, rank, n, sp):
    """48 calls with no host synchronisation, cycling the zero-copy AR / RS /
    AG, their fallbacks, the staged direct AR / RS / AG (below the threshold,
    path forced), a rooted direct broadcast and an LL all-reduce."""
    bad = []
    st = Stats(comm)
    plan = [(B2B[i % len(B2B)], 700 + i) for i in range(48)]
    calls = []
    for kind, tag in plan:
        coll = {"ar": AR, "rs": RS, "ag": AG}.get(kind[3:], None)
        if kind == "bc":
            root = tag % n
            src = make_input(U8, SUM, 5000, root, tag)
            b = Buf(5000)
            if rank == root:
                b.put(src)
            calls.append((b, src, root))
        elif kind == "ll":
            calls.append(Call(rank, n, (AR, F32, SUM, 256, False, 0), tag))
        elif kind.startswith("st"):
            calls.append(Call(rank, n, (coll, U8 if coll == AG else F32, SUM, 1500 // n, False, 0), tag))
        else:
            count = {AR: 12_001, RS: 4099, AG: 16_385}[coll]
            calls.append(Call(rank, n, (coll, U8 if coll == AG else F32, SUM, count, coll != AR, 0), tag))
        if kind.startswith("zc"):
            for b in calls[-1].bufs():
                b.register(comm)
    live = comm.reg_stats()[3]
    warmup(comm, sp)
    for (kind, tag), c in zip(plan, calls):
        if kind == "bc":
            comm.set_algo("direct")
            comm.broadcast(c[0].ptr, c[0].ptr, 5000, U8, c[2], sp)
            comm.set_algo(None)
            continue
        if kind.startswith("st"):
            comm.set_algo("direct")
            if c.eligible():
                bad.append(("the staged call is eligible", kind))
        c.issue(comm, sp)
        comm.set_algo(None)
        if kind[:2] in ("zc", "fb"):
            st.expect(c, kind.startswith("zc"))
    torch.cuda.synchronize()
    for i, ((kind, tag), c) in enumerate(zip(plan, calls)):
        if kind == "bc":
            if not np.array_equal(c[0].data(), c[1]) or not c[0].guards_ok():
                bad.append((i, kind))
        elif c.check():
            bad.append((i, kind, c.check()))
    if st.want[1] < 12 or st.want[2] < 12 or live < 20:
        bad.append(("planned", st.want, live))
    return bad + st.bad(live)


def case_capture(comm, rank, n, sp):
    """[AR, RS, AG] zero-copy captured, replayed three times with fresh inputs.
    Imports happen at eager enqueues only, so one eager eligible call precedes
    the capture."""
    bad = []
    st = Stats(comm)
    calls = [Call(rank, n, s, 800 + i) for i, s in enumerate(((AR, F32, SUM, 12_001, False, 4),
                                                             (RS, BF16, SUM, 8195, True, 0),
                                                             (AG, U8, SUM, 16_385, False, 0)))]
    for c in calls:
        for b in c.bufs():
            b.register(comm)
    warmup(comm, sp)
    calls[0].issue(comm, sp)
    st.expect(calls[0], True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        for c in calls:
            c.issue(comm, s.cuda_stream)
        g.capture_end()
    for it in range(3):
        for i, c in enumerate(calls):
            c.refill(810 + 3 * it + i)
            st.expect(c, True)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        bad += [(it, i, w) for i, c in enumerate(calls) for w in c.check()]
    if st.want != [10, 10, 0]:
        bad.append(("planned", st.want))
    return bad + st.bad(5)


def case_wrap(comm, rank, n, sp):
    """The direct epoch seeded at 0xfffffffd, then four zero-copy calls across the wrap."""
    bad = []
    st = Stats(comm)
    calls = [Call(rank, n, s, 900 + i) for i, s in enumerate(((AR, F32, SUM, 8193, True, 0), (RS, F32, SUM, 4099, False, 0),
                                                             (AG, U8, SUM, 16_385, True, 0),
                                                             (AR, I32, MAX, 16_391, False, 4)))]
    for c in calls:
        for b in c.bufs():
            b.register(comm)
    comm.set_algo("ring")  # the warm-up leaves no inbox flag behind
    warmup(comm, sp)
    comm.set_algo(None)
    comm.debug_set_epochs(0xFFFFFFFD, 0xFFFFFFFD)
    for i, c in enumerate(calls):
        c.issue(comm, sp)
        st.expect(c, True)
        torch.cuda.synchronize()
        if comm.async_error() or c.check():
            bad.append((i, c.check()))
    if st.want != [4, 4, 0]:
        bad.append(("planned", st.want))
    return bad + st.bad(6)


def case_fences(comm, rank, n, sp):
    st = Stats(comm)
    specs = [(AR, BF16, AVG, 16_386, False, 2), (RS, F32, PROD, 4099, True, 0), (AG, U8, SUM, 16_385, False, 0)]
    bad = run_batch(comm, rank, n, sp, specs, st, 1000)
    if os.environ.get("VCCL_FENCES") != "1" or st.want != [6, 3, 3]:
        bad.append(("setup", st.want))
    return bad + st.bad()


def case_off(comm, rank, n, sp):
    """The path is off (threshold unset, a net peer, or Direct excluded):
    *handle == buff, the stats stay zero, the call takes today's path, and
    vcclCommSetRegThreshold has no registry to switch on."""
    bad = []
    c = Call(rank, n, (AR, F32, SUM, 16_391, False, 0), 1100)
    algo = comm.coll_algo(AR, 16_391, F32)
    for b in c.bufs():
        b.register(comm)
        if b.handle != b.base:
            bad.append(("handle", b.handle, b.base))
    if comm.set_reg_threshold(THRESH) != 0:
        bad.append(("effective",))
    warmup(comm, sp)
    c.issue(comm, sp)
    torch.cuda.synchronize()
    bad += c.check()
    for b in c.bufs():
        b.deregister(comm)
    if comm.reg_stats() != (0, 0, 0, 0, 0) or comm.coll_algo(AR, 16_391, F32) != algo:
        bad.append(("stats", comm.reg_stats()))
    return bad


CASES = {"allreduce": case_allreduce, "reducescatter": case_reducescatter, "allgather": case_allgather,
         "mixed": case_mixed, "reregister": case_reregister, "b2b": case_b2b, "capture": case_capture,
         "wrap": case_wrap, "fences": case_fences, "off": case_off}


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

    base = [c.reg_stats() for c in comms]
    want = 0
    for i, spec in enumerate(((AR, F32, SUM, 16_391, False, 4), (RS, BF16, SUM, 8195, True, 0),
                              (AG, U8, SUM, 16_385, False, 0), (AR, I32, MAX, 8193, True, 0))):
        zc = each(lambda r: Call(r, n, spec, 1200 + i))
        fb = each(lambda r: Call(r, n, spec, 1200 + i))
        each(lambda r: [b.register(comms[r]) for b in zc[r].bufs()])
        grouped(each(lambda r: Call(r, n, (AR, F32, SUM, 64, True, 0), 0)))  # the warm-up
        grouped(zc)
        grouped(fb)
        want += 1
        for r in range(n):
            torch.cuda.set_device(dev_of[r])
            bad += [(i, r, w) for w in zc[r].check(fb[r])]
        each(lambda r: [b.deregister(comms[r]) for b in zc[r].bufs()])
    for r in range(n):
        torch.cuda.set_device(dev_of[r])
        d = [a - b for a, b in zip(comms[r].reg_stats()[:3], base[r][:3])]
        if d != [2 * want, want, want]:
            bad.append(("reg stats", r, d))
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
