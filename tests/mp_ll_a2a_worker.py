#!/usr/bin/env python3
"""One rank of the one-hop LL all-to-all tests (tests/test_gpu_ll_a2a.py).

argv: rank nranks uid_hex case
The parent sets the shared-GPU geometry of the LL and p2p tests and
VCCL_LL_A2A_THRESHOLD (or leaves it out, case "off").  Every received byte is
compared with a seeded payload both ends can compute; destinations are
sentinel-filled with 64 guard bytes on each side; every case ends by comparing
vcclCommA2aStats with what vcclLLA2aPlan predicts.  Exit 0 on success."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tests import _mp  # noqa: E402
from vccl_amd import nccl  # noqa: E402

U8, F32, BF16 = nccl.ncclUint8, nccl.ncclFloat32, nccl.ncclBfloat16
SENTINEL = 0xB7
GUARD = 64
LIMIT = 65536                 # VCCL_LL_A2A_THRESHOLD of the tests, bytes per pair
SLOT_LINES = (1 << 20) // 8   # VCCL_LL_THRESHOLD of the test geometry: one slot
FIFO_BYTES = 70_000           # a uniform row above the limit


def payload(nbytes, src, dst, tag):
    return np.random.default_rng((tag * 64 + src) * 64 + dst + 1).integers(0, 256, nbytes, dtype=np.uint8)


class Dest:
    """nbytes of output `off` bytes past a 16-byte boundary, GUARD sentinel bytes on each side."""

    def __init__(self, nbytes, off=0):
        self.n, self.lo = nbytes, GUARD + off
        self.buf = torch.full((nbytes + off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def ok(self, want):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == SENTINEL).all() and np.array_equal(b[self.lo:self.lo + self.n], want)
                    and (b[self.lo + self.n:] == SENTINEL).all())


class Src:
    def __init__(self, data, off=0):
        self.buf = torch.zeros(data.size + off + 16, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[off:off + data.size] = torch.from_numpy(data).cuda()
        self.ptr = self.buf.data_ptr() + off


class Stats:
    """What vcclCommA2aStats must have grown by, from the pure plan."""

    def __init__(self, comm, rank, n):
        self.comm, self.rank, self.n = comm, rank, n
        self.base = comm.a2a_stats()
        self.want = [0, 0, 0]

    def expect(self, send_bytes, recv_bytes, uniform, limit=LIMIT):
        pl = nccl.ll_a2a_plan(self.n, self.rank, send_bytes, recv_bytes, uniform, limit, SLOT_LINES)
        fifo = len(pl["res_sends"]) + len(pl["res_recvs"])
        self.want[0] += int(pl["launch"])
        self.want[1] += 2 * self.n - fifo
        self.want[2] += fifo
        return pl

    def bad(self):
        got = [a - b for a, b in zip(self.comm.a2a_stats(), self.base)]
        return [] if got == self.want else [("a2a stats", got, self.want)]


def uniform_call(rank, n, nbytes, tag, soff=0, doff=0):
    send = np.concatenate([payload(nbytes, rank, p, tag) for p in range(n)])
    want = np.concatenate([payload(nbytes, p, rank, tag) for p in range(n)])
    return Src(send, soff), Dest(nbytes * n, doff), want


def run_uniform(comm, st, rank, n, sp, nbytes, tag, soff=0, doff=0, dt=U8):
    src, dst, want = uniform_call(rank, n, nbytes, tag, soff, doff)
    st.expect([nbytes] * n, [nbytes] * n, True)
    comm.all_to_all(src.ptr, dst.ptr, nbytes // nccl.TYPE_SIZE[dt], dt, sp)
    return src, dst, want


def v_call(rank, n, cnt, esz, tag):
    """cnt[a][b] elements of esz bytes from a to b; gaps between the blocks on both sides."""
    sc = [int(cnt[rank][p]) for p in range(n)]
    rc = [int(cnt[p][rank]) for p in range(n)]
    sd, rd, so, ro = [], [], 3, 5
    for p in range(n):
        sd.append(so)
        rd.append(ro)
        so += sc[p] + 7 * (p + 1)
        ro += rc[p] + 3 * (p + 2)
    send = np.zeros(so * esz, np.uint8)
    want = np.full(ro * esz, SENTINEL, np.uint8)
    for p in range(n):
        send[sd[p] * esz:(sd[p] + sc[p]) * esz] = payload(sc[p] * esz, rank, p, tag)
        want[rd[p] * esz:(rd[p] + rc[p]) * esz] = payload(rc[p] * esz, p, rank, tag)
    return Src(send), Dest(ro * esz), want, (sc, sd, rc, rd)


def run_v(comm, st, rank, n, sp, cnt, dt, tag):
    esz = nccl.TYPE_SIZE[dt]
    src, dst, want, (sc, sd, rc, rd) = v_call(rank, n, cnt, esz, tag)
    pl = st.expect([c * esz for c in sc], [c * esz for c in rc], False)
    comm.all_to_allv(src.ptr, sc, sd, dst.ptr, rc, rd, dt, sp)
    return src, dst, want, pl


def mixed_matrix(n, seed=77):
    """bf16 element counts: zero counts, rank 1's row empty, pairs at the limit
    and 2 bytes above it, one 300 KB pair (two wraps of a p2p part's FIFO in
    the test geometry), a self block above the limit."""
    m = np.random.default_rng(seed + n).choice([0, 1, 5, 37, 1000, 20_000], size=(n, n))
    m[1, :] = 0
    m[0, 1] = LIMIT // 2
    m[2, 0] = LIMIT // 2 + 1
    m[0, 2] = 150_000
    m[0, 0] = 40_000
    m[2, 2] = 9
    return m


# -------------------------------------------------------------------- cases
def case_uniform(comm, rank, n, sp):
    bad, tag = [], 0
    st = Stats(comm, rank, n)
    for nbytes, dt in ((1, U8), (7, U8), (8, U8), (9, U8), (4099, U8), (LIMIT, U8), (4000, F32)):
        for soff, doff in ((0, 0), (1, 3), (3, 1)):
            tag += 1
            src, dst, want = run_uniform(comm, st, rank, n, sp, nbytes, tag, soff, doff, dt)
            torch.cuda.synchronize()
            if not dst.ok(want):
                bad.append((nbytes, soff, doff))
    if st.want != [21, 42 * n, 0]:
        bad.append(("planned", st.want))
    # one byte over the limit: today's path, no LL launch
    src, dst, want = run_uniform(comm, st, rank, n, sp, LIMIT + 1, 99)
    torch.cuda.synchronize()
    if not dst.ok(want) or st.want != [21, 42 * n, 2 * n]:
        bad.append(("over the limit", st.want))
    return bad + st.bad()


def case_v_mixed(comm, rank, n, sp):
    bad = []
    st = Stats(comm, rank, n)
    m = mixed_matrix(n)
    for it in range(2):
        src, dst, want, pl = run_v(comm, st, rank, n, sp, m, BF16, 200 + it)
        torch.cuda.synchronize()
        if not dst.ok(want):
            bad.append(("alltoallv", it))
        if not pl["launch"] or (rank == 0 and sorted(pl["res_sends"]) != [0, 2]) or \
                (rank == 1 and (pl["res_sends"] or not all(pl["send_ll"]))):
            bad.append(("plan", pl["res_sends"]))
    return bad + st.bad()


def case_group_mixed(comm, rank, n, sp):
    """One group: a plain send to r+1, an all-to-allv, a plain recv from r-1, a
    4 MiB all-reduce.  The all-to-allv's pairs above the limit sit on r -> r+2,
    so the plain pair is the only FIFO message between r and r+1 and matching by
    call order per peer is the same with the path on or off."""
    bad = []
    st = Stats(comm, rank, n)
    nxt, prv = (rank + 1) % n, (rank - 1) % n
    m = np.random.default_rng(5).choice([0, 3, 900, 30_000], size=(n, n))
    for r in range(n):
        m[r, (r + 2) % n] = 100_000 + r
    src, dst, want, (sc, sd, rc, rd) = v_call(rank, n, m, 2, 300)
    pl = st.expect([c * 2 for c in sc], [c * 2 for c in rc], False)
    if pl["res_sends"] != [(rank + 2) % n] or pl["res_recvs"] != [(rank - 2) % n]:
        bad.append(("plan", pl["res_sends"], pl["res_recvs"]))
    ps, pd = Src(payload(5001, rank, nxt, 301)), Dest(5001, 1)
    cnt = 1 << 20
    x = torch.empty(cnt, device="cuda")
    bench.pattern_fill(x, rank, n, base=3 << 20)
    y = torch.full_like(x, float("nan"))
    torch.cuda.synchronize()
    nccl.group_start()
    comm.send(ps.ptr, 5001, U8, nxt, sp)
    comm.all_to_allv(src.ptr, sc, sd, dst.ptr, rc, rd, BF16, sp)
    comm.recv(pd.ptr, 5001, U8, prv, sp)
    comm.all_reduce(x.data_ptr(), y.data_ptr(), cnt, F32, nccl.ncclSum, sp)
    nccl.group_end()
    torch.cuda.synchronize()
    if not dst.ok(want):
        bad.append(("alltoallv",))
    if not pd.ok(payload(5001, prv, rank, 301)):
        bad.append(("plain recv",))
    if not bench.pattern_ok(y, n, base=3 << 20):
        bad.append(("all-reduce",))
    return bad + st.bad()


def ints_f32(count, rank, tag):
    return ((np.arange(count) * 7 + 13 * rank + tag) % 11 + rank).astype(np.float32)


def case_b2b(comm, rank, n, sp):
    """No host synchronisation between calls: 64 LL all-to-alls into 64
    outputs, then 48 calls cycling LL all-to-all, LL all-reduce, rooted LL
    broadcast, FIFO all-to-all and mixed all-to-allv."""
    bad = []
    st = Stats(comm, rank, n)
    if comm.coll_algo(0, 1024, F32) != "ll" or comm.coll_algo(3, 4096, U8) != "ll":
        bad.append(("paths", comm.coll_algo(0, 1024, F32), comm.coll_algo(3, 4096, U8)))
    small = np.array([[0 if (a + b) % 3 == 0 else 100 + 40 * a + b for b in range(n)] for a in range(n)])
    small[0, n - 1] = 40_000  # one pair above the limit (bf16 elements)
    plan = [("a2a", i) for i in range(64)] + [(("a2a", "ar", "bc", "fifo", "v")[i % 5], 64 + i) for i in range(48)]
    prep = []
    for kind, tag in plan:
        if kind in ("a2a", "fifo"):
            nb = 4096 if kind == "a2a" else FIFO_BYTES
            src, dst, want = uniform_call(rank, n, nb, tag)
            st.expect([nb] * n, [nb] * n, True)
            prep.append((src, dst, want, nb))
        elif kind == "v":
            src, dst, want, arg = v_call(rank, n, small, 2, tag)
            st.expect([c * 2 for c in arg[0]], [c * 2 for c in arg[2]], False)
            prep.append((src, dst, want, arg))
        elif kind == "ar":
            prep.append((Src(ints_f32(1024, rank, tag).view(np.uint8)), Dest(4096),
                         sum(ints_f32(1024, r, tag) for r in range(n)).view(np.uint8), None))
        else:
            root = tag % n
            want = payload(4096, root, root, tag)
            prep.append((Src(want) if rank == root else None, Dest(4096), want, root))
    torch.cuda.synchronize()
    for (kind, tag), (src, dst, want, arg) in zip(plan, prep):
        if kind in ("a2a", "fifo"):
            comm.all_to_all(src.ptr, dst.ptr, arg, U8, sp)
        elif kind == "v":
            comm.all_to_allv(src.ptr, arg[0], arg[1], dst.ptr, arg[2], arg[3], BF16, sp)
        elif kind == "ar":
            comm.all_reduce(src.ptr, dst.ptr, 1024, F32, nccl.ncclSum, sp)
        else:
            comm.broadcast(src.ptr if src else 0, dst.ptr, 4096, U8, arg, sp)
    torch.cuda.synchronize()
    for i, ((kind, tag), (src, dst, want, arg)) in enumerate(zip(plan, prep)):
        if not dst.ok(want):
            bad.append((i, kind))
    return bad + st.bad()


def case_capture(comm, rank, n, sp):
    """[all-to-all, mixed all-to-allv, all-to-all] captured on one stream,
    replayed three times with fresh inputs."""
    bad = []
    st = Stats(comm, rank, n)
    m = np.array([[0, 35_000], [50, 9]])  # bf16 elements: 0 -> 1 above the limit
    a_src, a_dst, _ = uniform_call(rank, n, 40 << 10, 0)
    c_src, c_dst, _ = uniform_call(rank, n, 777, 0)
    v_src, v_dst, _, (sc, sd, rc, rd) = v_call(rank, n, m, 2, 0)
    for nb in (40 << 10, 777):
        st.expect([nb] * n, [nb] * n, True)
    st.expect([c * 2 for c in sc], [c * 2 for c in rc], False)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        comm.all_to_all(a_src.ptr, a_dst.ptr, 40 << 10, U8, s.cuda_stream)
        comm.all_to_allv(v_src.ptr, sc, sd, v_dst.ptr, rc, rd, BF16, s.cuda_stream)
        comm.all_to_all(c_src.ptr, c_dst.ptr, 777, U8, s.cuda_stream)
        g.capture_end()
    for it in range(3):
        wants = []
        for (src, dst), fresh in (((a_src, a_dst), uniform_call(rank, n, 40 << 10, 400 + it)),
                                  ((v_src, v_dst), v_call(rank, n, m, 2, 410 + it)),
                                  ((c_src, c_dst), uniform_call(rank, n, 777, 420 + it))):
            src.buf.copy_(fresh[0].buf)
            dst.buf.fill_(SENTINEL)
            wants.append(fresh[2])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for name, dst, want in zip(("a2a", "a2av", "a2a 2"), (a_dst, v_dst, c_dst), wants):
            if not dst.ok(want):
                bad.append(("replay", it, name))
    return bad + st.bad()


def case_wrap(comm, rank, n, sp):
    """The LL epoch seeded just below the 32-bit wrap on every rank between
    calls, then four all-to-alls across it (epochs ...ffff, 2, 3, 4)."""
    bad = []
    st = Stats(comm, rank, n)
    comm.set_algo("ring")  # a call before the seeding that leaves no LL line behind
    x = torch.ones(1024, device="cuda")
    comm.all_reduce(x.data_ptr(), x.data_ptr(), 1024, F32, nccl.ncclSum, sp)
    torch.cuda.synchronize()
    comm.set_algo(None)
    comm.debug_set_epochs(0xFFFFFFFE, 0xFFFFFFFE)
    for i, nb in enumerate((4099, 8, LIMIT, 1)):
        src, dst, want = run_uniform(comm, st, rank, n, sp, nb, 500 + i, i % 2, 1)
        torch.cuda.synchronize()
        if comm.async_error() or not dst.ok(want):
            bad.append((i, nb))
    return bad + st.bad()


def case_off(comm, rank, n, sp):
    """The path is off (threshold unset, a net peer, or LL excluded): no LL
    launch, results exact where the comm can send at all (a comm with a net
    peer refuses point-to-point as before); where nothing else forbids it,
    vcclCommSetA2aThreshold turns the path on and off again."""
    bad = []
    can_be_on = os.environ.get("NCCL_PROTO") is None and os.environ.get("VCCL_NET_FORCE") is None
    net = os.environ.get("VCCL_NET_FORCE") is not None

    def one(nb, tag, limit):
        src, dst, want = uniform_call(rank, n, nb, tag)
        st.expect([nb] * n, [nb] * n, True, limit)
        comm.all_to_all(src.ptr, dst.ptr, nb, U8, sp)
        torch.cuda.synchronize()
        if not dst.ok(want):
            bad.append(("alltoall", nb, limit))

    st = Stats(comm, rank, n)
    if net:
        src, dst, want = uniform_call(rank, n, 4099, 1)
        rc = nccl.lib().ncclAllToAll(src.ptr, dst.ptr, 4099, U8, comm.handle, sp)
        if rc != nccl.ncclInvalidUsage:
            bad.append(("alltoall on a net comm returned", rc))
    else:
        one(4099, 1, 0)
        one(FIFO_BYTES, 2, 0)
    eff = comm.set_a2a_threshold(LIMIT)
    if eff != (LIMIT if can_be_on else 0):
        bad.append(("effective", eff))
    if not net:
        one(4099, 3, eff)
        one(LIMIT + 1, 4, eff)
        if comm.set_a2a_threshold(8 << 20) != (1 << 20 if can_be_on else 0):  # clamped to the slot
            bad.append(("clamp",))
        if comm.set_a2a_threshold(0) != 0:
            bad.append(("off again",))
        one(4099, 5, 0)
    if st.want[0] != (1 if can_be_on else 0):
        bad.append(("planned launches", st.want))
    return bad + st.bad()


CASES = {"uniform": case_uniform, "v_mixed": case_v_mixed, "group_mixed": case_group_mixed, "b2b": case_b2b,
         "capture": case_capture, "wrap": case_wrap, "off": case_off}


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
