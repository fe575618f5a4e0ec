#!/usr/bin/env python3
"""One rank of the one-hop direct all-to-all tests (tests/test_gpu_direct_a2a.py).

argv: rank nranks uid_hex case
The parent sets the shared-GPU geometry of the LL all-to-all tests and
VCCL_DIRECT_A2A_THRESHOLD (or leaves it out, case "off"); VCCL_LL_A2A_THRESHOLD
is read back from the environment, so a case runs two-way (direct + FIFO) or
three-way (LL + direct + FIFO) as the parent chose.  Every received byte is
compared with a seeded payload both ends can compute; destinations are
sentinel-filled with 64 guard bytes on each side; every case ends by comparing
vcclCommA2aStatsEx with what vcclDirectA2aPlan predicts.  Exit 0 on success."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tests import _mp  # noqa: E402
from tests.mp_ll_a2a_worker import SENTINEL, SLOT_LINES, Dest, Src, ints_f32, payload, uniform_call, v_call  # noqa: E402
from vccl_amd import nccl  # noqa: E402

U8, F32, BF16 = nccl.ncclUint8, nccl.ncclFloat32, nccl.ncclBfloat16
AR, RS, AG, BC, RED = 0, 1, 2, 3, 4
LIMIT = 98_304                # VCCL_DIRECT_A2A_THRESHOLD of the tests, bytes per pair
LL_LIMIT = int(os.environ.get("VCCL_LL_A2A_THRESHOLD", "0"))
FIFO_BYTES = 120_000          # a uniform row above the limit


def region_bytes(n):
    """host/setup.cc: the inbox region of this comm's VCCL_DIRECT_CHUNK_BYTES."""
    chunk = max(int(os.environ.get("VCCL_DIRECT_CHUNK_BYTES", 16 << 20)), 64 << 10)
    return (chunk + n - 1) // n // 256 * 256 + 256


class Stats:
    """What vcclCommA2aStatsEx must have grown by, from the pure plan:
    [LL launches, LL pairs, direct launches, direct pairs, FIFO pairs]."""

    def __init__(self, comm, rank, n):
        self.comm, self.rank, self.n = comm, rank, n
        self.base = comm.a2a_stats_ex()
        self.base3 = comm.a2a_stats()
        self.want = [0, 0, 0, 0, 0]

    def expect(self, send_bytes, recv_bytes, uniform, limit=LIMIT, ll_limit=LL_LIMIT):
        pl = nccl.direct_a2a_plan(self.n, self.rank, send_bytes, recv_bytes, uniform, ll_limit, limit, SLOT_LINES)
        paths = pl["send_path"] + pl["recv_path"]
        for i, v in enumerate((int(pl["ll_launch"]), paths.count(nccl.A2A_LL), int(pl["direct_launch"]),
                               paths.count(nccl.A2A_DIRECT), paths.count(nccl.A2A_FIFO))):
            self.want[i] += v
        return pl

    def bad(self):
        got = [a - b for a, b in zip(self.comm.a2a_stats_ex(), self.base)]
        got3 = [a - b for a, b in zip(self.comm.a2a_stats(), self.base3)]
        out = [] if got == self.want else [("a2a stats", got, self.want)]
        # vcclCommA2aStats keeps its meaning: the LL and FIFO counts alone
        return out + ([] if got3 == [self.want[0], self.want[1], self.want[4]] else [("a2a stats (3)", got3)])


def run_uniform(comm, st, rank, n, sp, nbytes, tag, soff=0, doff=0, dt=U8, limit=LIMIT):
    src, dst, want = uniform_call(rank, n, nbytes, tag, soff, doff)
    st.expect([nbytes] * n, [nbytes] * n, True, limit)
    comm.all_to_all(src.ptr, dst.ptr, nbytes // nccl.TYPE_SIZE[dt], dt, sp)
    return src, dst, want


def run_v(comm, st, rank, n, sp, cnt, dt, tag, limit=LIMIT):
    esz = nccl.TYPE_SIZE[dt]
    src, dst, want, (sc, sd, rc, rd) = v_call(rank, n, cnt, esz, tag)
    pl = st.expect([c * esz for c in sc], [c * esz for c in rc], False, limit)
    comm.all_to_allv(src.ptr, sc, sd, dst.ptr, rc, rd, dt, sp)
    return src, dst, want, pl


def mixed_matrix(n, seed=91):
    """bf16 element counts: zero counts, rank 1's row empty, pairs of 16,382 /
    16,386 / 98,304 / 98,306 bytes, one 300 KB pair (two wraps of a p2p part's
    FIFO in the test geometry), a self block above the limit; the small
    entries fall under a 4 KiB LL limit when the parent sets one."""
    m = np.random.default_rng(seed + n).choice([0, 1, 5, 37, 1000, 20_000], size=(n, n))
    m[1, :] = 0
    m[0, 1] = LIMIT // 2
    m[2, 0] = LIMIT // 2 + 1
    m[2, 1] = 8191
    m[2, 2] = 8193            # a self block within the limit: a local copy in the direct kernel
    m[0, 2] = 150_000
    m[0, 0] = 60_000
    return m


# -------------------------------------------------------------------- cases
def case_uniform(comm, rank, n, sp):
    bad, tag = [], 0
    st = Stats(comm, rank, n)
    sizes = [(1, U8), (15, U8), (16, U8), (17, U8), (16_384, U8), (16_385, U8), (49_153, U8), (LIMIT, U8),
             (12_000, F32)]
    for nbytes, dt in sizes:
        for soff, doff in ((0, 0), (1, 3), (3, 1)):
            tag += 1
            src, dst, want = run_uniform(comm, st, rank, n, sp, nbytes, tag, soff, doff, dt)
            torch.cuda.synchronize()
            if not dst.ok(want):
                bad.append((nbytes, soff, doff))
    calls = 3 * len(sizes)
    if st.want != [0, 0, calls, 2 * n * calls, 0]:
        bad.append(("planned", st.want))
    # one byte over the limit: today's path, no direct launch
    src, dst, want = run_uniform(comm, st, rank, n, sp, LIMIT + 1, 99)
    torch.cuda.synchronize()
    if not dst.ok(want) or st.want != [0, 0, calls, 2 * n * calls, 2 * n]:
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
        if not pl["direct_launch"] or pl["ll_launch"] != (LL_LIMIT > 0) or \
                (rank == 0 and pl["res_sends"] != [0, 2]) or (rank == 0 and pl["res_recvs"] != [0, 2]) or \
                (rank == 0 and pl["send_path"][1] != nccl.A2A_DIRECT) or \
                (rank == 2 and (pl["send_path"][1], pl["send_path"][2]) != (nccl.A2A_DIRECT,) * 2) or \
                (rank == 1 and (pl["res_sends"] or nccl.A2A_FIFO in pl["send_path"])):
            bad.append(("plan", pl))
        if LL_LIMIT and not (nccl.A2A_LL in pl["send_path"] + pl["recv_path"]):
            bad.append(("no LL pair in the three-way call", pl["send_path"]))
    return bad + st.bad()


def case_clamp(comm, rank, n, sp):
    """The threshold asks for 1 MiB: the effective limit is what a region
    holds; a pair exactly at it is exact, a pair 2 bytes over goes to the FIFOs."""
    bad = []
    cap = (region_bytes(n) - 16) // 16 * 16
    if nccl.direct_a2a_max(None, region_bytes(n), nranks=n) != cap or comm.set_direct_a2a_threshold(1 << 20) != cap:
        bad.append(("effective", cap))
    st = Stats(comm, rank, n)
    m = np.random.default_rng(17).choice([0, 3, 900, 30_000], size=(n, n))
    m[0, 1] = cap // 2
    m[1, 0] = cap // 2 + 1
    src, dst, want, pl = run_v(comm, st, rank, n, sp, m, BF16, 250, limit=cap)
    torch.cuda.synchronize()
    if not dst.ok(want):
        bad.append(("alltoallv",))
    if (rank == 0 and (pl["send_path"][1], pl["recv_path"][1]) != (nccl.A2A_DIRECT, nccl.A2A_FIFO)) or \
            (rank == 1 and (pl["send_path"][0], pl["recv_path"][0]) != (nccl.A2A_FIFO, nccl.A2A_DIRECT)):
        bad.append(("plan", pl["send_path"], pl["recv_path"]))
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
    if pl["res_sends"] != [(rank + 2) % n] or pl["res_recvs"] != [(rank - 2) % n] or not pl["direct_launch"]:
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


B2B_CYCLE = ("a2a", "ar", "rs", "ag", "bc", "red", "fifo", "v")


def case_b2b(comm, rank, n, sp):
    """No host synchronisation between calls: 48 calls cycling the direct
    all-to-all, the direct all-reduce, reduce-scatter and all-gather, the rooted
    direct broadcast and reduce, a FIFO all-to-all and a mixed all-to-allv — all
    six direct kernels on one inbox."""
    bad = []
    st = Stats(comm, rank, n)
    comm.set_algo("direct")  # every collective on the inbox, at any size
    for coll, cnt in ((AR, 30_000), (RS, 1000), (AG, 1000), (BC, 1000), (RED, 1000)):
        a = comm.coll_algo(coll, cnt, U8 if coll in (AG, BC) else F32)
        if a != "direct":
            bad.append(("path", coll, a))
    small = np.array([[0 if (a + b) % 3 == 0 else 100 + 40 * a + b for b in range(n)] for a in range(n)])
    small[0, n - 1] = 60_000  # one pair above the limit (bf16 elements)
    small[n - 1, 0] = 30_000  # ... and a mid-size direct one
    cnt = 6000 * n            # f32 elements of the reductions; bytes of the all-gather and broadcast
    plan = [(B2B_CYCLE[i % len(B2B_CYCLE)], 600 + i) for i in range(48)]
    prep = []
    for kind, tag in plan:
        root = tag % n
        if kind in ("a2a", "fifo"):
            nb = 40_001 if kind == "a2a" else FIFO_BYTES
            src, dst, want = uniform_call(rank, n, nb, tag, tag % 2, tag % 3)
            st.expect([nb] * n, [nb] * n, True)
            prep.append((src, dst, want, nb))
        elif kind == "v":
            src, dst, want, arg = v_call(rank, n, small, 2, tag)
            st.expect([c * 2 for c in arg[0]], [c * 2 for c in arg[2]], False)
            prep.append((src, dst, want, arg))
        elif kind == "ar":
            prep.append((Src(ints_f32(cnt, rank, tag).view(np.uint8)), Dest(4 * cnt),
                         sum(ints_f32(cnt, r, tag) for r in range(n)).view(np.uint8), None))
        elif kind == "rs":
            per = cnt // n
            total = sum(ints_f32(cnt, r, tag) for r in range(n))
            prep.append((Src(ints_f32(cnt, rank, tag).view(np.uint8)), Dest(4 * per),
                         total[rank * per:(rank + 1) * per].view(np.uint8), None))
        elif kind == "ag":
            per = cnt // n
            prep.append((Src(payload(per, rank, rank, tag)), Dest(cnt),
                         np.concatenate([payload(per, r, r, tag) for r in range(n)]), None))
        elif kind == "bc":
            want = payload(cnt, root, root, tag)
            prep.append((Src(want) if rank == root else None, Dest(cnt), want, root))
        else:
            total = sum(ints_f32(cnt, r, tag) for r in range(n)).view(np.uint8)
            prep.append((Src(ints_f32(cnt, rank, tag).view(np.uint8)), Dest(4 * cnt),
                         total if rank == root else np.full(4 * cnt, SENTINEL, np.uint8), root))
    torch.cuda.synchronize()
    for (kind, tag), (src, dst, want, arg) in zip(plan, prep):
        if kind in ("a2a", "fifo"):
            comm.all_to_all(src.ptr, dst.ptr, arg, U8, sp)
        elif kind == "v":
            comm.all_to_allv(src.ptr, arg[0], arg[1], dst.ptr, arg[2], arg[3], BF16, sp)
        elif kind == "ar":
            comm.all_reduce(src.ptr, dst.ptr, cnt, F32, nccl.ncclSum, sp)
        elif kind == "rs":
            comm.reduce_scatter(src.ptr, dst.ptr, cnt // n, F32, nccl.ncclSum, sp)
        elif kind == "ag":
            comm.all_gather(src.ptr, dst.ptr, cnt // n, U8, sp)
        elif kind == "bc":
            comm.broadcast(src.ptr if src else 0, dst.ptr, cnt, U8, arg, sp)
        else:
            comm.reduce(src.ptr, dst.ptr if rank == arg else 0, cnt, F32, nccl.ncclSum, arg, sp)
    torch.cuda.synchronize()
    for i, ((kind, tag), (src, dst, want, arg)) in enumerate(zip(plan, prep)):
        if not dst.ok(want):
            bad.append((i, kind))
    if st.want[2] != 12 or st.want[0] != 0:
        bad.append(("planned launches", st.want))
    return bad + st.bad()


def case_capture(comm, rank, n, sp):
    """[all-to-all, mixed all-to-allv, all-to-all] captured on one stream,
    replayed three times with fresh inputs."""
    bad = []
    st = Stats(comm, rank, n)
    m = np.array([[0, 60_000], [20_000, 9]])  # bf16 elements: 0 -> 1 above the limit, 1 -> 0 direct
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
    if st.want[2] != 3:
        bad.append(("planned launches", st.want))
    return bad + st.bad()


def case_wrap(comm, rank, n, sp):
    """The direct epoch seeded just below the 32-bit wrap on every rank between
    calls, then four all-to-alls across it (epochs ...ffff, 2, 3, 4)."""
    bad = []
    st = Stats(comm, rank, n)
    comm.set_algo("ring")  # a call before the seeding that leaves no inbox flag behind
    x = torch.ones(1024, device="cuda")
    comm.all_reduce(x.data_ptr(), x.data_ptr(), 1024, F32, nccl.ncclSum, sp)
    torch.cuda.synchronize()
    comm.set_algo(None)
    comm.debug_set_epochs(0xFFFFFFFE, 0xFFFFFFFE)
    for i, nb in enumerate((16_385, 16, LIMIT, 1)):
        src, dst, want = run_uniform(comm, st, rank, n, sp, nb, 500 + i, i % 2, 1)
        torch.cuda.synchronize()
        if comm.async_error() or not dst.ok(want):
            bad.append((i, nb))
    if st.want[2] != 4:
        bad.append(("planned launches", st.want))
    return bad + st.bad()


def case_fences(comm, rank, n, sp):
    """VCCL_FENCES=1: the acquire / release branches of direct_wait / direct_post."""
    bad = []
    st = Stats(comm, rank, n)
    for i, (nb, soff, doff) in enumerate(((49_153, 1, 3), (LIMIT, 0, 0), (17, 3, 1))):
        src, dst, want = run_uniform(comm, st, rank, n, sp, nb, 700 + i, soff, doff)
        torch.cuda.synchronize()
        if not dst.ok(want):
            bad.append((nb, soff, doff))
    if os.environ.get("VCCL_FENCES") != "1" or st.want[2] != 3:
        bad.append(("setup", st.want))
    return bad + st.bad()


def case_off(comm, rank, n, sp):
    """The path is off (threshold unset, a net peer, or Direct excluded): no
    direct launch, results exact where the comm can send at all (a comm with a
    net peer refuses point-to-point as before); where nothing else forbids it,
    vcclCommSetDirectA2aThreshold turns the path on and off again."""
    bad = []
    can_be_on = os.environ.get("NCCL_ALGO") is None and os.environ.get("VCCL_NET_FORCE") is None
    net = os.environ.get("VCCL_NET_FORCE") is not None
    cap = (region_bytes(n) - 16) // 16 * 16

    def one(nb, tag, limit):
        src, dst, want = uniform_call(rank, n, nb, tag)
        st.expect([nb] * n, [nb] * n, True, limit)
        comm.all_to_all(src.ptr, dst.ptr, nb, U8, sp)
        torch.cuda.synchronize()
        if not dst.ok(want):
            bad.append(("alltoall", nb, limit))

    st = Stats(comm, rank, n)
    if net:
        src, dst, want = uniform_call(rank, n, 40_001, 1)
        rc = nccl.lib().ncclAllToAll(src.ptr, dst.ptr, 40_001, U8, comm.handle, sp)
        if rc != nccl.ncclInvalidUsage:
            bad.append(("alltoall on a net comm returned", rc))
    else:
        one(40_001, 1, 0)
        one(FIFO_BYTES, 2, 0)
    eff = comm.set_direct_a2a_threshold(LIMIT)
    if eff != (LIMIT if can_be_on else 0):
        bad.append(("effective", eff))
    if not net:
        one(40_001, 3, eff)
        one(LIMIT + 1, 4, eff)
        if comm.set_direct_a2a_threshold(64 << 20) != (cap if can_be_on else 0):  # clamped to the region
            bad.append(("clamp",))
        if comm.set_direct_a2a_threshold(0) != 0:
            bad.append(("off again",))
        one(40_001, 5, 0)
    if st.want[2] != (1 if can_be_on else 0):
        bad.append(("planned launches", st.want))
    return bad + st.bad()


CASES = {"uniform": case_uniform, "v_mixed": case_v_mixed, "clamp": case_clamp, "group_mixed": case_group_mixed,
         "b2b": case_b2b, "capture": case_capture, "wrap": case_wrap, "fences": case_fences, "off": case_off}


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
