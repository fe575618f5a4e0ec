#!/usr/bin/env python3
"""One rank of the direct broadcast / reduce tests (tests/test_gpu_direct_rooted.py).

argv: rank nranks uid_hex case outdir
The parent sets the shared-GPU geometry and VCCL_DIRECT_ROOTED_THRESHOLD (or
leaves it out, case "off").  Every case checks what it can locally; reduce
outputs go to outdir/rank<r>.npz for the parent's oracle check.  Exit 0 when
the local checks pass."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tests import ring_cases as RC  # noqa: E402
from tests import _mp  # noqa: E402
from tests.mp_ll_rooted_worker import (GROUP_AR, GROUP_BCASTS, GROUP_REDUCES, SENTINEL, Dest,  # noqa: E402
                                       group_reduce_input, ints_f32, ints_sum, payload, to_dev)
from vccl_amd import nccl  # noqa: E402

U8, F32 = nccl.ncclUint8, nccl.ncclFloat32
AR, RS, AG, BC, RED = 0, 1, 2, 3, 4
DIRECT_ROOTED_MAX = 8 << 20
MULTI_RED, MULTI_BC = 300_001, 1_200_007


def region_bytes(n):
    """host/setup.cc: the inbox region of this comm's VCCL_DIRECT_CHUNK_BYTES."""
    chunk = max(int(os.environ.get("VCCL_DIRECT_CHUNK_BYTES", 16 << 20)), 64 << 10)
    return (chunk + n - 1) // n // 256 * 256 + 256


def bcast_chunk(n):
    return nccl.direct_rooted_plan(BC, n, 0, 0, 1 << 30, U8, region_bytes(n))["chunk_elts"]


def bcast_sizes(n):
    sizes = [1, 15, 16, 17, 4099, 65541]
    for k in (1, 257):
        sizes += [16 * (n - 1) * k - 1, 16 * (n - 1) * k + 1]
    return sizes + [3 * bcast_chunk(n) + 5]


def multi_reduce_input(rank):
    return np.random.default_rng(9100 + rank).uniform(-1, 1, MULTI_RED).astype(np.float32)


def run_bcast(comm, rank, root, nbytes, off, inplace, tag, sp):
    """One broadcast into a guarded destination; True when every byte is right."""
    want = payload(nbytes, tag)
    dst = Dest(nbytes, off)
    if inplace:
        if rank == root:
            dst.buf[off:off + nbytes] = to_dev(want)
        torch.cuda.synchronize()
        nccl.check(nccl.lib().ncclBcast(ctypes.c_void_p(dst.ptr), ctypes.c_size_t(nbytes), U8, root, comm.handle,
                                        ctypes.c_void_p(sp)), "ncclBcast")
    else:
        src = to_dev(want) if rank == root else None
        torch.cuda.synchronize()
        comm.broadcast(src.data_ptr() if rank == root else 0, dst.ptr, nbytes, U8, root, sp)
    torch.cuda.synchronize()
    return dst.ok(want)


def case_bcast(comm, rank, n, sp, res):
    bad, tag = [], 0
    for nbytes in bcast_sizes(n):
        if comm.coll_algo(BC, nbytes, U8) != "direct":
            bad.append(("algo", nbytes, comm.coll_algo(BC, nbytes, U8)))
        for root in range(n):
            for off in (0, 1, 3):
                for inplace in (False, True):
                    tag += 1
                    if not run_bcast(comm, rank, root, nbytes, off, inplace, tag, sp):
                        bad.append((nbytes, root, off, inplace))
    return bad


def case_reduce(comm, rank, n, sp, res):
    bad = []
    for ri, (name, op, dt, count, inplace) in enumerate(RC.REDUCE_CASES):
        x = RC.gen_reduce_input(ri, rank)
        want_algo = "direct" if x.nbytes <= DIRECT_ROOTED_MAX else "ring"
        algo = comm.coll_algo(RED, count, dt)
        if algo != want_algo:
            bad.append((name, "algo", algo))
        for root in range(n):
            xb = to_dev(x)
            if inplace:
                comm.reduce(xb.data_ptr(), xb.data_ptr(), count, dt, op, root, sp)
                yb = xb
            else:
                yb = torch.full((x.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
                null = rank != root and (rank + root) % 2 == 1  # a non-root's recvbuff: NULL or untouched
                comm.reduce(xb.data_ptr(), 0 if null else yb.data_ptr(), count, dt, op, root, sp)
            torch.cuda.synchronize()
            if rank == root:
                res[f"{name}_r{root}"] = yb.cpu().numpy().view(x.dtype)
            elif inplace and not np.array_equal(yb.cpu().numpy(), x.view(np.uint8)):
                bad.append((name, root, "non-root buffer written"))
            elif not inplace and not bool((yb == SENTINEL).all()):
                bad.append((name, root, "non-root output written"))
            if not inplace and not np.array_equal(xb.cpu().numpy(), x.view(np.uint8)):
                bad.append((name, root, "input written"))
    return bad


def case_multichunk(comm, rank, n, sp, res):
    """VCCL_DIRECT_CHUNK_BYTES=65536: about 19 chunks per call."""
    bad = []
    nch_red = nccl.direct_rooted_plan(RED, n, rank, 0, MULTI_RED, F32, region_bytes(n))["n_chunks"]
    nch_bc = nccl.direct_rooted_plan(BC, n, rank, 0, MULTI_BC, U8, region_bytes(n))["n_chunks"]
    if min(nch_red, nch_bc) < 17:
        bad.append(("chunks", nch_red, nch_bc))
    if comm.coll_algo(RED, MULTI_RED, F32) != "direct" or comm.coll_algo(BC, MULTI_BC, U8) != "direct":
        bad.append(("algo",))
    x = multi_reduce_input(rank)
    for root in (0, n - 1):
        xb = to_dev(x)
        yb = torch.full((x.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        comm.reduce(xb.data_ptr(), yb.data_ptr() if rank == root else 0, MULTI_RED, F32, nccl.ncclSum, root, sp)
        torch.cuda.synchronize()
        if rank == root:
            res[f"multi_r{root}"] = yb.cpu().numpy().view(np.float32)
        if not np.array_equal(xb.cpu().numpy(), x.view(np.uint8)):
            bad.append(("reduce input written", root))
        for off, inplace in ((0, False), (3, True)):
            if not run_bcast(comm, rank, root, MULTI_BC, off, inplace, 400 + 10 * root + off, sp):
                bad.append(("bcast", root, off, inplace))
    return bad


def case_groups(comm, rank, n, sp, res):
    bad = []
    # five broadcasts from different roots, one of them empty: one launch
    outs, wants = [], []
    for i, (tdt, code, cnt, root) in enumerate(GROUP_BCASTS):
        esz = nccl.TYPE_SIZE[code]
        want = payload(cnt * esz, 700 + i)
        dst = Dest(cnt * esz)
        if rank == root % n:
            dst.buf[:cnt * esz] = to_dev(want)
        outs.append(dst)
        wants.append(want)
    res["bcast_group_algos"] = np.array(comm.group_algos([(BC, cnt, code, 0) for _, code, cnt, _ in GROUP_BCASTS]))
    torch.cuda.synchronize()
    ops0, fused0 = comm.launch_stats()
    nccl.group_start()
    for i, (tdt, code, cnt, root) in enumerate(GROUP_BCASTS):
        comm.broadcast(outs[i].ptr, outs[i].ptr, cnt, code, root % n, sp)
    comm.broadcast(0, 0, 0, F32, 0, sp)  # count 0: no task, no launch
    nccl.group_end()
    torch.cuda.synchronize()
    ops1, fused1 = comm.launch_stats()
    if (ops1 - ops0, fused1 - fused0) != (len(GROUP_BCASTS), 1):
        bad.append(("bcast group launches", ops1 - ops0, fused1 - fused0))
    for i, want in enumerate(wants):
        if not outs[i].ok(want):
            bad.append(("bcast group", i))
    # four reduces of one type and op to different roots + a 4 MiB all-reduce
    ins = [to_dev(group_reduce_input(k, rank)) for k in range(len(GROUP_REDUCES))]
    routs = [torch.full_like(b, SENTINEL) for b in ins]
    x = torch.empty(GROUP_AR, device="cuda")
    bench.pattern_fill(x, rank, n, base=5 << 20)
    y = torch.full_like(x, float("nan"))
    gcalls = [(RED, cnt, F32, nccl.ncclSum) for cnt, _ in GROUP_REDUCES] + [(AR, GROUP_AR, F32, nccl.ncclSum)]
    res["group_algos"] = np.array(comm.group_algos(gcalls))
    torch.cuda.synchronize()
    ops0, fused0 = comm.launch_stats()
    nccl.group_start()
    for k, (cnt, root) in enumerate(GROUP_REDUCES):
        comm.reduce(ins[k].data_ptr(), routs[k].data_ptr(), cnt, F32, nccl.ncclSum, root % n, sp)
    comm.all_reduce(x.data_ptr(), y.data_ptr(), GROUP_AR, F32, nccl.ncclSum, sp)
    nccl.group_end()
    torch.cuda.synchronize()
    ops1, fused1 = comm.launch_stats()
    if (ops1 - ops0, fused1 - fused0) != (len(GROUP_REDUCES) + 1, 1):
        bad.append(("reduce group launches", ops1 - ops0, fused1 - fused0))
    for k, (cnt, root) in enumerate(GROUP_REDUCES):
        if rank == root % n:
            res[f"group{k}"] = routs[k].cpu().numpy().view(np.float32)
        elif not bool((routs[k] == SENTINEL).all()):
            bad.append(("reduce group", k, "non-root output written"))
    if not bench.pattern_ok(y, n, base=5 << 20):
        bad.append(("group all-reduce",))
    return bad


# the back-to-back cycle: (kind, f32 elements or bytes); the all-reduces span
# 1, 2 and 3 chunks of the 128 KiB inbox of this case, so their last chunk
# leaves either parity behind
B2B_CYCLE = [("ar", 30_000), ("bc", 250_001), ("red", 60_001), ("rs", 64_000),("ar", 62_500), ("ag", 230_000),
             ("bc", 299_999), ("ar", 75_000), ("red", 74_999)]
B2B_CALLS = 96


def case_b2b(comm, rank, n, sp, res):
    """No host synchronisation between calls: the test of the inbox reuse rule."""
    bad = []
    comm.set_algo("direct")  # every collective on the inbox, at any size
    for coll, cnt in ((AR, 30_000), (RS, 1000), (AG, 1000), (BC, 1000), (RED, 1000)):
        a = comm.coll_algo(coll, cnt, U8 if coll in (AG, BC) else F32)
        if a != "direct":
            bad.append(("path", coll, a))
    reg = region_bytes(n)
    chunks = sorted({-(-cnt // ((reg - 16) // 4 * n // (n * 4) * (n * 4))) for kind, cnt in B2B_CYCLE if kind == "ar"})
    if chunks != [1, 2, 3]:
        bad.append(("all-reduce chunks", chunks))
    plan, srcs, dsts = [], [], []
    for i in range(B2B_CALLS):
        kind, cnt = B2B_CYCLE[i % len(B2B_CYCLE)]
        root, tag = i % n, 500 + i
        plan.append((kind, cnt, root, tag))
        if kind == "bc":
            srcs.append(to_dev(payload(cnt, tag)) if rank == root else None)
            dsts.append(Dest(cnt, i % 2))
        elif kind == "ag":
            per = cnt // n
            srcs.append(to_dev(payload(per, tag * 16 + rank)))
            dsts.append(Dest(per * n))
        elif kind == "rs":
            per = cnt // n
            srcs.append(to_dev(ints_f32(per * n, rank, tag)))
            dsts.append(Dest(4 * per))
        else:
            srcs.append(to_dev(ints_f32(cnt, rank, tag)))
            dsts.append(Dest(4 * cnt))
    torch.cuda.synchronize()
    for (kind, cnt, root, tag), src, dst in zip(plan, srcs, dsts):
        if kind == "bc":
            comm.broadcast(src.data_ptr() if rank == root else 0, dst.ptr, cnt, U8, root, sp)
        elif kind == "red":
            comm.reduce(src.data_ptr(), dst.ptr if rank == root else 0, cnt, F32, nccl.ncclSum, root, sp)
        elif kind == "ar":
            comm.all_reduce(src.data_ptr(), dst.ptr, cnt, F32, nccl.ncclSum, sp)
        elif kind == "rs":
            comm.reduce_scatter(src.data_ptr(), dst.ptr, cnt // n, F32, nccl.ncclSum, sp)
        else:
            comm.all_gather(src.data_ptr(), dst.ptr, cnt // n, U8, sp)
    torch.cuda.synchronize()
    for i, ((kind, cnt, root, tag), dst) in enumerate(zip(plan, dsts)):
        if kind == "bc":
            want = payload(cnt, tag)
        elif kind == "ag":
            want = np.concatenate([payload(cnt // n, tag * 16 + r) for r in range(n)])
        elif kind == "rs":
            per = cnt // n
            want = ints_sum(per * n, n, tag)[rank * per:(rank + 1) * per].view(np.uint8)
        elif kind == "ar" or rank == root:
            want = ints_sum(cnt, n, tag).view(np.uint8)
        else:
            want = np.full(4 * cnt, SENTINEL, np.uint8)
        if not dst.ok(want):
            bad.append((i, kind, root))
    return bad


def case_capture(comm, rank, n, sp, res):
    """[broadcast root 0, reduce root 1, broadcast root 1] captured on one
    stream, replayed three times with fresh inputs."""
    bad = []
    nb, cnt = 40 << 10, 5000
    if comm.coll_algo(BC, nb, U8) != "direct" or comm.coll_algo(RED, cnt, F32) != "direct":
        bad.append(("path",))
    b0, b1 = Dest(nb), Dest(nb)
    rin = torch.zeros(cnt, device="cuda")
    rout = Dest(4 * cnt)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="relaxed")
        comm.broadcast(b0.ptr, b0.ptr, nb, U8, 0, s.cuda_stream)
        comm.reduce(rin.data_ptr(), rout.ptr if rank == 1 else 0, cnt, F32, nccl.ncclSum, 1, s.cuda_stream)
        comm.broadcast(b1.ptr, b1.ptr, nb, U8, 1, s.cuda_stream)
        g.capture_end()
    for it in range(3):
        for root, b in ((0, b0), (1, b1)):
            b.buf.fill_(SENTINEL)
            if rank == root:
                b.buf[:nb] = to_dev(payload(nb, 900 + 10 * it + root))
        rin.copy_(torch.from_numpy(ints_f32(cnt, rank, 40 + it)))
        rout.buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_r = ints_sum(cnt, n, 40 + it).view(np.uint8) if rank == 1 else np.full(4 * cnt, SENTINEL, np.uint8)
        if not (b0.ok(payload(nb, 900 + 10 * it)) and b1.ok(payload(nb, 901 + 10 * it)) and rout.ok(want_r)):
            bad.append(("replay", it))
    return bad


def case_wrap(comm, rank, n, sp, res):
    """The direct epoch seeded just below the 32-bit wrap on every rank between
    calls, then two broadcasts and two reduces across it."""
    bad = []
    comm.set_algo("ring")  # a call before the seeding that leaves no inbox flag behind
    x = torch.ones(1024, device="cuda")
    comm.all_reduce(x.data_ptr(), x.data_ptr(), 1024, F32, nccl.ncclSum, sp)
    torch.cuda.synchronize()
    comm.set_algo(None)
    comm.debug_set_epochs(0xFFFFFFFE, 0xFFFFFFFE)
    nb, cnt = 4099, 3001
    for i, kind in enumerate(("bc", "red", "bc", "red")):
        root = i % n
        if kind == "bc":
            want = payload(nb, 300 + i)
            src = to_dev(want) if rank == root else None
            dst = Dest(nb, 1)
            comm.broadcast(src.data_ptr() if rank == root else 0, dst.ptr, nb, U8, root, sp)
        else:
            src = to_dev(ints_f32(cnt, rank, 300 + i))
            dst = Dest(4 * cnt)
            comm.reduce(src.data_ptr(), dst.ptr if rank == root else 0, cnt, F32, nccl.ncclSum, root, sp)
            want = ints_sum(cnt, n, 300 + i).view(np.uint8) if rank == root else np.full(4 * cnt, SENTINEL, np.uint8)
        torch.cuda.synchronize()
        if comm.async_error() or not dst.ok(want):
            bad.append((i, kind))
    return bad


def case_off(comm, rank, n, sp, res):
    """The path is off: both collectives report a ring at every size, and still run."""
    bad = []
    for coll, dt, esz in ((BC, U8, 1), (RED, F32, 4)):
        for nbytes in (8, 4096, 100 << 10, 1 << 20, 8 << 20, 64 << 20):
            a = comm.coll_algo(coll, nbytes // esz, dt)
            if a not in ("ring", "ll128"):
                bad.append((coll, nbytes, a))
    want = payload(300_001, 77)
    src = to_dev(want) if rank == 0 else None
    dst = Dest(300_001)
    comm.broadcast(src.data_ptr() if rank == 0 else 0, dst.ptr, 300_001, U8, 0, sp)
    torch.cuda.synchronize()
    if not dst.ok(want):
        bad.append(("broadcast",))
    return bad


CASES = {"bcast": case_bcast, "reduce": case_reduce, "multichunk": case_multichunk, "groups": case_groups,
         "b2b": case_b2b, "capture": case_capture, "wrap": case_wrap, "off": case_off}


def main():
    rank, n = int(sys.argv[1]), int(sys.argv[2])
    uid = nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3]))
    case, outdir = sys.argv[4], sys.argv[5]
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
