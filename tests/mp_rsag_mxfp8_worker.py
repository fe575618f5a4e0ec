"""One rank of tests/test_gpu_rsag_mxfp8.py: the direct reduce-scatter and all-gather in the MXFP8 wire format
 against the CPU model of tests/mp_ar_mxfp8_worker.py.  argv: rank nranks uid_hex case
outdir.  Every rank derives all ranks' inputs from the seed and checks its own output; exit 0 when it is right."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests.mp_ar_mxfp8_worker import (SENTINEL, TYPES, allreduce, inputs, model_allreduce, roundtrip,  # noqa: E402
                                      same, small_ints)

AR, RS, AG, PAD = 0, 1, 2, 8
HALF_ULP = {9: 2.0 ** -8, 6: 2.0 ** -11}


def fold(pieces):  # every + a float32 add, ascending rank order
    acc = roundtrip(pieces[0])
    for x in pieces[1:]:
        acc = acc + roundtrip(x)
    return acc


def model(coll, xs, p, c, t):
    """Rank p's output.  Reduce-scatter: xs[r] holds n * c elements, blocks cut within [p c, p c + c); all-gather:
    xs[r] holds c elements."""
    if coll == RS:
        return fold([x[p * c:(p + 1) * c] for x in xs]).to(t)
    return torch.cat([roundtrip(x).to(t) for x in xs])


def rs_bound(xs, p, c, dt):
    """(exact float64 sum, tolerance): sum_r amax_r(block) / 14 (the E4M3 half ulp 16 against a scaled block maximum
    above 224) + the narrowing's half ulp + the binary32 adds' n * 2^-23 * sum_r amax_r(block)."""
    pieces = [x[p * c:(p + 1) * c].double() for x in xs]
    exact = sum(pieces)
    amax = torch.zeros((c + 31) // 32 * 32, dtype=torch.float64)
    for x in pieces:
        v = torch.zeros_like(amax)
        v[:c] = x.abs()
        amax += v.view(-1, 32).amax(1, keepdim=True).expand(-1, 32).reshape(-1)
    return exact, amax[:c] / 14 + HALF_ULP[dt] * exact.abs() + len(xs) * 2.0 ** -23 * amax[:c]


def three_chunk_count(n):
    """A per-rank count that moves through the inbox in three chunks (host/plan.cc direct_mx_plan, one shard)."""
    region = (max(int(os.environ["VCCL_DIRECT_CHUNK_BYTES"]), 64 << 10) + n - 1) // n // 256 * 256 + 256
    return 2 * (region // 528 * 512) + 1031


def call(comm, rank, n, sp, coll, x, dt, c, mode, op=0):
    """One reduce-scatter / all-gather of x (float32 values, exact in the type) with per-rank count c; returns
    (output, every byte outside it intact).  off1: both buffers one element past 16-byte alignment."""
    t, off = TYPES[dt], int(mode == "off1")
    nin, nout = (n * c, c) if coll == RS else (c, n * c)
    if mode == "inplace":  # one buffer: the larger operand between two pads, the smaller at its rank's block
        raw = torch.full(((n * c + 2 * PAD) * t.itemsize,), SENTINEL, dtype=torch.uint8).cuda()
        lo, o0 = (PAD, PAD + rank * c) if coll == RS else (PAD + rank * c, PAD)
        raw.view(t)[lo:lo + nin] = x.to(t).cuda()
        send = raw.view(t)[lo:]
    else:
        send = torch.zeros(nin + off, dtype=t).cuda()[off:]
        send[:] = x.to(t).cuda()
        raw, o0 = torch.full(((nout + off + PAD) * t.itemsize,), SENTINEL, dtype=torch.uint8).cuda(), off
    before = raw.cpu().view(t)
    recv = raw.view(t)[o0:]
    if coll == RS:
        comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), c, dt, op, sp)
    else:
        comm.all_gather(send.data_ptr(), recv.data_ptr(), c, dt, sp)
    torch.cuda.synchronize()
    got = raw.cpu().view(t)
    return got[o0:o0 + nout], same(got[:o0], before[:o0]) and same(got[o0 + nout:], before[o0 + nout:])


def case_cases(comm, nccl, rank, n, sp):
    bad = []
    for dt in (9, 6):
        for c in (1, 33, 513, 4099, three_chunk_count(n)):
            for coll in (RS, AG):
                xs = [inputs(7919 * c + 31 * dt + 3 * coll + r, n * c if coll == RS else c) for r in range(n)]
                exp = model(coll, xs, rank, c, TYPES[dt])
                if coll == RS:
                    exact, tol = rs_bound(xs, rank, c, dt)
                    err = (exp.double() - exact).abs()
                    print(f"dt {dt} c {c}: max err / tol {float((err / tol.clamp_min(1e-300)).max()):.4f}")
                    if not bool((err <= tol).all()):
                        bad.append((dt, c, "bound"))
                for mode in ("out", "inplace", "off1"):
                    before = comm.rsag_mxfp8_stats()
                    got, intact = call(comm, rank, n, sp, coll, xs[rank], dt, c, mode)
                    moved = tuple(a - b for a, b in zip(comm.rsag_mxfp8_stats(), before))
                    if not (same(got, exp) and intact and moved == (int(coll == RS), int(coll == AG))):
                        bad.append((dt, c, coll, mode, same(got, exp), intact, moved))
    return bad


def case_mixed(comm, nccl, rank, n, sp):
    """n = 4: native and MXFP8 kernels in turn on one inbox, the untouched calls, a mixed group, the switch off."""
    bad, c, bf = [], 1024, torch.bfloat16
    xs = [small_ints(200 + r, n * c) for r in range(n)]
    mine = slice(rank * c, (rank + 1) * c)
    exact = torch.stack(xs).sum(0)[mine]
    ys = [x[:c] for x in xs]  # the all-gather's inputs
    mx_rs, mx_ag = model(RS, xs, rank, c, bf), model(AG, ys, rank, c, bf)
    native_ag = torch.cat(ys).to(bf)
    assert not same(mx_rs, exact.to(bf)) and not same(mx_ag, native_ag)  # the format shows on these inputs

    def step(name, coll, x, dt, exp, grows, op=nccl.ncclSum):
        before = comm.rsag_mxfp8_stats() + (comm.ar_mxfp8_stats(),)
        got, intact = call(comm, rank, n, sp, coll, x, dt, c, "out", op)
        moved = tuple(a - b for a, b in zip(comm.rsag_mxfp8_stats() + (comm.ar_mxfp8_stats(),), before))
        bad.extend([name] * (not (same(got, exp) and intact and moved == grows)))

    if [comm.coll_algo(k, 4, dt) for k in (RS, AG) for dt in (9, 6)] != ["direct"] * 4 or \
            comm.coll_algo(RS, 4, 7) == "direct" or comm.coll_algo(AG, 4, 1) == "direct" or \
            comm.coll_algo(RS, c, 7) != "direct":
        bad.append("algo")
    step("f32 native rs", RS, xs[rank], 7, exact, (0, 0, 0))
    step("mx rs", RS, xs[rank], 9, mx_rs, (1, 0, 0))
    b = torch.arange(4099, dtype=torch.uint8).cuda() + rank  # a native byte all-gather
    out = torch.zeros(n * 4099, dtype=torch.uint8).cuda()
    comm.all_gather(b.data_ptr(), out.data_ptr(), 4099, 1, sp)
    torch.cuda.synchronize()
    exp = torch.cat([torch.arange(4099, dtype=torch.uint8) + r for r in range(n)])
    bad.extend(["u8 ag"] * (not same(out.cpu(), exp)))
    step("mx ag", AG, ys[rank], 9, mx_ag, (0, 1, 0))
    before = comm.rsag_mxfp8_stats() + (comm.ar_mxfp8_stats(),)
    got, intact = allreduce(comm, nccl, sp, ys[rank], 9, nccl.ncclSum, "out")
    after = comm.rsag_mxfp8_stats() + (comm.ar_mxfp8_stats(),)
    bad.extend(["mx ar"] * (not (same(got, model_allreduce(ys, bf)) and intact and
                                 after == before[:2] + (before[2] + 1,))))
    step("mx rs 2", RS, xs[rank], 9, mx_rs, (1, 0, 0))
    # the calls the switch leaves alone: avg (premultiplied by 1 / 4, exact) and max
    step("bf16 avg", RS, xs[rank], 9, (exact * 0.25).to(bf), (0, 0, 0), nccl.ncclAvg)
    step("bf16 max", RS, xs[rank], 9, torch.stack(xs).amax(0)[mine].to(bf), (0, 0, 0), nccl.ncclMax)
    # one group: an eligible reduce-scatter and a native one
    before = comm.rsag_mxfp8_stats()
    a, f = xs[rank].to(bf).cuda(), xs[rank].cuda()
    ya, yf = torch.zeros(c, dtype=bf).cuda(), torch.zeros(c).cuda()
    nccl.group_start()
    comm.reduce_scatter(a.data_ptr(), ya.data_ptr(), c, 9, nccl.ncclSum, sp)
    comm.reduce_scatter(f.data_ptr(), yf.data_ptr(), c, 7, nccl.ncclSum, sp)
    nccl.group_end()
    torch.cuda.synchronize()
    bad.extend(["group"] * (not (same(ya.cpu(), mx_rs) and same(yf.cpu(), exact) and
                                 comm.rsag_mxfp8_stats() == (before[0] + 1, before[1]))))
    bad.extend(["threshold 0"] * (comm.set_rsag_mxfp8_threshold(0) != 0))  # off again: native bits, counters unmoved
    step("bf16 native rs", RS, xs[rank], 9, exact.to(bf), (0, 0, 0))
    step("bf16 native ag", AG, ys[rank], 9, native_ag, (0, 0, 0))
    return bad


def main():
    from tests import _mp
    from vccl_amd import nccl
    rank, n, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4]
    _mp.bind(rank, n)
    comm = nccl.Comm.init_rank(n, nccl.unique_id_from_bytes(bytes.fromhex(sys.argv[3])), rank)
    bad = {"cases": case_cases, "mixed": case_mixed}[case](comm, nccl, rank, n, torch.cuda.current_stream().cuda_stream)
    err = comm.async_error()
    comm.destroy()
    if bad or err:
        print(f"rank {rank} case {case}: {bad[:8]} ({len(bad)} bad) async error {err}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
