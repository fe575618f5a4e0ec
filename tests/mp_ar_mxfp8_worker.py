"""One rank of tests/test_gpu_ar_mxfp8.py, and the CPU model of the MXFP8 wire format that
the tests compare against.  argv: rank nranks uid_hex case outdir.  Every rank derives all ranks' inputs from the
seed and checks its own output; exit 0 when it is right."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

AR, RS, SENTINEL = 0, 1, 0x5a
TYPES = {6: torch.float16, 7: torch.float32, 9: torch.bfloat16}


def encode(x):
    """float32 vector -> (payload bytes [tiles * 512], scale bytes [tiles * 16]); blocks of 32 by element index,
    the last tile padded with zeros."""
    n = (x.numel() + 511) // 512 * 512
    v = torch.zeros(n, dtype=torch.float32)
    v[:x.numel()] = x
    v = v.view(-1, 32)
    amax = v.abs().amax(1).double()
    special = ~torch.isfinite(v).all(1)
    safe = torch.where((amax > 0) & ~special, amax, torch.ones_like(amax))
    e0 = torch.frexp(safe)[1] - 1 - 8  # floor(log2 amax) - 8
    e = e0 + (torch.ldexp(safe, -e0) > 448)
    s = torch.where(amax == 0, 127, (e + 127).clamp(0, 254))
    s = torch.where(special, 255, s)
    scaled = torch.ldexp(v.double(), (127 - s)[:, None].expand_as(v)).float().clamp(-448, 448)
    p = scaled.to(torch.float8_e4m3fn).view(torch.uint8).clone()
    p[special] = 0
    return p.reshape(-1), s.to(torch.uint8)


def decode(p, s):
    w = p.view(torch.float8_e4m3fn).float().double().view(-1, 32)
    v = torch.ldexp(w, (s.int() - 127)[:, None].expand(-1, 32)).float()
    v[s == 255] = float("nan")
    return v.reshape(-1)


def wire(x):  # the tile layout: 512 payload bytes, then the tile's 16 scale bytes
    p, s = encode(x)
    return torch.cat([p.view(-1, 512), s.view(-1, 16)], 1).reshape(-1)


def roundtrip(x):
    return decode(*encode(x))[:x.numel()]


def model_allreduce(xs, t):  # every + a float32 add, ascending rank order; one narrowing
    acc = roundtrip(xs[0])
    for x in xs[1:]:
        acc = acc + roundtrip(x)
    return roundtrip(acc).to(t)


def inputs(seed, count):
    """m * 2^k, m = +-(1 + j / 128), k per element from [-12, 4]; block 1 and tile 1 all zero (where they exist)."""
    g = np.random.default_rng(seed)
    m = (1 + g.integers(0, 128, count) / 128.0) * g.choice([-1.0, 1.0], count)
    x = torch.from_numpy(np.ldexp(m, g.integers(-12, 5, count)).astype(np.float32))
    x[32:64] = 0
    x[512:1024] = 0
    return x


def small_ints(seed, count):  # k / 4, |k| <= 31: every native fold of up to 8 of them is exact in any order
    return torch.from_numpy(np.random.default_rng(seed).integers(-31, 32, count).astype(np.float32)) * 0.25


def three_chunk_count(n):
    """A count that moves through the inbox in three chunks (host/setup.cc's region, host/plan.cc direct_mx_plan)."""
    region = (max(int(os.environ["VCCL_DIRECT_CHUNK_BYTES"]), 64 << 10) + n - 1) // n // 256 * 256 + 256
    return 2 * (region // 528 * n * 512) + 1031


def allreduce(comm, nccl, sp, x, dt, op, mode):
    """One all-reduce of x (float32 values, exact in the type); returns (result, sentinels intact)."""
    t, off = TYPES[dt], int(mode == "off1")
    esz, count = t.itemsize, x.numel()
    send = torch.zeros(count + off, dtype=t).cuda()
    send[off:] = x.to(t).cuda()
    raw = torch.full(((count + off + 8) * esz,), SENTINEL, dtype=torch.uint8).cuda()
    recv = raw.view(t)
    if mode == "inplace":
        recv[:count] = send
    comm.all_reduce(send[off:].data_ptr() if mode != "inplace" else recv.data_ptr(), recv[off:].data_ptr(), count, dt,
                    op, sp)
    torch.cuda.synchronize()
    got = raw.cpu()
    intact = bool((got[:off * esz] == SENTINEL).all()) and bool((got[(off + count) * esz:] == SENTINEL).all())
    return got[off * esz:(off + count) * esz].view(t), intact


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def case_cases(comm, nccl, rank, n, sp):
    bad = []
    for dt in (9, 6):
        for count in (1, 33, 513, 4099, three_chunk_count(n)):
            xs = [inputs(7919 * count + 31 * dt + r, count) for r in range(n)]
            exp = model_allreduce(xs, TYPES[dt])
            for mode in ("out", "inplace", "off1"):
                before = comm.ar_mxfp8_stats()
                got, intact = allreduce(comm, nccl, sp, xs[rank], dt, nccl.ncclSum, mode)
                if not (same(got, exp) and intact and comm.ar_mxfp8_stats() == before + 1):
                    bad.append((dt, count, mode, same(got, exp), intact))
    return bad


def case_mixed(comm, nccl, rank, n, sp):
    """n = 4: native and MXFP8 kernels in turn on one inbox, the untouched calls, a mixed group, the switch off."""
    from oracle import oracle as O
    bad, count = [], 4099
    xs = [small_ints(100 + r, count) for r in range(n)]
    exact = torch.stack(xs).sum(0)
    bits = [O.f32_to_bf16_bits(x.numpy()) for x in xs]
    native_bf16 = torch.from_numpy(O.allreduce(nccl.ncclSum, 9, bits).view(np.int16)).view(torch.bfloat16)
    assert same(native_bf16, exact.to(torch.bfloat16))
    mx = model_allreduce(xs, torch.bfloat16)

    def step(name, dt, op, exp, grows):
        before = comm.ar_mxfp8_stats()
        got, intact = allreduce(comm, nccl, sp, xs[rank], dt, op, "out")
        bad.extend([name] * (not (same(got, exp) and intact and comm.ar_mxfp8_stats() == before + grows)))

    def reduce_scatter(name, per=count // n):
        x, y = xs[rank].cuda(), torch.zeros(per, device="cuda")
        comm.reduce_scatter(x.data_ptr(), y.data_ptr(), per, 7, nccl.ncclSum, sp)
        torch.cuda.synchronize()
        bad.extend([name] * (not same(y.cpu(), exact[rank * per:(rank + 1) * per])))

    # an eligible call reports the direct path at any size; the native f32 calls below run the native direct kernels
    if comm.coll_algo(AR, 4, 9) != "direct" or comm.coll_algo(AR, 4, 7) == "direct" or \
            comm.coll_algo(AR, count, 7) != "direct" or comm.coll_algo(RS, count // n, 7) != "direct":
        bad.append("algo")
    step("f32 native", 7, nccl.ncclSum, exact, 0)
    step("mx 1", 9, nccl.ncclSum, mx, 1)
    reduce_scatter("reduce-scatter")
    step("mx 2", 9, nccl.ncclSum, mx, 1)
    # the calls the switch leaves alone: avg (premultiplied by 1 / 4, exact), max, and f32 above
    step("bf16 avg", 9, nccl.ncclAvg, (exact * 0.25).to(torch.bfloat16), 0)
    step("bf16 max", 9, nccl.ncclMax, torch.stack(xs).amax(0).to(torch.bfloat16), 0)
    # one group: an eligible call and a native all-reduce
    before = comm.ar_mxfp8_stats()
    a, b = xs[rank].to(torch.bfloat16).cuda(), xs[rank].cuda()
    ya, yb = torch.zeros_like(a), torch.zeros_like(b)
    nccl.group_start()
    comm.all_reduce(a.data_ptr(), ya.data_ptr(), count, 9, nccl.ncclSum, sp)
    comm.all_reduce(b.data_ptr(), yb.data_ptr(), count, 7, nccl.ncclSum, sp)
    nccl.group_end()
    torch.cuda.synchronize()
    bad.extend(["group"] * (not (same(ya.cpu(), mx) and same(yb.cpu(), exact) and comm.ar_mxfp8_stats() == before + 1)))
    bad.extend(["threshold 0"] * (comm.set_ar_mxfp8_threshold(0) != 0))  # off again: native bits, counter unmoved
    step("bf16 native", 9, nccl.ncclSum, native_bf16, 0)
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
