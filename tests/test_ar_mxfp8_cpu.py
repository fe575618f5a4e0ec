"""The MXFP8 wire format's contract on the CPU (tests/mp_ar_mxfp8_worker.py holds the model): the format is sane, and
the entry points refuse what they must.  Bounds are derived: half an E4M3 ulp is |x| * 2^-4; a scaled value below the
E4M3 normals rounds to a multiple of 2^-9 * 2^e, half of which is 2^-10 * 2^e <= amax_block * 2^-17 (2^e <= amax /
224: amax * 2^-e > 224 by the choice of e)."""
import ctypes

import pytest
import torch

from tests.mp_ar_mxfp8_worker import encode, inputs, model_allreduce, roundtrip, small_ints, wire
from vccl_amd import nccl

N = 4099


def bound(x):  # per element: max(|x| * 2^-4, amax of its block * 2^-17)
    n = (x.numel() + 31) // 32 * 32
    v = torch.zeros(n, dtype=torch.float64)
    v[:x.numel()] = x.double().abs()
    amax = v.view(-1, 32).amax(1, keepdim=True).expand(-1, 32).reshape(-1)
    return torch.maximum(v * 2.0 ** -4, amax * 2.0 ** -17)[:x.numel()]


def test_roundtrip_bound():
    x = inputs(1, N)
    y = roundtrip(x)
    assert bool(((y.double() - x.double()).abs() <= bound(x)).all())
    assert bool((y[32:64] == 0).all()) and bool((y[512:1024] == 0).all())
    p, s = encode(x)
    assert int(s[1]) == 127 and bool((s[16:32] == 127).all()) and wire(x).numel() == (N + 511) // 512 * 528


@pytest.mark.parametrize("t,half_ulp", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_allreduce_bound(t, half_ulp):
    """n = 8: the n + 1 passes' bounds, the binary32 adds' roundings and the final narrowing's half ulp."""
    xs = [inputs(10 + r, N) for r in range(8)]
    ys = [roundtrip(x) for x in xs]
    acc = ys[0]
    for y in ys[1:]:
        acc = acc + y
    tol = sum(bound(x) for x in xs) + bound(acc) + 7 * 2.0 ** -24 * sum(y.double().abs() for y in ys)
    out = model_allreduce(xs, t)
    tol = tol + out.double().abs() * half_ulp
    assert bool(((out.double() - sum(x.double() for x in xs)).abs() <= tol).all())


def test_differs_from_native():
    """What the GPU tests expect is not what the native fold gives, for both families of inputs they use."""
    for xs in ([inputs(7919 * N + 31 * 9 + r, N) for r in range(2)], [small_ints(100 + r, N) for r in range(4)]):
        native = torch.stack(xs).sum(0).to(torch.bfloat16)
        assert not torch.equal(model_allreduce(xs, torch.bfloat16).view(torch.int16), native.view(torch.int16))


def test_refusals():
    L = nccl.lib()
    eff, n = ctypes.c_int64(-1), ctypes.c_uint64(0)
    assert L.vcclCommSetArMxfp8Threshold(None, 1, ctypes.byref(eff)) == nccl.ncclInvalidArgument
    assert L.vcclCommArMxfp8Stats(None, ctypes.byref(n)) == nccl.ncclInvalidArgument
    buf = (ctypes.c_char * 1056)()
    p = ctypes.addressof(buf)
    assert L.vcclMxfp8Pack(p, nccl.ncclFloat64, 8, p, None) == nccl.ncclInvalidArgument
    assert L.vcclMxfp8Unpack(p, nccl.ncclFloat8e4m3, 8, p, None) == nccl.ncclInvalidArgument
    assert L.vcclMxfp8Pack(p, nccl.ncclFloat16, 8, (p + 15) // 16 * 16 + 8, None) == nccl.ncclInvalidArgument
