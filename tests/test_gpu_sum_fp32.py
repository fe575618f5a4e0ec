"""fp32-accumulated f16 / bf16 / fp8 sums: vcclReduceCopyWide, and the staged direct all-reduce / reduce-scatter
under VCCL_SUM_FP32=1 (tests/mp_sum_fp32_worker.py, one process per rank).  Inputs are k / 4 for small integers k:
the binary32 sum of up to 8 of them (premultiplied by 1 / 4 or not) is exact in any order, so the expected output
is that sum cast once to the type, bit for bit.  A fold that rounds at every step gives other bits — asserted on
the CPU wherever the two can differ: three or more inputs (two are one rounding either way), 4099 elements."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.mp_sum_fp32_worker import TYPES, expected, native_fold, values  # noqa: E402
from tests.test_gpu_ll_rooted import GEOM  # noqa: E402
from vccl_amd import nccl  # noqa: E402

SENTINEL, N_MAX = 0x5a, 4099
ENGINE_INPUTS = {dt: [values(dt, 100 * dt + s, N_MAX) for s in range(8)] for dt in TYPES}


def differ(dt, xs):
    return not torch.equal(native_fold(dt, xs).view(torch.uint8), expected(dt, xs).view(torch.uint8))


@pytest.mark.parametrize("shift", ["aligned", "srcs", "srcs_dsts"])
@pytest.mark.parametrize("n_elts", [1, N_MAX])
@pytest.mark.parametrize("n_srcs,n_dsts", [(2, 1), (3, 1), (8, 1), (8, 2)])
@pytest.mark.parametrize("op", [nccl.vcclDevSum, nccl.vcclDevPreMulSum])
@pytest.mark.parametrize("dt", sorted(TYPES))
def test_reduce_copy_wide(dt, op, n_srcs, n_dsts, n_elts, shift):
    """PreMulSum scales all sources but the last by 1 / 4; the bytes around every destination stay untouched."""
    t, esz = TYPES[dt][0], TYPES[dt][0].itemsize
    pre = n_srcs - 1 if op == nccl.vcclDevPreMulSum else 0
    raw = [x[:n_elts] for x in ENGINE_INPUTS[dt][:n_srcs]]
    xs = [x * (0.25 if s < pre else 1.0) for s, x in enumerate(raw)]
    exp = expected(dt, xs)
    assert n_srcs < 3 or n_elts < N_MAX or differ(dt, xs)
    so, do = int(shift != "aligned"), int(shift == "srcs_dsts")
    srcs = [torch.cat([torch.zeros(so), x]).to(t).cuda() for x in raw]
    dsts = [torch.full(((n_elts + do + 1) * esz,), SENTINEL, dtype=torch.uint8).cuda() for _ in range(n_dsts)]
    quarter = int.from_bytes(bytes(torch.tensor([0.25]).to(t).view(torch.uint8).tolist()), "little")
    nccl.reduce_copy_wide(op, dt, quarter, [b[so:].data_ptr() for b in srcs], [d[do * esz:].data_ptr() for d in dsts],
                          n_elts, torch.cuda.current_stream().cuda_stream, pre_op_srcs=pre)
    torch.cuda.synchronize()
    for d in dsts:
        got = d.cpu()
        assert torch.equal(got[do * esz:(do + n_elts) * esz], exp.view(torch.uint8))
        assert bool((got[:do * esz] == SENTINEL).all()) and bool((got[(do + n_elts) * esz:] == SENTINEL).all())


@pytest.mark.parametrize("op,dt", [(nccl.vcclDevSum, nccl.ncclFloat32), (nccl.vcclDevProd, nccl.ncclBfloat16)])
def test_reduce_copy_wide_refuses(op, dt):
    """Only Sum / PreMulSum over f16, bf16, e4m3 and e5m2 have a wide kernel."""
    p = (ctypes.c_void_p * 1)(torch.zeros(64, device="cuda").data_ptr())  # source and destination
    assert nccl.lib().vcclReduceCopyWide(op, dt, 0, 0, 1, p, 1, p, 8, None) == nccl.ncclInvalidArgument


def run_case(n, case, extra):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = {k: v for k, v in os.environ.items() if k not in ("VCCL_SUM_FP32", "NCCL_PROTO", "NCCL_ALGO")}
    env.update(GEOM, VCCL_SPIN_TIMEOUT_S="20", VCCL_NET_FORCE="0", **extra)
    with tempfile.TemporaryDirectory() as d:
        worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_sum_fp32_worker.py")
        procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case, d], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
        outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
        assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)
        return [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(n)]


@pytest.mark.parametrize("n", [3, 4, 8])
def test_collectives(n):
    """The worker's case_colls; n = 4 also: an f32 sum and a bf16 max all-reduce equal those of a comm created
    without the variable, on which the bf16 sum is the native fold, as it always was."""
    for dt in (9, 10) + ((6, 11) if n == 4 else ()):
        assert differ(dt, [values(dt, 1000 * N_MAX + 17 * dt + r, N_MAX) for r in range(n)]), (n, dt)
    on = run_case(n, "colls", {"VCCL_SUM_FP32": "1"})
    off = run_case(n, "plain", {}) if n == 4 else []
    # unset, 8 KiB takes the one-hop LL path, whose identity chain folds x_0 + (x_1 + (x_2 + x_3))
    xs = [values(9, 30 + r, N_MAX) for r in reversed(range(n))]
    assert differ(9, xs)
    for r in range(len(off)):
        assert str(off[r]["bf16_sum_algo"]) == "ll" and str(on[r]["bf16_sum_algo"]) == "direct"
        assert str(on[r]["f32_sum_algo"]) == str(off[r]["f32_sum_algo"])
        assert all(np.array_equal(on[r][k], off[r][k]) for k in ("f32_sum", "bf16_max"))
        assert np.array_equal(off[r]["bf16_sum"], native_fold(9, xs).view(torch.uint8).numpy())
        assert np.array_equal(on[r]["bf16_sum"], expected(9, xs).view(torch.uint8).numpy())


@pytest.mark.parametrize("n", [3, 4, 8])
def test_three_chunks(n):
    """bf16 and e4m3 sums that move through the inbox in three chunks (the all-reduce's third reuses parity 0)."""
    run_case(n, "chunks", {"VCCL_SUM_FP32": "1", "VCCL_DIRECT_CHUNK_BYTES": "65536"})
