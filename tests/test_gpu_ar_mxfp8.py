"""The MXFP8 wire format on the GPU: vcclMxfp8Pack / vcclMxfp8Unpack on one device, and the direct all-reduce in the
format (VCCL_AR_MXFP8_THRESHOLD, one process per rank, tests/mp_ar_mxfp8_worker.py), bit for bit against the CPU
model of the contract in that module.  The inbox is GEOM's with 64 KiB chunks, as test_gpu_sum_fp32.py's chunk case
shrinks it, so the three-chunk count stays small."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.mp_ar_mxfp8_worker import SENTINEL, TYPES, decode, encode, inputs, wire  # noqa: E402
from tests.test_gpu_ll_rooted import GEOM  # noqa: E402
from vccl_amd import nccl  # noqa: E402


def pack_unpack(dt, x, off):
    """x through vcclMxfp8Pack and back; returns (wire bytes, unpacked values), sentinels checked."""
    t, count = TYPES[dt], x.numel()
    esz, nwire = t.itemsize, nccl.mxfp8_wire_bytes(count)
    sp = torch.cuda.current_stream().cuda_stream
    src = torch.zeros(count + off, dtype=t).cuda()
    src[off:] = x.to(t).cuda()
    w = torch.full((nwire + 64,), SENTINEL, dtype=torch.uint8).cuda()
    dst = torch.full(((count + off + 8) * esz,), SENTINEL, dtype=torch.uint8).cuda()
    nccl.mxfp8_pack(src[off:].data_ptr(), dt, count, w.data_ptr(), sp)
    nccl.mxfp8_unpack(w.data_ptr(), dt, count, dst[off * esz:].data_ptr(), sp)
    torch.cuda.synchronize()
    w, dst = w.cpu(), dst.cpu()
    assert bool((w[nwire:] == SENTINEL).all())
    assert bool((dst[:off * esz] == SENTINEL).all()) and bool((dst[(off + count) * esz:] == SENTINEL).all())
    return w[:nwire], dst[off * esz:(off + count) * esz]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("count", [1, 31, 32, 33, 511, 512, 513, 4099])
@pytest.mark.parametrize("dt", sorted(TYPES))
def test_pack_unpack(dt, count, off):
    x = inputs(count + dt, count)
    got_wire, got = pack_unpack(dt, x, off)
    assert torch.equal(got_wire, wire(x))
    assert torch.equal(got, decode(*encode(x))[:count].to(TYPES[dt]).view(torch.uint8))


def test_pack_special_blocks():
    """A NaN in block 1 and an infinity in block 3 of 128 elements: exactly those two blocks decode to NaN."""
    x = inputs(5, 128)
    x[40], x[100] = float("nan"), float("-inf")
    got_wire, got = pack_unpack(nccl.ncclFloat32, x, 0)
    assert torch.equal(got_wire, wire(x))
    y = got.view(torch.float32)
    assert torch.isnan(y).view(4, 32).all(1).tolist() == [False, True, False, True]
    assert torch.equal(y[:32], decode(*encode(x))[:32]) and torch.equal(y[64:96], decode(*encode(x))[64:96])


def run_case(n, case, extra):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    drop = ("VCCL_AR_MXFP8_THRESHOLD", "VCCL_SUM_FP32", "NCCL_PROTO", "NCCL_ALGO")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(GEOM, VCCL_SPIN_TIMEOUT_S="20", VCCL_NET_FORCE="0", VCCL_DIRECT_CHUNK_BYTES="65536",
               VCCL_AR_MXFP8_THRESHOLD="1", **extra)
    with tempfile.TemporaryDirectory() as d:
        worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_ar_mxfp8_worker.py")
        procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case, d], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
        outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
        assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_allreduce(n):
    """The worker's case_cases: {bf16, f16} x {1, 33, 513, 4099, three chunks} x {out of place, in place, one element
    past alignment}: the model's bits on every rank, sentinels intact, one more counted launch per call."""
    run_case(n, "cases", {})


def test_same_comm():
    """n = 4, the worker's case_mixed, with 16 KiB calls on the direct path and VCCL_SUM_FP32 on as well (the MXFP8
    op wins where both apply)."""
    run_case(4, "mixed", {"VCCL_LL_THRESHOLD": "4096", "VCCL_LL_RSAG_THRESHOLD": "4096", "VCCL_SUM_FP32": "1"})


def test_one_rank_comm_stays_off():
    comm = nccl.Comm.init_rank(1, nccl.get_unique_id(), 0)
    assert comm.set_ar_mxfp8_threshold(1) == 0 and comm.ar_mxfp8_stats() == 0
    with pytest.raises(nccl.VcclError):
        comm.set_ar_mxfp8_threshold(-1)
    comm.destroy()
