"""The direct reduce-scatter and all-gather in the MXFP8 wire format (VCCL_RSAG_MXFP8_THRESHOLD, DESIGN.md section
4.20), one process per rank (tests/mp_rsag_mxfp8_worker.py), bit for bit against the CPU model of the contract, the
reduce-scatter also against the exact float64 sum within a derived bound.  The inbox is GEOM's with 64 KiB chunks,
as test_gpu_ar_mxfp8.py shrinks it, so the three-chunk count stays small."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.test_gpu_ll_rooted import GEOM  # noqa: E402
from vccl_amd import nccl  # noqa: E402


def run_case(n, case, extra):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    drop = ("VCCL_RSAG_MXFP8_THRESHOLD", "VCCL_AR_MXFP8_THRESHOLD", "VCCL_SUM_FP32", "VCCL_REG_THRESHOLD",
            "NCCL_PROTO", "NCCL_ALGO")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(GEOM, VCCL_SPIN_TIMEOUT_S="20", VCCL_NET_FORCE="0", VCCL_DIRECT_CHUNK_BYTES="65536",
               VCCL_RSAG_MXFP8_THRESHOLD="1", **extra)
    with tempfile.TemporaryDirectory() as d:
        worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_rsag_mxfp8_worker.py")
        procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case, d], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
        outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
        assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_reducescatter_allgather(n):
    """The worker's case_cases: {bf16, f16} x {reduce-scatter, all-gather} x {1, 33, 513, 4099, three chunks} per
    rank x {out of place, in place, one element past alignment}: the model's bits on every rank, every byte around
    the output intact, the call's own counter moved by one; the reduce-scatter's model within
    sum_r amax_r(block) / 14 + half an ulp of the type + n 2^-23 sum_r amax_r(block) of the exact float64 sum."""
    run_case(n, "cases", {})


def test_same_comm():
    """n = 4, the worker's case_mixed: native and MXFP8 kernels alternate on one inbox with VCCL_SUM_FP32 and the
    all-reduce's switch on as well; avg / max, f32 and byte calls stay native; a mixed group; the switch off."""
    run_case(4, "mixed", {"VCCL_LL_THRESHOLD": "4096", "VCCL_LL_RSAG_THRESHOLD": "4096", "VCCL_SUM_FP32": "1",
                          "VCCL_AR_MXFP8_THRESHOLD": "1"})


def test_one_rank_comm_stays_off():
    comm = nccl.Comm.init_rank(1, nccl.get_unique_id(), 0)
    assert comm.set_rsag_mxfp8_threshold(1) == 0 and comm.rsag_mxfp8_stats() == (0, 0)
    with pytest.raises(nccl.VcclError):
        comm.set_rsag_mxfp8_threshold(-1)
    comm.destroy()
