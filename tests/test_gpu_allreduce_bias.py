"""ncclAllReduceWithBias (tests/mp_allreduce_bias_worker.py, one process per rank).  Inputs and bias are k / 4 for small
integers k, every partial result exact in the type: the expectation, op over inputs and bias in float64 cast once, is
compared bit for bit.  Every case: the worker's table, a NULL bias; LL: the refusals; Direct: three chunks, a group."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.mp_allreduce_bias_worker import BF16, E4M3, ROWS, run_rows  # noqa: E402
from tests.mp_sum_fp32_worker import expected, native_fold  # noqa: E402
from tests.test_gpu_ll_rooted import GEOM  # noqa: E402
from vccl_amd import nccl  # noqa: E402

PATHS = {"ll": {}, "direct": {"NCCL_ALGO": "Direct", "VCCL_DIRECT_CHUNK_BYTES": "65536"}, "ring": {"NCCL_ALGO": "Ring"},
         "ll128": {"NCCL_PROTO": "LL128"}, "ll2": {"VCCL_SUM_FP32": "2"}, "direct1": {"VCCL_SUM_FP32": "1"}}


def run_case(n, case):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = {k: v for k, v in os.environ.items() if k not in ("VCCL_SUM_FP32", "NCCL_PROTO", "NCCL_ALGO")}
    env.update(GEOM, VCCL_SPIN_TIMEOUT_S="20", VCCL_NET_FORCE="0", **PATHS[case.partition("+")[0]])
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_allreduce_bias_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("path", ["ll", "direct", "ring", "ll128"])  # GEOM sends counts this small to LL
@pytest.mark.parametrize("n", [2, 4])
def test_paths(n, path):
    run_case(n, path)


def test_one_rank():
    comm = nccl.Comm.init_rank(1, nccl.get_unique_id(), 0)
    assert run_rows(comm, 0, 1, torch.cuda.current_stream().cuda_stream, ROWS) == []
    comm.destroy()


@pytest.mark.parametrize("path", ["ll", "direct", "ll2", "direct1"])
def test_bias_enters_the_fold(path):
    """2 ranks, inputs big and 1, bias 1.  bf16 256 + 1 and e4m3 16 + 1 are ties that round to even, back to 256 and
    16 (e4m3 keeps 4 significant bits: 17 lies between 16 = 1.000b x 2^4 and 18 = 1.001b x 2^4), so the native fold
    stays at big twice; 258 and 18 are exact: under VCCL_SUM_FP32 the fused bias gives big + 2, an appended one big."""
    for dt, big in ((BF16, 256.0), (E4M3, 16.0)):
        xs = [torch.tensor([v]) for v in (big, 1.0, 1.0)]
        code = {BF16: 9, E4M3: 10}[dt]
        assert native_fold(code, xs).float().item() == big and expected(code, xs).float().item() == big + 2
    run_case(2, path + "+order")
