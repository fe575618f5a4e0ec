"""Level 2 of the fp32-accumulated f16 / bf16 / fp8 sums (VCCL_SUM_FP32=2): the one-hop LL all-reduce and
reduce-scatter, the zero-copy kernels over registered buffers and ncclReduce (tests/mp_sum_fp32_l2_worker.py, one
process per rank).  Inputs are k / 4 for small integers k, as in tests/test_gpu_sum_fp32.py: their binary32 sum is
exact in any order, so every output is that sum cast once to the type, bit for bit.  A fold that rounds at every
step gives other bits — asserted here on the CPU for every 4099-element input set of three or more ranks."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.mp_sum_fp32_l2_worker import RS_COUNT, types_ops  # noqa: E402
from tests.mp_sum_fp32_worker import values  # noqa: E402
from tests.test_gpu_ll_rooted import GEOM  # noqa: E402
from tests.test_gpu_sum_fp32 import differ  # noqa: E402
from vccl_amd import nccl  # noqa: E402

CLEARED = ("VCCL_SUM_FP32", "NCCL_PROTO", "NCCL_ALGO", "VCCL_REG_THRESHOLD", "VCCL_REG_ROOTED_THRESHOLD")
# the zero-copy thresholds: the smallest power of two that leaves the worker's 256-byte warm-up all-reduce below it
REG = {"VCCL_REG_THRESHOLD": "512", "VCCL_REG_ROOTED_THRESHOLD": "512"}
CASES = {  # case: (worker case, environment on top of VCCL_SUM_FP32=2, [(seed, elements per rank / n)] of its inputs)
    # all-reduces of 1 and 4099 elements, a reduce-scatter of RS_COUNT per rank, in and out of place: `ll`, exact
    "ll": ("ll", {}, [(1000 * 4099, 4099), (1000 * RS_COUNT, -RS_COUNT)]),
    # ... and with the LL threshold switched off: `direct`, the same bytes
    "ll_off": ("ll", {"VCCL_LL_THRESHOLD": "0"}, []),
    # 4099 elements, all-reduce / reduce-scatter / reduce to root n - 1: zero-copy on registered buffers, the wide
    # staged fallback on unregistered ones, counted as such by vcclCommRegStats / vcclCommRegRootedStats
    "zero_copy": ("reg", REG, [(2000 * 4099, 4099), (2000 * 4099 + 5, -4099), (2000 * 4099 + 20, 4099)]),
    # ncclReduce to roots 0 and n - 1 of 1, 4099 and a three-chunk count: `direct`, exact, non-roots untouched
    "reduce": ("reduce", {"VCCL_DIRECT_CHUNK_BYTES": "65536"}, [(2000 * 4099 + 20, 4099)])}


def run_case(n, case, extra):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = {k: v for k, v in os.environ.items() if k not in CLEARED}
    env.update(GEOM, VCCL_SPIN_TIMEOUT_S="20", VCCL_NET_FORCE="0", **extra)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_sum_fp32_l2_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n", [3, 4, 8])
def test_level2(n, case):
    worker_case, extra, seeds = CASES[case]
    for seed, n_elts in seeds:  # a negative count: per rank of a reduce-scatter, n times as many in all
        for dt, _ in types_ops(n):
            assert differ(dt, [values(dt, seed + 17 * dt + r, abs(n_elts) * (n if n_elts < 0 else 1)) for r in range(n)])
    run_case(n, worker_case, dict(extra, VCCL_SUM_FP32="2"))


def test_levels():
    """The worker's case_levels, on a comm created without the variable."""
    assert differ(9, [values(9, 30 + r, 4099) for r in range(4)])
    run_case(4, "levels", {})
