"""The SIMPLE ring of the fp32-accumulated f16 / bf16 / fp8 sums (VCCL_SUM_FP32_RING_THRESHOLD; device/ring_wide.hpp;
tests/mp_sum_fp32_ring_worker.py, one process per rank).  4 KiB slots: 1024 binary32 per slice.  Inputs of the exact
test are k / 4 for small integers k, as in tests/test_gpu_sum_fp32.py: their binary32 sum is exact in any order, so
every output is that sum cast once to the type, bit for bit, where a ring that rounds at every hop gives other bits —
asserted here on the CPU for the input sets of three or more ranks."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.mp_sum_fp32_ring_worker import AR, RS, multi_slice_count, types_ops  # noqa: E402
from tests.mp_sum_fp32_worker import values  # noqa: E402
from tests.test_gpu_ll_rooted import GEOM  # noqa: E402
from tests.test_gpu_sum_fp32 import differ  # noqa: E402
from vccl_amd import nccl  # noqa: E402

CLEARED = ("VCCL_SUM_FP32", "VCCL_SUM_FP32_RING_THRESHOLD", "NCCL_PROTO", "NCCL_ALGO", "VCCL_REG_THRESHOLD",
           "VCCL_SLICE_BYTES")
RING = {"VCCL_SUM_FP32": "1", "VCCL_SUM_FP32_RING_THRESHOLD": "1"}


def run_case(n, case, extra):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = {k: v for k, v in os.environ.items() if k not in CLEARED}
    env.update(GEOM, VCCL_SLOT_BYTES="4096", VCCL_LL_THRESHOLD="0", VCCL_SPIN_TIMEOUT_S="20", VCCL_NET_FORCE="0",
               **extra)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_sum_fp32_ring_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_exact(n):
    """All-reduce and reduce-scatter, in and out of place, of 1, 4099 and a multi-slice count: `ring`, exact.  n = 2
    adds f16 and e5m2 (no binary32 hop), n = 3 buffers one element past alignment, n = 4 ncclAvg (premultiplied)."""
    if n >= 3:
        for dt, _ in types_ops(n):
            for coll in (AR, RS):
                for count in (4099, multi_slice_count(coll, n, dt)):
                    total = count * (n if coll == RS else 1)
                    assert differ(dt, [values(dt, 1000 * count + 17 * dt + r, total) for r in range(n)])
    run_case(n, "exact", RING)


def test_order():
    """8 ranks, order-sensitive inputs: the wide ring's bits are the staged direct wide kernel's."""
    run_case(8, "order", RING)


def test_switch():
    """The worker's case_switch, on a comm created without the variables."""
    run_case(4, "switch", {})
