"""The LL protocol for small ncclSend / ncclRecv on MI355X (tests/mp_p2p_ll_worker.py: one
process per rank, ranks sharing the GPU).  The geometry of test_gpu_p2p.py plus an LL threshold of 4096 bytes and
LL slots of 1 KiB of data: a 4096-byte message is four steps, two of them wrap the FIFO.  Spins are bounded
(VCCL_SPIN_TIMEOUT_S), so a protocol bug fails instead of hanging."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.test_gpu_p2p import GEOM, P2P_KNOBS  # noqa: E402
from vccl_amd import nccl  # noqa: E402

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_p2p_ll_worker.py")
LL = {"VCCL_P2P_LL_THRESHOLD": "4096", "VCCL_P2P_LL_STEP_BYTES": "1024"}


@pytest.mark.parametrize("n,case,extra", [
    (2, "sizes", LL),     # 1: sizes 0 .. 4097 x source offsets {0, 1, 3} x destination offsets {0, 2, 5}; guards; the LL / FIFO split
    (2, "counters", LL),  # 2: 40 ungrouped Send / Recv, 8 B and 4096 B alternating: persistent steps, stale lines
    (4, "mixed", LL),     # 3: three messages to one peer across the threshold; an all-to-allv with LL, FIFO and empty pairs
    (2, "wrap", LL),      # 4: case 2's sequence from step 0x7ffffff0 and from 0xfffffff0
    (2, "capture", LL),   # 5: a captured 2 KiB exchange replayed 3 times, eager LL exchanges around it
    (2, "once", {}),      # 6: threshold unset: the size list once, no LL message, exact results
    (2, "once", {**LL, "VCCL_FENCES": "1"}),  # 7: the size list once with fences
])
def test_ll(n, case, extra):
    uid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = dict(os.environ)
    for k in P2P_KNOBS + tuple(k[5:] for k in LL):
        env.pop("VCCL_" + k, None)
        env.pop("NCCL_" + k, None)
    env.update({**GEOM, "VCCL_SPIN_TIMEOUT_S": "20", **extra})
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(n), uid, case], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)
