"""One-hop direct path of ncclAllToAll / ncclAllToAllv on MI355X
(tests/mp_direct_a2a_worker.py: one process per rank, ranks sharing the GPU
where the box has fewer GPUs than ranks).  The path is opt-in: the tests set
VCCL_DIRECT_A2A_THRESHOLD to 96 KiB per pair on top of the shared-GPU geometry
of the LL all-to-all tests (a 1 MiB inbox chunk, at most 16 direct blocks, a
16 KiB p2p step with 2 parts per peer, so a 300 KB pair wraps a part's FIFO
twice).  Every case ends by checking vcclCommA2aStatsEx against what
vcclDirectA2aPlan predicts.  Spins are bounded (VCCL_SPIN_TIMEOUT_S), so a
protocol bug fails a test instead of hanging the GPU."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.test_gpu_ll_a2a import GEOM  # noqa: E402
from vccl_amd import nccl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A2A = {"VCCL_DIRECT_A2A_THRESHOLD": "98304"}
CLEARED = ("DIRECT_A2A_THRESHOLD", "LL_A2A_THRESHOLD", "LL_ROOTED_THRESHOLD", "DIRECT_ROOTED_THRESHOLD",
           "P2P_NVL_CHUNKSIZE", "P2P_PARTS", "P2P_MIN_PART_BYTES", "P2P_BUFFERS", "FENCES")


def run_case(n, case, extra=A2A):
    uid = nccl.get_unique_id()
    hexid = nccl.unique_id_to_bytes(uid).hex()
    env = dict(os.environ)
    for k in CLEARED:
        env.pop("VCCL_" + k, None)
        env.pop("NCCL_" + k, None)
    for k in ("NCCL_PROTO", "NCCL_ALGO", "VCCL_NET_FORCE"):
        env.pop(k, None)
    env.update(GEOM)
    env["VCCL_SPIN_TIMEOUT_S"] = "20"
    env.update(extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_direct_a2a_worker.py"),
                               str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_uniform(n):
    """ncclAllToAll of 1, 15, 16, 17, 16384, 16385, 49153 (4 blocks of 12304,
    the last one 12241) and 98304 bytes (6 blocks) per pair (u8) and 3000 f32,
    source / destination 0, 1 and 3 bytes past a 16-byte boundary: every byte
    exact, the 64 bytes before and after the output intact, one direct launch
    per call and no LL or FIFO pair; a final 98305-byte row takes the FIFO path
    with no direct launch."""
    run_case(n, "uniform")


@pytest.mark.parametrize("n", [3, 4, 8])
def test_v_mixed(n):
    """bf16 ncclAllToAllv from a seeded matrix with zero counts, rank 1's row
    empty, pairs of 16382 / 16386 / 98304 / 98306 bytes, a 300 KB pair and a
    self block above the limit, gaps in the displacements, twice: exact output,
    gap bytes intact, direct / FIFO pairs as planned on every rank."""
    run_case(n, "v_mixed")


@pytest.mark.parametrize("n", [3, 4, 8])
def test_v_three_way(n):
    """The same with VCCL_LL_A2A_THRESHOLD=4096: one call splits three ways —
    an LL launch, a direct launch, the FIFO launch."""
    run_case(n, "v_mixed", extra=dict(A2A, VCCL_LL_A2A_THRESHOLD="4096"))


def test_clamp():
    """n = 8, the threshold at 1 MiB: the effective limit is the region
    capacity (131312 bytes in the test geometry); a pair exactly at it is
    exact, a pair 2 bytes over goes to the FIFOs."""
    run_case(8, "clamp", extra={"VCCL_DIRECT_A2A_THRESHOLD": str(1 << 20)})


def test_group_mixed():
    """n = 4, one group: a plain send to r+1, an ncclAllToAllv with direct and
    FIFO pairs, a plain recv from r-1 and a 4 MiB all-reduce; all outputs exact."""
    run_case(4, "group_mixed")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """No host synchronisation between calls: 48 calls cycling the direct
    all-to-all, the direct all-reduce, reduce-scatter and all-gather, the rooted
    direct broadcast and reduce, a FIFO all-to-all and a mixed all-to-allv; one
    synchronise, every output checked."""
    run_case(n, "b2b", extra=dict(A2A, VCCL_DIRECT_ROOTED_THRESHOLD=str(8 << 20)))


def test_capture_replay():
    """n = 2: [all-to-all, mixed all-to-allv, all-to-all] captured on one
    stream, replayed three times with fresh inputs."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the direct epoch seeded at 0xfffffffe, then four all-to-alls
    across the wrap."""
    run_case(2, "wrap")


def test_fences():
    """n = 4 with VCCL_FENCES=1: the fenced branches of the flag hand-off."""
    run_case(4, "fences", extra=dict(A2A, VCCL_FENCES="1"))


@pytest.mark.parametrize("extra", [{}, dict(A2A, VCCL_NET_FORCE="1"), dict(A2A, NCCL_ALGO="^Direct")],
                         ids=["unset", "net", "no_direct"])
def test_off_switches(extra):
    """Threshold unset, or set with a net peer or with Direct excluded by
    NCCL_ALGO: zero direct launches, results exact (a comm with a net peer
    refuses point-to-point as it always did); vcclCommSetDirectA2aThreshold
    turns the path on and off again on the unset comm, clamped to the region,
    the counters following, and stays at 0 on the other two."""
    run_case(2, "off", extra=extra)
