"""One-hop LL path of ncclAllToAll / ncclAllToAllv on MI355X
(tests/mp_ll_a2a_worker.py: one process per rank, ranks sharing the GPU where
the box has fewer GPUs than ranks).  The path is opt-in: the tests set
VCCL_LL_A2A_THRESHOLD to 64 KiB per pair on top of the shared-GPU geometry of
the LL tests (a 1 MiB slot) and of the p2p tests (a 16 KiB step, 2 parts per
peer, so a 300 KB pair wraps a part's FIFO twice).  Every case ends by checking
vcclCommA2aStats against what vcclLLA2aPlan predicts.  Spins are bounded
(VCCL_SPIN_TIMEOUT_S), so a protocol bug fails a test instead of hanging the
GPU."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from vccl_amd import nccl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_gpu_ll_rooted.py GEOM and tests/test_gpu_p2p.py GEOM, united
GEOM = {"VCCL_NCHANNELS": "14", "VCCL_NTHREADS": "512", "VCCL_SLOT_BYTES": str(256 << 10),
        "VCCL_ALLOW_SHARED_DEVICE": "1", "VCCL_LL_THRESHOLD": str(1 << 20),
        "VCCL_LL_MAX_BLOCKS": "32", "VCCL_DIRECT_THRESHOLD": str(4 << 20),
        "VCCL_DIRECT_MAX_BLOCKS": "16", "VCCL_DIRECT_CHUNK_BYTES": str(1 << 20),
        "VCCL_DIRECT_RSAG_THRESHOLD": str(64 << 20), "VCCL_RING_WAVE": "1", "VCCL_RING_WAVE_MIN": "0",
        "VCCL_P2P_NVL_CHUNKSIZE": "16384", "VCCL_P2P_PARTS": "2", "VCCL_P2P_MIN_PART_BYTES": "4096"}
A2A = {"VCCL_LL_A2A_THRESHOLD": "65536"}
CLEARED = ("LL_A2A_THRESHOLD", "LL_ROOTED_THRESHOLD", "P2P_NVL_CHUNKSIZE", "P2P_PARTS", "P2P_MIN_PART_BYTES",
           "P2P_BUFFERS", "FENCES")


def run_case(n, case, extra=A2A):
    uid = nccl.get_unique_id()
    hexid = nccl.unique_id_to_bytes(uid).hex()
    env = dict(os.environ)
    for k in CLEARED:
        env.pop("VCCL_" + k, None)
        env.pop("NCCL_" + k, None)
    for k in ("NCCL_PROTO", "NCCL_ALGO", "VCCL_NET_FORCE"):
        env.pop(k, None)
    env.setdefault("VCCL_SPIN_TIMEOUT_S", "20")
    env.update(GEOM)
    env.update(extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_ll_a2a_worker.py"),
                               str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_uniform(n):
    """ncclAllToAll of 1, 7, 8, 9, 4099 and 65536 bytes per pair (u8) and 1000
    f32, source / destination 0, 1 and 3 bytes past a 16-byte boundary: every
    byte exact, the 64 bytes before and after the output intact, one LL launch
    per call and no FIFO pair; a final 65537-byte row takes the FIFO path with
    no LL launch."""
    run_case(n, "uniform")


@pytest.mark.parametrize("n", [3, 4, 8])
def test_v_mixed(n):
    """bf16 ncclAllToAllv from a seeded matrix with zero counts, rank 1's row
    empty, pairs of 65536 and 65538 bytes, a 300 KB pair and a self block above
    the limit, gaps in the displacements, twice: exact output, gap bytes
    intact, llPairs / fifoPairs as planned on every rank."""
    run_case(n, "v_mixed")


def test_group_mixed():
    """n = 4, one group: a plain send to r+1, an ncclAllToAllv with LL and FIFO
    pairs, a plain recv from r-1 and a 4 MiB all-reduce; all outputs exact."""
    run_case(4, "group_mixed")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """No host synchronisation between calls: 64 LL all-to-alls into 64
    outputs, then 48 calls cycling LL all-to-all, LL all-reduce, rooted LL
    broadcast, FIFO all-to-all and mixed all-to-allv; one synchronise, every
    output checked."""
    run_case(n, "b2b", extra=dict(A2A, VCCL_LL_ROOTED_THRESHOLD=str(1 << 20)))


def test_capture_replay():
    """n = 2: [all-to-all, mixed all-to-allv, all-to-all] captured on one
    stream, replayed three times with fresh inputs."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the LL epoch seeded at 0xfffffffe, then four all-to-alls across
    the wrap."""
    run_case(2, "wrap")


@pytest.mark.parametrize("extra", [{}, dict(A2A, VCCL_NET_FORCE="1"), dict(A2A, NCCL_PROTO="^LL")],
                         ids=["unset", "net", "no_ll"])
def test_off_switches(extra):
    """Threshold unset, or set with a net peer or with LL excluded by
    NCCL_PROTO: zero LL launches, results exact (a comm with a net peer refuses
    point-to-point as it always did); vcclCommSetA2aThreshold turns the path on
    and off again on the unset comm, clamped to the slot, the counters
    following, and stays at 0 on the other two."""
    run_case(2, "off", extra=extra)
