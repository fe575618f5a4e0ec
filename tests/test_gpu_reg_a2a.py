"""Zero-copy ncclAllToAll / ncclAllToAllv over ncclCommRegister'ed send buffers
on MI355X (tests/mp_reg_a2a_worker.py: one process per rank, ranks sharing the
GPU where the box has fewer GPUs than ranks).  The path is opt-in: the tests set
VCCL_REG_A2A_THRESHOLD=32768 on top of the shared-GPU geometry of the
all-to-all tests.  Every output is compared byte for byte with the same call on
unregistered copies (the fallback through the per-peer FIFOs) and with the
value computed on the host; the 64 bytes before and after each buffer stay
intact; every case ends by checking vcclCommRegA2aStats on every rank.  Spins
are bounded (VCCL_SPIN_TIMEOUT_S), so a protocol bug fails a test instead of
hanging the GPU."""
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
REG = {"VCCL_REG_A2A_THRESHOLD": "32768"}
CLEARED = ("REG_THRESHOLD", "REG_A2A_THRESHOLD", "DIRECT_A2A_THRESHOLD", "LL_A2A_THRESHOLD", "LL_ROOTED_THRESHOLD",
           "DIRECT_ROOTED_THRESHOLD", "FENCES", "P2P_BUFFERS")


def run_case(n, case, extra=REG, single=False):
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = dict(os.environ)
    for k in CLEARED:
        env.pop("VCCL_" + k, None)
        env.pop("NCCL_" + k, None)
    for k in ("NCCL_PROTO", "NCCL_ALGO", "VCCL_NET_FORCE"):
        env.pop(k, None)
    env.update(GEOM)
    env["VCCL_SPIN_TIMEOUT_S"] = "20"
    env.update(extra)
    worker = os.path.join(ROOT, "tests", "mp_reg_a2a_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(1 if single else n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * len(procs), "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_uniform(n):
    """u8 at 32 767 bytes per pair (no eligible launch, today's path), 32 768,
    32 769 and 1 MiB + 3 (many slices; more than one FIFO's 8 x 16 KiB x 2
    parts on the fallback); bf16 at 16 383, 16 384 and 16 385 elements; the send
    and the receive pointer 0, 1 and 4 bytes past the registered base,
    independently."""
    run_case(n, "uniform")


def test_small_pairs():
    """n = 4, the threshold lowered to 16: 40 bytes per pair, uniform and as a
    v-call (whose grid leaves most workgroups an empty slice); 15 bytes: today's path."""
    run_case(4, "small")


@pytest.mark.parametrize("n", [3, 4, 8])
def test_v_calls(n):
    """Random counts with zero pairs, a zero row and a zero column, non-monotonic
    displacements with gaps, misaligned pointers: zero-copy.  One rank whose
    largest pair is below the threshold: fallback counted on all ranks."""
    run_case(n, "v")


def test_mixed_registration():
    """n = 4: rank 1 unregistered; rank 1 registered 16 bytes short of its last
    block — fallback on all four ranks, exact; every sendbuff registered and no
    recvbuff: zero-copy, twice."""
    run_case(4, "mixed")


def test_group():
    """n = 4: two eligible all-to-alls and a plain send / recv ring in one
    group, zero-copy and fallback; nine all-to-alls in one group, the ninth on
    today's path."""
    run_case(4, "group")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """40 calls with no host synchronisation cycling this path zero-copy, its
    fallback, a zero-copy all-reduce, an LL all-to-all, a direct all-to-all and
    plain send / recv; one synchronise, every output checked."""
    run_case(n, "b2b", extra=dict(REG, VCCL_REG_THRESHOLD="32768", VCCL_LL_A2A_THRESHOLD="4096",
                                  VCCL_DIRECT_A2A_THRESHOLD="16384"))


def test_capture_replay():
    """n = 2: [zero-copy, fallback] captured, replayed three times with fresh
    inputs; the counters grow per replay."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the direct epoch seeded at 0xfffffffd, four calls across the wrap."""
    run_case(2, "wrap")


def test_fences():
    """n = 4 with VCCL_FENCES=1: the fenced branches of the flag hand-off."""
    run_case(4, "fences", extra=dict(REG, VCCL_FENCES="1"))


def test_single_process():
    """n = 2 ncclCommInitAll ranks in one process: the peers' send buffers are
    addressed by raw pointer."""
    run_case(2, "single", single=True)


def test_reregister():
    """n = 2: deregister, then register another allocation into the same entry."""
    run_case(2, "reregister")


@pytest.mark.parametrize("extra", [{}, dict(REG, VCCL_NET_FORCE="1"), dict(REG, NCCL_ALGO="^Direct"),
                                   dict(REG, VCCL_P2P_BUFFERS="0")], ids=["unset", "net", "no_direct", "no_p2p"])
def test_off_switches(extra):
    """Threshold unset, or set with a net peer, with Direct excluded by
    NCCL_ALGO, or without point-to-point buffers: the stats all zero,
    vcclCommSetRegA2aThreshold stays at 0, and the call behaves as today."""
    run_case(2, "off", extra=extra)
