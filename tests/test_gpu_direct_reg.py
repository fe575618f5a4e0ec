"""Zero-copy direct all-reduce / reduce-scatter / all-gather over
ncclCommRegister'ed buffers on MI355X (tests/mp_direct_reg_worker.py: one
process per rank, ranks sharing the GPU where the box has fewer GPUs than
ranks).  The path is opt-in: the tests set VCCL_REG_THRESHOLD=32768 on top of
the shared-GPU geometry of the all-to-all tests.  Every output is compared bit
for bit with the same call on unregistered copies (the same kernel's fallback,
the staged direct path), integer and integer-valued results with the exact
value too; the 64 bytes before and after each buffer stay intact; every case
ends by checking vcclCommRegStats on every rank.  Spins are bounded
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

from tests.test_gpu_ll_a2a import GEOM  # noqa: E402
from vccl_amd import nccl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = {"VCCL_REG_THRESHOLD": "32768"}
CLEARED = ("REG_THRESHOLD", "DIRECT_A2A_THRESHOLD", "LL_A2A_THRESHOLD", "LL_ROOTED_THRESHOLD",
           "DIRECT_ROOTED_THRESHOLD", "FENCES")


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
    worker = os.path.join(ROOT, "tests", "mp_direct_reg_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(1 if single else n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * len(procs), "\n".join(outs)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_allreduce(n):
    """f32 sum, bf16 avg, i32 max; 8191 (for the 4-byte types 4 bytes below
    the threshold: no eligible launch), 8192, 8193, 16391 and 1 048 579
    elements, bf16 also at twice those counts (the same bytes, so the same
    edge); out of place and in place; user pointers 0 and 4 bytes (bf16: 2)
    past the registered base.  Every eligible call zero-copy, bit-identical to
    the staged path."""
    run_case(n, "allreduce")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_reducescatter(n):
    """bf16 sum with recvcount 8195 (the peers' blocks sit at other
    alignments), f32 prod 4099, u8 sum 65 537; in place (recvbuff = sendbuff +
    rank * count) and out of place."""
    run_case(n, "reducescatter")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_allgather(n):
    """1 MiB + 1 byte and 16 385 bytes per rank, in place and out of place."""
    run_case(n, "allgather")


def test_mixed_registration():
    """n = 4: rank 1 unregistered, only its recvbuff unregistered, its call 16
    bytes past the end of its registration — fallback counted on all four
    ranks, exact; after rank 1 registers and a warm-up, zero-copy on all."""
    run_case(4, "mixed")


def test_reregister():
    """n = 2: deregister, register another allocation that lands in the same
    entries: zero-copy, exact; free the allocation after deregistering and call
    on a new one: exact; a bad handle is ncclInvalidArgument."""
    run_case(2, "reregister")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """48 calls with no host synchronisation cycling zero-copy AR / RS / AG,
    fallback calls, the staged direct AR / RS / AG, a rooted direct broadcast
    and an LL all-reduce; one synchronise, every output checked."""
    run_case(n, "b2b", extra=dict(REG, VCCL_DIRECT_ROOTED_THRESHOLD=str(8 << 20)))


def test_capture_replay():
    """n = 2: [AR, RS, AG] zero-copy captured, replayed three times with fresh inputs."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the direct epoch seeded at 0xfffffffd, four calls across the wrap."""
    run_case(2, "wrap")


def test_fences():
    """n = 4 with VCCL_FENCES=1: the fenced branches of the flag hand-off."""
    run_case(4, "fences", extra=dict(REG, VCCL_FENCES="1"))


def test_single_process():
    """n = 2 ncclCommInitAll ranks in one process: the peers' buffers are
    addressed by raw pointer, one collective per comm in each group."""
    run_case(2, "single", single=True)


@pytest.mark.parametrize("extra", [{}, dict(REG, VCCL_NET_FORCE="1"), dict(REG, NCCL_ALGO="^Direct")],
                         ids=["unset", "net", "no_direct"])
def test_off_switches(extra):
    """Threshold unset, or set with a net peer or with Direct excluded by
    NCCL_ALGO: *handle == buff, the stats all zero, the call takes today's
    path, and vcclCommSetRegThreshold stays at 0 (no registry to switch on)."""
    run_case(2, "off", extra=extra)
