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


def run_case(n, case, extra=REG, single=False, outdir=None):
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
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case] + ([outdir] if outdir else []), env=env,
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


@pytest.mark.parametrize("n", [2, 3, 4])
def test_payload_fold_order(n):
    """Order-sensitive payloads (tests/_payloads.py hard_input: specials
    between finite values of 21 binades) through f32 / bf16 sum, bf16 avg and
    f32 prod all-reduces and f32 / bf16 sum reduce-scatters, registered and
    unregistered: the worker holds the two bit-identical and counts the
    zero-copy and fallback outcomes; here both are held bit-exact to the ring's
    owner-map fold on GEOM's 14 channels, 256 KiB slots and 512 threads — the
    order the zero-copy kernels' header comments promise."""
    import tempfile

    import numpy as np

    from tests import _payloads as P
    from tests import _ring
    from tests._util import assert_bitexact
    from tests.mp_direct_reg_worker import AR, PAYLOAD_SEED, PAYLOAD_SPECS
    with tempfile.TemporaryDirectory() as d:
        run_case(n, "payload", outdir=d)
        res = [np.load(os.path.join(d, f"rank{r}.npz")) for r in range(n)]
        for i, (coll, dt, op, count, _, _) in enumerate(PAYLOAD_SPECS):
            total = count * (1 if coll == AR else n)
            ins = [P.hard_input(dt, op, total, r, n, PAYLOAD_SEED) for r in range(n)]
            if coll == AR:
                exp = [_ring.expected_allreduce(op, dt, ins, 14, 256 << 10, nthreads=512)] * n
            else:
                exp = _ring.expected_reducescatter(op, dt, ins, 14, 256 << 10, nthreads=512)
            for r in range(n):
                P.assert_cap(dt, exp[r], f"spec {i} n={n} rank {r}")
                for key in ("zc", "fb"):
                    got = res[r][f"{key}{i}"].view(ins[0].dtype)
                    assert_bitexact(dt, got, exp[r], what=f"{key} spec {i} {PAYLOAD_SPECS[i]} n={n} rank {r}")
