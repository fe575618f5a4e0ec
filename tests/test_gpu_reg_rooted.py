"""Zero-copy ncclBroadcast / ncclBcast / ncclReduce over ncclCommRegister'ed
buffers on MI355X (tests/mp_reg_rooted_worker.py: one process per rank, ranks
sharing the GPU where the box has fewer GPUs than ranks).  The path is opt-in:
the tests set VCCL_REG_ROOTED_THRESHOLD=32768 on top of the shared-GPU geometry
of the rooted tests, so the oracle's partition matches.  Every case ends by
checking vcclCommRegRootedStats on every rank and that vcclCommRegStats did not
move.  Spins are bounded (VCCL_SPIN_TIMEOUT_S), so a protocol bug fails a test
instead of hanging the GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import _ring
from tests import ring_cases as RC
from tests._util import assert_bitexact, assert_fold_tolerance, exact_f64

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.test_gpu_ll_rooted import GEOM, NCH, SLOT  # noqa: E402
from vccl_amd import nccl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = {"VCCL_REG_ROOTED_THRESHOLD": "32768"}
CLEARED = ("REG_THRESHOLD", "DIRECT_A2A_THRESHOLD", "LL_A2A_THRESHOLD", "LL_ROOTED_THRESHOLD",
           "DIRECT_ROOTED_THRESHOLD", "FENCES", "REG_ROOTED_THRESHOLD")


def run_case(n, case, extra=REG, single=False):
    """The rank processes of `case`; returns what each saved."""
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
    worker = os.path.join(ROOT, "tests", "mp_reg_rooted_worker.py")
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([sys.executable, worker, str(r), str(n), hexid, case, d], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(1 if single else n)]
        outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
        assert [p.returncode for p in procs] == [0] * len(procs), "\n".join(outs)
        return [] if single else [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(n)]


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_broadcast(n):
    """32 767 bytes (ineligible: no launch counted), 32 768, 32 769, 32 768 +
    16 (n-1) +- 1, 65 541 and 1 MiB + 3; every root for n <= 4, roots 0, 3 and 7
    at n = 8; ncclBroadcast out of place with the non-roots' sendbuff NULL and
    ncclBcast in place; user pointers 0, 4 and 3 bytes past the registered base,
    differing between root and non-roots.  Every byte exact, the 64 bytes before
    and after each output intact, the root's input untouched, every eligible
    call counted as zero-copy."""
    run_case(n, "bcast")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_reduce(n):
    """Every RC.REDUCE_CASES row at every root for n <= 4, roots 0 and n - 1 at
    n = 8, on registered inputs and on unregistered copies (the same kernel's
    fallback, the staged path): rows of at least 32 768 bytes count as zero-copy
    / fallback, the rest as no launch; the two results are bit-identical (checked
    by the worker), and bit-exact against the oracle's fold on the call's SIMPLE
    partition; fp sum / prod also within the fold tolerance of the exact value.
    Every input and every non-root recvbuff stays untouched (the worker), the 16
    MiB i64 row (16 chunks) and the in-place row included."""
    res = run_case(n, "reduce")
    for ri, (name, op, dt, count, _) in enumerate(RC.REDUCE_CASES):
        ins = [RC.gen_reduce_input(ri, r) for r in range(n)]
        for root in (range(n) if n <= 4 else (0, n - 1)):
            exp = _ring.expected_reduce(op, dt, ins, root, NCH, SLOT, proto=_ring.S.PROTO_SIMPLE)
            got = res[root][f"{name}_r{root}"].view(ins[0].dtype)
            assert_bitexact(dt, got, exp, minmax=op in (2, 3), what=f"reduce {name} n={n} root {root}")
            if op in RC.TOLERANCE_OPS and dt in (6, 7, 8, 9):
                assert_fold_tolerance(dt, op, got, exact_f64(dt, op, ins), ins, exp_is_exact=True,
                                      what=f"reduce {name} n={n} root {root} vs exact")


def test_mixed_registration():
    """n = 4: the root's sendbuff unregistered; one non-root's recvbuff
    unregistered; one rank's reduce input 16 bytes past the end of its
    registration — fallback counted on all four ranks, exact; after that rank
    registers and a warm-up, zero-copy on all.  n = 2: a broadcast with only the
    root registered is zero-copy (nobody reads the non-root's recvbuff)."""
    run_case(4, "mixed")
    run_case(2, "mixed2")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """48 calls with no host synchronisation on a 128 KiB inbox, roots
    rotating: zero-copy broadcast, zero-copy reduce of 1 and 3 chunks, their
    fallbacks, a zero-copy all-reduce, the staged direct broadcast and reduce,
    an LL all-reduce; one synchronise, every output checked."""
    run_case(n, "b2b", extra=dict(REG, VCCL_REG_THRESHOLD="32768", VCCL_DIRECT_ROOTED_THRESHOLD=str(8 << 20),
                                  VCCL_DIRECT_CHUNK_BYTES="131072"))


def test_capture_replay():
    """n = 2: [broadcast root 0, reduce root 1, broadcast root 1] captured after
    an eager warm-up that imported the buffers, replayed three times with fresh
    inputs; the counters advance by 3 per replay."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the direct epoch seeded at 0xfffffffd, two broadcasts and two reduces across the wrap."""
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
    NCCL_ALGO: the new stats all zero, the calls take today's path with exact
    results, and without a registry *handle == buff and
    vcclCommSetRegRootedThreshold stays at 0.  `unset` runs twice: with no
    registration variable at all, and with VCCL_REG_THRESHOLD alone — there a
    registry exists (ncclCommRegister hands out its own handles, as before), and
    rooted calls still move no counter."""
    run_case(2, "off", extra=extra)
    if not extra:
        run_case(2, "off", extra={"VCCL_REG_THRESHOLD": "32768"})
