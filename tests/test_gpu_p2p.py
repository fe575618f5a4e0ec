"""ncclSend / ncclRecv / ncclAllToAll / ncclAllToAllv on MI355X
(tests/mp_p2p_worker.py: one process per rank, ranks sharing the GPU where
the box has fewer GPUs than ranks, as the broadcast test does).

Test geometry: a 16 KiB step, 2 parts per peer, a second part from 4 KiB —
one part's FIFO (8 slots) wraps at 128 KiB, so the sizes up to 300 KiB cross
every path: no part, one part, both parts, a step boundary, one and two wraps.
Spins are bounded (VCCL_SPIN_TIMEOUT_S) so a protocol bug fails the test
instead of hanging the GPU."""
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
# The shared-GPU geometry of the collective tests (every rank's workgroups
# co-resident on one device) plus the p2p test geometry.
GEOM = {"VCCL_NCHANNELS": "14", "VCCL_NTHREADS": "512", "VCCL_SLOT_BYTES": str(256 << 10),
        "VCCL_ALLOW_SHARED_DEVICE": "1", "VCCL_LL_THRESHOLD": str(1 << 20), "VCCL_LL_MAX_BLOCKS": "32",
        "VCCL_DIRECT_THRESHOLD": str(4 << 20), "VCCL_DIRECT_MAX_BLOCKS": "16",
        "VCCL_DIRECT_CHUNK_BYTES": str(1 << 20), "VCCL_DIRECT_RSAG_THRESHOLD": str(64 << 20),
        "VCCL_P2P_NVL_CHUNKSIZE": "16384", "VCCL_P2P_PARTS": "2", "VCCL_P2P_MIN_PART_BYTES": "4096"}
P2P_KNOBS = ("P2P_NVL_CHUNKSIZE", "P2P_PARTS", "P2P_MIN_PART_BYTES", "P2P_BUFFERS", "FENCES")


def run_case(n, case, extra=None, defaults=False):
    uid = nccl.get_unique_id()
    hexid = nccl.unique_id_to_bytes(uid).hex()
    env = dict(os.environ)
    for k in P2P_KNOBS:
        env.pop("VCCL_" + k, None)
        env.pop("NCCL_" + k, None)
    env.setdefault("VCCL_SPIN_TIMEOUT_S", "20")
    if defaults:
        for k in GEOM:
            env.pop(k, None)
        env["VCCL_ALLOW_SHARED_DEVICE"] = "1"
    else:
        env.update(GEOM)
    env.update(extra or {})
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_p2p_worker.py"),
                               str(r), str(n), hexid, case], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
    outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
    assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)


def test_exchange_sizes_offsets_types():
    """n = 2, grouped exchange both ways: sizes 0 B - 300 KiB x source offsets
    {0, 1, 3} x destination offsets {0, 2, 5} x u8 / bf16 / f32."""
    run_case(2, "exchange")


def test_ungrouped_back_to_back():
    """n = 2: rank 0 Send / rank 1 Recv and the reverse, 1 KiB and 300 KiB, 20
    iterations back to back (the persistent step counters)."""
    run_case(2, "ungrouped")


@pytest.mark.parametrize("n", [3, 4])
def test_ring_shift_and_sweeps(n):
    """Send to r + 1, recv from r - 1 in a group; two and three messages to
    one peer in one group are matched in call order."""
    run_case(n, "ring_shift")


def test_full_exchange_and_self_pairs():
    """n = 4: every pair a distinct size (one zero), self pairs out of place
    and in place; an unmatched self send fails ncclGroupEnd with
    ncclInvalidUsage and leaves every buffer untouched."""
    run_case(4, "full_exchange")


def test_all_to_all():
    """n = 4: ncclAllToAll of 1, 1000 and 70 001 f32; ncclAllToAllv with uneven
    counts, a zero count and gaps in the displacements; in place refused."""
    run_case(4, "all_to_all")


def test_mixed_with_collectives():
    """n = 4: all-reduce, a grouped exchange, all-reduce on one comm and two
    streams: as if sequential."""
    run_case(4, "mixed")


def test_argument_errors_on_a_live_comm():
    """Peer -1 / n, a bad datatype, a NULL buffer with count > 0:
    ncclInvalidArgument; a group containing one fails at End."""
    run_case(2, "arg_errors")


def test_eight_ranks_library_defaults():
    """n = 8 at library defaults (only the shared-device switch): all-to-alls
    of 64 KiB and 2 MiB per pair within the co-residency caps."""
    run_case(8, "defaults", defaults=True)


def test_capture_replay():
    """n = 2: a grouped exchange of 40 KiB captured on one stream, replayed 3
    times with fresh payloads; eager exchanges before and after."""
    run_case(2, "capture")


def test_exchange_with_fences():
    """n = 2 with VCCL_FENCES=1: the size list once."""
    run_case(2, "fences", extra={"VCCL_FENCES": "1"})
