"""Two-hop direct ncclBroadcast / ncclReduce on MI355X (tests/
mp_direct_rooted_worker.py: one process per rank, ranks sharing the GPU where
the box has fewer GPUs than ranks).  The path is opt-in: the tests set
VCCL_DIRECT_ROOTED_THRESHOLD to 8 MiB and leave VCCL_LL_ROOTED_THRESHOLD unset,
in the shared-GPU geometry of the rooted LL tests.  Spins are bounded
(VCCL_SPIN_TIMEOUT_S), so a protocol bug fails a test instead of hanging the
GPU."""
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
ROOTED = {"VCCL_DIRECT_ROOTED_THRESHOLD": str(8 << 20)}
CLEARED = ("VCCL_LL_ROOTED_THRESHOLD", "NCCL_LL_ROOTED_THRESHOLD", "VCCL_DIRECT_ROOTED_THRESHOLD",
           "NCCL_DIRECT_ROOTED_THRESHOLD", "NCCL_PROTO", "NCCL_ALGO", "VCCL_NET_FORCE")


def run_case(n, case, extra=ROOTED):
    """The n rank processes of `case`; returns what each saved."""
    uid = nccl.get_unique_id()
    hexid = nccl.unique_id_to_bytes(uid).hex()
    env = dict(os.environ)
    for k in CLEARED:
        env.pop(k, None)
    env.update(GEOM)
    env["VCCL_SPIN_TIMEOUT_S"] = "20"
    env.update(extra)
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_direct_rooted_worker.py"),
                                   str(r), str(n), hexid, case, d], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
        outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
        assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)
        return [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(n)]


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_broadcast(n):
    """1, 15, 16, 17, 4099 and 65541 bytes, 16 (n-1) k +- 1 for k = 1 and 257,
    and 3 chunks + 5, from every root, out of place (a non-root's sendbuff
    NULL) and ncclBcast in place, destinations 0, 1 and 3 bytes past a 16-byte
    boundary: coll_algo reports direct, every byte exact, the bytes before and
    the 64 after each output intact."""
    run_case(n, "bcast")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_reduce(n):
    """RC.REDUCE_CASES at every root: the rows of at most 8 MiB take the direct
    path, the larger ones the ring as before; all bit-exact against the
    oracle's fold on the call's SIMPLE partition (root's successor first, root
    last); fp sum / prod also within the fold tolerance of the exact value.  A
    non-root's recvbuff and every input stay untouched (checked by the worker)."""
    res = run_case(n, "reduce")
    for ri, (name, op, dt, count, _) in enumerate(RC.REDUCE_CASES):
        ins = [RC.gen_reduce_input(ri, r) for r in range(n)]
        for root in range(n):
            exp = _ring.expected_reduce(op, dt, ins, root, NCH, SLOT, proto=_ring.S.PROTO_SIMPLE)
            got = res[root][f"{name}_r{root}"]
            assert_bitexact(dt, got, exp, minmax=op in (2, 3), what=f"reduce {name} n={n} root {root}")
            if op in RC.TOLERANCE_OPS and dt in (6, 7, 8, 9):
                assert_fold_tolerance(dt, op, got, exact_f64(dt, op, ins), ins, exp_is_exact=True,
                                      what=f"reduce {name} n={n} root {root} vs exact")


@pytest.mark.parametrize("n", [2, 4])
def test_multichunk(n):
    """VCCL_DIRECT_CHUNK_BYTES=65536: a 300,001-element f32 sum reduce and a
    1,200,007-byte broadcast, about 19 chunks each, root 0 and root n - 1."""
    from tests.mp_direct_rooted_worker import multi_reduce_input
    res = run_case(n, "multichunk", extra=dict(ROOTED, VCCL_DIRECT_CHUNK_BYTES="65536"))
    ins = [multi_reduce_input(r) for r in range(n)]
    for root in (0, n - 1):
        exp = _ring.expected_reduce(0, 7, ins, root, NCH, SLOT, proto=_ring.S.PROTO_SIMPLE)
        assert_bitexact(7, res[root][f"multi_r{root}"], exp, what=f"multichunk reduce n={n} root {root}")


@pytest.mark.parametrize("n", [2, 4])
def test_groups(n):
    """One group of five broadcasts from different roots (u8 x 1, bf16 x
    70,000, f32 x 77, i32 x 5,000, one empty) and one of four f32-sum reduces
    to different roots plus a 4 MiB all-reduce: each run of rooted calls is one
    launch, group_algos agree across ranks, every output exact — the reduces
    against their place in VCCL's group plan."""
    from tests.mp_ll_rooted_worker import GROUP_AR, GROUP_REDUCES, group_reduce_input
    res = run_case(n, "groups")
    for key in ("bcast_group_algos", "group_algos"):
        for r in range(n):
            assert list(res[r][key]) == list(res[0][key]), (key, r)
    assert [str(a) for a in res[0]["bcast_group_algos"]] == ["direct"] * 4
    algos = [str(a) for a in res[0]["group_algos"]]
    assert algos[:4] == ["direct"] * 4
    calls = [("red", 0, 7, cnt) for cnt, _ in GROUP_REDUCES] + [("ar", 0, 7, GROUP_AR)]
    works = _ring.group_works(calls, n, NCH, SLOT, algos=algos)
    for k, (cnt, root) in enumerate(GROUP_REDUCES):
        ins = [group_reduce_input(k, r) for r in range(n)]
        exp = _ring.expected_reduce(0, 7, ins, root % n, NCH, SLOT, proto=_ring.S.PROTO_SIMPLE, work=works[k])
        assert_bitexact(7, res[root % n][f"group{k}"], exp, what=f"group reduce {k} n={n} root {root % n}")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """The test of the inbox reuse rule: 96 calls with no host synchronisation
    on a 128 KiB inbox, cycling through the forced direct all-reduce (1, 2 and
    3 chunks: the issue's 1 and 3 both end on parity 0, the 2-chunk call ends
    on parity 1, so both final parities occur), direct reduce-scatter, direct
    all-gather, broadcast and reduce (200-300 KB each; the 1-chunk all-reduce
    120 KB) with the root rotating; one synchronise, every output checked."""
    run_case(n, "b2b", extra=dict(ROOTED, VCCL_DIRECT_CHUNK_BYTES=str(128 << 10)))


def test_capture_replay():
    """n = 2: [broadcast root 0, reduce root 1, broadcast root 1] captured on
    one stream, replayed three times with fresh inputs."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the direct epoch seeded at 0xfffffffe, then two broadcasts and
    two reduces across the wrap."""
    run_case(2, "wrap")


@pytest.mark.parametrize("extra", [{}, dict(ROOTED, VCCL_NET_FORCE="1"), dict(ROOTED, NCCL_ALGO="Ring"),
                                   dict(ROOTED, NCCL_ALGO="^Direct"), {"NCCL_ALGO": "Direct"}],
                         ids=["unset", "net", "algo_ring", "no_direct", "direct_unset"])
def test_off_switches(extra):
    """Threshold unset; set with a net peer, with NCCL_ALGO=Ring or with Direct
    excluded; NCCL_ALGO=Direct with the threshold unset: both collectives
    report the ring (or LL128 in its window) at every size."""
    run_case(2, "off", extra=extra)
