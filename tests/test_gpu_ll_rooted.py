"""One-hop LL ncclBroadcast / ncclReduce on MI355X (tests/mp_ll_rooted_worker.py:
one process per rank, ranks sharing the GPU where the box has fewer GPUs than
ranks).  The path is opt-in: the tests set VCCL_LL_ROOTED_THRESHOLD to the
slot (1 MiB in the shared-GPU geometry of the collective tests).  Spins are
bounded (VCCL_SPIN_TIMEOUT_S), so a protocol bug fails a test instead of
hanging the GPU."""
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

from vccl_amd import nccl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_gpu_collectives.py TEST_GEOM's values
GEOM = {"VCCL_NCHANNELS": "14", "VCCL_NTHREADS": "512", "VCCL_SLOT_BYTES": str(256 << 10),
        "VCCL_ALLOW_SHARED_DEVICE": "1", "VCCL_LL_THRESHOLD": str(1 << 20),
        "VCCL_LL_MAX_BLOCKS": "32", "VCCL_DIRECT_THRESHOLD": str(4 << 20),
        "VCCL_DIRECT_MAX_BLOCKS": "16", "VCCL_DIRECT_CHUNK_BYTES": str(1 << 20),
        "VCCL_DIRECT_RSAG_THRESHOLD": str(64 << 20), "VCCL_RING_WAVE": "1", "VCCL_RING_WAVE_MIN": "0"}
NCH, SLOT = 14, 256 << 10
ROOTED = {"VCCL_LL_ROOTED_THRESHOLD": str(1 << 20)}
LL_ROWS = ("red_f32_sum_one", "red_f16_sum", "red_f32_avg", "red_i32_max", "red_u8_prod", "red_f64_min",
           "red_bf16_prod", "red_f32_sum_inplace")


def run_case(n, case, extra=ROOTED):
    """The n rank processes of `case`; returns what each saved."""
    uid = nccl.get_unique_id()
    hexid = nccl.unique_id_to_bytes(uid).hex()
    env = dict(os.environ)
    for k in ("VCCL_LL_ROOTED_THRESHOLD", "NCCL_LL_ROOTED_THRESHOLD", "NCCL_PROTO", "NCCL_ALGO", "VCCL_NET_FORCE"):
        env.pop(k, None)
    env.setdefault("VCCL_SPIN_TIMEOUT_S", "20")
    env.update(GEOM)
    env.update(extra)
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_ll_rooted_worker.py"),
                                   str(r), str(n), hexid, case, d], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
        outs = [p.communicate(timeout=300)[0].decode(errors="replace")[-2000:] for p in procs]
        assert [p.returncode for p in procs] == [0] * n, "\n".join(outs)
        return [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(n)]


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_broadcast(n):
    """1, 7, 8, 9, 4099 and 65541 bytes from every root, out of place (a
    non-root's sendbuff NULL) and ncclBcast in place, destinations 0, 1 and 3
    bytes past a 16-byte boundary: coll_algo reports LL, every byte exact, the
    bytes before and the 64 after each output intact."""
    run_case(n, "bcast")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_reduce(n):
    """RC.REDUCE_CASES at every root: the rows of at most 1 MiB take LL and are
    bit-exact against the oracle's fold on the call's LL partition (root's
    successor first, root last), the larger ones take the ring as before; fp
    sum / prod also within the fold tolerance of the exact value.  A non-root's
    recvbuff and every input stay untouched (checked by the worker)."""
    res = run_case(n, "reduce")
    differs = {}
    for ri, (name, op, dt, count, _) in enumerate(RC.REDUCE_CASES):
        ins = [RC.gen_reduce_input(ri, r) for r in range(n)]
        ll = name in LL_ROWS
        assert ll == (ins[0].nbytes <= 1 << 20)
        for root in range(n):
            exp = _ring.expected_reduce(op, dt, ins, root, NCH, SLOT,
                                        proto=_ring.S.PROTO_LL if ll else _ring.S.PROTO_SIMPLE)
            got = res[root][f"{name}_r{root}"]
            assert_bitexact(dt, got, exp, minmax=op in (2, 3), what=f"reduce {name} n={n} root {root}")
            if op in RC.TOLERANCE_OPS and dt in (6, 7, 8, 9):
                assert_fold_tolerance(dt, op, got, exact_f64(dt, op, ins), ins, exp_is_exact=True,
                                      what=f"reduce {name} n={n} root {root} vs exact")
            if ll and n in (4, 8) and name in ("red_f16_sum", "red_f32_avg", "red_f32_sum_inplace"):
                simple = _ring.expected_reduce(op, dt, ins, root, NCH, SLOT, proto=_ring.S.PROTO_SIMPLE)
                differs[name] = differs.get(name, False) or not np.array_equal(exp.view(np.uint8),
                                                                              simple.view(np.uint8))
    # the LL order is not the SIMPLE ring's: the bit-exact check tells them apart
    assert all(differs.values()), differs


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
    assert [str(a) for a in res[0]["bcast_group_algos"]] == ["ll"] * 4
    algos = [str(a) for a in res[0]["group_algos"]]
    assert algos[:4] == ["ll"] * 4 and algos[4] != "ll"
    calls = [("red", 0, 7, cnt) for cnt, _ in GROUP_REDUCES] + [("ar", 0, 7, GROUP_AR)]
    works = _ring.group_works(calls, n, NCH, SLOT, algos=algos)
    for k, (cnt, root) in enumerate(GROUP_REDUCES):
        ins = [group_reduce_input(k, r) for r in range(n)]
        exp = _ring.expected_reduce(0, 7, ins, root % n, NCH, SLOT, proto=_ring.S.PROTO_LL, work=works[k])
        assert_bitexact(7, res[root % n][f"group{k}"], exp, what=f"group reduce {k} n={n} root {root % n}")


@pytest.mark.parametrize("n", [2, 4])
def test_back_to_back(n):
    """No host synchronisation between calls: 64 broadcasts of 4 KiB from one
    root into 64 outputs, 64 more with the root rotating, then 48 calls mixing
    broadcast, reduce and the LL all-reduce; one synchronise, every output
    checked."""
    run_case(n, "b2b")


def test_capture_replay():
    """n = 2: [broadcast root 0, reduce root 1, broadcast root 1] captured on
    one stream, replayed three times with fresh inputs."""
    run_case(2, "capture")


def test_epoch_wrap():
    """n = 2: the LL epoch seeded at 0xfffffffe, then two broadcasts and two
    reduces across the wrap."""
    run_case(2, "wrap")


@pytest.mark.parametrize("extra", [{}, dict(ROOTED, VCCL_NET_FORCE="1"), dict(ROOTED, NCCL_PROTO="^LL")],
                         ids=["unset", "net", "no_ll"])
def test_off_switches(extra):
    """Threshold unset, or set with a net peer or with LL excluded by
    NCCL_PROTO: both collectives report the ring (or LL128 in its window) at
    every size."""
    run_case(2, "off", extra=extra)
