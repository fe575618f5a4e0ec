"""Special-value and order-sensitive payloads through every fold path on MI355X
(tests/mp_payload_worker.py: one process per rank, one comm, ranks sharing the
GPU where the box has fewer GPUs than ranks).

tests/_payloads.py hard_input streams — NaNs, infinities, -0 that must survive
a sum, subnormals, x + (-x), sums that overflow or saturate, an fp8 infinity
code that must narrow to max-finite, round-to-even ties, a SumPostDiv dividend
at the signed minimum, between finite values of 21 binades — go through the
one-hop LL all-reduce / reduce-scatter / reduce, the staged direct path, the
SIMPLE ring with the workgroup and with the per-wave hand-off and the LL128
ring, for f16, bf16, f32, f64, both fp8, i8, i32, u64 and every op, at 2, 3
and 4 ranks.  The parent regenerates the inputs and holds every output
bit-exact to the oracle's fold in that path's order (NaN by NaN-ness, +0 == -0
for min / max only); no tolerance enters.  Each n's worker processes run once
(a module-scoped fixture) and every path's test reads what they saved.

The geometry is TEST_GEOM of the collective tests plus the LL128 FIFOs
(VCCL_LL128_ALLOC) and the opt-in one-hop LL ncclReduce
(VCCL_LL_ROOTED_THRESHOLD, without which a forced LL reduce takes the ring).
Spins are bounded (VCCL_SPIN_TIMEOUT_S), so a protocol bug fails a test
instead of hanging the GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import _mp
from tests import _payloads as P
from tests import ring_cases as RC
from tests._util import assert_bitexact

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.test_gpu_collectives import TEST_GEOM  # noqa: E402
from tests.mp_payload_worker import MIS, PAIR_TYPES, PASSES  # noqa: E402
from vccl_amd import nccl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCH, SLOT = int(TEST_GEOM["VCCL_NCHANNELS"]), int(TEST_GEOM["VCCL_SLOT_BYTES"])
_RUNS = {}


def _run(n):
    """The n rank processes, once per module; what each rank saved."""
    if n in _RUNS:
        return _RUNS[n]
    hexid = nccl.unique_id_to_bytes(nccl.get_unique_id()).hex()
    env = dict(os.environ)
    for k in ("NCCL_PROTO", "NCCL_ALGO", "VCCL_NET_FORCE", "VCCL_FENCES", "VCCL_LL_CHAIN", "VCCL_REG_THRESHOLD"):
        env.pop(k, None)
    env.update(TEST_GEOM)
    env.update(VCCL_LL128_ALLOC="1", VCCL_LL_ROOTED_THRESHOLD=str(1 << 20), VCCL_SPIN_TIMEOUT_S="20")
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_payload_worker.py"),
                                   str(r), str(n), hexid, d], env=_mp.worker_env(env),
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
        logs = []
        for p in procs:
            try:
                out, _ = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            logs.append(out.decode(errors="replace")[-2000:])
        assert [p.returncode for p in procs] == [0] * n, "\n".join(logs)
        _RUNS[n] = [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(n)]
    return _RUNS[n]


@pytest.mark.parametrize("name,path,wave,reduce_too", PASSES, ids=[p[0] for p in PASSES])
@pytest.mark.parametrize("n", P.MATRIX_RANKS)
def test_fold_path(n, name, path, wave, reduce_too):
    """All-reduce 8 209, reduce-scatter 2 053 per rank and (LL, ring) reduce
    8 209 to root n - 1 on one forced path: every (type, op) bit-exact to the
    oracle's fold in the path's order."""
    res = _run(n)
    for dt in P.MATRIX_TYPES:
        for op in P.MATRIX_OPS:
            what = f"{name} {O.TYPE_NAMES[dt]} {O.OP_NAMES[op]} n={n}"
            mm = op in (2, 3)
            ar = [P.hard_input(dt, op, P.AR_COUNT, r, n, P.SEED) for r in range(n)]
            rs = [P.hard_input(dt, op, n * P.RS_COUNT, r, n, P.SEED) for r in range(n)]
            exp = RC.expected_on_path(path, "ar", op, dt, ar, NCH, SLOT)
            P.assert_cap(dt, exp, "ar " + what)
            for r in range(n):
                assert_bitexact(dt, res[r][f"{name}_ar_{dt}_{op}"], exp, minmax=mm, what=f"ar {what} rank {r}")
            exps = RC.expected_on_path(path, "rs", op, dt, rs, NCH, SLOT)
            for r in range(n):
                P.assert_cap(dt, exps[r], f"rs {what} rank {r}")
                assert_bitexact(dt, res[r][f"{name}_rs_{dt}_{op}"], exps[r], minmax=mm, what=f"rs {what} rank {r}")
            if reduce_too:
                exp = RC.expected_on_path(path, "red", op, dt, ar, NCH, SLOT, root=n - 1)
                P.assert_cap(dt, exp, "red " + what)
                assert_bitexact(dt, res[n - 1][f"{name}_red_{dt}_{op}"], exp, minmax=mm, what="red " + what)


@pytest.mark.parametrize("n", P.MATRIX_RANKS)
def test_ll_ragged_last_line(n):
    """LL all-reduce of 8 209 f16 and 4 099 bf16 into a receive pointer 2 bytes
    past alignment: the last line is zero padded and folded on the padding;
    only the output's byte count keeps it out (guards checked by the worker)."""
    res = _run(n)
    for dt, count in MIS:
        ins = [P.hard_input(dt, 0, count, r, n, P.SEED + 1) for r in range(n)]
        exp = RC.expected_on_path("ll", "ar", 0, dt, ins, NCH, SLOT)
        P.assert_cap(dt, exp, f"ll mis {O.TYPE_NAMES[dt]} n={n}")
        for r in range(n):
            assert_bitexact(dt, res[r][f"ll_mis_{dt}"], exp, what=f"ll mis {O.TYPE_NAMES[dt]} n={n} rank {r}")


@pytest.mark.parametrize("dt", PAIR_TYPES, ids=[O.TYPE_NAMES[t] for t in PAIR_TYPES])
def test_ll_all_byte_pairs(dt):
    """n = 2: every (a, b) byte pair through the LL kernels' per-element
    functors (u8, i8, E4M3, E5M2; every op), as an all-reduce of 65 536 and a
    reduce-scatter whose blocks are the two halves."""
    res = _run(2)
    ins = [x.view(O.NP_DTYPE[dt]) for x in P.all_pairs_u8()]
    for op in P.MATRIX_OPS:
        what = f"pairs {O.TYPE_NAMES[dt]} {O.OP_NAMES[op]}"
        exp = RC.expected_on_path("ll", "ar", op, dt, ins, NCH, SLOT)
        exps = RC.expected_on_path("ll", "rs", op, dt, ins, NCH, SLOT)
        if dt in P.F8_TYPES:
            assert 4 * P.classes(dt, exp)["nan"] <= exp.size, what
        for r in range(2):
            assert_bitexact(dt, res[r][f"pairs_ar_{dt}_{op}"], exp, minmax=op in (2, 3), what=f"ar {what} rank {r}")
            assert_bitexact(dt, res[r][f"pairs_rs_{dt}_{op}"], exps[r], minmax=op in (2, 3), what=f"rs {what} rank {r}")
