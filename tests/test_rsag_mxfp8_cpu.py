"""The MXFP8 reduce-scatter / all-gather without a GPU: the entry points refuse a NULL comm, and the worker's model
(tests/mp_rsag_mxfp8_worker.py) agrees with the all-reduce model's building blocks on one tiny case."""
import ctypes

import torch

from tests.mp_ar_mxfp8_worker import inputs, model_allreduce, roundtrip
from tests.mp_rsag_mxfp8_worker import AG, RS, fold, model, rs_bound
from vccl_amd import nccl


def test_refusals():
    L = nccl.lib()
    eff, rs, ag = ctypes.c_int64(-1), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vcclCommSetRsAgMxfp8Threshold(None, 1, ctypes.byref(eff)) == nccl.ncclInvalidArgument and eff.value == -1
    assert L.vcclCommRsAgMxfp8Stats(None, ctypes.byref(rs), ctypes.byref(ag)) == nccl.ncclInvalidArgument
    assert (rs.value, ag.value) == (7, 7)


def test_model_agrees_with_allreduce_model():
    """n = 3, c = 40 (a block boundary inside every rank's block): the reduce-scatter is the all-reduce of the
    rank's pieces without the second pass through the format, cut by the index within the piece; the all-gather
    is the one-rank all-reduce of every input; and the derived bound holds for the model."""
    n, c, t = 3, 40, torch.bfloat16
    xs = [inputs(50 + r, n * c) for r in range(n)]
    for p in range(n):
        pieces = [x[p * c:(p + 1) * c] for x in xs]
        assert torch.equal(roundtrip(fold(pieces)).to(t), model_allreduce(pieces, t))
        assert torch.equal(model(RS, xs, p, c, t), fold(pieces).to(t))
        exact, tol = rs_bound(xs, p, c, 9)
        assert bool(((model(RS, xs, p, c, t).double() - exact).abs() <= tol).all())
    # blocks follow the piece, not the send buffer: piece 2 starts 16 elements into a block of the whole input
    assert not torch.equal(fold([x[2 * c:] for x in xs]), fold(xs)[2 * c:])
    ys = [x[:c] for x in xs]
    assert torch.equal(model(AG, ys, 0, c, t), torch.cat([model_allreduce([y], t) for y in ys]))
