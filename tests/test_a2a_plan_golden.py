"""Replay of tests/golden/a2a_plan.json (recorded by tests/golden/gen_a2a_plan.py
at the commit before the two all-to-all planners became one): the full outputs
of vcclLLA2aPlan and vcclDirectA2aPlan, stores / polls included, every refusal
by its error code, and rows of vcclRootedAlgo / vcclRootedAlgoEx taken with the
rooted thresholds set in the environment.  Equality is demanded.  No GPU call."""
import json
import os

import pytest

from vccl_amd import nccl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a2a_plan.json")


def _plain(x):
    """As JSON stores it (tuples as lists)."""
    return json.loads(json.dumps(x))


def _or_code(f):
    try:
        return _plain(f())
    except nccl.VcclError as e:
        return e.code


def a2a_outputs(inp):
    """inp = [nranks, rank, uniform, ll limit, direct limit, lines per slot,
    minCTAs, maxCTAs, directMaxBlocks, send bytes, recv bytes] -> the two
    exports' outputs, each field by field in a fixed order, or the error code."""
    n, rank, uniform, ll, d, lines, minc, maxc, dmb, send, recv = inp

    def ll_plan():
        p = nccl.ll_a2a_plan(n, rank, send, recv, bool(uniform), ll, lines)
        return [p["launch"], p["send_ll"], p["recv_ll"], p["stores"], p["polls"], p["res_sends"], p["res_recvs"]]

    def direct_plan():
        p = nccl.direct_a2a_plan(n, rank, send, recv, bool(uniform), ll, d, lines, minc, maxc, dmb)
        return [p["ll_launch"], p["direct_launch"], p["send_path"], p["recv_path"], p["n_blocks"], p["blk_bytes"],
                p["res_sends"], p["res_recvs"]]

    return [_or_code(ll_plan), _or_code(direct_plan)]


def rooted_outputs(inp):
    """inp = [coll, count, dtype, nranks, policy words, LL threshold or None,
    llAllowed, anyNet, direct threshold or None, directAllowed] -> the outputs
    of vcclRootedAlgo and vcclRootedAlgoEx (None: from the environment)."""
    coll, count, dtype, n, words, thr, ll_ok, net, dthr, d_ok = inp
    pol = dict(zip(nccl.POLICY_FIELDS, words))
    return [_or_code(lambda: nccl.rooted_algo(coll, count, dtype, n, pol, thr, bool(ll_ok), bool(net))),
            _or_code(lambda: nccl.rooted_algo_ex(coll, count, dtype, n, pol, thr, bool(ll_ok), bool(net), dthr,
                                                 bool(d_ok)))]


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_what_it_should(recorded):
    a2a = recorded["a2a"]
    assert len(a2a) >= 300 and len(recorded["rooted"]) >= 36
    assert {c[0][0] for c in a2a} >= set(range(2, 10))
    assert {(c[0][3] > 0, c[0][4] > 0) for c in a2a} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c[0][2] for c in a2a} == {0, 1}
    assert any(isinstance(c[1][0], int) for c in a2a) and any(isinstance(c[1][1], int) for c in a2a)
    assert any(not isinstance(c[1][0], int) and c[1][0][0] for c in a2a)            # an LL launch
    assert any(not isinstance(c[1][1], int) and c[1][1][1] for c in a2a)            # a direct launch
    assert any(c[0][8] == 1 for c in a2a)                                           # directMaxBlocks 1


def test_all_to_all_plans_replay(recorded):
    for inp, want in recorded["a2a"]:
        assert a2a_outputs(inp) == want, inp


def test_rooted_algo_rows_replay(recorded, monkeypatch):
    for k in ("LL_ROOTED_THRESHOLD", "DIRECT_ROOTED_THRESHOLD"):
        monkeypatch.delenv("NCCL_" + k, raising=False)
        monkeypatch.setenv("VCCL_" + k, str(recorded["env"]["VCCL_" + k]))
    for inp, want in recorded["rooted"]:
        assert rooted_outputs(inp) == want, inp
