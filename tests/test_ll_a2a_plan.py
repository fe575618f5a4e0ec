"""CPU checks of the one-hop LL all-to-all (host/plan.cc ll_a2a_max /
a2a_plan through vcclLLA2aPlan): the per-pair limit with its off switches, the pair rule's
symmetry between the two ends, the line-0 rule, the launch rule, the residual
sends and recvs as a matched set for the p2p planner, and the slot simulator of
tests/test_ll_rooted_plan.py run over sequences that mix all-to-all(v) plans
with the other LL collectives.  No GPU call is made."""
import itertools
import random

import pytest

from tests.test_ll_rooted_plan import _call_plans, _simulate, SIM_LINES
from vccl_amd import nccl

SLOT = 1 << 20
LIMIT = 512             # bytes per pair in the layout tests
LINES = LIMIT // 8      # ... which is the whole slot
SIZES = (0, 1, 7, 8, 9, LIMIT - 1, LIMIT, LIMIT + 1, 3 * LIMIT)


# ---------------------------------------------------------------- the limit
def test_ll_a2a_max_grid():
    """Clamped to the slot; 0 for a threshold of 0, without LL buffers, with
    LL excluded, with a net peer, below 2 or above 8 ranks, without p2p."""
    for thr, slot, allowed, net, n, p2p in itertools.product(
            (0, 1, 4096, SLOT, 8 << 20), (0, 4096, SLOT), (True, False), (False, True), range(1, 11), (True, False)):
        off = thr == 0 or slot == 0 or not allowed or net or n < 2 or n > 8 or not p2p
        assert nccl.ll_a2a_max(thr, slot, allowed, net, n, p2p) == (0 if off else min(thr, slot)), \
            (thr, slot, allowed, net, n, p2p)


def test_threshold_from_environment(monkeypatch):
    monkeypatch.delenv("VCCL_LL_A2A_THRESHOLD", raising=False)
    monkeypatch.delenv("NCCL_LL_A2A_THRESHOLD", raising=False)
    assert nccl.ll_a2a_max(None, SLOT) == 0  # the default is off
    monkeypatch.setenv("VCCL_LL_A2A_THRESHOLD", "4096")
    assert nccl.ll_a2a_max(None, SLOT) == 4096
    assert nccl.ll_a2a_max(None, 1024) == 1024
    monkeypatch.delenv("VCCL_LL_A2A_THRESHOLD")
    monkeypatch.setenv("NCCL_LL_A2A_THRESHOLD", "65536")
    assert nccl.ll_a2a_max(None, SLOT) == 65536
    # the rooted threshold is another knob
    monkeypatch.delenv("NCCL_LL_A2A_THRESHOLD")
    monkeypatch.setenv("VCCL_LL_ROOTED_THRESHOLD", "4096")
    assert nccl.ll_a2a_max(None, SLOT) == 0


# ---------------------------------------------------------------- layout
def _matrix(rng, n):
    """bytes[r][p] of the ordered pair r -> p; self pairs symmetric by construction."""
    return [[rng.choice(SIZES) for _ in range(n)] for _ in range(n)]


def _plans(m, n, limit=LIMIT, lines=LINES, uniform=False):
    return [nccl.ll_a2a_plan(n, r, m[r], [m[p][r] for p in range(n)], uniform, limit, lines) for r in range(n)]


@pytest.mark.parametrize("n", range(2, 9))
def test_pair_symmetry(n):
    """r's "send to p is LL" is p's "recv from r is LL"; what r stores at p is
    what p polls from r, range for range; line 0 of every ordered pair is
    stored once and polled once; no range leaves the slot."""
    rng = random.Random(4100 + n)
    for trial in range(50):
        m = _matrix(rng, n)
        plans = _plans(m, n)
        for r, p in itertools.product(range(n), range(n)):
            want = m[r][p] <= LIMIT
            assert plans[r]["send_ll"][p] == want and plans[p]["recv_ll"][r] == want, (trial, r, p, m[r][p])
            if r == p:
                assert not [x for x in plans[r]["stores"] + plans[r]["polls"] if x[0] == r]
                continue
            stores = [x[1:] for x in plans[r]["stores"] if x[0] == p]
            polled = [x[1:] for x in plans[p]["polls"] if x[0] == r]
            assert stores == polled and len(stores) == 1, (trial, r, p)
            part, a, b = stores[0]
            data = want and m[r][p] > 0
            assert (part, a, b) == ((0, 0, (m[r][p] + 7) // 8) if data else (-1, 0, 1)), (trial, r, p, m[r][p])
            assert 0 <= a < b <= LINES
        assert all(pl["launch"] for pl in plans)
    with pytest.raises(nccl.VcclError):  # a limit beyond the slot is no comm's
        nccl.ll_a2a_plan(n, 0, [8] * n, [8] * n, False, LIMIT + 8, LINES)
    with pytest.raises(nccl.VcclError):  # uniform means one value
        nccl.ll_a2a_plan(n, 0, [8] * (n - 1) + [16], [8] * n, True, LIMIT, LINES)


@pytest.mark.parametrize("n", range(2, 9))
def test_launch_rule(n):
    for b in SIZES:
        m = [[b] * n for _ in range(n)]
        ll = 0 < b <= LIMIT
        for pl in _plans(m, n, uniform=True):
            # uniform: one LL launch and no FIFO work at all, or today's path untouched
            assert pl["launch"] == ll
            assert pl["send_ll"] == [ll] * n and pl["recv_ll"] == [ll] * n
            assert pl["res_sends"] == ([] if ll else list(range(n))) and pl["res_recvs"] == pl["res_sends"]
            assert len(pl["stores"]) == len(pl["polls"]) == (n - 1 if ll else 0)
        for pl in _plans(m, n, limit=0, uniform=True) + _plans(m, n, limit=0):  # off: nothing is LL
            assert not pl["launch"] and not any(pl["send_ll"] + pl["recv_ll"]) and not pl["stores"] + pl["polls"]
            assert pl["res_sends"] == list(range(n)) == pl["res_recvs"]
    # v: a launch on every rank, even one whose row and column are all over the limit, or all zero
    m = [[8] * n for _ in range(n)]
    for p in range(n):
        m[0][p] = m[p][0] = 3 * LIMIT
        if n > 2:
            m[1][p] = m[p][1] = 0
    m[0][0] = 3 * LIMIT
    plans = _plans(m, n)
    assert all(pl["launch"] for pl in plans)
    assert plans[0]["res_sends"] == list(range(n)) and not any(plans[0]["send_ll"])
    assert all(x[1] == -1 for x in plans[0]["stores"] + plans[0]["polls"]) and len(plans[0]["stores"]) == n - 1
    if n > 2:
        assert plans[1]["res_sends"] == [0] and plans[1]["send_ll"][1:] == [True] * (n - 1)
        assert all(x[1] == -1 for x in plans[1]["stores"])


@pytest.mark.parametrize("n", range(2, 9))
def test_residuals_are_a_matched_set(n):
    """Every rank's residual sends and recvs, as calls of the p2p planner:
    each residual send has its recv of the same bytes at the other end, and the
    planner moves exactly those bytes."""
    rng = random.Random(4200 + n)
    for trial in range(50):
        m = _matrix(rng, n)
        plans = _plans(m, n)
        sends = {(r, p, m[r][p]) for r in range(n) for p in plans[r]["res_sends"]}
        recvs = {(p, r, m[p][r]) for r in range(n) for p in plans[r]["res_recvs"]}
        assert sends == recvs == {(r, p, m[r][p]) for r in range(n) for p in range(n) if m[r][p] > LIMIT}
        sent, got = {}, {}
        for r in range(n):
            calls = []
            for p in range(n):  # the expansion order: send p, recv p
                if p in plans[r]["res_sends"]:
                    calls.append((nccl.P2P_SEND, p, m[r][p], 1000 + 2 * p))
                if p in plans[r]["res_recvs"]:
                    calls.append((nccl.P2P_RECV, p, m[p][r], 1001 + 2 * p))
            items, _ = nccl.p2p_plan(r, n, calls, parts=2, min_part_bytes=256, step_bytes=4096)
            for it in items:
                if it["kind"] == nccl.P2P_SEND:
                    sent[(r, it["peer"])] = sent.get((r, it["peer"]), 0) + it["bytes"]
                elif it["kind"] == nccl.P2P_RECV:
                    got[(it["peer"], r)] = got.get((it["peer"], r), 0) + it["bytes"]
                else:
                    sent[(r, r)] = got[(r, r)] = sent.get((r, r), 0) + it["bytes"]
        assert sent == got == {(r, p): b for r, p, b in sends}, trial


# ---------------------------------------------------------------- simulator
def _a2a_call(rng, n):
    """One all-to-all(v) launch as per-rank (stores, polls) for _simulate."""
    limit = SIM_LINES * 8
    if rng.random() < 0.3:
        m = [[rng.choice([1, 8, 100, limit])] * n] * n
        plans = _plans(m, n, limit, SIM_LINES, uniform=True)
    else:
        m = [[rng.choice([0, 1, 9, limit - 1, limit, limit + 1, 3 * limit]) for _ in range(n)] for _ in range(n)]
        plans = _plans(m, n, limit, SIM_LINES)
    assert all(pl["launch"] for pl in plans)
    return [(pl["stores"], pl["polls"]) for pl in plans]


def test_slot_simulator_mixed_sequences():
    """30-call sequences mixing all-to-all(v) launches with all-reduce,
    reduce-scatter, all-gather, broadcast and reduce: no store lands on a line
    its reader has not consumed."""
    for s in range(120):
        rng = random.Random(7000 + s)
        n = rng.randint(2, 8)
        seq = [_a2a_call(rng, n) if rng.random() < 0.5 else _call_plans(rng, n) for _ in range(30)]
        assert _simulate(n, seq) is None, (s, n)


def test_slot_simulator_witness():
    """n = 2, three v-calls in a row in which one direction carries data and
    the other zero bytes: the writer waits for nobody's data, so without the
    token it laps the reader and its third call stores into the parity slot the
    reader still polls at the first.  The simulator's scheduler breaks a tie
    between two ranks at the same point towards the HIGHER rank, so it only
    lets the writer run ahead when the writer is rank 1: with 0 -> 1 carrying
    the data it advances the two ranks in step and never reaches the state, so
    that orientation is simulated with the two ranks' labels swapped (the same
    plans, as the layout check below shows)."""
    def seq_of(m):
        return [[(pl["stores"], pl["polls"]) for pl in _plans(m, 2, SIM_LINES * 8, SIM_LINES)] for _ in range(3)]
    fwd, rev = seq_of([[0, 64], [0, 0]]), seq_of([[0, 0], [64, 0]])  # 0 -> 1 carries the data / 1 -> 0 does
    assert fwd[0][0] == ([(1, 0, 0, 8)], [(1, -1, 0, 1)]) and fwd[0][1] == ([(0, -1, 0, 1)], [(0, 0, 0, 8)])
    swap = lambda rs: [(1 - p, part, a, b) for p, part, a, b in rs]
    assert [[(swap(st), swap(po)) for st, po in reversed(call)] for call in fwd] == rev
    assert _simulate(2, rev, tokens=False) == (1, 0, 2, 0)
    assert _simulate(2, rev) is None and _simulate(2, fwd) is None
