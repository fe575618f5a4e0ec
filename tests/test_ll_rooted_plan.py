"""CPU checks of the one-hop LL broadcast / reduce (host/plan.cc): the
selection with its opt-in threshold (vcclRootedAlgo), the invariants of the
launch's line layout (vcclLLRootedPlan), and a slot simulator that runs
random sequences of LL calls under an adversarial scheduler and looks for a
store into a parity slot whose previous content its reader has not consumed —
none with the library's plans, at least one once the arrival token lines are
taken out.  No GPU call is made."""
import itertools
import random

import pytest

from tests import _ring
from vccl_amd import nccl

BC, RED = 3, 4
SLOT = 1 << 20  # bytes of one LL slot in the selection grid


def _policy(force, ll_slot, ll128):
    return {"force": force, "ll_slot": ll_slot, "ll_max": 128 << 10, "ll_rsag_max": 512 << 10, "ll128": ll128,
            "ll128_min": 64 << 10, "ll128_max": (1 << 20) if ll128 else 0, "direct": 1, "direct_max": 8 << 20,
            "direct_rsag_max": 8 << 20}


# ---------------------------------------------------------------- selection
@pytest.mark.parametrize("coll,name,dt,esz", [(BC, "bc", nccl.ncclUint8, 1), (RED, "red", nccl.ncclFloat32, 4)])
def test_selection_grid(coll, name, dt, esz):
    """Threshold 0: exactly tests/_ring.select_algo's answer (the ring, or
    LL128 in its window) for every input.  A threshold: clamped to the slot;
    zeroed without LL buffers, with LL excluded, with a net peer, above 8
    ranks; a call of at most that many bytes takes LL when the path is
    automatic or forced LL, every other force keeps today's outcome."""
    thr = 96 << 10
    sizes = [4, thr - 4, thr, thr + 4, 100 << 10, SLOT, SLOT + 4, 4 << 20]
    for n, force, ll_slot, ll128, allowed, net in itertools.product(
            range(1, 10), range(5), (0, SLOT), (0, 1), (True, False), (False, True)):
        pol = _policy(force, ll_slot, ll128)
        for nbytes in sizes:
            count = nbytes // esz
            ring = _ring.select_algo(pol, name, esz, count, n)
            assert ring in ("ring", "ll128")
            got, eff = nccl.rooted_algo(coll, count, dt, n, pol, 0, allowed, net)
            assert (got, eff) == (ring, 0), (n, force, ll_slot, ll128, allowed, net, nbytes)
            for t in (thr, 8 << 20):
                want_eff = 0 if (not allowed or net or ll_slot == 0 or n > 8) else min(t, ll_slot)
                got, eff = nccl.rooted_algo(coll, count, dt, n, pol, t, allowed, net)
                assert eff == want_eff, (n, force, ll_slot, allowed, net, t)
                ll = n >= 2 and want_eff > 0 and nbytes <= want_eff and force in (0, 2)
                assert got == ("ll" if ll else ring), (n, force, ll_slot, ll128, allowed, net, nbytes, t)


def test_selection_threshold_from_environment(monkeypatch):
    pol = _policy(0, SLOT, 0)
    monkeypatch.delenv("VCCL_LL_ROOTED_THRESHOLD", raising=False)
    monkeypatch.delenv("NCCL_LL_ROOTED_THRESHOLD", raising=False)
    assert nccl.rooted_algo(BC, 8, nccl.ncclUint8, 4, pol) == ("ring", 0)  # the default is off
    monkeypatch.setenv("VCCL_LL_ROOTED_THRESHOLD", "4096")
    assert nccl.rooted_algo(BC, 4096, nccl.ncclUint8, 4, pol) == ("ll", 4096)
    assert nccl.rooted_algo(RED, 1025, nccl.ncclFloat32, 4, pol) == ("ring", 4096)
    # the other collectives are untouched by it
    for coll, nm in ((0, "ar"), (1, "rs"), (2, "ag")):
        for count in (8, 4096, 1 << 20):
            assert nccl.rooted_algo(coll, count, nccl.ncclFloat32, 4, pol)[0] == \
                _ring.select_algo(pol, nm, 1 if nm == "ag" else 4, count * (4 if nm == "ag" else 1), 4)


# ---------------------------------------------------------------- layout
def _random_parts(rng, n, slot_lines):
    k = rng.randint(1, 16)
    parts, left = [], slot_lines * 8
    for _ in range(k):
        b = rng.choice([0, 1, 7, 8, 9, rng.randint(0, max(0, left))])
        b = min(b, left)
        left -= (b + 7) // 8 * 8
        parts.append((rng.randrange(n), b))
    return parts


@pytest.mark.parametrize("n", range(2, 9))
def test_layout_invariants(n):
    """What a rank stores at a peer is what that peer polls from it; parts
    never overlap; line 0 of every ordered pair is stored and polled exactly
    once per launch."""
    rng = random.Random(100 + n)
    slot_lines = 512
    for trial in range(60):
        coll = rng.choice([BC, RED])
        parts = _random_parts(rng, n, slot_lines) if trial else [(rng.randrange(n), slot_lines * 8)]
        plans = [nccl.ll_rooted_plan(coll, n, r, parts, slot_lines) for r in range(n)]
        line0 = plans[0][0]
        ends = [l0 + (b + 7) // 8 for l0, (_, b) in zip(line0, parts)]
        assert line0[0] == 0 and all(line0[i + 1] == ends[i] for i in range(len(parts) - 1)) and ends[-1] <= slot_lines
        for r in range(n):
            assert plans[r][0] == line0
            for peer in range(n):
                if peer == r:
                    assert not [x for x in plans[r][1] + plans[r][2] if x[0] == r]
                    continue
                stores = sorted(x[1:] for x in plans[r][1] if x[0] == peer)
                polled = sorted(x[1:] for x in plans[peer][2] if x[0] == r)
                assert stores == polled, (coll, parts, r, peer)
                # data ranges are whole parts of the right root, disjoint
                for part, a, b in stores:
                    if part >= 0:
                        assert (a, b) == (line0[part], ends[part]) and a < b
                        assert parts[part][0] == (peer if coll == RED else r)
                lines = [l for _, a, b in stores for l in range(a, b)]
                assert len(lines) == len(set(lines))
                assert lines.count(0) == 1, (coll, parts, r, peer)
    with pytest.raises(nccl.VcclError):
        nccl.ll_rooted_plan(BC, n, 0, [(0, slot_lines * 8), (1, 1)], slot_lines)


# ---------------------------------------------------------------- simulator
SIM_LINES = 64


def _call_plans(rng, n):
    """One LL call as per-rank (stores, polls) range lists [(peer, a, b)]."""
    kind = rng.choice(["ar", "rs", "ag", "bc", "red"])
    if kind in ("bc", "red"):
        parts = _random_parts(rng, n, SIM_LINES)
        if all(b == 0 for _, b in parts):
            parts[0] = (parts[0][0], 8)
        out = []
        for r in range(n):
            _, st, po = nccl.ll_rooted_plan(BC if kind == "bc" else RED, n, r, parts, SIM_LINES)
            out.append((st, po))
        return out
    lines = rng.randint(1, SIM_LINES)  # every rank writes to and waits for every peer
    every = lambda r: [(p, 0, 0, lines) for p in range(n) if p != r]
    return [(every(r), every(r)) for r in range(n)]


def _simulate(n, seq, tokens=True):
    """Runs `seq` (a list of per-rank (stores, polls)) with call k on parity
    k & 1: a rank first issues every store of its call, then waits until every
    polled range carries the call's epoch, then retires it.  The scheduler
    always advances the rank furthest ahead that can move.  Returns the first
    (writer, reader, call, earlier call) whose store lands on a line the reader
    still has to poll at the earlier call of the same parity, or None."""
    def keep(rs):
        return [x for x in rs if tokens or x[1] >= 0]
    pos = [0] * n          # the call a rank is in
    stored = [False] * n   # ... and whether its stores are out
    def can_move(r):
        k = pos[r]
        if k >= len(seq):
            return False
        if not stored[r]:
            return True
        return all(pos[p] > k or (pos[p] == k and stored[p]) for p, _, a, b in keep(seq[k][r][1]))
    while True:
        movers = [r for r in range(n) if can_move(r)]
        if not movers:
            assert all(p == len(seq) for p in pos), "the simulated ranks deadlocked"
            return None
        r = max(movers, key=lambda q: (pos[q], stored[q], q))
        k = pos[r]
        if stored[r]:
            pos[r], stored[r] = k + 1, False
            continue
        for peer, _, a, b in keep(seq[k][r][0]):
            for k2 in range(k - 2, pos[peer] - 1, -2):  # same parity, not yet retired by the reader
                for q, _, a2, b2 in keep(seq[k2][peer][1]):
                    if q == r and a < b2 and a2 < b:
                        return (r, peer, k, k2)
        stored[r] = True


def test_slot_simulator():
    """30-call sequences of all-reduce, reduce-scatter, all-gather, broadcast
    and reduce with random roots: no store ever lands on an unconsumed line of
    the same parity; without the token lines the same simulator finds one."""
    hazards = 0
    for s in range(200):
        rng = random.Random(9000 + s)
        n = rng.randint(2, 8)
        seq = [_call_plans(rng, n) for _ in range(30)]
        assert _simulate(n, seq) is None, (s, n)
        hazards += _simulate(n, seq, tokens=False) is not None
    assert hazards >= 1
