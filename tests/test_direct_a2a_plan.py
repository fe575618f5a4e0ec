"""CPU checks of the one-hop direct all-to-all (host/plan.cc direct_a2a_max /
a2a_plan through vcclDirectA2aPlan): the per-pair limit with its clamp and off switches, the
parent's plan at limit 0, the three-way pair rule's symmetry between the two
ends, the launch rule, the comm-wide geometry, the residual sends and recvs as
a matched set for the p2p planner and its FIFO simulator, and the region-and-
flag simulator of tests/test_direct_rooted_plan.py run over sequences that mix
the all-to-all with the other five direct kernels.  No GPU call is made."""
import itertools
import random

import pytest

from tests.test_direct_rooted_plan import (AG, AR, BC, RED, RS, _allreduce_ops, _one_hop_ops, _rooted_ops,
                                           _simulate, region_of)
from tests.test_p2p_plan import RECV, SEND, simulate as fifo_simulate
from vccl_amd import nccl

FIFO, LL, DIRECT = nccl.A2A_FIFO, nccl.A2A_LL, nccl.A2A_DIRECT
A2A = 5                 # the sixth kind of the inbox simulator's call lists
REGION = region_of(1 << 20, 8)   # 131328: the 8-rank region of a 1 MiB chunk
LL_LIMIT = 512          # bytes per pair in the layout tests ...
LINES = LL_LIMIT // 8   # ... which is the whole LL slot
D_LIMIT = 40_000        # the direct limit of the layout tests
SIZES = (0, 1, 15, 16, 17, LL_LIMIT, LL_LIMIT + 1, 16_384, 16_385, D_LIMIT - 1, D_LIMIT, D_LIMIT + 1, 3 * D_LIMIT)


def blocks_of(m_bytes, min_ctas, max_ctas, direct_max_blocks):
    """The stated formula: ceil(M / 16 KiB), maxCTAs / minCTAs, then the caps last."""
    nb = -(-m_bytes // (16 << 10))
    nb = max(min(nb, max_ctas), min_ctas)
    nb = max(1, min(nb, direct_max_blocks, 128))
    blk = (-(-m_bytes // nb) + 15) // 16 * 16
    return -(-m_bytes // blk), blk


# ---------------------------------------------------------------- the limit
def test_direct_a2a_max_clamp_and_off_switches():
    cap = (REGION - 16) // 16 * 16
    assert cap == 131_312
    for thr in (1, 4096, 98_304, cap - 1, cap):
        assert nccl.direct_a2a_max(thr, REGION) == thr
    for thr in (cap + 1, 1 << 20, 1 << 40):
        assert nccl.direct_a2a_max(thr, REGION) == cap
    assert nccl.direct_a2a_max(1 << 20, 4111) == 4080  # (4111 - 16) rounded down to 16
    on = dict(threshold=98_304, region_bytes=REGION, direct_allowed=True, any_net=False, nranks=4, has_p2p=True)
    assert nccl.direct_a2a_max(**on) == 98_304
    # each off condition alone
    for off in (dict(threshold=0), dict(region_bytes=0), dict(direct_allowed=False), dict(any_net=True),
                dict(nranks=1), dict(nranks=9), dict(has_p2p=False)):
        assert nccl.direct_a2a_max(**dict(on, **off)) == 0, off
    for n in range(2, 9):
        assert nccl.direct_a2a_max(**dict(on, nranks=n)) == 98_304


def test_threshold_from_environment(monkeypatch):
    for k in ("VCCL_DIRECT_A2A_THRESHOLD", "NCCL_DIRECT_A2A_THRESHOLD"):
        monkeypatch.delenv(k, raising=False)
    assert nccl.direct_a2a_max(None, REGION) == 0  # the default is off
    monkeypatch.setenv("VCCL_DIRECT_A2A_THRESHOLD", "4096")
    assert nccl.direct_a2a_max(None, REGION) == 4096
    assert nccl.direct_a2a_max(None, 1040) == 1024
    # an explicit threshold never reads the environment
    assert nccl.direct_a2a_max(0, REGION) == 0
    assert nccl.direct_a2a_max(8192, REGION) == 8192
    # the LL all-to-all and the rooted direct thresholds are other knobs
    monkeypatch.delenv("VCCL_DIRECT_A2A_THRESHOLD")
    monkeypatch.setenv("VCCL_LL_A2A_THRESHOLD", "4096")
    monkeypatch.setenv("VCCL_DIRECT_ROOTED_THRESHOLD", "4096")
    assert nccl.direct_a2a_max(None, REGION) == 0


# ------------------------------------------------------- the parent at limit 0
def test_limit_zero_is_the_ll_plan():
    """With directA2aMax = 0 the LL bits, the launch flag and the residuals are
    vcclLLA2aPlan's, for uniform and v-calls, LL on or off."""
    rng = random.Random(31)
    for _ in range(2000):
        n = rng.randint(2, 8)
        ll_limit = rng.choice([0, LL_LIMIT])
        rank = rng.randrange(n)
        if rng.random() < 0.4:
            b = rng.choice(SIZES)
            send, recv, uniform = [b] * n, [b] * n, True
        else:
            send = [rng.choice(SIZES) for _ in range(n)]
            recv = [rng.choice(SIZES) for _ in range(n)]
            if rng.random() < 0.7:
                recv[rank] = send[rank]
            uniform = False
        old = nccl.ll_a2a_plan(n, rank, send, recv, uniform, ll_limit, LINES)
        new = nccl.direct_a2a_plan(n, rank, send, recv, uniform, ll_limit, 0, LINES, rng.choice([1, 4]),
                                   rng.choice([8, 64]), rng.choice([16, 64]))
        assert new["ll_launch"] == old["launch"] and not new["direct_launch"]
        assert [p == LL for p in new["send_path"]] == old["send_ll"]
        assert [p == LL for p in new["recv_path"]] == old["recv_ll"]
        assert DIRECT not in new["send_path"] + new["recv_path"]
        assert new["res_sends"] == old["res_sends"] and new["res_recvs"] == old["res_recvs"]
        assert (new["n_blocks"], new["blk_bytes"]) == (0, 0)


# ---------------------------------------------------------------- layout
def _matrix(rng, n):
    """bytes[r][p] of the ordered pair r -> p; self pairs symmetric by construction."""
    return [[rng.choice(SIZES) for _ in range(n)] for _ in range(n)]


def _plans(m, n, ll_limit=LL_LIMIT, d_limit=D_LIMIT, uniform=False, **bounds):
    return [nccl.direct_a2a_plan(n, r, m[r], [m[p][r] for p in range(n)], uniform, ll_limit, d_limit, LINES, **bounds)
            for r in range(n)]


def _path_of(b, ll_limit, d_limit):
    if ll_limit > 0 and b <= ll_limit:
        return LL
    return DIRECT if d_limit > 0 and b <= d_limit else FIFO


@pytest.mark.parametrize("n", range(2, 9))
def test_pair_symmetry(n):
    """r's sendPath[p] is p's recvPath[r] and is what the three-way rule gives
    B; the three paths partition the 2n sends and recvs of every rank; the
    launch flags are the same on every rank of a call."""
    rng = random.Random(5100 + n)
    for trial in range(50):
        m = _matrix(rng, n)
        ll_limit, d_limit = rng.choice([0, LL_LIMIT]), rng.choice([D_LIMIT, D_LIMIT, 16_384, 0])
        plans = _plans(m, n, ll_limit, d_limit)
        for r, p in itertools.product(range(n), range(n)):
            want = _path_of(m[r][p], ll_limit, d_limit)
            assert plans[r]["send_path"][p] == want == plans[p]["recv_path"][r], (trial, r, p, m[r][p])
        for r, pl in enumerate(plans):
            assert set(pl["send_path"] + pl["recv_path"]) <= {FIFO, LL, DIRECT}
            assert pl["res_sends"] == [p for p in range(n) if pl["send_path"][p] == FIFO]
            assert pl["res_recvs"] == [p for p in range(n) if pl["recv_path"][p] == FIFO]
            # a v-call: each launch iff its limit is on, whatever the row and column hold
            assert pl["ll_launch"] == (ll_limit > 0) and pl["direct_launch"] == (d_limit > 0), (trial, r)
        assert len({(pl["ll_launch"], pl["direct_launch"], pl["n_blocks"], pl["blk_bytes"]) for pl in plans}) == 1


@pytest.mark.parametrize("n", range(2, 9))
def test_launch_rule(n):
    for b, ll_limit in itertools.product(SIZES, (0, LL_LIMIT)):
        m = [[b] * n for _ in range(n)]
        ll = 0 < b <= ll_limit
        direct = not ll and 0 < b <= D_LIMIT
        path = LL if ll else DIRECT if direct else FIFO
        for pl in _plans(m, n, ll_limit, uniform=True):
            # uniform: one LL launch, or one direct launch, and nothing else; or today's path untouched
            assert (pl["ll_launch"], pl["direct_launch"]) == (ll, direct), (b, ll_limit)
            assert pl["send_path"] == [path] * n == pl["recv_path"]
            assert pl["res_sends"] == ([] if ll or direct else list(range(n))) == pl["res_recvs"]
            assert (pl["n_blocks"], pl["blk_bytes"]) == (blocks_of(b, 1, 64, 64) if direct else (0, 0))
    # v: one direct launch on every rank, even one whose row and column hold no direct pair
    m = [[8_000] * n for _ in range(n)]
    for p in range(n):
        m[0][p] = m[p][0] = 3 * D_LIMIT
    plans = _plans(m, n, 0)
    assert all(pl["direct_launch"] and not pl["ll_launch"] for pl in plans)
    assert plans[0]["res_sends"] == list(range(n)) == plans[0]["res_recvs"]
    assert plans[1]["send_path"] == [FIFO] + [DIRECT] * (n - 1)
    # without a direct launch no pair is direct
    assert all(DIRECT not in pl["send_path"] + pl["recv_path"] for pl in _plans(m, n, 0, 0))


def test_self_block():
    """LL as the LL rule has it; else direct when both lengths agree and fit;
    else a FIFO-launch copy (or its refusal)."""
    n, r = 4, 2
    for s, q, ll_limit, want in ((100, 100, LL_LIMIT, LL), (100, 100, 0, DIRECT), (D_LIMIT, D_LIMIT, LL_LIMIT, DIRECT),
                                 (D_LIMIT + 1, D_LIMIT + 1, LL_LIMIT, FIFO), (100, 600, LL_LIMIT, FIFO),
                                 (600, 700, LL_LIMIT, FIFO), (0, 0, 0, DIRECT), (0, 0, LL_LIMIT, LL)):
        send, recv = [1000] * n, [1000] * n
        send[r], recv[r] = s, q
        pl = nccl.direct_a2a_plan(n, r, send, recv, False, ll_limit, D_LIMIT, LINES)
        assert (pl["send_path"][r], pl["recv_path"][r]) == (want, want), (s, q, ll_limit)


# ---------------------------------------------------------------- geometry
@pytest.mark.parametrize("n", range(2, 9))
def test_geometry_is_comm_wide(n):
    """A v-call's grid and block length come from the limit alone: identical on
    every rank whatever its row and column; a uniform call's come from B.  The
    blocks tile [0, M) exactly once in 16-byte multiples."""
    rng = random.Random(5300 + n)
    for trial in range(50):
        d_limit = rng.choice([17, 4096, 16_384, 16_385, 49_153, 98_304, 131_312, 2_097_392])
        bounds = dict(min_ctas=rng.choice([1, 1, 4, 40]), max_ctas=rng.choice([2, 32, 64]),
                      direct_max_blocks=rng.choice([1, 16, 28, 64, 1000]))
        sizes = (0, 1, d_limit // 2, d_limit, d_limit + 1)
        m = [[rng.choice(sizes) for _ in range(n)] for _ in range(n)]
        plans = _plans(m, n, rng.choice([0, 16]), d_limit, **bounds)
        want = blocks_of(d_limit, **bounds)
        assert all((pl["n_blocks"], pl["blk_bytes"]) == want for pl in plans), (trial, d_limit, bounds)
        b = rng.choice([1, 15, 16, 17, 16_384, 16_385, 49_153, d_limit])
        if b <= d_limit:
            for pl in _plans([[b] * n] * n, n, 0, d_limit, uniform=True, **bounds):
                assert (pl["n_blocks"], pl["blk_bytes"]) == blocks_of(b, **bounds), (trial, b, bounds)
        for m_bytes in (d_limit, b):
            nb, blk = blocks_of(m_bytes, **bounds)
            assert blk % 16 == 0 and nb >= 1 and (nb - 1) * blk < m_bytes <= nb * blk
            spans = [(i * blk, min(m_bytes, (i + 1) * blk)) for i in range(nb)]
            assert spans[0][0] == 0 and spans[-1][1] == m_bytes
            assert all(a[1] == c[0] and a[0] < a[1] for a, c in zip(spans, spans[1:]))


def test_geometry_caps_in_order():
    """maxCTAs, then minCTAs, then directMaxBlocks and the 128-block ceiling last."""
    def geo(m_bytes, **bounds):
        pl = nccl.direct_a2a_plan(2, 0, [m_bytes] * 2, [m_bytes] * 2, True, 0, 1 << 30, LINES, **bounds)
        return pl["n_blocks"], pl["blk_bytes"]
    assert geo(49_153) == (4, 12_304)       # 4 blocks of 12,304; the last one 12,241
    assert 49_153 - 3 * 12_304 == 12_241
    assert geo(98_304) == (6, 16_384)
    assert geo(1 << 20) == (64, 16_384)
    assert geo(1 << 20, max_ctas=4) == (4, 1 << 18)                                   # maxCTAs
    assert geo(16_384, min_ctas=8) == (8, 2048)                                       # minCTAs over the size
    assert geo(1 << 20, min_ctas=8, max_ctas=4) == (8, 1 << 17)                       # minCTAs after maxCTAs
    assert geo(16_384, min_ctas=32, direct_max_blocks=16) == (16, 1024)               # the cap after minCTAs
    assert geo(8 << 20, min_ctas=500, max_ctas=1000, direct_max_blocks=1000) == (128, 1 << 16)  # the ceiling
    assert geo(1) == (1, 16) and geo(17, min_ctas=8) == (2, 16)  # 16-byte blocks: fewer than asked for


# ---------------------------------------------------------------- residuals
@pytest.mark.parametrize("n", range(2, 9))
def test_residuals_are_a_matched_set(n):
    """Every rank's residual sends and recvs, as calls of the p2p planner in
    the expansion order: vcclP2pPlan accepts them, each residual send has its
    recv of the same bytes at the other end, and the FIFO simulator of
    tests/test_p2p_plan.py completes and delivers exactly those bytes."""
    rng = random.Random(5200 + n)
    for trial in range(20):
        m = _matrix(rng, n)
        ll_limit = rng.choice([0, LL_LIMIT])
        plans = _plans(m, n, ll_limit)
        sends = {(r, p, m[r][p]) for r in range(n) for p in plans[r]["res_sends"]}
        recvs = {(p, r, m[p][r]) for r in range(n) for p in plans[r]["res_recvs"]}
        assert sends == recvs == {(r, p, m[r][p]) for r in range(n) for p in range(n) if m[r][p] > D_LIMIT}
        calls, addr = [], 0x1000
        for r in range(n):
            mine = []
            for p in range(n):  # the expansion order: send p, recv p
                addr += 0x200000
                if p in plans[r]["res_sends"]:
                    mine.append((SEND, p, m[r][p], addr))
                if p in plans[r]["res_recvs"]:
                    mine.append((RECV, p, m[p][r], addr + 0x100000))
            calls.append(mine)
        got, copied = fifo_simulate(n, calls, 2, rng.choice([0, 1, 2]), rng.choice([3, 120]))
        assert got == {(r, p, 0): b for r, p, b in sends if r != p}, trial
        assert copied == {(r, 0): b for r, p, b in sends if r == p}, trial


# ---------------------------------------------------------------- inbox reuse
def _a2a_ops(n, rank, pl, e, tag, ack=True):
    """direct_alltoall's phase order: a store per direct send, post 0, wait 0 on
    every peer, a read per direct recv, post 1 (the acknowledgement), wait 1 on
    every peer — flags to and from every peer whatever moves."""
    peers = [(rank + k) % n for k in range(1, n)]
    ops = [("store", p, 0, 0, tag) for p in peers if pl["send_path"][p] == DIRECT]
    ops += [("post", 0, 0, e)] + [("wait", 0, 0, p, e) for p in peers]
    ops += [("read", 0, 0, p, tag) for p in peers if pl["recv_path"][p] == DIRECT]
    if ack:
        ops += [("post", 1, 0, e)] + [("wait", 1, 0, p, e) for p in peers]
    return ops


def _a2a_plans(rng, n):
    limit = 4096
    if rng.random() < 0.3:
        return _plans([[rng.choice([1, 100, limit])] * n] * n, n, 0, limit, uniform=True)
    m = [[rng.choice([0, 1, limit - 1, limit, limit + 1, 3 * limit]) for _ in range(n)] for _ in range(n)]
    return _plans(m, n, rng.choice([0, 16]), limit)


def _programs(n, calls, ack=True):
    """tests/test_direct_rooted_plan.py _programs with the sixth kind: calls =
    [(kind, root, chunks or the all-to-all's per-rank plans)]."""
    progs = [[] for _ in range(n)]
    e = 0
    for ci, (kind, root, arg) in enumerate(calls):
        n_chunks = 1 if kind == A2A else arg
        for r in range(n):
            if kind == A2A:
                progs[r] += _a2a_ops(n, r, arg[r], e + 1, (ci, 0), ack)
            elif kind == AR:
                progs[r] += _allreduce_ops(n, r, e, ci, n_chunks)
            else:
                for c in range(n_chunks):
                    if kind in (RS, AG):
                        progs[r] += _one_hop_ops(n, r, e + 1 + c, (ci, c))
                    else:
                        progs[r] += _rooted_ops(kind, n, r, root, e + 1 + c, (ci, c))
        e += n_chunks  # one epoch per chunk in every kernel, one chunk per all-to-all
    return progs


def _random_calls(rng, n, count=30):
    calls = []
    for _ in range(count):
        kind = rng.choice([AR, RS, AG, BC, RED, A2A, A2A])
        calls.append((kind, rng.randrange(n), _a2a_plans(rng, n) if kind == A2A else rng.randint(1, 3)))
    return calls


def test_any_order_of_the_six_kernels_reuses_one_inbox_safely():
    for seq in range(200):
        rng = random.Random(9000 + seq)
        n = rng.randint(2, 8)
        calls = _random_calls(rng, n)
        assert any(c[0] == A2A for c in calls)
        hazard = _simulate(n, _programs(n, calls), rng)
        assert hazard is None, (seq, n, [c[:2] for c in calls], hazard)


def test_simulator_reports_the_missing_acknowledgement():
    """The same simulator, the all-to-all's acknowledgement round removed: a
    rank one call ahead overwrites region (0, r) at a peer that still collects."""
    n = 4
    full = [[10_000 if r != p else 0 for p in range(n)] for r in range(n)]
    calls = [(A2A, 0, _plans(full, n, 0, 16_384)) for _ in range(3)]
    found = [_simulate(n, _programs(n, calls, ack=False), random.Random(s)) for s in range(12)]
    assert any(h and ("lands on region" in h or "overwritten" in h) for h in found), found
    assert all(_simulate(n, _programs(n, calls), random.Random(s)) is None for s in range(12))
    hits = 0
    for seq in range(200):
        rng = random.Random(9000 + seq)
        n = rng.randint(2, 8)
        calls = _random_calls(rng, n)
        hits += _simulate(n, _programs(n, calls, ack=False), rng) is not None
    assert hits > 0
