"""CPU tests of the zero-copy all-to-all's host half (host/plan.cc reg_a2a_max,
reg_a2a_eligible, reg_a2a_plan through vcclRegA2aMax / vcclRegA2aEligible /
vcclRegA2aPlan): the threshold and its off switches, the eligibility rule, the
step lists of one launch — every receive block tiled exactly once by the
workgroups' pulls, at the sender's displacements — all ranks' lists under an
adversarial scheduler, and the FIFO fallback: the p2p planner's lists with a
flagged call's items dropped on every rank still complete (the planner and the
FIFO simulator are tests/test_p2p_plan.py's).  No GPU needed."""
import ctypes
import random

import pytest

from tests import test_p2p_plan as P
from vccl_amd import nccl

T = 32768
SEND, RECV, COPY = nccl.P2P_SEND, nccl.P2P_RECV, nccl.P2P_COPY


# ------------------------------------------------------------------ threshold
def test_max_truth_table(monkeypatch):
    monkeypatch.delenv("VCCL_REG_A2A_THRESHOLD", raising=False)
    monkeypatch.delenv("NCCL_REG_A2A_THRESHOLD", raising=False)
    monkeypatch.setenv("VCCL_REG_THRESHOLD", "65536")  # the other path's knob switches nothing on here
    assert nccl.reg_a2a_max(None, nranks=4) == 0
    for inbox in (False, True):
        for direct in (False, True):
            for net in (False, True):
                for p2p in (False, True):
                    for regs in (False, True):
                        for n in (1, 2, 8, 9):
                            want = T if inbox and direct and not net and p2p and regs and 2 <= n <= 8 else 0
                            got = nccl.reg_a2a_max(T, inbox, direct, net, n, p2p, regs)
                            assert got == want, (inbox, direct, net, p2p, regs, n)
                            # 0 wherever reg_max gives 0
                            assert nccl.reg_max(T, inbox, direct, net, n) != 0 or got == 0
    assert nccl.reg_a2a_max(0, nranks=4) == 0
    assert nccl.reg_a2a_max(1 << 40, nranks=8) == 1 << 40  # no clamp: nothing to fit
    monkeypatch.setenv("VCCL_REG_A2A_THRESHOLD", "4096")
    assert nccl.reg_a2a_max(None, nranks=4) == 4096
    eff = ctypes.c_int64()
    assert nccl.lib().vcclRegA2aMax(T, 1, 1, 0, 0, 1, 1, ctypes.byref(eff)) == nccl.ncclInvalidArgument
    assert nccl.lib().vcclRegA2aMax(T, 1, 1, 0, 4, 1, 1, None) == nccl.ncclInvalidArgument


def test_eligibility():
    assert not nccl.reg_a2a_eligible(True, T - 1, T)
    assert nccl.reg_a2a_eligible(True, T, T) and nccl.reg_a2a_eligible(True, T + 1, T)
    assert nccl.reg_a2a_eligible(True, 1 << 40, T)            # no upper limit
    for b in (0, 1, T - 1, T):                                # every v-call: its size is part of the vote
        assert nccl.reg_a2a_eligible(False, b, T)
    assert not nccl.reg_a2a_eligible(True, 1 << 20, 0) and not nccl.reg_a2a_eligible(False, 1 << 20, 0)  # off
    for uniform in (True, False):                             # the 9th of a group takes today's path
        assert [nccl.reg_a2a_eligible(uniform, 1 << 20, T, i) for i in range(10)] == [True] * 8 + [False] * 2
    assert nccl.REG_A2A_MAX_CALLS == 8
    e = ctypes.c_int()
    L = nccl.lib()
    assert L.vcclRegA2aEligible(1, T, T, -1, ctypes.byref(e)) == nccl.ncclInvalidArgument
    assert L.vcclRegA2aEligible(1, T, -1, 0, ctypes.byref(e)) == nccl.ncclInvalidArgument
    assert L.vcclRegA2aEligible(1, T, T, 0, None) == nccl.ncclInvalidArgument


# ----------------------------------------------------------------------- plan
def random_matrix(rng, n):
    """Byte counts with zero pairs, a zero row and a zero column; send offsets
    per row in shuffled (non-monotonic) order with gaps; likewise receive offsets."""
    sizes = [0, 0, 1, 15, 16, 17, 40, 4096, 16384, 16385, 100_003, (1 << 20) + 3]
    sb = [[rng.choice(sizes) for _ in range(n)] for _ in range(n)]
    zr, zc = rng.randrange(n), rng.randrange(n)
    for p in range(n):
        sb[zr][p] = 0
        sb[p][zc] = 0

    def offsets(lengths):
        order = list(range(n))
        rng.shuffle(order)
        off, pos = [0] * n, rng.choice([0, 1, 4])
        for p in order:
            off[p] = pos
            pos += lengths[p] + rng.choice([0, 3, 16])
        return off
    so = [offsets(sb[r]) for r in range(n)]
    ro = [offsets([sb[p][r] for p in range(n)]) for r in range(n)]
    return sb, so, ro


def plans_of(n, sb, so, ro, uniform=False, **kw):
    return [nccl.reg_a2a_plan(n, r, sb, so, ro[r], uniform, **kw) for r in range(n)]


@pytest.mark.parametrize("n", range(2, 9))
def test_plan_tiles_every_receive_block(n):
    rng = random.Random(7000 + n)
    for trial in range(30):
        uniform = trial % 5 == 0
        if uniform:
            B = rng.choice([1, 40, T - 1, T, T + 1, (1 << 20) + 3])
            sb = [[B] * n for _ in range(n)]
            so = [[p * B for p in range(n)] for _ in range(n)]
            ro = [[p * B for p in range(n)] for _ in range(n)]
        else:
            sb, so, ro = random_matrix(rng, n)
        kw = rng.choice([{}, dict(min_ctas=4), dict(max_ctas=3), dict(direct_max_blocks=14), dict(max_ctas=200,
                                                                                                  direct_max_blocks=200)])
        plans = plans_of(n, sb, so, ro, uniform, **kw)
        grid = plans[0]["n_blocks"]
        assert all(pl["n_blocks"] == grid for pl in plans) and 1 <= grid <= 128   # one grid on every rank
        for r, pl in enumerate(plans):
            steps = pl["steps"]
            assert all(s[0] in nccl.REG_A2A_STEP_KINDS for s in steps)
            assert all(s[3] != r for s in steps if s[0] == "wait")
            moves = [s for s in steps if s[0] in ("pull", "self")]
            # the peers in the kernel's rotation, the self block last; nothing but posts touches a peer
            assert [s[3] for s in moves] == [(r + k) % n for k in range(1, n + 1)]
            assert [s[0] for s in moves] == ["pull"] * (n - 1) + ["self"]
            for kind, ep, ph, p, poff, ooff, nbytes, blk in moves:
                assert ep == 1
                assert nbytes == sb[p][r] and poff == so[p][r] and ooff == ro[r][p]  # the sender's displacement
                assert blk >= 16 and blk % 16 == 0
                # workgroup b pulls [b * blk, min((b + 1) * blk, bytes)): a tiling of the block by the grid
                slices = [(b * blk, min((b + 1) * blk, nbytes)) for b in range(grid)]
                covered = [x for x in slices if x[1] > x[0]]
                assert sum(hi - lo for lo, hi in covered) == nbytes
                assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
                assert not covered or (covered[0][0] == 0 and covered[-1][1] == nbytes)
            # the receive blocks do not overlap in my recvbuff
            spans = sorted((s[5], s[5] + s[6]) for s in moves if s[6] > 0)
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_plan_bad_arguments():
    L = nccl.lib()
    ns, nb = ctypes.c_int(), ctypes.c_int()
    st = (ctypes.c_int64 * 800)()

    def call(n=4, rank=0, uniform=0, min_ctas=1, max_ctas=64, dmb=64, cap=100, sizes=None, nbp=ctypes.byref(nb)):
        m = max(n, 1)
        mat = ctypes.c_size_t * (m * m)
        sb = mat(*(sizes or [100] * (m * m)))
        return L.vcclRegA2aPlan(n, rank, sb, mat(), (ctypes.c_size_t * m)(), uniform, min_ctas, max_ctas, dmb, nbp,
                                cap, ctypes.byref(ns), st)
    assert call() == nccl.ncclSuccess and ns.value == 21
    bad = nccl.ncclInvalidArgument
    assert call(n=1) == bad and call(n=9) == bad and call(rank=4) == bad and call(rank=-1) == bad
    assert call(min_ctas=-1) == bad and call(max_ctas=0) == bad and call(dmb=0) == bad and call(nbp=None) == bad
    assert call(uniform=1, sizes=[100] * 15 + [101]) == bad
    assert call(cap=3) == bad and ns.value == 21  # cap too small: the count is still reported


# ------------------------------------------------------------------ simulator
def simulate(n, sb, so, ro, rng, verdict):
    """All ranks' step lists together, one step of a random runnable rank at a
    time.  A flag is (epoch, phase, writer) at a reader; a wait blocks until its
    flag is up.  Checked as the steps run: a vote follows every peer's
    descriptor; a peer's block is read only after that peer's (0, 0) post of
    this launch was seen; a rank leaves only after every reader's close — no
    read of its sendbuff is still to come.  verdict 0: the lists end after
    epoch 0 (nothing is read)."""
    plans = [[s for s in pl["steps"] if verdict or s[1] == 0] for pl in plans_of(n, sb, so, ro)]
    pc = [0] * n
    flags, seen = set(), set()
    pending = {p: [] for p in range(n)}
    for r, steps in enumerate(plans):
        for s in steps:
            if s[0] == "pull" and s[6] > 0:
                pending[s[3]].append((r, s[4], s[6]))
    while any(pc[r] < len(plans[r]) for r in range(n)):
        ready = [r for r in range(n) if pc[r] < len(plans[r]) and
                 (plans[r][pc[r]][0] != "wait" or (plans[r][pc[r]][1], plans[r][pc[r]][2], plans[r][pc[r]][3], r) in flags)]
        assert ready, ("deadlock", n, [plans[r][pc[r]] for r in range(n) if pc[r] < len(plans[r])])
        r = rng.choice(ready)
        kind, epoch, phase, peer, poff, ooff, nbytes, blk = plans[r][pc[r]]
        if kind == "post":
            for q in range(n):
                if q != r:
                    assert (epoch, phase, r, q) not in flags  # raised once
                    flags.add((epoch, phase, r, q))
        elif kind == "wait":
            seen.add((epoch, phase, peer, r))
        elif kind == "vote":
            assert all((0, 0, q, r) in seen for q in range(n) if q != r), ("vote before a descriptor", r)
        elif kind == "pull" and nbytes > 0:
            assert (0, 0, peer, r) in seen and (0, 1, peer, r) in seen, ("read before ready", n, r, peer)
            assert 0 <= poff and poff == so[peer][r]
            pending[peer].remove((r, poff, nbytes))
        pc[r] += 1
        if pc[r] == len(plans[r]):
            assert not pending[r] or not verdict, ("left while a peer still reads", n, r, pending[r])
    rounds = 4 if verdict else 2
    assert len(flags) == rounds * n * (n - 1) and seen == flags


@pytest.mark.parametrize("n", range(2, 9))
def test_no_deadlock_no_read_before_ready(n):
    rng = random.Random(9000 + n)
    for _ in range(12):
        sb, so, ro = random_matrix(rng, n)
        for verdict in (1, 0):
            simulate(n, sb, so, ro, rng, verdict)


# ------------------------------------------------- the fallback through the FIFOs
def a2a_group(rng, n, parts):
    """A matched random group mixing plain sends and recvs with 1-3
    all-to-alls, each expanded as the API does (send p, recv p for every p).
    Returns per rank the calls and the indices flagged per all-to-all."""
    sizes = P.sizes_for(parts)
    big = max(sizes)  # more steps per part than a FIFO has slots

    def size(a, b, B):
        """A message of more than kSteps steps per part travels only from a
        lower to a higher rank.  A list cut into launches between a send and its
        round's recv blocks until the peer's later launch drains the FIFO; ranks
        exchanging such messages in one round (a cycle r -> r + d -> ... -> r, all
        items of one (sweep, round, part) key) then wait for each other — a
        property of today's cut lists with or without this feature (the plan
        with nothing dropped is today's), which a rank-ordered rule excludes:
        every such cycle has a descent."""
        return B if B != big or a < b else P.STEP

    calls, _ = P.random_group(rng, n, parts)
    calls = [[(k, p, size(r, p, B) if k == SEND else size(p, r, B), addr) for k, p, B, addr in c]
             for r, c in enumerate(calls)]
    flagged = [[] for _ in range(n)]
    addr = 0x7000_0000
    for a in range(rng.randint(1, 3)):
        mat = [[size(r, p, rng.choice(sizes)) for p in range(n)] for r in range(n)]
        front = rng.random() < 0.5  # ahead of or behind everything so far, alike on every rank (it is collective)
        for r in range(n):
            at = 0 if front else len(calls[r])
            block = []
            for p in range(n):
                addr += 0x200000
                block.append((SEND, p, mat[r][p], addr))
                block.append((RECV, p, mat[p][r], addr + 0x100000))
            calls[r][at:at] = block
            flagged[r] = [[i + len(block) if i >= at else i for i in f] for f in flagged[r]]
            flagged[r].append(list(range(at, at + len(block))))
    return calls, flagged


def run_dropping(monkeypatch, n, calls, parts, g_cap, max_works, drop):
    """tests/test_p2p_plan.py's simulator on the planner's lists, the items of
    the calls in drop[rank] turned into no-ops: a workgroup steps past a dropped
    item without touching a FIFO, which is what p2p_run's skip does (the item
    keeps its place in its launch and its workgroup's list).  The simulator's
    no-op is a zero-byte copy; the invariants are checked on the real list."""
    real_plan, real_check = P.plan, P.check_invariants

    def plan(rank, n_, calls_, parts_, **kw):
        items, n_wgs = real_plan(rank, n_, calls_, parts_, **kw)
        real_check(items, n_wgs)
        out = []
        for it in items:
            if it["call"] in drop[rank] or (it["kind"] == COPY and it["call2"] in drop[rank]):
                assert it["kind"] != COPY or (it["call"] in drop[rank] and it["call2"] in drop[rank])
                it = dict(it, kind=COPY, call2=it["call"], bytes=0, dropped=True)
            out.append(it)
        return out, n_wgs
    monkeypatch.setattr(P, "plan", plan)
    monkeypatch.setattr(P, "check_invariants", lambda items, n_wgs: None)
    try:
        return P.simulate(n, calls, parts, g_cap, max_works)
    finally:
        monkeypatch.setattr(P, "plan", real_plan)
        monkeypatch.setattr(P, "check_invariants", real_check)


def delivered(n, calls, skip):
    """{(src, dst, k): bytes} of the messages whose call is not in skip[rank]; k
    counts every send of src to dst, dropped ones included (the simulator's nth)."""
    want = {}
    for r in range(n):
        cnt = {}
        for i, c in enumerate(calls[r]):
            if c[0] != SEND:
                continue
            k = cnt.get(c[1], 0)
            cnt[c[1]] = k + 1
            if c[1] != r and c[2] and i not in skip[r]:
                want[r, c[1], k] = c[2]
    return want


def test_fifo_fallback_with_dropped_calls(monkeypatch):
    rng = random.Random(20261021)
    for g in range(100):
        n = 2 + g % 7
        parts = rng.choice([1, 2, 4, 8])
        calls, flagged = a2a_group(rng, n, parts)
        # which all-to-alls settled on zero-copy: the same on every rank (D is)
        verdicts = [rng.random() < 0.6 for _ in flagged[0]]
        drop = [{i for f, d in zip(flagged[r], verdicts) if d for i in f} for r in range(n)]
        none = [set() for _ in range(n)]
        for g_cap, max_works in ((1, 120), (2, 120), (0, 120), (0, 3), (2, 3)):
            got, _ = run_dropping(monkeypatch, n, calls, parts, g_cap, max_works, drop)
            assert got == delivered(n, calls, drop), (g, g_cap, max_works)
            # dropping none is today's plan, through the unpatched simulator
            got0, _ = P.simulate(n, calls, parts, g_cap, max_works)
            assert got0 == delivered(n, calls, none), (g, g_cap, max_works)


def test_python_surface():
    for m in ("reg_a2a_stats", "set_reg_a2a_threshold"):
        assert callable(getattr(nccl.Comm, m))
    for name in ("vcclRegA2aMax", "vcclRegA2aEligible", "vcclRegA2aPlan", "vcclCommRegA2aStats",
                 "vcclCommSetRegA2aThreshold"):
        assert name in nccl.EXPORTED and getattr(nccl.lib(), name).argtypes is not None
