"""CPU tests of the zero-copy direct path's host half (host/plan.cc reg_max,
reg_eligible, reg_plan through vcclRegMax / vcclRegEligible / vcclRegPlan): the
threshold and its off switches, the eligibility rule, and the step lists of one
zero-copy launch — coverage of inputs and outputs, nothing written to a peer,
and all ranks' lists run together under an adversarial scheduler: no deadlock,
no read of a buffer before its owner said it is ready, no write under a
reader, no rank leaving while a peer still reads it.  No GPU needed."""
import random

import pytest

from vccl_amd import nccl

AR, RS, AG, BC, RED = 0, 1, 2, 3, 4
U8, F32, BF16 = nccl.ncclUint8, nccl.ncclFloat32, nccl.ncclBfloat16
T = 32768


# ---------------------------------------------------------------- eligibility
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_threshold_edge_per_collective(n):
    """One byte below / at the threshold: AR count * esz, RS / AG nRanks * count * esz."""
    assert not nccl.reg_eligible(AR, T // 4 - 1, F32, n, T) and nccl.reg_eligible(AR, T // 4, F32, n, T)
    assert not nccl.reg_eligible(AR, T - 1, U8, n, T) and nccl.reg_eligible(AR, T, U8, n, T)
    for coll in (RS, AG):
        thr = n * 1000  # a threshold the n blocks can hit exactly
        assert nccl.reg_eligible(coll, 1000, U8, n, thr)
        assert not nccl.reg_eligible(coll, 1000, U8, n, thr + 1)
        assert nccl.reg_eligible(coll, 500, BF16, n, thr) and not nccl.reg_eligible(coll, 500, BF16, n, thr + 1)
    assert nccl.reg_eligible(AR, 1 << 28, F32, n, T)  # any size above: no upper limit


def test_only_ar_rs_ag_and_no_group_of_two():
    for coll in (BC, RED):
        assert not nccl.reg_eligible(coll, 1 << 20, F32, 4, T)
    for coll in (AR, RS, AG):
        assert nccl.reg_eligible(coll, 1 << 20, F32, 4, T, 0)
        assert nccl.reg_eligible(coll, 1 << 20, F32, 4, T, 1)   # a group of one
        assert not nccl.reg_eligible(coll, 1 << 20, F32, 4, T, 2)
        assert not nccl.reg_eligible(coll, 1 << 20, F32, 4, 0)  # threshold 0: off
    L = nccl.lib()
    import ctypes
    e = ctypes.c_int()
    assert L.vcclRegEligible(5, 1, F32, 4, T, 0, ctypes.byref(e)) == nccl.ncclInvalidArgument
    assert L.vcclRegEligible(AR, 1, 12, 4, T, 0, ctypes.byref(e)) == nccl.ncclInvalidArgument
    assert L.vcclRegEligible(AR, 1, F32, 4, T, 0, None) == nccl.ncclInvalidArgument


def test_off_switches(monkeypatch):
    monkeypatch.delenv("VCCL_REG_THRESHOLD", raising=False)
    monkeypatch.delenv("NCCL_REG_THRESHOLD", raising=False)
    assert nccl.reg_max(T, nranks=4) == T
    assert nccl.reg_max(None, nranks=4) == 0           # the environment: unset
    assert nccl.reg_max(0, nranks=4) == 0
    assert nccl.reg_max(T, inbox=False, nranks=4) == 0
    assert nccl.reg_max(T, direct_allowed=False, nranks=4) == 0
    assert nccl.reg_max(T, any_net=True, nranks=4) == 0
    assert nccl.reg_max(T, nranks=1) == 0 and nccl.reg_max(T, nranks=9) == 0
    assert nccl.reg_max(T, nranks=2) == T and nccl.reg_max(T, nranks=8) == T
    assert nccl.reg_max(1 << 40, nranks=8) == 1 << 40  # no clamp: the path has no inbox to fit


def test_threshold_from_the_environment():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VCCL_REG_THRESHOLD="65536")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1])\n"
                        "from vccl_amd import nccl; print(nccl.reg_max(None, nranks=4))", root],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1] == "65536", r.stderr


# ----------------------------------------------------------------------- plan
DTYPES = ((F32, 4), (BF16, 2), (U8, 1))


def counts_of(n):
    return sorted({1, n - 1, 4095, 4096, 4097, 1_000_003})


def sizes(coll, count, esz, n):
    """(bytes of a rank's sendbuff, bytes of its recvbuff)."""
    if coll == AR:
        return count * esz, count * esz
    return (n * count * esz, count * esz) if coll == RS else (count * esz, n * count * esz)


def covered_once(ranges, total):
    """Disjoint, and their union is [0, total)."""
    pos = 0
    for lo, ln in sorted(r for r in ranges if r[1] > 0):
        if lo != pos:
            return False
        pos = lo + ln
    return pos == total


@pytest.mark.parametrize("coll", [AR, RS, AG])
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_plan_data_movement(coll, n):
    for dt, esz in DTYPES:
        for count in counts_of(n):
            for nb in (1, 5, 16):
                plans = [nccl.reg_plan(coll, count, dt, n, r, nb) for r in range(n)]
                sbytes, rbytes = sizes(coll, count, esz, n)
                reads = {(p, b): [] for p in range(n) for b in ("send", "recv")}  # per source buffer
                for r, pl in enumerate(plans):
                    steps = pl["steps"]
                    moves = [s for s in steps if s[0] in ("fold", "copy")]
                    # every step is a post, a wait on a peer, or a read into MY recvbuff: nothing writes to a peer
                    assert all(s[0] in nccl.REG_STEP_KINDS for s in steps)
                    assert all(s[3] != r for s in steps if s[0] == "wait")
                    # the local writes cover the output exactly once (a fold's n sources write one range)
                    writes = {(s[6], s[7]) for s in moves if s[0] == "fold"}
                    assert len(writes) <= 1
                    assert covered_once(list(writes) + [(s[6], s[7]) for s in moves if s[0] == "copy"], rbytes), \
                        (coll, n, dt, count, r)
                    if coll != AG:  # a fold reads every rank once, own input included, all the same range
                        folds = [s for s in moves if s[0] == "fold"]
                        assert sorted(s[3] for s in folds) == list(range(n))
                        assert len({(s[4], s[5], s[6], s[7]) for s in folds}) == 1 and folds[0][4] == "send"
                    for s in moves:
                        assert 0 <= s[5] and s[5] + s[7] <= (sbytes if s[4] == "send" else rbytes)
                        reads[(s[3], s[4])].append((r, s[5], s[7]))
                    # geometry: nb blocks of blk_elts cover a shard, in whole 16-byte units
                    blk = pl["blk_elts"]
                    align = max(1, 16 // esz)
                    shard = {AR: -(-(-(-count // n)) // align) * align, RS: count, AG: count * esz}[coll]
                    assert blk * (1 if coll == AG else esz) % 16 == 0 and blk * nb >= shard
                    assert blk == pl["blk_elts"] == plans[0]["blk_elts"]
                for p in range(n):
                    if coll == AG:  # every block is read once per reader
                        assert sorted(x[0] for x in reads[(p, "send")]) == list(range(n))
                        assert all(x[1:] == (0, sbytes) for x in reads[(p, "send")])
                        assert not reads[(p, "recv")]
                        continue
                    # AR and RS: every input element is read exactly once across the ranks
                    assert covered_once([x[1:] for x in reads[(p, "send")]], sbytes), (coll, n, dt, count, p)
                    if coll == AR:  # the owner's shard of its recvbuff is pulled once by every other rank
                        own = [s for s in plans[p]["steps"] if s[0] == "fold"][0]
                        assert sorted(x[0] for x in reads[(p, "recv")] if x[2] > 0) == \
                            ([q for q in range(n) if q != p] if own[7] > 0 else [])
                        assert all(x[1:] == (own[6], own[7]) for x in reads[(p, "recv")])
                    else:
                        assert not reads[(p, "recv")]


def test_plan_rejects_other_collectives():
    import ctypes
    L = nccl.lib()
    ns, blk = ctypes.c_int(), ctypes.c_int64()
    st = (ctypes.c_int64 * 800)()
    for args in ((BC, 100, F32, 4, 0, 4), (AR, 0, F32, 4, 0, 4), (AR, 100, F32, 1, 0, 4), (AR, 100, F32, 9, 0, 4),
                 (AR, 100, F32, 4, 4, 4), (AR, 100, F32, 4, 0, 0), (AR, 100, F32, 4, 0, 129), (AR, 100, 12, 4, 0, 4)):
        assert L.vcclRegPlan(*args, ctypes.byref(blk), 100, ctypes.byref(ns), st) == nccl.ncclInvalidArgument, args
    assert L.vcclRegPlan(AR, 100, F32, 4, 0, 4, ctypes.byref(blk), 3, ctypes.byref(ns), st) == \
        nccl.ncclInvalidArgument and ns.value > 3  # cap too small: the count is still reported


# ------------------------------------------------------------------ simulator
def simulate(coll, n, count, dt, esz, in_place, rng):
    """All ranks' step lists together, one step of a random runnable rank at a
    time.  A flag is (epoch, phase, writer) at a reader; a wait blocks until
    its flag is up.  Buffer rules checked as the steps execute:
      * a peer's sendbuff is read only after that peer's (0, 0) flag of this
        launch ("my input is ready") was seen by the reader;
      * a peer's recvbuff (the all-reduce's pull) is read only after the reader
        saw the owner's (1, 0) flag, which the owner posted after its fold;
      * in place (sendbuff aliases recvbuff): a rank overwrites bytes of its
        buffer only once no peer's read of those bytes is still to come;
      * a rank finishes only after every peer's reads of its buffers are done."""
    plans = [nccl.reg_plan(coll, count, dt, n, r, 4)["steps"] for r in range(n)]
    sbytes, rbytes = sizes(coll, count, esz, n)
    # where the recvbuff sits inside the rank's sendbuff when the call is in place
    alias = {AR: lambda r: 0, RS: lambda r: r * rbytes, AG: lambda r: -r * sbytes}[coll] if in_place else None
    pc = [0] * n
    flags = set()       # (epoch, phase, writer, reader)
    seen = set()        # (epoch, phase, writer, reader): the reader passed its wait
    pending = {p: [] for p in range(n)}  # reads of p's buffers still to come: (reader, buf, lo, len)
    for r, steps in enumerate(plans):
        for s in steps:
            if s[0] in ("fold", "copy") and s[3] != r and s[7] > 0:
                pending[s[3]].append((r, s[4], s[5], s[7]))

    def overlaps(a0, alen, b0, blen):
        return a0 < b0 + blen and b0 < a0 + alen

    while any(pc[r] < len(plans[r]) for r in range(n)):
        ready = []
        for r in range(n):
            if pc[r] == len(plans[r]):
                continue
            s = plans[r][pc[r]]
            if s[0] != "wait" or (s[1], s[2], s[3], r) in flags:
                ready.append(r)
        assert ready, ("deadlock", coll, n, [plans[r][pc[r]] for r in range(n) if pc[r] < len(plans[r])])
        r = rng.choice(ready)
        kind, epoch, phase, peer, buf, poff, ooff, nb = plans[r][pc[r]]
        if kind == "post":
            for q in range(n):
                if q != r:
                    flags.add((epoch, phase, r, q))
        elif kind == "wait":
            seen.add((epoch, phase, peer, r))
        elif nb > 0 and not (coll == AG and in_place and peer == r):  # in place the kernel skips the own block
            if peer != r:
                need = (0, 0, peer, r) if buf == "send" else (1, 0, peer, r)
                assert need in seen, ("read before ready", coll, n, r, plans[r][pc[r]])
                pending[peer].remove((r, buf, poff, nb))
            # the write into my recvbuff [ooff, ooff + nb): no peer may still have to read those bytes
            for (q, b, lo, ln) in pending[r]:
                if b == "recv":  # the fold produces what they will read; later writes must stay clear of it
                    assert kind == "fold" or not overlaps(ooff, nb, lo, ln), ("write under a recvbuff reader", r)
                elif alias is not None:
                    # my sendbuff byte x is my recvbuff byte x - alias(r)
                    assert not overlaps(ooff + alias(r), nb, lo, ln), ("in-place write under a reader", coll, n, r, q)
        pc[r] += 1
        if pc[r] == len(plans[r]):
            assert not pending[r], ("left while a peer still reads", coll, n, r, pending[r])
    # every wait had its matching post, flags are raised once per (epoch, phase, writer, reader)
    assert len(flags) == 4 * n * (n - 1) and seen == flags


@pytest.mark.parametrize("coll", [AR, RS, AG])
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_no_deadlock_no_read_before_ready(coll, n):
    rng = random.Random(1000 * coll + n)
    for dt, esz in DTYPES:
        for count in counts_of(n):
            for in_place in (False, True):
                for _ in range(3):
                    simulate(coll, n, count, dt, esz, in_place, rng)


def test_python_surface():
    for m in ("register", "deregister", "reg_stats", "set_reg_threshold"):
        assert callable(getattr(nccl.Comm, m))
    for name in ("vcclRegMax", "vcclRegEligible", "vcclRegPlan", "vcclRegTableNew", "vcclCommRegStats",
                 "vcclCommSetRegThreshold"):
        assert name in nccl.EXPORTED and getattr(nccl.lib(), name).argtypes is not None
