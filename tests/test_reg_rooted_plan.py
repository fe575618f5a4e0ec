"""CPU checks of the zero-copy broadcast / reduce over registered buffers
(DESIGN.md 4.16): the threshold and the eligibility rule, that the existing
answers do not move, the step lists of host/plan.cc reg_rooted_plan (the
kernels' phase order), and two simulations — all ranks' lists together under an
adversarial scheduler on the user buffers, and random sequences mixing these
launches with the staged kernels' and the zero-copy AR / RS / AG lists on one
inbox and one flag array.  No GPU."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from tests.test_direct_rooted_plan import (_allreduce_ops, _one_hop_ops, _rooted_ops, _simulate,  # noqa: F401
                                           region_of)
from vccl_amd import nccl

AR, RS, AG, BC, RED = 0, 1, 2, 3, 4
U8, F32, BF16 = nccl.ncclUint8, nccl.ncclFloat32, nccl.ncclBfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32768


# ------------------------------------------------------- threshold, eligibility
def test_threshold_edges():
    for coll, dt, esz in ((BC, U8, 1), (RED, F32, 4), (BC, F32, 4), (RED, BF16, 2)):
        assert not nccl.reg_rooted_eligible(coll, T // esz - 1, dt, T)   # esz bytes below (u8: one byte)
        assert nccl.reg_rooted_eligible(coll, T // esz, dt, T)           # exactly at
        assert nccl.reg_rooted_eligible(coll, (1 << 40) // esz, dt, T)   # no upper limit
        assert not nccl.reg_rooted_eligible(coll, (1 << 40) // esz, dt, 0)  # off
        assert nccl.reg_rooted_eligible(coll, T // esz, dt, T, 0) and nccl.reg_rooted_eligible(coll, T // esz, dt, T, 1)
        assert not nccl.reg_rooted_eligible(coll, T // esz, dt, T, 2)    # a multi-collective group: today's path
    assert not nccl.reg_rooted_eligible(BC, T - 1, U8, T) and nccl.reg_rooted_eligible(BC, T, U8, T)
    L, out = nccl.lib(), ctypes.c_int()
    for coll in (AR, RS, AG, 5, -1):
        assert L.vcclRegRootedEligible(coll, T, U8, T, 0, ctypes.byref(out)) == nccl.ncclInvalidArgument
    assert L.vcclRegRootedEligible(BC, T, 99, T, 0, ctypes.byref(out)) == nccl.ncclInvalidArgument
    assert L.vcclRegRootedEligible(BC, T, U8, T, 0, None) == nccl.ncclInvalidArgument
    assert L.vcclRegRootedEligible(BC, T, U8, -1, 0, ctypes.byref(out)) == nccl.ncclInvalidArgument
    assert L.vcclRegRootedEligible(BC, T, U8, T, -1, ctypes.byref(out)) == nccl.ncclInvalidArgument


def test_off_switches_of_the_threshold():
    assert nccl.reg_rooted_max(T, nranks=4) == T
    assert nccl.reg_rooted_max(1 << 40, nranks=8) == 1 << 40  # no clamp
    assert nccl.reg_rooted_max(0, nranks=4) == 0
    assert nccl.reg_rooted_max(T, inbox=False, nranks=4) == 0
    assert nccl.reg_rooted_max(T, direct_allowed=False, nranks=4) == 0
    assert nccl.reg_rooted_max(T, any_net=True, nranks=4) == 0
    assert nccl.reg_rooted_max(T, nranks=1) == 0 and nccl.reg_rooted_max(T, nranks=9) == 0
    assert nccl.reg_rooted_max(T, nranks=2) == T and nccl.reg_rooted_max(T, nranks=8) == T
    assert nccl.reg_rooted_max(T, nranks=4, all_registries=False) == 0
    for kw in (dict(inbox=False), dict(direct_allowed=False), dict(any_net=True), dict(nranks=1), dict(nranks=9)):
        assert nccl.reg_max(T, **kw) == 0 == nccl.reg_rooted_max(T, **kw)  # 0 wherever reg_max gives 0


def _run(code, **env):
    e = dict(os.environ)
    for k in ("VCCL_REG_ROOTED_THRESHOLD", "NCCL_REG_ROOTED_THRESHOLD", "VCCL_REG_THRESHOLD", "NCCL_REG_THRESHOLD"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1])\n" + code, ROOT],
                       capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()[-1]


def test_threshold_from_the_environment():
    code = "from vccl_amd import nccl; print(nccl.reg_rooted_max(None, nranks=4), nccl.reg_max(None, nranks=4), sep=',')"
    assert _run(code, VCCL_REG_ROOTED_THRESHOLD="65536") == "65536,0"   # its own variable
    assert _run(code) == "0,0"                                          # the default: off
    assert _run(code, VCCL_REG_THRESHOLD="4096") == "0,4096"


_DIGEST = """
import hashlib, random
from vccl_amd import nccl
from tests.test_direct_rooted_plan import BASE
POL = dict(BASE, ll128=1, ll128_min=128 << 10, ll128_max=1 << 20)
rng, h = random.Random(77), hashlib.sha256()
for _ in range(3000):
    coll, dt = rng.randrange(5), rng.choice([1, 2, 4, 6, 7, 8, 9])
    count, n = rng.choice([1, 100, 8191, 8192, 8193, 1 << 20, rng.randrange(1, 1 << 26)]), rng.randint(1, 9)
    eff, g = rng.choice([0, 1, 32768, 1 << 20]), rng.randrange(3)
    row = [nccl.reg_eligible(coll, count, dt, n, eff, g),
           nccl.reg_max(rng.choice([None, 0, 32768]), bool(rng.randrange(2)), bool(rng.randrange(2)),
                        bool(rng.randrange(2)), n)]
    if coll >= 3:
        row.append(nccl.rooted_algo_ex(coll, count, dt, n, POL, rng.choice([0, 1 << 20]), True, False,
                                       rng.choice([0, 8 << 20]), True))
    h.update(repr(row).encode())
print(h.hexdigest())
"""


def test_existing_answers_unchanged():
    """vcclRegEligible, vcclRegMax and vcclRootedAlgoEx over 3000 random draws:
    the same with the new variable set as without it, and vcclRegEligible /
    vcclRegMax equal to their rule restated here."""
    rng = random.Random(5)
    for _ in range(3000):
        coll, dt = rng.randrange(5), rng.choice([U8, F32, BF16])
        esz = nccl.TYPE_SIZE[dt]
        count, n = rng.choice([1, 8191, 8192, 8193, rng.randrange(1, 1 << 24)]), rng.randint(1, 9)
        eff, g = rng.choice([0, 1, T, 1 << 20]), rng.randrange(3)
        nbytes = count * esz * (1 if coll == AR else n)
        want = eff > 0 and g <= 1 and coll in (AR, RS, AG) and nbytes >= eff
        assert nccl.reg_eligible(coll, count, dt, n, eff, g) == want
        flags = [bool(rng.randrange(2)) for _ in range(3)]
        thr = rng.choice([0, T])
        assert nccl.reg_max(thr, flags[0], flags[1], flags[2], n) == \
            (thr if flags[0] and flags[1] and not flags[2] and 2 <= n <= 8 else 0)
    if hasattr(nccl, "rooted_algo_ex"):
        assert _run(_DIGEST) == _run(_DIGEST, VCCL_REG_ROOTED_THRESHOLD="32768")


# ----------------------------------------------------------------- step lists
def bcast_counts(n):
    return sorted({1, 15, 16, 17, 16 * (n - 1) - 1, 16 * (n - 1) + 1, 4099, 65541})


RED_COUNTS = (1, 5, 4099, 70_001)
RED_TYPES = ((U8, 1), (BF16, 2), (F32, 4))


def region_for(nbytes, n, chunks):
    """A region size that cuts a reduce of nbytes into about `chunks` chunks."""
    return max(64, (-(-nbytes // chunks) // n + 16 + 255) // 256 * 256 + 16)


def covered_once(ranges, total):
    pos = 0
    for lo, ln in sorted(r for r in ranges if r[1] > 0):
        if lo != pos:
            return False
        pos = lo + ln
    return pos == total


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_broadcast_steps(n):
    for count in bcast_counts(n):
        for nb in (1, 3, 16):
            for root in range(n):
                plans = [nccl.reg_rooted_plan(BC, count, U8, n, r, root, region_of(64 << 10, n), nb) for r in range(n)]
                shard = -(-(-(-count // (n - 1))) // 16) * 16
                for r, pl in enumerate(plans):
                    st = pl["steps"]
                    assert pl["n_chunks"] == 1 and pl["blk_elts"] % 16 == 0 and pl["blk_elts"] * nb >= shard
                    assert all(s[0] in ("post", "wait", "copy") for s in st)   # nothing is written to a peer
                    assert {s[1] for s in st} == {0, 1}                        # two epoch positions
                    moves = [s for s in st if s[0] == "copy"]
                    for s in moves:
                        assert 0 <= s[5] and s[5] + s[7] <= count and s[5] == s[6]  # inside what the descriptor announced
                    if r == root:
                        assert all(s[3] == r and s[4] == "send" for s in moves)     # the local copy only
                    else:
                        # a non-root's sendbuff never appears: it reads the root's sendbuff, the others' recvbuffs
                        assert all(s[3] != r for s in moves)
                        assert all((s[4] == "send") == (s[3] == root) for s in moves)
                        own = direct_owner_shard(root, r, n)
                        assert [s for s in moves if s[3] == root] == \
                            [("copy", 1, 0, root, "send", min(own * shard, count), min(own * shard, count),
                              min((own + 1) * shard, count) - min(own * shard, count))]
                    assert covered_once([(s[6], s[7]) for s in moves], count), (n, count, root, r)
                    # what a peer pulls out of my recvbuff is exactly my own shard
                    for q, pq in enumerate(plans):
                        for s in pq["steps"]:
                            if s[0] == "copy" and s[3] == r and q != r and s[4] == "recv" and s[7] > 0:
                                mine = [m for m in moves if m[3] == root and m[4] == "send"]
                                assert r != root and (s[5], s[7]) == (mine[0][6], mine[0][7])


def direct_owner_shard(root, rank, n):
    return (rank - root - 1 + n) % n


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_reduce_steps(n):
    for dt, esz in RED_TYPES:
        for count in RED_COUNTS:
            for chunks in (1, 2, 3):
                region = region_for(count * esz, n, chunks) if chunks > 1 else region_of(16 << 20, n)
                for root in range(n):
                    for nb in (1, 3, 16):
                        plans = [nccl.reg_rooted_plan(RED, count, dt, n, r, root, region, nb) for r in range(n)]
                        staged = nccl.direct_rooted_plan(RED, n, 0, root, count, dt, region)
                        written = []   # the root's recvbuff
                        for r, pl in enumerate(plans):
                            st = pl["steps"]
                            assert (pl["n_chunks"], pl["chunk_elts"]) == (staged["n_chunks"], staged["chunk_elts"])
                            assert {s[1] for s in st} == set(range(1 + pl["n_chunks"]))   # 1 + nChunks positions
                            for ep in range(1, 1 + pl["n_chunks"]):
                                ch = [s for s in st if s[1] == ep]
                                folds = [s for s in ch if s[0] == "fold"]
                                assert sorted(s[3] for s in folds) == list(range(n))       # the n user inputs
                                assert len({(s[4], s[5], s[7]) for s in folds}) == 1 and folds[0][4] == "send"
                                assert 0 <= folds[0][5] and folds[0][5] + folds[0][7] <= count * esz
                                assert folds[0][7] <= region                               # the shard fits a region
                                stores = [s for s in ch if s[0] == "store_root"]
                                collects = [s for s in ch if s[0] == "collect"]
                                if r == root:
                                    assert not stores and all(s[6] == s[5] for s in folds)
                                    written.append((folds[0][6], folds[0][7]))
                                    written += [(s[6], s[7]) for s in collects]
                                    assert sorted(s[3] for s in collects) == [q for q in range(n) if q != r]
                                else:
                                    # nothing but flags and region (1, r) of the root is written to a peer; my
                                    # recvbuff never appears
                                    assert not collects and all(s[6] == -1 for s in folds)
                                    assert [(s[3], s[6], s[7]) for s in stores] == [(root, folds[0][5], folds[0][7])]
                                kinds = [s[0] for s in ch if s[0] != "wait"]
                                assert kinds[0] == "post" and kinds.index("fold") > 0
                                assert kinds.index("post", 1) > max(i for i, k in enumerate(kinds) if k != "collect"
                                                                      and k != "post")
                            assert all(s[4] == "send" for s in st)
                        assert covered_once(written, count * esz), (n, dt, count, chunks, root)
                        # a collect of shard o matches o's store
                        for o in range(n):
                            if o == root:
                                continue
                            so = [(s[1], s[6], s[7]) for s in plans[o]["steps"] if s[0] == "store_root"]
                            co = [(s[1], s[6], s[7]) for s in plans[root]["steps"] if s[0] == "collect" and s[3] == o]
                            assert so == co


def test_plan_rejects_bad_arguments():
    L = nccl.lib()
    ns, blk, ch, nc = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    st = (ctypes.c_int64 * 8000)()

    def call(coll, count, dt, n, rank, root, region, nb, cap=1000):
        return L.vcclRegRootedPlan(coll, count, dt, n, rank, root, region, nb, ctypes.byref(blk), ctypes.byref(ch),
                                   ctypes.byref(nc), cap, ctypes.byref(ns), st)
    assert call(BC, 100, U8, 4, 0, 0, 65536, 4) == 0
    for args in ((AR, 100, F32, 4, 0, 0, 65536, 4), (BC, 0, U8, 4, 0, 0, 65536, 4), (BC, 100, U8, 1, 0, 0, 65536, 4),
                 (BC, 100, U8, 9, 0, 0, 65536, 4), (BC, 100, U8, 4, 4, 0, 65536, 4), (BC, 100, U8, 4, 0, 4, 65536, 4),
                 (BC, 100, U8, 4, 0, 0, 65536, 0), (BC, 100, U8, 4, 0, 0, 65536, 129), (RED, 100, 99, 4, 0, 0, 65536, 4),
                 (RED, 100, F32, 4, 0, 0, 16, 4)):
        assert call(*args) == nccl.ncclInvalidArgument, args
    assert call(BC, 100, U8, 4, 0, 0, 65536, 4, cap=3) == nccl.ncclInvalidArgument and ns.value > 3


# ------------------------------------------- all ranks together, user buffers
def simulate(coll, n, root, count, dt, esz, region, in_place, rng, drop_close=False):
    """All ranks' step lists together, one step of a random runnable rank at a
    time (test_reg_plan.py's simulator with the rooted rules).  Returns the
    first hazard, None when every rank ends:
      * the root's sendbuff / a reduce input is read only after its owner's
        (0, 0) flag of this launch ("my input is ready") was seen;
      * a broadcast owner's shard of its recvbuff is read only after the
        reader saw the owner's (1, 0) flag, posted after the owner's pull;
      * no write lands under a reader still to come, in place included (the
        root's collect into a recvbuff that is its input);
      * no rank leaves while a peer still reads one of its buffers."""
    plans = [nccl.reg_rooted_plan(coll, count, dt, n, r, root, region, 4)["steps"] for r in range(n)]
    if drop_close:
        last = max(s[1] for s in plans[0])
        plans = [[s for s in p if not (s[1] == last and s[2] == 1)] for p in plans]
    pc, flags, seen = [0] * n, set(), set()
    pending = {p: [] for p in range(n)}
    for r, steps in enumerate(plans):
        for s in steps:
            if s[0] in ("fold", "copy") and s[3] != r and s[7] > 0:
                pending[s[3]].append((r, s[4], s[5], s[7]))

    def overlaps(a0, alen, b0, blen):
        return a0 < b0 + blen and b0 < a0 + alen

    while any(pc[r] < len(plans[r]) for r in range(n)):
        ready = [r for r in range(n) if pc[r] < len(plans[r]) and
                 (plans[r][pc[r]][0] != "wait" or plans[r][pc[r]][1:4] + (r,) in flags)]
        if not ready:
            return "deadlock"
        r = rng.choice(ready)
        kind, epoch, phase, peer, buf, poff, ooff, nb = plans[r][pc[r]]
        if kind == "post":
            flags.update((epoch, phase, r, q) for q in range(n) if q != r)
        elif kind == "wait":
            seen.add((epoch, phase, peer, r))
        elif kind in ("fold", "copy", "collect") and nb > 0:
            if kind != "collect" and peer != r:
                need = (0, 0, peer, r) if buf == "send" else (1, 0, peer, r)
                if need not in seen:
                    return f"read before ready: rank {r} {plans[r][pc[r]]}"
                pending[peer].remove((r, buf, poff, nb))
            skip = coll == BC and peer == r and in_place        # ncclBcast: the root copies nothing
            if ooff >= 0 and not skip:                           # a write into my recvbuff
                producing = coll == BC and kind == "copy" and peer == root and r != root
                for (q, b, lo, ln) in pending[r]:
                    if (b == "recv" or in_place) and not producing and overlaps(ooff, nb, lo, ln):
                        return f"write under a reader: rank {r} {plans[r][pc[r]]} vs rank {q}"
        pc[r] += 1
        if pc[r] == len(plans[r]) and pending[r]:
            return f"rank {r} left while a peer still reads its buffer"
    return None if seen == flags else "a flag nobody waited for"


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_no_hazard_on_the_user_buffers(n):
    rng = random.Random(4000 + n)
    for root in range(n):
        for in_place in (False, True):
            for count in bcast_counts(n):
                for _ in range(2):
                    assert simulate(BC, n, root, count, U8, 1, region_of(64 << 10, n), in_place, rng) is None
            for dt, esz in RED_TYPES:
                for count in RED_COUNTS:
                    for chunks in (1, 3):
                        region = region_for(count * esz, n, chunks) if chunks > 1 else region_of(16 << 20, n)
                        assert simulate(RED, n, root, count, dt, esz, region, in_place, rng) is None


def test_simulator_reports_the_missing_closing_round():
    """The broadcast's closing (1) round removed: an owner leaves while a peer
    still pulls its shard."""
    found = [simulate(BC, 4, s % 4, 65541, U8, 1, region_of(64 << 10, 4), False, random.Random(s), drop_close=True)
             for s in range(24)]
    assert any(h and "left while a peer still reads" in h for h in found), found
    assert all(simulate(BC, 4, s % 4, 65541, U8, 1, region_of(64 << 10, 4), False, random.Random(s)) is None
               for s in range(24))


# -------------------------------------------- mixed sequences, inbox and flags
ZC_BC, ZC_RED, FB_BC, FB_RED, ZC_AR = 10, 11, 12, 13, 14
_NEG = None


def _flag_ops(steps, n, rank, root, e0, call):
    """A zero-copy launch's region and flag operations from its step list:
    epoch word k is position e0 + 1 + k of the comm's sequence."""
    ops = []
    for kind, ep, ph, peer, buf, poff, ooff, nb in steps:
        e = e0 + 1 + ep
        if kind == "wait":
            ops.append(("wait", ph, 0, peer, e))
        elif kind == "post":
            ops.append(("post", ph, 0, e))
        elif kind == "store_root":
            ops.append(("store", peer, 1, 0, (call, ep)))
        elif kind == "collect":
            ops.append(("read", 1, 0, peer, (call, ep)))
    return ops


def _negotiation(n, rank, e):
    peers = [(rank + k) % n for k in range(1, n)]
    return ([("post", 0, 0, e)] + [("wait", 0, 0, p, e) for p in peers] + [("post", 1, 0, e)] +
            [("wait", 1, 0, p, e) for p in peers])


def _mixed_programs(n, calls):
    progs = [[] for _ in range(n)]
    e = 0
    for ci, (kind, root, n_chunks) in enumerate(calls):
        used = n_chunks
        for r in range(n):
            if kind == AR:
                progs[r] += _allreduce_ops(n, r, e, ci, n_chunks)
            elif kind in (RS, AG):
                for c in range(n_chunks):
                    progs[r] += _one_hop_ops(n, r, e + 1 + c, (ci, c))
            elif kind in (BC, RED):
                for c in range(n_chunks):
                    progs[r] += _rooted_ops(kind, n, r, root, e + 1 + c, (ci, c))
            elif kind in (FB_BC, FB_RED):  # negotiate, then the staged part
                progs[r] += _negotiation(n, r, e + 1)
                for c in range(n_chunks):
                    progs[r] += _rooted_ops(BC if kind == FB_BC else RED, n, r, root, e + 2 + c, (ci, c))
                used = 1 + n_chunks
            elif kind == ZC_AR:  # DESIGN 4.14's list: two positions
                progs[r] += _flag_ops(nccl.reg_plan(AR, 70_001, F32, n, r, 4)["steps"], n, r, root, e, ci)
                used = 2
            elif kind == ZC_BC:
                steps = nccl.reg_rooted_plan(BC, 65_541, U8, n, r, root, region_of(64 << 10, n), 4)["steps"]
                progs[r] += _flag_ops(steps, n, r, root, e, ci)
                used = 2
            else:
                region = region_for(70_001 * 4, n, n_chunks) if n_chunks > 1 else region_of(16 << 20, n)
                pl = nccl.reg_rooted_plan(RED, 70_001, F32, n, r, root, region, 4)
                progs[r] += _flag_ops(pl["steps"], n, r, root, e, ci)
                used = 1 + pl["n_chunks"]
        e += used
    return progs


def test_mixed_sequences_reuse_one_inbox_safely():
    """200 sequences of 30 calls mixing the two zero-copy rooted launches, their
    fallbacks, the staged kernels and the zero-copy all-reduce: no store on an
    unread region, no flag overwritten before its waiter saw it, nobody stuck."""
    kinds = [AR, RS, AG, BC, RED, ZC_BC, ZC_RED, FB_BC, FB_RED, ZC_AR]
    for seq in range(200):
        rng = random.Random(3000 + seq)
        n = rng.randint(2, 8)
        calls = [(rng.choice(kinds), rng.randrange(n), rng.randint(1, 3)) for _ in range(30)]
        hazard = _simulate(n, _mixed_programs(n, calls), rng)
        assert hazard is None, (seq, n, calls, hazard)


def test_python_surface():
    for m in ("reg_rooted_stats", "set_reg_rooted_threshold"):
        assert callable(getattr(nccl.Comm, m))
    for name in ("vcclRegRootedMax", "vcclRegRootedEligible", "vcclRegRootedPlan", "vcclCommRegRootedStats",
                 "vcclCommSetRegRootedThreshold"):
        assert name in nccl.EXPORTED and getattr(nccl.lib(), name).argtypes is not None
    assert nccl.REG_ROOTED_STEP_KINDS[4:] == ("store_root", "collect")
