"""CPU tests of the two-hop direct ncclBroadcast / ncclReduce (host/plan.cc
select_algo, direct_rooted_max, direct_rooted_plan): the selection with its
opt-in threshold (vcclRootedAlgoEx), the geometry and data movement of the
step lists (vcclDirectRootedPlan) replayed with numpy, and a region-and-flag
simulator that runs random sequences of all five direct collectives on one
inbox under an adversarial scheduler (the inbox reuse rule of
device/direct.hpp).  No GPU needed."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import _ring
from vccl_amd import nccl

S = _ring.S
AR, RS, AG, BC, RED = 0, 1, 2, 3, 4
U8, F32 = 1, 7
NCH, SLOT = 14, 256 << 10


def region_of(chunk_bytes, n):
    """host/setup.cc: the inbox region of VCCL_DIRECT_CHUNK_BYTES = chunk_bytes."""
    return (chunk_bytes + n - 1) // n // 256 * 256 + 256


# ------------------------------------------------------------------ selection
BASE = dict(force=0, ll_slot=1 << 20, ll_max=64 << 10, ll_rsag_max=128 << 10, ll128=0, ll128_min=0, ll128_max=0,
            direct=1, direct_max=8 << 20, direct_rsag_max=8 << 20)


def test_threshold_zero_is_the_parent_selection():
    """With the direct threshold 0, vcclRootedAlgoEx answers exactly as
    vcclRootedAlgo for every policy, collective, size and rank count."""
    rng = random.Random(12)
    for _ in range(4000):
        pol = dict(force=rng.randrange(5), ll_slot=rng.choice([0, 4096, 1 << 20]),
                   ll_max=rng.choice([0, 4096, 64 << 10]), ll_rsag_max=rng.choice([0, 128 << 10]),
                   ll128=rng.randrange(2), ll128_min=rng.choice([0, 64 << 10]),
                   ll128_max=rng.choice([0, 1 << 20, 1 << 40]), direct=rng.randrange(2),
                   direct_max=rng.choice([0, 8 << 20]), direct_rsag_max=rng.choice([0, 8 << 20]))
        coll, dt = rng.randrange(5), rng.choice([1, 7, 9, 4])
        count = rng.choice([1, 17, 1000, 5000, 70_001, 1 << 20, 1 << 24])
        n = rng.choice([1, 2, 3, 4, 8, 9, 16])
        thr = rng.choice([0, 4096, 1 << 20])
        ll_allowed, any_net = rng.random() < 0.8, rng.random() < 0.2
        old = nccl.rooted_algo(coll, count, dt, n, pol, thr, ll_allowed, any_net)
        new = nccl.rooted_algo_ex(coll, count, dt, n, pol, thr, ll_allowed, any_net, 0, rng.random() < 0.5)
        assert new == (old[0], old[1], 0), (pol, coll, dt, count, n, thr)


@pytest.mark.parametrize("coll,dt,esz", [(BC, U8, 1), (RED, F32, 4)])
def test_selection_order(coll, dt, esz):
    """LL, then the LL128 window, then direct up to the threshold, then the ring."""
    pol = dict(BASE, ll128=1, ll128_min=128 << 10, ll128_max=1 << 20)
    want = [(1 << 10, "ll"), (64 << 10, "ll"), (100 << 10, "direct"), (128 << 10, "ll128"), (1 << 20, "ll128"),
            ((1 << 20) + 16, "direct"), (8 << 20, "direct"), ((8 << 20) + 16, "ring"), (64 << 20, "ring")]
    for nbytes, path in want:
        got = nccl.rooted_algo_ex(coll, nbytes // esz, dt, 4, pol, 64 << 10, True, False, 8 << 20, True)
        assert got == (path, 64 << 10, 8 << 20), (nbytes, got)
    # the other collectives never look at the rooted thresholds
    for c in (AR, RS, AG):
        for nbytes in (1 << 10, 1 << 20, 64 << 20):
            a = nccl.rooted_algo_ex(c, nbytes // 4, F32, 4, pol, 64 << 10, True, False, 8 << 20, True)[0]
            assert a == nccl.rooted_algo(c, nbytes // 4, F32, 4, pol, 64 << 10)[0]


@pytest.mark.parametrize("coll,dt,esz", [(BC, U8, 1), (RED, F32, 4)])
def test_forced_direct_only_when_opted_in(coll, dt, esz):
    pol = dict(BASE, force=3, ll128=1, ll128_min=128 << 10, ll128_max=1 << 20)
    for nbytes in (16, 512 << 10, 8 << 20, 1 << 30):
        assert nccl.rooted_algo_ex(coll, nbytes // esz, dt, 4, pol, 64 << 10, True, False, 4096, True)[0] == "direct"
        off = nccl.rooted_algo_ex(coll, nbytes // esz, dt, 4, pol, 64 << 10, True, False, 0, True)[0]
        assert off == nccl.rooted_algo(coll, nbytes // esz, dt, 4, pol, 64 << 10)[0] and off in ("ring", "ll128")
    # the other forces keep what they had, opted in or not
    for force in (1, 2, 4):
        p = dict(pol, force=force)
        for nbytes in (16, 512 << 10, 8 << 20):
            a = nccl.rooted_algo_ex(coll, nbytes // esz, dt, 4, p, 64 << 10, True, False, 8 << 20, True)[0]
            assert a == nccl.rooted_algo(coll, nbytes // esz, dt, 4, p, 64 << 10)[0]


def test_off_switches(monkeypatch):
    monkeypatch.delenv("VCCL_DIRECT_ROOTED_THRESHOLD", raising=False)
    monkeypatch.delenv("NCCL_DIRECT_ROOTED_THRESHOLD", raising=False)
    on = dict(direct_threshold=8 << 20)
    for coll, dt in ((BC, U8), (RED, F32)):
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 8, BASE, 0, **on) == ("direct", 0, 8 << 20)
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 8, BASE, 0)[0::2] == ("ring", 0)  # the environment: unset
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 8, dict(BASE, direct=0), 0, **on)[0::2] == ("ring", 0)
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 8, BASE, 0, direct_allowed=False, **on)[0::2] == ("ring", 0)
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 8, BASE, 0, any_net=True, **on)[0::2] == ("ring", 0)
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 9, BASE, 0, **on)[0::2] == ("ring", 0)
        assert nccl.rooted_algo_ex(coll, 1 << 18, dt, 1, BASE, 0, **on)[0] == "ring"
    monkeypatch.setenv("VCCL_DIRECT_ROOTED_THRESHOLD", "65536")
    assert nccl.rooted_algo_ex(BC, 65536, U8, 4, BASE, 0) == ("direct", 0, 65536)
    assert nccl.rooted_algo_ex(BC, 65537, U8, 4, BASE, 0)[0] == "ring"


# ------------------------------------------------------------------- geometry
def _plans(coll, n, root, count, dt, region, chunk):
    return [nccl.direct_rooted_plan(coll, n, r, root, count, dt, region, chunk) for r in range(n)]


@pytest.mark.parametrize("chunk_bytes", [64 << 10, 16 << 20])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("coll,dt,esz", [(BC, U8, 1), (RED, F32, 4), (RED, 9, 2)])
def test_geometry(coll, dt, esz, n, chunk_bytes):
    region = region_of(chunk_bytes, n)
    g = nccl.direct_rooted_plan(coll, n, 0, 0, 1 << 40, dt, region)
    full = g["chunk_elts"]
    shards = n if coll == RED else n - 1
    assert len(g["owners"]) == shards and full * esz <= shards * (region - 16)
    for count, root in ((2 * full + 4099, n - 1), (full, 0), (full + 1, 1), (5, 0)):
        n_chunks = -(-count // full)
        first_shard = None
        for c in range(n_chunks):
            plans = _plans(coll, n, root, count, dt, region, c)
            c0, cc = c * full * esz, min(full, count - c * full) * esz
            p0 = plans[0]
            assert p0["n_chunks"] == n_chunks and p0["chunk_elts"] == min(full, count)
            assert p0["owners"] == ([(root + 1 + j) % n for j in range(n - 1)] if coll == BC else list(range(n)))
            shard_b = p0["shard_elts"] * esz
            assert shard_b % 16 == 0 and shard_b <= region - 16        # each shard fits a region
            first_shard = first_shard or shard_b
            assert shard_b <= first_shard                               # a short chunk only empties high blocks ...
            for r in range(n):
                for st in plans[r]["steps"]:
                    if st[0] in ("store", "read"):                      # ... every shard starts its region
                        assert st[4] == 0 and st[6] <= shard_b
            # the shards tile the chunk exactly
            if coll == BC:
                cover = sorted((s[5], s[6]) for s in plans[root]["steps"] if s[0] == "store")
            else:
                cover = sorted((s[5], s[6]) for s in plans[root]["steps"] if s[0] in ("store", "local") and
                               (s[1] == 0 or s[7] == "fold"))
            pos = c0
            for off, nb in cover:
                assert off == pos or nb == 0
                pos += nb
            assert pos == c0 + cc
            # what r stores at p is byte for byte what p reads
            for r in range(n):
                for kind, ph, peer, reg, roff, uoff, nb, src in plans[r]["steps"]:
                    if kind != "store":
                        continue
                    assert reg == r and peer != r
                    q = plans[peer]["steps"]
                    if coll == RED and ph == 0:   # consumed by peer's fold of its own shard
                        folds = [s for s in q if s[7] == "fold"]
                        assert len(folds) == 1 and (folds[0][5], folds[0][6]) == (uoff, nb)
                        assert ("wait", 0, r) in [s[:3] for s in q[:q.index(folds[0])]]
                    else:
                        reads = [s for s in q if s[0] == "read" and (s[1], s[3]) == (ph, r)]
                        assert len(reads) == 1 and reads[0][4:7] == (roff, uoff, nb), (r, peer, ph)
                        assert ("wait", ph, r) in [s[:3] for s in q[:q.index(reads[0])]]


# ----------------------------------------------------------------------- data
def _fold(rank, root, n, inputs, inbox, lo, hi, op, dtype, chan, rings):
    dev_op, arg = O.host_to_dev_redop(op, dtype, n)
    pre = dev_op == O.DEV_PREMULSUM
    npdt = inputs[rank].dtype
    src = {q: inbox[rank][0, q][:(hi - lo) * npdt.itemsize].view(npdt) for q in range(n) if q != rank}
    src[rank] = inputs[rank][lo:hi]
    res = np.empty(hi - lo, npdt)
    ch = chan[lo:hi]
    for c in np.unique(ch):
        sel = np.nonzero(ch == c)[0]
        ring = rings[c % len(rings)]
        res[sel] = O.ring_fold(dev_op, dtype, arg, pre, [src[q][sel] for q in ring],
                               np.full(sel.size, ring.index(root), np.int32))
    return res


def _replay(coll, n, root, inputs, dtype, op, region):
    """Run the step lists of all ranks chunk by chunk (every rank steps until a
    wait blocks it).  inputs[r] is None where the kernel must not look (a
    broadcast non-root's sendbuff); outs[r] likewise (a reduce non-root's
    recvbuff).  Returns the outputs as bytes."""
    npdt = inputs[root].dtype
    esz = npdt.itemsize
    count = inputs[root].size
    dt = U8 if coll == BC else dtype
    nbytes = count * esz
    outs = [np.zeros(nbytes, np.uint8) if coll == BC or r == root else None for r in range(n)]
    chan = rings = None
    if coll == RED:
        chan = S.channel_of(_ring._sched("red", count, esz, n, NCH, SLOT, 512, S.PROTO_SIMPLE), count)
        rings = _ring.ring_orders(n)
    inbox = [dict() for _ in range(n)]
    flags = {}
    n_chunks = nccl.direct_rooted_plan(coll, n, 0, root, nbytes if coll == BC else count, dt, region)["n_chunks"]
    for c in range(n_chunks):
        progs = [p["steps"] for p in _plans(coll, n, root, nbytes if coll == BC else count, dt, region, c)]
        pc = [0] * n
        moved = True
        while moved:
            moved = False
            for r in range(n):
                while pc[r] < len(progs[r]):
                    kind, ph, peer, reg, roff, uoff, nb, src = progs[r][pc[r]]
                    if kind == "wait":
                        if flags.get((r, ph, peer)) != c + 1:
                            break
                    elif kind == "post":
                        for q in range(n):
                            if q != r:
                                flags[q, ph, r] = c + 1
                    elif kind in ("store", "local"):
                        if src == "send":
                            data = inputs[r].view(np.uint8)[uoff:uoff + nb]
                        elif src == "region":
                            data = inbox[r][0, root][roff:roff + nb]
                        else:
                            data = _fold(r, root, n, inputs, inbox, uoff // esz, (uoff + nb) // esz, op, dtype, chan,
                                         rings).view(np.uint8)
                        if kind == "store":
                            assert roff + nb <= region - 16
                            inbox[peer][ph, reg] = data.copy()
                        else:
                            outs[r][uoff:uoff + nb] = data
                    else:
                        outs[r][uoff:uoff + nb] = inbox[r][ph, reg][roff:roff + nb]
                    pc[r] += 1
                    moved = True
        assert all(pc[r] == len(progs[r]) for r in range(n)), "a rank is stuck on a flag nobody raises"
    return outs


COUNTS = (1, 5, 3_001, 100_003, 786_433)
TYPES = {"f32": (7, 0), "bf16": (9, 0), "u8": (1, 2), "i64": (4, 0)}  # dtype code, op of the reduce


def _inputs(name, n, count, seed):
    dtype, _ = TYPES[name]
    rng = np.random.default_rng(seed)
    if name == "bf16":
        return [O.f32_to_bf16_bits(rng.uniform(-1, 1, count).astype(np.float32)) for _ in range(n)]
    if name == "f32":
        return [rng.uniform(-1, 1, count).astype(np.float32) for _ in range(n)]
    return [rng.integers(0, 100, count).astype(O.NP_DTYPE[dtype]) for _ in range(n)]


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("name", list(TYPES))
def test_replay_matches_expected(name, n):
    dtype, op = TYPES[name]
    roots = range(n) if n == 3 else (0, n - 1) if name in ("f32", "u8") else (1, n // 2)
    for ci, count in enumerate(COUNTS):
        ins = _inputs(name, n, count, 100 * n + ci)
        region = region_of((64 << 10) if ci % 2 == 0 or count > 500_000 else (16 << 20), n)
        for root in roots:
            exp = _ring.expected_reduce(op, dtype, ins, root, NCH, SLOT, proto=S.PROTO_SIMPLE)
            outs = _replay(RED, n, root, ins, dtype, op, region)
            assert np.array_equal(outs[root], exp.view(np.uint8)), ("reduce", name, n, count, root)
            bins = [ins[r] if r == root else None for r in range(n)]
            outs = _replay(BC, n, root, bins, dtype, op, region)
            for r in range(n):
                assert np.array_equal(outs[r], ins[root].view(np.uint8)), ("broadcast", name, n, count, root, r)


# ------------------------------------------------------------------- protocol
# Programs of region and flag operations, one list per rank:
#   ("wait", phase, parity, from, epoch)      ("post", phase, parity, epoch)
#   ("store", peer, phase, parity, tag)       into region (phase, parity, me) of peer
#   ("read", phase, parity, region, tag)      my region (phase, parity, region)
# tag = (call, chunk): what the region must hold when it is read.
_STEP_CACHE = {}


def _rooted_steps(coll, n, rank, root):
    key = (coll, n, rank, root)
    if key not in _STEP_CACHE:
        dt = U8 if coll == BC else F32
        _STEP_CACHE[key] = nccl.direct_rooted_plan(coll, n, rank, root, 4096, dt, region_of(64 << 10, n), 0)["steps"]
    return _STEP_CACHE[key]


def _rooted_ops(coll, n, rank, root, e, tag, ack=True):
    """One chunk of a rooted call, from the library's own step list."""
    ops = []
    for kind, ph, peer, reg, roff, uoff, nb, src in _rooted_steps(coll, n, rank, root):
        if coll == BC and ph == 1 and not ack:
            continue  # the broken variant: no closing acknowledgement round
        if kind == "wait":
            ops.append(("wait", ph, 0, peer, e))
        elif kind == "post":
            ops.append(("post", ph, 0, e))
        elif kind == "read":
            ops.append(("read", ph, 0, reg, tag))
        elif kind == "store":
            if src == "region" and (not ops or ops[-1][0] != "store"):
                ops.append(("read", 0, 0, root, tag))
            if src == "fold":
                ops += [("read", 0, 0, q, tag) for q in range(n) if q != rank]
            ops.append(("store", peer, ph, 0, tag))
        elif src == "fold":  # the root's own fold
            ops += [("read", 0, 0, q, tag) for q in range(n) if q != rank]
    return ops


def _one_hop_ops(n, rank, e, tag):
    """direct_reducescatter_part / direct_allgather_part, one chunk: scatter,
    post 0, wait 0, read, post 1 (the acknowledgement), wait 1."""
    peers = [(rank + k) % n for k in range(1, n)]
    return ([("store", p, 0, 0, tag) for p in peers] + [("post", 0, 0, e)] +
            [("wait", 0, 0, p, e) for p in peers] + [("read", 0, 0, p, tag) for p in peers] +
            [("post", 1, 0, e)] + [("wait", 1, 0, p, e) for p in peers])


def _allreduce_ops(n, rank, e0, call, n_chunks):
    """direct_allreduce_part's phase order: chunks double-buffered by parity,
    chunk c+1's scatter issued after chunk c's fold and before its gather."""
    peers = [(rank + k) % n for k in range(1, n)]
    ops = [("store", p, 0, 0, (call, 0)) for p in peers] + [("post", 0, 0, e0 + 1)]
    for c in range(n_chunks):
        par, e, tag = c & 1, e0 + 1 + c, (call, c)
        ops += [("wait", 0, par, p, e) for p in peers] + [("read", 0, par, p, tag) for p in peers]
        ops += [("store", p, 1, par, tag) for p in peers] + [("post", 1, par, e)]
        if c + 1 < n_chunks:
            ops += [("store", p, 0, par ^ 1, (call, c + 1)) for p in peers] + [("post", 0, par ^ 1, e + 1)]
        ops += [("wait", 1, par, p, e) for p in peers] + [("read", 1, par, p, tag) for p in peers]
    return ops


def _programs(n, calls, ack=True):
    progs = [[] for _ in range(n)]
    e = 0
    for ci, (kind, root, n_chunks) in enumerate(calls):
        for r in range(n):
            if kind == AR:
                progs[r] += _allreduce_ops(n, r, e, ci, n_chunks)
            else:
                for c in range(n_chunks):
                    if kind in (RS, AG):
                        progs[r] += _one_hop_ops(n, r, e + 1 + c, (ci, c))
                    else:
                        progs[r] += _rooted_ops(kind, n, r, root, e + 1 + c, (ci, c), ack)
        e += n_chunks  # one epoch per chunk in every kernel
    return progs


def _simulate(n, progs, rng):
    """Run the programs under an adversarial scheduler.  Returns the first
    hazard: a store landing on a region whose earlier content its reader has
    not read yet, a read seeing the wrong content, a flag overwritten before
    its waiter saw it, or a rank stuck for good; None when every rank ends."""
    pending_reads = [dict() for _ in range(n)]   # rank -> region key -> [(pc, tag)]
    pending_waits = [dict() for _ in range(n)]   # rank -> flag key -> [(pc, epoch)]
    for r in range(n):
        for i, op in enumerate(progs[r]):
            if op[0] == "read":
                pending_reads[r].setdefault(op[1:4], []).append((i, op[4]))
            elif op[0] == "wait":
                pending_waits[r].setdefault(op[1:4], []).append((i, op[4]))
    region, flag, pc = {}, {}, [0] * n
    victim, mode = rng.randrange(n), rng.randrange(3)

    def step(r):
        op = progs[r][pc[r]]
        if op[0] == "wait":
            if flag.get((r,) + op[1:4]) != op[4]:
                return False
        elif op[0] == "post":
            _, ph, par, e = op
            for q in range(n):
                if q == r:
                    continue
                for i, we in pending_waits[q].get((ph, par, r), ()):
                    if i >= pc[q] and we < e:
                        return f"flag ({ph},{par},{r}) at {q} overwritten with {e} before its waiter saw {we}"
                flag[q, ph, par, r] = e
        elif op[0] == "store":
            _, peer, ph, par, tag = op
            for i, t in pending_reads[peer].get((ph, par, r), ()):
                if i >= pc[peer] and t < tag:
                    return f"store {tag} of {r} lands on region ({ph},{par},{r}) at {peer} before {t} was read"
            region[peer, ph, par, r] = tag
        else:
            _, ph, par, reg, tag = op
            if region.get((r, ph, par, reg)) != tag:
                return f"rank {r} reads {region.get((r, ph, par, reg))} in region ({ph},{par},{reg}), wants {tag}"
        pc[r] += 1
        return True

    def run(r, budget):
        moved = False
        while budget > 0 and pc[r] < len(progs[r]):
            res = step(r)
            if res is not True:
                return res if res else moved
            moved, budget = True, budget - 1
        return moved

    while any(pc[r] < len(progs[r]) for r in range(n)):
        order = list(range(n))
        rng.shuffle(order)
        if mode == 0:      # starve the victim: it moves only when nobody else can
            order = [r for r in order if r != victim]
        elif mode == 1:    # rush the victim as far as it gets, the others a step at a time
            order = [victim] + [r for r in order if r != victim]
        moved = False
        for r in order:
            budget = 1 << 30 if mode != 2 or rng.random() < 0.3 else rng.randrange(1, 6)
            if mode == 1 and r != victim:
                budget = rng.randrange(1, 4)
            res = run(r, budget)
            if isinstance(res, str):
                return res
            moved |= res
        if not moved:
            res = run(victim, rng.randrange(1, 8)) if mode == 0 else False
            if isinstance(res, str):
                return res
            if not res:
                return "stuck: " + str([progs[r][pc[r]] for r in range(n) if pc[r] < len(progs[r])][:4])
    return None


def _random_calls(rng, n, count=30):
    return [(rng.choice([AR, RS, AG, BC, RED]), rng.randrange(n), rng.randint(1, 3)) for _ in range(count)]


def test_any_order_of_the_five_kernels_reuses_one_inbox_safely():
    for seq in range(200):
        rng = random.Random(1000 + seq)
        n = rng.randint(2, 8)
        calls = _random_calls(rng, n)
        hazard = _simulate(n, _programs(n, calls), rng)
        assert hazard is None, (seq, n, calls, hazard)


def test_simulator_reports_the_missing_acknowledgement():
    """The same simulator, the broadcast's closing round removed: an owner one
    chunk ahead overwrites region (0, o) at a peer that still gathers."""
    n = 4
    calls = [(BC, 1, 3), (BC, 2, 3)]
    found = [_simulate(n, _programs(n, calls, ack=False), random.Random(s)) for s in range(12)]
    assert any(h and ("lands on region" in h or "overwritten" in h) for h in found), found
    assert all(_simulate(n, _programs(n, calls), random.Random(s)) is None for s in range(12))
    hits = 0
    for seq in range(200):
        rng = random.Random(1000 + seq)
        n = rng.randint(2, 8)
        calls = _random_calls(rng, n)
        hits += _simulate(n, _programs(n, calls, ack=False), rng) is not None
    assert hits > 0
