"""CPU checks of the point-to-point planner (vcclP2pPlan, host/plan.cc): the
round pairing, the message split both ends agree on (I3), and a simulator
that runs every rank's plan against FIFOs of kSteps slots — one connection
direction per workgroup (I1), items in increasing (sweep, round, part) order
(I2), every run completes and every recv gets its matching send's bytes, for
one, two and unbounded workgroups per direction and with the list cut into
launches of three items.  No GPU call is made."""
import ctypes
import os
import random
import re

import pytest

from vccl_amd import nccl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_STEPS = 8
STEP = 4096
MIN_PART = 4096
SEND, RECV, COPY = nccl.P2P_SEND, nccl.P2P_RECV, nccl.P2P_COPY


def sizes_for(parts, min_part=MIN_PART, step=STEP):
    return [0, 1, 15, 16, 17, min_part - 1, min_part, min_part + 1, parts * min_part + 5, 3 * K_STEPS * step + 7]


def plan(rank, n, calls, parts, **kw):
    kw.setdefault("min_part_bytes", MIN_PART)
    kw.setdefault("step_bytes", STEP)
    return nccl.p2p_plan(rank, n, calls, parts=parts, **kw)


# ---------------------------------------------------------------- pairing
@pytest.mark.parametrize("n", range(1, 9))
def test_round_pairing(n):
    """Round d pairs "send to (r + d) mod n" with "recv from (r - d) mod n":
    per rank both are permutations, and send(r, d) = s <=> recv(s, d) = r."""
    send_of, recv_of = {}, {}
    for r in range(n):
        calls = [(SEND, p, 64) for p in range(n)] + [(RECV, p, 64) for p in range(n)]
        items, _ = plan(r, n, calls, 1)
        for it in items:
            if it["kind"] == COPY:
                assert it["round"] == 0 and it["peer"] == r
                send_of[r, 0] = recv_of[r, 0] = r
            elif it["kind"] == SEND:
                assert (r, it["round"]) not in send_of
                send_of[r, it["round"]] = it["peer"]
            else:
                assert (r, it["round"]) not in recv_of
                recv_of[r, it["round"]] = it["peer"]
    for r in range(n):
        assert sorted(send_of[r, d] for d in range(n)) == list(range(n))
        assert sorted(recv_of[r, d] for d in range(n)) == list(range(n))
        for d in range(n):
            assert send_of[r, d] == (r + d) % n and recv_of[r, d] == (r - d) % n
            assert recv_of[send_of[r, d], d] == r


# ---------------------------------------------------------------- the split
@pytest.mark.parametrize("parts", [1, 2, 4, 8])
def test_split_agreement(parts):
    """I3: the split of B bytes depends on B and the comm-wide constants only
    — the same for the sender and the receiver at any rank pair; part lengths
    are multiples of 16 except the last and sum to B; ceil(len / step) steps."""
    n = 4
    for B in sizes_for(parts):
        seen = set()
        for r in range(n):
            for p in range(n):
                if p == r:
                    continue
                for kind in (SEND, RECV):
                    items, _ = plan(r, n, [(kind, p, B)], parts)
                    assert all(it["kind"] == kind and it["peer"] == p and it["sweep"] == 0 for it in items)
                    seen.add(tuple((it["part"], it["offset"], it["bytes"], it["steps"]) for it in items))
        assert len(seen) == 1, (B, seen)
        split = seen.pop()
        want_parts = max(1, min(parts, -(-B // MIN_PART))) if B else 0
        assert len(split) == want_parts, (B, split)
        off = 0
        for q, (part, o, ln, steps) in enumerate(split):
            assert part == q and o == off and ln > 0
            assert ln % 16 == 0 or q == len(split) - 1
            assert steps == -(-ln // STEP)
            off += ln
        assert off == B
        if split:  # alignUp(ceil(B / p), 16)
            assert split[0][2] == min(B, (-(-B // want_parts) + 15) // 16 * 16)


# ---------------------------------------------------------------- simulator
def random_group(rng, n, parts):
    """Per rank its calls (kind, peer, bytes, buffer) in a random call order
    that keeps the per-peer order; and per ordered pair the message sizes."""
    sizes = sizes_for(parts)
    msgs = {}
    for a in range(n):
        for b in range(n):
            k = rng.choice([0, 0, 0, 1, 1, 2, 3])
            msgs[a, b] = [rng.choice(sizes) for _ in range(k)]
    calls = []
    addr = 0x1000
    for r in range(n):
        mine = []
        for p in range(n):
            for B in msgs[r, p]:
                addr += 0x100000
                mine.append([SEND, p, B, addr])
            for B in msgs[p, r]:
                addr += 0x100000
                mine.append([RECV, p, B, addr])
        # a self pair in place: the same buffer on both calls
        ss = [c for c in mine if c[0] == SEND and c[1] == r]
        rr = [c for c in mine if c[0] == RECV and c[1] == r]
        for s, q in zip(ss, rr):
            if rng.random() < 0.3:
                q[3] = s[3]
        # shuffle, then restore the per-(kind, peer) order
        order = list(range(len(mine)))
        rng.shuffle(order)
        by_key = {}
        for c in mine:
            by_key.setdefault((c[0], c[1]), []).append(c)
        shuffled = []
        for i in order:
            key = (mine[i][0], mine[i][1])
            shuffled.append(by_key[key].pop(0))
        calls.append([tuple(c) for c in shuffled])
    return calls, msgs


def check_invariants(items, n_wgs):
    owner = {}
    last = {}
    for it in items:
        wg, kind = it["wg"], it["kind"]
        assert 0 <= wg < 2 * n_wgs
        assert (wg >= n_wgs) == (kind == RECV)          # direction split
        if kind != COPY:                                # I1
            conn = (kind, it["peer"], it["part"])
            assert owner.setdefault(conn, wg) == wg, conn
        key = (it["sweep"], it["round"], it["part"])   # I2
        assert last.get(wg, (-1, -1, -1)) < key, (wg, key)
        last[wg] = key
    assert [it["launch"] for it in items] == sorted(it["launch"] for it in items)


def simulate(n, calls, parts, g_cap, max_works):
    """Runs every rank's launches in order; per tick each workgroup of each
    rank's current launch moves at most one step.  Returns the messages
    delivered as {(src, dst, k): bytes}."""
    plans = []
    for r in range(n):
        items, n_wgs = plan(r, n, calls[r], parts, g_cap=g_cap, max_works=max_works)
        check_invariants(items, n_wgs)
        assert max((it["launch"] for it in items), default=-1) == (len(items) - 1) // max_works
        assert all(sum(1 for it in items if it["launch"] == L) <= max_works for L in {it["launch"] for it in items})
        plans.append(items)
    # the k-th send of a to b / recv of b from a, by call index
    nth = []
    for r in range(n):
        cnt, m = {}, {}
        for i, c in enumerate(calls[r]):
            key = (c[0], c[1])
            m[i] = cnt.get(key, 0)
            cnt[key] = m[i] + 1
        nth.append(m)
    fifos = {}       # (src, dst, part) -> list of tokens
    got = {}         # (src, dst, k) -> bytes received
    copied = {}
    launch = [0] * n
    # per rank and launch: {wg: [item, ...]}
    queues = []
    for r in range(n):
        per = {}
        for it in plans[r]:
            per.setdefault(it["launch"], {}).setdefault(it["wg"], []).append(dict(it, done=0))
        queues.append(per)
    n_launch = [max(q, default=-1) + 1 for q in queues]
    ticks = 0
    while any(launch[r] < n_launch[r] for r in range(n)):
        progress = False
        for r in range(n):
            if launch[r] >= n_launch[r]:
                continue
            wgs = queues[r][launch[r]]
            for wg in list(wgs):
                q = wgs[wg]
                it = q[0]
                if it["kind"] == COPY:
                    copied[r, nth[r][it["call"]]] = copied.get((r, nth[r][it["call"]]), 0) + it["bytes"]
                    assert nth[r][it["call"]] == nth[r][it["call2"]]
                    it["done"] = it["steps"] = 1
                    moved = True
                else:
                    ln = min(STEP, it["bytes"] - it["done"] * STEP)
                    if it["kind"] == SEND:
                        f = fifos.setdefault((r, it["peer"], it["part"]), [])
                        moved = len(f) < K_STEPS
                        if moved:
                            f.append((nth[r][it["call"]], it["offset"] + it["done"] * STEP, ln))
                    else:
                        f = fifos.setdefault((it["peer"], r, it["part"]), [])
                        moved = bool(f)
                        if moved:  # the bytes of the matching send, in call order
                            assert f.pop(0) == (nth[r][it["call"]], it["offset"] + it["done"] * STEP, ln)
                            key = (it["peer"], r, nth[r][it["call"]])
                            got[key] = got.get(key, 0) + ln
                    if moved:
                        it["done"] += 1
                if moved:
                    progress = True
                    if it["done"] >= it["steps"]:
                        q.pop(0)
                        if not q:
                            del wgs[wg]
            if not wgs:
                launch[r] += 1
                progress = True
        ticks += 1
        assert progress, f"deadlock at tick {ticks}: launches {launch} of {n_launch}"
    assert all(not f for f in fifos.values())
    return got, copied


def test_simulator_random_groups():
    rng = random.Random(20251020)
    for g in range(200):
        n = 2 + g % 7
        parts = rng.choice([1, 2, 4, 8])
        calls, msgs = random_group(rng, n, parts)
        want = {(a, b, k): B for (a, b), v in msgs.items() if a != b for k, B in enumerate(v) if B}
        for g_cap, max_works in ((1, 120), (2, 120), (0, 120), (0, 3), (2, 3)):
            got, copied = simulate(n, calls, parts, g_cap, max_works)
            assert got == want, (g, g_cap, max_works)
            for r in range(n):  # self pairs: copied whole unless in place
                sends = [c for c in calls[r] if c[0] == SEND and c[1] == r]
                recvs = [c for c in calls[r] if c[0] == RECV and c[1] == r]
                for k, (s, q) in enumerate(zip(sends, recvs)):
                    assert copied.get((r, k), 0) == (0 if s[3] == q[3] else s[2]), (g, r, k)


# ---------------------------------------------------------------- self cases
def test_self_cases():
    n = 4
    for r in range(n):
        for calls in ([(SEND, r, 100)], [(RECV, r, 100)], [(SEND, r, 100), (SEND, r, 100), (RECV, r, 100)],
                      [(SEND, r, 100), (RECV, r, 96)]):
            with pytest.raises(nccl.VcclError) as e:
                plan(r, n, calls + [(SEND, (r + 1) % n, 64), (RECV, (r + 3) % n, 64)], 2)
            assert e.value.code == nccl.ncclInvalidUsage
        # in place: dropped; out of place: one copy per part
        items, _ = plan(r, n, [(SEND, r, 3 * MIN_PART, 0x5000), (RECV, r, 3 * MIN_PART, 0x5000)], 2)
        assert items == []
        items, _ = plan(r, n, [(SEND, r, 3 * MIN_PART, 0x5000), (RECV, r, 3 * MIN_PART, 0x9000)], 2)
        assert [(it["kind"], it["call"], it["call2"], it["bytes"]) for it in items] == \
            [(COPY, 0, 1, 3 * MIN_PART // 2)] * 2
    # one rank: self traffic only
    items, n_wgs = plan(0, 1, [(RECV, 0, 10, 0x100), (SEND, 0, 10, 0x200)], 4)
    assert n_wgs == 1 and [(it["kind"], it["call"], it["call2"]) for it in items] == [(COPY, 1, 0)]
    # a zero-byte message is matched and moves nothing
    assert plan(0, 2, [(SEND, 1, 0), (RECV, 1, 0)], 4)[0] == []


def test_grid_bounds():
    """Workgroups per direction: the connections in use, the floor first, then the cap."""
    calls = [(SEND, 1, 8 * MIN_PART), (RECV, 1, 8 * MIN_PART), (SEND, 2, 1), (RECV, 3, 1)]
    assert plan(0, 4, calls, 4)[1] == 5
    assert plan(0, 4, calls, 4, g_cap=3)[1] == 3
    assert plan(0, 4, calls, 4, g_min=9)[1] == 9
    assert plan(0, 4, calls, 4, g_min=9, g_cap=2)[1] == 2
    assert plan(0, 4, [(SEND, 1, 0)], 4)[1] == 1


def test_bad_arguments():
    L = nccl.lib()
    n_items = ctypes.c_int()
    one = (ctypes.c_int * 1)(0)
    peer = (ctypes.c_int * 1)(1)
    nb = (ctypes.c_size_t * 1)(64)
    out = (ctypes.c_int64 * 12)()

    def call(rank=0, n=2, parts=2, min_part=4096, step=4096, max_works=120, kinds=one, peers=peer):
        return L.vcclP2pPlan(rank, n, 1, kinds, peers, nb, None, parts, min_part, step, 1, 0, max_works, 1,
                             ctypes.byref(n_items), None, out)
    assert call() == nccl.ncclSuccess and n_items.value == 1
    bad = nccl.ncclInvalidArgument
    assert call(n=9) == bad and call(rank=2) == bad and call(parts=0) == bad and call(parts=9) == bad
    assert call(min_part=255) == bad and call(step=4095) == bad and call(step=4096 + 256) == bad
    assert call(max_works=0) == bad and call(max_works=121) == bad
    assert call(kinds=(ctypes.c_int * 1)(2)) == bad and call(peers=(ctypes.c_int * 1)(2)) == bad


# ---------------------------------------------------------------- the surface
def test_python_surface():
    for m in ("send", "recv", "all_to_all", "all_to_allv"):
        assert callable(getattr(nccl.Comm, m))
    assert "vcclP2pPlan" in nccl.EXPORTED and hasattr(nccl.lib(), "vcclP2pPlan")
    text = open(os.path.join(ROOT, "include", "vccl_ext.h")).read()
    assert re.search(r"^ncclResult_t vcclP2pPlan\(", text, flags=re.M)
    for name in ("ncclSend", "ncclRecv", "ncclAllToAll", "ncclAllToAllv"):
        assert name in nccl.EXPORTED and getattr(nccl.lib(), name).argtypes
