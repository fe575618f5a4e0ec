#!/usr/bin/env python3
"""Record tests/golden/a2a_plan.json: the all-to-all plan exports and the rooted
path exports of the library as built, through vccl_amd.nccl.

Recorded at the commit before ll_a2a_plan / direct_a2a_plan became a2a_plan and
the vccl* exports moved to host/ext.cc; tests/test_a2a_plan_golden.py replays
it against every later build.  Re-recording is only right when an export's
behaviour is meant to change.

  python tests/golden/gen_a2a_plan.py      (from the repository root, after make)
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_a2a_plan_golden import GOLDEN, a2a_outputs, rooted_outputs  # noqa: E402

ENV = {"VCCL_LL_ROOTED_THRESHOLD": 2048, "VCCL_DIRECT_ROOTED_THRESHOLD": 65536}
LINES = 64                        # an LL slot of 512 bytes
LL_LIMITS = (512, 96)             # the whole slot, and part of it
D_LIMITS = (40_000, 16_384, 2_097_392)
# (minCTAs, maxCTAs, directMaxBlocks): the defaults, minCTAs above and maxCTAs
# below the natural block count, a cap of 1, minCTAs above the cap
BOUNDS = ((1, 64, 64), (8, 64, 64), (1, 2, 64), (1, 64, 1), (40, 64, 16), (500, 1000, 1000))


def sizes_for(ll, d):
    """0, 1, at and one past each limit, and a few in between."""
    s = {0, 1, 8, 17, 600, 16_385}
    for lim in (ll, d):
        if lim > 0:
            s |= {lim - 1, lim, lim + 1}
    return sorted(s)


def a2a_cases():
    rng = random.Random(20261020)
    cases = []
    for n in range(2, 10):        # 9: one past kOrderMaxRanks and kDirectMaxRanks, refused by both
        for ll_on in (False, True):
            for d_on in (False, True):
                for uniform in (1, 0):
                    for trial in range(5):
                        ll = rng.choice(LL_LIMITS) if ll_on else 0
                        d = rng.choice(D_LIMITS) if d_on else 0
                        sizes = sizes_for(ll, d)
                        rank = rng.randrange(n)
                        if uniform:
                            b = sizes[(trial * 5 + n) % len(sizes)] if trial < 4 else rng.choice(sizes)
                            send = recv = [b] * n
                        else:
                            send = [rng.choice(sizes) for _ in range(n)]
                            recv = [rng.choice(sizes) for _ in range(n)]
                            if trial % 2 == 0:
                                recv[rank] = send[rank]       # a self block that agrees ...
                            elif recv[rank] == send[rank]:
                                recv[rank] = send[rank] + 1   # ... and one that does not
                        cases.append([n, rank, uniform, ll, d, LINES, *rng.choice(BOUNDS), send, recv])
    # the geometry alone: a uniform call of M bytes under every set of bounds
    for m in (1, 17, 16_384, 16_385, 49_153, 98_304, 1 << 20, 8 << 20):
        for b in BOUNDS:
            cases.append([2, 0, 1, 0, 1 << 30, LINES, *b, [m, m], [m, m]])
    # refusals: a limit above the slot, a uniform call with unequal rows, a rank
    # out of range, no lines at all (the LL export refuses, the direct one plans)
    cases.append([4, 0, 0, 520, 40_000, LINES, 1, 64, 64, [8] * 4, [8] * 4])
    cases.append([4, 0, 1, 512, 40_000, LINES, 1, 64, 64, [8, 8, 8, 16], [8] * 4])
    cases.append([4, 0, 1, 512, 40_000, LINES, 1, 64, 64, [8] * 4, [8, 8, 8, 16]])
    cases.append([4, 4, 0, 512, 40_000, LINES, 1, 64, 64, [8] * 4, [8] * 4])
    cases.append([4, 1, 0, 0, 40_000, 0, 1, 64, 64, [8, 0, 50_000, 1], [8, 0, 40_000, 1]])
    cases.append([4, 1, 0, 0, 0, 0, 1, 64, 64, [8, 0, 50_000, 1], [8, 0, 40_000, 1]])
    cases.append([4, 1, 0, 0, 40_000, LINES, 0, 0, 64, [8] * 4, [8] * 4])
    cases.append([4, 1, 0, 0, 40_000, LINES, 1, 64, 0, [8] * 4, [8] * 4])
    cases.append([4, 1, 0, 0, 40_000, LINES, -1, 64, 64, [8] * 4, [8] * 4])
    return cases


def rooted_cases():
    rng = random.Random(20261021)
    rows = []
    counts = (1, 256, 2048, 2049, 4096, 4097, 65_536, 65_537, 1 << 20)
    for i in range(48):
        coll = 3 + i % 2
        words = [rng.choice([0, 0, 0, 1, 2, 3, 4]), rng.choice([0, 4096]), 1024, 8192, rng.choice([0, 1]), 16_384,
                 rng.choice([0, 32_768]), rng.choice([0, 1, 1]), 1 << 20, 1 << 20]
        thr = rng.choice([None, None, 0, 1024, 1 << 20])
        dthr = rng.choice([None, None, 0, 4096, 1 << 20])
        rows.append([coll, rng.choice(counts), rng.choice([1, 7]), rng.choice([1, 2, 4, 8, 9, 64]), words, thr,
                     rng.choice([1, 1, 0]), rng.choice([0, 0, 1]), dthr, rng.choice([1, 1, 0])])
    # where the environment decides: vcclRootedAlgoEx reads VCCL_DIRECT_ROOTED_THRESHOLD, vcclRootedAlgo must not
    for i in range(16):
        words = [rng.choice([0, 0, 3]), rng.choice([0, 4096]), 1024, 8192, 0, 0, 0, 1, 1 << 20, 1 << 20]
        rows.append([3 + i % 2, rng.choice(counts), rng.choice([1, 7]), rng.choice([2, 4, 8]), words,
                     rng.choice([None, 0]), 1, 0, None, 1])
    ok = [0, 4096, 1024, 8192, 0, 0, 0, 1, 1 << 20, 1 << 20]
    for bad in ([5] + ok[1:], [-1] + ok[1:], [0, -1] + ok[2:]):   # refused policy words
        rows.append([3, 4096, 1, 4, bad, None, 1, 0, None, 1])
    rows.append([3, 4096, 1, 65, ok, None, 1, 0, None, 1])        # above kMaxRanks
    rows.append([5, 4096, 1, 4, ok, None, 1, 0, None, 1])         # not a collective
    return rows


def main():
    os.environ.pop("NCCL_LL_ROOTED_THRESHOLD", None)
    os.environ.pop("NCCL_DIRECT_ROOTED_THRESHOLD", None)
    os.environ.update({k: str(v) for k, v in ENV.items()})
    a2a = [[c, a2a_outputs(c)] for c in a2a_cases()]
    rooted = [[r, rooted_outputs(r)] for r in rooted_cases()]
    enc = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(GOLDEN, "w") as f:
        f.write('{"source":"tests/golden/gen_a2a_plan.py","env":%s,\n"a2a":[\n' % enc(ENV))
        f.write(",\n".join(enc(c) for c in a2a))
        f.write('\n],\n"rooted":[\n')
        f.write(",\n".join(enc(r) for r in rooted))
        f.write("\n]}\n")
    print(f"wrote {GOLDEN}: {len(a2a)} all-to-all cases, {len(rooted)} rooted rows, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
