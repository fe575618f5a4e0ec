"""CPU checks of the LL send / recv plan (vcclP2pLLMax, vcclP2pPlanEx, host/plan.cc): the threshold's clamps, the
plan without LL unchanged, which messages become LL items and in how many steps, both ends agreeing, one workgroup
per LL connection direction.  No GPU call is made."""
import pytest

from vccl_amd import nccl

LL_MAX, LL_STEP = 4096, 1024
SIZES = (0, 1, 8, 1023, 1024, 1025, LL_MAX, LL_MAX + 1, 300 << 10)
KW = {"parts": 2, "min_part_bytes": 4096, "step_bytes": 16384}
GROUPS = [(2, 0, 0), (4, 1, 0), (4, 5, 1), (8, 2, 3)]  # ranks, seed, workgroup cap
LL_KINDS = (nccl.P2P_LL_SEND, nccl.P2P_LL_RECV)


def group(rank, n, seed):
    """Three messages to and from every other rank (three sweeps), sizes walking SIZES; and a self pair."""
    calls = [(nccl.P2P_SEND, rank, 77), (nccl.P2P_RECV, rank, 77)]
    for k, p in ((k, p) for k in range(3) for p in range(n) if p != rank):
        calls.append((nccl.P2P_SEND, p, SIZES[(seed + 3 * rank + p + 4 * k) % len(SIZES)]))
        calls.append((nccl.P2P_RECV, p, SIZES[(seed + 3 * p + rank + 4 * k) % len(SIZES)]))
    return calls


@pytest.mark.parametrize("kw,want", [
    ({}, 4096), ({"threshold": 0}, 0),
    ({"has_p2p": False}, 0), ({"ll_allowed": False}, 0), ({"any_net": True}, 0),  # no connections, NCCL_PROTO, a net peer
    ({"nranks": 1}, 0), ({"nranks": 8}, 4096), ({"nranks": 9}, 0),
    ({"step_bytes": 1020}, 0), ({"step_bytes": 0}, 0), ({"step_bytes": 8}, 4096),
])
def test_threshold_clamps(kw, want):
    assert nccl.p2p_ll_max(**{"threshold": 4096, **kw}) == want


@pytest.mark.parametrize("n,seed,g_cap", GROUPS)
def test_ll_items(n, seed, g_cap):
    key = ("kind", "sweep", "round", "part", "peer", "offset", "bytes", "steps")
    plans = {}
    for r in range(n):
        calls = group(r, n, seed)
        base = nccl.p2p_plan(r, n, calls, g_cap=g_cap, **KW)
        assert nccl.p2p_plan(r, n, calls, g_cap=g_cap, ll_max=0, **KW) == base  # llMax 0 is vcclP2pPlan
        items, n_wgs = plans[r] = nccl.p2p_plan(r, n, calls, g_cap=g_cap, ll_max=LL_MAX, ll_step_bytes=LL_STEP, **KW)
        for c, (kind, peer, nbytes) in enumerate(calls):
            mine = [[it[k] for k in key] for it in items if it["call"] == c]
            if 0 < nbytes <= LL_MAX and peer != r:  # one item, the whole message, ceil(B / step) steps
                assert mine == [[LL_KINDS[kind], mine[0][1], mine[0][2], 0, peer, 0, nbytes, -(-nbytes // LL_STEP)]]
            else:  # the empty message, B = LL_MAX + 1 and the self copy: as without LL
                assert mine == [[it[k] for k in key] for it in base[0] if it["call"] == c]
        owner = {}
        for it in (it for it in items if it["kind"] in LL_KINDS):  # I1, on its side of the grid
            assert owner.setdefault((it["kind"], it["peer"]), it["wg"]) == it["wg"] < 2 * n_wgs
            assert (it["wg"] >= n_wgs) == (it["kind"] == nccl.P2P_LL_RECV)
        keys = [(it["sweep"], it["round"], it["part"]) for it in items]
        assert keys == sorted(keys)  # I2
    for a, b in ((a, b) for a in range(n) for b in range(n) if a != b):  # I3: a's LL sends to b mirror b's LL recvs from a
        sends, recvs = [[(it["sweep"], it["bytes"], it["steps"]) for it in plans[x][0] if (it["kind"], it["peer"]) == k]
                        for x, k in ((a, (nccl.P2P_LL_SEND, b)), (b, (nccl.P2P_LL_RECV, a)))]
        assert sends == recvs and sends
