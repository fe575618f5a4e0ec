"""What initialisation decides before it touches the GPU (vcclCommSetup,
host/setup.cc) — CPU checks.

The channel model and its clamps, step / slot validation, the thread count,
the path thresholds and buffer sizes, NCCL_ALGO / NCCL_PROTO exclusions, net
peers, the shared-GPU cap and the two refusals, the LL chain and each
channel's ring view.  Expected values are worked out from the knobs'
documented defaults and from the tests' own restatements (tests/_ring.py
ring sets and channel model, tests/_mp.py co-residency cap), never from the
library.
"""
import ctypes
import os
import re

import pytest

from tests import _mp, _ring
from vccl_amd import nccl

KIB, MIB = 1 << 10, 1 << 20
MAX_CHANNELS = 128   # kMaxChannels
U64_MAX = (1 << 64) - 1


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    """Library defaults: no knob of this process's environment leaks in."""
    for k in list(os.environ):
        if (k.startswith(("NCCL_", "VCCL_")) and k != "VCCL_LIB") or k == "GPU_MAX_HW_QUEUES":
            monkeypatch.delenv(k)
    return monkeypatch


def peers(n, host=lambda r: 7, bus=lambda r: 0x100 + r, pid=lambda r: 1000 + r, cus=lambda r: 256):
    """One rank per GPU of one host, a process each, unless told otherwise."""
    return [(pid(r), host(r), bus(r), cus(r)) for r in range(n)]


def setup(n, rank=0, **kw):
    p = kw.pop("peers", None) or peers(n)
    return nccl.comm_setup(n, rank, p, **kw)


def refused(n, rank=0, **kw):
    with pytest.raises(nccl.VcclError) as e:
        setup(n, rank, **kw)
    return e.value.code


# ---------------------------------------------------------------- defaults
@pytest.mark.parametrize("n,nch", [(1, 0), (2, 16), (3, 32), (4, 48), (5, 64), (6, 64), (7, 60), (8, 63)])
def test_default_channels_threads_step(n, nch):
    s = setup(n)
    assert s["nChannels"] == nch
    if n > 1:
        assert nch == _ring.n_channels(n)
    assert (s["nThreads"], s["stepBytes"], s["slotBytes"]) == (512, 512 * KIB, 512 * KIB)
    assert s["shareBlockCap"] == 0 and not s["anyNet"] and s["netPeer"] == [0] * n


def test_one_rank_sizes_nothing():
    s = setup(1)
    assert [s[k] for k in nccl.SETUP_SIZES] == [0] * 5 and not s["ll128Wanted"]
    assert s["llMaxBytes"] == s["directMaxBytes"] == s["llRsAgMaxBytes"] == 0


def test_bad_arguments():
    assert refused(0) == nccl.ncclInvalidArgument
    with pytest.raises(nccl.VcclError) as e:
        nccl.comm_setup(65, 0, peers(65))
    assert e.value.code == nccl.ncclInvalidArgument
    assert refused(2, rank=2) == nccl.ncclInvalidArgument
    assert refused(2, rank=-1) == nccl.ncclInvalidArgument
    assert refused(2, channel=16) == nccl.ncclInvalidArgument  # channels 0..15
    pid, cus, net = (ctypes.c_int * 2)(1, 2), (ctypes.c_int * 2)(256, 256), (ctypes.c_int * 2)()
    host, bus = (ctypes.c_uint64 * 2)(7, 7), (ctypes.c_int64 * 2)(1, 2)
    good = [pid, host, bus, cus, (ctypes.c_int64 * 19)(), (ctypes.c_int64 * 5)(), (ctypes.c_int * 3)(), net,
            (ctypes.c_int * 8)()]
    assert nccl.lib().vcclCommSetup(2, 0, 1, 128, *good, 0, None, None) == nccl.ncclSuccess
    for k in range(len(good)):
        args = list(good)
        args[k] = None
        assert nccl.lib().vcclCommSetup(2, 0, 1, 128, *args, 0, None, None) == nccl.ncclInvalidArgument, k


# ---------------------------------------------------------------- channel clamps
def test_channel_knobs(clean_env):
    clean_env.setenv("NCCL_NCHANNELS", "12")
    assert setup(2)["nChannels"] == 12 and setup(8)["nChannels"] == 12
    clean_env.delenv("NCCL_NCHANNELS")
    clean_env.setenv("VCCL_CHANNELS_PER_RING", "2")
    assert setup(8)["nChannels"] == 14 == _ring.n_channels(8, per_ring=2)
    assert setup(4)["nChannels"] == 12


def test_cta_bounds():
    assert setup(8, max_ctas=8)["nChannels"] == 8
    assert setup(2, min_ctas=32, max_ctas=64)["nChannels"] == 32
    assert setup(2, min_ctas=1, max_ctas=16)["nChannels"] == 16


def test_max_nchannels_newer_name_wins(clean_env):
    clean_env.setenv("NCCL_MAX_NRINGS", "10")
    assert setup(2)["nChannels"] == 10
    clean_env.setenv("NCCL_MAX_NCHANNELS", "4")
    assert setup(2)["nChannels"] == 4
    clean_env.setenv("NCCL_MAX_NRINGS", "4")
    clean_env.setenv("NCCL_MAX_NCHANNELS", "10")
    assert setup(2)["nChannels"] == 10


def test_min_nchannels_and_ceiling(clean_env):
    clean_env.setenv("NCCL_MIN_NCHANNELS", "40")
    assert setup(2)["nChannels"] == 40
    clean_env.setenv("NCCL_MIN_NCHANNELS", "500")
    assert setup(2)["nChannels"] == MAX_CHANNELS
    clean_env.delenv("NCCL_MIN_NCHANNELS")
    clean_env.setenv("NCCL_NCHANNELS", "1000")
    assert setup(2)["nChannels"] == MAX_CHANNELS
    clean_env.setenv("NCCL_NCHANNELS", "0")
    assert setup(2)["nChannels"] == 1


# ---------------------------------------------------------------- step / slot / threads
def test_step_and_slot(clean_env):
    clean_env.setenv("NCCL_BUFFSIZE", "4194304")
    s = setup(2)
    assert (s["stepBytes"], s["slotBytes"]) == (524288, 524288)
    clean_env.setenv("NCCL_BUFFSIZE", "2097152")
    s = setup(2)
    assert (s["stepBytes"], s["slotBytes"]) == (262144, 262144)
    assert s["fifoBytes"] > 16 * 8 * 262144  # 16 channels x NCCL_STEPS slots (+ padding)
    clean_env.setenv("VCCL_SLICE_BYTES", "131072")  # a 4-step chunk in 4 slots: 131072 is too small
    assert setup(2)["slotBytes"] == 262144
    assert "VCCL_SLICE_BYTES" in nccl.last_error()


def test_bad_slot_bytes_warns(clean_env):
    clean_env.setenv("VCCL_SLOT_BYTES", "5000")  # not a 4096 multiple
    s = setup(2)
    assert (s["stepBytes"], s["slotBytes"]) == (524288, 524288)
    assert "multiple of 4096" in nccl.last_error()


def test_slice_smaller_than_step_falls_back(clean_env):
    clean_env.setenv("VCCL_SLICE_BYTES", "262144")
    s = setup(2)
    assert (s["stepBytes"], s["slotBytes"]) == (524288, 524288)
    clean_env.setenv("VCCL_SLICE_BYTES", "1048576")  # larger is fine
    assert setup(2)["slotBytes"] == 1048576


def test_nthreads(clean_env):
    clean_env.setenv("NCCL_NTHREADS", "256")
    assert setup(2)["nThreads"] == 256
    clean_env.setenv("NCCL_NTHREADS", "384")
    assert setup(2)["nThreads"] == 512


# ---------------------------------------------------------------- thresholds and sizes
def test_thresholds_two_ranks():
    s = setup(2)
    assert s["llMaxBytes"] == 64 * KIB and s["llRsAgMaxBytes"] == 2 * 64 * KIB
    assert s["directMaxBytes"] == 0 and s["directRsAgMaxBytes"] == 0
    assert s["flagBytes"] == 16 * 2 * 128  # two 128-byte flag lines per channel
    assert s["inboxBytes"] > 0  # NCCL_ALGO=Direct can still take a bucket


@pytest.mark.parametrize("n", [4, 8])
def test_thresholds_four_and_eight(n):
    s = setup(n)
    assert s["llMaxBytes"] == 128 * KIB and s["llRsAgMaxBytes"] == n * 128 * KIB
    assert s["directMaxBytes"] == s["directRsAgMaxBytes"] == 8 * MIB
    assert s["llLines"] == 131072  # the 1 MiB VCCL_LL_GROUP_BYTES slot in 8-byte lines
    assert s["llBytes"] == 2 * n * 131072 * 16
    assert s["directMaxBlocks"] == 64
    assert s["ll128MinBytes"] == s["ll128MaxBytes"] == 0 and s["ll128Bytes"] == 0 and not s["ll128Wanted"]


def test_inbox_eight_and_nine():
    s = setup(8)
    assert s["dRegionBytes"] == (16 * MIB // 8) // 256 * 256 + 256
    assert s["inboxBytes"] == 4 * 8 * s["dRegionBytes"]  # kDirectInboxRegions x n regions
    s = setup(9)
    assert s["inboxBytes"] == 0 and s["dRegionBytes"] == 0
    assert s["directMaxBytes"] == s["directRsAgMaxBytes"] == s["llRsAgMaxBytes"] == 0
    assert s["llMaxBytes"] == 128 * KIB and s["llBytes"] > 0


def test_ll_threshold_zero(clean_env):
    clean_env.setenv("VCCL_LL_THRESHOLD", "0")
    s = setup(4)
    assert s["llMaxBytes"] == 0 and s["llRsAgMaxBytes"] == 0 and s["llBytes"] == 0 and s["llLines"] == 0
    assert s["directMaxBytes"] == 8 * MIB


# ---------------------------------------------------------------- NCCL_PROTO / NCCL_ALGO
def ll128_slot_bytes():
    """576,000 data bytes (15/16 of the 614,400-byte step, 1,920 B grain) in
    1 KiB rounds whose lines each give 8 bytes to the flag: 600 rounds with
    128-byte lines (8 a round), 643 with the library's 64-byte lines (16)."""
    line = int(re.search(r"\((\d+)-byte lines\)", nccl.lib().vcclBuildInfo().decode()).group(1))
    rounds = {128: 600, 64: 643}[line]
    data = 1024 - 8 * (1024 // line)
    assert (rounds - 1) * data < 576000 <= rounds * data
    return rounds * 1024


def test_proto_ll128(clean_env):
    clean_env.setenv("NCCL_PROTO", "LL128")
    s = setup(2)
    assert s["algoForce"] == 4 and s["ll128Wanted"] and not s["ll128Drop"]
    assert s["ll128StepBytes"] == 614400 and s["ll128Threads"] == 640
    assert s["ll128SlotBytes"] == ll128_slot_bytes()
    assert s["ll128Bytes"] == 16 * 8 * s["ll128SlotBytes"]
    assert (s["ll128MinBytes"], s["ll128MaxBytes"]) == (0, U64_MAX)
    assert s["llMaxBytes"] == 0 and s["llBytes"] > 0


def test_ll128_window(clean_env):
    clean_env.setenv("VCCL_LL128", "1")
    s = setup(4)
    assert s["algoForce"] == 0 and s["ll128Wanted"]
    assert (s["ll128MinBytes"], s["ll128MaxBytes"]) == (64 * KIB, MIB)
    assert s["ll128Bytes"] == 48 * 8 * ll128_slot_bytes()
    clean_env.delenv("VCCL_LL128")
    clean_env.setenv("VCCL_LL128_ALLOC", "1")  # the buffers only
    s = setup(4)
    assert s["ll128Wanted"] and s["ll128Bytes"] > 0 and s["ll128MaxBytes"] == 0


def test_proto_simple_keeps_ll_buffer(clean_env):
    clean_env.setenv("NCCL_PROTO", "Simple")
    s = setup(4)
    assert s["llMaxBytes"] == 0 and s["llRsAgMaxBytes"] == 0
    assert s["llBytes"] == 2 * 4 * 131072 * 16
    assert s["directMaxBytes"] == 8 * MIB


def test_algo_ring_drops_direct(clean_env):
    clean_env.setenv("NCCL_ALGO", "Ring")
    s = setup(4)
    assert s["directMaxBytes"] == s["directRsAgMaxBytes"] == 0 and s["inboxBytes"] > 0
    assert s["llMaxBytes"] == 0 and s["llRsAgMaxBytes"] == 4 * 128 * KIB  # the ring-LL RS / AG stays


def test_unknown_name_fails(clean_env):
    clean_env.setenv("NCCL_ALGO", "Rnig")
    assert refused(2) == nccl.ncclInvalidUsage
    clean_env.delenv("NCCL_ALGO")
    clean_env.setenv("NCCL_PROTO", "LL256")
    assert refused(2) == nccl.ncclInvalidUsage


# ---------------------------------------------------------------- net
def two_hosts(n):
    return peers(n, host=lambda r: 7 if r < n // 2 else 8, bus=lambda r: 0x100 + r % (n // 2))


def test_two_hosts(clean_env):
    for rank in range(4):
        s = setup(4, rank, peers=two_hosts(4))
        assert s["anyNet"] and s["ll128Drop"]
        assert s["netPeer"] == [int((r < 2) != (rank < 2)) for r in range(4)]
        for k in ("llMaxBytes", "llRsAgMaxBytes", "directMaxBytes", "directRsAgMaxBytes", "ll128MinBytes",
                  "ll128MaxBytes"):
            assert s[k] == 0, k
        assert s["nChannels"] == min(_ring.n_channels(4), 8) == 8
    clean_env.setenv("VCCL_NET_NCHANNELS", "2")
    assert setup(4, peers=two_hosts(4))["nChannels"] == 2


def test_two_hosts_ll128_becomes_simple(clean_env):
    clean_env.setenv("NCCL_PROTO", "LL128")
    s = setup(2, peers=two_hosts(2))
    assert s["algoForce"] == 1 and s["ll128Wanted"] and s["ll128Drop"]
    assert (s["ll128MinBytes"], s["ll128MaxBytes"]) == (0, 0)


def test_net_force(clean_env):
    one_gpu = peers(2, bus=lambda r: 0x100)
    assert refused(2, peers=one_gpu) == nccl.ncclInvalidUsage
    clean_env.setenv("VCCL_NET_FORCE", "1")
    s = setup(2, 1, peers=one_gpu)  # no duplicate-GPU refusal
    assert s["anyNet"] and s["netPeer"] == [1, 0] and s["nChannels"] == 8
    assert setup(4, 2)["netPeer"] == [1, 1, 0, 1]


# ---------------------------------------------------------------- shared GPUs
def on_devices(n, ndev, cus=lambda r: 256, pid=lambda r: 1000 + r):
    return peers(n, bus=lambda r: 0x100 + r % ndev, cus=cus, pid=pid)


def test_duplicate_gpu_refused():
    assert refused(8, peers=on_devices(8, 1)) == nccl.ncclInvalidUsage
    assert "Duplicate GPU detected : rank 0 and rank 1" in nccl.last_error()
    assert refused(8, 5, peers=on_devices(8, 7)) == nccl.ncclInvalidUsage  # ranks 0 and 7 only


@pytest.mark.parametrize("n,ndev,cap", [(8, 1, 28), (8, 2, 56), (2, 1, 112)])
def test_shared_gpu_cap(clean_env, n, ndev, cap):
    clean_env.setenv("VCCL_ALLOW_SHARED_DEVICE", "1")
    clean_env.setattr(_mp, "device_count", lambda: ndev)
    assert cap == max(1, 256 * 7 // 8 // (n // ndev))
    for rank in (0, n - 1):
        s = setup(n, rank, peers=on_devices(n, ndev))
        assert s["shareBlockCap"] == cap
        assert s["nChannels"] == _mp.shared_channel_cap(n, _ring.n_channels(n), 256) == min(_ring.n_channels(n), cap)
        assert s["directMaxBlocks"] == min(64, cap)
        assert s["fifoBytes"] == setup(n)["fifoBytes"]  # sized for the uncapped count


def test_smallest_cu_count_governs(clean_env):
    clean_env.setenv("VCCL_ALLOW_SHARED_DEVICE", "1")
    s = setup(8, peers=on_devices(8, 1, cus=lambda r: 64 if r == 7 else 256))
    assert s["shareBlockCap"] == s["nChannels"] == 64 * 7 // 8 // 8 == 7


# ---------------------------------------------------------------- hardware queues
@pytest.mark.parametrize("queues,passes,fails", [(None, 3, 4), ("4", 3, 4), ("8", 4, 8)])
def test_hardware_queue_refusal(clean_env, queues, passes, fails):
    clean_env.setenv("VCCL_ALLOW_SHARED_DEVICE", "1")
    if queues:
        clean_env.setenv("GPU_MAX_HW_QUEUES", queues)
    one_process = lambda n: on_devices(n, 1, pid=lambda r: 4242)
    assert setup(passes, peers=one_process(passes))["shareBlockCap"] == 256 * 7 // 8 // passes
    for rank in (0, fails - 1):
        assert refused(fails, rank, peers=one_process(fails)) == nccl.ncclInvalidUsage
    assert "hardware queues" in nccl.last_error()
    assert setup(8, peers=on_devices(8, 1))["nChannels"] == 28  # a process each: never


# ---------------------------------------------------------------- LL chain
def test_ll_chain(clean_env):
    assert setup(2)["llChain"] == [0, 1] and setup(8)["llChain"] == list(range(8))
    clean_env.setenv("VCCL_LL_CHAIN", "1,0")
    assert setup(2)["llChain"] == [1, 0]
    for bad in ("0,0", "0", "0,2", "1,0,", "x"):
        clean_env.setenv("VCCL_LL_CHAIN", bad)
        if bad == "1,0,":
            assert setup(2)["llChain"] == [1, 0]  # a trailing comma ends the list
            continue
        assert refused(2) == nccl.ncclInvalidUsage, bad
        assert "not a permutation of the 2 ranks" in nccl.last_error()
    clean_env.setenv("VCCL_LL_CHAIN", "0,0")
    assert setup(9)["llChain"] == list(range(8))  # ignored above 8 ranks
    clean_env.setenv("VCCL_LL_CHAIN", "3,1,2,0")
    assert setup(4, 2)["llChain"] == [3, 1, 2, 0]


# ---------------------------------------------------------------- ring view
@pytest.mark.parametrize("n", range(2, 9))
def test_ring_view_and_tables(n):
    rings = _ring.ring_orders(n)
    nch = _ring.n_channels(n)
    for rank in range(n):
        for ch in range(nch):
            ring = rings[ch % len(rings)]
            pos = ring.index(rank)
            s = setup(n, rank, channel=ch)
            assert (s["ringPos"], s["next"], s["prev"]) == (pos, ring[(pos + 1) % n], ring[(pos - 1) % n]), (rank, ch)
        assert s["nRings"] == len(rings)
        for k, ring in enumerate(rings):
            pos = ring.index(rank)
            assert s["rsOrder"][k][:n] == [ring[(pos + 1 + j) % n] for j in range(n)]
            assert s["ringAt"][k][:n] == ring
