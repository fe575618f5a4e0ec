"""ctypes binding of libvccl.so's C ABI (include/nccl.h, include/vccl_device.h).

This is the binding a Python caller of the reference would write against
libnccl (same function names, enum values, argument order and error codes —
see INTEGRATION.md).  It loads the in-tree ``vccl_amd/lib/libvccl.so`` and
raises ``VcclError`` if the library is missing: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import time
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VCCL_LIB") or os.path.join(_HERE, "lib", "libvccl.so")

# ncclResult_t (nccl.h.in:40-48)
ncclSuccess, ncclUnhandledCudaError, ncclSystemError, ncclInternalError = 0, 1, 2, 3
ncclInvalidArgument, ncclInvalidUsage, ncclRemoteError, ncclInProgress = 4, 5, 6, 7
# ncclRedOp_t (nccl.h.in:221-236)
ncclSum, ncclProd, ncclMax, ncclMin, ncclAvg = 0, 1, 2, 3, 4
# ncclDataType_t (nccl.h.in:239-252)
ncclInt8, ncclUint8, ncclInt32, ncclUint32, ncclInt64, ncclUint64 = 0, 1, 2, 3, 4, 5
ncclFloat16, ncclFloat32, ncclFloat64, ncclBfloat16 = 6, 7, 8, 9
ncclFloat8e4m3, ncclFloat8e5m2, ncclNumTypes = 10, 11, 12
# ncclScalarResidence_t
ncclScalarDevice, ncclScalarHostImmediate = 0, 1
# vcclDevRedOp_t (include/vccl_device.h)
vcclDevSum, vcclDevProd, vcclDevMinMax, vcclDevPreMulSum, vcclDevSumPostDiv = 0, 1, 2, 3, 4
vcclDevCopy = 15

TYPE_SIZE = {0: 1, 1: 1, 2: 4, 3: 4, 4: 8, 5: 8, 6: 2, 7: 4, 8: 8, 9: 2, 10: 1, 11: 1}

# Every symbol include/*.h declares (checked by tests/test_abi.py).
EXPORTED = [
    "ncclGetVersion", "ncclGetUniqueId", "ncclCommInitRankConfig", "ncclCommInitRank",
    "ncclCommInitAll", "ncclCommFinalize", "ncclCommDestroy", "ncclCommAbort",
    "ncclGetErrorString", "ncclGetLastError", "ncclCommGetAsyncError", "ncclCommCount",
    "ncclCommCuDevice", "ncclCommUserRank", "ncclRedOpCreatePreMulSum", "ncclRedOpDestroy",
    "ncclAllReduce", "ncclReduceScatter", "ncclAllGather", "ncclGroupStart", "ncclGroupEnd",
    "vcclReduceCopy", "vcclReduceCopyEx", "vcclHostToDevRedOp", "vcclKernelTypeOf",
    "vcclBuildInfo", "vcclBootstrapAllGather", "vcclCommCollAlgo", "vcclCommSetAlgo",
    "vcclCommLaunchStats", "vcclCommNetStats", "vcclCommSetFences", "vcclCommDebugSetEpochs",
    "vcclCommSetRingWave", "vcclCommRingTrace", "vcclCommGroupAlgos",
    "vcclRingPartition", "vcclRingChunkOf", "vcclRingOrders", "vcclGroupPlan", "vcclGroupPlanEx", "vcclAlgoSelection",
    "vcclCommSetup",
    # rooted rings, split and debug reload
    "ncclReduce", "ncclBcast", "ncclBroadcast", "ncclCommSplit", "ncclResetDebugInit",
    # point-to-point over per-peer FIFOs (RCCL's all-to-alls grouped from them) and its planner
    "ncclSend", "ncclRecv", "ncclAllToAll", "ncclAllToAllv", "vcclP2pPlan",
    # one-hop LL broadcast / reduce: the selection with its threshold, and the launch's line layout
    "vcclRootedAlgo", "vcclLLRootedPlan",
    # two-hop direct broadcast / reduce: the selection with both thresholds, and one call's geometry and steps
    "vcclRootedAlgoEx", "vcclDirectRootedPlan",
    # one-hop LL all-to-all: the per-pair limit, one call's LL / FIFO split, the counters, the live knob
    "vcclLLA2aMax", "vcclLLA2aPlan", "vcclCommA2aStats", "vcclCommSetA2aThreshold",
    # one-hop direct all-to-all: the per-pair limit, one call's LL / direct / FIFO split, the counters, the live knob
    "vcclDirectA2aMax", "vcclDirectA2aPlan", "vcclCommA2aStatsEx", "vcclCommSetDirectA2aThreshold",
    # zero-copy direct AR / RS / AG over registered buffers: the threshold, the eligibility rule, one launch's
    # steps, the registration table on its own, the counters, the live knob
    "vcclRegMax", "vcclRegEligible", "vcclRegPlan", "vcclRegTableNew", "vcclRegTableInsert", "vcclRegTableFind",
    "vcclRegTableRemove", "vcclRegTableFree", "vcclCommRegStats", "vcclCommSetRegThreshold",
    # zero-copy all-to-all(v) over registered send buffers: the threshold, the eligibility rule, one launch's
    # steps, the counters, the live knob
    "vcclRegA2aMax", "vcclRegA2aEligible", "vcclRegA2aPlan", "vcclCommRegA2aStats", "vcclCommSetRegA2aThreshold",
    # zero-copy broadcast / reduce over registered buffers: the threshold, the eligibility rule, one launch's
    # steps, the counters, the live knob
    "vcclRegRootedMax", "vcclRegRootedEligible", "vcclRegRootedPlan", "vcclCommRegRootedStats",
    "vcclCommSetRegRootedThreshold",
    # out of scope, exported so libnccl-linked binaries load: WARN + ncclInvalidUsage
    "ncclGroupSimulateEnd",
    # memory / registration / scalable init (what a libnccl caller such as
    # PyTorch's nccl backend imports)
    "ncclMemAlloc", "ncclMemFree", "ncclCommInitRankScalable", "ncclCommRegister", "ncclCommDeregister",
]
ALGO_NAMES = {0: "ring", 1: "ll", 2: "direct", 3: "one_rank", 4: "ll128"}


class VcclError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = lib().ncclGetErrorString(code).decode() if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} (ncclResult_t={code})")


class ncclUniqueId(ctypes.Structure):
    _fields_ = [("internal", ctypes.c_char * 128)]


class vcclLaunchConfig(ctypes.Structure):
    _fields_ = [("blockSize", ctypes.c_int), ("unroll", ctypes.c_int),
                ("gridBlocks", ctypes.c_int), ("ntLoads", ctypes.c_int),
                ("ntStores", ctypes.c_int), ("order", ctypes.c_int)]


class ncclConfig_t(ctypes.Structure):
    """nccl.h.in:57-85 (include/nccl.h), filled as NCCL_CONFIG_INITIALIZER."""
    _fields_ = [("size", ctypes.c_size_t), ("magic", ctypes.c_uint), ("version", ctypes.c_uint),
                ("blocking", ctypes.c_int), ("cgaClusterSize", ctypes.c_int), ("minCTAs", ctypes.c_int),
                ("maxCTAs", ctypes.c_int), ("netName", ctypes.c_void_p), ("splitShare", ctypes.c_int),
                ("trafficClass", ctypes.c_int)]

    @classmethod
    def initializer(cls, **kw) -> "ncclConfig_t":
        undef = -2147483648  # NCCL_CONFIG_UNDEF_INT
        c = cls(ctypes.sizeof(cls), 0xcafebeef, get_version(), undef, undef, undef, undef, None, undef, undef)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


_lib = None


def last_error(comm=None) -> str:
    """ncclGetLastError: the last WARN's text (comm unused, may be None)."""
    return (lib().ncclGetLastError(comm) or b"").decode(errors="replace")


def lib() -> ctypes.CDLL:
    """Load libvccl.so (fails loudly if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `make -j8` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    c_int, c_size, vp, u64 = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint64
    pcomm = ctypes.POINTER(vp)
    sig = {
        "ncclGetVersion": [ctypes.POINTER(c_int)],
        "ncclGetUniqueId": [ctypes.POINTER(ncclUniqueId)],
        "ncclCommInitRank": [pcomm, c_int, ncclUniqueId, c_int],
        "ncclCommInitAll": [pcomm, c_int, ctypes.POINTER(c_int)],
        "ncclCommInitRankConfig": [pcomm, c_int, ncclUniqueId, c_int, ctypes.POINTER(ncclConfig_t)],
        "ncclCommFinalize": [vp],
        "ncclCommDestroy": [vp],
        "ncclCommAbort": [vp],
        "ncclCommGetAsyncError": [vp, ctypes.POINTER(c_int)],
        "ncclCommCount": [vp, ctypes.POINTER(c_int)],
        "ncclCommCuDevice": [vp, ctypes.POINTER(c_int)],
        "ncclCommUserRank": [vp, ctypes.POINTER(c_int)],
        "ncclRedOpCreatePreMulSum": [ctypes.POINTER(c_int), vp, c_int, c_int, vp],
        "ncclRedOpDestroy": [c_int, vp],
        "ncclAllReduce": [vp, vp, c_size, c_int, c_int, vp, vp],
        "ncclReduceScatter": [vp, vp, c_size, c_int, c_int, vp, vp],
        "ncclAllGather": [vp, vp, c_size, c_int, vp, vp],
        "ncclBroadcast": [vp, vp, c_size, c_int, c_int, vp, vp],
        "ncclReduce": [vp, vp, c_size, c_int, c_int, c_int, vp, vp],
        "ncclSend": [vp, c_size, c_int, c_int, vp, vp],
        "ncclRecv": [vp, c_size, c_int, c_int, vp, vp],
        "ncclAllToAll": [vp, vp, c_size, c_int, vp, vp],
        "ncclAllToAllv": [vp, ctypes.POINTER(c_size), ctypes.POINTER(c_size), vp, ctypes.POINTER(c_size),
                          ctypes.POINTER(c_size), c_int, vp, vp],
        "vcclP2pPlan": [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_size),
                        ctypes.POINTER(u64), c_int, c_size, c_size, c_int, c_int, c_int, c_int,
                        ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64)],
        "ncclGroupStart": [],
        "ncclGroupEnd": [],
        "vcclReduceCopy": [c_int, c_int, u64, c_int, c_int, c_int, ctypes.POINTER(vp), c_int,
                           ctypes.POINTER(vp), c_size, vp],
        "vcclReduceCopyEx": [c_int, c_int, u64, c_int, c_int, c_int, ctypes.POINTER(vp), c_int,
                             ctypes.POINTER(vp), c_size, vp, ctypes.POINTER(vcclLaunchConfig)],
        "vcclHostToDevRedOp": [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(u64)],
        "vcclKernelTypeOf": [c_int, c_int],
        "vcclBootstrapAllGather": [ctypes.POINTER(ncclUniqueId), c_int, c_int, vp, c_size],
        "vcclCommSetFences": [vp, c_int],
        "vcclCommSetRingWave": [vp, c_int, ctypes.POINTER(ctypes.c_ulonglong)],
        "vcclRingPartition": [c_int, c_size, c_int, c_int, c_int, c_int, c_size, c_int,
                              ctypes.POINTER(ctypes.c_int64)],
        "vcclCommDebugSetEpochs": [vp, ctypes.c_uint32, ctypes.c_uint32],
        "vcclRingChunkOf": [c_size, c_int, c_int, c_int, c_size, c_int, c_size,
                            ctypes.POINTER(ctypes.c_int64)],
        "vcclRingOrders": [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
        "vcclGroupPlan": [c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_size), ctypes.POINTER(c_int),
                          ctypes.POINTER(c_int), c_int, c_int, c_size, c_int, ctypes.POINTER(c_int),
                          ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64)],
        "vcclGroupPlanEx": [c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_size), ctypes.POINTER(c_int),
                            ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(ctypes.c_int64),
                            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                            ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64)],
        "vcclCommGroupAlgos": [vp, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_size), ctypes.POINTER(c_int),
                               ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
        "vcclRootedAlgo": [c_int, c_size, c_int, c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, c_int, c_int,
                           ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int)],
        "vcclRootedAlgoEx": [c_int, c_size, c_int, c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, c_int, c_int,
                             ctypes.c_int64, c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                             ctypes.POINTER(c_int)],
        "vcclDirectRootedPlan": [c_int, c_int, c_int, c_int, c_size, c_int, ctypes.c_int64, c_int, c_int,
                                 ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                 ctypes.POINTER(ctypes.c_int64)],
        "vcclLLRootedPlan": [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_size),
                             ctypes.c_int64, c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int),
                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64)],
        "vcclLLA2aMax": [ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)],
        "vcclLLA2aPlan": [c_int, c_int, ctypes.POINTER(c_size), ctypes.POINTER(c_size), c_int, ctypes.c_int64,
                          ctypes.c_int64, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int),
                          ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
        "vcclCommA2aStats": [vp, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong),
                             ctypes.POINTER(ctypes.c_ulonglong)],
        "vcclCommSetA2aThreshold": [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
        "vcclDirectA2aMax": [ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_int,
                             ctypes.POINTER(ctypes.c_int64)],
        "vcclDirectA2aPlan": [c_int, c_int, ctypes.POINTER(c_size), ctypes.POINTER(c_size), c_int, ctypes.c_int64,
                              ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, ctypes.POINTER(c_int),
                              ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                              ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int),
                              ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
        "vcclCommA2aStatsEx": [vp] + [ctypes.POINTER(ctypes.c_ulonglong)] * 5,
        "vcclCommSetDirectA2aThreshold": [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
        "ncclCommRegister": [vp, vp, c_size, ctypes.POINTER(vp)],
        "ncclCommDeregister": [vp, vp],
        "vcclRegMax": [ctypes.c_int64, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)],
        "vcclRegEligible": [c_int, c_size, c_int, c_int, ctypes.c_int64, c_int, ctypes.POINTER(c_int)],
        "vcclRegPlan": [c_int, c_size, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64), c_int,
                        ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64)],
        "vcclRegTableNew": [ctypes.POINTER(vp)],
        "vcclRegTableInsert": [vp, u64, c_size, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_uint32)],
        "vcclRegTableFind": [vp, u64, c_size, ctypes.POINTER(c_int), ctypes.POINTER(u64),
                             ctypes.POINTER(ctypes.c_uint32)],
        "vcclRegTableRemove": [vp, c_int],
        "vcclRegTableFree": [vp],
        "vcclCommRegStats": [vp] + [ctypes.POINTER(ctypes.c_ulonglong)] * 3 + [ctypes.POINTER(c_int)] * 2,
        "vcclCommSetRegThreshold": [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
        "vcclRegRootedMax": [ctypes.c_int64, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)],
        "vcclRegRootedEligible": [c_int, c_size, c_int, ctypes.c_int64, c_int, ctypes.POINTER(c_int)],
        "vcclRegRootedPlan": [c_int, c_size, c_int, c_int, c_int, c_int, c_size, c_int,
                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int),
                              c_int, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64)],
        "vcclCommRegRootedStats": [vp] + [ctypes.POINTER(ctypes.c_ulonglong)] * 3,
        "vcclCommSetRegRootedThreshold": [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
        "vcclRegA2aMax": [ctypes.c_int64, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)],
        "vcclRegA2aEligible": [c_int, c_size, ctypes.c_int64, c_int, ctypes.POINTER(c_int)],
        "vcclRegA2aPlan": [c_int, c_int, ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size),
                           c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, ctypes.POINTER(c_int),
                           ctypes.POINTER(ctypes.c_int64)],
        "vcclCommRegA2aStats": [vp] + [ctypes.POINTER(ctypes.c_ulonglong)] * 3,
        "vcclCommSetRegA2aThreshold": [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
        "vcclAlgoSelection": [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(c_int),
                              ctypes.POINTER(c_int)],
        "vcclCommSetup": [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(u64),
                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_int64),
                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                          ctypes.POINTER(c_int), c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = c_int
    L.ncclGetErrorString.argtypes = [c_int]
    L.ncclGetErrorString.restype = ctypes.c_char_p
    for name in ("ncclGetLastError", "pncclGetLastError"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = ctypes.c_char_p
    L.vcclBuildInfo.argtypes = []
    L.vcclBuildInfo.restype = ctypes.c_char_p
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != ncclSuccess:
        raise VcclError(rc, what)


def get_version() -> int:
    v = ctypes.c_int()
    check(lib().ncclGetVersion(ctypes.byref(v)), "ncclGetVersion")
    return v.value


def get_unique_id() -> ncclUniqueId:
    uid = ncclUniqueId()
    check(lib().ncclGetUniqueId(ctypes.byref(uid)), "ncclGetUniqueId")
    return uid


def unique_id_to_bytes(uid: ncclUniqueId) -> bytes:
    return ctypes.string_at(ctypes.addressof(uid), 128)  # .internal stops at the first NUL


def unique_id_from_bytes(b: bytes) -> ncclUniqueId:
    uid = ncclUniqueId()
    ctypes.memmove(ctypes.byref(uid), b, 128)
    return uid


def bootstrap_allgather(uid: ncclUniqueId, rank: int, nranks: int, mine: bytes) -> list[bytes]:
    """One all-gather round over the TCP rendezvous (host only)."""
    n = len(mine)
    buf = ctypes.create_string_buffer(n * nranks)
    ctypes.memmove(ctypes.addressof(buf) + rank * n, mine, n)
    check(lib().vcclBootstrapAllGather(ctypes.byref(uid), rank, nranks, buf, n),
          "vcclBootstrapAllGather")
    raw = buf.raw
    return [raw[i * n:(i + 1) * n] for i in range(nranks)]


def host_to_dev_redop(op: int, dtype: int, nranks: int) -> tuple[int, int]:
    d, a = ctypes.c_int(), ctypes.c_uint64()
    check(lib().vcclHostToDevRedOp(op, dtype, nranks, ctypes.byref(d), ctypes.byref(a)),
          "vcclHostToDevRedOp")
    return d.value, a.value


def kernel_type_of(dev_op: int, dtype: int) -> int:
    return lib().vcclKernelTypeOf(dev_op, dtype)


PROTO_LL128, PROTO_SIMPLE = 1, 2


def ring_partition(coll: int, count: int, dtype: int, nranks: int, nchannels: int,
                   slot_bytes: int, nthreads: int = 512, proto: int = PROTO_SIMPLE) -> tuple[int, ...]:
    """vcclRingPartition: (channelLo, channelHi, countLo, countMid, countHi,
    chunkLo, chunkMid, chunkHi) of the ring's cbd partition (host only);
    slot_bytes = the protocol's FIFO step, nthreads = NCCL_NTHREADS (SIMPLE)
    or NCCL_LL128_NTHREADS (LL128)."""
    out = (ctypes.c_int64 * 8)()
    check(lib().vcclRingPartition(coll, count, dtype, nranks, nchannels, proto, slot_bytes, nthreads,
                                  out),
          "vcclRingPartition")
    return tuple(out)


def ring_orders(nranks: int) -> list[list[int]]:
    """vcclRingOrders: the library's ring set for nranks ranks."""
    out = (ctypes.c_int * (16 * nranks))()
    nr = ctypes.c_int()
    check(lib().vcclRingOrders(nranks, 16, out, ctypes.byref(nr)), "vcclRingOrders")
    return [list(out[k * nranks:(k + 1) * nranks]) for k in range(nr.value)]


def ring_chunk_of(count: int, dtype: int, nranks: int, nchannels: int, slot_bytes: int,
                  i: int, nthreads: int = 512) -> tuple[int, int, int]:
    """vcclRingChunkOf: (channel, ring chunk c, chunk end) of all-reduce
    element i on the ring's partition (the direct all-reduce's fold lookup)."""
    out = (ctypes.c_int64 * 3)()
    check(lib().vcclRingChunkOf(count, dtype, nranks, nchannels, slot_bytes, nthreads, i, out),
          "vcclRingChunkOf")
    return tuple(out)


def group_plan(calls, nranks: int, nchannels: int, slot_bytes: int = 512 << 10,
               nthreads: int = 512):
    """vcclGroupPlan: VCCL's multi-task plan of a group of ring / direct calls.
    calls = [(coll, count, dtype, op)]; returns (order, plan_of, parts) with
    parts[i] = (channelLo, channelHi, countLo, countMid, countHi, chunkLo,
    chunkMid, chunkHi) as ring_partition gives it."""
    n = len(calls)
    ci = ctypes.c_int * n
    colls, dts, ops = ci(*[c[0] for c in calls]), ci(*[c[2] for c in calls]), ci(*[c[3] for c in calls])
    counts = (ctypes.c_size_t * n)(*[c[1] for c in calls])
    order, plan_of = ci(), ci()
    cbd = (ctypes.c_int64 * (8 * n))()
    check(lib().vcclGroupPlan(n, colls, counts, dts, ops, nranks, nchannels, slot_bytes, nthreads, order,
                              plan_of, cbd), "vcclGroupPlan")
    return list(order), list(plan_of), [tuple(cbd[8 * i:8 * i + 8]) for i in range(n)]


POLICY_FIELDS = ("force", "ll_slot", "ll_max", "ll_rsag_max", "ll128", "ll128_min", "ll128_max", "direct",
                 "direct_max", "direct_rsag_max")


def group_plan_ex(calls, nranks: int, nchannels: int, policy: dict | None, slot_bytes: int = 512 << 10,
                  nthreads: int = 512, ll128_step: int = 120 * 640 * 8, ll128_threads: int = 640):
    """vcclGroupPlanEx: the plan a comm lays a group out on — a path per
    aggregate from `policy` (POLICY_FIELDS; None = every call on the SIMPLE
    ring).  Returns (algos, order, plan_of, parts), algos as ALGO_NAMES."""
    n = len(calls)
    ci = ctypes.c_int * n
    colls, dts, ops = ci(*[c[0] for c in calls]), ci(*[c[2] for c in calls]), ci(*[c[3] for c in calls])
    counts = (ctypes.c_size_t * n)(*[c[1] for c in calls])
    geo = (ctypes.c_int64 * 4)(slot_bytes, nthreads, ll128_step, ll128_threads)
    pol = None if policy is None else (ctypes.c_int64 * 10)(*[int(policy[k]) for k in POLICY_FIELDS])
    algos, order, plan_of = ci(), ci(), ci()
    cbd = (ctypes.c_int64 * (8 * n))()
    check(lib().vcclGroupPlanEx(n, colls, counts, dts, ops, nranks, nchannels, geo, pol, algos, order, plan_of,
                                cbd), "vcclGroupPlanEx")
    return ([ALGO_NAMES[a] for a in algos], list(order), list(plan_of),
            [tuple(cbd[8 * i:8 * i + 8]) for i in range(n)])


def rooted_algo(coll: int, count: int, dtype: int, nranks: int, policy: dict, threshold: int | None = None,
                ll_allowed: bool = True, any_net: bool = False) -> tuple[str, int]:
    """vcclRootedAlgo: (path, effective threshold) of one call on `policy`
    (POLICY_FIELDS) plus the rooted LL threshold in bytes as a comm would take
    it (None: VCCL_LL_ROOTED_THRESHOLD from the environment)."""
    pol = (ctypes.c_int64 * 10)(*[int(policy[k]) for k in POLICY_FIELDS])
    eff, a = ctypes.c_int64(), ctypes.c_int()
    check(lib().vcclRootedAlgo(coll, count, dtype, nranks, pol, -1 if threshold is None else threshold,
                               int(ll_allowed), int(any_net), ctypes.byref(eff), ctypes.byref(a)), "vcclRootedAlgo")
    return ALGO_NAMES[a.value], eff.value


def rooted_algo_ex(coll: int, count: int, dtype: int, nranks: int, policy: dict, threshold: int | None = None,
                   ll_allowed: bool = True, any_net: bool = False, direct_threshold: int | None = None,
                   direct_allowed: bool = True) -> tuple[str, int, int]:
    """vcclRootedAlgoEx: (path, effective LL threshold, effective direct
    threshold) of one call on `policy` (POLICY_FIELDS) plus the rooted LL and
    rooted direct thresholds in bytes as a comm would take them (None:
    VCCL_LL_ROOTED_THRESHOLD / VCCL_DIRECT_ROOTED_THRESHOLD from the
    environment)."""
    pol = (ctypes.c_int64 * 10)(*[int(policy[k]) for k in POLICY_FIELDS])
    eff, deff, a = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    check(lib().vcclRootedAlgoEx(coll, count, dtype, nranks, pol, -1 if threshold is None else threshold,
                                 int(ll_allowed), int(any_net), -1 if direct_threshold is None else direct_threshold,
                                 int(direct_allowed), ctypes.byref(eff), ctypes.byref(deff), ctypes.byref(a)),
          "vcclRootedAlgoEx")
    return ALGO_NAMES[a.value], eff.value, deff.value


DIRECT_STEP_KINDS = ("wait", "store", "read", "post", "local")
DIRECT_STEP_SRCS = ("send", "region", "fold")


def direct_rooted_plan(coll: int, nranks: int, rank: int, root: int, count: int, dtype: int, region_bytes: int,
                       chunk: int = -1):
    """vcclDirectRootedPlan: one direct broadcast (coll 3) / reduce (coll 4) as
    `rank` runs it on inbox regions of region_bytes.  Returns a dict: chunk_elts
    (a broadcast: bytes), n_chunks, shard_elts (of `chunk`), owners (per shard)
    and steps, the ordered steps of `chunk` (-1: none) as tuples (kind, phase,
    peer, region, region offset, user offset, bytes, src) with kind from
    DIRECT_STEP_KINDS, src from DIRECT_STEP_SRCS and offsets / lengths in bytes."""
    cap = 4 * nranks + 8
    geo = (ctypes.c_int64 * 4)()
    owners = (ctypes.c_int * nranks)()
    steps = (ctypes.c_int64 * (8 * cap))()
    ns = ctypes.c_int()
    check(lib().vcclDirectRootedPlan(coll, nranks, rank, root, count, dtype, region_bytes, chunk, cap, geo, owners,
                                     ctypes.byref(ns), steps), "vcclDirectRootedPlan")
    out = []
    for i in range(ns.value):
        k, ph, peer, reg, roff, uoff, nb, src = steps[8 * i:8 * i + 8]
        out.append((DIRECT_STEP_KINDS[k], ph, peer, reg, roff, uoff, nb, DIRECT_STEP_SRCS[src]))
    return {"chunk_elts": geo[0], "n_chunks": geo[1], "shard_elts": geo[2], "owners": list(owners[:geo[3]]),
            "steps": out}


def ll_rooted_plan(coll: int, nranks: int, rank: int, parts, lines_per_slot: int):
    """vcclLLRootedPlan: the line layout of one rooted LL launch as `rank` sees
    it.  coll 3 broadcast / 4 reduce; parts = [(root, bytes)].  Returns (line0
    per part, stores, polls); stores / polls = [(peer, part, first line, end
    line)], part -1 = the arrival token line."""
    k = len(parts)
    roots = (ctypes.c_int * k)(*[p[0] for p in parts])
    nbytes = (ctypes.c_size_t * k)(*[p[1] for p in parts])
    cap = (nranks - 1) * (k + 1)
    line0 = (ctypes.c_int64 * k)()
    st, po = (ctypes.c_int64 * (4 * cap))(), (ctypes.c_int64 * (4 * cap))()
    ns, np_ = ctypes.c_int(), ctypes.c_int()
    check(lib().vcclLLRootedPlan(coll, nranks, rank, k, roots, nbytes, lines_per_slot, cap, line0, ctypes.byref(ns),
                                 st, ctypes.byref(np_), po), "vcclLLRootedPlan")
    return (list(line0), [tuple(st[4 * i:4 * i + 4]) for i in range(ns.value)],
            [tuple(po[4 * i:4 * i + 4]) for i in range(np_.value)])


def ll_a2a_max(threshold: int | None, ll_slot_bytes: int, ll_allowed: bool = True, any_net: bool = False,
               nranks: int = 8, has_p2p: bool = True) -> int:
    """vcclLLA2aMax: the per-pair limit of the one-hop LL all-to-all as a comm
    takes it (None: VCCL_LL_A2A_THRESHOLD from the environment; 0 = off)."""
    eff = ctypes.c_int64()
    check(lib().vcclLLA2aMax(-1 if threshold is None else threshold, ll_slot_bytes, int(ll_allowed), int(any_net),
                             nranks, int(has_p2p), ctypes.byref(eff)), "vcclLLA2aMax")
    return eff.value


def ll_a2a_plan(nranks: int, rank: int, send_bytes, recv_bytes, uniform: bool, ll_a2a_max: int,
                lines_per_slot: int) -> dict:
    """vcclLLA2aPlan: one all-to-all(v) call's split between the LL launch and
    the FIFO launch as `rank` runs it.  Returns launch, send_ll / recv_ll (per
    peer), stores / polls = [(peer, part, first line, end line)] (part 0 data,
    -1 the zero arrival token), res_sends / res_recvs (peers left to the FIFOs)."""
    n = nranks
    arr = ctypes.c_size_t * n
    ci = ctypes.c_int * n
    sll, rll, rs, rr = ci(), ci(), ci(), ci()
    st, po = (ctypes.c_int64 * (4 * n))(), (ctypes.c_int64 * (4 * n))()
    launch, nrs, nrr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().vcclLLA2aPlan(n, rank, arr(*send_bytes), arr(*recv_bytes), int(uniform), ll_a2a_max, lines_per_slot,
                              sll, rll, ctypes.byref(launch), st, po, ctypes.byref(nrs), rs, ctypes.byref(nrr), rr),
          "vcclLLA2aPlan")
    k = n - 1 if launch.value else 0
    return {"launch": bool(launch.value), "send_ll": [bool(x) for x in sll], "recv_ll": [bool(x) for x in rll],
            "stores": [tuple(st[4 * i:4 * i + 4]) for i in range(k)],
            "polls": [tuple(po[4 * i:4 * i + 4]) for i in range(k)],
            "res_sends": list(rs[:nrs.value]), "res_recvs": list(rr[:nrr.value])}


REG_STEP_KINDS = ("post", "wait", "fold", "copy")
REG_BUFS = ("send", "recv")
REG_MAX_ENTRIES = 32


def reg_max(threshold: int | None, inbox: bool = True, direct_allowed: bool = True, any_net: bool = False,
            nranks: int = 8) -> int:
    """vcclRegMax: VCCL_REG_THRESHOLD as a comm takes it (None: from the
    environment; 0 = off)."""
    eff = ctypes.c_int64()
    check(lib().vcclRegMax(-1 if threshold is None else threshold, int(inbox), int(direct_allowed), int(any_net),
                           nranks, ctypes.byref(eff)), "vcclRegMax")
    return eff.value


def reg_eligible(coll: int, count: int, dtype: int, nranks: int, effective: int, group_calls: int = 0) -> bool:
    """vcclRegEligible: whether a call launches the negotiating zero-copy kernel."""
    out = ctypes.c_int()
    check(lib().vcclRegEligible(coll, count, dtype, nranks, effective, group_calls, ctypes.byref(out)),
          "vcclRegEligible")
    return bool(out.value)


def reg_plan(coll: int, count: int, dtype: int, nranks: int, rank: int, nblocks: int) -> dict:
    """vcclRegPlan: one zero-copy launch as `rank` runs it on nblocks workgroups.
    Returns blk_elts and steps = [(kind, epoch, phase, peer, buf, peer offset,
    own offset, bytes)] with kind from REG_STEP_KINDS and buf from REG_BUFS."""
    cap = 8 * nranks + 16
    steps = (ctypes.c_int64 * (8 * cap))()
    ns, blk = ctypes.c_int(), ctypes.c_int64()
    check(lib().vcclRegPlan(coll, count, dtype, nranks, rank, nblocks, ctypes.byref(blk), cap, ctypes.byref(ns),
                            steps), "vcclRegPlan")
    out = []
    for i in range(ns.value):
        k, ep, ph, peer, buf, poff, ooff, nb = steps[8 * i:8 * i + 8]
        out.append((REG_STEP_KINDS[k], ep, ph, peer, REG_BUFS[buf], poff, ooff, nb))
    return {"blk_elts": blk.value, "steps": out}


REG_ROOTED_STEP_KINDS = REG_STEP_KINDS + ("store_root", "collect")


def reg_rooted_max(threshold: int | None, inbox: bool = True, direct_allowed: bool = True, any_net: bool = False,
                   nranks: int = 8, all_registries: bool = True) -> int:
    """vcclRegRootedMax: VCCL_REG_ROOTED_THRESHOLD as a comm takes it (None:
    from the environment); 0 = the zero-copy broadcast / reduce is off."""
    eff = ctypes.c_int64()
    check(lib().vcclRegRootedMax(-1 if threshold is None else threshold, int(inbox), int(direct_allowed),
                                 int(any_net), nranks, int(all_registries), ctypes.byref(eff)), "vcclRegRootedMax")
    return eff.value


def reg_rooted_eligible(coll: int, count: int, dtype: int, effective: int, group_calls: int = 0) -> bool:
    """vcclRegRootedEligible: whether a broadcast / reduce launches the
    negotiating zero-copy kernel."""
    out = ctypes.c_int()
    check(lib().vcclRegRootedEligible(coll, count, dtype, effective, group_calls, ctypes.byref(out)),
          "vcclRegRootedEligible")
    return bool(out.value)


def reg_rooted_plan(coll: int, count: int, dtype: int, nranks: int, rank: int, root: int, region_bytes: int,
                    nblocks: int) -> dict:
    """vcclRegRootedPlan: one zero-copy broadcast / reduce launch as `rank`
    runs it on nblocks workgroups.  Returns blk_elts (the broadcast's block
    length; 0 for a reduce), chunk_elts, n_chunks and steps = [(kind, epoch,
    phase, peer, buf, peer offset, own offset, bytes)] with kind from
    REG_ROOTED_STEP_KINDS and buf from REG_BUFS."""
    blk, chunk, nch, ns = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    args = (coll, count, dtype, nranks, rank, root, region_bytes, nblocks, ctypes.byref(blk), ctypes.byref(chunk),
            ctypes.byref(nch))
    rc = lib().vcclRegRootedPlan(*args, 0, ctypes.byref(ns), None)  # the step count first
    if ns.value == 0:
        check(rc, "vcclRegRootedPlan")
    cap = ns.value
    steps = (ctypes.c_int64 * (8 * cap))()
    check(lib().vcclRegRootedPlan(*args, cap, ctypes.byref(ns), steps), "vcclRegRootedPlan")
    out = []
    for i in range(ns.value):
        k, ep, ph, peer, buf, poff, ooff, nb = steps[8 * i:8 * i + 8]
        out.append((REG_ROOTED_STEP_KINDS[k], ep, ph, peer, REG_BUFS[buf], poff, ooff, nb))
    return {"blk_elts": blk.value, "chunk_elts": chunk.value, "n_chunks": nch.value, "steps": out}


REG_A2A_STEP_KINDS = ("post", "wait", "vote", "pull", "self")
REG_A2A_MAX_CALLS = 8


def reg_a2a_max(threshold: int | None, inbox: bool = True, direct_allowed: bool = True, any_net: bool = False,
                nranks: int = 8, has_p2p: bool = True, all_registries: bool = True) -> int:
    """vcclRegA2aMax: VCCL_REG_A2A_THRESHOLD as a comm takes it (None: from the
    environment; 0 = off)."""
    eff = ctypes.c_int64()
    check(lib().vcclRegA2aMax(-1 if threshold is None else threshold, int(inbox), int(direct_allowed), int(any_net),
                              nranks, int(has_p2p), int(all_registries), ctypes.byref(eff)), "vcclRegA2aMax")
    return eff.value


def reg_a2a_eligible(uniform: bool, pair_bytes: int, effective: int, index: int = 0) -> bool:
    """vcclRegA2aEligible: whether an all-to-all launches the negotiating
    zero-copy kernel; index = the eligible all-to-alls of its comm before it in its group."""
    out = ctypes.c_int()
    check(lib().vcclRegA2aEligible(int(uniform), pair_bytes, effective, index, ctypes.byref(out)),
          "vcclRegA2aEligible")
    return bool(out.value)


def reg_a2a_plan(nranks: int, rank: int, send_bytes, send_off, recv_off, uniform: bool, min_ctas: int = 1,
                 max_ctas: int = 64, direct_max_blocks: int = 64) -> dict:
    """vcclRegA2aPlan: one zero-copy all-to-all launch as `rank` runs it.
    send_bytes / send_off: n x n (row r = rank r's bytes / byte offsets per
    peer); recv_off: this rank's n receive offsets.  Returns n_blocks and steps
    = [(kind, epoch, phase, peer, peer offset, own offset, bytes, slice
    bytes)] with kind from REG_A2A_STEP_KINDS."""
    n = nranks
    mat = ctypes.c_size_t * (n * n)
    cap = 6 * n + 8
    steps = (ctypes.c_int64 * (8 * cap))()
    ns, nb = ctypes.c_int(), ctypes.c_int()
    check(lib().vcclRegA2aPlan(n, rank, mat(*[x for row in send_bytes for x in row]),
                               mat(*[x for row in send_off for x in row]), (ctypes.c_size_t * n)(*recv_off),
                               int(uniform), min_ctas, max_ctas, direct_max_blocks, ctypes.byref(nb), cap,
                               ctypes.byref(ns), steps), "vcclRegA2aPlan")
    out = []
    for i in range(ns.value):
        k, ep, ph, peer, poff, ooff, nbytes, blk = steps[8 * i:8 * i + 8]
        out.append((REG_A2A_STEP_KINDS[k], ep, ph, peer, poff, ooff, nbytes, blk))
    return {"n_blocks": nb.value, "steps": out}


class RegTable:
    """vcclRegTable*: the registration table on its own (no comm, no GPU)."""

    def __init__(self):
        self.handle = ctypes.c_void_p()
        check(lib().vcclRegTableNew(ctypes.byref(self.handle)), "vcclRegTableNew")

    def insert(self, addr: int, nbytes: int) -> tuple[int, int]:
        """(entry, generation); entry -1: refused (the table is full)."""
        e, g = ctypes.c_int(), ctypes.c_uint32()
        check(lib().vcclRegTableInsert(self.handle, addr, nbytes, ctypes.byref(e), ctypes.byref(g)),
              "vcclRegTableInsert")
        return e.value, g.value

    def find(self, addr: int, nbytes: int) -> tuple[int, int, int]:
        """(entry, offset in it, generation); entry -1: not registered."""
        e, o, g = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint32()
        check(lib().vcclRegTableFind(self.handle, addr, nbytes, ctypes.byref(e), ctypes.byref(o), ctypes.byref(g)),
              "vcclRegTableFind")
        return e.value, o.value, g.value

    def remove(self, entry: int) -> int:
        """The result code (ncclInvalidArgument for an entry that is not live)."""
        return lib().vcclRegTableRemove(self.handle, entry)

    def free(self):
        if self.handle:
            lib().vcclRegTableFree(self.handle)
            self.handle = ctypes.c_void_p()


A2A_FIFO, A2A_LL, A2A_DIRECT = 0, 1, 2


def direct_a2a_max(threshold: int | None, region_bytes: int, direct_allowed: bool = True, any_net: bool = False,
                   nranks: int = 8, has_p2p: bool = True) -> int:
    """vcclDirectA2aMax: the per-pair limit of the one-hop direct all-to-all as
    a comm takes it (None: VCCL_DIRECT_A2A_THRESHOLD from the environment; 0 = off)."""
    eff = ctypes.c_int64()
    check(lib().vcclDirectA2aMax(-1 if threshold is None else threshold, region_bytes, int(direct_allowed),
                                 int(any_net), nranks, int(has_p2p), ctypes.byref(eff)), "vcclDirectA2aMax")
    return eff.value


def direct_a2a_plan(nranks: int, rank: int, send_bytes, recv_bytes, uniform: bool, ll_a2a_max: int,
                    direct_a2a_max: int, lines_per_slot: int, min_ctas: int = 1, max_ctas: int = 64,
                    direct_max_blocks: int = 64) -> dict:
    """vcclDirectA2aPlan: one all-to-all(v) call's split between the LL launch,
    the direct launch and the FIFO launch as `rank` runs it.  Returns
    ll_launch / direct_launch, send_path / recv_path (per peer: A2A_FIFO,
    A2A_LL, A2A_DIRECT), n_blocks / blk_bytes (the direct launch's geometry),
    res_sends / res_recvs (peers left to the FIFOs)."""
    n = nranks
    arr = ctypes.c_size_t * n
    ci = ctypes.c_int * n
    sp, rp, rs, rr = ci(), ci(), ci(), ci()
    ll, dl, nb, nrs, nrr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    blk = ctypes.c_int64()
    check(lib().vcclDirectA2aPlan(n, rank, arr(*send_bytes), arr(*recv_bytes), int(uniform), ll_a2a_max,
                                  direct_a2a_max, lines_per_slot, min_ctas, max_ctas, direct_max_blocks, sp, rp,
                                  ctypes.byref(ll), ctypes.byref(dl), ctypes.byref(nb), ctypes.byref(blk),
                                  ctypes.byref(nrs), rs, ctypes.byref(nrr), rr), "vcclDirectA2aPlan")
    return {"ll_launch": bool(ll.value), "direct_launch": bool(dl.value), "send_path": list(sp), "recv_path": list(rp),
            "n_blocks": nb.value, "blk_bytes": blk.value,
            "res_sends": list(rs[:nrs.value]), "res_recvs": list(rr[:nrr.value])}


P2P_SEND, P2P_RECV, P2P_COPY = 0, 1, 2
P2P_ITEM_FIELDS = ("launch", "wg", "kind", "sweep", "round", "part", "peer", "call", "call2", "offset", "bytes",
                   "steps")


def p2p_plan(rank: int, nranks: int, calls, parts: int = 4, min_part_bytes: int = 64 << 10,
             step_bytes: int = 512 << 10, g_min: int = 1, g_cap: int = 0, max_works: int = 120):
    """vcclP2pPlan: the plan of one rank's grouped sends and recvs (host only).
    calls = [(kind P2P_SEND / P2P_RECV, peer, bytes[, buffer address])] in call
    order.  Returns (items, n_wgs): items as dicts of P2P_ITEM_FIELDS in
    execution order, n_wgs workgroups per direction (send workgroups
    [0, n_wgs), recv workgroups [n_wgs, 2 n_wgs)).  Raises VcclError
    (ncclInvalidUsage) for an unmatched self send or recv."""
    n = len(calls)
    ci = ctypes.c_int * max(n, 1)
    kinds, peers = ci(*[c[0] for c in calls]), ci(*[c[1] for c in calls])
    nbytes = (ctypes.c_size_t * max(n, 1))(*[c[2] for c in calls])
    buffs = (ctypes.c_uint64 * max(n, 1))(*[c[3] if len(c) > 3 else 2 * i + 1 for i, c in enumerate(calls)])
    cap = max(1, n * parts)
    items = (ctypes.c_int64 * (12 * cap))()
    n_items, n_wgs = ctypes.c_int(), ctypes.c_int()
    check(lib().vcclP2pPlan(rank, nranks, n, kinds, peers, nbytes, buffs, parts, min_part_bytes, step_bytes, g_min,
                            g_cap, max_works, cap, ctypes.byref(n_items), ctypes.byref(n_wgs), items), "vcclP2pPlan")
    return ([dict(zip(P2P_ITEM_FIELDS, items[12 * k:12 * k + 12])) for k in range(n_items.value)], n_wgs.value)


def algo_selection(algo: str | None, proto: str | None) -> tuple[int, int]:
    """vcclAlgoSelection: (force, allowed mask) for NCCL_ALGO / NCCL_PROTO strings."""
    f, a = ctypes.c_int(), ctypes.c_int()
    check(lib().vcclAlgoSelection(algo.encode() if algo is not None else None,
                                  proto.encode() if proto is not None else None, ctypes.byref(f),
                                  ctypes.byref(a)), "vcclAlgoSelection")
    return f.value, a.value


SETUP_FIELDS = ("nChannels", "stepBytes", "slotBytes", "nThreads", "algoForce", "algoAllowed", "llMaxBytes",
                "llLines", "llRsAgMaxBytes", "directMaxBytes", "directRsAgMaxBytes", "directMaxBlocks",
                "dRegionBytes", "ll128StepBytes", "ll128Threads", "ll128SlotBytes", "ll128MinBytes",
                "ll128MaxBytes", "shareBlockCap")
SETUP_SIZES = ("fifoBytes", "flagBytes", "llBytes", "inboxBytes", "ll128Bytes")


def comm_setup(nranks: int, rank: int, peers, min_ctas: int = 1, max_ctas: int = 128,
               channel: int | None = None) -> dict:
    """vcclCommSetup: what init decides for `rank` of `nranks` under the
    current environment (host only).  peers = [(pid, hostHash, busId,
    cuCount)] per rank.  Returns SETUP_FIELDS and SETUP_SIZES by name (the
    unsigned thresholds as 64-bit unsigned), anyNet, ll128Wanted, ll128Drop,
    netPeer, llChain, nRings, rsOrder, ringAt (8 x 8 each), and with
    `channel` ringPos / next / prev."""
    n = len(peers)
    pid = (ctypes.c_int * n)(*[p[0] for p in peers])
    host = (ctypes.c_uint64 * n)(*[p[1] for p in peers])
    bus = (ctypes.c_int64 * n)(*[p[2] for p in peers])
    cus = (ctypes.c_int * n)(*[p[3] for p in peers])
    setup, sizes = (ctypes.c_int64 * len(SETUP_FIELDS))(), (ctypes.c_int64 * len(SETUP_SIZES))()
    flags, net, chain = (ctypes.c_int * 3)(), (ctypes.c_int * max(nranks, 1))(), (ctypes.c_int * 8)()
    ring, tables = (ctypes.c_int * 3)(), (ctypes.c_int * 129)()
    check(lib().vcclCommSetup(nranks, rank, min_ctas, max_ctas, pid, host, bus, cus, setup, sizes, flags, net,
                              chain, channel if channel is not None else 0,
                              ring if channel is not None else None, tables), "vcclCommSetup")
    out = {k: v % (1 << 64) if k.endswith("Bytes") else v for k, v in zip(SETUP_FIELDS, setup)}
    out.update(zip(SETUP_SIZES, sizes))
    out.update(anyNet=bool(flags[0]), ll128Wanted=bool(flags[1]), ll128Drop=bool(flags[2]),
               netPeer=list(net[:nranks]), llChain=list(chain[:min(nranks, 8)]), nRings=tables[0],
               rsOrder=[list(tables[1 + 8 * k:9 + 8 * k]) for k in range(8)],
               ringAt=[list(tables[65 + 8 * k:73 + 8 * k]) for k in range(8)])
    if channel is not None:
        out.update(ringPos=ring[0], next=ring[1], prev=ring[2])
    return out


def reduce_copy(dev_op: int, dtype: int, red_arg: int, srcs, dsts, n_elts: int, stream: int = 0,
                pre_op_srcs: int = 0, post_op: bool = False, config: dict | None = None) -> None:
    """vcclReduceCopy on raw device pointers (ints)."""
    s = (ctypes.c_void_p * len(srcs))(*srcs)
    d = (ctypes.c_void_p * len(dsts))(*dsts)
    if config:
        cfg = vcclLaunchConfig(**config)
        rc = lib().vcclReduceCopyEx(dev_op, dtype, red_arg, pre_op_srcs, int(post_op), len(srcs),
                                    s, len(dsts), d, n_elts, stream, ctypes.byref(cfg))
    else:
        rc = lib().vcclReduceCopy(dev_op, dtype, red_arg, pre_op_srcs, int(post_op), len(srcs), s,
                                  len(dsts), d, n_elts, stream)
    check(rc, "vcclReduceCopy")


class Comm:
    """Owning wrapper over ncclComm_t."""

    def __init__(self, handle: int):
        self.handle = ctypes.c_void_p(handle)

    @classmethod
    def init_rank(cls, nranks: int, uid: ncclUniqueId, rank: int, config: "ncclConfig_t | None" = None) -> "Comm":
        h = ctypes.c_void_p()
        if config is None:
            rc = lib().ncclCommInitRank(ctypes.byref(h), nranks, uid, rank)
        else:
            rc = lib().ncclCommInitRankConfig(ctypes.byref(h), nranks, uid, rank, ctypes.byref(config))
        if rc == ncclInProgress:  # a non-blocking comm: poll its state, as a caller must
            st = ctypes.c_int(ncclInProgress)
            while st.value == ncclInProgress:
                check(lib().ncclCommGetAsyncError(h, ctypes.byref(st)), "ncclCommGetAsyncError")
                if st.value == ncclInProgress:
                    time.sleep(1e-3)
            rc = st.value
        check(rc, "ncclCommInitRankConfig" if config is not None else "ncclCommInitRank")
        return cls(h.value)

    @classmethod
    def init_all(cls, devices: list[int]) -> list["Comm"]:
        n = len(devices)
        hs = (ctypes.c_void_p * n)()
        dl = (ctypes.c_int * n)(*devices)
        check(lib().ncclCommInitAll(hs, n, dl), "ncclCommInitAll")
        return [cls(hs[i]) for i in range(n)]

    def _q(self, fn, what):
        v = ctypes.c_int()
        check(fn(self.handle, ctypes.byref(v)), what)
        return v.value

    @property
    def count(self) -> int:
        return self._q(lib().ncclCommCount, "ncclCommCount")

    @property
    def rank(self) -> int:
        return self._q(lib().ncclCommUserRank, "ncclCommUserRank")

    @property
    def device(self) -> int:
        return self._q(lib().ncclCommCuDevice, "ncclCommCuDevice")

    def async_error(self) -> int:
        return self._q(lib().ncclCommGetAsyncError, "ncclCommGetAsyncError")

    def all_reduce(self, send: int, recv: int, count: int, dtype: int, op: int, stream: int = 0):
        check(lib().ncclAllReduce(send, recv, count, dtype, op, self.handle, stream), "ncclAllReduce")

    def reduce_scatter(self, send: int, recv: int, recvcount: int, dtype: int, op: int,
                       stream: int = 0):
        check(lib().ncclReduceScatter(send, recv, recvcount, dtype, op, self.handle, stream),
              "ncclReduceScatter")

    def all_gather(self, send: int, recv: int, sendcount: int, dtype: int, stream: int = 0):
        check(lib().ncclAllGather(send, recv, sendcount, dtype, self.handle, stream), "ncclAllGather")

    def broadcast(self, send: int, recv: int, count: int, dtype: int, root: int, stream: int = 0):
        check(lib().ncclBroadcast(send, recv, count, dtype, root, self.handle, stream), "ncclBroadcast")

    def reduce(self, send: int, recv: int, count: int, dtype: int, op: int, root: int, stream: int = 0):
        """ncclReduce (reduce.h ring): `count` elements reduced into root's `recv`."""
        check(lib().ncclReduce(send, recv, count, dtype, op, root, self.handle, stream), "ncclReduce")

    def send(self, buf: int, count: int, dtype: int, peer: int, stream: int = 0):
        """ncclSend: `count` elements to `peer` (matched by its ncclRecv)."""
        check(lib().ncclSend(buf, count, dtype, peer, self.handle, stream), "ncclSend")

    def recv(self, buf: int, count: int, dtype: int, peer: int, stream: int = 0):
        """ncclRecv: `count` elements from `peer` (matched by its ncclSend)."""
        check(lib().ncclRecv(buf, count, dtype, peer, self.handle, stream), "ncclRecv")

    def all_to_all(self, send: int, recv: int, count: int, dtype: int, stream: int = 0):
        """ncclAllToAll (RCCL): block p of `send` (count elements) to rank p, block p of `recv` from it."""
        check(lib().ncclAllToAll(send, recv, count, dtype, self.handle, stream), "ncclAllToAll")

    def all_to_allv(self, send: int, sendcounts, sdispls, recv: int, recvcounts, rdispls, dtype: int,
                    stream: int = 0):
        """ncclAllToAllv (RCCL): per-peer counts and displacements in elements."""
        n = len(sendcounts)
        arr = ctypes.c_size_t * n
        check(lib().ncclAllToAllv(send, arr(*sendcounts), arr(*sdispls), recv, arr(*recvcounts), arr(*rdispls),
                                  dtype, self.handle, stream), "ncclAllToAllv")

    def a2a_stats(self) -> tuple[int, int, int]:
        """vcclCommA2aStats: (LL all-to-all launches, sends + recvs of this
        comm's all-to-alls that went by LL, ... that went to the p2p FIFOs)."""
        a, b, c = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
        check(lib().vcclCommA2aStats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
              "vcclCommA2aStats")
        return a.value, b.value, c.value

    def set_a2a_threshold(self, nbytes: int) -> int:
        """vcclCommSetA2aThreshold: the per-pair LL all-to-all limit for later
        calls (every rank alike); returns the effective limit."""
        eff = ctypes.c_int64()
        check(lib().vcclCommSetA2aThreshold(self.handle, nbytes, ctypes.byref(eff)), "vcclCommSetA2aThreshold")
        return eff.value

    def a2a_stats_ex(self) -> tuple[int, int, int, int, int]:
        """vcclCommA2aStatsEx: (LL launches, LL pairs, direct launches, direct
        pairs, FIFO pairs) of this comm's all-to-alls; pairs = sends + recvs."""
        v = [ctypes.c_ulonglong() for _ in range(5)]
        check(lib().vcclCommA2aStatsEx(self.handle, *[ctypes.byref(x) for x in v]), "vcclCommA2aStatsEx")
        return tuple(x.value for x in v)

    def set_direct_a2a_threshold(self, nbytes: int) -> int:
        """vcclCommSetDirectA2aThreshold: the per-pair direct all-to-all limit
        for later calls (every rank alike); returns the effective limit."""
        eff = ctypes.c_int64()
        check(lib().vcclCommSetDirectA2aThreshold(self.handle, nbytes, ctypes.byref(eff)),
              "vcclCommSetDirectA2aThreshold")
        return eff.value

    def register(self, buf: int, nbytes: int) -> int:
        """ncclCommRegister: the handle (an integer)."""
        h = ctypes.c_void_p()
        check(lib().ncclCommRegister(self.handle, buf, nbytes, ctypes.byref(h)), "ncclCommRegister")
        return h.value or 0

    def deregister(self, handle: int):
        check(lib().ncclCommDeregister(self.handle, handle), "ncclCommDeregister")

    def reg_stats(self) -> tuple[int, int, int, int, int]:
        """vcclCommRegStats (synchronises the device): eligible launches,
        zero-copy outcomes, fallback outcomes, live registrations, imported ranges."""
        a, b, c = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
        d, e = ctypes.c_int(), ctypes.c_int()
        check(lib().vcclCommRegStats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d),
                                     ctypes.byref(e)), "vcclCommRegStats")
        return a.value, b.value, c.value, d.value, e.value

    def set_reg_threshold(self, nbytes: int) -> int:
        """vcclCommSetRegThreshold: every rank alike, outside a group; the effective value."""
        eff = ctypes.c_int64()
        check(lib().vcclCommSetRegThreshold(self.handle, nbytes, ctypes.byref(eff)), "vcclCommSetRegThreshold")
        return eff.value

    def reg_rooted_stats(self) -> tuple[int, int, int]:
        """vcclCommRegRootedStats (synchronises the device): eligible broadcast
        / reduce launches, zero-copy, fallback."""
        a, b, c = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
        check(lib().vcclCommRegRootedStats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
              "vcclCommRegRootedStats")
        return a.value, b.value, c.value

    def set_reg_rooted_threshold(self, nbytes: int) -> int:
        """vcclCommSetRegRootedThreshold: every rank alike, outside a group; the effective value."""
        eff = ctypes.c_int64()
        check(lib().vcclCommSetRegRootedThreshold(self.handle, nbytes, ctypes.byref(eff)),
              "vcclCommSetRegRootedThreshold")
        return eff.value

    def reg_a2a_stats(self) -> tuple[int, int, int]:
        """vcclCommRegA2aStats (synchronises the device): eligible all-to-all
        launches, zero-copy outcomes, fallback outcomes."""
        a, b, c = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
        check(lib().vcclCommRegA2aStats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
              "vcclCommRegA2aStats")
        return a.value, b.value, c.value

    def set_reg_a2a_threshold(self, nbytes: int) -> int:
        """vcclCommSetRegA2aThreshold: every rank alike, outside a group; the effective value."""
        eff = ctypes.c_int64()
        check(lib().vcclCommSetRegA2aThreshold(self.handle, nbytes, ctypes.byref(eff)), "vcclCommSetRegA2aThreshold")
        return eff.value

    def coll_algo(self, coll: int, count: int, dtype: int) -> str:
        """vcclCommCollAlgo: "ring" | "ll" | "direct" | "ll128" | "one_rank" (coll 0 AR, 1 RS, 2 AG, 3 broadcast, 4 reduce)."""
        a = ctypes.c_int()
        check(lib().vcclCommCollAlgo(self.handle, coll, ctypes.c_size_t(count), dtype,
                                     ctypes.byref(a)), "vcclCommCollAlgo")
        return ALGO_NAMES[a.value]

    def group_algos(self, calls) -> list[str]:
        """vcclCommGroupAlgos: the path of every call of a group on this comm
        (its aggregate's); calls = [(coll 0 AR / 1 RS / 2 AG, count, dtype, op)]."""
        n = len(calls)
        ci = ctypes.c_int * n
        out = ci()
        check(lib().vcclCommGroupAlgos(self.handle, n, ci(*[c[0] for c in calls]),
                                       (ctypes.c_size_t * n)(*[c[1] for c in calls]), ci(*[c[2] for c in calls]),
                                       ci(*[c[3] for c in calls]), out), "vcclCommGroupAlgos")
        return [ALGO_NAMES[a] for a in out]

    def split(self, color: int, key: int):
        """ncclCommSplit: the new communicator of this rank's color (None for
        NCCL_SPLIT_NOCOLOR = -1).  Collective over this comm."""
        h = ctypes.c_void_p()
        check(lib().ncclCommSplit(self.handle, color, key, ctypes.byref(h), None), "ncclCommSplit")
        return Comm(h.value) if h.value else None

    def set_algo(self, algo: str | None):
        """vcclCommSetAlgo: force "ring" | "ll" | "direct" | "ll128" for later calls; None = automatic."""
        code = -1 if algo is None else {v: k for k, v in ALGO_NAMES.items()}[algo]
        check(lib().vcclCommSetAlgo(self.handle, code), "vcclCommSetAlgo")

    def launch_stats(self) -> tuple[int, int]:
        """vcclCommLaunchStats: (collectives enqueued, fused group launches)."""
        a, b = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        check(lib().vcclCommLaunchStats(self.handle, ctypes.byref(a), ctypes.byref(b)),
              "vcclCommLaunchStats")
        return a.value, b.value

    def n_channels(self) -> int:
        """The ring channel count of this communicator (vcclCommRingTrace's
        size query, which needs no trace buffer)."""
        nch = ctypes.c_int()
        lib().vcclCommRingTrace(self.handle, None, 0, ctypes.byref(nch), None)
        return nch.value

    def ring_trace(self):
        """vcclCommRingTrace: the SIMPLE ring's slot timeline of the last launch
        as a numpy structured array [nChannels, cap] (VCCL_RING_TRACE at init)."""
        import numpy as np
        nch, cap = ctypes.c_int(), ctypes.c_int()
        lib().vcclCommRingTrace(self.handle, None, 0, ctypes.byref(nch), ctypes.byref(cap))
        dt = np.dtype([("t0", "<u8"), ("t1", "<u8"), ("t2", "<u8"), ("t3", "<u8"), ("t4", "<u8"),
                       ("shape", "<u4"), ("bytes", "<u4"), ("step", "<u8"), ("tc", "<u8")])
        out = np.zeros((nch.value, cap.value), dtype=dt)
        check(lib().vcclCommRingTrace(self.handle, out.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.c_size_t(out.nbytes), None, None), "vcclCommRingTrace")
        return out

    def net_stats(self) -> tuple[int, int, int]:
        """vcclCommNetStats: (bytes sent, bytes received, connections) of the net proxy."""
        a, b, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        check(lib().vcclCommNetStats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)),
              "vcclCommNetStats")
        return a.value, b.value, n.value

    def set_fences(self, on: bool):
        """vcclCommSetFences: system-scope fences around every slot hand-off (VCCL_FENCES)."""
        check(lib().vcclCommSetFences(self.handle, int(bool(on))), "vcclCommSetFences")

    def set_ring_wave(self, on: bool | None) -> int:
        """vcclCommSetRingWave: the SIMPLE ring's per-wave slot hand-off for
        later launches (VCCL_RING_WAVE; None leaves it); returns the ring
        launches that ran the per-wave kernel so far."""
        n = ctypes.c_ulonglong(0)
        check(lib().vcclCommSetRingWave(self.handle, -1 if on is None else int(bool(on)), ctypes.byref(n)),
              "vcclCommSetRingWave")
        return int(n.value)

    def debug_set_epochs(self, ll_epoch: int, direct_epoch: int):
        """vcclCommDebugSetEpochs: overwrite the LL / direct call epochs (wrap tests)."""
        check(lib().vcclCommDebugSetEpochs(self.handle, ll_epoch, direct_epoch),
              "vcclCommDebugSetEpochs")

    def create_premulsum(self, scalar_ptr: int, dtype: int, residence: int) -> int:
        op = ctypes.c_int()
        check(lib().ncclRedOpCreatePreMulSum(ctypes.byref(op), scalar_ptr, dtype, residence,
                                             self.handle), "ncclRedOpCreatePreMulSum")
        return op.value

    def destroy_op(self, op: int):
        check(lib().ncclRedOpDestroy(op, self.handle), "ncclRedOpDestroy")

    def destroy(self):
        if self.handle:
            check(lib().ncclCommDestroy(self.handle), "ncclCommDestroy")
            self.handle = ctypes.c_void_p()

    def abort(self):
        if self.handle:
            check(lib().ncclCommAbort(self.handle), "ncclCommAbort")
            self.handle = ctypes.c_void_p()


def group_start():
    check(lib().ncclGroupStart(), "ncclGroupStart")


def group_end():
    check(lib().ncclGroupEnd(), "ncclGroupEnd")
