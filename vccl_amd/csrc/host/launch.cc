// Task -> stream ordering -> work descriptors -> kernel launch.
//
// The launch side of the reference's dispatch surface (taskAppend
// enqueue.cc:2315-2442 onwards, the nRanks==1 shortcut ncclLaunchOneRank
// onerank.cu:47-83) for one node: the planner picks a path per call
// (select_algo: one-shot LL, LL128 ring, two-shot direct, SIMPLE ring over
// xGMI); the ring's channel partition is VCCL's own cbd split (cbd_schedule,
// ring.hpp cbd_part).  Each comm's calls of a group are laid out on VCCL's
// multi-task plan (group_plan) and launched in plan order, runs of one path
// fused into one launch (launch_group).
#include "launch.h"

#include <algorithm>

#include "../../../include/vccl_device.h"
#include "../device/dispatch.hpp"
#include "../device/launch.hpp"
#include "../device/p2p_launch.hpp"
#include "../device/ring_launch.hpp"
#include "regcomm.h"

namespace vccl {

// The host uses one set of collective codes: Coll (plan.h) is what the
// launchers of ring_launch.hpp / launch.hpp take as kColl*.
static_assert((int)kAllReduce == (int)kCollAllReduce, "Coll and kColl* are one enumeration");
static_assert((int)kReduceScatter == (int)kCollReduceScatter, "Coll and kColl* are one enumeration");
static_assert((int)kAllGather == (int)kCollAllGather, "Coll and kColl* are one enumeration");
static_assert((int)kBroadcast == (int)kCollBroadcast, "Coll and kColl* are one enumeration");
static_assert((int)kReduce == (int)kCollReduce, "Coll and kColl* are one enumeration");
// ... and one set of device op codes: plan.cc encodes ops as vcclDevRedOp_t.
static_assert((int)OP_SUM == (int)vcclDevSum && (int)OP_PROD == (int)vcclDevProd &&
                  (int)OP_MINMAX == (int)vcclDevMinMax && (int)OP_PREMULSUM == (int)vcclDevPreMulSum &&
                  (int)OP_SUMPOSTDIV == (int)vcclDevSumPostDiv,
              "OP_* and vcclDevRedOp_t are one enumeration");

// Order launches of one comm across different user streams (the reference
// serialises through its internal strong stream, enqueue.cc:1445-1548).
// The null stream (0) is a valid user stream, so "no launch yet" is a flag of
// its own, not a null lastStream.
//
// Graph capture (the reference's strong streams track capture the same way,
// misc/strongstream.cc): launches on a capturing stream are ordered only
// against earlier launches of the SAME capture, through an event recorded
// inside it (a fork/join inside the graph); they neither wait on the eager
// lastLaunch event (recorded outside the capture) nor overwrite it, so eager
// work before and after the capture keeps its own ordering.
struct CaptureState {
  bool active;
  unsigned long long id;
};
static ncclResult_t capture_state(hipStream_t s, CaptureState* cs) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  HIPCHECK(hipStreamGetCaptureInfo(s, &st, &id));
  cs->active = st == hipStreamCaptureStatusActive;
  cs->id = id;
  return ncclSuccess;
}
// The ordering state of capture `id`: comm->caps is a pool of kMaxCaptures
// entries created at init (no HIP object is created during a capture); a new
// id takes the least recently used entry whose capture has ended.  When every
// entry still belongs to a live capture, the call fails (ncclInvalidUsage)
// rather than silently dropping a live capture's ordering.
// A capture is live while its last stream still captures under its id; a
// stream destroyed since reads as ended (HIP validates the handle and fails
// the query — tests/mp_graph_worker.py captures_on_destroyed_streams).
static bool capture_live(const ncclComm::CapOrder& c) {
  if (!c.used || !c.has) return false;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(c.last, &st, &id) != hipSuccess) return false;
  return st == hipStreamCaptureStatusActive && id == c.id;
}
static ncclResult_t capture_entry(ncclComm* comm, unsigned long long id, bool create, ncclComm::CapOrder** out) {
  *out = nullptr;
  auto& caps = comm->caps;
  for (size_t i = 0; i < caps.size(); i++) {
    if (caps[i].used && caps[i].id == id) {
      std::rotate(caps.begin(), caps.begin() + i, caps.begin() + i + 1);  // to the front
      *out = &caps[0];
      return ncclSuccess;
    }
  }
  if (!create || caps.empty()) return ncclSuccess;
  for (size_t i = caps.size(); i-- > 0;) {  // least recently used first
    if (capture_live(caps[i])) continue;
    std::rotate(caps.begin(), caps.begin() + i, caps.begin() + i + 1);
    caps[0].id = id;
    caps[0].used = true;
    caps[0].last = nullptr;
    caps[0].has = false;
    *out = &caps[0];
    return ncclSuccess;
  }
  VWARN("more than %d stream captures are active on this communicator at once", (int)caps.size());
  return ncclInvalidUsage;
}
// One capture query per call: stream_order fills `cs`, stream_mark and
// stream_last_event reuse it (the capture state of s cannot change between
// them — the caller holds the thread).
static ncclResult_t stream_order(ncclComm* comm, hipStream_t s, CaptureState* cs) {
  NCCLCHECK(capture_state(s, cs));
  if (cs->active) {
    ncclComm::CapOrder* c;
    NCCLCHECK(capture_entry(comm, cs->id, true, &c));  // reserved before the launch
    if (c && c->has && c->last != s) HIPCHECK(hipStreamWaitEvent(s, c->ev, 0));
    return ncclSuccess;
  }
  if (comm->hasLastLaunch && comm->lastStream != s)
    HIPCHECK(hipStreamWaitEvent(s, comm->lastLaunch, 0));
  return ncclSuccess;
}
// The event the launches of an eager call bind to their kernel's completion
// (hipExtLaunchKernel stopEvent): the comm's ordering event, recorded by the
// kernel's own completion signal instead of a separate marker packet — a
// marker costs ~5 us of GPU time per call on MI355X (profiles/r04q: LL 8 B
// 10.1 -> 5.7 us per call back to back, 1 MiB ring 17.5 -> 12.7).
// VCCL_LAUNCH_EVENT=0: record markers.  Captures keep markers (graph edges).
static hipEvent_t stop_event(ncclComm* comm, const CaptureState& cs) {
  static const bool bind = param_int("LAUNCH_EVENT", 1) != 0;
  return bind && !cs.active ? comm->lastLaunch : nullptr;
}
static ncclResult_t stream_mark(ncclComm* comm, hipStream_t s, const CaptureState& cs) {
  if (cs.active) {
    ncclComm::CapOrder* c;
    NCCLCHECK(capture_entry(comm, cs.id, true, &c));
    if (!c) return ncclInternalError;
    HIPCHECK(hipEventRecord(c->ev, s));
    c->last = s;
    c->has = true;
    return ncclSuccess;
  }
  // VCCL_DEBUG_NO_MARK=1: no marker packet (measurement only: correct for a
  // comm driven from ONE stream, where stream order suffices).  The launch is
  // still tracked: through the stop event when the kernel bound
  // it, else by its stream, so destroy / finalize / abort still wait for it.
  static const bool noMark = param_int("DEBUG_NO_MARK", 0) != 0;
  const bool bound = stop_event(comm, cs) != nullptr;
  if (!noMark && !bound) HIPCHECK(hipEventRecord(comm->lastLaunch, s));  // else bound to the kernel
  comm->lastUnmarked = noMark && !bound;
  comm->lastStream = s;
  comm->hasLastLaunch = true;
  return ncclSuccess;
}
// The event stream_mark just recorded on s (for joining other streams).
static hipEvent_t stream_last_event(ncclComm* comm, const CaptureState& cs) {
  return cs.active ? comm->caps[0].ev : comm->lastLaunch;
}

// ncclLaunchOneRank (onerank.cu:47-83): a copy, or the PreMulSum kernel.  An
// in-place call without a preOp enqueues nothing.
static ncclResult_t launch_one_rank(const Task& t) {
  const size_t bytes = t.count * (size_t)type_size(t.datatype);
  RCArgs a = {};
  a.srcs[0] = (const char*)t.sendbuff;
  a.dsts[0] = (char*)t.recvbuff;
  a.nSrcs = a.nDsts = 1;
  if (is_copy_coll(t.coll) || t.devOp != OP_PREMULSUM) {  // AG: a plain copy
    if (t.recvbuff == t.sendbuff) return ncclSuccess;
    // Small buckets: the library's own byte-copy kernel (one launch) — a
    // hipMemcpyAsync D2D costs more host time than the whole 1 KiB copy
    // (BASELINE config 1).  Large ones: the runtime's copy engine path.
    static const size_t kKernelCopyMax = (size_t)param_int("ONERANK_KERNEL_COPY_BYTES", 1 << 20);
    if (bytes <= kKernelCopyMax) {
      hipError_t e = reduce_copy_launch(OP_COPY, (int)ncclUint8, 0, a, (int64_t)bytes, nullptr, t.stream);
      return e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
    }
    HIPCHECK(hipMemcpyAsync(t.recvbuff, t.sendbuff, bytes, hipMemcpyDeviceToDevice, t.stream));
    return ncclSuccess;
  }
  a.preOpSrcs = 1;  // onerank.cu:43: PreOpSrcs=1, postOp=true
  a.postOp = 1;
  a.argPtr = t.argPtr;
  hipError_t e = reduce_copy_launch(t.devOp, (int)t.datatype, t.arg, a, (int64_t)t.count, nullptr, t.stream);
  return e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

AlgoPolicy policy_of(const ncclComm* c) {
  return AlgoPolicy{.nRanks = c->nRanks, .algoForce = c->algoForce,
                    .llSlotBytes = c->llBuf ? (int64_t)c->llLines * 8 : 0,
                    .llMax = c->llMaxBytes, .llRsAgMax = c->llRsAgMaxBytes,
                    .ll128 = c->ll128Buf != nullptr, .ll128Min = c->ll128MinBytes, .ll128Max = c->ll128MaxBytes,
                    .direct = c->dPeers != nullptr, .directMax = c->directMaxBytes,
                    .directRsAgMax = c->directRsAgMaxBytes, .llRootedMax = c->llRootedMaxBytes,
                    .directRootedMax = c->directRootedMaxBytes};
}

int kernel_type_of_call(int coll, int devOp, ncclDataType_t datatype) {
  return is_copy_coll(coll) ? (int)K_U8 : kernel_type_of(devOp, (int)datatype);
}

// A call's partition: its place in its group's plan (launch_planned, under
// the protocol of the path its aggregate took — the caller asks for that
// same protocol), else the plan of the call alone under `proto`.
static CbdPlan task_plan(const Task& t, int proto) {
  const ncclComm* comm = t.comm;
  if (t.planned) return t.plan;
  const CallSize sz = call_size(t.coll, t.count, t.datatype);
  const bool ll128 = proto == kProtoLL128;
  return cbd_schedule(t.coll, sz.count, sz.eltSize, comm->nRanks, comm->nChannels, proto,
                      ll128 ? comm->ll128StepBytes : proto == kProtoLL ? kLLStepBytes : comm->stepBytes,
                      ll128 ? comm->ll128Threads : comm->nThreads);
}

// What every work descriptor takes from its call's comm and op.
template <class Work>
static void fill_op_fields(Work& w, const Task& t) {
  w.comm = t.comm->devComm;
  w.redArg = t.arg;
  w.redArgPtr = t.argPtr;  // ncclScalarDevice: dereferenced by the kernel (nccl.h.in:255-262)
  w.redArgBytes = type_size(t.datatype);
  w.preOp = t.devOp == OP_PREMULSUM;
  w.nRanks = t.comm->nRanks;
}

// The ring work of one call (its kernel element type and device op too).
static ncclResult_t ring_work_of(const Task& t, bool ll128, RingWork* out, int* ktOut, int* devOpOut) {
  ncclComm* comm = t.comm;
  RingWork w{};
  fill_op_fields(w, t);
  w.channels = comm->devChannels;
  w.slotBytes = comm->slotBytes;
  const int kt = kernel_type_of_call(t.coll, t.devOp, t.datatype);
  if (kt < 0) return ncclInvalidArgument;
  const CbdPlan p = task_plan(t, ll128 ? kProtoLL128 : kProtoSimple);
  if (p.channelHi >= comm->nChannels || p.channelLo < 0 || p.channelLo > p.channelHi)
    return ncclInternalError;
  const uint64_t count = (uint64_t)call_size(t.coll, t.count, t.datatype).count;  // copies: bytes
  w.nChannels = p.channelHi + 1;  // idle channels above channelHi are not launched
  w.ll128SlotBytes = ll128 ? comm->ll128SlotBytes : 0;
  // the call's own part of the work: buffers, count, root and its partition
  *out = ring_work_with(w, RingPart{t.sendbuff, t.recvbuff, count, t.root, p.channelLo, p.channelHi, p.countLo,
                                    p.countMid, p.countHi, p.chunkLo, p.chunkMid, p.chunkHi});
  *ktOut = kt;
  *devOpOut = is_copy_coll(t.coll) ? (int)OP_COPY : t.devOp;
  return ncclSuccess;
}

// The per-wave SIMPLE ring kernels exist for the bandwidth regime only
// (ring_kernels.hip PART 4): sums over f32 / f16 / bf16 and the byte-copy
// all-gather / broadcast.
static bool ring_wave_kernel(int kt, int devOp, int coll) {
  if (coll == kCollAllGather || coll == kCollBroadcast) return kt == K_U8;
  return devOp == OP_SUM && (kt == K_F32 || kt == K_F16 || kt == K_BF16);
}

// Dispatch a typed launcher over the kernel element type.
template <class F>
static hipError_t by_kernel_type(int kt, F&& f) {
  switch (kt) {
    case K_U8: return f.template operator()<K_U8>();
    case K_U32: return f.template operator()<K_U32>();
    case K_U64: return f.template operator()<K_U64>();
    case K_F16: return f.template operator()<K_F16>();
    case K_F32: return f.template operator()<K_F32>();
    case K_F64: return f.template operator()<K_F64>();
    case K_BF16: return f.template operator()<K_BF16>();
    case K_F8E4M3: return f.template operator()<K_F8E4M3>();
    case K_F8E5M2: return f.template operator()<K_F8E5M2>();
  }
  return hipErrorInvalidValue;
}

// 1 .. kRingMaxWorks ring calls of one comm with the same collective, kernel
// type and op (fusable) in one launch on ts[0].stream; SIMPLE or LL128.  A
// SIMPLE launch takes the per-wave hand-off when the comm asks for it
// (VCCL_RING_WAVE / vcclCommSetRingWave) and the kernel exists: same FIFOs,
// partition and fold, so the two mix freely on a channel.
static ncclResult_t launch_ring(const Task* ts, int nTasks, bool ll128, hipEvent_t stop) {
  const Task& t = ts[0];
  ncclComm* comm = t.comm;
  if (nTasks < 1 || nTasks > kRingMaxWorks) return ncclInternalError;
  if (ll128 && !comm->ll128Buf) return ncclInternalError;
  RingBatch b{};
  int kt = -1, devOp = -1;
  NCCLCHECK(ring_work_of(t, ll128, &b.w, &kt, &devOp));
  for (int i = 1; i < nTasks; i++) {
    RingWork wi;
    int kti, opi;
    NCCLCHECK(ring_work_of(ts[i], ll128, &wi, &kti, &opi));
    if (kti != kt || opi != devOp) return ncclInternalError;
    b.more[i - 1] = ring_part_of(wi);
    b.w.nChannels = std::max(b.w.nChannels, wi.nChannels);
  }
  b.nParts = nTasks;
  const int v = ll128 ? kRingVariantLL128
                : comm->ringWave && ring_wave_kernel(kt, devOp, t.coll) ? kRingVariantWave : kRingVariantSimple;
  const hipError_t e = by_kernel_type(
      kt, [&]<int K>() { return ring_launch_any<K>(v, t.coll, devOp, b, comm->nThreads, t.stream, stop); });
  if (e != hipSuccess) {
    VWARN("ring kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  if (v == kRingVariantWave) comm->waveLaunches++;
  return ncclSuccess;
}

// The cbd partition of a reduce-scatter's block, for the one-hop LL / direct
// reduce-scatters' per-channel fold order: the ring's, under VCCL's protocol
// for the path (LL: the LL ring's cells, enqueue.cc:599; direct: SIMPLE).
static CbdLite rs_cbd(const Task& t, int proto) {
  const CbdPlan p = task_plan(t, proto);
  return CbdLite{p.channelLo, p.channelHi, p.countLo, p.countMid, (int64_t)t.count};
}

// One-hop LL collectives: `ts` holds 1 .. kLLMaxParts calls of one comm with
// the same collective, type and op (fusable) whose lines — all-reduce,
// broadcast (any roots) and reduce (any roots): the call's, reduce-scatter /
// all-gather: one rank's block's — fit one slot;
// they run as one launch on ts[0].stream (the caller orders the other
// streams around it).
static int64_t ll_lines_of(const Task& t) {
  return ((int64_t)t.count * type_size(t.datatype) + 7) / 8;
}
static int64_t ll_lines_of(int64_t bytes) { return (bytes + 7) / 8; }  // ... of a payload given in bytes
// A bounded grid (256-thread workgroups, each thread looping over lines):
// one workgroup per 256 lines, within the comm's CTA bounds (minCTAs /
// maxCTAs, default 1 / 128), and never above VCCL_LL_MAX_BLOCKS (256): every
// rank's LL workgroups must be resident at once for the peers' spins to
// complete, so that co-residency cap is applied LAST (tests that
// put 8 ranks on ONE GPU lower it).
static int ll_grid(const ncclComm* comm, int64_t lines) {
  int maxBlocks = (int)std::max<int64_t>(1, param_int("LL_MAX_BLOCKS", 256));
  if (comm->shareBlockCap > 0) maxBlocks = std::min(maxBlocks, comm->shareBlockCap);
  int grid = (int)std::max<int64_t>(1, (lines + 255) / 256);
  grid = std::max(std::min(grid, comm->maxCTAs), comm->minCTAs);
  return std::max(1, std::min(grid, maxBlocks));
}
static ncclResult_t launch_ll(const Task* ts, int nTasks, hipEvent_t stop) {
  const Task& t = ts[0];
  ncclComm* comm = t.comm;
  LLWork w{};
  fill_op_fields(w, t);
  w.rank = comm->rank;
  w.linesPerSlot = comm->llLines;
  w.localBuf = comm->llBuf;
  for (int r = 0; r < comm->nRanks; r++) w.peerBuf[r] = comm->llPeer[r];
  if (nTasks < 1 || nTasks > kLLMaxParts) return ncclInternalError;
  const bool rooted = t.coll == kBroadcast || t.coll == kReduce;
  int64_t lines = 0;
  for (int i = 0; i < nTasks; i++) {
    if (ts[i].coll != t.coll) return ncclInternalError;
    w.parts[i].send = (const char*)ts[i].sendbuff;
    w.parts[i].recv = (char*)ts[i].recvbuff;
    w.parts[i].nbytes = (int64_t)ts[i].count * type_size(ts[i].datatype);
    w.parts[i].line0 = lines;
    // reduce: the call's own partition, as the reduce-scatter takes its block's
    if (t.coll == kReduceScatter || t.coll == kReduce) w.parts[i].cbd = rs_cbd(ts[i], kProtoLL);
    lines += ll_lines_of(ts[i]);
  }
  w.nParts = nTasks;
  w.nLines = lines;
  if (lines > comm->llLines) return ncclInternalError;
  if (rooted) {
    // the layout is ll_rooted_plan's (plan.cc): per-part roots, every part
    // with at least one line (a zero-count call never becomes a task)
    if (comm->nRanks > kOrderMaxRanks) return ncclInternalError;
    std::vector<int> roots(nTasks);
    std::vector<int64_t> bytes(nTasks);
    for (int i = 0; i < nTasks; i++) roots[i] = ts[i].root, bytes[i] = w.parts[i].nbytes;
    LLRootedPlanOut lp;
    if (ll_rooted_plan(t.coll, comm->nRanks, comm->rank, roots, bytes, comm->llLines, &lp) != ncclSuccess ||
        lp.nLines != lines)
      return ncclInternalError;
    for (int i = 0; i < nTasks; i++) {
      if (lp.line0[i] != w.parts[i].line0 || bytes[i] <= 0) return ncclInternalError;
      w.partRoot[i] = (int8_t)roots[i];
    }
  }
  const bool copy = is_copy_coll(t.coll);
  const int kt = copy ? K_U8 : kernel_type_of(t.devOp, (int)t.datatype);
  if (kt < 0) return ncclInvalidArgument;
  const int grid = ll_grid(comm, lines);
  const int devOp = copy ? OP_COPY : t.devOp;
  const hipError_t e = by_kernel_type(kt, [&]<int K>() { return ll_launch<K>(t.coll, devOp, w, grid, t.stream, stop); });
  if (e != hipSuccess) {
    VWARN("LL kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

// The direct work of one call (direct.hpp): two-shot all-reduce, one-hop
// reduce-scatter / all-gather, two-hop broadcast / reduce (chunk and shard
// from plan.cc direct_rooted_plan, whose step list is the kernels' phase
// order).  `blkForce` > 0 imposes the block length (a fused batch's common
// geometry, launch_direct).
static ncclResult_t direct_work_of(const Task& t, DirectWork* out, int* ktOut, int* devOpOut, int64_t blkForce = 0) {
  ncclComm* comm = t.comm;
  const int n = comm->nRanks;
  const bool ag = is_copy_coll(t.coll);
  const bool rooted = t.coll == kBroadcast || t.coll == kReduce;
  const auto [count, esz] = call_size(t.coll, t.count, t.datatype);  // all-gather / broadcast: bytes
  const int64_t eltAlign = std::max<int64_t>(1, 16 / esz);
  DirectWork w{};
  fill_op_fields(w, t);
  w.peers = comm->dPeers;
  w.sendbuff = t.sendbuff;
  w.recvbuff = t.recvbuff;
  w.count = (uint64_t)count;
  w.rank = comm->rank;
  w.root = rooted ? t.root : 0;
  const int64_t regionElts = (comm->dRegionBytes - 16) / esz;
  int64_t shard0;
  if (rooted) {
    if (n < 2 || t.root < 0 || t.root >= n) return ncclInternalError;
    DirectRootedPlanOut rp;
    if (direct_rooted_plan(t.coll, n, comm->rank, t.root, count, esz, comm->dRegionBytes, -1, &rp) != ncclSuccess)
      return ncclInternalError;
    w.chunkElts = rp.chunkElts;
    shard0 = direct_shard_elts(w.chunkElts, (int)rp.owner.size(), eltAlign);
    // reduce: the call's own partition under SIMPLE, as the ring reduce folds it
    if (t.coll == kReduce) w.cbd = rs_cbd(t, kProtoSimple);
  } else if (t.coll == kAllReduce) {
    // Chunk: as many elements as fit one shard per inbox region, a multiple
    // of n x 16 bytes; the shard of the largest chunk is cut into blocks.
    const int64_t chunkMax = regionElts * n / (n * eltAlign) * (n * eltAlign);
    w.chunkElts = std::min<int64_t>(count, chunkMax);
    shard0 = direct_shard_elts(w.chunkElts, n, eltAlign);
    // the ring's partition of this bucket: phase 2 folds every element in the
    // order VCCL's ring all-reduce gives it on these channels (ar_chunk_of)
    const CbdPlan p = task_plan(t, kProtoSimple);
    w.cbd = CbdLite{p.channelLo, p.channelHi, p.countLo, p.countMid, count};
    w.arChunk = p.chunkLo;
  } else {
    // Reduce-scatter / all-gather: a chunk is a range of ONE rank's block
    // (count elements) that fits a region; it is cut into blocks directly.
    w.chunkElts = std::min<int64_t>(count, regionElts / eltAlign * eltAlign);
    shard0 = w.chunkElts;
    if (t.coll == kReduceScatter) w.cbd = rs_cbd(t, kProtoSimple);
  }
  w.nChunks = (int)((count + w.chunkElts - 1) / w.chunkElts);
  // Blocks of >= 16 KiB within the CTA bounds, then the co-residency caps (plan.h).
  w.blkElts = direct_blk_elts(shard0, esz, comm->minCTAs, comm->maxCTAs, comm->directMaxBlocks);
  if (blkForce > 0) {
    if (blkForce < w.blkElts || blkForce % eltAlign) return ncclInternalError;
    w.blkElts = blkForce;
  }
  w.nBlocks = (int)((shard0 + w.blkElts - 1) / w.blkElts);
  w.regionBytes = comm->dRegionBytes;
  if (shard0 * esz > w.regionBytes || w.nBlocks > kDirectMaxBlocks || w.nBlocks < 1)
    return ncclInternalError;
  const int kt = ag ? K_U8 : kernel_type_of(t.devOp, (int)t.datatype);
  if (kt < 0) return ncclInvalidArgument;
  *out = w;
  *ktOut = kt;
  *devOpOut = ag ? OP_COPY : t.devOp;
  return ncclSuccess;
}

// 1 .. kDirectMaxWorks direct calls of one comm with the same collective,
// kernel type and op in one launch on ts[0].stream (the largest part's grid).
// Every part of a batch uses ONE block length (the largest part's): block b
// then covers the same inbox bytes [b * blkElts, (b + 1) * blkElts) in every
// part, so the per-block flags that order a part's region reuse also order
// the next part's (a kernel boundary no longer separates them) — with
// per-part lengths, workgroup b's next-part scatter could overwrite bytes a
// peer's workgroup b' was still folding.
static ncclResult_t launch_direct(const Task* ts, int nTasks, hipEvent_t stop) {
  const Task& t = ts[0];
  if (nTasks < 1 || nTasks > kDirectMaxWorks) return ncclInternalError;
  DirectBatch b{};
  int kt = -1, devOp = -1;
  int64_t blk = 0;
  for (int i = 0; i < nTasks; i++) {
    DirectWork wi;
    int kti, opi;
    NCCLCHECK(direct_work_of(ts[i], &wi, &kti, &opi));
    if (i > 0 && (kti != kt || opi != devOp)) return ncclInternalError;
    kt = kti;
    devOp = opi;
    blk = std::max(blk, wi.blkElts);
  }
  NCCLCHECK(direct_work_of(t, &b.w, &kt, &devOp, nTasks > 1 ? blk : 0));
  for (int i = 1; i < nTasks; i++) {
    DirectWork wi;
    int kti, opi;
    NCCLCHECK(direct_work_of(ts[i], &wi, &kti, &opi, blk));
    b.more[i - 1] = direct_part_of(wi);
    b.w.nBlocks = std::max(b.w.nBlocks, wi.nBlocks);
  }
  b.nParts = nTasks;
  const hipError_t e = by_kernel_type(kt, [&]<int K>() { return direct_launch<K>(t.coll, devOp, b, t.stream, stop); });
  if (e != hipSuccess) {
    VWARN("direct kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

// Zero-copy over registered buffers (device/direct_reg.hpp).  Eligibility is
// plan.cc reg_eligible's: from the call's arguments and comm-wide values alone,
// so every rank launches the negotiating kernel for the same calls, ahead of
// select_algo's choice and at any size above the threshold; its fallback is
// the staged direct path at any size, decided on the device.
static bool reg_task_eligible(const Task& t) {
  const ncclComm* c = t.comm;
  return c->reg && c->dPeers &&
         reg_eligible(t.coll, (int64_t)t.count, type_size(t.datatype), c->nRanks, c->reg->threshold, t.groupColls);
}
// The rooted calls' rule (plan.cc reg_rooted_eligible), on the comm's own
// threshold: a broadcast or reduce, alone or its comm's only collective of its
// group; the fallback is the staged direct rooted part at any size, whether or
// not VCCL_DIRECT_ROOTED_THRESHOLD is set.
static bool reg_rooted_task_eligible(const Task& t) {
  const ncclComm* c = t.comm;
  return c->reg && c->reg->rootedStats && c->dPeers &&
         reg_rooted_eligible(t.coll, (int64_t)t.count, type_size(t.datatype), c->regRootedMaxBytes, t.groupColls);
}
// What the two zero-copy launches share.  The staged geometry is
// direct_work_of's (the fallback runs it as it is); the import table is brought
// up to date first (nothing in the steady state, nothing inside a capture).
static ncclResult_t reg_work_of(const Task& t, DirectRegWork* rw, int* kt, int* devOp) {
  ncclComm* comm = t.comm;
  CaptureState cs{false, 0};
  NCCLCHECK(capture_state(t.stream, &cs));
  NCCLCHECK(reg_refresh(comm, cs.active));
  NCCLCHECK(direct_work_of(t, &rw->w, kt, devOp));
  rw->reg = comm->reg->tabDev;
  return ncclSuccess;
}
// The descriptor: this rank's registrations, as of now, of the buffers of
// `needMine` — those some peer will read; the others travel as kRegNone and
// are never looked up (a broadcast non-root's sendbuff may be NULL).
static void reg_describe_mine(const Task& t, DirectRegWork* rw, uint64_t sendBytes, uint64_t recvBytes) {
  RegDesc& d = rw->mine;
  d.sendBytes = sendBytes;
  d.recvBytes = recvBytes;
  d.sendEntry = d.recvEntry = kRegNone;
  if (rw->needMine & kRegSend) reg_describe(t.comm, t.sendbuff, sendBytes, &d.sendEntry, &d.sendGen, &d.sendOff);
  if (rw->needMine & kRegRecv) reg_describe(t.comm, t.recvbuff, recvBytes, &d.recvEntry, &d.recvGen, &d.recvOff);
}
// The zero-copy block length is plan.cc reg_plan's on the staged grid.
static ncclResult_t launch_direct_reg(const Task& t, hipEvent_t stop) {
  ncclComm* comm = t.comm;
  DirectRegWork rw{};
  int kt = -1, devOp = -1;
  NCCLCHECK(reg_work_of(t, &rw, &kt, &devOp));
  const auto [count, esz] = call_size(t.coll, t.count, t.datatype);
  RegPlanOut rp;
  NCCLCHECK(reg_plan(t.coll, comm->nRanks, comm->rank, count, esz, rw.w.nBlocks, &rp));
  rw.stats = comm->reg->stats;
  rw.zcBlkElts = rp.blkElts;
  // what the peers read of mine: the whole input; the all-reduce's output too
  rw.needMine = rw.needPeer = rw.needRootPeer = t.coll == kAllReduce ? kRegSend | kRegRecv : kRegSend;
  reg_describe_mine(t, &rw, (uint64_t)(t.coll == kReduceScatter ? count * comm->nRanks : count) * (uint64_t)esz,
                    t.coll == kAllReduce ? (uint64_t)count * (uint64_t)esz : 0);
  const hipError_t e =
      by_kernel_type(kt, [&]<int K>() { return direct_reg_launch<K>(t.coll, devOp, rw, t.stream, stop); });
  if (e != hipSuccess) {
    VWARN("zero-copy direct kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}
// Broadcast / reduce (device/direct_reg.hpp reg_broadcast_zc / reg_reduce_zc):
// plan.cc reg_rooted_plan gives the broadcast's block length on the staged grid
// and must agree with the staged chunking the reduce runs on.  Roles: the
// broadcast root announces sendbuff and reads nobody; a non-root announces
// recvbuff (n > 2: the other non-roots pull its shard from there), reads the
// root's sendbuff and the other non-roots' recvbuffs; a reduce announces and
// reads sendbuff everywhere.
static ncclResult_t launch_direct_reg_rooted(const Task& t, hipEvent_t stop) {
  ncclComm* comm = t.comm;
  const int n = comm->nRanks;
  DirectRegWork rw{};
  int kt = -1, devOp = -1;
  NCCLCHECK(reg_work_of(t, &rw, &kt, &devOp));
  const auto [count, esz] = call_size(t.coll, t.count, t.datatype);
  RegRootedPlanOut rp;
  NCCLCHECK(reg_rooted_plan(t.coll, n, comm->rank, t.root, count, esz, comm->dRegionBytes, rw.w.nBlocks, &rp));
  if (t.coll == kReduce && (rp.nChunks != rw.w.nChunks || rp.chunkElts != rw.w.chunkElts)) return ncclInternalError;
  rw.stats = comm->reg->rootedStats;
  rw.zcBlkElts = rp.blkElts;
  const bool isRoot = comm->rank == t.root;
  if (t.coll == kReduce) {
    rw.needMine = rw.needPeer = rw.needRootPeer = kRegSend;
  } else {
    rw.needMine = isRoot ? kRegSend : n > 2 ? kRegRecv : 0;
    rw.needPeer = isRoot ? 0 : kRegRecv;
    rw.needRootPeer = isRoot ? 0 : kRegSend;
  }
  const uint64_t bytes = (uint64_t)count * (uint64_t)esz;
  reg_describe_mine(t, &rw, bytes, bytes);
  const hipError_t e =
      by_kernel_type(kt, [&]<int K>() { return direct_reg_launch_rooted<K>(t.coll, devOp, rw, t.stream, stop); });
  if (e != hipSuccess) {
    VWARN("zero-copy rooted kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

// A call's path: select_algo on the comm's thresholds.
static int choose_algo(const Task& t) {
  return select_algo(policy_of(t.comm), t.coll, type_size(t.datatype), (int64_t)t.count);
}

// 1 .. max_parts(algo) fusable calls as one launch of path `algo`.
constexpr int kAlgoDirectReg = 100;  // launch.cc only: one eligible call, the zero-copy kernel
constexpr int kAlgoDirectRegRooted = 101;  // ... a broadcast / reduce
// The zero-copy path of a call that is eligible for one, else `algo`.
static int reg_algo_or(const Task& t, int algo) {
  return reg_task_eligible(t) ? kAlgoDirectReg : reg_rooted_task_eligible(t) ? kAlgoDirectRegRooted : algo;
}
static ncclResult_t launch_path(int algo, const Task* ts, int n, hipEvent_t stop) {
  if (algo == kAlgoDirectReg) return n == 1 ? launch_direct_reg(ts[0], stop) : ncclInternalError;
  if (algo == kAlgoDirectRegRooted) return n == 1 ? launch_direct_reg_rooted(ts[0], stop) : ncclInternalError;
  return algo == kAlgoLL ? launch_ll(ts, n, stop)
         : algo == kAlgoDirect ? launch_direct(ts, n, stop) : launch_ring(ts, n, algo == kAlgoRingLL128, stop);
}

ncclResult_t launch_task(const Task& t) {
  ncclComm* comm = t.comm;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  ncclResult_t r;
  if (comm->nRanks == 1) {
    // One rank: the copy / PreMulSum kernel goes straight onto the caller's
    // stream with no cross-stream ordering, as ncclLaunchOneRank does
    // (enqueue.cc:2386-2388 — it bypasses the plan and the strong stream); an
    // in-place call without a preOp enqueues nothing.
    r = launch_one_rank(t);
  } else {
    CaptureState cs{false, 0};
    r = stream_order(comm, t.stream, &cs);
    if (r == ncclSuccess) {
      const int reg = reg_algo_or(t, -1);
      r = launch_path(reg >= 0 ? reg : choose_algo(t), &t, 1, stop_event(comm, cs));
    }
    if (r == ncclSuccess) r = stream_mark(comm, t.stream, cs);
  }
  comm->opCount++;  // whatever the outcome
  return r;
}

// Group aggregation (enqueue.cc:352-508 ncclPrepareTasks / :518-769
// scheduleCollTasksToPlan pack a group's collectives into one kernel plan,
// common.h:260-293 RunWorkBatch runs a plan's works in order): a run of
// consecutive calls of one comm that take the same algorithm — LL, direct or
// ring — with the same collective, kernel type and op becomes ONE launch
// carrying up to 16 works (LL all-reduces: lines within one slot).  A ZeRO
// loop's bucketed reduce-scatters launch once per group.  The decision
// depends only on the call sequence, never on streams, so every rank fuses
// identically.  The fused launch runs on the first task's stream; the other
// tasks' streams are joined before it and wait for it after.
// Same comm, collective, kernel type and op (the caller compares the paths).
static bool fusable(const Task& a, const Task& b) {
  if (a.comm != b.comm || a.coll != b.coll) return false;
  if (is_copy_coll(a.coll)) return true;  // byte copies: any type
  return a.datatype == b.datatype && a.devOp == b.devOp && a.arg == b.arg && a.argPtr == b.argPtr;
}
static int max_parts(int algo) {
  return algo == kAlgoLL ? kLLMaxParts : algo == kAlgoDirect ? kDirectMaxWorks : kRingMaxWorks;
}

// Runs of calls of one comm, each run one launch (1 .. max_parts calls), in
// order on the first task's stream; the other tasks' streams are joined
// before the first launch and wait for the last.
static ncclResult_t launch_runs(const std::vector<std::vector<Task>>& runs, const std::vector<int>& algos) {
  ncclComm* comm = runs[0][0].comm;
  const hipStream_t s0 = runs[0][0].stream;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  std::vector<hipStream_t> others;
  size_t nTasks = 0;
  for (const auto& run : runs) {
    nTasks += run.size();
    for (const Task& t : run)
      if (t.stream != s0 && std::find(others.begin(), others.end(), t.stream) == others.end())
        others.push_back(t.stream);
  }
  CaptureState cs{false, 0};
  ncclResult_t r = stream_order(comm, s0, &cs);
  for (hipStream_t s : others) {
    if (r != ncclSuccess) break;
    if (hipEventRecord(comm->joinEvent, s) != hipSuccess ||
        hipStreamWaitEvent(s0, comm->joinEvent, 0) != hipSuccess)
      r = ncclUnhandledCudaError;
  }
  bool bound = false;  // a launch of this sequence carries the ordering event
  for (size_t k = 0; k < runs.size() && r == ncclSuccess; k++) {
    // every launch goes onto s0 (the launchers use their first task's
    // stream): runs of one comm must never overlap on its channels
    std::vector<Task> run = runs[k];
    for (Task& t : run) t.stream = s0;
    const int n = (int)run.size();
    const hipEvent_t stop = stop_event(comm, cs);  // every launch: the last binding is the group's end
    r = launch_path(algos[k], run.data(), n, stop);
    bound |= r == ncclSuccess && stop != nullptr;
    if (n > 1) comm->fusedLaunches++;
  }
  if (r == ncclSuccess) {
    r = stream_mark(comm, s0, cs);
  } else if (bound) {
    // an earlier run already bound the ordering event to its
    // kernel on s0, so the next call from another stream must still wait on
    // it even though a later run of this sequence failed
    comm->lastStream = s0;
    comm->hasLastLaunch = true;
    comm->lastUnmarked = false;
  }
  const hipEvent_t done = stream_last_event(comm, cs);
  for (hipStream_t s : others)
    if (r == ncclSuccess && hipStreamWaitEvent(s, done, 0) != hipSuccess)
      r = ncclUnhandledCudaError;
  comm->opCount += nTasks;
  return r;
}

// A group's calls of one comm (`idx`, in call order, nRanks > 1) on VCCL's
// plan for them (group_plan): each (func, op, type) aggregate takes the path
// select_algo gives its summed count, as ncclPrepareTasks gives getAlgoInfo's
// choice to every member; every call is placed on the plan's channels under
// its path's protocol — the ring, LL128 ring and direct path fold every
// element in the order of that place, the LL reduce-scatter per channel of
// it, and LL calls shift the running channel cursor as in VCCL — and the
// calls launch in plan order, consecutive calls of one plan and path with the
// same collective, type and op fused (<= max_parts; LL calls while their lines
// fit one slot).
static ncclResult_t launch_planned(std::vector<Task>& tasks, const std::vector<int>& idx) {
  ncclComm* comm = tasks[idx[0]].comm;
  std::vector<GroupTask> g;
  for (int j : idx) {
    const Task& t = tasks[j];
    g.push_back(group_task_of(t.coll, t.count, t.datatype, t.devOp, kernel_type_of_call(t.coll, t.devOp, t.datatype)));
  }
  GroupPlanOut plan;
  const AlgoPolicy pol = policy_of(comm);
  group_plan(g, comm->nRanks, comm->nChannels,
             PlanGeometry{comm->stepBytes, comm->nThreads, comm->ll128StepBytes, comm->ll128Threads}, &pol, &plan);
  for (size_t k = 0; k < idx.size(); k++) {
    if (plan.planOf[k] < 0) return ncclInternalError;
    tasks[idx[k]].planned = true;
    tasks[idx[k]].plan = plan.cbd[k];
  }
  std::vector<std::vector<Task>> runs;
  std::vector<int> runAlgo, runPlan;
  std::vector<int64_t> runLines;
  static const bool fusePlanned = param_int("GROUP_PLAN_FUSE", 1) != 0;
  for (int k : plan.order) {
    Task t = tasks[idx[k]];
    // the comm's only collective of the group, eligible for the zero-copy
    // kernel: its partition is the call's alone, as outside a group
    const int a = reg_algo_or(t, plan.algo[k]);
    const bool zeroCopy = a == kAlgoDirectReg || a == kAlgoDirectRegRooted;
    if (zeroCopy) t.planned = false;
    const int64_t lines = a == kAlgoLL ? ll_lines_of(t) : 0;
    if (fusePlanned && !runs.empty() && runPlan.back() == plan.planOf[k] && runAlgo.back() == a &&
        runs.back().size() < (size_t)max_parts(a) && fusable(runs.back()[0], t) &&
        (a != kAlgoLL || runLines.back() + lines <= comm->llLines)) {
      runs.back().push_back(t);
      runLines.back() += lines;
      continue;
    }
    runs.push_back({t});
    runAlgo.push_back(a);
    runPlan.push_back(plan.planOf[k]);
    runLines.push_back(lines);
  }
  return launch_runs(runs, runAlgo);
}

// ------------------------------------------------------------ point-to-point
static_assert(kP2pSend == 0 && kP2pRecv == 1 && kP2pCopy == 2, "P2pItem::kind is the device's work kind");

ncclResult_t p2p_usable(const ncclComm* c, const char* api) {
  if (c->nRanks == 1 || c->p2pConns) return ncclSuccess;
  if (c->p2pOff == kP2pOffEnv)
    VWARN("%s : this communicator has no point-to-point buffers (VCCL_P2P_BUFFERS=0)", api);
  else if (c->p2pOff == kP2pOffRanks)
    VWARN("%s : point-to-point needs at most %d ranks, this communicator has %d", api, kP2pMaxRanks, c->nRanks);
  else
    VWARN("%s : point-to-point through the net proxy is not supported (a peer of this communicator is on "
          "another node)", api);
  return ncclInvalidUsage;
}

// p2p_plan's rule: the k-th send to self needs the k-th recv from self, of the same length.
static ncclResult_t check_self_pairs(const ncclComm* comm, const std::vector<Task>& ts) {
  const int me = comm->rank;
  std::vector<int64_t> selfSends, selfRecvs;
  for (const Task& t : ts) {
    if (t.coll == kTaskA2a) {
      selfSends.push_back(t.a2a->sendBytes[me]);
      selfRecvs.push_back(t.a2a->recvBytes[me]);
    } else if (t.root == me) {
      (t.coll == kTaskSend ? selfSends : selfRecvs).push_back((int64_t)t.count * type_size(t.datatype));
    }
  }
  if (selfSends == selfRecvs) return ncclSuccess;
  VWARN("ncclGroupEnd : a send to self needs its recv from self of the same length in the same group (rank %d); "
        "none of this communicator's sends and recvs were launched", me);
  return ncclInvalidUsage;
}

// The sends and recvs of one comm's group (call order), as 1 .. launches of
// the p2p kernel on the first task's stream, the other tasks' streams joined
// around them exactly as launch_runs does.
static ncclResult_t launch_p2p(const std::vector<Task>& ts) {
  ncclComm* comm = ts[0].comm;
  const hipStream_t s0 = ts[0].stream;
  const int n = comm->nRanks;
  const bool conns = comm->p2pConns != nullptr;
  const P2pGeometry geo{conns ? comm->p2pParts : 1, conns ? comm->p2pMinPartBytes : (int64_t)64 << 10,
                        conns ? comm->p2pStepBytes : 512 << 10};
  std::vector<P2pCall> calls;
  for (const Task& t : ts) {
    const bool send = t.coll == kTaskSend;
    calls.push_back(P2pCall{send ? kP2pCallSend : kP2pCallRecv, t.root, (int64_t)t.count * type_size(t.datatype),
                            (uint64_t)(uintptr_t)(send ? t.sendbuff : (const void*)t.recvbuff)});
  }
  comm->opCount += ts.size();  // whatever the outcome
  // The grid (invariant I4): every rank's send and receive workgroups are
  // resident at once — the CTA floor first, then the caps, as launch_ll and
  // direct_work_of apply them.
  int gCap = std::max(1, comm->maxCTAs / 2);
  if (comm->shareBlockCap > 0) gCap = std::max(1, std::min(gCap, comm->shareBlockCap / 2));
  P2pPlanOut plan;
  NCCLCHECK(check_self_pairs(comm, ts));  // the one refusal p2p_plan has
  NCCLCHECK(p2p_plan(comm->rank, n, calls, geo, (comm->minCTAs + 1) / 2, gCap, kP2pMaxWorks, &plan));
  if (plan.items.empty()) return ncclSuccess;  // zero-byte messages and in-place self pairs only
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  std::vector<hipStream_t> others;
  for (const Task& t : ts)
    if (t.stream != s0 && std::find(others.begin(), others.end(), t.stream) == others.end()) others.push_back(t.stream);
  CaptureState cs{false, 0};
  ncclResult_t r = stream_order(comm, s0, &cs);
  for (hipStream_t s : others) {
    if (r != ncclSuccess) break;
    if (hipEventRecord(comm->joinEvent, s) != hipSuccess || hipStreamWaitEvent(s0, comm->joinEvent, 0) != hipSuccess)
      r = ncclUnhandledCudaError;
  }
  // the verdicts of the zero-copy all-to-alls launched ahead of this (launch_comm_p2p)
  const bool anySkip = std::any_of(ts.begin(), ts.end(), [](const Task& t) { return t.skip > 0; });
  if (anySkip && (!comm->reg || !comm->reg->a2aDev)) return ncclInternalError;
  bool bound = false;
  for (size_t k = 0; k < plan.items.size() && r == ncclSuccess;) {
    P2pBatch b{};
    b.comm = comm->devComm;
    b.conns = comm->p2pConns;
    b.skip = anySkip ? comm->reg->a2aDev->skip : nullptr;
    b.nConns = conns ? n * geo.parts : 0;
    b.stepBytes = (int)geo.stepBytes;
    b.nSendWgs = plan.nWgs;
    const int launch = plan.items[k].launch;
    for (; k < plan.items.size() && plan.items[k].launch == launch; k++) {
      const P2pItem& it = plan.items[k];
      if (b.nWorks >= kP2pMaxWorks || (it.kind != kP2pCopy && (!conns || it.peer == comm->rank)))
        return ncclInternalError;
      P2pWork& w = b.works[b.nWorks++];
      w.kind = (int8_t)it.kind;
      w.wg = (int16_t)it.wg;
      w.conn = (int16_t)(it.peer * geo.parts + it.part);
      w.bytes = it.bytes;
      w.skip = (int8_t)ts[it.call].skip;  // a copy: its send's, which is its recv's
      if (it.kind != kP2pRecv) w.a = (const char*)ts[it.call].sendbuff + it.offset;
      if (it.kind != kP2pSend) w.b = (char*)ts[it.kind == kP2pCopy ? it.call2 : it.call].recvbuff + it.offset;
    }
    const hipEvent_t stop = stop_event(comm, cs);
    const hipError_t e = p2p_launch(b, 2 * plan.nWgs, s0, stop);
    if (e != hipSuccess) {
      VWARN("p2p kernel launch failed: %s", hipGetErrorString(e));
      r = ncclUnhandledCudaError;
    }
    bound |= r == ncclSuccess && stop != nullptr;
  }
  if (r == ncclSuccess) {
    r = stream_mark(comm, s0, cs);
  } else if (bound) {  // as launch_runs: an earlier launch already carries the ordering event
    comm->lastStream = s0;
    comm->hasLastLaunch = true;
    comm->lastUnmarked = false;
  }
  const hipEvent_t done = stream_last_event(comm, cs);
  for (hipStream_t s : others)
    if (r == ncclSuccess && hipStreamWaitEvent(s, done, 0) != hipSuccess) r = ncclUnhandledCudaError;
  return r;
}

// ---------------------------------------------------------------- all-to-all
// The rotated per-peer table of one all-to-all launch (coll_types.hpp A2aPeer):
// entry k is rank (me + k) mod n's, its direction bits set where `plan` gave
// the pair to `path`.
static void fill_a2a_peers(const Task& t, const A2aPlanOut& plan, int path, A2aPeer* table) {
  const int n = t.comm->nRanks, me = t.comm->rank;
  const A2aArgs& a = *t.a2a;
  for (int k = 0; k < n; k++) {
    const int p = (me + k) % n;
    A2aPeer& e = table[k];
    e.send = t.sendbuff ? (const char*)t.sendbuff + a.sendOff[p] : nullptr;
    e.recv = t.recvbuff ? (char*)t.recvbuff + a.recvOff[p] : nullptr;
    e.sendBytes = a.sendBytes[p];
    e.recvBytes = a.recvBytes[p];
    e.sendHere = plan.sendPath[p] == path;
    e.recvHere = plan.recvPath[p] == path;
  }
}

// The LL launch of one ncclAllToAll(v) (ll.hpp ll_alltoall) on the call's
// stream, ordered against the comm's other launches like a call outside a
// group (launch_task).  The tables go in rotated to this rank, the LL pairs'
// lines flattened in that order.  Plain ncclSend / ncclRecv never come here:
// they are not collective — a peer outside the exchange launches nothing, so
// the arrival barrier the slot reuse rests on (ll.hpp header) would not hold.
static ncclResult_t launch_ll_a2a(const Task& t, const A2aPlanOut& plan) {
  ncclComm* comm = t.comm;
  const int n = comm->nRanks, me = comm->rank;
  if (n > kLLA2aMaxRanks || !comm->llBuf || (int)comm->llPeer.size() < n) return ncclInternalError;
  LLA2aWork w{};
  w.comm = comm->devComm;
  w.rank = me;
  w.nRanks = n;
  w.linesPerSlot = comm->llLines;
  w.localBuf = comm->llBuf;
  fill_a2a_peers(t, plan, kA2aLL, w.peer);
  int64_t sl = 0, rl = 0;
  for (int k = 0; k < n; k++) {
    w.peerBuf[k] = comm->llPeer[(me + k) % n];
    const A2aPeer& e = w.peer[k];
    w.sendLine0[k] = sl;
    w.recvLine0[k] = rl;
    if (k == 0) continue;  // the self block is not part of the flattening
    const int64_t s = e.sendHere ? ll_lines_of(e.sendBytes) : 0, r = e.recvHere ? ll_lines_of(e.recvBytes) : 0;
    if (s > comm->llLines || r > comm->llLines) return ncclInternalError;
    sl += s;
    rl += r;
  }
  for (int k = n; k <= kLLA2aMaxRanks; k++) w.sendLine0[k] = sl, w.recvLine0[k] = rl;
  const int grid = ll_grid(comm, std::max(sl, rl));
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  CaptureState cs{false, 0};
  NCCLCHECK(stream_order(comm, t.stream, &cs));
  const hipError_t e = ll_a2a_launch(w, grid, t.stream, stop_event(comm, cs));
  if (e != hipSuccess) {
    VWARN("LL all-to-all kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return stream_mark(comm, t.stream, cs);
}

// The direct launch of one ncclAllToAll(v) (direct.hpp direct_alltoall) on the
// call's stream, ordered against the comm's other launches exactly like
// launch_ll_a2a.  The table goes in rotated to this rank; the grid is the
// plan's nBlocks, already under the co-residency caps the other direct kernels
// take (directMaxBlocks, which ranks sharing a GPU lower; kDirectMaxBlocks).
static ncclResult_t launch_direct_a2a(const Task& t, const A2aPlanOut& plan) {
  ncclComm* comm = t.comm;
  const int n = comm->nRanks, me = comm->rank;
  if (n > kDirectMaxRanks || !comm->dPeers || plan.nBlocks < 1 || plan.nBlocks > kDirectMaxBlocks ||
      plan.blkBytes < 16 || plan.blkBytes % 16)
    return ncclInternalError;
  // what the grid covers, and what a region holds (the last block may be short)
  const int64_t cover = std::min<int64_t>((int64_t)plan.nBlocks * plan.blkBytes, comm->dRegionBytes - 16);
  DirectA2aWork w{};
  w.comm = comm->devComm;
  w.peers = comm->dPeers;
  w.rank = me;
  w.nRanks = n;
  w.nBlocks = plan.nBlocks;
  w.blkBytes = plan.blkBytes;
  w.regionBytes = comm->dRegionBytes;
  fill_a2a_peers(t, plan, kA2aDirect, w.peer);
  for (int k = 0; k < n; k++) {
    const A2aPeer& e = w.peer[k];
    if ((e.sendHere && e.sendBytes > cover) || (e.recvHere && e.recvBytes > cover)) return ncclInternalError;
  }
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  CaptureState cs{false, 0};
  NCCLCHECK(stream_order(comm, t.stream, &cs));
  const hipError_t e = direct_a2a_launch(w, t.stream, stop_event(comm, cs));
  if (e != hipSuccess) {
    VWARN("direct all-to-all kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return stream_mark(comm, t.stream, cs);
}

// The zero-copy launch of one eligible ncclAllToAll(v) (direct_reg.hpp
// direct_reg_alltoall; plan.cc reg_a2a_plan is its step list) on the call's
// stream, ordered like launch_direct_a2a, the import table brought up to date
// first as launch_direct_reg does.  The grid is comm-wide (reg_a2a_blocks); the
// slices are the reader's own (reg_a2a_blk per receive block).  The descriptors
// are this rank's registrations of each block it sends, as of now.  selfPaired:
// the call's self send and self recv are each other's match in the group's
// sweep order — rank-local, so it enters the vote, not the eligibility.
static ncclResult_t launch_reg_a2a(const Task& t, int skipIdx, bool selfPaired) {
  ncclComm* comm = t.comm;
  const int n = comm->nRanks, me = comm->rank;
  const A2aArgs& a = *t.a2a;
  if (n > kDirectMaxRanks || !comm->dPeers || !comm->reg || !comm->reg->a2aDev || skipIdx < 0 ||
      skipIdx >= kRegA2aMaxCalls)
    return ncclInternalError;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  CaptureState cs{false, 0};
  NCCLCHECK(stream_order(comm, t.stream, &cs));
  NCCLCHECK(reg_refresh(comm, cs.active));
  DirectRegA2aWork w{};
  w.comm = comm->devComm;
  w.peers = comm->dPeers;
  w.reg = comm->reg->tabDev;
  w.dev = comm->reg->a2aDev;
  w.rank = me;
  w.nRanks = n;
  w.skipIdx = skipIdx;
  w.nBlocks = reg_a2a_blocks(a.uniform, a.sendBytes[0], comm->minCTAs, comm->maxCTAs, comm->directMaxBlocks);
  if (w.nBlocks < 1 || w.nBlocks > kDirectMaxBlocks) return ncclInternalError;
  bool ok = selfPaired && a.sendBytes[me] == a.recvBytes[me];
  for (int k = 0; k < n; k++) {
    const int p = (me + k) % n;
    RegA2aPeer& e = w.peer[k];
    e.send = t.sendbuff ? (const char*)t.sendbuff + a.sendOff[p] : nullptr;
    e.recv = t.recvbuff ? (char*)t.recvbuff + a.recvOff[p] : nullptr;
    e.sendBytes = a.sendBytes[p];
    e.recvBytes = a.recvBytes[p];
    e.blkBytes = reg_a2a_blk(e.recvBytes, comm->minCTAs, comm->maxCTAs, comm->directMaxBlocks);
    if ((e.recvBytes + e.blkBytes - 1) / e.blkBytes > w.nBlocks) return ncclInternalError;
    e.entry = kRegNone;
    if (k > 0 && e.sendBytes > 0) {  // my block for p as p will address it
      reg_describe(comm, e.send, (uint64_t)e.sendBytes, &e.entry, &e.gen, &e.regOff);
      ok = ok && e.entry != kRegNone;
    }
  }
  w.selfOk = ok && reg_a2a_size_vote(n, me, a.sendBytes, a.recvBytes, a.uniform, comm->regA2aMaxBytes);
  const hipError_t e = direct_reg_a2a_launch(w, t.stream, stop_event(comm, cs));
  if (e != hipSuccess) {
    VWARN("zero-copy all-to-all kernel launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return stream_mark(comm, t.stream, cs);
}

// One comm's sends, recvs and all-to-all tasks of a group (call order): each
// all-to-all's LL launch, then its direct launch, in call order, then the one
// p2p launch with the plain sends and recvs and the all-to-alls' residual
// pairs, in call order per peer — so matching by sweep is what it was.  An
// all-to-all eligible for the zero-copy path (reg_a2a_eligible) launches that
// kernel instead of the LL and direct ones, and ALL its pairs, the self copy
// included, join the p2p launch predicated on its verdict: the host cannot
// know whether the kernel moved them.
static ncclResult_t launch_comm_p2p(const std::vector<Task>& mine) {
  if (std::none_of(mine.begin(), mine.end(), [](const Task& t) { return t.coll == kTaskA2a; }))
    return launch_p2p(mine);
  ncclComm* comm = mine[0].comm;
  const int n = comm->nRanks, me = comm->rank;
  // launch_p2p's refusal, before any LL or direct launch: a refused group launches nothing
  if (check_self_pairs(comm, mine) != ncclSuccess) {
    comm->opCount += mine.size();
    return ncclInvalidUsage;
  }
  std::vector<Task> fifo;
  int nReg = 0;                        // eligible all-to-alls so far: collective, so the same on every rank
  size_t selfSends = 0, selfRecvs = 0;  // to self, so far (the sweep a self pair is matched in)
  for (const Task& t : mine) {
    if (t.coll != kTaskA2a) {
      if (t.root == me) (t.coll == kTaskSend ? selfSends : selfRecvs)++;
      fifo.push_back(t);
      continue;
    }
    const A2aArgs& a = *t.a2a;
    const bool selfPaired = selfSends++ == selfRecvs++;
    auto expand = [&](int p, bool send, int skip) {  // the API's own expansion of pair p
      return send ? Task{.coll = kTaskSend, .sendbuff = t.sendbuff ? (const char*)t.sendbuff + a.sendOff[p] : nullptr,
                         .recvbuff = nullptr, .count = (size_t)a.sendBytes[p], .datatype = ncclUint8,
                         .devOp = t.devOp, .root = p, .comm = comm, .stream = t.stream, .skip = skip}
                  : Task{.coll = kTaskRecv, .sendbuff = nullptr,
                         .recvbuff = t.recvbuff ? (char*)t.recvbuff + a.recvOff[p] : nullptr,
                         .count = (size_t)a.recvBytes[p], .datatype = ncclUint8, .devOp = t.devOp, .root = p,
                         .comm = comm, .stream = t.stream, .skip = skip};
    };
    if (comm->reg && reg_a2a_eligible(a.uniform, a.sendBytes[0], comm->regA2aMaxBytes, nReg)) {
      // opCount: launch_p2p counts the 2 n expanded calls, as the FIFO expansion does
      NCCLCHECK(launch_reg_a2a(t, nReg, selfPaired));
      nReg++;
      for (int p = 0; p < n; p++) {
        fifo.push_back(expand(p, true, nReg));
        fifo.push_back(expand(p, false, nReg));
      }
      continue;
    }
    A2aPlanOut plan;
    if (a2a_plan(n, me, a.sendBytes, a.recvBytes, a.uniform, comm->llA2aMaxBytes, comm->directA2aMaxBytes,
                 comm->llLines, comm->minCTAs, comm->maxCTAs, comm->directMaxBlocks, &plan) != ncclSuccess)
      return ncclInternalError;
    const size_t nFifo = plan.resSends.size() + plan.resRecvs.size();
    const size_t nDirect = (size_t)std::count(plan.sendPath.begin(), plan.sendPath.end(), (char)kA2aDirect) +
                           (size_t)std::count(plan.recvPath.begin(), plan.recvPath.end(), (char)kA2aDirect);
    comm->a2aLLPairs += 2 * (size_t)n - nFifo - nDirect;
    comm->a2aDirectPairs += nDirect;
    comm->a2aFifoPairs += nFifo;
    comm->opCount += 2 * (size_t)n - nFifo;  // as the FIFO path counts them; whatever the outcome
    if (plan.llLaunch) {
      comm->a2aLLLaunches++;
      NCCLCHECK(launch_ll_a2a(t, plan));
    }
    if (plan.directLaunch) {
      comm->a2aDirectLaunches++;
      NCCLCHECK(launch_direct_a2a(t, plan));
    }
    for (int p = 0; p < n; p++) {  // the API's own expansion order: send p, recv p
      if (plan.sendPath[p] == kA2aFifo) fifo.push_back(expand(p, true, 0));
      if (plan.recvPath[p] == kA2aFifo) fifo.push_back(expand(p, false, 0));
    }
  }
  return fifo.empty() ? ncclSuccess : launch_p2p(fifo);
}

static ncclResult_t launch_group_colls(std::vector<Task>& tasks) {
  ncclResult_t ret = ncclSuccess;
  const size_t n = tasks.size();
  for (Task& t : tasks)
    t.groupColls = (int)std::count_if(tasks.begin(), tasks.end(), [&](const Task& o) { return o.comm == t.comm; });
  std::vector<char> done(n, 0);
  const bool fuse = param_int("GROUP_FUSE", 1) != 0;
  // VCCL_GROUP_PLAN=0: every call keeps its own path and the partition of a
  // call planned alone (runs of consecutive fusable calls still fuse)
  const bool plan = fuse && param_int("GROUP_PLAN", 1) != 0;
  std::vector<int> algo(n, -1);
  if (fuse && !plan)
    for (size_t i = 0; i < n; i++) algo[i] = tasks[i].comm->nRanks > 1 ? choose_algo(tasks[i]) : -1;
  for (size_t i = 0; i < n; i++) {
    if (done[i]) continue;
    ncclResult_t r;
    if (plan && tasks[i].comm->nRanks > 1) {
      // every call of this comm in the group, one VCCL plan
      std::vector<int> idx;
      for (size_t j = i; j < n; j++)
        if (!done[j] && tasks[j].comm == tasks[i].comm) idx.push_back((int)j);
      for (int j : idx) done[j] = 1;
      r = launch_planned(tasks, idx);
    } else if (algo[i] >= 0) {
      std::vector<Task> batch{tasks[i]};
      int64_t lines = ll_lines_of(tasks[i]);
      for (size_t j = i + 1; j < n && batch.size() < (size_t)max_parts(algo[i]); j++) {
        if (done[j] || tasks[j].comm != tasks[i].comm) continue;
        if (algo[j] != algo[i] || !fusable(tasks[i], tasks[j])) break;
        if (algo[i] == kAlgoLL) {
          if (lines + ll_lines_of(tasks[j]) > tasks[i].comm->llLines) break;
          lines += ll_lines_of(tasks[j]);
        }
        batch.push_back(tasks[j]);
        done[j] = 1;
      }
      r = batch.size() == 1 ? launch_task(tasks[i]) : launch_runs({batch}, {algo[i]});
    } else {
      r = launch_task(tasks[i]);
    }
    if (ret == ncclSuccess) ret = r;
  }
  return ret;
}

ncclResult_t launch_group(std::vector<Task>& tasks) {
  std::vector<Task> colls, p2p;
  for (const Task& t : tasks) (is_p2p(t.coll) || t.coll == kTaskA2a ? p2p : colls).push_back(t);
  ncclResult_t ret = colls.empty() ? ncclSuccess : launch_group_colls(colls);
  // per comm (first appearance): its sends, recvs and all-to-alls behind its collectives
  std::vector<char> done(p2p.size(), 0);
  for (size_t i = 0; i < p2p.size(); i++) {
    if (done[i]) continue;
    std::vector<Task> mine;
    for (size_t j = i; j < p2p.size(); j++)
      if (!done[j] && p2p[j].comm == p2p[i].comm) {
        mine.push_back(p2p[j]);
        done[j] = 1;
      }
    const ncclResult_t r = launch_comm_p2p(mine);
    if (ret == ncclSuccess) ret = r;
  }
  return ret;
}

}  // namespace vccl
