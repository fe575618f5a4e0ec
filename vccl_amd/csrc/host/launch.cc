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
#include "../device/ring_launch.hpp"
#include "order.h"
#include "regcomm.h"

namespace vccl {

// The host uses one set of collective codes: Coll (plan.h) is what the
// launchers of ring_launch.hpp / launch.hpp take as kColl*.
static_assert((int)kAllReduce == (int)kCollAllReduce && (int)kReduceScatter == (int)kCollReduceScatter &&
                  (int)kAllGather == (int)kCollAllGather && (int)kBroadcast == (int)kCollBroadcast &&
                  (int)kReduce == (int)kCollReduce, "Coll and kColl* are one enumeration");
// ... and one set of device op codes: plan.cc encodes ops as vcclDevRedOp_t.
static_assert((int)OP_SUM == (int)vcclDevSum && (int)OP_PROD == (int)vcclDevProd &&
                  (int)OP_MINMAX == (int)vcclDevMinMax && (int)OP_PREMULSUM == (int)vcclDevPreMulSum &&
                  (int)OP_SUMPOSTDIV == (int)vcclDevSumPostDiv,
              "OP_* and vcclDevRedOp_t are one enumeration");
static_assert((int)OP_SUM_MXFP8 == kSumMxOp && (int)OP_COPY_MXFP8 == kCopyMxOp && (int)OP_COPY == kCopyOp,
              "plan.h names the MXFP8 op codes without the kernel headers");
static_assert((int)OP_SUM_WIDE == kSumWideOp && (int)OP_PREMULSUM_WIDE == kPreMulSumWideOp,
              "the wide op codes of plan.h are dispatch.hpp's");

ncclResult_t launch_result(hipError_t e, const char* family) {
  if (e == hipSuccess) return ncclSuccess;
  VWARN("%s kernel launch failed: %s", family, hipGetErrorString(e));
  return ncclUnhandledCudaError;
}

// ncclLaunchOneRank (onerank.cu:47-83): a copy, or the PreMulSum kernel.  An
// in-place call without a preOp enqueues nothing.
// ncclAllReduceWithBias: recv = op(first, acc), one launch of the engine's two-source reduce-copy with the call's
// native functor on its stream.  One rank: first = sendbuff, the whole call.  More ranks, on a path without a bias
// kernel (the rings, the zero-copy kernels): first = recvbuff, right behind the launch that carried the plain
// collective — for a native functor op(F, acc) rounds as the fused fold's last step does.
static ncclResult_t launch_bias_rc(const Task& t, const void* first) {
  RCArgs a = {};
  a.srcs[0] = (const char*)first;
  a.srcs[1] = (const char*)t.acc;
  a.dsts[0] = (char*)t.recvbuff;
  a.nSrcs = 2;
  a.nDsts = 1;
  const hipError_t e = reduce_copy_launch(native_op_of(t.devOp), (int)t.datatype, t.arg, a, (int64_t)t.count, nullptr,
                                          t.stream);
  if (e != hipSuccess) {
    VWARN("bias reduce-copy launch failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

static ncclResult_t launch_one_rank(const Task& t) {
  if (t.acc) return launch_bias_rc(t, t.sendbuff);
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
                    .directRootedMax = c->directRootedMaxBytes,
                    .sumFp32RingMin = sum_fp32_ring_of(*c, sum_fp32_level(c))};
}

int kernel_type_of_call(int coll, int devOp, ncclDataType_t datatype) {
  return is_copy_coll(coll) ? (int)K_U8 : kernel_type_of(native_op_of(devOp), (int)datatype);
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
  w.preOp = native_op_of(t.devOp) == OP_PREMULSUM;
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
  // a wide op code: the wide ring's kernels, SIMPLE with the workgroup hand-off whatever the comm's wave setting
  if (is_wide_op(devOp) && (ll128 || (t.coll != kAllReduce && t.coll != kReduceScatter))) return ncclInternalError;
  const int v = is_wide_op(devOp) ? kRingVariantWide
                : ll128 ? kRingVariantLL128
                : comm->ringWave && ring_wave_kernel(kt, devOp, t.coll) ? kRingVariantWave : kRingVariantSimple;
  NCCLCHECK(launch_result(by_kernel_type(kt, [&]<int K>() {
    return ring_launch_any<K>(v, t.coll, devOp, b, comm->nThreads, t.stream, stop);
  }), "ring"));
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
static int64_t ll_lines_of(const Task& t) { return ll_lines_of((int64_t)t.count * type_size(t.datatype)); }
// A bounded grid (256-thread workgroups, each thread looping over lines):
// one workgroup per 256 lines, within the comm's CTA bounds (minCTAs /
// maxCTAs, default 1 / 128), and never above VCCL_LL_MAX_BLOCKS (256): every
// rank's LL workgroups must be resident at once for the peers' spins to
// complete, so that co-residency cap is applied LAST (tests that
// put 8 ranks on ONE GPU lower it).
int ll_grid(const ncclComm* comm, int64_t lines) {
  int maxBlocks = (int)std::max<int64_t>(1, param_int("LL_MAX_BLOCKS", 256));
  if (comm->shareBlockCap > 0) maxBlocks = std::min(maxBlocks, comm->shareBlockCap);
  int grid = (int)std::max<int64_t>(1, (lines + 255) / 256);
  grid = std::max(std::min(grid, comm->maxCTAs), comm->minCTAs);
  return std::max(1, std::min(grid, maxBlocks));
}
static ncclResult_t launch_ll(const Task* ts, int nTasks, hipEvent_t stop) {
  const Task& t = ts[0];
  ncclComm* comm = t.comm;
  LLBiasWork bw{};  // bw.acc: a bias launch's per-part pointers (ncclAllReduceWithBias)
  LLWork& w = bw.w;
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
    bw.acc[i] = (const char*)ts[i].acc;
    if ((ts[i].acc != nullptr) != (t.acc != nullptr)) return ncclInternalError;  // bias calls fuse among themselves
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
  const int kt = kernel_type_of_call(t.coll, t.devOp, t.datatype);  // a wide op: its type's unit
  if (kt < 0) return ncclInvalidArgument;
  if (is_wide_op(t.devOp) && rooted) return ncclInternalError;  // the wide reduce never takes the rooted LL
  const int grid = ll_grid(comm, lines);
  const int devOp = copy ? OP_COPY : t.devOp;
  if (t.acc && t.coll != kAllReduce) return ncclInternalError;
  return launch_result(by_kernel_type(kt, [&]<int K>() {
    return t.acc ? ll_launch_bias<K>(devOp, bw, grid, t.stream, stop) : ll_launch<K>(t.coll, devOp, w, grid, t.stream, stop);
  }), "LL");
}

// The launch geometry of one direct call, from the one planner that applies (plan.h); blkForce as there.
static ncclResult_t direct_geometry_of(const Task& t, int64_t blkForce, DirectPlanOut* g) {
  const ncclComm* c = t.comm;
  ncclResult_t r;
  if (is_mx_op(t.devOp)) {
    // whole wire tiles: the all-reduce's n shards, or one rank's block of the reduce-scatter (OP_SUM_MXFP8) / the
    // all-gather (OP_COPY_MXFP8), the count in elements for the all-gather too (its kernel is typed)
    const bool rsag = t.coll == kReduceScatter || t.coll == kAllGather;
    if ((t.coll != kAllReduce && !rsag) || (t.datatype != ncclFloat16 && t.datatype != ncclBfloat16) ||
        (t.devOp == OP_COPY_MXFP8) != (t.coll == kAllGather))
      return ncclInternalError;
    r = direct_mx_plan(rsag ? 1 : c->nRanks, (int64_t)t.count, c->dRegionBytes, c->minCTAs, c->maxCTAs,
                       c->directMaxBlocks, blkForce, g);
  } else {
    const auto [count, esz] = call_size(t.coll, t.count, t.datatype);  // all-gather / broadcast: bytes
    r = direct_plan(t.coll, c->nRanks, count, esz, c->dRegionBytes, c->minCTAs, c->maxCTAs, c->directMaxBlocks,
                    blkForce, g);
  }
  return r == ncclSuccess ? ncclSuccess : ncclInternalError;
}

// The direct work of one call (direct.hpp): the comm and op fields, the planner's geometry, the fold order.
static ncclResult_t direct_work_of(const Task& t, int64_t blkForce, DirectWork* out, int* ktOut, int* devOpOut) {
  ncclComm* comm = t.comm;
  const bool mx = is_mx_op(t.devOp), rooted = t.coll == kBroadcast || t.coll == kReduce;
  if (rooted && (comm->nRanks < 2 || t.root < 0 || t.root >= comm->nRanks)) return ncclInternalError;
  DirectPlanOut g;
  NCCLCHECK(direct_geometry_of(t, blkForce, &g));
  const int kt = mx ? (t.datatype == ncclFloat16 ? (int)K_F16 : (int)K_BF16)
                    : kernel_type_of_call(t.coll, t.devOp, t.datatype);  // a wide op: its type's unit
  if (kt < 0) return ncclInvalidArgument;
  const int64_t count = mx ? (int64_t)t.count : call_size(t.coll, t.count, t.datatype).count;
  DirectWork w{};
  fill_op_fields(w, t);
  w.peers = comm->dPeers;
  w.sendbuff = t.sendbuff;
  w.recvbuff = t.recvbuff;
  w.count = (uint64_t)count;
  w.rank = comm->rank;
  w.root = rooted ? t.root : 0;
  w.chunkElts = g.chunkElts;
  w.nChunks = g.nChunks;
  w.blkElts = g.blkElts;
  w.nBlocks = g.nBlocks;
  w.regionBytes = comm->dRegionBytes;
  if (mx) {  // folds in rank order: no partition
  } else if (t.coll == kAllReduce) {
    // the ring's partition of this bucket: phase 2 folds every element in the
    // order VCCL's ring all-reduce gives it on these channels (ar_chunk_of)
    const CbdPlan p = task_plan(t, kProtoSimple);
    w.cbd = CbdLite{p.channelLo, p.channelHi, p.countLo, p.countMid, count};
    w.arChunk = p.chunkLo;
  } else if (t.coll == kReduceScatter || t.coll == kReduce) {
    // the call's own partition under SIMPLE, as the ring folds it
    w.cbd = rs_cbd(t, kProtoSimple);
  }
  *out = w;
  *ktOut = kt;
  *devOpOut = !mx && is_copy_coll(t.coll) ? (int)OP_COPY : t.devOp;
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
  DirectBiasBatch bb{};  // bb.acc: a bias launch's per-part pointers (ncclAllReduceWithBias)
  DirectBatch& b = bb.b;
  int kt = -1, devOp = -1;
  int64_t blk = 0;  // a batch's common block length: the largest part's natural one (0: one call, its own)
  for (int i = 0; i < nTasks && nTasks > 1; i++) {
    DirectPlanOut g;
    NCCLCHECK(direct_geometry_of(ts[i], 0, &g));
    blk = std::max(blk, g.blkElts);
  }
  for (int i = 0; i < nTasks; i++) {
    DirectWork wi;
    int kti, opi;
    NCCLCHECK(direct_work_of(ts[i], blk, &wi, &kti, &opi));
    if (i > 0 && (kti != kt || opi != devOp || (ts[i].acc != nullptr) != (t.acc != nullptr))) return ncclInternalError;
    kt = kti;
    devOp = opi;
    bb.acc[i] = (const char*)ts[i].acc;
    if (i == 0) {
      b.w = wi;
    } else {
      b.more[i - 1] = direct_part_of(wi);
      b.w.nBlocks = std::max(b.w.nBlocks, wi.nBlocks);
    }
  }
  b.nParts = nTasks;
  if (t.acc && t.coll != kAllReduce) return ncclInternalError;
  hipError_t e;
  if (is_mx_op(devOp)) {  // the MXFP8 kernels, one per collective, over the two 16-bit float types
    if (t.acc) return ncclInternalError;
    if (t.coll == kReduceScatter) {
      e = kt == K_F16 ? direct_launch_mx_rs<K_F16>(b, t.stream, stop) : direct_launch_mx_rs<K_BF16>(b, t.stream, stop);
      if (e == hipSuccess) t.comm->rsMxfp8Launches += (uint64_t)nTasks;
    } else if (t.coll == kAllGather) {
      e = kt == K_F16 ? direct_launch_mx_ag<K_F16>(b, t.stream, stop) : direct_launch_mx_ag<K_BF16>(b, t.stream, stop);
      if (e == hipSuccess) t.comm->agMxfp8Launches += (uint64_t)nTasks;
    } else {
      e = kt == K_F16 ? direct_launch_mx<K_F16>(b, t.stream, stop) : direct_launch_mx<K_BF16>(b, t.stream, stop);
      if (e == hipSuccess) t.comm->arMxfp8Launches += (uint64_t)nTasks;
    }
  } else {
    e = by_kernel_type(kt, [&]<int K>() {
      return t.acc ? direct_launch_bias<K>(devOp, bb, t.stream, stop)
                   : direct_launch<K>(t.coll, devOp, b, t.stream, stop);
    });
  }
  return launch_result(e, "direct");
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
// What the two zero-copy launches share.  The staged geometry is the staged
// path's own (direct_work_of: the fallback runs it as it is); the import table is brought
// up to date first (nothing in the steady state, nothing inside a capture).
static ncclResult_t reg_work_of(const Task& t, DirectRegWork* rw, int* kt, int* devOp) {
  ncclComm* comm = t.comm;
  CaptureState cs{false, 0};
  NCCLCHECK(capture_state(t.stream, &cs));
  NCCLCHECK(reg_refresh(comm, cs.active));
  NCCLCHECK(direct_work_of(t, 0, &rw->w, kt, devOp));
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
  return launch_result(
      by_kernel_type(kt, [&]<int K>() { return direct_reg_launch<K>(t.coll, devOp, rw, t.stream, stop); }),
      "zero-copy direct");
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
  return launch_result(
      by_kernel_type(kt, [&]<int K>() { return direct_reg_launch_rooted<K>(t.coll, devOp, rw, t.stream, stop); }),
      "zero-copy rooted");
}

// The paths of a launch: select_algo's, and the zero-copy kernels over registered buffers that pre-empt it.
enum { kAlgoDirectReg = kAlgoRingLL128 + 1, kAlgoDirectRegRooted };  // ... the all-reduce / RS / AG's, a broadcast / reduce's
struct PathTraits {
  int maxParts;    // the fusable calls one launch carries (1: single-call only)
  bool fusesBias;  // the kernels fold a bias themselves; else each bias call gets its reduce-copy (launch_path)
};
static PathTraits path_traits(int algo) {
  switch (algo) {
    case kAlgoLL: return {kLLMaxParts, true};
    case kAlgoDirect: return {kDirectMaxWorks, true};
    case kAlgoDirectReg:
    case kAlgoDirectRegRooted: return {1, false};
    default: return {kRingMaxWorks, false};
  }
}
// A call's path.  planAlgo: the answer of its group's plan for its aggregate; < 0: the call alone.
static int path_of(const Task& t, int planAlgo) {
  const bool wide = is_wide_op(t.devOp), mx = is_mx_op(t.devOp);
  // Zero-copy first, for a call eligible for it.  An MXFP8 call never negotiates; nor does a wide sum at level 1,
  // which keeps to the staged path, or with a bias at any level, which must enter the staged kernel's binary32 fold.
  if (!mx && !(wide && (sum_fp32_level(t.comm) < 2 || t.acc))) {
    if (reg_task_eligible(t)) return kAlgoDirectReg;
    if (reg_rooted_task_eligible(t)) return kAlgoDirectRegRooted;
  }
  if (planAlgo >= 0) return planAlgo;
  if (mx) return kAlgoDirect;  // the staged direct launch at every size
  if (wide) {
    // staged direct; at level 2 LL where select_algo answers LL; the wide ring from the comm's threshold up
    const int a =
        sum_fp32_algo(sum_fp32_level(t.comm), policy_of(t.comm), t.coll, type_size(t.datatype), (int64_t)t.count);
    // a bias call never takes the wide ring: a bias added behind it would not enter the binary32 fold
    return t.acc && a == kAlgoRing ? (int)kAlgoDirect : a;
  }
  return select_algo(policy_of(t.comm), t.coll, type_size(t.datatype), (int64_t)t.count);
}

// 1 .. maxParts fusable calls as one launch of path `algo`.
static ncclResult_t launch_path_only(int algo, const Task* ts, int n, hipEvent_t stop) {
  if (n < 1 || n > path_traits(algo).maxParts) return ncclInternalError;
  switch (algo) {
    case kAlgoDirectReg: return launch_direct_reg(ts[0], stop);
    case kAlgoDirectRegRooted: return launch_direct_reg_rooted(ts[0], stop);
    case kAlgoLL: return launch_ll(ts, n, stop);
    case kAlgoDirect: return launch_direct(ts, n, stop);
    default: return launch_ring(ts, n, algo == kAlgoRingLL128, stop);
  }
}
// ... with the bias tail of a path that fuses none: the ordering event is recorded behind the reduce-copies
// instead of bound to the collective.
static ncclResult_t launch_path(int algo, const Task* ts, int n, hipEvent_t stop) {
  if (path_traits(algo).fusesBias || std::none_of(ts, ts + n, [](const Task& t) { return t.acc != nullptr; }))
    return launch_path_only(algo, ts, n, stop);
  if (std::any_of(ts, ts + n, [](const Task& t) { return is_wide_op(t.devOp); })) return ncclInternalError;
  NCCLCHECK(launch_path_only(algo, ts, n, nullptr));
  for (int i = 0; i < n; i++)
    if (ts[i].acc) NCCLCHECK(launch_bias_rc(ts[i], ts[i].recvbuff));  // on ts[i].stream = the run's stream
  return record_stop(stop, ts[0].stream);
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
    OrderScope order(comm, t.stream);
    r = order.begin();
    if (r == ncclSuccess) r = order.ran(launch_path(path_of(t, -1), &t, 1, order.stop()));
    r = order.end(r);
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
  if (a.comm != b.comm || a.coll != b.coll || (a.acc != nullptr) != (b.acc != nullptr)) return false;
  if (is_copy_coll(a.coll) && !is_mx_op(a.devOp) && !is_mx_op(b.devOp)) return true;  // byte copies: any type
  return a.datatype == b.datatype && a.devOp == b.devOp && a.arg == b.arg && a.argPtr == b.argPtr;
}
// Whether `t` joins `run` (calls of path `algo`, `lines` LL lines so far): room, fusable, LL lines within one slot.
static bool can_join(const std::vector<Task>& run, int64_t lines, const Task& t, int algo) {
  return run.size() < (size_t)path_traits(algo).maxParts && fusable(run[0], t) &&
         (algo != kAlgoLL || lines + ll_lines_of(t) <= t.comm->llLines);
}

// Runs of calls of one comm, each run one launch (1 .. maxParts calls), in
// order on the first task's stream; the other tasks' streams are joined
// before the first launch and wait for the last.
static ncclResult_t launch_runs(const std::vector<std::vector<Task>>& runs, const std::vector<int>& algos) {
  ncclComm* comm = runs[0][0].comm;
  const hipStream_t s0 = runs[0][0].stream;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  OrderScope order(comm, s0);
  size_t nTasks = 0;
  for (const auto& run : runs) {
    nTasks += run.size();
    for (const Task& t : run) order.join(t.stream);
  }
  ncclResult_t r = order.begin();
  for (size_t k = 0; k < runs.size() && r == ncclSuccess; k++) {
    // every launch goes onto s0 (the launchers use their first task's
    // stream): runs of one comm must never overlap on its channels
    std::vector<Task> run = runs[k];
    for (Task& t : run) t.stream = s0;
    const int n = (int)run.size();
    r = order.ran(launch_path(algos[k], run.data(), n, order.stop()));  // the last binding is the group's end
    if (n > 1) comm->fusedLaunches++;
  }
  r = order.end(r);
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
// same collective, type and op fused (can_join).
static ncclResult_t launch_planned(std::vector<Task>& tasks, const std::vector<int>& idx) {
  ncclComm* comm = tasks[idx[0]].comm;
  std::vector<GroupTask> g;
  for (int j : idx) {
    const Task& t = tasks[j];
    g.push_back(group_task_of(t.coll, t.count, t.datatype, t.devOp, kernel_type_of_call(t.coll, t.devOp, t.datatype),
                              t.acc != nullptr));
  }
  GroupPlanOut plan;
  const AlgoPolicy pol = policy_of(comm);
  sum_fp32_group_rule(g, sum_fp32_level(comm), pol);
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
    const int a = path_of(t, plan.algo[k]);
    if (a == kAlgoDirectReg || a == kAlgoDirectRegRooted) t.planned = false;
    if (fusePlanned && !runs.empty() && runPlan.back() == plan.planOf[k] && runAlgo.back() == a &&
        can_join(runs.back(), runLines.back(), t, a)) {
      runs.back().push_back(t);
    } else {
      runs.push_back({t});
      runAlgo.push_back(a);
      runPlan.push_back(plan.planOf[k]);
      runLines.push_back(0);
    }
    runLines.back() += ll_lines_of(t);
  }
  return launch_runs(runs, runAlgo);
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
    for (size_t i = 0; i < n; i++) algo[i] = tasks[i].comm->nRanks > 1 ? path_of(tasks[i], -1) : -1;
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
      for (size_t j = i + 1; j < n; j++) {
        if (done[j] || tasks[j].comm != tasks[i].comm) continue;
        if (algo[j] != algo[i] || !can_join(batch, lines, tasks[j], algo[i])) break;
        lines += ll_lines_of(tasks[j]);
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
