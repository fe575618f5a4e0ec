// VCCL's planner restated for one node (plan.h): the op encoding, the cbd
// channel partition, the path selection and the multi-task group plan.
#include "plan.h"

#include <algorithm>
#include <cstring>

#include "../../../include/vccl_device.h"
#include "../device/coll_types.hpp"

namespace vccl {

// The device op codes (vcclDevRedOp_t = ncclDevRedOp_t, device.h:34-38; the
// kernels' OP_* of dispatch.hpp are the same values, tied in launch.cc).
enum : int { OP_SUM = vcclDevSum, OP_PROD = vcclDevProd, OP_MINMAX = vcclDevMinMax, OP_PREMULSUM = vcclDevPreMulSum,
             OP_SUMPOSTDIV = vcclDevSumPostDiv };

int type_size(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: case ncclFloat8e4m3: case ncclFloat8e5m2: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return -1;
  }
}

// __nv_cvt_float_to_fp8(f, __NV_SATFINITE, fmt) for the avg scalar
// (enqueue.cc:2265-2272): RN-even to `mbits` mantissa bits with exponent bias
// `bias`, magnitudes past max finite saturate, NaN -> 0x7f.
static uint8_t f32_to_fp8_satfinite(float f, int mbits, int bias, uint32_t maxCode) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t s = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return 0x7fu;
  const int e = (int)(a >> 23) - 127, emin = 1 - bias;
  if (a == 0) return (uint8_t)s;
  const uint64_t m = (a & 0x7fffffu) | 0x800000u;
  const int shift = (e >= emin ? e : emin) - mbits - e + 23;  // >= 23 - mbits
  uint64_t q = 0;
  if (shift < 40) {
    q = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) q++;
  }
  uint64_t code = e >= emin ? ((uint64_t)(e + bias) << mbits) + (q - (1ull << mbits)) : q;
  if (e > 15 + bias || code > maxCode) code = maxCode;
  return (uint8_t)(s | code);
}

// hostToDevRedOp (enqueue.cc:2217-2310) for built-in ops.
ncclResult_t host_to_dev_redop(ncclRedOp_t op, ncclDataType_t dt, int nRanks, int* devOp, uint64_t* arg) {
  const int nbits = 8 * type_size(dt);
  if (nbits <= 0) return ncclInvalidArgument;
  const uint64_t allBits = ~0ull >> (64 - nbits);
  const uint64_t signBit = allBits ^ (allBits >> 1);
  const bool isSigned = dt == ncclInt8 || dt == ncclInt32 || dt == ncclInt64;
  *arg = 0;
  switch ((int)op) {
    case ncclSum: *devOp = OP_SUM; return ncclSuccess;
    case ncclProd: *devOp = OP_PROD; return ncclSuccess;
    case ncclMin:
    case ncclMax:
      *devOp = OP_MINMAX;
      if (isSigned) *arg ^= signBit;
      if (op == ncclMax) *arg ^= allBits;
      return ncclSuccess;
    case ncclAvg:
      switch ((int)dt) {
        case ncclInt8: case ncclInt32: case ncclInt64:
        case ncclUint8: case ncclUint32: case ncclUint64:
          *devOp = OP_SUMPOSTDIV;
          *arg = ((uint64_t)nRanks << 1) | (isSigned ? 1 : 0);
          return ncclSuccess;
        case ncclFloat16: {
          *devOp = OP_PREMULSUM;
          _Float16 h = (_Float16)(float)(1.0 / nRanks);
          uint16_t b;
          memcpy(&b, &h, 2);
          *arg = b;
          return ncclSuccess;
        }
        case ncclBfloat16: {
          *devOp = OP_PREMULSUM;
          __bf16 h = (__bf16)(float)(1.0 / nRanks);
          uint16_t b;
          memcpy(&b, &h, 2);
          *arg = b;
          return ncclSuccess;
        }
        case ncclFloat32: {
          *devOp = OP_PREMULSUM;
          float f = (float)(1.0 / nRanks);
          uint32_t b;
          memcpy(&b, &f, 4);
          *arg = b;
          return ncclSuccess;
        }
        case ncclFloat64: {
          *devOp = OP_PREMULSUM;
          double d = 1.0 / nRanks;
          memcpy(arg, &d, 8);
          return ncclSuccess;
        }
        case ncclFloat8e4m3:
          *devOp = OP_PREMULSUM;
          *arg = f32_to_fp8_satfinite((float)(1.0 / nRanks), 3, 7, 0x7eu);
          return ncclSuccess;
        case ncclFloat8e5m2:
          *devOp = OP_PREMULSUM;
          *arg = f32_to_fp8_satfinite((float)(1.0 / nRanks), 2, 15, 0x7bu);
          return ncclSuccess;
      }
      return ncclInvalidArgument;
  }
  return ncclInvalidArgument;
}

// VCCL's channel partition of ring collectives: the host side of
// scheduleCollTasksToPlan (enqueue.cc:518-769) with the ring channel tuning
// of topoGetAlgoInfo (:1902-1925) and calcCollChunking's RING chunk
// (:2027-2032, 2093), so every element lands on the same channel and the same
// chunk of the same loop as in VCCL — hence the same ring and fold order.
// `count` / `eltSize` are already AG-rewritten to bytes.  Restated for the
// tests in oracle/vccl_sched.py.
//
// proto: kProtoSimple or kProtoLL128.  stepBytes: that protocol's FIFO step
// (buffSize / NCCL_STEPS).  nThreads: maxThreads[RING][proto] — NCCL_NTHREADS
// for SIMPLE (the ring kernel's own block size here, comm->nThreads),
// NCCL_LL128_NTHREADS (640) for LL128 (tuning.cc:198-211).
static int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }
int64_t traffic_per_byte(int coll, int nRanks) {  // ncclFuncTrafficPerByte (enqueue.cc:67-74)
  return coll == kAllReduce ? 2 : coll == kBroadcast || coll == kReduce ? 1 : nRanks;
}

// nMaxChannels of a task (or of an aggregate of tasks, ncclPrepareTasks):
// the ring / tree channel tuning on nBytes = eltSize * ncclFuncMaxSendRecvCount
// (enqueue.cc:1955, 1921-1924); thread thresholds (comm.h:38-40,
// tuning.cc:489-493) SIMPLE 64, LL128 8, LL 8 — times nRanks for the ring's
// LL (reduce-scatter / all-gather), not for the all-reduce's LL, which VCCL
// runs on its tree.  nThreads: maxThreads of the protocol (tuning.cc:198-211:
// NCCL_NTHREADS for SIMPLE and LL, NCCL_LL128_NTHREADS for LL128).
int ring_nmax_channels(int coll, int64_t count, int64_t eltSize, int nRanks, int commChannels,
                       int proto, int64_t nThreads) {
  const int64_t threshold = proto == kProtoSimple ? 64
                            : proto == kProtoLL128 || coll == kAllReduce ? 8 : 8 * (int64_t)nRanks;
  // ncclFuncMaxSendRecvCount (enqueue.h:36-38): RS / AG move n blocks
  const int64_t nBytes =
      eltSize * (coll == kReduceScatter || coll == kAllGather ? (int64_t)nRanks * count : count);
  int64_t nc = commChannels;
  while (nBytes < nc * nThreads * threshold && nc >= 2) nc--;
  return (int)nc;
}

// The cbd cell split of one task at the cursor (enqueue.cc:597-644; LL
// counts its traffic 4x, :599), then the cursor advanced past it (:667-681).
CbdPlan cbd_place(PlanCursor& pc, int coll, int64_t count, int64_t eltSize, int nRanks, int proto, int64_t stepBytes) {
  const bool ll128 = proto == kProtoLL128, ll = proto == kProtoLL;
  const uint64_t tpb = (uint64_t)traffic_per_byte(coll, nRanks) * (ll ? 4 : 1);
  const uint64_t cellSize = (uint64_t)div_up(div_up(kMinTraffic, tpb), 16) * 16;
  const uint64_t eltsPerCell = cellSize / (uint64_t)eltSize;
  const uint64_t cells = (uint64_t)div_up(count * eltSize, (int64_t)cellSize);
  const uint64_t trafficPerElement = (uint64_t)eltSize * tpb;
  const uint64_t trafficPerCell = cellSize * tpb;
  const uint64_t tpc = pc.trafficPerChannel;
  uint64_t cellsPerChannel = std::min(cells, (tpc + trafficPerCell - 1) / trafficPerCell);
  uint64_t cellsLo;
  if (pc.channelId + 1 == pc.nMax) cellsLo = cells;  // on the last channel everything goes to "lo"
  else cellsLo = std::min(cells, (tpc - pc.currentTraffic + trafficPerCell - 1) / trafficPerCell);
  int nMid = (int)((cells - cellsLo) / cellsPerChannel);
  uint64_t cellsHi = (cells - cellsLo) % cellsPerChannel;
  int nCh = (cellsLo != 0 ? 1 : 0) + nMid + (cellsHi != 0 ? 1 : 0);
  if (pc.nMax < pc.channelId + nCh) {  // overflowed the available channels
    nMid = pc.nMax - pc.channelId - 2;
    cellsPerChannel = (cells - cellsLo) / (uint64_t)(nMid + 1);
    cellsHi = cellsPerChannel + (cells - cellsLo) % (uint64_t)(nMid + 1);
  }
  if (cellsHi == 0 && nMid != 0) {
    cellsHi = cellsPerChannel;
    nMid -= 1;
  }
  if (cellsLo == 0) {  // least channel skipped: the next one becomes the least
    pc.channelId += 1;
    if (nMid == 0) {
      cellsLo = cellsHi;
      cellsHi = 0;
    } else {
      cellsLo = cellsPerChannel;
      nMid -= 1;
    }
  }
  CbdPlan p{};
  p.countMid = nMid != 0 ? (int64_t)(cellsPerChannel * eltsPerCell) : 0;
  p.countLo = (int64_t)(cellsLo * eltsPerCell);
  p.countHi = (int64_t)(cellsHi * eltsPerCell);
  (p.countHi != 0 ? p.countHi : p.countLo) -= (int64_t)(cells * eltsPerCell) - count;
  nCh = (p.countLo != 0 ? 1 : 0) + nMid + (cellsHi != 0 ? 1 : 0);
  p.channelLo = pc.channelId;
  p.channelHi = pc.channelId + nCh - 1;
  // RING chunk (calcCollChunking, enqueue.cc:2027-2032, 2093): SIMPLE =
  // chunkSteps (4) FIFO steps of buffSize / NCCL_STEPS (= one slot here);
  // LL128 = one step, 15/16 of it data; LL = half a step; rounded down to
  // the protocol grain (device.h:290-295: SIMPLE 512, LL128 1920, LL 16);
  // independent of size.
  // (broadcast / reduce: BROADCAST_CHUNKSTEPS / REDUCE_CHUNKSTEPS 1,
  // collectives.h:23-26)
  const int64_t grain = ll128 ? 1920 : ll ? 16 : 512;
  const int64_t chunkBytes =
      ll128 ? stepBytes / 16 * 15 : ll ? stepBytes / 2 : (coll == kBroadcast || coll == kReduce ? 1 : 4) * stepBytes;
  const int64_t chunkElts = chunkBytes / grain * grain / eltSize;
  p.chunkLo = p.chunkMid = p.chunkHi = chunkElts;
  // advance the cursor (enqueue.cc:667-681)
  if (p.countHi != 0) {
    pc.channelId += nCh - 1;
    pc.currentTraffic = cellsHi * eltsPerCell * trafficPerElement;
  } else if (nMid != 0) {
    pc.channelId += nCh;
    pc.currentTraffic = 0;
  } else {
    pc.currentTraffic += cellsLo * eltsPerCell * trafficPerElement;
  }
  if (pc.currentTraffic >= tpc && pc.channelId + 1 != pc.nMax) {
    pc.channelId += 1;
    pc.currentTraffic = 0;
  }
  return p;
}

// A plan holding one ring collective (a call outside a group).
CbdPlan cbd_schedule(int coll, int64_t count, int64_t eltSize, int nRanks, int commChannels,
                     int proto, int64_t stepBytes, int64_t nThreads) {
  const int nc = ring_nmax_channels(coll, count, eltSize, nRanks, commChannels, proto, nThreads);
  const uint64_t traffic = std::max<uint64_t>(
      kMinTraffic, (uint64_t)(count * eltSize) * traffic_per_byte(coll, nRanks) * (proto == kProtoLL ? 4 : 1));
  PlanCursor pc{std::max<uint64_t>(kMinTraffic, traffic / (uint64_t)std::min(nc, commChannels)), 0, 0,
                commChannels};
  return cbd_place(pc, coll, count, eltSize, nRanks, proto, stepBytes);
}

// ---------------------------------------------------------------- paths
// The path of a bucket (VCCL's topoGetAlgoInfo, enqueue.cc:1805-1945, reduced
// to one node over a full xGMI mesh): buckets up to the LL threshold take the
// one-hop LL path, the LL128 window (when enabled) the LL128 ring, up to the
// direct threshold the direct path (all-reduce two-shot, reduce-scatter /
// all-gather one-hop), larger ones the SIMPLE ring.  NCCL_ALGO / NCCL_PROTO
// force one: Ring/SIMPLE -> ring; Tree/LL -> LL where it fits; Direct -> direct
// where the mesh has it; LL128 -> the LL128 ring where its FIFOs exist;
// anything that does not fit falls through to the ring.  Broadcast and reduce
// take their rings unless the comm opted into the one-hop rooted LL kernels
// (llRootedMax, VCCL_LL_ROOTED_THRESHOLD; 0 = off) or the two-hop rooted direct
// kernels (directRootedMax, VCCL_DIRECT_ROOTED_THRESHOLD; 0 = off), in the
// order of the other collectives: LL, the LL128 window, direct, ring; forced
// Direct takes any size on a comm that opted in.  A pure function of
// the comm's thresholds (AlgoPolicy), so the group planner can ask it for an
// aggregate of calls as ncclPrepareTasks asks getAlgoInfo (enqueue.cc:398).
// count in elements of eltSize (all-gather: any element type, or bytes)
int select_algo(const AlgoPolicy& p, int coll, int64_t eltSize, int64_t count) {
  if (p.nRanks < 2 || p.algoForce == 1) return kAlgoRing;
  // NCCL_PROTO=LL128 (or vcclCommSetAlgo): the LL128 ring for every size
  if (p.algoForce == 4) return p.ll128 ? kAlgoRingLL128 : kAlgoRing;
  if (coll == kBroadcast || coll == kReduce) {
    const uint64_t bytes = (uint64_t)(count * eltSize);
    // the one-hop rooted LL kernels, when the comm opted in (llRootedMax, off
    // by default): automatic or forced LL; every other force keeps its ring
    if (p.llRootedMax > 0 && p.llSlotBytes > 0 && p.nRanks <= kOrderMaxRanks && bytes <= p.llRootedMax &&
        bytes <= (uint64_t)p.llSlotBytes && (p.algoForce == 0 || p.algoForce == 2))
      return kAlgoLL;
    // the two-hop direct kernels, when the comm opted in (directRootedMax, off
    // by default): forced Direct at any size, else behind the LL128 window
    const bool directOk = p.directRootedMax > 0 && p.direct && p.nRanks <= kDirectMaxRanks;
    if (directOk && p.algoForce == 3) return kAlgoDirect;
    // the rings of broadcast.h / reduce.h: SIMPLE or the LL128 window
    if (p.ll128 && p.ll128Max && bytes >= p.ll128Min && bytes <= p.ll128Max) return kAlgoRingLL128;
    return directOk && p.algoForce == 0 && bytes <= p.directRootedMax ? kAlgoDirect : kAlgoRing;
  }
  const uint64_t block = (uint64_t)(count * eltSize);
  // Reduce-scatter / all-gather: one rank's block must fit an LL slot; the
  // thresholds are on the whole bucket (n blocks), as the reference's tuner
  // sizes RS / AG (enqueue.cc:1955, ncclFuncMaxSendRecvCount).
  const uint64_t bytes = coll == kAllReduce ? block : block * (uint64_t)p.nRanks;
  const bool llFits = coll == kAllReduce
                          ? p.llSlotBytes > 0 && bytes <= p.llMax
                          : p.llSlotBytes > 0 && p.nRanks <= kOrderMaxRanks &&
                                block <= (uint64_t)p.llSlotBytes && bytes <= p.llRsAgMax;
  const bool directFits = p.direct && bytes <= (coll == kAllReduce ? p.directMax : p.directRsAgMax);
  if (p.algoForce == 2) return llFits ? kAlgoLL : kAlgoRing;
  // Forced direct: any bucket the inbox can stream (the size threshold only
  // steers the automatic choice); needs every peer's inbox mapped (no net
  // peers)
  if (p.algoForce == 3) return p.direct && p.nRanks <= kDirectMaxRanks ? kAlgoDirect : kAlgoRing;
  if (llFits) return kAlgoLL;
  // the LL128 ring over its window (the bucket, as the tuner sizes it), ahead
  // of the direct path
  if (p.ll128 && p.ll128Max && bytes >= p.ll128Min && bytes <= p.ll128Max) return kAlgoRingLL128;
  if (directFits) return kAlgoDirect;
  return kAlgoRing;
}
uint64_t ll_rooted_max(int64_t threshold, int64_t llSlotBytes, bool llAllowed, bool anyNet, int nRanks) {
  if (threshold <= 0 || llSlotBytes <= 0 || !llAllowed || anyNet || nRanks > kOrderMaxRanks) return 0;
  return (uint64_t)std::min(threshold, llSlotBytes);
}
uint64_t direct_rooted_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks) {
  if (threshold <= 0 || !inbox || !directAllowed || anyNet || nRanks > kDirectMaxRanks) return 0;
  return (uint64_t)threshold;
}
// The protocol VCCL runs a path's calls with: the one-hop LL stands in for
// VCCL's LL (tree for the all-reduce, ring otherwise), the direct path for a
// SIMPLE ring call.
int proto_of_algo(int algo) {
  return algo == kAlgoLL ? kProtoLL : algo == kAlgoRingLL128 ? kProtoLL128 : kProtoSimple;
}

// ---------------------------------------------------------------- group plan
// VCCL's plan for a group's collectives of one comm:
//  * taskAppend: trafficBytes = count * eltSize * trafficPerByte, inserted
//    into the size sorter (enqueue.cc:2405-2413; comm.h:294-343: 81 bins of
//    u32fpEncode(min(bytes, 1 GiB) >> 10, 2 bits) in descending size, LIFO
//    within a bin, bitops.h:252-262);
//  * ncclPrepareTasks (enqueue.cc:352-437): the sorted list binned by
//    (func, devOp, type) in LIFO order — each bin size-ascending, bins in
//    order of first appearance; runs within 4x of the run's first
//    trafficBytes aggregated; the path (select_algo, standing in for
//    getAlgoInfo's tuner) and nMaxChannels chosen on the aggregate's count
//    and given to every member; an LL member's trafficBytes x4 (:418);
//  * scheduleCollTasksToPlan (enqueue.cc:518-769): trafficPerChannel = the
//    plan's traffic / min(sum nMaxChannels, comm channels), each task placed
//    at the running channelId / currentTraffic under its protocol; a task
//    that would overflow the kernel-argument budget (testBudget :278-286:
//    16-byte work batches within 4 KiB - 32 B of kernel arguments, 96-byte
//    works within half the 1 MiB work FIFO; batches counted as
//    addWorkBatchToPlan :91-156 does, per device function and protocol)
//    starts the next plan.
// No policy: every call RING / SIMPLE.  Restated for the tests in
// oracle/vccl_sched.py (plan_schedule).
// group_task_of: all-gather / broadcast are int8 copies (enqueue.cc:2400-2404), keyed as such.
GroupTask group_task_of(int coll, size_t count, ncclDataType_t datatype, int devOp, int kernelType) {
  const bool ag = is_copy_coll(coll);
  const CallSize sz = call_size(coll, count, datatype);
  const int key = (coll * 16 + (ag ? (int)OP_SUM : devOp)) * 32;
  return GroupTask{coll, sz.count, sz.eltSize, key + (ag ? (int)ncclInt8 : (int)datatype), key + kernelType};
}
uint32_t u32fp_encode(uint32_t x, int bitsPerPow2) {  // bitops.h:252-262
  const int log2x = 31 - __builtin_clz(x | 1);
  const uint32_t mantissa = x >> (log2x >= bitsPerPow2 ? log2x - bitsPerPow2 : 0) & ((1u << bitsPerPow2) - 1);
  const uint32_t exponent = log2x >= bitsPerPow2 ? log2x - (bitsPerPow2 - 1) : 0;
  return exponent << bitsPerPow2 | mantissa;
}
void group_plan(const std::vector<GroupTask>& ts, int nRanks, int commChannels, const PlanGeometry& geo,
                const AlgoPolicy* pol, GroupPlanOut* out) {
  const int n = (int)ts.size();
  std::vector<uint64_t> traffic(n);
  for (int i = 0; i < n; i++)
    traffic[i] = (uint64_t)(ts[i].count * ts[i].eltSize) * traffic_per_byte(ts[i].coll, nRanks);
  // the size sorter: bins in descending size, LIFO within a bin
  constexpr int kBinCount = 1 + (30 - 10) * 4;
  std::vector<std::vector<int>> bins(kBinCount);
  for (int i = 0; i < n; i++) {
    const uint32_t x = (uint32_t)(std::min<uint64_t>(traffic[i], 1ull << 30) >> 10);
    bins[kBinCount - 1 - (int)u32fp_encode(x, 2)].push_back(i);
  }
  std::vector<int> sorted;
  for (auto& b : bins) sorted.insert(sorted.end(), b.rbegin(), b.rend());
  // (func, op, type) bins, LIFO, in order of first appearance
  std::vector<int> keys;
  std::vector<std::vector<int>> byKey;
  for (int i : sorted) {
    const size_t k = std::find(keys.begin(), keys.end(), ts[i].binKey) - keys.begin();
    if (k == keys.size()) {
      keys.push_back(ts[i].binKey);
      byKey.emplace_back();
    }
    byKey[k].insert(byKey[k].begin(), i);
  }
  auto step_of = [&](int proto) {
    return proto == kProtoLL ? kLLStepBytes : proto == kProtoLL128 ? geo.ll128StepBytes : geo.stepBytes;
  };
  std::vector<int> nMax(n), proto(n), queue;
  out->algo.assign(n, kAlgoRing);
  for (auto& lst : byKey) {
    for (size_t a = 0; a < lst.size();) {
      size_t e = a + 1;
      int64_t aggCount = ts[lst[a]].count;
      while (e < lst.size() && traffic[lst[e]] < 4 * traffic[lst[a]]) aggCount += ts[lst[e++]].count;
      const GroupTask& h = ts[lst[a]];
      const int algo = pol ? select_algo(*pol, h.coll, h.eltSize, aggCount) : kAlgoRing;
      const int pr = proto_of_algo(algo);
      const int nc = ring_nmax_channels(h.coll, aggCount, h.eltSize, nRanks, commChannels, pr,
                                        pr == kProtoLL128 ? geo.ll128Threads : geo.nThreads);
      for (size_t j = a; j < e; j++) {
        nMax[lst[j]] = nc;
        proto[lst[j]] = pr;
        out->algo[lst[j]] = algo;
        if (pr == kProtoLL) traffic[lst[j]] *= 4;
      }
      a = e;
    }
    queue.insert(queue.end(), lst.begin(), lst.end());
  }
  out->order = queue;
  out->planOf.assign(n, -1);
  out->cbd.assign(n, CbdPlan{});
  constexpr int64_t kWorkBytes = 96, kBatchBytes = 16;   // sizeof ncclDevWorkColl / ncclDevWorkBatch
  constexpr int64_t kInArgs = (4 << 10) - 32;            // workArgsBytes - sizeof(ncclDevKernelArgs)
  constexpr int64_t kOutArgs = (1 << 20) / 2;            // workFifoBytes / 2
  auto budget_ok = [&](int64_t nBatches, int64_t workBytes) {
    const int64_t bb = nBatches * kBatchBytes;
    return bb + workBytes <= kInArgs || (bb <= kInArgs && workBytes <= kOutArgs);
  };
  size_t head = 0;
  for (int plan = 0; head < queue.size(); plan++) {
    int nPlanColls = 0;
    uint64_t tb = 0;
    int nch = 0;
    for (size_t q = head, wb = 0; q < queue.size(); q++) {
      if (!budget_ok(div_up(nPlanColls, 4), (int64_t)wb + kWorkBytes)) break;
      nPlanColls++;
      wb += kWorkBytes;
      tb += std::max<uint64_t>(kMinTraffic, traffic[queue[q]]);
      nch = std::min(nch + nMax[queue[q]], commChannels);
    }
    PlanCursor pc{std::max<uint64_t>(kMinTraffic, tb / (uint64_t)std::max(nch, 1)), 0, 0, commChannels};
    // per channel: the work batch being filled (addWorkBatchToPlan)
    std::vector<int> lastFunc(commChannels, -1);
    std::vector<int64_t> offsetBase(commChannels, 0), wipBytes(commChannels, 0);
    int64_t nWorkBatches = 0, workBytes = 0;
    while (nPlanColls != 0 && head < queue.size()) {
      const int i = queue[head];
      PlanCursor trial = pc;
      const CbdPlan p = cbd_place(trial, ts[i].coll, ts[i].count, ts[i].eltSize, nRanks, proto[i],
                                  step_of(proto[i]));
      const int nChTask = p.channelHi - p.channelLo + 1;
      if (!budget_ok(nWorkBatches + nChTask, workBytes + kWorkBytes)) break;  // the next plan
      pc = trial;
      const int func = ts[i].funcKey * 4 + proto[i];  // devFuncId: (func, op, type, algo, proto)
      for (int c = p.channelLo; c <= p.channelHi && c < commChannels; c++) {
        const bool fresh = lastFunc[c] < 0 || lastFunc[c] != func ||
                           wipBytes[c] + kWorkBytes > 1024;  // NCCL_MAX_DEV_WORK_BATCH_BYTES
        const int64_t off = fresh ? 0 : workBytes - offsetBase[c];
        if (fresh || 63 * kWorkBytes < off) {
          offsetBase[c] = workBytes;
          if (fresh) wipBytes[c] = 0;
          nWorkBatches++;
        }
        lastFunc[c] = func;
        wipBytes[c] += kWorkBytes;
      }
      workBytes += kWorkBytes;
      out->planOf[i] = plan;
      out->cbd[i] = p;
      head++;
      nPlanColls--;
    }
  }
}

// ------------------------------------------------------------ rooted LL
ncclResult_t ll_rooted_plan(int coll, int nRanks, int rank, const std::vector<int>& roots,
                            const std::vector<int64_t>& bytes, int64_t linesPerSlot, LLRootedPlanOut* out) {
  const bool reduce = coll == kReduce;
  const int nParts = (int)roots.size();
  out->line0.assign(nParts, 0);
  out->stores.clear();
  out->polls.clear();
  int64_t lines = 0;
  int root0 = -1;  // the root of the part holding line 0
  for (int i = 0; i < nParts; i++) {
    out->line0[i] = lines;
    const int64_t nl = (bytes[i] + 7) / 8;
    if (nl > 0 && root0 < 0) root0 = roots[i];
    lines += nl;
  }
  out->nLines = lines;
  if (lines > linesPerSlot) return ncclInvalidArgument;
  for (int k = 1; k < nRanks; k++) {
    const int peer = (rank + k) % nRanks;
    for (int i = 0; i < nParts; i++) {
      const int64_t l0 = out->line0[i], l1 = l0 + (bytes[i] + 7) / 8;
      if (l1 == l0) continue;
      // broadcast: the root writes to everyone; reduce: everyone to the root
      if (reduce ? roots[i] == peer : roots[i] == rank) out->stores.push_back(LLRange{peer, i, l0, l1});
      if (reduce ? roots[i] == rank : roots[i] == peer) out->polls.push_back(LLRange{peer, i, l0, l1});
    }
    if (root0 < 0 || !ll_rooted_line0_is_data(reduce, rank, peer, root0)) out->stores.push_back(LLRange{peer, -1, 0, 1});
    if (root0 < 0 || !ll_rooted_line0_is_data(reduce, peer, rank, root0)) out->polls.push_back(LLRange{peer, -1, 0, 1});
  }
  return ncclSuccess;
}

// ------------------------------------------------------------ rooted direct
// The steps below are direct.hpp's phase order (direct_broadcast_part: scatter,
// forward, gather, ack; direct_reduce_part: scatter, fold, collect), rank by
// rank; the peer loops run in the kernels' rotation, (rank + k) mod n.
ncclResult_t direct_rooted_plan(int coll, int nRanks, int rank, int root, int64_t count, int64_t eltSize,
                                int64_t regionBytes, int chunk, DirectRootedPlanOut* out) {
  const bool reduce = coll == kReduce;
  const int n = nRanks, nShards = direct_rooted_shards(reduce, n);
  const int64_t esz = eltSize, eltAlign = std::max<int64_t>(1, 16 / esz);
  const int64_t regionElts = (regionBytes - 16) / esz / eltAlign * eltAlign;  // whole 16-byte units
  if (regionElts < eltAlign || nShards < 1) return ncclInvalidArgument;
  out->owner.clear();
  out->steps.clear();
  out->chunkElts = std::min<int64_t>(count, regionElts * nShards);
  const int64_t nChunks = out->chunkElts > 0 ? (count + out->chunkElts - 1) / out->chunkElts : 0;
  if (nChunks > INT32_MAX) return ncclInvalidArgument;
  out->nChunks = (int)nChunks;
  out->shardElts = 0;
  for (int j = 0; j < nShards; j++) out->owner.push_back(reduce ? j : direct_bcast_owner(root, j, n));
  if (chunk < 0) return ncclSuccess;
  if (chunk >= out->nChunks) return ncclInvalidArgument;
  const int64_t c0 = (int64_t)chunk * out->chunkElts, cc = std::min(out->chunkElts, count - c0);
  const int64_t shard = direct_shard_elts(cc, nShards, eltAlign);
  out->shardElts = shard;
  auto off_of = [&](int j) { return (c0 + std::min((int64_t)j * shard, cc)) * esz; };          // user offset, bytes
  auto len_of = [&](int j) { return (std::min((int64_t)(j + 1) * shard, cc) - std::min((int64_t)j * shard, cc)) * esz; };
  auto& st = out->steps;
  auto peers = [&](auto f) {
    for (int k = 1; k < n; k++) f((rank + k) % n);
  };
  if (!reduce) {
    if (rank == root) {
      for (int j = 0; j < nShards; j++)  // scatter
        st.push_back(DirectStep{kDStepStore, 0, out->owner[j], root, 0, off_of(j), len_of(j), kDSrcSend});
    } else {
      const int mine = direct_bcast_shard_of(root, rank, n);
      st.push_back(DirectStep{kDStepWait, 0, root, 0, 0, 0, 0, 0});  // the root alone
      peers([&](int q) {  // forward
        if (q != root) st.push_back(DirectStep{kDStepStore, 0, q, rank, 0, off_of(mine), len_of(mine), kDSrcRegion});
      });
      st.push_back(DirectStep{kDStepRead, 0, rank, root, 0, off_of(mine), len_of(mine), 0});
    }
    st.push_back(DirectStep{kDStepPost, 0, 0, 0, 0, 0, 0, 0});
    peers([&](int q) { st.push_back(DirectStep{kDStepWait, 0, q, 0, 0, 0, 0, 0}); });  // gather
    if (rank == root) {
      st.push_back(DirectStep{kDStepLocal, 0, rank, 0, 0, c0 * esz, cc * esz, kDSrcSend});
    } else {
      peers([&](int o) {
        if (o == root) return;
        const int j = direct_bcast_shard_of(root, o, n);
        st.push_back(DirectStep{kDStepRead, 0, rank, o, 0, off_of(j), len_of(j), 0});
      });
    }
    st.push_back(DirectStep{kDStepPost, 1, 0, 0, 0, 0, 0, 0});  // ack
    peers([&](int q) { st.push_back(DirectStep{kDStepWait, 1, q, 0, 0, 0, 0, 0}); });
    return ncclSuccess;
  }
  peers([&](int p) { st.push_back(DirectStep{kDStepStore, 0, p, rank, 0, off_of(p), len_of(p), kDSrcSend}); });  // scatter
  st.push_back(DirectStep{kDStepPost, 0, 0, 0, 0, 0, 0, 0});
  peers([&](int q) { st.push_back(DirectStep{kDStepWait, 0, q, 0, 0, 0, 0, 0}); });  // fold
  if (rank == root) st.push_back(DirectStep{kDStepLocal, 0, rank, 0, 0, off_of(rank), len_of(rank), kDSrcFold});
  else st.push_back(DirectStep{kDStepStore, 1, root, rank, 0, off_of(rank), len_of(rank), kDSrcFold});
  st.push_back(DirectStep{kDStepPost, 1, 0, 0, 0, 0, 0, 0});
  peers([&](int q) { st.push_back(DirectStep{kDStepWait, 1, q, 0, 0, 0, 0, 0}); });  // collect
  if (rank == root)
    peers([&](int o) { st.push_back(DirectStep{kDStepRead, 1, rank, o, 0, off_of(o), len_of(o), 0}); });
  return ncclSuccess;
}

// -------------------------------------------------------- registered buffers
uint64_t reg_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks) {
  if (threshold <= 0 || !inbox || !directAllowed || anyNet || nRanks < 2 || nRanks > kDirectMaxRanks) return 0;
  return (uint64_t)threshold;
}
int64_t reg_call_bytes(int coll, int64_t count, int64_t typeSize, int nRanks) {
  return coll == kAllReduce ? count * typeSize : (int64_t)nRanks * count * typeSize;
}
bool reg_eligible(int coll, int64_t count, int64_t typeSize, int nRanks, uint64_t effective, int groupCalls) {
  if (effective == 0 || groupCalls > 1) return false;
  if (coll != kAllReduce && coll != kReduceScatter && coll != kAllGather) return false;
  return (uint64_t)reg_call_bytes(coll, count, typeSize, nRanks) >= effective;
}

// The steps below are the zero-copy kernels' order, rank by
// rank; the peer loops run in the direct kernels' rotation, (rank + k) mod n.
ncclResult_t reg_plan(int coll, int nRanks, int rank, int64_t count, int64_t eltSize, int nBlocks, RegPlanOut* out) {
  if (coll != kAllReduce && coll != kReduceScatter && coll != kAllGather) return ncclInvalidArgument;
  const int n = nRanks;
  const int64_t esz = eltSize, eltAlign = std::max<int64_t>(1, 16 / esz);
  const int64_t shard = coll == kAllReduce ? direct_shard_elts(count, n, eltAlign) : count;
  out->shardElts = shard;
  out->blkElts = ((shard + nBlocks - 1) / nBlocks + eltAlign - 1) / eltAlign * eltAlign;
  auto& st = out->steps;
  st.clear();
  auto post = [&](int epoch, int phase) { st.push_back(RegStep{kRStepPost, epoch, phase, 0, 0, 0, 0, 0}); };
  auto wait = [&](int epoch, int phase) {
    for (int k = 1; k < n; k++) st.push_back(RegStep{kRStepWait, epoch, phase, (rank + k) % n, 0, 0, 0, 0});
  };
  // epoch 0: descriptors out ("my input is ready"), descriptors in, verdicts out, verdicts in
  post(0, 0);
  wait(0, 0);
  post(0, 1);
  wait(0, 1);
  if (coll == kAllReduce) {
    // shard o = elements [o * shard, min((o + 1) * shard, count)), owned by rank o
    auto lo_of = [&](int o) { return std::min((int64_t)o * shard, count) * esz; };
    auto len_of = [&](int o) { return std::min((int64_t)(o + 1) * shard, count) * esz - lo_of(o); };
    for (int k = 0; k < n; k++)  // fold my shard from the n inputs
      st.push_back(RegStep{kRStepFold, 1, 0, (rank + k) % n, kRBufSend, lo_of(rank), lo_of(rank), len_of(rank)});
    post(1, 0);  // "shard `rank` of my recvbuff is final, and I have finished reading your inputs"
    wait(1, 0);
    for (int k = 1; k < n; k++) {  // pull the other owners' shards from THEIR recvbuff
      const int o = (rank + k) % n;
      st.push_back(RegStep{kRStepCopy, 1, 0, o, kRBufRecv, lo_of(o), lo_of(o), len_of(o)});
    }
    post(1, 1);  // "finished reading your recvbuff"
    wait(1, 1);
    return ncclSuccess;
  }
  for (int k = 0; k < n; k++) {
    const int p = (rank + k) % n;
    if (coll == kReduceScatter)  // block `rank` of every input -> my recvbuff
      st.push_back(RegStep{kRStepFold, 1, 0, p, kRBufSend, (int64_t)rank * count * esz, 0, count * esz});
    else  // every rank's input -> block p of my recvbuff
      st.push_back(RegStep{kRStepCopy, 1, 0, p, kRBufSend, 0, (int64_t)p * count * esz, count * esz});
  }
  post(1, 0);  // "I have finished reading you"
  wait(1, 0);
  post(1, 1);  // the closing round (reuse rule R2, direct.hpp)
  wait(1, 1);
  return ncclSuccess;
}

// -------------------------------------- rooted collectives over registered buffers
uint64_t reg_rooted_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks,
                        bool allRegistries) {
  if (!allRegistries) return 0;
  return reg_max(threshold, inbox, directAllowed, anyNet, nRanks);
}
bool reg_rooted_eligible(int coll, int64_t count, int64_t typeSize, uint64_t effective, int groupCalls) {
  if (effective == 0 || groupCalls > 1) return false;
  if (coll != kBroadcast && coll != kReduce) return false;
  return (uint64_t)(count * typeSize) >= effective;
}

// The steps below are reg_broadcast_zc's / reg_reduce_zc's order
// (device/direct_reg.hpp), rank by rank; the peer loops run in the direct
// kernels' rotation, (rank + k) mod n.
ncclResult_t reg_rooted_plan(int coll, int nRanks, int rank, int root, int64_t count, int64_t eltSize,
                             int64_t regionBytes, int nBlocks, RegRootedPlanOut* out) {
  if (coll != kBroadcast && coll != kReduce) return ncclInvalidArgument;
  const int n = nRanks;
  if (n < 2 || n > kDirectMaxRanks || rank < 0 || rank >= n || root < 0 || root >= n || nBlocks < 1 || count < 1)
    return ncclInvalidArgument;
  const int64_t esz = eltSize, eltAlign = std::max<int64_t>(1, 16 / esz);
  auto& st = out->steps;
  st.clear();
  auto post = [&](int epoch, int phase) { st.push_back(RegStep{kRStepPost, epoch, phase, 0, 0, 0, 0, 0}); };
  auto wait = [&](int epoch, int phase) {
    for (int k = 1; k < n; k++) st.push_back(RegStep{kRStepWait, epoch, phase, (rank + k) % n, 0, 0, 0, 0});
  };
  // epoch 0: descriptors out, descriptors in, verdicts out, verdicts in
  post(0, 0);
  wait(0, 0);
  post(0, 1);
  wait(0, 1);
  if (coll == kBroadcast) {
    // shard j = bytes [j * shard, min((j + 1) * shard, count)), owned by direct_bcast_owner(root, j, n)
    const int64_t shard = direct_shard_elts(count, n - 1, 16);
    out->shardElts = shard;
    out->blkElts = ((shard + nBlocks - 1) / nBlocks + 15) / 16 * 16;
    out->nChunks = 1;
    out->chunkElts = count;
    auto lo_of = [&](int j) { return std::min((int64_t)j * shard, count); };
    auto len_of = [&](int j) { return std::min((int64_t)(j + 1) * shard, count) - lo_of(j); };
    if (rank != root) {  // my shard, from the root's sendbuff
      const int j = direct_bcast_shard_of(root, rank, n);
      st.push_back(RegStep{kRStepCopy, 1, 0, root, kRBufSend, lo_of(j), lo_of(j), len_of(j)});
    } else {  // send -> recv, shard by shard (nothing in place)
      for (int j = 0; j < n - 1; j++)
        st.push_back(RegStep{kRStepCopy, 1, 0, rank, kRBufSend, lo_of(j), lo_of(j), len_of(j)});
    }
    post(1, 0);  // "my shard in my recvbuff is final, and I have finished reading the root"
    wait(1, 0);
    if (rank != root) {
      for (int k = 1; k < n; k++) {  // the other shards, from their owners' recvbuff
        const int o = (rank + k) % n;
        if (o == root) continue;
        const int j = direct_bcast_shard_of(root, o, n);
        st.push_back(RegStep{kRStepCopy, 1, 0, o, kRBufRecv, lo_of(j), lo_of(j), len_of(j)});
      }
    }
    post(1, 1);  // "finished reading your recvbuff"
    wait(1, 1);
    return ncclSuccess;
  }
  DirectRootedPlanOut geo;
  if (direct_rooted_plan(kReduce, n, rank, root, count, esz, regionBytes, -1, &geo) != ncclSuccess)
    return ncclInvalidArgument;
  out->chunkElts = geo.chunkElts;
  out->nChunks = geo.nChunks;
  out->shardElts = direct_shard_elts(geo.chunkElts, n, eltAlign);
  out->blkElts = 0;
  for (int c = 0; c < geo.nChunks; c++) {
    const int ep = 1 + c;
    const int64_t c0 = (int64_t)c * geo.chunkElts, cc = std::min(geo.chunkElts, count - c0);
    const int64_t shard = direct_shard_elts(cc, n, eltAlign);
    auto off_of = [&](int o) { return (c0 + std::min((int64_t)o * shard, cc)) * esz; };
    auto len_of = [&](int o) { return (c0 + std::min((int64_t)(o + 1) * shard, cc)) * esz - off_of(o); };
    post(ep, 0);  // no data: R1, and my collect of the previous chunk precedes it
    wait(ep, 0);
    for (int k = 0; k < n; k++)  // fold my shard from the n user inputs
      st.push_back(RegStep{kRStepFold, ep, 0, (rank + k) % n, kRBufSend, off_of(rank),
                           rank == root ? off_of(rank) : (int64_t)-1, len_of(rank)});
    if (rank != root) st.push_back(RegStep{kRStepStoreRoot, ep, 1, root, 0, 0, off_of(rank), len_of(rank)});
    post(ep, 1);  // "my shard is delivered, and I have finished reading your inputs of this chunk"
    wait(ep, 1);
    if (rank == root)
      for (int k = 1; k < n; k++) {
        const int o = (rank + k) % n;
        st.push_back(RegStep{kRStepCollect, ep, 1, o, 0, 0, off_of(o), len_of(o)});
      }
  }
  return ncclSuccess;
}

// ------------------------------------------- all-to-all over registered buffers
uint64_t reg_a2a_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks, bool hasP2p,
                     bool allRegistries) {
  if (!hasP2p || !allRegistries) return 0;
  return reg_max(threshold, inbox, directAllowed, anyNet, nRanks);
}
bool reg_a2a_eligible(bool uniform, int64_t pairBytes, uint64_t effective, int index) {
  if (effective == 0 || index < 0 || index >= kRegA2aMaxCalls) return false;
  return !uniform || (uint64_t)pairBytes >= effective;
}
bool reg_a2a_size_vote(int nRanks, int rank, const int64_t* sendBytes, const int64_t* recvBytes, bool uniform,
                       uint64_t effective) {
  if (uniform) return true;
  int64_t largest = 0;
  for (int p = 0; p < nRanks; p++)
    if (p != rank) largest = std::max({largest, sendBytes[p], recvBytes[p]});
  return (uint64_t)largest >= effective;
}
int reg_a2a_blocks(bool uniform, int64_t pairBytes, int minCTAs, int maxCTAs, int directMaxBlocks) {
  if (uniform) {
    const int64_t blk = reg_a2a_blk(pairBytes, minCTAs, maxCTAs, directMaxBlocks);
    return (int)std::max<int64_t>(1, (pairBytes + blk - 1) / blk);
  }
  // direct_blk_elts' block count for a block of any length
  const int64_t nb = std::max<int64_t>(std::min<int64_t>(kDirectMaxBlocks, maxCTAs), minCTAs);
  return (int)std::max<int64_t>(1, std::min<int64_t>({nb, (int64_t)directMaxBlocks, (int64_t)kDirectMaxBlocks}));
}
int64_t reg_a2a_blk(int64_t bytes, int minCTAs, int maxCTAs, int directMaxBlocks) {
  return std::max<int64_t>(16, direct_blk_elts(bytes, 1, minCTAs, maxCTAs, directMaxBlocks));
}

// The steps below are direct_reg_alltoall's order (device/direct_reg.hpp), rank
// by rank; the peer loops run in the direct kernels' rotation, (rank + k) mod n.
ncclResult_t reg_a2a_plan(int nRanks, int rank, const int64_t* sendBytes, const int64_t* sendOff,
                          const int64_t* recvOff, bool uniform, int minCTAs, int maxCTAs, int directMaxBlocks,
                          RegA2aPlanOut* out) {
  const int n = nRanks;
  if (n < 2 || n > kDirectMaxRanks || rank < 0 || rank >= n) return ncclInvalidArgument;
  out->nBlocks = reg_a2a_blocks(uniform, sendBytes[0], minCTAs, maxCTAs, directMaxBlocks);
  auto& st = out->steps;
  st.clear();
  auto post = [&](int epoch, int phase) { st.push_back(RegA2aStep{kAStepPost, epoch, phase, 0, 0, 0, 0, 0}); };
  auto wait = [&](int epoch, int phase) {
    for (int k = 1; k < n; k++) st.push_back(RegA2aStep{kAStepWait, epoch, phase, (rank + k) % n, 0, 0, 0, 0});
  };
  post(0, 0);  // the descriptor of my block for each peer, "my input is ready"
  wait(0, 0);
  st.push_back(RegA2aStep{kAStepVote, 0, 0, 0, 0, 0, 0, 0});
  post(0, 1);
  wait(0, 1);
  for (int k = 1; k <= n; k++) {  // the peers in rotation, then the self block
    const int p = (rank + k) % n;
    const int64_t bytes = sendBytes[(size_t)p * n + rank];
    const int64_t blk = reg_a2a_blk(bytes, minCTAs, maxCTAs, directMaxBlocks);
    if ((bytes + blk - 1) / blk > out->nBlocks) return ncclInternalError;
    st.push_back(RegA2aStep{p == rank ? kAStepSelf : kAStepPull, 1, 0, p, sendOff[(size_t)p * n + rank], recvOff[p],
                            bytes, blk});
  }
  post(1, 0);  // "I have finished reading you"
  wait(1, 0);
  post(1, 1);  // the closing round (reuse rule R2, direct.hpp)
  wait(1, 1);
  return ncclSuccess;
}

// ---------------------------------------------------------------- all-to-all
uint64_t ll_a2a_max(int64_t threshold, int64_t llSlotBytes, bool llAllowed, bool anyNet, int nRanks, bool hasP2p) {
  if (threshold <= 0 || llSlotBytes <= 0 || !llAllowed || anyNet || nRanks < 2 || nRanks > kOrderMaxRanks || !hasP2p)
    return 0;
  return (uint64_t)std::min(threshold, llSlotBytes);
}
uint64_t direct_a2a_max(int64_t threshold, int64_t regionBytes, bool directAllowed, bool anyNet, int nRanks,
                        bool hasP2p) {
  if (threshold <= 0 || regionBytes <= 16 || !directAllowed || anyNet || nRanks < 2 || nRanks > kDirectMaxRanks ||
      !hasP2p)
    return 0;
  return (uint64_t)std::min(threshold, (regionBytes - 16) / 16 * 16);
}

ncclResult_t a2a_plan(int nRanks, int rank, const int64_t* sendBytes, const int64_t* recvBytes, bool uniform,
                      uint64_t llA2aMax, uint64_t directA2aMax, int64_t linesPerSlot, int minCTAs, int maxCTAs,
                      int directMaxBlocks, A2aPlanOut* out) {
  const int n = nRanks;
  // the launch rule: a v-call launches every path that is on; a uniform call,
  // whose pairs all carry sendBytes[0], the one path they all take
  const int uniformPath = a2a_pair_path(llA2aMax, directA2aMax, sendBytes[0]);
  auto launches = [&](uint64_t limit, int path) {
    return limit > 0 && (!uniform || (sendBytes[0] > 0 && uniformPath == path));
  };
  out->llLaunch = launches(llA2aMax, kA2aLL);
  out->directLaunch = launches(directA2aMax, kA2aDirect);
  // a path without its launch takes no pair
  const uint64_t llMax = out->llLaunch ? llA2aMax : 0, directMax = out->directLaunch ? directA2aMax : 0;
  out->sendPath.assign(n, kA2aFifo);
  out->recvPath.assign(n, kA2aFifo);
  out->stores.clear();
  out->polls.clear();
  out->resSends.clear();
  out->resRecvs.clear();
  for (int k = 0; k < n; k++) {  // the kernels' rotation
    const int p = (rank + k) % n;
    // the self block: its path when both lengths agree, else the FIFO launch's copy (or its refusal)
    if (p == rank && sendBytes[p] != recvBytes[p]) continue;
    const int s = out->sendPath[p] = (char)a2a_pair_path(llMax, directMax, sendBytes[p]);
    const int r = out->recvPath[p] = (char)a2a_pair_path(llMax, directMax, recvBytes[p]);
    if (p == rank || !out->llLaunch) continue;
    const int64_t sl = s == kA2aLL ? (sendBytes[p] + 7) / 8 : 0, rl = r == kA2aLL ? (recvBytes[p] + 7) / 8 : 0;
    if (sl > linesPerSlot || rl > linesPerSlot) return ncclInvalidArgument;
    out->stores.push_back(sl > 0 ? LLRange{p, 0, 0, sl} : LLRange{p, -1, 0, 1});
    out->polls.push_back(rl > 0 ? LLRange{p, 0, 0, rl} : LLRange{p, -1, 0, 1});
  }
  for (int p = 0; p < n; p++) {
    if (out->sendPath[p] == kA2aFifo) out->resSends.push_back(p);
    if (out->recvPath[p] == kA2aFifo) out->resRecvs.push_back(p);
  }
  out->nBlocks = 0;
  out->blkBytes = 0;
  if (out->directLaunch) {
    const int64_t M = uniform ? sendBytes[0] : (int64_t)directA2aMax;
    out->blkBytes = direct_blk_elts(M, 1, minCTAs, maxCTAs, directMaxBlocks);
    out->nBlocks = (int)((M + out->blkBytes - 1) / out->blkBytes);
  }
  return ncclSuccess;
}

// ------------------------------------------------------------ point-to-point
P2pSplit p2p_split(int64_t bytes, const P2pGeometry& g) {
  if (bytes <= 0) return P2pSplit{0, 0};
  const int64_t want = (bytes + g.minPartBytes - 1) / g.minPartBytes;
  const int64_t p = std::max<int64_t>(1, std::min<int64_t>(want, g.parts));
  const int64_t len = ((bytes + p - 1) / p + 15) / 16 * 16;
  return P2pSplit{(int)((bytes + len - 1) / len), len};
}

ncclResult_t p2p_plan(int rank, int nRanks, const std::vector<P2pCall>& calls, const P2pGeometry& g, int gMin,
                      int gCap, int maxWorks, P2pPlanOut* out) {
  out->items.clear();
  out->nWgs = out->nLaunches = 0;
  const int n = nRanks;
  // per peer, in call order (enqueue.cc:2318-2337)
  std::vector<std::vector<int>> sends(n), recvs(n);
  for (int i = 0; i < (int)calls.size(); i++)
    (calls[i].kind == kP2pCallSend ? sends : recvs)[calls[i].peer].push_back(i);
  // self traffic is matched inside the group (enqueue.cc:1057-1066)
  if (sends[rank].size() != recvs[rank].size()) return ncclInvalidUsage;
  for (size_t s = 0; s < sends[rank].size(); s++)
    if (calls[sends[rank][s]].bytes != calls[recvs[rank][s]].bytes) return ncclInvalidUsage;
  size_t nSweeps = 0;
  for (int p = 0; p < n; p++) nSweeps = std::max({nSweeps, sends[p].size(), recvs[p].size()});
  // a send-side / receive-side connection -> its index in order of first use
  std::vector<int> sendIx(n * g.parts, -1), recvIx(n * g.parts, -1);
  int nSend = 0, nRecv = 0;
  for (size_t s = 0; s < nSweeps; s++) {
    for (int d = 0; d < n; d++) {
      const int to = (rank + d) % n, from = (rank - d + n) % n;
      const int sc = s < sends[to].size() ? sends[to][s] : -1;
      const int rc = s < recvs[from].size() ? recvs[from][s] : -1;
      if (d == 0) {  // both or neither (checked above)
        if (sc < 0 || calls[sc].buff == calls[rc].buff) continue;
        const P2pSplit sp = p2p_split(calls[sc].bytes, g);
        for (int q = 0; q < sp.nParts; q++) {
          const int64_t off = q * sp.partBytes;
          int& ix = sendIx[rank * g.parts + q];
          if (ix < 0) ix = nSend++;
          out->items.push_back(P2pItem{0, ix, 2, (int)s, d, q, rank, sc, rc, off,
                                       std::min(sp.partBytes, calls[sc].bytes - off), 0});
        }
        continue;
      }
      const P2pSplit ss = sc >= 0 ? p2p_split(calls[sc].bytes, g) : P2pSplit{0, 0};
      const P2pSplit rs = rc >= 0 ? p2p_split(calls[rc].bytes, g) : P2pSplit{0, 0};
      for (int q = 0; q < std::max(ss.nParts, rs.nParts); q++) {
        if (q < ss.nParts) {
          const int64_t off = q * ss.partBytes, len = std::min(ss.partBytes, calls[sc].bytes - off);
          int& ix = sendIx[to * g.parts + q];
          if (ix < 0) ix = nSend++;
          out->items.push_back(P2pItem{0, ix, 0, (int)s, d, q, to, sc, -1, off, len,
                                       (len + g.stepBytes - 1) / g.stepBytes});
        }
        if (q < rs.nParts) {
          const int64_t off = q * rs.partBytes, len = std::min(rs.partBytes, calls[rc].bytes - off);
          int& ix = recvIx[from * g.parts + q];
          if (ix < 0) ix = nRecv++;
          out->items.push_back(P2pItem{0, ix, 1, (int)s, d, q, from, rc, -1, off, len,
                                       (len + g.stepBytes - 1) / g.stepBytes});
        }
      }
    }
  }
  // the grid: one workgroup per connection in use and direction, within the
  // CTA floor and then the co-residency cap (I4)
  int G = std::max(std::max(nSend, nRecv), gMin);
  if (gCap > 0) G = std::min(G, gCap);
  G = std::max(G, 1);
  out->nWgs = G;
  for (size_t k = 0; k < out->items.size(); k++) {
    P2pItem& it = out->items[k];
    it.wg = it.kind == 1 ? G + it.wg % G : it.wg % G;  // I1: a function of the connection alone
    it.launch = (int)(k / (size_t)maxWorks);
  }
  out->nLaunches = (int)((out->items.size() + maxWorks - 1) / maxWorks);
  return ncclSuccess;
}

}  // namespace vccl
