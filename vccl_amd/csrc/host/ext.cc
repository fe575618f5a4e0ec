// The vccl* extension exports (include/vccl_ext.h) that belong to the call
// path: wrappers over the pure planner (plan.h) on explicit inputs, and the
// queries and knobs of a live comm (launch.h, core.h).  Host only unless a
// comment says otherwise; the nccl* API itself is enqueue.cc.
#include <algorithm>
#include <vector>

#include "../../../include/vccl_device.h"
#include "../../../include/vccl_ext.h"
#include "../device/coll_types.hpp"
#include "../device/dispatch.hpp"
#include "launch.h"
#include "regcomm.h"

namespace vccl {

// The internal path codes (plan.h kAlgo*) and the public vcclAlgo_t.
static int public_algo(int a) {
  return a == kAlgoLL ? vcclAlgoLL : a == kAlgoDirect ? vcclAlgoDirect
         : a == kAlgoRingLL128 ? vcclAlgoLL128 : vcclAlgoRing;
}
static int internal_algo(int pub) {  // -1: not a path a call can be given
  return pub == vcclAlgoRing ? kAlgoRing : pub == vcclAlgoLL ? kAlgoLL
         : pub == vcclAlgoDirect ? kAlgoDirect : pub == vcclAlgoLL128 ? kAlgoRingLL128 : -1;
}

// The ten policy words of vccl_ext.h are AlgoPolicy's fields after nRanks, in
// order.  false: a forced path outside 0 .. 4.
static bool policy_of_words(const int64_t* q, int nRanks, AlgoPolicy* pol) {
  if (q[0] < 0 || q[0] > 4) return false;
  *pol = AlgoPolicy{nRanks, (int)q[0], q[1], (uint64_t)q[2], (uint64_t)q[3], q[4] != 0, (uint64_t)q[5],
                    (uint64_t)q[6], q[7] != 0, (uint64_t)q[8], (uint64_t)q[9]};
  return true;
}

// LLRange vectors as the exports report them: four words per range.
static void put_ranges(const std::vector<LLRange>& v, int64_t* o) {
  for (size_t k = 0; k < v.size(); k++) {
    o[4 * k] = v[k].peer, o[4 * k + 1] = v[k].part, o[4 * k + 2] = v[k].line0, o[4 * k + 3] = v[k].line1;
  }
}

// The per-peer byte rows of an all-to-all plan export, checked (a uniform
// call's rows all hold sendBytes[0]) and copied for a2a_plan.
static bool a2a_rows(int nRanks, const size_t* sendBytes, const size_t* recvBytes, int uniform, int64_t* sb,
                     int64_t* rb) {
  for (int p = 0; p < nRanks; p++) {
    if (sendBytes[p] > (size_t)1 << 60 || recvBytes[p] > (size_t)1 << 60) return false;
    if (uniform && (sendBytes[p] != sendBytes[0] || recvBytes[p] != sendBytes[0])) return false;
    sb[p] = (int64_t)sendBytes[p];
    rb[p] = (int64_t)recvBytes[p];
  }
  return true;
}
static void put_residuals(const A2aPlanOut& out, int* nResSends, int* resSends, int* nResRecvs, int* resRecvs) {
  *nResSends = (int)out.resSends.size();
  *nResRecvs = (int)out.resRecvs.size();
  std::copy(out.resSends.begin(), out.resSends.end(), resSends);
  std::copy(out.resRecvs.begin(), out.resRecvs.end(), resRecvs);
}

}  // namespace vccl

using namespace vccl;

VCCL_EXPORT ncclResult_t vcclHostToDevRedOp(ncclRedOp_t op, ncclDataType_t datatype, int nRanks,
                                            int* devOp, uint64_t* opArg) {
  if (!devOp || !opArg || nRanks < 1) return ncclInvalidArgument;
  if ((int)datatype < 0 || (int)datatype >= (int)ncclNumTypes) return ncclInvalidArgument;
  return host_to_dev_redop(op, datatype, nRanks, devOp, opArg);
}

VCCL_EXPORT const char* vcclBuildInfo(void) {
#define VCCL_STR2(x) #x
#define VCCL_STR(x) VCCL_STR2(x)
  return "vccl-mi355x " __DATE__ " gfx950; one-shot LL / two-shot direct / SIMPLE ring / LL128 ring "
         "(" VCCL_STR(VCCL_LL128_LINE) "-byte lines) over xGMI (uncached receiver buffers); "
         "reduce-copy 16B packs; VCCL group plans";
}

VCCL_EXPORT ncclResult_t vcclCommCollAlgo(ncclComm_t comm, int coll, size_t count, ncclDataType_t datatype, int* algo) {
  NCCLCHECK(comm_check(comm, "vcclCommCollAlgo"));
  if (!algo || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1) return ncclInvalidArgument;
  if (comm->nRanks == 1) {
    *algo = vcclAlgoOneRank;
    return ncclSuccess;
  }
  // the public collective codes are the Coll values (vccl_ext.h)
  *algo = public_algo(select_algo(policy_of(comm), coll, type_size(datatype), (int64_t)count));
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRingPartition(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                           int nChannels, int proto, size_t stepBytes, int nThreads,
                                           int64_t* out) {
  if (!out || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1 || nRanks < 1 ||
      nChannels < 1 || nChannels > kMaxChannels || count == 0 || stepBytes < 4096 || nThreads < 64 ||
      (proto != kProtoSimple && proto != kProtoLL128 && proto != kProtoLL))
    return ncclInvalidArgument;
  const CallSize sz = call_size(coll, count, datatype);
  cbd_words(cbd_schedule(coll, sz.count, sz.eltSize, nRanks, nChannels, proto, (int64_t)stepBytes, nThreads), out);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRingChunkOf(size_t count, ncclDataType_t datatype, int nRanks, int nChannels,
                                         size_t slotBytes, int nThreads, size_t i, int64_t* out) {
  if (!out || type_size(datatype) < 1 || nRanks < 1 || nChannels < 1 || nChannels > kMaxChannels ||
      count == 0 || i >= count || slotBytes < 4096 || nThreads < 64)
    return ncclInvalidArgument;
  const int64_t esz = type_size(datatype);
  const CbdPlan p = cbd_schedule(kAllReduce, (int64_t)count, esz, nRanks, nChannels, kProtoSimple,
                                 (int64_t)slotBytes, nThreads);
  const CbdLite cbd{p.channelLo, p.channelHi, p.countLo, p.countMid, (int64_t)count};
  int k;
  int64_t end;
  out[0] = ar_chunk_of(cbd, p.chunkLo, nRanks, std::max<int64_t>(1, 16 / esz), (int64_t)i, &k, &end);
  out[1] = k;
  out[2] = end;
  return ncclSuccess;
}

// The group planner on explicit inputs.
static ncclResult_t group_plan_export(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                                      const int* ops, int nRanks, int nChannels, const PlanGeometry& geo,
                                      const AlgoPolicy* pol, int* algos, int* order, int* planOf, int64_t* cbd) {
  if (nCalls < 1 || !colls || !counts || !datatypes || !ops || !order || !planOf || !cbd || nRanks < 1 ||
      nChannels < 1 || nChannels > kMaxChannels || geo.stepBytes < 4096 || geo.nThreads < 64 ||
      geo.ll128StepBytes < 1920 * 16 || geo.ll128Threads < 64)
    return ncclInvalidArgument;
  std::vector<GroupTask> g;
  for (int i = 0; i < nCalls; i++) {
    const ncclDataType_t dt = (ncclDataType_t)datatypes[i];
    const int c = colls[i];
    if (c < kAllReduce || c > kReduce || type_size(dt) < 1 || counts[i] == 0) return ncclInvalidArgument;
    int devOp = OP_SUM;
    uint64_t arg = 0;
    if (!is_copy_coll(c)) NCCLCHECK(host_to_dev_redop((ncclRedOp_t)ops[i], dt, nRanks, &devOp, &arg));
    const int kt = kernel_type_of_call(c, devOp, dt);
    if (kt < 0) return ncclInvalidArgument;
    g.push_back(group_task_of(c, counts[i], dt, devOp, kt));
  }
  GroupPlanOut p;
  group_plan(g, nRanks, nChannels, geo, pol, &p);
  for (int i = 0; i < nCalls; i++) {
    order[i] = p.order[i];
    planOf[i] = p.planOf[i];
    if (algos) algos[i] = public_algo(p.algo[i]);
    cbd_words(p.cbd[i], cbd + 8 * (size_t)i);
  }
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclGroupPlan(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                                       const int* ops, int nRanks, int nChannels, size_t stepBytes, int nThreads,
                                       int* order, int* planOf, int64_t* cbd) {
  const PlanGeometry geo{(int64_t)stepBytes, nThreads, kDefaultLL128.stepBytes, kDefaultLL128.nThreads};
  return group_plan_export(nCalls, colls, counts, datatypes, ops, nRanks, nChannels, geo, nullptr, nullptr, order,
                           planOf, cbd);
}

VCCL_EXPORT ncclResult_t vcclGroupPlanEx(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                                         const int* ops, int nRanks, int nChannels, const int64_t* geometry,
                                         const int64_t* policy, int* algos, int* order, int* planOf,
                                         int64_t* cbd) {
  if (!geometry) return ncclInvalidArgument;
  const PlanGeometry geo{geometry[0], geometry[1], geometry[2], geometry[3]};
  AlgoPolicy pol;
  if (policy && !policy_of_words(policy, nRanks, &pol)) return ncclInvalidArgument;
  return group_plan_export(nCalls, colls, counts, datatypes, ops, nRanks, nChannels, geo, policy ? &pol : nullptr,
                           algos, order, planOf, cbd);
}

// The path every call of a group would take on this comm (its aggregate's, as
// launch_planned lays the group out); no launch.
VCCL_EXPORT ncclResult_t vcclCommGroupAlgos(ncclComm_t comm, int nCalls, const int* colls, const size_t* counts,
                                            const int* datatypes, const int* ops, int* algos) {
  NCCLCHECK(comm_check(comm, "vcclCommGroupAlgos"));
  if (nCalls < 1 || !algos) return ncclInvalidArgument;
  if (comm->nRanks == 1) {
    for (int i = 0; i < nCalls; i++) algos[i] = vcclAlgoOneRank;
    return ncclSuccess;
  }
  std::vector<int> order(nCalls), planOf(nCalls);
  std::vector<int64_t> cbd(8 * (size_t)nCalls);
  const AlgoPolicy pol = policy_of(comm);
  // without LL128 FIFOs no call takes the LL128 ring: its geometry is moot
  const bool ll128 = comm->ll128StepBytes > 0;
  const PlanGeometry geo{comm->stepBytes, comm->nThreads, ll128 ? comm->ll128StepBytes : kDefaultLL128.stepBytes,
                         ll128 ? comm->ll128Threads : kDefaultLL128.nThreads};
  return group_plan_export(nCalls, colls, counts, datatypes, ops, comm->nRanks, comm->nChannels, geo, &pol, algos,
                           order.data(), planOf.data(), cbd.data());
}

// The point-to-point planner on explicit inputs.
VCCL_EXPORT ncclResult_t vcclP2pPlan(int rank, int nRanks, int nCalls, const int* kinds, const int* peers,
                                     const size_t* bytes, const uint64_t* buffs, int parts, size_t minPartBytes,
                                     size_t stepBytes, int gMin, int gCap, int maxWorks, int cap, int* nItems,
                                     int* nWgs, int64_t* items) {
  if (nRanks < 1 || nRanks > kP2pMaxRanks || rank < 0 || rank >= nRanks || nCalls < 0 || (nCalls && (!kinds || !peers || !bytes)) ||
      parts < 1 || parts > kP2pMaxParts || minPartBytes < 256 || stepBytes < 4096 || stepBytes % 512 || maxWorks < 1 ||
      maxWorks > kP2pMaxWorks || !nItems || cap < 0 || (cap && !items))
    return ncclInvalidArgument;
  std::vector<P2pCall> calls;
  for (int i = 0; i < nCalls; i++) {
    if ((kinds[i] != kP2pCallSend && kinds[i] != kP2pCallRecv) || peers[i] < 0 || peers[i] >= nRanks)
      return ncclInvalidArgument;
    calls.push_back(P2pCall{kinds[i], peers[i], (int64_t)bytes[i], buffs ? buffs[i] : (uint64_t)(2 * i + 1)});
  }
  P2pPlanOut plan;
  NCCLCHECK(p2p_plan(rank, nRanks, calls, P2pGeometry{parts, (int64_t)minPartBytes, (int64_t)stepBytes}, gMin, gCap,
                     maxWorks, &plan));
  *nItems = (int)plan.items.size();
  if (nWgs) *nWgs = plan.nWgs;
  if ((int)plan.items.size() > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < plan.items.size(); k++) {
    const P2pItem& it = plan.items[k];
    const int64_t v[12] = {it.launch, it.wg, it.kind, it.sweep, it.round, it.part,
                           it.peer,   it.call, it.call2, it.offset, it.bytes, it.steps};
    for (int j = 0; j < 12; j++) items[12 * k + j] = v[j];
  }
  return ncclSuccess;
}

// select_algo on an explicit policy with the rooted LL and rooted direct
// thresholds as a comm would carry them (a negative one: from the environment).
static ncclResult_t rooted_algo(int coll, size_t count, ncclDataType_t datatype, int nRanks, const int64_t* policy,
                                int64_t threshold, int llAllowed, int anyNet, int64_t directThreshold,
                                int directAllowed, int64_t* effective, int64_t* directEffective, int* algo) {
  AlgoPolicy pol;
  if (!policy || !algo || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1 || nRanks < 1 ||
      nRanks > kMaxRanks || !policy_of_words(policy, nRanks, &pol) || policy[1] < 0)
    return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("LL_ROOTED_THRESHOLD", 0);
  if (directThreshold < 0) directThreshold = param_int("DIRECT_ROOTED_THRESHOLD", 0);
  pol.llRootedMax = ll_rooted_max(threshold, pol.llSlotBytes, llAllowed != 0, anyNet != 0, nRanks);
  pol.directRootedMax = direct_rooted_max(directThreshold, pol.direct, directAllowed != 0, anyNet != 0, nRanks);
  if (effective) *effective = (int64_t)pol.llRootedMax;
  if (directEffective) *directEffective = (int64_t)pol.directRootedMax;
  const CallSize sz = call_size(coll, count, datatype);
  *algo = public_algo(select_algo(pol, coll, sz.eltSize, sz.count));  // one rank: the ring, as select_algo says
  return ncclSuccess;
}

// The rooted direct threshold fixed at 0: this export predates it and never
// reads VCCL_DIRECT_ROOTED_THRESHOLD.
VCCL_EXPORT ncclResult_t vcclRootedAlgo(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                        const int64_t* policy, int64_t threshold, int llAllowed, int anyNet,
                                        int64_t* effective, int* algo) {
  return rooted_algo(coll, count, datatype, nRanks, policy, threshold, llAllowed, anyNet, 0, 0, effective, nullptr,
                     algo);
}

VCCL_EXPORT ncclResult_t vcclRootedAlgoEx(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                          const int64_t* policy, int64_t threshold, int llAllowed, int anyNet,
                                          int64_t directThreshold, int directAllowed, int64_t* effective,
                                          int64_t* directEffective, int* algo) {
  return rooted_algo(coll, count, datatype, nRanks, policy, threshold, llAllowed, anyNet, directThreshold,
                     directAllowed, effective, directEffective, algo);
}

// One rooted direct call's geometry and the steps of one chunk as `rank` runs it.
VCCL_EXPORT ncclResult_t vcclDirectRootedPlan(int coll, int nRanks, int rank, int root, size_t count,
                                              ncclDataType_t datatype, int64_t regionBytes, int chunk, int cap,
                                              int64_t* geometry, int* owners, int* nSteps, int64_t* steps) {
  if ((coll != kBroadcast && coll != kReduce) || nRanks < 2 || nRanks > kDirectMaxRanks || rank < 0 ||
      rank >= nRanks || root < 0 || root >= nRanks || type_size(datatype) < 1 || count == 0 ||
      count > (size_t)1 << 56 || regionBytes < 32 || regionBytes > (int64_t)1 << 40 || !geometry || !nSteps ||
      cap < 0 || (cap && !steps))
    return ncclInvalidArgument;
  const CallSize sz = call_size(coll, count, datatype);
  DirectRootedPlanOut out;
  NCCLCHECK(direct_rooted_plan(coll, nRanks, rank, root, sz.count, sz.eltSize, regionBytes, chunk, &out));
  geometry[0] = out.chunkElts;
  geometry[1] = out.nChunks;
  geometry[2] = out.shardElts;
  geometry[3] = (int64_t)out.owner.size();
  if (owners)
    for (size_t j = 0; j < out.owner.size(); j++) owners[j] = out.owner[j];
  *nSteps = (int)out.steps.size();
  if (*nSteps > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < out.steps.size(); k++) {
    const DirectStep& d = out.steps[k];
    const int64_t v[8] = {d.kind, d.phase, d.peer, d.region, d.regionOff, d.userOff, d.bytes, d.src};
    for (int j = 0; j < 8; j++) steps[8 * k + j] = v[j];
  }
  return ncclSuccess;
}

// The line layout of one rooted LL launch.
VCCL_EXPORT ncclResult_t vcclLLRootedPlan(int coll, int nRanks, int rank, int nParts, const int* roots,
                                          const size_t* bytes, int64_t linesPerSlot, int cap, int64_t* line0,
                                          int* nStores, int64_t* stores, int* nPolls, int64_t* polls) {
  if ((coll != kBroadcast && coll != kReduce) || nRanks < 2 || nRanks > kOrderMaxRanks || rank < 0 ||
      rank >= nRanks || nParts < 1 || nParts > kLLMaxParts || !roots || !bytes || linesPerSlot < 1 || cap < 0 ||
      !nStores || !nPolls || (cap && (!stores || !polls)))
    return ncclInvalidArgument;
  std::vector<int> r(roots, roots + nParts);
  std::vector<int64_t> b(nParts);
  for (int i = 0; i < nParts; i++) {
    if (r[i] < 0 || r[i] >= nRanks || bytes[i] > (size_t)linesPerSlot * 8) return ncclInvalidArgument;
    b[i] = (int64_t)bytes[i];
  }
  LLRootedPlanOut out;
  NCCLCHECK(ll_rooted_plan(coll, nRanks, rank, r, b, linesPerSlot, &out));
  *nStores = (int)out.stores.size();
  *nPolls = (int)out.polls.size();
  if (line0)
    for (int i = 0; i < nParts; i++) line0[i] = out.line0[i];
  if (*nStores > cap || *nPolls > cap) return ncclInvalidArgument;
  put_ranges(out.stores, stores);
  put_ranges(out.polls, polls);
  return ncclSuccess;
}

// A comm's VCCL_LL_A2A_THRESHOLD as it takes effect.
VCCL_EXPORT ncclResult_t vcclLLA2aMax(int64_t threshold, int64_t llSlotBytes, int llAllowed, int anyNet, int nRanks,
                                      int hasP2p, int64_t* effective) {
  if (!effective || llSlotBytes < 0 || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("LL_A2A_THRESHOLD", 0);
  *effective = (int64_t)ll_a2a_max(threshold, llSlotBytes, llAllowed != 0, anyNet != 0, nRanks, hasP2p != 0);
  return ncclSuccess;
}

// One all-to-all(v) call's split between the LL launch and the FIFO launch as
// `rank` runs it: a2a_plan with the direct path off.
VCCL_EXPORT ncclResult_t vcclLLA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* recvBytes,
                                       int uniform, int64_t llA2aMax, int64_t linesPerSlot, int* sendLL, int* recvLL,
                                       int* launch, int64_t* stores, int64_t* polls, int* nResSends, int* resSends,
                                       int* nResRecvs, int* resRecvs) {
  if (nRanks < 2 || nRanks > kOrderMaxRanks || rank < 0 || rank >= nRanks || !sendBytes || !recvBytes ||
      llA2aMax < 0 || linesPerSlot < 1 || llA2aMax > linesPerSlot * 8 || !sendLL || !recvLL || !launch || !stores ||
      !polls || !nResSends || !resSends || !nResRecvs || !resRecvs)
    return ncclInvalidArgument;
  int64_t sb[kOrderMaxRanks], rb[kOrderMaxRanks];
  if (!a2a_rows(nRanks, sendBytes, recvBytes, uniform, sb, rb)) return ncclInvalidArgument;
  A2aPlanOut out;
  NCCLCHECK(a2a_plan(nRanks, rank, sb, rb, uniform != 0, (uint64_t)llA2aMax, 0, linesPerSlot, 1, 1, 1, &out));
  *launch = out.llLaunch;
  for (int p = 0; p < nRanks; p++) sendLL[p] = out.sendPath[p] == kA2aLL, recvLL[p] = out.recvPath[p] == kA2aLL;
  put_ranges(out.stores, stores);  // nRanks - 1 ranges with a launch, else none
  put_ranges(out.polls, polls);
  put_residuals(out, nResSends, resSends, nResRecvs, resRecvs);
  return ncclSuccess;
}

// A comm's VCCL_DIRECT_A2A_THRESHOLD as it takes effect.
VCCL_EXPORT ncclResult_t vcclDirectA2aMax(int64_t threshold, int64_t regionBytes, int directAllowed, int anyNet,
                                          int nRanks, int hasP2p, int64_t* effective) {
  if (!effective || regionBytes < 0 || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("DIRECT_A2A_THRESHOLD", 0);
  *effective =
      (int64_t)direct_a2a_max(threshold, regionBytes, directAllowed != 0, anyNet != 0, nRanks, hasP2p != 0);
  return ncclSuccess;
}

// One all-to-all(v) call's three-way split between the LL launch, the direct
// launch and the FIFO launch as `rank` runs it.
VCCL_EXPORT ncclResult_t vcclDirectA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* recvBytes,
                                           int uniform, int64_t llA2aMax, int64_t directA2aMax, int64_t linesPerSlot,
                                           int minCTAs, int maxCTAs, int directMaxBlocks, int* sendPath,
                                           int* recvPath, int* llLaunch, int* directLaunch, int* nBlocks,
                                           int64_t* blkBytes, int* nResSends, int* resSends, int* nResRecvs,
                                           int* resRecvs) {
  if (nRanks < 2 || nRanks > kDirectMaxRanks || rank < 0 || rank >= nRanks || !sendBytes || !recvBytes ||
      llA2aMax < 0 || linesPerSlot < 0 || linesPerSlot > (int64_t)1 << 40 || llA2aMax > linesPerSlot * 8 ||
      directA2aMax < 0 || directA2aMax > (int64_t)1 << 40 || minCTAs < 0 || maxCTAs < 1 || directMaxBlocks < 1 ||
      !sendPath || !recvPath || !llLaunch || !directLaunch || !nBlocks || !blkBytes || !nResSends || !resSends ||
      !nResRecvs || !resRecvs)
    return ncclInvalidArgument;
  int64_t sb[kOrderMaxRanks], rb[kOrderMaxRanks];
  if (!a2a_rows(nRanks, sendBytes, recvBytes, uniform, sb, rb)) return ncclInvalidArgument;
  A2aPlanOut out;
  NCCLCHECK(a2a_plan(nRanks, rank, sb, rb, uniform != 0, (uint64_t)llA2aMax, (uint64_t)directA2aMax, linesPerSlot,
                     minCTAs, maxCTAs, directMaxBlocks, &out));
  *llLaunch = out.llLaunch;
  *directLaunch = out.directLaunch;
  *nBlocks = out.nBlocks;
  *blkBytes = out.blkBytes;
  for (int p = 0; p < nRanks; p++) sendPath[p] = out.sendPath[p], recvPath[p] = out.recvPath[p];
  put_residuals(out, nResSends, resSends, nResRecvs, resRecvs);
  return ncclSuccess;
}

// The all-to-all counters of a comm; `api` names the export in comm_check's warning.
static ncclResult_t a2a_stats(ncclComm_t comm, const char* api, unsigned long long* llLaunches,
                              unsigned long long* llPairs, unsigned long long* directLaunches,
                              unsigned long long* directPairs, unsigned long long* fifoPairs) {
  NCCLCHECK(comm_check(comm, api));
  if (llLaunches) *llLaunches = comm->a2aLLLaunches;
  if (llPairs) *llPairs = comm->a2aLLPairs;
  if (directLaunches) *directLaunches = comm->a2aDirectLaunches;
  if (directPairs) *directPairs = comm->a2aDirectPairs;
  if (fifoPairs) *fifoPairs = comm->a2aFifoPairs;
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t vcclCommA2aStats(ncclComm_t comm, unsigned long long* llLaunches, unsigned long long* llPairs,
                                          unsigned long long* fifoPairs) {
  return a2a_stats(comm, "vcclCommA2aStats", llLaunches, llPairs, nullptr, nullptr, fifoPairs);
}
VCCL_EXPORT ncclResult_t vcclCommA2aStatsEx(ncclComm_t comm, unsigned long long* llLaunches,
                                            unsigned long long* llPairs, unsigned long long* directLaunches,
                                            unsigned long long* directPairs, unsigned long long* fifoPairs) {
  return a2a_stats(comm, "vcclCommA2aStatsEx", llLaunches, llPairs, directLaunches, directPairs, fifoPairs);
}

// A tuning / measurement knob: every rank must call it alike, between calls.
VCCL_EXPORT ncclResult_t vcclCommSetA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetA2aThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  comm->llA2aMaxBytes = ll_a2a_max_of(*comm, bytes, comm->nRanks, comm->p2pOff == kP2pOffNet,
                                      comm->p2pConns != nullptr && comm->llBuf != nullptr &&
                                          (int)comm->llPeer.size() >= comm->nRanks);
  if (effective) *effective = (int64_t)comm->llA2aMaxBytes;
  return ncclSuccess;
}

// Likewise for the direct all-to-all.
VCCL_EXPORT ncclResult_t vcclCommSetDirectA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetDirectA2aThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  comm->directA2aMaxBytes = direct_a2a_max_of(*comm, bytes, comm->nRanks, comm->p2pOff == kP2pOffNet,
                                              comm->p2pConns != nullptr && comm->dPeers != nullptr);
  if (effective) *effective = (int64_t)comm->directA2aMaxBytes;
  return ncclSuccess;
}

// -------------------------------------------------------- registered buffers
// A comm's VCCL_REG_THRESHOLD as it takes effect (the registry bit of the init
// all-gather aside: this is the arithmetic).
VCCL_EXPORT ncclResult_t vcclRegMax(int64_t threshold, int inbox, int directAllowed, int anyNet, int nRanks,
                                    int64_t* effective) {
  if (!effective || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("REG_THRESHOLD", 0);
  *effective = (int64_t)reg_max(threshold, inbox != 0, directAllowed != 0, anyNet != 0, nRanks);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRegEligible(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                         int64_t effective, int groupCalls, int* eligible) {
  if (!eligible || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1 || nRanks < 1 || effective < 0 ||
      groupCalls < 0 || count > (size_t)1 << 56)
    return ncclInvalidArgument;
  *eligible = reg_eligible(coll, (int64_t)count, type_size(datatype), nRanks, (uint64_t)effective, groupCalls);
  return ncclSuccess;
}

// The ordered steps of one zero-copy launch as `rank` runs it on nBlocks workgroups.
VCCL_EXPORT ncclResult_t vcclRegPlan(int coll, size_t count, ncclDataType_t datatype, int nRanks, int rank,
                                     int nBlocks, int64_t* blkElts, int cap, int* nSteps, int64_t* steps) {
  if ((coll != kAllReduce && coll != kReduceScatter && coll != kAllGather) || nRanks < 2 ||
      nRanks > kDirectMaxRanks || rank < 0 || rank >= nRanks || type_size(datatype) < 1 || count == 0 ||
      count > (size_t)1 << 56 || nBlocks < 1 || nBlocks > kDirectMaxBlocks || !nSteps || cap < 0 || (cap && !steps))
    return ncclInvalidArgument;
  const CallSize sz = call_size(coll, count, datatype);
  RegPlanOut out;
  NCCLCHECK(reg_plan(coll, nRanks, rank, sz.count, sz.eltSize, nBlocks, &out));
  if (blkElts) *blkElts = out.blkElts;
  *nSteps = (int)out.steps.size();
  if (*nSteps > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < out.steps.size(); k++) {
    const RegStep& d = out.steps[k];
    const int64_t v[8] = {d.kind, d.epoch, d.phase, d.peer, d.buf, d.peerOff, d.ownOff, d.bytes};
    for (int j = 0; j < 8; j++) steps[8 * k + j] = v[j];
  }
  return ncclSuccess;
}

// The pure registration table on its own: no comm, no GPU.
struct vcclRegTable {
  RegTable t;
};
VCCL_EXPORT ncclResult_t vcclRegTableNew(vcclRegTable_t** table) {
  if (!table) return ncclInvalidArgument;
  *table = new vcclRegTable();
  reg_table_clear(&(*table)->t);
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t vcclRegTableInsert(vcclRegTable_t* table, uint64_t addr, size_t bytes, int* entry,
                                            uint32_t* generation) {
  if (!table || !entry) return ncclInvalidArgument;
  *entry = reg_insert(&table->t, addr, bytes);  // -1: full (or an empty range) — refused, not an error
  if (generation) *generation = *entry < 0 ? 0 : table->t.e[*entry].generation;
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t vcclRegTableFind(const vcclRegTable_t* table, uint64_t addr, size_t bytes, int* entry,
                                          uint64_t* offset, uint32_t* generation) {
  if (!table || !entry) return ncclInvalidArgument;
  uint64_t off = 0;
  *entry = reg_find(&table->t, addr, bytes, &off);
  if (offset) *offset = *entry < 0 ? 0 : off;
  if (generation) *generation = *entry < 0 ? 0 : table->t.e[*entry].generation;
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t vcclRegTableRemove(vcclRegTable_t* table, int entry) {
  if (!table || !reg_remove(&table->t, entry)) return ncclInvalidArgument;
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t vcclRegTableFree(vcclRegTable_t* table) {
  delete table;
  return ncclSuccess;
}

// Synchronises the device, then reads the three device-resident counters.
VCCL_EXPORT ncclResult_t vcclCommRegStats(ncclComm_t comm, unsigned long long* launches,
                                          unsigned long long* zeroCopy, unsigned long long* fallback,
                                          int* liveEntries, int* imported) {
  NCCLCHECK(comm_check(comm, "vcclCommRegStats"));
  unsigned long long w[3] = {0, 0, 0};
  if (comm->reg) {
    DeviceGuard dev(comm->device);
    HIPCHECK(dev.status);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(w, comm->reg->stats, sizeof(w), hipMemcpyDeviceToHost));
  }
  if (launches) *launches = w[0];
  if (zeroCopy) *zeroCopy = w[1];
  if (fallback) *fallback = w[2];
  if (liveEntries) *liveEntries = comm->reg ? reg_live_count(&comm->reg->table) : 0;
  if (imported) *imported = comm->reg ? reg_imported_count(comm) : 0;
  return ncclSuccess;
}

// A tuning / measurement knob: every rank must call it alike, outside a group.
// A comm initialised without a registry has none to switch on: 0 stays 0.
VCCL_EXPORT ncclResult_t vcclCommSetRegThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetRegThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  if (comm->reg)  // a registry exists only where no peer is behind the net proxy
    comm->reg->threshold = reg_max_of(*comm, bytes, comm->nRanks, false, comm->dPeers != nullptr);
  if (effective) *effective = comm->reg ? (int64_t)comm->reg->threshold : 0;
  return ncclSuccess;
}

// -------------------------------------- rooted collectives over registered buffers
// A comm's VCCL_REG_ROOTED_THRESHOLD as it takes effect (the arithmetic).
VCCL_EXPORT ncclResult_t vcclRegRootedMax(int64_t threshold, int inbox, int directAllowed, int anyNet, int nRanks,
                                          int allRegistries, int64_t* effective) {
  if (!effective || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("REG_ROOTED_THRESHOLD", 0);
  *effective = (int64_t)reg_rooted_max(threshold, inbox != 0, directAllowed != 0, anyNet != 0, nRanks,
                                       allRegistries != 0);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRegRootedEligible(int coll, size_t count, ncclDataType_t datatype, int64_t effective,
                                               int groupCalls, int* eligible) {
  if (!eligible || (coll != kBroadcast && coll != kReduce) || type_size(datatype) < 1 || effective < 0 ||
      groupCalls < 0 || count > (size_t)1 << 56)
    return ncclInvalidArgument;
  *eligible = reg_rooted_eligible(coll, (int64_t)count, type_size(datatype), (uint64_t)effective, groupCalls);
  return ncclSuccess;
}

// The ordered steps of one zero-copy broadcast / reduce launch as `rank` runs it on nBlocks workgroups.
VCCL_EXPORT ncclResult_t vcclRegRootedPlan(int coll, size_t count, ncclDataType_t datatype, int nRanks, int rank,
                                           int root, size_t regionBytes, int nBlocks, int64_t* blkElts,
                                           int64_t* chunkElts, int* nChunks, int cap, int* nSteps, int64_t* steps) {
  if ((coll != kBroadcast && coll != kReduce) || nRanks < 2 || nRanks > kDirectMaxRanks || rank < 0 ||
      rank >= nRanks || root < 0 || root >= nRanks || type_size(datatype) < 1 || count == 0 ||
      count > (size_t)1 << 56 || regionBytes < 32 || regionBytes > (size_t)1 << 40 || nBlocks < 1 ||
      nBlocks > kDirectMaxBlocks || !nSteps || cap < 0 || (cap && !steps))
    return ncclInvalidArgument;
  const CallSize sz = call_size(coll, count, datatype);
  RegRootedPlanOut out;
  NCCLCHECK(reg_rooted_plan(coll, nRanks, rank, root, sz.count, sz.eltSize, (int64_t)regionBytes, nBlocks, &out));
  if (blkElts) *blkElts = out.blkElts;
  if (chunkElts) *chunkElts = out.chunkElts;
  if (nChunks) *nChunks = out.nChunks;
  *nSteps = (int)out.steps.size();
  if (*nSteps > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < out.steps.size(); k++) {
    const RegStep& d = out.steps[k];
    const int64_t v[8] = {d.kind, d.epoch, d.phase, d.peer, d.buf, d.peerOff, d.ownOff, d.bytes};
    for (int j = 0; j < 8; j++) steps[8 * k + j] = v[j];
  }
  return ncclSuccess;
}

// Synchronises the device, then reads the three device-resident counters.
VCCL_EXPORT ncclResult_t vcclCommRegRootedStats(ncclComm_t comm, unsigned long long* launches,
                                                unsigned long long* zeroCopy, unsigned long long* fallback) {
  NCCLCHECK(comm_check(comm, "vcclCommRegRootedStats"));
  unsigned long long w[3] = {0, 0, 0};
  if (comm->reg && comm->reg->rootedStats) {
    DeviceGuard dev(comm->device);
    HIPCHECK(dev.status);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(w, comm->reg->rootedStats, sizeof(w), hipMemcpyDeviceToHost));
  }
  if (launches) *launches = w[0];
  if (zeroCopy) *zeroCopy = w[1];
  if (fallback) *fallback = w[2];
  return ncclSuccess;
}

// A tuning / measurement knob: every rank must call it alike, outside a group.
// A comm initialised without a registry has none to switch on: 0 stays 0.
VCCL_EXPORT ncclResult_t vcclCommSetRegRootedThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetRegRootedThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  if (comm->reg) {  // a registry exists only where every rank has one and no peer is behind the net proxy
    const size_t eff = reg_rooted_max_of(*comm, bytes, comm->nRanks, false, comm->dPeers != nullptr, true);
    if (eff > 0) NCCLCHECK(reg_rooted_alloc(comm));
    comm->regRootedMaxBytes = eff;
  }
  if (effective) *effective = (int64_t)comm->regRootedMaxBytes;
  return ncclSuccess;
}

// ------------------------------------------- all-to-all over registered buffers
// A comm's VCCL_REG_A2A_THRESHOLD as it takes effect (the arithmetic).
VCCL_EXPORT ncclResult_t vcclRegA2aMax(int64_t threshold, int inbox, int directAllowed, int anyNet, int nRanks,
                                       int hasP2p, int allRegistries, int64_t* effective) {
  if (!effective || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("REG_A2A_THRESHOLD", 0);
  *effective = (int64_t)reg_a2a_max(threshold, inbox != 0, directAllowed != 0, anyNet != 0, nRanks, hasP2p != 0,
                                    allRegistries != 0);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRegA2aEligible(int uniform, size_t pairBytes, int64_t effective, int index,
                                            int* eligible) {
  if (!eligible || effective < 0 || index < 0 || pairBytes > (size_t)1 << 60) return ncclInvalidArgument;
  *eligible = reg_a2a_eligible(uniform != 0, (int64_t)pairBytes, (uint64_t)effective, index);
  return ncclSuccess;
}

// The ordered steps of one zero-copy all-to-all launch as `rank` runs it.
VCCL_EXPORT ncclResult_t vcclRegA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* sendOff,
                                        const size_t* recvOff, int uniform, int minCTAs, int maxCTAs,
                                        int directMaxBlocks, int* nBlocks, int cap, int* nSteps, int64_t* steps) {
  if (nRanks < 2 || nRanks > kDirectMaxRanks || rank < 0 || rank >= nRanks || !sendBytes || !sendOff || !recvOff ||
      minCTAs < 0 || maxCTAs < 1 || directMaxBlocks < 1 || !nBlocks || !nSteps || cap < 0 || (cap && !steps))
    return ncclInvalidArgument;
  const int n = nRanks;
  std::vector<int64_t> sb((size_t)n * n), so((size_t)n * n), ro(n);
  for (int i = 0; i < n * n; i++) {
    if (sendBytes[i] > (size_t)1 << 56 || sendOff[i] > (size_t)1 << 56) return ncclInvalidArgument;
    if (uniform && sendBytes[i] != sendBytes[0]) return ncclInvalidArgument;
    sb[i] = (int64_t)sendBytes[i];
    so[i] = (int64_t)sendOff[i];
  }
  for (int p = 0; p < n; p++) {
    if (recvOff[p] > (size_t)1 << 56) return ncclInvalidArgument;
    ro[p] = (int64_t)recvOff[p];
  }
  RegA2aPlanOut out;
  NCCLCHECK(reg_a2a_plan(n, rank, sb.data(), so.data(), ro.data(), uniform != 0, minCTAs, maxCTAs, directMaxBlocks,
                         &out));
  *nBlocks = out.nBlocks;
  *nSteps = (int)out.steps.size();
  if (*nSteps > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < out.steps.size(); k++) {
    const RegA2aStep& d = out.steps[k];
    const int64_t v[8] = {d.kind, d.epoch, d.phase, d.peer, d.peerOff, d.ownOff, d.bytes, d.blkBytes};
    for (int j = 0; j < 8; j++) steps[8 * k + j] = v[j];
  }
  return ncclSuccess;
}

// Synchronises the device, then reads the three device-resident counters.
VCCL_EXPORT ncclResult_t vcclCommRegA2aStats(ncclComm_t comm, unsigned long long* launches,
                                             unsigned long long* zeroCopy, unsigned long long* fallback) {
  NCCLCHECK(comm_check(comm, "vcclCommRegA2aStats"));
  unsigned long long w[3] = {0, 0, 0};
  if (comm->reg && comm->reg->a2aDev) {
    DeviceGuard dev(comm->device);
    HIPCHECK(dev.status);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(w, &comm->reg->a2aDev->stats, sizeof(w), hipMemcpyDeviceToHost));
  }
  if (launches) *launches = w[0];
  if (zeroCopy) *zeroCopy = w[1];
  if (fallback) *fallback = w[2];
  return ncclSuccess;
}

// A tuning / measurement knob: every rank must call it alike, outside a group.
// A comm initialised without a registry has none to switch on: 0 stays 0.
VCCL_EXPORT ncclResult_t vcclCommSetRegA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetRegA2aThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  if (comm->reg) {  // a registry exists only where every rank has one and no peer is behind the net proxy
    const size_t eff = reg_a2a_max_of(*comm, bytes, comm->nRanks, false, comm->dPeers != nullptr,
                                      comm->p2pConns != nullptr, true);
    if (eff > 0) NCCLCHECK(reg_a2a_alloc(comm));
    comm->regA2aMaxBytes = eff;
  }
  if (effective) *effective = (int64_t)comm->regA2aMaxBytes;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclCommSetAlgo(ncclComm_t comm, int algo) {
  NCCLCHECK(comm_check(comm, "vcclCommSetAlgo"));
  const int a = internal_algo(algo);
  if (algo != -1 && a < 0) return ncclInvalidArgument;
  // algoForce (core.h): 0 automatic, else 1 + the path; forced LL128 without
  // its buffers runs the SIMPLE ring (select_algo)
  comm->algoForce = algo == -1 ? 0 : a + 1;
  return ncclSuccess;
}

// Copies the ring trace off the device (and clears it).
VCCL_EXPORT ncclResult_t vcclCommRingTrace(ncclComm_t comm, void* hostBuf, size_t bytes, int* nChannels,
                                           int* cap) {
  NCCLCHECK(comm_check(comm, "vcclCommRingTrace"));
  if (nChannels) *nChannels = comm->nChannels;
  if (cap) *cap = comm->ringTraceCap;
  if (!comm->ringTrace) return ncclInvalidUsage;
  const size_t need = (size_t)comm->nChannels * comm->ringTraceCap * sizeof(RingTraceRec);
  if (!hostBuf || bytes < need) return ncclInvalidArgument;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  const hipError_t e = hipMemcpy(hostBuf, comm->ringTrace, need, hipMemcpyDeviceToHost);
  if (e == hipSuccess) (void)hipMemset(comm->ringTrace, 0, need);
  return e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

VCCL_EXPORT ncclResult_t vcclCommLaunchStats(ncclComm_t comm, unsigned long long* collectives,
                                             unsigned long long* fusedLaunches) {
  NCCLCHECK(comm_check(comm, "vcclCommLaunchStats"));
  if (collectives) *collectives = comm->opCount;
  if (fusedLaunches) *fusedLaunches = comm->fusedLaunches;
  return ncclSuccess;
}
