// A group's sends, recvs and all-to-alls of one comm -> work descriptors -> launches of the p2p kernel and of
// the LL, direct and zero-copy all-to-all kernels (launch.cc launch_group calls launch_comm_p2p per comm).
#include <algorithm>

#include "../device/p2p_launch.hpp"
#include "../device/ring_launch.hpp"
#include "launch.h"
#include "order.h"
#include "regcomm.h"

namespace vccl {

// ------------------------------------------------------------ point-to-point
static_assert(kP2pSend == 0 && kP2pRecv == 1 && kP2pCopy == 2 && kP2pLLSend == 3 && kP2pLLRecv == 4,
              "P2pItem::kind is the device's work kind");

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

// The sends and recvs of one comm's group (call order), as 1 .. launches of the p2p kernel on the first task's
// stream, the other tasks' streams joined around them (OrderScope).
static ncclResult_t launch_p2p(const std::vector<Task>& ts) {
  ncclComm* comm = ts[0].comm;
  const hipStream_t s0 = ts[0].stream;
  const int n = comm->nRanks;
  const bool conns = comm->p2pConns != nullptr;
  // LL messages only on a comm that has the LL FIFOs (VCCL_P2P_LL_THRESHOLD at init)
  const bool ll = conns && comm->p2pLLConns != nullptr && comm->p2pLLMaxBytes > 0;
  const P2pGeometry geo{conns ? comm->p2pParts : 1, conns ? comm->p2pMinPartBytes : (int64_t)64 << 10,
                        conns ? comm->p2pStepBytes : 512 << 10, ll ? (int64_t)comm->p2pLLMaxBytes : 0,
                        ll ? comm->p2pLLStepBytes : 0};
  std::vector<P2pCall> calls;
  for (const Task& t : ts) {
    const bool send = t.coll == kTaskSend;
    calls.push_back(P2pCall{send ? kP2pCallSend : kP2pCallRecv, t.root, (int64_t)t.count * type_size(t.datatype),
                            (uint64_t)(uintptr_t)(send ? t.sendbuff : (const void*)t.recvbuff)});
    // as planned (a self pair is a copy; a zero-copy all-to-all may still drop its items on the device)
    (t.root != comm->rank && p2p_is_ll(calls.back().bytes, geo) ? comm->p2pLLMessages : comm->p2pFifoMessages)++;
  }
  comm->opCount += ts.size();  // whatever the outcome
  // The grid (invariant I4): every rank's send and receive workgroups are resident at once — the CTA floor first,
  // then the caps, as ll_grid and direct_blk_elts apply them.
  int gCap = std::max(1, comm->maxCTAs / 2);
  if (comm->shareBlockCap > 0) gCap = std::max(1, std::min(gCap, comm->shareBlockCap / 2));
  P2pPlanOut plan;
  NCCLCHECK(check_self_pairs(comm, ts));  // the one refusal p2p_plan has
  NCCLCHECK(p2p_plan(comm->rank, n, calls, geo, (comm->minCTAs + 1) / 2, gCap, kP2pMaxWorks, &plan));
  if (plan.items.empty()) return ncclSuccess;  // zero-byte messages and in-place self pairs only
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  OrderScope order(comm, s0);
  for (const Task& t : ts) order.join(t.stream);
  ncclResult_t r = order.begin();
  // the verdicts of the zero-copy all-to-alls launched ahead of this (launch_comm_p2p)
  const bool anySkip = std::any_of(ts.begin(), ts.end(), [](const Task& t) { return t.skip > 0; });
  if (anySkip && (!comm->reg || !comm->reg->a2aDev)) return ncclInternalError;
  for (size_t k = 0; k < plan.items.size() && r == ncclSuccess;) {
    P2pBatch b{};
    b.comm = comm->devComm;
    b.conns = comm->p2pConns;
    b.skip = anySkip ? comm->reg->a2aDev->skip : nullptr;
    b.nConns = conns ? n * geo.parts : 0;
    b.stepBytes = (int)geo.stepBytes;
    b.nSendWgs = plan.nWgs;
    if (ll) {
      b.llConns = comm->p2pLLConns;
      b.nLLConns = n;
      b.llStepLines = comm->p2pLLStepBytes / 8;
    }
    const int launch = plan.items[k].launch;
    for (; k < plan.items.size() && plan.items[k].launch == launch; k++) {
      const P2pItem& it = plan.items[k];
      if (b.nWorks >= kP2pMaxWorks || (it.kind != kP2pCopy && (!conns || it.peer == comm->rank)))
        return ncclInternalError;
      P2pWork& w = b.works[b.nWorks++];
      w.kind = (int8_t)it.kind;
      w.wg = (int16_t)it.wg;
      const bool llItem = it.kind == kP2pLLSend || it.kind == kP2pLLRecv;
      if (llItem && !ll) return ncclInternalError;
      w.conn = (int16_t)(llItem ? it.peer : it.peer * geo.parts + it.part);
      w.bytes = it.bytes;
      w.skip = (int8_t)ts[it.call].skip;  // a copy: its send's, which is its recv's
      if (it.kind != kP2pRecv && it.kind != kP2pLLRecv) w.a = (const char*)ts[it.call].sendbuff + it.offset;
      if (it.kind != kP2pSend && it.kind != kP2pLLSend)
        w.b = (char*)ts[it.kind == kP2pCopy ? it.call2 : it.call].recvbuff + it.offset;
    }
    r = order.ran(launch_result(p2p_launch(b, 2 * plan.nWgs, s0, order.stop()), "p2p"));
  }
  return order.end(r);
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

// The LL launch of one ncclAllToAll(v) (ll.hpp ll_alltoall) on the call's stream, ordered against the comm's other
// launches like a call outside a group (launch_task).  The tables go in rotated to this rank, the LL pairs' lines
// flattened in that order.  Plain ncclSend / ncclRecv never come here: they are not collective — a peer outside the
// exchange launches nothing, so the arrival barrier the slot reuse rests on (ll.hpp header) would not hold.
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
  OrderScope order(comm, t.stream);
  ncclResult_t r = order.begin();
  if (r == ncclSuccess) r = order.ran(launch_result(ll_a2a_launch(w, grid, t.stream, order.stop()), "LL all-to-all"));
  return order.end(r);
}

// The direct launch of one ncclAllToAll(v) (direct.hpp direct_alltoall) on the call's stream, ordered against the
// comm's other launches exactly like launch_ll_a2a.  The table goes in rotated to this rank; the grid is the plan's
// nBlocks, already under the co-residency caps the other direct kernels take (directMaxBlocks, which ranks sharing a
// GPU lower; kDirectMaxBlocks).
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
  OrderScope order(comm, t.stream);
  ncclResult_t r = order.begin();
  if (r == ncclSuccess) r = order.ran(launch_result(direct_a2a_launch(w, t.stream, order.stop()), "direct all-to-all"));
  return order.end(r);
}

// The zero-copy launch of one eligible ncclAllToAll(v) (direct_reg.hpp direct_reg_alltoall; plan.cc reg_a2a_plan is
// its step list) on the call's stream, ordered like launch_direct_a2a, the import table brought up to date first as
// launch_direct_reg does.  The grid is comm-wide (reg_a2a_blocks); the slices are the reader's own (reg_a2a_blk per
// receive block).  The descriptors are this rank's registrations of each block it sends, as of now.  selfPaired: the
// call's self send and self recv are each other's match in the group's sweep order — rank-local, so it enters the
// vote, not the eligibility.
static ncclResult_t launch_reg_a2a(const Task& t, int skipIdx, bool selfPaired) {
  ncclComm* comm = t.comm;
  const int n = comm->nRanks, me = comm->rank;
  const A2aArgs& a = *t.a2a;
  if (n > kDirectMaxRanks || !comm->dPeers || !comm->reg || !comm->reg->a2aDev || skipIdx < 0 ||
      skipIdx >= kRegA2aMaxCalls)
    return ncclInternalError;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  OrderScope order(comm, t.stream);
  NCCLCHECK(order.begin());
  NCCLCHECK(reg_refresh(comm, order.capture().active));
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
  return order.end(order.ran(launch_result(direct_reg_a2a_launch(w, t.stream, order.stop()), "zero-copy all-to-all")));
}

// One comm's sends, recvs and all-to-all tasks of a group (call order): each all-to-all's LL launch, then its direct
// launch, in call order, then the one p2p launch with the plain sends and recvs and the all-to-alls' residual pairs,
// in call order per peer — so matching by sweep is what it was.  An all-to-all eligible for the zero-copy path
// (reg_a2a_eligible) launches that kernel instead of the LL and direct ones, and ALL its pairs, the self copy
// included, join the p2p launch predicated on its verdict: the host cannot know whether the kernel moved them.
ncclResult_t launch_comm_p2p(const std::vector<Task>& mine) {
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

}  // namespace vccl
