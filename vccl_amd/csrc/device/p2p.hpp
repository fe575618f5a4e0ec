// Point-to-point kernel for gfx950: ncclSend / ncclRecv (and the all-to-alls
// grouped from them) over per-peer FIFOs in the receiver's uncached memory.
//
// The reference runs p2p as send / recv primitives of its SIMPLE protocol on
// per-peer connections (sendrecv.h runSend / runRecv over prims_simple.h).
// Here a launch carries a work list (P2pBatch, p2p_types.hpp); workgroups are
// direction-split — [0, nSendWgs) send, the rest receive — so a send never
// waits on its own rank's receive work.  Each workgroup runs its items in
// list order, and every connection direction belongs to one workgroup for the
// whole launch (the planner's invariants I1 / I2, host/plan.h).
//
// A step is the ring's slot hand-off unchanged (ring.hpp prim_wg): the sender
// waits for credit, copies user source -> peer slot (source nontemporal, slot
// stores sc0 sc1), every wave drains, a barrier, one thread stores the tail;
// the receiver waits for the tail, copies slot -> user destination with
// sc0 sc1 loads, drains, a barrier, one thread stores the head.  Its bounded
// spins (abort word, spin timeout, kErrSpinTimeout) and its VCCL_FENCES
// branches come with it.  Slots are used from offset 0, so only the user
// pointer's own misalignment reaches the engine's realigning path, on each
// side independently.
#pragma once
#include "p2p_types.hpp"
#include "ring.hpp"

namespace vccl {

template <int UNROLL>
__device__ __forceinline__ void p2p_run(const P2pBatch& b) {
  using Fn = FnCopy<uint8_t>;
  const Fn fn(0);
  __shared__ WaveSync ws;
  __shared__ uint64_t shStep[kP2pMaxConns];   // this direction's counters
  __shared__ uint64_t shDirty;                // connections this workgroup advanced
  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  const bool sendWg = wg < b.nSendWgs;
  if (tid == 0) {
    for (int i = 0; i < kSyncDepth; i++) ws.done[i] = 0;
    ws.tail = ws.head = 0;
    ws.abort = 0;
    ws.poller = 0;
    shDirty = 0;
  }
  if (tid < b.nConns && tid < kP2pMaxConns) shStep[tid] = sendWg ? b.conns[tid].sendStep : b.conns[tid].recvStep;
  const DevComm* m = b.comm;
  RingCtx r;
  r.ch = nullptr;
  r.comm = m;
  r.tid = tid;
  r.nthreads = blockDim.x;
  r.slotBytes = b.stepBytes;
  r.ll128Slot = 0;
  r.ws = (VCCL_LDS WaveSync*)&ws;
  r.shAbort = &r.ws->abort;
  r.trace = nullptr;
  r.traceN = 0;
  r.traceCap = 0;
  r.recvFifo = r.sendFifo = nullptr;
  r.recvTail = r.sendHead = nullptr;
  r.nextRecvTail = r.prevSendHead = nullptr;
  r.sendSizes = nullptr;
  r.recvSizes = nullptr;
  r.ll128Recv = r.ll128Send = nullptr;
  r.ringPos = 0;
  r.ringRanks = nullptr;
  r.abortFlag = m->abortFlag;
  r.errorFlag = m->errorFlag;
  r.spinTimeout = m->spinTimeoutTicks;
  r.useFences = m->useFences;
  r.pollMode = m->pollMode;
  r.waveMin = 0;
  r.lane = tid & 63;
  r.nWaves = (int)(blockDim.x >> 6);
  r.seq = 0;
  r.pend = false;
  r.recvStep = r.sendStep = 0;
  __syncthreads();

  for (int i = 0; i < b.nWorks; i++) {
    const P2pWork& w = b.works[i];
    if (w.wg != wg) continue;
    // An item of a zero-copy all-to-all that settled on D = 1 (P2pBatch::skip):
    // dropped before its connection's counter is touched.  The word was
    // written by an earlier launch and is the same on both ends of the message;
    // the branch is uniform, and never taken with a null pointer or index 0.
    if (w.skip > 0 && b.skip && __hip_atomic_load(b.skip + (w.skip - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      continue;
    if (w.kind == kP2pCopy) {
      // self traffic: a plain copy, no connection
      RCArgs a;
      a.srcs[0] = w.a;
      a.dsts[0] = w.b;
      a.nSrcs = a.nDsts = 1;
      a.preOpSrcs = 0;
      a.postOp = 0;
      reduce_copy<Fn, 1, 1, UNROLL, uniform_pol(kNT, kNT), 0, true>(fn, a, w.bytes, 0, 1, tid, r.nthreads);
      continue;
    }
    if (r.aborted()) break;
    const int ci = w.conn;
    const P2pConn& c = b.conns[ci];
    const int64_t step = b.stepBytes;
    if (w.kind == kP2pSend) {
      r.sendFifo = c.sendFifo;
      r.sendHead = uniform_ptr(c.sendHead);
      r.nextRecvTail = c.nextRecvTail;
      r.sendStep = shStep[ci];
      for (int64_t o = 0; o < w.bytes; o += step) {
        const int64_t len = w.bytes - o < step ? w.bytes - o : step;
        r.template prim_wg<Fn, false, true, true, false, UNROLL>(fn, w.a + o, nullptr, len, false);
      }
    } else {
      r.recvFifo = c.recvFifo;
      r.recvTail = uniform_ptr(c.recvTail);
      r.prevSendHead = c.prevSendHead;
      r.recvStep = shStep[ci];
      for (int64_t o = 0; o < w.bytes; o += step) {
        const int64_t len = w.bytes - o < step ? w.bytes - o : step;
        r.template prim_wg<Fn, true, false, false, true, UNROLL>(fn, nullptr, w.b + o, len, false);
      }
    }
    // the connection's counter for its next item in this launch (every
    // thread read the old one before the item's first barrier)
    if (tid == 0) {
      shStep[ci] = w.kind == kP2pSend ? r.sendStep : r.recvStep;
      shDirty |= 1ull << ci;
    }
    __syncthreads();
  }
  __syncthreads();
  // An aborted step leaves its counter where the step began, as the ring does.
  if (tid < b.nConns && tid < kP2pMaxConns && ((shDirty >> tid) & 1)) {
    if (sendWg) b.conns[tid].sendStep = shStep[tid];
    else b.conns[tid].recvStep = shStep[tid];
  }
}

}  // namespace vccl
