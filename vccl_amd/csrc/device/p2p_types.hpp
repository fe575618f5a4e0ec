// Host/device-shared layout of the point-to-point transport (POD, no HIP
// types): ncclSend / ncclRecv and the all-to-alls built on them.
//
// A connection is (sender, receiver, part): a FIFO of kSteps slots in the
// RECEIVER's uncached memory and two flags of one kFlagStride line each — the
// tail in the receiver's memory, written by the sender (slots posted), the
// head in the sender's memory, written by the receiver (slots consumed).  The
// ring's credit scheme (ring_types.hpp) per pair instead of per ring edge.
//
//   receive buffer of a rank: [sender rank][part][kSteps slots][slot stride]
//   flag block of a rank:     [peer][part][0 tail of peer -> me | 1 head of me -> peer]
//
// Slots are written and read at offset 0 and keep the ring's stride
// (slot_stride: the step plus kSlotPad), so the ring's hand-off (ring.hpp
// prim_wg) addresses them unchanged.
#pragma once
#include <stdint.h>

#include "ring_types.hpp"

namespace vccl {

constexpr int kP2pMaxRanks = 8;   // per-peer FIFOs: one node's full mesh
constexpr int kP2pMaxParts = 8;   // connections per ordered pair (VCCL_P2P_PARTS)
constexpr int kP2pMaxConns = kP2pMaxRanks * kP2pMaxParts;
constexpr int kP2pThreads = 512;  // threads per workgroup (the ring's launch bound)

// One entry per (peer, part), index peer * parts + part, device-resident.
// The step counters persist across launches: the workgroup that drives a
// connection's direction reads its counter at kernel start and writes it back
// at kernel end, as DevChannel::recvStep / sendStep are — no host-side
// per-call state, so captured launches replay correctly.
struct P2pConn {
  // send side: data goes to the PEER's memory
  char* sendFifo;             // peer's buffer [me][part] (remote)
  uint64_t* nextRecvTail;     // peer's tail of me -> peer (remote)
  uint64_t* sendHead;         // local: slots the peer consumed
  // receive side: data arrives in MY memory
  char* recvFifo;             // my buffer [peer][part] (local)
  uint64_t* recvTail;         // local: slots the peer posted
  uint64_t* prevSendHead;     // peer's head of peer -> me (remote)
  uint64_t sendStep;
  uint64_t recvStep;
};

enum : int { kP2pSend = 0, kP2pRecv = 1, kP2pCopy = 2 };

// One work item: `bytes` of one part of one message (or of a self copy).
//   send: a = user source;  recv: b = user destination;  copy: a -> b.
struct P2pWork {
  const char* a;
  char* b;
  int64_t bytes;
  int16_t conn;  // peer * parts + part (unused by a copy)
  int16_t wg;    // the workgroup that runs it
  int8_t kind;   // kP2pSend / kP2pRecv / kP2pCopy
  int8_t skip;   // 1 .. 8: dropped when P2pBatch::skip[skip - 1] == 1; 0: never
  int8_t pad[2];
};
static_assert(sizeof(P2pWork) == 32, "work item layout");

// A launch's work list, in increasing (sweep, round, part) order; workgroup
// g runs the items with wg == g in list order.  Workgroups [0, nSendWgs) send
// (and run the self copies), the rest receive.  By-value kernel argument: at
// most 4 KiB.
constexpr int kP2pMaxWorks = 120;
struct P2pBatch {
  DevComm* comm;     // device-resident
  P2pConn* conns;    // device-resident, nRanks * parts entries (null at one rank)
  // The verdicts of the group's zero-copy all-to-alls (device-resident, written
  // by the launches ahead of this one on the stream; direct_reg.hpp
  // direct_reg_alltoall): word i == 1 means call i + 1 moved its bytes itself
  // and its items here are dropped — on every rank alike, so both ends drop the
  // same matched messages.  Null: nothing is ever dropped.
  const uint32_t* skip;
  int nWorks;
  int nConns;
  int stepBytes;
  int nSendWgs;
  P2pWork works[kP2pMaxWorks];
};
static_assert(sizeof(P2pBatch) <= 4096, "kernel-argument budget");

}  // namespace vccl
