// A communicator's setup as arithmetic (setup.cc): the channel count, FIFO
// geometry, path thresholds and buffer sizes from (nRanks, CTA bounds) and the
// environment; what the exchanged peer identities switch off or cap; the ring
// tables of a rank.  No runtime call, no communicator, no stream — init.cc
// applies the results, vcclCommSetup (vccl_ext.h) shows them to the CPU tests.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/nccl.h"
#include "../device/p2p_types.hpp"
#include "../device/ring_types.hpp"

namespace vccl {

// Ring orders for one node: for n in {2,4,8} the
// arc-balanced ring sets over the fully connected xGMI mesh; Walecki's rings
// for odd n, two Hamiltonian cycles both ways for 6; otherwise the
// identity ring.  Returns the list of rings (each a permutation of 0..n-1).
std::vector<std::vector<int>> ring_orders(int nranks);
// NCCL_ALGO / NCCL_PROTO lists -> the forced path and the allowed ones
// (vcclAlgoSelection, vccl_ext.h).
ncclResult_t algo_proto_select(const char* algo, const char* proto, int* force, int* allowed);

#pragma GCC visibility push(hidden)  // internal: the library's exported symbols stay as they were

// The fields of ncclComm (core.h, which derives from this) that the setup
// decides.  vcclCommSetup reports them in this order.
struct CommSetup {
  int nChannels = 0;
  int stepBytes = 0;  // VCCL's FIFO step: the partition / chunk unit (slotBytes = the FIFO slot)
  int slotBytes = 0;
  int nThreads = 0;
  int algoForce = 0;     // NCCL_ALGO/NCCL_PROTO: 0 auto, 1 ring/SIMPLE, 2 tree/LL, 3 direct, 4 LL128 ring
  int algoAllowed = 15;  // paths the NCCL_ALGO / NCCL_PROTO lists leave (algo_proto_select)
  size_t llMaxBytes = 0;      // largest all-reduce carried by LL
  int llLines = 0;            // lines per (parity, source) slot = llMaxBytes / 8
  size_t llRsAgMaxBytes = 0;  // largest RS / AG bucket (n blocks) on the one-hop LL path
  size_t directMaxBytes = 0;      // largest all-reduce carried by the direct path
  size_t directRsAgMaxBytes = 0;  // largest RS / AG bucket on the one-hop direct path
  int directMaxBlocks = 0;
  int64_t dRegionBytes = 0;
  // VCCL's LL128 partition and chunk (ll128ChunkBytes of data per step,
  // enqueue.cc:2027-2032) and thread count (NCCL_LL128_NTHREADS,
  // tuning.cc:198-211) for the channel tuning.
  int64_t ll128StepBytes = 0;  // NCCL_LL128_BUFFSIZE / NCCL_STEPS (init.cc:617-633)
  int ll128Threads = 640;
  int64_t ll128SlotBytes = 0;
  size_t ll128MinBytes = 0, ll128MaxBytes = 0;  // automatic LL128 window (0 = off)
  int shareBlockCap = 0;  // ranks sharing a GPU: workgroups per launch that stay co-resident (0 = no cap)
  // Point-to-point connections (device/p2p_types.hpp; not part of what
  // vcclCommSetup reports): parts per ordered pair (VCCL_P2P_PARTS), the step
  // (NCCL_P2P_NVL_CHUNKSIZE, init.cc:626), the smallest message a second part
  // is opened for (VCCL_P2P_MIN_PART_BYTES).  p2pOff: why the comm has none
  // (kP2pOff*), 0 when it has them.
  int p2pParts = 0;
  int p2pStepBytes = 0;
  int64_t p2pMinPartBytes = 0;
  int p2pOff = 0;
  // Largest ncclBroadcast / ncclReduce on the one-hop LL path
  // (VCCL_LL_ROOTED_THRESHOLD, plan.h ll_rooted_max; default 0 = off; not part
  // of what vcclCommSetup reports)
  size_t llRootedMaxBytes = 0;
  // Largest ordered pair of an ncclAllToAll(v) on the one-hop LL path
  // (VCCL_LL_A2A_THRESHOLD, plan.h ll_a2a_max; default 0 = off; not part of
  // what vcclCommSetup reports either)
  size_t llA2aMaxBytes = 0;
  // Largest ncclBroadcast / ncclReduce on the two-hop direct path
  // (VCCL_DIRECT_ROOTED_THRESHOLD, plan.h direct_rooted_max; default 0 = off;
  // not part of what vcclCommSetup reports either)
  size_t directRootedMaxBytes = 0;
  // Largest ordered pair of an ncclAllToAll(v) on the one-hop direct path
  // (VCCL_DIRECT_A2A_THRESHOLD, plan.h direct_a2a_max; default 0 = off; not
  // part of what vcclCommSetup reports either)
  size_t directA2aMaxBytes = 0;
};
enum { kP2pOn = 0, kP2pOffEnv = 1, kP2pOffRanks = 2, kP2pOffNet = 3 };

// Bytes of the buffers a rank allocates (0 = none).  Sized for the channel
// count before the net or shared-GPU caps; the LL buffer and the inbox exist
// even when NCCL_ALGO / NCCL_PROTO drop their path from the automatic choice
// (vcclCommSetAlgo may still pick it).
struct SetupSizes {
  size_t fifoBytes = 0, flagBytes = 0, llBytes = 0, inboxBytes = 0, ll128Bytes = 0;
  bool wantLL128 = false;
  size_t p2pBytes = 0, p2pFlagBytes = 0;  // the p2p receive buffer and flag block
};
// Everything one rank decides on its own, in the order the knobs have always
// been read.  nChannels is 0 and nothing is sized at nRanks == 1.  Fails
// with algo_proto_select's result.
ncclResult_t setup_local(int nRanks, int minCTAs, int maxCTAs, CommSetup* s, SetupSizes* z);

// CommSetup::llA2aMaxBytes for a VCCL_LL_A2A_THRESHOLD of `threshold` on a comm
// whose other fields are decided (setup_local; vcclCommSetA2aThreshold).
size_t ll_a2a_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool hasP2p);
// CommSetup::directA2aMaxBytes for a VCCL_DIRECT_A2A_THRESHOLD of `threshold`,
// likewise (setup_local; vcclCommSetDirectA2aThreshold).
size_t direct_a2a_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool hasP2p);

// A comm's VCCL_REG_THRESHOLD of `threshold` as it takes effect (plan.h
// reg_max; inbox: every peer's inbox and direct flags are mapped).
size_t reg_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool inbox);
// A comm's VCCL_REG_A2A_THRESHOLD likewise (plan.h reg_a2a_max; hasP2p: the
// comm has point-to-point connections; allRegistries: every rank created its
// registry).
size_t reg_a2a_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool inbox, bool hasP2p,
                      bool allRegistries);
// A comm's VCCL_REG_ROOTED_THRESHOLD likewise (plan.h reg_rooted_max).
size_t reg_rooted_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool inbox,
                         bool allRegistries);

// What a rank publishes about where it runs (a PeerMap's identity fields).
struct PeerId {
  int pid;
  uint64_t hostHash;
  int64_t busId;
  uint16_t cuCount;
};
inline uint16_t cu_count_of(int cus) { return (uint16_t)(cus < 1 ? 1 : cus > 65535 ? 65535 : cus); }
struct MeshSetup {
  std::vector<char> netPeer;  // per rank: reached through the net proxy
  bool anyNet = false;
  bool dropLL128 = false;     // free the local LL128 buffer: its ring is off
};
// What the peer table decides: net peers and what they switch off, the
// channel caps, and the two refusals (ncclInvalidUsage).  Every rank
// evaluates every pair / group of the same table, so all ranks agree.
ncclResult_t setup_mesh(int rank, const std::vector<PeerId>& peers, CommSetup* s, MeshSetup* m);

// DevComm::nRings / rsOrder / ringAt of `rank`.
void ring_tables(const std::vector<std::vector<int>>& rings, int nRanks, int rank, DevComm* dc);
// DevComm::llChain from VCCL_LL_CHAIN (identity by default).
ncclResult_t ll_chain(int nRanks, int8_t* chain);
// `rank` on the ring of channel `ch`; ringRanks (may be null): the ring
// rotated to start at `rank` (DevChannel::ringRanks).
struct RingView {
  int pos, next, prev;
};
RingView ring_view(const std::vector<std::vector<int>>& rings, int ch, int rank, int* ringRanks);

#pragma GCC visibility pop
}  // namespace vccl
