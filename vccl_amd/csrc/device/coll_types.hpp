// Work descriptors and buffer layouts of the one-hop LL (ll.hpp) and direct
// (direct.hpp) collectives, shared by the host planner and the kernels.  Kept
// apart from the kernel code so host objects and the other kernel families do
// not recompile when a kernel body changes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ring_types.hpp"

namespace vccl {

// ------------------------------------------------------------------- LL
constexpr int kLLMaxParts = 16;

// One call of an LL launch.  All-reduce: nbytes = count * sizeof(T).
// Reduce-scatter / all-gather: nbytes = the bytes of ONE rank's block (send
// holds n blocks for a reduce-scatter, recv n blocks for an all-gather); the
// reduce-scatter folds each line on the ring of its channel (VCCL's cbd
// partition of the block, `cbd`, DevComm::rsOrder).  Broadcast / reduce:
// nbytes = the call's bytes; the part's root is LLWork::partRoot[i], and a
// reduce folds on the ring of each element's channel like the reduce-scatter
// (`cbd` = the call's partition under the LL protocol).
struct LLPart {
  const char* send;
  char* recv;
  int64_t nbytes;
  int64_t line0;           // first line of this part in the slot
  CbdLite cbd;             // reduce-scatter / reduce only
};

struct LLWork {
  DevComm* comm;
  uint64_t redArg;
  const void* redArgPtr;
  int redArgBytes;
  int preOp;
  int nRanks, rank;
  int linesPerSlot;        // capacity of one (parity, source) slot
  int nParts;              // 1 .. kLLMaxParts calls of one collective in this launch
  int64_t nLines;          // lines of all parts (<= linesPerSlot)
  char* localBuf;          // my LL buffer: [2 parities][nRanks sources][linesPerSlot] lines
  char* peerBuf[kMaxRanks];  // every rank's LL buffer mapped here (peerBuf[rank] = local)
  LLPart parts[kLLMaxParts];
  int8_t partRoot[kLLMaxParts];  // broadcast / reduce: the root of each part (nRanks <= kOrderMaxRanks)
};
// hipModuleLaunchKernel's by-value argument segment is 4 KiB
static_assert(sizeof(LLWork) <= 4096, "LLWork must fit the kernel-argument budget");

// Rooted LL launches (ll.hpp ll_broadcast / ll_reduce; host/plan.cc
// ll_rooted_plan): line 0 of slot (parity, writer) at `reader` carries data
// when the writer is the root of the part holding line 0 (broadcast) or the
// reader is (reduce); otherwise the writer stores the zero arrival token there.
__host__ __device__ __forceinline__ bool ll_rooted_line0_is_data(bool reduce, int writer, int reader, int root0) {
  return reduce ? reader == root0 : writer == root0;
}

// One row of an all-to-all launch's per-peer table (LLA2aWork, DirectA2aWork;
// host/plan.cc a2a_plan gives every ordered pair to one launch of its call).
// The tables are ROTATED to the rank: entry k belongs to rank (rank + k) mod
// nRanks, entry 0 to the rank itself.
struct A2aPeer {
  const char* send;        // my block for this peer
  char* recv;              // where this peer's block lands
  int64_t sendBytes, recvBytes;
  int32_t sendHere, recvHere;  // this direction travels in this launch
};
// One-hop LL all-to-all (ll.hpp ll_alltoall).  An ordered pair that travels
// here moves its bytes as lines [0, ceil(bytes / 8)) of slot (parity, writer) at
// the reader; every other pair moves in the direct or FIFO launch of the same
// call and only exchanges the zero arrival token on line 0 here.  The LL pairs'
// lines are flattened in entry order: entry k's send lines are the grid-stride
// indices [sendLine0[k], sendLine0[k + 1]), likewise recvLine0.
constexpr int kLLA2aMaxRanks = kOrderMaxRanks;
struct LLA2aWork {
  DevComm* comm;
  int rank, nRanks;
  int linesPerSlot;        // capacity of one (parity, source) slot
  int pad;
  char* localBuf;          // my LL buffer
  char* peerBuf[kLLA2aMaxRanks];  // rotated: peerBuf[k] = the LL buffer of rank (rank + k) mod nRanks
  A2aPeer peer[kLLA2aMaxRanks];
  int64_t sendLine0[kLLA2aMaxRanks + 1], recvLine0[kLLA2aMaxRanks + 1];  // [1 .. nRanks]; [nRanks] = the totals
};
static_assert(sizeof(LLA2aWork) <= 4096, "LLA2aWork must fit the kernel-argument budget");

// Byte offset of the (parity, source rank) slot inside an LL buffer.
__host__ __device__ __forceinline__ size_t ll_slot_off(int parity, int src, int nRanks,
                                                       int linesPerSlot) {
  return ((size_t)parity * nRanks + src) * (size_t)linesPerSlot * 16;
}

// --------------------------------------------------------------- direct
constexpr int kDirectMaxRanks = 8;     // phase 2 folds all n inputs in registers
constexpr int kDirectMaxBlocks = 128;
constexpr int kDirectFlagStride = 64;  // bytes between flags
constexpr int kDirectThreads = 512;
constexpr int kDirectUnroll = 2;

// Every rank's inbox and flag array, mapped into this process (device memory,
// so runtime peer indices never index a by-value kernel argument).
struct DirectPeers {
  char* buf[kDirectMaxRanks];
  char* flags[kDirectMaxRanks];
};

struct DirectWork {
  DevComm* comm;
  const DirectPeers* peers;
  const void* sendbuff;
  void* recvbuff;
  uint64_t count;        // elements
  uint64_t redArg;
  const void* redArgPtr;
  int redArgBytes;
  int preOp;
  int nRanks, rank;
  int nBlocks;           // workgroups (block b of every shard -> workgroup b)
  int nChunks;           // the bucket moves through the inbox in chunks
  int64_t chunkElts;     // elements per chunk (last one shorter)
  int64_t blkElts;       // elements per block, the same for every chunk
  int64_t regionBytes;   // bytes per (phase, rank) inbox region
  // VCCL's cbd channel partition (host/plan.cc cbd_schedule, the ring's
  // own) of the recvcount block (reduce-scatter) or of the whole bucket
  // (all-reduce, with the ring chunk arChunk): channel c of [channelLo,
  // channelHi] folds on ring c mod nRings (DevComm::rsOrder / ringAt), so
  // the direct path reproduces the ring's (= VCCL's) fold order exactly.
  CbdLite cbd;
  int64_t arChunk;
  int root;              // broadcast / reduce: the root's rank
  int pad;
};

// Shard length of a chunk of `cc` elements: ceil(cc / n) in 16-byte units.
// The block length stays that of the first (largest) chunk, so block b sits
// at the same inbox offset in every chunk (a shorter last chunk only leaves
// high blocks empty) — the buffer-reuse argument (direct.hpp header) needs
// fixed offsets.
__host__ __device__ __forceinline__ int64_t direct_shard_elts(int64_t cc, int n, int64_t eltAlign) {
  return ((cc + n - 1) / n + eltAlign - 1) / eltAlign * eltAlign;
}
// The rooted direct collectives (direct.hpp direct_broadcast_part /
// direct_reduce_part; host/plan.cc direct_rooted_plan).  A reduce cuts a chunk
// into n shards as the all-reduce does, shard o owned by rank o.  A broadcast
// cuts it into n - 1 shards of whole 16-byte units, shard j owned by the j-th
// rank after the root.
__host__ __device__ __forceinline__ int direct_rooted_shards(bool reduce, int n) { return reduce ? n : n - 1; }
__host__ __device__ __forceinline__ int direct_bcast_owner(int root, int j, int n) { return (root + 1 + j) % n; }
__host__ __device__ __forceinline__ int direct_bcast_shard_of(int root, int rank, int n) {
  return (rank - root - 1 + n) % n;  // rank != root
}

// Inbox: [2 phases][2 parities][nRanks sources][region]; flags likewise.
// The all-reduce double-buffers its chunks by parity (direct.hpp); the
// one-hop reduce-scatter / all-gather / all-to-all and the rooted broadcast /
// reduce use parity 0.
constexpr int kDirectInboxRegions = 4;  // regions per source: phases x parities
__host__ __device__ __forceinline__ size_t direct_region_off(int phase, int parity, int src, int nRanks,
                                                             int64_t regionBytes) {
  return (((size_t)phase * 2 + parity) * nRanks + src) * (size_t)regionBytes;
}
__host__ __device__ __forceinline__ size_t direct_flag_off(int phase, int parity, int src, int b) {
  return ((((size_t)phase * 2 + parity) * kDirectMaxRanks + src) * kDirectMaxBlocks + b) *
         kDirectFlagStride;
}
constexpr size_t kDirectFlagBytes =
    (size_t)kDirectInboxRegions * kDirectMaxRanks * kDirectMaxBlocks * kDirectFlagStride;

// Group aggregation of direct calls (DirectBatch: part 0 in `w`, the others
// as DirectPart — what differs per call), run in order by one launch.
constexpr int kDirectMaxWorks = 16;
struct DirectPart {
  const void* sendbuff;
  void* recvbuff;
  uint64_t count;
  int nChunks;
  int root;              // broadcast / reduce: the part's root (roots may differ per part)
  int64_t chunkElts, blkElts;
  CbdLite cbd;
  int64_t arChunk;
};
struct DirectBatch {
  DirectWork w;
  int nParts;
  DirectPart more[kDirectMaxWorks - 1];
};
// hipModuleLaunchKernel's by-value argument segment is 4 KiB
static_assert(sizeof(DirectBatch) <= 4096, "DirectBatch must fit the kernel-argument budget");
// One-hop direct all-to-all(v) (direct.hpp direct_alltoall; the table is
// A2aPeer's, rotated like LLA2aWork's).  An ordered pair that travels here
// moves its bytes as [0, bytes) of region (0, 0, writer) at the reader;
// workgroup b moves bytes [b * blkBytes, (b + 1) * blkBytes) of every pair.
// Every other pair moves in the LL or FIFO launch of the same call and only
// exchanges flags here.
struct DirectA2aWork {
  DevComm* comm;
  const DirectPeers* peers;
  int rank, nRanks;
  int nBlocks;             // workgroups, the same on every rank of the call
  int pad;
  int64_t blkBytes;        // bytes per block, a multiple of 16
  int64_t regionBytes;     // bytes per (phase, rank) inbox region
  A2aPeer peer[kDirectMaxRanks];
};
static_assert(sizeof(DirectA2aWork) <= 4096, "DirectA2aWork must fit the kernel-argument budget");

// Zero-copy direct collectives over registered buffers (direct_reg.hpp,
// DESIGN.md §4.14): the import table, the descriptor that travels in a flag
// line, and the launch's work.
constexpr int kRegTableEntries = 32;       // host/reg.h kRegMaxEntries
constexpr uint32_t kRegNone = 0xffffffffu;

// The import table: peer p's registered ranges as THIS process addresses them
// (host/regcomm.cc).  It lives in host-pinned mapped memory: the host updates
// it with plain stores while no launch of the comm is in flight, so an enqueue
// never puts a copy on a stream (which could queue behind the spinning kernel
// of another comm of the same process, ncclCommInitAll).  The three counters
// (bumped by workgroup 0) are device-resident.
struct RegPeerEntry {
  char* base;            // nullptr: not imported
  uint64_t size;
  uint32_t generation;
  uint32_t pad;
};
struct RegPeers {
  RegPeerEntry e[kDirectMaxRanks][kRegTableEntries];
};
struct RegStats {
  unsigned long long launches, zeroCopy, fallback;
};

// What travels in a phase-0 flag line behind the 4-byte epoch.
struct RegDesc {
  uint64_t sendOff, recvOff;
  uint64_t sendBytes, recvBytes;
  uint32_t sendEntry, sendGen;   // kRegNone: not registered
  uint32_t recvEntry, recvGen;
};
static_assert(sizeof(RegDesc) + 8 <= kDirectFlagStride, "the descriptor rides in the flag's line");

struct DirectRegWork {
  DirectWork w;          // the staged geometry (the fallback runs it as it is)
  const RegPeers* reg;   // host-pinned, mapped
  RegStats* stats;       // device-resident
  RegDesc mine;
  int64_t zcBlkElts;     // host/plan.cc reg_plan / reg_rooted_plan on w.nBlocks
  // Which buffers the negotiation covers, as kRegSend | kRegRecv bits: `mine`
  // — my own buffers some peer will read (they must be registered); `peer` /
  // `rootPeer` — what I read of a peer that is not / that is rank w.root (it
  // must resolve in my import table).  All-reduce: send | recv everywhere;
  // reduce-scatter / all-gather: send everywhere; the rooted kernels differ by
  // role (host/launch.cc launch_direct_reg_rooted).
  uint8_t needMine, needPeer, needRootPeer;
  uint8_t pad8;
  int pad;
};
enum : uint8_t { kRegSend = 1, kRegRecv = 2 };
static_assert(sizeof(DirectRegWork) <= 4096, "DirectRegWork must fit the kernel-argument budget");

// Zero-copy all-to-all(v) over registered send buffers (direct_reg.hpp
// direct_reg_alltoall).  The table is rotated to the rank like
// A2aPeer's: entry k belongs to rank (rank + k) mod nRanks.  {entry, gen,
// regOff} name my block for that peer inside my registrations (kRegNone: not
// registered, or nothing to send) — the descriptor that travels to it; blkBytes
// is the slice length of ITS block for me (plan.h direct_blk_elts of recvBytes
// at element size 1): only the reader slices, so nothing but the grid has to
// agree between ranks.
constexpr int kRegA2aMaxCalls = 8;  // eligible all-to-alls per comm and group (one skip word each)
struct RegA2aPeer {
  const char* send;        // my block for this peer (the self copy reads entry 0's)
  char* recv;              // where this peer's block lands
  int64_t sendBytes, recvBytes;
  int64_t blkBytes;        // slice b = bytes [b * blkBytes, (b + 1) * blkBytes) of the peer's block
  uint64_t regOff;
  uint32_t entry, gen;
};
// Device-resident per comm: the three counters (bumped by workgroup 0, so graph
// replays count) and the verdict D of each eligible call of the current group,
// which the FIFO launch behind it reads (p2p_types.hpp P2pBatch::skip).
struct RegA2aDev {
  RegStats stats;
  uint32_t skip[kRegA2aMaxCalls];
};
struct DirectRegA2aWork {
  DevComm* comm;
  const DirectPeers* peers;
  const RegPeers* reg;     // host-pinned, mapped
  RegA2aDev* dev;
  int rank, nRanks;
  int nBlocks;             // workgroups, the same on every rank of the call
  int skipIdx;             // this call's skip word, 0 .. kRegA2aMaxCalls - 1
  int selfOk;              // my part of the vote: every block I send is registered, and (v-call) my largest pair
                           // reaches the threshold
  int pad;
  RegA2aPeer peer[kDirectMaxRanks];
};
static_assert(sizeof(DirectRegA2aWork) <= 4096, "DirectRegA2aWork must fit the kernel-argument budget");

__host__ __device__ inline DirectPart direct_part_of(const DirectWork& w) {
  return DirectPart{w.sendbuff, w.recvbuff, w.count, w.nChunks, w.root, w.chunkElts, w.blkElts, w.cbd,
                    w.arChunk};
}
__host__ __device__ inline DirectWork direct_work_with(DirectWork w, const DirectPart& p) {
  w.sendbuff = p.sendbuff;
  w.recvbuff = p.recvbuff;
  w.count = p.count;
  w.nChunks = p.nChunks;
  w.root = p.root;
  w.chunkElts = p.chunkElts;
  w.blkElts = p.blkElts;
  w.cbd = p.cbd;
  w.arChunk = p.arChunk;
  return w;
}

}  // namespace vccl
