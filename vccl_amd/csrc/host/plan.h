// The restatement of VCCL's planner (plan.cc): pure integer arithmetic on
// plain structs — no runtime call, no communicator, no stream.  launch.cc
// reads a comm into these inputs; the plan exports (ext.cc) and through
// them the CPU parity tests (oracle/vccl_sched.py) pass explicit ones.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/nccl.h"
#include "../device/coll_types.hpp"
#include "../device/ring_types.hpp"

#pragma GCC visibility push(hidden)  // internal: the library's exported symbols stay the C ABI's
namespace vccl {

// The values of vcclColl_t (vccl_ext.h) and of the launchers' kColl* codes
// (ring_launch.hpp; tied in launch.cc).
enum Coll { kAllReduce = 0, kReduceScatter = 1, kAllGather = 2, kBroadcast = 3, kReduce = 4 };
// Byte-copy collectives: the host rewrites them as int8 (enqueue.cc:2400-2404).
inline bool is_copy_coll(int coll) { return coll == kAllGather || coll == kBroadcast; }

int type_size(ncclDataType_t t);

// A call's (count, eltSize) as the planner takes them: the byte copies have
// eltSize 1 and count in bytes.
struct CallSize {
  int64_t count, eltSize;
};
inline CallSize call_size(int coll, size_t count, ncclDataType_t datatype) {
  const int64_t tsz = type_size(datatype);
  return is_copy_coll(coll) ? CallSize{(int64_t)count * tsz, 1} : CallSize{(int64_t)count, tsz};
}

// One call's part of VCCL's channel partition (ncclDevWorkColl channelLo /
// channelHi + cbd, device.h:258-287): channels [channelLo, channelHi] carry
// parts of countLo / countMid... / countHi elements, moved in chunks of
// chunkLo / chunkMid / chunkHi elements.
struct CbdPlan {
  int channelLo, channelHi;
  int64_t countLo, countMid, countHi;
  int64_t chunkLo, chunkMid, chunkHi;  // elements
};
// The eight words vcclRingPartition / vcclGroupPlan report a partition as.
inline void cbd_words(const CbdPlan& p, int64_t* out) {
  const int64_t v[8] = {p.channelLo, p.channelHi, p.countLo, p.countMid, p.countHi, p.chunkLo, p.chunkMid, p.chunkHi};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

// The paths a call can take (select_algo).
enum { kAlgoRing = 0, kAlgoLL = 1, kAlgoDirect = 2, kAlgoRingLL128 = 3 };

ncclResult_t host_to_dev_redop(ncclRedOp_t op, ncclDataType_t dt, int nRanks, int* devOp, uint64_t* arg);

constexpr uint64_t kMinTraffic = 16 << 10;  // MinTrafficPerChannel, enqueue.cc:528
int64_t traffic_per_byte(int coll, int nRanks);
int ring_nmax_channels(int coll, int64_t count, int64_t eltSize, int nRanks, int commChannels, int proto,
                       int64_t nThreads);

// The running channel position of a plan (scheduleCollTasksToPlan's
// trafficPerChannel / channelId / currentTraffic, enqueue.cc:549-565).
struct PlanCursor {
  uint64_t trafficPerChannel;
  int channelId;
  uint64_t currentTraffic;
  int nMax;  // nMaxChannels[kind] = comm->nChannels
};

// VCCL's LL step (the default LL buffer, init.cc:617: 8 lines x 512 threads
// x NCCL_STEPS x 16 B, over NCCL_STEPS): only the chunk fields of an LL
// task's plan use it, and the one-hop LL kernels ignore those.
constexpr int64_t kLLStepBytes = 8 * 512 * 16;

CbdPlan cbd_place(PlanCursor& pc, int coll, int64_t count, int64_t eltSize, int nRanks, int proto, int64_t stepBytes);
CbdPlan cbd_schedule(int coll, int64_t count, int64_t eltSize, int nRanks, int commChannels, int proto,
                     int64_t stepBytes, int64_t nThreads);

// The thresholds select_algo decides on (a comm's: launch.cc policy_of).
struct AlgoPolicy {
  int nRanks = 1, algoForce = 0;
  int64_t llSlotBytes = 0;                 // 0: no LL buffers
  uint64_t llMax = 0, llRsAgMax = 0;
  bool ll128 = false;                      // LL128 FIFOs mapped
  uint64_t ll128Min = 0, ll128Max = 0;     // automatic LL128 window (max 0 = off)
  bool direct = false;                     // every peer's inbox mapped
  uint64_t directMax = 0, directRsAgMax = 0;
  uint64_t llRootedMax = 0;                // largest broadcast / reduce on the one-hop LL path (0 = off)
  uint64_t directRootedMax = 0;            // largest broadcast / reduce on the two-hop direct path (0 = off)
};
// A comm's VCCL_LL_ROOTED_THRESHOLD as it takes effect: clamped to what one
// LL slot holds; 0 without LL buffers, with LL excluded by NCCL_PROTO, with a
// peer behind the net proxy, or with more ranks than the fold-order tables.
uint64_t ll_rooted_max(int64_t threshold, int64_t llSlotBytes, bool llAllowed, bool anyNet, int nRanks);
// A comm's VCCL_DIRECT_ROOTED_THRESHOLD as it takes effect: 0 without mapped
// inboxes, with Direct excluded by NCCL_ALGO, with a peer behind the net
// proxy, or above kDirectMaxRanks ranks.
uint64_t direct_rooted_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks);
int select_algo(const AlgoPolicy& p, int coll, int64_t eltSize, int64_t count);
int proto_of_algo(int algo);

struct GroupTask {
  int coll;
  int64_t count, eltSize;  // AG in bytes
  int binKey;              // (func, devOp, type): ncclPrepareTasks' bins
  int funcKey;             // the device function (batches merge per function)
};
// A call as the group planner takes it.  kernelType: dispatch.hpp
// kernel_type_of (K_U8 for a byte copy), passed in so no kernel header is
// needed here.
GroupTask group_task_of(int coll, size_t count, ncclDataType_t datatype, int devOp, int kernelType);

struct PlanGeometry {
  int64_t stepBytes, nThreads;            // SIMPLE: FIFO step, NCCL_NTHREADS
  int64_t ll128StepBytes, ll128Threads;   // LL128: step, NCCL_LL128_NTHREADS
};
// VCCL's default LL128 geometry: NCCL_LL128_BUFFSIZE / NCCL_STEPS, NCCL_LL128_NTHREADS.
constexpr struct {
  int64_t stepBytes, nThreads;
} kDefaultLL128{120 * 640 * 8, 640};
struct GroupPlanOut {
  std::vector<int> order;        // tasks in execution (plan) order
  std::vector<int> planOf;       // per task: the plan (kernel) it lands in
  std::vector<int> algo;         // per task: the path of its aggregate
  std::vector<CbdPlan> cbd;      // per task, under the path's protocol
};
uint32_t u32fp_encode(uint32_t x, int bitsPerPow2);
void group_plan(const std::vector<GroupTask>& ts, int nRanks, int commChannels, const PlanGeometry& geo,
                const AlgoPolicy* pol, GroupPlanOut* out);

// ------------------------------------------------------------ rooted LL
// The line layout of one rooted LL launch (device/ll.hpp ll_broadcast /
// ll_reduce) as `rank` sees it: part i (root roots[i], bytes[i] bytes) sits at
// lines [line0[i], line0[i] + ceil(bytes[i] / 8)) of every slot.  stores: the
// line ranges this rank writes into slot (parity, rank) of `peer`'s buffer;
// polls: the line ranges it reads from slot (parity, peer) of its own.  A
// range of part -1 is the arrival token: line 0 of every ordered pair that
// carries no data line 0 (ll_rooted_line0_is_data).  ncclInvalidArgument when
// the lines do not fit one slot.
struct LLRange {
  int peer, part;          // part -1: the token line
  int64_t line0, line1;    // [line0, line1)
};
struct LLRootedPlanOut {
  std::vector<int64_t> line0;  // per part
  int64_t nLines = 0;
  std::vector<LLRange> stores, polls;
};
ncclResult_t ll_rooted_plan(int coll, int nRanks, int rank, const std::vector<int>& roots,
                            const std::vector<int64_t>& bytes, int64_t linesPerSlot, LLRootedPlanOut* out);

// ------------------------------------------------------------ rooted direct
// One direct broadcast / reduce (device/direct.hpp direct_broadcast_part /
// direct_reduce_part) as `rank` runs it: the chunk length, the shards of chunk
// `chunk` and their owners, and the ordered steps of that chunk.  The step
// order IS the kernel's phase order — the two are kept side by side and name
// each other; host/launch.cc direct_work_of takes its geometry from here.
// Lengths and offsets in bytes; a step covers a whole shard (workgroup b moves
// bytes [b * blk, (b + 1) * blk) of it, so region offsets are 0).
//   kDStepWait   {phase, peer = from}
//   kDStepStore  {peer, phase, region = the writer's, regionOff, userOff, bytes, src}
//                src kDSrcSend: sendbuff[userOff ..]; kDSrcRegion: my own region
//                (0, root) (the broadcast's forward); kDSrcFold: the fold of my
//                shard, my input at userOff and my regions (0, q) (the reduce)
//   kDStepRead   {phase, region = the source's, regionOff, userOff, bytes}:
//                my region -> recvbuff[userOff ..]
//   kDStepPost   {phase}: my flag at every peer
//   kDStepLocal  {userOff, bytes, src}: kDSrcSend: sendbuff -> recvbuff (the
//                broadcast root, out of place); kDSrcFold: the root's own
//                shard folded straight into recvbuff
enum { kDStepWait = 0, kDStepStore = 1, kDStepRead = 2, kDStepPost = 3, kDStepLocal = 4 };
enum { kDSrcSend = 0, kDSrcRegion = 1, kDSrcFold = 2 };
struct DirectStep {
  int kind, phase, peer, region;
  int64_t regionOff, userOff, bytes;
  int src;
};
struct DirectRootedPlanOut {
  int64_t chunkElts = 0;   // elements per chunk (the last one shorter)
  int nChunks = 0;
  int64_t shardElts = 0;   // of chunk `chunk`
  std::vector<int> owner;  // per shard
  std::vector<DirectStep> steps;
};
// count in elements of eltSize (a broadcast: bytes, eltSize 1).  chunk < 0:
// the geometry only.  ncclInvalidArgument when a region cannot hold 16 bytes.
ncclResult_t direct_rooted_plan(int coll, int nRanks, int rank, int root, int64_t count, int64_t eltSize,
                                int64_t regionBytes, int chunk, DirectRootedPlanOut* out);

// -------------------------------------------------------- registered buffers
// The zero-copy direct all-reduce / reduce-scatter / all-gather over
// ncclCommRegister'ed buffers (reg.h holds the table): the
// host's half — the threshold, the eligibility rule and the step list of one
// zero-copy launch.
// A comm's VCCL_REG_THRESHOLD (bytes) as it takes effect: 0 without mapped
// inboxes and direct flags, with Direct excluded by NCCL_ALGO, with a peer
// behind the net proxy, or with fewer than 2 or more than kDirectMaxRanks ranks.
uint64_t reg_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks);
// A call's size as the threshold measures it: the all-reduce's count * esz,
// the whole nRanks-block buffer of a reduce-scatter (recvcount) / all-gather
// (sendcount).
int64_t reg_call_bytes(int coll, int64_t count, int64_t typeSize, int nRanks);
// From the call's own arguments and comm-wide values alone (a rank cannot
// know what its peers registered): effective > 0, an all-reduce, reduce-
// scatter or all-gather, not a member of a group that holds more than one
// collective (groupCalls = the collectives of the call's group, 0 or 1 for a
// call alone), and at least `effective` bytes.
bool reg_eligible(int coll, int64_t count, int64_t typeSize, int nRanks, uint64_t effective, int groupCalls);
// One zero-copy launch as `rank` runs it on a grid of nBlocks workgroups: two
// positions of the comm's direct epoch sequence.  Epoch 0 negotiates (the
// descriptors travel with the phase-0 flags, the verdicts with the phase-1
// flags); epoch 1 moves the data with no inbox: one "chunk", every rank PULLS
// from its peers' registered buffers and stores into its own recvbuff only.
//   kRStepPost  {epoch, phase}: my flag at every peer
//   kRStepWait  {epoch, phase, peer}: that peer's flag at me
//   kRStepFold  {epoch, peer, buf, peerOff, ownOff, bytes}: `peer`'s buffer
//               `buf` at peerOff is one source of the n-source fold stored at
//               recvbuff[ownOff ..] (peer == rank: my own input); the n fold
//               steps of a launch are ONE reduce-copy, listed in rank rotation
//               (the fold order itself is the ring's, from the comm's tables)
//   kRStepCopy  {epoch, peer, buf, peerOff, ownOff, bytes}: a plain copy of
//               peer's buffer into recvbuff[ownOff ..] (peer == rank, buf
//               send: the all-gather's own block, skipped by the kernel when
//               the call is in place)
// Offsets and lengths in bytes; a step covers a whole shard, of which
// workgroup b moves elements [b * blkElts, (b + 1) * blkElts).  shardElts: the
// all-reduce's direct_shard_elts of the whole count, a reduce-scatter's
// recvcount, an all-gather's bytes per rank; blkElts = alignUp(ceil(shardElts
// / nBlocks), 16 bytes).  count in elements of eltSize (an all-gather: bytes,
// eltSize 1).  ncclInvalidArgument for any other collective.
enum { kRStepPost = 0, kRStepWait = 1, kRStepFold = 2, kRStepCopy = 3 };
enum { kRBufSend = 0, kRBufRecv = 1 };
struct RegStep {
  int kind, epoch, phase, peer, buf;
  int64_t peerOff, ownOff, bytes;
};
struct RegPlanOut {
  int64_t shardElts = 0, blkElts = 0;
  std::vector<RegStep> steps;
};
ncclResult_t reg_plan(int coll, int nRanks, int rank, int64_t count, int64_t eltSize, int nBlocks, RegPlanOut* out);

// -------------------------------------- rooted collectives over registered buffers
// The zero-copy ncclBroadcast / ncclBcast / ncclReduce (device/direct_reg.hpp
// reg_broadcast_zc / reg_reduce_zc): the host's half.
// A comm's VCCL_REG_ROOTED_THRESHOLD (bytes) as it takes effect: 0 wherever
// reg_max gives 0, or when any rank failed to create its registry.  No upper
// clamp: the broadcast uses no inbox, the reduce moves through it in chunks.
uint64_t reg_rooted_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks,
                        bool allRegistries);
// From the call's own arguments and comm-wide values alone: effective > 0, a
// broadcast or a reduce of count * typeSize >= effective bytes, alone or its
// comm's only collective of its group (groupCalls <= 1).  An eligible call
// launches the negotiating kernel ahead of select_algo's choice at any size;
// its on-device fallback is the staged direct rooted part, never the ring.
bool reg_rooted_eligible(int coll, int64_t count, int64_t typeSize, uint64_t effective, int groupCalls);
// One launch as `rank` runs it on nBlocks workgroups — device/direct_reg.hpp
// reg_broadcast_zc / reg_reduce_zc keep this order and name this list.  Epoch 0
// negotiates as in reg_plan; the broadcast then spends ONE more position on the
// whole byte count, the reduce one per chunk of the staged geometry
// (direct_rooted_plan on regionBytes): epoch 1 + c is chunk c.  RegStep's words,
// with two more kinds:
//   kRStepPost / kRStepWait  as reg_plan's
//   kRStepCopy  {epoch, peer, buf, peerOff, ownOff, bytes}: peer's buffer `buf`
//               -> recvbuff[ownOff ..]: a non-root's pull of its own shard from
//               the root's sendbuff, of another shard from its owner's recvbuff;
//               peer == rank, buf send: the broadcast root's local send -> recv
//               copy (skipped by the kernel in place)
//   kRStepFold  {epoch, peer, buf send, peerOff, ownOff, bytes}: one source of
//               the owner's n-source fold of its shard of the chunk, listed in
//               rank rotation (the fold order is the ring reduce's, from the
//               comm's tables).  On the root the fold lands at recvbuff[ownOff
//               ..]; on any other owner ownOff is -1 and the result goes where
//               the kRStepStoreRoot that follows the n fold steps says
//   kRStepStoreRoot  {epoch, peer = the root, ownOff = the shard's user offset,
//               bytes}: the folded shard -> region (1, rank) of the root's inbox
//   kRStepCollect    {epoch, peer = o, ownOff, bytes}: the root copies its region
//               (1, o) -> recvbuff[ownOff ..]
// Offsets and lengths in bytes; a step covers a whole shard, of which workgroup
// b moves [b * blk, (b + 1) * blk): blkElts is the broadcast's zero-copy block
// length, alignUp(ceil(shard / nBlocks), 16) bytes of its n - 1 shards of the
// whole count (shardElts), and the reduce's 0 (its blocks are the staged
// geometry's).  count in elements of eltSize (a broadcast: bytes, eltSize 1).
enum { kRStepStoreRoot = 4, kRStepCollect = 5 };
struct RegRootedPlanOut {
  int64_t shardElts = 0, blkElts = 0;
  int nChunks = 0;           // reduce: the staged chunk count; broadcast: 1
  int64_t chunkElts = 0;
  std::vector<RegStep> steps;
};
ncclResult_t reg_rooted_plan(int coll, int nRanks, int rank, int root, int64_t count, int64_t eltSize,
                             int64_t regionBytes, int nBlocks, RegRootedPlanOut* out);

// ------------------------------------------- all-to-all over registered buffers
// The zero-copy ncclAllToAll(v) (device/direct_reg.hpp direct_reg_alltoall,
// DESIGN.md §4.15): the host's half.
// A comm's VCCL_REG_A2A_THRESHOLD (bytes per ordered pair) as it takes effect:
// 0 wherever reg_max gives 0, on a comm without point-to-point connections (the
// fallback needs the FIFOs), or when any rank failed to create its registry.
uint64_t reg_a2a_max(int64_t threshold, bool inbox, bool directAllowed, bool anyNet, int nRanks, bool hasP2p,
                     bool allRegistries);
// From comm-wide values only, so every rank launches the negotiating kernel for
// the same calls: the index-th (from 0) all-to-all of its comm in its group,
// fewer than kRegA2aMaxCalls before it; a uniform call of pairBytes >=
// effective; EVERY v-call (a rank knows only its row and column: size enters as
// part of the rank's vote).  An eligible call pre-empts a2a_plan: none of its
// pairs go to the LL or direct all-to-all launch.
bool reg_a2a_eligible(bool uniform, int64_t pairBytes, uint64_t effective, int index);
// A v-call rank's part of the vote: its largest pair with another rank, send or
// receive, reaches the threshold (a uniform call passed it to be eligible).
bool reg_a2a_size_vote(int nRanks, int rank, const int64_t* sendBytes, const int64_t* recvBytes, bool uniform,
                       uint64_t effective);
// The grid, the same on every rank: a uniform call's ceil(B / direct_blk_elts(B,
// 1, ...)); a v-call's largest grid under the CTA bounds and co-residency caps.
int reg_a2a_blocks(bool uniform, int64_t pairBytes, int minCTAs, int maxCTAs, int directMaxBlocks);
// The slice length of one block of `bytes` bytes: direct_blk_elts at element
// size 1 (at least 16), whose ceil(bytes / that) slices never exceed the grid.
// Chosen by the reader alone: the sender takes no part in a pull.
int64_t reg_a2a_blk(int64_t bytes, int minCTAs, int maxCTAs, int directMaxBlocks);
// One launch as `rank` runs it.  sendBytes / sendOff: the whole n x n matrices,
// row r rank r's (bytes and byte offsets in r's sendbuff, column p = for peer
// p); recvOff: this rank's n receive offsets.  Steps, in the kernel's order:
//   kAStepPost  {epoch, phase}: my flag at every peer (epoch 0 phase 0 carries
//               the per-peer descriptor, phase 1 the vote)
//   kAStepWait  {epoch, phase, peer}
//   kAStepVote  {epoch 0}: ok_me from the descriptors just read
//   kAStepPull  {epoch 1, peer, peerOff = the sender's displacement for me,
//               ownOff, bytes, blkBytes}: workgroup b moves bytes [b * blkBytes,
//               (b + 1) * blkBytes) of it; peers in rotation (rank + k) mod n
//   kAStepSelf  {epoch 1, peerOff (in my sendbuff), ownOff, bytes, blkBytes}
// then the closing rounds (post / wait (1, 0), post / wait (1, 1)).  With D = 0
// the launch ends after epoch 0: the list's prefix.
enum { kAStepPost = 0, kAStepWait = 1, kAStepVote = 2, kAStepPull = 3, kAStepSelf = 4 };
struct RegA2aStep {
  int kind, epoch, phase, peer;
  int64_t peerOff, ownOff, bytes, blkBytes;
};
struct RegA2aPlanOut {
  int nBlocks = 0;
  std::vector<RegA2aStep> steps;
};
ncclResult_t reg_a2a_plan(int nRanks, int rank, const int64_t* sendBytes, const int64_t* sendOff,
                          const int64_t* recvOff, bool uniform, int minCTAs, int maxCTAs, int directMaxBlocks,
                          RegA2aPlanOut* out);

// ---------------------------------------------------------------- all-to-all
// A comm's VCCL_LL_A2A_THRESHOLD (bytes per ordered pair) as it takes effect:
// clamped to what one LL slot holds; 0 without LL buffers, with LL excluded by
// NCCL_PROTO, with a peer behind the net proxy, with fewer than 2 or more than
// kOrderMaxRanks ranks, or on a comm without point-to-point connections (the
// pairs above the limit need them).
uint64_t ll_a2a_max(int64_t threshold, int64_t llSlotBytes, bool llAllowed, bool anyNet, int nRanks, bool hasP2p);
// A comm's VCCL_DIRECT_A2A_THRESHOLD (bytes per ordered pair) as it takes
// effect: clamped to what one inbox region holds ((regionBytes - 16) rounded
// down to 16 bytes, the slack launch.cc direct_work_of leaves); 0 without
// mapped inboxes (regionBytes == 0), with Direct excluded by NCCL_ALGO, with a
// peer behind the net proxy, with fewer than 2 or more than kDirectMaxRanks
// ranks, or on a comm without point-to-point connections.
uint64_t direct_a2a_max(int64_t threshold, int64_t regionBytes, bool directAllowed, bool anyNet, int nRanks,
                        bool hasP2p);
// Pair rule, three-way, from B and the two comm-wide limits alone (so both
// ends agree, nothing else enters): the ordered pair (writer -> reader) of B
// bytes travels by LL iff llA2aMax > 0 && B <= llA2aMax (B = 0 counts as LL:
// its token is all it needs); else direct iff directA2aMax > 0 && B <=
// directA2aMax (B = 0 included); else the FIFOs.
enum { kA2aFifo = 0, kA2aLL = 1, kA2aDirect = 2 };
inline int a2a_pair_path(uint64_t llA2aMax, uint64_t directA2aMax, int64_t bytes) {
  if (llA2aMax > 0 && (uint64_t)bytes <= llA2aMax) return kA2aLL;
  return directA2aMax > 0 && (uint64_t)bytes <= directA2aMax ? kA2aDirect : kA2aFifo;
}
// The direct kernels' block length for a shard of `len` elements of `esz`
// bytes (launch.cc direct_work_of, a2a_plan): nb = ceil(len / 16 KiB) blocks
// (one 512-thread x 2-pack hunk each) clamped by maxCTAs / minCTAs, then by the
// co-residency caps directMaxBlocks and kDirectMaxBlocks LAST, so NCCL_MIN_CTAS
// cannot push past them; the length is alignUp(ceil(len / nb), 16
// bytes), in elements.  The caller's grid is ceil(len / that).
inline int64_t direct_blk_elts(int64_t len, int64_t esz, int minCTAs, int maxCTAs, int directMaxBlocks) {
  const int64_t minBlk = (16 << 10) / esz, eltAlign = std::max<int64_t>(1, 16 / esz);
  int64_t nb = (len + minBlk - 1) / minBlk;
  nb = std::max<int64_t>(std::min<int64_t>(nb, maxCTAs), minCTAs);
  nb = std::max<int64_t>(1, std::min<int64_t>({nb, (int64_t)directMaxBlocks, (int64_t)kDirectMaxBlocks}));
  return ((len + nb - 1) / nb + eltAlign - 1) / eltAlign * eltAlign;
}
// One ncclAllToAll (uniform) / ncclAllToAllv call as `rank` runs it (device/
// ll.hpp ll_alltoall, device/direct.hpp direct_alltoall).  Launch rule,
// identical on every rank: a uniform call of B bytes per pair is one LL launch
// and nothing else when 0 < B <= llA2aMax, else one direct launch and nothing
// else when 0 < B <= directA2aMax, else the FIFO path whole; a v-call has an LL
// launch whenever llA2aMax > 0 — peers may hold LL pairs among themselves and
// expect this rank's arrival token — then exactly one direct launch iff
// directA2aMax > 0 — even when this rank's row and column hold no direct pair:
// peers wait for its flags — then the FIFO launch for the residual pairs, those
// above both limits.  A path without its launch takes no pair.  The self block
// takes its path (a local copy in that path's kernel, which skips it when the
// pointers coincide) when both its lengths agree; otherwise it stays a
// FIFO-launch copy (or its refusal).
// LL: pair (r -> p)'s data occupies lines [0, ceil(B / 8)) of slot (parity, r)
// at p; stores / polls list them as LLRange{peer, 0, 0, lines} and the 1-line
// zero token of every other pair as LLRange{peer, -1, 0, 1}, in the kernel's
// rotation (rank + k) mod n, so line 0 of every ordered pair is written once
// and read once per launch; both are empty without an LL launch.
// ncclInvalidArgument when an LL pair exceeds the slot.
// Direct geometry, from comm-wide values only (M = B for a uniform call,
// directA2aMax for a v-call: a rank knows only its row and column): blkBytes =
// direct_blk_elts(M, 1, ...), nBlocks = ceil(M / blkBytes); both 0 without a
// direct launch.  Pair (r -> p) occupies bytes [0, B) of region (0, 0, r) at p;
// one chunk, one epoch per launch.
// resSends / resRecvs: the peers whose send / recv stays on the FIFOs, in peer
// order.  With directA2aMax == 0 this is the two-way LL / FIFO plan
// (vcclLLA2aPlan), and the CTA bounds and directMaxBlocks go unread.
struct A2aPlanOut {
  std::vector<char> sendPath, recvPath;  // per peer: kA2aFifo / kA2aLL / kA2aDirect
  bool llLaunch = false, directLaunch = false;
  int nBlocks = 0;
  int64_t blkBytes = 0;
  std::vector<LLRange> stores, polls;
  std::vector<int> resSends, resRecvs;
};
ncclResult_t a2a_plan(int nRanks, int rank, const int64_t* sendBytes, const int64_t* recvBytes, bool uniform,
                      uint64_t llA2aMax, uint64_t directA2aMax, int64_t linesPerSlot, int minCTAs, int maxCTAs,
                      int directMaxBlocks, A2aPlanOut* out);

// ------------------------------------------------------------ point-to-point
// The plan of a group's ncclSend / ncclRecv calls of one comm on its per-peer
// connections (device/p2p_types.hpp), restating the reference's queueing
// (enqueue.cc:1042-1109, :2318-2337; round pairing init.cc:1117-1137 on one
// flat node): sends and recvs are queued per peer in call order; sweep s takes
// the s-th send to and the s-th recv from every peer; within a sweep round
// d = 0..n-1 pairs "send to (rank + d) mod n" with "recv from (rank - d) mod n".
// A message of B bytes uses p = clamp(ceil(B / minPartBytes), 1, parts) parts
// of alignUp(ceil(B / p), 16) bytes (the last one shorter); part q travels on
// connection (peer, q) in ceil(bytes / stepBytes) steps.  Both ends derive
// that from B and the comm-wide constants alone.  A zero-byte message is
// matched and moves nothing.
//
// Invariants of every plan:
//   I1  a connection direction is driven by one workgroup for the whole group;
//   I2  a workgroup runs its items in increasing (sweep, round, part) order;
//   I3  sender and receiver compute the same (sweep, parts, part sizes, steps);
//   I4  (the caller's gCap) every rank's whole grid is co-resident.
// With I1-I3 a blocked item waits on a workgroup at a lower or equal key whose
// own wait is on the other direction, so no cycle exists for any matched set
// of calls, any grid, and any cut of the list into launches.
enum { kP2pCallSend = 0, kP2pCallRecv = 1 };
struct P2pCall {
  int kind;       // kP2pCallSend / kP2pCallRecv
  int peer;
  int64_t bytes;
  uint64_t buff;  // the user buffer's address (self pairs: same buffer = no copy)
};
struct P2pGeometry {
  int parts;
  int64_t minPartBytes, stepBytes;
};
struct P2pSplit {
  int nParts;         // parts that carry bytes (0 for an empty message)
  int64_t partBytes;  // part q covers [q * partBytes, min(B, (q + 1) * partBytes))
};
P2pSplit p2p_split(int64_t bytes, const P2pGeometry& g);
struct P2pItem {
  int launch, wg;
  int kind;  // device/p2p_types.hpp kP2pSend / kP2pRecv / kP2pCopy
  int sweep, round, part, peer;
  int call, call2;  // the call; a copy: the send and its recv
  int64_t offset, bytes, steps;
};
struct P2pPlanOut {
  std::vector<P2pItem> items;  // in (sweep, round, part) order, a send before its round's recv
  int nWgs = 0;                // workgroups per direction (the grid is twice that)
  int nLaunches = 0;
};
// gMin / gCap: the CTA floor, applied before the cap (gCap <= 0: none).
// maxWorks: items per launch.  ncclInvalidUsage: a send to self without its
// recv, or the reverse, or the two of different lengths.
ncclResult_t p2p_plan(int rank, int nRanks, const std::vector<P2pCall>& calls, const P2pGeometry& g, int gMin,
                      int gCap, int maxWorks, P2pPlanOut* out);

}  // namespace vccl
#pragma GCC visibility pop
