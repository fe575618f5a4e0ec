/*
 * vccl-mi355x communicator extensions (host only, no GPU work).
 *
 *   vcclCommCollAlgo  which algorithm ncclAllReduce / ncclReduceScatter /
 *                     ncclAllGather would run for (count, datatype) on this
 *                     communicator — the outcome of the tuner step
 *                     topoGetAlgoInfo (src/enqueue.cc:1805-1945) that VCCL
 *                     only reports through NCCL_DEBUG=INFO logs.  For
 *                     benchmarks and tests; enqueues nothing.
 *   vcclCommSetAlgo   per-communicator override of that choice (the
 *                     NCCL_ALGO / NCCL_PROTO environment, graph/tuning.cc:
 *                     354-373, read once at init): -1 = automatic, otherwise
 *                     a vcclAlgo_t; an algorithm that cannot carry a call
 *                     (bucket above its buffer, not an all-reduce) falls
 *                     through to the ring, as with the environment.
 *   vcclCommLaunchStats  collectives enqueued on this communicator so far and
 *                     how many launches carried more than one of them (group
 *                     aggregation of small all-reduces into one LL launch).
 *   vcclCommRingTrace the SIMPLE ring's slot timeline of the last launch
 *                     (VCCL_RING_TRACE=<records per channel> at init, else
 *                     ncclInvalidUsage): per channel `cap` records of 56 bytes
 *                     {t0 entry, t1 credits seen, t2 released, t3 payload
 *                     drained, t4 flags stored (s_memrealtime, 100 MHz);
 *                     uint32 shape = RECV | SEND<<1 | SRC<<2 | DST<<3; uint32
 *                     payload bytes; uint64 step}, unused records zero.  A
 *                     measurement hook (no reference counterpart).
 *   vcclCommNetStats  payload bytes this rank's net proxy has sent / received
 *                     and its connection count (0 when every peer is reached
 *                     over xGMI).  The net transport carries ring connections
 *                     to peers on other nodes (or every connection with
 *                     VCCL_NET_FORCE=1) through host-pinned staging buffers
 *                     and TCP, as the reference's proxy + net transport
 *                     (src/proxy.cc:914-971, src/transport/net.cc:1293-1482).
 *   vcclCommSetFences  switch the system-scope acquire/release fences around
 *                     every FIFO slot / inbox hand-off on (1) or off (0, the
 *                     default: write-through sc0 sc1 payload accesses need no
 *                     fence) — the VCCL_FENCES=1 safety valve at run time, so
 *                     one process can check a transport both ways.  Blocks
 *                     until the device is idle; call with no collective of
 *                     this communicator in flight.
 *   vcclCommSetRingWave  the SIMPLE ring's slot hand-off for this
 *                     communicator's later launches: 0 (the default, or
 *                     VCCL_RING_WAVE=0 at init) the workgroup hand-off — every
 *                     wave drains its stores, a barrier, one thread posts, as
 *                     the reference's postPeer after its barrier
 *                     (src/device/prims_simple.h:183-319); 1 the per-wave
 *                     hand-off, each wave draining its slot behind its next
 *                     slot's loads and the last one posting,
 *                     for the kernels built with it (sums over f32 / f16 /
 *                     bf16, the byte-copy all-gather and broadcast; other
 *                     calls keep the workgroup hand-off).  Same FIFOs,
 *                     partition and fold either way, so results are
 *                     identical and calls may switch between the two.
 *                     perWave -1 leaves the setting as it is; *waveLaunches
 *                     (may be NULL): ring launches that ran the per-wave
 *                     kernel so far.  Host only.
 *   vcclCommDebugSetEpochs  overwrite the device-resident call epochs of the
 *                     one-shot LL and two-shot direct paths (tests of the
 *                     32-bit wrap; the reference's TEST_LL_CLEANUP knob,
 *                     src/include/device.h:70-77, serves the same purpose).
 *                     Every rank must set the same values between calls.
 *   vcclRingPartition  the channel partition the ring algorithm uses for a
 *                     call (host only): VCCL's cbd split and chunking
 *                     (scheduleCollTasksToPlan, src/enqueue.cc:518-644, for a
 *                     plan of one collective) for `nChannels` channels,
 *                     protocol `proto` (2 SIMPLE, 1 LL128, 0 LL) with a FIFO step
 *                     of `stepBytes` (that protocol's buffer size / 8) and
 *                     `nThreads` ring threads (NCCL_NTHREADS: the channel
 *                     tuning's maxThreads[RING][SIMPLE], tuning.cc:198-200).
 *                     out[0..7]
 *                     = channelLo, channelHi, countLo, countMid, countHi,
 *                     chunkLo, chunkMid, chunkHi (elements; bytes for
 *                     all-gather, which the reference runs as int8).
 *   vcclRingOrders     the arc-balanced ring set for n ranks (SURVEY.md
 *                     Appendix D; Walecki's decomposition for odd n).
 *   vcclRingChunkOf    for element i of an all-reduce on that partition:
 *                     out[0] = its channel, out[1] = the ring chunk c of its
 *                     loop (the chunk that finishes at ring position c,
 *                     src/device/all_reduce.h:32-64), out[2] = the end of that
 *                     chunk — the lookup the direct all-reduce folds by.
 *   vcclGroupPlan      the partition a GROUP of calls of one
 *                     communicator gets (host only): VCCL's multi-task plan —
 *                     the size sorter and (func, op, type) bins with 4x
 *                     aggregation of ncclPrepareTasks (src/enqueue.cc:352-437)
 *                     and scheduleCollTasksToPlan's shared trafficPerChannel,
 *                     running channelId and currentTraffic, split into kernel
 *                     plans at the argument budget (:518-769).  Inputs per
 *                     call: colls[i], counts[i] (AR count, RS recvcount, AG
 *                     sendcount), datatypes[i], ops[i] (ncclRedOp_t built-in;
 *                     ignored for all-gather).  Outputs: order[0..n) the calls
 *                     in plan (execution) order, planOf[i] the kernel plan of
 *                     call i, cbd[8 i .. 8 i + 8) its partition as in
 *                     vcclRingPartition.  Every call is taken as RING /
 *                     SIMPLE (LL128 geometry: VCCL's defaults).
 *   vcclGroupPlanEx    the same plan with a path per aggregate, as a comm
 *                     lays out a group: each aggregate takes the path the
 *                     library's selection gives its summed count (VCCL gives
 *                     getAlgoInfo's choice to every member, enqueue.cc:
 *                     387-427) and is placed under that path's protocol (LL
 *                     traffic x4).  geometry[4] = SIMPLE step bytes,
 *                     NCCL_NTHREADS, LL128 step bytes, NCCL_LL128_NTHREADS;
 *                     policy[10] (NULL: every call RING / SIMPLE) =
 *                     algoForce (0 automatic, 1 ring, 2 LL, 3 direct,
 *                     4 LL128), LL slot bytes (0: no LL buffers), LL
 *                     all-reduce max bytes, LL RS / AG max bucket bytes,
 *                     LL128 FIFOs (0/1), LL128 window min, max (0: off),
 *                     direct inboxes (0/1), direct all-reduce max bytes,
 *                     direct RS / AG max bucket bytes; algos[i] (may be
 *                     NULL) = the vcclAlgo_t of call i.
 *   vcclRootedAlgo     the path of one call on an explicit policy that also
 *                     carries the rooted LL threshold (host only): policy[10]
 *                     as in vcclGroupPlanEx; `threshold` = the comm's
 *                     VCCL_LL_ROOTED_THRESHOLD in bytes (negative: read it
 *                     from the environment; default 0 = off); llAllowed = the
 *                     NCCL_ALGO / NCCL_PROTO lists leave protocol LL; anyNet =
 *                     a peer is reached through the net proxy.  *effective
 *                     (may be NULL) = the threshold as the comm takes it:
 *                     clamped to the LL slot (policy[1]), 0 without LL
 *                     buffers, with LL excluded, with a net peer or above 8
 *                     ranks.  A broadcast or reduce of at most that many
 *                     bytes takes vcclAlgoLL (automatic or forced LL); with 0
 *                     every call takes what vcclGroupPlanEx's policy gives it.
 *   vcclRootedAlgoEx   vcclRootedAlgo plus the rooted direct threshold (host
 *                     only): directThreshold = the comm's
 *                     VCCL_DIRECT_ROOTED_THRESHOLD in bytes (negative: read it
 *                     from the environment; default 0 = off); directAllowed =
 *                     the NCCL_ALGO list leaves Direct.  *directEffective (may
 *                     be NULL) = the threshold as the comm takes it: 0 without
 *                     mapped inboxes (policy[7]), with Direct excluded, with a
 *                     net peer or above 8 ranks.  A broadcast or reduce takes,
 *                     in this order, vcclAlgoLL (as vcclRootedAlgo), the LL128
 *                     window, vcclAlgoDirect up to that many bytes, the ring;
 *                     forced Direct (policy[0] = 3) takes vcclAlgoDirect at any
 *                     size, but only with a non-zero effective threshold: with
 *                     0 every call takes what vcclRootedAlgo gives it.
 *   vcclDirectRootedPlan  one direct broadcast / reduce (root `root`, `count`
 *                     elements of `datatype`) on inbox regions of regionBytes,
 *                     as rank `rank` runs it (host only).
 *                     geometry[4] = elements per chunk (a broadcast: bytes),
 *                     chunks, the shard length of chunk `chunk`, shards;
 *                     owners[shards] (may be NULL) = the owner of each shard
 *                     (a reduce: n shards, shard o at rank o; a broadcast:
 *                     n - 1 shards of whole 16-byte units, shard j at rank
 *                     (root + 1 + j) mod n); steps = the ordered steps of
 *                     chunk `chunk` (chunk < 0: none), 8 words each {kind,
 *                     phase, peer, region, region offset, user offset, bytes,
 *                     src}, offsets and lengths in bytes, the kernels' phase
 *                     order (device/direct.hpp):
 *                       kind 0 wait   flag (phase, peer) in my flag array;
 *                       kind 1 store  into inbox region (phase, region = me)
 *                              of `peer`, from src 0 sendbuff at the user
 *                              offset, 1 my own region (0, root) (the
 *                              broadcast's forward), 2 the fold of my shard
 *                              (my input at the user offset and my regions
 *                              (0, q), in the ring reduce's order);
 *                       kind 2 read   my region (phase, region) -> recvbuff at
 *                              the user offset;
 *                       kind 3 post   my flag of `phase` at every peer;
 *                       kind 4 local  src 0 sendbuff -> recvbuff (the
 *                              broadcast root, out of place), src 2 the
 *                              root's own shard folded into recvbuff.
 *                     ncclInvalidArgument when the step count exceeds cap.
 *   vcclLLRootedPlan   the line layout of one rooted LL launch (broadcast or
 *                     reduce, 1..16 parts with a root and a byte count each) as
 *                     rank `rank` sees it (host only): line0[i]
 *                     (may be NULL) = the first slot line of part i; stores /
 *                     polls = 4 words per range {peer, part (-1: the arrival
 *                     token), first line, end line}: the lines this rank
 *                     writes into its slot at `peer`, and the lines it reads
 *                     from `peer`'s slot in its own buffer.
 *                     ncclInvalidArgument when the lines exceed linesPerSlot
 *                     or a range count exceeds cap.
 *   vcclLLA2aMax       a comm's VCCL_LL_A2A_THRESHOLD (bytes per ordered pair of
 *                     an ncclAllToAll(v); negative: read it from the
 *                     environment; default 0 = off) as it takes effect (host
 *                     only): clamped to the LL slot
 *                     (llSlotBytes), 0 without LL buffers, with LL excluded,
 *                     with a net peer, below 2 or above 8 ranks, or without
 *                     point-to-point connections.
 *   vcclLLA2aPlan      how one ncclAllToAll (uniform != 0: every entry of both
 *                     rows the same) / ncclAllToAllv call of sendBytes[nRanks]
 *                     / recvBytes[nRanks] splits, as rank `rank` runs it, on a
 *                     comm whose effective limit is llA2aMax (host only).  The
 *                     ordered pair of B bytes is an LL pair iff llA2aMax > 0 and
 *                     B <= llA2aMax; *launch = the call has an LL launch (a
 *                     uniform call iff 0 < B <= llA2aMax, a v-call iff llA2aMax
 *                     > 0; without one no pair is LL).  sendLL / recvLL[nRanks]
 *                     = the pair bit of each direction; stores / polls = with
 *                     a launch nRanks - 1 ranges of 4 words {peer, part (0 data,
 *                     -1 the zero arrival token), first line, end line}: what
 *                     this rank writes into its slot at `peer` and reads from
 *                     `peer`'s slot in its own buffer; resSends / resRecvs
 *                     [<= nRanks] = the peers whose send / recv stays on the
 *                     p2p FIFOs, in peer order.
 *   vcclCommA2aStats   cumulative: LL all-to-all launches, and the sends + recvs
 *                     (2 nRanks per call, the self block included) of this
 *                     comm's all-to-alls that went by LL / to the p2p FIFOs.
 *   vcclCommSetA2aThreshold  re-derives the per-pair limit on a live comm from
 *                     `bytes` (as VCCL_LL_A2A_THRESHOLD at init); *effective
 *                     (may be NULL) = the result.  A tuning / measurement knob:
 *                     every rank must call it alike, outside a group.
 *   vcclDirectA2aMax   a comm's VCCL_DIRECT_A2A_THRESHOLD (bytes per ordered pair
 *                     of an ncclAllToAll(v); negative: read it from the
 *                     environment; default 0 = off) as it takes effect (host
 *                     only): clamped to what one inbox region
 *                     holds ((regionBytes - 16) rounded down to 16 bytes), 0
 *                     without mapped inboxes (regionBytes 0), with Direct
 *                     excluded, with a net peer, below 2 or above 8 ranks, or
 *                     without point-to-point connections.
 *   vcclDirectA2aPlan  vcclLLA2aPlan's three-way successor: how one call splits
 *                     on a comm whose effective limits are llA2aMax and
 *                     directA2aMax (host only).  The ordered pair of B bytes is
 *                     an LL pair as above; else a direct pair iff directA2aMax
 *                     > 0 and B <= directA2aMax (B = 0 included); else a FIFO
 *                     pair.  *llLaunch as vcclLLA2aPlan's *launch; *directLaunch
 *                     = a uniform call without an LL launch iff 0 < B <=
 *                     directA2aMax, a v-call iff directA2aMax > 0 (every rank
 *                     launches, pairs or not); a path without its launch takes
 *                     no pair.  sendPath / recvPath[nRanks] = 0 FIFO, 1 LL, 2
 *                     direct.  *nBlocks / *blkBytes = the direct launch's grid
 *                     and block length (0 without one), the same on every rank
 *                     of a call: from M = B (uniform) or directA2aMax (v),
 *                     ceil(M / 16 KiB) clamped by maxCTAs / minCTAs, then by
 *                     directMaxBlocks and 128; blkBytes = ceil(M / blocks)
 *                     rounded up to 16.  resSends / resRecvs [<= nRanks] = the
 *                     FIFO peers in peer order.  With directA2aMax 0 the LL
 *                     bits, *llLaunch and the residuals are vcclLLA2aPlan's.
 *   vcclCommA2aStatsEx vcclCommA2aStats plus the direct path: direct launches
 *                     and the sends + recvs that went through the inbox (the
 *                     LL and FIFO counts are those paths' alone in both).
 *   vcclCommSetDirectA2aThreshold  vcclCommSetA2aThreshold for the direct
 *                     limit (as VCCL_DIRECT_A2A_THRESHOLD at init).
 *   vcclAlgoSelection  how NCCL_ALGO / NCCL_PROTO strings select paths (the
 *                     reference's parseList, graph/tuning.cc:53-116: comma
 *                     lists, a leading '^' excludes): *force = 0 automatic,
 *                     1 SIMPLE ring, 2 LL, 3 direct, 4 LL128 ring; *allowed =
 *                     bit 0 LL, bit 1 LL128, bit 2 SIMPLE, bit 3 direct.
 *                     ncclInvalidUsage for an unknown name, as at init.
 *   vcclCommSetup      everything initialisation decides before it touches
 *                     the GPU, for given ranks and environment: the channel
 *                     count, step / slot, thresholds, buffer sizes, net peers,
 *                     shared-GPU caps, ring tables (see its declaration).
 */
#ifndef VCCL_EXT_H_
#define VCCL_EXT_H_
#include <stddef.h>
#include <stdint.h>

#include "nccl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  vcclCollAllReduce = 0,
  vcclCollReduceScatter = 1,
  vcclCollAllGather = 2,
  vcclCollBroadcast = 3,
  vcclCollReduce = 4
} vcclColl_t;
typedef enum {
  vcclAlgoRing = 0,     /* SIMPLE ring over arc-balanced ring sets */
  vcclAlgoLL = 1,       /* one-hop LL: all-reduce (chain-tree fold), RS / AG, opt-in broadcast / reduce
                           (the opt-in LL and direct all-to-alls are per pair, not a vcclAlgo_t:
                           vcclCommA2aStatsEx) */
  vcclAlgoDirect = 2,   /* direct over the full mesh: two-shot all-reduce, one-hop RS / AG, opt-in
                           two-hop broadcast (scatter + all-gather) / reduce (reduce-scatter + gather) */
  vcclAlgoOneRank = 3,  /* nRanks == 1: copy / PreMulSum kernel */
  vcclAlgoLL128 = 4     /* ring over LL128 FIFOs (64-byte lines by default, in-line flags) */
} vcclAlgo_t;

ncclResult_t vcclCommCollAlgo(ncclComm_t comm, int coll, size_t count, ncclDataType_t datatype,
                              int* algo);
ncclResult_t vcclCommSetAlgo(ncclComm_t comm, int algo);
/* The vcclAlgo_t every call of a group would take on this comm: the path of
 * its 4x aggregate in VCCL's plan (see vcclGroupPlanEx); nothing launched.
 * colls / counts / datatypes / ops as in vcclGroupPlan. */
ncclResult_t vcclCommGroupAlgos(ncclComm_t comm, int nCalls, const int* colls, const size_t* counts,
                                const int* datatypes, const int* ops, int* algos);
ncclResult_t vcclCommLaunchStats(ncclComm_t comm, unsigned long long* collectives,
                                 unsigned long long* fusedLaunches);
ncclResult_t vcclCommRingTrace(ncclComm_t comm, void* hostBuf, size_t bytes, int* nChannels, int* cap);
ncclResult_t vcclCommNetStats(ncclComm_t comm, uint64_t* bytesSent, uint64_t* bytesReceived,
                              int* connections);
ncclResult_t vcclCommSetFences(ncclComm_t comm, int useFences);
ncclResult_t vcclCommSetRingWave(ncclComm_t comm, int perWave, unsigned long long* waveLaunches);
ncclResult_t vcclCommDebugSetEpochs(ncclComm_t comm, uint32_t llEpoch, uint32_t directEpoch);
ncclResult_t vcclRingPartition(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                               int nChannels, int proto, size_t stepBytes, int nThreads,
                               int64_t* out);
ncclResult_t vcclRingChunkOf(size_t count, ncclDataType_t datatype, int nRanks, int nChannels,
                             size_t slotBytes, int nThreads, size_t i, int64_t* out);
/* The ring set of an nRanks communicator: orders[k * nRanks + i] = the rank
 * at position i of ring k (channel c runs on ring c mod nRings). */
ncclResult_t vcclRingOrders(int nRanks, int maxRings, int* orders, int* nRings);
ncclResult_t vcclGroupPlan(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                           const int* ops, int nRanks, int nChannels, size_t stepBytes, int nThreads,
                           int* order, int* planOf, int64_t* cbd);
ncclResult_t vcclGroupPlanEx(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                             const int* ops, int nRanks, int nChannels, const int64_t* geometry,
                             const int64_t* policy, int* algos, int* order, int* planOf, int64_t* cbd);
ncclResult_t vcclAlgoSelection(const char* algo, const char* proto, int* force, int* allowed);
ncclResult_t vcclRootedAlgo(int coll, size_t count, ncclDataType_t datatype, int nRanks, const int64_t* policy,
                            int64_t threshold, int llAllowed, int anyNet, int64_t* effective, int* algo);
ncclResult_t vcclRootedAlgoEx(int coll, size_t count, ncclDataType_t datatype, int nRanks, const int64_t* policy,
                              int64_t threshold, int llAllowed, int anyNet, int64_t directThreshold,
                              int directAllowed, int64_t* effective, int64_t* directEffective, int* algo);
ncclResult_t vcclDirectRootedPlan(int coll, int nRanks, int rank, int root, size_t count, ncclDataType_t datatype,
                                  int64_t regionBytes, int chunk, int cap, int64_t* geometry, int* owners,
                                  int* nSteps, int64_t* steps);
ncclResult_t vcclLLRootedPlan(int coll, int nRanks, int rank, int nParts, const int* roots, const size_t* bytes,
                              int64_t linesPerSlot, int cap, int64_t* line0, int* nStores, int64_t* stores,
                              int* nPolls, int64_t* polls);
ncclResult_t vcclLLA2aMax(int64_t threshold, int64_t llSlotBytes, int llAllowed, int anyNet, int nRanks,
                          int hasP2p, int64_t* effective);
ncclResult_t vcclLLA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* recvBytes, int uniform,
                           int64_t llA2aMax, int64_t linesPerSlot, int* sendLL, int* recvLL, int* launch,
                           int64_t* stores, int64_t* polls, int* nResSends, int* resSends, int* nResRecvs,
                           int* resRecvs);
ncclResult_t vcclCommA2aStats(ncclComm_t comm, unsigned long long* llLaunches, unsigned long long* llPairs,
                              unsigned long long* fifoPairs);
ncclResult_t vcclCommSetA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective);
ncclResult_t vcclDirectA2aMax(int64_t threshold, int64_t regionBytes, int directAllowed, int anyNet, int nRanks,
                              int hasP2p, int64_t* effective);
ncclResult_t vcclDirectA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* recvBytes, int uniform,
                               int64_t llA2aMax, int64_t directA2aMax, int64_t linesPerSlot, int minCTAs,
                               int maxCTAs, int directMaxBlocks, int* sendPath, int* recvPath, int* llLaunch,
                               int* directLaunch, int* nBlocks, int64_t* blkBytes, int* nResSends, int* resSends,
                               int* nResRecvs, int* resRecvs);
ncclResult_t vcclCommA2aStatsEx(ncclComm_t comm, unsigned long long* llLaunches, unsigned long long* llPairs,
                                unsigned long long* directLaunches, unsigned long long* directPairs,
                                unsigned long long* fifoPairs);
ncclResult_t vcclCommSetDirectA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective);
/* Zero-copy direct all-reduce / reduce-scatter / all-gather over
 * ncclCommRegister'ed buffers (opt-in: VCCL_REG_THRESHOLD=<bytes> at init,
 * default 0 = off).
 *   vcclRegMax       the threshold as a comm takes it (threshold < 0: from the
 *                    environment): 0 without mapped inboxes (inbox), with
 *                    Direct excluded by NCCL_ALGO, with a peer behind the net
 *                    proxy, or with fewer than 2 / more than 8 ranks.
 *   vcclRegEligible  whether a call launches the negotiating kernel: effective
 *                    > 0, coll 0 / 1 / 2, groupCalls (the collectives of the
 *                    call's comm in its group; 0 or 1 alone) <= 1, and at
 *                    least `effective` bytes (all-reduce count * size, reduce-
 *                    scatter / all-gather nRanks * count * size).
 *   vcclRegPlan      the ordered steps of one zero-copy launch as `rank` runs
 *                    it on nBlocks workgroups (the staged direct grid of the
 *                    call): steps[8 k ..] = kind (0 post, 1 wait, 2 read-fold,
 *                    3 read-copy), epoch (0 negotiate, 1 data), phase, peer,
 *                    the peer's buffer read (0 sendbuff, 1 recvbuff), its byte
 *                    offset, the byte offset in my recvbuff, bytes — in the
 *                    kernel's order; every write is to the rank's own recvbuff.
 *                    *blkElts: elements (an all-gather: bytes) of a shard one
 *                    workgroup moves.  ncclInvalidArgument when cap < *nSteps.
 *   vcclRegTable*    the registration table on its own (no comm, no GPU): 32
 *                    entries; Insert hands out the lowest free entry (*entry =
 *                    -1 when full: refused, not an error) and its generation
 *                    (odd = live; +1 on insert, +1 on removal); Find gives the
 *                    lowest live entry holding the whole of [addr, addr +
 *                    bytes) and the offset in it (*entry = -1: none); Remove
 *                    frees a live entry (ncclInvalidArgument otherwise).
 *   vcclCommRegStats  synchronises the device, then: eligible launches, zero-
 *                    copy outcomes, fallback outcomes (device-resident, so
 *                    graph replays count), this rank's live registrations and
 *                    the peers' ranges it has imported.  All 0 on a comm
 *                    without a registry.
 *   vcclCommSetRegThreshold  the threshold for later calls; every rank calls
 *                    it alike, outside a group.  A comm initialised with neither
 *                    VCCL_REG_THRESHOLD nor VCCL_REG_A2A_THRESHOLD has no
 *                    registry: *effective stays 0. */
typedef struct vcclRegTable vcclRegTable_t;
ncclResult_t vcclRegMax(int64_t threshold, int inbox, int directAllowed, int anyNet, int nRanks, int64_t* effective);
ncclResult_t vcclRegEligible(int coll, size_t count, ncclDataType_t datatype, int nRanks, int64_t effective,
                             int groupCalls, int* eligible);
ncclResult_t vcclRegPlan(int coll, size_t count, ncclDataType_t datatype, int nRanks, int rank, int nBlocks,
                         int64_t* blkElts, int cap, int* nSteps, int64_t* steps);
ncclResult_t vcclRegTableNew(vcclRegTable_t** table);
ncclResult_t vcclRegTableInsert(vcclRegTable_t* table, uint64_t addr, size_t bytes, int* entry,
                                uint32_t* generation);
ncclResult_t vcclRegTableFind(const vcclRegTable_t* table, uint64_t addr, size_t bytes, int* entry,
                              uint64_t* offset, uint32_t* generation);
ncclResult_t vcclRegTableRemove(vcclRegTable_t* table, int entry);
ncclResult_t vcclRegTableFree(vcclRegTable_t* table);
ncclResult_t vcclCommRegStats(ncclComm_t comm, unsigned long long* launches, unsigned long long* zeroCopy,
                              unsigned long long* fallback, int* liveEntries, int* imported);
ncclResult_t vcclCommSetRegThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective);
/* Zero-copy ncclAllToAll / ncclAllToAllv over ncclCommRegister'ed send buffers
 * (opt-in: VCCL_REG_A2A_THRESHOLD, bytes per ordered pair, default 0 = off;
 * DESIGN.md 4.15).  Only sendbuff needs registering.
 *   vcclRegA2aMax    the threshold as a comm takes it (threshold < 0: from the
 *                    environment): 0 wherever vcclRegMax gives 0, without
 *                    point-to-point connections (hasP2p = 0: the fallback needs
 *                    the FIFOs), or when a rank failed to create its registry
 *                    (allRegistries = 0).
 *   vcclRegA2aEligible  whether the all-to-all that has `index` eligible ones
 *                    of its comm before it in its group launches the
 *                    negotiating kernel: effective > 0, index < 8, and a
 *                    uniform call of pairBytes >= effective or any v-call.
 *   vcclRegA2aPlan   one launch as `rank` runs it.  sendBytes / sendOff: the
 *                    nRanks x nRanks matrices, row r rank r's bytes and byte
 *                    offsets in its sendbuff per peer; recvOff: this rank's
 *                    nRanks receive offsets.  *nBlocks: the grid.  steps[8 *
 *                    cap]: kind (0 post, 1 wait, 2 vote, 3 pull, 4 self copy),
 *                    epoch, phase, peer, the byte offset in the peer's
 *                    sendbuff, the byte offset in my recvbuff, bytes, and the
 *                    slice length (workgroup b moves bytes [b * slice, (b + 1)
 *                    * slice) of the block) — in the kernel's order; with the
 *                    verdict 0 the launch ends after epoch 0.
 *                    ncclInvalidArgument when cap < *nSteps.
 *   vcclCommRegA2aStats  synchronises the device, then: eligible launches,
 *                    zero-copy outcomes, fallback outcomes (device-resident,
 *                    so graph replays count).  All 0 without a registry.
 *   vcclCommSetRegA2aThreshold  the threshold for later calls; every rank
 *                    calls it alike, outside a group.  A comm initialised with
 *                    neither VCCL_REG_THRESHOLD nor VCCL_REG_A2A_THRESHOLD has
 *                    no registry: *effective stays 0. */
ncclResult_t vcclRegA2aMax(int64_t threshold, int inbox, int directAllowed, int anyNet, int nRanks, int hasP2p,
                           int allRegistries, int64_t* effective);
ncclResult_t vcclRegA2aEligible(int uniform, size_t pairBytes, int64_t effective, int index, int* eligible);
ncclResult_t vcclRegA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* sendOff,
                            const size_t* recvOff, int uniform, int minCTAs, int maxCTAs, int directMaxBlocks,
                            int* nBlocks, int cap, int* nSteps, int64_t* steps);
ncclResult_t vcclCommRegA2aStats(ncclComm_t comm, unsigned long long* launches, unsigned long long* zeroCopy,
                                 unsigned long long* fallback);
ncclResult_t vcclCommSetRegA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective);
/* Zero-copy ncclBroadcast / ncclBcast / ncclReduce over ncclCommRegister'ed
 * buffers (opt-in: VCCL_REG_ROOTED_THRESHOLD=<bytes> at init, default 0 = off;
 * DESIGN.md 4.16).  A broadcast needs the root's sendbuff and (more than 2
 * ranks) the non-roots' recvbuffs registered, a reduce every rank's sendbuff.
 *   vcclRegRootedMax  the threshold as a comm takes it (threshold < 0: from the
 *                    environment): 0 wherever vcclRegMax gives 0, or when a rank
 *                    failed to create its registry (allRegistries = 0).  No
 *                    upper clamp.
 *   vcclRegRootedEligible  whether a call launches the negotiating kernel:
 *                    effective > 0, coll 3 (broadcast) or 4 (reduce; any other
 *                    is ncclInvalidArgument), groupCalls <= 1, and count * size
 *                    >= effective.  vcclRegEligible is untouched: it refuses
 *                    both collectives.
 *   vcclRegRootedPlan  the ordered steps of one launch as `rank` runs it on
 *                    nBlocks workgroups, regionBytes per inbox region: steps[8 k
 *                    ..] = kind (0 post, 1 wait, 2 read-fold, 3 read-copy, 4
 *                    store into region (1, me) of the root, 5 collect region
 *                    (1, peer)), epoch (0 negotiate; broadcast: 1 data; reduce:
 *                    1 + c for chunk c of the staged geometry), phase, peer,
 *                    the peer's buffer read (0 sendbuff, 1 recvbuff), its byte
 *                    offset, the byte offset in my recvbuff (kind 2 on a
 *                    non-root owner: -1, the fold lands where the kind-4 step
 *                    behind it says; kinds 4 / 5: the shard's user offset),
 *                    bytes — in the kernel's order.  *blkElts: the bytes of a
 *                    shard one workgroup moves in the zero-copy broadcast (a
 *                    reduce: 0, its blocks are the staged ones); *chunkElts,
 *                    *nChunks: the reduce's staged chunking (broadcast: the
 *                    whole count, 1).  ncclInvalidArgument when cap < *nSteps
 *                    (*nSteps is set first).
 *   vcclCommRegRootedStats  synchronises the device, then: eligible launches,
 *                    zero-copy outcomes, fallback outcomes — counters of their
 *                    own (device-resident, so graph replays count); rooted calls
 *                    never move vcclCommRegStats.  All 0 without a registry.
 *   vcclCommSetRegRootedThreshold  the threshold for later calls; every rank
 *                    calls it alike, outside a group.  A comm initialised with
 *                    none of the three VCCL_REG_*THRESHOLD variables has no
 *                    registry: *effective stays 0. */
ncclResult_t vcclRegRootedMax(int64_t threshold, int inbox, int directAllowed, int anyNet, int nRanks,
                              int allRegistries, int64_t* effective);
ncclResult_t vcclRegRootedEligible(int coll, size_t count, ncclDataType_t datatype, int64_t effective, int groupCalls,
                                   int* eligible);
ncclResult_t vcclRegRootedPlan(int coll, size_t count, ncclDataType_t datatype, int nRanks, int rank, int root,
                               size_t regionBytes, int nBlocks, int64_t* blkElts, int64_t* chunkElts, int* nChunks,
                               int cap, int* nSteps, int64_t* steps);
ncclResult_t vcclCommRegRootedStats(ncclComm_t comm, unsigned long long* launches, unsigned long long* zeroCopy,
                                    unsigned long long* fallback);
ncclResult_t vcclCommSetRegRootedThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective);
/* What initialisation decides for rank `rank` of an nRanks communicator with
 * CTA bounds minCTAs / maxCTAs (a comm's defaults: 1 / 128), from the
 * environment as at init and each rank's identity pid[r], hostHash[r],
 * busId[r], cuCount[r] (host only, nothing allocated).  Outputs:
 *   setup[19]  nChannels, stepBytes, slotBytes, nThreads, algoForce,
 *              algoAllowed, llMaxBytes, llLines, llRsAgMaxBytes,
 *              directMaxBytes, directRsAgMaxBytes, directMaxBlocks,
 *              dRegionBytes, ll128StepBytes, ll128Threads, ll128SlotBytes,
 *              ll128MinBytes, ll128MaxBytes, shareBlockCap
 *   sizes[5]   bytes of the FIFO, flag, LL, direct inbox and LL128 buffers
 *              (0: not allocated)
 *   flags[3]   a peer is reached through the net proxy; LL128 buffers are
 *              wanted; the local LL128 buffer is dropped again (net)
 *   netPeer[nRanks]           1 = reached through the net proxy
 *   llChain[min(nRanks, 8)]   the LL fold chain (VCCL_LL_CHAIN)
 *   ring[3]    (may be NULL) ring position, next and previous rank of `rank`
 *              on channel `channel` (0 <= channel < nChannels; the count is
 *              known only once the setup has run, so a refusal below comes
 *              before ncclInvalidArgument for a channel out of range)
 *   ringTables[129]  (may be NULL) nRings, rsOrder[8][8], ringAt[8][8] of the
 *              device communicator
 * Returns what init would for these inputs: ncclInvalidUsage for an unknown
 * NCCL_ALGO / NCCL_PROTO name, two ranks on one GPU, more ranks of one process
 * on a GPU than hardware queues, or a VCCL_LL_CHAIN that is no permutation. */
ncclResult_t vcclCommSetup(int nRanks, int rank, int minCTAs, int maxCTAs, const int* pid,
                           const uint64_t* hostHash, const int64_t* busId, const int* cuCount,
                           int64_t* setup, int64_t* sizes, int* flags, int* netPeer, int* llChain,
                           int channel, int* ring, int* ringTables);

/* The plan of one rank's grouped ncclSend / ncclRecv calls on the per-peer
 * connections (host only, nothing launched).  Calls in call
 * order: kinds[i] 0 send / 1 recv, peers[i], bytes[i], buffs[i] the buffer's
 * address (NULL: all distinct; a self send and recv on one address need no
 * copy).  parts (1..8), minPartBytes (>= 256) and stepBytes (>= 4096, a
 * multiple of 512) are the comm-wide constants; gMin / gCap bound the
 * workgroups per direction (gCap <= 0: one per connection in use); a launch
 * carries at most maxWorks (1..120) items.  *nItems = the work items, *nWgs
 * (may be NULL) = workgroups per direction (send workgroups [0, nWgs), recv
 * workgroups [nWgs, 2 nWgs)); items[12 k ..] = launch, workgroup, kind (0
 * send, 1 recv, 2 local copy), sweep, round, part, peer, call, second call (a
 * copy's recv, else -1), byte offset in the message, bytes, FIFO steps — in
 * execution order.  ncclInvalidUsage: a send to self without its recv of the
 * same length, or the reverse; ncclInvalidArgument also when cap < *nItems. */
ncclResult_t vcclP2pPlan(int rank, int nRanks, int nCalls, const int* kinds, const int* peers,
                         const size_t* bytes, const uint64_t* buffs, int parts, size_t minPartBytes,
                         size_t stepBytes, int gMin, int gCap, int maxWorks, int cap, int* nItems,
                         int* nWgs, int64_t* items);

#ifdef __cplusplus
}
#endif
#endif /* VCCL_EXT_H_ */
