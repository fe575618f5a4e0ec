// The communicator's setup as arithmetic (setup.h): ring sets, NCCL_ALGO /
// NCCL_PROTO selection, the channel model and its clamps, FIFO geometry, path
// thresholds, buffer sizes, what the peer table caps or refuses, and the ring
// tables of a rank.  Nothing here touches the GPU, a communicator or the
// bootstrap: init.cc applies the results; vcclCommSetup exports them.
#include "setup.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../../include/vccl_ext.h"
#include "../device/coll_types.hpp"
#include "../device/ring_launch.hpp"  // kRingMaxThreads
#include "core.h"                     // VWARN / VINFO / param_int
#include "plan.h"                     // ll_rooted_max, direct_rooted_max, ll_a2a_max, direct_a2a_max

namespace vccl {

// Walecki's decomposition of the complete graph on an odd number of vertices
// n = 2m + 1 into m edge-disjoint Hamiltonian cycles: vertex n-1 (the hub)
// followed by the zigzag k, k+1, k-1, k+2, k-2, ... over 0..2m-1 (mod 2m),
// k = 0..m-1.  Each cycle run in both directions gives n-1 arc-disjoint
// directed rings that use every xGMI link once per direction.
static std::vector<std::vector<int>> walecki_rings(int n) {
  const int m = (n - 1) / 2, h = 2 * m;
  std::vector<std::vector<int>> out;
  for (int k = 0; k < m; k++) {
    std::vector<int> cyc{n - 1, k};
    for (int j = 1; (int)cyc.size() < n; j++) {
      cyc.push_back(((k + j) % h + h) % h);
      if ((int)cyc.size() < n) cyc.push_back(((k - j) % h + h) % h);
    }
    out.push_back(cyc);
    std::vector<int> rev{cyc[0]};
    for (int i = n - 1; i >= 1; i--) rev.push_back(cyc[i]);
    out.push_back(rev);
  }
  // rotate each ring to start at rank 0 (cosmetic: a ring is a cycle)
  for (auto& r : out) std::rotate(r.begin(), std::find(r.begin(), r.end(), 0), r.end());
  return out;
}

// Ring sets over the fully connected xGMI mesh (SURVEY.md Appendix D,
// verified by tests/test_ring_schedule.py):
//   8 GPUs: 7 arc-disjoint directed Hamiltonian cycles (every link carries
//           one ring per direction);
//   4 GPUs: all 6 directed Hamiltonian cycles (every arc in exactly 2: no
//           arc-disjoint decomposition exists);
//   odd n (3, 5, 7): Walecki's n-1 arc-disjoint directed rings;
//   6 GPUs: two edge-disjoint Hamiltonian cycles, both directions (4 of each
//           rank's 5 links; K6 has no directed Hamiltonian decomposition);
//   2 GPUs: the single ring.
std::vector<std::vector<int>> ring_orders(int n) {
  if (n == 8)
    return {{0, 1, 2, 3, 4, 5, 6, 7}, {0, 2, 1, 3, 5, 4, 7, 6}, {0, 3, 1, 4, 6, 2, 7, 5},
            {0, 4, 1, 5, 7, 2, 6, 3}, {0, 5, 3, 6, 1, 7, 4, 2}, {0, 6, 5, 2, 4, 3, 7, 1},
            {0, 7, 3, 2, 5, 1, 6, 4}};
  if (n == 4)
    return {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1}};
  if (n == 6)
    return {{0, 1, 2, 3, 4, 5}, {0, 5, 4, 3, 2, 1}, {0, 2, 4, 1, 5, 3}, {0, 3, 5, 1, 4, 2}};
  if (n >= 3 && n % 2 == 1 && n - 1 <= kOrderMaxRings) return walecki_rings(n);
  std::vector<int> id(n);
  for (int i = 0; i < n; i++) id[i] = i;
  return {id};
}

// NCCL_ALGO / NCCL_PROTO (read once at init): the reference's parseList
// (graph/tuning.cc:53-116) — a comma list of names, case-insensitive, a
// leading '^' enables everything but the listed ones; per-collective
// "func:list" entries after a ';' are not supported here (WARNed and
// ignored).  Unknown names, or lists that leave no protocol or no algorithm
// at all, fail init with ncclInvalidUsage.  Paths: the one-hop LL
// all-reduce (protocol LL, algorithm Tree: it restates VCCL's chain-tree LL
// fold), the one-hop LL reduce-scatter / all-gather (protocol LL, algorithm
// Tree or Ring: they restate VCCL's ring-LL fold), the LL128 ring, the SIMPLE
// ring, and the direct path (algorithm "Direct", an extension; allowed only
// while NCCL_ALGO is unset or lists it).  A path is forced when it is the
// only one the lists leave; otherwise the excluded ones are dropped from the
// automatic choice.  A pair the reference accepts but no path here serves
// (e.g. Tree with Simple: VCCL's SIMPLE tree is out of scope) falls back to
// the SIMPLE ring, or the LL128 ring when Simple is excluded, with a WARN
// (ADVICE r4, r5); with neither allowed it fails (ncclInvalidUsage).
enum { kAllowLL = 1, kAllowLL128 = 2, kAllowSimple = 4, kAllowDirect = 8, kAllowLLRsAg = 16 };
static ncclResult_t parse_name_list(const char* env, const char* str, const char* const* names, int nNames,
                                    unsigned* mask) {
  *mask = (1u << nNames) - 1;
  if (!str || !*str) return ncclSuccess;
  std::string s(str);
  const size_t semi = s.find(';');
  if (semi != std::string::npos) {
    VWARN("%s=%s: per-collective entries are not supported, using \"%s\"", env, str, s.substr(0, semi).c_str());
    s = s.substr(0, semi);
  }
  if (s.find(':') != std::string::npos) {
    VWARN("%s=%s: per-collective entries are not supported, ignored", env, str);
    return ncclSuccess;
  }
  bool exclude = false;
  if (!s.empty() && s[0] == '^') {
    exclude = true;
    s = s.substr(1);
  }
  unsigned listed = 0;
  size_t pos = 0;
  while (pos <= s.size()) {
    size_t comma = s.find(',', pos);
    if (comma == std::string::npos) comma = s.size();
    const std::string tok = s.substr(pos, comma - pos);
    pos = comma + 1;
    if (tok.empty()) continue;
    int k = 0;
    while (k < nNames && strcasecmp(tok.c_str(), names[k]) != 0) k++;
    if (k == nNames) {
      VWARN("Unrecognized element token \"%s\" when parsing %s=\"%s\"", tok.c_str(), env, str);
      return ncclInvalidUsage;
    }
    listed |= 1u << k;
  }
  *mask = exclude ? ((1u << nNames) - 1) & ~listed : listed;
  return ncclSuccess;
}
ncclResult_t algo_proto_select(const char* algo, const char* proto, int* force, int* allowed) {
  static const char* const kProtos[] = {"LL", "LL128", "Simple"};
  static const char* const kAlgos[] = {"Tree", "Ring", "CollnetDirect", "CollnetChain", "NVLS", "NVLSTree",
                                       "PAT", "Direct"};
  unsigned p = 0, a = 0;
  NCCLCHECK(parse_name_list("NCCL_PROTO", proto, kProtos, 3, &p));
  NCCLCHECK(parse_name_list("NCCL_ALGO", algo, kAlgos, 8, &a));
  if (p == 0 || a == 0) {
    VWARN("NCCL_ALGO=%s / NCCL_PROTO=%s leave no %s", algo ? algo : "", proto ? proto : "",
          p == 0 ? "protocol" : "algorithm");
    return ncclInvalidUsage;
  }
  const bool tree = a & 1, ring = a & 2, direct = a & 0x80;
  // the one-hop LL all-reduce restates VCCL's chain-tree LL fold (Tree), the
  // one-hop LL reduce-scatter / all-gather its ring-LL one (Tree or Ring, as
  // before: VCCL's tree carries no RS / AG); the direct path moves
  // SIMPLE-style bulk copies
  int m = 0;
  if ((p & 1) && tree) m |= kAllowLL | kAllowLLRsAg;
  if ((p & 1) && ring) m |= kAllowLLRsAg;
  if ((p & 2) && ring) m |= kAllowLL128;
  if ((p & 4) && ring) m |= kAllowSimple;
  if ((p & 4) && direct) m |= kAllowDirect;
  if (m == 0) {
    // No path here serves the pair (e.g. Tree + Simple: VCCL's SIMPLE tree is
    // out of scope).  Fall back only to a ring whose protocol the user still
    // allows: the SIMPLE ring, else the LL128 ring; a list that
    // leaves only LL with no LL path for its algorithms is refused.
    const int fb = (p & 4) ? kAllowSimple : (p & 2) ? kAllowLL128 : 0;
    if (!fb) {
      VWARN("NCCL_ALGO=%s / NCCL_PROTO=%s: no path of this library serves that pair with an allowed protocol",
            algo ? algo : "", proto ? proto : "");
      return ncclInvalidUsage;
    }
    VWARN("NCCL_ALGO=%s / NCCL_PROTO=%s: no path of this library serves that pair; using the %s ring",
          algo ? algo : "", proto ? proto : "", fb == kAllowSimple ? "SIMPLE" : "LL128");
    m = fb;
  }
  const int f = m == kAllowDirect ? 3 : m == kAllowLL128 ? 4 : m == kAllowSimple ? 1
                : (m & ~(kAllowLL | kAllowLLRsAg)) == 0 ? 2 : 0;
  *force = f;
  *allowed = m;
  return ncclSuccess;
}

// Channel count: NCCL_NCHANNELS total, else VCCL_CHANNELS_PER_RING x rings,
// by default from a link-bound model, within VCCL's
// MAXCHANNELS of 64 (device.h:62) so that VCCL can run the same geometry:
//   channels per ring = ceil(H * L / (k * R)), at most 64 / rings in all,
// L = 76.8 GB/s per xGMI link and direction (MI355X spec), k = rings
// sharing an arc (2 for the 4-GPU set of all 6 Hamiltonian cycles, else 1),
// R = 40 GB/s, the per-channel rate of the ring step shapes that read the
// own input from HBM (tools/step_probe, profiles/r03l: 36-44 GB/s at 96
// concurrent channels), H = 8 headroom for remote-store latency that no
// single-GPU run can measure (a channel then carries <= 1/8 of its local
// rate at link peak).  2 GPUs: 16; 3: 2 x 16; 4: 6 x 8 = 48; 5, 6: 4 x 16
// = 64; 7: 6 x 10 = 60; 8: 7 x 9 = 63.  The shared-GPU rehearsals, which
// are bound by CUs rather than links, set their counts with the knobs.
static int channel_count(int n, int minCTAs, int maxCTAs) {
  const int nRings = (int)ring_orders(n).size();
  const int arcShare = n == 4 ? 2 : 1;
  const int perRingModel = (int)((8 * 768 + 10 * 40 * arcShare - 1) / (10 * 40 * arcShare));  // ceil(8*76.8/(40k))
  int perRing = (int)param_int("CHANNELS_PER_RING",
                               std::max(1, std::min(perRingModel, kVcclMaxChannels / nRings)));
  int nch = (int)param_int("NCHANNELS", (int64_t)perRing * nRings);
  // minCTAs / maxCTAs bound the channel count (graph/connect.cc:486-490), and
  // so do NCCL_MIN_NCHANNELS / NCCL_MAX_NCHANNELS (legacy MIN_NRINGS /
  // MAX_NRINGS, connect.cc:326-360)
  nch = std::max(minCTAs, std::min(nch, maxCTAs));
  int64_t minNch = param_int("MIN_NRINGS", -2), maxNch = param_int("MAX_NRINGS", -2);
  if (param_int("MIN_NCHANNELS", -2) != -2) minNch = param_int("MIN_NCHANNELS", -2);
  if (param_int("MAX_NCHANNELS", -2) != -2) maxNch = param_int("MAX_NCHANNELS", -2);
  if (maxNch != -2) nch = std::min<int64_t>(nch, std::max<int64_t>(1, maxNch));
  if (minNch > 0) nch = std::max<int64_t>(nch, minNch);
  nch = std::max(1, std::min(nch, kMaxChannels));
  return n > 1 ? nch : 0;
}

// Step = VCCL's FIFO step: NCCL_BUFFSIZE / NCCL_STEPS (init.cc:619-633,
// 4 MiB -> 512 KiB), or VCCL_SLOT_BYTES directly.  It sets VCCL's
// partition and ring chunk (4 steps, cbd_schedule), hence the fold order.
// The FIFO slot (the unit a chunk crosses the FIFO in, one flag hand-off
// each) is the step unless VCCL_SLICE_BYTES sets it apart without touching
// the fold order.  A chunk may span at most kSteps / 2 slots: a recv-send
// step needs free slots while its successor still holds the previous
// step's (the reference's chunkSteps 4 of NCCL_STEPS 8); 8 slots of 256 KiB
// for a 2 MiB chunk deadlock the n = 2 all-reduce (profiles/r03n).
static void step_and_slot(CommSetup* s) {
  const int64_t buffSize = param_int("BUFFSIZE", -2);
  s->stepBytes = (int)param_int("SLOT_BYTES", buffSize > 0 ? buffSize / kSteps : 512 << 10);
  if (s->stepBytes < 4096 || s->stepBytes % 4096 || s->stepBytes > (64 << 20)) {
    VWARN("slot size (NCCL_BUFFSIZE / 8 or VCCL_SLOT_BYTES) must be a multiple of 4096 up to "
          "64 MiB, using 524288");
    s->stepBytes = 512 << 10;
  }
  s->slotBytes = (int)param_int("SLICE_BYTES", s->stepBytes);
  if (s->slotBytes < 4096 || s->slotBytes % 4096 || s->slotBytes > (64 << 20) ||
      (int64_t)s->slotBytes * (kSteps / 2) < (int64_t)s->stepBytes * 4) {
    VWARN("VCCL_SLICE_BYTES must be a multiple of 4096 up to 64 MiB and hold a ring chunk (4 steps of %d B) "
          "in %d slots, using the step", s->stepBytes, kSteps / 2);
    s->slotBytes = s->stepBytes;
  }
}

// The one-hop paths of an n > 1 comm: thresholds, LL slot and inbox region.
static void one_hop_paths(int n, CommSetup* s, SetupSizes* z) {
  // LL buffers for the one-shot small-bucket all-reduce.
  // LL vs direct crossover (profiles/r01_sweep_algos_*.log): LL pays one
  // hop but moves 2(n-1)x the bucket per rank, the direct path two hops
  // and 2(n-1)/n x; LL wins up to ~64 KiB (2 ranks) / ~128 KiB (more).
  s->llMaxBytes = (size_t)param_int("LL_THRESHOLD", n <= 2 ? (64 << 10) : (128 << 10));
  s->llMaxBytes = (s->llMaxBytes + 7) / 8 * 8;
  if (s->llMaxBytes > 0) {
    // Slot capacity: the single-call threshold, or more for group
    // aggregation (VCCL_LL_GROUP_BYTES): a group's run of small all-reduces
    // fills one slot even when their sum is above the single-call
    // threshold — one LL launch still beats one launch per bucket there.
    const int64_t groupBytes = std::max<int64_t>(param_int("LL_GROUP_BYTES", 1 << 20), 0);
    s->llLines = (int)((std::max<int64_t>((int64_t)s->llMaxBytes, groupBytes) + 7) / 8);
    z->llBytes = (size_t)2 * n * s->llLines * 16;
  }
  // Inbox of the direct collectives (direct.hpp): 2 phases x n regions of
  // one shard of a VCCL_DIRECT_CHUNK_BYTES chunk each, plus the epoch
  // flags.  Larger buckets stream through the inbox chunk by chunk.
  // Two-shot direct all-reduce up to VCCL_DIRECT_THRESHOLD (8 MiB from 4
  // ranks), the SIMPLE ring above: the ring, with VCCL's own partition, is
  // the north-star path and keeps VCCL's fold order for large buckets; the
  // direct path's two hops (vs 2(n-1)) matter where the per-hop latency
  // does, i.e. small and mid buckets at n >= 4 (profiles/r02e/lat_n4.log,
  // lat_n8.log).  Above 8 MiB the ring's continuous pipeline wins (4 ranks:
  // 16 MiB 111 vs 121 us, 64 MiB 330 vs 504 us, profiles/r03g/lat_n4.log).
  // At n = 2 the ring IS two hops and its channels beat the direct path at
  // every size above LL (profiles/r02/lat_n2.log, r03r: 1 GiB ring 655 vs
  // direct ~220 GB/s).
  s->directMaxBytes = n <= kDirectMaxRanks
                          ? (size_t)param_int("DIRECT_THRESHOLD", n >= 4 ? (int64_t)8 << 20 : 0)
                          : 0;
  s->directMaxBlocks = (int)std::max<int64_t>(
      1, std::min<int64_t>(param_int("DIRECT_MAX_BLOCKS", 64), kDirectMaxBlocks));
  // Reduce-scatter / all-gather (the whole bucket, n blocks): one-hop LL
  // while one rank's block fits a slot and the bucket is at most n x the
  // all-reduce LL threshold (each rank sends 2(n-1)/n x the bucket as LL
  // lines, vs 2(n-1) x for the LL all-reduce), the one-hop direct path up
  // to VCCL_DIRECT_RSAG_THRESHOLD, the SIMPLE ring above.
  s->llRsAgMaxBytes = n <= kOrderMaxRanks && s->llMaxBytes > 0
                          ? (size_t)param_int("LL_RSAG_THRESHOLD", (int64_t)n * s->llMaxBytes)
                          : 0;
  // (The one-hop path saves n-2 hops over the ring: nothing at n = 2, and
  // the 2-rank rehearsal has the ring ahead at 1-8 MiB, profiles/r02h; at
  // n = 8 the one-hop paths lead at <= 1 MiB, profiles/r02e/lat_n8.log.)
  s->directRsAgMaxBytes =
      n <= kDirectMaxRanks
          ? (size_t)param_int("DIRECT_RSAG_THRESHOLD", n >= 4 ? (int64_t)8 << 20 : 0) : 0;
  // The inbox exists whenever the mesh allows the direct path, so that
  // NCCL_ALGO=Direct can take any bucket even where no size defaults to it.
  if (n <= kDirectMaxRanks) {
    const int64_t chunk = std::max<int64_t>(param_int("DIRECT_CHUNK_BYTES", 16 << 20), 64 << 10);
    s->dRegionBytes = (chunk + n - 1) / n / 256 * 256 + 256;
    z->inboxBytes = (size_t)kDirectInboxRegions * n * s->dRegionBytes;
  } else {
    s->directMaxBytes = s->directRsAgMaxBytes = 0;
  }
}

// LL128 ring buffers: with NCCL_PROTO=LL128, or VCCL_LL128=1 (the
// automatic window VCCL_LL128_MIN..MAX, default 64 KiB - 1 MiB, inside
// the range VCCL's tuner gives LL128, enqueue.cc:2032).  VCCL's LL128 step
// (NCCL_LL128_BUFFSIZE / 8, default 120 x 640 x 8 x 8 B / 8 = 614,400 B)
// carries 15/16 of it as data, rounded to the 1,920 B grain: 576,000 B per
// chunk; the slot holds that many data bytes in lines of kLL128LineBytes
// (rounds of 1 KiB: 643 with the default 64-byte line, 600 with a 128-byte one).
// (VCCL_LL128_ALLOC=1: the buffers only — vcclCommSetAlgo may pick the
// LL128 ring per call, the automatic choice is unchanged)
static void ll128_ring(CommSetup* s, SetupSizes* z) {
  // NCCL_PROTO without SIMPLE but with LL128 (e.g. "LL,LL128"): the LL128
  // ring carries every call LL does not
  const bool ll128Only = (s->algoAllowed & kAllowLL128) && !(s->algoAllowed & kAllowSimple);
  z->wantLL128 = s->algoForce == 4 || ll128Only || param_int("LL128", 0) != 0 ||
                 param_int("LL128_ALLOC", 0) != 0;
  if (!z->wantLL128) return;
  s->ll128StepBytes = std::max<int64_t>(param_int("LL128_BUFFSIZE", 120 * 640 * kSteps * 8) / kSteps, 1920 * 16);
  s->ll128Threads = (int)std::max<int64_t>(param_int("LL128_NTHREADS", 640), 64);
  const int64_t chunk = s->ll128StepBytes / 16 * 15 / 1920 * 1920;
  s->ll128SlotBytes = (chunk + kLL128RoundData - 1) / kLL128RoundData * kLL128RoundWire;
  z->ll128Bytes = (size_t)s->nChannels * kSteps * s->ll128SlotBytes;
  if (ll128Only) {
    s->ll128MinBytes = 0;
    s->ll128MaxBytes = ~(size_t)0;
  } else if (param_int("LL128", 0) != 0 && (s->algoAllowed & kAllowLL128)) {
    s->ll128MinBytes = (size_t)param_int("LL128_MIN", 64 << 10);
    // 1 MiB: the rehearsals have the LL128 ring ahead of the SIMPLE ring
    // up to 256 KiB - 1 MiB and behind at 8 MiB, inside
    // VCCL's own 64 KiB - 8 MiB LL128 range (enqueue.cc:2032)
    s->ll128MaxBytes = (size_t)param_int("LL128_MAX", 1 << 20);
  }
}

// Per-peer point-to-point connections (device/p2p_types.hpp): every rank of a
// 2..8-rank comm holds, per sender and part, kSteps slots of the step.  The
// defaults are the reference's NVLink ones and are unmeasured on xGMI.
static void p2p_connections(int n, CommSetup* s, SetupSizes* z) {
  if (param_int("P2P_BUFFERS", 1) == 0) {
    s->p2pOff = kP2pOffEnv;
    return;
  }
  if (n > kP2pMaxRanks) {
    s->p2pOff = kP2pOffRanks;
    return;
  }
  s->p2pParts = (int)std::max<int64_t>(1, std::min<int64_t>(param_int("P2P_PARTS", 4), kP2pMaxParts));
  int64_t step = param_int("P2P_NVL_CHUNKSIZE", 512 << 10);
  if (step < 4096 || step % 512 || step > (64 << 20)) {
    VWARN("NCCL_P2P_NVL_CHUNKSIZE must be a multiple of 512 from 4096 to 64 MiB, using 524288");
    step = 512 << 10;
  }
  s->p2pStepBytes = (int)step;
  s->p2pMinPartBytes = std::max<int64_t>(256, param_int("P2P_MIN_PART_BYTES", 64 << 10));
  z->p2pBytes = (size_t)n * s->p2pParts * kSteps * slot_stride(s->p2pStepBytes);
  z->p2pFlagBytes = (size_t)n * s->p2pParts * 2 * kFlagStride;
}

ncclResult_t setup_local(int n, int minCTAs, int maxCTAs, CommSetup* s, SetupSizes* z) {
  s->nChannels = channel_count(n, minCTAs, maxCTAs);
  step_and_slot(s);
  NCCLCHECK(algo_proto_select(getenv("NCCL_ALGO"), getenv("NCCL_PROTO"), &s->algoForce, &s->algoAllowed));
  // Threads per ring channel (NCCL_NTHREADS, tuning.cc:198-200): 256 or 512
  // (the ring kernel's launch bound, ring_launch.hpp kRingMaxThreads).
  s->nThreads = (int)param_int("NTHREADS", kRingMaxThreads);
  if (s->nThreads != 256 && s->nThreads != 512) {
    if (s->nThreads != kRingMaxThreads)
      VINFO("NCCL_NTHREADS=%d not supported by the ring kernel, using %d", s->nThreads, kRingMaxThreads);
    s->nThreads = kRingMaxThreads;
  }
  if (n > 1) {
    z->fifoBytes = (size_t)s->nChannels * kSteps * slot_stride(s->slotBytes);
    z->flagBytes = (size_t)s->nChannels * 2 * kFlagStride;
    one_hop_paths(n, s, z);
    ll128_ring(s, z);
    p2p_connections(n, s, z);
  }
  // paths NCCL_ALGO / NCCL_PROTO exclude drop out of the automatic choice
  // (after llRsAgMaxBytes took its default from llMaxBytes; the buffers stay)
  if (!(s->algoAllowed & kAllowLL)) s->llMaxBytes = 0;
  if (!(s->algoAllowed & kAllowLLRsAg)) s->llRsAgMaxBytes = 0;
  if (!(s->algoAllowed & kAllowDirect)) s->directMaxBytes = s->directRsAgMaxBytes = 0;
  // Rooted LL (ncclBroadcast / ncclReduce in one hop): opt-in, off by default —
  // the size where one hop stops winning over xGMI is unmeasured.  The
  // reference runs both on its ring under LL: protocol LL with Tree or Ring.
  s->llRootedMaxBytes = (size_t)ll_rooted_max(param_int("LL_ROOTED_THRESHOLD", 0), (int64_t)s->llLines * 8,
                                              (s->algoAllowed & kAllowLLRsAg) != 0, false, n);
  // Rooted direct (ncclBroadcast / ncclReduce in two hops on every link):
  // opt-in the same way — no one-rank-per-GPU row exists to set a default.
  s->directRootedMaxBytes = (size_t)direct_rooted_max(param_int("DIRECT_ROOTED_THRESHOLD", 0), s->dRegionBytes > 0,
                                                      (s->algoAllowed & kAllowDirect) != 0, false, n);
  // LL all-to-all (the small pairs of ncclAllToAll(v) in one hop): opt-in the
  // same way, bytes per ordered pair; the pairs above it keep the p2p FIFOs
  s->llA2aMaxBytes = ll_a2a_max_of(*s, param_int("LL_A2A_THRESHOLD", 0), n, false, n > 1 && s->p2pOff == kP2pOn);
  // Direct all-to-all (the mid-size pairs, 16-byte payload stores through the
  // inbox): opt-in the same way, bytes per ordered pair, at most one region
  s->directA2aMaxBytes =
      direct_a2a_max_of(*s, param_int("DIRECT_A2A_THRESHOLD", 0), n, false, n > 1 && s->p2pOff == kP2pOn);
  return ncclSuccess;
}

size_t ll_a2a_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool hasP2p) {
  return (size_t)ll_a2a_max(threshold, (int64_t)s.llLines * 8, (s.algoAllowed & kAllowLLRsAg) != 0, anyNet, nRanks,
                            hasP2p);
}

size_t direct_a2a_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool hasP2p) {
  return (size_t)direct_a2a_max(threshold, s.dRegionBytes, (s.algoAllowed & kAllowDirect) != 0, anyNet, nRanks,
                                hasP2p);
}

size_t reg_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool inbox) {
  return (size_t)reg_max(threshold, inbox, (s.algoAllowed & kAllowDirect) != 0, anyNet, nRanks);
}

size_t reg_a2a_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool inbox, bool hasP2p,
                      bool allRegistries) {
  return (size_t)reg_a2a_max(threshold, inbox, (s.algoAllowed & kAllowDirect) != 0, anyNet, nRanks, hasP2p,
                             allRegistries);
}

size_t reg_rooted_max_of(const CommSetup& s, int64_t threshold, int nRanks, bool anyNet, bool inbox,
                         bool allRegistries) {
  return (size_t)reg_rooted_max(threshold, inbox, (s.algoAllowed & kAllowDirect) != 0, anyNet, nRanks, allRegistries);
}

static bool same_gpu(const PeerId& a, const PeerId& b) { return a.hostHash == b.hostHash && a.busId == b.busId; }

ncclResult_t setup_mesh(int rank, const std::vector<PeerId>& peers, CommSetup* s, MeshSetup* m) {
  const int n = (int)peers.size();
  // Transport per peer (the reference's selectTransport, transport.cc:
  // 37-68, reduced to two): xGMI peer memory within the node, the net proxy
  // (proxy.cc) to a peer on another node — or to every peer with
  // VCCL_NET_FORCE=1, which runs the inter-node path on one node.
  const bool netForce = param_int("NET_FORCE", 0) != 0;
  m->netPeer.assign(n, 0);
  m->anyNet = false;
  for (int r = 0; r < n; r++) {
    if (r == rank) continue;
    m->netPeer[r] = netForce || peers[r].hostHash != peers[rank].hostHash;
    m->anyNet |= m->netPeer[r] != 0;
  }
  m->dropLL128 = m->anyNet;
  if (m->anyNet) {
    // LL and the two-shot direct path need every peer's memory mapped
    // (full xGMI mesh): all-reduce takes the ring.  Net channels move
    // through the proxy, a few are enough (NCCL's net defaults use 2-4).
    s->llMaxBytes = s->llRsAgMaxBytes = s->llRootedMaxBytes = s->llA2aMaxBytes = 0;
    s->directMaxBytes = s->directRsAgMaxBytes = s->directRootedMaxBytes = s->directA2aMaxBytes = 0;
    s->ll128MinBytes = s->ll128MaxBytes = 0;
    if (s->algoForce == 4) s->algoForce = 1;  // LL128 lines need the xGMI mesh: SIMPLE
    // ... so no LL128 FIFO is mapped: the local one is dropped too
    // (dropLL128), so that neither the automatic choice nor
    // vcclCommSetAlgo(LL128) can pick a ring whose channels carry no LL128
    // slots
    if (!s->p2pOff) s->p2pOff = kP2pOffNet;  // p2p FIFOs need every peer's memory mapped too
    s->nChannels = std::max(1, std::min(s->nChannels, (int)param_int("NET_NCHANNELS", 8)));
    VINFO("rank %d: inter-node ring through the net proxy, %d channels", rank, s->nChannels);
  }
  // init.cc:732-735: two ranks on one GPU is invalid usage.  The escape hatch
  // exists for protocol tests on a 1-GPU machine only.  Checked over every
  // pair, so every rank fails together.
  if (!param_int("ALLOW_SHARED_DEVICE", 0) && !netForce) {
    for (int q = 0; q < n; q++)
      for (int r = q + 1; r < n; r++)
        if (same_gpu(peers[r], peers[q])) {
          VWARN("Duplicate GPU detected : rank %d and rank %d both on device %lx", q, r, (long)peers[q].busId);
          return ncclInvalidUsage;
        }
  }
  {
    // Ranks sharing a GPU (VCCL_ALLOW_SHARED_DEVICE: rehearsals on fewer GPUs
    // than ranks) spin on each other, so all their ring workgroups must be
    // resident at once: one 512-thread ring workgroup fills a CU (176-232
    // VGPRs), so k ranks on a device get at most 7/8 of its CUs / k channels
    // (e.g. 4 ranks on 256 CUs: 56), the rest left to the other kernels.
    // Computed from the shared peer table, so every rank picks the same
    // count (the partition depends on it); the FIFO was sized for the
    // uncapped count, its tail stays unused.  Real one-rank-per-GPU runs are
    // untouched.
    int share = 1, cus = 1 << 30;
    for (int q = 0; q < n; q++) {
      int k = 0;
      for (int r = 0; r < n; r++) k += same_gpu(peers[r], peers[q]);
      share = std::max(share, k);
      cus = std::min(cus, (int)peers[q].cuCount);
    }
    if (share > 1) {
      const int cap = std::max(1, cus * 7 / 8 / share);
      s->shareBlockCap = cap;  // the LL and direct grids too (launch.cc)
      s->directMaxBlocks = std::min(s->directMaxBlocks, cap);
      if (s->nChannels > cap) {
        VINFO("rank %d: %d ranks share a GPU of %d CUs: %d -> %d ring channels", rank, share, cus,
              s->nChannels, cap);
        s->nChannels = cap;
      }
    }
  }
  {
    // Ranks of this comm that share ONE device inside ONE process (allowed
    // only through VCCL_ALLOW_SHARED_DEVICE) spin on each other, so their
    // kernels must be co-resident.  HIP gives a process GPU_MAX_HW_QUEUES
    // hardware queues (4 by default) and deals streams to them round-robin,
    // one of them taken by the process's first (null / runtime) stream: with
    // more sharing ranks than the remaining queues, two ranks' kernels
    // serialise on one queue and every peer spins until the timeout
    // (profiles/r01_diag_protocol.log).  Refuse that configuration up front.
    // Every rank evaluates every (process, device) group from the same peer
    // table, so all ranks fail together (none is left waiting at the final
    // barrier).
    const char* hq = getenv("GPU_MAX_HW_QUEUES");
    const int hwQueues = hq && atoi(hq) > 0 ? atoi(hq) : 4;
    for (int q = 0; q < n; q++) {
      int sameDev = 0;
      for (int r = 0; r < n; r++) sameDev += peers[r].pid == peers[q].pid && same_gpu(peers[r], peers[q]);
      if (sameDev > 1 && sameDev > hwQueues - 1) {
        VWARN("%d ranks of this communicator share device %lx in one process, but only %d of the "
              "process's %d hardware queues can keep their kernels co-resident",
              sameDev, (long)peers[q].busId, hwQueues - 1, hwQueues);
        return ncclInvalidUsage;
      }
    }
  }
  return ncclSuccess;
}

// reduce-scatter fold order of this rank on each ring (ring_types.hpp)
void ring_tables(const std::vector<std::vector<int>>& rings, int n, int rank, DevComm* dc) {
  dc->nRings = std::min((int)rings.size(), kOrderMaxRings);
  for (int k = 0; k < dc->nRings && n <= kOrderMaxRanks; k++) {
    const auto& ring = rings[k];
    const int pos = (int)(std::find(ring.begin(), ring.end(), rank) - ring.begin());
    for (int j = 0; j < n; j++) dc->rsOrder[k][j] = (int8_t)ring[(pos + 1 + j) % n];
    for (int j = 0; j < n; j++) dc->ringAt[k][j] = (int8_t)ring[j];
  }
}

// LL chain (DevComm::llChain): VCCL_LL_CHAIN="r0,r1,..." (root first), a
// permutation of the ranks, else the identity.  Every rank must pass the
// same order.
ncclResult_t ll_chain(int n, int8_t* chain) {
  for (int j = 0; j < n && j < kOrderMaxRanks; j++) chain[j] = (int8_t)j;
  const char* chainEnv = getenv("VCCL_LL_CHAIN");
  if (!chainEnv || !*chainEnv || n > kOrderMaxRanks) return ncclSuccess;
  std::vector<int> order;
  for (const char* q = chainEnv; *q;) {
    char* end = nullptr;
    const long v = strtol(q, &end, 10);
    if (end == q) break;
    order.push_back((int)v);
    q = *end == ',' ? end + 1 : end;
  }
  std::vector<int> seen(n, 0);
  bool okChain = (int)order.size() == n;
  for (int v : order) okChain = okChain && v >= 0 && v < n && !seen[v]++;
  if (!okChain) {
    VWARN("VCCL_LL_CHAIN=%s is not a permutation of the %d ranks", chainEnv, n);
    return ncclInvalidUsage;
  }
  for (int j = 0; j < n; j++) chain[j] = (int8_t)order[j];
  return ncclSuccess;
}

RingView ring_view(const std::vector<std::vector<int>>& rings, int ch, int rank, int* ringRanks) {
  const auto& ring = rings[ch % rings.size()];
  const int n = (int)ring.size();
  const int pos = (int)(std::find(ring.begin(), ring.end(), rank) - ring.begin());
  if (ringRanks)
    for (int k = 0; k < n; k++) ringRanks[k] = ring[(pos + k) % n];
  return RingView{pos, ring[(pos + 1) % n], ring[(pos + n - 1) % n]};
}

}  // namespace vccl

using namespace vccl;

// vccl_ext.h: the ring set the library uses for nRanks ranks.
VCCL_EXPORT ncclResult_t vcclRingOrders(int nRanks, int maxRings, int* orders, int* nRings) {
  if (nRanks < 1 || nRanks > kMaxRanks || maxRings < 1 || !orders || !nRings) return ncclInvalidArgument;
  const auto rings = ring_orders(nRanks);
  *nRings = (int)rings.size();
  if ((int)rings.size() > maxRings) return ncclInvalidArgument;
  for (size_t k = 0; k < rings.size(); k++)
    for (int i = 0; i < nRanks; i++) orders[k * nRanks + i] = rings[k][i];
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclAlgoSelection(const char* algo, const char* proto, int* force, int* allowed) {
  if (!force || !allowed) return ncclInvalidArgument;
  return algo_proto_select(algo, proto, force, allowed);
}

// vccl_ext.h: what init decides for such a communicator, with no GPU.
VCCL_EXPORT ncclResult_t vcclCommSetup(int nRanks, int rank, int minCTAs, int maxCTAs, const int* pid,
                                       const uint64_t* hostHash, const int64_t* busId, const int* cuCount,
                                       int64_t* setup, int64_t* sizes, int* flags, int* netPeer, int* llChain,
                                       int channel, int* ring, int* ringTables) {
  if (nRanks < 1 || nRanks > kMaxRanks || rank < 0 || rank >= nRanks || !pid || !hostHash || !busId ||
      !cuCount || !setup || !sizes || !flags || !netPeer || !llChain)
    return ncclInvalidArgument;
  CommSetup s;
  SetupSizes z;
  NCCLCHECK(setup_local(nRanks, minCTAs, maxCTAs, &s, &z));
  std::vector<PeerId> peers(nRanks);
  for (int r = 0; r < nRanks; r++) peers[r] = PeerId{pid[r], hostHash[r], busId[r], cu_count_of(cuCount[r])};
  MeshSetup m;
  NCCLCHECK(setup_mesh(rank, peers, &s, &m));
  DevComm dc{};
  const auto rings = ring_orders(nRanks);
  ring_tables(rings, nRanks, rank, &dc);
  NCCLCHECK(ll_chain(nRanks, dc.llChain));
  // the channel range is known only now: a refusal above comes first
  if (ring && (channel < 0 || channel >= s.nChannels)) return ncclInvalidArgument;
  const int64_t words[19] = {
      s.nChannels, s.stepBytes, s.slotBytes, s.nThreads, s.algoForce, s.algoAllowed,
      (int64_t)s.llMaxBytes, s.llLines, (int64_t)s.llRsAgMaxBytes,
      (int64_t)s.directMaxBytes, (int64_t)s.directRsAgMaxBytes, s.directMaxBlocks, s.dRegionBytes,
      s.ll128StepBytes, s.ll128Threads, s.ll128SlotBytes, (int64_t)s.ll128MinBytes, (int64_t)s.ll128MaxBytes,
      s.shareBlockCap};  // CommSetup in declared order
  for (int i = 0; i < 19; i++) setup[i] = words[i];
  const size_t bytes[5] = {z.fifoBytes, z.flagBytes, z.llBytes, z.inboxBytes, z.ll128Bytes};
  for (int i = 0; i < 5; i++) sizes[i] = (int64_t)bytes[i];
  flags[0] = m.anyNet;
  flags[1] = z.wantLL128;
  flags[2] = m.dropLL128;
  for (int r = 0; r < nRanks; r++) netPeer[r] = m.netPeer[r];
  for (int j = 0; j < nRanks && j < kOrderMaxRanks; j++) llChain[j] = dc.llChain[j];
  if (ring) {
    const RingView v = ring_view(rings, channel, rank, nullptr);
    ring[0] = v.pos, ring[1] = v.next, ring[2] = v.prev;
  }
  if (ringTables) {
    ringTables[0] = dc.nRings;
    for (int k = 0; k < kOrderMaxRings; k++)
      for (int j = 0; j < kOrderMaxRanks; j++) {
        ringTables[1 + k * kOrderMaxRanks + j] = dc.rsOrder[k][j];
        ringTables[1 + (kOrderMaxRings + k) * kOrderMaxRanks + j] = dc.ringAt[k][j];
      }
  }
  return ncclSuccess;
}
