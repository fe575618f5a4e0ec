// Host-only exercise of the library's C ABI under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make sanitize`; the reference's ASAN=1 /
// UBSAN=1 build knobs, makefiles/common.mk:98-109).  No GPU call is made:
// the planner exports (vcclGroupPlanEx, vcclRingPartition, vcclRingChunkOf,
// vcclAlgoSelection), the communicator setup (vcclCommSetup) under random
// environments, the registration table (vcclRegTable*) against a reference
// model with the zero-copy threshold, eligibility and step lists, the op
// encoding, error strings and the argument checks that reject bad handles
// before any device work.  Random inputs from a fixed
// seed; prints a summary and exits non-zero on an unexpected result (the
// sanitizers abort on any memory or UB error).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "nccl.h"
#include "vccl_device.h"
#include "vccl_ext.h"

static int g_fail = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__);     \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

int main() {
  std::mt19937_64 rng(20261018);
  auto pick = [&](std::initializer_list<int64_t> v) { return *(v.begin() + rng() % v.size()); };
  const int dts[] = {ncclInt8, ncclUint8, ncclInt32, ncclUint32, ncclInt64, ncclUint64,
                     ncclFloat16, ncclFloat32, ncclFloat64, ncclBfloat16};
  long groups = 0, calls = 0;
  for (int trial = 0; trial < 3000; trial++) {
    const int n = (int)pick({1, 2, 3, 4, 6, 7, 8});
    const int nch = (int)pick({1, 2, 14, 16, 56, 63, 64, 128});
    const int k = 1 + (int)(rng() % 40);
    std::vector<int> colls(k), dt(k), ops(k), algos(k, -1), order(k, -1), planOf(k, -1);
    std::vector<size_t> counts(k);
    for (int i = 0; i < k; i++) {
      colls[i] = (int)(rng() % 5);  // AR, RS, AG, broadcast, reduce
      dt[i] = dts[rng() % 10];
      ops[i] = (int)(rng() % 4);
      counts[i] = (size_t)pick({1, 7, 100, 4096, 65537, 1 << 20, (1 << 22) + 3}) + rng() % 17;
    }
    std::vector<int64_t> cbd(8 * (size_t)k, -1);
    const int64_t geo[4] = {(int64_t)pick({64 << 10, 256 << 10, 512 << 10}), pick({256, 512}),
                            120 * 640 * 8, 640};
    const int64_t ll = pick({0, 64 << 10, 1 << 20});
    const int64_t pol[10] = {pick({0, 0, 1, 2, 3, 4}), pick({0, 1 << 20}), ll, n * ll, pick({0, 1}),
                             64 << 10, pick({0, 1 << 20}), pick({0, 1}), pick({0, 4 << 20, 8 << 20}),
                             pick({0, 64 << 20})};
    const ncclResult_t r = vcclGroupPlanEx(k, colls.data(), counts.data(), dt.data(), ops.data(), n, nch, geo,
                                           (trial & 1) ? pol : nullptr, algos.data(), order.data(),
                                           planOf.data(), cbd.data());
    EXPECT(r == ncclSuccess);
    if (r != ncclSuccess) continue;
    groups++;
    calls += k;
    std::vector<int> seen(k, 0);
    for (int i = 0; i < k; i++) {
      EXPECT(order[i] >= 0 && order[i] < k);
      if (order[i] >= 0 && order[i] < k) seen[order[i]]++;
      EXPECT(planOf[i] >= 0);
      EXPECT(algos[i] == vcclAlgoRing || algos[i] == vcclAlgoLL || algos[i] == vcclAlgoDirect ||
             algos[i] == vcclAlgoLL128);
      const int64_t* c = &cbd[8 * (size_t)i];
      EXPECT(c[0] >= 0 && c[0] <= c[1] && c[1] < nch);
      // the parts cover the call: lo + mid * (channels - 2) + hi (AG in bytes)
      const int64_t nCh = c[1] - c[0] + 1;
      const int64_t cover = nCh == 1 ? c[2] : c[2] + c[3] * (nCh - 2) + c[4];
      const int64_t want = colls[i] == 2 || colls[i] == 3 ? (int64_t)counts[i] * (dt[i] == ncclFloat64 || dt[i] == ncclInt64 ||
                                                                  dt[i] == ncclUint64 ? 8
                                                                  : dt[i] == ncclFloat16 || dt[i] == ncclBfloat16 ? 2
                                                                  : dt[i] <= ncclUint8 ? 1 : 4)
                                         : (int64_t)counts[i];
      EXPECT(cover == want);
    }
    for (int i = 0; i < k; i++) EXPECT(seen[i] == 1);
  }
  // invalid planner inputs are rejected, not read past
  {
    int c = 0, d = ncclFloat32, o = 0, a, ord, p;
    size_t cnt = 0;
    int64_t cb[8];
    const int64_t geo[4] = {512 << 10, 512, 120 * 640 * 8, 640};
    EXPECT(vcclGroupPlanEx(1, &c, &cnt, &d, &o, 2, 8, geo, nullptr, &a, &ord, &p, cb) == ncclInvalidArgument);
    cnt = 10;
    EXPECT(vcclGroupPlanEx(0, &c, &cnt, &d, &o, 2, 8, geo, nullptr, &a, &ord, &p, cb) == ncclInvalidArgument);
    EXPECT(vcclGroupPlanEx(1, &c, &cnt, &d, &o, 2, 0, geo, nullptr, &a, &ord, &p, cb) == ncclInvalidArgument);
    EXPECT(vcclGroupPlanEx(1, &c, &cnt, &d, &o, 2, 8, nullptr, nullptr, &a, &ord, &p, cb) == ncclInvalidArgument);
    d = 99;
    EXPECT(vcclGroupPlanEx(1, &c, &cnt, &d, &o, 2, 8, geo, nullptr, &a, &ord, &p, cb) == ncclInvalidArgument);
  }
  // single-call partitions and the direct all-reduce's chunk lookup
  long parts = 0;
  for (int trial = 0; trial < 20000; trial++) {
    const int n = (int)pick({1, 2, 4, 8}), nch = (int)pick({1, 3, 16, 64});
    const int proto = (int)pick({0, 1, 2});
    const size_t count = 1 + rng() % (3 << 20);
    const int d = dts[rng() % 10];
    int64_t out[8];
    const size_t step = proto == 1 ? 614400 : proto == 0 ? 65536 : 512 << 10;
    EXPECT(vcclRingPartition((int)(rng() % 5), count, (ncclDataType_t)d, n, nch, proto, step,
                             proto == 1 ? 640 : 512, out) == ncclSuccess);
    int64_t ck[3];
    EXPECT(vcclRingChunkOf(count, (ncclDataType_t)d, n, nch, 512 << 10, 512, rng() % count, ck) == ncclSuccess);
    EXPECT(ck[0] >= 0 && ck[0] < nch && ck[1] >= 0 && ck[1] < n);
    parts++;
  }
  // NCCL_ALGO / NCCL_PROTO strings: random garbage never crashes
  const char* words[] = {"Ring", "Tree", "Direct", "LL", "LL128", "Simple", "^", ",", ";", ":", "allreduce",
                         "", " ", "ring", "^ll", "x"};
  long strs = 0;
  for (int trial = 0; trial < 20000; trial++) {
    std::string a, p;
    for (int j = (int)(rng() % 5); j > 0; j--) a += words[rng() % 16];
    for (int j = (int)(rng() % 5); j > 0; j--) p += words[rng() % 16];
    int f = -1, al = -1;
    const ncclResult_t r = vcclAlgoSelection(rng() % 4 ? a.c_str() : nullptr, rng() % 4 ? p.c_str() : nullptr,
                                             &f, &al);
    EXPECT(r == ncclSuccess || r == ncclInvalidUsage);
    strs++;
  }
  // the communicator setup (vcclCommSetup): random rank counts, peer
  // identities that collide, knobs set to values and junk, random chains
  const char* knobs[] = {"NCCL_NCHANNELS", "VCCL_CHANNELS_PER_RING", "NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS",
                         "NCCL_MAX_NRINGS", "NCCL_BUFFSIZE", "VCCL_SLOT_BYTES", "VCCL_SLICE_BYTES", "NCCL_NTHREADS",
                         "VCCL_LL_THRESHOLD", "VCCL_LL_GROUP_BYTES", "VCCL_LL_RSAG_THRESHOLD",
                         "VCCL_DIRECT_THRESHOLD", "VCCL_DIRECT_RSAG_THRESHOLD", "VCCL_DIRECT_MAX_BLOCKS",
                         "VCCL_DIRECT_CHUNK_BYTES", "VCCL_LL128", "VCCL_LL128_ALLOC", "NCCL_LL128_BUFFSIZE",
                         "NCCL_LL128_NTHREADS", "VCCL_LL128_MIN", "VCCL_LL128_MAX", "VCCL_NET_FORCE",
                         "VCCL_NET_NCHANNELS", "VCCL_ALLOW_SHARED_DEVICE"};
  const char* algos[] = {"Ring", "Tree", "Direct", "^Tree", "ring,tree", "Rnig", "7"};
  const char* protos[] = {"LL", "LL128", "Simple", "^LL", "LL,LL128", "LL256", ""};
  const char* junk[] = {"", "x", "-", "0x", "12abc", " 7", "1e9", "Ring", "LL128", "^LL", "Simple,LL"};
  long setups = 0, refusals = 0;
  for (int trial = 0; trial < 20000; trial++) {
    for (const char* k : knobs) {
      const int how = (int)(rng() % 8);
      if (how >= 3) unsetenv(k);
      else if (how == 2) setenv(k, junk[rng() % 11], 1);
      else setenv(k, std::to_string(pick({-1, 0, 1, 2, 3, 4, 8, 64, 100, 4096, 5000, 65536, 262144, 1 << 20,
                                          (1 << 22) + 1, 1ll << 31, 1ll << 40}) - (int64_t)(rng() % 2)).c_str(), 1);
    }
    if (rng() % 4) unsetenv("NCCL_ALGO");
    else setenv("NCCL_ALGO", algos[rng() % 7], 1);
    if (rng() % 4) unsetenv("NCCL_PROTO");
    else setenv("NCCL_PROTO", protos[rng() % 7], 1);
    const int n = (int)pick({1, 2, 3, 4, 6, 7, 8, 9, 64});
    std::string chain;
    for (int j = (int)(rng() % (n + 2)); j > 0 && rng() % 3; j--)
      chain += (rng() % 9 ? std::to_string((int64_t)(rng() % (n + 1)) - (rng() % 16 == 0)) : std::string("z")) +
               (rng() % 8 ? "," : "");
    if (rng() % 2) {  // a permutation as often as not
      chain.clear();
      std::vector<int> perm(n);
      for (int j = 0; j < n; j++) perm[j] = j;
      std::shuffle(perm.begin(), perm.end(), rng);
      for (int j = 0; j < n; j++) chain += std::to_string(perm[j]) + (j + 1 < n ? "," : "");
    }
    if (rng() % 3 == 0) setenv("VCCL_LL_CHAIN", chain.c_str(), 1);
    else unsetenv("VCCL_LL_CHAIN");
    std::vector<int> pid(n), cus(n), net(n, -1);
    std::vector<uint64_t> host(n);
    std::vector<int64_t> bus(n);
    const int nPid = 1 + (int)(rng() % 3), nHost = 1 + (int)(rng() % 8 == 0), nBus = (int)pick({1, 2, n, n, n, 2 * n});
    for (int r = 0; r < n; r++) {
      pid[r] = 100 + (int)(rng() % nPid);
      host[r] = rng() % nHost;
      bus[r] = rng() % 16 ? r % nBus : (int64_t)(rng() % nBus);
      cus[r] = (int)pick({-5, 0, 1, 64, 256, 304, 70000});
    }
    int64_t words[19], sizes[5];
    int flags[3], chainOut[8], ring[3], tables[129];
    const int rank = (int)(rng() % n), ch = (int)(rng() % 4);
    const ncclResult_t r = vcclCommSetup(n, rank, (int)pick({1, 1, 4, 200}), (int)pick({128, 128, 2, 64}),
                                         pid.data(), host.data(), bus.data(), cus.data(), words, sizes, flags,
                                         net.data(), chainOut, ch, rng() % 2 ? ring : nullptr,
                                         rng() % 2 ? tables : nullptr);
    EXPECT(r == ncclSuccess || r == ncclInvalidUsage || r == ncclInvalidArgument);
    setups++;
    if (r != ncclSuccess) {
      refusals++;
      continue;
    }
    EXPECT(words[0] >= 0 && words[0] <= 128);  // nChannels within kMaxChannels
    EXPECT((words[0] == 0) == (n == 1));
    for (int q = 0; q < n; q++) EXPECT(net[q] == 0 || net[q] == 1);
  }
  for (const char* k : knobs) unsetenv(k);
  for (const char* k : {"VCCL_LL_CHAIN", "NCCL_ALGO", "NCCL_PROTO"}) unsetenv(k);
  {
    int i1[1] = {0}, f[3], c8[8];
    uint64_t h[1] = {0};
    int64_t b[1] = {0}, w[19], s[5];
    EXPECT(vcclCommSetup(0, 0, 1, 128, i1, h, b, i1, w, s, f, i1, c8, 0, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetup(65, 0, 1, 128, i1, h, b, i1, w, s, f, i1, c8, 0, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetup(1, 1, 1, 128, i1, h, b, i1, w, s, f, i1, c8, 0, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetup(1, 0, 1, 128, nullptr, h, b, i1, w, s, f, i1, c8, 0, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetup(1, 0, 1, 128, i1, h, b, i1, w, s, f, i1, c8, 0, nullptr, nullptr) == ncclSuccess);
  }
  // op encoding, error strings, handle checks (no device work)
  for (int op = 0; op < 6; op++)
    for (int d = 0; d < 13; d++) {
      int devOp = -1;
      uint64_t arg = 0;
      (void)vcclHostToDevRedOp((ncclRedOp_t)op, (ncclDataType_t)d, 4, &devOp, &arg);
    }
  for (int e = -1; e < 12; e++) EXPECT(ncclGetErrorString((ncclResult_t)e) != nullptr);
  int v = 0;
  EXPECT(ncclCommCount(nullptr, &v) == ncclInvalidArgument);
  {
    int c = 0, d = ncclFloat32, o = 0, a = -1;
    size_t cnt = 4;
    EXPECT(vcclCommGroupAlgos(nullptr, 1, &c, &cnt, &d, &o, &a) == ncclInvalidArgument);
  }
  EXPECT(ncclAllReduce(nullptr, nullptr, 4, ncclFloat32, ncclSum, nullptr, nullptr) == ncclInvalidArgument);
  EXPECT(ncclGroupStart() == ncclSuccess);
  EXPECT(ncclAllGather(nullptr, nullptr, 4, ncclFloat32, nullptr, nullptr) == ncclInvalidArgument);
  const ncclResult_t ge = ncclGroupEnd();
  EXPECT(ge == ncclInvalidArgument);  // the group fails as a whole (enqueue.cc:2516)
  EXPECT(vcclBuildInfo() != nullptr);
  // the point-to-point planner on random call lists (self traffic matched or
  // not), and the NULL-comm answers of the p2p entry points
  long p2pPlans = 0;
  for (int trial = 0; trial < 3000; trial++) {
    const int n = 1 + (int)(rng() % 8), rank = (int)(rng() % n), k = (int)(rng() % 24);
    const int prt = (int)pick({1, 2, 4, 8}), maxWorks = (int)pick({1, 3, 120});
    std::vector<int> kinds(k + 1), peers(k + 1);
    std::vector<size_t> nb(k + 1);
    for (int i = 0; i < k; i++) {
      kinds[i] = (int)(rng() % 2);
      peers[i] = (int)(rng() % n);
      nb[i] = (size_t)pick({0, 1, 17, 4096, 65537, 3 << 20}) + rng() % 3;
    }
    int nItems = -1, nWgs = -1;
    std::vector<int64_t> items(12 * (size_t)std::max(1, k * prt), -1);
    const ncclResult_t r = vcclP2pPlan(rank, n, k, kinds.data(), peers.data(), nb.data(), nullptr, prt, 4096, 16384,
                                       1, (int)pick({0, 1, 3}), maxWorks, k * prt, &nItems, &nWgs, items.data());
    EXPECT(r == ncclSuccess || r == ncclInvalidUsage);
    if (r == ncclSuccess) {
      EXPECT(nItems >= 0 && nItems <= k * prt && nWgs >= 1);
      for (int i = 0; i < nItems; i++) {
        const int64_t* it = &items[12 * (size_t)i];
        EXPECT(it[0] == i / maxWorks && it[1] >= 0 && it[1] < 2 * nWgs && it[2] >= 0 && it[2] <= 2);
        EXPECT(it[5] >= 0 && it[5] < prt && it[6] >= 0 && it[6] < n && it[7] >= 0 && it[7] < k);
        EXPECT(it[10] > 0 && it[9] + it[10] <= (int64_t)nb[it[7]]);
      }
    }
    p2pPlans++;
  }
  EXPECT(ncclSend(nullptr, 4, ncclFloat32, 0, nullptr, nullptr) == ncclInvalidUsage);
  EXPECT(ncclRecv(nullptr, 4, ncclFloat32, 0, nullptr, nullptr) == ncclInvalidUsage);
  EXPECT(ncclAllToAll(nullptr, nullptr, 4, ncclFloat32, nullptr, nullptr) == ncclInvalidUsage);
  EXPECT(ncclAllToAllv(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ncclFloat32, nullptr, nullptr) ==
         ncclInvalidUsage);
  // the rooted LL selection (vcclRootedAlgo) and launch layout
  // (vcclLLRootedPlan) on random policies, thresholds, part lists and caps
  long rooted = 0;
  for (int trial = 0; trial < 20000; trial++) {
    const int n = (int)pick({0, 1, 2, 3, 4, 8, 9, 64, 65});
    const int64_t slot = pick({0, 0, 8, 4096, 1 << 20, -1});
    const int64_t pol[10] = {pick({0, 0, 1, 2, 3, 4, 5}), slot, pick({0, 1 << 20}), pick({0, 4 << 20}), pick({0, 1}),
                             64 << 10, pick({0, 1 << 20}), pick({0, 1}), pick({0, 8 << 20}), pick({0, 64 << 20})};
    const int64_t thr = pick({-1, 0, 1, 4096, 1 << 20, 1ll << 40});
    if (rng() % 4 == 0) setenv("VCCL_LL_ROOTED_THRESHOLD", junk[rng() % 11], 1);
    else if (rng() % 2) setenv("VCCL_LL_ROOTED_THRESHOLD", "65536", 1);
    else unsetenv("VCCL_LL_ROOTED_THRESHOLD");
    int64_t eff = -7;
    int algo = -7;
    const int coll = (int)(rng() % 7) - 1;
    const size_t count = (size_t)pick({0, 1, 8, 4097, 1 << 20, 1 << 24});
    const ncclResult_t r = vcclRootedAlgo(coll, count, (ncclDataType_t)dts[rng() % 10], n, rng() % 16 ? pol : nullptr,
                                          thr, (int)(rng() % 2), (int)(rng() % 2), rng() % 2 ? &eff : nullptr,
                                          rng() % 16 ? &algo : nullptr);
    EXPECT(r == ncclSuccess || r == ncclInvalidArgument);
    if (r == ncclSuccess) {
      EXPECT(algo == vcclAlgoRing || algo == vcclAlgoLL || algo == vcclAlgoDirect || algo == vcclAlgoLL128);
      EXPECT(eff == -7 || (eff >= 0 && eff <= (slot > 0 ? slot : 0)));
    }
    const int nr = (int)pick({1, 2, 3, 5, 8, 9}), k = (int)(rng() % 19);
    const int64_t lps = pick({0, 1, 16, 512, 131072});
    std::vector<int> roots(k + 1);
    std::vector<size_t> nb(k + 1);
    for (int i = 0; i < k; i++) {
      roots[i] = (int)(rng() % (nr + 1)) - (rng() % 32 == 0);
      nb[i] = (size_t)pick({0, 1, 7, 8, 9, 100, 4096}) + (rng() % 64 == 0 ? (size_t)lps * 8 : 0);
    }
    const int cap = (int)pick({0, 1, 4, (nr - 1) * (k + 1), 200});
    std::vector<int64_t> l0(k + 1, -1), st(4 * (size_t)cap + 1, -1), po(4 * (size_t)cap + 1, -1);
    int ns = -1, np = -1;
    const ncclResult_t q = vcclLLRootedPlan((int)pick({3, 4, 4, 3, 2}), nr, (int)(rng() % (nr + 1)), k, roots.data(),
                                            nb.data(), lps, cap, rng() % 4 ? l0.data() : nullptr, &ns,
                                            rng() % 8 ? st.data() : nullptr, &np, rng() % 8 ? po.data() : nullptr);
    EXPECT(q == ncclSuccess || q == ncclInvalidArgument);
    if (q == ncclSuccess) {
      EXPECT(ns >= nr - 1 && ns <= cap && np >= nr - 1 && np <= cap);  // line 0 of every pair, at least
      for (int i = 0; i < ns; i++) {
        const int64_t* x = &st[4 * (size_t)i];
        EXPECT(x[0] >= 0 && x[0] < nr && x[1] >= -1 && x[1] < k && x[2] >= 0 && x[2] < x[3] && x[3] <= lps);
      }
      for (int i = 0; i < np; i++) {
        const int64_t* x = &po[4 * (size_t)i];
        EXPECT(x[0] >= 0 && x[0] < nr && x[1] >= -1 && x[1] < k && x[2] >= 0 && x[2] < x[3] && x[3] <= lps);
      }
    }
    EXPECT(st[4 * (size_t)cap] == -1 && po[4 * (size_t)cap] == -1);  // nothing past cap ranges
    rooted++;
  }
  unsetenv("VCCL_LL_ROOTED_THRESHOLD");
  // the rooted direct selection (vcclRootedAlgoEx) and one call's geometry and
  // steps (vcclDirectRootedPlan) on random policies, thresholds, regions and caps
  long directRooted = 0;
  for (int trial = 0; trial < 20000; trial++) {
    const int n = (int)pick({0, 1, 2, 3, 4, 8, 9, 64, 65});
    const int64_t pol[10] = {pick({0, 0, 1, 2, 3, 4, 5}), pick({0, 4096, 1 << 20, -1}), pick({0, 1 << 20}),
                             pick({0, 4 << 20}), pick({0, 1}), 64 << 10, pick({0, 1 << 20}), pick({0, 1}),
                             pick({0, 8 << 20}), pick({0, 64 << 20})};
    if (rng() % 4 == 0) setenv("VCCL_DIRECT_ROOTED_THRESHOLD", junk[rng() % 11], 1);
    else if (rng() % 2) setenv("VCCL_DIRECT_ROOTED_THRESHOLD", "65536", 1);
    else unsetenv("VCCL_DIRECT_ROOTED_THRESHOLD");
    int64_t eff = -7, deff = -7;
    int algo = -7;
    const int64_t dthr = pick({-1, 0, 1, 4096, 8 << 20, 1ll << 40});
    const ncclResult_t r = vcclRootedAlgoEx((int)(rng() % 7) - 1, (size_t)pick({0, 1, 8, 4097, 1 << 20, 1 << 24}),
                                            (ncclDataType_t)dts[rng() % 10], n, rng() % 16 ? pol : nullptr,
                                            pick({-1, 0, 4096}), (int)(rng() % 2), (int)(rng() % 2), dthr,
                                            (int)(rng() % 2), rng() % 2 ? &eff : nullptr, rng() % 2 ? &deff : nullptr,
                                            rng() % 16 ? &algo : nullptr);
    EXPECT(r == ncclSuccess || r == ncclInvalidArgument);
    if (r == ncclSuccess) {
      EXPECT(algo == vcclAlgoRing || algo == vcclAlgoLL || algo == vcclAlgoDirect || algo == vcclAlgoLL128);
      EXPECT(deff == -7 || deff >= 0);
      EXPECT(deff <= 0 || (pol[7] != 0 && n <= 8));
    }
    const int nr = (int)pick({1, 2, 3, 5, 8, 9}), coll = (int)pick({3, 4, 4, 3, 2});
    const int64_t region = pick({0, 16, 32, 272, 8448, 2097408, 1ll << 41});
    const size_t count = (size_t)pick({0, 1, 15, 4099, 100003, 1 << 22}) << (rng() % 64 == 0 ? 40 : 0);
    const int chunk = (int)pick({-1, 0, 0, 1, 2, 1000});
    const int cap = (int)pick({0, 1, 8, 4 * nr + 8, 200});
    int64_t geo[4] = {-1, -1, -1, -1};
    std::vector<int> own(9, -1);
    std::vector<int64_t> st(8 * (size_t)cap + 1, -1);
    int ns = -1;
    const ncclResult_t q = vcclDirectRootedPlan(coll, nr, (int)(rng() % (nr + 1)), (int)(rng() % (nr + 1)), count,
                                                (ncclDataType_t)dts[rng() % 10], region, chunk, cap,
                                                rng() % 16 ? geo : nullptr, rng() % 4 ? own.data() : nullptr, &ns,
                                                rng() % 8 ? st.data() : nullptr);
    EXPECT(q == ncclSuccess || q == ncclInvalidArgument);
    if (q == ncclSuccess) {
      EXPECT(geo[0] >= 1 && geo[1] >= 1 && geo[3] == (coll == 4 ? nr : nr - 1) && ns >= 0 && ns <= cap);
      EXPECT(chunk < 0 ? ns == 0 : geo[2] >= 1);
      for (int i = 0; i < ns; i++) {
        const int64_t* x = &st[8 * (size_t)i];
        EXPECT(x[0] >= 0 && x[0] <= 4 && x[1] >= 0 && x[1] <= 1 && x[2] >= 0 && x[2] < nr && x[3] >= 0 && x[3] < nr);
        EXPECT(x[4] == 0 && x[5] >= 0 && x[6] >= 0 && x[7] >= 0 && x[7] <= 2);
        if (x[0] == 1 || x[0] == 2) EXPECT(x[6] <= region - 16);
      }
    }
    EXPECT(st[8 * (size_t)cap] == -1 && own[8] == -1);  // nothing past cap steps or the shard count
    directRooted++;
  }
  unsetenv("VCCL_DIRECT_ROOTED_THRESHOLD");
  // the LL all-to-all limit (vcclLLA2aMax) and one call's split (vcclLLA2aPlan)
  // on random byte matrices, limits, slots and invalid arguments
  long a2a = 0;
  for (int trial = 0; trial < 20000; trial++) {
    if (rng() % 4 == 0) setenv("VCCL_LL_A2A_THRESHOLD", junk[rng() % 11], 1);
    else if (rng() % 2) setenv("VCCL_LL_A2A_THRESHOLD", "65536", 1);
    else unsetenv("VCCL_LL_A2A_THRESHOLD");
    const int64_t slot = pick({0, 8, 4096, 1 << 20, -1});
    int64_t eff = -7;
    const ncclResult_t r = vcclLLA2aMax(pick({-1, 0, 1, 4096, 1 << 20, 1ll << 40}), slot, (int)(rng() % 2),
                                        (int)(rng() % 2), (int)pick({0, 1, 2, 8, 9, 64}), (int)(rng() % 2),
                                        rng() % 16 ? &eff : nullptr);
    EXPECT(r == ncclSuccess || r == ncclInvalidArgument);
    if (r == ncclSuccess) EXPECT(eff >= 0 && eff <= (slot > 0 ? slot : 0));
    const int n = (int)pick({1, 2, 3, 4, 5, 8, 8, 9}), rank = (int)(rng() % (n + 1)) - (rng() % 32 == 0);
    const int64_t lps = pick({0, 1, 16, 512, 131072});
    const int64_t lim = pick({0, 8, 100, 4096, lps * 8, lps * 8 + 1, -1});
    const int uniform = (int)(rng() % 3 == 0);
    std::vector<size_t> sb(n + 1), rb(n + 1);
    const size_t u = (size_t)pick({0, 1, 8, 4096, 4097});
    for (int p = 0; p < n; p++) {
      sb[p] = uniform && rng() % 16 ? u : (size_t)pick({0, 1, 7, 8, 9, 100, 4096, 4097, 1 << 20}) + rng() % 2;
      rb[p] = uniform && rng() % 16 ? u : (size_t)pick({0, 1, 7, 8, 9, 100, 4096, 4097, 1 << 20}) + rng() % 2;
      if (rng() % 256 == 0) sb[p] = ~(size_t)0;
    }
    std::vector<int> sll(n + 1, -1), rll(n + 1, -1), rs(n + 1, -1), rr(n + 1, -1);
    std::vector<int64_t> st(4 * (size_t)n + 1, -1), po(4 * (size_t)n + 1, -1);
    int launch = -1, nrs = -1, nrr = -1;
    const ncclResult_t q = vcclLLA2aPlan(n, rank, rng() % 32 ? sb.data() : nullptr, rb.data(), uniform, lim, lps,
                                         sll.data(), rng() % 32 ? rll.data() : nullptr, &launch, st.data(), po.data(),
                                         &nrs, rs.data(), &nrr, rr.data());
    EXPECT(q == ncclSuccess || q == ncclInvalidArgument);
    if (q == ncclSuccess) {
      EXPECT(launch == 0 || launch == 1);
      EXPECT(nrs >= 0 && nrs <= n && nrr >= 0 && nrr <= n);
      int nll = 0;
      for (int p = 0; p < n; p++) {
        EXPECT((sll[p] == 0 || sll[p] == 1) && (rll[p] == 0 || rll[p] == 1));
        if (!launch) EXPECT(!sll[p] && !rll[p]);
        if (sll[p]) EXPECT((int64_t)sb[p] <= lim);
        if (rll[p]) EXPECT((int64_t)rb[p] <= lim);
        nll += sll[p] + rll[p];
      }
      EXPECT(nll + nrs + nrr == 2 * n);
      for (int i = 0; i < (launch ? n - 1 : 0); i++) {
        for (const int64_t* x : {&st[4 * (size_t)i], &po[4 * (size_t)i]})
          EXPECT(x[0] >= 0 && x[0] < n && x[0] != rank && (x[1] == 0 || x[1] == -1) && x[2] == 0 && x[3] >= 1 &&
                 x[3] <= lps);
      }
      if (!launch) EXPECT(st[0] == -1 && po[0] == -1);
    }
    EXPECT(st[4 * (size_t)(n - 1)] == -1 && po[4 * (size_t)(n - 1)] == -1);  // nothing past n - 1 ranges
    EXPECT(sll[n] == -1 && rll[n] == -1 && rs[n] == -1 && rr[n] == -1);
    a2a++;
  }
  unsetenv("VCCL_LL_A2A_THRESHOLD");
  EXPECT(vcclCommA2aStats(nullptr, nullptr, nullptr, nullptr) == ncclInvalidArgument);
  EXPECT(vcclCommSetA2aThreshold(nullptr, 4096, nullptr) == ncclInvalidArgument);
  // the direct all-to-all limit (vcclDirectA2aMax) and one call's three-way
  // split (vcclDirectA2aPlan) on random byte matrices, limits, bounds and
  // invalid arguments
  long directA2a = 0;
  for (int trial = 0; trial < 20000; trial++) {
    if (rng() % 4 == 0) setenv("VCCL_DIRECT_A2A_THRESHOLD", junk[rng() % 11], 1);
    else if (rng() % 2) setenv("VCCL_DIRECT_A2A_THRESHOLD", "98304", 1);
    else unsetenv("VCCL_DIRECT_A2A_THRESHOLD");
    const int64_t region = pick({0, 8, 16, 17, 4096, 131328, -1});
    int64_t eff = -7;
    const ncclResult_t r = vcclDirectA2aMax(pick({-1, 0, 1, 4096, 1 << 20, 1ll << 40}), region, (int)(rng() % 2),
                                            (int)(rng() % 2), (int)pick({0, 1, 2, 8, 9, 64}), (int)(rng() % 2),
                                            rng() % 16 ? &eff : nullptr);
    EXPECT(r == ncclSuccess || r == ncclInvalidArgument);
    if (r == ncclSuccess) EXPECT(eff >= 0 && eff <= (region > 16 ? region - 16 : 0));
    const int n = (int)pick({1, 2, 3, 4, 5, 8, 8, 9}), rank = (int)(rng() % (n + 1)) - (rng() % 32 == 0);
    const int64_t lps = pick({0, 1, 16, 512, 131072});
    const int64_t lim = pick({0, 8, 100, lps * 8, lps * 8 + 1, -1});
    const int64_t dlim = pick({0, 1, 16, 4097, 98304, 1 << 21, -1, 1ll << 41});
    const int minC = (int)pick({-1, 0, 1, 4, 1000}), maxC = (int)pick({0, 1, 32, 64, 1000});
    const int dmb = (int)pick({0, 1, 16, 64, 1000});
    const int uniform = (int)(rng() % 3 == 0);
    std::vector<size_t> sb(n + 1), rb(n + 1);
    const size_t u = (size_t)pick({0, 1, 8, 4096, 4097, 98304});
    for (int p = 0; p < n; p++) {
      sb[p] = uniform && rng() % 16 ? u : (size_t)pick({0, 1, 7, 8, 9, 100, 4096, 4097, 98304, 1 << 21}) + rng() % 2;
      rb[p] = uniform && rng() % 16 ? u : (size_t)pick({0, 1, 7, 8, 9, 100, 4096, 4097, 98304, 1 << 21}) + rng() % 2;
      if (rng() % 256 == 0) sb[p] = ~(size_t)0;
    }
    std::vector<int> sp(n + 1, -1), rp(n + 1, -1), rs(n + 1, -1), rr(n + 1, -1);
    int ll = -1, dl = -1, nb = -1, nrs = -1, nrr = -1;
    int64_t blk = -1;
    const ncclResult_t q = vcclDirectA2aPlan(n, rank, rng() % 32 ? sb.data() : nullptr, rb.data(), uniform, lim, dlim,
                                             lps, minC, maxC, dmb, sp.data(), rng() % 32 ? rp.data() : nullptr, &ll,
                                             &dl, rng() % 32 ? &nb : nullptr, &blk, &nrs, rs.data(), &nrr, rr.data());
    EXPECT(q == ncclSuccess || q == ncclInvalidArgument);
    if (q == ncclSuccess) {
      EXPECT((ll == 0 || ll == 1) && (dl == 0 || dl == 1) && !(uniform && ll && dl));
      EXPECT(nrs >= 0 && nrs <= n && nrr >= 0 && nrr <= n);
      int nPath[3] = {0, 0, 0};
      for (int p = 0; p < n; p++) {
        EXPECT(sp[p] >= 0 && sp[p] <= 2 && rp[p] >= 0 && rp[p] <= 2);
        if (!ll) EXPECT(sp[p] != 1 && rp[p] != 1);
        if (!dl) EXPECT(sp[p] != 2 && rp[p] != 2);
        if (sp[p] == 1) EXPECT((int64_t)sb[p] <= lim);
        if (rp[p] == 1) EXPECT((int64_t)rb[p] <= lim);
        if (sp[p] == 2) EXPECT((int64_t)sb[p] <= dlim);
        if (rp[p] == 2) EXPECT((int64_t)rb[p] <= dlim);
        nPath[sp[p]]++;
        nPath[rp[p]]++;
      }
      EXPECT(nPath[0] == nrs + nrr && nPath[0] + nPath[1] + nPath[2] == 2 * n);
      if (dl) {
        const int64_t M = uniform ? (int64_t)sb[0] : dlim;
        EXPECT(nb >= 1 && nb <= 128 && nb <= dmb && blk >= 16 && blk % 16 == 0);
        EXPECT((int64_t)nb * blk >= M && (int64_t)(nb - 1) * blk < M);
      } else {
        EXPECT(nb == 0 && blk == 0);
      }
    }
    EXPECT(sp[n] == -1 && rp[n] == -1 && rs[n] == -1 && rr[n] == -1);
    directA2a++;
  }
  unsetenv("VCCL_DIRECT_A2A_THRESHOLD");
  EXPECT(vcclCommA2aStatsEx(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ncclInvalidArgument);
  EXPECT(vcclCommSetDirectA2aThreshold(nullptr, 4096, nullptr) == ncclInvalidArgument);
  // the registration table (vcclRegTable*) against a reference model under
  // random inserts, lookups and removals, with invalid entries and handles;
  // the zero-copy threshold, eligibility and step lists on random arguments
  long regOps = 0;
  {
    struct Model {
      bool live;
      uint64_t addr, bytes;
      uint32_t gen;
    };
    Model m[32] = {};
    vcclRegTable_t* t = nullptr;
    EXPECT(vcclRegTableNew(&t) == ncclSuccess && t != nullptr);
    EXPECT(vcclRegTableNew(nullptr) == ncclInvalidArgument);
    for (int trial = 0; trial < 40000; trial++) {
      const uint64_t addr = rng() % 64 == 0 ? ~(uint64_t)0 - rng() % 8 : 4096 + rng() % 8192;
      const size_t bytes = (size_t)pick({0, 1, 2, 100, 4096});
      const int op = (int)(rng() % 4);
      if (op == 0) {
        int e = -7;
        uint32_t g = 77;
        EXPECT(vcclRegTableInsert(t, addr, bytes, &e, rng() % 8 ? &g : nullptr) == ncclSuccess);
        int want = -1;
        if (bytes > 0 && addr + bytes >= addr)
          for (int i = 0; i < 32 && want < 0; i++)
            if (!m[i].live) want = i;
        EXPECT(e == want);
        if (e >= 0 && e < 32) m[e] = Model{true, addr, bytes, m[e].gen + 1};
        if (e >= 0 && g != 77) EXPECT(g == m[e].gen && (g & 1u));
      } else if (op == 1) {
        const int e = (int)(rng() % 40) - 4;
        const bool ok = e >= 0 && e < 32 && m[e].live;
        EXPECT(vcclRegTableRemove(t, e) == (ok ? ncclSuccess : ncclInvalidArgument));
        if (ok) m[e].live = false, m[e].gen++;
      } else {
        int e = -7;
        uint64_t off = 99;
        uint32_t g = 77;
        EXPECT(vcclRegTableFind(t, addr, bytes, &e, &off, &g) == ncclSuccess);
        int want = -1;
        for (int i = 0; i < 32 && want < 0; i++)
          if (m[i].live && addr + bytes >= addr && addr >= m[i].addr && addr < m[i].addr + m[i].bytes &&
              addr + bytes <= m[i].addr + m[i].bytes)
            want = i;
        EXPECT(e == want);
        if (e >= 0 && e < 32) EXPECT(off == addr - m[e].addr && g == m[e].gen);
      }
      regOps++;
    }
    EXPECT(vcclRegTableInsert(t, 1, 1, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclRegTableFind(nullptr, 1, 1, nullptr, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclRegTableRemove(nullptr, 0) == ncclInvalidArgument);
    EXPECT(vcclRegTableFree(t) == ncclSuccess && vcclRegTableFree(nullptr) == ncclSuccess);
    for (int trial = 0; trial < 20000; trial++) {
      const int n = (int)pick({0, 1, 2, 3, 4, 8, 9}), rank = (int)(rng() % (n + 1)) - (rng() % 32 == 0);
      const int coll = (int)(rng() % 6), dt = rng() % 16 ? dts[rng() % 10] : 12;
      const size_t count = (size_t)pick({0, 1, 7, 4095, 4096, 4097, 1000003}) + rng() % 3;
      int64_t eff = -7;
      const ncclResult_t r0 = vcclRegMax(pick({-1, 0, 1, 32768, 1ll << 40}), (int)(rng() % 2), (int)(rng() % 2),
                                         (int)(rng() % 2), n, rng() % 16 ? &eff : nullptr);
      EXPECT(r0 == ncclSuccess || r0 == ncclInvalidArgument);
      if (r0 == ncclSuccess) EXPECT(eff >= 0 && (eff == 0 || (n >= 2 && n <= 8)));
      int el = -7;
      const ncclResult_t r1 = vcclRegEligible(coll, count, (ncclDataType_t)dt, n, pick({-1, 0, 1, 32768}),
                                              (int)pick({-1, 0, 1, 2, 40}), &el);
      EXPECT(r1 == ncclSuccess || r1 == ncclInvalidArgument);
      if (r1 == ncclSuccess) EXPECT((el == 0 || el == 1) && (coll <= 2 || el == 0));
      const int nb = (int)pick({0, 1, 5, 16, 128, 129}), cap = (int)pick({0, 8, 80});
      std::vector<int64_t> steps(8 * (size_t)cap + 8, -1);
      int ns = -7;
      int64_t blk = -7;
      const ncclResult_t r2 = vcclRegPlan(coll, count, (ncclDataType_t)dt, n, rank, nb, rng() % 8 ? &blk : nullptr, cap,
                                          &ns, steps.data());
      EXPECT(r2 == ncclSuccess || r2 == ncclInvalidArgument);
      if (r2 == ncclSuccess) EXPECT(ns > 0 && ns <= cap && (blk == -7 || blk > 0));
      EXPECT(steps[8 * (size_t)cap] == -1);
      regOps++;
    }
    EXPECT(vcclCommRegStats(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetRegThreshold(nullptr, 4096, nullptr) == ncclInvalidArgument);
    // the zero-copy all-to-all's threshold, eligibility and step lists on
    // random byte matrices, offsets, bounds and invalid arguments
    for (int trial = 0; trial < 20000; trial++) {
      if (rng() % 2) setenv("VCCL_REG_A2A_THRESHOLD", rng() % 4 ? "32768" : junk[rng() % 11], 1);
      else unsetenv("VCCL_REG_A2A_THRESHOLD");
      const int n = (int)pick({0, 1, 2, 3, 4, 8, 9}), rank = (int)(rng() % (n + 1)) - (rng() % 32 == 0);
      int64_t eff = -7;
      const ncclResult_t r0 = vcclRegA2aMax(pick({-1, 0, 1, 32768, 1ll << 40}), (int)(rng() % 2), (int)(rng() % 2),
                                            (int)(rng() % 2), n, (int)(rng() % 2), (int)(rng() % 2),
                                            rng() % 16 ? &eff : nullptr);
      EXPECT(r0 == ncclSuccess || r0 == ncclInvalidArgument);
      if (r0 == ncclSuccess) EXPECT(eff >= 0 && (eff == 0 || (n >= 2 && n <= 8)));
      int el = -7;
      const int index = (int)pick({-1, 0, 1, 7, 8, 9});
      const ncclResult_t r1 = vcclRegA2aEligible((int)(rng() % 2), (size_t)pick({0, 1, 32767, 32768, 1 << 20}),
                                                 pick({-1, 0, 1, 32768}), index, rng() % 16 ? &el : nullptr);
      EXPECT(r1 == ncclSuccess || r1 == ncclInvalidArgument);
      if (r1 == ncclSuccess) EXPECT((el == 0 || el == 1) && (index < 8 || el == 0));
      const int uniform = (int)(rng() % 2), cap = (int)pick({0, 8, 64});
      const size_t m = (size_t)(n > 0 ? n : 1);
      std::vector<size_t> sb(m * m), so(m * m), ro(m);
      const size_t ub = (size_t)pick({0, 1, 40, 32768, (1 << 20) + 3});
      for (size_t i = 0; i < m * m; i++) {
        sb[i] = uniform && rng() % 64 ? ub : (size_t)pick({0, 1, 17, 4096, 100003, 1ll << 57});
        so[i] = (size_t)pick({0, 1, 4, 4096, 1 << 22}) + rng() % 3;
      }
      for (size_t i = 0; i < m; i++) ro[i] = (size_t)pick({0, 3, 4096, 1 << 22});
      std::vector<int64_t> steps(8 * (size_t)cap + 8, -1);
      int ns = -7, nb = -7;
      const ncclResult_t r2 = vcclRegA2aPlan(n, rank, rng() % 32 ? sb.data() : nullptr, so.data(), ro.data(), uniform,
                                             (int)pick({-1, 0, 1, 4, 200}), (int)pick({0, 1, 32, 64, 500}),
                                             (int)pick({0, 1, 14, 64, 128, 300}), rng() % 32 ? &nb : nullptr, cap, &ns,
                                             steps.data());
      EXPECT(r2 == ncclSuccess || r2 == ncclInvalidArgument);
      if (r2 == ncclSuccess) {
        EXPECT(ns == 5 * n + 1 && ns <= cap && nb >= 1 && nb <= 128);
        for (int k = 0; k < ns; k++) {  // every pull's slices fit the grid
          const int64_t bytes = steps[8 * k + 6], blk = steps[8 * k + 7];
          if (steps[8 * k] >= 3) EXPECT(blk >= 16 && blk % 16 == 0 && (bytes + blk - 1) / blk <= nb);
        }
      }
      EXPECT(steps[8 * (size_t)cap] == -1);
      regOps++;
    }
    unsetenv("VCCL_REG_A2A_THRESHOLD");
    EXPECT(vcclCommRegA2aStats(nullptr, nullptr, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetRegA2aThreshold(nullptr, 4096, nullptr) == ncclInvalidArgument);
    // the zero-copy broadcast / reduce: threshold, eligibility and step lists
    // on random counts, roots, regions, grids and invalid arguments
    for (int trial = 0; trial < 20000; trial++) {
      if (rng() % 2) setenv("VCCL_REG_ROOTED_THRESHOLD", rng() % 4 ? "32768" : junk[rng() % 11], 1);
      else unsetenv("VCCL_REG_ROOTED_THRESHOLD");
      const int n = (int)pick({0, 1, 2, 3, 4, 8, 9}), rank = (int)(rng() % (n + 1)) - (rng() % 32 == 0);
      const int root = (int)(rng() % (n + 1)) - (rng() % 32 == 0);
      const int coll = (int)(rng() % 6), dt = rng() % 16 ? dts[rng() % 10] : 12;
      const size_t count = (size_t)pick({0, 1, 15, 4095, 4096, 4097, 70001, 1000003}) + rng() % 3;
      int64_t eff = -7;
      const ncclResult_t r0 = vcclRegRootedMax(pick({-1, 0, 1, 32768, 1ll << 40}), (int)(rng() % 2), (int)(rng() % 2),
                                               (int)(rng() % 2), n, (int)(rng() % 2), rng() % 16 ? &eff : nullptr);
      EXPECT(r0 == ncclSuccess || r0 == ncclInvalidArgument);
      if (r0 == ncclSuccess) EXPECT(eff >= 0 && (eff == 0 || (n >= 2 && n <= 8)));
      int el = -7;
      const ncclResult_t r1 = vcclRegRootedEligible(coll, count, (ncclDataType_t)dt, pick({-1, 0, 1, 32768}),
                                                    (int)pick({-1, 0, 1, 2, 40}), rng() % 16 ? &el : nullptr);
      EXPECT(r1 == ncclSuccess || r1 == ncclInvalidArgument);
      if (r1 == ncclSuccess) EXPECT((el == 0 || el == 1) && (coll == 3 || coll == 4));
      const int nb = (int)pick({0, 1, 5, 16, 128, 129}), cap = (int)pick({0, 8, 80, 4000});
      const size_t region = (size_t)pick({0, 16, 32, 272, 4112, 65792, 2097408});
      std::vector<int64_t> steps(8 * (size_t)cap + 8, -1);
      int ns = -7, nch = -7;
      int64_t blk = -7, chunk = -7;
      const ncclResult_t r2 = vcclRegRootedPlan(coll, count, (ncclDataType_t)dt, n, rank, root, region, nb,
                                                rng() % 8 ? &blk : nullptr, &chunk, &nch, cap, &ns, steps.data());
      EXPECT(r2 == ncclSuccess || r2 == ncclInvalidArgument);
      if (r2 == ncclSuccess) {
        EXPECT(ns > 0 && ns <= cap && nch >= 1 && chunk >= 1 && (coll == 3 || coll == 4));
        for (int k = 0; k < ns; k++) EXPECT(steps[8 * k] >= 0 && steps[8 * k] <= 5 && steps[8 * k + 7] >= 0);
      }
      EXPECT(steps[8 * (size_t)cap] == -1);
      regOps++;
    }
    unsetenv("VCCL_REG_ROOTED_THRESHOLD");
    EXPECT(vcclCommRegRootedStats(nullptr, nullptr, nullptr, nullptr) == ncclInvalidArgument);
    EXPECT(vcclCommSetRegRootedThreshold(nullptr, 4096, nullptr) == ncclInvalidArgument);
  }
  printf("host_api_check: %ld registration table operations, thresholds and zero-copy plans\n", regOps);
  printf("host_api_check: %ld all-to-all limits and plans\n", a2a);
  printf("host_api_check: %ld direct all-to-all limits and plans\n", directA2a);
  printf("host_api_check: %ld rooted selections and layouts\n", rooted);
  printf("host_api_check: %ld rooted direct selections and plans\n", directRooted);
  printf("host_api_check: %ld p2p plans\n", p2pPlans);
  printf("host_api_check: %ld groups (%ld calls), %ld partitions, %ld selection strings, %ld setups (%ld refused), "
         "%d failures\n", groups, calls, parts, strs, setups, refusals, g_fail);
  return g_fail == 0 ? 0 : 1;
}
