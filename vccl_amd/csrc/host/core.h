// Internal host-side structures of libvccl (not part of the ABI).
//
// The communicator keeps only what the MI355X ring needs; its fields map to
// the reference's ncclComm (src/include/comm.h) where one exists.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/nccl.h"
#include "../device/ring_types.hpp"
#include "setup.h"

namespace vccl {
struct DirectPeers;  // direct.hpp
struct RegComm;      // regcomm.h
}

namespace vccl {

// ----------------------------------------------------------------- logging
// NCCL_DEBUG=WARN|INFO|TRACE (debug.h:22-34); VCCL_DEBUG is an alias.
enum LogLevel { kLogNone = 0, kLogWarn = 1, kLogInfo = 2, kLogTrace = 3 };
int log_level();
void reset_log_level();
// The last WARN's text (ncclGetLastError), kept whatever the log level.
const char* last_error();
void log_msg(int level, const char* file, int line, const char* fmt, ...)
    __attribute__((format(printf, 4, 5)));
#define VWARN(...) ::vccl::log_msg(::vccl::kLogWarn, __FILE__, __LINE__, __VA_ARGS__)
#define VINFO(...)                                                                   \
  do {                                                                               \
    if (::vccl::log_level() >= ::vccl::kLogInfo)                                     \
      ::vccl::log_msg(::vccl::kLogInfo, __FILE__, __LINE__, __VA_ARGS__);            \
  } while (0)

#define HIPCHECK(cmd)                                                                \
  do {                                                                               \
    hipError_t e_ = (cmd);                                                           \
    if (e_ != hipSuccess) {                                                          \
      VWARN("HIP failure '%s' in %s", hipGetErrorString(e_), #cmd);                 \
      return ncclUnhandledCudaError;                                                 \
    }                                                                                \
  } while (0)
#define NCCLCHECK(cmd)                                                               \
  do {                                                                               \
    ncclResult_t r_ = (cmd);                                                         \
    if (r_ != ncclSuccess) return r_;                                                \
  } while (0)

// The C ABI (include/nccl.h, vccl_ext.h, vccl_bootstrap.h): everything else is hidden.
#define VCCL_EXPORT extern "C" __attribute__((visibility("default")))

// ----------------------------------------------------------------- params
// NCCL_PARAM idiom (param.h:17-25): env NCCL_<name> (or VCCL_<name>), cached.
int64_t param_int(const char* name, int64_t deflt);

// ----------------------------------------------------------------- bootstrap
struct Bootstrap;  // opaque (bootstrap.cc)
ncclResult_t bootstrap_get_unique_id(ncclUniqueId* id);
// The socket to the root (ncclCommAbort shuts it to end a pending init).
int bootstrap_fd(const Bootstrap* b);
// `abortReq` (optional): stop retrying the root when it is raised.
ncclResult_t bootstrap_init(const ncclUniqueId* id, int rank, int nranks, Bootstrap** out,
                            const std::atomic<bool>* abortReq = nullptr);
// allgather of `bytes` per rank: buf holds nranks*bytes, own slot filled in.
ncclResult_t bootstrap_allgather(Bootstrap* b, void* buf, size_t bytes);
ncclResult_t bootstrap_barrier(Bootstrap* b);
void bootstrap_close(Bootstrap* b);
uint32_t bootstrap_local_ip(Bootstrap* b);

// ----------------------------------------------------------------- net proxy
// Inter-node ring connections through host-pinned staging buffers moved by a
// proxy thread pair over TCP (proxy.cc).  Opaque here.
struct NetProxy;

// ----------------------------------------------------------------- comm
// The buffers a rank publishes to its peers.
enum { kMapFifo = 0, kMapFlag = 1, kMapLL = 2, kMapDirect = 3, kMapDirectFlag = 4, kMapLL128 = 5, kMapP2p = 6,
       kMapP2pFlag = 7, kMapCount = 8 };
struct PeerMap {               // what one rank published about itself
  int pid;
  int device;
  uint64_t hostHash;
  int64_t busId;               // PCI domain/bus/device: the GPU's identity across processes
  uint32_t netIp;              // net proxy listener (network order), see proxy.cc
  uint16_t netPort;
  uint16_t cuCount;            // compute units of the device (co-residency cap of shared GPUs)
  struct {
    hipIpcMemHandle_t handle;  // for peers in other processes
    char* ptr;                 // raw pointer (valid only in the owner process)
  } buf[kMapCount];
  // VCCL_REG_THRESHOLD: the name of this rank's buffer registry in shared
  // memory and whether it exists (regcomm.h); ANDed over the ranks at init
  char regShm[48];
  int regOk;
};

struct UserRedOp {             // ncclRedOpCreatePreMulSum state (enqueue.cc:2528-2567)
  int freeNext;                // -1 = allocated
  ncclDataType_t datatype;
  int devOp;
  bool argIsPtr;
  uint64_t arg;
};

}  // namespace vccl

// The channel count, FIFO geometry, thresholds and caps are CommSetup's
// (setup.h): decided by setup.cc, read as c->nChannels, c->llMaxBytes, ...
struct ncclComm : vccl::CommSetup {
  uint64_t magic;
  int rank = 0, nRanks = 1, device = 0;
  uint64_t* ringTrace = nullptr;  // VCCL_RING_TRACE: nChannels x ringTraceCap RingTraceRec
  int ringTraceCap = 0;
  vccl::Bootstrap* bootstrap = nullptr;
  // device resources
  char* fifoBuf = nullptr;     // nChannels * kSteps * slotBytes, uncached
  char* flagBuf = nullptr;     // nChannels * 2 flags * kFlagStride, uncached
  // one-shot LL all-reduce (ll.hpp): [2 parities][nRanks][llLines] 16 B lines
  char* llBuf = nullptr;
  std::vector<char*> llPeer;   // every rank's LL buffer mapped into this process
  // LL128 ring (ring.hpp prim_ll128): nChannels x kSteps slots of
  // ll128SlotBytes, uncached
  char* ll128Buf = nullptr;
  // two-shot direct all-reduce (direct.hpp): inbox [2 phases][nRanks][dRegionBytes]
  char* dBuf = nullptr;
  char* dFlags = nullptr;      // kDirectFlagBytes of epoch flags
  vccl::DirectPeers* dPeers = nullptr;  // device-resident peer table
  // point-to-point (p2p_types.hpp): receive buffer [sender][part][kSteps slots],
  // flag block [peer][part][tail | head], both uncached and mapped by every
  // peer; the device-resident connection table (null: no p2p on this comm,
  // p2pOff says why)
  char* p2pBuf = nullptr;
  char* p2pFlags = nullptr;
  vccl::P2pConn* p2pConns = nullptr;
  // ncclCommRegister'ed buffers and the peers' imported ones (regcomm.h);
  // null unless VCCL_REG_THRESHOLD, VCCL_REG_A2A_THRESHOLD or
  // VCCL_REG_ROOTED_THRESHOLD took effect at init
  vccl::RegComm* reg = nullptr;
  // Smallest ordered pair of a uniform ncclAllToAll on the zero-copy path over
  // registered send buffers, and the size vote of a v-call
  // (VCCL_REG_A2A_THRESHOLD, plan.h reg_a2a_max; default 0 = off)
  size_t regA2aMaxBytes = 0;
  // Smallest ncclBroadcast / ncclReduce on the zero-copy path over registered
  // buffers (VCCL_REG_ROOTED_THRESHOLD, plan.h reg_rooted_max; default 0 = off)
  size_t regRootedMaxBytes = 0;
  vccl::NetProxy* net = nullptr;  // inter-node ring connections (proxy.cc)
  int netListenFd = -1;        // proxy listener, open from init until connections are made
  vccl::DevComm* devComm = nullptr;
  vccl::DevChannel* devChannels = nullptr;
  volatile int* abortFlag = nullptr;  // host pinned, mapped
  int* errorFlag = nullptr;           // host pinned, mapped
  std::vector<void*> ipcOpened;       // peer mappings to close
  std::vector<vccl::PeerMap> peers;
  // ordering of launches on this comm across user streams
  hipEvent_t lastLaunch = nullptr;
  hipEvent_t joinEvent = nullptr;     // joins other streams into a fused group launch
  hipStream_t lastStream = nullptr;
  bool hasLastLaunch = false;         // lastLaunch/lastStream are valid
  // VCCL_DEBUG_NO_MARK=1 with no stop event bound: the last launch left no
  // event, so waiting for the comm's work polls lastStream instead
  bool lastUnmarked = false;
  // the same ordering inside each stream capture, keyed by capture id (two
  // captures on one comm may interleave): events recorded in the
  // graph, a small pool reused least-recently-used first (never destroyed
  // while the comm lives — a graph may still reference one)
  struct CapOrder {
    unsigned long long id = 0;
    bool used = false;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool has = false;
  };
  static constexpr int kMaxCaptures = 16;
  std::vector<CapOrder> caps;         // most recently used first
  uint64_t fusedLaunches = 0;         // group launches that carried > 1 collective
  int ringWave = 0;                   // SIMPLE ring launches take the per-wave hand-off (VCCL_RING_WAVE)
  uint64_t waveLaunches = 0;          // ring launches that ran the per-wave kernel
  // ncclAllToAll(v) on this comm (vcclCommA2aStats / vcclCommA2aStatsEx): LL
  // and direct launches, and the sends + recvs (self block included) that went
  // by LL / through the direct inbox / to the p2p FIFOs
  uint64_t a2aLLLaunches = 0, a2aLLPairs = 0, a2aFifoPairs = 0;
  uint64_t a2aDirectLaunches = 0, a2aDirectPairs = 0;
  // CTA (workgroup) bounds of every collective launch: ncclConfig_t
  // minCTAs / maxCTAs or NCCL_MIN_CTAS / NCCL_MAX_CTAS (init.cc:1478-1540)
  int minCTAs = 1, maxCTAs = 64;
  // Non-blocking communicator (ncclConfig_t.blocking = 0 / NCCL_COMM_BLOCKING=0,
  // group.cc:553-576): ncclCommInitRank* returns ncclInProgress and the
  // initialisation runs on initThread; ncclCommGetAsyncError reports
  // ncclInProgress until it ends, then its result.  Every other call on the
  // comm waits for it first (comm_check).
  int blocking = 1;
  std::atomic<bool> initPending{false};
  // ncclCommAbort of a pending non-blocking init: raise initAbort, shut the
  // bootstrap socket (initFd, published once connected) so a wait on peers
  // that never come ends at once
  std::atomic<bool> initAbort{false};
  std::atomic<int> initFd{-1};
  ncclResult_t initResult = ncclSuccess;
  std::thread initThread;
  std::mutex initMutex;
  // state
  std::atomic<int> asyncError{0};
  std::vector<vccl::UserRedOp> userOps;
  int userOpFreeHead = 0;
  uint64_t opCount = 0;
  bool destroyed = false;
};

namespace vccl {
// Makes `device` current for a scope: hipSetDevice only when it differs from
// the current one, the previous device restored on scope exit (that result
// ignored).  status: the failure of the query or of the switch, for HIPCHECK
// where either is an error.  A failed query leaves the device alone unless
// `ignoreQuery` (the teardown paths, which switch regardless).
struct __attribute__((visibility("hidden"))) DeviceGuard {
  const int device;
  int old = -1;
  hipError_t status;
  explicit DeviceGuard(int dev, bool ignoreQuery = false) : device(dev), status(hipGetDevice(&old)) {
    if (status != hipSuccess) old = -1;
    if (status == hipSuccess || ignoreQuery) status = old != device ? hipSetDevice(device) : hipSuccess;
  }
  ~DeviceGuard() {
    if (old >= 0 && old != device) (void)hipSetDevice(old);
  }
  DeviceGuard(const DeviceGuard&) = delete;
};

constexpr uint64_t kCommMagic = 0x76636363'6c6d6933ull;  // "vccclmi3"
// A valid, live comm whose initialisation has ended (a non-blocking one is
// waited for); its result unless allowFailedInit (destroy / abort).
ncclResult_t comm_check(const ncclComm* comm, const char* api, bool allowFailedInit = false);
// The same without waiting for a non-blocking initialisation (GetAsyncError).
ncclResult_t comm_check_live(const ncclComm* comm, const char* api);
// Waits until every eager launch of `comm` has completed (init.cc).
ncclResult_t comm_wait_own_launches(ncclComm* comm);
// The comm's device error word as a result code (init.cc).
ncclResult_t error_word_result(ncclComm* comm);

// Net proxy (proxy.cc).  net_listen opens this rank's listener before the
// peer exchange (address published in `me`); net_connect builds the
// connections of every channel whose prev / next is flagged in netPeer,
// points those channel ends at host-pinned staging memory and starts the
// proxy threads; net_stop joins them and frees everything (idempotent).
ncclResult_t net_listen(ncclComm* c, PeerMap* me);
ncclResult_t net_connect(ncclComm* c, const std::vector<std::vector<int>>& rings,
                         std::vector<DevChannel>& chans, const std::vector<char>& netPeer);
void net_stop(ncclComm* c);
}  // namespace vccl
