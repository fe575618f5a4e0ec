// Communicator lifecycle: unique id, init (rank / all), destroy, abort, queries.
//
// Reference: src/init.cc (ncclCommInitRankDev :1651-1730, ncclCommInitAll
// :1750-1814, initTransportsRank :672-1276, setupChannel :599-615) and the
// P2P transport (src/transport/p2p.cc:209-560).  MI355X design: no topology
// search — one node, fully connected xGMI mesh, fixed arc-balanced ring sets
// (SURVEY.md Appendix D); each channel's FIFO and flags live in the receiver's
// HBM (uncached) and are mapped into the sender by hipIpc* (multi-process) or
// peer access (single process).
//
// What a communicator is set up WITH — ring sets, the channel count and its
// clamps, step / slot, thresholds, buffer sizes, the net and shared-GPU caps
// and refusals, the ring tables — is arithmetic in setup.cc (checked on the
// CPU through vcclCommSetup); this file connects, allocates, maps and uploads.
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <string>
#include <thread>

#include "../../../include/vccl_ext.h"
#include "../device/coll_types.hpp"
#include "../device/ring_launch.hpp"
#include "core.h"
#include "regcomm.h"
#include "setup.h"

namespace vccl {

ncclResult_t comm_check_live(const ncclComm* comm, const char* api) {
  if (comm == nullptr) {
    VWARN("%s : comm argument is NULL", api);
    return ncclInvalidArgument;
  }
  if (comm->magic != kCommMagic || comm->destroyed) {
    VWARN("%s : comm argument is invalid or destroyed", api);
    return ncclInvalidArgument;
  }
  return ncclSuccess;
}

// Joins a non-blocking comm's initialisation thread (once, whichever caller
// gets there first).
static void wait_init(ncclComm* c) {
  if (c->blocking) return;
  std::lock_guard<std::mutex> g(c->initMutex);
  if (c->initThread.joinable()) c->initThread.join();
}

// ncclCommEnsureReady (init.cc:300-317): a comm whose non-blocking
// initialisation has not ended is not usable yet — every call but
// ncclCommGetAsyncError and ncclCommAbort fails with ncclInvalidArgument
// (ncclCommDestroy too, init.cc:2066), it does not wait.
ncclResult_t comm_check(const ncclComm* comm, const char* api, bool allowFailedInit) {
  NCCLCHECK(comm_check_live(comm, api));
  ncclComm* c = const_cast<ncclComm*>(comm);
  if (!c->blocking && c->initPending.load(std::memory_order_acquire)) {
    VWARN("%s : Attempt to use communicator before the previous operation returned ncclSuccess", api);
    return ncclInvalidArgument;
  }
  wait_init(c);
  if (!allowFailedInit && c->initResult != ncclSuccess) {
    VWARN("%s : the communicator's initialisation failed (%d)", api, (int)c->initResult);
    return c->initResult;
  }
  return ncclSuccess;
}

static uint64_t host_hash() {
  char name[256] = {0};
  gethostname(name, sizeof(name) - 1);
  uint64_t h = 1469598103934665603ull;
  for (char* p = name; *p; p++) h = (h ^ (uint8_t)*p) * 1099511628211ull;
  return h;
}

static ncclResult_t alloc_uncached(void** p, size_t bytes) {
  // NCCL_FIFO_ALLOC: 0 = uncached (default), 1 = fine-grained, 2 = coarse (hipMalloc)
  int mode = (int)param_int("FIFO_ALLOC", 0);
  hipError_t e;
  if (mode == 2) e = hipMalloc(p, bytes);
  else e = hipExtMallocWithFlags(p, bytes, mode == 1 ? hipDeviceMallocFinegrained : hipDeviceMallocUncached);
  if (e != hipSuccess) {
    VWARN("FIFO allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

template <typename T>
static void free_null(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}
template <typename T>
static void host_free_null(T*& p) {
  if (p) (void)hipHostFree((void*)p);
  p = nullptr;
}
static void destroy_null(hipEvent_t& e) {
  if (e) (void)hipEventDestroy(e);
  e = nullptr;
}

static void free_resources(ncclComm* c) {
  net_stop(c);  // first: its threads read the host staging memory and flags
  reg_destroy(c);  // the buffer registry, its imports and every handle still out
  for (void* p : c->ipcOpened) (void)hipIpcCloseMemHandle(p);
  c->ipcOpened.clear();
  free_null(c->fifoBuf);
  free_null(c->flagBuf);
  free_null(c->llBuf);
  free_null(c->ll128Buf);
  free_null(c->dBuf);
  free_null(c->dFlags);
  free_null(c->dPeers);
  free_null(c->p2pBuf);
  free_null(c->p2pFlags);
  free_null(c->p2pConns);
  free_null(c->devComm);
  free_null(c->ringTrace);
  free_null(c->devChannels);
  host_free_null(c->abortFlag);
  host_free_null(c->errorFlag);
  destroy_null(c->lastLaunch);
  destroy_null(c->joinEvent);
  for (auto& cap : c->caps) destroy_null(cap.ev);
  c->caps.clear();
}

// Map a peer's buffer into this process/device.
static ncclResult_t map_peer(ncclComm* c, const PeerMap& p, int which, char** out) {
  const PeerMap& me = c->peers[c->rank];
  if (p.pid == me.pid && p.hostHash == me.hostHash) {
    if (p.device != c->device) {
      hipError_t e = hipDeviceEnablePeerAccess(p.device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        VWARN("hipDeviceEnablePeerAccess(%d -> %d) failed: %s", c->device, p.device,
              hipGetErrorString(e));
        return ncclUnhandledCudaError;
      }
      (void)hipGetLastError();
    }
    *out = p.buf[which].ptr;
    return ncclSuccess;
  }
  void* ptr = nullptr;
  hipError_t e = hipIpcOpenMemHandle(&ptr, p.buf[which].handle, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) {
    VWARN("hipIpcOpenMemHandle failed: %s", hipGetErrorString(e));
    return ncclUnhandledCudaError;
  }
  c->ipcOpened.push_back(ptr);
  *out = (char*)ptr;
  return ncclSuccess;
}

// Every rank's buffer of one kind as this process addresses it: of[rank] the
// own one, a peer's through map_peer; a net peer's (reached through the
// proxy) is left as it is.
static ncclResult_t map_all(ncclComm* c, int which, const std::vector<char>& netPeer, char** of) {
  for (int r = 0; r < c->nRanks; r++) {
    if (r == c->rank) of[r] = c->peers[r].buf[which].ptr;
    else if (!netPeer[r]) NCCLCHECK(map_peer(c, c->peers[r], which, &of[r]));
  }
  return ncclSuccess;
}

static ncclResult_t connect_bootstrap(ncclComm* c, const ncclUniqueId* id) {
  VINFO("rank %d/%d dev %d: bootstrap", c->rank, c->nRanks, c->device);
  NCCLCHECK(bootstrap_init(id, c->rank, c->nRanks, &c->bootstrap, &c->initAbort));
  // an abort of a pending non-blocking init shuts this socket (ncclCommAbort);
  // publish first, then look at the flag, so one of the two sides sees the other
  c->initFd.store(bootstrap_fd(c->bootstrap));
  if (c->initAbort.load()) {
    VWARN("rank %d: communicator initialisation aborted", c->rank);
    return ncclRemoteError;
  }
  return ncclSuccess;
}

static ncclResult_t create_flags_and_events(ncclComm* c) {
  HIPCHECK(hipHostMalloc((void**)&c->abortFlag, sizeof(int), hipHostMallocMapped));
  HIPCHECK(hipHostMalloc((void**)&c->errorFlag, sizeof(int), hipHostMallocMapped));
  *c->abortFlag = 0;
  *c->errorFlag = 0;
  // Ordering events (stream_order / stream_mark): only ever waited on by
  // other streams of this device, never by the host.  VCCL_EVENT_FENCE: 0 =
  // HIP's default system-scope release when the event is recorded, 1 =
  // device-scope release (hipEventReleaseToDevice), 2 = no system fence
  // (hipEventDisableSystemFence).
  const int64_t evMode = param_int("EVENT_FENCE", 0);
  const unsigned evFlags = hipEventDisableTiming | (evMode == 1   ? hipEventReleaseToDevice
                                                    : evMode == 2 ? hipEventDisableSystemFence
                                                                  : 0u);
  HIPCHECK(hipEventCreateWithFlags(&c->lastLaunch, evFlags));
  HIPCHECK(hipEventCreateWithFlags(&c->joinEvent, evFlags));
  c->caps.resize(ncclComm::kMaxCaptures);
  for (auto& cap : c->caps) HIPCHECK(hipEventCreateWithFlags(&cap.ev, evFlags));
  return ncclSuccess;
}

// One of this rank's buffers, published in `me`: the IPC handle for peers in
// other processes, the raw pointer for those in this one.
static ncclResult_t alloc_published(PeerMap* me, int which, char** buf, size_t bytes, bool zero) {
  NCCLCHECK(alloc_uncached((void**)buf, bytes));
  if (zero) HIPCHECK(hipMemset(*buf, 0, bytes));
  HIPCHECK(hipIpcGetMemHandle(&me->buf[which].handle, *buf));
  me->buf[which].ptr = *buf;
  return ncclSuccess;
}

// Where this rank runs, and the buffers setup_local sized (setup.cc).
static ncclResult_t alloc_buffers(ncclComm* c, const SetupSizes& z, PeerMap* me) {
  me->pid = (int)getpid();
  me->device = c->device;
  me->hostHash = host_hash();
  int dom = 0, bus = 0, dev = 0, cus = 0;
  HIPCHECK(hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, c->device));
  HIPCHECK(hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, c->device));
  HIPCHECK(hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, c->device));
  me->busId = ((int64_t)dom << 16) | (bus << 8) | dev;
  HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  me->cuCount = cu_count_of(cus);
  if (c->nRanks == 1) return ncclSuccess;
  VINFO("rank %d: alloc fifo %zu B", c->rank, z.fifoBytes);
  NCCLCHECK(alloc_published(me, kMapFifo, &c->fifoBuf, z.fifoBytes, false));
  NCCLCHECK(alloc_published(me, kMapFlag, &c->flagBuf, z.flagBytes, true));
  if (z.llBytes) NCCLCHECK(alloc_published(me, kMapLL, &c->llBuf, z.llBytes, true));
  if (z.inboxBytes) {
    NCCLCHECK(alloc_published(me, kMapDirect, &c->dBuf, z.inboxBytes, false));
    NCCLCHECK(alloc_published(me, kMapDirectFlag, &c->dFlags, kDirectFlagBytes, true));
  }
  if (z.wantLL128) NCCLCHECK(alloc_published(me, kMapLL128, &c->ll128Buf, z.ll128Bytes, true));
  if (z.p2pBytes) {
    VINFO("rank %d: alloc p2p %zu B (%d parts x %d B steps)", c->rank, z.p2pBytes, c->p2pParts, c->p2pStepBytes);
    NCCLCHECK(alloc_published(me, kMapP2p, &c->p2pBuf, z.p2pBytes, false));
    NCCLCHECK(alloc_published(me, kMapP2pFlag, &c->p2pFlags, z.p2pFlagBytes, true));
  }
  return ncclSuccess;
}

static ncclResult_t exchange_peers(ncclComm* c, PeerMap* me) {
  if (c->nRanks > 1) NCCLCHECK(net_listen(c, me));
  VINFO("rank %d: exchange peer info", c->rank);
  c->peers.assign(c->nRanks, PeerMap{});
  c->peers[c->rank] = *me;
  return bootstrap_allgather(c->bootstrap, c->peers.data(), sizeof(PeerMap));
}

// setup_mesh (setup.cc) over the exchanged table.
static ncclResult_t apply_mesh(ncclComm* c, MeshSetup* mesh) {
  std::vector<PeerId> ids;
  for (const PeerMap& p : c->peers) ids.push_back(PeerId{p.pid, p.hostHash, p.busId, p.cuCount});
  NCCLCHECK(setup_mesh(c->rank, ids, c, mesh));
  if (mesh->dropLL128) free_null(c->ll128Buf);
  if (c->p2pOff) {  // a net peer: its memory is not mapped
    free_null(c->p2pBuf);
    free_null(c->p2pFlags);
  }
  return ncclSuccess;
}

static ncclResult_t upload_dev_comm(ncclComm* c, const std::vector<std::vector<int>>& rings, bool anyNet) {
  const int n = c->nRanks;
  DevComm dc{};
  dc.rank = c->rank;
  dc.nRanks = n;
  dc.nChannels = c->nChannels;
  dc.slotBytes = c->slotBytes;
  HIPCHECK(hipHostGetDevicePointer((void**)&dc.abortFlag, (void*)c->abortFlag, 0));
  HIPCHECK(hipHostGetDevicePointer((void**)&dc.errorFlag, c->errorFlag, 0));
  dc.spinTimeoutTicks = (uint64_t)param_int("SPIN_TIMEOUT_S", 60) * 100000000ull;
  // FIFO payload moves with sc0 sc1 write-through accesses, so no L2
  // writeback / invalidate is needed per slot; VCCL_FENCES=1 adds the
  // system-scope release/acquire fences back (A/B and safety valve).
  dc.useFences = (int)param_int("FENCES", 0);
  if (anyNet) dc.useFences = 1;  // slots and flags in host memory: full system-scope fences
  dc.pollMode = (int)param_int("POLL_MODE", 0);
  // The per-wave SIMPLE ring (ring_kernels.hip PART 4) for this comm's
  // launches (VCCL_RING_WAVE=1 or vcclCommSetRingWave; default off: no gain
  // on a shared GPU).  Inside it, slots below
  // VCCL_RING_WAVE_MIN (a full default slot) still take the workgroup
  // hand-off (latency-bound slots, profiles/r05k); 0 = always per wave.
  c->ringWave = param_int("RING_WAVE", 0) != 0;
  dc.ringWaveMin = std::max<int64_t>(0, param_int("RING_WAVE_MIN", 512 << 10));
  // Opt-in slot timeline of the SIMPLE ring (vcclCommRingTrace)
  c->ringTraceCap = n > 1 ? (int)std::max<int64_t>(0, std::min<int64_t>(param_int("RING_TRACE", 0), 1 << 16)) : 0;
  if (c->ringTraceCap > 0) {
    const size_t tb = (size_t)c->nChannels * c->ringTraceCap * sizeof(RingTraceRec);
    HIPCHECK(hipMalloc((void**)&c->ringTrace, tb));
    HIPCHECK(hipMemset(c->ringTrace, 0, tb));
  }
  dc.trace = c->ringTrace;
  dc.traceCap = c->ringTraceCap;
  ring_tables(rings, n, c->rank, &dc);
  NCCLCHECK(ll_chain(n, dc.llChain));
  HIPCHECK(hipMalloc((void**)&c->devComm, sizeof(DevComm)));
  HIPCHECK(hipMemcpy(c->devComm, &dc, sizeof(dc), hipMemcpyHostToDevice));
  return ncclSuccess;
}

// The point-to-point connection table (p2p_types.hpp): for every peer and
// part, the slots and flags of both directions.
static ncclResult_t connect_p2p(ncclComm* c, const MeshSetup& mesh) {
  if (!c->p2pBuf || mesh.anyNet) return ncclSuccess;
  const int n = c->nRanks, parts = c->p2pParts, me = c->rank;
  std::vector<char*> bufOf(n), flagOf(n);
  NCCLCHECK(map_all(c, kMapP2p, mesh.netPeer, bufOf.data()));
  NCCLCHECK(map_all(c, kMapP2pFlag, mesh.netPeer, flagOf.data()));
  const size_t perConn = (size_t)kSteps * slot_stride(c->p2pStepBytes);
  auto fifo = [&](int owner, int sender, int q) { return bufOf[owner] + ((size_t)sender * parts + q) * perConn; };
  auto flag = [&](int owner, int peer, int q, int which) {
    return (uint64_t*)(flagOf[owner] + (((size_t)peer * parts + q) * 2 + which) * kFlagStride);
  };
  std::vector<P2pConn> conns((size_t)n * parts);
  for (int p = 0; p < n; p++)
    for (int q = 0; q < parts; q++) {
      P2pConn& k = conns[(size_t)p * parts + q];
      memset(&k, 0, sizeof(k));
      if (p == me) continue;  // self traffic is a local copy
      k.sendFifo = fifo(p, me, q);
      k.nextRecvTail = flag(p, me, q, 0);
      k.sendHead = flag(me, p, q, 1);
      k.recvFifo = fifo(me, p, q);
      k.recvTail = flag(me, p, q, 0);
      k.prevSendHead = flag(p, me, q, 1);
    }
  HIPCHECK(hipMalloc((void**)&c->p2pConns, sizeof(P2pConn) * conns.size()));
  HIPCHECK(hipMemcpy(c->p2pConns, conns.data(), sizeof(P2pConn) * conns.size(), hipMemcpyHostToDevice));
  return ncclSuccess;
}

// Peer mappings, the direct path's peer table and every channel's ring ends.
static ncclResult_t connect_channels(ncclComm* c, const std::vector<std::vector<int>>& rings,
                                     const MeshSetup& mesh) {
  const int n = c->nRanks;
  std::vector<char*> fifoOf(n), flagOf(n), ll128Of(n, nullptr);
  NCCLCHECK(map_all(c, kMapFifo, mesh.netPeer, fifoOf.data()));
  NCCLCHECK(map_all(c, kMapFlag, mesh.netPeer, flagOf.data()));
  // the one-hop paths and the LL128 ring need the full xGMI mesh
  if (c->dBuf && !mesh.anyNet) {
    DirectPeers dp{};
    NCCLCHECK(map_all(c, kMapDirect, mesh.netPeer, dp.buf));
    NCCLCHECK(map_all(c, kMapDirectFlag, mesh.netPeer, dp.flags));
    HIPCHECK(hipMalloc((void**)&c->dPeers, sizeof(DirectPeers)));
    HIPCHECK(hipMemcpy(c->dPeers, &dp, sizeof(dp), hipMemcpyHostToDevice));
  }
  c->llPeer.assign(n, nullptr);
  if (c->llBuf && !mesh.anyNet) NCCLCHECK(map_all(c, kMapLL, mesh.netPeer, c->llPeer.data()));
  if (c->ll128Buf && !mesh.anyNet) NCCLCHECK(map_all(c, kMapLL128, mesh.netPeer, ll128Of.data()));
  std::vector<DevChannel> chans(c->nChannels);
  const size_t fifoPerCh = (size_t)kSteps * slot_stride(c->slotBytes);
  const size_t ll128PerCh = (size_t)kSteps * c->ll128SlotBytes;
  for (int ch = 0; ch < c->nChannels; ch++) {
    DevChannel& d = chans[ch];
    memset(&d, 0, sizeof(d));
    const RingView v = ring_view(rings, ch, c->rank, d.ringRanks);
    d.ringPos = v.pos;
    auto flag = [&](int r, int which) {
      return (uint64_t*)(flagOf[r] + ((size_t)ch * 2 + which) * kFlagStride);
    };
    d.recvFifo = c->fifoBuf + ch * fifoPerCh;
    d.recvTail = flag(c->rank, 0);
    d.prevSendHead = flag(v.prev, 1);
    d.sendFifo = fifoOf[v.next] + ch * fifoPerCh;
    d.nextRecvTail = flag(v.next, 0);
    d.sendHead = flag(c->rank, 1);
    d.recvStep = d.sendStep = 0;
    d.sendSizes = nullptr;
    d.recvSizes = nullptr;
    d.ll128Recv = ll128Of[c->rank] ? ll128Of[c->rank] + ch * ll128PerCh : nullptr;
    d.ll128Send = ll128Of[v.next] ? ll128Of[v.next] + ch * ll128PerCh : nullptr;
    // a net end's pointers are set by net_connect below
    if (mesh.netPeer[v.prev]) {
      d.recvFifo = nullptr;
      d.recvTail = d.prevSendHead = nullptr;
    }
    if (mesh.netPeer[v.next]) {
      d.sendFifo = nullptr;
      d.nextRecvTail = d.sendHead = nullptr;
    }
  }
  if (mesh.anyNet) NCCLCHECK(net_connect(c, rings, chans, mesh.netPeer));
  else net_stop(c);  // close the unused listener
  HIPCHECK(hipMalloc((void**)&c->devChannels, sizeof(DevChannel) * c->nChannels));
  HIPCHECK(hipMemcpy(c->devChannels, chans.data(), sizeof(DevChannel) * c->nChannels,
                     hipMemcpyHostToDevice));
  return ncclSuccess;
}

static ncclResult_t init_rank(ncclComm* c, const ncclUniqueId* id) {
  NCCLCHECK(connect_bootstrap(c, id));
  SetupSizes sizes;
  NCCLCHECK(setup_local(c->nRanks, c->minCTAs, c->maxCTAs, c, &sizes));
  NCCLCHECK(create_flags_and_events(c));
  PeerMap me{};
  NCCLCHECK(alloc_buffers(c, sizes, &me));
  reg_create(c, &me);  // VCCL_REG_THRESHOLD / _A2A_ / _ROOTED_: this rank's buffer registry, named in `me`
  NCCLCHECK(exchange_peers(c, &me));
  MeshSetup mesh;
  NCCLCHECK(apply_mesh(c, &mesh));
  const auto rings = ring_orders(c->nRanks);
  NCCLCHECK(upload_dev_comm(c, rings, mesh.anyNet));
  VINFO("rank %d: map peers", c->rank);
  if (c->nRanks > 1) NCCLCHECK(connect_channels(c, rings, mesh));
  if (c->nRanks > 1) NCCLCHECK(connect_p2p(c, mesh));
  NCCLCHECK(reg_connect(c, mesh.anyNet));  // every peer's registry mapped before the barrier ...
  VINFO("rank %d: final barrier", c->rank);
  NCCLCHECK(bootstrap_barrier(c->bootstrap));
  reg_unlink(c);  // ... so its name can go after it
  VINFO("comm %p rank %d/%d dev %d: %d channels x %d threads, step %d B, FIFO slot %d B", (void*)c, c->rank,
        c->nRanks, c->device, c->nChannels, c->nThreads, c->stepBytes, c->slotBytes);
  VINFO("rank %d: thresholds LL %zu, LL RS/AG %zu, direct %zu, direct RS/AG %zu, LL128 [%zu, %zu]%s, "
        "algo force %d", c->rank, c->llMaxBytes, c->llRsAgMaxBytes, c->directMaxBytes,
        c->directRsAgMaxBytes, c->ll128MinBytes, c->ll128MaxBytes, c->ll128Buf ? " (buffers)" : "",
        c->algoForce);
  return ncclSuccess;
}

// ncclConfig_t + NCCL_* environment -> CTA bounds and blocking mode
// (envConfigOverride, init.cc:1472-1545: env wins, non-positive values are
// ignored, both capped at MAXCHANNELS, min > max sets min = max).
static ncclResult_t apply_config(ncclComm* c, const ncclConfig_t* config) {
  int minC = NCCL_CONFIG_UNDEF_INT, maxC = NCCL_CONFIG_UNDEF_INT;
  int blocking = NCCL_CONFIG_UNDEF_INT;
  if (config) {
    if (config->magic != 0xcafebeef) {
      VWARN("ncclCommInitRankConfig: config not initialised with NCCL_CONFIG_INITIALIZER");
      return ncclInvalidArgument;
    }
    if ((config->minCTAs != NCCL_CONFIG_UNDEF_INT && config->minCTAs <= 0) ||
        (config->maxCTAs != NCCL_CONFIG_UNDEF_INT && config->maxCTAs <= 0) ||
        (config->blocking != NCCL_CONFIG_UNDEF_INT && config->blocking != 0 &&
         config->blocking != 1)) {
      VWARN("ncclCommInitRankConfig: invalid config (blocking %d, minCTAs %d, maxCTAs %d)",
            config->blocking, config->minCTAs, config->maxCTAs);
      return ncclInvalidArgument;  // init.cc:1603-1612
    }
    minC = config->minCTAs;
    maxC = config->maxCTAs;
    blocking = config->blocking;
  }
  const int64_t envMin = param_int("MIN_CTAS", NCCL_CONFIG_UNDEF_INT);
  const int64_t envMax = param_int("MAX_CTAS", NCCL_CONFIG_UNDEF_INT);
  const int64_t envBlocking = param_int("COMM_BLOCKING", NCCL_CONFIG_UNDEF_INT);
  if (envMin != NCCL_CONFIG_UNDEF_INT && envMin > 0) minC = (int)envMin;
  if (envMax != NCCL_CONFIG_UNDEF_INT && envMax > 0) maxC = (int)envMax;
  if (envBlocking == 0 || envBlocking == 1) blocking = (int)envBlocking;
  c->minCTAs = minC == NCCL_CONFIG_UNDEF_INT ? 1 : std::min(minC, kMaxChannels);
  c->maxCTAs = maxC == NCCL_CONFIG_UNDEF_INT ? kMaxChannels : std::min(maxC, kMaxChannels);
  if (c->minCTAs > c->maxCTAs) c->minCTAs = c->maxCTAs;
  c->blocking = blocking == 0 ? 0 : 1;
  return ncclSuccess;
}

ncclResult_t comm_init_rank(ncclComm_t* out, int nranks, const ncclUniqueId* id, int rank,
                            int device, const ncclConfig_t* config) {
  if (!out) return ncclInvalidArgument;
  *out = nullptr;
  if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks) {
    VWARN("ncclCommInitRank : invalid rank %d / nranks %d", rank, nranks);
    return ncclInvalidArgument;
  }
  auto* c = new ncclComm();
  c->magic = kCommMagic;
  c->rank = rank;
  c->nRanks = nranks;
  c->device = device;
  c->userOpFreeHead = 0;
  if (ncclResult_t cr = apply_config(c, config); cr != ncclSuccess) {
    c->magic = 0;
    delete c;
    return cr;
  }
  if (!c->blocking) {
    // Non-blocking (group.cc:553-576): the handle now, the initialisation on
    // a thread of its own; ncclCommGetAsyncError says when it has ended.  On
    // failure the comm keeps no resources and only destroy / abort accept it.
    c->initPending.store(true, std::memory_order_relaxed);
    c->asyncError.store(ncclInProgress, std::memory_order_relaxed);
    const ncclUniqueId idCopy = *id;
    *out = c;
    c->initThread = std::thread([c, idCopy]() {
      (void)hipSetDevice(c->device);
      const ncclResult_t r = init_rank(c, &idCopy);
      // on failure the bootstrap socket stays open until destroy / abort
      // closes it: an abort may still be shutting it down (initFd)
      if (r != ncclSuccess) free_resources(c);
      c->initResult = r;
      c->asyncError.store(r, std::memory_order_release);
      c->initPending.store(false, std::memory_order_release);
    });
    return ncclInProgress;
  }
  ncclResult_t r = init_rank(c, id);
  if (r != ncclSuccess) {
    free_resources(c);
    bootstrap_close(c->bootstrap);
    c->magic = 0;
    delete c;
    return r;
  }
  *out = c;
  return ncclSuccess;
}

// Wait for THIS comm's launches only — its ordering event, which every eager
// launch of the comm records (bound to the kernel's completion, or a marker
// behind it; launch.cc stream_mark), and the launches of one comm are
// serialised through it, so the last one done means all done.  The
// reference's commReclaim likewise waits on the comm's own strong stream
// (src/init.cc:2079-2111), never the whole device: a hipDeviceSynchronize
// here would also wait for other comms' kernels (possibly stuck on a lost
// peer of their own) and for unrelated user work.  timeoutS < 0: no bound.
// Captured launches belong to their graphs (the caller's to wait for).
static bool wait_own_launches(ncclComm* c, double timeoutS) {
  if (!c->hasLastLaunch || !c->lastLaunch) return true;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    // an unmarked launch (VCCL_DEBUG_NO_MARK without a bound stop event) is
    // done once its stream has drained
    const hipError_t e = c->lastUnmarked ? hipStreamQuery(c->lastStream) : hipEventQuery(c->lastLaunch);
    if (e != hipErrorNotReady) return true;  // done (or the event is unusable: nothing to wait for)
    if (timeoutS >= 0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeoutS)
      return false;
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

ncclResult_t comm_wait_own_launches(ncclComm* c) { return wait_own_launches(c, -1) ? ncclSuccess : ncclInternalError; }

ncclResult_t comm_destroy(ncclComm* c, bool abort) {
  DeviceGuard dev(c->device, /*ignoreQuery=*/true);
  // ncclCommAbort (init.cc:2079-2111): raise the abort word every spin of the
  // comm's kernels polls (ring.hpp / ll.hpp / direct.hpp, as checkAbort,
  // primitives.h:142-152), then wait for the comm's own work only.
  if (abort && c->abortFlag) __atomic_store_n((int*)c->abortFlag, 1, __ATOMIC_RELEASE);
  // An aborting kernel leaves within a few hundred spins; one still queued
  // behind other work on its stream will read the abort word when it starts,
  // so after the bound the comm's memory is left allocated (a kernel may
  // still touch it) rather than freed under it.
  const double bound = abort ? (double)param_int("ABORT_WAIT_S", 10) : -1.0;
  const bool drained = wait_own_launches(c, bound);
  // Peers in OTHER processes may still post a last credit into our flags:
  // rendezvous before freeing.  Not after an abort or an error: the peer that
  // failed may never come (the kernels have ended, so no credit is in
  // flight from this side either).  Comms of one process (ncclCommInitAll) are
  // legitimately destroyed one after another by a single thread (as with the
  // reference), so a barrier there would deadlock; their kernels are already
  // complete once their own launches are.
  bool remotePeers = false;
  for (const auto& p : c->peers) remotePeers |= p.pid != (int)getpid();
  const bool failed = c->asyncError.load() != 0 || (c->errorFlag && *(volatile int*)c->errorFlag);
  if (!abort && !failed && remotePeers && c->bootstrap && c->nRanks > 1) (void)bootstrap_barrier(c->bootstrap);
  if (!drained) {
    VWARN("comm %p rank %d: its last launch has not ended %.0f s after the abort; its device memory is left "
          "allocated", (void*)c, c->rank, bound);
    net_stop(c);
  } else {
    free_resources(c);
  }
  bootstrap_close(c->bootstrap);
  c->bootstrap = nullptr;
  c->destroyed = true;
  c->magic = 0;
  delete c;
  return ncclSuccess;
}

}  // namespace vccl

using namespace vccl;

#define VCCL_ALIAS(name) __attribute__((alias(#name), visibility("default")))

VCCL_EXPORT ncclResult_t ncclGetVersion(int* version) {
  if (!version) return ncclInvalidArgument;
  *version = NCCL_VERSION_CODE;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId) {
  return bootstrap_get_unique_id(uniqueId);
}

VCCL_EXPORT ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId,
                                          int rank) {
  int dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  return comm_init_rank(comm, nranks, &commId, rank, dev, nullptr);
}

VCCL_EXPORT ncclResult_t ncclCommInitRankConfig(ncclComm_t* comm, int nranks,
                                                ncclUniqueId commId, int rank,
                                                ncclConfig_t* config) {
  int dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  return comm_init_rank(comm, nranks, &commId, rank, dev, config);
}

// nccl.h.in:178-181: several roots spread the bootstrap of very large jobs;
// one node needs one, so every rank joins the root of commIds[0] (the same
// array on every rank).
VCCL_EXPORT ncclResult_t ncclCommInitRankScalable(ncclComm_t* newcomm, int nranks, int myrank, int nId,
                                                  ncclUniqueId* commIds, ncclConfig_t* config) {
  if (nId < 1 || !commIds) {
    VWARN("ncclCommInitRankScalable: nId %d, commIds %p", nId, (void*)commIds);
    return ncclInvalidArgument;
  }
  int dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  return comm_init_rank(newcomm, nranks, &commIds[0], myrank, dev, config);
}

// nccl.h.in:104-111: device memory for any buffer the library is handed.
VCCL_EXPORT ncclResult_t ncclMemAlloc(void** ptr, size_t size) {
  if (!ptr) return ncclInvalidArgument;
  *ptr = nullptr;
  if (size == 0) return ncclSuccess;
  HIPCHECK(hipMalloc(ptr, size));
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t ncclMemFree(void* ptr) {
  if (ptr) HIPCHECK(hipFree(ptr));
  return ncclSuccess;
}

// nccl.h.in:208-217: buffer registration enables zero-copy in the reference
// (src/register/register.cc).  Every collective works on unregistered buffers;
// on a comm created with VCCL_REG_THRESHOLD the range is recorded and made
// addressable by the comm's other ranks (regcomm.h) — local, non-collective —
// and the direct all-reduce / reduce-scatter / all-gather of at least the
// threshold run zero-copy when every rank's buffers are registered (DESIGN.md
// §4.14); VCCL_REG_A2A_THRESHOLD and VCCL_REG_ROOTED_THRESHOLD do the same for
// the all-to-all (§4.15) and for broadcast / reduce (§4.16).  Without them registration is accepted and does nothing, as before.
VCCL_EXPORT ncclResult_t ncclCommRegister(const ncclComm_t comm, void* buff, size_t size, void** handle) {
  NCCLCHECK(comm_check(comm, "ncclCommRegister"));
  if (!handle) return ncclInvalidArgument;
  if (comm->reg) return reg_register(comm, buff, size, handle);
  *handle = buff;
  return ncclSuccess;
}
VCCL_EXPORT ncclResult_t ncclCommDeregister(const ncclComm_t comm, void* handle) {
  NCCLCHECK(comm_check(comm, "ncclCommDeregister"));
  if (comm->reg) return reg_deregister(comm, handle);
  return ncclSuccess;
}

// nccl.h.in:173-174 (src/init.cc ncclCommSplit): the ranks of `comm` with
// one color form a new communicator, ranked by (key, parent rank); color
// NCCL_SPLIT_NOCOLOR joins none (*newcomm = NULL).  Collective over the
// parent: its bootstrap carries every rank's (color, key), then the new
// roots' ids — the first member of each color hosts its group's root — and
// the members initialise as with ncclCommInitRankConfig on the parent's
// device (config NULL: the parent's CTA bounds).
VCCL_EXPORT ncclResult_t ncclCommSplit(ncclComm_t comm, int color, int key, ncclComm_t* newcomm,
                                       ncclConfig_t* config) {
  if (newcomm) *newcomm = nullptr;
  NCCLCHECK(comm_check(comm, "ncclCommSplit"));
  if (!newcomm) return ncclInvalidArgument;
  if (color < NCCL_SPLIT_NOCOLOR) {
    VWARN("ncclCommSplit: invalid color %d", color);
    return ncclInvalidArgument;
  }
  const int n = comm->nRanks, me = comm->rank;
  struct Entry {
    int color, key;
  };
  std::vector<Entry> ents((size_t)n);
  ents[me] = Entry{color, key};
  if (n > 1) NCCLCHECK(bootstrap_allgather(comm->bootstrap, ents.data(), sizeof(Entry)));
  std::vector<int> members;
  if (color != NCCL_SPLIT_NOCOLOR)
    for (int r = 0; r < n; r++)
      if (ents[r].color == color) members.push_back(r);
  std::stable_sort(members.begin(), members.end(),
                   [&](int a, int b) { return ents[a].key < ents[b].key; });  // ties: parent rank
  std::vector<ncclUniqueId> ids((size_t)n);
  memset(ids.data(), 0, ids.size() * sizeof(ncclUniqueId));
  if (!members.empty() && members[0] == me) NCCLCHECK(bootstrap_get_unique_id(&ids[me]));
  if (n > 1) NCCLCHECK(bootstrap_allgather(comm->bootstrap, ids.data(), sizeof(ncclUniqueId)));
  VINFO("ncclCommSplit: comm %p rank %d color %d key %d -> %zu ranks", (void*)comm, me, color, key,
        members.size());
  if (members.empty()) return ncclSuccess;
  const int newRank = (int)(std::find(members.begin(), members.end(), me) - members.begin());
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  // config NULL: the parent's (copyCommConfig, src/init.cc:2160-2161) — its
  // CTA bounds, so the child gets the parent's channel count
  ncclConfig_t inherit = NCCL_CONFIG_INITIALIZER;
  inherit.minCTAs = comm->minCTAs;
  inherit.maxCTAs = comm->maxCTAs;
  return comm_init_rank(newcomm, (int)members.size(), &ids[members[0]], newRank, comm->device,
                        config ? config : &inherit);
}

VCCL_EXPORT ncclResult_t ncclCommInitAll(ncclComm_t* comms, int ndev, const int* devlist) {
  if (!comms || ndev < 1) return ncclInvalidArgument;
  int ndevices = 0;
  HIPCHECK(hipGetDeviceCount(&ndevices));
  std::vector<int> seen(ndevices, 0);
  for (int i = 0; i < ndev; i++) {
    int d = devlist ? devlist[i] : i;
    if (d < 0 || d >= ndevices) {
      VWARN("ncclCommInitAll : invalid device %d (totalnDev=%d)", d, ndevices);
      return ncclInvalidArgument;
    }
    if (seen[d]++ && !param_int("ALLOW_SHARED_DEVICE", 0)) return ncclInvalidUsage;  // init.cc:1782-1786
  }
  ncclUniqueId id;
  NCCLCHECK(bootstrap_get_unique_id(&id));
  std::vector<ncclResult_t> res(ndev, ncclSuccess);
  std::vector<std::thread> th;
  for (int i = 0; i < ndev; i++) {
    th.emplace_back([&, i] {
      int d = devlist ? devlist[i] : i;
      if (hipSetDevice(d) != hipSuccess) {
        res[i] = ncclUnhandledCudaError;
        return;
      }
      res[i] = comm_init_rank(&comms[i], ndev, &id, i, d, nullptr);
      if (res[i] == ncclInProgress) {  // NCCL_COMM_BLOCKING=0: InitAll still returns initialised comms
        wait_init(comms[i]);
        res[i] = comms[i]->initResult;
      }
    });
  }
  for (auto& t : th) t.join();
  for (int i = 0; i < ndev; i++) {
    if (res[i] != ncclSuccess) {
      for (int j = 0; j < ndev; j++)
        if (comms[j]) comm_destroy(comms[j], true), comms[j] = nullptr;
      return res[i];
    }
  }
  return ncclSuccess;
}

// ncclCommFinalize (init.cc commFinalize): every operation of the comm has
// completed when it returns — its own launches, not the whole device.
VCCL_EXPORT ncclResult_t ncclCommFinalize(ncclComm_t comm) {
  NCCLCHECK(comm_check(comm, "ncclCommFinalize"));
  DeviceGuard dev(comm->device, /*ignoreQuery=*/true);
  return comm_wait_own_launches(comm);
}

VCCL_EXPORT ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  if (comm == nullptr) return ncclSuccess;  // init.cc: destroying NULL is a no-op
  NCCLCHECK(comm_check(comm, "ncclCommDestroy", true));
  return comm_destroy(comm, false);
}

VCCL_EXPORT ncclResult_t ncclCommAbort(ncclComm_t comm) {
  if (comm == nullptr) return ncclSuccess;
  NCCLCHECK(comm_check_live(comm, "ncclCommAbort"));
  if (comm->initPending.load()) {
    // a non-blocking init still running (init.cc commAbort of an initialising
    // comm): stop it — no more root retries, and the bootstrap socket shut so
    // a wait on peers that never come returns at once
    comm->initAbort.store(true);
    const int fd = comm->initFd.load();
    if (fd >= 0) (void)shutdown(fd, SHUT_RDWR);
  }
  wait_init(comm);  // the init thread ends promptly once told to
  return comm_destroy(comm, true);
}

VCCL_EXPORT const char* ncclGetErrorString(ncclResult_t r) {
  switch (r) {  // src/init.cc ncclGetErrorString wording
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled cuda error (run with NCCL_DEBUG=INFO for details)";
    case ncclSystemError: return "unhandled system error (run with NCCL_DEBUG=INFO for details)";
    case ncclInternalError: return "internal error - please report this issue to the NCCL developers";
    case ncclInvalidArgument: return "invalid argument (run with NCCL_DEBUG=WARN for details)";
    case ncclInvalidUsage: return "invalid usage (run with NCCL_DEBUG=WARN for details)";
    case ncclRemoteError: return "remote process exited or there was a network error";
    case ncclInProgress: return "NCCL operation in progress";
    default: return "unknown result code";
  }
}

// The comm's device error word as an ncclResult_t (ring_types.hpp): a spin
// that made no progress — a peer stopped — is ncclRemoteError; a net slot
// whose landed byte count is not its step's slice length is caught before
// it is reduced and reported as ncclInternalError.
ncclResult_t vccl::error_word_result(ncclComm* comm) {
  const int w = *(volatile int*)comm->errorFlag;
  if (w == kErrSlotSize) {
    VWARN("rank %d: a net slot landed with a byte count that is not its step's slice length; the call was "
          "stopped before reducing it", comm->rank);
    return ncclInternalError;
  }
  return w ? ncclRemoteError : ncclSuccess;
}

// The text of the last WARN, whatever NCCL_DEBUG filters (debug.cc:29,
// :265-272 ncclLastError; init.cc:2223-2225: comm unused, may be NULL).
VCCL_EXPORT const char* ncclGetLastError(ncclComm_t) { return last_error(); }

VCCL_EXPORT ncclResult_t ncclCommGetAsyncError(ncclComm_t comm, ncclResult_t* asyncError) {
  NCCLCHECK(comm_check_live(comm, "ncclCommGetAsyncError"));
  if (!asyncError) return ncclInvalidArgument;
  if (comm->initPending.load(std::memory_order_acquire)) {  // non-blocking init still running
    *asyncError = ncclInProgress;
    return ncclSuccess;
  }
  wait_init(comm);  // ended: reap its thread
  int e = comm->asyncError.load();
  if (e == 0 && comm->errorFlag && *(volatile int*)comm->errorFlag) {
    e = error_word_result(comm);
    comm->asyncError = e;
  }
  *asyncError = (ncclResult_t)e;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t ncclCommCount(const ncclComm_t comm, int* count) {
  NCCLCHECK(comm_check(comm, "ncclCommCount"));
  if (!count) return ncclInvalidArgument;
  *count = comm->nRanks;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t ncclCommCuDevice(const ncclComm_t comm, int* device) {
  NCCLCHECK(comm_check(comm, "ncclCommCuDevice"));
  if (!device) return ncclInvalidArgument;
  *device = comm->device;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t ncclCommUserRank(const ncclComm_t comm, int* rank) {
  NCCLCHECK(comm_check(comm, "ncclCommUserRank"));
  if (!rank) return ncclInvalidArgument;
  *rank = comm->rank;
  return ncclSuccess;
}

// vccl_ext.h: run-time fence toggle and the epoch-wrap test hook.
VCCL_EXPORT ncclResult_t vcclCommSetFences(ncclComm_t comm, int useFences) {
  NCCLCHECK(comm_check(comm, "vcclCommSetFences"));
  if (useFences != 0 && useFences != 1) return ncclInvalidArgument;
  if (comm->nRanks < 2 || !comm->devComm) return ncclSuccess;
  DeviceGuard dev(comm->device, /*ignoreQuery=*/true);
  HIPCHECK(dev.status);
  NCCLCHECK(comm_wait_own_launches(comm));
  HIPCHECK(hipMemcpy((char*)comm->devComm + offsetof(DevComm, useFences), &useFences, sizeof(int),
                     hipMemcpyHostToDevice));
  return ncclSuccess;
}

// vccl_ext.h: the SIMPLE ring's slot hand-off for later launches (host
// only: the launcher picks the kernel; both leave the channel's FIFO state
// identical, so no wait is needed).
VCCL_EXPORT ncclResult_t vcclCommSetRingWave(ncclComm_t comm, int perWave, unsigned long long* waveLaunches) {
  NCCLCHECK(comm_check(comm, "vcclCommSetRingWave"));
  if (perWave != 0 && perWave != 1 && perWave != -1) return ncclInvalidArgument;
  if (perWave >= 0) comm->ringWave = perWave;
  if (waveLaunches) *waveLaunches = comm->waveLaunches;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclCommDebugSetEpochs(ncclComm_t comm, uint32_t llEpoch,
                                                uint32_t directEpoch) {
  NCCLCHECK(comm_check(comm, "vcclCommDebugSetEpochs"));
  if (comm->nRanks < 2 || !comm->devComm) return ncclSuccess;
  DeviceGuard dev(comm->device, /*ignoreQuery=*/true);
  HIPCHECK(dev.status);
  NCCLCHECK(comm_wait_own_launches(comm));
  HIPCHECK(hipMemcpy((char*)comm->devComm + offsetof(DevComm, llEpoch), &llEpoch, sizeof(uint32_t),
                     hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy((char*)comm->devComm + offsetof(DevComm, dEpoch), &directEpoch,
                     sizeof(uint32_t), hipMemcpyHostToDevice));
  return ncclSuccess;
}

// nccl.h.in:191-193: reload the logging level from NCCL_DEBUG / VCCL_DEBUG
VCCL_EXPORT void ncclResetDebugInit() { reset_log_level(); }

// pnccl* profiling aliases (src/include/core.h:18-31)
extern "C" {
void pncclResetDebugInit() VCCL_ALIAS(ncclResetDebugInit);
ncclResult_t pncclGetVersion(int*) VCCL_ALIAS(ncclGetVersion);
ncclResult_t pncclGetUniqueId(ncclUniqueId*) VCCL_ALIAS(ncclGetUniqueId);
ncclResult_t pncclCommInitRank(ncclComm_t*, int, ncclUniqueId, int) VCCL_ALIAS(ncclCommInitRank);
ncclResult_t pncclCommInitRankConfig(ncclComm_t*, int, ncclUniqueId, int, ncclConfig_t*)
    VCCL_ALIAS(ncclCommInitRankConfig);
ncclResult_t pncclCommInitAll(ncclComm_t*, int, const int*) VCCL_ALIAS(ncclCommInitAll);
ncclResult_t pncclCommSplit(ncclComm_t, int, int, ncclComm_t*, ncclConfig_t*) VCCL_ALIAS(ncclCommSplit);
ncclResult_t pncclCommInitRankScalable(ncclComm_t*, int, int, int, ncclUniqueId*, ncclConfig_t*)
    VCCL_ALIAS(ncclCommInitRankScalable);
ncclResult_t pncclMemAlloc(void**, size_t) VCCL_ALIAS(ncclMemAlloc);
ncclResult_t pncclMemFree(void*) VCCL_ALIAS(ncclMemFree);
ncclResult_t pncclCommRegister(const ncclComm_t, void*, size_t, void**) VCCL_ALIAS(ncclCommRegister);
ncclResult_t pncclCommDeregister(const ncclComm_t, void*) VCCL_ALIAS(ncclCommDeregister);
ncclResult_t pncclCommFinalize(ncclComm_t) VCCL_ALIAS(ncclCommFinalize);
ncclResult_t pncclCommDestroy(ncclComm_t) VCCL_ALIAS(ncclCommDestroy);
ncclResult_t pncclCommAbort(ncclComm_t) VCCL_ALIAS(ncclCommAbort);
const char* pncclGetErrorString(ncclResult_t) VCCL_ALIAS(ncclGetErrorString);
const char* pncclGetLastError(ncclComm_t) VCCL_ALIAS(ncclGetLastError);
ncclResult_t pncclCommGetAsyncError(ncclComm_t, ncclResult_t*) VCCL_ALIAS(ncclCommGetAsyncError);
ncclResult_t pncclCommCount(const ncclComm_t, int*) VCCL_ALIAS(ncclCommCount);
ncclResult_t pncclCommCuDevice(const ncclComm_t, int*) VCCL_ALIAS(ncclCommCuDevice);
ncclResult_t pncclCommUserRank(const ncclComm_t, int*) VCCL_ALIAS(ncclCommUserRank);
}
