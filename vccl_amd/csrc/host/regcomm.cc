// The registry in shared memory and the import cache (regcomm.h).
#include "regcomm.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "plan.h"

namespace vccl {

static bool same_process(const ncclComm* c, int p) {
  const PeerMap &a = c->peers[c->rank], &b = c->peers[p];
  return a.pid == b.pid && a.hostHash == b.hostHash;
}

void reg_create(ncclComm* c, PeerMap* me) {
  me->regOk = 0;
  me->regShm[0] = 0;
  if (c->nRanks < 2 || (param_int("REG_THRESHOLD", 0) <= 0 && param_int("REG_A2A_THRESHOLD", 0) <= 0 &&
                        param_int("REG_ROOTED_THRESHOLD", 0) <= 0))
    return;
  static std::atomic<unsigned> serial{0};
  char name[sizeof(me->regShm)];
  snprintf(name, sizeof(name), "/vccl-reg-%d-%u-%d", (int)getpid(), serial.fetch_add(1), c->rank);
  const int fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
  if (fd < 0) {
    VINFO("rank %d: no buffer registry (shm_open %s failed)", c->rank, name);
    return;
  }
  void* m = ftruncate(fd, sizeof(RegShm)) == 0
                ? mmap(nullptr, sizeof(RegShm), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0)
                : MAP_FAILED;
  close(fd);
  if (m == MAP_FAILED) {
    shm_unlink(name);
    return;
  }
  memset(m, 0, sizeof(RegShm));
  auto* r = new RegComm();
  reg_table_clear(&r->table);
  r->mine = (RegShm*)m;
  r->shmName = name;
  r->linked = true;
  memset(r->importOf, -1, sizeof(r->importOf));
  memset(r->seen, 0, sizeof(r->seen));
  c->reg = r;
  memcpy(me->regShm, name, sizeof(name));
  me->regOk = 1;
}

ncclResult_t reg_connect(ncclComm* c, bool anyNet) {
  const int n = c->nRanks;
  // one bit per rank, ANDed: the threshold takes effect everywhere or nowhere
  bool all = c->reg != nullptr;
  for (const PeerMap& p : c->peers) all = all && p.regOk != 0;
  const uint64_t eff = all ? reg_max_of(*c, param_int("REG_THRESHOLD", 0), n, anyNet, c->dPeers != nullptr) : 0;
  const uint64_t effA2a = reg_a2a_max_of(*c, param_int("REG_A2A_THRESHOLD", 0), n, anyNet, c->dPeers != nullptr,
                                         c->p2pConns != nullptr, all);
  const uint64_t effRooted =
      reg_rooted_max_of(*c, param_int("REG_ROOTED_THRESHOLD", 0), n, anyNet, c->dPeers != nullptr, all);
  if (eff == 0 && effA2a == 0 && effRooted == 0) {
    reg_destroy(c);
    return ncclSuccess;
  }
  RegComm* r = c->reg;
  r->peer.assign(n, nullptr);
  for (int p = 0; p < n; p++) {
    if (p == c->rank) {
      r->peer[p] = r->mine;
      continue;
    }
    char name[sizeof(c->peers[p].regShm) + 1] = {0};
    memcpy(name, c->peers[p].regShm, sizeof(c->peers[p].regShm));
    const int fd = shm_open(name, O_RDONLY, 0);
    void* m = fd >= 0 ? mmap(nullptr, sizeof(RegShm), PROT_READ, MAP_SHARED, fd, 0) : MAP_FAILED;
    if (fd >= 0) close(fd);
    if (m == MAP_FAILED) {
      VWARN("rank %d: cannot map the buffer registry of rank %d (%s)", c->rank, p, name);
      return ncclSystemError;
    }
    r->peer[p] = (const RegShm*)m;
  }
  HIPCHECK(hipHostMalloc((void**)&r->tab, sizeof(RegPeers), hipHostMallocMapped));
  memset(r->tab, 0, sizeof(RegPeers));
  HIPCHECK(hipHostGetDevicePointer((void**)&r->tabDev, r->tab, 0));
  HIPCHECK(hipMalloc((void**)&r->stats, sizeof(RegStats)));
  HIPCHECK(hipMemset(r->stats, 0, sizeof(RegStats)));
  if (effA2a > 0) NCCLCHECK(reg_a2a_alloc(c));
  if (effRooted > 0) NCCLCHECK(reg_rooted_alloc(c));
  r->threshold = eff;
  c->regA2aMaxBytes = (size_t)effA2a;
  c->regRootedMaxBytes = (size_t)effRooted;
  VINFO("rank %d: buffer registry %s, zero-copy threshold %llu B, all-to-all %llu B per pair, rooted %llu B", c->rank,
        r->shmName.c_str(), (unsigned long long)eff, (unsigned long long)effA2a, (unsigned long long)effRooted);
  return ncclSuccess;
}

// The all-to-all path's counters and skip words: only on a comm that switches
// the path on (at init or through vcclCommSetRegA2aThreshold).
ncclResult_t reg_a2a_alloc(ncclComm* c) {
  RegComm* r = c->reg;
  if (!r || r->a2aDev) return ncclSuccess;
  DeviceGuard dev(c->device);
  HIPCHECK(dev.status);
  HIPCHECK(hipMalloc((void**)&r->a2aDev, sizeof(RegA2aDev)));
  HIPCHECK(hipMemset(r->a2aDev, 0, sizeof(RegA2aDev)));
  return ncclSuccess;
}

// The rooted path's counters, likewise only where the path is switched on (at
// init or through vcclCommSetRegRootedThreshold).
ncclResult_t reg_rooted_alloc(ncclComm* c) {
  RegComm* r = c->reg;
  if (!r || r->rootedStats) return ncclSuccess;
  DeviceGuard dev(c->device);
  HIPCHECK(dev.status);
  HIPCHECK(hipMalloc((void**)&r->rootedStats, sizeof(RegStats)));
  HIPCHECK(hipMemset(r->rootedStats, 0, sizeof(RegStats)));
  return ncclSuccess;
}

void reg_unlink(ncclComm* c) {
  if (c->reg && c->reg->linked) shm_unlink(c->reg->shmName.c_str());
  if (c->reg) c->reg->linked = false;
}

void reg_destroy(ncclComm* c) {
  RegComm* r = c->reg;
  if (!r) return;
  reg_unlink(c);
  for (auto& im : r->imports)
    if (im.base) (void)hipIpcCloseMemHandle(im.base);
  for (size_t p = 0; p < r->peer.size(); p++)
    if (r->peer[p] && r->peer[p] != r->mine) munmap((void*)r->peer[p], sizeof(RegShm));
  if (r->mine) munmap(r->mine, sizeof(RegShm));
  if (r->tab) (void)hipHostFree(r->tab);
  if (r->stats) (void)hipFree(r->stats);
  if (r->a2aDev) (void)hipFree(r->a2aDev);
  if (r->rootedStats) (void)hipFree(r->rootedStats);
  c->regA2aMaxBytes = 0;
  c->regRootedMaxBytes = 0;
  for (RegHandle* h : r->handles) delete h;
  delete r;
  c->reg = nullptr;
}

// The owner's side of the seqlock.
static void shm_write(RegShmEntry* e, uint32_t generation, const hipIpcMemHandle_t* h, uint64_t allocAddr,
                      uint64_t offset, uint64_t size) {
  __atomic_store_n(&e->seq, e->seq + 1, __ATOMIC_RELAXED);  // odd: being written
  __atomic_thread_fence(__ATOMIC_RELEASE);
  if (h) {
    e->handle = *h;
    e->allocAddr = allocAddr;
    e->offset = offset;
    e->size = size;
    e->pid = (int)getpid();
  }
  __atomic_store_n(&e->generation, generation, __ATOMIC_RELAXED);
  __atomic_store_n(&e->seq, e->seq + 1, __ATOMIC_RELEASE);
}
// A reader's: false when the owner kept writing (try again at the next call).
static bool shm_read(const RegShmEntry* e, RegShmEntry* out) {
  for (int tries = 0; tries < 64; tries++) {
    const uint32_t s0 = __atomic_load_n(&e->seq, __ATOMIC_ACQUIRE);
    if (s0 & 1u) continue;
    memcpy(out, (const void*)e, sizeof(*out));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (__atomic_load_n(&e->seq, __ATOMIC_RELAXED) == s0) return true;
  }
  return false;
}

ncclResult_t reg_register(ncclComm* c, void* buff, size_t size, void** handle) {
  RegComm* r = c->reg;
  auto* h = new RegHandle{-1};
  r->handles.push_back(h);
  *handle = h;
  if (!buff || size == 0) return ncclSuccess;
  // A full table, a host pointer or an export failure: the handle is good, the
  // range counts as unregistered.
  DeviceGuard dev(c->device);
  if (dev.status != hipSuccess) return ncclSuccess;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, buff) != hipSuccess || attr.type != hipMemoryTypeDevice ||
      attr.device != c->device) {
    (void)hipGetLastError();
    return ncclSuccess;
  }
  void* base = nullptr;
  size_t asz = 0;
  hipIpcMemHandle_t ipc;
  if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &asz, (hipDeviceptr_t)buff) != hipSuccess || !base ||
      (uintptr_t)buff + size > (uintptr_t)base + asz || hipIpcGetMemHandle(&ipc, base) != hipSuccess) {
    (void)hipGetLastError();
    return ncclSuccess;
  }
  const int entry = reg_insert(&r->table, (uint64_t)(uintptr_t)buff, size);
  if (entry < 0) return ncclSuccess;
  shm_write(&r->mine->e[entry], r->table.e[entry].generation, &ipc, (uint64_t)(uintptr_t)base,
            (uint64_t)((uintptr_t)buff - (uintptr_t)base), size);
  h->entry = entry;
  return ncclSuccess;
}

ncclResult_t reg_deregister(ncclComm* c, void* handle) {
  RegComm* r = c->reg;
  auto it = std::find(r->handles.begin(), r->handles.end(), (RegHandle*)handle);
  if (!handle || it == r->handles.end()) {
    VWARN("ncclCommDeregister : handle %p was not returned by ncclCommRegister on this communicator", handle);
    return ncclInvalidArgument;
  }
  RegHandle* h = *it;
  r->handles.erase(it);
  if (h->entry >= 0 && reg_remove(&r->table, h->entry))
    shm_write(&r->mine->e[h->entry], r->table.e[h->entry].generation, nullptr, 0, 0, 0);
  delete h;
  return ncclSuccess;
}

void reg_describe(const ncclComm* c, const void* p, uint64_t bytes, uint32_t* entry, uint32_t* gen, uint64_t* off) {
  uint64_t o = 0;
  const int e = reg_find(&c->reg->table, (uint64_t)(uintptr_t)p, bytes, &o);
  *entry = e < 0 ? kRegNone : (uint32_t)e;
  *gen = e < 0 ? 0 : c->reg->table.e[e].generation;
  *off = e < 0 ? 0 : o;
}

int reg_imported_count(const ncclComm* c) {
  int k = 0;
  for (int p = 0; p < kDirectMaxRanks; p++)
    for (int i = 0; i < kRegMaxEntries; i++) k += c->reg->tab->e[p][i].base != nullptr;
  return k;
}

static void import_release(RegComm* r, int p, int i) {
  const int k = r->importOf[p][i];
  r->importOf[p][i] = -1;
  if (k < 0) return;
  RegComm::Import& im = r->imports[k];
  if (--im.refs == 0 && im.base) {
    (void)hipIpcCloseMemHandle(im.base);
    (void)hipGetLastError();
    im.base = nullptr;  // the slot is reused by the next open
  }
}

static char* import_open(ncclComm* c, int p, int i, const RegShmEntry& s) {
  RegComm* r = c->reg;
  if (same_process(c, p)) return (char*)(uintptr_t)s.allocAddr;  // as map_peer (init.cc)
  int freeSlot = -1;
  for (size_t k = 0; k < r->imports.size(); k++) {
    RegComm::Import& im = r->imports[k];
    if (!im.base) {
      freeSlot = (int)k;
      continue;
    }
    if (im.peer == p && memcmp(&im.handle, &s.handle, sizeof(s.handle)) == 0) {
      im.refs++;
      r->importOf[p][i] = (int)k;
      return (char*)im.base;
    }
  }
  void* ptr = nullptr;
  if (hipIpcOpenMemHandle(&ptr, s.handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !ptr) {
    (void)hipGetLastError();
    return nullptr;
  }
  const RegComm::Import im{p, s.handle, ptr, 1};
  if (freeSlot >= 0) r->imports[freeSlot] = im;
  else r->imports.push_back(im), freeSlot = (int)r->imports.size() - 1;
  r->importOf[p][i] = freeSlot;
  return (char*)ptr;
}

ncclResult_t reg_refresh(ncclComm* c, bool capturing) {
  RegComm* r = c->reg;
  const int n = c->nRanks, me = c->rank;
  bool changed = false;
  for (int p = 0; p < n && !changed; p++) {
    if (p == me) continue;
    for (int i = 0; i < kRegMaxEntries; i++)
      if (__atomic_load_n(&r->peer[p]->e[i].generation, __ATOMIC_RELAXED) != r->seen[p][i]) {
        changed = true;
        break;
      }
  }
  if (!changed || capturing) return ncclSuccess;
  // the kernels read the table: no launch of this comm may be in flight
  NCCLCHECK(comm_wait_own_launches(c));
  for (int p = 0; p < n; p++) {
    if (p == me) continue;
    for (int i = 0; i < kRegMaxEntries; i++) {
      RegShmEntry s;
      if (__atomic_load_n(&r->peer[p]->e[i].generation, __ATOMIC_RELAXED) == r->seen[p][i]) continue;
      if (!shm_read(&r->peer[p]->e[i], &s)) continue;
      import_release(r, p, i);
      RegPeerEntry& t = r->tab->e[p][i];
      t = RegPeerEntry{nullptr, 0, s.generation, 0};
      if (s.generation & 1u) {
        char* base = import_open(c, p, i, s);
        if (base) t = RegPeerEntry{base + s.offset, s.size, s.generation, 0};
      }
      r->seen[p][i] = s.generation;
    }
  }
  __atomic_thread_fence(__ATOMIC_RELEASE);  // the table is host memory the next kernel reads: no copy, no stream
  return ncclSuccess;
}

}  // namespace vccl
