// A communicator's buffer registry and import cache: what
// ncclCommRegister / ncclCommDeregister do on a comm created with
// VCCL_REG_THRESHOLD, VCCL_REG_A2A_THRESHOLD or VCCL_REG_ROOTED_THRESHOLD set
// (any of them builds the registry; each switches on its own path only), and what an eligible call
// reads at its enqueue.
//
// Registry: one per rank and comm, in POSIX shared memory created at init (its
// name travels in PeerMap; every rank maps every peer's read-only before the
// init barrier, the creator unlinks it after).  kRegMaxEntries entries, each
// {generation, IPC handle of the allocation, the range's offset in it, size,
// owner pid} written under a seqlock, so a reader never sees a torn entry.
// Registration is local and non-collective (register.cc of the reference): no
// rank waits for another in either call.
//
// Import: lazy and purely local.  At the enqueue of an eligible call a rank
// compares each peer's generations with what it last saw; nothing else happens
// when nothing changed.  A new entry's allocation is opened once per IPC
// handle (the runtime refuses a second open), a same-process peer's is its raw
// pointer, vanished entries are closed; the result is the device-resident
// RegPeers table the kernels check descriptors against (direct_reg.hpp), in
// host-pinned mapped memory: a refresh stores into it after waiting for the
// comm's own launches and puts nothing on any stream — a copy could queue
// behind the spinning kernel of another comm of this process (ncclCommInitAll),
// which waits for the very launch this enqueue is about to make.  It is
// skipped while the stream captures: a stale table only means fallback.  A
// failed import leaves the entry empty; it is never an error.
#pragma once
#include <string>
#include <vector>

#include "core.h"
// behind core.h: the shared device types need the HIP runtime's qualifiers
#include "../device/coll_types.hpp"
#include "reg.h"

#pragma GCC visibility push(hidden)
namespace vccl {

static_assert(kRegTableEntries == kRegMaxEntries, "the device table mirrors the registry");

struct RegShmEntry {
  uint32_t seq;         // seqlock: odd while the owner writes
  uint32_t generation;  // RegEntry::generation (odd: live)
  hipIpcMemHandle_t handle;
  uint64_t allocAddr;   // the allocation's base in the owner process
  uint64_t offset, size;
  int pid, pad;
};
struct RegShm {
  RegShmEntry e[kRegMaxEntries];
};

struct RegHandle {  // what ncclCommRegister hands out
  int entry;        // -1: the range counts as unregistered
};

struct RegComm {
  uint64_t threshold = 0;  // effective (plan.h reg_max); 0: no call is eligible
  RegTable table;          // my registrations
  RegShm* mine = nullptr;
  std::string shmName;
  bool linked = false;     // the name still exists
  std::vector<const RegShm*> peer;  // every rank's registry (mine included)
  std::vector<RegHandle*> handles;
  // the import cache
  struct Import {
    int peer;
    hipIpcMemHandle_t handle;
    void* base;
    int refs;
  };
  std::vector<Import> imports;
  int importOf[kDirectMaxRanks][kRegMaxEntries];
  uint32_t seen[kDirectMaxRanks][kRegMaxEntries];  // generation last processed
  RegPeers* tab = nullptr;     // the import table: host-pinned, mapped
  RegPeers* tabDev = nullptr;  // ... as the kernels address it
  RegStats* stats = nullptr;   // device-resident counters
  // The zero-copy all-to-all (VCCL_REG_A2A_THRESHOLD, plan.h reg_a2a_max; the
  // effective value is ncclComm::regA2aMaxBytes): its counters and the skip
  // words of a group's eligible calls, device-resident
  RegA2aDev* a2aDev = nullptr;
  // The zero-copy broadcast / reduce (VCCL_REG_ROOTED_THRESHOLD, plan.h
  // reg_rooted_max; the effective value is ncclComm::regRootedMaxBytes): its
  // three counters, device-resident, apart from `stats`
  RegStats* rootedStats = nullptr;
};

// init.cc: before the peer exchange (fills me->regShm / regOk), after the
// peers are mapped, after the init barrier, and at teardown.
void reg_create(ncclComm* c, PeerMap* me);
ncclResult_t reg_connect(ncclComm* c, bool anyNet);
ncclResult_t reg_a2a_alloc(ncclComm* c);  // RegComm::a2aDev, once (also vcclCommSetRegA2aThreshold)
ncclResult_t reg_rooted_alloc(ncclComm* c);  // RegComm::rootedStats, once (also vcclCommSetRegRootedThreshold)
void reg_unlink(ncclComm* c);
void reg_destroy(ncclComm* c);
// The API bodies on a comm with a registry.
ncclResult_t reg_register(ncclComm* c, void* buff, size_t size, void** handle);
ncclResult_t reg_deregister(ncclComm* c, void* handle);
// launch.cc: bring the import table up to date (no-op in the steady state).
ncclResult_t reg_refresh(ncclComm* c, bool capturing);
// {entry, generation, offset} of [p, p + bytes) in my registrations; entry
// kRegNone when it is not inside one.
void reg_describe(const ncclComm* c, const void* p, uint64_t bytes, uint32_t* entry, uint32_t* gen, uint64_t* off);
int reg_imported_count(const ncclComm* c);

}  // namespace vccl
#pragma GCC visibility pop
