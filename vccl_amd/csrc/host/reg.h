// The registration table behind ncclCommRegister / ncclCommDeregister
// (reference: src/register/register.cc ncclRegister / ncclCommDeregister — a
// per-comm cache of registered ranges, looked up by address at enqueue).  Pure
// host code: plain integers, no runtime call, no communicator, so the table
// logic — insert, lookup of an interior pointer plus length, overlap, removal,
// generation, capacity — is checked on the CPU (vcclRegTable*, ext.cc).
//
// A table is a fixed array of kRegMaxEntries entries.  Every entry carries a
// generation that counts its writes like a seqlock: odd = live, even = free,
// +1 on insert, +1 on removal — so a reader that remembers (entry, generation)
// sees any later deregistration or reuse of the entry as a changed generation,
// and a reused entry never repeats a generation of a former occupant.
#pragma once
#include <cstddef>
#include <cstdint>

#pragma GCC visibility push(hidden)
namespace vccl {

constexpr int kRegMaxEntries = 32;

struct RegEntry {
  uint32_t generation;   // odd: live
  uint32_t pad;
  uint64_t addr, bytes;  // the registered range [addr, addr + bytes)
};
struct RegTable {
  RegEntry e[kRegMaxEntries];
};

inline bool reg_live(const RegEntry& e) { return (e.generation & 1u) != 0; }

void reg_table_clear(RegTable* t);
// Records [addr, addr + bytes) in the lowest free entry and returns its index;
// -1 when the table is full, bytes is 0 or the range wraps the address space
// (the range then simply counts as unregistered).  Ranges may overlap or
// repeat: every registration is an entry of its own with its own handle, as
// the API hands one out per call.
int reg_insert(RegTable* t, uint64_t addr, uint64_t bytes);
// The lowest live entry that holds the whole of [addr, addr + bytes) — an
// interior pointer is fine, one byte past the end is not, and a range that
// only the union of two entries covers is not registered.  bytes 0 asks for
// addr itself (addr == the end of a range is outside it).  -1: none.
int reg_find(const RegTable* t, uint64_t addr, uint64_t bytes, uint64_t* offset);
// Frees a live entry (generation + 1).  false: out of range or not live.
bool reg_remove(RegTable* t, int entry);
int reg_live_count(const RegTable* t);

}  // namespace vccl
#pragma GCC visibility pop
