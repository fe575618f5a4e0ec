// The registration table (reg.h): pure host code, no HIP call.
#include "reg.h"

#include <cstring>

namespace vccl {

void reg_table_clear(RegTable* t) { memset(t, 0, sizeof(*t)); }

int reg_insert(RegTable* t, uint64_t addr, uint64_t bytes) {
  if (bytes == 0 || addr + bytes < addr) return -1;
  for (int i = 0; i < kRegMaxEntries; i++) {
    RegEntry& e = t->e[i];
    if (reg_live(e)) continue;
    e.addr = addr;
    e.bytes = bytes;
    e.generation++;  // even -> odd: live
    return i;
  }
  return -1;
}

int reg_find(const RegTable* t, uint64_t addr, uint64_t bytes, uint64_t* offset) {
  if (addr + bytes < addr) return -1;
  for (int i = 0; i < kRegMaxEntries; i++) {
    const RegEntry& e = t->e[i];
    if (!reg_live(e) || addr < e.addr || addr - e.addr >= e.bytes) continue;
    if (bytes > e.bytes - (addr - e.addr)) continue;
    if (offset) *offset = addr - e.addr;
    return i;
  }
  return -1;
}

bool reg_remove(RegTable* t, int entry) {
  if (entry < 0 || entry >= kRegMaxEntries || !reg_live(t->e[entry])) return false;
  t->e[entry].generation++;  // odd -> even: free
  return true;
}

int reg_live_count(const RegTable* t) {
  int n = 0;
  for (const RegEntry& e : t->e) n += reg_live(e);
  return n;
}

}  // namespace vccl
