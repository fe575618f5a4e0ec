// Zero-copy direct all-reduce / reduce-scatter / all-gather over
// ncclCommRegister'ed buffers (opt-in, VCCL_REG_THRESHOLD).
//
// Reference role: the reference's registered-buffer collectives
// (src/register/coll_reg.cc: with every rank's user buffer registered a
// kernel addresses the peers' buffers directly and the staging copies
// disappear).  Here: the direct kernels of direct.hpp without their inbox.
// A rank cannot know whether its peers passed registered buffers, so every
// rank launches this kernel for every eligible call (host/plan.cc
// reg_eligible) and the kernel settles the rest, on the direct grid, flags
// and epochs (workgroup b talks only to its namesakes):
//
//   epoch k (negotiate)
//     post (0, me, b) at every peer, my descriptor in the flag's 64-byte line
//          (written by the lane that raises the flag, drained before the flag
//          store: the inbox's payload-then-flag hand-off) — {entry,
//          generation, offset, bytes} of sendbuff in my registration table,
//          the all-reduce adds the same for recvbuff; an unregistered buffer
//          sends entry kRegNone.  An ordinary phase-0 flag: "my input is ready";
//     wait (0, *, b); ok_me = my own buffers are registered, and for every
//          peer: its descriptor names an entry my import table (RegPeers)
//          holds at the same generation, and offset + bytes lies inside it;
//     post (1, me, b) carrying ok_me;  wait (1, *, b);
//     D = AND of the n verdicts — the same in every workgroup of every rank.
//   D = 0: the staged direct path exactly — direct_*_part (direct.hpp) on the
//     geometry the DirectWork carries, from epoch k + 1 on.
//   D = 1, epoch k + 1: no inbox, one "chunk"; every rank PULLS (sc0 sc1 loads
//     from the peers' buffers) and stores into its own recvbuff only — nothing
//     here writes a peer's memory but flags.  The step list is host/plan.cc
//     reg_plan's, kept side by side with this order:
//       reduce-scatter  fold block b of shard `me` from the n inputs in the
//                       staged kernel's order (cbd_channel_of + rsOrder);
//                       post (0) "I have finished reading you"; wait (0);
//                       post (1); wait (1);
//       all-gather      copy block b of every rank's input into recvbuff (my
//                       own only when out of place); the same two rounds;
//       all-reduce      fold block b of shard `me` (direct_shard_elts of the
//                       whole count) from the n inputs, every element in the
//                       ring order its ar_chunk_of lookup gives (as
//                       direct_allreduce_part), write-through into my
//                       recvbuff; post (0) "shard `me` of my recvbuff is
//                       final, and I have finished reading your inputs";
//                       wait (0); pull block b of every other shard o from
//                       o's RECVBUFF; post (1) "finished reading your
//                       recvbuff"; wait (1).
//       In place is safe: shard o of any input is read only by o, and a rank
//       overwrites foreign shards of its buffer only after every peer's (0).
// Epoch positions per launch: 2 (zero-copy) or 1 + the staged count
// (fallback), the same on every rank since D is; R1 / R2 of direct.hpp hold in
// both epochs (the proof sits next to the rule in direct.hpp's header).
#pragma once
#include "direct.hpp"

namespace vccl {

// The pointers the negotiation resolved, rank-indexed (LDS).
struct RegResolved {
  const char* send[kDirectMaxRanks];
  const char* recv[kDirectMaxRanks];
  int ok[kDirectMaxRanks];
};

__device__ __forceinline__ void reg_st64(char* line, int off, uint64_t v) {
  __hip_atomic_store((uint64_t*)(line + off), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void reg_st32(char* line, int off, uint32_t v) {
  __hip_atomic_store((uint32_t*)(line + off), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t reg_ld64(const char* line, int off) {
  return __hip_atomic_load((const uint64_t*)(line + off), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint32_t reg_ld32(const char* line, int off) {
  return __hip_atomic_load((const uint32_t*)(line + off), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// direct_post with a payload in the line: lane k of wave 0 writes the words
// into flag line (phase, 0, me, b) at peer (me + k) mod n, drains, then raises
// the flag.  Layout: +0 epoch, +4 verdict (phase 1), +8 the RegDesc (phase 0).
__device__ __forceinline__ void reg_post(const DirectWork& w, const DirectPeers& P, int phase, int b, uint32_t e,
                                         const RegDesc* d, uint32_t verdict) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= 1 && k < w.nRanks) {
    const int p = w.rank + k < w.nRanks ? w.rank + k : w.rank + k - w.nRanks;
    char* line = P.flags[p] + direct_flag_off(phase, 0, w.rank, b);
    if (d) {
      reg_st64(line, 8, d->sendOff);
      reg_st64(line, 16, d->recvOff);
      reg_st64(line, 24, d->sendBytes);
      reg_st64(line, 32, d->recvBytes);
      reg_st32(line, 40, d->sendEntry);
      reg_st32(line, 44, d->sendGen);
      reg_st32(line, 48, d->recvEntry);
      reg_st32(line, 52, d->recvGen);
    } else {
      reg_st32(line, 4, verdict);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // payload, then flag
    if (w.comm->useFences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store((uint32_t*)line, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// One registered range of peer t as the descriptor names it, checked against
// my import table: the pointer, or nullptr.  `need`: the bytes I will read.
__device__ __forceinline__ const char* reg_resolve(const RegPeers* reg, int t, uint32_t entry, uint32_t gen,
                                                   uint64_t off, uint64_t bytes, uint64_t need) {
  if (entry >= (uint32_t)kRegTableEntries) return nullptr;
  const RegPeerEntry& pe = reg->e[t][entry];
  if (!pe.base || pe.generation != gen) return nullptr;
  const uint64_t len = bytes > need ? bytes : need;
  if (off > pe.size || len > pe.size - off) return nullptr;
  return pe.base + off;
}

// Epoch k.  Returns D; fills `rs` with every peer's pointers when D = 1.
__device__ __forceinline__ bool reg_negotiate(const DirectRegWork& rw, uint32_t e, RegResolved* rs, int* shFail) {
  const DirectWork& w = rw.w;
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, b = blockIdx.x, t = threadIdx.x;
  const char* myFlags = P.flags[me];
  reg_post(w, P, 0, b, e, &rw.mine, 0);
  const bool live = direct_wait(w, myFlags, 0, 0, b, e, shFail);
  if (t < n) {
    int ok = 0;
    const char* s = nullptr;
    const char* r = nullptr;
    if (t == me) {
      ok = (!(rw.needMine & kRegSend) || rw.mine.sendEntry != kRegNone) &&
           (!(rw.needMine & kRegRecv) || rw.mine.recvEntry != kRegNone);
    } else if (live) {
      // what I will read of rank t (the rooted kernels: by t's role)
      const uint8_t need = t == w.root ? rw.needRootPeer : rw.needPeer;
      const char* line = myFlags + direct_flag_off(0, 0, t, b);
      ok = 1;
      if (need & kRegSend) {
        s = reg_resolve(rw.reg, t, reg_ld32(line, 40), reg_ld32(line, 44), reg_ld64(line, 8), reg_ld64(line, 24),
                        rw.mine.sendBytes);
        ok = s != nullptr;
      }
      if (need & kRegRecv) {
        r = reg_resolve(rw.reg, t, reg_ld32(line, 48), reg_ld32(line, 52), reg_ld64(line, 16), reg_ld64(line, 32),
                        rw.mine.recvBytes);
        ok = ok && r != nullptr;
      }
    }
    rs->send[t] = s;
    rs->recv[t] = r;
    rs->ok[t] = ok;
  }
  __syncthreads();
  uint32_t okMe = 1;
  for (int q = 0; q < n; q++) okMe &= (uint32_t)rs->ok[q];
  reg_post(w, P, 1, b, e, nullptr, okMe);
  bool D = direct_wait(w, myFlags, 1, 0, b, e, shFail) && okMe;
  if (D)
    for (int q = 0; q < n; q++)
      if (q != me) D = D && reg_ld32(myFlags + direct_flag_off(1, 0, q, b), 4) != 0;
  __syncthreads();  // the verdict reads precede any later post
  return D;
}

// The two closing rounds of the one-hop zero-copy kernels.
__device__ __forceinline__ void reg_close(const DirectWork& w, const DirectPeers& P, int b, uint32_t e, int* shFail) {
  direct_post(w, P, 0, 0, b, e);
  (void)direct_wait(w, P.flags[w.rank], 0, 0, b, e, shFail);
  direct_post(w, P, 1, 0, b, e);
  (void)direct_wait(w, P.flags[w.rank], 1, 0, b, e, shFail);
}

template <class Fn>
__device__ __forceinline__ void reg_reducescatter_zc(const DirectRegWork& rw, const RegResolved& rs, uint32_t e,
                                                     int* shFail) {
  using T = typename Fn::EltType;
  constexpr int64_t esz = (int64_t)sizeof(T);
  const DirectWork& w = rw.w;
  const Fn fn(load_op_arg(w.redArgPtr, w.redArgBytes, w.redArg));
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int64_t count = (int64_t)w.count;
  const int64_t lo = (int64_t)b * rw.zcBlkElts < count ? (int64_t)b * rw.zcBlkElts : count;
  const int64_t hi = lo + rw.zcBlkElts < count ? lo + rw.zcBlkElts : count;
  char* out = (char*)w.recvbuff;
  for (int64_t cur = lo; cur < hi;) {
    int64_t end;
    const int ch = cbd_channel_of(w.cbd, cur, &end);
    end = end < hi ? end : hi;
    const int8_t* order = w.comm->rsOrder[ch % w.comm->nRings];
    const char* s[kDirectMaxRanks];
    char* d[kDirectMaxRanks] = {out + cur * esz};
#pragma unroll
    for (int j = 0; j < kDirectMaxRanks; j++) {
      const int q = j < n ? order[j] : me;
      s[j] = (q == me ? (const char*)w.sendbuff : rs.send[q]) + ((int64_t)me * count + cur) * esz;
    }
    direct_rc<Fn, kDirectUnroll, kSys, kSys, kSys>(fn, s, n, w.preOp ? n : 0, true, d, 1, end - cur, threadIdx.x,
                                                   blockDim.x);
    cur = end;
  }
  reg_close(w, *w.peers, b, e, shFail);
}

__device__ __forceinline__ void reg_allgather_zc(const DirectRegWork& rw, const RegResolved& rs, uint32_t e,
                                                 int* shFail) {
  using Fn = FnCopy<uint8_t>;
  const Fn fn(0);
  const DirectWork& w = rw.w;
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int64_t count = (int64_t)w.count;
  const int64_t lo = (int64_t)b * rw.zcBlkElts < count ? (int64_t)b * rw.zcBlkElts : count;
  const int64_t hi = lo + rw.zcBlkElts < count ? lo + rw.zcBlkElts : count;
  char* out = (char*)w.recvbuff;
  for (int k = 0; k < n; k++) {
    const int o = me + k < n ? me + k : me + k - n;
    const char* s[kDirectMaxRanks] = {(o == me ? (const char*)w.sendbuff : rs.send[o]) + lo};
    char* d[kDirectMaxRanks] = {out + (int64_t)o * count + lo};
    if (o == me && s[0] == d[0]) continue;  // in place: my block is already there
    direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, hi - lo, threadIdx.x, blockDim.x);
  }
  reg_close(w, *w.peers, b, e, shFail);
}

template <class Fn>
__device__ __forceinline__ void reg_allreduce_zc(const DirectRegWork& rw, const RegResolved& rs, uint32_t e,
                                                 int* shFail) {
  using T = typename Fn::EltType;
  constexpr int64_t esz = (int64_t)sizeof(T);
  const DirectWork& w = rw.w;
  const DirectPeers& P = *w.peers;
  const Fn fn(load_op_arg(w.redArgPtr, w.redArgBytes, w.redArg));
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t eltAlign = 16 / sizeof(T) ? 16 / sizeof(T) : 1;
  const int64_t count = (int64_t)w.count;
  const int64_t shardElts = direct_shard_elts(count, n, eltAlign);
  auto block_of = [&](int o, int64_t* off, int64_t* len) {  // block b of shard o
    int64_t shardEnd = (int64_t)(o + 1) * shardElts;
    shardEnd = shardEnd < count ? shardEnd : count;
    const int64_t lo = (int64_t)o * shardElts + (int64_t)b * rw.zcBlkElts;
    const int64_t hi = lo + rw.zcBlkElts < shardEnd ? lo + rw.zcBlkElts : shardEnd;
    *off = lo;
    *len = hi > lo ? hi - lo : 0;
  };
  char* out = (char*)w.recvbuff;
  {
    // The fold of my block: direct_allreduce_part's walk — each wave a span of
    // whole 16-byte packs, ring chunk by ring chunk — on the peers' inputs.
    int64_t off, len;
    block_of(me, &off, &len);
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int64_t span = ((len + eltAlign - 1) / eltAlign + nw - 1) / nw * eltAlign;
    int64_t cur = (int64_t)wv * span < len ? (int64_t)wv * span : len;
    const int64_t wend = cur + span < len ? cur + span : len;
    while (cur < wend) {
      int k;
      int64_t segEnd;
      const int ch = ar_chunk_of(w.cbd, w.arChunk, n, eltAlign, off + cur, &k, &segEnd);
      segEnd -= off;
      const int64_t end = segEnd < wend ? segEnd : wend;
      const int8_t* R = w.comm->ringAt[ch % w.comm->nRings];
      const char* s[kDirectMaxRanks];
      char* d[kDirectMaxRanks] = {out + (off + cur) * esz};
#pragma unroll
      for (int j = 0; j < kDirectMaxRanks; j++) {
        int pos = k + 1 + j;
        pos = pos >= n ? pos - n : pos;
        pos = pos >= n ? pos - n : pos;
        const int q = j < n ? __builtin_amdgcn_readfirstlane(R[pos]) : me;
        s[j] = (q == me ? (const char*)w.sendbuff : rs.send[q]) + (off + cur) * esz;
      }
      direct_rc<Fn, kDirectUnroll, kSys, kSys, kSys>(fn, s, n, w.preOp ? n : 0, true, d, 1, end - cur, lane, 64);
      cur = end;
    }
  }
  direct_post(w, P, 0, 0, b, e);
  if (direct_wait(w, P.flags[me], 0, 0, b, e, shFail)) {
    for (int k = 1; k < n; k++) {
      const int o = me + k < n ? me + k : me + k - n;
      int64_t off, len;
      block_of(o, &off, &len);
      const char* s[kDirectMaxRanks] = {rs.recv[o] + off * esz};
      char* d[kDirectMaxRanks] = {out + off * esz};
      direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, len, tid, nt);
    }
  }
  direct_post(w, P, 1, 0, b, e);
  (void)direct_wait(w, P.flags[me], 1, 0, b, e, shFail);
}

// ------------------------------------------------------- broadcast / reduce
// Zero-copy rooted collectives (opt-in, VCCL_REG_ROOTED_THRESHOLD; DESIGN.md
// §4.16): the two-hop kernels of direct.hpp with the user buffers in the place
// of the inbox.  Which buffers a rank announces and resolves follows its role
// (DirectRegWork::needMine / needPeer / needRootPeer, host/launch.cc): the
// broadcast root announces sendbuff, a non-root recvbuff (nothing at n = 2:
// nobody reads it) and never looks at its own sendbuff; a reduce announces
// sendbuff on every rank and recvbuff nowhere.  The step lists are host/plan.cc
// reg_rooted_plan's, kept side by side with these orders.
//
// Broadcast, D = 1, epoch k + 1 — one position, no inbox, any size.  Shards are
// direct_broadcast_part's of the WHOLE byte count (n - 1 shards of whole 16-byte
// units, shard j owned by direct_bcast_owner(root, j, n)); workgroup b moves
// bytes [b * zcBlkElts, (b + 1) * zcBlkElts) of a shard:
//   non-root o   pull my block of my shard from the ROOT's sendbuff into my
//                recvbuff (write-through, drained by the post);
//                post (0) "my shard in my recvbuff is final, and I have finished
//                reading the root";  wait (0) on every peer;
//                pull block b of every other shard from its OWNER's recvbuff;
//                post (1) "finished reading your recvbuff";  wait (1);
//   root         copy send -> recv locally when they differ; post (0); wait (0)
//                — only now is its sendbuff released; post (1); wait (1).
// Every rank writes only its own recvbuff, flags aside.  In place (ncclBcast)
// needs no extra care: shard o of a rank's buffer is read only from its owner
// o, and only after o's (0).  Alignments differ freely (direct_rc's shifted path).
__device__ __forceinline__ void reg_broadcast_zc(const DirectRegWork& rw, const RegResolved& rs, uint32_t e,
                                                 int* shFail) {
  using Fn = FnCopy<uint8_t>;
  const Fn fn(0);
  const DirectWork& w = rw.w;
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, root = w.root, b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t count = (int64_t)w.count;  // bytes
  const int64_t shard = direct_shard_elts(count, n - 1, 16);
  auto block_of = [&](int j, int64_t* off, int64_t* len) {  // block b of shard j
    int64_t shardEnd = (int64_t)(j + 1) * shard;
    shardEnd = shardEnd < count ? shardEnd : count;
    const int64_t lo = (int64_t)j * shard + (int64_t)b * rw.zcBlkElts;
    const int64_t hi = lo + rw.zcBlkElts < shardEnd ? lo + rw.zcBlkElts : shardEnd;
    *off = lo;
    *len = hi > lo ? hi - lo : 0;
  };
  char* out = (char*)w.recvbuff;
  if (me != root) {
    int64_t off, len;
    block_of(direct_bcast_shard_of(root, me, n), &off, &len);
    const char* s[kDirectMaxRanks] = {rs.send[root] + off};
    char* d[kDirectMaxRanks] = {out + off};
    direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, len, tid, nt);
  } else if ((const char*)w.sendbuff != out) {
    for (int j = 0; j < n - 1; j++) {
      int64_t off, len;
      block_of(j, &off, &len);
      const char* s[kDirectMaxRanks] = {(const char*)w.sendbuff + off};
      char* d[kDirectMaxRanks] = {out + off};
      direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, len, tid, nt);
    }
  }
  direct_post(w, P, 0, 0, b, e);
  if (direct_wait(w, P.flags[me], 0, 0, b, e, shFail) && me != root) {
    for (int k = 1; k < n; k++) {
      const int o = me + k < n ? me + k : me + k - n;
      if (o == root) continue;
      int64_t off, len;
      block_of(direct_bcast_shard_of(root, o, n), &off, &len);
      const char* s[kDirectMaxRanks] = {rs.recv[o] + off};
      char* d[kDirectMaxRanks] = {out + off};
      direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, len, tid, nt);
    }
  }
  direct_post(w, P, 1, 0, b, e);
  (void)direct_wait(w, P.flags[me], 1, 0, b, e, shFail);
}

// Reduce, D = 1 — direct_reduce_part minus its scatter, on the same DirectWork
// chunk geometry (so either outcome consumes 1 + nChunks positions; `e` enters
// as chunk 0's epoch and leaves as the last chunk's).  Per chunk:
//   post (0); wait (0)   no data moves: the round keeps R1 and orders the root's
//                collect of the previous chunk before anyone rewrites a (1, *)
//                region;
//   fold         owner o folds block b of shard o from the n USER INPUTS (peer
//                pointers for q != me, sendbuff for q = me) in exactly
//                direct_reduce_part's order — the channel from the call's cbd
//                under SIMPLE, ringAt[ch mod nRings], from the root's successor
//                round to the root, preOp on every input, postOp once; the root
//                straight into recvbuff, any other owner into region (1, o) of
//                the ROOT's inbox (the staged push, unchanged);
//   post (1)     "my shard is delivered, and I have finished reading your
//                inputs of this chunk";  wait (1);
//   collect      the root copies its regions (1, o) into recvbuff.
// A non-root never touches recvbuff.  In place at the root is legal: shard o of
// the root's input is read by o alone and overwritten only after o's (1).
template <class Fn>
__device__ __forceinline__ void reg_reduce_zc(const DirectRegWork& rw, const RegResolved& rs, uint32_t& e,
                                              int* shFail) {
  using T = typename Fn::EltType;
  constexpr int64_t esz = (int64_t)sizeof(T);
  const DirectWork& w = rw.w;
  const Fn fn(load_op_arg(w.redArgPtr, w.redArgBytes, w.redArg));
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, root = w.root, b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t eltAlign = 16 / sizeof(T) ? 16 / sizeof(T) : 1;
  const int64_t count = (int64_t)w.count;
  char* myBuf = P.buf[me];
  const char* myFlags = P.flags[me];
  const int64_t inOff = (int64_t)b * w.blkElts * esz;  // block offset in a region
  for (int c = 0; c < w.nChunks; c++) {
    if (c) e = epoch_after(e);
    if (*shFail) continue;
    const int64_t c0 = (int64_t)c * w.chunkElts;
    const int64_t cc = count - c0 < w.chunkElts ? count - c0 : w.chunkElts;
    const int64_t shardElts = direct_shard_elts(cc, n, eltAlign);
    auto block_of = [&](int o, int64_t* off, int64_t* len) {  // block b of shard o, chunk-relative
      int64_t shardEnd = (int64_t)(o + 1) * shardElts;
      shardEnd = shardEnd < cc ? shardEnd : cc;
      const int64_t lo = (int64_t)o * shardElts + (int64_t)b * w.blkElts;
      const int64_t hi = lo + w.blkElts < shardEnd ? lo + w.blkElts : shardEnd;
      *off = lo;
      *len = hi > lo ? hi - lo : 0;
    };
    direct_post(w, P, 0, 0, b, e);
    if (direct_wait(w, myFlags, 0, 0, b, e, shFail)) {
      int64_t off, len;
      block_of(me, &off, &len);
      for (int64_t cur = 0; cur < len;) {
        int64_t end;
        const int ch = cbd_channel_of(w.cbd, c0 + off + cur, &end);
        end -= c0 + off;
        end = end < len ? end : len;
        const int8_t* R = w.comm->ringAt[ch % w.comm->nRings];
        int k = 0;  // the root's position on this ring
#pragma unroll
        for (int p = 0; p < kDirectMaxRanks; p++)
          if (p < n && R[p] == root) k = p;
        k = __builtin_amdgcn_readfirstlane(k);
        const char* s[kDirectMaxRanks];
        char* d[kDirectMaxRanks] = {
            me == root ? (char*)w.recvbuff + (c0 + off + cur) * esz
                       : P.buf[root] + direct_region_off(1, 0, me, n, w.regionBytes) + inOff + cur * esz};
#pragma unroll
        for (int j = 0; j < kDirectMaxRanks; j++) {
          int pos = k + 1 + j;
          pos = pos >= n ? pos - n : pos;
          pos = pos >= n ? pos - n : pos;
          const int q = j < n ? __builtin_amdgcn_readfirstlane(R[pos]) : me;
          s[j] = (q == me ? (const char*)w.sendbuff : rs.send[q]) + (c0 + off + cur) * esz;
        }
        direct_rc<Fn, kDirectUnroll, kSys, kSys, kSys>(fn, s, n, w.preOp ? n : 0, true, d, 1, end - cur, tid, nt);
        cur = end;
      }
    }
    direct_post(w, P, 1, 0, b, e);
    if (direct_wait(w, myFlags, 1, 0, b, e, shFail) && me == root) {
      for (int k = 1; k < n; k++) {
        const int o = me + k < n ? me + k : me + k - n;
        int64_t off, len;
        block_of(o, &off, &len);
        const char* s[kDirectMaxRanks] = {myBuf + direct_region_off(1, 0, o, n, w.regionBytes) + inOff};
        char* d[kDirectMaxRanks] = {(char*)w.recvbuff + (c0 + off) * esz};
        direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, len, tid, nt);
      }
    }
  }
}

// One launch: negotiate, then `zc` (zero-copy: one epoch, the reduce one per
// chunk — it advances `e` itself) or `staged` (the direct_*_part of the
// collective).  The counters are workgroup 0's.
template <class ZC, class Staged>
__device__ __forceinline__ void direct_reg_run(const DirectRegWork& rw, ZC zc, Staged staged) {
  __shared__ int shFail;
  __shared__ RegResolved rs;
  const DirectWork& w = rw.w;
  uint32_t e = epoch_after(__hip_atomic_load(&w.comm->dEpoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  if (threadIdx.x == 0) shFail = 0;
  __syncthreads();
  const bool D = reg_negotiate(rw, e, &rs, &shFail);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicAdd(&rw.stats->launches, 1ull);
    atomicAdd(D ? &rw.stats->zeroCopy : &rw.stats->fallback, 1ull);
  }
  if (D) {
    e = epoch_after(e);
    zc(rw, rs, e, &shFail);
  } else {
    staged(w, e, shFail);
  }
  epoch_retire(&w.comm->dEpoch, &w.comm->dDone, e);
}

// ---------------------------------------------------------------- all-to-all
// Zero-copy all-to-all(v) (opt-in, VCCL_REG_A2A_THRESHOLD): a
// launch of its own on the direct grid, ahead of the call's FIFO items in the
// comm's p2p launch.  Only sendbuff has to be registered — nobody touches a
// peer's recvbuff.  The step list is host/plan.cc reg_a2a_plan's, kept side by
// side with this order:
//   epoch k (negotiate)
//     post (0, me, b) at every peer p with the descriptor of MY BLOCK FOR p in
//          the flag's line (reg_post's layout, the send words only): {entry,
//          generation, offset of the block inside my registration, its bytes};
//          kRegNone when the block is empty or not registered;
//     wait (0, *, b); ok_me = the host's part (every block I send is
//          registered; a v-call: my largest pair reaches the threshold), and
//          for every peer I receive from: its descriptor names an entry my
//          import table holds at that generation, offset + bytes lies inside
//          it, and bytes equals what I expect;
//     post (1, me, b) carrying ok_me;  wait (1, *, b);  D = AND of the n votes.
//   D = 1, epoch k + 1: for k = 1 .. n - 1 pull slice b of the block rank
//     (me + k) mod n holds for me (sc0 sc1 loads) into my recvbuff, any
//     alignment on either side (direct_rc's shifted path); the self block is a
//     local copy; reg_close.  Nothing writes a peer's memory but flags.
//   D = 0: nothing more — the FIFO items behind this launch move the call.
// Workgroup 0 stores D into the call's skip word (p2p.hpp drops the call's FIFO
// items on D = 1) and bumps the counters.  Epoch positions per launch: 2 or 1,
// the same on every rank since D is; R1 / R2 of direct.hpp hold in both epochs
// exactly as for the zero-copy AR / RS / AG (the header's list).
__device__ __forceinline__ void reg_a2a_post(const DirectWork& w, const DirectPeers& P, int b, uint32_t e,
                                             const RegA2aPeer* sh) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= 1 && k < w.nRanks) {
    const int p = w.rank + k < w.nRanks ? w.rank + k : w.rank + k - w.nRanks;
    char* line = P.flags[p] + direct_flag_off(0, 0, w.rank, b);
    reg_st64(line, 8, sh[k].regOff);
    reg_st64(line, 24, (uint64_t)sh[k].sendBytes);
    reg_st32(line, 40, sh[k].entry);
    reg_st32(line, 44, sh[k].gen);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // payload, then flag
    if (w.comm->useFences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store((uint32_t*)line, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__device__ __forceinline__ void direct_reg_alltoall(const DirectRegA2aWork& w) {
  using Fn = FnCopy<uint8_t>;
  const Fn fn(0);
  __shared__ RegA2aPeer sh[kDirectMaxRanks];   // rotated: entry k = rank (me + k) mod n
  __shared__ const char* shSrc[kDirectMaxRanks];
  __shared__ int shOk[kDirectMaxRanks];
  __shared__ int shFail;
#pragma unroll
  for (int i = 0; i < kDirectMaxRanks; i++)
    if ((int)threadIdx.x == i) sh[i] = w.peer[i];
  if (threadIdx.x == 0) shFail = 0;
  __syncthreads();
  // what direct_wait / direct_post / reg_post read of a DirectWork
  DirectWork dw{};
  dw.comm = w.comm;
  dw.nRanks = w.nRanks;
  dw.rank = w.rank;
  const DirectPeers& P = *w.peers;
  const int n = w.nRanks, me = w.rank, b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const char* myFlags = P.flags[me];
  uint32_t e = epoch_after(__hip_atomic_load(&w.comm->dEpoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  reg_a2a_post(dw, P, b, e, sh);
  const bool live = direct_wait(dw, myFlags, 0, 0, b, e, &shFail);
  if (tid < n) {  // thread k: rank (me + k) mod n
    const int k = tid, q = me + k < n ? me + k : me + k - n;
    int ok = 0;
    const char* s = nullptr;
    if (k == 0) {
      ok = w.selfOk;
    } else if (live) {
      const uint64_t need = (uint64_t)sh[k].recvBytes;
      if (need == 0) {
        ok = 1;
      } else {
        const char* line = myFlags + direct_flag_off(0, 0, q, b);
        const uint64_t bytes = reg_ld64(line, 24);
        s = reg_resolve(w.reg, q, reg_ld32(line, 40), reg_ld32(line, 44), reg_ld64(line, 8), bytes, need);
        ok = s != nullptr && bytes == need;
      }
    }
    shSrc[k] = s;
    shOk[k] = ok;
  }
  __syncthreads();
  uint32_t okMe = 1;
  for (int k = 0; k < n; k++) okMe &= (uint32_t)shOk[k];
  reg_post(dw, P, 1, b, e, nullptr, okMe);
  bool D = direct_wait(dw, myFlags, 1, 0, b, e, &shFail) && okMe;
  if (D)
    for (int q = 0; q < n; q++)
      if (q != me) D = D && reg_ld32(myFlags + direct_flag_off(1, 0, q, b), 4) != 0;
  __syncthreads();  // the verdict reads precede any later post
  if (b == 0 && tid == 0) {
    w.dev->skip[w.skipIdx] = D ? 1u : 0u;
    atomicAdd(&w.dev->stats.launches, 1ull);
    atomicAdd(D ? &w.dev->stats.zeroCopy : &w.dev->stats.fallback, 1ull);
  }
  if (D) {
    e = epoch_after(e);
    for (int k = 1; k < n; k++) {  // rotated: every rank starts at its own successor
      const int64_t lo = (int64_t)b * sh[k].blkBytes;
      const int64_t hi = lo + sh[k].blkBytes < sh[k].recvBytes ? lo + sh[k].blkBytes : sh[k].recvBytes;
      if (hi <= lo) continue;
      const char* s[kDirectMaxRanks] = {shSrc[k] + lo};
      char* d[kDirectMaxRanks] = {sh[k].recv + lo};
      direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, hi - lo, tid, nt);
    }
    if (sh[0].send != sh[0].recv) {  // the self block (nothing when already in place)
      const int64_t lo = (int64_t)b * sh[0].blkBytes;
      const int64_t hi = lo + sh[0].blkBytes < sh[0].recvBytes ? lo + sh[0].blkBytes : sh[0].recvBytes;
      if (hi > lo) {
        const char* s[kDirectMaxRanks] = {sh[0].send + lo};
        char* d[kDirectMaxRanks] = {sh[0].recv + lo};
        direct_rc<Fn, kDirectCopyUnroll, kSys, kSys, kSys>(fn, s, 1, 0, false, d, 1, hi - lo, tid, nt);
      }
    }
    reg_close(dw, P, b, e, &shFail);
  }
  epoch_retire(&w.comm->dEpoch, &w.comm->dDone, e);
}

}  // namespace vccl
