// The SIMPLE ring of the fp32-accumulated sums (FnSumWide / FnPreMulSumWide
// over f16, bf16, e4m3, e5m2): the ring all-reduce and
// reduce-scatter of ring.hpp with the running sum travelling in binary32.
//
// Wire format of one chunk on its way round the ring:
//   hop 1        the sender's raw elements of type T — the native send-only
//                step, untouched (FnSum<T> as the copy functor, the native
//                slot offsets, no premultiply);
//   hops 2 ..    the running sum as binary32 from slot offset 0, in the
//                reduce-scatter phase;
//   final step   one narrowing (Wide<T>::down / down_word): T to the user
//                output and, in the all-reduce, T to the next rank's slot —
//                the all-gather phase is the native copy steps.
// The receiver of a raw hop applies pre(x) = widen(x) * scalar to the received
// element and to its own, the receiver of a binary32 hop to its own only; the
// first source of the fold is assigned, every later one added in binary32:
//   y = narrow_T((pre(x_0) + pre(x_1)) + ...),  x_0 the ring successor of the
// chunk's finishing position — the order of the native ring and of the staged
// direct wide kernels.
//
// A hop crosses the FIFO slot by slot: ceil(nelem / (slotBytes / 4)) slices
// in binary32, ceil(nelem / (slotBytes / sizeof(T))) in T, both derived from
// the same nelem on either side.  A step whose two sides use different
// formats walks the finer slices and takes / posts the coarser slot at its
// first / last one.
//
// Sub-chunks.  A ring step's hop stays in the FIFO until the successor's NEXT
// step, so a hop may span at most kSteps / 2 slots (host/setup.cc
// step_and_slot; the native chunk is exactly that: 4 steps).  The same chunk
// in binary32 would span 8 (f16 / bf16) or 16 (fp8) and every rank would wait
// for a credit only its successor's next step can give.  So with n > 2 each
// chunk goes round in 4 / sizeof(T) passes, pass q moving sub-range q of every
// chunk of the loop through the whole schedule: a binary32 hop is again at
// most 4 slots, credits, kSteps and the host's partition are the native
// ring's, and every element still finishes at the ring position of its chunk
// — the fold order does not change.
//
// The hand-off is prim_wg's (workgroup barrier pair, drain, post by thread
// 0); the per-wave hand-off, LL128 and net peers are not served.
#pragma once
#include "ring.hpp"

namespace vccl {

enum : int { kWireRaw = 0, kWireF32 = 1 };                           // what the receive slot holds
enum : int { kWideToF32Slot = 0, kWideToUser = 1, kWideToUserSlot = 2 };  // where the fold goes

// 16-byte packs of own input per thread in flight: 2 for every type, in the
// folds and in the kernels' native copy steps.  A fold's pack is 4 registers
// of own input and 8 (f16 / bf16) or 16 (fp8) of binary32 slot words that
// become the accumulator.  The 16-bit all-reduce kernels, which carry four
// folds and three native copy steps, need scratch with either at kRingUnroll
// (bf16: 132 bytes, 66 VGPR spills with the copies at 4; 448 / 328 with both
// at 4); at 2 and 2 no instantiation does (direct_fold_unroll's rule; DESIGN
// §4.17.2 has the table).
#ifndef VCCL_RING_WIDE_UNROLL
#define VCCL_RING_WIDE_UNROLL 2
#endif
template <class Fn>
constexpr int ring_wide_unroll() { return VCCL_RING_WIDE_UNROLL; }
#ifndef VCCL_RING_WIDE_COPY_UNROLL
#define VCCL_RING_WIDE_COPY_UNROLL 2
#endif
template <class T>
constexpr int ring_wide_copy_unroll() { return VCCL_RING_WIDE_COPY_UNROLL; }

// Four binary32 words of a slot <-> two accumulator pairs.  Through scalar
// temporaries: __builtin_bit_cast applied to a vector component (v.y) reads
// component 0 of the vector.
__device__ __forceinline__ void quad_to_f32(u32x4 v, f32x2* p) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  p[0] = f32x2{__builtin_bit_cast(float, w[0]), __builtin_bit_cast(float, w[1])};
  p[1] = f32x2{__builtin_bit_cast(float, w[2]), __builtin_bit_cast(float, w[3])};
}
__device__ __forceinline__ u32x4 quad_of_f32(const f32x2* p) {
  const float f[4] = {p[0].x, p[0].y, p[1].x, p[1].y};
  return u32x4{__builtin_bit_cast(uint32_t, f[0]), __builtin_bit_cast(uint32_t, f[1]), __builtin_bit_cast(uint32_t, f[2]),
               __builtin_bit_cast(uint32_t, f[3])};
}

// acc = in (+) pre(own) over nelem elements: `in` raw T (pre applied, the
// fold's first source) or binary32; the result as binary32 to `slot`, or
// narrowed to `user` (and to `slot`).  Own input nt, slots sc0 sc1.
//
// Packs when every T-typed operand shares one address modulo 16: the < 16
// bytes up to the boundary and the tail go element by element, the binary32
// operand then sits at a 4-byte-aligned offset (dwordx4 accesses need no
// more).  Operands that disagree modulo 16 take the element path for the
// whole slice: no realignment here.
template <class Fn, int IN, int OUT, int U>
__device__ __forceinline__ void wide_fold(const Fn& fn, const char* own, const char* in, char* slot, char* user,
                                          int64_t nelem, int tid, int nthreads) {
  using T = typename Fn::EltType;
  using W = Wide<T>;
  constexpr int EPP = 16 / (int)sizeof(T);  // elements per pack
  constexpr int NQ = EPP / 4;               // 16-byte quads of binary32 per pack
  constexpr int OWNP = VCCL_RING_SRC_POL;
  constexpr int USERP = OUT == kWideToUser ? VCCL_RING_OUT_POL : VCCL_RING_OUT2_POL;
  const uintptr_t m = (uintptr_t)own & 15;
  bool agree = m % sizeof(T) == 0;
  if (IN == kWireRaw) agree &= ((uintptr_t)in & 15) == m;
  if (OUT != kWideToF32Slot) agree &= ((uintptr_t)user & 15) == m;
  if (OUT == kWideToUserSlot) agree &= ((uintptr_t)slot & 15) == m;
  int64_t head = agree ? (int64_t)((16 - m) & 15) / (int64_t)sizeof(T) : 0;
  if (head > nelem) head = nelem;
  const int64_t nPacks = agree ? (nelem - head) / EPP : 0;
  const int64_t tail0 = head + nPacks * EPP;

  const char* ownB = own + head * (int64_t)sizeof(T);
  const char* inB = in + head * (int64_t)(IN == kWireRaw ? sizeof(T) : 4);
  char* slotB = slot + head * (int64_t)(OUT == kWideToF32Slot ? 4 : sizeof(T));
  char* userB = user + head * (int64_t)sizeof(T);
  for (int64_t base = 0; base < nPacks; base += (int64_t)nthreads * U) {
    u32x4 o[U], r[U][IN == kWireRaw ? 1 : NQ];
    // every load of the hunk before the first add
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t p = base + (int64_t)u * nthreads + tid;
      if (p < nPacks) {
        o[u] = ld16<OWNP>(ownB, p * 16);
        if constexpr (IN == kWireRaw) {
          r[u][0] = ld16<kSys>(inB, p * 16);
        } else {
#pragma unroll
          for (int q = 0; q < NQ; q++) r[u][q] = ld16<kSys>(inB, p * (int64_t)(EPP * 4) + q * 16);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t p = base + (int64_t)u * nthreads + tid;
      if (p < nPacks) {
        WidePack<T> a;
        if constexpr (IN == kWireRaw) {
          a = acc_first(fn, r[u][0], true);
        } else {
#pragma unroll
          for (int q = 0; q < NQ; q++) quad_to_f32(r[u][q], &a.p[2 * q]);
        }
        acc_add(fn, a, o[u], true);  // widen (up_word), premultiply, v_pk_add_f32
        if constexpr (OUT == kWideToF32Slot) {
#pragma unroll
          for (int q = 0; q < NQ; q++) st16<kSys>(slotB, p * (int64_t)(EPP * 4) + q * 16, quad_of_f32(&a.p[2 * q]));
        } else {
          const u32x4 y = acc_done(fn, a, true);  // the one narrowing (down_word)
          if constexpr (OUT == kWideToUserSlot) st16<kSys>(slotB, p * 16, y);
          st16<USERP>(userB, p * 16, y);
        }
      }
    }
  }
  // Element path: the head, the tail, or (operands apart modulo 16) the slice.
  const int64_t nEdge = head + (nelem - tail0);
  for (int64_t e = tid; e < nEdge; e += nthreads) {
    const int64_t i = e < head ? e : tail0 + (e - head);
    const T x = ldT<OWNP, T>(own, i);
    float a;
    if constexpr (IN == kWireRaw) a = elt_first(fn, ldT<kSys, T>(in, i), true);
    else a = ldT<kSys, float>(in, i);
    elt_add(fn, a, x, true);
    if constexpr (OUT == kWideToF32Slot) {
      stT<kSys, float>(slot, i, a);
    } else {
      const T y = W::down(a);
      if constexpr (OUT == kWideToUserSlot) stT<kSys, T>(slot, i, y);
      stT<USERP, T>(user, i, y);
    }
  }
}

// One slot hand-off of the wide ring: RingCtx::prim_wg with the fold above.
// Always receives; sends unless OUT is the user output alone.  in / slot:
// this slice inside the current receive / send slot.  acqRecv / relRecv (and
// acqSend / relSend): this slice is the first / last one of its slot on that
// side — the credit is awaited at the first, the flag posted and the step
// counted at the last; a slice in between touches neither flag of that side.
template <class Fn, int IN, int OUT, int U>
__device__ __forceinline__ void prim_wide(RingCtx& r, const Fn& fn, const void* src, void* dst, int64_t nelem,
                                          int64_t inOff, int64_t slotOff, bool acqRecv, bool relRecv, bool acqSend,
                                          bool relSend) {
  constexpr bool SEND = OUT != kWideToUser;
  const bool tr = r.trace != nullptr && r.traceN < r.traceCap;
  uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, tc = 0;
  if (r.tid == 0 && !r.aborted()) {
    if (tr) t0 = __builtin_amdgcn_s_memrealtime();
    bool ok = true;
    if (acqRecv) ok = r.spin_ge(r.recvTail, r.recvStep + 1);
    if (SEND && acqSend && ok && r.sendStep + 1 > (uint64_t)kSteps) ok = r.spin_ge(r.sendHead, r.sendStep + 1 - kSteps);
    if (!ok) r.set_aborted();
    if (r.useFences) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system-scope acquire
      drain_vmem();
    }
    if (tr) t1 = __builtin_amdgcn_s_memrealtime();
  }
  __syncthreads();
  if (r.aborted()) return;
  if (r.tid == 0 && tr) t2 = __builtin_amdgcn_s_memrealtime();
  if (nelem > 0) {
    const char* in = r.recvFifo + (int64_t)(r.recvStep % kSteps) * slot_stride(r.slotBytes) + inOff;
    char* slot = SEND ? r.sendFifo + (int64_t)(r.sendStep % kSteps) * slot_stride(r.slotBytes) + slotOff : nullptr;
    wide_fold<Fn, IN, OUT, U>(fn, (const char*)src, in, slot, (char*)dst, nelem, r.tid, r.nthreads);
  }
  if (r.tid == 0 && tr) tc = __builtin_amdgcn_s_memrealtime();
  drain_vmem();  // every storing wave: its write-through payload stores are complete
  __syncthreads();
  if (r.tid == 0) {
    if (tr) t3 = __builtin_amdgcn_s_memrealtime();
    if (r.useFences) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system-scope release (L2 writeback)
      drain_vmem();
    }
    if (SEND && relSend) st_sys(r.nextRecvTail, r.sendStep + 1);
    if (relRecv) st_sys(r.prevSendHead, r.recvStep + 1);
    if (tr) {
      VCCL_GLOBAL RingTraceRec& rec = r.trace[r.traceN];
      rec.t0 = t0;
      rec.t1 = t1;
      rec.t2 = t2;
      rec.t3 = t3;
      rec.t4 = __builtin_amdgcn_s_memrealtime();
      rec.shape = 1u | (SEND ? 2u : 0u) | 4u | (OUT != kWideToF32Slot ? 8u : 0u);
      rec.bytes = (uint32_t)(nelem > 0 ? nelem * (int64_t)sizeof(typename Fn::EltType) : 0);
      rec.step = SEND ? r.sendStep : r.recvStep;
      rec.tc = tc;
    }
  }
  if (tr) r.traceN++;
  if (SEND && relSend) r.sendStep++;
  if (relRecv) r.recvStep++;
}

// One ring step of `nelem` elements on the wide ring.  recvOff / sendOff: the
// byte offset of a raw T chunk inside its slots (the native step's); a
// binary32 slice starts at slot offset 0.  An empty step hands over one empty
// slot on each side.
template <class Fn, int IN, int OUT, int U>
__device__ __forceinline__ void ring_step_wide(RingCtx& r, const Fn& fn, const void* src, void* dst, int64_t nelem,
                                               int recvOff = 0, int sendOff = 0) {
  using T = typename Fn::EltType;
  const int64_t eltsT = (int64_t)r.slotBytes / (int64_t)sizeof(T), elts32 = (int64_t)r.slotBytes / 4;
  const int64_t inElts = IN == kWireF32 ? elts32 : eltsT, outElts = OUT == kWideToF32Slot ? elts32 : eltsT;
  const int64_t g = inElts < outElts ? inElts : outElts;  // the finer side's slice; it divides the coarser
  const int64_t nSlices = nelem > 0 ? div_up(nelem, g) : 1;
  for (int64_t s = 0; s < nSlices; s++) {
    const int64_t o = s * g;
    int64_t len = nelem - o < g ? nelem - o : g;
    if (len < 0) len = 0;
    const bool last = s == nSlices - 1;
    const int64_t inSub = o % inElts, outSub = o % outElts;
    const void* sp = (const void*)((const T*)src + o);
    void* dp = OUT != kWideToF32Slot ? (void*)((T*)dst + o) : nullptr;
    prim_wide<Fn, IN, OUT, U>(r, fn, sp, dp, len, IN == kWireF32 ? 0 : recvOff + inSub * (int64_t)sizeof(T),
                              OUT == kWideToF32Slot ? 0 : sendOff + outSub * (int64_t)sizeof(T), inSub == 0,
                              last || inSub + g == inElts, outSub == 0, last || outSub + g == outElts);
  }
}

// Elements per pass of a chunk of chunkCount elements (the sub-chunks above):
// the chunk's 4 / sizeof(T)-th part, a multiple of 16 bytes; the whole chunk
// at n == 2, where no binary32 crosses a link.  The same on every rank.
template <class T>
__device__ __forceinline__ int64_t wide_sub_chunk(int64_t chunkCount, int n) {
  const int64_t passes = n == 2 ? 1 : 4 / (int64_t)sizeof(T), eltAlign = 16 / sizeof(T);
  return align_up(div_up(chunkCount, passes), eltAlign);
}

// ----------------------------------------------------------------- AllReduce
// ring_allreduce's schedule (same chunks, same steps); n == 2 has no binary32
// hop: the raw chunk is folded and narrowed by its one receiver.
template <class Fn, int U>
__device__ __forceinline__ void ring_allreduce_wide(RingCtx& r, const Fn& fn, const RingWork& w, int c) {
  using T = typename Fn::EltType;
  using CFn = FnSum<T>;  // the native steps copy (one source)
  constexpr int CU = ring_wide_copy_unroll<T>();
  const CFn cfn;
  const int n = w.nRanks;
  const int64_t eltAlign = 16 / sizeof(T);
  int64_t gridOff, chCount, chunkCount;
  if (!cbd_part(w, c, &gridOff, &chCount, &chunkCount)) return;
  const T* in = (const T*)w.sendbuff;
  T* out = (T*)w.recvbuff;
  const int ringIx = r.ringPos;
  const int64_t loopCount = (int64_t)n * chunkCount;
  auto modRanks = [n](int x) { return x >= n ? x - n : x; };
  for (int64_t eo = 0; eo < chCount; eo += loopCount) {
    const int64_t rem = chCount - eo;
    if (rem < loopCount) chunkCount = align_up(div_up(rem, n), eltAlign);
    const int64_t sub = wide_sub_chunk<T>(chunkCount, n);
    for (int64_t so = 0; so < chunkCount; so += sub) {  // the passes (one when n == 2)
      auto off_of = [&](int chunk) { return gridOff + eo + chunk * chunkCount + so; };
      auto len_of = [&](int chunk) {
        int64_t l = rem - (int64_t)chunk * chunkCount;
        l = (l < chunkCount ? (l < 0 ? 0 : l) : chunkCount) - so;  // what the chunk holds from `so` on
        return l < sub ? (l < 0 ? 0 : l) : sub;
      };
      int chunk = modRanks(ringIx + n - 1);  // step 0: own chunk, raw
      ring_step<CFn, false, true, true, false, CU>(r, cfn, in + off_of(chunk), nullptr, len_of(chunk), false);
      for (int j = 2; j < n; ++j) {  // n-2 recv-fold-send: binary32 out, raw in at the first
        chunk = modRanks(ringIx + n - j);
        if (j == 2)
          ring_step_wide<Fn, kWireRaw, kWideToF32Slot, U>(r, fn, in + off_of(chunk), nullptr, len_of(chunk));
        else
          ring_step_wide<Fn, kWireF32, kWideToF32Slot, U>(r, fn, in + off_of(chunk), nullptr, len_of(chunk));
      }
      chunk = ringIx;  // final fold: narrowed once, output + send
      if (n == 2)
        ring_step_wide<Fn, kWireRaw, kWideToUserSlot, U>(r, fn, in + off_of(chunk), out + off_of(chunk),
                                                         len_of(chunk));
      else
        ring_step_wide<Fn, kWireF32, kWideToUserSlot, U>(r, fn, in + off_of(chunk), out + off_of(chunk),
                                                         len_of(chunk));
      for (int j = 1; j < n - 1; ++j) {  // the all-gather phase: native copies
        chunk = modRanks(ringIx + n - j);
        ring_step<CFn, true, true, false, true, CU>(r, cfn, nullptr, out + off_of(chunk), len_of(chunk), false);
      }
      chunk = modRanks(ringIx + 1);
      ring_step<CFn, true, false, false, true, CU>(r, cfn, nullptr, out + off_of(chunk), len_of(chunk), false);
    }
  }
}

// ------------------------------------------------------------- ReduceScatter
// ring_reducescatter's schedule; the raw first hop keeps the native slot
// offset (the block's misalignment), the binary32 hops start at offset 0.
template <class Fn, int U>
__device__ __forceinline__ void ring_reducescatter_wide(RingCtx& r, const Fn& fn, const RingWork& w, int c) {
  using T = typename Fn::EltType;
  using CFn = FnSum<T>;
  constexpr int CU = ring_wide_copy_unroll<T>();
  const CFn cfn;
  const int n = w.nRanks;
  const int64_t count = (int64_t)w.count;
  int64_t gridOff, chCount, chunkCount;
  if (!cbd_part(w, c, &gridOff, &chCount, &chunkCount)) return;
  const T* in = (const T*)w.sendbuff;
  T* out = (T*)w.recvbuff;
  const VCCL_LDS int* ringRanks = r.ringRanks;
  auto mis = [&](int k) { return (int)(((int64_t)k * count * (int64_t)sizeof(T)) & 15); };
  const int64_t sub = wide_sub_chunk<T>(chunkCount, n);
  // a block's fold order is its owner's alone, whatever the chunk: the passes are simply chunks of `sub` elements
  for (int64_t eo = 0; eo < chCount; eo += sub) {
    const int64_t nelem = chCount - eo < sub ? chCount - eo : sub;
    const int64_t dataOff = gridOff + eo;
    int rankDest = ringRanks[n - 1];
    ring_step<CFn, false, true, true, false, CU>(r, cfn, in + dataOff + rankDest * count, nullptr, nelem, false, 0,
                                                 mis(rankDest));
    for (int j = 2; j < n; ++j) {
      rankDest = ringRanks[n - j];
      if (j == 2)
        ring_step_wide<Fn, kWireRaw, kWideToF32Slot, U>(r, fn, in + dataOff + rankDest * count, nullptr, nelem,
                                                        mis(rankDest), 0);
      else
        ring_step_wide<Fn, kWireF32, kWideToF32Slot, U>(r, fn, in + dataOff + rankDest * count, nullptr, nelem);
    }
    rankDest = ringRanks[0];
    if (n == 2)
      ring_step_wide<Fn, kWireRaw, kWideToUser, U>(r, fn, in + dataOff + rankDest * count, out + dataOff, nelem,
                                                   mis(rankDest), 0);
    else
      ring_step_wide<Fn, kWireF32, kWideToUser, U>(r, fn, in + dataOff + rankDest * count, out + dataOff, nelem);
  }
}

}  // namespace vccl
