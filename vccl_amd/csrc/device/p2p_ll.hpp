// The LL step of the point-to-point kernel for gfx950: a small ncclSend /
// ncclRecv (and a small residual pair of an all-to-all) on the pair's LL FIFO
// (p2p_types.hpp P2pLLConn) instead of the SIMPLE slot hand-off of p2p.hpp.
//
// The reference runs messages up to NCCL_P2P_LL_THRESHOLD over prims_ll.h
// (sendrecv.h, enqueue.cc:771-831): the flag travels inside the 16-byte line,
// so a step costs ONE cross-device trip — the sender's stores — where the
// SIMPLE step costs two dependent ones (data, drain, barrier, tail; then the
// receiver's loads).  Here:
//
//   send step   thread 0 waits for credit (head >= step + 1 - kSteps: the slot's
//               previous tenant has been read), a barrier, then thread t loads
//               8 user bytes for each of lines t, t + nthreads, ... (ll_load8
//               absorbs a misaligned source and the message's tail) and issues
//               one sc0 sc1 16-byte store per line into the peer's slot, flag
//               (uint32_t)(step + 1) in both halves.  All of a thread's lines
//               are issued back to back; nothing waits: no drain, no tail, no
//               barrier after the stores.
//   recv step   thread t polls the same lines of its own slot, up to
//               kP2pLLBatch line loads in flight before the first flag check;
//               only a line that has not arrived is polled again (ll.hpp
//               ll_read_line: abort word, error word, spin timeout).  Data goes
//               to the user destination with ll_store8.  Then a barrier and
//               one relaxed system-scope store head = step + 1: the slot has
//               been READ, which is all the credit asserts, so no drain.
//
// The credit is what lets this path exist outside a collective: the epoch-
// parity buffers of ll.hpp are reused by whoever calls next and need every
// launch to be an arrival barrier; a slot here is reused only by the same
// sender, and only after the receiver's head says it was read.
//
// Flag wrap (the reference's cleanup rule, prims_ll.h:81-87, device.h:70-79):
// a line a short message leaves untouched keeps an old flag, which a step
// 2^32 later would take for its own.  On the eight steps with
// (step & 0x7ffffff8) == 0x7ffffff8 — every slot once, just before bit 31 and
// bit 32 of the counter turn — the sender also writes every remaining line of
// the slot with zero data and the step's flag, so no line older than half the
// flag space survives, and the all-zero flag of step 2^32 - 1 never meets a
// never-written line.  Such a step drains its stores before it ends, and the
// next step on the connection begins with a barrier behind its credit wait: a
// fill is complete in memory before any later store to the same line (eight
// steps on, by the same thread — lines map to threads by l mod nthreads in
// both) is issued, so it cannot overtake it.
#pragma once
#include "ll.hpp"
#include "p2p_types.hpp"
#include "ring.hpp"

namespace vccl {

constexpr int kP2pLLBatch = 4;  // line loads in flight per thread before the first flag check

__device__ __forceinline__ bool p2p_ll_cleanup_step(uint64_t step) {
  return ((uint32_t)step & 0x7ffffff8u) == 0x7ffffff8u;
}

// One message of `bytes` (> 0) bytes from `src` in ceil(bytes / stepData)
// steps.  Returns the connection's send step after it; on an abort (r.aborted())
// the step the failed wait belonged to, as the SIMPLE path leaves it.
__device__ __forceinline__ uint64_t p2p_ll_send(RingCtx& r, const P2pLLConn& c, uint64_t step, const char* src,
                                                int64_t bytes, int stepLines) {
  const int64_t stepData = (int64_t)stepLines * 8;
  const uint64_t* head = uniform_ptr(c.sendHead);
  char* const fifo = c.sendFifo;
  for (int64_t o = 0; o < bytes; o += stepData, step++) {
    const int64_t len = bytes - o < stepData ? bytes - o : stepData;
    if (r.tid == 0 && !r.aborted()) {
      if (step + 1 > (uint64_t)kSteps && !r.spin_ge(head, step + 1 - kSteps)) r.set_aborted();
      if (r.useFences) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        drain_vmem();
      }
    }
    __syncthreads();
    if (r.aborted()) return step;
    const int nData = (int)((len + 7) / 8);
    const bool cleanup = p2p_ll_cleanup_step(step);
    const int nLines = cleanup ? stepLines : nData;
    const uint32_t flag = (uint32_t)(step + 1);
    char* const slot = fifo + (int64_t)(step % kSteps) * stepLines * 16;
    for (int l = r.tid; l < nLines; l += r.nthreads) {
      const uint64_t v = l < nData ? ll_load8(src + o, l, len) : 0;
      u32x4 line;
      line.x = (uint32_t)v;
      line.y = flag;
      line.z = (uint32_t)(v >> 32);
      line.w = flag;
      const SysAddr d = sys_addr(slot + (int64_t)l * 16);
      __builtin_amdgcn_raw_buffer_store_b128(line, d.r, d.voff, 0, kSysAux);
    }
    if (cleanup || r.useFences) {
      if (r.useFences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      drain_vmem();  // a fill is in memory before this thread's next store to the line (header)
    }
  }
  return step;
}

// The matching receive into `dst`.
__device__ __forceinline__ uint64_t p2p_ll_recv(RingCtx& r, const P2pLLConn& c, uint64_t step, char* dst,
                                                int64_t bytes, int stepLines) {
  const int64_t stepData = (int64_t)stepLines * 8;
  const char* const fifo = c.recvFifo;
  uint64_t* const head = c.peerHead;
  for (int64_t o = 0; o < bytes; o += stepData, step++) {
    const int64_t len = bytes - o < stepData ? bytes - o : stepData;
    const int nData = (int)((len + 7) / 8);
    const uint32_t flag = (uint32_t)(step + 1);
    const char* const slot = fifo + (int64_t)(step % kSteps) * stepLines * 16;
    bool ok = !r.aborted();
    for (int l0 = r.tid; l0 < nData && ok; l0 += kP2pLLBatch * r.nthreads) {
      u32x4 v[kP2pLLBatch];
#pragma unroll
      for (int k = 0; k < kP2pLLBatch; k++) {
        const int l = l0 + k * r.nthreads;
        if (l < nData) {
          const SysAddr a = sys_addr(slot + (int64_t)l * 16);
          v[k] = __builtin_amdgcn_raw_buffer_load_b128(a.r, a.voff, 0, kSysAux);
        }
      }
#pragma unroll
      for (int k = 0; k < kP2pLLBatch; k++) {
        const int l = l0 + k * r.nthreads;
        if (l >= nData) break;
        uint64_t x;
        if (v[k].y == flag && v[k].w == flag) {
          x = (uint64_t)v[k].x | ((uint64_t)v[k].z << 32);
        } else {
          ok = ll_read_line(slot + (int64_t)l * 16, flag, r.comm, &x);
          if (!ok) break;
        }
        if (r.useFences) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        ll_store8(dst + o, l, len, x);
      }
    }
    if (!ok) r.set_aborted();
    __syncthreads();
    if (r.aborted()) return step;
    if (r.tid == 0) {
      if (r.useFences) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        drain_vmem();
      }
      st_sys(head, step + 1);
    }
  }
  return step;
}

}  // namespace vccl
