// Host-side declarations for the ring kernels (one specialisation per kernel
// element type, compiled in parallel).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "coll_types.hpp"
#include "dispatch.hpp"
#include "ring_types.hpp"

namespace vccl {

enum : int { kCollAllReduce = 0, kCollReduceScatter = 1, kCollAllGather = 2, kCollBroadcast = 3, kCollReduce = 4 };
// 16-byte packs per thread per operand in flight in a ring step: 4 (2 for
// the fp8 types, whose per-element prod / min / max / PreMulSum kernels
// spill at 4).  Twice round 1's 2 keeps twice the write-through stores in
// flight per channel: the 2-rank rehearsal's all-gather 1 GiB 2614 ->
// 1714 us, all-reduce -2 %, reduce-scatter -1 % (profiles/r02w).
#ifndef VCCL_RING_UNROLL
#define VCCL_RING_UNROLL 4
#endif
constexpr int kRingUnroll = VCCL_RING_UNROLL;
constexpr int kRingMaxThreads = 512;  // k_ring launch bound (ring_kernels.hip)

// Every launcher takes `stop`: an event the kernel's own completion signal
// records (hipExtLaunchKernel's stopEvent) — the comm's ordering event,
// recorded without a separate marker packet; nullptr = none.
//
// w.w.nChannels workgroups (the largest part's channelHi + 1); the SIMPLE
// ring, or the same schedules over LL128 FIFOs (separate objects).
template <int K>
hipError_t ring_launch(int coll, int devOp, const RingBatch& w, int nthreads, hipStream_t stream,
                       hipEvent_t stop);
template <int K>
hipError_t ring_launch_ll128(int coll, int devOp, const RingBatch& w, int nthreads, hipStream_t stream,
                             hipEvent_t stop);
// The SIMPLE ring with the per-wave slot hand-off (ring.hpp prim_ws): only
// the bandwidth-regime kernels — sum over f32 / f16 / bf16 (all-reduce,
// reduce-scatter, reduce) and the byte-copy all-gather / broadcast — see
// ring_wave_kernel(); every other call takes ring_launch.
template <int K>
hipError_t ring_launch_wave(int coll, int devOp, const RingBatch& w, int nthreads, hipStream_t stream,
                            hipEvent_t stop);
enum : int { kRingVariantSimple = 0, kRingVariantLL128 = 1, kRingVariantWave = 2 };
template <int K>
inline hipError_t ring_launch_any(int variant, int coll, int devOp, const RingBatch& w, int nthreads,
                                  hipStream_t stream, hipEvent_t stop) {
  if (variant == kRingVariantLL128) return ring_launch_ll128<K>(coll, devOp, w, nthreads, stream, stop);
  if constexpr (K == K_U8 || K == K_F32 || K == K_F16 || K == K_BF16)
    if (variant == kRingVariantWave) return ring_launch_wave<K>(coll, devOp, w, nthreads, stream, stop);
  return ring_launch<K>(coll, devOp, w, nthreads, stream, stop);
}

// One-hop LL collectives (ll.hpp): 256-thread workgroups, `grid` of them.
// All-gather and broadcast only in the K_U8 unit (byte copies).
template <int K>
hipError_t ll_launch(int coll, int devOp, const LLWork& w, int grid, hipStream_t stream, hipEvent_t stop);

// One-hop LL all-to-all(v) (ll.hpp ll_alltoall): a byte copy, built once in
// the K_U8 unit; 256-thread workgroups, `grid` of them.
hipError_t ll_a2a_launch(const LLA2aWork& w, int grid, hipStream_t stream, hipEvent_t stop);

// Direct collectives over the full mesh (direct.hpp): two-shot all-reduce,
// one-hop reduce-scatter / all-gather, 1 .. kDirectMaxWorks calls per launch;
// b.w.nBlocks workgroups (the largest part's) of kDirectThreads threads.
// All-gather only in the K_U8 unit.
template <int K>
hipError_t direct_launch(int coll, int devOp, const DirectBatch& b, hipStream_t stream, hipEvent_t stop);

// Zero-copy direct all-reduce / reduce-scatter / all-gather over registered
// buffers, with the staged kernel of the same collective as its in-kernel
// fallback (direct_reg.hpp): one call per launch, rw.w.nBlocks workgroups.
// Built apart from the direct kernels, the all-reduce in an object of its own
// (direct_reg_kernels.hip, VCCL_REG_PART 0 / 1): each kernel carries its
// staged fallback, and the fp8 units are the build's longest compiles.
template <int K>
hipError_t direct_reg_launch_ar(int devOp, const DirectRegWork& rw, hipStream_t stream, hipEvent_t stop);
template <int K>
hipError_t direct_reg_launch_rsag(int coll, int devOp, const DirectRegWork& rw, hipStream_t stream, hipEvent_t stop);
template <int K>
inline hipError_t direct_reg_launch(int coll, int devOp, const DirectRegWork& rw, hipStream_t stream,
                                    hipEvent_t stop) {
  return coll == kCollAllReduce ? direct_reg_launch_ar<K>(devOp, rw, stream, stop)
                                : direct_reg_launch_rsag<K>(coll, devOp, rw, stream, stop);
}

// Zero-copy broadcast / reduce over registered buffers (direct_reg.hpp
// reg_broadcast_zc / reg_reduce_zc), the staged rooted part of direct.hpp as the
// in-kernel fallback: one call per launch, rw.w.nBlocks workgroups.  A third
// object per kernel type (direct_reg_kernels.hip, VCCL_REG_PART 2); the
// byte-copy broadcast only in the K_U8 unit.
template <int K>
hipError_t direct_reg_launch_rooted(int coll, int devOp, const DirectRegWork& rw, hipStream_t stream,
                                    hipEvent_t stop);

// Zero-copy all-to-all(v) over registered send buffers (direct_reg.hpp
// direct_reg_alltoall): a byte copy, built once in the K_U8 unit of
// direct_reg_kernels.hip (part 1); w.nBlocks workgroups of kDirectThreads threads.
hipError_t direct_reg_a2a_launch(const DirectRegA2aWork& w, hipStream_t stream, hipEvent_t stop);

// One-hop direct all-to-all(v) (direct.hpp direct_alltoall): a byte copy,
// built once in the K_U8 unit; w.nBlocks workgroups of kDirectThreads threads.
hipError_t direct_a2a_launch(const DirectA2aWork& w, hipStream_t stream, hipEvent_t stop);

// hipLaunchKernelGGL, or with `stop` bound to the kernel's completion.
template <class F, class... A>
inline hipError_t launch_k(F kernel, dim3 grid, dim3 block, hipStream_t stream, hipEvent_t stop, A... args) {
  if (stop) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, nullptr, stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
  return hipGetLastError();
}

}  // namespace vccl
