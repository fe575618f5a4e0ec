// Zero-copy direct kernels over registered buffers (direct_reg.hpp) for ONE
// kernel element type (VCCL_KT) and ONE part (VCCL_REG_PART: 0 the all-reduce,
// 1 the reduce-scatter and, in the K_U8 unit, the byte-copy all-gather and the
// zero-copy all-to-all(v), which has no staged part: its fallback is the FIFOs;
// 2 the reduce and, in the K_U8 unit, the byte-copy broadcast) —
// separate objects, built in parallel with the collective kernels of
// ring_kernels.hip.  One call per launch; the staged part of the same
// collective is the fallback the negotiation may pick.
#include <hip/hip_runtime.h>

#include "direct_reg.hpp"
#include "dispatch.hpp"
#include "ring_launch.hpp"

#ifndef VCCL_KT
#error "compile with -DVCCL_KT=<kernel element type>"
#endif
#ifndef VCCL_REG_PART
#error "compile with -DVCCL_REG_PART=<0 all-reduce | 1 reduce-scatter / all-gather | 2 broadcast / reduce>"
#endif

namespace vccl {

#if VCCL_REG_PART == 0
template <class Fn>
__global__ __launch_bounds__(kDirectThreads) void k_direct_reg_allreduce(DirectRegWork rw) {
  direct_reg_run(
      rw, [](const DirectRegWork& r, const RegResolved& rs, uint32_t e, int* f) { reg_allreduce_zc<Fn>(r, rs, e, f); },
      [](const DirectWork& w, uint32_t& e, int& f) { direct_allreduce_part<Fn>(w, e, f); });
}

template <>
hipError_t direct_reg_launch_ar<VCCL_KT>(int devOp, const DirectRegWork& rw, hipStream_t stream, hipEvent_t stop) {
  using T = typename KTypeOf<VCCL_KT>::T;
  const dim3 grid(rw.w.nBlocks), block(kDirectThreads);
  hipError_t err = hipErrorInvalidValue;
  dispatch_op<T>(devOp, [&]<class Fn>() {
    if constexpr (!std::is_same<Fn, FnCopy<T>>::value)
      err = launch_k(k_direct_reg_allreduce<Fn>, grid, block, stream, stop, rw);
  });
  return err;
}

#elif VCCL_REG_PART == 2
template <class Fn>
__global__ __launch_bounds__(kDirectThreads) void k_direct_reg_reduce(DirectRegWork rw) {
  direct_reg_run(
      rw, [](const DirectRegWork& r, const RegResolved& rs, uint32_t& e, int* f) { reg_reduce_zc<Fn>(r, rs, e, f); },
      [](const DirectWork& w, uint32_t& e, int& f) { direct_reduce_part<Fn>(w, e, f); });
}
template <int K>  // the K_U8 unit only
__global__ __launch_bounds__(kDirectThreads) void k_direct_reg_broadcast(DirectRegWork rw) {
  direct_reg_run(
      rw, [](const DirectRegWork& r, const RegResolved& rs, uint32_t e, int* f) { reg_broadcast_zc(r, rs, e, f); },
      [](const DirectWork& w, uint32_t& e, int& f) { direct_broadcast_part(w, e, f); });
}

template <>
hipError_t direct_reg_launch_rooted<VCCL_KT>(int coll, int devOp, const DirectRegWork& rw, hipStream_t stream,
                                             hipEvent_t stop) {
  using T = typename KTypeOf<VCCL_KT>::T;
  const dim3 grid(rw.w.nBlocks), block(kDirectThreads);
  if (coll == kCollBroadcast) {
    if constexpr (VCCL_KT == K_U8) return launch_k(k_direct_reg_broadcast<K_U8>, grid, block, stream, stop, rw);
    return hipErrorInvalidValue;
  }
  hipError_t err = hipErrorInvalidValue;
  if (coll != kCollReduce) return err;
  dispatch_op<T>(devOp, [&]<class Fn>() {
    if constexpr (!std::is_same<Fn, FnCopy<T>>::value)
      err = launch_k(k_direct_reg_reduce<Fn>, grid, block, stream, stop, rw);
  });
  return err;
}

#else
template <class Fn>
__global__ __launch_bounds__(kDirectThreads) void k_direct_reg_reducescatter(DirectRegWork rw) {
  direct_reg_run(
      rw,
      [](const DirectRegWork& r, const RegResolved& rs, uint32_t e, int* f) { reg_reducescatter_zc<Fn>(r, rs, e, f); },
      [](const DirectWork& w, uint32_t& e, int& f) { direct_reducescatter_part<Fn>(w, e, f); });
}
template <int K>  // the K_U8 unit only
__global__ __launch_bounds__(kDirectThreads) void k_direct_reg_allgather(DirectRegWork rw) {
  direct_reg_run(
      rw, [](const DirectRegWork& r, const RegResolved& rs, uint32_t e, int* f) { reg_allgather_zc(r, rs, e, f); },
      [](const DirectWork& w, uint32_t& e, int& f) { direct_allgather_part(w, e, f); });
}

template <>
hipError_t direct_reg_launch_rsag<VCCL_KT>(int coll, int devOp, const DirectRegWork& rw, hipStream_t stream,
                                           hipEvent_t stop) {
  using T = typename KTypeOf<VCCL_KT>::T;
  const dim3 grid(rw.w.nBlocks), block(kDirectThreads);
  if (coll == kCollAllGather) {
    if constexpr (VCCL_KT == K_U8) return launch_k(k_direct_reg_allgather<K_U8>, grid, block, stream, stop, rw);
    return hipErrorInvalidValue;
  }
  hipError_t err = hipErrorInvalidValue;
  if (coll != kCollReduceScatter) return err;
  dispatch_op<T>(devOp, [&]<class Fn>() {
    if constexpr (!std::is_same<Fn, FnCopy<T>>::value)
      err = launch_k(k_direct_reg_reducescatter<Fn>, grid, block, stream, stop, rw);
  });
  return err;
}

#if VCCL_KT == 0  // K_U8: the byte-copy object also holds the zero-copy all-to-all(v)
__global__ __launch_bounds__(kDirectThreads) void k_direct_reg_alltoall(DirectRegA2aWork w) { direct_reg_alltoall(w); }
hipError_t direct_reg_a2a_launch(const DirectRegA2aWork& w, hipStream_t stream, hipEvent_t stop) {
  return launch_k(k_direct_reg_alltoall, dim3(w.nBlocks), dim3(kDirectThreads), stream, stop, w);
}
#endif
#endif

}  // namespace vccl
