// MXFP8 kernels for ONE kernel element type (VCCL_KT: K_F16, K_BF16 or K_F32;
// DESIGN.md §4.19): the codec on its own (mxfp8.hpp: vcclMxfp8Pack /
// vcclMxfp8Unpack) and, for the two 16-bit types, the two-shot direct
// all-reduce in the format (direct_mx.hpp).  Objects of their own: every other
// kernel is compiled as it always was.
#include <hip/hip_runtime.h>

#include "dispatch.hpp"
#include "launch.hpp"
#include "ring_launch.hpp"
#if VCCL_KT == 4
#include "mxfp8.hpp"
#else
#include "direct_mx.hpp"
#endif

#ifndef VCCL_KT
#error "compile with -DVCCL_KT=<3 f16 | 4 f32 | 6 bf16>"
#endif

namespace vccl {

constexpr int kMxCodecThreads = 256;

template <typename T>
__global__ __launch_bounds__(kMxCodecThreads) void k_mxfp8_pack(const char* src, char* wire, int64_t count) {
  mxfp8_pack<T>(src, wire, count);
}
template <typename T>
__global__ __launch_bounds__(kMxCodecThreads) void k_mxfp8_unpack(const char* wire, char* dst, int64_t count) {
  mxfp8_unpack<T>(wire, dst, count);
}

template <>
hipError_t mxfp8_codec_launch<VCCL_KT>(bool pack, const void* src, void* dst, int64_t count, hipStream_t stream) {
  using T = typename KTypeOf<VCCL_KT>::T;
  const int64_t nTiles = (count + kMxTileElts - 1) / kMxTileElts, perBlock = kMxCodecThreads / 64;
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((nTiles + perBlock - 1) / perBlock, kRcMaxGrid)));
  const dim3 block(kMxCodecThreads);
  if (pack) hipLaunchKernelGGL(k_mxfp8_pack<T>, grid, block, 0, stream, (const char*)src, (char*)dst, count);
  else hipLaunchKernelGGL(k_mxfp8_unpack<T>, grid, block, 0, stream, (const char*)src, (char*)dst, count);
  return hipGetLastError();
}

#if VCCL_KT != 4
template <typename T>
__global__ __launch_bounds__(kDirectThreads) void k_direct_allreduce_mx(DirectBatch b) {
  direct_batch_mx<T>(b);
}
template <>
hipError_t direct_launch_mx<VCCL_KT>(const DirectBatch& b, hipStream_t stream, hipEvent_t stop) {
  using T = typename KTypeOf<VCCL_KT>::T;
  return launch_k(k_direct_allreduce_mx<T>, dim3(b.w.nBlocks), dim3(kDirectThreads), stream, stop, b);
}

// the one-hop reduce-scatter and all-gather in the format
template <typename T>
__global__ __launch_bounds__(kDirectThreads) void k_direct_reducescatter_mx(DirectBatch b) {
  direct_batch_mx_rsag<T, false>(b);
}
template <typename T>
__global__ __launch_bounds__(kDirectThreads) void k_direct_allgather_mx(DirectBatch b) {
  direct_batch_mx_rsag<T, true>(b);
}
template <>
hipError_t direct_launch_mx_rs<VCCL_KT>(const DirectBatch& b, hipStream_t stream, hipEvent_t stop) {
  using T = typename KTypeOf<VCCL_KT>::T;
  return launch_k(k_direct_reducescatter_mx<T>, dim3(b.w.nBlocks), dim3(kDirectThreads), stream, stop, b);
}
template <>
hipError_t direct_launch_mx_ag<VCCL_KT>(const DirectBatch& b, hipStream_t stream, hipEvent_t stop) {
  using T = typename KTypeOf<VCCL_KT>::T;
  return launch_k(k_direct_allgather_mx<T>, dim3(b.w.nBlocks), dim3(kDirectThreads), stream, stop, b);
}
#endif

}  // namespace vccl
