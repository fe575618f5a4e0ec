// The point-to-point kernel (p2p.hpp): byte copies only, so one object
// serves every datatype (the host scales counts by the type size).
#include <hip/hip_runtime.h>

#include "p2p.hpp"
#include "p2p_launch.hpp"
#include "ring_launch.hpp"

namespace vccl {

__global__ __launch_bounds__(kP2pThreads) void k_p2p(P2pBatch b) { p2p_run<kRingUnroll>(b); }

hipError_t p2p_launch(const P2pBatch& b, int grid, hipStream_t stream, hipEvent_t stop) {
  if (grid < 1 || b.nWorks < 1 || b.nWorks > kP2pMaxWorks) return hipErrorInvalidValue;
  return launch_k(k_p2p, dim3(grid), dim3(kP2pThreads), stream, stop, b);
}

}  // namespace vccl
