// Host-side declaration of the point-to-point launcher (p2p_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "p2p_types.hpp"

namespace vccl {

// One launch of `grid` workgroups (b.nSendWgs senders, then the receivers) of
// kP2pThreads threads on `stream`; `stop` as for every launcher
// (ring_launch.hpp): an event bound to the kernel's completion, or nullptr.
hipError_t p2p_launch(const P2pBatch& b, int grid, hipStream_t stream, hipEvent_t stop);

}  // namespace vccl
