// Stream ordering of one comm's launches (order.cc): every launch site opens an OrderScope on the stream it
// launches on, takes its launches' stop event from it and ends it — alone or with other streams joined around it.
#pragma once
#include <vector>

#include "core.h"

#pragma GCC visibility push(hidden)  // internal, as plan.h
namespace vccl {

struct CaptureState {
  bool active;
  unsigned long long id;
};
ncclResult_t capture_state(hipStream_t s, CaptureState* cs);
// `stop` recorded on s behind work that could not bind it to a kernel (launch.cc launch_path's bias tail).
ncclResult_t record_stop(hipEvent_t stop, hipStream_t s);

// One ordered sequence of launches of `comm` on s0.  begin: s0 waits for the comm's last launch (of this capture,
// when s0 captures) and for the work queued on every joined stream.  stop: the event each launch binds to its
// kernel's completion (nullptr: none — a capture, VCCL_LAUNCH_EVENT=0); ran: the launch's result, passed through.
// end: on success the ordering event marks s0; after a failure an earlier launch that bound it still carries it
// (ADVICE r4); then the joined streams wait for it.
class OrderScope {
 public:
  OrderScope(ncclComm* comm, hipStream_t s0) : comm_(comm), s0_(s0) {}
  void join(hipStream_t s);  // no-op for s0 and for a stream already joined
  ncclResult_t begin();
  const CaptureState& capture() const { return cs_; }
  hipEvent_t stop() const;
  ncclResult_t ran(ncclResult_t r) { return bound_ |= r == ncclSuccess && stop() != nullptr, r; }
  ncclResult_t end(ncclResult_t r);

 private:
  ncclComm* comm_;
  hipStream_t s0_;
  std::vector<hipStream_t> others_;
  CaptureState cs_{false, 0};
  bool bound_ = false;  // a launch of this sequence carries the ordering event
};

}  // namespace vccl
#pragma GCC visibility pop
