// Stream ordering of one comm's launches: the ordering event, its capture
// pool, and the scope every launch site goes through (order.h).
#include "order.h"

#include <algorithm>

namespace vccl {

// Order launches of one comm across different user streams (the reference serialises through its internal strong
// stream, enqueue.cc:1445-1548). The null stream (0) is a valid user stream, so "no launch yet" is a flag of its own,
// not a null lastStream.
//
// Graph capture (the reference's strong streams track capture the same way, misc/strongstream.cc): launches on a
// capturing stream are ordered only against earlier launches of the SAME capture, through an event recorded inside it
// (a fork/join inside the graph); they neither wait on the eager lastLaunch event (recorded outside the capture) nor
// overwrite it, so eager work before and after the capture keeps its own ordering.
ncclResult_t capture_state(hipStream_t s, CaptureState* cs) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  HIPCHECK(hipStreamGetCaptureInfo(s, &st, &id));
  cs->active = st == hipStreamCaptureStatusActive;
  cs->id = id;
  return ncclSuccess;
}
// The ordering state of capture `id`: comm->caps is a pool of kMaxCaptures entries created at init (no HIP object is
// created during a capture); a new id takes the least recently used entry whose capture has ended.  When every entry
// still belongs to a live capture, the call fails (ncclInvalidUsage) rather than silently dropping a live capture's
// ordering. A capture is live while its last stream still captures under its id; a stream destroyed since
// reads as ended (HIP validates the handle and fails the query — tests/mp_graph_worker.py
// captures_on_destroyed_streams).
static bool capture_live(const ncclComm::CapOrder& c) {
  if (!c.used || !c.has) return false;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(c.last, &st, &id) != hipSuccess) return false;
  return st == hipStreamCaptureStatusActive && id == c.id;
}
static ncclResult_t capture_entry(ncclComm* comm, unsigned long long id, bool create, ncclComm::CapOrder** out) {
  *out = nullptr;
  auto& caps = comm->caps;
  for (size_t i = 0; i < caps.size(); i++) {
    if (caps[i].used && caps[i].id == id) {
      std::rotate(caps.begin(), caps.begin() + i, caps.begin() + i + 1);  // to the front
      *out = &caps[0];
      return ncclSuccess;
    }
  }
  if (!create || caps.empty()) return ncclSuccess;
  for (size_t i = caps.size(); i-- > 0;) {  // least recently used first
    if (capture_live(caps[i])) continue;
    std::rotate(caps.begin(), caps.begin() + i, caps.begin() + i + 1);
    caps[0].id = id;
    caps[0].used = true;
    caps[0].last = nullptr;
    caps[0].has = false;
    *out = &caps[0];
    return ncclSuccess;
  }
  VWARN("more than %d stream captures are active on this communicator at once", (int)caps.size());
  return ncclInvalidUsage;
}
// One capture query per call: stream_order fills `cs`, stream_mark and stream_last_event reuse it (the capture state
// of s cannot change between them — the caller holds the thread).
static ncclResult_t stream_order(ncclComm* comm, hipStream_t s, CaptureState* cs) {
  NCCLCHECK(capture_state(s, cs));
  if (cs->active) {
    ncclComm::CapOrder* c;
    NCCLCHECK(capture_entry(comm, cs->id, true, &c));  // reserved before the launch
    if (c && c->has && c->last != s) HIPCHECK(hipStreamWaitEvent(s, c->ev, 0));
    return ncclSuccess;
  }
  if (comm->hasLastLaunch && comm->lastStream != s)
    HIPCHECK(hipStreamWaitEvent(s, comm->lastLaunch, 0));
  return ncclSuccess;
}
// The event the launches of an eager call bind to their kernel's completion (hipExtLaunchKernel stopEvent): the
// comm's ordering event, recorded by the kernel's own completion signal instead of a separate marker packet — a
// marker costs ~5 us of GPU time per call on MI355X (profiles/r04q: LL 8 B 10.1 -> 5.7 us per call back to back, 1
// MiB ring 17.5 -> 12.7). VCCL_LAUNCH_EVENT=0: record markers.  Captures keep markers (graph edges).
static hipEvent_t stop_event(ncclComm* comm, const CaptureState& cs) {
  static const bool bind = param_int("LAUNCH_EVENT", 1) != 0;
  return bind && !cs.active ? comm->lastLaunch : nullptr;
}
static ncclResult_t stream_mark(ncclComm* comm, hipStream_t s, const CaptureState& cs) {
  if (cs.active) {
    ncclComm::CapOrder* c;
    NCCLCHECK(capture_entry(comm, cs.id, true, &c));
    if (!c) return ncclInternalError;
    HIPCHECK(hipEventRecord(c->ev, s));
    c->last = s;
    c->has = true;
    return ncclSuccess;
  }
  // VCCL_DEBUG_NO_MARK=1: no marker packet (measurement only: correct for a comm driven from ONE stream, where stream
  // order suffices).  The launch is still tracked: through the stop event when the kernel bound it, else
  // by its stream, so destroy / finalize / abort still wait for it.
  static const bool noMark = param_int("DEBUG_NO_MARK", 0) != 0;
  const bool bound = stop_event(comm, cs) != nullptr;
  if (!noMark && !bound) HIPCHECK(hipEventRecord(comm->lastLaunch, s));  // else bound to the kernel
  comm->lastUnmarked = noMark && !bound;
  comm->lastStream = s;
  comm->hasLastLaunch = true;
  return ncclSuccess;
}
// The event stream_mark just recorded on s (for joining other streams).
static hipEvent_t stream_last_event(ncclComm* comm, const CaptureState& cs) {
  return cs.active ? comm->caps[0].ev : comm->lastLaunch;
}

ncclResult_t record_stop(hipEvent_t stop, hipStream_t s) {
  if (stop) HIPCHECK(hipEventRecord(stop, s));
  return ncclSuccess;
}

void OrderScope::join(hipStream_t s) {
  if (s != s0_ && std::find(others_.begin(), others_.end(), s) == others_.end()) others_.push_back(s);
}
ncclResult_t OrderScope::begin() {
  NCCLCHECK(stream_order(comm_, s0_, &cs_));
  for (hipStream_t s : others_) {
    HIPCHECK(hipEventRecord(comm_->joinEvent, s));
    HIPCHECK(hipStreamWaitEvent(s0_, comm_->joinEvent, 0));
  }
  return ncclSuccess;
}
hipEvent_t OrderScope::stop() const { return stop_event(comm_, cs_); }
ncclResult_t OrderScope::end(ncclResult_t r) {
  if (r == ncclSuccess) {
    r = stream_mark(comm_, s0_, cs_);
  } else if (bound_) {
    // an earlier launch already bound the ordering event to its kernel on s0, so the next call from
    // another stream must still wait on it even though a later launch of this sequence failed
    comm_->lastStream = s0_;
    comm_->hasLastLaunch = true;
    comm_->lastUnmarked = false;
  }
  if (r != ncclSuccess || others_.empty()) return r;
  const hipEvent_t done = stream_last_event(comm_, cs_);
  for (hipStream_t s : others_) HIPCHECK(hipStreamWaitEvent(s, done, 0));
  return ncclSuccess;
}

}  // namespace vccl
