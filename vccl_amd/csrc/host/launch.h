// What launch.cc offers the API file (enqueue.cc) and the extension exports
// (ext.cc): a checked call as a Task, its launch alone or as part of a group,
// and the path queries.
#pragma once
#include <vector>

#include "core.h"
#include "plan.h"

#pragma GCC visibility push(hidden)  // internal, as plan.h
namespace vccl {

// Task::coll of a point-to-point call (beside plan.h's Coll values).
enum { kTaskSend = 5, kTaskRecv = 6 };
inline bool is_p2p(int coll) { return coll == kTaskSend || coll == kTaskRecv; }
// ... and of an ncclAllToAll(v) on a comm whose one-hop LL or direct all-to-all
// is on (llA2aMaxBytes > 0 || directA2aMaxBytes > 0) or whose zero-copy
// all-to-all is (regA2aMaxBytes > 0, which pre-empts the other two for the
// calls plan.h reg_a2a_eligible names): one task; launch_group
// gives its pairs within the limits to one LL launch and one direct launch
// (plan.h a2a_plan) and turns the rest into sends and recvs of the
// group's p2p launch.  With both paths off the API expands the call into sends
// and recvs itself, as it always did.
enum { kTaskA2a = 7 };
struct A2aArgs {  // bytes; per peer (nRanks <= kOrderMaxRanks whenever the path is on)
  int64_t sendBytes[kOrderMaxRanks], recvBytes[kOrderMaxRanks];
  int64_t sendOff[kOrderMaxRanks], recvOff[kOrderMaxRanks];
  bool uniform;
};

struct Task {
  int coll;
  const void* sendbuff;
  void* recvbuff;
  size_t count;
  ncclDataType_t datatype;
  int devOp;
  uint64_t arg;
  const void* argPtr;  // ncclScalarDevice PreMulSum scalar
  int root;            // broadcast / reduce; send / recv: the peer
  ncclComm* comm;
  hipStream_t stream;
  // Set by the group planner (launch_planned): this call's partition inside
  // its group's VCCL plan, under the protocol of the path its aggregate took;
  // otherwise the call is planned alone (cbd_schedule).
  bool planned;
  CbdPlan plan;
  // kTaskA2a: the call's rows, owned by the API layer until launch_group returns
  const A2aArgs* a2a;
  // The collectives of this call's comm in its group (launch_group_colls); 0
  // outside a group.  More than one: not eligible for the zero-copy path.
  int groupColls;
  // A send / recv expanded from an all-to-all that launched the zero-copy
  // kernel (launch_comm_p2p): 1 .. kRegA2aMaxCalls, the skip word its FIFO items
  // are predicated on (device/p2p_types.hpp P2pWork::skip); 0: never dropped.
  int skip;
};

// The one place that reads a comm into the planner's thresholds.
AlgoPolicy policy_of(const ncclComm* c);
// The kernel element type of a call (K_U8 for the byte copies), -1: no kernel.
int kernel_type_of_call(int coll, int devOp, ncclDataType_t datatype);
// One call outside a group.
ncclResult_t launch_task(const Task& t);
// A group's calls, at the outermost ncclGroupEnd: per comm its collectives,
// then each of its all-to-all tasks' LL launch and direct launch, then its
// sends and recvs with the all-to-alls' residual pairs (launch_p2p).
ncclResult_t launch_group(std::vector<Task>& tasks);
// Why `comm` cannot send or receive (WARN + ncclInvalidUsage), else ncclSuccess.
ncclResult_t p2p_usable(const ncclComm* comm, const char* api);

}  // namespace vccl
#pragma GCC visibility pop
