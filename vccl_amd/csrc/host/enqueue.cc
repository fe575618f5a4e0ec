// Collective API -> argument check -> op encoding -> task -> launch.
// (The planner lives in plan.cc, the launch path in launch.cc, the vccl*
// exports in ext.cc.)
//
// Keeps the observable semantics of the reference's dispatch surface
// (collectives.cc:77-158 -> ncclEnqueueCheck enqueue.cc:2448-2525 -> ArgsCheck
// misc/argcheck.cc:45-86 -> taskAppend enqueue.cc:2315-2442 with
// hostToDevRedOp :2217-2310), re-implemented for one node.  Group semantics
// (group.cc:92-110, :393-506): calls between ncclGroupStart/End are queued per
// thread and launched at the outermost ncclGroupEnd (launch_group).  ncclSend /
// ncclRecv (collectives.cc:160-186) take the same road as p2p tasks;
// ncclAllToAll(v) is an internal group of them — or, on a comm that opted into
// the one-hop LL or direct all-to-all (VCCL_LL_A2A_THRESHOLD,
// VCCL_DIRECT_A2A_THRESHOLD), one task of its own whose small pairs take one LL
// launch and whose mid-size pairs one direct launch (launch.cc launch_comm_p2p).
// This file holds the nccl* entry points, their pnccl* aliases and the group
// handling; the vccl* extension exports live in ext.cc.
#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>

#include "../../../include/vccl_device.h"
#include "../device/coll_types.hpp"
#include "../device/dispatch.hpp"
#include "launch.h"

namespace vccl {

static thread_local int tl_groupDepth = 0;
static thread_local std::vector<Task> tl_tasks;
static thread_local ncclResult_t tl_groupError = ncclSuccess;

// ncclGroupErrCheck (enqueue.cc:2516): inside a group the first failing call
// is remembered, and the outermost ncclGroupEnd then launches nothing of the
// group and returns that error (group.cc:528, :591).
static ncclResult_t group_result(ncclResult_t r) {
  if (r != ncclSuccess && tl_groupDepth > 0 && tl_groupError == ncclSuccess) tl_groupError = r;
  return r;
}

static ncclResult_t resolve_op(ncclComm* comm, ncclRedOp_t op, ncclDataType_t dt, int* devOp,
                               uint64_t* arg, const void** argPtr) {
  *argPtr = nullptr;
  if ((int)op < (int)ncclNumOps) return host_to_dev_redop(op, dt, comm->nRanks, devOp, arg);
  const int ix = (int)op - (int)ncclNumOps;
  if (ix >= (int)comm->userOps.size() || comm->userOps[ix].freeNext != -1) return ncclInvalidArgument;
  const UserRedOp& u = comm->userOps[ix];
  if (u.datatype != dt) {  // enqueue.cc:2301-2305
    VWARN("Data type supplied to user-created ncclRedOp_t does not match type given to reduction operation");
    return ncclInvalidArgument;
  }
  *devOp = u.devOp;
  *arg = u.argIsPtr ? 0 : u.arg;
  if (u.argIsPtr) *argPtr = (const void*)u.arg;
  return ncclSuccess;
}

// ArgsCheck (misc/argcheck.cc:45-86) minus the root check (no rooted colls).
static ncclResult_t args_check(ncclComm* comm, const char* name, ncclDataType_t dt, ncclRedOp_t op, bool hasOp) {
  if ((int)dt < 0 || (int)dt >= (int)ncclNumTypes) {
    VWARN("%s : invalid type %d", name, (int)dt);
    return ncclInvalidArgument;
  }
  if (hasOp) {
    if ((int)op < 0 || (int)op > (int)ncclMaxRedOp) {
      VWARN("%s : invalid reduction operation %d", name, (int)op);
      return ncclInvalidArgument;
    }
    const int ix = (int)op - (int)ncclNumOps;
    if (ix >= 0 && (ix >= (int)comm->userOps.size() || comm->userOps[ix].freeNext != -1)) {
      VWARN("%s : reduction operation %d unknown to this communicator", name, (int)op);
      return ncclInvalidArgument;
    }
  }
  // fp8 (enqueue.cc:2379-2384 requires sm90 in the reference): native on gfx950
  return ncclSuccess;
}

static ncclResult_t enqueue_check_impl(int coll, const char* name, const void* sendbuff,
                                       void* recvbuff, size_t count, ncclDataType_t dt,
                                       ncclRedOp_t op, ncclComm* comm, hipStream_t stream, int root) {
  NCCLCHECK(comm_check(comm, name));
  if ((coll == kBroadcast || coll == kReduce) && (root < 0 || root >= comm->nRanks)) {  // argcheck.cc:66-69
    VWARN("%s : invalid root %d (root should be in the 0..%d range)", name, root, comm->nRanks);
    return ncclInvalidArgument;
  }
  NCCLCHECK(args_check(comm, name, dt, op, !is_copy_coll(coll)));
  VINFO("%s: opCount %lx sendbuff %p recvbuff %p count %zu datatype %d op %d comm %p [nranks=%d] stream %p",
        name, (unsigned long)comm->opCount, sendbuff, recvbuff, count, (int)dt, (int)op,
        (void*)comm, comm->nRanks, (void*)stream);
  if (count == 0) return ncclSuccess;  // enqueue.cc:2372
  // broadcast: a non-root's sendbuff is never read, reduce: a non-root's
  // recvbuff never written (argcheck.cc:76-81)
  if ((!recvbuff && !(coll == kReduce && comm->rank != root)) ||
      (!sendbuff && !(coll == kBroadcast && comm->rank != root))) {
    VWARN("%s : NULL buffer", name);
    return ncclInvalidArgument;
  }
  Task t{.coll = coll, .sendbuff = sendbuff, .recvbuff = recvbuff, .count = count, .datatype = dt,
         .devOp = OP_COPY, .root = root, .comm = comm, .stream = stream};
  if (!is_copy_coll(coll)) NCCLCHECK(resolve_op(comm, op, dt, &t.devOp, &t.arg, &t.argPtr));
  if (*(volatile int*)comm->errorFlag) {
    const ncclResult_t e = error_word_result(comm);
    comm->asyncError = e;
    return e;
  }
  if (tl_groupDepth > 0) {
    tl_tasks.push_back(t);
    return ncclSuccess;
  }
  return launch_task(t);
}

static ncclResult_t enqueue_check(int coll, const char* name, const void* sendbuff, void* recvbuff,
                                  size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm* comm,
                                  hipStream_t stream, int root = 0) {
  return group_result(enqueue_check_impl(coll, name, sendbuff, recvbuff, count, dt, op, comm, stream, root));
}

}  // namespace vccl

using namespace vccl;

// Out-of-scope calls of the reference API (include/nccl.h):
// exported so a binary linked against libnccl loads, never silently wrong.
static ncclResult_t out_of_scope(const char* name) {
  VWARN("%s is not part of this library's scope", name);
  return ncclInvalidUsage;
}
// ncclSend / ncclRecv / ncclAllToAll(v) without a communicator: the reference
// dereferences it (collectives.cc:165); here WARN + ncclInvalidUsage.
static ncclResult_t p2p_null_comm(const char* name) {
  VWARN("%s : comm argument is NULL", name);
  return ncclInvalidUsage;
}

// What every send or recv needs after its peer and type checks, in this
// order: a buffer, a comm without a recorded error, point-to-point connections.
static ncclResult_t p2p_buffer_check(ncclComm* comm, const char* name, const void* buff, size_t count) {
  if (!buff && count > 0) {
    VWARN("%s : NULL buffer", name);
    return ncclInvalidArgument;
  }
  if (*(volatile int*)comm->errorFlag) {
    const ncclResult_t e = error_word_result(comm);
    comm->asyncError = e;
    return e;
  }
  return p2p_usable(comm, name);
}

// ncclSend / ncclRecv (collectives.cc:160-186 -> ncclEnqueueCheck): checked,
// then queued in the thread's group or launched alone.
static ncclResult_t p2p_check_impl(bool send, const char* name, const void* buff, size_t count, ncclDataType_t dt,
                                   int peer, ncclComm* comm, hipStream_t stream) {
  NCCLCHECK(comm_check(comm, name));
  if (peer < 0 || peer >= comm->nRanks) {  // argcheck.cc:58-61
    VWARN("%s : invalid peer %d (peer should be in the 0..%d range)", name, peer, comm->nRanks);
    return ncclInvalidArgument;
  }
  NCCLCHECK(args_check(comm, name, dt, ncclSum, false));
  NCCLCHECK(p2p_buffer_check(comm, name, buff, count));
  VINFO("%s: opCount %lx buff %p count %zu datatype %d peer %d comm %p [nranks=%d] stream %p", name,
        (unsigned long)comm->opCount, buff, count, (int)dt, peer, (void*)comm, comm->nRanks, (void*)stream);
  Task t{.coll = send ? kTaskSend : kTaskRecv, .sendbuff = send ? buff : nullptr,
         .recvbuff = send ? nullptr : const_cast<void*>(buff), .count = count, .datatype = dt, .devOp = OP_COPY,
         .root = peer, .comm = comm, .stream = stream};
  if (tl_groupDepth > 0) {
    tl_tasks.push_back(t);
    return ncclSuccess;
  }
  std::vector<Task> one{t};
  return launch_group(one);
}
static ncclResult_t p2p_check(bool send, const char* name, const void* buff, size_t count, ncclDataType_t dt,
                              int peer, ncclComm* comm, hipStream_t stream) {
  return group_result(p2p_check_impl(send, name, buff, count, dt, peer, comm, stream));
}

VCCL_EXPORT ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer,
                                  ncclComm_t comm, hipStream_t stream) {
  if (!comm) return p2p_null_comm("ncclSend");
  return p2p_check(true, "Send", sendbuff, count, datatype, peer, comm, stream);
}
VCCL_EXPORT ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                                  hipStream_t stream) {
  if (!comm) return p2p_null_comm("ncclRecv");
  return p2p_check(false, "Recv", recvbuff, count, datatype, peer, comm, stream);
}

// Peer p's element count and offset in an all-to-all's send or recv buffer:
// the v-call's arrays, or (NULL arrays) `count` elements at p * count.
struct A2aRow {
  size_t count, off;
};
static A2aRow a2a_row(const size_t* counts, const size_t* displs, size_t count, int p) {
  return A2aRow{counts ? counts[p] : count, displs ? displs[p] : (size_t)p * count};
}

// The all-to-all of a comm whose one-hop LL or direct all-to-all is on
// (llA2aMaxBytes > 0 || directA2aMaxBytes > 0) or whose zero-copy all-to-all is
// (regA2aMaxBytes > 0): ONE queued task (kTaskA2a) — launch_group splits its
// pairs between the LL launch, the direct launch and the p2p launch, or gives
// an eligible call to the zero-copy launch with the p2p launch as its fallback.  The per-pair checks of the expansion below, in
// its order; the rows live in tl_a2a until the group has launched.
static thread_local std::deque<A2aArgs> tl_a2a;
static ncclResult_t all_to_all_task(const char* name, const void* sendbuff, const size_t* sendcounts,
                                    const size_t* sdispls, void* recvbuff, const size_t* recvcounts,
                                    const size_t* rdispls, size_t count, ncclDataType_t dt, ncclComm* comm,
                                    hipStream_t stream) {
  const size_t esz = (size_t)type_size(dt);
  const int n = comm->nRanks;
  A2aArgs a{};
  a.uniform = sendcounts == nullptr;
  ncclResult_t r = ncclSuccess;
  for (int p = 0; p < n && r == ncclSuccess; p++) {
    const A2aRow s = a2a_row(sendcounts, sdispls, count, p), q = a2a_row(recvcounts, rdispls, count, p);
    a.sendBytes[p] = (int64_t)(s.count * esz), a.sendOff[p] = (int64_t)(s.off * esz);
    a.recvBytes[p] = (int64_t)(q.count * esz), a.recvOff[p] = (int64_t)(q.off * esz);
    r = p2p_buffer_check(comm, name, sendbuff, s.count);
    if (r == ncclSuccess) r = p2p_buffer_check(comm, name, recvbuff, q.count);
  }
  if (r != ncclSuccess) return group_result(r);
  VINFO("%s: opCount %lx sendbuff %p recvbuff %p count %zu datatype %d comm %p [nranks=%d] stream %p", name,
        (unsigned long)comm->opCount, sendbuff, recvbuff, count, (int)dt, (void*)comm, n, (void*)stream);
  Task t{.coll = kTaskA2a, .sendbuff = sendbuff, .recvbuff = recvbuff, .count = count, .datatype = dt,
         .devOp = OP_COPY, .root = 0, .comm = comm, .stream = stream};
  if (tl_groupDepth > 0) {
    tl_a2a.push_back(a);
    t.a2a = &tl_a2a.back();  // a deque: earlier tasks' rows stay where they are
    tl_tasks.push_back(t);
    return ncclSuccess;
  }
  t.a2a = &a;
  std::vector<Task> one{t};
  return launch_group(one);
}

// RCCL's all-to-alls: an internal group of n sends and n recvs (the self block
// a local copy).  counts / displacements in elements; NULL arrays = the
// uniform all-to-all of `count` elements per pair.
static ncclResult_t all_to_all(const char* name, const void* sendbuff, const size_t* sendcounts, const size_t* sdispls,
                               void* recvbuff, const size_t* recvcounts, const size_t* rdispls, size_t count,
                               ncclDataType_t dt, ncclComm* comm, hipStream_t stream) {
  ncclResult_t r = comm_check(comm, name);
  if (r == ncclSuccess) r = args_check(comm, name, dt, ncclSum, false);
  if (r == ncclSuccess && sendbuff == recvbuff) {
    VWARN("%s : in-place operation is not supported (sendbuff == recvbuff)", name);
    r = ncclInvalidArgument;
  }
  if (r != ncclSuccess) return group_result(r);
  const size_t esz = (size_t)type_size(dt);
  const int n = comm->nRanks;
  static_assert(kDirectMaxRanks <= kOrderMaxRanks, "A2aArgs holds kOrderMaxRanks rows");
  // ... or whose zero-copy all-to-all is (regA2aMaxBytes > 0, at most kDirectMaxRanks ranks)
  if ((comm->llA2aMaxBytes > 0 || comm->directA2aMaxBytes > 0 || comm->regA2aMaxBytes > 0) && n <= kOrderMaxRanks)
    return all_to_all_task(name, sendbuff, sendcounts, sdispls, recvbuff, recvcounts, rdispls, count, dt, comm, stream);
  ncclGroupStart();
  for (int p = 0; p < n && r == ncclSuccess; p++) {
    const A2aRow s = a2a_row(sendcounts, sdispls, count, p), q = a2a_row(recvcounts, rdispls, count, p);
    r = p2p_check(true, name, sendbuff ? (const char*)sendbuff + s.off * esz : nullptr, s.count, dt, p, comm, stream);
    if (r == ncclSuccess)
      r = p2p_check(false, name, recvbuff ? (char*)recvbuff + q.off * esz : nullptr, q.count, dt, p, comm, stream);
  }
  const ncclResult_t e = ncclGroupEnd();  // an inner group: launches only when this is the outermost
  if (r == ncclSuccess) comm->a2aFifoPairs += 2 * (size_t)n;  // vcclCommA2aStats: every pair on the FIFOs
  return r != ncclSuccess ? r : e;
}

VCCL_EXPORT ncclResult_t ncclAllToAll(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                      ncclComm_t comm, hipStream_t stream) {
  if (!comm) return p2p_null_comm("ncclAllToAll");
  return all_to_all("AllToAll", sendbuff, nullptr, nullptr, recvbuff, nullptr, nullptr, count, datatype, comm, stream);
}
VCCL_EXPORT ncclResult_t ncclAllToAllv(const void* sendbuff, const size_t sendcounts[], const size_t sdispls[],
                                       void* recvbuff, const size_t recvcounts[], const size_t rdispls[],
                                       ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream) {
  if (!comm) return p2p_null_comm("ncclAllToAllv");
  if (!sendcounts || !sdispls || !recvcounts || !rdispls) {
    VWARN("AllToAllv : NULL count or displacement array");
    return group_result(ncclInvalidArgument);
  }
  return all_to_all("AllToAllv", sendbuff, sendcounts, sdispls, recvbuff, recvcounts, rdispls, 0, datatype, comm,
                    stream);
}

VCCL_EXPORT ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                       ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
  return enqueue_check(kAllReduce, "AllReduce", sendbuff, recvbuff, count, datatype, op, comm, stream);
}
VCCL_EXPORT ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount,
                                           ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                                           hipStream_t stream) {
  return enqueue_check(kReduceScatter, "ReduceScatter", sendbuff, recvbuff, recvcount, datatype, op, comm, stream);
}
VCCL_EXPORT ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount,
                                       ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream) {
  return enqueue_check(kAllGather, "AllGather", sendbuff, recvbuff, sendcount, datatype, ncclSum, comm, stream);
}
// broadcast.h / collectives.cc:125-158: the ring broadcast, count elements of
// datatype from root's sendbuff to every rank's recvbuff (bytes on the wire).
VCCL_EXPORT ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count,
                                       ncclDataType_t datatype, int root, ncclComm_t comm, hipStream_t stream) {
  return enqueue_check(kBroadcast, "Broadcast", sendbuff, recvbuff, count, datatype, ncclSum, comm, stream,
                       root);
}
// reduce.h / collectives.cc:132-143: the ring reduce, count elements of
// datatype reduced from every rank's sendbuff into root's recvbuff (a
// non-root's recvbuff is never written, argcheck.cc:79-81)
VCCL_EXPORT ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                    ncclRedOp_t op, int root, ncclComm_t comm, hipStream_t stream) {
  return enqueue_check(kReduce, "Reduce", sendbuff, recvbuff, count, datatype, op, comm, stream, root);
}
// collectives.cc:112-123: the in-place broadcast
VCCL_EXPORT ncclResult_t ncclBcast(void* buff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm,
                                   hipStream_t stream) {
  return ncclBroadcast(buff, buff, count, datatype, root, comm, stream);
}

VCCL_EXPORT ncclResult_t ncclGroupStart(void) {
  tl_groupDepth++;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t ncclGroupEnd(void) {
  if (tl_groupDepth == 0) {
    VWARN("ncclGroupEnd: not in a group call.");
    return ncclInvalidUsage;
  }
  if (--tl_groupDepth > 0) return ncclSuccess;
  const ncclResult_t err = tl_groupError;
  tl_groupError = ncclSuccess;
  std::vector<Task> tasks;
  tasks.swap(tl_tasks);
  if (err != ncclSuccess) {  // a call of the group failed: drop the whole group
    VWARN("ncclGroupEnd: a call in the group failed (%d); %zu queued calls not launched",
          (int)err, tasks.size());
    tl_a2a.clear();
    return err;
  }
  const ncclResult_t r = launch_group(tasks);
  tl_a2a.clear();  // the all-to-all tasks' rows: launched, no longer referenced
  return r;
}

// nccl.h.in:472-473: ends the group like ncclGroupEnd but launches nothing;
// the run-time estimate needs the tuner's cost model (out of scope).
VCCL_EXPORT ncclResult_t ncclGroupSimulateEnd(ncclSimInfo_t* simInfo) {
  if (tl_groupDepth == 0) {
    VWARN("ncclGroupSimulateEnd: not in a group call.");
    return ncclInvalidUsage;
  }
  if (--tl_groupDepth > 0) return ncclSuccess;
  tl_groupError = ncclSuccess;
  tl_tasks.clear();
  tl_a2a.clear();
  if (simInfo) simInfo->estimatedTime = NCCL_UNDEF_FLOAT;
  return out_of_scope("ncclGroupSimulateEnd");
}

VCCL_EXPORT ncclResult_t ncclRedOpCreatePreMulSum(ncclRedOp_t* op, void* scalar, ncclDataType_t datatype,
                                                  ncclScalarResidence_t residence, ncclComm_t comm) {
  NCCLCHECK(comm_check(comm, "ncclRedOpCreatePreMulSum"));
  if (!op || !scalar) return ncclInvalidArgument;
  const int sz = type_size(datatype);
  if (sz < 1) return ncclInvalidArgument;
  int ix = -1;
  for (int i = 0; i < (int)comm->userOps.size(); i++)
    if (comm->userOps[i].freeNext != -1) { ix = i; break; }
  if (ix < 0) {
    comm->userOps.push_back(UserRedOp{});
    ix = (int)comm->userOps.size() - 1;
  }
  UserRedOp& u = comm->userOps[ix];
  u.freeNext = -1;
  u.datatype = datatype;
  u.devOp = OP_PREMULSUM;
  if (residence == ncclScalarHostImmediate) {
    u.argIsPtr = false;
    u.arg = 0;
    memcpy(&u.arg, scalar, (size_t)sz);
  } else {
    u.argIsPtr = true;
    u.arg = (uint64_t)(uintptr_t)scalar;
  }
  *op = (ncclRedOp_t)((int)ncclNumOps + ix);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t ncclRedOpDestroy(ncclRedOp_t op, ncclComm_t comm) {
  if (0 <= (int)op && (int)op < (int)ncclNumOps) {
    VWARN("ncclRedOpDestroy : operator is a NCCL builtin.");
    return ncclInvalidArgument;
  }
  if ((int)op < 0) {
    VWARN("ncclRedOpDestroy :  operator is garbage.");
    return ncclInvalidArgument;
  }
  if (comm == nullptr) {
    VWARN("ncclRedOpDestroy : invalid communicator passed.");
    return ncclInvalidArgument;
  }
  NCCLCHECK(comm_check(comm, "ncclRedOpDestroy"));
  const int ix = (int)op - (int)ncclNumOps;
  if (ix >= (int)comm->userOps.size() || comm->userOps[ix].freeNext != -1) {
    VWARN("ncclRedOpDestroy : operator unknown to this communicator.");
    return ncclInvalidArgument;
  }
  comm->userOps[ix].freeNext = 0;  // free
  return ncclSuccess;
}

// The profiling aliases (nccl.h: every nccl* entry point also as pnccl*).
#define VCCL_PALIAS(name) VCCL_EXPORT decltype(name) p##name __attribute__((alias(#name)));
VCCL_PALIAS(ncclAllReduce) VCCL_PALIAS(ncclReduceScatter) VCCL_PALIAS(ncclAllGather) VCCL_PALIAS(ncclBroadcast)
VCCL_PALIAS(ncclReduce) VCCL_PALIAS(ncclBcast) VCCL_PALIAS(ncclGroupStart) VCCL_PALIAS(ncclGroupEnd)
VCCL_PALIAS(ncclGroupSimulateEnd) VCCL_PALIAS(ncclRedOpCreatePreMulSum) VCCL_PALIAS(ncclRedOpDestroy)
VCCL_PALIAS(ncclSend) VCCL_PALIAS(ncclRecv) VCCL_PALIAS(ncclAllToAll) VCCL_PALIAS(ncclAllToAllv)
