// Collective API -> argument check -> op encoding -> task -> launch.
// (The planner lives in plan.cc, the launch path in launch.cc.)
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
// launch and whose mid-size pairs one direct launch (launch.cc launch_comm_p2p).  The vccl*
// extension exports at the end are wrappers over plan.h and launch.h.
#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>

#include "../../../include/vccl_device.h"
#include "../../../include/vccl_ext.h"
#include "../device/coll_types.hpp"
#include "../device/dispatch.hpp"
#include "launch.h"

namespace vccl {

static thread_local int tl_groupDepth = 0;
static thread_local std::vector<Task> tl_tasks;
static thread_local ncclResult_t tl_groupError = ncclSuccess;

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

// ncclGroupErrCheck (enqueue.cc:2516): inside a group the first failing call
// is remembered, and the outermost ncclGroupEnd then launches nothing of the
// group and returns that error (group.cc:528, :591).
static ncclResult_t enqueue_check(int coll, const char* name, const void* sendbuff, void* recvbuff,
                                  size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm* comm,
                                  hipStream_t stream, int root = 0) {
  const ncclResult_t r = enqueue_check_impl(coll, name, sendbuff, recvbuff, count, dt, op, comm, stream, root);
  if (r != ncclSuccess && tl_groupDepth > 0 && tl_groupError == ncclSuccess) tl_groupError = r;
  return r;
}

// The internal path codes (plan.h kAlgo*) and the public vcclAlgo_t.
static int public_algo(int a) {
  return a == kAlgoLL ? vcclAlgoLL : a == kAlgoDirect ? vcclAlgoDirect
         : a == kAlgoRingLL128 ? vcclAlgoLL128 : vcclAlgoRing;
}
static int internal_algo(int pub) {  // -1: not a path a call can be given
  return pub == vcclAlgoRing ? kAlgoRing : pub == vcclAlgoLL ? kAlgoLL
         : pub == vcclAlgoDirect ? kAlgoDirect : pub == vcclAlgoLL128 ? kAlgoRingLL128 : -1;
}

}  // namespace vccl

using namespace vccl;

#define VCCL_EXPORT extern "C" __attribute__((visibility("default")))

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
  if (!buff && count > 0) {
    VWARN("%s : NULL buffer", name);
    return ncclInvalidArgument;
  }
  if (*(volatile int*)comm->errorFlag) {
    const ncclResult_t e = error_word_result(comm);
    comm->asyncError = e;
    return e;
  }
  NCCLCHECK(p2p_usable(comm, name));
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
  const ncclResult_t r = p2p_check_impl(send, name, buff, count, dt, peer, comm, stream);
  if (r != ncclSuccess && tl_groupDepth > 0 && tl_groupError == ncclSuccess) tl_groupError = r;
  return r;
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

// The all-to-all of a comm whose one-hop LL or direct all-to-all is on
// (llA2aMaxBytes > 0 || directA2aMaxBytes > 0): ONE queued task (kTaskA2a) —
// launch_group splits its pairs between the LL launch, the direct launch and
// the p2p launch.  The per-pair checks of the expansion below, in
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
  auto pair_check = [&](const void* buff, size_t cnt) -> ncclResult_t {  // p2p_check_impl's, after its peer and type checks
    if (!buff && cnt > 0) {
      VWARN("%s : NULL buffer", name);
      return ncclInvalidArgument;
    }
    if (*(volatile int*)comm->errorFlag) {
      const ncclResult_t e = error_word_result(comm);
      comm->asyncError = e;
      return e;
    }
    return p2p_usable(comm, name);
  };
  ncclResult_t r = ncclSuccess;
  for (int p = 0; p < n && r == ncclSuccess; p++) {
    const size_t sc = sendcounts ? sendcounts[p] : count, so = sdispls ? sdispls[p] : (size_t)p * count;
    const size_t rc = recvcounts ? recvcounts[p] : count, ro = rdispls ? rdispls[p] : (size_t)p * count;
    a.sendBytes[p] = (int64_t)(sc * esz), a.sendOff[p] = (int64_t)(so * esz);
    a.recvBytes[p] = (int64_t)(rc * esz), a.recvOff[p] = (int64_t)(ro * esz);
    r = pair_check(sendbuff, sc);
    if (r == ncclSuccess) r = pair_check(recvbuff, rc);
  }
  if (r != ncclSuccess) {
    if (tl_groupDepth > 0 && tl_groupError == ncclSuccess) tl_groupError = r;
    return r;
  }
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
  if (r != ncclSuccess) {
    if (tl_groupDepth > 0 && tl_groupError == ncclSuccess) tl_groupError = r;
    return r;
  }
  const size_t esz = (size_t)type_size(dt);
  const int n = comm->nRanks;
  static_assert(kDirectMaxRanks <= kOrderMaxRanks, "A2aArgs holds kOrderMaxRanks rows");
  if ((comm->llA2aMaxBytes > 0 || comm->directA2aMaxBytes > 0) && n <= kOrderMaxRanks)
    return all_to_all_task(name, sendbuff, sendcounts, sdispls, recvbuff, recvcounts, rdispls, count, dt, comm, stream);
  ncclGroupStart();
  for (int p = 0; p < n && r == ncclSuccess; p++) {
    const size_t sc = sendcounts ? sendcounts[p] : count, so = sdispls ? sdispls[p] : (size_t)p * count;
    const size_t rc = recvcounts ? recvcounts[p] : count, ro = rdispls ? rdispls[p] : (size_t)p * count;
    r = p2p_check(true, name, sendbuff ? (const char*)sendbuff + so * esz : nullptr, sc, dt, p, comm, stream);
    if (r == ncclSuccess)
      r = p2p_check(false, name, recvbuff ? (char*)recvbuff + ro * esz : nullptr, rc, dt, p, comm, stream);
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
    if (tl_groupDepth > 0 && tl_groupError == ncclSuccess) tl_groupError = ncclInvalidArgument;
    return ncclInvalidArgument;
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

VCCL_EXPORT ncclResult_t vcclHostToDevRedOp(ncclRedOp_t op, ncclDataType_t datatype, int nRanks,
                                            int* devOp, uint64_t* opArg) {
  if (!devOp || !opArg || nRanks < 1) return ncclInvalidArgument;
  if ((int)datatype < 0 || (int)datatype >= (int)ncclNumTypes) return ncclInvalidArgument;
  return host_to_dev_redop(op, datatype, nRanks, devOp, opArg);
}

VCCL_EXPORT const char* vcclBuildInfo(void) {
#define VCCL_STR2(x) #x
#define VCCL_STR(x) VCCL_STR2(x)
  return "vccl-mi355x " __DATE__ " gfx950; one-shot LL / two-shot direct / SIMPLE ring / LL128 ring "
         "(" VCCL_STR(VCCL_LL128_LINE) "-byte lines) over xGMI (uncached receiver buffers); "
         "reduce-copy 16B packs; VCCL group plans";
}

// The profiling aliases (nccl.h: every nccl* entry point also as pnccl*).
#define VCCL_PALIAS(name) VCCL_EXPORT decltype(name) p##name __attribute__((alias(#name)));
VCCL_PALIAS(ncclAllReduce) VCCL_PALIAS(ncclReduceScatter) VCCL_PALIAS(ncclAllGather) VCCL_PALIAS(ncclBroadcast)
VCCL_PALIAS(ncclReduce) VCCL_PALIAS(ncclBcast) VCCL_PALIAS(ncclGroupStart) VCCL_PALIAS(ncclGroupEnd)
VCCL_PALIAS(ncclGroupSimulateEnd) VCCL_PALIAS(ncclRedOpCreatePreMulSum) VCCL_PALIAS(ncclRedOpDestroy)
VCCL_PALIAS(ncclSend) VCCL_PALIAS(ncclRecv) VCCL_PALIAS(ncclAllToAll) VCCL_PALIAS(ncclAllToAllv)

// ---------------------------------------------------------------- vccl_ext.h
VCCL_EXPORT ncclResult_t vcclCommCollAlgo(ncclComm_t comm, int coll, size_t count, ncclDataType_t datatype, int* algo) {
  NCCLCHECK(comm_check(comm, "vcclCommCollAlgo"));
  if (!algo || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1) return ncclInvalidArgument;
  if (comm->nRanks == 1) {
    *algo = vcclAlgoOneRank;
    return ncclSuccess;
  }
  // the public collective codes are the Coll values (vccl_ext.h)
  *algo = public_algo(select_algo(policy_of(comm), coll, type_size(datatype), (int64_t)count));
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRingPartition(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                           int nChannels, int proto, size_t stepBytes, int nThreads,
                                           int64_t* out) {
  if (!out || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1 || nRanks < 1 ||
      nChannels < 1 || nChannels > kMaxChannels || count == 0 || stepBytes < 4096 || nThreads < 64 ||
      (proto != kProtoSimple && proto != kProtoLL128 && proto != kProtoLL))
    return ncclInvalidArgument;
  const CallSize sz = call_size(coll, count, datatype);
  cbd_words(cbd_schedule(coll, sz.count, sz.eltSize, nRanks, nChannels, proto, (int64_t)stepBytes, nThreads), out);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclRingChunkOf(size_t count, ncclDataType_t datatype, int nRanks, int nChannels,
                                         size_t slotBytes, int nThreads, size_t i, int64_t* out) {
  if (!out || type_size(datatype) < 1 || nRanks < 1 || nChannels < 1 || nChannels > kMaxChannels ||
      count == 0 || i >= count || slotBytes < 4096 || nThreads < 64)
    return ncclInvalidArgument;
  const int64_t esz = type_size(datatype);
  const CbdPlan p = cbd_schedule(kAllReduce, (int64_t)count, esz, nRanks, nChannels, kProtoSimple,
                                 (int64_t)slotBytes, nThreads);
  const CbdLite cbd{p.channelLo, p.channelHi, p.countLo, p.countMid, (int64_t)count};
  int k;
  int64_t end;
  out[0] = ar_chunk_of(cbd, p.chunkLo, nRanks, std::max<int64_t>(1, 16 / esz), (int64_t)i, &k, &end);
  out[1] = k;
  out[2] = end;
  return ncclSuccess;
}

// vccl_ext.h: the group planner on explicit inputs (host only).
static ncclResult_t group_plan_export(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                                      const int* ops, int nRanks, int nChannels, const PlanGeometry& geo,
                                      const AlgoPolicy* pol, int* algos, int* order, int* planOf, int64_t* cbd) {
  if (nCalls < 1 || !colls || !counts || !datatypes || !ops || !order || !planOf || !cbd || nRanks < 1 ||
      nChannels < 1 || nChannels > kMaxChannels || geo.stepBytes < 4096 || geo.nThreads < 64 ||
      geo.ll128StepBytes < 1920 * 16 || geo.ll128Threads < 64)
    return ncclInvalidArgument;
  std::vector<GroupTask> g;
  for (int i = 0; i < nCalls; i++) {
    const ncclDataType_t dt = (ncclDataType_t)datatypes[i];
    const int c = colls[i];
    if (c < kAllReduce || c > kReduce || type_size(dt) < 1 || counts[i] == 0) return ncclInvalidArgument;
    int devOp = OP_SUM;
    uint64_t arg = 0;
    if (!is_copy_coll(c)) NCCLCHECK(host_to_dev_redop((ncclRedOp_t)ops[i], dt, nRanks, &devOp, &arg));
    const int kt = kernel_type_of_call(c, devOp, dt);
    if (kt < 0) return ncclInvalidArgument;
    g.push_back(group_task_of(c, counts[i], dt, devOp, kt));
  }
  GroupPlanOut p;
  group_plan(g, nRanks, nChannels, geo, pol, &p);
  for (int i = 0; i < nCalls; i++) {
    order[i] = p.order[i];
    planOf[i] = p.planOf[i];
    if (algos) algos[i] = public_algo(p.algo[i]);
    cbd_words(p.cbd[i], cbd + 8 * (size_t)i);
  }
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclGroupPlan(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                                       const int* ops, int nRanks, int nChannels, size_t stepBytes, int nThreads,
                                       int* order, int* planOf, int64_t* cbd) {
  const PlanGeometry geo{(int64_t)stepBytes, nThreads, kDefaultLL128.stepBytes, kDefaultLL128.nThreads};
  return group_plan_export(nCalls, colls, counts, datatypes, ops, nRanks, nChannels, geo, nullptr, nullptr, order,
                           planOf, cbd);
}

VCCL_EXPORT ncclResult_t vcclGroupPlanEx(int nCalls, const int* colls, const size_t* counts, const int* datatypes,
                                         const int* ops, int nRanks, int nChannels, const int64_t* geometry,
                                         const int64_t* policy, int* algos, int* order, int* planOf,
                                         int64_t* cbd) {
  if (!geometry) return ncclInvalidArgument;
  const PlanGeometry geo{geometry[0], geometry[1], geometry[2], geometry[3]};
  if (policy && (policy[0] < 0 || policy[0] > 4)) return ncclInvalidArgument;
  const int64_t* q = policy;  // the ten words are AlgoPolicy's fields after nRanks, in order
  AlgoPolicy pol;
  if (q) pol = AlgoPolicy{nRanks, (int)q[0], q[1], (uint64_t)q[2], (uint64_t)q[3], q[4] != 0, (uint64_t)q[5],
                          (uint64_t)q[6], q[7] != 0, (uint64_t)q[8], (uint64_t)q[9]};
  return group_plan_export(nCalls, colls, counts, datatypes, ops, nRanks, nChannels, geo, policy ? &pol : nullptr,
                           algos, order, planOf, cbd);
}

// vccl_ext.h: the path every call of a group would take on this comm (its
// aggregate's, as launch_planned lays the group out); no launch.
VCCL_EXPORT ncclResult_t vcclCommGroupAlgos(ncclComm_t comm, int nCalls, const int* colls, const size_t* counts,
                                            const int* datatypes, const int* ops, int* algos) {
  NCCLCHECK(comm_check(comm, "vcclCommGroupAlgos"));
  if (nCalls < 1 || !algos) return ncclInvalidArgument;
  if (comm->nRanks == 1) {
    for (int i = 0; i < nCalls; i++) algos[i] = vcclAlgoOneRank;
    return ncclSuccess;
  }
  std::vector<int> order(nCalls), planOf(nCalls);
  std::vector<int64_t> cbd(8 * (size_t)nCalls);
  const AlgoPolicy pol = policy_of(comm);
  // without LL128 FIFOs no call takes the LL128 ring: its geometry is moot
  const bool ll128 = comm->ll128StepBytes > 0;
  const PlanGeometry geo{comm->stepBytes, comm->nThreads, ll128 ? comm->ll128StepBytes : kDefaultLL128.stepBytes,
                         ll128 ? comm->ll128Threads : kDefaultLL128.nThreads};
  return group_plan_export(nCalls, colls, counts, datatypes, ops, comm->nRanks, comm->nChannels, geo, &pol, algos,
                           order.data(), planOf.data(), cbd.data());
}

// vccl_ext.h: the point-to-point planner on explicit inputs (host only).
VCCL_EXPORT ncclResult_t vcclP2pPlan(int rank, int nRanks, int nCalls, const int* kinds, const int* peers,
                                     const size_t* bytes, const uint64_t* buffs, int parts, size_t minPartBytes,
                                     size_t stepBytes, int gMin, int gCap, int maxWorks, int cap, int* nItems,
                                     int* nWgs, int64_t* items) {
  if (nRanks < 1 || nRanks > kP2pMaxRanks || rank < 0 || rank >= nRanks || nCalls < 0 || (nCalls && (!kinds || !peers || !bytes)) ||
      parts < 1 || parts > kP2pMaxParts || minPartBytes < 256 || stepBytes < 4096 || stepBytes % 512 || maxWorks < 1 ||
      maxWorks > kP2pMaxWorks || !nItems || cap < 0 || (cap && !items))
    return ncclInvalidArgument;
  std::vector<P2pCall> calls;
  for (int i = 0; i < nCalls; i++) {
    if ((kinds[i] != kP2pCallSend && kinds[i] != kP2pCallRecv) || peers[i] < 0 || peers[i] >= nRanks)
      return ncclInvalidArgument;
    calls.push_back(P2pCall{kinds[i], peers[i], (int64_t)bytes[i], buffs ? buffs[i] : (uint64_t)(2 * i + 1)});
  }
  P2pPlanOut plan;
  NCCLCHECK(p2p_plan(rank, nRanks, calls, P2pGeometry{parts, (int64_t)minPartBytes, (int64_t)stepBytes}, gMin, gCap,
                     maxWorks, &plan));
  *nItems = (int)plan.items.size();
  if (nWgs) *nWgs = plan.nWgs;
  if ((int)plan.items.size() > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < plan.items.size(); k++) {
    const P2pItem& it = plan.items[k];
    const int64_t v[12] = {it.launch, it.wg, it.kind, it.sweep, it.round, it.part,
                           it.peer,   it.call, it.call2, it.offset, it.bytes, it.steps};
    for (int j = 0; j < 12; j++) items[12 * k + j] = v[j];
  }
  return ncclSuccess;
}

// vccl_ext.h: select_algo on an explicit policy with the rooted LL threshold
// as a comm would carry it (host only).
VCCL_EXPORT ncclResult_t vcclRootedAlgo(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                        const int64_t* policy, int64_t threshold, int llAllowed, int anyNet,
                                        int64_t* effective, int* algo) {
  if (!policy || !algo || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1 || nRanks < 1 ||
      nRanks > kMaxRanks || policy[0] < 0 || policy[0] > 4 || policy[1] < 0)
    return ncclInvalidArgument;
  const int64_t* q = policy;
  AlgoPolicy pol{nRanks, (int)q[0], q[1], (uint64_t)q[2], (uint64_t)q[3], q[4] != 0, (uint64_t)q[5],
                 (uint64_t)q[6], q[7] != 0, (uint64_t)q[8], (uint64_t)q[9]};
  if (threshold < 0) threshold = param_int("LL_ROOTED_THRESHOLD", 0);
  pol.llRootedMax = ll_rooted_max(threshold, pol.llSlotBytes, llAllowed != 0, anyNet != 0, nRanks);
  if (effective) *effective = (int64_t)pol.llRootedMax;
  const CallSize sz = call_size(coll, count, datatype);
  *algo = public_algo(select_algo(pol, coll, sz.eltSize, sz.count));  // one rank: the ring, as select_algo says
  return ncclSuccess;
}

// vccl_ext.h: vcclRootedAlgo plus the rooted direct threshold (host only).
VCCL_EXPORT ncclResult_t vcclRootedAlgoEx(int coll, size_t count, ncclDataType_t datatype, int nRanks,
                                          const int64_t* policy, int64_t threshold, int llAllowed, int anyNet,
                                          int64_t directThreshold, int directAllowed, int64_t* effective,
                                          int64_t* directEffective, int* algo) {
  if (!policy || !algo || coll < kAllReduce || coll > kReduce || type_size(datatype) < 1 || nRanks < 1 ||
      nRanks > kMaxRanks || policy[0] < 0 || policy[0] > 4 || policy[1] < 0)
    return ncclInvalidArgument;
  const int64_t* q = policy;
  AlgoPolicy pol{nRanks, (int)q[0], q[1], (uint64_t)q[2], (uint64_t)q[3], q[4] != 0, (uint64_t)q[5],
                 (uint64_t)q[6], q[7] != 0, (uint64_t)q[8], (uint64_t)q[9]};
  if (threshold < 0) threshold = param_int("LL_ROOTED_THRESHOLD", 0);
  if (directThreshold < 0) directThreshold = param_int("DIRECT_ROOTED_THRESHOLD", 0);
  pol.llRootedMax = ll_rooted_max(threshold, pol.llSlotBytes, llAllowed != 0, anyNet != 0, nRanks);
  pol.directRootedMax = direct_rooted_max(directThreshold, pol.direct, directAllowed != 0, anyNet != 0, nRanks);
  if (effective) *effective = (int64_t)pol.llRootedMax;
  if (directEffective) *directEffective = (int64_t)pol.directRootedMax;
  const CallSize sz = call_size(coll, count, datatype);
  *algo = public_algo(select_algo(pol, coll, sz.eltSize, sz.count));
  return ncclSuccess;
}

// vccl_ext.h: one rooted direct call's geometry and the steps of one chunk
// as `rank` runs it (host only).
VCCL_EXPORT ncclResult_t vcclDirectRootedPlan(int coll, int nRanks, int rank, int root, size_t count,
                                              ncclDataType_t datatype, int64_t regionBytes, int chunk, int cap,
                                              int64_t* geometry, int* owners, int* nSteps, int64_t* steps) {
  if ((coll != kBroadcast && coll != kReduce) || nRanks < 2 || nRanks > kDirectMaxRanks || rank < 0 ||
      rank >= nRanks || root < 0 || root >= nRanks || type_size(datatype) < 1 || count == 0 ||
      count > (size_t)1 << 56 || regionBytes < 32 || regionBytes > (int64_t)1 << 40 || !geometry || !nSteps ||
      cap < 0 || (cap && !steps))
    return ncclInvalidArgument;
  const CallSize sz = call_size(coll, count, datatype);
  DirectRootedPlanOut out;
  NCCLCHECK(direct_rooted_plan(coll, nRanks, rank, root, sz.count, sz.eltSize, regionBytes, chunk, &out));
  geometry[0] = out.chunkElts;
  geometry[1] = out.nChunks;
  geometry[2] = out.shardElts;
  geometry[3] = (int64_t)out.owner.size();
  if (owners)
    for (size_t j = 0; j < out.owner.size(); j++) owners[j] = out.owner[j];
  *nSteps = (int)out.steps.size();
  if (*nSteps > cap) return ncclInvalidArgument;
  for (size_t k = 0; k < out.steps.size(); k++) {
    const DirectStep& d = out.steps[k];
    const int64_t v[8] = {d.kind, d.phase, d.peer, d.region, d.regionOff, d.userOff, d.bytes, d.src};
    for (int j = 0; j < 8; j++) steps[8 * k + j] = v[j];
  }
  return ncclSuccess;
}

// vccl_ext.h: the line layout of one rooted LL launch (host only).
VCCL_EXPORT ncclResult_t vcclLLRootedPlan(int coll, int nRanks, int rank, int nParts, const int* roots,
                                          const size_t* bytes, int64_t linesPerSlot, int cap, int64_t* line0,
                                          int* nStores, int64_t* stores, int* nPolls, int64_t* polls) {
  if ((coll != kBroadcast && coll != kReduce) || nRanks < 2 || nRanks > kOrderMaxRanks || rank < 0 ||
      rank >= nRanks || nParts < 1 || nParts > kLLMaxParts || !roots || !bytes || linesPerSlot < 1 || cap < 0 ||
      !nStores || !nPolls || (cap && (!stores || !polls)))
    return ncclInvalidArgument;
  std::vector<int> r(roots, roots + nParts);
  std::vector<int64_t> b(nParts);
  for (int i = 0; i < nParts; i++) {
    if (r[i] < 0 || r[i] >= nRanks || bytes[i] > (size_t)linesPerSlot * 8) return ncclInvalidArgument;
    b[i] = (int64_t)bytes[i];
  }
  LLRootedPlanOut out;
  NCCLCHECK(ll_rooted_plan(coll, nRanks, rank, r, b, linesPerSlot, &out));
  *nStores = (int)out.stores.size();
  *nPolls = (int)out.polls.size();
  if (line0)
    for (int i = 0; i < nParts; i++) line0[i] = out.line0[i];
  if (*nStores > cap || *nPolls > cap) return ncclInvalidArgument;
  auto put = [](const std::vector<LLRange>& v, int64_t* o) {
    for (size_t k = 0; k < v.size(); k++) {
      o[4 * k] = v[k].peer, o[4 * k + 1] = v[k].part, o[4 * k + 2] = v[k].line0, o[4 * k + 3] = v[k].line1;
    }
  };
  put(out.stores, stores);
  put(out.polls, polls);
  return ncclSuccess;
}

// vccl_ext.h: a comm's VCCL_LL_A2A_THRESHOLD as it takes effect (host only).
VCCL_EXPORT ncclResult_t vcclLLA2aMax(int64_t threshold, int64_t llSlotBytes, int llAllowed, int anyNet, int nRanks,
                                      int hasP2p, int64_t* effective) {
  if (!effective || llSlotBytes < 0 || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("LL_A2A_THRESHOLD", 0);
  *effective = (int64_t)ll_a2a_max(threshold, llSlotBytes, llAllowed != 0, anyNet != 0, nRanks, hasP2p != 0);
  return ncclSuccess;
}

// vccl_ext.h: one all-to-all(v) call's split between the LL launch and the
// FIFO launch as `rank` runs it (host only).
VCCL_EXPORT ncclResult_t vcclLLA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* recvBytes,
                                       int uniform, int64_t llA2aMax, int64_t linesPerSlot, int* sendLL, int* recvLL,
                                       int* launch, int64_t* stores, int64_t* polls, int* nResSends, int* resSends,
                                       int* nResRecvs, int* resRecvs) {
  if (nRanks < 2 || nRanks > kOrderMaxRanks || rank < 0 || rank >= nRanks || !sendBytes || !recvBytes ||
      llA2aMax < 0 || linesPerSlot < 1 || llA2aMax > linesPerSlot * 8 || !sendLL || !recvLL || !launch || !stores ||
      !polls || !nResSends || !resSends || !nResRecvs || !resRecvs)
    return ncclInvalidArgument;
  int64_t sb[kOrderMaxRanks], rb[kOrderMaxRanks];
  for (int p = 0; p < nRanks; p++) {
    if (sendBytes[p] > (size_t)1 << 60 || recvBytes[p] > (size_t)1 << 60) return ncclInvalidArgument;
    if (uniform && (sendBytes[p] != sendBytes[0] || recvBytes[p] != sendBytes[0])) return ncclInvalidArgument;
    sb[p] = (int64_t)sendBytes[p];
    rb[p] = (int64_t)recvBytes[p];
  }
  LLA2aPlanOut out;
  NCCLCHECK(ll_a2a_plan(nRanks, rank, sb, rb, uniform != 0, (uint64_t)llA2aMax, linesPerSlot, &out));
  *launch = out.launch;
  for (int p = 0; p < nRanks; p++) sendLL[p] = out.sendLL[p], recvLL[p] = out.recvLL[p];
  auto put = [](const std::vector<LLRange>& v, int64_t* o) {  // nRanks - 1 ranges with a launch, else none
    for (size_t k = 0; k < v.size(); k++) {
      o[4 * k] = v[k].peer, o[4 * k + 1] = v[k].part, o[4 * k + 2] = v[k].line0, o[4 * k + 3] = v[k].line1;
    }
  };
  put(out.stores, stores);
  put(out.polls, polls);
  *nResSends = (int)out.resSends.size();
  *nResRecvs = (int)out.resRecvs.size();
  std::copy(out.resSends.begin(), out.resSends.end(), resSends);
  std::copy(out.resRecvs.begin(), out.resRecvs.end(), resRecvs);
  return ncclSuccess;
}

// vccl_ext.h: a comm's VCCL_DIRECT_A2A_THRESHOLD as it takes effect (host only).
VCCL_EXPORT ncclResult_t vcclDirectA2aMax(int64_t threshold, int64_t regionBytes, int directAllowed, int anyNet,
                                          int nRanks, int hasP2p, int64_t* effective) {
  if (!effective || regionBytes < 0 || nRanks < 1) return ncclInvalidArgument;
  if (threshold < 0) threshold = param_int("DIRECT_A2A_THRESHOLD", 0);
  *effective =
      (int64_t)direct_a2a_max(threshold, regionBytes, directAllowed != 0, anyNet != 0, nRanks, hasP2p != 0);
  return ncclSuccess;
}

// vccl_ext.h: one all-to-all(v) call's three-way split between the LL launch,
// the direct launch and the FIFO launch as `rank` runs it (host only).
VCCL_EXPORT ncclResult_t vcclDirectA2aPlan(int nRanks, int rank, const size_t* sendBytes, const size_t* recvBytes,
                                           int uniform, int64_t llA2aMax, int64_t directA2aMax, int64_t linesPerSlot,
                                           int minCTAs, int maxCTAs, int directMaxBlocks, int* sendPath,
                                           int* recvPath, int* llLaunch, int* directLaunch, int* nBlocks,
                                           int64_t* blkBytes, int* nResSends, int* resSends, int* nResRecvs,
                                           int* resRecvs) {
  if (nRanks < 2 || nRanks > kDirectMaxRanks || rank < 0 || rank >= nRanks || !sendBytes || !recvBytes ||
      llA2aMax < 0 || linesPerSlot < 0 || linesPerSlot > (int64_t)1 << 40 || llA2aMax > linesPerSlot * 8 ||
      directA2aMax < 0 || directA2aMax > (int64_t)1 << 40 || minCTAs < 0 || maxCTAs < 1 || directMaxBlocks < 1 ||
      !sendPath || !recvPath || !llLaunch || !directLaunch || !nBlocks || !blkBytes || !nResSends || !resSends ||
      !nResRecvs || !resRecvs)
    return ncclInvalidArgument;
  int64_t sb[kOrderMaxRanks], rb[kOrderMaxRanks];
  for (int p = 0; p < nRanks; p++) {
    if (sendBytes[p] > (size_t)1 << 60 || recvBytes[p] > (size_t)1 << 60) return ncclInvalidArgument;
    if (uniform && (sendBytes[p] != sendBytes[0] || recvBytes[p] != sendBytes[0])) return ncclInvalidArgument;
    sb[p] = (int64_t)sendBytes[p];
    rb[p] = (int64_t)recvBytes[p];
  }
  DirectA2aPlanOut out;
  NCCLCHECK(direct_a2a_plan(nRanks, rank, sb, rb, uniform != 0, (uint64_t)llA2aMax, (uint64_t)directA2aMax,
                            linesPerSlot, minCTAs, maxCTAs, directMaxBlocks, &out));
  *llLaunch = out.llLaunch;
  *directLaunch = out.directLaunch;
  *nBlocks = out.nBlocks;
  *blkBytes = out.blkBytes;
  for (int p = 0; p < nRanks; p++) sendPath[p] = out.sendPath[p], recvPath[p] = out.recvPath[p];
  *nResSends = (int)out.resSends.size();
  *nResRecvs = (int)out.resRecvs.size();
  std::copy(out.resSends.begin(), out.resSends.end(), resSends);
  std::copy(out.resRecvs.begin(), out.resRecvs.end(), resRecvs);
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclCommA2aStats(ncclComm_t comm, unsigned long long* llLaunches, unsigned long long* llPairs,
                                          unsigned long long* fifoPairs) {
  NCCLCHECK(comm_check(comm, "vcclCommA2aStats"));
  if (llLaunches) *llLaunches = comm->a2aLLLaunches;
  if (llPairs) *llPairs = comm->a2aLLPairs;
  if (fifoPairs) *fifoPairs = comm->a2aFifoPairs;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclCommA2aStatsEx(ncclComm_t comm, unsigned long long* llLaunches,
                                            unsigned long long* llPairs, unsigned long long* directLaunches,
                                            unsigned long long* directPairs, unsigned long long* fifoPairs) {
  NCCLCHECK(comm_check(comm, "vcclCommA2aStatsEx"));
  if (llLaunches) *llLaunches = comm->a2aLLLaunches;
  if (llPairs) *llPairs = comm->a2aLLPairs;
  if (directLaunches) *directLaunches = comm->a2aDirectLaunches;
  if (directPairs) *directPairs = comm->a2aDirectPairs;
  if (fifoPairs) *fifoPairs = comm->a2aFifoPairs;
  return ncclSuccess;
}

// A tuning / measurement knob: every rank must call it alike, between calls.
VCCL_EXPORT ncclResult_t vcclCommSetA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetA2aThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  comm->llA2aMaxBytes = ll_a2a_max_of(*comm, bytes, comm->nRanks, comm->p2pOff == kP2pOffNet,
                                      comm->p2pConns != nullptr && comm->llBuf != nullptr &&
                                          (int)comm->llPeer.size() >= comm->nRanks);
  if (effective) *effective = (int64_t)comm->llA2aMaxBytes;
  return ncclSuccess;
}

// Likewise for the direct all-to-all.
VCCL_EXPORT ncclResult_t vcclCommSetDirectA2aThreshold(ncclComm_t comm, int64_t bytes, int64_t* effective) {
  NCCLCHECK(comm_check(comm, "vcclCommSetDirectA2aThreshold"));
  if (bytes < 0) return ncclInvalidArgument;
  comm->directA2aMaxBytes = direct_a2a_max_of(*comm, bytes, comm->nRanks, comm->p2pOff == kP2pOffNet,
                                              comm->p2pConns != nullptr && comm->dPeers != nullptr);
  if (effective) *effective = (int64_t)comm->directA2aMaxBytes;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclCommSetAlgo(ncclComm_t comm, int algo) {
  NCCLCHECK(comm_check(comm, "vcclCommSetAlgo"));
  const int a = internal_algo(algo);
  if (algo != -1 && a < 0) return ncclInvalidArgument;
  // algoForce (core.h): 0 automatic, else 1 + the path; forced LL128 without
  // its buffers runs the SIMPLE ring (select_algo)
  comm->algoForce = algo == -1 ? 0 : a + 1;
  return ncclSuccess;
}

VCCL_EXPORT ncclResult_t vcclCommRingTrace(ncclComm_t comm, void* hostBuf, size_t bytes, int* nChannels,
                                           int* cap) {
  NCCLCHECK(comm_check(comm, "vcclCommRingTrace"));
  if (nChannels) *nChannels = comm->nChannels;
  if (cap) *cap = comm->ringTraceCap;
  if (!comm->ringTrace) return ncclInvalidUsage;
  const size_t need = (size_t)comm->nChannels * comm->ringTraceCap * sizeof(RingTraceRec);
  if (!hostBuf || bytes < need) return ncclInvalidArgument;
  DeviceGuard dev(comm->device);
  HIPCHECK(dev.status);
  const hipError_t e = hipMemcpy(hostBuf, comm->ringTrace, need, hipMemcpyDeviceToHost);
  if (e == hipSuccess) (void)hipMemset(comm->ringTrace, 0, need);
  return e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

VCCL_EXPORT ncclResult_t vcclCommLaunchStats(ncclComm_t comm, unsigned long long* collectives,
                                             unsigned long long* fusedLaunches) {
  NCCLCHECK(comm_check(comm, "vcclCommLaunchStats"));
  if (collectives) *collectives = comm->opCount;
  if (fusedLaunches) *fusedLaunches = comm->fusedLaunches;
  return ncclSuccess;
}
