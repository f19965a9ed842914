// A stand-in for librccl, for tests only: the twelve entry points the engine resolves (load_rccl_once in csrc/nb_comm.hip),
// with all ranks as threads of ONE process on ONE device.  RCCL itself refuses two ranks on one device; with this library
// behind NB_RCCL_LIB several rank handles run the engine's own native-collective path against real foreign rows on the one
// GPU a test box has (tests/test_rccl_ranks_gpu.py).  Who belongs to a communicator, the host barrier and the abort flag
// live in shim_group.c, which has no HIP in it.
//
// A collective is asynchronous, as RCCL's are: it enqueues event waits, copies and at most one kernel on the caller's stream
// and returns; it never synchronises a stream or the device.  The protocol of ncclAllGather(send, recv, count, type, comm, st):
//   1. record "my rows are written" on st
//   2. host barrier (a stream wait on an event nobody has recorded yet is a no-op: the barrier must come before the waits)
//   3. for every peer, ascending: st waits for the peer's event, then copies its `count` elements into recv + p * count
//   4. record "I have read everyone" on st
//   5. second host barrier, then st waits for every peer's read event: later work on st that overwrites the send rows is
//      ordered behind the peers' reads
// ncclReduceScatter is the same with one kernel in place of the copies: recv[i] = the sum over ranks d = 0, 1, ... of
// send_d[rank * count + i], from +0, ascending, in the element type -- the order of nb_sym_sum_shards and nb_peer_sum.
//
// NB_SHIM_LATE_US (read when a communicator is created) makes every collective land late: a host function enqueued on st
// sleeps that long before the copies, so that an engine that forgets a wait reads stale rows instead of getting lucky.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

#include <unistd.h>

#include "shim_group.h"

#define NB_SHIM_VERSION 10203       // what ncclGetVersion reports: below 20000, no RCCL ever carried it

struct ncclComm {
    shim_group* group = nullptr;
    int nranks = 0, rank = 0;
    uint64_t seq = 0;               // collectives issued on this communicator
    long late_us = 0;
};

namespace {

// what a rank publishes in its slots of the group
enum { kSlotWritten = 0, kSlotRead = 1, kSlotSend = 2 };

struct Peers { const void* p[SHIM_MAX_RANKS]; };

// out[i] = +0 + in_0[i] + in_1[i] + ...   (adds only: nothing to contract, nothing reassociated)
template <typename T>
__global__ void shim_sum(const Peers src, T* out, size_t count, int nranks)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    T s = 0;
    for (int d = 0; d < nranks; ++d) s += ((const T*)src.p[d])[i];
    out[i] = s;
}

void sleep_us(void* us) { std::this_thread::sleep_for(std::chrono::microseconds((long)(intptr_t)us)); }

void free_events(shim_group* g)
{
    for (int r = 0; r < SHIM_MAX_RANKS; ++r) {
        void** slot = shim_group_slot(g, r);
        if (!slot) break;
        if (slot[kSlotWritten]) (void)hipEventDestroy((hipEvent_t)slot[kSlotWritten]);
        if (slot[kSlotRead]) (void)hipEventDestroy((hipEvent_t)slot[kSlotRead]);
    }
}

size_t size_of(ncclDataType_t t) { return t == ncclFloat ? 4 : t == ncclDouble ? 8 : 0; }

ncclResult_t broken(ncclComm* c) { shim_group_abort(c->group); return ncclInternalError; }

#define SHIM_HIP(c, call) do { if ((call) != hipSuccess) { (void)hipGetLastError(); return broken(c); } } while (0)
#define SHIM_BARRIER(c, phase) do { if (shim_group_barrier((c)->group, (c)->rank, ((c)->seq << 2) | (phase)) != SHIM_OK) return broken(c); } while (0)

// One collective.  reduce: the kernel; otherwise the copies of an all-gather.
ncclResult_t collective(bool reduce, const void* send, void* recv, size_t count, ncclDataType_t type, ncclComm* c, hipStream_t st)
{
    const size_t esz = size_of(type);
    if (!c || !c->group) return ncclInvalidArgument;
    if (!send || !recv || !esz) return ncclInvalidArgument;
    if (shim_group_aborted(c->group)) return ncclInternalError;
    ++c->seq;
    void** mine = shim_group_slot(c->group, c->rank);
    mine[kSlotSend] = const_cast<void*>(send);
    SHIM_HIP(c, hipEventRecord((hipEvent_t)mine[kSlotWritten], st));                     // 1
    SHIM_BARRIER(c, reduce ? 2u : 0u);                                                   // 2
    for (int p = 0; p < c->nranks; ++p)                                                  // 3
        if (p != c->rank) SHIM_HIP(c, hipStreamWaitEvent(st, (hipEvent_t)shim_group_slot(c->group, p)[kSlotWritten], 0));
    if (c->late_us > 0) SHIM_HIP(c, hipLaunchHostFunc(st, sleep_us, (void*)(intptr_t)c->late_us));
    if (reduce) {
        Peers src{};
        for (int p = 0; p < c->nranks; ++p) src.p[p] = (const char*)shim_group_slot(c->group, p)[kSlotSend] + esz * count * c->rank;
        const unsigned block = 256, grid = (unsigned)((count + block - 1) / block);
        if (count) {
            if (type == ncclFloat) hipLaunchKernelGGL(shim_sum<float>, dim3(grid), dim3(block), 0, st, src, (float*)recv, count, c->nranks);
            else hipLaunchKernelGGL(shim_sum<double>, dim3(grid), dim3(block), 0, st, src, (double*)recv, count, c->nranks);
            SHIM_HIP(c, hipGetLastError());
        }
    } else {
        for (int p = 0; p < c->nranks; ++p) {
            const void* from = shim_group_slot(c->group, p)[kSlotSend];
            char* to = (char*)recv + esz * count * p;
            if (to == (const char*)from) continue;                                       // the in-place form: the own block stays
            if (count) SHIM_HIP(c, hipMemcpyAsync(to, from, esz * count, hipMemcpyDeviceToDevice, st));
        }
    }
    SHIM_HIP(c, hipEventRecord((hipEvent_t)mine[kSlotRead], st));                        // 4
    SHIM_BARRIER(c, reduce ? 3u : 1u);                                                   // 5
    for (int p = 0; p < c->nranks; ++p)
        if (p != c->rank) SHIM_HIP(c, hipStreamWaitEvent(st, (hipEvent_t)shim_group_slot(c->group, p)[kSlotRead], 0));
    return ncclSuccess;
}

std::atomic<uint64_t> g_ids{0};

}  // namespace

extern "C" {

ncclResult_t ncclGetVersion(int* version)
{
    if (!version) return ncclInvalidArgument;
    *version = NB_SHIM_VERSION;
    return ncclSuccess;
}

ncclResult_t ncclGetUniqueId(ncclUniqueId* id)
{
    if (!id) return ncclInvalidArgument;
    memset(id, 0, sizeof *id);
    const uint64_t words[3] = {0x6e622d7368696d21ull, (uint64_t)getpid(), ++g_ids};      // never all zero, never twice in a process
    memcpy(id->internal, words, sizeof words);
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank)
{
    if (!comm) return ncclInvalidArgument;
    *comm = nullptr;
    if (nranks < 1 || nranks > SHIM_MAX_RANKS || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    ncclComm* c = new (std::nothrow) ncclComm;
    if (!c) return ncclSystemError;
    c->nranks = nranks; c->rank = rank;
    if (const char* late = getenv("NB_SHIM_LATE_US")) c->late_us = atol(late);
    hipEvent_t written = nullptr, read = nullptr;
    if (hipEventCreateWithFlags(&written, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&read, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (written) (void)hipEventDestroy(written);
        delete c;
        return ncclUnhandledCudaError;
    }
    static_assert(sizeof id.internal == SHIM_ID_BYTES, "the group key is the whole id");
    if (shim_group_join((const unsigned char*)id.internal, nranks, rank, &c->group) != SHIM_OK) {
        (void)hipEventDestroy(written); (void)hipEventDestroy(read);
        delete c;
        return ncclInternalError;
    }
    // the events belong to the group, not to the rank: a peer may still enqueue a wait for them after this rank has gone
    void** mine = shim_group_slot(c->group, rank);
    mine[kSlotWritten] = written; mine[kSlotRead] = read;
    shim_group_on_free(c->group, free_events);
    *comm = c;
    return ncclSuccess;
}

// nb_multi's RCCL mode wants one device per shard: not what this library is for
ncclResult_t ncclCommInitAll(ncclComm_t*, int, const int*) { return ncclInvalidUsage; }
ncclResult_t ncclGroupStart() { return ncclInvalidUsage; }
ncclResult_t ncclGroupEnd() { return ncclInvalidUsage; }

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    if (!comm) return ncclSuccess;
    if (comm->group) shim_group_leave(comm->group, comm->rank);      // never waits for the peers
    delete comm;
    return ncclSuccess;
}

ncclResult_t ncclCommCount(const ncclComm_t comm, int* count)
{
    if (!comm || !count) return ncclInvalidArgument;
    *count = comm->nranks;
    return ncclSuccess;
}

ncclResult_t ncclCommUserRank(const ncclComm_t comm, int* rank)
{
    if (!comm || !rank) return ncclInvalidArgument;
    *rank = comm->rank;
    return ncclSuccess;
}

ncclResult_t ncclAllGather(const void* send, void* recv, size_t count, ncclDataType_t type, ncclComm_t comm, hipStream_t st)
{
    return collective(false, send, recv, count, type, comm, st);
}

ncclResult_t ncclReduceScatter(const void* send, void* recv, size_t count, ncclDataType_t type, ncclRedOp_t op, ncclComm_t comm, hipStream_t st)
{
    if (op != ncclSum) return ncclInvalidArgument;
    return collective(true, send, recv, count, type, comm, st);
}

const char* ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "shim: unhandled HIP error";
    case ncclSystemError: return "shim: system error";
    case ncclInternalError: return "shim: the group aborted (a HIP error, a barrier that timed out, ranks out of step, or a rank that left)";
    case ncclInvalidArgument: return "shim: invalid argument";
    case ncclInvalidUsage: return "shim: not supported by the stand-in library";
    default: return "shim: unknown result code";
    }
}

// for the test driver: one of its rank threads has died, nobody may wait for it
void nb_shim_abort_all(void) { shim_abort_all(); }

}  // extern "C"
