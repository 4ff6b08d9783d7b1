// gather.cpp — mte_gather_summaries of include/mte.h, and the only unit that sees RCCL.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mte.h"
#include "engine_host.hpp"
#include "gather_plan.hpp"

// ------------------------------------------------------------------------------------------------
// The one collective of the path: an all-gather of the per-document summary records over
// RCCL (xGMI on one node). librccl is opened on first use, so hosts that never gather (one GPU, the
// CPU tests) do not need it.
namespace {
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclAllGather) allGather = nullptr;
    decltype(&ncclGetErrorString) errStr = nullptr;
    bool ok() {
        if (h) return true;
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) return false;
        getUniqueId = (decltype(getUniqueId))dlsym(h, "ncclGetUniqueId");
        commInitRank = (decltype(commInitRank))dlsym(h, "ncclCommInitRank");
        commDestroy = (decltype(commDestroy))dlsym(h, "ncclCommDestroy");
        allGather = (decltype(allGather))dlsym(h, "ncclAllGather");
        errStr = (decltype(errStr))dlsym(h, "ncclGetErrorString");
        if (!getUniqueId || !commInitRank || !commDestroy || !allGather || !errStr) {
            dlclose(h);
            h = nullptr;
        }
        return h != nullptr;
    }
};
Rccl& rccl() {
    static Rccl r;
    return r;
}
std::mutex& rccl_mu() {
    static std::mutex m;
    return m;
}
}  // namespace
static_assert(sizeof(ncclUniqueId) == MTE_RCCL_ID_BYTES, "ncclUniqueId size");

int mte_rccl_unique_id(uint8_t* id) {
    if (!id) return MTE_E_ARG;
    std::lock_guard<std::mutex> g(rccl_mu());
    if (!rccl().ok()) return MTE_E_UNSUPPORTED;
    ncclUniqueId u;
    if (rccl().getUniqueId(&u) != ncclSuccess) return MTE_E_HIP;
    memcpy(id, &u, sizeof u);
    return MTE_OK;
}

int mte_rccl_comm_create(mte_engine* e, const uint8_t* id, int rank, int world, void** comm) {
    if (!e || !id || !comm || world < 1 || rank < 0 || rank >= world) return MTE_E_ARG;
    *comm = nullptr;
    {
        std::lock_guard<std::mutex> g(rccl_mu());
        if (!rccl().ok()) return set_err(e, MTE_E_UNSUPPORTED, "librccl not available");
    }
    HIP_TRY(e, hipSetDevice(e->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t c = nullptr;
    ncclResult_t r = rccl().commInitRank(&c, world, u, rank);
    if (r != ncclSuccess) return set_err(e, MTE_E_HIP, std::string("ncclCommInitRank: ") + rccl().errStr(r));
    *comm = (void*)c;
    return MTE_OK;
}

void mte_rccl_comm_destroy(void* comm) {
    if (comm && rccl().ok()) rccl().commDestroy((ncclComm_t)comm);
}

// The gather itself: every rank's records into `res` (rank order). One count all-gather and one
// record all-gather; the caller sizes nothing beforehand.
static int gather_all(mte_engine* e, int rank, int world, void* comm, std::vector<mte_doc_summary>& res) {
    if (!e || world < 1 || rank < 0 || rank >= world || (world > 1 && !comm)) return MTE_E_ARG;
    const size_t nd = e->P.n_docs;
    std::vector<mte_doc_summary> mine(nd);
    int rc = nd ? mte_summaries(e, mine.data(), nd) : MTE_OK;
    if (rc) return rc;
    if (world == 1) {
        res.swap(mine);
        return MTE_OK;
    }
    HIP_TRY(e, hipSetDevice(e->device));
    ncclComm_t c = (ncclComm_t)comm;
    // 1) every rank's record count, 2) the records padded to the largest count
    DevBuf<uint64_t> cnt, all_cnt;
    HIP_TRY(e, cnt.alloc(1));
    HIP_TRY(e, all_cnt.alloc((size_t)world));
    const uint64_t mine_n = nd;
    HIP_TRY(e, hipMemcpyAsync(cnt.p, &mine_n, 8, hipMemcpyHostToDevice, e->stream));
    ncclResult_t r = rccl().allGather(cnt.p, all_cnt.p, 1, ncclUint64, c, e->stream);
    if (r != ncclSuccess) return set_err(e, MTE_E_HIP, std::string("ncclAllGather: ") + rccl().errStr(r));
    std::vector<uint64_t> counts((size_t)world);
    HIP_TRY(e, hipMemcpyAsync(counts.data(), all_cnt.p, 8 * (size_t)world, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    const GatherPlan g = gather_plan(counts.data(), world);
    const size_t words = sizeof(mte_doc_summary) / 8;  // 32-B records as 4 u64 words
    std::vector<mte_doc_summary> blk(g.stride), flat(g.stride * (size_t)world);
    gather_pack(mine.data(), nd, g, blk.data());
    DevBuf<uint64_t> send, recv;
    HIP_TRY(e, send.alloc(g.stride * words));
    HIP_TRY(e, recv.alloc(g.stride * words * (size_t)world));
    HIP_TRY(e, hipMemcpyAsync(send.p, blk.data(), g.stride * sizeof(mte_doc_summary), hipMemcpyHostToDevice, e->stream));
    r = rccl().allGather(send.p, recv.p, g.stride * words, ncclUint64, c, e->stream);
    if (r != ncclSuccess) return set_err(e, MTE_E_HIP, std::string("ncclAllGather: ") + rccl().errStr(r));
    HIP_TRY(e, hipMemcpyAsync(flat.data(), recv.p, flat.size() * sizeof(mte_doc_summary), hipMemcpyDeviceToHost,
                              e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    res.resize(g.total);
    gather_concat(flat.data(), counts.data(), world, g, res.data());
    return MTE_OK;
}

int mte_gather_summaries(mte_engine* e, int rank, int world, void* comm, mte_doc_summary* out, size_t cap,
                         size_t* n) {
    if (!e || world < 1 || rank < 0 || rank >= world || (world > 1 && !comm)) return MTE_E_ARG;
    if (!out && world == 1) {  // size query on one rank: no collective
        if (n) *n = e->P.n_docs;
        return MTE_OK;
    }
    // (with world > 1 a size query runs the full record all-gather, like the call that follows it:
    // mte_gather_summaries_alloc does both in one collective)
    std::vector<mte_doc_summary> res;
    if (int rc = gather_all(e, rank, world, comm, res)) return rc;
    if (n) *n = res.size();
    if (!out) return MTE_OK;
    if (cap < res.size()) return MTE_E_RANGE;
    std::copy(res.begin(), res.end(), out);
    return MTE_OK;
}

int mte_gather_summaries_alloc(mte_engine* e, int rank, int world, void* comm, mte_doc_summary** out, size_t* n) {
    if (!out || !n) return MTE_E_ARG;
    *out = nullptr;
    *n = 0;
    std::vector<mte_doc_summary> res;
    if (int rc = gather_all(e, rank, world, comm, res)) return rc;
    void* p = malloc(res.empty() ? 1 : res.size() * sizeof(mte_doc_summary));
    if (!p) return set_err(e, MTE_E_NOMEM, "gather buffer");
    if (!res.empty()) memcpy(p, res.data(), res.size() * sizeof(mte_doc_summary));
    *out = (mte_doc_summary*)p;
    *n = res.size();
    return MTE_OK;
}

void mte_free(void* p) { free(p); }
