// tnml_comm.hip -- collectives: the front end of the three transports (RCCL, the in-process communicator, the cross-process
// one-shot exchange), the carried slots of a finished bond update, and the replica check.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- RCCL -----------------------------------------------------------------------------------
int tnml_comm_unique_id(void* id128) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return tnml_fail(nullptr, "ncclGetUniqueId failed");
    memcpy(id128, &id, sizeof id);
    return 0;
}
int tnml_comm_init(tnml_ctx* c, const void* id128) {
    // a single rank needs no communicator; TNML_FORCE_COMM=1 builds a 1-rank one anyway so that the RCCL path
    // (communicator setup, stream-ordered all-reduce) can be exercised on a one-GPU box
    if (c->cfg.nranks == 1 && !(getenv("TNML_FORCE_COMM") && atoi(getenv("TNML_FORCE_COMM")))) return 0;
    ncclUniqueId id; memcpy(&id, id128, sizeof id);
    HIPCK(c, hipSetDevice(c->cfg.device));
    ncclResult_t r = ncclCommInitRank(&c->comm, c->cfg.nranks, id, c->cfg.rank);
    if (r != ncclSuccess) return tnml_fail(c, "ncclCommInitRank failed: %s", ncclGetErrorString(r));
    return 0;
}
// sum over ranks of a fp64 device buffer, in stream order (replaces stdx::accumulate, fixedL.cc:385,402,421,427)
int allreduce(tnml_ctx* c, double* buf, size_t count) {
    if (c->ipc) { ProfScope ps(c, KC_ALLREDUCE); c->allreduce_calls += 1; return ipc_comm_exchange(c, buf, count, 0); }
    if (c->local) { ProfScope ps(c, KC_ALLREDUCE); c->allreduce_calls += 1; return local_comm_exchange(c, buf, count, 0); }
    if (!c->comm) {
        if (c->cfg.nranks == 1) return 0;
        return tnml_fail(c, "nranks > 1 but tnml_comm_init was not called");
    }
    ProfScope ps(c, KC_ALLREDUCE);
    c->allreduce_calls += 1;
    ncclResult_t r = ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) return tnml_fail(c, "ncclAllReduce failed: %s", ncclGetErrorString(r));
    return 0;
}
int allreduce_sum(tnml_ctx* c, double* buf, size_t count) { return allreduce(c, buf, count); }
// the carried slots of a finished bond update (after-SVD cost partials, fingerprint pieces) have just been summed over the ranks by an
// all-reduce that covered them: hand them to the host report they belong to
int carry_deliver(tnml_ctx* c) {
    if (c->carry_slot < 0) return 0;
    const int slot = c->carry_slot;
    c->carry_slot = -1;
    if (!c->pend[slot].carry_direct)      // (one rank: k_reduce_partials has mirrored the cost partials into the report block itself)
        HIPCK(c, hipMemcpyAsync(pend_host(c, slot) + TNML_CARRY, c->tail + TNML_CARRY, sizeof(double) * TNML_CARRYN, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipEventRecord(c->pend[slot].ev2, c->stream));
    if (c->multi())                                        // delivered: the next packed all-reduce must not sum (and so scale by nranks) what is left here
        HIPCK(c, hipMemsetAsync(c->tail + TNML_CARRY, 0, sizeof(double) * TNML_CARRYN, c->stream));
    return 0;
}
// the packed buffer [tail | G] of the current bond (n = elements of G)
int allreduce_packed(tnml_ctx* c, size_t n) {
    TCK(allreduce(c, c->arbuf, TNML_TAILN + n));
    return carry_deliver(c);
}
int bcast_rank0(tnml_ctx* c, double* buf, size_t count) {
    if (c->ipc) { c->bcast_calls += 1; return ipc_comm_exchange(c, buf, count, 1); }
    if (c->local) { c->bcast_calls += 1; return local_comm_exchange(c, buf, count, 1); }
    if (!c->comm) return 0;
    c->bcast_calls += 1;
    ncclResult_t r = ncclBroadcast(buf, buf, count, ncclDouble, 0, c->comm, c->stream);
    if (r != ncclSuccess) return tnml_fail(c, "ncclBroadcast failed: %s", ncclGetErrorString(r));
    return 0;
}
int tnml_collective_mode(tnml_ctx* c) { return c->ipc ? 4 : (c->local ? local_comm_mode(c) : (c->comm ? 1 : 0)); }
int tnml_collective_stats(tnml_ctx* c, int64_t* allreduces, int64_t* broadcasts) {
    if (allreduces) *allreduces = c->allreduce_calls;
    if (broadcasts) *broadcasts = c->bcast_calls;
    return 0;
}
// fingerprint of the replicated site tensors j0..j1 as exact integer pieces -> out8 (device; see k_fingerprint_pieces)
int replica_fingerprint(tnml_ctx* c, int j0, int j1, double* out8) {
    for (int j = j0; j <= j1; ++j) {
        const SiteT& s = c->W[j];
        TCK(launch_fingerprint(c, s.a, (size_t)s.ml * 2 * s.mr * s.L, 0x9E3779B97F4A7C15ull * (unsigned long long)(2 * j + 1), c->fprint, j == j0));
    }
    return launch_fingerprint_pieces(c, c->fprint, out8);
}
// sums S_i, Q_i of the fingerprint pieces over R ranks: every rank held the same fingerprint iff R Q_i == S_i^2 for all four pieces
bool fingerprint_agrees(const double* sums8, int nranks) {
    for (int i = 0; i < 4; ++i) if ((double)nranks * sums8[4 + i] != sums8[i] * sums8[i]) return false;
    return true;
}
int tnml_replica_check(tnml_ctx* c, int* nranks_in_comm) {
    CollScope coll_(c);
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (nranks_in_comm) *nranks_in_comm = 1;
    if (!c->multi()) return c->cfg.nranks == 1 ? 0 : tnml_fail(c, "tnml_replica_check: nranks > 1 but tnml_comm_init was not called");
    int cnt = 0;
    if (c->local) cnt = local_comm_size(c);
    else if (c->ipc) cnt = c->cfg.nranks;
    else if (ncclCommCount(c->comm, &cnt) != ncclSuccess) return tnml_fail(c, "ncclCommCount failed");
    if (nranks_in_comm) *nranks_in_comm = cnt;
    if (cnt != c->cfg.nranks) return tnml_fail(c, "communicator has %d ranks, context was created for %d", cnt, c->cfg.nranks);
    TCK(check_W(c));
    if (c->pend_count) return tnml_fail(c, "tnml_replica_check: a bond update is in flight");
    TCK(replica_fingerprint(c, 1, c->N, c->tail + TNML_FPSLOT));
    TCK(allreduce(c, c->tail + TNML_FPSLOT, 8));
    double h[8];
    HIPCK(c, hipMemcpyAsync(h, c->tail + TNML_FPSLOT, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    if (!fingerprint_agrees(h, c->cfg.nranks)) return tnml_fail(c, "replicas of the weight MPS differ between ranks");
    return 0;
}
