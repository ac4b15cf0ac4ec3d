// spl_collective.h -- the RCCL side: NCCL_TRY, comm_create and the ragged all-gather of CSR results (allgatherv_csr).  Needs spl_comm
// (spl_ctx.h), the RCCL binding (spl_comm.h) and the kernels k_csr_counts / k_rebase_offsets.
#pragma once
namespace {

#define NCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return fail(SPL_EDEVICE, std::string(#expr) + ": " + rccl().GetErrorString(r_));       \
    } while (0)

int comm_create(const uint8_t* id, int rank, int world, int device, spl_comm** out) {
    Rccl& R = rccl();
    if (!R.lib) return fail(SPL_EDEVICE, "spl_comm_create: " + R.err);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<spl_comm> c(new spl_comm());
    c->rank = rank; c->world = world; c->device = device;
    ncclUniqueId uid;
    static_assert(sizeof uid.internal == SPL_COMM_ID_BYTES, "SPL_COMM_ID_BYTES must be RCCL's NCCL_UNIQUE_ID_BYTES");
    memcpy(uid.internal, id, SPL_COMM_ID_BYTES);
    NCCL_TRY(R.CommInitRank(&c->comm, world, uid, rank));
    SPL_TRY(c->d_cnt.alloc(4));
    SPL_TRY(c->d_cnts.alloc(4 * (size_t)world));
    SPL_TRY(c->h_cnts.alloc(4 * (size_t)world));
    *out = c.release();
    return SPL_OK;
}

// The device side of the exact form: every rank's {T, N} (host memory, `stride` u64 words per rank, T and N first) -> the prefix table, and
// the launch that turns the received LOCAL offsets into offsets of the global id array (+ the closing entry).  allgatherv_csr and the test
// seam spl_debug_rebase_offsets both come through here, each with 1 <= W <= COMM_MAX_WORLD (spl_comm_create / the seam refuse anything else).
RankTable rank_table(const uint64_t* counts, size_t stride, uint32_t W) {
    RankTable tab{};
    for (uint32_t p = 0; p < W; p++) {
        tab.t_pre[p + 1] = tab.t_pre[p] + counts[stride * p];
        tab.n_pre[p + 1] = tab.n_pre[p] + counts[stride * p + 1];
    }
    return tab;
}
int rebase_offsets(uint64_t* d_all_off, const uint64_t* counts, size_t stride, uint32_t W, hipStream_t s) {
    const RankTable tab = rank_table(counts, stride, W);
    uint64_t nmax = 1;
    for (uint32_t p = 0; p < W; p++) nmax = std::max<uint64_t>(nmax, counts[stride * p + 1]);
    hipLaunchKernelGGL(k_rebase_offsets, dim3((uint32_t)std::min<uint64_t>((nmax + 255) / 256, 1024), W), dim3(256), 0, s, d_all_off, tab, W);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int allgatherv_csr(spl_comm* c, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, uint32_t* d_all_ids,
                   uint64_t all_ids_cap, uint64_t* d_all_off, uint64_t all_off_cap, uint64_t* n_tokens_total, uint64_t* n_docs_total,
                   hipStream_t s) {
    Rccl& R = rccl();
    HIP_TRY(hipSetDevice(c->device));
    const int W = c->world;
    // (1) every rank's {T, N} and the capacities of ITS result buffers: 32 bytes per rank, then the one host
    // synchronisation of the exchange
    hipLaunchKernelGGL(k_csr_counts, dim3(1), dim3(64), 0, s, d_out_off, n_docs, all_ids_cap, all_off_cap, c->d_cnt.get());
    NCCL_TRY(R.AllGather(c->d_cnt.get(), c->d_cnts.get(), 4, ncclUint64, c->comm, s));
    HIP_TRY(hipMemcpyAsync(c->h_cnts.host(), c->d_cnts.get(), 32 * (size_t)W, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const RankTable tab = rank_table(c->h_cnts.host(), 4, (uint32_t)W);
    uint64_t min_ids_cap = ~0ull, min_off_cap = ~0ull;
    for (int p = 0; p < W; p++) {
        min_ids_cap = std::min(min_ids_cap, c->h_cnts.host()[4 * p + 2]);
        min_off_cap = std::min(min_off_cap, c->h_cnts.host()[4 * p + 3]);
    }
    if (n_tokens_total) *n_tokens_total = tab.t_pre[W];
    if (n_docs_total) *n_docs_total = tab.n_pre[W];
    // Every rank sees the same totals AND the same (smallest) capacities, so every rank takes the same branch even when
    // the ranks passed buffers of different sizes: nobody is left waiting in a collective its peer never entered.
    if (tab.t_pre[W] > min_ids_cap || tab.n_pre[W] + 1 > min_off_cap)
        return fail(SPL_ECAPACITY, "spl_allgatherv_csr: the global CSR does not fit the smallest buffers any rank gave (" +
                                   std::to_string(tab.t_pre[W]) + " tokens, " + std::to_string(tab.n_pre[W]) + " documents; capacities " +
                                   std::to_string(min_ids_cap) + " ids, " + std::to_string(min_off_cap) + " offsets)");
    // (2) exactly T_r ids and N_r offsets from every rank, each straight to its place: one message per peer and
    // direction, all links busy at once (xGMI is point to point; no ring, no padding)
    const uint64_t T = c->h_cnts.host()[4 * c->rank], N = c->h_cnts.host()[4 * c->rank + 1];
    NCCL_TRY(R.GroupStart());
    for (int p = 0; p < W; p++) {
        if (T) NCCL_TRY(R.Send(d_ids, T, ncclUint32, p, c->comm, s));
        if (N) NCCL_TRY(R.Send(d_out_off, N, ncclUint64, p, c->comm, s));
        const uint64_t Tp = c->h_cnts.host()[4 * p], Np = c->h_cnts.host()[4 * p + 1];
        if (Tp) NCCL_TRY(R.Recv(d_all_ids + tab.t_pre[p], Tp, ncclUint32, p, c->comm, s));
        if (Np) NCCL_TRY(R.Recv(d_all_off + tab.n_pre[p], Np, ncclUint64, p, c->comm, s));
    }
    NCCL_TRY(R.GroupEnd());
    // (3) local offsets -> offsets in the global id array, and the closing entry
    return rebase_offsets(d_all_off, c->h_cnts.host(), 4, (uint32_t)W, s);
}
}  // namespace
