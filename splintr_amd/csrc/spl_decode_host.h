// spl_decode_host.h -- spl_decode_batch's host side: the decode scratch and the two launch pairs both paths share, a large batch as a
// pipeline of chunks (decode_pipelined), and spl_decode_batch_impl.  Needs Ctx and upload_decode (spl_ctx.h), pick_stream_beside (spl_streams.h).
#pragma once
namespace {

// ---- decode of a LARGE batch as a pipeline -------------------------------------------------------------------------------------
// In one piece (below) a 12.5 M-token batch is 0.9 ms of H2D, 0.3 ms of kernels and 0.75 ms of D2H one after the other.  Here the batch goes
// in chunks of whole documents through two slots of scratch: the ids of chunk k + 1 travel in and are measured (k_decode_len / k_decode_scan on
// the compute stream) while chunk k's bytes are gathered (k_decode_copy / k_decode_docs on a second compute stream, picked to run beside the
// first) and travel out.  The host learns a chunk's byte count from pinned memory, knows where its bytes go in the ONE result, and launches
// its second half; document offsets leave the device already rebased.
struct DecOut {
    std::shared_ptr<PinnedPool> pool; uint8_t* b = nullptr; uint64_t* o = nullptr; size_t bcap = 0, ocap = 0;
    ~DecOut() { if (b) pool->put(b, bcap); if (o) pool->put(o, ocap); }
};
// A slot's scratch for n_ids ids in n_docs documents.  Grows, never shrinks: a steady stream of calls allocates nothing.
int dec_reserve(Ctx::DecSlot& ds, uint64_t n_ids, uint64_t n_docs) {
    if (n_ids > ds.cap_ids || !ds.ids) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t cap = n_ids + n_ids / 4 + 4096;
        ds.cap_ids = 0;
        SPL_TRY(ds.ids.alloc(cap)); SPL_TRY(ds.blk.alloc(cap / DEC_BLK + 4)); SPL_TRY(ds.idoff.alloc(cap + 1));
        ds.cap_ids = cap;
    }
    if (n_docs + 1 > ds.cap_docs || !ds.first) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t cap = n_docs + 1 + n_docs / 4 + 1024;
        ds.cap_docs = 0;
        SPL_TRY(ds.first.alloc(cap)); SPL_TRY(ds.docoff.alloc(cap));
        ds.cap_docs = cap;
    }
    return SPL_OK;
}
// The kernels' arguments for n_ids ids in n_docs documents that lie in the slot (a.out: the slot's, as it is now)
DecodeArgs dec_args(const Ctx* c, const Ctx::DecSlot& ds, uint64_t n_ids, uint64_t n_docs) {
    DecodeArgs a{};
    a.ids = ds.ids.get(); a.n_ids = n_ids; a.tok_off = c->d_tok_off.get(); a.tok_bytes = c->d_tok_bytes.get(); a.max_id = c->dec_max_id;
    a.sp_ids = c->d_dec_sp_ids.get(); a.sp_off = c->d_dec_sp_off.get(); a.n_sp = c->dec_n_sp;
    a.blk = ds.blk.get(); a.id_off = ds.idoff.get(); a.doc_first = ds.first.get(); a.n_docs = n_docs; a.doc_off = ds.docoff.get(); a.out = ds.out.get();
    return a;
}
// First half: every id's length, summed per block and scanned -- the output's byte count ends up behind the blocks' sums (a.blk[n_blk])
uint64_t dec_launch_len(const DecodeArgs& a, hipStream_t s) {
    const uint64_t n_blk = (a.n_ids + DEC_BLK - 1) / DEC_BLK;
    if (n_blk) hipLaunchKernelGGL(k_decode_len, dim3((uint32_t)n_blk), dim3(NT), 0, s, a);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, s, a.blk, n_blk);
    return n_blk;
}
// Second half: the bytes gathered into a.out, the documents' offsets (+ a.out_base) into a.doc_off
int dec_launch_copy(const DecodeArgs& a, hipStream_t s) {
    const uint64_t n_blk = (a.n_ids + DEC_BLK - 1) / DEC_BLK;
    if (n_blk) hipLaunchKernelGGL(k_decode_copy, dim3((uint32_t)n_blk), dim3(NT), 0, s, a);
    else HIP_TRY(hipMemsetAsync(a.id_off, 0, 8, s));              // (a chunk of empty documents: id_off[0] = 0)
    hipLaunchKernelGGL(k_decode_docs, dim3((uint32_t)((a.n_docs + 1 + 255) / 256)), dim3(256), 0, s, a);
    return SPL_OK;
}

int decode_pipelined(spl_tokenizer* t, Ctx* c, const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs, DecOut& o) {
    struct DC { uint64_t d0, d1; };
    std::vector<DC> ch;
    uint64_t max_ids = 0, max_docs = 0;
    for (uint64_t d = 0; d < n_docs;) {
        uint64_t e = d + 1;
        while (e < n_docs && ids_off[e + 1] - ids_off[d] <= t->dec_chunk_ids) e++;
        ch.push_back(DC{d, e});
        max_ids = std::max(max_ids, ids_off[e] - ids_off[d]);
        max_docs = std::max(max_docs, e - d);
        d = e;
    }
    const uint64_t n = ids_off[n_docs] - ids_off[0];
    int rc;
    if (!c->s_dec2) {
        HIP_TRY(hipDeviceSynchronize());
        double cf = 0;
        hipStream_t picked = nullptr;
        if (t->pick_streams) { if ((rc = pick_stream_beside({c->s_cmp.get(), c->s_d2h.get(), c->s_h2d.get()}, &picked, &cf))) return rc; c->s_dec2.reset(picked); }
        else SPL_TRY(c->s_dec2.create());
    }
    for (auto& ds : c->dslot) {
        if (!ds.ev_in) for (Event* e : {&ds.ev_in, &ds.ev_len, &ds.ev_cp, &ds.ev_out}) SPL_TRY(e->create());
        SPL_TRY(dec_reserve(ds, max_ids, max_docs));
    }
    if (!c->h_dtot.ensure(t->pool, ch.size() * 8)) return fail(SPL_EDEVICE, "spl_decode_batch: pinned allocation failed");
    uint64_t* const h_tot = (uint64_t*)c->h_dtot.p;
    // the result: a first guess of its size (5 bytes per token), moved to a larger buffer if a chunk does not fit
    o.b = (uint8_t*)t->pool->get(n * 5 + 4096, o.bcap);
    if (!o.b) return fail(SPL_EDEVICE, "spl_decode_batch: pinned allocation failed");
    auto args_of = [&](size_t k) { return dec_args(c, c->dslot[k & 1], ids_off[ch[k].d1] - ids_off[ch[k].d0], ch[k].d1 - ch[k].d0); };
    auto submit_len = [&](size_t k) -> int {                  // ids in, lengths, the chunk's byte count to pinned memory
        const DC& q = ch[k];
        Ctx::DecSlot& ds = c->dslot[k & 1];
        if (k >= 2) { HIP_TRY(hipStreamWaitEvent(c->s_h2d.get(), ds.ev_cp.get(), 0)); HIP_TRY(hipStreamWaitEvent(c->s_cmp.get(), ds.ev_cp.get(), 0)); }   // the slot's previous chunk has been gathered
        const DecodeArgs a = args_of(k);
        if (a.n_ids) HIP_TRY(hipMemcpyAsync(ds.ids.get(), ids + ids_off[q.d0], a.n_ids * 4, hipMemcpyHostToDevice, c->s_h2d.get()));
        HIP_TRY(hipMemcpyAsync(ds.first.get(), ids_off + q.d0, (a.n_docs + 1) * 8, hipMemcpyHostToDevice, c->s_h2d.get()));
        HIP_TRY(hipEventRecord(ds.ev_in.get(), c->s_h2d.get()));
        HIP_TRY(hipStreamWaitEvent(c->s_cmp.get(), ds.ev_in.get(), 0));
        const uint64_t n_blk = dec_launch_len(a, c->s_cmp.get());
        HIP_TRY(hipMemcpyAsync(&h_tot[k], ds.blk.get() + n_blk, 8, hipMemcpyDeviceToHost, c->s_cmp.get()));
        HIP_TRY(hipEventRecord(ds.ev_len.get(), c->s_cmp.get()));
        return SPL_OK;
    };
    uint64_t base = 0;
    auto finish = [&](size_t k) -> int {                      // bytes gathered, rebased offsets, both on their way into the result
        const DC& q = ch[k];
        Ctx::DecSlot& ds = c->dslot[k & 1];
        HIP_TRY(hipEventSynchronize(ds.ev_len.get()));
        const uint64_t total = h_tot[k];
        if (total + 16 > ds.cap_out) {                        // (grow-only; the slot's previous bytes have left: its event first)
            if (k >= 2) HIP_TRY(hipEventSynchronize(ds.ev_out.get()));
            SPL_TRY(ds.out.grow(&ds.cap_out, total + 16, total + total / 4 + 4096));
        }
        if (base + total > o.bcap) {                          // the guess was too small: what is still to come is at most 128 bytes per token
            HIP_TRY(hipStreamSynchronize(c->s_d2h.get()));
            const uint64_t rest_ids = ids_off[n_docs] - ids_off[q.d1];
            size_t ncap = 0;
            uint8_t* nb = (uint8_t*)t->pool->get(base + total + rest_ids * 8 + 4096, ncap);
            if (!nb) return fail(SPL_EDEVICE, "spl_decode_batch: pinned allocation failed");
            memcpy(nb, o.b, base);
            t->pool->put(o.b, o.bcap);
            o.b = nb; o.bcap = ncap;
        }
        DecodeArgs a = args_of(k);
        a.out_base = base;
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(c->s_dec2.get(), ds.ev_out.get(), 0));     // the slot's previous bytes and offsets have left
        HIP_TRY(hipStreamWaitEvent(c->s_dec2.get(), ds.ev_len.get(), 0));
        SPL_TRY(dec_launch_copy(a, c->s_dec2.get()));
        HIP_TRY(hipEventRecord(ds.ev_cp.get(), c->s_dec2.get()));
        HIP_TRY(hipStreamWaitEvent(c->s_d2h.get(), ds.ev_cp.get(), 0));
        if (total) HIP_TRY(hipMemcpyAsync(o.b + base, ds.out.get(), total, hipMemcpyDeviceToHost, c->s_d2h.get()));
        const bool last = k + 1 == ch.size();
        HIP_TRY(hipMemcpyAsync(o.o + q.d0, ds.docoff.get(), (a.n_docs + (last ? 1 : 0)) * 8, hipMemcpyDeviceToHost, c->s_d2h.get()));
        HIP_TRY(hipEventRecord(ds.ev_out.get(), c->s_d2h.get()));
        base += total;
        return SPL_OK;
    };
    if ((rc = submit_len(0))) return rc;
    for (size_t k = 1; k < ch.size(); k++) {
        if ((rc = submit_len(k))) return rc;
        if ((rc = finish(k - 1))) return rc;
    }
    if ((rc = finish(ch.size() - 1))) return rc;
    HIP_TRY(hipStreamSynchronize(c->s_d2h.get()));
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int spl_decode_batch_impl(spl_tokenizer* t, const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs, uint8_t** out_bytes,
                     uint64_t** out_off) {
    if (!t || !ids_off || !out_bytes || !out_off) return fail(SPL_EINVAL, "spl_decode_batch: null argument");
    for (uint64_t d = 0; d < n_docs; d++)
        if (ids_off[d + 1] < ids_off[d]) return fail(SPL_EINVAL, "spl_decode_batch: ids_off must be non-decreasing");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_streams(*c);
    if (rc) return rc;
    if ((rc = upload_decode(t, c))) return rc;
    const uint64_t n = ids_off[n_docs] - ids_off[0];
    if (n && !ids) return fail(SPL_EINVAL, "spl_decode_batch: null ids");
    // outputs in pinned memory from the handle's pool (the D2H copies run at PCIe speed into it; pageable
    // memory would be staged by the runtime page by page); returned to the pool on every error path
    DecOut o;
    o.pool = t->pool;
    o.o = (uint64_t*)t->pool->get((n_docs + 1) * 8, o.ocap);
    if (!o.o) return fail(SPL_EDEVICE, "spl_decode_batch: pinned allocation failed");
    uint64_t total = 0;
    if (n >= 3 * t->dec_chunk_ids && n_docs >= 3) {
        if ((rc = decode_pipelined(t, c, ids, ids_off, n_docs, o))) return rc;
    } else if (n) {
        Ctx::DecSlot& ds = c->dec;
        SPL_TRY(dec_reserve(ds, n, n_docs));
        HIP_TRY(hipMemcpyAsync(ds.ids.get(), ids + ids_off[0], n * 4, hipMemcpyHostToDevice, c->s_cmp.get()));
        HIP_TRY(hipMemcpyAsync(ds.first.get(), ids_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->s_cmp.get()));
        DecodeArgs a = dec_args(c, ds, n, n_docs);
        const uint64_t n_blk = dec_launch_len(a, c->s_cmp.get());
        uint64_t* h_total = (uint64_t*)o.o;                       // (pinned: the count lands without a staging copy)
        HIP_TRY(hipMemcpyAsync(h_total, ds.blk.get() + n_blk, 8, hipMemcpyDeviceToHost, c->s_cmp.get()));
        HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));                  // the output size: the one host round trip
        total = *h_total;
        SPL_TRY(ds.out.grow(&ds.cap_out, total + 16, (total + 16) + (total + 16) / 4 + 1024));
        a.out = ds.out.get();
        SPL_TRY(dec_launch_copy(a, c->s_cmp.get()));
        HIP_TRY(hipGetLastError());
        o.b = (uint8_t*)t->pool->get(total ? total : 1, o.bcap);
        if (!o.b) return fail(SPL_EDEVICE, "spl_decode_batch: pinned allocation failed");
        if (total) HIP_TRY(hipMemcpyAsync(o.b, ds.out.get(), total, hipMemcpyDeviceToHost, c->s_cmp.get()));
        HIP_TRY(hipMemcpyAsync(o.o, ds.docoff.get(), (n_docs + 1) * 8, hipMemcpyDeviceToHost, c->s_cmp.get()));
        HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));
    } else {
        o.b = (uint8_t*)t->pool->get(1, o.bcap);
        if (!o.b) return fail(SPL_EDEVICE, "spl_decode_batch: pinned allocation failed");
        for (uint64_t d = 0; d <= n_docs; d++) o.o[d] = 0;
    }
    loose().add(o.b, t->pool, o.bcap);
    loose().add(o.o, t->pool, o.ocap);
    *out_bytes = o.b; *out_off = o.o;
    o.b = nullptr; o.o = nullptr;
    return SPL_OK;
}
}  // namespace
