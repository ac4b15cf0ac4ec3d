// spl_sp_host.h -- SentencePiece mode, host side (the kernels: spl_k_sp.h): the workspace (sp_reserve), one device call -- the special
// scan over the caller's text, count pass, scan, ONE synchronisation for the rewritten length, write pass, then launch_all on the
// rewritten text with its chunk starts as external boundaries -- and spl_encode_batch's host-to-host form.  Needs launch_all
// (spl_launch.h) and ensure_streams (spl_ctx.h).
#pragma once
namespace {

constexpr int KI_SP_COUNT = KI_N, KI_SP_WRITE = KI_N + 1;      // profile slots behind the encode path's (spl_kernel_name)
const char* const k_sp_names[2] = {"k_sp_rewrite<count>+k_decode_scan", "k_sp_rewrite<write>"};

// words of one bitmap of the literal scan over n bytes, as check_call lays them out (CallShape::uw)
size_t sp_scan_words(uint64_t n_bytes) { return (size_t)(n_bytes / RANK_BLK + 1) * 32 + 32; }

// The workspace of calls of up to max_bytes of text and max_docs documents: the encode path's own for three times the bytes, the
// rewritten text (16-byte groups), a count per tile, the rewritten offsets, two bitmaps over the rewritten text; for a handle with
// special tokens the literal scan's bitmaps and ids over the caller's text.
int sp_reserve(spl_tokenizer* tk, Ctx* c, uint64_t max_bytes, uint64_t max_docs) {
    SPL_TRY(reserve(c, 3 * max_bytes, max_docs));
    if (max_bytes > c->sp_cap_bytes || !c->d_sp_text) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t nb = std::max(max_bytes, c->sp_cap_bytes);
        c->sp_cap_bytes = 0;
        SPL_TRY(c->d_sp_text.alloc(3 * nb + 64));
        SPL_TRY(c->d_sp_cnt.alloc(nb / SPT_TB + 4));
        SPL_TRY(c->d_sp_bits.alloc(2 * (3 * nb / 32 + 4)));
        c->sp_cap_bytes = nb;
    }
    if (max_docs > c->sp_cap_docs || !c->d_sp_off) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t nd = std::max(max_docs, c->sp_cap_docs);
        c->sp_cap_docs = 0;
        SPL_TRY(c->d_sp_off.alloc(nd + 1));
        c->sp_cap_docs = nd;
    }
    if (!tk->specials.empty()) {
        const uint64_t need = 4 * sp_scan_words(c->sp_cap_bytes) + c->sp_cap_bytes + 64;
        SPL_TRY(c->d_sp_scan.grow(&c->sp_scan_cap, need, need));
    }
    return SPL_OK;
}

int encode_device_sp(spl_tokenizer* tk, Ctx* c, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                     uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_out_off, hipStream_t s, const SlabOut* so) {
    if (n_bytes > SP_MAX_BYTES) return fail(SPL_EINVAL, "SentencePiece mode: a device call takes at most 64 MiB of text (split the corpus at document boundaries -- spl_encode_batch does that by itself)");
    if (((uintptr_t)d_utf8 & 15) != 0) return fail(SPL_EINVAL, "text buffer must be 16-byte aligned");
    if (n_docs > 0xFFFFFFF0ull) return fail(SPL_EINVAL, "n_docs per device call must be < 2^32 - 16");
    if (n_bytes && !n_docs) return fail(SPL_EINVAL, "SentencePiece mode: text without a document");
    if (!n_bytes)                                             // (nothing to rewrite: the encode path's own empty call)
        return launch_all(tk, c, {.text = d_utf8, .n_bytes = 0, .doc_off = d_doc_off, .n_docs = n_docs, .flags = flags, .ids = d_ids,
                                  .ids_cap = ids_cap, .out_off = d_out_off, .stream = s, .slab = so});
    const bool special = (flags & SPL_WITH_SPECIAL) && !tk->specials.empty();
    SPL_TRY(sp_reserve(tk, c, n_bytes, n_docs));
    Event ev[3];
    if (c->prof) for (auto& e : ev) SPL_TRY(e.create(hipEventDefault));
    SpArgs a{};
    a.t.text = d_utf8; a.t.n_bytes = (uint32_t)n_bytes; a.t.doc_off = d_doc_off; a.t.n_docs = (uint32_t)n_docs;
    a.t.ucls1 = c->dt.ucls_stage1; a.t.ucls2 = c->dt.ucls_stage2; a.t.shift = c->dt.ucls_shift;
    if (special) {
        // the literals are found in the CALLER's text (a literal's bytes are never rewritten): the encode path's scan kernels over bitmaps of
        // this workspace, which the write pass moves to the rewritten positions
        SPL_TRY(upload_specials(tk, c));
        const size_t uw = sp_scan_words(n_bytes);
        uint32_t* const bm = c->d_sp_scan.get();
        HIP_TRY(hipMemsetAsync(bm, 0, 4 * uw * 4, s));
        Batch b{};
        b.text = d_utf8; b.n_bytes = (uint32_t)n_bytes; b.doc_off = d_doc_off; b.n_docs = (uint32_t)n_docs;
        b.tbits = bm; b.tstart = bm + uw; b.skip = bm + 2 * uw; b.spcand = tk->special_general ? bm + 3 * uw : nullptr;
        b.stage = bm + 4 * uw;
        b.sp_lits = c->d_sp_lits.get(); b.n_special = (uint32_t)tk->specials.size();
        hipLaunchKernelGGL(k_mark_docs, dim3((uint32_t)((n_docs + 255) / 256)), dim3(256), 0, s, b);
        if (!tk->special_general) hipLaunchKernelGGL(k_special_scan, dim3((uint32_t)((n_bytes + 255) / 256)), dim3(256), 0, s, b);
        else {
            hipLaunchKernelGGL(k_special_ends, dim3((uint32_t)((n_bytes + 255) / 256)), dim3(256), 0, s, b);
            hipLaunchKernelGGL(k_special_select, dim3((uint32_t)((n_docs + 255) / 256)), dim3(256), 0, s, b);
        }
        a.t.tbits = b.tbits; a.t.tstart = b.tstart; a.t.skip = b.skip; a.stage_in = b.stage;
    }
    const uint32_t ntiles = (uint32_t)((n_bytes + SPT_TB - 1) / SPT_TB);
    a.cnt = c->d_sp_cnt.get();
    if (c->prof) HIP_TRY(hipEventRecord(ev[0].get(), s));
    hipLaunchKernelGGL(k_sp_rewrite<false>, dim3(ntiles), dim3(SPT_NT), 0, s, a);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, s, a.cnt, (uint64_t)ntiles);
    if (c->prof) HIP_TRY(hipEventRecord(ev[1].get(), s));
    HIP_TRY(hipGetLastError());
    // the ONE synchronisation: the encode path takes the rewritten length from the host
    uint64_t conv = 0;
    HIP_TRY(hipMemcpyAsync(&conv, a.cnt + ntiles, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t n_out = n_bytes + 2 * conv;
    if (conv > n_bytes) return fail(SPL_EDEVICE, "SentencePiece mode: the count pass reports more spaces than bytes");
    const uint64_t bw = n_out / 32 + 4;
    a.out = c->d_sp_text.get(); a.starts = c->d_sp_bits.get(); a.out_doc_off = c->d_sp_off.get();
    HIP_TRY(hipMemsetAsync(c->d_sp_bits.get(), 0, 2 * bw * 4, s));
    if (special) {
        // where launch_all's tile part will look for them: the layout of check_call / fill_batch for n_out bytes
        const size_t uw = sp_scan_words(n_out);
        HIP_TRY(hipMemsetAsync(c->d_zero.get(), 0, ((tk->special_general ? 4 : 3) * uw + QCOUNT_WORDS) * 4, s));
        c->bitmap_dirty = true;
        a.o_tbits = c->d_zero.get(); a.o_tstart = c->d_zero.get() + uw; a.o_skip = c->d_zero.get() + 2 * uw;
        a.stage_out = c->d_stage.get();
    }
    hipLaunchKernelGGL(k_sp_rewrite<true>, dim3(ntiles), dim3(SPT_NT), 0, s, a);
    if (c->prof) HIP_TRY(hipEventRecord(ev[2].get(), s));
    HIP_TRY(hipGetLastError());
    ExtIn ext;
    ext.d_starts = c->d_sp_bits.get(); ext.d_gaps = c->d_sp_bits.get() + bw;
    if (special) ext.d_status = c->d_sp_bits.get() + 2 * bw - 1;      // (non-null: the literals' bitmaps are the GPU's; nothing writes the word -- the front part does not run)
    SPL_TRY(launch_all(tk, c, {.text = c->d_sp_text.get(), .n_bytes = n_out, .doc_off = c->d_sp_off.get(), .n_docs = n_docs, .flags = flags,
                               .ids = d_ids, .ids_cap = ids_cap, .out_off = d_out_off, .stream = s, .slab = so, .ext = &ext,
                               .part = special ? LaunchPart::Tiles : LaunchPart::All}));
    if (c->prof) {
        HIP_TRY(hipEventSynchronize(ev[2].get()));
        for (int k = 0; k < 2; k++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ev[k].get(), ev[k + 1].get()));
            c->prof_ms[KI_SP_COUNT + k] += ms; c->prof_n[KI_SP_COUNT + k] += 1;
        }
    }
    return SPL_OK;
}

// spl_encode_batch on a SentencePiece, WordPiece or Unigram handle (the latter two through encode_device_wp, spl_wp_host.h, and encode_device_uni, spl_uni_host.h: the same limit): pieces of whole documents of at most SP_MAX_BYTES, one after the other -- text and offsets
// to the device, the device call above with n_bytes ids of room, once more with the need it reported if that was short, the ids back.
int encode_host_sp(spl_tokenizer* tk, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, spl_result* r) {
    Ctx* c = tk->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(ensure_streams(*c));
    hipStream_t s = c->s_cmp.get();
    r->pool = tk->pool;
    r->n_docs = n_docs;
    r->off = (uint64_t*)tk->pool->get((n_docs + 1) * 8, r->off_cap);
    if (!r->off) return fail(SPL_EDEVICE, "pinned result allocation failed");
    r->off[0] = 0;
    std::vector<uint32_t> all;
    std::vector<uint64_t> rel;
    for (uint64_t d = 0; d < n_docs;) {
        uint64_t e = d + 1;
        const uint64_t lo = doc_off[d];
        if (doc_off[e] - lo > SP_MAX_BYTES) return fail(SPL_EINVAL, std::string("spl_encode_batch: ") + (tk->uni ? "Unigram" : tk->wp ? "WordPiece" : "SentencePiece") + " mode takes documents of at most 64 MiB");
        while (e < n_docs && doc_off[e + 1] - lo <= SP_MAX_BYTES) e++;
        const uint64_t nb = doc_off[e] - lo, nd = e - d;
        rel.resize(nd + 1);
        for (uint64_t i = 0; i <= nd; i++) rel[i] = doc_off[d + i] - lo;
        SPL_TRY(c->d_sph_text.grow(&c->sph_text_cap, nb + 16, nb + nb / 4 + 4096));
        SPL_TRY(c->d_sph_off.grow(&c->sph_off_cap, nd + 1, nd + nd / 4 + 1024));
        SPL_TRY(c->d_sph_oo.grow(&c->sph_oo_cap, nd + 1, nd + nd / 4 + 1024));
        SPL_TRY(c->d_sph_ids.grow(&c->sph_ids_cap, nb + 16, nb + nb / 4 + 4096));
        if (nb) HIP_TRY(hipMemcpyAsync(c->d_sph_text.get(), utf8 + lo, nb, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->d_sph_off.get(), rel.data(), (nd + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));                        // (rel is reused by the next piece)
        uint64_t need = 0;
        for (int pass = 0; pass < 2; pass++) {
            SPL_TRY((tk->uni ? encode_device_uni : tk->wp ? encode_device_wp : encode_device_sp)(tk, c, c->d_sph_text.get(), nb, c->d_sph_off.get(), nd, flags, c->d_sph_ids.get(), c->sph_ids_cap, c->d_sph_oo.get(), s, nullptr));
            HIP_TRY(hipMemcpyAsync(&need, c->d_sph_oo.get() + nd, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (need <= c->sph_ids_cap) break;
            if (pass) return fail(SPL_EDEVICE, "spl_encode_batch: the token count changed between two passes");
            SPL_TRY(c->d_sph_ids.grow(&c->sph_ids_cap, need, need + 4096));
        }
        const uint64_t t0 = all.size();
        all.resize(t0 + need);
        if (need) HIP_TRY(hipMemcpy(all.data() + t0, c->d_sph_ids.get(), need * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(r->off + d + 1, c->d_sph_oo.get() + 1, nd * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 1; i <= nd; i++) r->off[d + i] += t0;
        d = e;
    }
    r->n_tokens = all.size();
    r->ids = (uint32_t*)tk->pool->get((all.size() + 16) * 4, r->ids_cap);
    if (!r->ids) return fail(SPL_EDEVICE, "pinned result allocation failed");
    if (!all.empty()) memcpy(r->ids, all.data(), all.size() * 4);
    return SPL_OK;
}
}  // namespace
