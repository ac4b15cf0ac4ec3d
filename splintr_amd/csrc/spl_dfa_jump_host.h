// spl_dfa_jump_host.h -- the host half of spl_dfa_jump_index_device / spl_dfa_jump_device (spl_k_dfa_jump.h): the refusals (all of them
// before the device is touched), the build of the jump index -- force, runs, the runs compacted into a bytes CSR by the count-scan-write
// driver (spl_seqscan_host.h), the handle's own device encode over those n_states documents, the scatter -- and the step's one launch.
// The BUILD may allocate (Ctx::d_jmscr, grow-only, and the encode's workspace) and synchronises the stream ONCE, to read the runs' total
// bytes: the encode takes n_bytes from the host.  The STEP neither allocates nor synchronises after spl_dfa_reserve_device.
#pragma once
namespace {

static_assert(JM_MAX_BYTES == SPL_DFA_JUMP_MAX_BYTES && JM_MAX_IDS == SPL_DFA_JUMP_MAX_IDS, "spl_k_dfa_jump.h and splintr_hip.h must agree on the layout");
static_assert(SPL_DFA_JUMP_INDEX_BYTES(3) == 3 * 322, "the macro sizes a jump index");

// the scratch of one build, in uint64 words: the scan's sums and counts, the two CSRs' offsets, then the runs' text (16-byte aligned,
// readable to the next multiple of 16) and the ids (a byte is at most an id)
struct JmScratch {
    uint64_t S; uint64_t* base;
    uint64_t scan_words() const { return seq_n_blocks(S) + 1 + S; }
    uint64_t* doc_off() const { return base + scan_words(); }
    uint64_t* out_off() const { return doc_off() + S + 1; }
    uint64_t text_at() const { return (scan_words() + 2 * (S + 1) + 1) & ~1ull; }
    uint8_t* text() const { return reinterpret_cast<uint8_t*>(base + text_at()); }
    uint64_t text_cap() const { return S * JM_MAX_BYTES; }
    uint32_t* ids() const { return reinterpret_cast<uint32_t*>(base + text_at() + S * JM_MAX_BYTES / 8 + 2); }
    uint64_t words() const { return text_at() + S * JM_MAX_BYTES / 8 + 2 + S * JM_MAX_BYTES / 2; }
};

int dfa_jump_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, void* d_jump_index, hipStream_t st) {
    const std::string who = "spl_dfa_jump_index_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    SPL_TRY(dfa_refuse_table(who, d_table, n_states));
    if (!d_jump_index) return fail(SPL_EINVAL, who + ": d_jump_index is null");
    if (col_misaligned(d_jump_index, 4)) return fail(SPL_EINVAL, who + ": d_jump_index is not 4-byte aligned");
    if ((const void*)d_jump_index == (const void*)d_table) return fail(SPL_EINVAL, who + ": d_jump_index coincides with d_table");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t S = n_states;
    JmScratch scr{S, nullptr};
    SPL_TRY(c->d_jmscr.grow(&c->jmscr_cap, scr.words(), scr.words()));
    scr.base = c->d_jmscr.get();
    const JmIndex ix = jm_index(d_jump_index, S);
    uint32_t* force = ix.ids;                                                   // (the first S words of the ids: the scatter overwrites them)
    const uint32_t per = JM_NT / DF_WAVE, grid = (S + per - 1) / per;
    hipLaunchKernelGGL(k_dfa_force, dim3(grid), dim3(JM_NT), 0, st, dfa_tab(d_table, S), force);
    hipLaunchKernelGGL(k_dfa_runs, dim3(grid), dim3(JM_NT), 0, st, (const uint32_t*)force, S, ix.run, ix.run_len);
    HIP_TRY(hipGetLastError());
    if (t->jump_phase == 1) return SPL_OK;                                      // (measuring only: the index is incomplete)
    // the runs as S documents
    const SeqScratch s{S, scr.base};
    const uint64_t n_blk = s.n_blk();
    seq_launch(s, SEQ_ONE_MAX, st,
        [&] { hipLaunchKernelGGL(k_dfa_jump_one, dim3(1), dim3(SEQ_ONE_NT), 0, st, (const uint8_t*)ix.run, (const uint8_t*)ix.run_len, S, scr.text(), scr.text_cap(), scr.doc_off()); },
        [&](dim3 g, dim3 wg) { hipLaunchKernelGGL(k_dfa_jump_len, g, wg, 0, st, (const uint8_t*)ix.run_len, (uint64_t)S, n_blk, s.per_seq(0), s.blk); },
        [&](dim3 g, dim3 wg) {
            hipLaunchKernelGGL(k_dfa_jump_write, g, wg, 0, st, (const uint8_t*)ix.run, (const uint8_t*)ix.run_len, (uint64_t)S, n_blk, (const uint64_t*)s.per_seq(0),
                               (const uint64_t*)s.blk, scr.text(), scr.text_cap(), scr.doc_off());
        });
    HIP_TRY(hipGetLastError());
    // the ONE synchronisation: the encode takes the bytes' total from the host
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, scr.doc_off() + S, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (total > scr.text_cap()) return fail(SPL_EDEVICE, who + ": the runs hold more bytes than 64 a state");
    if (t->jump_phase == 2) return SPL_OK;
    if (total) {
        if (t->regex) SPL_TRY(encode_device_custom(t, c, scr.text(), total, scr.doc_off(), S, 0u, scr.ids(), scr.text_cap(), scr.out_off(), st, nullptr));
        else SPL_TRY(launch_all(t, c, {.text = scr.text(), .n_bytes = total, .doc_off = scr.doc_off(), .n_docs = S, .flags = 0u,
                                       .ids = scr.ids(), .ids_cap = scr.text_cap(), .out_off = scr.out_off(), .stream = st}));
    } else HIP_TRY(hipMemsetAsync(scr.out_off(), 0, (S + 1) * 8, st));           // (no run at all: S empty rows)
    if (t->jump_phase == 3) return SPL_OK;
    hipLaunchKernelGGL(k_dfa_jump_scatter, dim3(grid), dim3(JM_NT), 0, st, (const uint32_t*)scr.ids(), (const uint64_t*)scr.out_off(), scr.text_cap(), S,
                       ix.ids, ix.n_ids);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int dfa_jump_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out, const spl_dfa_jump_out* jo, hipStream_t st) {
    const std::string who = "spl_dfa_jump_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!jo) return fail(SPL_EINVAL, who + ": the jump struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_dfa_jump_out", jo->struct_size, sizeof(spl_dfa_jump_out), "the struct"));
    if (!jo->row_len_out || jo->row_len_out > SPL_DFA_JUMP_MAX_IDS)
        return fail(SPL_EINVAL, who + ": row_len_out is " + std::to_string(jo->row_len_out) + ", not in 1 .. SPL_DFA_JUMP_MAX_IDS (64)");
    if (!jo->d_jump_index) return fail(SPL_EINVAL, who + ": d_jump_index is null");
    if (!jo->d_forced_ids) return fail(SPL_EINVAL, who + ": d_forced_ids is null");
    if (!jo->d_forced_len) return fail(SPL_EINVAL, who + ": d_forced_len is null");
    if (col_misaligned(jo->d_jump_index, 4) || col_misaligned(jo->d_forced_ids, 4) || col_misaligned(jo->d_forced_len, 4))
        return fail(SPL_EINVAL, who + ": d_jump_index, d_forced_ids or d_forced_len is not 4-byte aligned");
    SPL_TRY(dfa_refuse_step(t, who, in, o, out));
    // the two new outputs coincide with nothing
    const void* others[] = {in->d_ids, in->d_len, in->d_state_in, in->d_table, in->d_index, jo->d_jump_index, out->d_state_out, out->d_mask, out->d_live};
    const void* mine[] = {jo->d_forced_ids, jo->d_forced_len};
    const char* mn[] = {"d_forced_ids", "d_forced_len"};
    for (int i = 0; i < 2; i++)
        for (const void* p : others)
            if (p && mine[i] == p) return fail(SPL_EINVAL, who + ": " + mn[i] + " coincides with another array of the call");
    if (mine[0] == mine[1]) return fail(SPL_EINVAL, who + ": d_forced_len coincides with d_forced_ids");
    const void* outs[] = {out->d_state_out, out->d_mask, out->d_live};
    for (const void* p : outs)
        if (p && p == jo->d_jump_index) return fail(SPL_EINVAL, who + ": d_jump_index coincides with an output array");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const DfIn a = dfa_in_of(in, o, out);
    const JmIndex ix = jm_index(const_cast<void*>(jo->d_jump_index), in->n_states);
    const JmStep j{ix.ids, ix.n_ids, jo->row_len_out};
    const JmOut co{dfa_out_of(o, out), jo->d_forced_ids, jo->d_forced_len, jo->row_len_out};
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    hipLaunchKernelGGL(k_dfa_jump, dim3(1, gy, gz), dim3(DF_WAVE), 0, st, a, dfa_hl_tab(c), dfa_tab(in->d_table, in->n_states), dfa_index_of(in, o), j, co);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
