// spl_draft_host.h -- the host half of spl_dfa_draft_device / spl_nest_draft_device (spl_k_draft.h): the refusals (everything the step
// refuses, through the step's own checks, then the draft's; all of them before the device is touched) and the one launch of each.  After
// spl_dfa_reserve_device / spl_nest_reserve_device a call neither allocates nor synchronises.
#pragma once
namespace {

static_assert(DR_MAX_NODES == SPL_DRAFT_MAX_NODES && DR_PARENT_PER_SEQ == SPL_DRAFT_PARENT_PER_SEQ, "spl_k_draft.h and splintr_hip.h must agree");

// What the draft asks beyond the step.  The step's own refusals ran over `as_step`: the draft's mask and state rows where the step has
// its own (a state array that is not wanted is stood in for by an address no array has; nothing dereferences it).
int draft_refuse(const std::string& who, uint64_t n_seqs, uint32_t row_len, const void* const* ins, int n_ins, const spl_draft_out* dr) {
    if (row_len > SPL_DRAFT_MAX_NODES) return fail(SPL_EINVAL, who + ": row_len is " + std::to_string(row_len) + ", above SPL_DRAFT_MAX_NODES (64)");
    SPL_TRY(refuse_unknown_bits(who, "draft flag", dr->flags, SPL_DRAFT_PARENT_PER_SEQ));
    if (!dr->d_ok) return fail(SPL_EINVAL, who + ": d_ok is null");
    if (col_misaligned(dr->d_parent, 4)) return fail(SPL_EINVAL, who + ": d_parent is not 4-byte aligned");
    if ((dr->flags & SPL_DRAFT_PARENT_PER_SEQ) && !dr->d_parent) return fail(SPL_EINVAL, who + ": SPL_DRAFT_PARENT_PER_SEQ without d_parent");
    if ((1ull + row_len) * n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": (1 + row_len) * n_seqs >= 2^31");
    // no output may coincide with an input -- the state rows that are read included -- or with another output
    const void* outs[] = {dr->d_mask, dr->d_ok, dr->d_live, dr->d_state_out};
    const char* on[] = {"d_mask", "d_ok", "d_live", "d_state_out"};
    for (int i = 0; i < 4; i++) {
        if (!outs[i]) continue;
        if (outs[i] == (const void*)dr->d_parent) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < n_ins; j++)
            if (outs[i] == ins[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with " + on[j]);
    }
    return SPL_OK;
}
int draft_refuse_struct(const std::string& who, const spl_draft_out* dr) {
    if (!dr) return fail(SPL_EINVAL, who + ": the draft struct is null");
    return refuse_struct_size(who, "spl_draft_out", dr->struct_size, sizeof(spl_draft_out), "the struct");
}
// a state array the step's checks can be shown where the draft wants none
alignas(8) const uint64_t k_draft_no_state[1] = {0};

int dfa_draft_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_draft_out* dr, hipStream_t st) {
    const std::string who = "spl_dfa_draft_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    SPL_TRY(draft_refuse_struct(who, dr));
    spl_dfa_out as_step{};
    as_step.struct_size = sizeof(spl_dfa_out);
    as_step.d_state_out = dr->d_state_out ? dr->d_state_out : const_cast<uint64_t*>(k_draft_no_state);
    as_step.d_mask = dr->d_mask; as_step.d_live = dr->d_live;
    SPL_TRY(dfa_refuse_step(t, who, in, o, &as_step));
    const void* ins[] = {in->d_ids, in->d_len, in->d_state_in, in->d_table, in->d_index};
    SPL_TRY(draft_refuse(who, in->n_seqs, in->row_len, ins, 5, dr));
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const DfIndex x = dfa_index_of(in, o);
    const DfIn a = dfa_in_of(in, o, &as_step);
    const DrIn g{dr->d_parent, (dr->flags & SPL_DRAFT_PARENT_PER_SEQ) ? 1u : 0u};
    const DrDfaOut co{dr->d_state_out, reinterpret_cast<uint32_t*>(dr->d_mask), dr->d_live, dr->d_ok, o->n_words};
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    hipLaunchKernelGGL(k_dfa_draft, dim3(1 + in->row_len, gy, gz), dim3(DF_WAVE), 0, st, a, g, dfa_hl_tab(c), dfa_tab(in->d_table, in->n_states), x, co);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int nest_draft_device(spl_tokenizer* t, const spl_nest_in* in, const spl_nest_opts* o, const spl_draft_out* dr, hipStream_t st) {
    const std::string who = "spl_nest_draft_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    SPL_TRY(draft_refuse_struct(who, dr));
    spl_nest_out as_step{};
    as_step.struct_size = sizeof(spl_nest_out);
    as_step.d_state_out = dr->d_state_out ? dr->d_state_out : const_cast<uint64_t*>(k_draft_no_state);
    as_step.d_mask = dr->d_mask; as_step.d_live = dr->d_live;
    SPL_TRY(nest_refuse_step(t, who, in, o, &as_step));
    const void* ins[] = {in->d_ids, in->d_len, in->d_state_in, in->d_table, in->d_index};
    SPL_TRY(draft_refuse(who, in->n_seqs, in->row_len, ins, 5, dr));
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const NsIndexAt ix(const_cast<int32_t*>(in->d_index), in->n_states, o->n_words, in->dep_cap);
    const NsIndex x{ix.rows, ix.dep_off, ix.dep_ids, ix.some, ix.stride, in->dep_cap};
    DfIn a{};
    a.ids = in->d_ids; a.len = in->d_len; a.state_in = in->d_state_in; a.n_seqs = B;
    a.row_len = in->row_len; a.flags = o->flags; a.n_words = o->n_words;
    a.v4 = o->n_words % 4 == 0 && !col_misaligned(dr->d_mask, 16) && !col_misaligned(in->d_index, 16) ? 1u : 0u;
    a.n_end = o->n_end;
    for (uint32_t i = 0; i < o->n_end; i++) a.end_ids[i] = o->end_ids[i];
    const DrIn g{dr->d_parent, (dr->flags & SPL_DRAFT_PARENT_PER_SEQ) ? 1u : 0u};
    const DrNestOut co{dr->d_state_out, reinterpret_cast<uint32_t*>(dr->d_mask), dr->d_live, dr->d_ok, o->n_words};
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    hipLaunchKernelGGL(k_nest_draft, dim3(1 + in->row_len, gy, gz), dim3(DF_WAVE), 0, st, a, g, dfa_hl_tab(c), ns_tab(in->d_table, in->n_states, in->n_ret), x,
                       NsStep{o->max_depth}, co);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
