// spl_dfa_host.h -- the host half of spl_dfa_reserve_device / spl_dfa_index_device / spl_dfa_step_device (spl_k_dfa.h): the refusals (all
// of them before the device is touched), the tables (spl_heal_host.h's upload_heal: the decode tables and id -> rank, which says which ids
// are ordinary; shared with token healing and guided choice), the index's two launches and the step's one.  The DFA table and the index
// are the caller's device memory.  After the reserve a call neither allocates nor synchronises.
#pragma once
namespace {

static_assert(DF_KEEP_FREE == SPL_DFA_KEEP_FREE && DF_I64 == SPL_DFA_I64, "spl_k_dfa.h and splintr_hip.h must agree on the flags");
static_assert(DF_DEAD == SPL_DFA_DEAD && DF_MAX_STATES == SPL_DFA_MAX_STATES && DF_STATE_WORDS == SPL_DFA_STATE_WORDS && DF_MAX_END == SPL_DFA_MAX_END,
              "spl_k_dfa.h and splintr_hip.h must agree on the layout");
static_assert(SPL_DFA_TABLE_BYTES(3) == 3 * 513 && SPL_DFA_INDEX_BYTES(3, 5) == 3 * (8 * 4 + 1), "the macros size a table and an index");
static_assert(sizeof(((spl_dfa_opts*)nullptr)->end_ids) == sizeof(((DfIn*)nullptr)->end_ids), "the END ids travel by value");

int dfa_reserve_device(spl_tokenizer* t) {
    if (!t) return fail(SPL_EINVAL, "spl_dfa_reserve_device: null handle");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    return upload_heal(t, c);
}

// what every call asks of a table
int dfa_refuse_table(const std::string& who, const uint8_t* d_table, uint32_t n_states) {
    if (!d_table) return fail(SPL_EINVAL, who + ": d_table is null");
    if (col_misaligned(d_table, 2)) return fail(SPL_EINVAL, who + ": d_table is not 2-byte aligned (uint16 transitions)");
    if (!n_states || n_states > SPL_DFA_MAX_STATES)
        return fail(SPL_EINVAL, who + ": n_states is " + std::to_string(n_states) + ", not in 1 .. SPL_DFA_MAX_STATES (4096)");
    return SPL_OK;
}
// what the index and the steps ask of a table and a row width
int dfa_refuse_shape(const spl_tokenizer* t, const std::string& who, const uint8_t* d_table, uint32_t n_states, uint32_t n_words) {
    SPL_TRY(dfa_refuse_table(who, d_table, n_states));
    const uint32_t max_id = t->ht.max_id;
    if ((uint64_t)n_words * 32 < (uint64_t)max_id + 1)
        return fail(SPL_EINVAL, who + ": n_words is too small: " + std::to_string(n_words) + " words for ids up to " + std::to_string(max_id));
    if (n_words > (1u << 26)) return fail(SPL_EINVAL, who + ": n_words is above 2^26");
    return SPL_OK;
}

HlTab dfa_hl_tab(const Ctx* c) {
    return HlTab{c->d_tok_off.get(), c->d_tok_bytes.get(), c->dec_max_id, c->d_heal_sorted.get(), c->d_heal_rank.get(), c->d_heal_parent.get(), c->heal_n};
}
DfTab dfa_tab(const uint8_t* d_table, uint32_t n_states) {
    return DfTab{reinterpret_cast<const uint16_t*>(d_table), d_table + (size_t)n_states * 512, n_states};
}

int dfa_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, uint32_t n_words, int32_t* d_index, hipStream_t st) {
    const std::string who = "spl_dfa_index_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    SPL_TRY(dfa_refuse_shape(t, who, d_table, n_states, n_words));
    if (!d_index) return fail(SPL_EINVAL, who + ": d_index is null");
    if (col_misaligned(d_index, 4)) return fail(SPL_EINVAL, who + ": d_index is not 4-byte aligned");
    if ((const void*)d_index == (const void*)d_table) return fail(SPL_EINVAL, who + ": d_index coincides with d_table");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint32_t stride = df_stride(n_words);
    uint32_t* rows = reinterpret_cast<uint32_t*>(d_index);
    uint8_t* some = reinterpret_cast<uint8_t*>(d_index) + (size_t)n_states * stride * 4;
    const uint32_t per = DF_INDEX_NT / DF_WAVE, waves = stride / 2;                 // (a wavefront owns 64 ids: two words of every row)
    hipLaunchKernelGGL(k_dfa_index, dim3((waves + per - 1) / per, (n_states + DF_INDEX_STATES - 1) / DF_INDEX_STATES), dim3(DF_INDEX_NT), 0, st,
                       dfa_hl_tab(c), dfa_tab(d_table, n_states), stride, rows);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_dfa_some, dim3((n_states + per - 1) / per), dim3(DF_INDEX_NT), 0, st, rows, stride, n_states, some);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

// everything spl_dfa_step_device refuses (spl_dfa_jump_device refuses the same, under its own name)
int dfa_refuse_step(const spl_tokenizer* t, const std::string& who, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out) {
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!in) return fail(SPL_EINVAL, who + ": the input struct is null");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!out) return fail(SPL_EINVAL, who + ": the output struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_dfa_in", in->struct_size, sizeof(spl_dfa_in), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_dfa_opts", o->struct_size, sizeof(spl_dfa_opts), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_dfa_out", out->struct_size, sizeof(spl_dfa_out), "the struct"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_DFA_KEEP_FREE | SPL_DFA_I64));
    if (in->n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    SPL_TRY(dfa_refuse_shape(t, who, in->d_table, in->n_states, o->n_words));
    if (!in->d_index) return fail(SPL_EINVAL, who + ": d_index is null");
    if (!in->d_state_in) return fail(SPL_EINVAL, who + ": d_state_in is null");
    if (!out->d_state_out) return fail(SPL_EINVAL, who + ": d_state_out is null");
    if (!out->d_mask) return fail(SPL_EINVAL, who + ": d_mask is null");
    if (!in->d_ids && in->n_seqs && in->row_len) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (col_misaligned(in->d_ids, (o->flags & SPL_DFA_I64) ? 8 : 4)) return fail(SPL_EINVAL, who + ": d_ids is not aligned to its element type (int32, or int64 with SPL_DFA_I64)");
    if (col_misaligned(in->d_len, 4) || col_misaligned(out->d_mask, 4) || col_misaligned(in->d_index, 4))
        return fail(SPL_EINVAL, who + ": d_len, d_index or d_mask is not 4-byte aligned");
    if (col_misaligned(in->d_state_in, 8) || col_misaligned(out->d_state_out, 8)) return fail(SPL_EINVAL, who + ": a state array is not 8-byte aligned");
    // outputs may coincide with nothing but themselves: state out with state in is the one exception
    const void* ins[] = {in->d_ids, in->d_len, in->d_state_in, in->d_table, in->d_index};
    const void* outs[] = {out->d_state_out, out->d_mask, out->d_live};
    const char* on[] = {"d_state_out", "d_mask", "d_live"};
    for (int i = 0; i < 3; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < 5; j++)
            if (outs[i] == ins[j] && !(i == 0 && j == 2)) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with " + on[j]);
    }
    if (!o->n_end) return fail(SPL_EINVAL, who + ": n_end is 0: no sequence could ever finish");
    if (o->n_end > SPL_DFA_MAX_END) return fail(SPL_EINVAL, who + ": n_end is above SPL_DFA_MAX_END (8)");
    for (uint32_t i = 0; i < o->n_end; i++)
        if ((uint64_t)o->end_ids[i] >= (uint64_t)o->n_words * 32)
            return fail(SPL_EINVAL, who + ": END id " + std::to_string(o->end_ids[i]) + " is at or above 32 * n_words");
    return SPL_OK;
}

// the kernels' arguments of a step that passed dfa_refuse_step
DfIndex dfa_index_of(const spl_dfa_in* in, const spl_dfa_opts* o) {
    const uint32_t stride = df_stride(o->n_words);
    return DfIndex{reinterpret_cast<const uint32_t*>(in->d_index), reinterpret_cast<const uint8_t*>(in->d_index) + (size_t)in->n_states * stride * 4, stride};
}
DfIn dfa_in_of(const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out) {
    DfIn a{};
    a.ids = in->d_ids; a.len = in->d_len; a.state_in = in->d_state_in; a.n_seqs = in->n_seqs;
    a.row_len = in->row_len; a.flags = o->flags; a.n_words = o->n_words;
    a.v4 = o->n_words % 4 == 0 && !col_misaligned(out->d_mask, 16) && !col_misaligned(in->d_index, 16) ? 1u : 0u;
    a.n_end = o->n_end;
    for (uint32_t i = 0; i < o->n_end; i++) a.end_ids[i] = o->end_ids[i];
    return a;
}
DfOut dfa_out_of(const spl_dfa_opts* o, const spl_dfa_out* out) {
    return DfOut{out->d_state_out, reinterpret_cast<uint32_t*>(out->d_mask), out->d_live, o->n_words};
}

int dfa_step_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out, hipStream_t st) {
    SPL_TRY(dfa_refuse_step(t, "spl_dfa_step_device", in, o, out));
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const DfIndex x = dfa_index_of(in, o);
    const DfIn a = dfa_in_of(in, o, out);
    const DfOut co = dfa_out_of(o, out);
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    hipLaunchKernelGGL(k_dfa_step, dim3(1, gy, gz), dim3(DF_WAVE), 0, st, a, dfa_hl_tab(c), dfa_tab(in->d_table, in->n_states), x, co);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
