// spl_choice_host.h -- the host half of spl_choice_reserve_device / spl_choice_step_device (spl_k_choice.h): the refusals (all of them
// before the device is touched), the tables (spl_heal_host.h's upload_heal: the ordinary ids sorted by their bytes, id -> rank and the prefix
// order, shared with token healing) and the one launch.  No scratch: the row of a sequence is built in the LDS of the wavefront that owns
// it.  After the reserve a call neither allocates nor synchronises.
#pragma once
namespace {

static_assert(CH_THEN_FREE == SPL_CHOICE_THEN_FREE && CH_KEEP_FREE == SPL_CHOICE_KEEP_FREE && CH_I64 == SPL_CHOICE_I64,
              "spl_k_choice.h and splintr_hip.h must agree on the flags");
static_assert(CH_SLOTS == SPL_CHOICE_SLOTS && CH_MAX_LEN == SPL_CHOICE_MAX_LEN && CH_TABLE_BYTES == SPL_CHOICE_TABLE_BYTES &&
              CH_STATE_WORDS == SPL_CHOICE_STATE_WORDS && CH_MAX_END == SPL_CHOICE_MAX_END,
              "spl_k_choice.h and splintr_hip.h must agree on the layout");
static_assert(sizeof(((spl_choice_opts*)nullptr)->end_ids) == sizeof(((ChIn*)nullptr)->end_ids), "the END ids travel by value");

int choice_reserve_device(spl_tokenizer* t) {
    if (!t) return fail(SPL_EINVAL, "spl_choice_reserve_device: null handle");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    return upload_heal(t, c);
}

int choice_step_device(spl_tokenizer* t, const spl_choice_in* in, const spl_choice_opts* o, const spl_choice_out* out, hipStream_t st) {
    const std::string who = "spl_choice_step_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!in) return fail(SPL_EINVAL, who + ": the input struct is null");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!out) return fail(SPL_EINVAL, who + ": the output struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_choice_in", in->struct_size, sizeof(spl_choice_in), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_choice_opts", o->struct_size, sizeof(spl_choice_opts), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_choice_out", out->struct_size, sizeof(spl_choice_out), "the struct"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_CHOICE_THEN_FREE | SPL_CHOICE_KEEP_FREE | SPL_CHOICE_I64));
    if (in->n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    if (!in->d_table) return fail(SPL_EINVAL, who + ": d_table is null");
    if (!in->d_state_in) return fail(SPL_EINVAL, who + ": d_state_in is null");
    if (!out->d_state_out) return fail(SPL_EINVAL, who + ": d_state_out is null");
    if (!out->d_mask) return fail(SPL_EINVAL, who + ": d_mask is null");
    if (!in->d_ids && in->n_seqs && in->row_len) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (col_misaligned(in->d_ids, (o->flags & SPL_CHOICE_I64) ? 8 : 4)) return fail(SPL_EINVAL, who + ": d_ids is not aligned to its element type (int32, or int64 with SPL_CHOICE_I64)");
    if (col_misaligned(in->d_len, 4) || col_misaligned(out->d_mask, 4)) return fail(SPL_EINVAL, who + ": d_len or d_mask is not 4-byte aligned");
    if (col_misaligned(in->d_state_in, 8) || col_misaligned(out->d_state_out, 8)) return fail(SPL_EINVAL, who + ": a state array is not 8-byte aligned");
    // outputs may coincide with nothing but themselves: state out with state in is the one exception
    const void* ins[] = {in->d_ids, in->d_len, in->d_state_in, in->d_table};
    const void* outs[] = {out->d_state_out, out->d_mask, out->d_live};
    const char* on[] = {"d_state_out", "d_mask", "d_live"};
    for (int i = 0; i < 3; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < 4; j++)
            if (outs[i] == ins[j] && !(i == 0 && j == 2)) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with " + on[j]);
    }
    const uint32_t max_id = t->ht.max_id;
    if ((uint64_t)o->n_words * 32 < (uint64_t)max_id + 1)
        return fail(SPL_EINVAL, who + ": n_words is too small: " + std::to_string(o->n_words) + " words for ids up to " + std::to_string(max_id));
    if (o->n_words > (1u << 26)) return fail(SPL_EINVAL, who + ": n_words is above 2^26");
    if (o->n_end > SPL_CHOICE_MAX_END) return fail(SPL_EINVAL, who + ": n_end is above SPL_CHOICE_MAX_END (8)");
    if (!o->n_end && !(o->flags & SPL_CHOICE_THEN_FREE))
        return fail(SPL_EINVAL, who + ": no END id and no SPL_CHOICE_THEN_FREE: no sequence could ever finish");
    for (uint32_t i = 0; i < o->n_end; i++)
        if ((uint64_t)o->end_ids[i] >= (uint64_t)o->n_words * 32)
            return fail(SPL_EINVAL, who + ": END id " + std::to_string(o->end_ids[i]) + " is at or above 32 * n_words");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const HlTab tab{c->d_tok_off.get(), c->d_tok_bytes.get(), c->dec_max_id, c->d_heal_sorted.get(), c->d_heal_rank.get(), c->d_heal_parent.get(), c->heal_n};
    ChIn a{};
    a.ids = in->d_ids; a.len = in->d_len; a.state_in = in->d_state_in; a.table = in->d_table; a.n_seqs = B;
    a.row_len = in->row_len; a.flags = o->flags; a.n_words = o->n_words; a.piece = t->choice_piece;
    a.v4 = o->n_words % 4 == 0 && !col_misaligned(out->d_mask, 16) ? 1u : 0u;
    a.n_end = o->n_end;
    for (uint32_t i = 0; i < o->n_end; i++) a.end_ids[i] = o->end_ids[i];
    const ChOut co{out->d_state_out, reinterpret_cast<uint32_t*>(out->d_mask), out->d_live, o->n_words};
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    const size_t lds = sizeof(uint32_t) * std::min(o->n_words, a.piece);
    hipLaunchKernelGGL(k_choice, dim3(1, gy, gz), dim3(CH_WAVE), lds, st, a, tab, co);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
