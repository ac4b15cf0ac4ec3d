// spl_heal_host.h -- the host half of spl_heal_reserve_device / spl_heal_begin_device / spl_heal_step_device: the refusals (all of them
// before the device is touched), the tables (built ONCE per context beside upload_decode's, again after spl_add_special: the ordinary ids
// sorted by their bytes, id -> rank, and every rank's parent in the prefix order), the scratch (Ctx::d_heal_scr: lo, hi and up to 63 partial
// ids per sequence, 264 bytes each, grow-only, shared with nothing) and the two launches of spl_k_heal.h.  A call within what was reserved
// neither allocates nor synchronises.
#pragma once
namespace {

static_assert(HL_AUTO == SPL_HEAL_AUTO && HL_KEEP_FREE == SPL_HEAL_KEEP_FREE && HL_I64 == SPL_HEAL_I64 && HL_PAD_LEFT == SPL_HEAL_PAD_LEFT,
              "spl_k_heal.h and splintr_hip.h must agree on the flags");
static_assert(HL_STATE_WORDS == SPL_HEAL_STATE_WORDS && HL_MAX_P == SPL_HEAL_MAX_PREFIX && HL_MAX_BACK == SPL_HEAL_MAX_BACK,
              "spl_k_heal.h and splintr_hip.h must agree on the layout");

// sorted, rank and parent of the vocabulary proper (spl_k_heal.h has the definitions)
int upload_heal(spl_tokenizer* tk, Ctx* c) {
    SPL_TRY(upload_decode(tk, c));
    if (c->heal_uploaded) return SPL_OK;
    const HostTables& ht = tk->ht;
    std::vector<uint32_t> sorted, rank, parent;
    if (!hl_build(ht.tok_off.data(), ht.tok_bytes.data(), ht.tok_present.data(), ht.max_id, sorted, rank, parent))
        return fail(SPL_EINVAL, "spl_heal_reserve_device: more than 63 ids spell prefixes of one 64-byte string (equal byte strings under many ids)");
    const uint32_t n = (uint32_t)sorted.size();
    HIP_TRY(hipDeviceSynchronize());
    SPL_TRY(c->d_heal_sorted.upload(sorted));
    SPL_TRY(c->d_heal_rank.upload(rank));
    SPL_TRY(c->d_heal_parent.upload(parent));
    c->heal_n = n;
    c->heal_uploaded = true;
    return SPL_OK;
}

int heal_prepare(spl_tokenizer* t, Ctx* c, uint64_t max_seqs) {
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_heal(t, c));
    return c->d_heal_scr.grow(&c->heal_cap, max_seqs * HL_SCR, std::max<uint64_t>(max_seqs, 64) * HL_SCR);
}

int heal_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    const std::string who = "spl_heal_reserve_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (max_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": max_seqs >= 2^31");
    return heal_prepare(t, t->ctx[0].get(), max_seqs);
}

int heal_device(spl_tokenizer* t, bool begin, const spl_heal_in* in, const spl_heal_opts* o, const spl_heal_out* out, hipStream_t st) {
    const std::string who = begin ? "spl_heal_begin_device" : "spl_heal_step_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!in) return fail(SPL_EINVAL, who + ": the input struct is null");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!out) return fail(SPL_EINVAL, who + ": the output struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_heal_in", in->struct_size, sizeof(spl_heal_in), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_heal_opts", o->struct_size, sizeof(spl_heal_opts), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_heal_out", out->struct_size, sizeof(spl_heal_out), "the struct"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, begin ? SPL_HEAL_AUTO | SPL_HEAL_KEEP_FREE | SPL_HEAL_I64 | SPL_HEAL_PAD_LEFT
                                                             : SPL_HEAL_KEEP_FREE | SPL_HEAL_I64));
    if (in->n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    if (begin && o->max_back > SPL_HEAL_MAX_BACK) return fail(SPL_EINVAL, who + ": max_back is above SPL_HEAL_MAX_BACK (8)");
    if (!out->d_state_out) return fail(SPL_EINVAL, who + ": d_state_out is null");
    if (!out->d_mask) return fail(SPL_EINVAL, who + ": d_mask is null");
    if (begin && !out->d_n_back) return fail(SPL_EINVAL, who + ": d_n_back is null");
    if (!begin && !in->d_state_in) return fail(SPL_EINVAL, who + ": d_state_in is null");
    if (!in->d_ids && in->n_seqs && in->row_len) return fail(SPL_EINVAL, who + ": d_ids is null");
    if ((o->flags & SPL_HEAL_PAD_LEFT) && !in->d_len) return fail(SPL_EINVAL, who + ": SPL_HEAL_PAD_LEFT needs d_len (where a left-padded row's tokens begin)");
    if (col_misaligned(in->d_ids, (o->flags & SPL_HEAL_I64) ? 8 : 4)) return fail(SPL_EINVAL, who + ": d_ids is not aligned to its element type (int32, or int64 with SPL_HEAL_I64)");
    if (col_misaligned(in->d_len, 4) || col_misaligned(out->d_mask, 4) || col_misaligned(out->d_n, 4) || col_misaligned(out->d_n_back, 4))
        return fail(SPL_EINVAL, who + ": d_len, d_mask, d_n or d_n_back is not 4-byte aligned");
    if (col_misaligned(in->d_state_in, 8) || col_misaligned(out->d_state_out, 8)) return fail(SPL_EINVAL, who + ": a state array is not 8-byte aligned");
    // outputs may coincide with nothing but themselves: state out with state in is the one exception
    const void* ins[] = {in->d_ids, in->d_len, begin ? nullptr : in->d_state_in};
    const void* outs[] = {out->d_state_out, out->d_mask, out->d_live, out->d_n, begin ? out->d_n_back : nullptr};
    const char* on[] = {"d_state_out", "d_mask", "d_live", "d_n", "d_n_back"};
    for (int i = 0; i < 5; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < 3; j++)
            if (outs[i] == ins[j] && !(i == 0 && j == 2)) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with " + on[j]);
    }
    const uint32_t max_id = t->ht.max_id;
    if ((uint64_t)o->n_words * 32 < (uint64_t)max_id + 1)
        return fail(SPL_EINVAL, who + ": n_words is too small: " + std::to_string(o->n_words) + " words for ids up to " + std::to_string(max_id));
    if (o->n_words > (1u << 26)) return fail(SPL_EINVAL, who + ": n_words is above 2^26");

    Ctx* c = t->ctx[0].get();
    SPL_TRY(heal_prepare(t, c, in->n_seqs));
    HlTab tab{c->d_tok_off.get(), c->d_tok_bytes.get(), c->dec_max_id, c->d_heal_sorted.get(), c->d_heal_rank.get(), c->d_heal_parent.get(), c->heal_n};
    HlIn a{};
    a.ids = in->d_ids; a.len = in->d_len; a.state_in = begin ? nullptr : in->d_state_in; a.n_seqs = in->n_seqs;
    a.row_len = in->row_len; a.flags = o->flags; a.max_back = begin ? o->max_back : 0; a.min_keep = o->min_keep;
    const HlOut po{out->d_state_out, out->d_live, begin ? out->d_n_back : nullptr, c->d_heal_scr.get()};
    const uint64_t B = in->n_seqs;
    if (B && t->heal_phase != 2) {
        const dim3 grid((uint32_t)((B + HL_PLAN_NT / HL_WAVE - 1) / (HL_PLAN_NT / HL_WAVE)));
        if (begin) hipLaunchKernelGGL(k_heal_plan<true>, grid, dim3(HL_PLAN_NT), 0, st, a, tab, po);
        else hipLaunchKernelGGL(k_heal_plan<false>, grid, dim3(HL_PLAN_NT), 0, st, a, tab, po);
    }
    if ((B || out->d_n) && t->heal_phase != 1) {
        const uint32_t spw = hl_spw(B, o->n_words);
        const uint64_t groups = B ? (B + spw - 1) / spw : 1;
        const uint32_t gy = (uint32_t)std::min<uint64_t>(groups, 65535), gz = (uint32_t)((groups + gy - 1) / gy);
        const dim3 grid(B ? (o->n_words + HL_WG_WORDS - 1) / HL_WG_WORDS : 1, gy, gz);
        hipLaunchKernelGGL(k_heal_fill, grid, dim3(HL_FILL_NT), 0, st, tab, c->d_heal_scr.get(), B, spw, o->n_words, o->flags,
                           reinterpret_cast<uint32_t*>(out->d_mask), out->d_n);
    }
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
