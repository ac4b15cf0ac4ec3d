// spl_chat_host.h -- the host half of spl_chat_device: the refusals (all of them before the handle or the device is touched) and the two
// launches of spl_k_chat.h, k_chat_turns and k_collate_chat.  Nothing is allocated and nothing synchronises; the order of the launches is
// the stream's.
#pragma once
namespace {

static_assert(CHAT_DROP_OLDEST == SPL_CHAT_DROP_OLDEST && CHAT_PIN_FIRST == SPL_CHAT_PIN_FIRST && CHAT_NO_ROLE == SPL_CHAT_NO_ROLE &&
              CHAT_MAX_ROLES == SPL_CHAT_MAX_ROLES && CHAT_MAX_HEADER == SPL_CHAT_MAX_HEADER && CHAT_MAX_FOOTER == SPL_CHAT_MAX_FOOTER &&
              CHAT_MAX_BOS == SPL_CHAT_MAX_BOS && CHAT_MAX_GEN == SPL_CHAT_MAX_GEN,
              "spl_k_chat.h and splintr_hip.h must agree on the flags and the limits");
static_assert((SPL_CHAT_DROP_OLDEST | SPL_CHAT_PIN_FIRST) == (SPL_PAIR_KEEP_TAIL_A | SPL_PAIR_KEEP_TAIL_B), "the collate family's flag bits 32 and 64");

int chat_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_off, uint64_t n_docs, const int32_t* d_turn_doc,
                const uint8_t* d_turn_role, const uint8_t* d_turn_train, uint64_t n_turns, const uint64_t* d_conv_off, uint64_t n_convs,
                const spl_chat_opts* o, void* d_rows, void* d_labels, uint8_t* d_loss, uint8_t* d_mask, uint8_t* d_role, uint8_t* d_special,
                int32_t* d_len, int32_t* d_kept, int32_t* d_turn_col, uint32_t* d_status, void* d_work, hipStream_t st) {
    const std::string who = "spl_chat_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!d_rows) return fail(SPL_EINVAL, who + ": d_rows is null");
    if (!d_off) return fail(SPL_EINVAL, who + ": d_off is null");
    if (!d_conv_off) return fail(SPL_EINVAL, who + ": d_conv_off is null");
    if (!d_status) return fail(SPL_EINVAL, who + ": d_status is null");
    if (!d_work) return fail(SPL_EINVAL, who + ": d_work is null");
    SPL_TRY(refuse_struct_size(who, "spl_chat_opts", o->struct_size, sizeof(spl_chat_opts), "the struct (968 bytes)"));
    if (o->flags & (SPL_COLLATE_KEEP_TAIL | SPL_COLLATE_BOS | SPL_COLLATE_EOS))
        return fail(SPL_EINVAL, who + ": SPL_COLLATE_KEEP_TAIL, _BOS and _EOS are not flags of this call: bos and gen take the place of BOS "
                                      "and EOS, SPL_CHAT_DROP_OLDEST that of KEEP_TAIL");
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_COLLATE_I64 | SPL_COLLATE_PAD_LEFT | SPL_CHAT_DROP_OLDEST | SPL_CHAT_PIN_FIRST));
    if ((o->flags & SPL_CHAT_PIN_FIRST) && !(o->flags & SPL_CHAT_DROP_OLDEST))
        return fail(SPL_EINVAL, who + ": SPL_CHAT_PIN_FIRST is valid only together with SPL_CHAT_DROP_OLDEST");
    if (o->n_roles < 1 || o->n_roles > SPL_CHAT_MAX_ROLES) return fail(SPL_EINVAL, who + ": n_roles is not in 1 .. SPL_CHAT_MAX_ROLES");
    if (o->n_bos > SPL_CHAT_MAX_BOS) return fail(SPL_EINVAL, who + ": n_bos exceeds SPL_CHAT_MAX_BOS");
    if (o->n_gen > SPL_CHAT_MAX_GEN) return fail(SPL_EINVAL, who + ": n_gen exceeds SPL_CHAT_MAX_GEN");
    for (uint32_t r = 0; r < o->n_roles; r++) {
        if (o->n_header[r] > SPL_CHAT_MAX_HEADER) return fail(SPL_EINVAL, who + ": n_header[" + std::to_string(r) + "] exceeds SPL_CHAT_MAX_HEADER");
        if (o->n_footer[r] > SPL_CHAT_MAX_FOOTER) return fail(SPL_EINVAL, who + ": n_footer[" + std::to_string(r) + "] exceeds SPL_CHAT_MAX_FOOTER");
    }
    if (o->train_content >> o->n_roles) return fail(SPL_EINVAL, who + ": train_content has a bit at or above n_roles");
    if (o->train_footer >> o->n_roles) return fail(SPL_EINVAL, who + ": train_footer has a bit at or above n_roles");
    if (o->row_len == 0) return fail(SPL_EINVAL, who + ": row_len is 0");
    if (o->row_len < o->n_bos + o->n_gen) return fail(SPL_EINVAL, who + ": row_len is smaller than bos + gen, which every row holds");
    if (n_docs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_docs >= 2^31");
    if (n_turns >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_turns >= 2^31");
    if (n_convs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_convs >= 2^31");
    if (!d_turn_doc && n_turns > n_docs) return fail(SPL_EINVAL, who + ": d_turn_doc is null (turn t takes document t) and n_turns exceeds n_docs");
    if (n_convs > (1ull << 63) / o->row_len) return fail(SPL_EINVAL, who + ": n_convs * row_len is beyond 2^63 elements");
    if (col_misaligned(d_rows, 16)) return fail(SPL_EINVAL, who + ": d_rows is not 16-byte aligned");
    if (col_misaligned(d_labels, 16)) return fail(SPL_EINVAL, who + ": d_labels is not 16-byte aligned");
    if (col_misaligned(d_len, 16)) return fail(SPL_EINVAL, who + ": d_len is not 16-byte aligned");
    if (col_misaligned(d_kept, 16)) return fail(SPL_EINVAL, who + ": d_kept is not 16-byte aligned");
    if (col_misaligned(d_turn_col, 16)) return fail(SPL_EINVAL, who + ": d_turn_col is not 16-byte aligned");
    if (col_misaligned(d_work, 16)) return fail(SPL_EINVAL, who + ": d_work is not 16-byte aligned");
    if (col_misaligned(d_loss, 4)) return fail(SPL_EINVAL, who + ": d_loss is not 4-byte aligned");
    if (col_misaligned(d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    if (col_misaligned(d_role, 4)) return fail(SPL_EINVAL, who + ": d_role is not 4-byte aligned");
    if (col_misaligned(d_special, 4)) return fail(SPL_EINVAL, who + ": d_special is not 4-byte aligned");
    if (col_misaligned(d_turn_doc, 4)) return fail(SPL_EINVAL, who + ": d_turn_doc is not 4-byte aligned");
    if (col_misaligned(d_conv_off, 8)) return fail(SPL_EINVAL, who + ": d_conv_off is not 8-byte aligned");
    if (n_turns && !d_turn_role) return fail(SPL_EINVAL, who + ": d_turn_role is null");
    if (n_docs && !d_ids) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (n_convs == 0) return SPL_OK;
    ChatGeo g{};
    g.flags = o->flags; g.L = o->row_len; g.pad_id = o->pad_id; g.ignore_id = o->ignore_id;
    g.n_bos = o->n_bos; g.n_gen = o->n_gen; g.n_roles = o->n_roles; g.train_content = o->train_content; g.train_footer = o->train_footer;
    chat_set_counts(g, o->n_header, o->n_footer);
    ChatTpl tpl{};
    for (uint32_t r = 0; r < o->n_roles; r++) {
        for (uint32_t j = 0; j < o->n_header[r]; j++) tpl.w[r * CHAT_MAX_HEADER + j] = o->header[r][j];
        for (uint32_t j = 0; j < o->n_footer[r]; j++) tpl.w[CHAT_TPL_FOOTER + r * CHAT_MAX_FOOTER + j] = o->footer[r][j];
    }
    for (uint32_t j = 0; j < o->n_bos; j++) tpl.w[CHAT_TPL_BOS + j] = o->bos[j];
    for (uint32_t j = 0; j < o->n_gen; j++) tpl.w[CHAT_TPL_GEN + j] = o->gen[j];
    const ChatSrc s{d_ids, d_off, d_turn_doc, d_turn_role, d_turn_train, d_conv_off, (uint32_t)n_docs, (uint32_t)n_turns, (uint32_t)n_convs};
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    const uint32_t turn_grid = (uint32_t)((n_convs + CHAT_WAVES - 1) / CHAT_WAVES);
    hipLaunchKernelGGL(k_chat_turns, dim3(turn_grid), dim3(COL_NT), 0, st, s, g, tpl, d_work, d_len, d_kept, d_turn_col, d_status);
    uint32_t gx, gy, gz;
    cpair_grid(n_convs * g.L, gx, gy, gz);
    const dim3 grid(gx, gy, gz);
    if (g.flags & COL_I64) hipLaunchKernelGGL(k_collate_chat<true>, grid, dim3(COL_NT), 0, st, s, g, d_work, d_rows, d_labels, d_loss, d_mask, d_role, d_special);
    else hipLaunchKernelGGL(k_collate_chat<false>, grid, dim3(COL_NT), 0, st, s, g, d_work, d_rows, d_labels, d_loss, d_mask, d_role, d_special);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
