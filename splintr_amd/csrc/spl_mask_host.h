// spl_mask_host.h -- the host half of spl_utf8_mask_reserve_device / spl_utf8_mask_device (spl_k_utf8mask.h) and of spl_mask_apply_device
// (spl_k_maskapply.h): the refusals (all of them before the device is touched), the UTF-8 class table (built ONCE per context by
// k_utf8_table behind upload_decode's tables, again after spl_add_special: 17 rows of the known ids' words, rounded up to four) and the
// one launch of each call.  After the reserve a call neither allocates nor synchronises; the apply needs no reserve at all.
#pragma once
namespace {

static_assert(UM_AND == SPL_UTF8_AND, "spl_k_utf8mask.h and splintr_hip.h must agree on the flag");
static_assert(MA_F32 == SPL_F32 && MA_F16 == SPL_F16 && MA_BF16 == SPL_BF16, "spl_k_maskapply.h and splintr_hip.h must agree on the dtypes");

// the words of a mask row that cover every id the handle knows
uint32_t utf8_min_words(const spl_tokenizer* t) { return std::max(t->ht.max_id, t->max_special_id) / 32 + 1; }

DecTab utf8_dec_tab(const Ctx* c) {
    return DecTab{c->d_tok_off.get(), c->d_tok_bytes.get(), c->dec_max_id, c->d_dec_sp_ids.get(), c->d_dec_sp_off.get(), c->dec_n_sp, c->d_dec_spbits.get()};
}

int upload_utf8(spl_tokenizer* tk, Ctx* c) {
    SPL_TRY(upload_decode(tk, c));
    if (c->u8_uploaded) return SPL_OK;
    const HostTables& ht = tk->ht;
    std::vector<uint32_t> present(ht.max_id / 32 + 1, 0);         // the vocabulary proper, a bit per id of the dense table
    for (uint32_t id = 0; id <= ht.max_id; id++)
        if (ht.tok_present[id]) present[id >> 5] |= 1u << (id & 31);
    const uint32_t stride = (utf8_min_words(tk) + 3u) & ~3u;
    HIP_TRY(hipDeviceSynchronize());
    c->u8_stride = 0;
    SPL_TRY(c->d_u8_present.upload(present));
    SPL_TRY(c->d_u8_rows.alloc((size_t)UM_ROWS * stride));
    const uint32_t waves = stride / 2, per = UM_NT / UM_WAVE;       // (a wavefront owns 64 ids: two words of every row)
    hipLaunchKernelGGL(k_utf8_table, dim3((waves + per - 1) / per), dim3(UM_NT), 0, (hipStream_t)0, utf8_dec_tab(c), c->d_u8_present.get(), stride,
                       c->d_u8_rows.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    c->u8_stride = stride;
    c->u8_uploaded = true;
    return SPL_OK;
}

int utf8_mask_reserve_device(spl_tokenizer* t) {
    if (!t) return fail(SPL_EINVAL, "spl_utf8_mask_reserve_device: null handle");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    return upload_utf8(t, c);
}

int utf8_mask_device(spl_tokenizer* t, const uint64_t* d_state, uint64_t n_seqs, const spl_decode_opts* o, uint32_t flags, uint32_t n_words,
                     int32_t* d_mask, uint8_t* d_live, hipStream_t st) {
    const std::string who = "spl_utf8_mask_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    SPL_TRY(refuse_struct_size(who, "spl_decode_opts", o->struct_size, sizeof(spl_decode_opts), "the struct"));
    SPL_TRY(refuse_unknown_bits(who, "flag", flags, SPL_UTF8_AND));
    SPL_TRY(refuse_unknown_bits(who, "decode flag", o->flags, SPL_DECODE_I64 | SPL_DECODE_PAD_LEFT | SPL_DECODE_SKIP_SPECIAL));
    if (n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    if (!d_state) return fail(SPL_EINVAL, who + ": d_state is null");
    if (!d_mask) return fail(SPL_EINVAL, who + ": d_mask is null");
    if (col_misaligned(d_state, 8)) return fail(SPL_EINVAL, who + ": d_state is not 8-byte aligned");
    if (col_misaligned(d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    const uint32_t need = utf8_min_words(t);
    if (n_words < need)
        return fail(SPL_EINVAL, who + ": n_words is too small: " + std::to_string(n_words) + " words for ids up to " + std::to_string(std::max(t->ht.max_id, t->max_special_id)));
    if (n_words > (1u << 26)) return fail(SPL_EINVAL, who + ": n_words is above 2^26");
    if ((const void*)d_state == (const void*)d_mask || (d_live && ((const void*)d_live == (const void*)d_state || (const void*)d_live == (const void*)d_mask)))
        return fail(SPL_EINVAL, who + ": d_state, d_mask and d_live must be three arrays");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_utf8(t, c));
    if (!n_seqs) return SPL_OK;
    const UmTab tab{c->d_u8_rows.get(), c->u8_stride};
    const uint32_t skip = (o->flags & SPL_DECODE_SKIP_SPECIAL) ? 1u : 0u;
    const bool v4 = n_words % 4 == 0 && !col_misaligned(d_mask, 16);
    const uint32_t per_wg = UM_NT * (v4 ? 4u : 1u);
    const uint32_t gy = (uint32_t)std::min<uint64_t>(n_seqs, 65535), gz = (uint32_t)((n_seqs + gy - 1) / gy);
    const dim3 grid((n_words + per_wg - 1) / per_wg, gy, gz);
    if (v4) hipLaunchKernelGGL(k_utf8_mask<true>, grid, dim3(UM_NT), 0, st, tab, d_state, n_seqs, skip, flags, n_words, reinterpret_cast<uint32_t*>(d_mask), d_live);
    else hipLaunchKernelGGL(k_utf8_mask<false>, grid, dim3(UM_NT), 0, st, tab, d_state, n_seqs, skip, flags, n_words, reinterpret_cast<uint32_t*>(d_mask), d_live);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int mask_apply_device(spl_tokenizer* t, const spl_mask_apply* a, hipStream_t st) {
    const std::string who = "spl_mask_apply_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!a) return fail(SPL_EINVAL, who + ": the request struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_mask_apply", a->struct_size, sizeof(spl_mask_apply), "the struct"));
    if (a->dtype > SPL_BF16) return fail(SPL_EINVAL, who + ": dtype is none of SPL_F32, SPL_F16, SPL_BF16");
    if (a->n_rows >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_rows >= 2^31");
    if (a->n_words > (1u << 26)) return fail(SPL_EINVAL, who + ": n_words is above 2^26");
    if (a->row_stride < a->n_cols) return fail(SPL_EINVAL, who + ": row_stride is below n_cols");
    if (a->mask_stride < a->n_words) return fail(SPL_EINVAL, who + ": mask_stride is below n_words");
    if (a->row_stride >= (1ull << 40) || a->mask_stride >= (1ull << 40)) return fail(SPL_EINVAL, who + ": row_stride or mask_stride is 2^40 or more");
    const bool work = a->n_rows && a->n_cols && a->n_words;
    if (work && !a->d_logits) return fail(SPL_EINVAL, who + ": d_logits is null");
    if (work && !a->d_mask) return fail(SPL_EINVAL, who + ": d_mask is null");
    const uint32_t es = ma_elem_bytes(a->dtype);
    if (col_misaligned(a->d_logits, es)) return fail(SPL_EINVAL, who + ": d_logits is not aligned to its element type");
    if (col_misaligned(a->d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    if (!work) return SPL_OK;
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    MaArgs k{};
    k.logits = (uint64_t)(uintptr_t)a->d_logits; k.mask = reinterpret_cast<const uint32_t*>(a->d_mask); k.live = a->d_live;
    k.n_rows = a->n_rows; k.row_stride = a->row_stride; k.mask_stride = a->mask_stride;
    k.n_cols = a->n_cols; k.n_words = a->n_words; k.es = es; k.ninf = ma_ninf(a->dtype);
    const uint64_t pieces = ma_grid_pieces(es, ma_n_eff(a->n_cols, a->n_words));
    const uint32_t gy = (uint32_t)std::min<uint64_t>(a->n_rows, 65535), gz = (uint32_t)((a->n_rows + gy - 1) / gy);
    const dim3 grid((uint32_t)((pieces + MA_NT - 1) / MA_NT), gy, gz);
    if (es == 4) hipLaunchKernelGGL(k_mask_apply<4>, grid, dim3(MA_NT), 0, st, k);
    else hipLaunchKernelGGL(k_mask_apply<2>, grid, dim3(MA_NT), 0, st, k);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
