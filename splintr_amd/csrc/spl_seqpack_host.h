// spl_seqpack_host.h -- the host half of spl_seqpack_device: the refusals (all of them before the device is touched) and the two launches
// of spl_k_seqpack.h, the plan of the strategy (one workgroup) and k_seqpack_gather.  Nothing is allocated and nothing synchronises; the
// order of the launches is the stream's.
#pragma once
namespace {

static_assert(SQP_NEXT_FIT == SPL_SEQPACK_NEXT_FIT && SQP_BFD == SPL_SEQPACK_BEST_FIT_DECREASING && SQP_MASK_FIRST == SPL_SEQPACK_MASK_FIRST &&
              SQP_BFD_MAX_L == SPL_SEQPACK_BFD_MAX_ROW_LEN, "spl_k_seqpack.h and splintr_hip.h must agree on the values");
static_assert((SPL_SEQPACK_MASK_FIRST & (SPL_COLLATE_I64 | SPL_COLLATE_PAD_LEFT | SPL_COLLATE_KEEP_TAIL | SPL_COLLATE_BOS | SPL_COLLATE_EOS)) == 0,
              "a flag bit of its own");

int seqpack_device(spl_tokenizer* t, const spl_seqpack_in* in, const spl_seqpack_opts* o, const spl_seqpack_out* out, void* d_work, hipStream_t st) {
    const std::string who = "spl_seqpack_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!in) return fail(SPL_EINVAL, who + ": the input struct is null");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!out) return fail(SPL_EINVAL, who + ": the output struct is null");
    SPL_TRY(refuse_struct_size(who, "spl_seqpack_in", in->struct_size, sizeof(spl_seqpack_in), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_seqpack_opts", o->struct_size, sizeof(spl_seqpack_opts), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_seqpack_out", out->struct_size, sizeof(spl_seqpack_out), "the struct"));
    if (!out->d_rows) return fail(SPL_EINVAL, who + ": d_rows is null");
    if (!out->d_status) return fail(SPL_EINVAL, who + ": d_status is null");
    if (!d_work) return fail(SPL_EINVAL, who + ": d_work is null");
    if (in->d_lengths && in->d_off) return fail(SPL_EINVAL, who + ": both input forms are given: d_lengths (rows) and d_off (CSR)");
    if (!in->d_lengths && !in->d_off) return fail(SPL_EINVAL, who + ": neither input form is given: d_lengths (rows) or d_off (CSR)");
    if (o->flags & (SPL_COLLATE_BOS | SPL_COLLATE_EOS)) return fail(SPL_EINVAL, who + ": SPL_COLLATE_BOS and _EOS are not flags of this call");
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_COLLATE_I64 | SPL_COLLATE_PAD_LEFT | SPL_COLLATE_KEEP_TAIL | SPL_SEQPACK_MASK_FIRST));
    if ((o->flags & SPL_COLLATE_PAD_LEFT) && in->d_off) return fail(SPL_EINVAL, who + ": SPL_COLLATE_PAD_LEFT says how input ROWS are padded; a CSR has no padding");
    if (o->strategy != SPL_SEQPACK_NEXT_FIT && o->strategy != SPL_SEQPACK_BEST_FIT_DECREASING) return fail(SPL_EINVAL, who + ": unknown strategy");
    if (o->row_len == 0) return fail(SPL_EINVAL, who + ": row_len is 0");
    if (o->strategy == SPL_SEQPACK_BEST_FIT_DECREASING && o->row_len > SPL_SEQPACK_BFD_MAX_ROW_LEN)
        return fail(SPL_EINVAL, who + ": best_fit_decreasing takes row_len up to SPL_SEQPACK_BFD_MAX_ROW_LEN (32768)");
    if (in->n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    if (out->max_rows >= (1ull << 31)) return fail(SPL_EINVAL, who + ": max_rows >= 2^31");
    if (out->d_cu && out->max_rows * o->row_len >= (1ull << 31)) return fail(SPL_EINVAL, who + ": d_cu is int32: max_rows * row_len must be below 2^31");
    if (in->n_seqs && !in->d_ids) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (in->n_seqs && in->d_lengths && in->in_len == 0) return fail(SPL_EINVAL, who + ": in_len is 0");
    const void* a16[] = {out->d_rows, out->d_labels, out->d_pos, out->d_seq, out->d_place, out->d_fill, out->d_cu, out->d_n, d_work};
    const char* n16[] = {"d_rows", "d_labels", "d_pos", "d_seq", "d_place", "d_fill", "d_cu", "d_n", "d_work"};
    for (int i = 0; i < 9; i++) if (col_misaligned(a16[i], 16)) return fail(SPL_EINVAL, who + ": " + n16[i] + " is not 16-byte aligned");
    for (int k = 0; k < 4; k++) if (col_misaligned(out->d_bytes[k], 4)) return fail(SPL_EINVAL, who + ": a byte output is not 4-byte aligned");
    if (col_misaligned(out->d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    if (col_misaligned(in->d_lengths, 4)) return fail(SPL_EINVAL, who + ": d_lengths is not 4-byte aligned");
    if (col_misaligned(in->d_off, 8)) return fail(SPL_EINVAL, who + ": d_off is not 8-byte aligned");
    if (col_misaligned(in->d_ids, 4) || col_misaligned(in->d_labels, 4)) return fail(SPL_EINVAL, who + ": d_ids or the input d_labels is not 4-byte aligned");
    SqpIn si{in->d_ids, in->d_lengths, in->d_off, in->d_labels, in->d_bytes[0], in->d_bytes[1], in->d_bytes[2], in->d_bytes[3],
             (uint32_t)in->n_seqs, in->in_len};
    SqpGeo g{};
    g.flags = o->flags; g.strategy = o->strategy; g.L = o->row_len; g.pad_id = o->pad_id; g.ignore_id = o->ignore_id;
    g.fills = (uint32_t)o->fill[0] | (uint32_t)o->fill[1] << 8 | (uint32_t)o->fill[2] << 16 | (uint32_t)o->fill[3] << 24;
    g.R = (uint32_t)out->max_rows; g.lds_max = t->seqpack_lds_max;
    const SqpPlanOut po{out->d_place, out->d_fill, out->d_cu, out->d_n, out->d_status};
    // an output whose input companion is missing is not written (there is nothing to carry)
    const SqpRowsOut ro{out->d_rows, in->d_labels ? out->d_labels : nullptr, in->d_bytes[0] ? out->d_bytes[0] : nullptr,
                        in->d_bytes[1] ? out->d_bytes[1] : nullptr, in->d_bytes[2] ? out->d_bytes[2] : nullptr,
                        in->d_bytes[3] ? out->d_bytes[3] : nullptr, out->d_mask, out->d_pos, out->d_seq};
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    if (g.strategy == SQP_BFD) hipLaunchKernelGGL(k_seqpack_bfd, dim3(1), dim3(SQP_NT), 0, st, si, g, d_work, po);
    else hipLaunchKernelGGL(k_seqpack_next_fit, dim3(1), dim3(SQP_NT), 0, st, si, g, d_work, po);
    if (out->max_rows) {
        uint32_t gx, gy, gz;
        cpair_grid(out->max_rows * g.L, gx, gy, gz);
        const dim3 grid(gx, gy, gz);
        if (g.flags & COL_I64) hipLaunchKernelGGL(k_seqpack_gather<true>, grid, dim3(COL_NT), 0, st, si, g, d_work, ro);
        else hipLaunchKernelGGL(k_seqpack_gather<false>, grid, dim3(COL_NT), 0, st, si, g, d_work, ro);
    }
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
