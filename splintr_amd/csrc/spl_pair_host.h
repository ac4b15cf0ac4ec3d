// spl_pair_host.h -- the host half of spl_pair_device: the refusals (all of them before the handle or the device is touched) and the
// launch of k_collate_pair (spl_k_pair.h).  Nothing is allocated and nothing synchronises.
#pragma once
namespace {

static_assert(CPAIR_MAX_FIXED == SPL_PAIR_MAX_FIXED && CPAIR_KEEP_TAIL_A == SPL_PAIR_KEEP_TAIL_A && CPAIR_KEEP_TAIL_B == SPL_PAIR_KEEP_TAIL_B &&
              CPAIR_LONGEST_FIRST == SPL_PAIR_LONGEST_FIRST && CPAIR_ONLY_FIRST == SPL_PAIR_ONLY_FIRST && CPAIR_ONLY_SECOND == SPL_PAIR_ONLY_SECOND,
              "spl_k_pair.h and splintr_hip.h must agree on the flags and the truncation modes");

int pair_device(spl_tokenizer* t, const uint32_t* d_a_ids, const uint64_t* d_a_off, uint64_t n_a, const uint32_t* d_b_ids,
                const uint64_t* d_b_off, uint64_t n_b, const int32_t* d_a_idx, const int32_t* d_b_idx, uint64_t n_pairs,
                const spl_pair_opts* o_in, void* d_rows, uint8_t* d_mask, uint8_t* d_type, uint8_t* d_special, int32_t* d_len,
                int32_t* d_kept, uint32_t* d_status, hipStream_t st) {
    const std::string who = "spl_pair_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!o_in) return fail(SPL_EINVAL, who + ": the options are null");
    if (!d_rows) return fail(SPL_EINVAL, who + ": d_rows is null");
    if (!d_a_off || !d_b_off) return fail(SPL_EINVAL, who + (d_a_off ? ": d_b_off is null" : ": d_a_off is null"));
    if (!d_status) return fail(SPL_EINVAL, who + ": d_status is null");
    SPL_TRY(refuse_struct_size(who, "spl_pair_opts", o_in->struct_size, sizeof(spl_pair_opts), "the struct (416 bytes)"));
    if (o_in->flags & (SPL_COLLATE_KEEP_TAIL | SPL_COLLATE_BOS | SPL_COLLATE_EOS))
        return fail(SPL_EINVAL, who + ": SPL_COLLATE_KEEP_TAIL, _BOS and _EOS are not flags of this call: the fixed segments (prefix, middle, "
                                      "suffix) take the place of BOS and EOS, SPL_PAIR_KEEP_TAIL_A / _B that of KEEP_TAIL");
    SPL_TRY(refuse_unknown_bits(who, "flag", o_in->flags, SPL_COLLATE_I64 | SPL_COLLATE_PAD_LEFT | SPL_PAIR_KEEP_TAIL_A | SPL_PAIR_KEEP_TAIL_B));
    if (o_in->trunc > SPL_PAIR_ONLY_SECOND) return fail(SPL_EINVAL, who + ": trunc is none of SPL_PAIR_LONGEST_FIRST, _ONLY_FIRST, _ONLY_SECOND");
    if (o_in->n_prefix > SPL_PAIR_MAX_FIXED || o_in->n_middle > SPL_PAIR_MAX_FIXED || o_in->n_suffix > SPL_PAIR_MAX_FIXED)
        return fail(SPL_EINVAL, who + ": a fixed segment (n_prefix, n_middle, n_suffix) holds more than SPL_PAIR_MAX_FIXED ids");
    if (o_in->row_len == 0) return fail(SPL_EINVAL, who + ": row_len is 0");
    if (o_in->row_len < o_in->n_prefix + o_in->n_middle + o_in->n_suffix)
        return fail(SPL_EINVAL, who + ": row_len is smaller than the fixed segments every row holds");
    if (n_a >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_a >= 2^31");
    if (n_b >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_b >= 2^31");
    if (n_pairs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_pairs >= 2^31");
    if (!d_a_idx && n_pairs > n_a) return fail(SPL_EINVAL, who + ": d_a_idx is null (pair p takes document p of A) and n_pairs exceeds n_a");
    if (!d_b_idx && n_pairs > n_b) return fail(SPL_EINVAL, who + ": d_b_idx is null (pair p takes document p of B) and n_pairs exceeds n_b");
    if (n_pairs > (1ull << 63) / o_in->row_len) return fail(SPL_EINVAL, who + ": n_pairs * row_len is beyond 2^63 elements");
    if (col_misaligned(d_rows, 16)) return fail(SPL_EINVAL, who + ": d_rows is not 16-byte aligned");
    if (col_misaligned(d_len, 16)) return fail(SPL_EINVAL, who + ": d_len is not 16-byte aligned");
    if (col_misaligned(d_kept, 16)) return fail(SPL_EINVAL, who + ": d_kept is not 16-byte aligned");
    if (col_misaligned(d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    if (col_misaligned(d_type, 4)) return fail(SPL_EINVAL, who + ": d_type is not 4-byte aligned");
    if (col_misaligned(d_special, 4)) return fail(SPL_EINVAL, who + ": d_special is not 4-byte aligned");
    if (col_misaligned(d_a_idx, 4)) return fail(SPL_EINVAL, who + ": d_a_idx is not 4-byte aligned");
    if (col_misaligned(d_b_idx, 4)) return fail(SPL_EINVAL, who + ": d_b_idx is not 4-byte aligned");
    if (n_pairs && (!d_a_ids || !d_b_ids)) return fail(SPL_EINVAL, who + (d_a_ids ? ": d_b_ids is null" : ": d_a_ids is null"));
    if (n_pairs == 0) return SPL_OK;
    PairOpts o{};
    o.g.flags = o_in->flags; o.g.L = o_in->row_len; o.g.pad_id = o_in->pad_id; o.g.trunc = o_in->trunc;
    cpair_set_fixed(o, o_in->prefix, o_in->n_prefix, o_in->middle, o_in->n_middle, o_in->suffix, o_in->n_suffix);
    const PairSrc s{d_a_ids, d_a_off, d_b_ids, d_b_off, d_a_idx, d_b_idx, (uint32_t)n_a, (uint32_t)n_b};
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    uint32_t gx, gy, gz;
    cpair_grid(n_pairs * o.g.L, gx, gy, gz);
    const dim3 grid(gx, gy, gz);
    if (o.g.flags & COL_I64) hipLaunchKernelGGL(k_collate_pair<true>, grid, dim3(COL_NT), 0, st, s, (uint32_t)n_pairs, o, d_rows, d_mask, d_type, d_special, d_len, d_kept, d_status);
    else hipLaunchKernelGGL(k_collate_pair<false>, grid, dim3(COL_NT), 0, st, s, (uint32_t)n_pairs, o, d_rows, d_mask, d_type, d_special, d_len, d_kept, d_status);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
