// spl_collate_host.h -- the host half of spl_pad_device / spl_pack_device: the refusals (all of them before the handle or the device is
// touched) and the launches of k_collate_pad / k_collate_pack (spl_k_collate.h).  Nothing is allocated and nothing synchronises.
#pragma once
namespace {

static_assert(COL_I64 == SPL_COLLATE_I64 && COL_PAD_LEFT == SPL_COLLATE_PAD_LEFT && COL_KEEP_TAIL == SPL_COLLATE_KEEP_TAIL &&
              COL_BOS == SPL_COLLATE_BOS && COL_EOS == SPL_COLLATE_EOS, "spl_k_collate.h and splintr_hip.h must agree on the flags");

inline bool col_misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
// What every options struct and flag word is refused for (SPL_OK: not refused).  A caller's struct may be longer than this library's (only
// the fields known here are read), not shorter than `least`: `shorter` names that in the message, null for no such tail.
int refuse_struct_size(const std::string& who, const char* name, uint32_t have, size_t least, const char* shorter) {
    if (have >= least && have <= 4096) return SPL_OK;
    const std::string m = who + ": " + name + ".struct_size is not set";
    return fail(SPL_EINVAL, shorter ? m + ": it is shorter than " + shorter + " or above 4096" : m);
}
int refuse_unknown_bits(const std::string& who, const char* word, uint32_t bits, uint32_t known) {
    if (!(bits & ~known)) return SPL_OK;
    char b[64];
    snprintf(b, sizeof b, ": unknown %s bit 0x%x", word, bits & ~known);
    return fail(SPL_EINVAL, who + b);
}

// What both calls refuse alike; `o` receives the options the kernels take.
int collate_check(const std::string& who, bool pack, const spl_tokenizer* t, const uint64_t* d_out_off, uint64_t n_docs,
                  const spl_collate_opts* o_in, const void* d_rows, ColOpts& o) {
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!d_out_off) return fail(SPL_EINVAL, who + ": d_out_off is null");
    if (!o_in) return fail(SPL_EINVAL, who + ": the options are null");
    SPL_TRY(refuse_struct_size(who, "spl_collate_opts", o_in->struct_size, sizeof(spl_collate_opts), "the struct's six fields (24 bytes)"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o_in->flags, SPL_COLLATE_I64 | SPL_COLLATE_PAD_LEFT | SPL_COLLATE_KEEP_TAIL | SPL_COLLATE_BOS | SPL_COLLATE_EOS));
    if (pack && (o_in->flags & (SPL_COLLATE_PAD_LEFT | SPL_COLLATE_KEEP_TAIL)))
        return fail(SPL_EINVAL, who + ": SPL_COLLATE_PAD_LEFT and SPL_COLLATE_KEEP_TAIL are pad-mode flags (pack mode neither pads a document nor truncates)");
    if (o_in->row_len == 0) return fail(SPL_EINVAL, who + ": row_len is 0");
    if (!pack && o_in->row_len < col_k(o_in->flags))
        return fail(SPL_EINVAL, who + ": row_len is smaller than the BOS + EOS every row holds");
    if (n_docs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_docs >= 2^31");
    if (col_misaligned(d_rows, 16)) return fail(SPL_EINVAL, who + ": d_rows is not 16-byte aligned");
    o.flags = o_in->flags; o.L = o_in->row_len; o.pad_id = o_in->pad_id; o.bos_id = o_in->bos_id; o.eos_id = o_in->eos_id;
    return SPL_OK;
}

// one workgroup per COL_SPAN flat elements, sized from the OUTPUT; a workgroup takes several spans only beyond the grid's limit
inline uint32_t collate_grid(uint64_t total) {
    const uint64_t spans = (total + COL_SPAN - 1) / COL_SPAN;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(spans, 1), 0x7FFFFFFFull);
}

int pad_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, const spl_collate_opts* o_in,
               void* d_rows, uint8_t* d_mask, int32_t* d_len, hipStream_t st) {
    const std::string who = "spl_pad_device";
    ColOpts o{};
    if (int rc = collate_check(who, false, t, d_out_off, n_docs, o_in, d_rows, o)) return rc;
    if (col_misaligned(d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    if (col_misaligned(d_len, 16)) return fail(SPL_EINVAL, who + ": d_len is not 16-byte aligned");
    if (n_docs && (!d_rows || !d_ids)) return fail(SPL_EINVAL, who + (d_rows ? ": d_ids is null" : ": d_rows is null"));
    if (n_docs == 0) return SPL_OK;
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    const uint32_t grid = collate_grid(n_docs * o.L);
    if (o.flags & COL_I64) hipLaunchKernelGGL(k_collate_pad<true>, dim3(grid), dim3(COL_NT), 0, st, d_ids, d_out_off, n_docs, o, d_rows, d_mask, d_len);
    else hipLaunchKernelGGL(k_collate_pad<false>, dim3(grid), dim3(COL_NT), 0, st, d_ids, d_out_off, n_docs, o, d_rows, d_mask, d_len);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int pack_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, const spl_collate_opts* o_in,
                void* d_rows, uint64_t rows_cap, int32_t* d_doc, int32_t* d_pos, uint64_t* d_n, hipStream_t st) {
    const std::string who = "spl_pack_device";
    ColOpts o{};
    if (int rc = collate_check(who, true, t, d_out_off, n_docs, o_in, d_rows, o)) return rc;
    if (!d_n) return fail(SPL_EINVAL, who + ": d_n is null");
    if (col_misaligned(d_doc, 16)) return fail(SPL_EINVAL, who + ": d_doc is not 16-byte aligned");
    if (col_misaligned(d_pos, 16)) return fail(SPL_EINVAL, who + ": d_pos is not 16-byte aligned");
    if (rows_cap && !d_rows) return fail(SPL_EINVAL, who + ": d_rows is null");
    if (n_docs && !d_ids) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (rows_cap > (1ull << 63) / o.L) return fail(SPL_EINVAL, who + ": rows_cap * row_len is beyond 2^63 elements");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    const uint64_t total = rows_cap * o.L;
    const uint32_t grid = collate_grid(total);          // (at least one workgroup: d_n is always written)
    if (o.flags & COL_I64) hipLaunchKernelGGL(k_collate_pack<true>, dim3(grid), dim3(COL_NT), 0, st, d_ids, d_out_off, n_docs, o, d_rows, total, d_doc, d_pos, d_n);
    else hipLaunchKernelGGL(k_collate_pack<false>, dim3(grid), dim3(COL_NT), 0, st, d_ids, d_out_off, n_docs, o, d_rows, total, d_doc, d_pos, d_n);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
