// spl_decode_dev_host.h -- the host half of spl_decode_reserve_device / spl_decode_batch_device: the refusals (all of them before the handle
// or the device is touched), the block-sum scratch (Ctx::d_ddblk: 8 bytes per 1 024 ids, grow-only, shared with nothing) and the three
// launches (spl_k_decode_dev.h, k_decode_scan of spl_k_decode.h).  A call within what was reserved neither allocates nor synchronises.
#pragma once
namespace {

static_assert(DD_I64 == SPL_DECODE_I64 && DD_PAD_LEFT == SPL_DECODE_PAD_LEFT && DD_SKIP_SPECIAL == SPL_DECODE_SKIP_SPECIAL,
              "spl_k_decode_dev.h and splintr_hip.h must agree on the flags");
static_assert(DD_BLK == DEC_BLK, "k_decode_scan scans sums per DEC_BLK ids");

constexpr uint64_t DD_MAX_IDS = 1ull << 41;            // one workgroup per 1 024 ids, below 2^31 of them

// the longest byte string any id decodes to: one walk over the vocabulary and the specials, kept until the next spl_add_special
uint32_t max_token_bytes(const spl_tokenizer* t) {
    if (t->max_tok_bytes) return t->max_tok_bytes;
    uint32_t m = 0;
    for (uint32_t id = 0; id <= t->ht.max_id; id++)
        if (t->ht.tok_present[id]) m = std::max(m, t->ht.tok_off[id + 1] - t->ht.tok_off[id]);
    for (const auto& s : t->specials) m = std::max<uint32_t>(m, (uint32_t)s.lit.size());
    return t->max_tok_bytes = m;
}

// the decode tables on the device (synchronises once, the first time) and block sums for max_ids ids
int decode_dev_prepare(spl_tokenizer* t, Ctx* c, uint64_t max_ids) {
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_decode(t, c));
    const uint64_t need = dd_n_blocks(max_ids, DD_BLK) + 1;           // (+ 1: the total behind the sums)
    return c->d_ddblk.grow(&c->ddblk_cap, need, need + need / 4 + 64);
}

// spl_token_spans_device's block sums of bytes and of characters for max_ids ids (Ctx::d_snblk): two arrays of n_blk + 1 (the total behind
// the sums) in one allocation, grow-only, shared with nothing
int spans_scratch(Ctx* c, uint64_t max_ids) {
    const uint64_t need = 2 * (dd_n_blocks(max_ids, DD_BLK) + 1);
    return c->d_snblk.grow(&c->snblk_cap, need, need + need / 4 + 128);
}

int decode_reserve_device(spl_tokenizer* t, uint64_t max_ids) {
    const std::string who = "spl_decode_reserve_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (max_ids >= DD_MAX_IDS) return fail(SPL_EINVAL, who + ": max_ids is 2^41 or more");
    SPL_TRY(decode_dev_prepare(t, t->ctx[0].get(), max_ids));
    return spans_scratch(t->ctx[0].get(), max_ids);
}

// What spl_decode_batch_device and spl_token_spans_device refuse about their INPUT (the ids, their offsets or lengths, the options), in
// the decode's order; *slots_out = the slots the grid covers.  The handle and the device are not touched.
int decode_dev_check_in(const std::string& who, const spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap, const uint64_t* d_ids_off,
                        const int32_t* d_len, uint64_t n_docs, const spl_decode_opts* o, uint64_t* slots_out) {
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    SPL_TRY(refuse_struct_size(who, "spl_decode_opts", o->struct_size, sizeof(spl_decode_opts), "the struct's three fields (12 bytes)"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_DECODE_I64 | SPL_DECODE_PAD_LEFT | SPL_DECODE_SKIP_SPECIAL));
    const bool rows = o->row_len != 0;
    if (n_docs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_docs >= 2^31");
    if (!rows) {
        if (o->flags & SPL_DECODE_PAD_LEFT) return fail(SPL_EINVAL, who + ": SPL_DECODE_PAD_LEFT is a rows-mode flag (row_len is 0: CSR mode)");
        if (d_len) return fail(SPL_EINVAL, who + ": d_len must be null in CSR mode (row_len is 0)");
        if (!d_ids_off) return fail(SPL_EINVAL, who + ": d_ids_off is null in CSR mode (row_len is 0)");
    } else if (d_ids_off) {
        return fail(SPL_EINVAL, who + ": d_ids_off must be null in rows mode (row_len > 0)");
    }
    const uint64_t slots = rows ? n_docs * o->row_len : n_ids_cap;      // (n_docs < 2^31, row_len < 2^32: no overflow)
    if (slots >= DD_MAX_IDS) return fail(SPL_EINVAL, who + (rows ? ": n_docs * row_len is 2^41 or more" : ": n_ids_cap is 2^41 or more"));
    if (!d_ids && slots && n_docs) return fail(SPL_EINVAL, who + ": d_ids is null");
    *slots_out = slots;
    return SPL_OK;
}
// ... and the last of them (the decode refuses its d_bytes between the two)
int decode_dev_check_ids_aligned(const std::string& who, const void* d_ids, const spl_decode_opts* o) {
    const bool i64 = (o->flags & SPL_DECODE_I64) != 0;
    if (col_misaligned(d_ids, i64 ? 32 : 16))
        return fail(SPL_EINVAL, who + (i64 ? ": d_ids is not 32-byte aligned (four int64 ids)" : ": d_ids is not 16-byte aligned (four 32-bit ids)"));
    return SPL_OK;
}

// the kernels' view of a call's input and of the context's decode tables
DecIn decode_dev_in(const void* d_ids, uint64_t n_ids_cap, const uint64_t* d_ids_off, const int32_t* d_len, uint64_t n_docs, const spl_decode_opts* o) {
    DecIn a{};
    a.ids = d_ids; a.ids_off = d_ids_off; a.len = d_len; a.n_docs = n_docs; a.n_cap = o->row_len ? 0 : n_ids_cap; a.row_len = o->row_len; a.flags = o->flags;
    return a;
}
DecTab decode_dev_tab(const Ctx* c) {
    DecTab tab{};
    tab.tok_off = c->d_tok_off.get(); tab.tok_bytes = c->d_tok_bytes.get(); tab.max_id = c->dec_max_id;
    tab.sp_ids = c->d_dec_sp_ids.get(); tab.sp_off = c->d_dec_sp_off.get(); tab.n_sp = c->dec_n_sp; tab.sp_bits = c->d_dec_spbits.get();
    return tab;
}

int decode_batch_device(spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap, const uint64_t* d_ids_off, const int32_t* d_len,
                        uint64_t n_docs, const spl_decode_opts* o, uint8_t* d_bytes, uint64_t bytes_capacity, uint64_t* d_out_off,
                        hipStream_t st) {
    const std::string who = "spl_decode_batch_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!d_out_off) return fail(SPL_EINVAL, who + ": d_out_off is null");
    uint64_t slots = 0;
    SPL_TRY(decode_dev_check_in(who, t, d_ids, n_ids_cap, d_ids_off, d_len, n_docs, o, &slots));
    if (!d_bytes && bytes_capacity) return fail(SPL_EINVAL, who + ": d_bytes is null with bytes_capacity > 0");
    if (col_misaligned(d_bytes, 16)) return fail(SPL_EINVAL, who + ": d_bytes is not 16-byte aligned");
    SPL_TRY(decode_dev_check_ids_aligned(who, d_ids, o));
    const bool i64 = (o->flags & SPL_DECODE_I64) != 0;

    Ctx* c = t->ctx[0].get();
    SPL_TRY(decode_dev_prepare(t, c, slots));
    const DecIn a = decode_dev_in(d_ids, n_ids_cap, d_ids_off, d_len, n_docs, o);
    const DecTab tab = decode_dev_tab(c);
    const uint64_t n_blk = dd_n_blocks(slots, DD_BLK);
    const dim3 grid((uint32_t)std::min<uint64_t>(n_blk, 0x7FFFFFFFull)), wg(DD_NT);
    uint64_t* blk = c->d_ddblk.get();
    if (i64) hipLaunchKernelGGL(k_dec_len<true>, grid, wg, 0, st, a, tab, n_blk, blk);
    else hipLaunchKernelGGL(k_dec_len<false>, grid, wg, 0, st, a, tab, n_blk, blk);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, st, blk, n_blk);
    if (i64) hipLaunchKernelGGL(k_dec_gather<true>, grid, wg, 0, st, a, tab, n_blk, (const uint64_t*)blk, d_bytes, bytes_capacity, d_out_off);
    else hipLaunchKernelGGL(k_dec_gather<false>, grid, wg, 0, st, a, tab, n_blk, (const uint64_t*)blk, d_bytes, bytes_capacity, d_out_off);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
