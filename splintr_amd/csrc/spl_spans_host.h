// spl_spans_host.h -- the host half of spl_token_spans_device: the refusals (the decode's for the input -- decode_dev_check_in -- and its
// own for the outputs, all of them before the device is touched), the block-sum scratch (Ctx::d_snblk: two arrays of 8 bytes per 1 024
// ids, grow-only, shared with nothing; spans_scratch of spl_decode_dev_host.h, which spl_decode_reserve_device calls too) and the four launches (spl_k_spans.h,
// k_decode_scan of spl_k_decode.h once per array).  A call within what was reserved neither allocates nor synchronises.
#pragma once
namespace {

static_assert(SN_I64 == SPL_SPANS_I64, "spl_k_spans.h and splintr_hip.h must agree on the flag");

int token_spans_device(spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap, const uint64_t* d_ids_off, const int32_t* d_len,
                       uint64_t n_docs, const spl_decode_opts* o, uint32_t span_flags, void* d_byte_span, void* d_char_span,
                       uint64_t* d_byte_off, uint64_t* d_char_off, hipStream_t st) {
    const std::string who = "spl_token_spans_device";
    uint64_t slots = 0;
    SPL_TRY(decode_dev_check_in(who, t, d_ids, n_ids_cap, d_ids_off, d_len, n_docs, o, &slots));
    SPL_TRY(decode_dev_check_ids_aligned(who, d_ids, o));
    SPL_TRY(refuse_unknown_bits(who, "span_flags", span_flags, SPL_SPANS_I64));
    if (!d_byte_off) return fail(SPL_EINVAL, who + ": d_byte_off is null");
    if (col_misaligned(d_byte_span, 16)) return fail(SPL_EINVAL, who + ": d_byte_span is not 16-byte aligned");
    if (col_misaligned(d_char_span, 16)) return fail(SPL_EINVAL, who + ": d_char_span is not 16-byte aligned");
    if (max_token_bytes(t) > SN_MAX_TOKEN_BYTES)          // (the first refusal that reads the handle)
        return fail(SPL_EINVAL, who + ": a token of this handle is longer than 32 767 bytes (characters per id are counted in 15 bits)");

    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_decode(t, c));                         // (synchronises once, the first time)
    SPL_TRY(spans_scratch(c, slots));
    const DecIn a = decode_dev_in(d_ids, n_ids_cap, d_ids_off, d_len, n_docs, o);
    const DecTab tab = decode_dev_tab(c);
    const SpanTab stab{c->d_dec_nch.get(), c->d_dec_sp_nch.get()};
    const SpanOut out{d_byte_span, d_char_span, d_byte_off, d_char_off};
    const uint64_t n_blk = dd_n_blocks(slots, DD_BLK);
    const dim3 grid((uint32_t)std::min<uint64_t>(n_blk, 0x7FFFFFFFull)), wg(DD_NT);
    uint64_t* blk_b = c->d_snblk.get();
    uint64_t* blk_c = blk_b + n_blk + 1;
    const bool i64 = (o->flags & SPL_DECODE_I64) != 0, s64 = (span_flags & SPL_SPANS_I64) != 0;
    if (i64) hipLaunchKernelGGL(k_span_len<true>, grid, wg, 0, st, a, tab, stab, n_blk, blk_b, blk_c);
    else hipLaunchKernelGGL(k_span_len<false>, grid, wg, 0, st, a, tab, stab, n_blk, blk_b, blk_c);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, st, blk_b, n_blk);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, st, blk_c, n_blk);
#define SPL_SPAN_WRITE(I, S) hipLaunchKernelGGL((k_span_write<I, S>), grid, wg, 0, st, a, tab, stab, n_blk, (const uint64_t*)blk_b, (const uint64_t*)blk_c, out)
    if (i64) { if (s64) SPL_SPAN_WRITE(true, true); else SPL_SPAN_WRITE(true, false); }
    else { if (s64) SPL_SPAN_WRITE(false, true); else SPL_SPAN_WRITE(false, false); }
#undef SPL_SPAN_WRITE
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
