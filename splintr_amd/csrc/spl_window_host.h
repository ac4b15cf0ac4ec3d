// spl_window_host.h -- the host half of spl_window_device: the refusals (all of them before the handle or the device is touched) and the
// launches of spl_k_window.h -- the scan of the rows per document (one launch for a batch of one span, three otherwise) and the
// gather.  Nothing is allocated and nothing synchronises; the order of the launches is the stream's.
#pragma once
namespace {

inline uint64_t window_work_bytes(uint64_t n_docs) { return win_work_words(n_docs) * sizeof(uint64_t); }

int window_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, const spl_collate_opts* o_in,
                  uint32_t overlap, void* d_rows, uint64_t rows_cap, uint8_t* d_mask, int32_t* d_len, int32_t* d_row_doc,
                  int64_t* d_row_start, uint64_t* d_row_off, uint64_t* d_n, void* d_work, hipStream_t st) {
    const std::string who = "spl_window_device";
    ColOpts o{};
    if (int rc = collate_check(who, false, t, d_out_off, n_docs, o_in, d_rows, o)) return rc;
    const uint32_t k = col_k(o.flags);
    if (o.flags & COL_KEEP_TAIL)
        return fail(SPL_EINVAL, who + ": SPL_COLLATE_KEEP_TAIL has no meaning here (windows truncate nothing)");
    if (o.L <= k) return fail(SPL_EINVAL, who + ": row_len leaves no room for a token beside BOS + EOS (the body budget row_len - k must be at least 1)");
    if (overlap >= o.L - k) return fail(SPL_EINVAL, who + ": overlap must be smaller than the body budget row_len - k");
    if (!d_row_off) return fail(SPL_EINVAL, who + ": d_row_off is null");
    if (!d_n) return fail(SPL_EINVAL, who + ": d_n is null");
    if (!d_work && window_work_bytes(n_docs)) return fail(SPL_EINVAL, who + ": d_work is null (spl_window_work_bytes(n_docs) is not 0)");
    if (col_misaligned(d_mask, 4)) return fail(SPL_EINVAL, who + ": d_mask is not 4-byte aligned");
    if (col_misaligned(d_len, 16)) return fail(SPL_EINVAL, who + ": d_len is not 16-byte aligned");
    if (col_misaligned(d_row_doc, 16)) return fail(SPL_EINVAL, who + ": d_row_doc is not 16-byte aligned");
    if (col_misaligned(d_row_start, 16)) return fail(SPL_EINVAL, who + ": d_row_start is not 16-byte aligned");
    if (col_misaligned(d_row_off, 16)) return fail(SPL_EINVAL, who + ": d_row_off is not 16-byte aligned");
    if (col_misaligned(d_work, 8)) return fail(SPL_EINVAL, who + ": d_work is not 8-byte aligned");
    if (rows_cap && !d_rows) return fail(SPL_EINVAL, who + ": d_rows is null");
    if (n_docs && !d_ids) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (rows_cap > (1ull << 63) / o.L) return fail(SPL_EINVAL, who + ": rows_cap * row_len is beyond 2^63 elements");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    const WinGeo g{o.L - k, o.L - k - overlap};
    // 1. the scan: d_row_off and d_n, whatever rows_cap is
    const uint64_t spans = win_spans(n_docs);
    if (spans <= 1) {
        hipLaunchKernelGGL(k_window_scan, dim3(1), dim3(COL_NT), 0, st, d_out_off, n_docs, g, rows_cap, d_row_off, (uint64_t*)nullptr, d_n);
    } else {
        uint64_t* tot = static_cast<uint64_t*>(d_work);
        hipLaunchKernelGGL(k_window_scan, dim3((uint32_t)spans), dim3(COL_NT), 0, st, d_out_off, n_docs, g, rows_cap, d_row_off, tot, d_n);
        hipLaunchKernelGGL(k_window_totals, dim3(1), dim3(COL_NT), 0, st, tot, spans, t->win_chunk);
        hipLaunchKernelGGL(k_window_add, dim3((uint32_t)spans), dim3(COL_NT), 0, st, n_docs, rows_cap, d_row_off, (const uint64_t*)tot, d_n);
    }
    // 2. the gather: every element of the rows_cap rows (none: nothing to launch)
    const uint64_t total = rows_cap * o.L;
    if (total) {
        const uint32_t grid = collate_grid(total);
        if (o.flags & COL_I64)
            hipLaunchKernelGGL(k_window_gather<true>, dim3(grid), dim3(COL_NT), 0, st, d_ids, d_out_off, (const uint64_t*)d_row_off, n_docs, o, g,
                               d_rows, total, d_mask, d_len, d_row_doc, d_row_start);
        else
            hipLaunchKernelGGL(k_window_gather<false>, dim3(grid), dim3(COL_NT), 0, st, d_ids, d_out_off, (const uint64_t*)d_row_off, n_docs, o, g,
                               d_rows, total, d_mask, d_len, d_row_doc, d_row_start);
    }
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
