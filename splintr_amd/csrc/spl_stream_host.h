// spl_stream_host.h -- the host half of spl_stream_reserve_device / spl_stream_decode_device: the refusals (all of them before the handle or
// the device is touched), the scratch (Ctx::d_stblk: the block sums, the total behind them and one count per sequence -- 8 bytes per
// sequence and 8 per 16 of them, grow-only, shared with nothing) and the launches (spl_k_stream.h; k_decode_scan of spl_k_decode.h).  A call
// within what was reserved neither allocates nor synchronises.
#pragma once
namespace {

static_assert(ST_REPLACE == SPL_STREAM_REPLACE && ST_FINAL_ALL == SPL_STREAM_FINAL_ALL, "spl_k_stream.h and splintr_hip.h must agree on the flags");

// one call's arguments, as the entry point received them
struct StreamReq {
    const void* ids = nullptr; const int32_t* len = nullptr; uint64_t n_seqs = 0; const spl_decode_opts* o = nullptr; uint32_t stream_flags = 0;
    const uint8_t* fin = nullptr; const uint64_t* state_in = nullptr; uint64_t* state_out = nullptr;
    uint8_t* bytes = nullptr; uint64_t bytes_cap = 0; uint64_t* out_off = nullptr; hipStream_t stream = nullptr;
};

// the decode tables on the device (synchronises once, the first time) and scratch for max_seqs sequences
int stream_prepare(spl_tokenizer* t, Ctx* c, uint64_t max_seqs) {
    HIP_TRY(hipSetDevice(c->device));
    SPL_TRY(upload_decode(t, c));
    const uint64_t need = st_n_blocks(max_seqs) + 1 + max_seqs;
    return c->d_stblk.grow(&c->stblk_cap, need, need + need / 4 + 64);
}

int stream_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    const std::string who = "spl_stream_reserve_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (max_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": max_seqs >= 2^31");
    return stream_prepare(t, t->ctx[0].get(), max_seqs);
}

int stream_decode_device(spl_tokenizer* t, const StreamReq& q) {
    const std::string who = "spl_stream_decode_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!q.o) return fail(SPL_EINVAL, who + ": the options are null");
    if (!q.state_in) return fail(SPL_EINVAL, who + ": d_state_in is null");
    if (!q.state_out) return fail(SPL_EINVAL, who + ": d_state_out is null");
    if (!q.out_off) return fail(SPL_EINVAL, who + ": d_out_off is null");
    const uint32_t have = q.o->struct_size;       // the caller's struct may be longer than this library's: only the fields known here are read
    if (have < sizeof(spl_decode_opts) || have > 4096)
        return fail(SPL_EINVAL, who + ": spl_decode_opts.struct_size is not set: it is shorter than the struct's three fields (12 bytes) or above 4096");
    const uint32_t known = SPL_DECODE_I64 | SPL_DECODE_PAD_LEFT | SPL_DECODE_SKIP_SPECIAL, sknown = SPL_STREAM_REPLACE | SPL_STREAM_FINAL_ALL;
    char b[64];
    if (q.o->flags & ~known) {
        snprintf(b, sizeof b, ": unknown flag bit 0x%x", q.o->flags & ~known);
        return fail(SPL_EINVAL, who + b);
    }
    if (q.stream_flags & ~sknown) {
        snprintf(b, sizeof b, ": unknown stream_flags bit 0x%x", q.stream_flags & ~sknown);
        return fail(SPL_EINVAL, who + b);
    }
    if (q.o->row_len == 0) return fail(SPL_EINVAL, who + ": row_len is 0 (rows mode only: ids [n_seqs, row_len], row_len >= 1)");
    if (q.o->flags & SPL_DECODE_PAD_LEFT) return fail(SPL_EINVAL, who + ": SPL_DECODE_PAD_LEFT is refused (a step's ids are a row's first d_len[b])");
    if (q.n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    if (!q.ids && q.n_seqs) return fail(SPL_EINVAL, who + ": d_ids is null");
    if (!q.bytes && q.bytes_cap) return fail(SPL_EINVAL, who + ": d_bytes is null with bytes_capacity > 0");
    if (col_misaligned(q.bytes, 16)) return fail(SPL_EINVAL, who + ": d_bytes is not 16-byte aligned");

    Ctx* c = t->ctx[0].get();
    SPL_TRY(stream_prepare(t, c, q.n_seqs));
    StIn a{};
    a.ids = q.ids; a.len = q.len; a.fin = q.fin; a.state_in = q.state_in; a.n_seqs = q.n_seqs;
    a.row_len = q.o->row_len; a.dflags = q.o->flags; a.sflags = q.stream_flags;
    const DecTab tab = decode_dev_tab(c);
    const bool i64 = (q.o->flags & SPL_DECODE_I64) != 0;
    if (q.n_seqs <= t->stream_one_max) {
        if (i64) hipLaunchKernelGGL(k_stream_one<true>, dim3(1), dim3(ST_ONE_NT), 0, q.stream, a, tab, q.bytes, q.bytes_cap, q.out_off, q.state_out);
        else hipLaunchKernelGGL(k_stream_one<false>, dim3(1), dim3(ST_ONE_NT), 0, q.stream, a, tab, q.bytes, q.bytes_cap, q.out_off, q.state_out);
    } else {
        const uint64_t n_blk = st_n_blocks(q.n_seqs);
        const dim3 grid((uint32_t)n_blk), wg(ST_NT);             // (n_seqs < 2^31: fewer than 2^27 blocks)
        uint64_t* blk = c->d_stblk.get();
        uint64_t* cnt = blk + n_blk + 1;
        if (i64) hipLaunchKernelGGL(k_stream_len<true>, grid, wg, 0, q.stream, a, tab, n_blk, cnt, blk);
        else hipLaunchKernelGGL(k_stream_len<false>, grid, wg, 0, q.stream, a, tab, n_blk, cnt, blk);
        hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, q.stream, blk, n_blk);
        if (i64) hipLaunchKernelGGL(k_stream_write<true>, grid, wg, 0, q.stream, a, tab, n_blk, (const uint64_t*)cnt, (const uint64_t*)blk, q.bytes, q.bytes_cap, q.out_off, q.state_out);
        else hipLaunchKernelGGL(k_stream_write<false>, grid, wg, 0, q.stream, a, tab, n_blk, (const uint64_t*)cnt, (const uint64_t*)blk, q.bytes, q.bytes_cap, q.out_off, q.state_out);
    }
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
