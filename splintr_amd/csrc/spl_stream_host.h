// spl_stream_host.h -- the host half of spl_stream_reserve_device / spl_stream_decode_device: the refusals (all of them before the handle or
// the device is touched), the scratch (Ctx::d_stblk: the block sums, the total behind them and one count per sequence -- 8 bytes per
// sequence and 8 per 16 of them, grow-only, shared with nothing) and the launches (spl_k_stream.h through spl_seqscan_host.h).  A call within
// what was reserved neither allocates nor synchronises.
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
    return seq_scratch_grow(c->d_stblk, &c->stblk_cap, max_seqs, 1);
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
    SPL_TRY(refuse_struct_size(who, "spl_decode_opts", q.o->struct_size, sizeof(spl_decode_opts), "the struct's three fields (12 bytes)"));
    SPL_TRY(refuse_unknown_bits(who, "flag", q.o->flags, SPL_DECODE_I64 | SPL_DECODE_PAD_LEFT | SPL_DECODE_SKIP_SPECIAL));
    SPL_TRY(refuse_unknown_bits(who, "stream_flags", q.stream_flags, SPL_STREAM_REPLACE | SPL_STREAM_FINAL_ALL));
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
    const SeqScratch s{q.n_seqs, c->d_stblk.get()};
    const uint64_t n_blk = s.n_blk(), *cnt = s.per_seq(0), *blk = s.blk;
    seq_launch(s, t->stream_one_max, q.stream,
        [&] {
            if (i64) hipLaunchKernelGGL(k_stream_one<true>, dim3(1), dim3(ST_ONE_NT), 0, q.stream, a, tab, q.bytes, q.bytes_cap, q.out_off, q.state_out);
            else hipLaunchKernelGGL(k_stream_one<false>, dim3(1), dim3(ST_ONE_NT), 0, q.stream, a, tab, q.bytes, q.bytes_cap, q.out_off, q.state_out);
        },
        [&](dim3 grid, dim3 wg) {
            if (i64) hipLaunchKernelGGL(k_stream_len<true>, grid, wg, 0, q.stream, a, tab, n_blk, s.per_seq(0), s.blk);
            else hipLaunchKernelGGL(k_stream_len<false>, grid, wg, 0, q.stream, a, tab, n_blk, s.per_seq(0), s.blk);
        },
        [&](dim3 grid, dim3 wg) {
            if (i64) hipLaunchKernelGGL(k_stream_write<true>, grid, wg, 0, q.stream, a, tab, n_blk, cnt, blk, q.bytes, q.bytes_cap, q.out_off, q.state_out);
            else hipLaunchKernelGGL(k_stream_write<false>, grid, wg, 0, q.stream, a, tab, n_blk, cnt, blk, q.bytes, q.bytes_cap, q.out_off, q.state_out);
        });
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
