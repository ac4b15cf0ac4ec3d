// spl_stop_host.h -- the host half of spl_stop_reserve_device / spl_stop_match_device: the refusals (all of them before the handle or the
// device is touched), the scratch (Ctx::d_spblk: the block sums, the total behind them, and count, cut and hit per sequence -- 24 bytes per
// sequence and 8 per 16 of them, grow-only, shared with nothing) and the launches (spl_k_stop.h through spl_seqscan_host.h).  The
// handle gives its device and its scratch, nothing else: no table of the tokenizer is read.  A call within what was reserved neither
// allocates nor synchronises.
#pragma once
namespace {

static_assert(SP_INCLUDE == SPL_STOP_INCLUDE && SP_FINAL_ALL == SPL_STOP_FINAL_ALL, "spl_k_stop.h and splintr_hip.h must agree on the flags");
static_assert(SP_SLOTS == SPL_STOP_SLOTS && SP_MAX_LEN == SPL_STOP_MAX_LEN && SP_TABLE_BYTES == SPL_STOP_TABLE_BYTES &&
              SP_STATE_WORDS == SPL_STOP_STATE_WORDS, "spl_k_stop.h and splintr_hip.h must agree on the layout");

// one call's arguments, as the entry point received them
struct StopReq {
    const uint8_t* in = nullptr; uint64_t in_cap = 0; const uint64_t* in_off = nullptr; uint64_t n_seqs = 0;
    const uint8_t* table = nullptr; const uint64_t* mask = nullptr; const uint8_t* fin = nullptr; uint32_t flags = 0;
    const uint64_t* state_in = nullptr; uint64_t* state_out = nullptr;
    uint8_t* out = nullptr; uint64_t out_cap = 0; uint64_t* out_off = nullptr; int32_t* hit = nullptr; hipStream_t stream = nullptr;
};

int stop_prepare(Ctx* c, uint64_t max_seqs) {
    HIP_TRY(hipSetDevice(c->device));
    return seq_scratch_grow(c->d_spblk, &c->spblk_cap, max_seqs, 3);
}

int stop_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    const std::string who = "spl_stop_reserve_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (max_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": max_seqs >= 2^31");
    return stop_prepare(t->ctx[0].get(), max_seqs);
}

int stop_match_device(spl_tokenizer* t, const StopReq& q) {
    const std::string who = "spl_stop_match_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    if (!q.table) return fail(SPL_EINVAL, who + ": d_table is null");
    if (!q.state_in) return fail(SPL_EINVAL, who + ": d_state_in is null");
    if (!q.state_out) return fail(SPL_EINVAL, who + ": d_state_out is null");
    if (!q.out_off) return fail(SPL_EINVAL, who + ": d_out_off is null");
    if (!q.hit) return fail(SPL_EINVAL, who + ": d_hit is null");
    if (!q.in_off) return fail(SPL_EINVAL, who + ": d_in_off is null");
    if (!q.in && q.in_cap) return fail(SPL_EINVAL, who + ": d_in_bytes is null with in_capacity > 0");
    if (!q.out && q.out_cap) return fail(SPL_EINVAL, who + ": d_out_bytes is null with out_capacity > 0");
    if (col_misaligned(q.out, 16)) return fail(SPL_EINVAL, who + ": d_out_bytes is not 16-byte aligned");
    SPL_TRY(refuse_unknown_bits(who, "stop_flags", q.flags, SPL_STOP_INCLUDE | SPL_STOP_FINAL_ALL));
    if (q.n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");

    Ctx* c = t->ctx[0].get();
    SPL_TRY(stop_prepare(c, q.n_seqs));
    SpIn a{};
    a.in = q.in; a.in_cap = q.in_cap; a.in_off = q.in_off; a.n_seqs = q.n_seqs; a.table = q.table; a.mask = q.mask; a.fin = q.fin;
    a.flags = q.flags; a.state_in = q.state_in;
    const SeqScratch s{q.n_seqs, c->d_spblk.get()};
    const uint64_t n_blk = s.n_blk(), *cnt = s.per_seq(0), *cut = s.per_seq(1), *inf = s.per_seq(2), *blk = s.blk;
    seq_launch(s, t->stop_one_max, q.stream,
        [&] { hipLaunchKernelGGL(k_stop_one, dim3(1), dim3(SP_ONE_NT), 0, q.stream, a, q.out, q.out_cap, q.out_off, q.state_out, q.hit); },
        [&](dim3 grid, dim3 wg) { hipLaunchKernelGGL(k_stop_len, grid, wg, 0, q.stream, a, n_blk, s.per_seq(0), s.per_seq(1), s.per_seq(2), s.blk); },
        [&](dim3 grid, dim3 wg) {
            hipLaunchKernelGGL(k_stop_write, grid, wg, 0, q.stream, a, n_blk, cnt, cut, inf, blk, q.out, q.out_cap, q.out_off, q.state_out, q.hit);
        });
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
