// spl_ngram_host.h -- the host half of spl_ngram_reserve_device / spl_ngram_draft_device (spl_k_ngram.h): the refusals (all of them before
// the device is touched), the choice of the slices, the scratch of the sliced form (Ctx::d_ngscr: 8 pairs of 8 bytes per sequence and
// slice, grow-only, shared with nothing) and the one or two launches.  A call within what was reserved neither allocates nor synchronises.
#pragma once
namespace {

static_assert(NG_I64 == SPL_NGRAM_I64 && NG_EARLIEST == SPL_NGRAM_EARLIEST && NG_MAX_N == SPL_NGRAM_MAX_N && NG_MAX_DEPTH == SPL_NGRAM_MAX_DEPTH &&
              NG_MAX_BRANCHES == SPL_NGRAM_MAX_BRANCHES && NG_MAX_CAP == SPL_NGRAM_MAX_CAP && NG_MAX_SLICES == SPL_NGRAM_MAX_SLICES,
              "spl_k_ngram.h and splintr_hip.h must agree");

// THE AUTOMATIC CHOICE of the slices (opts.slices == 0), from what the host knows -- the sequences and the capacity; the lengths live on
// the device, and a slice beyond a sequence's length leaves at once.  Set from the table of profiles/ngram_draft.txt: slicing pays only
// where one workgroup per sequence streams a long history on a GPU that is not full -- histories of 64 K ids at 4 to 256 sequences (63 us
// against 27 at 256 sequences and four slices); at 1 K and 8 K ids, and at 4 096 sequences of any length, the second launch costs more
// than it saves.  So: one slice above NG_AUTO_MAX_SEQS sequences or below two slices of NG_AUTO_MIN_SLICE ids, else enough slices of at
// least that many ids for about NG_AUTO_WORKGROUPS workgroups.  (Between 256 and 4 096 sequences and between 8 K and 64 K ids nothing
// was measured: the rule interpolates.)
constexpr uint64_t NG_AUTO_WORKGROUPS = 1024, NG_AUTO_MAX_SEQS = 512;
constexpr uint32_t NG_AUTO_MIN_SLICE = 16384;
uint32_t ngram_auto_slices(uint64_t n_seqs, uint32_t cap) {
    if (n_seqs > NG_AUTO_MAX_SEQS || cap < 2 * NG_AUTO_MIN_SLICE) return 1;
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(NG_AUTO_WORKGROUPS / n_seqs, cap / NG_AUTO_MIN_SLICE), NG_MAX_SLICES);
}

int ngram_scratch(Ctx* c, uint64_t n_seqs, uint32_t slices) {
    const uint64_t need = n_seqs * slices * NG_MAX_BRANCHES;
    return c->d_ngscr.grow(&c->ngscr_cap, need, std::max<uint64_t>(need, 64 * NG_MAX_BRANCHES));
}

int ngram_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    if (!t) return fail(SPL_EINVAL, "spl_ngram_reserve_device: null handle");
    if (max_seqs >= (1ull << 31)) return fail(SPL_EINVAL, "spl_ngram_reserve_device: max_seqs >= 2^31");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    return ngram_scratch(c, max_seqs, NG_MAX_SLICES);
}

int ngram_refuse(const std::string& who, const spl_ngram_in* in, const spl_ngram_opts* o, const spl_ngram_out* out) {
    if (!in || !o || !out) return fail(SPL_EINVAL, who + ": a null struct");
    SPL_TRY(refuse_struct_size(who, "spl_ngram_in", in->struct_size, sizeof(spl_ngram_in), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_ngram_opts", o->struct_size, sizeof(spl_ngram_opts), "the struct"));
    SPL_TRY(refuse_struct_size(who, "spl_ngram_out", out->struct_size, sizeof(spl_ngram_out), "the struct"));
    SPL_TRY(refuse_unknown_bits(who, "flag", o->flags, SPL_NGRAM_I64 | SPL_NGRAM_EARLIEST));
    if (!o->min_n || o->min_n > o->max_n || o->max_n > SPL_NGRAM_MAX_N)
        return fail(SPL_EINVAL, who + ": min_n " + std::to_string(o->min_n) + " and max_n " + std::to_string(o->max_n) + " are not 1 <= min_n <= max_n <= SPL_NGRAM_MAX_N (8)");
    if (o->depth > SPL_NGRAM_MAX_DEPTH) return fail(SPL_EINVAL, who + ": depth is " + std::to_string(o->depth) + ", above SPL_NGRAM_MAX_DEPTH (64)");
    if (!o->branches || o->branches > SPL_NGRAM_MAX_BRANCHES)
        return fail(SPL_EINVAL, who + ": branches is " + std::to_string(o->branches) + ", not in 1 .. SPL_NGRAM_MAX_BRANCHES (8)");
    if (o->branches * o->depth > SPL_DRAFT_MAX_NODES)
        return fail(SPL_EINVAL, who + ": branches * depth is " + std::to_string(o->branches * o->depth) + ", above SPL_DRAFT_MAX_NODES (64)");
    if (o->slices > SPL_NGRAM_MAX_SLICES) return fail(SPL_EINVAL, who + ": slices is " + std::to_string(o->slices) + ", above SPL_NGRAM_MAX_SLICES (32)");
    if (in->cap > SPL_NGRAM_MAX_CAP) return fail(SPL_EINVAL, who + ": cap is " + std::to_string(in->cap) + ", above SPL_NGRAM_MAX_CAP (2^24)");
    if (in->n_seqs >= (1ull << 31)) return fail(SPL_EINVAL, who + ": n_seqs >= 2^31");
    if (!in->d_hist) return fail(SPL_EINVAL, who + ": d_hist is null");
    if (!in->d_len) return fail(SPL_EINVAL, who + ": d_len is null");
    if (!out->d_len) return fail(SPL_EINVAL, who + ": the output d_len is null");
    if (!in->d_new != !in->d_new_len) return fail(SPL_EINVAL, who + ": d_new and d_new_len come together");
    if (o->depth && (!out->d_ids || !out->d_count || !out->d_match || !out->d_from)) return fail(SPL_EINVAL, who + ": d_ids, d_count, d_match or d_from is null");
    if (o->depth && o->branches > 1 && !out->d_parent) return fail(SPL_EINVAL, who + ": more than one branch without d_parent");
    const uintptr_t es = (o->flags & SPL_NGRAM_I64) ? 8 : 4;
    if (col_misaligned(in->d_hist, es) || col_misaligned(in->d_new, es) || col_misaligned(out->d_ids, es))
        return fail(SPL_EINVAL, who + ": d_hist, d_new or d_ids is not aligned to its element type (int32, or int64 with SPL_NGRAM_I64)");
    if (col_misaligned(in->d_len, 4) || col_misaligned(in->d_new_len, 4) || col_misaligned(out->d_count, 4) || col_misaligned(out->d_match, 4) ||
        col_misaligned(out->d_from, 4) || col_misaligned(out->d_parent, 4) || col_misaligned(out->d_len, 4))
        return fail(SPL_EINVAL, who + ": an int32 array is not 4-byte aligned");
    // no output may coincide with an input or with another output; d_len alone may be the input's (hist is both by its nature)
    const void* outs[] = {out->d_ids, out->d_count, out->d_match, out->d_from, out->d_parent, out->d_full, out->d_len};
    const char* on[] = {"d_ids", "d_count", "d_match", "d_from", "d_parent", "d_full", "the output d_len"};
    const void* ins[] = {in->d_hist, in->d_new, in->d_new_len, in->d_len};
    for (int i = 0; i < 7; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < (i == 6 ? 3 : 4); j++)
            if (outs[i] == ins[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with an input array");
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return fail(SPL_EINVAL, who + ": " + on[i] + " coincides with " + on[j]);
    }
    if (in->d_new) {
        const uintptr_t h0 = (uintptr_t)in->d_hist, h1 = h0 + in->n_seqs * in->cap * es, n0 = (uintptr_t)in->d_new, n1 = n0 + in->n_seqs * in->new_row_len * es;
        if (n0 < h1 && h0 < n1) return fail(SPL_EINVAL, who + ": d_new overlaps d_hist");
    }
    return SPL_OK;
}

template <int W> void ngram_launch(const NgIn& a, const NgOut& po, uint2* scr, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(k_ngram<W>, grid, dim3(NG_NT), 0, st, a, po, scr);
}

int ngram_draft_device(spl_tokenizer* t, const spl_ngram_in* in, const spl_ngram_opts* o, const spl_ngram_out* out, hipStream_t st) {
    const std::string who = "spl_ngram_draft_device";
    if (!t) return fail(SPL_EINVAL, who + ": null handle");
    SPL_TRY(ngram_refuse(who, in, o, out));
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t B = in->n_seqs;
    if (!B) return SPL_OK;
    const uint32_t es = (o->flags & SPL_NGRAM_I64) ? 8 : 4;
    NgIn a{};
    a.hist = in->d_hist; a.len = in->d_len; a.tail = in->d_new; a.tail_len = in->d_new_len; a.n_seqs = B;
    a.cap = in->cap; a.tail_row = in->new_row_len; a.flags = o->flags; a.min_n = o->min_n; a.max_n = o->max_n; a.depth = o->depth;
    a.branches = o->branches; a.pad_id = o->pad_id;
    a.slice_len = ng_slice_len(in->cap, o->slices ? o->slices : ngram_auto_slices(B, in->cap));
    a.slices = ng_slices(in->cap, a.slice_len);
    a.v4 = !col_misaligned(in->d_hist, 16) && ((uint64_t)in->cap * es) % 16 == 0 ? 1u : 0u;
    const NgOut po{out->d_ids, out->d_count, out->d_match, out->d_from, o->depth ? out->d_parent : nullptr, out->d_len, out->d_full};
    if (a.slices > 1) SPL_TRY(ngram_scratch(c, B, a.slices));
    const uint32_t gy = (uint32_t)std::min<uint64_t>(B, 65535), gz = (uint32_t)((B + gy - 1) / gy);
    const dim3 grid(a.slices, gy, gz);
    if (o->branches == 1) ngram_launch<1>(a, po, c->d_ngscr.get(), grid, st);
    else if (o->branches <= 4) ngram_launch<4>(a, po, c->d_ngscr.get(), grid, st);
    else ngram_launch<8>(a, po, c->d_ngscr.get(), grid, st);
    if (a.slices > 1) hipLaunchKernelGGL(k_ngram_emit, dim3(1, gy, gz), dim3(NG_WAVE), 0, st, a, po, (const uint2*)c->d_ngscr.get());
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

}  // namespace
