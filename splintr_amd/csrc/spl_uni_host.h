// spl_uni_host.h -- Unigram mode, host side (the kernels: spl_k_uni.h): the check of keys and scores and the trie (uni_build, at
// spl_create; the table code is WordPiece mode's TrieBuilder), their upload and the workspace (uni_reserve), and one device call --
// k_uni_match<count>, k_uni_long<count>, k_decode_scan, k_uni_match<write>, k_uni_long<write> on the caller's stream.  The kernels read
// the caller's text and the grid comes from n_bytes: no rewrite pass and NO synchronisation.  Needs spl_wp_host.h.
#pragma once
namespace {

// Profile slots: a handle is of one mode, so a Unigram handle counts its four phases in the slots a WordPiece handle counts its four in
// (SPL_MAX_KERNELS is part of the ABI and has no four slots left); their names here are uni_phase_names (spl_kernel_name names
// WordPiece mode's).
constexpr int KI_UNI_FIRST = KI_WP_NORM_COUNT;
const char* const uni_phase_names[4] = {"k_uni_match<count>", "k_uni_long<count>+k_decode_scan", "k_uni_match<write>", "k_uni_long<write>"};

struct UniHost {
    std::vector<uint2> edges; std::vector<uint32_t> node_id; uint32_t bits = 0, max_probe = 0;
    std::vector<double> score;
    uint32_t marker_node = WP_NONE, unk_id = 0, prepend = 0;
    double unk_score = 0;
};

bool uni_utf8_ok(const uint8_t* k, uint32_t n) {
    for (uint32_t i = 0; i < n;) { uint32_t cp = 0; const uint32_t l = wp_decode(k + i, n - i, 0u, cp); if (!l) return false; i += l; }
    return true;
}

// Keys (id -> bytes: the handle's decoder table, one per line of `vocab`) and scores to the trie and the id -> score table.
int uni_build(const HostTables& ht, const double* scores, uint64_t n_scores, uint32_t unk_id, uint32_t uni_flags, UniHost& u, std::string& err) {
    const uint64_t n_keys = (uint64_t)ht.max_id + 1;
    if (!scores || n_scores != n_keys) { err = "Unigram mode: n_scores (" + std::to_string(n_scores) + ") is not the number of lines of the vocabulary (" + std::to_string(n_keys) + ")"; return 1; }
    if (unk_id >= n_keys) { err = "Unigram mode: unk_id is not an id of the vocabulary"; return 1; }
    double lo = std::numeric_limits<double>::infinity();
    for (uint64_t i = 0; i < n_keys; i++) {
        if (!std::isfinite(scores[i])) { err = "Unigram mode: the score of id " + std::to_string(i) + " is not finite"; return 1; }
        lo = std::min(lo, scores[i]);
    }
    if (lo - 10.0 >= 0.0) { err = "Unigram mode: min_score - 10 must be negative (the unk penalty would compete with the keys)"; return 1; }
    TrieBuilder tb(1);
    for (uint32_t id = 0; id <= ht.max_id; id++) {
        if (!ht.tok_present[id]) { err = "Unigram mode: id " + std::to_string(id) + " has no key"; return 1; }
        const uint8_t* k = ht.tok_bytes.data() + ht.tok_off[id];
        const uint32_t n = ht.tok_off[id + 1] - ht.tok_off[id];
        if (!uni_utf8_ok(k, n)) { err = "Unigram mode: the key of id " + std::to_string(id) + " is not well-formed UTF-8"; return 1; }
        tb.insert(0u, k, n, id);
        if (tb.node_id.size() >= (1u << 24)) { err = "Unigram mode: the vocabulary's trie has 2^24 nodes or more"; return 1; }
    }
    const uint8_t marker[3] = {0xE2, 0x96, 0x81};
    u.marker_node = tb.find(0u, marker, 3);
    tb.table(u.edges, u.bits, u.max_probe);
    u.node_id = std::move(tb.node_id);
    u.score.assign(scores, scores + n_keys);
    u.unk_id = unk_id; u.prepend = uni_flags & 1u; u.unk_score = lo - 10.0;
    return 0;
}

struct UniCtx {                                              // one GPU's share: the tables, and the workspace of uni_reserve
    DevBuf<uint32_t> node_id; DevBuf<uint2> edges; DevBuf<double> score;
    bool uploaded = false;
    DevBuf<uint64_t> cnt, lr_slot; DevBuf<uint32_t> lr_n, lr_start, lr_cnt, g_bid, g_bfrom; DevBuf<double> g_best;
    uint64_t cap_bytes = 0;
    DevBuf<uint64_t> cblk; uint64_t cblk_cap = 0;            // character spans only (spans_reserve, spl_wp_host.h)
};

// The workspace of calls of up to max_bytes of text: a count per tile, the long words' records (UNI_LREC a tile), and the long path's
// nodes -- 16 bytes per byte of text, indexed by raw position, so that no long word waits for room.
int uni_reserve(spl_tokenizer* tk, Ctx* c, uint64_t max_bytes, uint64_t /*max_docs*/) {
    if (!c->uni) c->uni = std::make_shared<UniCtx>();
    UniCtx& x = *c->uni;
    if (!x.uploaded) {
        const UniHost& u = *tk->uni;
        SPL_TRY(x.node_id.upload(u.node_id)); SPL_TRY(x.edges.upload(u.edges)); SPL_TRY(x.score.upload(u.score));
        x.uploaded = true;
    }
    if (max_bytes > x.cap_bytes || !x.cnt) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t nb = std::max(max_bytes, x.cap_bytes), nt = nb / UNI_TB + 2;
        x.cap_bytes = 0;
        SPL_TRY(x.cnt.alloc(nt + 1)); SPL_TRY(x.lr_n.alloc(nt));
        SPL_TRY(x.lr_start.alloc(nt * UNI_LREC)); SPL_TRY(x.lr_cnt.alloc(nt * UNI_LREC)); SPL_TRY(x.lr_slot.alloc(nt * UNI_LREC));
        SPL_TRY(x.g_best.alloc(nb + 2)); SPL_TRY(x.g_bid.alloc(nb + 2)); SPL_TRY(x.g_bfrom.alloc(nb + 2));
        x.cap_bytes = nb;
    }
    return SPL_OK;
}

// sr: the spans beside the ids (spl_encode_batch_spans_device) -- the two write kernels store a span per id; still no synchronisation.
int encode_device_uni_spans(spl_tokenizer* tk, Ctx* c, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                            uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_out_off, hipStream_t s, const SlabOut* so, const SpanReq* sr) {
    if ((flags & SPL_WITH_SPECIAL) && !tk->specials.empty())
        return fail(SPL_EINVAL, "Unigram mode: SPL_WITH_SPECIAL is refused on a handle with special tokens -- literals in the text are not looked for; <s> and </s> come from the pair and chat collation");
    if (n_bytes > UNI_MAX_BYTES) return fail(SPL_EINVAL, "Unigram mode: a device call takes at most 64 MiB of text (split the corpus at document boundaries -- spl_encode_batch does that by itself)");
    if (((uintptr_t)d_utf8 & 15) != 0) return fail(SPL_EINVAL, "text buffer must be 16-byte aligned");
    if (n_docs > 0xFFFFFFF0ull) return fail(SPL_EINVAL, "n_docs per device call must be < 2^32 - 16");
    if (n_bytes && !n_docs) return fail(SPL_EINVAL, "Unigram mode: text without a document");
    SPL_TRY(uni_reserve(tk, c, n_bytes, n_docs));
    UniCtx& x = *c->uni;
    const UniHost& u = *tk->uni;
    if (sr) SPL_TRY(spans_reserve(x.cblk, &x.cblk_cap, nullptr, nullptr, x.cap_bytes, sr->cspan != nullptr));
    Event ev[5];
    if (c->prof) for (auto& e : ev) SPL_TRY(e.create(hipEventDefault));
    if (!n_bytes) {                                          // (nothing to match: n_docs empty rows)
        HIP_TRY(hipMemsetAsync(d_out_off, 0, (n_docs + 1) * 8, s));
    } else {
        UniArgs a{};
        a.text = d_utf8; a.n_bytes = (uint32_t)n_bytes; a.doc_off = d_doc_off; a.n_docs = (uint32_t)n_docs;
        a.trie = WpTrie{x.edges.get(), (1u << u.bits) - 1u, 32u - u.bits, u.max_probe, x.node_id.get()};
        a.score = x.score.get(); a.marker_node = u.marker_node; a.unk_id = u.unk_id; a.prepend = u.prepend; a.unk_score = u.unk_score;
        a.cnt = x.cnt.get(); a.lr_n = x.lr_n.get(); a.lr_start = x.lr_start.get(); a.lr_cnt = x.lr_cnt.get(); a.lr_slot = x.lr_slot.get();
        a.g = UniNodes{x.g_best.get(), x.g_bid.get(), x.g_bfrom.get()};
        a.ids = d_ids; a.ids_cap = ids_cap; a.out_off = d_out_off;
        const uint32_t ntiles = (uint32_t)((n_bytes + UNI_TB - 1) / UNI_TB);
        const uint32_t nlong = std::min<uint32_t>(ntiles * UNI_LREC, 2048u);       // a grid-stride over the records: empty when none was logged
        if (c->prof) HIP_TRY(hipEventRecord(ev[0].get(), s));
        hipLaunchKernelGGL(k_uni_match<false>, dim3(ntiles), dim3(UNI_NT), 0, s, a);
        if (c->prof) HIP_TRY(hipEventRecord(ev[1].get(), s));
        hipLaunchKernelGGL(k_uni_long<false>, dim3(nlong), dim3(UNI_LB), 0, s, a, ntiles);
        hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, s, a.cnt, (uint64_t)ntiles);
        if (c->prof) HIP_TRY(hipEventRecord(ev[2].get(), s));
        if (sr) {
            if (sr->cspan) text_char_blocks(d_utf8, n_bytes, x.cblk.get(), s);
            a.so = TextSpanOut{d_utf8, d_doc_off, x.cblk.get(), sr->bspan, sr->cspan};
            hipLaunchKernelGGL((k_uni_match<true, true>), dim3(ntiles), dim3(UNI_NT), 0, s, a);
        } else hipLaunchKernelGGL(k_uni_match<true>, dim3(ntiles), dim3(UNI_NT), 0, s, a);
        if (c->prof) HIP_TRY(hipEventRecord(ev[3].get(), s));
        if (sr) hipLaunchKernelGGL((k_uni_long<true, true>), dim3(nlong), dim3(UNI_LB), 0, s, a, ntiles);
        else hipLaunchKernelGGL(k_uni_long<true>, dim3(nlong), dim3(UNI_LB), 0, s, a, ntiles);
        if (c->prof) HIP_TRY(hipEventRecord(ev[4].get(), s));
        HIP_TRY(hipGetLastError());
    }
    if (so)                                                  // the slab copy of the result, from the caller's ids as the encode path's own does
        hipLaunchKernelGGL(k_gatherv_pack, dim3(256), dim3(256), 0, s, d_ids, d_out_off, (uint32_t)n_docs, so->d_slab, (uint32_t)so->cap_words,
                           (uint32_t)so->max_docs, tk->slab_pack24 ? 1u : 0u, ids_cap);
    if (c->prof && n_bytes) {                                // (profiling is the one thing that waits)
        HIP_TRY(hipEventSynchronize(ev[4].get()));
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ev[k].get(), ev[k + 1].get()));
            c->prof_ms[KI_UNI_FIRST + k] += ms; c->prof_n[KI_UNI_FIRST + k] += 1;
        }
    }
    return SPL_OK;
}
int encode_device_uni(spl_tokenizer* tk, Ctx* c, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                      uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_out_off, hipStream_t s, const SlabOut* so) {
    return encode_device_uni_spans(tk, c, d_utf8, n_bytes, d_doc_off, n_docs, flags, d_ids, ids_cap, d_out_off, s, so, nullptr);
}
}  // namespace
