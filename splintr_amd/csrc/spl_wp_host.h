// spl_wp_host.h -- WordPiece mode, host side (the kernels: spl_k_wp.h): the check of the normalisation table and the trie (wp_build, at
// spl_create), their upload and the workspace (wp_reserve), and one device call -- count pass of the normaliser, scan, ONE synchronisation
// for the normalised length, write pass, then the matcher's count pass, scan and write pass.  Needs ensure_streams (spl_ctx.h).
// A span call (spl_encode_batch_spans_device) is the same call with the <write, map> / <write, span> variants of the two write passes and,
// for character spans, the character count of the caller's text in front of the matcher's (spans_reserve, text_char_blocks: Unigram
// mode's span call, spl_uni_host.h, uses them too).  Workspace of a span call beyond the mode's: 12 bytes per byte of text (the source
// map) and 8 bytes per 64 (the character count).
#pragma once
namespace {

constexpr int KI_WP_NORM_COUNT = KI_N + 2, KI_WP_NORM_WRITE = KI_N + 3, KI_WP_MATCH_COUNT = KI_N + 4, KI_WP_MATCH_WRITE = KI_N + 5;   // profile slots behind SentencePiece mode's
const char* const k_wp_names[4] = {"k_wp_norm<count>+k_decode_scan", "k_wp_norm<write>", "k_wp_match<count>+k_decode_scan", "k_wp_match<write>"};
static_assert(KI_WP_MATCH_WRITE < SPL_MAX_KERNELS, "profile slots");

// The handle's share of the mode: the table as the caller gave it (checked), the trie, the options.
struct WpHost {
    std::vector<uint16_t> s1; std::vector<uint32_t> s2, multi; uint32_t shift = 0;
    std::vector<uint2> edges; std::vector<uint32_t> node_id; uint32_t bits = 0, max_probe = 0;
    uint32_t unk_id = 0, max_chars = 100;
};

uint32_t wp_rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The table of splintr_amd/wordpiece.py build_norm_table.  Everything the kernels index with it is checked here, code point by code
// point: block numbers, expansion indices, and that no code point yields more than three times its own bytes (the staging of a tile and
// the factor 3 of the workspace rest on it).
int wp_load_table(const uint8_t* tab, uint64_t len, WpHost& w, std::string& err) {
    if (!tab || len < 32 || memcmp(tab, "SPLN", 4) != 0 || wp_rd32(tab + 4) != 1) { err = "bad normalisation table"; return 1; }
    const uint32_t shift = wp_rd32(tab + 8), n1 = wp_rd32(tab + 12), n2 = wp_rd32(tab + 16), nm = wp_rd32(tab + 20);
    if (shift < 4 || shift > 12 || n1 != (0x110000u >> shift) || !n2 || (n2 & ((1u << shift) - 1u)) || n2 > (1u << 24) || nm > (1u << 21)) { err = "bad normalisation table"; return 1; }
    const uint64_t at2 = 32 + 2ull * n1 + (2ull * n1 % 4 ? 2 : 0);
    if (len != at2 + 4ull * n2 + 4ull * nm) { err = "bad normalisation table (length)"; return 1; }
    w.shift = shift;
    w.s1.resize(n1); w.s2.resize(n2); w.multi.resize(nm);
    for (uint32_t i = 0; i < n1; i++) w.s1[i] = (uint16_t)(tab[32 + 2 * i] | tab[33 + 2 * i] << 8);
    for (uint32_t i = 0; i < n2; i++) w.s2[i] = wp_rd32(tab + at2 + 4ull * i);
    for (uint32_t i = 0; i < nm; i++) w.multi[i] = wp_rd32(tab + at2 + 4ull * n2 + 4ull * i);
    const WpNormTab t{w.s1.data(), w.s2.data(), w.multi.data(), shift};
    for (uint32_t cp = 0; cp < 0x110000u; cp++) {
        if (((uint32_t)w.s1[cp >> shift] + 1u) << shift > n2) { err = "bad normalisation table (block number)"; return 1; }
        const uint32_t e = wp_norm_entry(t, cp), n = e & 3u;
        if (n >= 2u && (uint64_t)(e >> 8) + n > nm) { err = "bad normalisation table (expansion index)"; return 1; }
        uint32_t bytes = 0;
        for (uint32_t k = 0; k < n; k++) bytes += wp_utf8_len(wp_norm_out(t, e, cp, k) & 0x1FFFFFu);
        if (bytes > 3u * wp_utf8_len(cp) || n > wp_utf8_len(cp)) { err = "normalisation table: a code point yields more than three times its bytes, or more code points than it has bytes"; return 1; }
    }
    return 0;
}

// A trie over byte strings in the layout the matchers probe (WpTrie, spl_k_wp.h): an open-addressing hash of (node << 8 | byte) -> child
// whose probe bound is measured at build, and node -> id.  WordPiece mode and Unigram mode (spl_uni_host.h) build theirs with it.
struct TrieBuilder {
    std::unordered_map<uint32_t, uint32_t> child;
    std::vector<uint32_t> node_id;
    explicit TrieBuilder(uint32_t roots) : node_id(roots, WP_NONE) {}
    void insert(uint32_t node, const uint8_t* k, uint32_t n, uint32_t id) {
        for (uint32_t i = 0; i < n; i++) {
            auto it = child.find(node << 8 | k[i]);
            if (it == child.end()) {
                it = child.emplace(node << 8 | k[i], (uint32_t)node_id.size()).first;
                node_id.push_back(WP_NONE);
            }
            node = it->second;
        }
        node_id[node] = id;
    }
    uint32_t find(uint32_t node, const uint8_t* k, uint32_t n) const {
        for (uint32_t i = 0; i < n && node != WP_NONE; i++) { auto it = child.find(node << 8 | k[i]); node = it == child.end() ? WP_NONE : it->second; }
        return node;
    }
    void table(std::vector<uint2>& edges, uint32_t& bits, uint32_t& max_probe) const {
        bits = 6;
        while ((1ull << bits) < 2 * child.size() + 2) bits++;
        edges.assign((size_t)1 << bits, make_uint2(WP_NONE, WP_NONE));
        max_probe = 0;
        const uint32_t mask = (1u << bits) - 1u;
        for (const auto& kv : child) {
            uint32_t h = (kv.first * 0x9E3779B1u) >> (32 - bits), k = 0;
            while (edges[(h + k) & mask].x != WP_NONE) k++;
            edges[(h + k) & mask] = make_uint2(kv.first, kv.second);
            max_probe = std::max(max_probe, k);
        }
    }
};

// The trie over the vocabulary's keys (id -> bytes: the handle's decoder table).  Node 0: the root of word-initial keys, every key as it
// is; node 1: the root of continuation keys, every key that begins with the prefix and goes on, without the prefix.
int wp_build_trie(const HostTables& ht, const std::string& prefix, WpHost& w, std::string& err) {
    TrieBuilder tb(2);
    for (uint32_t id = 0; id <= ht.max_id; id++) {
        if (!ht.tok_present[id]) continue;
        const uint8_t* k = ht.tok_bytes.data() + ht.tok_off[id];
        const uint32_t n = ht.tok_off[id + 1] - ht.tok_off[id];
        tb.insert(0u, k, n, id);
        if (n > prefix.size() && memcmp(k, prefix.data(), prefix.size()) == 0) tb.insert(1u, k + prefix.size(), n - (uint32_t)prefix.size(), id);
        if (tb.node_id.size() >= (1u << 24)) { err = "WordPiece mode: the vocabulary's trie has 2^24 nodes or more"; return 1; }
    }
    tb.table(w.edges, w.bits, w.max_probe);
    w.node_id = std::move(tb.node_id);
    return 0;
}

struct WpCtx {                                               // one GPU's share: the tables, and the workspace of wp_reserve
    DevBuf<uint16_t> s1; DevBuf<uint32_t> s2, multi, node_id; DevBuf<uint2> edges;
    bool uploaded = false;
    DevBuf<uint8_t> text, tstate; DevBuf<uint64_t> cnt, off; DevBuf<uint32_t> bits;
    uint64_t cap_bytes = 0, cap_docs = 0;
    DevBuf<uint32_t> map; DevBuf<uint64_t> cblk; uint64_t map_cap = 0, cblk_cap = 0;      // span calls only (spans_reserve)
};

// What spl_encode_batch_spans_device asks of a mode's device call beyond the encode: [ids_cap, 2] each, either may be null.
struct SpanReq { int32_t* bspan; int32_t* cspan; };

// The workspace of a span call on top of the mode's own, reserved by the first span call (and grown with the mode's): the character
// starts in front of every TS_BLK bytes of the text for character spans (8 bytes per 64 of text) and, WordPiece mode, the source map
// -- a word per byte of normalised text, 12 bytes per byte of text.
int spans_reserve(DevBuf<uint64_t>& cblk, uint64_t* cblk_cap, DevBuf<uint32_t>* map, uint64_t* map_cap, uint64_t cap_bytes, bool chars) {
    if (chars) SPL_TRY(cblk.grow(cblk_cap, cap_bytes / TS_BLK + 2, cap_bytes / TS_BLK + 2));
    if (map) SPL_TRY(map->grow(map_cap, 3 * cap_bytes + 64, 3 * cap_bytes + 64));
    return SPL_OK;
}
// cblk[i]: the character starts in text[0, TS_BLK * i), for every i up to the block that holds n_bytes.
void text_char_blocks(const uint8_t* d_utf8, uint64_t n_bytes, uint64_t* cblk, hipStream_t s) {
    const uint64_t n_blk = (n_bytes + TS_BLK - 1) / TS_BLK;
    hipLaunchKernelGGL(k_text_cstarts, dim3((uint32_t)((n_bytes + 16 * TS_NT - 1) / (16 * TS_NT))), dim3(TS_NT), 0, s, d_utf8, (uint32_t)n_bytes, cblk);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, s, cblk, n_blk);
}

// The workspace of calls of up to max_bytes of text and max_docs documents: the normalised text (three times the bytes), its word-start
// bits, a count per tile of either kernel (one array serves both, the normaliser's first), a state per tile, the normalised offsets.
int wp_reserve(spl_tokenizer* tk, Ctx* c, uint64_t max_bytes, uint64_t max_docs) {
    if (!c->wp) c->wp = std::make_shared<WpCtx>();
    WpCtx& x = *c->wp;
    if (!x.uploaded) {
        const WpHost& w = *tk->wp;
        SPL_TRY(x.s1.upload(w.s1)); SPL_TRY(x.s2.upload(w.s2)); SPL_TRY(x.multi.upload(w.multi));
        SPL_TRY(x.node_id.upload(w.node_id)); SPL_TRY(x.edges.upload(w.edges));
        x.uploaded = true;
    }
    if (max_bytes > x.cap_bytes || !x.text) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t nb = std::max(max_bytes, x.cap_bytes);
        x.cap_bytes = 0;
        SPL_TRY(x.text.alloc(3 * nb + 64));
        SPL_TRY(x.bits.alloc(3 * nb / 32 + 4));
        SPL_TRY(x.cnt.alloc(std::max(nb / WPN_TB, 3 * nb / WPM_TB) + 4));
        SPL_TRY(x.tstate.alloc(nb / WPN_TB + 4));
        x.cap_bytes = nb;
    }
    if (max_docs > x.cap_docs || !x.off) {
        HIP_TRY(hipDeviceSynchronize());
        const uint64_t nd = std::max(max_docs, x.cap_docs);
        x.cap_docs = 0;
        SPL_TRY(x.off.alloc(nd + 1));
        x.cap_docs = nd;
    }
    return SPL_OK;
}

// sr: the spans beside the ids (spl_encode_batch_spans_device) -- the normaliser's write pass leaves its source map, the matcher's stores
// a span per id; their time counts in the same profile slots.
int encode_device_wp_spans(spl_tokenizer* tk, Ctx* c, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                           uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_out_off, hipStream_t s, const SlabOut* so, const SpanReq* sr) {
    if ((flags & SPL_WITH_SPECIAL) && !tk->specials.empty())
        return fail(SPL_EINVAL, "WordPiece mode: SPL_WITH_SPECIAL is refused on a handle with special tokens -- literals in the text are not looked for; [CLS] and [SEP] come from the pair and chat collation");
    if (n_bytes > WP_MAX_BYTES) return fail(SPL_EINVAL, "WordPiece mode: a device call takes at most 64 MiB of text (split the corpus at document boundaries -- spl_encode_batch does that by itself)");
    if (((uintptr_t)d_utf8 & 15) != 0) return fail(SPL_EINVAL, "text buffer must be 16-byte aligned");
    if (n_docs > 0xFFFFFFF0ull) return fail(SPL_EINVAL, "n_docs per device call must be < 2^32 - 16");
    if (n_bytes && !n_docs) return fail(SPL_EINVAL, "WordPiece mode: text without a document");
    SPL_TRY(wp_reserve(tk, c, n_bytes, n_docs));
    WpCtx& x = *c->wp;
    const WpHost& w = *tk->wp;
    if (sr) SPL_TRY(spans_reserve(x.cblk, &x.cblk_cap, &x.map, &x.map_cap, x.cap_bytes, sr->cspan != nullptr));
    Event ev[5];
    if (c->prof) for (auto& e : ev) SPL_TRY(e.create(hipEventDefault));
    uint64_t n_out = 0;
    if (n_bytes) {
        WpNormArgs a{};
        a.text = d_utf8; a.n_bytes = (uint32_t)n_bytes; a.doc_off = d_doc_off; a.n_docs = (uint32_t)n_docs;
        a.tab = WpNormTab{x.s1.get(), x.s2.get(), x.multi.get(), w.shift};
        a.cnt = x.cnt.get(); a.tstate = x.tstate.get();
        a.out = x.text.get(); a.starts = x.bits.get(); a.out_doc_off = x.off.get(); a.map = sr ? x.map.get() : nullptr;
        const uint32_t ntiles = (uint32_t)((n_bytes + WPN_TB - 1) / WPN_TB);
        if (c->prof) HIP_TRY(hipEventRecord(ev[0].get(), s));
        hipLaunchKernelGGL(k_wp_norm<false>, dim3(ntiles), dim3(WPN_NT), 0, s, a);
        hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, s, a.cnt, (uint64_t)ntiles);
        if (c->prof) HIP_TRY(hipEventRecord(ev[1].get(), s));
        HIP_TRY(hipGetLastError());
        // the ONE synchronisation: the matcher's grid and the bitmap's length come from the normalised length
        HIP_TRY(hipMemcpyAsync(&n_out, a.cnt + ntiles, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n_out > 3 * n_bytes) return fail(SPL_EDEVICE, "WordPiece mode: the count pass reports more than three times the bytes");
        HIP_TRY(hipMemsetAsync(x.bits.get(), 0, (n_out / 32 + 4) * 4, s));
        if (sr) hipLaunchKernelGGL((k_wp_norm<true, true>), dim3(ntiles), dim3(WPN_NT), 0, s, a);
        else hipLaunchKernelGGL(k_wp_norm<true>, dim3(ntiles), dim3(WPN_NT), 0, s, a);
        if (c->prof) HIP_TRY(hipEventRecord(ev[2].get(), s));
        HIP_TRY(hipGetLastError());
    }
    if (!n_out) {                                            // (nothing to match: n_docs empty rows)
        HIP_TRY(hipMemsetAsync(d_out_off, 0, (n_docs + 1) * 8, s));
    } else {
        WpMatchArgs m{};
        m.text = x.text.get(); m.n_bytes = (uint32_t)n_out; m.starts = x.bits.get(); m.doc_off = x.off.get(); m.n_docs = (uint32_t)n_docs;
        m.trie = WpTrie{x.edges.get(), (1u << w.bits) - 1u, 32u - w.bits, w.max_probe, x.node_id.get()};
        m.unk_id = w.unk_id; m.max_chars = w.max_chars; m.halo = 4u * w.max_chars + 4u;
        m.cnt = x.cnt.get(); m.ids = d_ids; m.ids_cap = ids_cap; m.out_off = d_out_off;
        const uint32_t mtiles = (uint32_t)((n_out + WPM_TB - 1) / WPM_TB);
        hipLaunchKernelGGL(k_wp_match<false>, dim3(mtiles), dim3(WPM_NT), 0, s, m);
        hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, s, m.cnt, (uint64_t)mtiles);
        if (c->prof) HIP_TRY(hipEventRecord(ev[3].get(), s));
        if (sr) {
            if (sr->cspan) text_char_blocks(d_utf8, n_bytes, x.cblk.get(), s);
            m.map = x.map.get(); m.so = TextSpanOut{d_utf8, d_doc_off, x.cblk.get(), sr->bspan, sr->cspan};
            hipLaunchKernelGGL((k_wp_match<true, true>), dim3(mtiles), dim3(WPM_NT), 0, s, m);
        } else hipLaunchKernelGGL(k_wp_match<true>, dim3(mtiles), dim3(WPM_NT), 0, s, m);
        if (c->prof) HIP_TRY(hipEventRecord(ev[4].get(), s));
        HIP_TRY(hipGetLastError());
    }
    if (so)                                                  // the slab copy of the result, from the caller's ids as the encode path's own does
        hipLaunchKernelGGL(k_gatherv_pack, dim3(256), dim3(256), 0, s, d_ids, d_out_off, (uint32_t)n_docs, so->d_slab, (uint32_t)so->cap_words,
                           (uint32_t)so->max_docs, tk->slab_pack24 ? 1u : 0u, ids_cap);
    if (c->prof && n_out) {
        HIP_TRY(hipEventSynchronize(ev[4].get()));
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ev[k].get(), ev[k + 1].get()));
            c->prof_ms[KI_WP_NORM_COUNT + k] += ms; c->prof_n[KI_WP_NORM_COUNT + k] += 1;
        }
    }
    return SPL_OK;
}
int encode_device_wp(spl_tokenizer* tk, Ctx* c, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                     uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_out_off, hipStream_t s, const SlabOut* so) {
    return encode_device_wp_spans(tk, c, d_utf8, n_bytes, d_doc_off, n_docs, flags, d_ids, ids_cap, d_out_off, s, so, nullptr);
}
}  // namespace
