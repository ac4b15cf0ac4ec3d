// spl_host_split.h -- custom split patterns on the host cores: special-token literals and the pattern over one document or all of them
// (host_split_doc(s), the kept worker threads), the per-document fallback behind the device splitter (rx_patch_docs), and a custom-pattern
// handle's device-text call (encode_device_custom).  Needs launch_all and rx_* (spl_launch.h).
#pragma once
namespace {

// ---- custom split patterns: the host splitter over the documents of one pipeline chunk ------------------------
// Special-token literals on the host, with the reference matcher's semantics (Aho-Corasick, MatchKind::Standard,
// non-overlapping find_iter, tokenizer.rs:849-869; the same rule k_special_select implements): from the end of the
// previous match, the occurrence that ENDS first, the longest one on a tie.
struct SpHit { uint32_t start, len, id; };
void host_special_find(const spl_tokenizer* tk, const uint8_t* text, size_t n, std::vector<SpHit>& out) {
    uint8_t last_set[32] = {0};
    for (const auto& sp : tk->specials) { const uint8_t c = (uint8_t)sp.lit.back(); last_set[c >> 3] |= (uint8_t)(1u << (c & 7)); }
    size_t last = 0;
    for (size_t e = 1; e <= n; e++) {
        const uint8_t c = text[e - 1];
        if (!((last_set[c >> 3] >> (c & 7)) & 1u)) continue;
        const Special* best = nullptr;
        for (const auto& sp : tk->specials) {
            const size_t len = sp.lit.size();
            if ((uint8_t)sp.lit.back() != c || len > e - last || (best && len <= best->lit.size())) continue;
            if (memcmp(text + e - len, sp.lit.data(), len) == 0) best = &sp;
        }
        if (!best) continue;
        out.push_back(SpHit{(uint32_t)(e - best->lit.size()), (uint32_t)best->lit.size(), best->id});
        last = e;
    }
}

inline void host_or_bit(uint32_t* bm, uint64_t pos) { __atomic_fetch_or(&bm[pos >> 5], 1u << (pos & 31), __ATOMIC_RELAXED); }

// One document [lo, hi) of `text` (positions relative to the bitmaps' origin): chunk starts and gaps; with
// `special`, the literals first -- each a gap with a start bit at either end, its token on `hits` -- and the
// pattern over the stretches between them (encode_with_special, tokenizer.rs:842-874).
bool host_split_doc(const spl_tokenizer* tk, const uint8_t* text, uint64_t lo, uint64_t hi, bool special, uint32_t* starts,
                    uint32_t* gaps, std::vector<SpHit>* hits) {
    if (hi <= lo) return true;
    if (!special) return regex_split_bits(*tk->regex, text + lo, (size_t)(hi - lo), lo, starts, gaps);
    std::vector<SpHit> found;
    host_special_find(tk, text + lo, (size_t)(hi - lo), found);
    uint64_t at = lo;
    for (const SpHit& h : found) {
        const uint64_t a = lo + h.start, e = a + h.len;
        if (a > at && !regex_split_bits(*tk->regex, text + at, (size_t)(a - at), at, starts, gaps)) return false;
        host_or_bit(starts, a);
        for (uint64_t q = a; q < e; q++) host_or_bit(gaps, q);
        if (e < hi) host_or_bit(starts, e);
        hits->push_back(SpHit{(uint32_t)a, h.len, h.id});
        at = e;
    }
    if (hi > at && !regex_split_bits(*tk->regex, text + at, (size_t)(hi - at), at, starts, gaps)) return false;
    return true;
}

// Worker threads of the host splitter, kept: a 1 MB batch is 60 pieces of 16 KiB, and starting 59 threads for it took longer
// than the matching (1.7 ms against 0.2).  One parallel-for at a time (callers queue on run_mu: every caller uses all the
// workers anyway).  Process-wide, never destroyed (the workers are detached and idle on a condition variable).
struct WorkPool {
    std::mutex run_mu, mu;
    std::condition_variable cv_work, cv_done;
    unsigned n_threads = 0, want = 0, started = 0, done = 0, gen = 0;
    const std::function<void(unsigned)>* job = nullptr;
    void loop() {
        unsigned seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv_work.wait(lk, [&] { return gen != seen && started < want; });
            seen = gen;
            const unsigned k = ++started;
            const std::function<void(unsigned)>* f = job;
            lk.unlock();
            (*f)(k);
            lk.lock();
            if (++done == want) cv_done.notify_one();
        }
    }
    void run(unsigned nt, const std::function<void(unsigned)>& fn) {      // fn(0 .. nt - 1), fn(0) on the calling thread
        if (nt <= 1) { fn(0); return; }
        std::lock_guard<std::mutex> one(run_mu);
        {
            std::unique_lock<std::mutex> lk(mu);
            while (n_threads < nt - 1) { std::thread(&WorkPool::loop, this).detach(); n_threads++; }
            job = &fn; want = nt - 1; started = 0; done = 0; gen++;
        }
        cv_work.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return done == want; });
        job = nullptr; want = 0;
    }
};
WorkPool& work_pool() { static WorkPool* p = new WorkPool(); return *p; }

// All documents of a packed text (offsets relative to `text`), on up to `max_threads` threads pulling documents
// off a shared counter.  The bitmaps must be zeroed and hold n_bytes / 32 + 2 words.
int host_split_docs(const spl_tokenizer* tk, const uint8_t* text, const uint64_t* off, uint64_t nd, bool special, uint32_t* starts,
                    uint32_t* gaps, std::vector<SpHit>* hits, unsigned max_threads) {
    const uint64_t n_bytes = nd ? off[nd] - off[0] : 0;
    unsigned nt = std::max(1u, std::min<unsigned>(max_threads, std::thread::hardware_concurrency()));
    nt = (unsigned)std::min<uint64_t>(nt, std::max<uint64_t>(1, std::min<uint64_t>(nd, n_bytes >> 14)));    // >= 16 KiB of text per thread
    std::atomic<uint64_t> next{0};
    std::atomic<int> bad{0};
    std::vector<std::vector<SpHit>> part(nt);
    const std::function<void(unsigned)> work = [&](unsigned k) {
        try {
            for (;;) {
                const uint64_t d0 = next.fetch_add(16, std::memory_order_relaxed);      // documents in runs of 16
                if (d0 >= nd || bad.load(std::memory_order_relaxed)) return;
                for (uint64_t d = d0; d < std::min(nd, d0 + 16); d++)
                    if (!host_split_doc(tk, text, off[d] - off[0], off[d + 1] - off[0], special, starts, gaps, &part[k])) { bad.store(1); return; }
            }
        } catch (...) { bad.store(2); }                                 // (std::bad_alloc on a worker: reported, never thrown across the pool)
    };
    work_pool().run(nt, work);
    if (bad.load() == 2) return fail(SPL_EDEVICE, "the host splitter ran out of memory");
    if (bad.load()) return fail(SPL_EINVAL, "the split pattern ran out of its matching budget on this text (catastrophic backtracking)");
    if (hits) {
        for (auto& p : part) hits->insert(hits->end(), p.begin(), p.end());
        std::sort(hits->begin(), hits->end(), [](const SpHit& a, const SpHit& b) { return a.start < b.start; });
    }
    return SPL_OK;
}

// ---- per-document fallback of the device splitter ------------------------------------------------------------------
// The blocks k_rx_mark left in the context's pinned list (h_rx_bad: [0] count, then per block two words: the 256-byte block, first << 8 | last position in it
// that the matcher gave up on -- a match longer than ~1 KB, a runaway attempt): the documents those stretches touch are split HERE, on the calling thread,
// and their stretch of the two device bitmaps is patched (k_rx_patch, on `s`, behind the device split whose completion the caller has
// waited for); every other document keeps what the device splitter made.  `rel[0 .. nd]`: the documents' offsets relative to the
// bitmaps' origin; text_of(d): the first byte of document d on the host.  Up to round 4 ONE such position sent the whole batch through
// the host splitter ("a 5x cliff triggered by a single base64 blob").  Reference semantics: tokenizer.rs:729-808.
template <class TextOf>
int rx_patch_docs(spl_tokenizer* tk, Ctx* c, const uint64_t* rel, uint64_t nd, bool special, uint32_t* d_starts, uint32_t* d_gaps,
                  hipStream_t s, TextOf text_of, uint64_t* n_patched) {
    const uint32_t nb = std::min<uint32_t>(c->h_rx_bad.host()[0], RX_BAD_CAP);
    std::vector<uint64_t> docs;
    for (uint32_t i = 0; i < nb; i++) {
        // the (non-empty) documents that overlap [first, last] -- the positions of the listed block at which the matcher gave up
        const uint32_t blk = c->h_rx_bad.host()[1 + 2 * i], e = c->h_rx_bad.host()[2 + 2 * i];
        const uint64_t lo = (uint64_t)blk * RXB + ((e >> 8) & 255u), hi = (uint64_t)blk * RXB + (e & 255u) + 1;
        uint64_t d = (uint64_t)(std::upper_bound(rel + 1, rel + nd + 1, lo) - (rel + 1));      // first d with rel[d + 1] > lo
        for (; d < nd && rel[d] < hi; d++)
            if (rel[d + 1] > rel[d]) docs.push_back(d);
    }
    std::sort(docs.begin(), docs.end());
    docs.erase(std::unique(docs.begin(), docs.end()), docs.end());
    *n_patched = docs.size();
    if (docs.empty()) return SPL_OK;
    std::vector<uint32_t> patch, at;
    std::vector<SpHit> hits;
    for (uint64_t d : docs) {
        const uint64_t lo = rel[d], hi = rel[d + 1];
        const uint64_t w0 = lo >> 5, n = ((hi - 1) >> 5) - w0 + 1;
        TRACE("device split gave up inside document %llu [%llu, %llu): split on the host, %llu bitmap words patched", (unsigned long long)d,
              (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)n);
        at.push_back((uint32_t)patch.size());
        const size_t h = patch.size();
        patch.resize(h + 4 + 2 * n + 2, 0u);                     // (+ 2: the bit of position hi may fall into the word behind)
        patch[h] = (uint32_t)w0; patch[h + 1] = (uint32_t)n;
        patch[h + 2] = 0xFFFFFFFFu << (lo & 31);
        patch[h + 3] = (hi & 31) ? (1u << (hi & 31)) - 1u : 0xFFFFFFFFu;
        std::vector<uint32_t> st(n + 1, 0u), gp(n + 1, 0u);
        const uint64_t lo_b = lo - w0 * 32;                      // the document's first bit in these words
        const uint8_t* base = text_of(d) - lo_b;                 // (indexed by bit position: base + lo_b is the document's first byte)
        if (!host_split_doc(tk, base, lo_b, lo_b + (hi - lo), special, st.data(), gp.data(), &hits))
            return fail(SPL_EINVAL, "the split pattern ran out of its matching budget on this text (catastrophic backtracking)");
        memcpy(&patch[h + 4], st.data(), n * 4);
        memcpy(&patch[h + 4 + n], gp.data(), n * 4);
    }
    const size_t need = patch.size() + at.size();
    SPL_TRY(c->d_rx_patch.grow(&c->rx_patch_cap, need, need + need / 2 + 1024, &s));
    // (pageable -> device, blocking: the stream's earlier work -- the device split -- is through, the patch kernel follows on it)
    HIP_TRY(hipMemcpy(c->d_rx_patch.get(), patch.data(), patch.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_rx_patch.get() + patch.size(), at.data(), at.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rx_patch, dim3((uint32_t)docs.size()), dim3(256), 0, s, d_starts, d_gaps, (const uint32_t*)c->d_rx_patch.get(),
                       (const uint32_t*)(c->d_rx_patch.get() + patch.size()));
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

// A custom-pattern handle with its text in HBM (spl_encode_batch_device / _packed): the device splitter and the tile kernel in one go,
// then ONE stream synchronisation to read the splitter's status word; when the matcher gave up (rare: a match longer than ~1 KB) the text
// goes to the host once, is split there (special-token literals included) and the encode runs again on those boundaries.
int encode_device_custom(spl_tokenizer* t, Ctx* c, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                         uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_out_off, hipStream_t s, const SlabOut* so) {
    if (n_bytes > SPL_DIRECT_MAX_BYTES) return fail(SPL_EINVAL, "spl_encode_batch_device: a custom split pattern takes at most 256 MB per device call");
    const uint64_t bw = n_bytes / 32 + 4;
    SPL_TRY(c->d_rx_bits.grow(&c->rx_bits_cap, 2 * bw, 2 * bw + bw / 2));
    ExtIn ext;
    ext.d_starts = c->d_rx_bits.get(); ext.d_gaps = c->d_rx_bits.get() + bw;
    // (every launch below is this call on these boundaries: only the part that runs differs)
    LaunchReq rq{.text = d_utf8, .n_bytes = n_bytes, .doc_off = d_doc_off, .n_docs = n_docs, .flags = flags,
                 .ids = d_ids, .ids_cap = ids_cap, .out_off = d_out_off, .stream = s, .slab = so, .ext = &ext};
    if (t->rx_device && !t->rx_image.empty()) {
        int rc = rx_ensure(t, c);
        if (rc) return rc;
        rc = rx_next_status(c, s);
        if (rc) return rc;
        ext.d_status = c->d_rx_status.get() + c->rx_slot;
        // optimistic: splitter and tile kernel go out together, ONE synchronisation to read what the splitter gave up on -- except with special
        // tokens (the literal scan's bitmap would keep the first tile pass's bits): there the splitter goes first, the tile kernel behind the check
        const bool two_phase = (flags & SPL_WITH_SPECIAL) && !t->specials.empty();
        rq.part = two_phase ? LaunchPart::Front : LaunchPart::All;
        rc = launch_all(t, c, rq);
        if (rc) return rc;
        uint32_t gave_up = 1;
        HIP_TRY(hipMemcpyAsync(&gave_up, c->d_rx_status.get() + c->rx_slot, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!gave_up && c->h_rx_bad.host()[0] == 0) {
            if (two_phase) { rq.part = LaunchPart::Tiles; rc = launch_all(t, c, rq); if (rc) return rc; HIP_TRY(hipStreamSynchronize(s)); }
            return SPL_OK;
        }
        if (!gave_up) {
            // a few documents hold something the device matcher gives up on: THEIR text comes to the host, is split there, their stretch of
            // the bitmaps is patched and the tile kernel runs again on the patched bitmaps (the device split itself is not repeated)
            std::vector<uint64_t> off(n_docs + 1);
            HIP_TRY(hipMemcpy(off.data(), d_doc_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
            std::vector<std::vector<uint8_t>> keep;
            hipError_t cerr = hipSuccess;
            auto text_of = [&](uint64_t d) -> const uint8_t* {
                keep.emplace_back((size_t)(off[d + 1] - off[d]) + 16);
                const hipError_t e = hipMemcpy(keep.back().data(), d_utf8 + off[d], (size_t)(off[d + 1] - off[d]), hipMemcpyDeviceToHost);
                if (e != hipSuccess) cerr = e;
                return keep.back().data();
            };
            uint64_t n_patched = 0;
            const bool special = (flags & SPL_WITH_SPECIAL) && !t->specials.empty();
            rc = rx_patch_docs(t, c, off.data(), n_docs, special, c->d_rx_bits.get(), c->d_rx_bits.get() + bw, s, text_of, &n_patched);
            if (rc) return rc;
            if (cerr != hipSuccess) return fail(SPL_EDEVICE, std::string("hipMemcpy: ") + hipGetErrorString(cerr));
            t->rx_fallbacks += n_patched;
            rq.part = LaunchPart::Tiles;
            rc = launch_all(t, c, rq);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(s));
            return SPL_OK;
        }
        t->rx_fallbacks += n_docs;              // the whole batch (the list of blocks overflowed, or walks that never fall into step)
        ext.d_status = nullptr;
    }
    const bool special = (flags & SPL_WITH_SPECIAL) && !t->specials.empty();
    std::vector<uint8_t> text(n_bytes + 16);
    std::vector<uint64_t> off(n_docs + 1);
    if (n_bytes) HIP_TRY(hipMemcpyAsync(text.data(), d_utf8, n_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(off.data(), d_doc_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint32_t> bits(2 * bw, 0u);
    std::vector<SpHit> hits;
    int rc = host_split_docs(t, text.data(), off.data(), n_docs, special, bits.data(), bits.data() + bw, &hits, 128);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_rx_bits.get(), bits.data(), 2 * bw * 4, hipMemcpyHostToDevice, s));
    DevBuf<uint32_t> d_hits;
    std::vector<uint32_t> hp;
    if (!hits.empty()) {
        const uint64_t n = hits.size();
        hp.resize(2 * n);
        for (uint64_t i = 0; i < n; i++) { hp[i] = hits[i].start; hp[n + i] = hits[i].id; }
        SPL_TRY(d_hits.alloc(2 * n));
        if (hipMemcpyAsync(d_hits.get(), hp.data(), n * 8, hipMemcpyHostToDevice, s) != hipSuccess) return fail(SPL_EDEVICE, "hipMemcpyAsync failed");
        ext.d_sp_pos = d_hits.get(); ext.d_sp_id = d_hits.get() + n; ext.n_sp = (uint32_t)n;
    }
    rq.part = LaunchPart::All;
    rc = launch_all(t, c, rq);
    const hipError_t se = hipStreamSynchronize(s);           // (the vectors and the list die with this frame)
    if (rc) return rc;
    if (se != hipSuccess) return fail(SPL_EDEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    return SPL_OK;
}
}  // namespace
