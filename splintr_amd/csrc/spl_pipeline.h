// spl_pipeline.h -- spl_encode_batch's host side: lanes and chunks (lane_prepare, lane_submit), the latency path (encode_small) and
// encode_host, which runs a batch as one chunk or as producers plus a consumer.  Every device call is a LaunchReq built where it is made
// -- which form, where the offsets also go, the completion word -- and what came of it a LaunchDone: nothing is parked in the context, so
// an early return leaves nothing behind.  Needs launch_all (spl_launch.h), the host splitter and rx_patch_docs (spl_host_split.h),
// pick_stream_beside (spl_streams.h).
#pragma once
namespace {

// ------------------------------------------------------------------------------------------------
// Host pipeline.
//
// A batch is cut into LANES (one per GPU context: contiguous byte ranges of about equal size, cut at
// document boundaries or -- inside a large document -- behind a newline that is followed by an ASCII
// letter or digit, a context-free match boundary of every supported pattern, see is_sync rule (d))
// and every lane into CHUNKS of whole documents.  Per chunk: [host copy into pinned staging unless
// the caller's buffer is pinned] -> H2D on the copy stream -> kernels on the compute stream -> its
// token count back to the host.  The consumer walks the chunks in global order: as soon as a chunk's
// count is known its place in the result is known, and its ids and (rebased) offsets are copied
// straight into the pinned result on the D2H stream.  Three slots per GPU keep H2D, kernels and D2H
// of consecutive chunks in flight together.
struct Chunk {
    uint64_t lo, hi;             // byte range in the caller's text
    uint64_t dlo, dhi;           // caller's documents [dlo, dhi) have bytes in it (or start at its end, last chunk of the batch)
    bool cont;                   // the first of them started before `lo` (continuation piece: contributes no offset entry)
    uint64_t oo_at;              // first entry of its local output offsets in the lane's d_oo
};
struct Lane {
    Ctx* c = nullptr;
    uint64_t lo = 0, hi = 0;
    std::vector<Chunk> chunks;
    std::atomic<uint32_t> submitted{0};
    std::atomic<int> rc{0};
    std::string err;
    bool host_split = true;      // custom pattern: the split of this lane's chunks runs on the host cores (false: k_rx_match / k_rx_mark)
    uint64_t patched = 0;        // documents of this lane that the device splitter gave up on and the host split instead
};

bool is_pinned_host(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

bool ascii_alnum(uint8_t c) { return (c >= '0' && c <= '9') || ((c | 0x20) >= 'a' && (c | 0x20) <= 'z'); }

// documents that have bytes in [lo, hi): first and one-past-last; `last` = the batch's last range also
// takes the (empty) documents that start at its end
void doc_range(const uint64_t* doc_off, uint64_t n_docs, uint64_t lo, uint64_t hi, bool last, uint64_t& dlo, uint64_t& dhi, bool& cont) {
    // first document that starts at or after lo; if the one before it reaches beyond lo, that one is first
    const uint64_t* b = std::lower_bound(doc_off, doc_off + n_docs, lo);
    dlo = (uint64_t)(b - doc_off);
    cont = false;
    if (dlo > 0 && doc_off[dlo] > lo) { dlo--; cont = true; }        // doc_off[dlo] < lo < doc_off[dlo + 1]
    if (last) dhi = n_docs;
    else dhi = (uint64_t)(std::lower_bound(doc_off, doc_off + n_docs, hi) - doc_off);      // documents starting at hi belong to the next range
    if (dhi < dlo) dhi = dlo;
}

int lane_prepare(spl_tokenizer* tk, Lane& ln, const uint64_t* doc_off, uint64_t n_docs, bool last_lane, uint64_t chunk_target,
                 bool src_pinned) {
    Ctx* c = ln.c;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_streams(*c);
    if (rc) return rc;
    // chunks of whole documents (the lane's first and last document may be pieces)
    uint64_t dlo, dhi; bool cont;
    doc_range(doc_off, n_docs, ln.lo, ln.hi, last_lane, dlo, dhi, cont);
    auto start_of = [&](uint64_t d) { return std::max(doc_off[d], ln.lo); };
    auto end_of = [&](uint64_t d) { return std::min(doc_off[d + 1], ln.hi); };
    uint64_t max_bytes = 0, max_docs = 0, oo_words = 0;
    const uint64_t small = std::max<uint64_t>(chunk_target / 4, 512ull << 10);
    const bool ramp = tk->chunk_ramp && ln.hi - ln.lo >= 2 * chunk_target && chunk_target >= (2ull << 20);
    uint64_t d = dlo;
    do {
        Chunk ch{};
        ch.dlo = d;
        ch.lo = d < dhi ? start_of(d) : ln.lo;
        ch.cont = (d == dlo) && cont;
        uint64_t e = d;
        // (the lane's first and last chunk are a quarter of the others: what nothing overlaps is the first chunk's H2D and the
        //  last one's D2H -- 153 + 164 us of a 1.7 ms call on C3 with five equal chunks, profiles/r05_host_timeline.txt.  Round 2
        //  had measured such a ramp as no better, when a chunk cost ~80 us of host-side API work and the kernels were half as fast.)
        uint64_t lim = chunk_target;
        if (ramp && d < dhi) {
            const uint64_t rem = ln.hi - ch.lo;
            if (d == dlo) lim = small;
            else if (rem <= small + small / 2) lim = rem;
            else if (rem <= chunk_target + small) lim = rem - small;
        }
        while (e < dhi && (e == d || end_of(e) - ch.lo <= lim)) e++;
        ch.dhi = e;
        ch.hi = e > d ? end_of(e - 1) : ch.lo;
        if (e == dhi) ch.hi = ln.hi;
        if (ch.hi - ch.lo > 0x7FFF0000ull) return fail(SPL_EINVAL, "spl_encode_batch: a single document exceeds 2^31 bytes");
        ch.oo_at = oo_words;
        oo_words += (ch.dhi - ch.dlo) + 1;
        max_bytes = std::max(max_bytes, ch.hi - ch.lo);
        max_docs = std::max(max_docs, ch.dhi - ch.dlo);
        ln.chunks.push_back(ch);
        d = e;
    } while (d < dhi);
    // device staging and the lane's result buffers
    if (max_bytes > c->slot_cap_bytes || max_docs > c->slot_cap_docs || !c->d_text[0]) {
        HIP_TRY(hipDeviceSynchronize());
        c->free_slots();
        const uint64_t nb = std::max(max_bytes, c->slot_cap_bytes), nd = std::max(max_docs, c->slot_cap_docs);
        for (int i = 0; i < NSLOT; i++) {
            SPL_TRY(c->d_text[i].alloc(nb + 64));
            SPL_TRY(c->d_off[i].alloc(nd + 1));
        }
        c->slot_cap_bytes = nb; c->slot_cap_docs = nd;
    }
    const uint64_t lane_bytes = ln.hi - ln.lo;
    SPL_TRY(c->d_ids.grow(&c->ids_cap, lane_bytes + 16, lane_bytes + lane_bytes / 8 + 4096));
    SPL_TRY(c->d_oo.grow(&c->oo_cap, oo_words, oo_words + oo_words / 8 + 1024));
    for (int i = 0; i < NSLOT && (size_t)i < ln.chunks.size(); i++) {
        if (!src_pinned && !c->h_text[i].ensure(tk->pool, max_bytes + 64)) return fail(SPL_EDEVICE, "pinned staging allocation failed");
        if (!c->h_off[i].ensure(tk->pool, (max_docs + 1) * 8)) return fail(SPL_EDEVICE, "pinned staging allocation failed");
    }
    {
        if (!c->h_oo.ensure(tk->pool, oo_words * 8)) return fail(SPL_EDEVICE, "pinned staging allocation failed");
        void* dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, c->h_oo.p, 0));
        c->dh_oo = (uint64_t*)dp;
    }
    if (tk->regex) {                                         // boundary bitmaps of a chunk: starts | gaps
        const uint64_t words = 2 * (max_bytes / 32 + 4);
        if (words > c->ext_cap_words) {
            HIP_TRY(hipDeviceSynchronize());
            for (int i = 0; i < NSLOT; i++) SPL_TRY(c->d_ext[i].alloc(words));
            c->ext_cap_words = words;
        }
        for (int i = 0; i < NSLOT && (size_t)i < ln.chunks.size(); i++)
            if (!c->h_ext[i].ensure(tk->pool, words * 4)) return fail(SPL_EDEVICE, "pinned staging allocation failed");
    }
    while (c->ev_chunk.size() < ln.chunks.size()) {
        Event e;
        SPL_TRY(e.create());
        c->ev_chunk.push_back(std::move(e));
    }
    if (ln.chunks.size() >= 2 && !c->streams_picked && tk->pick_streams) {
        // the pipeline's first use on this context: copy streams that run beside the compute stream (and each other) instead of whatever
        // the runtime handed out -- a D2H of ids that shares the compute stream's pipe slows both
        HIP_TRY(hipDeviceSynchronize());
        hipStream_t d2h = nullptr, h2d = nullptr;
        double cf = 0;
        if ((rc = pick_stream_beside({c->s_cmp.get()}, &d2h, &cf))) return rc;
        TRACE("picked the D2H stream (conflict %.1f us)", cf);
        if ((rc = pick_stream_beside({c->s_cmp.get(), d2h}, &h2d, &cf))) return rc;
        TRACE("picked the H2D stream (conflict %.1f us)", cf);
        c->s_d2h.reset(d2h); c->s_h2d.reset(h2d);
        c->streams_picked = true;
    }
    // (not while per-kernel profiling is on: spl_profile_read reports this context's kernels -- with the twin it would cover every other chunk)
    if (tk->twin_streams && !tk->regex && ln.chunks.size() >= 3 && !c->prof) {
        if (!c->twin) {
            c->twin.reset(new Ctx());
            c->twin->device = c->device;
            c->twin->tables = c->tables;
            c->twin->dt = c->dt;
            if (tk->pick_streams) {
                HIP_TRY(hipDeviceSynchronize());
                double cf = 0;
                hipStream_t picked = nullptr;
                if ((rc = pick_stream_beside({c->s_cmp.get(), c->s_d2h.get(), c->s_h2d.get()}, &picked, &cf))) return rc;
                c->twin->s_cmp.reset(picked);
                TRACE("picked the twin's compute stream (conflict %.1f us)", cf);
            } else if ((rc = ensure_streams(*c->twin))) return rc;
        }
        if ((rc = reserve(c->twin.get(), max_bytes, max_docs))) return rc;
    }
    return reserve(c, max_bytes, max_docs);
}

// A batch of ONE chunk (encode_host finishes it on the compute stream itself): where the last kernel writes ids and offsets directly --
// device pointers of the pinned result; null: the lane's buffers --, whether the tile kernel reads the text where it lies, and, back,
// whether the offsets were written there.
struct Solo { uint32_t* ids = nullptr; uint64_t* off = nullptr; bool mapped = false; bool off_written = false; };

// producer: every chunk of one lane, in order (runs in the caller's thread for a single chunk: `one`)
int lane_submit(spl_tokenizer* tk, Lane& ln, const uint8_t* utf8, const uint64_t* doc_off, uint32_t flags, bool src_pinned, Solo* one = nullptr) {
    Ctx* c = ln.c;
    const bool solo = one != nullptr, mapped = solo && one->mapped;
    uint32_t* const ids_direct = solo ? one->ids : nullptr;
    HIP_TRY(hipSetDevice(c->device));
    for (size_t k = 0; k < ln.chunks.size(); k++) {
        const Chunk& ch = ln.chunks[k];
        const int sl = (int)(k % NSLOT);
        Ctx* const w = (!solo && c->twin && !c->prof && (k & 1)) ? c->twin.get() : c;     // whose workspace and compute stream run this chunk's kernels
        const uint64_t nb = ch.hi - ch.lo, nd = ch.dhi - ch.dlo;
        TRACE("submit dev %d chunk %zu/%zu bytes %llu docs %llu", c->device, k, ln.chunks.size(), (unsigned long long)nb, (unsigned long long)nd);
        if (k >= NSLOT) HIP_TRY(hipEventSynchronize(c->ev_h2d[sl].get()));     // the slot's pinned staging has been read
        uint64_t* rel = (uint64_t*)c->h_off[sl].p;               // the chunk's documents, clipped to its byte range
        for (uint64_t i = 0; i < nd; i++) rel[i] = std::min(std::max(doc_off[ch.dlo + i], ch.lo), ch.hi) - ch.lo;
        rel[nd] = nb;
        const uint8_t* src = utf8 + ch.lo;
        if (!src_pinned && nb) {
            // pageable text into pinned staging: one core copies ~20 GB/s, less than the pipeline behind it takes -- a few of the pool's threads
            uint8_t* const dst = (uint8_t*)c->h_text[sl].p;
            const unsigned nt = tk->copy_threads > 1 && nb >= (2ull << 20) ? (unsigned)std::min<uint64_t>(std::min<unsigned>((unsigned)tk->copy_threads, std::max(1u, std::thread::hardware_concurrency())), nb >> 19) : 1u;
            if (nt <= 1) memcpy(dst, src, nb);
            else {
                const uint64_t part = ((nb + nt - 1) / nt + 4095) & ~4095ull;
                const std::function<void(unsigned)> cp = [&](unsigned q) {
                    const uint64_t a = std::min<uint64_t>(nb, q * part), e = std::min<uint64_t>(nb, a + part);
                    if (e > a) memcpy(dst + a, src + a, e - a);
                };
                work_pool().run(nt, cp);
            }
            src = dst;
        }
        if (k >= NSLOT) HIP_TRY(hipStreamWaitEvent(c->s_h2d.get(), c->ev_cmp[sl].get(), 0));   // the slot's device text has been consumed
        // (a batch of ONE chunk has nothing to overlap: its copies go on the compute stream, no event in between)
        hipStream_t hs = solo ? c->s_cmp.get() : c->s_h2d.get();
        // ("direct_read": the one chunk of a batch whose text is pinned is not copied at all -- the tile kernel reads text and offsets over PCIe)
        const uint8_t* text_arg = c->d_text[sl].get();
        const uint64_t* off_arg = c->d_off[sl].get();
        bool no_fuse = false;
        if (mapped && nb) {
            void *tp = nullptr, *op = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&tp, (void*)src, 0));
            HIP_TRY(hipHostGetDevicePointer(&op, rel, 0));
            text_arg = (const uint8_t*)tp; off_arg = (const uint64_t*)op;
            // (text that arrives over PCIe while the kernel runs: the tiles of the fused mode would wait for the last of it, polling -- 94 against 86 us
            //  per 1 MB call; with the text copied first it is 92 fused against 95.  profiles/r06_surface_bisect.txt)
            no_fuse = true;
        } else {
        if (nb) HIP_TRY(hipMemcpyAsync(c->d_text[sl].get(), src, nb, hipMemcpyHostToDevice, hs));
        HIP_TRY(hipMemcpyAsync(c->d_off[sl].get(), rel, (nd + 1) * 8, hipMemcpyHostToDevice, hs));
        }
        if (!solo) {
            HIP_TRY(hipEventRecord(c->ev_h2d[sl].get(), c->s_h2d.get()));
            HIP_TRY(hipStreamWaitEvent(w->s_cmp.get(), c->ev_h2d[sl].get(), 0));
        }
        uint64_t* oo = c->d_oo.get() + ch.oo_at;
        c->solo_text = text_arg; c->solo_off = off_arg;          // (a one-chunk batch: where its tile kernel read text and offsets -- the per-document redo reads them again)
        ExtIn ext;
        if (tk->regex) {
            // custom pattern: the chunk's boundaries from the host splitter (this lane's producer thread plus helpers,
            // while the previous chunks are on the GPU), uploaded behind the text
            const uint64_t bw = nb / 32 + 4;
            ext.d_starts = c->d_ext[sl].get(); ext.d_gaps = c->d_ext[sl].get() + bw;
            const bool special = (flags & SPL_WITH_SPECIAL) && !tk->specials.empty();
            std::vector<SpHit> hits;
            if (!ln.host_split) {
                // ... or from the device splitter, on the compute stream behind the text's arrival; what it gives up on is
                // on the context's status word when the batch is done (encode_host then runs the batch again, split on the host)
                ext.d_status = c->d_rx_status.get() + c->rx_slot;    // (launch_all runs the splitter, behind the special-token scan)
                ext.d_status_host = c->h_rx_status.dev();           // (k_rx_mark leaves what was given up on in the pinned word: no copy back)
            } else {
            uint32_t* hb = (uint32_t*)c->h_ext[sl].p;
            memset(hb, 0, 2 * bw * 4);
            int rcs = host_split_docs(tk, utf8 + ch.lo, rel, nd, special, hb, hb + bw, &hits, 128);
            if (rcs) return rcs;
            HIP_TRY(hipMemcpyAsync(c->d_ext[sl].get(), hb, 2 * bw * 4, hipMemcpyHostToDevice, hs));
            }
            if (!hits.empty()) {
                const uint64_t n = hits.size();
                if (n > c->extsp_cap) {
                    HIP_TRY(hipDeviceSynchronize());
                    const uint64_t cap = n + n / 2 + 1024;
                    for (int i = 0; i < NSLOT; i++) SPL_TRY(c->d_extsp[i].alloc(2 * cap));
                    c->extsp_cap = cap;
                }
                if (!c->h_extsp[sl].ensure(tk->pool, c->extsp_cap * 8)) return fail(SPL_EDEVICE, "pinned staging allocation failed");
                uint32_t* hp = (uint32_t*)c->h_extsp[sl].p;
                for (uint64_t i = 0; i < n; i++) { hp[i] = hits[i].start; hp[n + i] = hits[i].id; }
                HIP_TRY(hipMemcpyAsync(c->d_extsp[sl].get(), hp, n * 8, hipMemcpyHostToDevice, hs));
                ext.d_sp_pos = c->d_extsp[sl].get(); ext.d_sp_id = c->d_extsp[sl].get() + n; ext.n_sp = (uint32_t)n;
            }
            if (!solo) {                                         // (the bitmaps went out behind the text's event: a second one)
                HIP_TRY(hipEventRecord(c->ev_h2d[sl].get(), c->s_h2d.get()));
                HIP_TRY(hipStreamWaitEvent(c->s_cmp.get(), c->ev_h2d[sl].get(), 0));
            }
        }
        int rc;
        const bool sp_flag = (flags & SPL_WITH_SPECIAL) && !tk->specials.empty();
        // (the offsets also go where the host reads them: a pipeline chunk's into the lane's pinned h_oo, the one chunk's into the result)
        LaunchReq rq{.text = text_arg, .n_bytes = nb, .doc_off = off_arg, .n_docs = nd, .flags = flags,
                     .ids = ids_direct ? ids_direct : c->d_ids.get() + (ch.lo - ln.lo), .ids_cap = nb + 16, .out_off = oo, .stream = w->s_cmp.get(),
                     .ext = tk->regex ? &ext : nullptr, .no_fuse = no_fuse, .off_host = solo ? one->off : c->dh_oo + ch.oo_at};
        LaunchDone done;
        if (tk->regex && !ln.host_split && (!solo || sp_flag)) {
            // (a one-chunk batch runs optimistically instead -- splitter and tile kernel out together, one more tile pass if a document needs
            //  it: encode_host --, except with special tokens: the first tile pass would leave token bits in the bitmap the literal scan has
            //  written, which only a fill per call clears)
            // device split of a pipeline chunk, per-document fallback: the splitter first; the producer waits for it (the GPU has the
            // previous chunk's tile kernel to run meanwhile), has the documents of the listed blocks split on the host -- normally none --
            // and their bits patched, then the tile kernel follows
            // (a custom pattern has no twin: w is c here)
            rq.part = LaunchPart::Front;
            rc = launch_all(tk, c, rq);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(c->ev_split.get(), c->s_cmp.get()));
            HIP_TRY(hipEventSynchronize(c->ev_split.get()));
            if (c->h_rx_status.host()[0] == 0 && c->h_rx_bad.host()[0] != 0) {
                const uint64_t bw = nb / 32 + 4;
                const uint8_t* const ctext = utf8 + ch.lo;
                uint64_t n_patched = 0;
                rc = rx_patch_docs(tk, c, rel, nd, (flags & SPL_WITH_SPECIAL) && !tk->specials.empty(), c->d_ext[sl].get(), c->d_ext[sl].get() + bw, c->s_cmp.get(),
                                   [&](uint64_t d) { return ctext + rel[d]; }, &n_patched);
                if (rc) return rc;
                ln.patched += n_patched;
                c->h_rx_bad.host()[0] = 0;                          // (dealt with: the one-chunk caller looks at it again)
            }
            rq.part = LaunchPart::Tiles;
            rc = launch_all(tk, c, rq, &done);
        } else
            rc = launch_all(tk, w, rq, &done);
        if (rc) return rc;
        if (solo) { one->off_written = done.off_host_written; break; }      // (the batch is ONE chunk: the caller finishes on the compute stream itself)
        HIP_TRY(hipEventRecord(c->ev_cmp[sl].get(), w->s_cmp.get()));
        // (the chunk's local offsets -- the last one is its token count -- are in pinned memory when the event fires: k_tile_out has written
        //  them there beside the device copy; up to round 4 an 8-byte copy fetched the count, a kernel rebased the offsets on the device and
        //  a second copy brought them back: three small operations and their launch gaps per chunk on the streams the kernels wait behind)
        if (!done.off_host_written) HIP_TRY(hipMemcpyAsync((uint64_t*)c->h_oo.p + ch.oo_at, oo, (nd + 1) * 8, hipMemcpyDeviceToHost, w->s_cmp.get()));
        HIP_TRY(hipEventRecord(c->ev_chunk[k].get(), w->s_cmp.get()));
        ln.submitted.store((uint32_t)k + 1, std::memory_order_release);
    }
    return SPL_OK;
}

// ---- the latency path: a batch of a few KB (Tokenizer.encode(text), src/python/bindings.rs:254-256 -> tokenizer.rs:729-808) ----------
// A 1 KB text through the pipeline below cost 47 us, of which the tile kernel's chain of phases is 17: two H2D copies (text, offsets), two
// launches, a stream synchronisation and ~10 us of host-side set-up around them.  Here: the text and its offsets are copied by the CPU
// into ONE small pinned buffer that the tile kernel reads where it lies (over PCIe: a handful of cache lines), k_tile_out writes ids and
// offsets straight into the pinned result and -- its last workgroup, behind a system-scope fence -- a completion word the host spins on.
// No copy engine, no event, no hipStreamSynchronize (every 256th call synchronises the stream so that the runtime retires its signals).
constexpr uint64_t SMALL_MAX_BYTES = 4096, SMALL_MAX_DOCS = 256;
constexpr size_t SMALL_TEXT = SMALL_MAX_BYTES + 64, SMALL_OFF = (SMALL_MAX_DOCS + 1) * 8;
void* dev_ptr_cached(Ctx* c, void* host) {
    for (int i = 0; i < 2; i++) if (c->dp_host[i] == host) return c->dp_dev[i];
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    c->dp_host[1] = c->dp_host[0]; c->dp_dev[1] = c->dp_dev[0];
    c->dp_host[0] = host; c->dp_dev[0] = d;
    return d;
}
int encode_small(spl_tokenizer* tk, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, spl_result* r) {
    Ctx* c = tk->ctx[0].get();
    const uint64_t n_bytes = doc_off[n_docs];
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_streams(*c);
    if (rc) return rc;
    if (!c->h_small) SPL_TRY(c->h_small.alloc(SMALL_TEXT + SMALL_OFF + 64, hipHostMallocPortable | hipHostMallocCoherent | hipHostMallocMapped));   // (coherent: the completion word must become visible while the kernel runs)
    volatile uint32_t* const done = (volatile uint32_t*)(c->h_small.host() + SMALL_TEXT + SMALL_OFF);
    memcpy(c->h_small.host(), utf8, n_bytes);
    memcpy(c->h_small.host() + SMALL_TEXT, doc_off, (n_docs + 1) * 8);
    if ((rc = reserve(c, std::max<uint64_t>(n_bytes, SMALL_MAX_BYTES), std::max<uint64_t>(n_docs, SMALL_MAX_DOCS)))) return rc;
    SPL_TRY(c->d_oo.grow(&c->oo_cap, n_docs + 1, SMALL_MAX_DOCS + 1 + 1024));
    r->pool = tk->pool;
    r->n_docs = n_docs;
    r->off = (uint64_t*)tk->pool->get((n_docs + 1) * 8, r->off_cap);
    r->ids = (uint32_t*)tk->pool->get((n_bytes + 16) * 4, r->ids_cap);      // (tokens <= bytes: the kernel writes into it directly)
    if (!r->off || !r->ids) return fail(SPL_EDEVICE, "pinned result allocation failed");
    uint32_t* const d_ids = (uint32_t*)dev_ptr_cached(c, r->ids);
    uint64_t* const d_off = (uint64_t*)dev_ptr_cached(c, r->off);
    if (!d_ids || !d_off) return fail(SPL_EDEVICE, "hipHostGetDevicePointer failed");
    c->done_seq = c->done_seq + 1u ? c->done_seq + 1u : 1u;                  // (never 0: the word's resting value)
    LaunchDone ld;
    rc = launch_all(tk, c, {.text = c->h_small.dev(), .n_bytes = n_bytes, .doc_off = (const uint64_t*)(c->h_small.dev() + SMALL_TEXT), .n_docs = n_docs, .flags = flags,
                            .ids = d_ids, .ids_cap = n_bytes + 16, .out_off = c->d_oo.get(), .stream = c->s_cmp.get(), .off_host = d_off,
                            .done_word = (uint32_t*)(c->h_small.dev() + SMALL_TEXT + SMALL_OFF), .done_seq = c->done_seq}, &ld);
    if (rc) return rc;
    const bool armed = ld.done_armed, offs = ld.off_host_written;
    if (!offs) HIP_TRY(hipMemcpyAsync(r->off, c->d_oo.get(), (n_docs + 1) * 8, hipMemcpyDeviceToHost, c->s_cmp.get()));
    bool seen = false;
    if (armed && offs) {
        // (a call normally completes in 25-40 us; a GPU that is busy with other work may take longer: after ~2 ms the stream is synchronised instead)
        const uint32_t want = c->done_seq;
        for (uint32_t spin = 0; spin < 400000u; spin++) {
            if (*done == want) { seen = true; break; }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#else
            std::this_thread::yield();
#endif
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen || (++c->small_calls & 255u) == 0u) HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));
    r->n_tokens = r->off[n_docs];
    return SPL_OK;
}

int encode_host(spl_tokenizer* tk, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, spl_result* r,
                bool host_split = true) {
    HT_T(ht0);
    const uint64_t n_bytes = doc_off[n_docs];
    const bool src_pinned = is_pinned_host(utf8);
    HT_T(hta);
    HT_ACC(3, ht0, hta);
    // ---- lanes ----------------------------------------------------------------------------------
    const size_t nl_max = tk->ctx.size();
    size_t nl = nl_max;
    if (n_bytes < (1ull << 20) * nl) nl = std::max<size_t>(1, (size_t)(n_bytes >> 20));      // at least 1 MiB per GPU
    std::vector<Lane> lanes(nl);
    const bool may_cut = tk->subdoc && !tk->regex && !((flags & SPL_WITH_SPECIAL) && tk->special_newline);   // (a custom pattern's context-free boundaries are unknown)
    {
        uint64_t prev = 0;
        for (size_t l = 0; l < nl; l++) {
            lanes[l].c = tk->ctx[l].get();
            lanes[l].host_split = host_split;
            lanes[l].lo = prev;
            uint64_t cutp = n_bytes;
            if (l + 1 < nl) {
                const uint64_t target = n_bytes / nl * (l + 1), tol = n_bytes / nl / 16;
                const uint64_t* b = std::lower_bound(doc_off, doc_off + n_docs + 1, target);
                const uint64_t after = *b, before = b > doc_off ? *(b - 1) : 0;
                const uint64_t nearest = (target - before <= after - target) ? before : after;
                cutp = nearest;
                const uint64_t dist = nearest > target ? nearest - target : target - nearest;
                if (dist > tol && may_cut && before < target && target < after) {
                    // inside one large document: the first newline + ASCII letter / digit at or after the target
                    const uint64_t lim = std::min<uint64_t>(after, target + (1ull << 20));
                    for (uint64_t i = std::max<uint64_t>(target, before + 1); i < lim; i++)
                        if (utf8[i - 1] == '\n' && ascii_alnum(utf8[i])) { cutp = i; break; }
                }
                if (cutp < prev) cutp = prev;
            }
            lanes[l].hi = cutp;
            prev = cutp;
        }
    }
    const uint64_t lane_max = [&] { uint64_t m = 0; for (auto& ln : lanes) m = std::max(m, ln.hi - ln.lo); return m; }();
    uint64_t chunk_target = tk->chunk_bytes;
    if (lane_max <= tk->single_max) chunk_target = std::max<uint64_t>(tk->single_max, 1);
    else chunk_target = std::min<uint64_t>(tk->chunk_bytes, std::max<uint64_t>(lane_max / 4, 1ull << 20));
    if (tk->chunk_bytes < tk->single_max) chunk_target = tk->chunk_bytes;                 // (tests: force small chunks)
    for (size_t l = 0; l < nl; l++) {
        int rc = lane_prepare(tk, lanes[l], doc_off, n_docs, l + 1 == nl, chunk_target, src_pinned);
        if (rc) return rc;
    }
    size_t n_chunks = 0;
    for (auto& ln : lanes) n_chunks += ln.chunks.size();
    HT_T(htb);
    HT_ACC(4, hta, htb);
    TRACE("encode_host: %llu bytes %llu docs, %zu lane(s), %zu chunk(s), target %llu, pinned src %d", (unsigned long long)n_bytes,
          (unsigned long long)n_docs, nl, n_chunks, (unsigned long long)chunk_target, (int)src_pinned);

    // ---- result buffers -------------------------------------------------------------------------------
    r->pool = tk->pool;
    r->n_docs = n_docs;
    r->off = (uint64_t*)tk->pool->get((n_docs + 1) * 8, r->off_cap);
    uint64_t est = (tk->est_div == 2 ? n_bytes * 3 / 8 : n_bytes / std::max<uint32_t>(tk->est_div, 1)) + 4096;   // default: 0.375 tokens per byte
    if (est > n_bytes) est = n_bytes;
    r->ids = (uint32_t*)tk->pool->get((est + 16) * 4, r->ids_cap);
    if (!r->off || !r->ids) return fail(SPL_EDEVICE, "pinned result allocation failed");

    // ---- one chunk: everything on the compute stream ---------------------------------------------------
    HT_T(ht1);
    HT_ACC(0, ht0, ht1);
    if (n_chunks == 1) {
        Lane& ln = lanes[0];
        Ctx* c = ln.c;
        const Chunk& ch = ln.chunks[0];
        const uint64_t nd = ch.dhi - ch.dlo;                          // == n_docs
        if (tk->direct_write && n_bytes) {
            // the encoder's last kernel writes the ids straight into the pinned result over PCIe (posted,
            // coalesced writes that overlap the kernel itself): no D2H copy of the ids, ONE synchronisation.
            // The result must hold the worst case, one token per byte (the pool recycles it).
            if (r->ids_cap < (n_bytes + 16) * 4) {
                tk->pool->put(r->ids, r->ids_cap);
                r->ids = (uint32_t*)tk->pool->get((n_bytes + 16) * 4, r->ids_cap);
                if (!r->ids) return fail(SPL_EDEVICE, "pinned result allocation failed");
            }
            void* dptr = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&dptr, r->ids, 0));
            // ... and the offsets into the pinned result as well: no copy back at all
            void* optr = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&optr, r->off, 0));
            // (not with a custom pattern: the device splitter's kernels read the text as well -- in place it would cross PCIe two or three times:
            //  216 against 182 us per 1 MB call, profiles/r06_surface_bisect.txt; round 5 had it on: the 5.50 -> 4.99 GB/s of VERDICT r05)
            const bool mapped = tk->direct_read && src_pinned && ((uintptr_t)(utf8 + ch.lo) & 15) == 0 && !tk->regex;
            // (completion by k_tile_out's word in pinned memory instead of the stream synchronisation -- what the latency path does for a handful of
            //  tiles -- was measured here too: 150 us against 93 for the 1 MB batch; 1250 workgroups each pay a system-scope fence.  Not adopted.)
            Solo one{.ids = (uint32_t*)dptr, .off = (uint64_t*)optr, .mapped = mapped};
            int rc = lane_submit(tk, ln, utf8, doc_off, flags, src_pinned, &one);
            if (rc) return rc;
            if (!one.off_written) HIP_TRY(hipMemcpyAsync(r->off, c->d_oo.get() + ch.oo_at, (nd + 1) * 8, hipMemcpyDeviceToHost, c->s_cmp.get()));
            HT_T(ht2);
            HT_ACC(1, ht1, ht2);
            HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));
            if (tk->regex && !ln.host_split && c->h_rx_status.host()[0] == 0 && c->h_rx_bad.host()[0] != 0) {
                // the device splitter gave up on a few documents (optimistic run: splitter and tile kernel went out together): split those
                // on the host, patch their bits, and run the tile kernel once more on the patched bitmaps -- its results overwrite the first run's
                const uint64_t nb = ch.hi - ch.lo, bw = nb / 32 + 4;
                const uint64_t* const rel = (const uint64_t*)c->h_off[0].p;
                const uint8_t* const ctext = utf8 + ch.lo;
                uint64_t n_patched = 0;
                rc = rx_patch_docs(tk, c, rel, nd, (flags & SPL_WITH_SPECIAL) && !tk->specials.empty(), c->d_ext[0].get(), c->d_ext[0].get() + bw, c->s_cmp.get(),
                                   [&](uint64_t d) { return ctext + rel[d]; }, &n_patched);
                if (rc) return rc;
                ExtIn ext;
                ext.d_starts = c->d_ext[0].get(); ext.d_gaps = c->d_ext[0].get() + bw;
                ext.d_status = c->d_rx_status.get() + c->rx_slot; ext.d_status_host = c->h_rx_status.dev();
                rc = launch_all(tk, c, {.text = c->solo_text, .n_bytes = nb, .doc_off = c->solo_off, .n_docs = nd, .flags = flags,
                                        .ids = (uint32_t*)dptr, .ids_cap = nb + 16, .out_off = c->d_oo.get() + ch.oo_at, .stream = c->s_cmp.get(),
                                        .ext = &ext, .part = LaunchPart::Tiles, .off_host = (uint64_t*)optr});
                if (rc) return rc;
                HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));
                ln.patched = n_patched;
            }
            if (ln.patched) { tk->rx_fallbacks += ln.patched; ln.patched = 0; }     // (a one-chunk batch WITH special tokens: patched inside lane_submit)
            HT_T(ht3);
            HT_ACC(2, ht2, ht3);
#ifdef SPL_HOST_TIMING
            if (++g_htn % 256 == 0) {
                fprintf(stderr, "[spl host timing] setup %.1f us (pinned? %.1f, lanes %.1f), submit %.1f us, sync wait %.1f us (avg of 256 calls)\n", g_ht[0] / 256, g_ht[3] / 256, g_ht[4] / 256, g_ht[1] / 256, g_ht[2] / 256);
                for (auto& x : g_ht) x = 0;
            }
#endif
            r->n_tokens = r->off[nd];
            return SPL_OK;
        }
        // ids copied back speculatively (a guess of their number), the rest -- if any -- after the count is known
        Solo one;
        int rc = lane_submit(tk, ln, utf8, doc_off, flags, src_pinned, &one);
        if (rc) return rc;
        const uint64_t spec = std::min<uint64_t>(r->ids_cap / 4, n_bytes);
        HIP_TRY(hipMemcpyAsync(r->off, c->d_oo.get() + ch.oo_at, (nd + 1) * 8, hipMemcpyDeviceToHost, c->s_cmp.get()));
        if (spec) HIP_TRY(hipMemcpyAsync(r->ids, c->d_ids.get(), spec * 4, hipMemcpyDeviceToHost, c->s_cmp.get()));
        HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));
        // ("direct_write" 0: this path has no second tile pass to give -- documents the device matcher gave up on send the batch through the
        //  host splitter as a whole, as a status word would)
        if (tk->regex && !ln.host_split && c->h_rx_bad.host()[0] != 0) c->h_rx_status.host()[0] |= RXS_REACH;
        const uint64_t T = r->off[nd];
        if (T > spec) {                                                // the guess was too small: a bigger buffer, the rest
            size_t ncap = 0;
            uint32_t* nids = (uint32_t*)tk->pool->get((T + 16) * 4, ncap);
            if (!nids) return fail(SPL_EDEVICE, "pinned result allocation failed");
            memcpy(nids, r->ids, spec * 4);
            tk->pool->put(r->ids, r->ids_cap);
            r->ids = nids; r->ids_cap = ncap;
            HIP_TRY(hipMemcpyAsync(r->ids + spec, c->d_ids.get() + spec, (T - spec) * 4, hipMemcpyDeviceToHost, c->s_cmp.get()));
            HIP_TRY(hipStreamSynchronize(c->s_cmp.get()));
        }
        r->n_tokens = T;
        return SPL_OK;
    }

    // ---- several chunks: a producer thread per lane, this thread places the results ------------------
    // (Tried for one GPU and dropped: "streamed" chunks -- the running token count kept on the device, every
    //  chunk's last kernel writing ids and offsets straight to their place in the pinned result, no per-chunk
    //  synchronisation, copies or second thread.  Bit-exact, but 12.5 GB/s against 15.8 on C3 (13.1 / 16.6 on C4):
    //  50 MB of ids stored over PCIe by the kernel serialise with the next chunk's kernels on the one stream,
    //  where the D2H copy engine overlaps them.  The one-chunk case above keeps the direct write: there is
    //  nothing to overlap with.)
    std::vector<std::thread> producers;
    struct Joiner {                                         // whatever happens below, no producer outlives the lanes
        std::vector<std::thread>& v;
        ~Joiner() { for (auto& th : v) if (th.joinable()) th.join(); }
    } joiner{producers};
    for (size_t l = 0; l < nl; l++) {
        Lane* ln = &lanes[l];
        producers.emplace_back([=] {
            g_err.clear();
            int rc = lane_submit(tk, *ln, utf8, doc_off, flags, src_pinned);
            if (rc) { ln->err = g_err; ln->rc.store(rc, std::memory_order_release); }
        });
    }
    int rc_all = SPL_OK;
    std::string err_all;
    uint64_t base = 0;
    std::vector<hsa_signal_t> dma_sigs;
    struct SigGuard { std::vector<hsa_signal_t>& v; ~SigGuard() { for (hsa_signal_t sg : v) { hsa_dma().SignalWait(sg, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED); hsa_dma().SignalDestroy(sg); } } } sig_guard{dma_sigs};
    auto consume = [&]() -> int {
        for (size_t l = 0; l < nl; l++) {
            Lane& ln = lanes[l];
            Ctx* c = ln.c;
            HIP_TRY(hipSetDevice(c->device));
            const uint64_t* const h_oo = (const uint64_t*)c->h_oo.p;
            for (size_t k = 0; k < ln.chunks.size(); k++) {
                while (ln.submitted.load(std::memory_order_acquire) <= k) {
                    if (ln.rc.load(std::memory_order_acquire)) return fail(ln.rc.load(), ln.err);
                    std::this_thread::yield();
                }
                HIP_TRY(hipEventSynchronize(c->ev_chunk[k].get()));
                TRACE("chunk %zu event", k);
                const Chunk& ch = ln.chunks[k];
                const uint64_t nd = ch.dhi - ch.dlo, T = h_oo[ch.oo_at + nd];
                TRACE("place lane %zu chunk %zu tokens %llu base %llu", l, k, (unsigned long long)T, (unsigned long long)base);
                if ((base + T + 16) * 4 > r->ids_cap) {
                    // the first guess was too small: move to a buffer that holds whatever may still come
                    for (size_t q = 0; q <= l; q++) { HIP_TRY(hipSetDevice(lanes[q].c->device)); HIP_TRY(hipStreamSynchronize(lanes[q].c->s_d2h.get())); }
                    // (sdma_d2h: the copies queued so far write into the OLD buffer -- they must have landed before it is copied and handed back)
                    for (hsa_signal_t sg : dma_sigs) { hsa_dma().SignalWait(sg, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED); hsa_dma().SignalDestroy(sg); }
                    dma_sigs.clear();
                    HIP_TRY(hipSetDevice(c->device));
                    const uint64_t rest = n_bytes - ch.lo;              // tokens <= bytes
                    size_t ncap = 0;
                    uint32_t* nids = (uint32_t*)tk->pool->get((base + rest + 16) * 4, ncap);
                    if (!nids) return fail(SPL_EDEVICE, "pinned result allocation failed");
                    memcpy(nids, r->ids, base * 4);
                    tk->pool->put(r->ids, r->ids_cap);
                    r->ids = nids; r->ids_cap = ncap;
                }
                if (T && tk->sdma_d2h && c->hsa_state == 0) c->hsa_state = hsa_agent_of(c->device, &c->hsa_agent) ? 1 : 2;
                if (T && tk->sdma_d2h && c->hsa_state == 1) {
                    // (the chunk's kernels are through -- the event above --, so the copy has no dependency; its signal is waited for at the end)
                    HsaDma& H = hsa_dma();
                    hsa_signal_t sg;
                    if (H.SignalCreate(1, 0, nullptr, &sg) != HSA_STATUS_SUCCESS) return fail(SPL_EDEVICE, "hsa_signal_create failed");
                    if (H.AsyncCopy(r->ids + base, H.cpu, c->d_ids.get() + (ch.lo - ln.lo), c->hsa_agent, T * 4, 0, nullptr, sg) != HSA_STATUS_SUCCESS) {
                        H.SignalDestroy(sg);
                        return fail(SPL_EDEVICE, "hsa_amd_memory_async_copy failed");
                    }
                    dma_sigs.push_back(sg);
                } else
                if (T) HIP_TRY(hipMemcpyAsync(r->ids + base, c->d_ids.get() + (ch.lo - ln.lo), T * 4, hipMemcpyDeviceToHost, c->s_d2h.get()));
                const uint64_t skip = ch.cont ? 1 : 0;
                {                                                      // the chunk's offsets, rebased: a few thousand additions on this thread
                    const uint64_t* const oo = h_oo + ch.oo_at;
                    uint64_t* const dst = r->off + ch.dlo;
                    for (uint64_t i = skip; i < nd; i++) dst[i] = oo[i] + base;
                }
                base += T;
            }
        }
        TRACE("all placed, waiting for the copies");
        for (auto& ln : lanes) { HIP_TRY(hipSetDevice(ln.c->device)); HIP_TRY(hipStreamSynchronize(ln.c->s_d2h.get())); }
        for (hsa_signal_t sg : dma_sigs) hsa_dma().SignalWait(sg, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
        return SPL_OK;
    };
    TRACE("encode_host: producers started");
    rc_all = consume();
    TRACE("encode_host: consumed");
    if (rc_all) err_all = g_err;
    for (auto& th : producers) th.join();
    for (auto& ln : lanes)
        if (!rc_all && ln.rc.load()) { rc_all = ln.rc.load(); err_all = ln.err; }
    if (rc_all) {
        for (auto& ln : lanes) { if (hipSetDevice(ln.c->device) == hipSuccess) (void)hipDeviceSynchronize(); }
        return fail(rc_all, err_all);
    }
    for (auto& ln : lanes) tk->rx_fallbacks += ln.patched;
    r->off[n_docs] = base;
    r->n_tokens = base;
    return SPL_OK;
}
}  // namespace
