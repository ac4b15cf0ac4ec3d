// spl_launch.h -- one device call.  What the call wants is a LaunchReq, filled with designated fields where the call is made; what the
// caller reads back is a LaunchDone; nothing of one call is kept in the context.  launch_all is the one entry point and a short sequence:
// check_call (what is refused, and the call's shape: mode, tiles, form), the chunk memo's turn (memo_before_launch; memo_ensure builds a
// whole Memo or none), fill_batch (the kernels' by-value Batch, filled once), then launch_queue, or launch_owned_front and
// launch_owned_tiles -- the two parts a caller may ask for one at a time (LaunchPart) --, then read_profile.  Behind it the device
// splitter's host half (rx_ensure / rx_next_status / rx_launch).  Needs Ctx and spl_tokenizer (spl_ctx.h), pick_mode (spl_mode.h) and
// pick_stream_beside (spl_streams.h).
#pragma once
namespace {

struct SlabOut { uint32_t* d_slab = nullptr; uint64_t cap_words = 0, max_docs = 0; };
// chunk boundaries given from outside (host splitter): device bitmaps, and the special tokens found on the host
constexpr uint32_t RX_STATUS_SLOTS = 8;
struct ExtIn {
    const uint32_t* d_starts = nullptr; const uint32_t* d_gaps = nullptr; const uint32_t* d_sp_pos = nullptr; const uint32_t* d_sp_id = nullptr; uint32_t n_sp = 0;
    // the two bitmaps are still to be made, by the device splitter, inside launch_all (behind the special-token kernels, whose bitmaps it reads):
    uint32_t* d_status = nullptr;          // non-null: yes; the status word it reports to
    uint32_t* d_status_host = nullptr;     // ... and (device pointer of) its pinned host copy, written by k_rx_mark itself
};
int rx_launch(spl_tokenizer* tk, Ctx* c, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
              uint32_t* d_starts, uint32_t* d_gaps, uint32_t* d_status, hipStream_t s, const Batch* sp = nullptr, uint32_t sp_words = 0,
              uint32_t* d_status_host = nullptr, bool bad_sets_status = false);

// Which part of a tile-owned call with the device splitter runs (per-document fallback): everything; only what comes in FRONT of the tile
// kernel (bitmap fills, special-token scan, the device splitter); only the tile kernel and k_tile_out, on bitmaps the caller may have patched.
enum class LaunchPart { All, Front, Tiles };
struct LaunchReq {
    const uint8_t* text = nullptr; uint64_t n_bytes = 0; const uint64_t* doc_off = nullptr; uint64_t n_docs = 0;     // device pointers, as all below
    uint32_t flags = 0;
    uint32_t* ids = nullptr; uint64_t ids_cap = 0; uint64_t* out_off = nullptr;
    hipStream_t stream = nullptr;
    const SlabOut* slab = nullptr;
    const ExtIn* ext = nullptr;
    LaunchPart part = LaunchPart::All;
    bool no_fuse = false;                  // the two-launch form even where the one launch applies (text read in place over PCIe: spl_pipeline.h)
    uint64_t* off_host = nullptr;          // where k_tile_out also stores the offsets (pinned results: one-chunk host batches, pipeline chunks, the latency path)
    uint32_t* done_word = nullptr;         // the completion word k_tile_out's last workgroup stores done_seq to (latency path)
    uint32_t done_seq = 0;
};
struct LaunchDone {
    bool off_host_written = false;         // the tile-owned mode stored the offsets at off_host
    bool done_armed = false;               // k_tile_out will store the completion word
};

// The chunk memo of a context (spl_k_memo.h, struct Memo): built at the first launch -- empty, or ("memo_first") seeded with the vocabulary's keys; the tiles log what it did not hold and raise the pinned
// flag; a launch that finds the flag raised first runs k_memo_fill on its stream -- encode the logged chunks, put them in -- and then
// its own kernels: the memo is only ever written between two launches of the stream that reads it.
// The seed of a NEW memo ("memo_first"): every vocabulary key of 2..64 bytes that finds one of its two slots free, as a one-token entry -- the
// placement decided here (memo_seed_plan), one compact record per key uploaded and scattered by ONE launch per table on the stream, in front
// of the first tile kernel that reads the table: "written only between launches" holds.  The copy is synchronous (the list is a local).
const spl::MemoSeedPlan& memo_seed_planned(spl_tokenizer* tk, uint32_t bits, uint32_t long_bits) {      // (the caller holds tk->seed_mu)
    if (!tk->seed_plan_valid || tk->seed_plan_bits != bits || tk->seed_plan_long_bits != long_bits) {
        spl::memo_seed_plan(tk->ht, bits, long_bits, tk->seed_plan);
        tk->seed_plan_bits = bits; tk->seed_plan_long_bits = long_bits; tk->seed_plan_valid = true;
    }
    return tk->seed_plan;
}
int memo_seed(spl_tokenizer* tk, Memo& m, hipStream_t s) {
    std::lock_guard<std::mutex> lock(tk->seed_mu);
    const spl::MemoSeedPlan& plan = memo_seed_planned(tk, tk->memo_bits, m.d_tab2 ? tk->memo_long_bits : 0u);
    m.seed_placed = plan.placed; m.seed_left = plan.left_out;
    DevBuf<uint32_t> d_list;
    const size_t n1 = plan.list.size(), n2 = plan.list2.size();
    if (!(n1 + n2)) return SPL_OK;
    SPL_TRY(d_list.alloc(n1 + n2));
    HIP_TRY(hipStreamSynchronize(nullptr));        // (the tables' zero fill ran on the default stream)
    if (n1) HIP_TRY(hipMemcpy(d_list.get(), plan.list.data(), n1 * 4, hipMemcpyHostToDevice));
    if (n2) HIP_TRY(hipMemcpy(d_list.get() + n1, plan.list2.data(), n2 * 4, hipMemcpyHostToDevice));
    const uint32_t c1 = (uint32_t)(n1 / 10), c2 = (uint32_t)(n2 / 18);
    if (c1) hipLaunchKernelGGL(k_memo_seed<false>, dim3((c1 + 255) / 256), dim3(256), 0, s, m.d_tab.get(), (MemoHi*)nullptr, m.mask, (const uint32_t*)d_list.get(), c1);
    if (c2) { const Memo2Parts p = m.parts2(); hipLaunchKernelGGL(k_memo_seed<true>, dim3((c2 + 255) / 256), dim3(256), 0, s, p.ent, p.hi, m.mask2, (const uint32_t*)(d_list.get() + n1), c2); }
    HIP_TRY(hipStreamSynchronize(s));              // (the list is freed here; once per memo)
    return SPL_OK;
}
// A whole memo or none: it is built in a local and moved into the context only when every piece is there and the seed is in.  A failure
// on the way frees what there was and leaves the context without a memo -- the next launch starts again from nothing.
int memo_ensure(spl_tokenizer* tk, Ctx* t, hipStream_t s) {
    if (t->memo) return SPL_OK;
    Memo m;
    const size_t slots = (size_t)1 << tk->memo_bits;
    SPL_TRY(m.d_tab.alloc_zeroed(slots));
    SPL_TRY(m.d_ext.alloc(slots));      // (only hits of seven to fourteen tokens ever touch it)
    SPL_TRY(m.d_claim.alloc_zeroed(slots));
    m.mask = (uint32_t)(slots - 1);
    // (the log of a context that takes LARGE batches is larger: a cold pass over 200 MB misses the vocabulary three million times, and at 65 536
    //  logged chunks a fill -- duplicates among them -- the memo needed a dozen passes to hold them all; one entry per 192 bytes of capacity, 16 384 a region at most)
    m.cap = (uint32_t)std::min<uint64_t>(16384, std::max<uint64_t>(tk->memo_log_cap, t->cap_bytes / ((uint64_t)SPL_MEMO_LOG_REGIONS * 192)));
    SPL_TRY(m.d_log.alloc((size_t)SPL_MEMO_LOG_REGIONS * m.cap * SPL_MEMO_LOG_WORDS));
    SPL_TRY(m.d_log_cnt.alloc_zeroed(2 * SPL_MEMO_LOG_REGIONS));              // (the second half: the log of chunks of 33..64 bytes)
    if (tk->memo_long_bits) {
        const size_t s2 = (size_t)1 << tk->memo_long_bits;
        m.cap2 = std::max<uint32_t>(m.cap / 8, 16);
        const size_t bytes = s2 * (sizeof(MemoEnt) + sizeof(MemoExt) + sizeof(MemoHi) + 4) + (size_t)SPL_MEMO_LOG_REGIONS * m.cap2 * SPL_MEMO_LOG_WORDS2 * 4;
        SPL_TRY(m.d_tab2.alloc(bytes));
        HIP_TRY(hipMemset(m.d_tab2.get(), 0, s2 * (sizeof(MemoEnt) + sizeof(MemoExt) + sizeof(MemoHi) + 4)));
        m.mask2 = (uint32_t)(s2 - 1);
    }
    SPL_TRY(m.d_stats.alloc_zeroed(2));
    SPL_TRY(m.h_flag.alloc(16));
    if (tk->memo_first) SPL_TRY(memo_seed(tk, m, s));
    t->memo = std::move(m);
    return SPL_OK;
}
int memo_before_launch(spl_tokenizer* tk, Ctx* t, hipStream_t s) {
    if (!tk->memo) { t->dt.memo = nullptr; t->dt.memo2 = nullptr; return SPL_OK; }
    int rc = memo_ensure(tk, t, s);
    if (rc) return rc;
    Memo& m = t->memo;
    m.tables(t->dt);
    m.since++;
    // (the flag was raised by an EARLIER launch's tiles, when one of the log's regions became half full)
    if (*(volatile uint32_t*)m.h_flag.host()) {
        *(volatile uint32_t*)m.h_flag.host() = 0;
        m.round++;
        hipLaunchKernelGGL(k_memo_fill<false>, dim3((m.cap + MEMO_FILL_NT - 1) / MEMO_FILL_NT, SPL_MEMO_LOG_REGIONS), dim3(MEMO_FILL_NT), 0, s, t->dt, m.d_tab.get(), m.d_ext.get(),
                           (MemoHi*)nullptr, (const uint32_t*)m.d_log.get(), (const uint32_t*)m.d_log_cnt.get(), m.cap, m.d_claim.get(), m.round, m.d_stats.get());
        if (m.d_tab2) {
            const Memo2Parts p = m.parts2();
            hipLaunchKernelGGL(k_memo_fill<true>, dim3((m.cap2 + MEMO_FILL_NT2 - 1) / MEMO_FILL_NT2, SPL_MEMO_LOG_REGIONS), dim3(MEMO_FILL_NT2), 0, s, t->dt, p.ent, p.ext, p.hi,
                               (const uint32_t*)p.log, (const uint32_t*)(m.d_log_cnt.get() + SPL_MEMO_LOG_REGIONS), m.cap2, p.claim, m.round, m.d_stats.get());
        }
        HIP_TRY(hipMemsetAsync(m.d_log_cnt.get(), 0, 2 * SPL_MEMO_LOG_REGIONS * 4, s));
        m.fills++;
        m.since = 0;
    }
    return SPL_OK;
}

// ---- the call's shape ---------------------------------------------------------------------------------------------
// What check_call derives from the request, the handle's options and the context: read by every step behind it, changed by none.
struct CallShape {
    bool special = false, general = false;   // the GPU's literal scan runs (SPL_WITH_SPECIAL and literals; not with the HOST splitter's boundaries); ... as the two-launch general matcher
    TileMode mode = TileMode::Refuse;
    uint32_t ntiles = 0;
    bool fuse = false;                       // tile-owned mode as ONE launch: no k_tile_out
    bool ranged = false;                     // ... as ranges of its tiles, k_pretok + k_tile_out per range
    bool prof = false;
    // bitmaps and queue counters packed back to back for THIS batch size, so that one memset clears them: words per bitmap, bitmaps in
    // use (tbits | tstart [| skip [| spcand]]), and all of them with the counters behind
    size_t uw = 0, nbm = 0, clear_words = 0;
};
int check_call(const spl_tokenizer* tk, const Ctx* t, const LaunchReq& rq, CallShape& sh) {
    static_assert(TileGeom<SPL_TILE_DIRECT_A>::Wv == TileGeom<SPL_TILE_SMALL>::Wv && TileGeom<SPL_TILE_DIRECT_B>::Wv == TileGeom<SPL_TILE_SMALL>::Wv &&
                  TileGeom<SPL_TILE_DIRECT_A>::TBv >= TileGeom<SPL_TILE_SMALL>::TBv && TileGeom<SPL_TILE_DIRECT_B>::TBv >= TileGeom<SPL_TILE_SMALL>::TBv,
                  "the workspace is sized for SPL_TILE_SMALL's window and tile count");
    const bool sp_asked = (rq.flags & SPL_WITH_SPECIAL) && !tk->specials.empty();
    if (((uintptr_t)rq.text & 15) != 0) return fail(SPL_EINVAL, "text buffer must be 16-byte aligned");
    if (rq.ext && rq.n_bytes > SPL_DIRECT_MAX_BYTES) return fail(SPL_EINVAL, "external chunk boundaries: at most 256 MB per device call");
    if (rq.n_bytes > 0x7FFF0000ull) return fail(SPL_EINVAL, "n_bytes per device call must be < 2^31 - 65536 (split the corpus at document boundaries; spl_encode_batch does that by itself)");
    if (rq.n_docs > 0xFFFFFFF0ull) return fail(SPL_EINVAL, "n_docs per device call must be < 2^32 - 16");
    // (external boundaries from the HOST splitter: the special tokens -- if any -- were found there; the GPU's literal scan stays off)
    sh.special = (!rq.ext || rq.ext->d_status) && sp_asked;
    sh.general = sh.special && tk->special_general;
    sh.mode = pick_mode(t->force_tile, rq.ext != nullptr, sh.special, rq.n_bytes);
    if (sh.mode == TileMode::Refuse)
        return fail(SPL_EINVAL, sp_asked
                                    ? "a device call with SPL_WITH_SPECIAL takes at most 256 MB: split the call at document boundaries -- spl_encode_batch does that by itself"
                                    : "this device call fits neither the tile-owned mode (256 MB) nor queue mode (2047 MiB, no forced geometry): split it at document boundaries");
    const bool queue = sh.mode == TileMode::Queue, direct_b = sh.mode == TileMode::OwnedB;
    const uint32_t tile_bytes = queue ? TileGeom<SPL_TILE_SMALL>::TBv : direct_b ? TileGeom<SPL_TILE_DIRECT_B>::TBv : TileGeom<SPL_TILE_DIRECT_A>::TBv;
    sh.ntiles = (uint32_t)((rq.n_bytes + tile_bytes - 1) / tile_bytes);
    sh.prof = t->prof;
    // ONE launch (spl_k_fuse.h): every tile resident at once, each learns its base from the others' published counts and writes its
    // part of the CSR itself
    sh.fuse = !queue && tk->fuse && !rq.no_fuse && sh.ntiles && sh.ntiles <= tk->fuse_max_tiles && rq.part != LaunchPart::Front;
    // A LARGE batch goes out as ranges of its tiles -- k_pretok and k_tile_out of range k, then of range k + 1, ...: what k_pretok leaves for
    // k_tile_out (the tiles' ids and records) is still in the caches when k_tile_out reads it (one launch pair over 215 MB: 42 GB/s; its
    // 27 MB ranges: 50), and on two streams the slow last tiles of one range run beside the next range's first.  A tile's base is the sum
    // of the counts of the tiles in front of it: k_tile_out of range k needs k_pretok of the ranges 0 .. k, nothing else.
    sh.ranged = direct_b && sh.ntiles && !sh.fuse && tk->range_tiles && sh.ntiles > tk->range_tiles + tk->range_tiles / 4 && !rq.slab && !sh.prof &&
                !rq.done_word && !rq.off_host && rq.part == LaunchPart::All;
    sh.uw = (size_t)(rq.n_bytes / RANK_BLK + 1) * 32 + 32;
    sh.nbm = sh.special ? (sh.general ? 4 : 3) : 2;
    sh.clear_words = sh.nbm * sh.uw + QCOUNT_WORDS;
    return SPL_OK;
}

// The kernels' by-value argument, filled ONCE for the call: from the request, the workspace, the memo, and -- read, not advanced -- the
// parities.  (The context only learns where this call's queue counters lie: spl_last_queue_counts.)
void fill_batch(const spl_tokenizer* tk, Ctx* t, const LaunchReq& rq, const CallShape& sh, Batch& b) {
    const bool queue = sh.mode == TileMode::Queue, tiles_run = sh.ntiles && rq.part != LaunchPart::Front;
    b.text = rq.text; b.n_bytes = (uint32_t)rq.n_bytes; b.doc_off = rq.doc_off; b.n_docs = (uint32_t)rq.n_docs;
    b.n_blk = (uint32_t)(rq.n_bytes / RANK_BLK + 1);
    b.tbits = t->d_zero.get(); b.tstart = t->d_zero.get() + sh.uw;
    b.skip = sh.special ? t->d_zero.get() + 2 * sh.uw : nullptr;
    b.spcand = sh.general ? t->d_zero.get() + 3 * sh.uw : nullptr;
    b.qcount = t->d_zero.get() + sh.nbm * sh.uw;
    b.sp_lits = t->d_sp_lits.get(); b.n_special = sh.special ? (uint32_t)tk->specials.size() : 0u;
    b.stage = t->d_stage.get(); b.rank_scr = t->d_rank.get(); b.aux = t->d_aux;
    b.q64 = t->d_q64.get(); b.qlong = t->d_qlong.get(); b.qdefer = t->d_qdefer.get();
    b.qcap64 = t->qcap64; b.qcaplong = t->qcaplong; b.qcapdefer = t->qcapdefer;
    b.dbg = (t->dbg_on || t->prof) ? t->d_dbg.get() : nullptr;
    b.stop_phase = (uint32_t)t->stop_phase;
    { static const uint32_t dbg_wg = [] { const char* e = getenv("SPL_DEBUG_WG"); return e ? (uint32_t)strtoul(e, nullptr, 10) : 0xFFFFFFFFu; }(); b.dbg_wg = dbg_wg; }
    b.blk_base = t->d_blk.get();
    b.id_limit = t->dt.id_limit;
    b.ids_out = rq.ids; b.ids_cap = rq.ids_cap; b.off_out = rq.out_off;
    if (rq.part != LaunchPart::Front) {                      // (the chunk memo, as memo_before_launch has just left it)
        const Memo& m = t->memo;
        if (t->dt.memo) { b.mlog = m.d_log.get(); b.mlog_cnt = m.d_log_cnt.get(); b.mlog_cap = m.cap; b.mflag = m.h_flag.dev(); }
        if (t->dt.memo && m.d_tab2) { b.mlog2 = m.parts2().log; b.mlog2_cap = m.cap2; }
        b.memo_first = (t->dt.memo && tk->memo_first) ? 1u : 0u;
    }
    b.tdesc = t->d_tdesc.get(); b.tile_ids = t->d_tile_ids.get(); b.tctl = t->d_tctl.get();
    b.tgroups = t->tgroups; b.tpar = t->tpar; b.tslot = (uint32_t)TileGeom<SPL_TILE_SMALL>::Wv + 1u;
    t->last_qcount = queue ? b.qcount : nullptr;
    if (queue) { b.tile_bits = t->d_tile_bits.get(); b.tcnt = t->d_tcnt.get(); return; }
    if (rq.slab && sh.ntiles) { b.slab = rq.slab->d_slab; b.slab_cap = (uint32_t)rq.slab->cap_words; b.slab_max_docs = (uint32_t)rq.slab->max_docs; b.slab_p24 = tk->slab_pack24 ? 1u : 0u; }
    if (sh.fuse) {                                           // this launch's parity to publish into, the other one -- what the previous fused launch left -- to zero
        uint8_t* const mine = t->d_fctl.get() + (size_t)t->fpar * FUSE_PARITY_BYTES, * const other = t->d_fctl.get() + (size_t)(t->fpar ^ 1u) * FUSE_PARITY_BYTES;
        b.ftc = (uint16_t*)mine; b.ftb = (uint32_t*)(mine + (size_t)FUSE_REPL * FUSE_STRIDE * 2);
        b.fzc = (uint16_t*)other; b.fzb = (uint32_t*)(other + (size_t)FUSE_REPL * FUSE_STRIDE * 2); b.fz_n = t->fprev;
    }
    if (tiles_run && rq.off_host) b.off_out2 = rq.off_host;
    if (tiles_run && rq.done_word) { b.done = rq.done_word; b.done_seq = rq.done_seq; }
    if (!sh.special) b.tstart = nullptr;
    b.qcount = nullptr;
    if (rq.ext) {
        b.ext_starts = rq.ext->d_starts; b.ext_gaps = rq.ext->d_gaps;
        if (rq.ext->n_sp > 0) b.skip = const_cast<uint32_t*>(rq.ext->d_gaps);     // (read-only here: the spans the literals' tokens lie in)
    }
}

// ---- the launches -------------------------------------------------------------------------------------------------
// (A/B on the 1 MB bench batch: folding these launches together -- clean-after-use bitmaps, one
//  tail kernel with a grid barrier and a last-workgroup scan -- was SLOWER than this plain
//  sequence: back-to-back launches overlap their dispatch with the previous kernel, while
//  single-workgroup tails and agent-scope fences sit on the critical path.)
#define MARK(i) do { if (sh.prof) HIP_TRY(hipEventRecord(t->ev[i].get(), s)); } while (0)
int launch_error() {
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? SPL_OK : fail(SPL_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(le));
}
// The parities a launch was given (fill_batch) are advanced once its k_pretok is out, not before: an error return in front of that leaves
// them as the previous launch left them, armed for the next.  A fused launch has used parity fpar for its ntiles counts (the next one zeroes
// them); any other, tpar -- k_tile_out zeroes the other parity's sums for the next call.
void commit_parities(Ctx* t, const CallShape& sh) {
    if (sh.fuse) { t->fpar ^= 1u; t->fprev = sh.ntiles; }
    else t->tpar ^= 1u;
}

int launch_queue(Ctx* t, const LaunchReq& rq, const CallShape& sh, const Batch& b) {
    hipStream_t s = rq.stream;
    const uint32_t ntiles = sh.ntiles;
    t->bitmap_dirty = true;
    HIP_TRY(hipMemsetAsync(t->d_zero.get(), 0, sh.clear_words * 4, s));
    MARK(KI_MARK);
    if (rq.n_docs) hipLaunchKernelGGL(k_mark_docs, dim3((uint32_t)((rq.n_docs + 255) / 256)), dim3(256), 0, s, b);
    MARK(KI_SPECIAL); MARK(KI_PRETOK);
    hipLaunchKernelGGL((k_pretok<SPL_TILE_SMALL>), dim3(ntiles), dim3(NT), 0, s, PRETOK_EARLY(t->dt, b), t->dt, b);
    commit_parities(t, sh);
    MARK(KI_DEFER);
    hipLaunchKernelGGL(k_deferred_wave, dim3(256), dim3(64), 0, s, t->dt, b);
    MARK(KI_BPELANES);
    hipLaunchKernelGGL(k_bpe_segments, dim3(std::min<uint32_t>(2048, ntiles / 4 + 8)), dim3(NT), 0, s, t->dt, b);
    MARK(KI_BPELONG);
    hipLaunchKernelGGL(k_bpe_long, dim3(std::min<uint32_t>(2048, ntiles / 4 + 8)), dim3(NT), 0, s, t->dt, b, 1);
    MARK(KI_COUNT);
    hipLaunchKernelGGL((k_range_count<SPL_TILE_SMALL>), dim3(ntiles), dim3(64), 0, s, b);
    MARK(KI_SCAN); MARK(KI_COMPACT);
    hipLaunchKernelGGL((k_range_out<SPL_TILE_SMALL>), dim3(ntiles), dim3(64), 0, s, b);
    MARK(KI_N);
    return SPL_OK;
}

// Tile-owned mode, what comes in FRONT of the tile kernel: the bitmaps' fill, the host-found literals, the GPU's literal scan, the device splitter.
int launch_owned_front(spl_tokenizer* tk, Ctx* t, const LaunchReq& rq, const CallShape& sh, const Batch& b) {
    hipStream_t s = rq.stream;
    const ExtIn* const ext = rq.ext;
    const bool ext_sp = ext && ext->n_sp > 0;
    if (sh.special) {
        // the three bitmaps are cleared per call; documents and literals are marked by the
        // multi-pass kernels, the tile kernel reads the bitmaps on top of its document search
        HIP_TRY(hipMemsetAsync(t->d_zero.get(), 0, sh.clear_words * 4, s));
        t->bitmap_dirty = true;
    } else if (ext_sp) {                   // the token bitmap takes the host-found literals: cleared per call
        HIP_TRY(hipMemsetAsync(t->d_zero.get(), 0, sh.uw * 4, s));
        t->bitmap_dirty = true;
    } else if (t->bitmap_dirty) {
        HIP_TRY(hipMemsetAsync(t->d_zero.get(), 0, t->zero_words * 4, s));
        t->bitmap_dirty = false;
    }
    if (ext_sp) hipLaunchKernelGGL(k_ext_specials, dim3((ext->n_sp + 255) / 256), dim3(256), 0, s, b, ext->d_sp_pos, ext->d_sp_id, ext->n_sp);
    MARK(KI_MARK);
    if (sh.special && rq.n_docs) hipLaunchKernelGGL(k_mark_docs, dim3((uint32_t)((rq.n_docs + 255) / 256)), dim3(256), 0, s, b);
    MARK(KI_SPECIAL);
    if (sh.special && rq.n_bytes) {
        if (!sh.general) hipLaunchKernelGGL(k_special_scan, dim3((uint32_t)((rq.n_bytes + 255) / 256)), dim3(256), 0, s, b);
        else {
            hipLaunchKernelGGL(k_special_ends, dim3((uint32_t)((rq.n_bytes + 255) / 256)), dim3(256), 0, s, b);
            hipLaunchKernelGGL(k_special_select, dim3((uint32_t)((rq.n_docs + 255) / 256)), dim3(256), 0, s, b);
        }
    }
    if (ext && ext->d_status)                                // the device splitter, behind the literal scan whose bitmaps it reads
        SPL_TRY(rx_launch(tk, t, rq.text, rq.n_bytes, rq.doc_off, rq.n_docs, const_cast<uint32_t*>(ext->d_starts), const_cast<uint32_t*>(ext->d_gaps),
                          ext->d_status, s, sh.special ? &b : nullptr, (uint32_t)sh.uw, ext->d_status_host));
    return SPL_OK;
}

// ... a LARGE batch as ranges of its tiles (CallShape::ranged), alternating between the caller's stream and a second one
int launch_ranged(spl_tokenizer* tk, Ctx* t, const LaunchReq& rq, const CallShape& sh, Batch& b) {
    hipStream_t s = rq.stream;
    const uint32_t ntiles = sh.ntiles;
    // (ranges of equal size, a multiple of 64 tiles: the tiles' counts are summed per group of 64)
    const uint32_t nr = (ntiles + tk->range_tiles - 1) / tk->range_tiles, R = (((ntiles + nr - 1) / nr) + 63u) & ~63u;
    const bool two = tk->range_streams == 2;
    if (two && t->s_rng.get() && t->s_rng_for != s && tk->pick_streams) { (void)hipStreamSynchronize(t->s_rng.get()); t->s_rng.reset(); }
    if (two && !t->s_rng) {
        // (a stream MEASURED to run beside the caller's: which hardware queue a stream gets is the runtime's choice -- pick_stream_beside)
        if (tk->pick_streams) { double cf = 0; hipStream_t picked = nullptr; SPL_TRY(pick_stream_beside({s}, &picked, &cf)); t->s_rng.reset(picked); }
        else SPL_TRY(t->s_rng.create());
        t->s_rng_for = s;
        if (!t->ev_rng_in) { SPL_TRY(t->ev_rng_in.create()); SPL_TRY(t->ev_rng_out.create()); }
    }
    while (two && t->ev_rng.size() < nr) { Event e; SPL_TRY(e.create()); t->ev_rng.push_back(std::move(e)); }
    if (two) { HIP_TRY(hipEventRecord(t->ev_rng_in.get(), s)); HIP_TRY(hipStreamWaitEvent(t->s_rng.get(), t->ev_rng_in.get(), 0)); }     // (what the caller's stream holds comes first)
    for (uint32_t k = 0; k < nr; k++) {
        hipStream_t st = (two && (k & 1u)) ? t->s_rng.get() : s;
        if (k * R >= ntiles) break;
        const uint32_t n = std::min(R, ntiles - k * R);
        b.tile0 = k * R;
        hipLaunchKernelGGL((k_pretok<SPL_TILE_DIRECT_B>), dim3(n), dim3(NT), 0, st, PRETOK_EARLY(t->dt, b), t->dt, b);
        if (!k) commit_parities(t, sh);
        if (two) {
            HIP_TRY(hipEventRecord(t->ev_rng[k].get(), st));
            if (k) HIP_TRY(hipStreamWaitEvent(st, t->ev_rng[k - 1].get(), 0));        // (k_pretok of range k - 1, on the other stream; the ranges before it: in order)
        }
        hipLaunchKernelGGL(k_tile_out, dim3(n), dim3(TOUT_NT), 0, st, tile_out_args(b));
    }
    b.tile0 = 0;
    if (two) { HIP_TRY(hipEventRecord(t->ev_rng_out.get(), t->s_rng.get())); HIP_TRY(hipStreamWaitEvent(s, t->ev_rng_out.get(), 0)); }
    return SPL_OK;
}

// Tile-owned mode, the tiles: ONE fused launch; or k_pretok -- whole, or as ranges -- and k_tile_out; or, without a byte, only the offsets' fill.
// (The latency path as ONE launch -- the last workgroup of the tile kernel turning every tile's record into the CSR by itself, no
//  k_tile_out -- was built and measured in round 5: 33.6 us per 1 KB call against 31.2 with the two launches, 23.9 against 22.8 for 13
//  bytes.  Two back-to-back launches overlap the second one's dispatch with the first kernel; the fused epilogue's device-scope fences,
//  L1-bypassing loads and serial walk over the tiles cost more than that launch.  Dropped.)
int launch_owned_tiles(spl_tokenizer* tk, Ctx* t, const LaunchReq& rq, const CallShape& sh, Batch& b) {
    hipStream_t s = rq.stream;
    const uint32_t ntiles = sh.ntiles;
    if (rq.part == LaunchPart::Tiles) { MARK(KI_MARK); MARK(KI_SPECIAL); }      // (the front's slots, which read_profile reads: it ran as a call of its own)
    MARK(KI_PRETOK);
    if (sh.ranged) SPL_TRY(launch_ranged(tk, t, rq, sh, b));
    else if (ntiles) {
        if (sh.mode == TileMode::OwnedB) hipLaunchKernelGGL((k_pretok<SPL_TILE_DIRECT_B>), dim3(ntiles), dim3(NT), 0, s, PRETOK_EARLY(t->dt, b), t->dt, b);
        else hipLaunchKernelGGL((k_pretok<SPL_TILE_DIRECT_A>), dim3(ntiles), dim3(NT), 0, s, PRETOK_EARLY(t->dt, b), t->dt, b);
        commit_parities(t, sh);
    }
    else HIP_TRY(hipMemsetAsync(rq.out_off, 0, (rq.n_docs + 1) * 8, s));
    MARK(KI_DEFER); MARK(KI_BPELANES); MARK(KI_BPELONG); MARK(KI_COUNT); MARK(KI_SCAN); MARK(KI_COMPACT);
    if (ntiles && !sh.fuse && !sh.ranged) {
        const uint32_t ng = (ntiles + 63u) / 64u;
        if (ng > tk->group_scan_min && tk->group_scan_min) {
            unsigned long long* const gpre = reinterpret_cast<unsigned long long*>(t->d_tctl.get() + ((16 + 2 * (size_t)t->tgroups + 1) & ~(size_t)1));
            hipLaunchKernelGGL(k_group_scan, dim3(1), dim3(256), 0, s, (const uint32_t*)(t->d_tctl.get() + 16 + b.tpar * t->tgroups), ng, gpre);
            b.gpre = gpre;
        }
        hipLaunchKernelGGL(k_tile_out, dim3(ntiles), dim3(TOUT_NT), 0, s, tile_out_args(b));
    }
    MARK(KI_N);
    return SPL_OK;
}
#undef MARK

// Per-kernel profiling (spl_profile_read): the time between the events of the slots whose kernels this call launched
int read_profile(Ctx* t, const CallShape& sh) {
    const bool queue = sh.mode == TileMode::Queue;
    HIP_TRY(hipEventSynchronize(t->ev[KI_N].get()));
    for (int i = 0; i < KI_N; i++) {
        // slots whose kernels were not launched in this mode would only show the event overhead
        const bool launched = queue ? (i != KI_SPECIAL && i != KI_SCAN)
                                    : (i == KI_PRETOK || (i == KI_COMPACT && !sh.fuse) || (sh.special && (i == KI_MARK || i == KI_SPECIAL)));
        if (!launched) continue;
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, t->ev[i].get(), t->ev[i + 1].get()));
        if (i == KI_PRETOK && sh.ntiles) {
            // the dominant kernel is timed on the device's wall clock instead (see k_pretok)
            unsigned long long span[2];
            HIP_TRY(hipMemcpy(span, t->d_dbg.get() + 14, 16, hipMemcpyDeviceToHost));
#ifndef SPL_DEBUG_STAMPS
            {   // the end: the latest of the workgroups' own words (spl_k_pretok.h)
                static thread_local std::vector<unsigned long long> ends;
                ends.resize(std::min<size_t>(sh.ntiles, 4 * (size_t)SPL_DEBUG_BLOCKS));
                HIP_TRY(hipMemcpy(ends.data(), t->d_dbg.get() + 16, ends.size() * 8, hipMemcpyDeviceToHost));
                span[1] = 0;
                for (unsigned long long e : ends) span[1] = std::max(span[1], e);
            }
#endif
            int khz = 0;
            HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, t->device));
            if (khz > 0 && span[1] > span[0]) ms = (float)((double)(span[1] - span[0]) / (double)khz);
        }
        t->prof_ms[i] += ms;
        t->prof_n[i] += 1;
    }
    return SPL_OK;
}

int launch_all(spl_tokenizer* tk, Ctx* t, const LaunchReq& rq, LaunchDone* done = nullptr) {
    hipStream_t s = rq.stream;
    CallShape sh;
    SPL_TRY(check_call(tk, t, rq, sh));
    if (sh.special) SPL_TRY(upload_specials(tk, t));
    SPL_TRY(reserve(t, rq.n_bytes, rq.n_docs));
    if (sh.prof && !t->ev_ready) {
        for (auto& e : t->ev) SPL_TRY(e.create(hipEventDefault));
        t->ev_ready = true;
    }
    if (sh.prof) {
        const unsigned long long init[2] = {~0ull, 0ull};
        HIP_TRY(hipMemcpyAsync(t->d_dbg.get() + 14, init, 16, hipMemcpyHostToDevice, s));
    }
    // (the chunk memo: a fill, if the earlier launches left something to put in)
    if (rq.part != LaunchPart::Front) SPL_TRY(memo_before_launch(tk, t, s));
    Batch b{};
    fill_batch(tk, t, rq, sh, b);
    // Single pass: small batches without special tokens are finished by ONE kernel.
    if (sh.mode == TileMode::Queue) SPL_TRY(launch_queue(t, rq, sh, b));
    else {
        if (rq.part != LaunchPart::Tiles) SPL_TRY(launch_owned_front(tk, t, rq, sh, b));
        if (rq.part == LaunchPart::Front) return launch_error();
        SPL_TRY(launch_owned_tiles(tk, t, rq, sh, b));
    }
    SPL_TRY(launch_error());
    if (rq.slab && (sh.mode == TileMode::Queue || !sh.ntiles))          // the slab copy of the result, where k_tile_out did not write it:
        // copied from the caller's ids, of which only ids_cap entries exist -- tokens the encode dropped are not in the slab either
        hipLaunchKernelGGL(k_gatherv_pack, dim3(256), dim3(256), 0, s, rq.ids, rq.out_off, (uint32_t)rq.n_docs, rq.slab->d_slab,
                           (uint32_t)rq.slab->cap_words, (uint32_t)rq.slab->max_docs, tk->slab_pack24 ? 1u : 0u, rq.ids_cap);
    if (done) { done->off_host_written = b.off_out2 != nullptr; done->done_armed = b.done != nullptr; }
    if (sh.prof) SPL_TRY(read_profile(t, sh));
    return SPL_OK;
}

// ---- custom split patterns on the device (spl_rx_split.h) ---------------------------------------------------------
// Uploads the program image (and the general-category table if a class set tests one) to this context once, grows the
// workspace, and launches the two kernels on `s`: d_starts / d_gaps (n_bytes / 32 + 2 words each, at least) are zeroed here;
// *d_status collects RXS_* bits (not cleared here: a batch of several chunks shares one word).
bool rx_applies(const spl_tokenizer* tk, uint32_t flags) {
    (void)flags;                           // (SPL_WITH_SPECIAL too: the literals are found by the GPU's own scan, as for the built-in patterns)
    return tk->regex && tk->rx_device && !tk->rx_image.empty();
}
int rx_ensure(spl_tokenizer* tk, Ctx* c) {
    if (c->d_rx_image) return SPL_OK;
    // (every piece only if it is not there yet: a call that failed half-way is repeated without leaking what it had allocated)
    if (tk->rx_image[7] && !tk->ht.gc_stage1.empty()) {
        if (!c->d_gc1) SPL_TRY(c->d_gc1.upload(tk->ht.gc_stage1));
        if (!c->d_gc2) SPL_TRY(c->d_gc2.upload(tk->ht.gc_stage2));
    }
    if (!c->d_rx_status) SPL_TRY(c->d_rx_status.alloc_zeroed(16));
    if (!c->h_rx_status) SPL_TRY(c->h_rx_status.alloc(16));
    if (!c->d_rx_bad) SPL_TRY(c->d_rx_bad.alloc_zeroed(1 + RX_BAD_CAP));
    if (!c->h_rx_bad) SPL_TRY(c->h_rx_bad.alloc(1 + 2 * RX_BAD_CAP));
    if (!c->ev_split) SPL_TRY(c->ev_split.create());
    return c->d_rx_image.upload(tk->rx_image);
}
// This batch's status word: the next one of the context's rotation -- cleared by the previous batch's k_rx_mark, or here if that batch launched none
int rx_next_status(Ctx* c, hipStream_t s) {
    c->rx_slot = (c->rx_slot + 1) % RX_STATUS_SLOTS;
    if (!c->rx_next_clean) HIP_TRY(hipMemsetAsync(c->d_rx_status.get() + c->rx_slot, 0, 4, s));
    c->rx_next_clean = false;
    return SPL_OK;
}
int rx_launch(spl_tokenizer* tk, Ctx* c, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
              uint32_t* d_starts, uint32_t* d_gaps, uint32_t* d_status, hipStream_t s, const Batch* sp, uint32_t sp_words, uint32_t* d_status_host,
              bool bad_sets_status) {
    if (n_bytes > SPL_DIRECT_MAX_BYTES) return fail(SPL_EINVAL, "device split: at most 256 MB per call");
    if (((uintptr_t)d_text & 15) != 0) return fail(SPL_EINVAL, "text buffer must be 16-byte aligned");
    int rc = rx_ensure(tk, c);
    if (rc) return rc;
    const uint64_t words = n_bytes / 32 + 2;
    if (!n_bytes) {                                    // (no block, no kernel: the two closing words by a fill)
        HIP_TRY(hipMemsetAsync(d_starts, 0, words * 4, s));
        HIP_TRY(hipMemsetAsync(d_gaps, 0, words * 4, s));
        return SPL_OK;
    }
    const uint64_t nblk = (n_bytes + RXB - 1) / RXB;
    // workspace, laid out by its CAPACITY in blocks (the per-block entries must stay where they are from call to call -- they are
    // told apart by generation, not cleared): blk | bskip | bad_hi | bad_lo | dstart | nx | gx
    if (nblk > c->rx_cap_blk) {
        const uint64_t cb = nblk + nblk / 4 + 16;
        const uint64_t cap = 16 * cb + 4 * (8 * cb + 2) + 4 * cb * RXB + 256;
        c->rx_cap_blk = 0;
        SPL_TRY(c->d_rx_ws.grow(&c->rx_ws_cap, cap, cap));
        c->rx_cap_blk = cb;
        c->rx_gen = 0xFFFFu;                           // (fresh memory: cleared below)
    }
    // the per-block entries carry the call's generation instead of being cleared per call (two fills of ~5 us each in front of the
    // kernels of a 1 MB batch); every 65 535 calls -- and on fresh memory -- the workspace is cleared once
    if (++c->rx_gen > 0xFFFFu) {
        HIP_TRY(hipMemsetAsync(c->d_rx_ws.get(), 0, c->rx_ws_cap, s));
        c->rx_gen = 1;
    }
    RxArgs a{};
    a.image = c->d_rx_image.get(); a.image_words = (uint32_t)tk->rx_image.size();
    a.text = d_text; a.doc_off = d_doc_off; a.n_bytes = (uint32_t)n_bytes; a.n_docs = (uint32_t)n_docs;
    a.ucls1 = c->dt.ucls_stage1; a.ucls2 = c->dt.ucls_stage2; a.shift = c->dt.ucls_shift;
    a.gc1 = c->d_gc1.get(); a.gc2 = c->d_gc2.get();
    a.blk = (uint32_t*)c->d_rx_ws.get(); a.bskip = a.blk + c->rx_cap_blk; a.bad_hi = a.bskip + c->rx_cap_blk; a.bad_lo = a.bad_hi + c->rx_cap_blk;
    a.dstart = a.bad_lo + c->rx_cap_blk;
    a.bad_list = c->d_rx_bad.get(); a.bad_host = c->h_rx_bad.dev(); a.bad_sets_status = bad_sets_status ? 1u : 0u;
    a.nx = (uint16_t*)(a.dstart + 8 * c->rx_cap_blk + 2); a.gx = a.nx + c->rx_cap_blk * RXB;
    a.gen = c->rx_gen; a.bm_words = (uint32_t)words;
    a.starts = d_starts; a.gaps = d_gaps; a.status = d_status; a.status_host = d_status_host;
    if (d_status >= c->d_rx_status.get() && d_status < c->d_rx_status.get() + RX_STATUS_SLOTS)          // (one of the context's own words: the next one in the rotation)
    {
        a.status_next = c->d_rx_status.get() + ((uint32_t)(d_status - c->d_rx_status.get()) + 1) % RX_STATUS_SLOTS;
        c->rx_next_clean = true;
    }
    if (sp) { a.sp_tstart = sp->tstart; a.sp_tbits = sp->tbits; a.sp_words = sp_words; }
    hipLaunchKernelGGL(k_rx_match, dim3((uint32_t)nblk), dim3(RXT), (a.image_words * 4 + 15) & ~15u, s, a);
    hipLaunchKernelGGL(k_rx_mark, dim3((uint32_t)nblk), dim3(RXB), 0, s, a);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}
}  // namespace
