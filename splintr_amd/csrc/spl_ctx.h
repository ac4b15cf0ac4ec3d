// spl_ctx.h -- what a handle IS: the per-GPU context (Ctx: tables, workspace, staging, streams -- every GPU resource an owner from
// spl_host_res.h -- and the chunk memo, one Memo that owns all of it), the handle, result and communicator structs of the C ABI, and what
// fills a context: upload_tables, upload_specials, upload_decode, reserve, ensure_streams.  A context holds what lasts from call to call;
// what one device call wants travels in its LaunchReq (spl_launch.h), never through a member here.
// Needs spl_host_res.h and the kernels' types (spl_kernels.hip, spl_tables.h, spl_regex.h, spl_comm.h).
#pragma once
#include <mutex>
namespace {

constexpr size_t QCOUNT_WORDS = 16;      // Batch::qcount
enum { KI_MARK = 0, KI_SPECIAL, KI_PRETOK, KI_DEFER, KI_BPELANES, KI_BPELONG, KI_COUNT, KI_SCAN, KI_COMPACT, KI_N };
const char* const k_names[KI_N] = {"memset+k_mark_docs", "k_special_scan", "k_pretok", "k_deferred_wave", "k_bpe_segments",
                                   "k_bpe_long", "k_range_count", "(unused)", "k_range_out|k_tile_out"};

struct Special { std::string lit; uint32_t id; };
constexpr int NSLOT = 3;                      // staging slots of the host pipeline per GPU

// The lookup tables of one handle on one GPU (upload_tables).  A context and its twin hold the same set.
struct TableSet {
    DevBuf<uint16_t> ucls_stage1; DevBuf<uint8_t> ucls_stage2;
    DevBuf<ShortEnt> short_tab; DevBuf<uint32_t> tiny_tab, t8_tab; DevBuf<LongEnt> long_tab; DevBuf<uint8_t> key_blob;
    DevBuf<uint64_t> pair_tab; DevBuf<uint32_t> byte_id, p8_tab; DevBuf<uint16_t> len_mask; DevBuf<PfxEnt> pfx; DevBuf<uint16_t> filt4;
    DevBuf<uint32_t> akind;
    DeviceTables view{};                       // what the kernels take by value (its memo fields stay empty: those are each context's own, Ctx::dt)
};

// The chunk memo of one context (spl_k_memo.h), everything of it: the table, the tiles' log of what it did not hold, one claim word per slot
// for k_memo_fill, the pinned flag the tiles raise, the counters.  Built as a whole by memo_ensure (spl_launch.h) and only then moved into
// the context; empty (false) until then and after Ctx::memo_drop.
struct Memo2Parts { MemoEnt* ent; MemoExt* ext; MemoHi* hi; uint32_t* claim; uint32_t* log; };      // (the parts of the second table's one allocation)
struct Memo {
    DevBuf<MemoEnt> d_tab; DevBuf<MemoExt> d_ext; DevBuf<uint32_t> d_log, d_log_cnt, d_claim;
    DevBuf<uint8_t> d_tab2;                   // the second table (chunks of 33..64 bytes), ONE allocation: entries | second lines | key bytes 32..63 | claim words | log
    uint32_t mask = 0, cap = 0, mask2 = 0, cap2 = 0;      // slots - 1 of either table; logged misses per region and fill
    DevBuf<unsigned long long> d_stats;
    HostMapped<uint32_t> h_flag;
    uint32_t round = 0;
    uint64_t fills = 0, since = 0;
    uint64_t seed_placed = 0, seed_left = 0;  // the vocabulary keys this memo was seeded with / that found neither slot free (memo_seed)
    explicit operator bool() const { return (bool)d_tab; }
    Memo2Parts parts2() const {
        const size_t s2 = (size_t)mask2 + 1;
        Memo2Parts m;
        m.ent = (MemoEnt*)d_tab2.get(); m.ext = (MemoExt*)(m.ent + s2); m.hi = (MemoHi*)(m.ext + s2); m.claim = (uint32_t*)(m.hi + s2); m.log = m.claim + s2;
        return m;
    }
    void tables(DeviceTables& dt) const {     // the memo fields of what the kernels take by value (all null for an empty memo)
        dt.memo = d_tab.get(); dt.memo_mask = mask; dt.memo_ext = d_ext.get();
        dt.memo2 = nullptr; dt.memo2_mask = 0; dt.memo2_ext = nullptr; dt.memo2_hi = nullptr;
        if (d_tab2) { const Memo2Parts m = parts2(); dt.memo2 = m.ent; dt.memo2_mask = mask2; dt.memo2_ext = m.ext; dt.memo2_hi = m.hi; }
    }
};

// Everything that lives on ONE GPU: lookup tables, workspace, and the host pipeline's streams and
// staging.  A handle has one context per device of spl_set_devices (one by default).  Every GPU resource is a member that
// frees itself (spl_host_res.h); the destructor only makes sure the device is idle and the twin goes first.
struct Ctx {
    int device = 0;
    std::shared_ptr<const TableSet> tables;
    DeviceTables dt{};                         // tables->view plus this context's memo
    DevBuf<uint32_t> d_tok_off;                // decode table (vocabulary + specials), rebuilt after spl_add_special
    DevBuf<uint8_t> d_tok_bytes;
    uint32_t dec_max_id = 0;
    DevBuf<uint32_t> d_dec_sp_ids, d_dec_sp_off; uint32_t dec_n_sp = 0;   // specials beyond the vocabulary's ids
    DevBuf<uint32_t> d_dec_spbits;             // one bit per id of the dense table: only the special map holds it (SPL_DECODE_SKIP_SPECIAL)
    DevBuf<uint16_t> d_dec_nch, d_dec_sp_nch;  // spl_token_spans_device: characters per dense id / per side-table entry (spl_k_spans.h: sn_entry)
    bool dec_uploaded = false;
    DevBuf<uint64_t> d_ddblk; uint64_t ddblk_cap = 0;   // spl_decode_batch_device: block sums, 8 bytes per 1 024 ids (grow-only; shared with nothing)
    DevBuf<uint64_t> d_stblk; uint64_t stblk_cap = 0;   // spl_stream_decode_device: block sums and per-sequence counts, 8 bytes per sequence and 8 per 16 of them (grow-only; shared with nothing)
    DevBuf<uint64_t> d_spblk; uint64_t spblk_cap = 0;   // spl_stop_match_device: block sums and per-sequence count, cut and hit, 24 bytes per sequence and 8 per 16 of them (grow-only; shared with nothing)
    DevBuf<uint64_t> d_snblk; uint64_t snblk_cap = 0;   // spl_token_spans_device: block sums of bytes and of characters, 16 bytes per 1 024 ids (grow-only; shared with nothing)
    DevBuf<uint32_t> d_heal_sorted, d_heal_rank, d_heal_parent; uint32_t heal_n = 0;   // spl_heal_*_device: the ordinary ids by their bytes, id -> rank, the prefix order (upload_heal; rebuilt after spl_add_special)
    bool heal_uploaded = false;
    DevBuf<uint32_t> d_heal_scr; uint64_t heal_cap = 0;   // ... lo, hi and up to 63 partial ids per sequence, 264 bytes each (grow-only; shared with nothing)
    DevBuf<uint64_t> d_jmscr; uint64_t jmscr_cap = 0;   // spl_dfa_jump_index_device: the runs' bytes CSR, their ids CSR and the scan's sums, 344 bytes per state (grow-only; shared with nothing)
    DevBuf<uint32_t> d_nsscr; uint64_t nsscr_cap = 0;   // spl_nest_index_device: the touching bitmap, a word per word of the index's rows, and a count per state (grow-only; shared with nothing)
    DevBuf<uint32_t> d_u8_present, d_u8_rows; uint32_t u8_stride = 0;   // spl_utf8_mask_device: the vocabulary proper as a bit per id, the class table's 17 rows of u8_stride words (upload_utf8; rebuilt after spl_add_special)
    bool u8_uploaded = false;
    DevBuf<uint8_t> d_sp_lits;                 // uploaded lazily; invalidated by spl_add_special
    bool sp_uploaded = false;
    // workspace
    uint64_t cap_bytes = 0, cap_docs = 0;
    DevBuf<uint32_t> d_zero;       // [tbits | tstart | skip | qcount]
    size_t zero_words = 0, bitmap_words = 0;
    DevBuf<uint32_t> d_stage;
    DevBuf<uint32_t> d_rank;
    uint32_t* d_aux = nullptr;    // inside d_rank's allocation
    DevBuf<uint2> d_q64, d_qlong; DevBuf<uint32_t> d_qdefer;
    uint32_t qcap64 = 0, qcaplong = 0, qcapdefer = 0;
    DevBuf<unsigned long long> d_dbg;
    DevBuf<uint32_t> d_blk;
    // tile-owned mode: tile records, the tiles' token slots, group sums; and whether the token bitmap may hold
    // stale bits (after hipMalloc or a multi-pass call) -- the single-pass kernel needs it all-zero
    DevBuf<TileDesc> d_tdesc;
    DevBuf<uint32_t> d_tile_bits, d_tcnt;     // queue mode
    DevBuf<uint32_t> d_tile_ids;
    DevBuf<uint32_t> d_tctl;
    uint32_t tgroups = 0, tpar = 0;
    // fused mode (spl_k_fuse.h): per parity the tiles' published token counts (FUSE_REPL copies of u16[FUSE_STRIDE], then the 32-bit side
    // array u32[FUSE_STRIDE]); a fused launch uses parity fpar and zeroes what the previous fused launch (fprev tiles) left in the other one
    DevBuf<uint8_t> d_fctl;
    uint32_t fpar = 0, fprev = 0;
    Memo memo;                                // chunk memo: empty until the first launch builds it (memo_ensure)
    // latency path (encode_small): text and offsets read where they lie in pinned host memory, completion by a word k_tile_out stores there
    uint32_t done_seq = 0;                    // the value the last call's completion word takes (it travels in that call's LaunchReq)
    HostMapped<uint8_t> h_small;              // pinned: [text 4096 + 64 | offsets 8 * 257 | completion word]
    uint32_t small_calls = 0;
    const void* dp_host[2] = {nullptr, nullptr}; void* dp_dev[2] = {nullptr, nullptr};   // device pointers of the last two pinned result buffers
    const uint8_t* solo_text = nullptr; const uint64_t* solo_off = nullptr;
    hsa_agent_t hsa_agent{}; int hsa_state = 0;    // this device's HSA agent for the SDMA copies (0 not looked for yet, 1 found, 2 none: hipMemcpyAsync)
    bool bitmap_dirty = true;
    // host pipeline (spl_encode_batch / spl_decode_batch)
    Stream s_cmp, s_h2d, s_d2h;
    DevBuf<uint8_t> d_text[NSLOT];
    DevBuf<uint64_t> d_off[NSLOT];
    uint64_t slot_cap_bytes = 0, slot_cap_docs = 0;
    DevBuf<uint32_t> d_ids; uint64_t ids_cap = 0;            // the lane's ids, chunk c at its byte offset
    DevBuf<uint64_t> d_oo; uint64_t oo_cap = 0;              // chunk-local output offsets, chunk after chunk
    // pipeline: the kernels of consecutive chunks alternate between this context and a TWIN on the same GPU -- a workspace and a compute
    // stream of its own, the tables shared -- so that chunk k + 1's tile kernel starts while the stragglers of chunk k's finish
    std::unique_ptr<Ctx> twin;
    bool streams_picked = false;              // the pipeline's copy streams have been chosen by measurement (pick_stream_beside)
    Pinned h_text[NSLOT], h_off[NSLOT], h_oo;          // h_oo: the pipeline chunks' local output offsets (k_tile_out writes them there: no copy, no count to fetch)
    uint64_t* dh_oo = nullptr;                          // its device-side address
    // custom split patterns: the chunk's boundary bitmaps (starts | gaps, back to back) and the special tokens the
    // host splitter found (positions | ids), per staging slot
    Pinned h_ext[NSLOT], h_extsp[NSLOT];
    DevBuf<uint32_t> d_ext[NSLOT]; uint64_t ext_cap_words = 0;
    DevBuf<uint32_t> d_extsp[NSLOT]; uint64_t extsp_cap = 0;
    // custom split patterns on the device (spl_rx_split.h): the program image, general categories, workspace, status word
    DevBuf<uint32_t> d_rx_image; DevBuf<uint16_t> d_gc1; DevBuf<uint8_t> d_gc2;
    DevBuf<uint8_t> d_rx_ws; uint64_t rx_ws_cap = 0, rx_cap_blk = 0; uint32_t rx_gen = 0xFFFFu;
    DevBuf<uint32_t> d_rx_status;                                   // RX_STATUS_SLOTS words, one per batch in rotation: a batch's k_rx_mark clears the next one's
    uint32_t rx_slot = 0;
    bool rx_next_clean = true;                                      // the next word of the rotation has been cleared (fresh memory; a k_rx_mark that ran)
    HostMapped<uint32_t> h_rx_status;                               // pinned copy: written behind every chunk's split, read when the batch is done
    DevBuf<uint32_t> d_rx_bits; uint64_t rx_bits_cap = 0;          // the two bitmaps of a device-text call (spl_encode_batch_device)
    DevBuf<uint32_t> d_rx_patch; uint64_t rx_patch_cap = 0;        // per-document fallback: the patch of one split (grow-only)
    DevBuf<uint32_t> d_rx_bad;                                      // [0] count, [1 .. RX_BAD_CAP] blocks the matcher gave up on (device list of one split)
    HostMapped<uint32_t> h_rx_bad;                                  // ... where k_rx_mark leaves it for the host (pinned)
    Event ev_split;                                                 // host pipeline: a chunk's split is through (the producer waits for it: per-document fallback)
    Event ev_h2d[NSLOT], ev_cmp[NSLOT];
    std::vector<Event> ev_chunk;
    // decode scratch (grow-only): the ids, their lengths' block sums, every id's offset, the documents' first ids and offsets, the bytes
    struct DecSlot {
        DevBuf<uint32_t> ids; DevBuf<uint64_t> blk, idoff, first, docoff;
        DevBuf<uint8_t> out; uint64_t cap_ids = 0, cap_docs = 0, cap_out = 0;
        Event ev_in, ev_len, ev_cp, ev_out;
    };
    DecSlot dec;                              // a batch decoded in one piece (its events stay unused)
    // decode pipeline (large batches): two slots of the same scratch, a second compute stream, events per slot
    DecSlot dslot[2];
    Stream s_dec2;
    Pinned h_dtot;
    // profiling
    bool prof = false;
    Event ev[KI_N + 1];
    // a large device batch as ranges of its tiles (launch_all): a second stream beside the caller's, one event per range (grow-only), the hand-overs
    Stream s_rng; hipStream_t s_rng_for = nullptr; std::vector<Event> ev_rng; Event ev_rng_in, ev_rng_out;
    bool ev_ready = false;
    double prof_ms[SPL_MAX_KERNELS]{};
    uint64_t prof_n[SPL_MAX_KERNELS]{};
    uint32_t* last_qcount = nullptr;
    bool dbg_on = false;
    int stop_phase = 0;     // spl_debug_phases bits 4..6 (profiling builds of the instruction mix per phase)
    int force_tile = 0;     // 0 auto, 1 small tiles, 4 queue mode, 5 tile-owned geometry B (spl_debug_phases bits 1..3; 2 and 3 are refused there)

    void free_workspace() {
        d_zero.reset(); d_stage.reset(); d_rank.reset(); d_aux = nullptr;
        d_q64.reset(); d_qlong.reset(); d_qdefer.reset(); d_blk.reset(); d_dbg.reset();
        d_tdesc.reset(); d_tile_ids.reset(); d_tctl.reset(); d_tile_bits.reset(); d_tcnt.reset(); d_fctl.reset();
        cap_bytes = cap_docs = 0;
    }
    void memo_drop() {                        // (a new geometry: the next launch builds an empty memo)
        if (!memo) return;
        if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return; }
        (void)hipDeviceSynchronize();
        memo = Memo{};
        memo.tables(dt);
    }
    void free_slots() {
        for (int i = 0; i < NSLOT; i++) { d_text[i].reset(); d_off[i].reset(); d_ext[i].reset(); d_extsp[i].reset(); }
        slot_cap_bytes = slot_cap_docs = 0; ext_cap_words = 0; extsp_cap = 0;
    }
    ~Ctx() {                                  // the device idle, the twin first; then the members, each freeing what it owns
        if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
        else (void)hipDeviceSynchronize();
        twin.reset();
    }
};

}  // namespace

struct spl_tokenizer {
    HostTables ht;
    // the memo's seed as last planned (memo_seed_plan, spl_tables.cpp), for the table sizes it was planned for: every context, every twin and every
    // memo built again behind clear_cache uploads this one
    std::mutex seed_mu;
    spl::MemoSeedPlan seed_plan;
    uint32_t seed_plan_bits = 0, seed_plan_long_bits = 0;
    bool seed_plan_valid = false;
    std::vector<Special> specials;
    uint32_t max_special_id = 0;
    mutable uint32_t max_tok_bytes = 0;       // spl_max_token_bytes, computed at its first call (0: not yet; spl_add_special resets it)
    bool special_newline = false;             // a literal contains '\n': no sub-document cuts with SPL_WITH_SPECIAL
    bool special_general = false;             // occurrences can overlap, or a literal exceeds SP_MAXLEN: the two-launch general matcher
    RegexPtr regex;                           // SPL_PATTERN_CUSTOM: the host splitter's program (null: one of the GPU scanner's patterns)
    std::vector<uint32_t> rx_image;           // ... and its image for the device splitter (empty: the program does not fit, the split stays on the host)
    int rx_device = 1;                        // spl_set_option("device_split"): 0 keeps a custom pattern's split on the host cores
    uint64_t rx_fallbacks = 0;                // DOCUMENTS the device splitter gave up on and the host split instead (spl_device_split_fallbacks)
    std::vector<std::unique_ptr<Ctx>> ctx;
    std::shared_ptr<PinnedPool> pool = std::make_shared<PinnedPool>();
    // host pipeline tuning (spl_set_option)
    uint64_t chunk_bytes = 5ull << 20;        // upper bound of one pipeline chunk (with the kernels of consecutive chunks on two streams 4 .. 6 MiB are best: C3 28.8 GB/s, 26.8 at 8 MiB)
    uint64_t single_max = 4ull << 20;         // batches up to this size run as ONE chunk
    uint32_t est_div = 2;                     // first guess of the token count: n_bytes / est_div
    int subdoc = 1;                           // cut documents at context-free boundaries to balance the GPUs
    int direct_write = 1;                     // one-chunk batches: the last kernel writes the ids straight into the pinned result
    int small_path = 1;                       // batches of up to 4 KB take the latency path (encode_small)
    int slab_pack24 = 0;                      // the ids of the all-gather slabs travel three bytes each (spl_set_option "slab_pack24": every rank alike)
    uint32_t stream_one_max = ST_ONE_DEFAULT;    // "stream_one_max": most sequences spl_stream_decode_device takes in its one-launch form
    uint32_t choice_piece = CH_PIECE;            // "choice_piece_words": tests and measuring only -- the words of a mask row spl_choice_step_device builds in LDS at once
    uint32_t heal_phase = 0;                     // "heal_phase": measuring only -- 1 the healing calls launch their plan alone, 2 their fill alone (over the scratch the last plan left)
    uint32_t jump_phase = 0;                     // "jump_phase": measuring only -- spl_dfa_jump_index_device returns behind 1 force and runs, 2 the compaction and its read-back, 3 the encode (the index is then incomplete)
    uint32_t stop_one_max = SP_ONE_DEFAULT;      // "stop_one_max": most sequences spl_stop_match_device takes in its one-launch form
    uint32_t seqpack_lds_max = SQP_LDS_MAX;  // "seqpack_lds_max" (tests): most sequences whose plan arrays spl_seqpack_device keeps in LDS, so that a few hundred reach the work-buffer form
    uint32_t win_chunk = WIN_CHUNK;          // "window_totals_chunk" (tests): span totals k_window_totals scans per round, so that a few thousand documents reach its second round
    int sdma_d2h = 0;                         // (measured, +0.5..3 %: not the default) pipeline chunks: their ids leave through hsa_amd_memory_async_copy (an SDMA engine) instead of hipMemcpyAsync
    uint64_t dec_chunk_ids = 2ull << 20;      // decode pipeline: ids per chunk (batches of fewer than three such chunks are decoded in one piece; C3: 28.3 GB/s at 1 M, 30.5 at 2 M, 29.6 at 3 M)
    int copy_threads = 4;                     // pipeline, pageable input: threads that copy a chunk into pinned staging
    int memo = 1;                             // the chunk memo (spl_k_memo.h); "memo_bits": log2 of its entries (64 bytes each), "memo_log_cap": logged misses per region and fill
    int memo_first = 1;                       // the memo is seeded with the vocabulary's keys and the tile kernel asks it BEFORE the vocabulary's tables (spl_k_pretok.h); 0: behind them, an unseeded memo
    uint32_t memo_bits = 20, memo_log_cap = 1024, memo_long_bits = 16;          // "memo_long_bits": log2 of the entries for chunks of 33..64 bytes (160 bytes each; 0: none)
    uint32_t range_tiles = 0;                 // "range_tiles" (measured, +2 % on the 215 MB configurations, -2 % on C3 in the bench line: not the default): batches of more than 1.25 x this many tiles go out as ranges of this many (k_pretok + k_tile_out per range; 0: one launch pair)
    uint32_t group_scan_min = 256;            // "group_scan_min": batches of more than this many groups of 64 tiles get the groups' prefix sums from k_group_scan (0: never)
    int range_streams = 2;                    // "range_streams": ... on the caller's stream alone (1) or alternating with a second one (2)
    int fuse = 1;                             // tile-owned mode as ONE launch (spl_k_fuse.h) for batches of up to fuse_max_tiles tiles; 0: k_pretok + k_tile_out
    uint32_t fuse_max_tiles = FUSE_MAX_TILES; // (every tile of such a launch is resident at once -- 256 CUs x 6 workgroups: a tile that waits for its base holds nobody up)
    int pick_streams = 1;                     // pipeline: its streams chosen by measurement so that they run side by side (pick_stream_beside)
    int twin_streams = 1;                     // pipeline: consecutive chunks' kernels on two streams / workspaces (Ctx::twin)
    int chunk_ramp = 0;                       // pipeline: a lane's first and last chunk are a quarter of the others (a shorter first H2D and last D2H)
    int direct_read = 1;                      // one-chunk batches from pinned memory: the tile kernel reads text and offsets where they lie (no H2D copy)
    uint64_t small_calls = 0;                 // ... and how many did (spl_small_path_calls)
};

// One rank of a node-wide communicator (one process per GPU; RCCL over xGMI).
struct spl_comm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    DevBuf<uint64_t> d_cnt;                   // [4] this rank's {T, N, capacity of its all_ids, of its all_off}
    DevBuf<uint64_t> d_cnts;                 // [4 * world] every rank's
    HostMapped<uint64_t> h_cnts;             // pinned copy
};

struct spl_result {
    std::shared_ptr<PinnedPool> pool;
    uint32_t* ids = nullptr; size_t ids_cap = 0;       // capacities in BYTES of the pinned buffers
    uint64_t* off = nullptr; size_t off_cap = 0;
    uint64_t n_tokens = 0, n_docs = 0;
    ~spl_result() { if (pool) { pool->put(ids, ids_cap); pool->put(off, off_cap); } }
};

namespace {

int upload_tables(Ctx& c, const HostTables& ht) {
    HIP_TRY(hipSetDevice(c.device));
    auto ts = std::make_shared<TableSet>();
    DeviceTables& dt = ts->view;
    SPL_TRY(ts->ucls_stage1.upload(ht.ucls_stage1)); dt.ucls_stage1 = ts->ucls_stage1.get();
    SPL_TRY(ts->ucls_stage2.upload(ht.ucls_stage2)); dt.ucls_stage2 = ts->ucls_stage2.get();
    SPL_TRY(ts->short_tab.upload(ht.short_tab)); dt.short_tab = ts->short_tab.get();
    SPL_TRY(ts->tiny_tab.upload(ht.tiny_tab)); dt.tiny_tab = ts->tiny_tab.get();
    SPL_TRY(ts->t8_tab.upload(ht.t8_tab)); dt.t8_tab = ts->t8_tab.get();
    SPL_TRY(ts->long_tab.upload(ht.long_tab)); dt.long_tab = ts->long_tab.get();
    SPL_TRY(ts->key_blob.upload(ht.key_blob)); dt.key_blob = ts->key_blob.get();
    SPL_TRY(ts->pair_tab.upload(ht.pair_tab)); dt.pair_tab = ts->pair_tab.get();
    SPL_TRY(ts->byte_id.upload(ht.byte_id)); dt.byte_id = ts->byte_id.get();
    SPL_TRY(ts->p8_tab.upload(ht.p8_tab)); dt.p8_tab = reinterpret_cast<const P8Bucket*>(ts->p8_tab.get());
    SPL_TRY(ts->len_mask.upload(ht.len_mask)); dt.len_mask = ts->len_mask.get();
    SPL_TRY(ts->pfx.upload(ht.pfx)); dt.pfx = ts->pfx.get();
    SPL_TRY(ts->filt4.upload(ht.filt4)); dt.filt4 = ts->filt4.get();
    dt.filt4_shift = ht.filt4_shift;
    dt.ucls_shift = ht.ucls_shift;
    dt.ascii_base = (uint32_t)ht.ucls_stage1[0] << ht.ucls_shift;
    {
        std::vector<uint32_t> ak(256);
        for (uint32_t ch = 0; ch < 128; ch++) {
            const KindEnt e = ascii_entry(ht.pattern, ch, ht.ucls_stage2[dt.ascii_base + ch]);
            ak[2 * ch] = e.x; ak[2 * ch + 1] = e.y;
        }
        SPL_TRY(ts->akind.upload(ak)); dt.akind = ts->akind.get();
    }
    dt.cjk_fast = ht.cjk_fast ? 1u : 0u;
    dt.short_mask = (uint32_t)(ht.short_tab.size() / SPL_SHORT_BUCKET) - 1;
    dt.tiny_mask = (uint32_t)((ht.tiny_tab.size() - 4) / SPL_TINY_WORDS) - 1;      // (slots; 4 words of padding behind them)
    dt.t8_mask = (uint32_t)((ht.t8_tab.size() - 4) / SPL_T8_WORDS) - 1;
    dt.long_mask = (uint32_t)ht.long_tab.size() - 1;
    dt.pair_mask = (uint32_t)(ht.pair_tab.size() / SPL_PAIR_BUCKET) - 1;
    dt.p8_mask = (uint32_t)(ht.p8_tab.size() / 2) - 1;
    dt.tiny_free = ht.tiny_free; dt.t8_free = ht.t8_free;
    dt.max_key_len = ht.max_key_len;
    dt.pattern = (uint32_t)ht.pattern;
    dt.all_bytes = ht.all_bytes ? 1u : 0u;
    dt.id_limit = ht.id_limit;
    c.dt = dt;
    c.tables = std::move(ts);
    return SPL_OK;
}

int ensure_streams(Ctx& c) {
    if (c.s_cmp) return SPL_OK;
    for (Stream* s : {&c.s_cmp, &c.s_h2d, &c.s_d2h}) SPL_TRY(s->create());
    for (int i = 0; i < NSLOT; i++) { SPL_TRY(c.ev_h2d[i].create()); SPL_TRY(c.ev_cmp[i].create()); }
    return SPL_OK;
}

int reserve(Ctx* t, uint64_t max_bytes, uint64_t max_docs) {
    if (max_bytes <= t->cap_bytes && max_docs <= t->cap_docs) return SPL_OK;
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    const uint64_t nb = std::max<uint64_t>(max_bytes, t->cap_bytes), nd = std::max<uint64_t>(max_docs, t->cap_docs);
    t->free_workspace();
    const size_t nblk = (size_t)(nb / RANK_BLK) + 2;
    t->bitmap_words = nblk * 32 + 64;
    t->zero_words = 4 * t->bitmap_words + QCOUNT_WORDS;      // tbits | tstart | skip | spcand, then the queue counters
    SPL_TRY(t->d_zero.alloc(t->zero_words));
    SPL_TRY(t->d_stage.alloc(nb + 8192));
    SPL_TRY(t->d_rank.alloc((nb + 8192) * 3));   // ranks + two words of aux per byte
    t->d_aux = t->d_rank.get() + (nb + 8192);
    const size_t tiles_s = (size_t)(nb / TileGeom<SPL_TILE_SMALL>::TBv) + 2;
    t->qcaplong = (uint32_t)(nb / 2 + 64);          // long chunks AND every miss of a deferred segment
    t->qcapdefer = (uint32_t)(2 * tiles_s + 64);
    t->qcap64 = (uint32_t)(nb / 17 + 64);
    SPL_TRY(t->d_q64.alloc(t->qcap64));
    SPL_TRY(t->d_dbg.alloc(16 + 4 * SPL_DEBUG_BLOCKS));
    SPL_TRY(t->d_qlong.alloc(t->qcaplong));
    SPL_TRY(t->d_qdefer.alloc(t->qcapdefer));
    SPL_TRY(t->d_blk.alloc(nblk + 2));
    {
        const size_t dbytes = (size_t)std::min<uint64_t>(nb, std::max<uint64_t>(SPL_DIRECT_MAX_BYTES, SPL_QUEUE_MAX_BYTES));
        const size_t tiles = dbytes / TileGeom<SPL_TILE_SMALL>::TBv + 2;
        t->tgroups = (uint32_t)(tiles / 64 + 2);
        SPL_TRY(t->d_tdesc.alloc(tiles));
        SPL_TRY(t->d_tile_ids.alloc(tiles * (size_t)(TileGeom<SPL_TILE_SMALL>::Wv + 1)));
        SPL_TRY(t->d_tile_bits.alloc(tiles * (size_t)TILE_BITS_W));
        SPL_TRY(t->d_tcnt.alloc(tiles));
        SPL_TRY(t->d_tctl.alloc_zeroed(16 + 2 * (size_t)t->tgroups + 2 + 2 * (size_t)t->tgroups));      // (control words, two parities of group sums, their prefix sums as u64)
        t->tpar = 0;
        SPL_TRY(t->d_fctl.alloc_zeroed(2 * FUSE_PARITY_BYTES));
        t->fpar = 0; t->fprev = 0;
    }
    t->bitmap_dirty = true;
    t->cap_bytes = nb;
    t->cap_docs = nd;
    return SPL_OK;
}

int upload_specials(spl_tokenizer* tk, Ctx* t) {
    if (t->sp_uploaded) return SPL_OK;
    std::vector<uint8_t> recs;
    if (!tk->special_general) {
        // 32-byte header: the set of FIRST bytes (256 bits); then one record per literal
        recs.assign(SP_HDR + tk->specials.size() * SP_REC + 16, 0);
        for (size_t k = 0; k < tk->specials.size(); k++) {
            const uint8_t c0 = (uint8_t)tk->specials[k].lit[0];
            recs[c0 >> 3] |= (uint8_t)(1u << (c0 & 7));
            uint8_t* r = recs.data() + SP_HDR + k * SP_REC;
            r[0] = (uint8_t)tk->specials[k].lit.size();
            memcpy(r + 4, &tk->specials[k].id, 4);
            memcpy(r + 8, tk->specials[k].lit.data(), tk->specials[k].lit.size());
        }
    } else {
        // general sets (k_special_ends / k_special_select): header = set of LAST bytes, records
        // {len, id, blob offset, last byte}, then the literal bytes
        const size_t n = tk->specials.size();
        recs.assign(SP_HDR + n * SPG_REC, 0);
        for (size_t k = 0; k < n; k++) {
            const std::string& lit = tk->specials[k].lit;
            const uint8_t cl = (uint8_t)lit.back();
            recs[cl >> 3] |= (uint8_t)(1u << (cl & 7));
            const uint32_t rec[4] = {(uint32_t)lit.size(), tk->specials[k].id, (uint32_t)(recs.size() - (SP_HDR + n * SPG_REC)), cl};
            memcpy(recs.data() + SP_HDR + k * SPG_REC, rec, 16);
            recs.insert(recs.end(), lit.begin(), lit.end());
        }
        recs.resize(recs.size() + 16, 0);
    }
    HIP_TRY(hipDeviceSynchronize());
    SPL_TRY(t->d_sp_lits.upload(recs));
    t->sp_uploaded = true;
    return SPL_OK;
}

// id -> bytes for decode: the vocabulary's decoder, then special_tokens_decoder for ids it lacks
// (Tokenizer::decode_bytes, src/core/tokenizer.rs:877-897).
int upload_decode(spl_tokenizer* tk, Ctx* t) {
    if (t->dec_uploaded) return SPL_OK;
    // dense id -> bytes table over the VOCABULARY's id range (special tokens fill the ids it lacks there);
    // special tokens beyond it go into a small sorted side table
    const uint32_t max_id = tk->ht.max_id;
    std::vector<const Special*> sp(max_id + 1, nullptr);
    std::vector<const Special*> far;
    for (const auto& s : tk->specials) {                      // (two literals with one id: the later one, as a map insert)
        if (s.id <= max_id) sp[s.id] = &s;
        else {
            bool seen = false;
            for (auto& f : far) if (f->id == s.id) { f = &s; seen = true; }
            if (!seen) far.push_back(&s);
        }
    }
    std::sort(far.begin(), far.end(), [](const Special* a, const Special* b) { return a->id < b->id; });
    std::vector<uint32_t> off(max_id + 2, 0), sp_bits(max_id / 32 + 1, 0);
    std::vector<uint8_t> bytes;
    bytes.reserve(tk->ht.tok_bytes.size() + 4096);
    for (uint32_t id = 0; id <= max_id; id++) {
        off[id] = (uint32_t)bytes.size();
        const bool in_vocab = tk->ht.tok_present[id];
        if (in_vocab) bytes.insert(bytes.end(), tk->ht.tok_bytes.begin() + tk->ht.tok_off[id], tk->ht.tok_bytes.begin() + tk->ht.tok_off[id + 1]);
        else if (sp[id]) { bytes.insert(bytes.end(), sp[id]->lit.begin(), sp[id]->lit.end()); sp_bits[id >> 5] |= 1u << (id & 31); }
    }
    off[max_id + 1] = (uint32_t)bytes.size();
    std::vector<uint32_t> sp_ids, sp_off;
    for (const Special* f : far) {
        sp_ids.push_back(f->id);
        sp_off.push_back((uint32_t)bytes.size());
        bytes.insert(bytes.end(), f->lit.begin(), f->lit.end());
    }
    sp_off.push_back((uint32_t)bytes.size());
    // characters per id (spl_token_spans_device), from the same bytes
    std::vector<uint16_t> nch(max_id + 1, 0), sp_nch(sp_ids.size(), 0);
    auto entry = [&](uint32_t a, uint32_t b) { return b - a > SN_MAX_TOKEN_BYTES ? (uint16_t)0 : sn_entry(bytes.data() + a, b - a); };      // (such a handle is refused there)
    for (uint32_t id = 0; id <= max_id; id++) nch[id] = entry(off[id], off[id + 1]);
    for (size_t k = 0; k < sp_ids.size(); k++) sp_nch[k] = entry(sp_off[k], sp_off[k + 1]);
    HIP_TRY(hipDeviceSynchronize());
    SPL_TRY(t->d_tok_off.upload(off));
    SPL_TRY(t->d_tok_bytes.upload(bytes));
    SPL_TRY(t->d_dec_sp_ids.upload(sp_ids));
    SPL_TRY(t->d_dec_sp_off.upload(sp_off));
    SPL_TRY(t->d_dec_spbits.upload(sp_bits));
    SPL_TRY(t->d_dec_nch.upload(nch));
    SPL_TRY(t->d_dec_sp_nch.upload(sp_nch));
    t->dec_n_sp = (uint32_t)sp_ids.size();
    t->dec_max_id = max_id;
    t->dec_uploaded = true;
    return SPL_OK;
}
}  // namespace
