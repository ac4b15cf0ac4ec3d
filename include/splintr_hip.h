/* splintr_hip.h -- C ABI of the MI355X (gfx950) batch BPE encoder.
 *
 * The reference (ml-rust/splintr v0.8.0) has no C ABI: its only boundary is the PyO3 class
 * `Tokenizer` (src/python/bindings.rs:57-446) over `core::Tokenizer` (src/core/tokenizer.rs).
 * Each entry point below names the reference interface it stands in for; INTEGRATION.md shows the
 * binding a maintainer would add on the reference side (a `mod hip` FFI block in Rust, or the
 * ctypes class this repo ships as splintr_amd.Tokenizer).
 *
 * Conventions: plain pointers and sizes, no exceptions, no aborts.  Functions returning int
 * return SPL_OK (0) or a negative SPL_E* code; spl_last_error() gives the thread-local message.
 * Text is UTF-8, documents are packed back to back: doc d = utf8[doc_off[d] .. doc_off[d+1]).
 * Results are CSR: ids[T] (u32) + out_off[n_docs+1] (u64), in document order -- the flattened
 * form of the reference's Vec<Vec<u32>>.  A handle is bound to one GPU (spl_set_devices: to
 * several, for the host entry point); one batch in flight per handle; different handles may be
 * used from different threads.
 *
 * Text that is not valid UTF-8 (the reference's core only ever sees &str, so it defines nothing
 * here): every byte that is not part of a well-formed sequence -- a stray continuation byte, a lead
 * byte with too few continuation bytes behind it -- is ONE character of the class "other"
 * ([^\s\p{L}\p{N}]); a lead byte takes the continuation bytes actually present (at most as many as
 * it announces) and the decoded value is looked up as it is (overlong forms and surrogates are not
 * rejected).  Nothing is dropped or replaced: the ids always decode back to the input bytes
 * (tests/test_gpu_parity.py::test_invalid_utf8_policy pins this against the oracle).
 */
#ifndef SPLINTR_HIP_H
#define SPLINTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPL_OK 0
#define SPL_EINVAL (-1)   /* bad argument / malformed table blob */
#define SPL_EDEVICE (-2)  /* HIP runtime error (no GPU, out of memory, launch failure) */
#define SPL_ECAPACITY (-3)/* caller-provided output buffer too small */

/* Split pattern ids: CL100K_BASE_PATTERN (src/core/tokenizer.rs:39), O200K_BASE_PATTERN (:42;
 * also LLAMA3_PATTERN :45 and deepseek_v3, src/python/bindings.rs:116-129). */
#define SPL_PATTERN_CL100K 0
#define SPL_PATTERN_O200K 1
/* MISTRAL_V3_PATTERN (src/core/tokenizer.rs:64; mistral_v3 / Tekken, src/python/bindings.rs:152-158) */
#define SPL_PATTERN_MISTRAL_V3 2
/* These three are the patterns the GPU scanner implements as closed forms.  ANY OTHER pattern (Tokenizer::new compiles whatever it
 * is given, src/core/tokenizer.rs:410-456): SPL_PATTERN_CUSTOM with the pattern text in spl_opts.  It is compiled by csrc/spl_regex.h
 * (a backtracking matcher over the same code-point class table: literals, classes, \s \d \w, every general category and -- with a
 * version-3 class table -- every SCRIPT as \p{..} (\p{Han}, \p{Hiragana}, \p{Latin} ...), groups, (?i:), (?>), alternation, greedy /
 * lazy / possessive quantifiers, look-ahead, ^ $ \A \Z \z \b \B -- upstream tiktoken's cl100k_base / o200k_base strings, Qwen2's and
 * GPT-2's are accepted as they are) and its split runs ON THE GPU (csrc/spl_rx_split.h: the same matcher program at every text position,
 * the walk from each document's start by pointer doubling) in front of the same probe / merge kernels; documents that hold something the
 * device matcher gives up on -- a match longer than ~1 KB -- are split on the host cores instead, one by one (spl_device_split_fallbacks).
 * What the matcher cannot express (binary properties, script extensions, look-behind, back-references, \p{Lu} under (?i), a pattern that
 * can match the empty string) is refused by spl_create with the construct named. */
#define SPL_PATTERN_CUSTOM 3

/* spl_opts.flags */
#define SPL_OPT_BYTE_LEVEL 1u /* Tokenizer::from_bytes_byte_level (src/core/tokenizer.rs:562-569): the
                                 vocabulary's keys are ByteLevel text (src/core/byte_level.rs:46-74) */

/* encode flags */
#define SPL_WITH_SPECIAL 1u /* encode_with_special semantics (src/core/tokenizer.rs:842-874) */
#define SPL_INTRA_DOC 2u    /* encode_rayon (tokenizer.rs:815-837): accepted, no effect -- the GPU
                               path is always chunk-parallel inside a document, output identical */

typedef struct spl_tokenizer spl_tokenizer;
typedef struct spl_result spl_result;

typedef struct spl_opts {
    uint32_t struct_size; /* sizeof(spl_opts) as the CALLER was compiled: fields beyond it read as 0, so the struct
                             can grow without breaking callers built against an earlier header (ABI versioning) */
    int32_t pattern;      /* SPL_PATTERN_* */
    int32_t device;       /* HIP device ordinal */
    uint32_t flags;       /* SPL_OPT_* */
    const char* pattern_text; /* SPL_PATTERN_CUSTOM: the split pattern, UTF-8, pattern_len bytes (no terminator needed) */
    uint64_t pattern_len;
} spl_opts;

/* Thread-local text of the last failure in this thread. */
const char* spl_last_error(void);

/* Number of visible HIP devices (0 if none / no driver). */
int spl_device_count(void);

/* Tokenizer::from_bytes / from_bytes_byte_level (src/core/tokenizer.rs:552-569) + with_full_options
 * (:410-456): parse the vocabulary and the code-point class table (tools/gen_unicode_tables.py),
 * build the lookup tables and upload them to the device.  Returns NULL on failure.
 * `vocab` is either the reference's on-disk format -- tiktoken text, one `base64(token) rank` per
 * line, parsed as load_tiktoken_bpe does (src/core/vocab.rs:57-89: last space separates, rank
 * trimmed, a later duplicate key replaces the earlier one) -- or this repo's packed SPLV container
 * (tools/pack_vocab.py), told apart by the container's magic.
 * Restrictions (refused with SPL_EINVAL): ids must be < 2^21 - 1 (2 097 150 at most; the pseudo ids of missing single bytes, max id + 1 + k, included); two different keys must not share an id; a ByteLevel vocabulary must hold
 * all 256 alphabet characters, each ranking below every longer token.  A vocabulary that LACKS single bytes is taken as the reference
 * takes it (src/core/bpe.rs:73-75, 99-111, 182-191: pairs are ranked by their concatenated bytes, a node whose bytes are no token is
 * dropped from the result): the missing bytes get pseudo ids behind the vocabulary's for the merge loops and are never emitted.
 * Keys of up to 8 bytes live in single-slot tables built by hash-and-displace: keys that share a two-byte prefix (1..4-byte keys, 16-bit
 * salt) or a four-byte-prefix filter slot (5..8-byte keys, 10-bit salt) share a salt; a table in which some group finds no salt is
 * doubled, up to 2^24 slots (4 000 keys under one two-byte prefix: 2^20 slots).  Only a group of more than about ten thousand keys is
 * refused (SPL_EINVAL, "could not give every key of the ... table a slot of its own"); the reference's hash map has no
 * such limit. */
spl_tokenizer* spl_create(const void* vocab, size_t vocab_len, const void* uclass_tab, size_t uclass_len,
                          const spl_opts* opts);

/* The GPUs spl_encode_batch spreads a host batch over (the degenerate form of the multi-GPU path:
 * one process, documents sharded by bytes, every GPU copies its part of the CSR straight into the
 * one pinned result).  Replaces the handle's device list; the tables are uploaded to each.  The same
 * ordinal may be listed more than once (independent pipelines on one GPU).  The device-pointer
 * entry points keep using the first device of the list. */
int spl_set_devices(spl_tokenizer* t, const int32_t* devices, uint32_t n);
uint32_t spl_n_devices(const spl_tokenizer* t);

/* Tuning switches (name, value; measurements behind each default: DESIGN.md section 5 and profiles/).
 *   "chunk_bytes"            upper bound of one pipeline chunk of spl_encode_batch (default 5 MiB)
 *   "single_chunk_max_bytes" batches up to this size run as ONE chunk (default 4 MiB)
 *   "result_estimate_div"    first guess of the token count = bytes / div (default 2; a result that outgrows it moves to a larger buffer)
 *   "subdoc_split"           0/1 (1): balance the GPUs by cutting large documents at context-free boundaries
 *   "direct_write"           0/1 (1): one-chunk batches -- the last kernel writes the ids straight into the pinned result
 *   "direct_read"            0/1 (1): one-chunk batches whose text comes from spl_host_alloc are read where they lie (no H2D copy)
 *   "device_split"           0/1 (1): a custom split pattern's split runs on the GPU (spl_split_device); 0 keeps it on the host cores
 *   "small_path"             0/1 (1): batches of at most 4 KB and 256 documents take the latency path (spl_small_path_calls)
 *   "memo"                   0/1 (1): the chunk memo (spl_memo_stats); "memo_bits" 4..22 (20): log2 of its entries for chunks of up to 32 bytes
 *                            (128 bytes each); "memo_long_bits" 0..20 (16; 0: none): ... for chunks of 33..64 bytes (164 bytes each);
 *                            "memo_log_cap" 1..65536 (1024): missed chunks the tiles log per region (of 64) between two fills
 *   "memo_first"             0/1 (1): a new memo is SEEDED with the vocabulary's keys of 2..64 bytes (spl_memo_seed_stats) and the tile kernel asks
 *                            it before the vocabulary's tables -- one memory trip for a vocabulary token and a learned chunk alike; 0: the memo
 *                            holds learned chunks only and is asked behind the tables.  Same results.  Changing it empties the memo ("memo_clear").
 *   "memo_clear"             (any value) empties the memo of every context: Tokenizer::clear_cache (src/core/tokenizer.rs:995-1000)
 *   "group_scan_min"         0..2^24 (256; 0: never): a batch of more than this many groups of 64 tiles gets the groups' prefix sums from one small launch
 *                            (k_group_scan) between k_pretok and k_tile_out instead of every tile adding up the sums of the groups in front of it
 *   "range_tiles"            0..2^24 (0: one launch pair): a device-resident batch of more than 1.25 x this many tiles goes out as ranges of its tiles --
 *                            k_pretok and k_tile_out per range -- alternating between the caller's stream and a second one ("range_streams" 1/2 (2))
 *   "fuse"                   0/1 (1): batches of up to "fuse_max_tiles" tiles (default and maximum 1536: about 1.2 MB) are ONE launch --
 *                            every tile learns the number of tokens in front of it from the other tiles' published counts and writes its
 *                            part of the CSR itself; 0: the tile kernel and k_tile_out, as for larger batches
 *   "twin_streams"           0/1 (1): the kernels of consecutive pipeline chunks run on two compute streams with a workspace each
 *   "pick_streams"           0/1 (1): the pipeline's copy streams and second compute stream are chosen by measurement at first use
 *                            (spl_pick_stream) so that they run side by side; costs 5-80 ms once per context
 *   "copy_threads"           1..64 (4): threads that copy a chunk of pageable text into pinned staging
 *   "chunk_ramp"             0/1 (0): a lane's first and last chunk a quarter of the others
 *   "sdma_d2h"               0/1 (0): the ids of a pipeline chunk leave through hsa_amd_memory_async_copy (an SDMA engine) instead of
 *                            hipMemcpyAsync; hipMemcpyAsync where the HSA runtime cannot be bound
 *   "decode_chunk_ids"       >= 1024 (2^21): spl_decode_batch pipelines batches of at least three such chunks through two slots
 *   "window_totals_chunk"    1..256 (256; for tests): the span totals spl_window_device's second scan launch takes per round, so that a batch
 *                            of a few thousand documents reaches its second round
 *   "stream_one_max"         0..1024 (64): spl_stream_decode_device takes its one-launch form up to this many sequences, the three-launch
 *                            form beyond (0: always three; profiles/stream_decode.txt has the measured crossing)
 *   "stop_one_max"           0..1024 (64): spl_stop_match_device takes its one-launch form up to this many sequences, the three-launch form
 *                            beyond (0: always three; profiles/stop_match.txt has the measured crossing)
 *   "heal_phase"             0..2 (0): measuring only -- 1: spl_heal_begin_device / spl_heal_step_device launch their plan alone, 2: their fill
 *                            alone, over the scratch the last plan left (profiles/token_mask.txt)
 *   "jump_phase"             0..3 (0): measuring only -- spl_dfa_jump_index_device returns behind 1: force and runs, 2: the compaction
 *                            and the read-back of its total, 3: the encode; the jump index is then incomplete (profiles/dfa_jump.txt)
 *   "slab_pack24"            0/1 (0): the ids of the all-gather slabs travel three bytes each; every rank alike; refused (SPL_EINVAL) when an
 *                            id of the tokenizer -- vocabulary or special token -- does not fit 24 bits
 * Unknown names and values out of range: SPL_EINVAL. */
int spl_set_option(spl_tokenizer* t, const char* name, int64_t value);
/* The current value of a switch of spl_set_option (every name above but "memo_clear", which holds nothing).  A null argument or an
 * unknown name: SPL_EINVAL, *value untouched. */
int spl_get_option(const spl_tokenizer* t, const char* name, int64_t* value);

/* One entry of the special_tokens map (src/core/tokenizer.rs:304, 429-434).  Call before the first
 * encode.  Literals are non-empty and at most 255 bytes; adding a literal again replaces its id.
 * Matching follows the reference's matcher (Aho-Corasick, MatchKind::Standard, non-overlapping
 * find_iter, tokenizer.rs:849-869): from the end of the previous match, the occurrence that ends
 * first, the longest one on a tie.  Sets in which no two occurrences can overlap (no literal
 * contains another, no proper suffix of one is a prefix of another or of itself, all literals <= 32
 * bytes -- every pretrained table) take a one-launch scan in which every occurrence is a match; any
 * other set takes a two-launch matcher (candidate ends, then a per-document walk). */
int spl_add_special(spl_tokenizer* t, const uint8_t* literal, size_t len, uint32_t id);

/* Tokenizer::vocab_size (src/core/tokenizer.rs:964-972): max id over vocab and specials, plus 1. */
uint32_t spl_vocab_size(const spl_tokenizer* t);

void spl_destroy(spl_tokenizer* t);

/* Pre-size the device workspace for batches of up to max_bytes / max_docs, so that later encode
 * calls neither allocate nor synchronise. */
int spl_reserve(spl_tokenizer* t, uint64_t max_bytes, uint64_t max_docs);

/* Tokenizer::encode_batch / encode_batch_with_special (src/core/tokenizer.rs:932-942) on HOST
 * buffers -- what PyTokenizer::encode_batch (src/python/bindings.rs:337-339) calls.  The batch is
 * cut into chunks of whole documents that flow through pinned staging -> H2D -> kernels -> D2H on
 * private streams, three chunks in flight per GPU, and over the GPUs of spl_set_devices.  `utf8`
 * may be pageable (it is copied through pinned staging) or come from spl_host_alloc (DMA reads it
 * directly).  *out lives in pinned memory owned by the library; release with spl_result_free (the
 * buffers are recycled; a result stays valid after spl_destroy). */
int spl_encode_batch(spl_tokenizer* t, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                     uint32_t flags, spl_result** out);
/* The latency path (Tokenizer::encode of ONE text, src/core/tokenizer.rs:729-808 -- "~50 MB/s", :266-268): a batch of at most 4096 bytes and
 * 256 documents on a handle with a built-in pattern does not go through the chunk pipeline.  The CPU copies text and offsets into one small
 * pinned buffer, the tile kernel reads them there (a few cache lines over PCIe) and writes ids and offsets into the pinned result; the last
 * tile to finish stores, behind a system-scope fence, a completion word the calling thread spins on: ONE launch ("fuse"), no copy engine,
 * no stream synchronisation.  spl_set_option("small_path", 0) turns the path off; spl_small_path_calls counts the calls that took it.
 * (Latencies per text size: DESIGN.md section 7.) */
uint64_t spl_small_path_calls(const spl_tokenizer* t);
const uint32_t* spl_result_tokens(const spl_result* r);   /* ids[T] */
const uint64_t* spl_result_offsets(const spl_result* r);  /* out_off[n_docs+1] */
uint64_t spl_result_n_tokens(const spl_result* r);
uint64_t spl_result_n_docs(const spl_result* r);
void spl_result_free(spl_result* r);

/* Pinned (page-locked, all-device) host memory for callers that build the packed corpus themselves. */
void* spl_host_alloc(size_t bytes);
void spl_host_free(void* p);

/* Same path with everything resident in HBM (device pointers).  Fully asynchronous on `hip_stream`
 * (a hipStream_t; NULL = the default stream) once spl_reserve has sized the workspace.
 *   d_utf8[n_bytes]       corpus, 16-byte aligned (SPL_EINVAL otherwise) and readable up to the next
 *                         multiple of 16; doc offsets d_doc_off[n_docs+1] with d_doc_off[0]==0,
 *                         d_doc_off[n_docs]==n_bytes
 *   d_ids[ids_capacity]   output ids; n_bytes entries always suffice
 *   d_out_off[n_docs+1]   output offsets; d_out_off[n_docs] is the total token count
 * What the call promises about the caller's buffers, in every execution mode and for every entry point that takes these arguments
 * (_packed, spl_encode_chunks_device, handles with SPL_PATTERN_CUSTOM; tests/test_gpu_encode_buffers.py), T being the token count:
 *   capacity   Tokens beyond ids_capacity are dropped (compare d_out_off[n_docs] with the capacity): d_ids[0 .. min(T, ids_capacity))
 *              are the first ids of the result, d_out_off is complete whatever the capacity is -- d_out_off[n_docs] == T, the NEED --
 *              and nothing is stored at or beyond d_ids[ids_capacity].  ids_capacity 0 is allowed (d_ids must still be a valid pointer).
 *   footprint  Nothing is stored at or beyond d_ids[T] either: with ids_capacity > T the entries d_ids[T .. ids_capacity) keep what the
 *              caller left in them.  Nothing is stored in front of d_ids[0] or outside d_out_off[0 .. n_docs].
 *   text tail  The bytes behind d_utf8[n_bytes] (up to the next multiple of 16) are read but never looked at: the result is that of
 *              the n_bytes bytes alone, whatever follows them -- zeros, text that would continue the last chunk, invalid UTF-8.
 * Size limits of ONE device call (SPL_EINVAL beyond them; spl_encode_batch on host buffers has none, it feeds
 * chunks of at most 5 MiB): n_bytes < 2^31 - 65536 (2047 MiB) without SPL_WITH_SPECIAL, n_bytes <= 256 MB with it and for handles with
 * SPL_PATTERN_CUSTOM (the special-token scan and the device splitter exist for the two-launch mode only).  Split a larger corpus at
 * document boundaries.
 * What is asynchronous: a handle with one of the three built-in patterns enqueues its kernels on `hip_stream` and returns -- no host
 * synchronisation, with or without SPL_WITH_SPECIAL.  A handle with SPL_PATTERN_CUSTOM synchronises `hip_stream` ONCE before it returns
 * (to read which documents, if any, the device splitter gave up on; see below).  All calls on one handle -- this one, spl_split_device,
 * spl_encode_chunks_device, spl_encode_batch -- share the handle's workspace: they must be stream-ordered (issued on the same stream, or
 * with the earlier one complete); different handles are independent. */
int spl_encode_batch_device(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                            uint64_t n_docs, uint32_t flags, uint32_t* d_ids, uint64_t ids_capacity,
                            uint64_t* d_out_off, void* hip_stream);

/* Handles with SPL_PATTERN_CUSTOM: spl_encode_batch / spl_decode_batch work as for every other handle (the split of each pipeline chunk
 * runs on the device splitter, csrc/spl_rx_split.h, behind the GPU's special-token scan with SPL_WITH_SPECIAL).  What the device matcher
 * gives up on is handled per DOCUMENT: the 256-byte blocks of such positions come back in a small pinned list, the documents they lie in
 * are split on the host cores by the calling (producer) thread -- while the previous chunk's tile kernel runs -- and their stretch of the
 * two bitmaps is patched before the tile kernel reads it; every other document keeps the device split.  Only a list that overflows (more
 * than 1024 such blocks in one chunk: a pattern that gives up everywhere) sends the whole batch through the host splitter.
 * spl_encode_batch_device / _packed run splitter and tile kernel in one go and synchronise `hip_stream` ONCE before they return; if
 * documents need the host, THEIR text (nothing else) is copied back, split, patched, and the tile kernel runs again on the patched bitmaps.
 * The halves are available separately:
 *   spl_split_host          the matches of the handle's pattern over a packed HOST corpus as two bitmaps of
 *                           n_bytes / 32 + 2 words each (zeroed here): bit p of start_bits -- a chunk, or a stretch of
 *                           bytes no match covers, starts at byte p; bit p of gap_bits -- byte p is dropped
 *                           (find_iter semantics, tokenizer.rs:729-808).  Multi-threaded over documents.
 *   spl_encode_chunks_device  spl_encode_batch_device with the chunk boundaries GIVEN (device copies of the two
 *                           bitmaps; any handle: the handle's own pattern is not consulted).  Up to 256 MB per call. */
int spl_split_host(spl_tokenizer* t, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t* start_bits,
                   uint32_t* gap_bits);
/*   spl_split_device        the same two bitmaps for a packed corpus that is in HBM, by the device splitter (the same matcher
 *                           program, one text position per lane, then the walk from each document's start by pointer doubling:
 *                           csrc/spl_rx_split.h), asynchronously on `hip_stream`.  Bitmaps of n_bytes / 32 + 2 words (zeroed
 *                           here); *d_status (one word, device memory, cleared by the CALLER -- calls may share it) is non-zero
 *                           afterwards if the text held something the device matcher gives up on (a match or look-ahead
 *                           reaching more than ~1 KB beyond its start, a runaway attempt): the bitmaps are then incomplete
 *                           and the split belongs to spl_split_host.  SPL_EINVAL if the pattern's program does not fit the
 *                           device matcher.  spl_encode_batch uses it for every batch and falls back by itself, document by document
 *                           (spl_set_option "device_split" 0 keeps the split on the host cores; spl_device_split_fallbacks counts the
 *                           DOCUMENTS the host split instead -- all of a batch's if the whole batch went there).  Up to 256 MB per call.
 *                           Shares the handle's splitter workspace with the encode calls: stream-ordered with them (see above). */
int spl_split_device(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                     uint32_t* d_start_bits, uint32_t* d_gap_bits, uint32_t* d_status, void* hip_stream);
uint64_t spl_device_split_fallbacks(const spl_tokenizer* t);
int spl_encode_chunks_device(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                             uint64_t n_docs, const uint32_t* d_start_bits, const uint32_t* d_gap_bits, uint32_t* d_ids,
                             uint64_t ids_capacity, uint64_t* d_out_off, void* hip_stream);

/* Ragged all-gather of the CSR result across the GPUs of a node (north_star: "RCCL all-gatherv
 * over xGMI"; the reference has nothing distributed).  RCCL has no all-gatherv, so every rank
 * packs {T, N, local offsets, ids} into a fixed-capacity slab of u32 words, ONE all-gather of
 * equal-sized slabs moves them (spl_allgather_slabs below, or the caller's own collective, e.g.
 * torch.distributed all_gather_into_tensor), and every rank unpacks the `world` slabs into the global CSR in
 * rank order.  Both kernels are asynchronous on `hip_stream`; no host synchronisation is needed
 * because the counts travel inside the slabs.
 *   slab: [0] T, [1] N, [2 .. 2+max_docs] local out_off, then ids; cap_words >= max_docs + 4.
 *   d_status[0] is set to 1 by the unpacker if any rank's ids exceeded its slab (re-run larger). */
int spl_gatherv_pack(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs,
                     uint32_t* d_slab, uint64_t cap_words, uint64_t max_docs, void* hip_stream);
int spl_gatherv_unpack(spl_tokenizer* t, const uint32_t* d_slabs, uint32_t world, uint64_t cap_words,
                       uint64_t max_docs, uint32_t* d_all_ids, uint64_t all_ids_cap, uint64_t* d_all_off,
                       uint32_t* d_status, void* hip_stream);
/* spl_encode_batch_device that ALSO leaves the result in slab form (the layout spl_gatherv_pack
 * makes) in d_slab[cap_words]: in tile-owned mode the last kernel writes both copies in one pass,
 * so the per-batch pack launch of a multi-GPU pipeline goes away; otherwise the pack kernel is
 * queued behind the encode.  The slab's header and offsets are complete whatever ids_capacity is.  With ids_capacity below the token
 * count the slab's ids at ranks >= ids_capacity are promised NOTHING: the tile-owned mode fills them from the tiles' own ids, the queued
 * pack kernel copies min(T, slab capacity, ids_capacity) ids out of d_ids and leaves the rest of the slab as it was. */
int spl_encode_batch_device_packed(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                                   uint64_t n_docs, uint32_t flags, uint32_t* d_ids, uint64_t ids_capacity,
                                   uint64_t* d_out_off, uint32_t* d_slab, uint64_t cap_words, uint64_t max_docs,
                                   void* hip_stream);
/* Bucketed form (fewer, larger collectives: xGMI rings are per-link bound and a collective has a
 * fixed launch cost): every rank packs up to `depth` consecutive batches into `depth` slabs laid
 * back to back, ONE all-gather moves world x depth slabs, and one launch unpacks the first
 * n_batches of them: batch j's global CSR goes to d_all_ids + j * all_ids_cap and
 * d_all_off + j * off_stride. */
int spl_gatherv_unpack_group(spl_tokenizer* t, const uint32_t* d_slabs, uint32_t world, uint32_t depth, uint32_t n_batches,
                             uint64_t cap_words, uint64_t max_docs, uint32_t* d_all_ids, uint64_t all_ids_cap,
                             uint64_t* d_all_off, uint64_t off_stride, uint32_t* d_status, void* hip_stream);

/* From the CSR to what a model on the same GPU reads: padding and sequence packing ON THE DEVICE, one launch each behind the encode on
 * the same stream.  The reference has no counterpart: it returns Vec<Vec<u32>> (src/core/tokenizer.rs:932-942) and leaves both to the caller.
 * Both calls are fully asynchronous on `hip_stream`, neither allocate nor synchronise, use the handle only for its device (as
 * spl_gatherv_pack does) and take ANY CSR with d_out_off[0] == 0 in device memory, not only one the handle produced.  The ids must
 * actually be there: after an encode whose d_out_off[n_docs] exceeded its ids_capacity the values of the dropped range are unspecified.
 * Ids are bit patterns (a special token's id may be any u32): int32 rows store the 32 bits, int64 rows (SPL_COLLATE_I64) ZERO-extend,
 * never sign-extend.  k = (BOS ? 1 : 0) + (EOS ? 1 : 0) below.
 *
 *   spl_pad_device   d_rows[n_docs, row_len]: row d = [bos_id] + tokens_d' + [eos_id], where tokens_d' is document d's ids cut to the
 *                    budget row_len - k -- the head is kept; with SPL_COLLATE_KEEP_TAIL the tail -- and BOS / EOS are never cut away.
 *                    The rest of the row is pad_id, on the right (SPL_COLLATE_PAD_LEFT: on the left).  d_mask[d, c] (bytes, NULL:
 *                    not wanted) = 1 where the entry is not padding, d_len[d] (NULL: not wanted) = the number of such entries
 *                    (k for an empty document).  n_docs == 0: nothing to do.
 *   spl_pack_device  the stream = the concatenation over d of [bos_id] tokens_d [eos_id], S = d_out_off[n_docs] + n_docs * k entries,
 *                    cut into n_rows = ceil(S / row_len) rows; nothing is truncated.  Element (r, c) is stream position
 *                    p = r * row_len + c.  For p < S its document is the LARGEST d with d_out_off[d] + d * k <= p (empty documents add
 *                    nothing when k == 0 and are skipped), j = p minus that start; the value is bos_id if BOS is on and j == 0,
 *                    eos_id if EOS is on and j == len_d + BOS, ids[d_out_off[d] + j - BOS] otherwise; d_doc[p] = d (the index
 *                    within the batch) and d_pos[p] = p - max(start_d, r * row_len): positions restart at a document's start and at a
 *                    row's start, a row being the attention context.  For p >= S, up to the end of the buffer: pad_id, d_doc = -1,
 *                    d_pos = 0.  Every element of the rows_cap rows is written, nothing at or beyond them; d_n[0] always receives
 *                    n_rows -- the need: compare it with rows_cap, as d_out_off[n_docs] with ids_capacity -- and d_n[1] receives S.
 *                    n_docs == 0 or S == 0: d_n = {0, 0}.  d_doc / d_pos [rows_cap * row_len] may be NULL.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null required pointer (d_rows is required
 * where there is a row to write); a struct_size of 0, shorter than the fields below or above 4096 (a longer struct up to that is accepted, its
 * tail ignored, as for spl_opts); row_len == 0; pad mode with row_len < k; SPL_COLLATE_PAD_LEFT or _KEEP_TAIL in pack mode; an unknown flag bit; d_rows,
 * d_doc, d_pos or d_len not 16-byte aligned, d_mask not 4-byte aligned; n_docs >= 2^31; rows_cap * row_len beyond 2^63. */
#define SPL_COLLATE_I64       1u   /* rows are int64 (torch.long); default int32 */
#define SPL_COLLATE_PAD_LEFT  2u   /* pad mode only */
#define SPL_COLLATE_KEEP_TAIL 4u   /* pad mode only: truncation drops the FRONT of a document */
#define SPL_COLLATE_BOS       8u
#define SPL_COLLATE_EOS       16u

typedef struct spl_collate_opts {
    uint32_t struct_size;   /* sizeof the struct as the CALLER was compiled: versioned exactly like spl_opts */
    uint32_t flags, row_len, pad_id, bos_id, eos_id;
} spl_collate_opts;

int spl_pad_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs,
                   const spl_collate_opts* o, void* d_rows /* [n_docs*row_len] */, uint8_t* d_mask /* NULL ok */,
                   int32_t* d_len /* NULL ok */, void* hip_stream);
int spl_pack_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs,
                    const spl_collate_opts* o, void* d_rows /* [rows_cap*row_len] */, uint64_t rows_cap,
                    int32_t* d_doc /* NULL ok */, int32_t* d_pos /* NULL ok */, uint64_t* d_n /* [2] */, void* hip_stream);

/* PAIRS: two CSRs joined into one row per pair of documents -- what a cross-encoder, a reranker, an NLI / QA model or an "instruction +
 * input" template reads, and what Hugging Face tokenizers call text_pair, with token_type_ids and the longest_first / only_first /
 * only_second truncation strategies.  The reference has no counterpart, as for pad and pack; the same conventions hold: one launch, fully
 * asynchronous on `hip_stream`, nothing allocated, nothing synchronised, the handle used only for its device, ANY CSRs in device memory,
 * ids as bit patterns (SPL_COLLATE_I64 zero-extends).  The two texts are encoded SEPARATELY (joining the strings first changes the
 * tokens at the seam), and a document that many pairs name -- one query against a thousand candidates -- is encoded once and read by each.
 *
 * Offsets   document i of a side is ids[off[i] .. off[i + 1]), i < n; the offsets are ABSOLUTE into that side's ids array and off[0] need
 *           not be 0.  The two sides may therefore be two slices of ONE encode result of n_a + n_b documents: d_a_ids = d_b_ids = its
 *           d_ids, d_a_off = its d_out_off, d_b_off = its d_out_off + n_a -- one encode launch for both sides.
 * Pairs     pair p takes document ia = d_a_idx ? d_a_idx[p] : p of A and ib = d_b_idx ? d_b_idx[p] : p of B (d_a_idx / d_b_idx
 *           [n_pairs], device memory).  An index that is negative, or at or beyond its side's document count, names an EMPTY document
 *           for that pair, and d_status[0] is set to 1 (a plain store of 1; the caller clears the word before the call and a call without
 *           such an index leaves it alone).  Nothing is read out of range.
 * Row       k = n_prefix + n_middle + n_suffix, B = row_len - k (the budget of the two documents together).  Row p is
 *           prefix + A' + middle + B' + suffix, then pad_id -- padding on the right, or on the left with SPL_COLLATE_PAD_LEFT.  The
 *           fixed segments (HOST arrays in the options, passed to the kernel by value) are on every row and never cut away:
 *           [CLS] a [SEP] b [SEP] is prefix = {CLS}, middle = {SEP}, suffix = {SEP}; RoBERTa's <s> a </s></s> b </s> has a middle of two ids.
 * Cut       la, lb = the two documents' lengths; a', b' = the ids kept.  la + lb <= B: both whole.  Otherwise, by `trunc`:
 *             SPL_PAIR_ONLY_SECOND    a' = min(la, B), b' = min(lb, B - a')
 *             SPL_PAIR_ONLY_FIRST     b' = min(lb, B), a' = min(la, B - b')
 *             SPL_PAIR_LONGEST_FIRST  Hugging Face's sequential rule: while a' + b' > B remove one id from the longer side, from B on a
 *                                     tie.  Evaluated in closed form, with hA = ceil(B / 2) and hB = floor(B / 2): la < hA gives
 *                                     (la, B - la); otherwise lb <= hB gives (B - lb, lb); otherwise (hA, hB).
 *           A' is the HEAD of document ia (its first a' ids), with SPL_PAIR_KEEP_TAIL_A its tail (its last a'); B' likewise with _B.
 * Outputs   every output is optional (NULL: not wanted) except d_rows; every element of every array that is given is written and
 *           nothing is written at or beyond n_pairs rows.  d_rows[p, c]: the row.  d_mask[p, c] = 1 where the entry is not padding.
 *           d_type[p, c] = 0 over prefix + A' + middle, 1 over B' + suffix, 0 on padding (BERT's token_type_ids).  d_special[p, c] = 1
 *           on the entries of the fixed segments and on padding, 0 on ids that come from a document (Hugging Face's special_tokens_mask
 *           after padding).  d_len[p] = k + a' + b'.  d_kept[2p], d_kept[2p + 1] = a', b': compare them with the documents' lengths to
 *           see what was truncated.  n_pairs == 0: nothing to do.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the handle or the device: a null handle, null options, a
 * null d_rows, d_a_off, d_b_off or d_status (always), null d_a_ids or d_b_ids with n_pairs > 0; a struct_size shorter than the struct
 * or above 4096 (a longer struct up to that is accepted, its tail ignored); an unknown flag bit; SPL_COLLATE_KEEP_TAIL, _BOS or _EOS
 * (the fixed segments and SPL_PAIR_KEEP_TAIL_A / _B take their place); trunc > 2; a segment count above SPL_PAIR_MAX_FIXED; row_len == 0
 * or row_len < k; n_a, n_b or n_pairs >= 2^31; a NULL index array with n_pairs above that side's document count; n_pairs * row_len beyond
 * 2^63; d_rows, d_len or d_kept not 16-byte aligned; d_mask, d_type, d_special, d_a_idx or d_b_idx not 4-byte aligned. */
#define SPL_PAIR_MAX_FIXED   32u    /* ids per fixed segment */
#define SPL_PAIR_KEEP_TAIL_A 32u    /* truncation drops the FRONT of side A (default: the head is kept) */
#define SPL_PAIR_KEEP_TAIL_B 64u
/* also accepted: SPL_COLLATE_I64, SPL_COLLATE_PAD_LEFT (same values, same meaning) */
#define SPL_PAIR_LONGEST_FIRST 0u
#define SPL_PAIR_ONLY_FIRST    1u
#define SPL_PAIR_ONLY_SECOND   2u

typedef struct spl_pair_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled: versioned exactly like spl_collate_opts */
    uint32_t flags, row_len, pad_id, trunc;
    uint32_t n_prefix, n_middle, n_suffix;          /* each 0 .. SPL_PAIR_MAX_FIXED */
    uint32_t prefix[32], middle[32], suffix[32];    /* HOST values, passed to the kernel by value */
} spl_pair_opts;

int spl_pair_device(spl_tokenizer* t,
                    const uint32_t* d_a_ids, const uint64_t* d_a_off, uint64_t n_a,
                    const uint32_t* d_b_ids, const uint64_t* d_b_off, uint64_t n_b,
                    const int32_t* d_a_idx /* [n_pairs], NULL: identity */, const int32_t* d_b_idx /* same */,
                    uint64_t n_pairs, const spl_pair_opts* o,
                    void* d_rows /* [n_pairs*row_len] */, uint8_t* d_mask, uint8_t* d_type, uint8_t* d_special,
                    int32_t* d_len /* [n_pairs] */, int32_t* d_kept /* [n_pairs*2] */,
                    uint32_t* d_status /* one word, cleared by the caller */, void* hip_stream);

/* CHAT: a CSR of MESSAGES joined into one row per multi-turn CONVERSATION, with a label mask -- what an instruction-tuned model reads and
 * what Hugging Face calls apply_chat_template with tokenize=True and return_assistant_tokens_mask=True.  Every message is wrapped in its role's control tokens
 * (ChatML's <|im_start|>role\n ... <|im_end|>\n, llama3's <|start_header_id|>role<|end_header_id|>\n\n ... <|eot_id|>), the turns are joined, and
 * only the turns of the trained roles carry labels.  spl_pair_device is the special case of two segments; this call has N turns, wrappers
 * per role, labels, and can drop the oldest turns.  The reference has no counterpart, as for pad, pack and pairs; the same conventions hold:
 * fully asynchronous on `hip_stream`, nothing allocated, nothing synchronised, the handle used only for its device, ANY CSR in device
 * memory, ids as bit patterns (SPL_COLLATE_I64 zero-extends).  The messages are encoded SEPARATELY and the control tokens come from the
 * options, never from message text: a message that contains the literal of a control token cannot forge a turn, and a message that many
 * conversations name -- a shared system prompt -- is encoded once and read by each.  Two launches: one wavefront per conversation scans
 * its turns, then a gather writes every output element once.
 *
 * Messages  document i is ids[off[i] .. off[i + 1]), i < n_docs; the offsets are ABSOLUTE into d_ids and off[0] need not be 0.
 * Turns     turn t (t < n_turns) has the role d_turn_role[t] (a byte, 0 .. n_roles - 1) and the content document
 *           d_turn_doc ? d_turn_doc[t] : t; it is TRAINABLE if d_turn_train ? d_turn_train[t] != 0 : true.  Conversation c (c < n_convs) owns
 *           the turns [d_conv_off[c], d_conv_off[c + 1]) -- a CSR over the turns.
 * Template  HOST values in the options: for every role r its header[r][0 .. n_header[r]) and footer[r][0 .. n_footer[r]); bos[0 .. n_bos)
 *           in front of every row; gen[0 .. n_gen), the generation prompt (an assistant header, for sampling), behind every row's body;
 *           n_gen == 0: none.  train_content and train_footer are bit masks over the roles (bit r: role r).
 * Body      the body of conversation c is the concatenation over its turns, in order, of header[r] + content + footer[r], r the turn's
 *           role, content the turn's document.  Its budget is B = row_len - n_bos - n_gen.  Row c is bos + body' + gen, then pad_id --
 *           padding on the right, or on the left with SPL_COLLATE_PAD_LEFT.  bos and gen are never cut away.
 * Cut       default: body' = the first min(len(body), B) entries of the body; the cut may fall inside a header, a content or a footer.
 *           SPL_CHAT_DROP_OLDEST: whole leading turns are removed instead.  t0 = the smallest turn index (within the conversation) for
 *           which the kept body -- the turns from t0 on -- has at most B entries.  With SPL_CHAT_PIN_FIRST (valid only together with
 *           DROP_OLDEST; it keeps a system prompt) the kept body is turn 0 followed by the turns from t0 on, t0 >= 1 the smallest such
 *           index for which turn 0 plus these turns have at most B entries; a conversation of fewer than two turns has nothing to drop.
 *           If no t0 fits, only the conversation's LAST turn is kept (after turn 0 when pinned), and that body is cut on the right at
 *           B like the default.  With no turn dropped the result equals the default.
 * Bad input is never read out of range and sets d_status[0] = 1 (a plain store of 1; the caller clears the word before the call and a
 *           call without bad input leaves it alone): a role >= n_roles -- the turn contributes NOTHING (no header, content or footer);
 *           a document index that is negative or >= n_docs -- the turn's content is empty (header and footer remain); a conversation
 *           whose turn range is reversed (d_conv_off[c + 1] < d_conv_off[c]) or reaches beyond n_turns -- it has no turns.  Only turns
 *           that a valid conversation contains are looked at: a bad turn outside every conversation is not reported.  Turn ranges that
 *           OVERLAP (one of them is then reversed, and reported) leave the rows and d_turn_col of the conversations involved
 *           unspecified; nothing is read or written out of range.
 * Outputs   every output is optional (NULL: not wanted, not written) except d_rows, d_status and d_work; every element of every array
 *           that is given is written -- d_turn_col with the exception below -- and nothing at or beyond n_convs rows.  An entry of a row
 *           is TRAINED if it is content of a turn that is trainable and whose role is in train_content, or footer of such a turn
 *           whose role is also in train_footer (the end-of-turn token the model must learn to emit).  Headers, bos, gen and padding are never trained.
 *             d_rows[c, col]      the row.
 *             d_labels[c, col]    same dtype as the rows: a trained entry holds its id (zero-extended in int64), every other entry
 *                                 ignore_id -- in int64 SIGN-extended from 32 bits, because -100 (0xFFFFFF9C) is a number.  Labels
 *                                 are not shifted; the model shifts.
 *             d_loss[c, col]      bytes: 1 on trained entries, 0 elsewhere.
 *             d_mask[c, col]      bytes: 1 where the entry is not padding.
 *             d_role[c, col]      bytes: the turn's role over its header, content and footer; SPL_CHAT_NO_ROLE on bos, gen and padding.
 *             d_special[c, col]   bytes: 1 on template entries (bos, headers, footers, gen) and on padding, 0 on ids from a document.
 *             d_len[c]            n_bos + len(body') + n_gen, the entries that are not padding.
 *             d_kept[2c]          the turns dropped (0 without DROP_OLDEST); d_kept[2c + 1] the entries of the kept body cut off on the
 *                                 right (saturated at 2^31 - 1).  Either being nonzero means truncation.
 *             d_turn_col[2t], d_turn_col[2t + 1]   the columns [c0, c1) of turn t's CONTENT in its conversation's row, clipped to the
 *                                 row; t is the turn's index in the d_turn_role array, not within its conversation.
 *                                 (-1, -1) for a dropped turn, for a turn wholly behind the cut -- one whose content begins
 *                                 at or behind the cut --, and for a bad turn (role or document index).  A content that is empty and
 *                                 begins before the cut gives c0 == c1.  d_rows[c, c0 .. c1) are the ids of the document that are in
 *                                 the row: mask a tool output, read back one message.  A turn that NO valid conversation contains is
 *                                 not written: fill the array before the call if such turns exist.
 *           d_len and d_turn_col are int32 like d_len of the pairs: for rows of 2^31 entries or more they hold the low 32 bits.
 *           n_convs == 0: nothing to do.
 * Work      d_work: spl_chat_work_bytes(n_turns, n_convs) bytes of device memory, 16-byte aligned, for this call alone until it has run
 *           (the template copy, one record per conversation, one start per turn).  The size is a pure function of its two arguments,
 *           monotone in both and a multiple of 16.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the handle or the device: a null handle, null options, a null
 * d_rows, d_off, d_conv_off, d_status or d_work (always), null d_turn_role with n_turns > 0, null d_ids with n_docs > 0; a struct_size
 * shorter than the struct or above 4096 (a longer struct up to that is accepted, its tail ignored); an unknown flag bit;
 * SPL_COLLATE_KEEP_TAIL, _BOS or _EOS; SPL_CHAT_PIN_FIRST without SPL_CHAT_DROP_OLDEST; n_roles outside 1 .. 8; n_bos > 8, n_gen > 16,
 * n_header[r] > 16 or n_footer[r] > 8 for a role r < n_roles; a bit of train_content or train_footer at or above n_roles; row_len == 0 or
 * row_len < n_bos + n_gen; n_docs, n_turns or n_convs >= 2^31; a NULL d_turn_doc with n_turns > n_docs; n_convs * row_len beyond 2^63;
 * d_rows, d_labels, d_len, d_kept, d_turn_col or d_work not 16-byte aligned; d_loss, d_mask, d_role, d_special or d_turn_doc not 4-byte
 * aligned; d_conv_off not 8-byte aligned. */
#define SPL_CHAT_DROP_OLDEST 32u    /* truncation removes whole leading turns (default: the body is cut on the right) */
#define SPL_CHAT_PIN_FIRST   64u    /* with DROP_OLDEST: turn 0 of every conversation is kept */
/* also accepted: SPL_COLLATE_I64, SPL_COLLATE_PAD_LEFT (same values, same meaning) */
#define SPL_CHAT_NO_ROLE     255u   /* d_role on bos, gen and padding */
#define SPL_CHAT_MAX_ROLES   8u
#define SPL_CHAT_MAX_HEADER  16u    /* ids per role header */
#define SPL_CHAT_MAX_FOOTER  8u     /* ids per role footer */
#define SPL_CHAT_MAX_BOS     8u
#define SPL_CHAT_MAX_GEN     16u

typedef struct spl_chat_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled: versioned exactly like spl_collate_opts */
    uint32_t flags, row_len, pad_id, ignore_id;
    uint32_t n_roles, train_content, train_footer;  /* 1 .. 8; bit masks over the roles */
    uint32_t n_bos, n_gen;                          /* 0 .. 8, 0 .. 16 */
    uint32_t n_header[8], n_footer[8];              /* each 0 .. 16, each 0 .. 8 */
    uint32_t bos[8], gen[16];                       /* HOST values, passed to the kernel by value */
    uint32_t header[8][16], footer[8][8];
} spl_chat_opts;

uint64_t spl_chat_work_bytes(uint64_t n_turns, uint64_t n_convs);
int spl_chat_device(spl_tokenizer* t,
                    const uint32_t* d_ids, const uint64_t* d_off, uint64_t n_docs,
                    const int32_t* d_turn_doc /* [n_turns], NULL: identity */, const uint8_t* d_turn_role /* [n_turns] */,
                    const uint8_t* d_turn_train /* [n_turns], NULL: all 1 */, uint64_t n_turns,
                    const uint64_t* d_conv_off /* [n_convs + 1] */, uint64_t n_convs, const spl_chat_opts* o,
                    void* d_rows /* [n_convs*row_len] */, void* d_labels /* same */, uint8_t* d_loss, uint8_t* d_mask, uint8_t* d_role,
                    uint8_t* d_special, int32_t* d_len /* [n_convs] */, int32_t* d_kept /* [n_convs*2] */,
                    int32_t* d_turn_col /* [n_turns*2] */, uint32_t* d_status /* one word, cleared by the caller */,
                    void* d_work /* spl_chat_work_bytes */, void* hip_stream);

/* WHOLE-SEQUENCE PACKING: n_seqs sequences binned into rows of row_len, several per row and NONE CUT IN TWO -- what a fine-tuning or
 * reranker trainer does to a padded batch before the model sees it (torchtune's PackedDataset, TRL's packing / padding_free, NeMo's
 * sequence packing).  Labels and up to four byte arrays travel with the ids, position ids restart at every sequence, and the boundaries
 * come out in the form a variable-length attention kernel takes.  spl_pack_device is the pre-training form (one stream cut every row_len,
 * documents cross rows, ids only); this call keeps every sequence whole.  The reference has no counterpart; the conventions of the
 * collate family hold: fully asynchronous on `hip_stream`, nothing allocated, nothing synchronised, the handle used only for its device
 * and its test options, ids as bit patterns.  Two launches: ONE workgroup plans, a gather writes every output element once.
 *
 * Input     exactly one of two forms, named by which of in->d_lengths and in->d_off is not NULL:
 *             rows form  d_ids [n_seqs, in_len] of the ROWS' dtype (int32, or int64 with SPL_COLLATE_I64: the low 32 bits are the id),
 *                        d_lengths int32 [n_seqs]; sequence i is d_ids[i, 0 .. len) -- or d_ids[i, in_len - len .. in_len) with
 *                        SPL_COLLATE_PAD_LEFT (the INPUT is left padded) -- as spl_pad_device, spl_pair_device and spl_chat_device leave it.
 *             CSR form   d_ids int32 [capacity], d_off [n_seqs + 1]: sequence i is d_ids[off[i] .. off[i + 1]), offsets ABSOLUTE, as
 *                        spl_encode_batch_device leaves it.  The ids (and labels) of a CSR are int32 whatever dtype the rows have.
 *           Companions in the layout AND element type of d_ids, each optional (NULL): d_labels; d_bytes[0 .. 3], uint8.
 * Clipping  a sequence's length is min(len, row_len): a longer one is cut and keeps its head, or its tail with SPL_COLLATE_KEEP_TAIL.
 *           A sequence of length 0 takes no place.
 * Placement o->strategy:
 *             SPL_SEQPACK_NEXT_FIT             order preserving.  Walk the sequences in index order with a current row fill f: a
 *                        non-empty sequence of clipped length l opens a new row if there is no row yet or f + l > row_len; it lands at
 *                        column f of the current row, then f += l.
 *             SPL_SEQPACK_BEST_FIT_DECREASING  the non-empty sequences are taken by clipped length DESCENDING, ties by ascending index.
 *                        Each goes into the open row whose residual capacity is the smallest one >= l; among rows of that same residual
 *                        into the one that reached that residual most recently (LIFO); if no row has room it opens a new row.  Rows are
 *                        numbered in opening order; within a row the sequences sit in placement order without gaps.
 *                        row_len <= SPL_SEQPACK_BFD_MAX_ROW_LEN (a table over the residuals lives in the 160 KB of a workgroup's LDS),
 *                        and ONE LANE places the sequences one after the other: measured at 0.9 us per sequence (1.2 us at row_len
 *                        16 384) where NEXT_FIT's whole plan costs 0.01 us per sequence (profiles/seqpack.txt, 2 500 sequences).
 *                        Beyond about 4 000 sequences -- where this walk outlasts the gather of a [2500, 16384] batch -- take
 *                        NEXT_FIT unless the rows saved (1 to 2 % there) are worth milliseconds.
 *           Worked by hand (the rows as lists of sequence indices):
 *             row_len 10, lengths 6 5 5 4             NEXT_FIT [0] [1 2] [3];  BEST_FIT_DECREASING [0 3] [1 2]
 *             row_len 10, lengths 3 0 7 1 12 10 5 5   NEXT_FIT [0 2] [3] [4] [5] [6 7] (sequence 1 unplaced, sequence 4 cut to 10);
 *                                                     BEST_FIT_DECREASING [4] [5] [2 0] [6 7] [3]
 *             row_len 7,  lengths 4 4 3 3 3 3         BEST_FIT_DECREASING [0 3] [1 2] [4 5] (the LIFO tie)
 *           Both plans run in one workgroup, which for n_seqs beyond a few thousand keeps its arrays in d_work instead of LDS: correct
 *           for every n_seqs < 2^31, but sized for batches (thousands of sequences), not corpora.  (For tests, spl_set_option
 *           "seqpack_lds_max", 0 .. 4096, default 4096, lowers the n_seqs up to which the arrays are in LDS.)
 * Outputs   out->d_rows, d_status and d_work are required, every other output is optional (NULL: not wanted, not written).  The
 *           [max_rows, row_len] arrays are written in full -- rows from n[0] on hold only padding -- and nothing behind them.
 *             d_rows       the ids; padding holds pad_id.
 *             d_labels     the rows' dtype; padding holds ignore_id; with SPL_SEQPACK_MASK_FIRST the entry at every sequence's FIRST
 *                          column holds ignore_id too (labels are not shifted: the model would otherwise learn a sequence's first
 *                          token from its neighbour's last).  In int64 a word equal to ignore_id is SIGN-extended (it is a number),
 *                          any other word ZERO-extended (an id).  Written only if in->d_labels is given as well.
 *             d_bytes[k]   byte array k; padding holds o->fill[k].  Written only if in->d_bytes[k] is given as well.
 *             d_mask       bytes: 1 where the entry is not padding.
 *             d_pos        int32: position ids, 0 at every sequence's first column, 0 in padding.
 *             d_seq        int32: the source sequence's index, -1 in padding.
 *             d_place      int32 [n_seqs, 2]: (row, column) of every sequence, (-1, -1) for an empty one.  Rows at or beyond max_rows
 *                          are reported here although they are not written.
 *             d_fill       int32 [max_rows]: the entries of a row that are not padding (0 from the rows written on).
 *             d_cu         int32 [n_seqs + max_rows + 1]: the ascending boundaries of the flattened view of the rows WRITTEN
 *                          (W = min(n[0], max_rows)): every sequence start row * row_len + column, the start of every row's padding
 *                          tail where it has one, and the closing W * row_len.  n[2] entries; the rest is not written.  (With max_rows
 *                          >= n[0] the closing entry is n[0] * row_len and the array is what a varlen attention call takes as it is.)
 *             d_n          int64 [4]: rows needed, ids placed (of all rows needed), entries of d_cu, sequences cut.
 *             d_status     one word, cleared by the caller; a plain store of 1 for a length below 0 or above in_len, or offsets that
 *                          decrease.  Such a sequence counts as empty.
 * Capacity  max_rows = n_seqs always suffices.  With fewer rows than needed the rows beyond max_rows are not written and n[0] still
 *           reports the need (spl_pack_device's contract).  NEXT_FIT never uses more than 2 * ceil(ids / row_len) rows.
 * Work      d_work: spl_seqpack_work_bytes(n_seqs, max_rows, strategy) bytes of device memory, 16-byte aligned, for this call alone
 *           until it has run.  A pure function of its arguments, monotone in the first two, a multiple of 16.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null handle, in, o, out, d_rows, d_status or
 * d_work; a struct_size shorter than a struct or above 4096; both input forms or neither; null d_ids with n_seqs > 0; an unknown flag
 * bit (SPL_COLLATE_BOS, _EOS are not flags of this call; SPL_COLLATE_PAD_LEFT only in the rows form); an unknown strategy;
 * row_len == 0; BEST_FIT_DECREASING with row_len > SPL_SEQPACK_BFD_MAX_ROW_LEN; n_seqs >= 2^31 or max_rows >= 2^31; max_rows * row_len
 * >= 2^31 with d_cu given (it is int32); the rows form with in_len == 0 while n_seqs > 0; d_rows, d_labels, d_pos, d_seq, d_place,
 * d_fill, d_cu, d_n or d_work not 16-byte aligned; a byte output or d_mask not 4-byte aligned; d_lengths not 4-byte, d_off not 8-byte
 * aligned.  The element type of d_ids cannot be seen from a pointer: the Python layer refuses a tensor of the wrong dtype. */
#define SPL_SEQPACK_NEXT_FIT            0u
#define SPL_SEQPACK_BEST_FIT_DECREASING 1u
#define SPL_SEQPACK_MASK_FIRST          32u   /* the label at every sequence's first column is ignore_id */
/* also accepted: SPL_COLLATE_I64, SPL_COLLATE_PAD_LEFT (the input rows are left padded), SPL_COLLATE_KEEP_TAIL */
#define SPL_SEQPACK_BFD_MAX_ROW_LEN     32768u

typedef struct spl_seqpack_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled */
    uint32_t flags, strategy, row_len, pad_id, ignore_id;
    uint8_t fill[4];                      /* what pads byte array k */
} spl_seqpack_opts;
typedef struct spl_seqpack_in {
    uint32_t struct_size, in_len;         /* in_len: the columns of the input rows (rows form) */
    uint64_t n_seqs;
    const void* d_ids; const int32_t* d_lengths; const uint64_t* d_off;
    const void* d_labels; const uint8_t* d_bytes[4];
} spl_seqpack_in;
typedef struct spl_seqpack_out {
    uint32_t struct_size, reserved;
    uint64_t max_rows;
    void* d_rows; void* d_labels; uint8_t* d_bytes[4]; uint8_t* d_mask;
    int32_t* d_pos; int32_t* d_seq; int32_t* d_place; int32_t* d_fill; int32_t* d_cu; int64_t* d_n;
    uint32_t* d_status;
} spl_seqpack_out;

uint64_t spl_seqpack_work_bytes(uint64_t n_seqs, uint64_t max_rows, uint32_t strategy);
int spl_seqpack_device(spl_tokenizer* t, const spl_seqpack_in* in, const spl_seqpack_opts* o, const spl_seqpack_out* out,
                       void* d_work /* spl_seqpack_work_bytes */, void* hip_stream);

/* SLIDING WINDOWS over the CSR: every document alone and complete, as rows of row_len that overlap by `overlap` ids -- the one
 * per-document layout that loses nothing (pad mode truncates, pack mode joins documents), and what Hugging Face tokenizers call
 * return_overflowing_tokens with stride = overlap.  The reference has no counterpart, as for pad and pack; the same conventions hold:
 * fully asynchronous on `hip_stream`, nothing allocated, nothing synchronised, the handle used only for its device, ANY CSR with
 * d_out_off[0] == 0, ids as bit patterns (SPL_COLLATE_I64 zero-extends).  spl_collate_opts is the struct of pad and pack, unchanged;
 * accepted flags: SPL_COLLATE_I64, _PAD_LEFT, _BOS, _EOS.
 *
 * k = BOS + EOS, B = row_len - k (the body budget, at least 1), overlap in 0 .. B - 1, step = B - overlap.  For document d of len_d ids:
 *   rows       n_w(d) = 1 if len_d <= B, else 1 + ceil((len_d - B) / step).  Every document has at least one row: an empty one's
 *              holds its k specials and padding, as in pad mode.
 *   window w   holds ids [w * step, min(w * step + B, len_d)) of the document, as [bos_id] + body + [eos_id], the rest pad_id -- on the
 *              right, or on the left with SPL_COLLATE_PAD_LEFT.  BOS and EOS are on every row; only a document's last window can be short.
 *   row index  d_row_off[d] = the sum of n_w(i) over i < d (exclusive; strictly increasing), d_row_off[n_docs] = the number of rows.
 *              Row r belongs to the largest d with d_row_off[d] <= r, and is its window w = r - d_row_off[d].
 * Outputs: d_rows[r, c] and d_mask[r, c] (1 where the entry is not padding) as in pad mode; d_len[r] = the entries of row r that are not
 * padding; d_row_doc[r] = d; d_row_start[r] = w * step, the body's first id within its document; d_row_off[n_docs + 1], the CSR of rows
 * per document (what a caller reduces over, to mean-pool a document's windows for example); d_n[0] = d_row_off[n_docs], the NEED --
 * compare it with rows_cap, as d_out_off[n_docs] with ids_capacity -- and d_n[1] = min(d_n[0], rows_cap), the rows that hold documents.
 * d_row_off and d_n are always written in full, also when rows_cap is too small or 0.  Every element of every per-row and per-element
 * array below rows_cap is written -- rows from d_n[0] on: pad_id, mask 0, len 0, doc -1, start 0 -- and nothing at or beyond rows_cap.
 * n_docs == 0: d_row_off[0] = 0, d_n = {0, 0}, every row padding.
 * d_work: spl_window_work_bytes(n_docs) bytes of device memory, a pure function of n_docs (0 for up to 4096 documents, where one launch
 * computes d_row_off; beyond that three launches do, through the workspace, and no workgroup of them ever waits for another one).
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the handle or the device: everything spl_pad_device
 * refuses; row_len <= k; overlap >= row_len - k; SPL_COLLATE_KEEP_TAIL (nothing is truncated); a null d_row_off or d_n; a null d_work
 * when spl_window_work_bytes(n_docs) > 0; d_rows, d_len, d_row_doc, d_row_start or d_row_off not 16-byte aligned, d_mask not 4-byte
 * aligned, d_work not 8-byte aligned; rows_cap * row_len beyond 2^63. */
uint64_t spl_window_work_bytes(uint64_t n_docs);
int spl_window_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs,
                      const spl_collate_opts* o, uint32_t overlap,
                      void* d_rows /* [rows_cap*row_len] */, uint64_t rows_cap,
                      uint8_t* d_mask /* [rows_cap*row_len], NULL ok */, int32_t* d_len /* [rows_cap], NULL ok */,
                      int32_t* d_row_doc /* [rows_cap], NULL ok */, int64_t* d_row_start /* [rows_cap], NULL ok */,
                      uint64_t* d_row_off /* [n_docs+1], required */, uint64_t* d_n /* [2], required */,
                      void* d_work /* spl_window_work_bytes(n_docs) bytes; NULL ok when that is 0 */, void* hip_stream);

/* ONE batch exchanged in WAVES (strong scaling, pipelined: the ids of wave k travel while wave k + 1 encodes).  The batch's documents, in
 * their order, are cut into waves and every wave into one contiguous slice per rank; rank r encodes its slice of wave k into a slab
 * (spl_encode_batch_device_packed), one all-gather of equal slabs moves the wave (spl_allgather_slabs / _p2p), and this call unpacks the
 * `world` slabs BEHIND what the waves before it left: d_run[0] tokens and d_run[1] documents (device memory, zeroed by the caller before wave
 * 0, advanced here -- in stream order, so no host synchronisation sits between the waves).  After the last wave d_all_ids / d_all_off hold
 * the CSR of the whole batch in document order and d_run its totals.  d_status[0] = 1 if a slab or a result buffer was too small. */
int spl_gatherv_unpack_at(spl_tokenizer* t, const uint32_t* d_slabs, uint32_t world, uint64_t cap_words, uint64_t max_docs,
                          uint32_t* d_all_ids, uint64_t all_ids_cap, uint64_t* d_all_off, uint64_t all_off_cap, uint64_t* d_run,
                          uint32_t* d_status, void* hip_stream);

/* The collective itself behind the C ABI (north_star: "an RCCL all-gatherv over xGMI to reassemble the ragged
 * token-id output"; the reference has nothing distributed -- src/core/tokenizer.rs:932-934 is a Rayon par_iter on
 * one host -- so these are this build's own entry points).  One process per GPU.  RCCL is bound at run time
 * (dlopen of librccl.so.1: a process that already holds a copy, e.g. PyTorch's, keeps using that one; a
 * single-GPU caller needs no RCCL).
 *   spl_comm_unique_id   one rank makes the 128-byte id (ncclGetUniqueId); the caller hands it to the others
 *                        (MPI, a file, a key-value store -- no transport is imposed)
 *   spl_comm_create      ncclCommInitRank on `device`; collective: every rank of `world` must call it
 *   spl_allgather_slabs  ONE ncclAllGather of equal-sized u32 slabs (the padded, synchronisation-free form:
 *                        slabs from spl_gatherv_pack / spl_encode_batch_device_packed, results through
 *                        spl_gatherv_unpack[_group]); asynchronous on hip_stream
 *   spl_allgatherv_csr   the exact form: every rank's {T, N} and the capacities of its result buffers first
 *                        (32 bytes per rank, ONE host synchronisation), then exactly T_r ids and N_r offsets per rank land at their place of
 *                        the global CSR by grouped ncclSend / ncclRecv -- one message per peer and direction,
 *                        every xGMI link busy at once, nothing padded -- and the offsets are rebased on the
 *                        device.  d_all_ids[all_ids_cap], d_all_off[all_off_cap >= N_total + 1]; the totals are
 *                        returned; SPL_ECAPACITY if they do not fit the SMALLEST buffers any rank passed -- decided
 *                        from the gathered capacities, so every rank returns it alike and none is left waiting
 *                        in the exchange.  Rank order == document order when rank r holds the r-th contiguous
 *                        shard. */
/* A new HIP stream on `device` that really runs BESIDE the given ones (an exchange stream beside the encoder's, a second encode stream
 * beside the first): HIP maps streams to hardware queues and queues to the four pipes of the command processor by what else the process has
 * created -- two busy streams on one queue run one behind the other, on one pipe they take turns -- and no API tells which.  This call
 * measures it: up to twelve candidates over the three priorities, a 120 us spin kernel on a given stream and four empty kernels on the
 * candidate (and the other way round); the first candidate without a conflict, else the least bad one.  *conflict_us (may be NULL): what is
 * left, 0 when the streams run side by side.  Costs a few ms (synchronises the given streams).  The stream belongs to the caller
 * (hipStreamDestroy). */
int spl_pick_stream(int device, void* const* busy_hip_streams, uint32_t n_busy, void** hip_stream_out, double* conflict_us);

#define SPL_COMM_ID_BYTES 128
typedef struct spl_comm spl_comm;
int spl_comm_unique_id(uint8_t id_out[SPL_COMM_ID_BYTES]);
spl_comm* spl_comm_create(const uint8_t id[SPL_COMM_ID_BYTES], int rank, int world, int device);
void spl_comm_destroy(spl_comm* c);
int spl_comm_rank(const spl_comm* c);
int spl_comm_world(const spl_comm* c);
int spl_allgather_slabs(spl_comm* c, const uint32_t* d_send, uint32_t* d_recv, uint64_t words_per_rank, void* hip_stream);
/* the same exchange as grouped ncclSend / ncclRecv -- one message per peer and direction, each over its own xGMI link, no ring: the other
 * candidate of bench.py's start-up calibration (which of the two wins depends on the message size and on RCCL's algorithm choice) */
int spl_allgather_slabs_p2p(spl_comm* c, const uint32_t* d_send, uint32_t* d_recv, uint64_t words_per_rank, void* hip_stream);
int spl_allgatherv_csr(spl_comm* c, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, uint32_t* d_all_ids,
                       uint64_t all_ids_cap, uint64_t* d_all_off, uint64_t all_off_cap, uint64_t* n_tokens_total,
                       uint64_t* n_docs_total, void* hip_stream);

/* Tokenizer::decode_bytes for a batch (src/core/tokenizer.rs:877-897, 944-958), HOST buffers:
 * ids CSR in, bytes CSR out.  An id of the vocabulary gives its token's bytes (ByteLevel: decoded
 * to raw bytes; a key that is not ByteLevel text gives the key itself, src/core/byte_level.rs:125-146),
 * otherwise an id of the special-token map gives its literal, any other id gives nothing.
 * *out_bytes / *out_off are library-owned (pinned host memory from the handle's pool: the copies back run at
 * PCIe speed); release each with spl_free. */
int spl_decode_batch(spl_tokenizer* t, const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs,
                     uint8_t** out_bytes, uint64_t** out_off);
void spl_free(void* p);

/* The same decode with everything in DEVICE memory: ids in HBM to a bytes CSR in HBM, three launches on `hip_stream`.
 * Per document the semantics are spl_decode_batch's (Tokenizer::decode_bytes): a vocabulary id gives its bytes (ByteLevel: the raw bytes;
 * a key that is not ByteLevel text gives the key itself), otherwise an id of the special map gives its literal, any other id gives
 * nothing; nothing is validated as UTF-8.  The output is d_bytes plus d_out_off[n_docs + 1]: d_out_off[0] = 0, d_out_off[n_docs] = the
 * byte count NEEDED.  Bytes at or beyond bytes_capacity are dropped (the ids_capacity convention of spl_encode_batch_device: compare the
 * need with the capacity); nothing at or beyond d_bytes + min(need, bytes_capacity) is written; every one of the n_docs + 1 offsets is
 * written exactly once, whatever the capacity; n_docs == 0 writes d_out_off[0] = 0.  d_bytes (16-byte aligned) and the u64 offsets are
 * exactly what spl_encode_batch_device takes as its input: decode with one handle, encode with another, two calls on one stream.
 * (That call wants its text readable up to the next multiple of 16, not zeroed: a d_bytes whose capacity is a multiple of 16 is enough; the
 * decode leaves the bytes between the need and that multiple unwritten.)
 *
 *   CSR mode (row_len == 0)   document d is ids[d_ids_off[d] .. d_ids_off[d + 1]), d_ids_off[0] == 0, d_len NULL.  The host does not know
 *                    d_ids_off[n_docs] without synchronising: the grid covers n_ids_cap, ANY upper bound (the ids_capacity of the encode
 *                    in front is one).  Ids at or beyond d_ids_off[n_docs] are not read.  If the CSR claims more than n_ids_cap every
 *                    offset is clamped to it: the dropped ids of an overflowed encode decode to nothing and are not read.
 *   rows mode (row_len > 0)   document r is row r of ids[n_docs, row_len] (what a sampler leaves, the inverse of spl_pad_device), d_ids_off
 *                    NULL, n_ids_cap ignored.  With d_len [n_docs] the valid entries of row r are its first d_len[r] -- with
 *                    SPL_DECODE_PAD_LEFT its last -- d_len[r] clamped to 0 .. row_len; with d_len NULL every entry is valid.  An entry
 *                    that is not valid contributes nothing.
 *   SPL_DECODE_I64   ids are 64-bit (torch.long); a value outside 0 .. 2^32 - 1 (-1, -100, anything sign-extended, 2^32 + 17) is an id of
 *                    neither map and gives nothing.  Without the flag ids are 32-bit patterns (int32 input is read as uint32).
 *   SPL_DECODE_SKIP_SPECIAL   an id the vocabulary lacks and the special map holds gives nothing; an id both maps hold is a vocabulary id
 *                    and is emitted (the reference looks in `decoder` first).
 *
 * spl_decode_reserve_device uploads the decode tables (synchronises once) and sizes the scratch -- 8 bytes per 1 024 ids, grow-only, shared
 * with neither spl_decode_batch nor the encode workspace -- for max_ids ids (rows mode: n_docs * row_len).  After it, calls within that
 * size neither allocate nor synchronise and are fully asynchronous on hip_stream; a call that was not reserved for does both once and is
 * then asynchronous.  Device decodes of ONE handle share that scratch: they need stream order among themselves; encode and decode calls
 * on one handle need only stream order between producer and consumer.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, o or d_out_off; a null d_ids where
 * there is an id to read; a null d_bytes with bytes_capacity > 0; a struct_size of 0, shorter than the fields below or above 4096 (a
 * longer struct up to that is accepted, its tail ignored); an unknown flag bit; SPL_DECODE_PAD_LEFT or d_len in CSR mode; a missing
 * d_ids_off in CSR mode, a d_ids_off in rows mode; d_bytes not 16-byte aligned; d_ids not aligned to four ids (16 bytes, 32 with
 * SPL_DECODE_I64); n_docs >= 2^31; an id count (n_ids_cap, or n_docs * row_len) of 2^41 or more (one workgroup per 1 024 ids). */
#define SPL_DECODE_I64          1u  /* ids are int64 (torch.long); default uint32/int32 bit patterns */
#define SPL_DECODE_PAD_LEFT     2u  /* rows mode only: a row's valid entries are its LAST d_len[r] */
#define SPL_DECODE_SKIP_SPECIAL 4u  /* ids that only the special-token map knows contribute nothing */

typedef struct spl_decode_opts {
    uint32_t struct_size;           /* sizeof the struct as the CALLER was compiled: versioned exactly like spl_opts / spl_collate_opts */
    uint32_t flags;
    uint32_t row_len;               /* 0: CSR mode; > 0: rows mode, ids are [n_docs, row_len] */
} spl_decode_opts;

int spl_decode_reserve_device(spl_tokenizer* t, uint64_t max_ids);
int spl_decode_batch_device(spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap,
                            const uint64_t* d_ids_off /* CSR mode: [n_docs+1] */,
                            const int32_t* d_len      /* rows mode: [n_docs], NULL = every entry valid */,
                            uint64_t n_docs, const spl_decode_opts* o,
                            uint8_t* d_bytes, uint64_t bytes_capacity,
                            uint64_t* d_out_off /* [n_docs+1] */, void* hip_stream);
uint32_t spl_max_token_bytes(const spl_tokenizer* t);   /* longest byte string any id decodes to (computed once, again after spl_add_special) */

/* Where every id lies in the text spl_decode_batch_device writes for the same input: per id slot a byte span and a character span counted
 * from its document's start, and the documents' global offsets.  A pure function of the ids -- the decode tables and a
 * segmented running sum, no text -- so it serves what the encoder leaves and what a sampler leaves alike.  d_ids, n_ids_cap, d_ids_off,
 * d_len, n_docs and o mean exactly what they mean for spl_decode_batch_device (CSR mode and rows mode, SPL_DECODE_I64 / _PAD_LEFT /
 * _SKIP_SPECIAL, the clamping to n_ids_cap).  slots = n_ids_cap in CSR mode, n_docs * row_len in rows mode.
 *
 * For slot i of document d (a CSR range or a row): len(i) = the bytes the device decode emits for the slot (0 for an invalid, skipped or
 * unknown one); nch(i) = how many of them START a character ((b & 0xC0) != 0x80); cont(i) = 1 if len(i) > 0 and the first byte is a
 * continuation byte; bs(i) / cs(i) = the sums of len(j) / nch(j) over the slots j < i of the same document.
 *   d_byte_span[i] = (bs(i), bs(i) + len(i))
 *   d_char_span[i] = (cs(i) - (cont(i) && cs(i) > 0 ? 1 : 0), cs(i) + nch(i))
 *   d_byte_off[d], d_char_off[d], d = 0 .. n_docs: the sums over ALL slots below the clamped start of document d (entry 0 = 0)
 * The character start is tiktoken's decode_with_offsets rule (a token that begins inside a character starts at that character), the
 * character end counts every character the token touches; for valid UTF-8 both index a Python str.  A zero-length slot gets the empty
 * span at its position.  d_byte_off equals spl_decode_batch_device's d_out_off entry for entry: the byte span of slot i of document d
 * indexes that call's d_bytes at d_byte_off[d] + start .. d_byte_off[d] + end.
 *
 * Checking a result: the spans describe the DECODED text.  Compare d_byte_off[d + 1] - d_byte_off[d] with the length of the text the ids
 * came from: they differ where an encode dropped bytes (a custom pattern that leaves gaps, a vocabulary that lacks a single byte, a
 * ByteLevel key that is not ByteLevel text), and the spans of such a document do not index the original text.
 *
 * Every span entry of every slot below `slots` is written exactly once; a slot at or beyond the clamped end (CSR mode: d_ids_off[n_docs]
 * clamped to n_ids_cap) belongs to no document and gets (0, 0).  Nothing at or beyond `slots` is written.  Every one of the n_docs + 1
 * offsets is written exactly once; n_docs == 0 writes only d_*_off[0] = 0.  Span entries are int32 pairs, or int64 pairs with
 * SPL_SPANS_I64; int32 entries saturate at INT32_MAX (a document beyond 2^31 - 1 bytes), the u64 offsets stay exact.  d_byte_span,
 * d_char_span and d_char_off may each be NULL (not wanted).
 *
 * Four launches on hip_stream, no atomics and no wait between workgroups.  Scratch: 16 bytes per 1 024 ids, grow-only, an allocation of
 * its own; spl_decode_reserve_device sizes it together with the decode's, and a call within that size neither allocates nor synchronises.
 * Span calls of ONE handle share that scratch: they need stream order among themselves, none with decode or encode calls beyond producer
 * and consumer.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: everything spl_decode_batch_device refuses for
 * t, d_ids, n_ids_cap, d_ids_off, d_len, n_docs and o; an unknown span_flags bit; a null d_byte_off; d_byte_span or d_char_span not
 * 16-byte aligned; a handle with a token longer than 32 767 bytes. */
#define SPL_SPANS_I64 1u   /* span entries are int64; default int32 */
int spl_token_spans_device(spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap,
                           const uint64_t* d_ids_off, const int32_t* d_len, uint64_t n_docs,
                           const spl_decode_opts* o, uint32_t span_flags,
                           void* d_byte_span    /* [slots, 2], NULL ok */,
                           void* d_char_span    /* [slots, 2], NULL ok */,
                           uint64_t* d_byte_off /* [n_docs+1], required */,
                           uint64_t* d_char_off /* [n_docs+1], NULL ok */,
                           void* hip_stream);

/* ONE STEP of n_seqs streaming decoders at once, everything in DEVICE memory: the reference's StreamingDecoder /
 * ByteLevelStreamingDecoder (src/core/streaming.rs; find_valid_utf8_len and is_incomplete_utf8, src/python/bindings.rs:591-640) as the pure
 * function  (state_in[b], ids[b, 0 .. row_len), len[b]) -> (bytes CSR, state_out[b]).  A sampler's step -- one id per live sequence, or a
 * few under speculative decoding -- goes in as rows; only complete UTF-8 characters come out.
 *
 * Per sequence the stream S is the pending bytes of its state followed by the bytes spl_decode_batch_device emits in rows mode for the
 * row's first clamp(d_len[b], 0, row_len) entries (d_len NULL: all of them): raw bytes for a ByteLevel vocabulary, the key itself for a key
 * that is not ByteLevel text, a special id's literal; nothing for an unknown id, for a value outside 0 .. 2^32 - 1 under SPL_DECODE_I64 and
 * for an id skipped under SPL_DECODE_SKIP_SPECIAL.  Well-formed is Unicode's table: leads C2 .. F4, the second byte narrowed after E0, ED,
 * F0 and F4.
 *
 * The state word (uint64; 0 is a fresh decoder, so a reset is the caller zeroing words; every bit not named is 0):
 *     bits 0..23  the pending bytes, first byte lowest     bits 24..25  their count     bit 26  stalled     bits 32..63  held
 * The reference's pending_bytes is the count where the sequence is not stalled and held where it is.
 *
 * Hold mode (default; the reference, step for step).  A stalled sequence emits nothing, held grows by the bytes added (saturating at
 * 2^32 - 1).  Otherwise the longest valid prefix of S is emitted; if nothing is left the state is 0; if what is left is the well-formed
 * beginning of one character that reaches the end of S (1 to 3 bytes) it is the new pending; anything else STALLS the sequence -- stalled
 * = 1, held = the bytes left, pending 0 -- and it never emits again, which is what the reference does (feed it a lone 0x80).
 * SPL_STREAM_REPLACE: S is cut into units from the left -- an ASCII byte; a lead with as many following bytes as conform to its row of the
 * table (all of them: a character, copied; the end of S first: the new pending; a non-conforming byte first: a maximal invalid subpart,
 * emitted as EF BF BD); any other byte (EF BF BD) -- which is Python's incremental decoder with errors="replace".  Never stalls.
 * Final -- d_final[b] != 0, or SPL_STREAM_FINAL_ALL for every sequence -- is applied behind the call's ids: a sequence that is not stalled
 * and has pending bytes emits one EF BF BD and its state becomes 0; a stalled one emits nothing and keeps its state (the caller reads the
 * flag; what the reference would flush is the lossy decode of the ids fed since, which the caller has).  d_len[b] == 0 without final
 * leaves d_state_out[b] == d_state_in[b] bit for bit.
 *
 * Output as the device decode's: d_out_off[b] = where sequence b's bytes start, d_out_off[n_seqs] = the byte count NEEDED; bytes at or beyond
 * bytes_capacity are dropped and nothing at or beyond min(need, capacity) is written; every offset and EVERY STATE WORD is written exactly
 * once whatever the capacity.  The state advances even where bytes were dropped: a caller that may have to repeat a call with a larger
 * buffer keeps d_state_in (passes another array as d_state_out).  d_state_out == d_state_in is allowed otherwise.
 *
 * Up to 64 sequences ("stream_one_max"; the two forms' medians cross between 64 and 80, profiles/stream_decode.txt) the call is ONE launch
 * of one workgroup, beyond that three.  spl_stream_reserve_device uploads
 * the decode tables (synchronises once) and sizes the scratch -- 8 bytes per sequence and 8 per 16 of them, grow-only, shared with nothing;
 * after it a call within that size neither allocates nor synchronises.  Streaming calls of ONE handle share the scratch: they need stream
 * order among themselves.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, o, d_state_in, d_state_out or d_out_off;
 * a null d_ids with n_seqs > 0; a null d_bytes with bytes_capacity > 0; struct_size below the struct's three fields or above 4096; an
 * unknown bit in o->flags or in stream_flags; row_len == 0 (rows mode only); SPL_DECODE_PAD_LEFT; d_bytes not 16-byte aligned;
 * n_seqs >= 2^31. */
#define SPL_STREAM_REPLACE   1u  /* replace mode: invalid bytes leave as U+FFFD, no sequence ever stalls */
#define SPL_STREAM_FINAL_ALL 2u  /* every sequence is final in this call */
int spl_stream_reserve_device(spl_tokenizer* t, uint64_t max_seqs);
int spl_stream_decode_device(spl_tokenizer* t, const void* d_ids /* [n_seqs, o->row_len] */,
                             const int32_t* d_len /* [n_seqs], NULL: all valid */, uint64_t n_seqs,
                             const spl_decode_opts* o, uint32_t stream_flags,
                             const uint8_t* d_final /* [n_seqs], NULL ok */,
                             const uint64_t* d_state_in, uint64_t* d_state_out,
                             uint8_t* d_bytes, uint64_t bytes_capacity,
                             uint64_t* d_out_off /* [n_seqs+1] */, void* hip_stream);

/* STOP STRINGS for n_seqs streaming sequences at once, everything in DEVICE memory: what a serving loop does with the
 * text of a step -- compare it against the request's stop strings, hold back what may still become one -- as the pure function
 * (state_in[b], the new bytes of b, mask[b], final[b]) -> (bytes CSR, hit[b], state_out[b]).  A stop string is text, not an id: it may
 * begin in the middle of one token and end in the middle of another, steps apart.
 *
 * The rule, per sequence, is one of the WHOLE text and does not depend on where the steps cut it.  T = every byte fed so far, S = the
 * stops its mask selects.  HIT: the smallest end e such that some s of S is a suffix of T[:e]; of the stops that end at e the longest wins
 * (its start is p), of equal strings the lowest slot.  The released text is T[:p] -- T[:e] under SPL_STOP_INCLUDE --, d_hit[b] is the slot,
 * and the sequence is STOPPED from then on: it ignores further input (the rest of the call that hit included), emits nothing, and its row
 * stays as it is bit for bit.  NO HIT: the released text is T[:|T| - h], h the length of the longest suffix of T that is a PROPER prefix of
 * some s of S (h <= 63) -- exactly the text that may still become a stop is held back, so nothing a client was shown is ever taken back and
 * the released length never decreases.  FINAL -- d_final[b] != 0, or SPL_STOP_FINAL_ALL -- is applied behind the call's bytes: without a
 * hit the held bytes leave too, h = 0, and the text is CLOSED: the tail is emptied, bytes fed later are matched as a new text (`released`
 * goes on counting).  A call's output for a sequence is its released text now less its released text before the call.  A sequence with no
 * new bytes and no final keeps its row bit for bit.  Where the stops and T are valid UTF-8 every cut is a character boundary.
 *
 * The table (SPL_STOP_TABLE_BYTES of device memory, the CALLER's): slot s is bytes [64 s, 64 s + len[s]), and uint8 len[64] lies behind the
 * 64 slots; a slot of length 0 or above 64 never matches.  d_mask[b] bit s: slot s applies to sequence b (NULL: every slot to everyone).  The
 * caller may rewrite a slot with a stream-ordered copy of its own -- a continuous-batching loop reusing a finished request's slots --, but
 * ONLY WHILE NO LIVE SEQUENCE'S MASK NAMES IT: a sequence's held bytes were held for the stops its mask named.
 *
 * The state row (SPL_STOP_STATE_WORDS uint64 per sequence; all zero is a fresh sequence, so a reset is the caller zeroing rows; every bit
 * not named is 0 and the tail's bytes from tail_len on are 0, so rows compare bit for bit):
 *     word 0      bits 0..6 tail_len     bits 8..14 held (h)     bit 16 stopped     bits 24..29 the slot that hit
 *     word 1      released: the bytes released so far; once stopped, the offset of the cut in the sequence's text
 *     words 2..9  the tail: the last min(|T|, 63) bytes of T (of T[:e] once stopped), the first byte lowest
 *
 * Input: any bytes CSR in device memory -- spl_stream_decode_device's d_bytes and d_out_off as they are.  An offset above in_capacity counts
 * as in_capacity and bytes beyond it are not read (an overflowed producer's convention).  Output as the streaming decode's: d_out_off[b] =
 * where sequence b's bytes start, d_out_off[n_seqs] = the byte count NEEDED; bytes at or beyond out_capacity are dropped and nothing at or
 * beyond min(need, capacity) is written; every offset, every hit (-1, or the slot: sticky) and EVERY STATE WORD is written exactly once
 * whatever the capacity.  The state advances even where bytes were dropped: a caller that may have to repeat a call keeps d_state_in
 * (passes another array as d_state_out); d_state_out == d_state_in is allowed otherwise.  That is the ONLY overlap allowed: the write pass
 * reads d_in_bytes, d_in_off, d_table, d_mask and d_final again while other workgroups write, so none of d_out_bytes, d_out_off, d_hit and
 * d_state_out may overlap any input (nor one another), and d_state_out may overlap d_state_in only as the same array.
 *
 * Up to 64 sequences ("stop_one_max"; the two forms' medians cross between 64 and 80, profiles/stop_match.txt) the call is ONE launch of
 * one workgroup, beyond that three.  The call is asynchronous on hip_stream; the handle is used for its device and its scratch only (no
 * table of the tokenizer is read).  spl_stop_reserve_device sizes the scratch -- 24 bytes per sequence and 8 per 16 of them, grow-only,
 * shared with nothing; after it a call within that size neither allocates nor synchronises.  Stop calls of ONE handle share the scratch:
 * they need stream order among themselves.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, d_table, d_state_in, d_state_out,
 * d_out_off, d_hit or d_in_off; a null d_in_bytes with in_capacity > 0; a null d_out_bytes with out_capacity > 0; d_out_bytes not 16-byte
 * aligned; an unknown bit in stop_flags; n_seqs >= 2^31. */
#define SPL_STOP_SLOTS       64
#define SPL_STOP_MAX_LEN     64
#define SPL_STOP_TABLE_BYTES (64 * 64 + 64)
#define SPL_STOP_STATE_WORDS 10
#define SPL_STOP_INCLUDE     1u  /* the stop string itself is released with the text in front of it */
#define SPL_STOP_FINAL_ALL   2u  /* every sequence is final in this call */
int spl_stop_reserve_device(spl_tokenizer* t, uint64_t max_seqs);
int spl_stop_match_device(spl_tokenizer* t,
                          const uint8_t* d_in_bytes, uint64_t in_capacity,
                          const uint64_t* d_in_off /* [n_seqs+1] */, uint64_t n_seqs,
                          const uint8_t* d_table /* SPL_STOP_TABLE_BYTES */,
                          const uint64_t* d_mask /* [n_seqs], NULL: all */,
                          const uint8_t* d_final /* [n_seqs], NULL ok */, uint32_t stop_flags,
                          const uint64_t* d_state_in, uint64_t* d_state_out /* [n_seqs, 10] */,
                          uint8_t* d_out_bytes, uint64_t out_capacity,
                          uint64_t* d_out_off /* [n_seqs+1] */,
                          int32_t* d_hit /* [n_seqs] */, void* hip_stream);

/* TOKEN HEALING for n_seqs sequences at once, everything in DEVICE memory: the input side of the sampler.  A prompt that
 * ends inside a word ("http:", "def foo(", a trailing space) ends with a token the model has rarely seen in front of the intended
 * continuation.  The remedy (guidance, llguidance): take the last token or tokens off the prompt and, until their bytes are spelled again,
 * let the model sample only ids whose bytes agree with them.  The id -> bytes tables already lie in HBM, so the mask [n_seqs, n_words] is
 * written where the sampler reads it; no trie on the host, no copy per step.  "The answer must begin with this text" is the same
 * primitive: the caller writes the text into the state rows and calls the step with row_len 0.
 *
 * b(t) is what spl_decode_batch_device emits for id t.  t is ORDINARY if it is an id of the vocabulary proper and b(t) has at least one
 * byte; ids that only the special-token map holds, ids the vocabulary lacks and ids above its largest id are not ordinary.
 *
 * Per sequence there is a pending prefix P of 0 .. SPL_HEAL_MAX_PREFIX bytes.
 *   |P| = 0   the sequence is FREE: its mask row is all ones, in every bit of every one of its n_words words.
 *   |P| >= 1  it is CONSTRAINED: bit t is set iff t is ordinary and either b(t) starts with P (t COVERS; it may be longer than 64 bytes) or
 *             P starts with b(t) and b(t) is shorter than P (t is PARTIAL).  Every other bit of the row is 0, bits beyond the largest id
 *             included.
 * The mask: int32 [n_seqs, n_words], n_words >= ceil((largest vocabulary id + 1) / 32) the caller's choice (a model's logits are often
 * wider than the vocabulary); bit t & 31 of word t >> 5 stands for id t, 1 = allowed -- the layout xgrammar's and vLLM's
 * apply_token_bitmask kernels read.
 *
 * STEP: per sequence the first clamp(d_len[b], 0, row_len) ids of row b of d_ids [n_seqs, row_len] (d_len NULL: all; row_len may be 0)
 * are applied in order.  Free: stays free, whatever the id.  t covers: P becomes empty, `healed` is set.  t is partial: its bytes leave the
 * front of P.  Anything else -- a special, an id of neither map, an int64 value outside 0 .. 2^32 - 1, an ordinary id that disagrees with
 * P -- BREAKS the sequence: P becomes empty, the sticky `broken` is set, and it runs free from then on.  The call then writes the mask of
 * the state it arrived at; row_len 0 only writes masks.
 *
 * BEGIN: prompts as rows d_ids [n_seqs, row_len] with d_len (NULL: every entry valid; SPL_HEAL_PAD_LEFT: a row's valid entries are its
 * LAST d_len[b], and d_len is required), o->max_back in 0 .. SPL_HEAL_MAX_BACK, o->min_keep.  Per sequence, with P empty, for j = 1, 2, ...
 * and t_j the j-th token from the end, stop at the first of: j > max_back; fewer than min_keep tokens would remain (len - j < min_keep);
 * t_j is not ordinary; |b(t_j)| + |P| > 64; under SPL_HEAL_AUTO only: no ordinary token's bytes start with b(t_j) + P and are strictly
 * longer than it.  Otherwise P := b(t_j) + P.  d_n_back[b] is the number of tokens taken: the caller feeds the model the first
 * len - n_back tokens; the rows are not written.  Without SPL_HEAL_AUTO exactly as many tokens are taken as the other limits allow; with
 * it "http" ":" is rolled back over ":" because "://" exists, and over "http" too only if some token extends "http:".
 *
 * The state row (SPL_HEAL_STATE_WORDS uint64 per sequence; all zero is free and fresh, so a reset is the caller zeroing rows; every bit not
 * named is 0 and P's bytes from |P| on are 0, so rows compare bit for bit):
 *     word 0      bits 0..6 |P|     bit 8 broken     bit 9 healed (it was constrained once and a covering token ended it)
 *     words 1..8  P, the first byte lowest
 * d_state_out may be d_state_in.  No other output may coincide with an input or with another output.
 *
 * Further outputs, each optional (NULL): d_live [n_seqs] uint8, 1 where the sequence is constrained after the call; d_n int32 [2], the
 * number of constrained sequences and the number that broke in this call (device memory, like everything else).
 * SPL_HEAL_KEEP_FREE: the rows of sequences that are free after the call are not written at all -- the caller filled them with ones
 * once; long after every prompt has healed the call then writes nothing.
 *
 * What the rule is NOT: the allowed set ignores the split pattern, as every implementation of healing does, so the healed ids need not be
 * the canonical encoding of the text; and UTF-8 validity of the continuation is not part of it (spl_utf8_mask_device below is, and ANDs
 * its rows into these).
 *
 * Two launches on hip_stream: a plan (a wavefront per sequence: the transition, then the covering ids as ONE range of the ordinary ids
 * sorted by their bytes, found with one pivot per lane, then the partial ids from the prefix order) and a fill (whole words, each written
 * once).  No atomics on global memory, no wait between workgroups.  spl_heal_reserve_device uploads the decode tables and builds the
 * sorted order, id -> rank and the prefix order (synchronises once; again after spl_add_special) and sizes the scratch -- 264 bytes per
 * sequence, grow-only, shared with nothing; after it a call within that size neither allocates nor synchronises.  Healing calls of ONE
 * handle share the scratch: they need stream order among themselves.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, in, o, out, d_state_out or d_mask; a
 * null d_state_in (step) or d_n_back (begin); a null d_ids where there is an id to read; SPL_HEAL_PAD_LEFT without d_len; a struct_size
 * shorter than a struct or above 4096; an unknown flag bit (SPL_HEAL_AUTO and _PAD_LEFT are flags of begin alone); n_words * 32 below the
 * largest vocabulary id + 1, or n_words above 2^26; max_back above SPL_HEAL_MAX_BACK; n_seqs >= 2^31; an array not aligned to its element
 * type; an output that coincides with an input (other than state out with state in) or with another output.  Arguments are refused,
 * never clamped.  The element type of d_ids cannot be seen from a pointer: SPL_HEAL_I64 names it, the Python layer refuses other dtypes.
 * A vocabulary in which more than 63 ids spell prefixes of one 64-byte string (many ids with equal bytes) is refused by the reserve. */
#define SPL_HEAL_AUTO        1u  /* begin: take a token only if some ordinary token extends what has been taken */
#define SPL_HEAL_KEEP_FREE   2u  /* rows of sequences that are free after the call are not written */
#define SPL_HEAL_I64         4u  /* d_ids are int64 (torch.long); default int32 / uint32 bit patterns */
#define SPL_HEAL_PAD_LEFT    8u  /* begin: a row's valid entries are its LAST d_len[b] */
#define SPL_HEAL_STATE_WORDS 9
#define SPL_HEAL_MAX_PREFIX  64
#define SPL_HEAL_MAX_BACK    8

typedef struct spl_heal_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled */
    uint32_t flags, n_words;
    uint32_t max_back, min_keep;          /* begin only */
} spl_heal_opts;
typedef struct spl_heal_in {
    uint32_t struct_size, row_len;        /* row_len: the columns of d_ids (step: may be 0) */
    uint64_t n_seqs;
    const void* d_ids; const int32_t* d_len;
    const uint64_t* d_state_in;           /* step only: [n_seqs, SPL_HEAL_STATE_WORDS] */
} spl_heal_in;
typedef struct spl_heal_out {
    uint32_t struct_size, reserved;
    uint64_t* d_state_out;                /* [n_seqs, SPL_HEAL_STATE_WORDS] */
    int32_t* d_mask;                      /* [n_seqs, n_words] */
    uint8_t* d_live; int32_t* d_n;        /* NULL ok */
    int32_t* d_n_back;                    /* begin only: [n_seqs] */
} spl_heal_out;

int spl_heal_reserve_device(spl_tokenizer* t, uint64_t max_seqs);
int spl_heal_begin_device(spl_tokenizer* t, const spl_heal_in* in, const spl_heal_opts* o, const spl_heal_out* out, void* hip_stream);
int spl_heal_step_device(spl_tokenizer* t, const spl_heal_in* in, const spl_heal_opts* o, const spl_heal_out* out, void* hip_stream);

/* UTF-8 CONTINUATION MASKS for n_seqs sequences at once, everything in DEVICE memory: which ids may be drawn next so that
 * the streaming decode never stalls (hold mode) and never emits U+FFFD (SPL_STREAM_REPLACE).  A byte-level BPE vocabulary holds thousands
 * of ids whose bytes are fragments of characters; one wrong draw behind a pending lead byte stalls a hold-mode sequence for good.
 *
 * THE RULE.  d_state [n_seqs] are the state words spl_stream_decode_device keeps (bits 0..23 the pending bytes, 24..25 their count, 26
 * stalled), o the decode options of that stream.  With p the pending bytes of a word -- 0 to 3 bytes, the well-formed beginning of one
 * character -- and e(t) the bytes the streaming decode emits for id t under o (nothing for an id only the special map holds under
 * SPL_DECODE_SKIP_SPECIAL): bit t & 31 of word t >> 5 of the row is 1 iff t is KNOWN (the vocabulary proper or the special map holds it)
 * and p + e(t) is PREFIX-VALID -- well-formed UTF-8, optionally followed by the well-formed beginning of one character that reaches the
 * end.  Well-formed is Unicode's table, the decoder's own: leads C2 .. F4, the second byte narrowed after E0, ED, F0 and F4.  Every other
 * bit is 0, those from the largest known id + 1 up to 32 * n_words included.  A known id with no bytes is allowed in every state.  In hold
 * mode the rule is "feeding t now does not stall the decoder".  A sequence that is STALLED has nothing left to protect: its row is all
 * ones and d_live[b] is 0; so is a word no decoder leaves (pending bytes that are not the beginning of a character).  Every other
 * sequence has d_live[b] 1.  Only SPL_DECODE_SKIP_SPECIAL of o->flags matters; o->row_len is not read.
 *
 * p matters only through one of eight classes -- start; one, two or three continuation bytes of any value owed; the four narrowed
 * second-byte states behind E0, ED, F0 and F4 -- so a call is a row gather from a table of 17 rows (per class the vocabulary's ids and,
 * apart, the special ids; the special ids of every class for SPL_DECODE_SKIP_SPECIAL) that spl_utf8_mask_reserve_device builds ON THE
 * DEVICE, once per handle and again after spl_add_special (it uploads the decode tables and synchronises once).
 *
 * SPL_UTF8_AND: the row is ANDed into what d_mask holds (spl_heal_step_device's mask, a grammar's), and a stalled sequence's row is not
 * touched; without it the row is written, every word exactly once.  d_live may be NULL.  ONE launch on hip_stream, asynchronous; after the
 * reserve a call neither allocates nor synchronises.  No atomics on global memory, no wait between workgroups.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, o, d_state or d_mask; a struct_size
 * shorter than spl_decode_opts or above 4096; an unknown bit in flags or in o->flags; n_words * 32 below the largest known id + 1 (the
 * largest of the vocabulary's and the special map's: spl_vocab_size), or n_words above 2^26; n_seqs >= 2^31; d_state not 8-byte or d_mask
 * not 4-byte aligned; two of d_state, d_mask and d_live at one address.  Arguments are refused, never clamped. */
#define SPL_UTF8_AND 1u  /* AND the row into d_mask instead of writing it */
int spl_utf8_mask_reserve_device(spl_tokenizer* t);
int spl_utf8_mask_device(spl_tokenizer* t, const uint64_t* d_state /* [n_seqs] */, uint64_t n_seqs, const spl_decode_opts* o, uint32_t flags,
                         uint32_t n_words, int32_t* d_mask /* [n_seqs, n_words] */, uint8_t* d_live /* [n_seqs], NULL ok */, void* hip_stream);

/* An allowed-token BITMASK applied to the logits in place, everything in DEVICE memory: the last link between this
 * library's masks and the sampler.  d_logits [n_rows, n_cols] of dtype, row r at element r * row_stride (row_stride >= n_cols, in elements);
 * d_mask int32 rows of n_words words, row r at word r * mask_stride (mask_stride >= n_words) -- the layout spl_heal_*_device and
 * spl_utf8_mask_device write, and xgrammar's; d_live uint8 [n_rows] or NULL.
 *
 * For every row r with d_live NULL or d_live[r] != 0 and every column c < min(n_cols, 32 * n_words): if bit c & 31 of word c >> 5 of mask
 * row r is 0, logits[r, c] becomes -inf of the dtype -- a store, not arithmetic: a NaN there becomes -inf.  Everything else keeps its bits
 * exactly, NaN payloads and -0.0 included: allowed columns, columns at or beyond 32 * n_words, the row_stride - n_cols elements behind a
 * row, rows that are not live.  The mask rows of rows that are not live are not read.
 *
 * The logits need no alignment beyond their element type: an odd n_cols with row_stride == n_cols puts every second half-precision row
 * on an odd 2-byte boundary, a sliced view moves the base.  A lane owns 16 bytes of a row by absolute address (8 half-precision columns or
 * 4 floats); the pieces at a row's two ends are handled element by element, the ones between with 16-byte accesses: all bits 1 -- neither
 * load nor store; all bits 0 -- a store without a load; mixed -- load, select, store.  ONE launch on hip_stream, asynchronous; it never
 * allocates or synchronises and needs no reserve.  No LDS, no atomics, no wait between workgroups.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t or a; a struct_size shorter than the
 * struct or above 4096; a dtype that is none of the three; a null d_logits or d_mask where there is a column to mask; row_stride below
 * n_cols or mask_stride below n_words (or either 2^40 or more); n_rows >= 2^31; n_words above 2^26; d_logits not aligned to its element
 * type, d_mask not 4-byte aligned.  Arguments are refused, never clamped. */
#define SPL_F32  0u
#define SPL_F16  1u
#define SPL_BF16 2u
typedef struct spl_mask_apply {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled */
    uint32_t dtype;                       /* SPL_F32, SPL_F16 or SPL_BF16 */
    void* d_logits;
    uint64_t n_rows;
    uint32_t n_cols, n_words;
    uint64_t row_stride;                  /* elements from a row of the logits to the next */
    uint64_t mask_stride;                 /* words from a row of the mask to the next */
    const int32_t* d_mask;
    const uint8_t* d_live;                /* NULL ok */
} spl_mask_apply;
int spl_mask_apply_device(spl_tokenizer* t, const spl_mask_apply* a, void* hip_stream);

/* GUIDED CHOICE for n_seqs sequences at once, everything in DEVICE memory: the answer of a sequence is exactly ONE OF
 * UP TO 64 BYTE STRINGS -- classification labels, yes / no, tool names, multiple choice (vLLM's guided_choice, Outlines' choice).  The
 * tables token healing sorts the vocabulary into already lie in HBM, so the mask [n_seqs, n_words] is written where the sampler reads it:
 * no trie on the host, no copy per step.  A finite set of strings needs no automaton; regular expressions are spl_dfa_step_device's (below), grammars stay out of scope.
 *
 * THE TABLE (SPL_CHOICE_TABLE_BYTES of device memory, the CALLER's; the stop table's layout): slot s is bytes [64 s, 64 s + len[s]) and
 * spells the choice c_s; uint8 len[64] lies behind the 64 slots.  len[s] = 0 is an empty slot and is never a choice (nor is a length
 * above 64).  One table serves every sequence of a call; a sequence selects its candidates in its state row.
 *
 * b(t) and ORDINARY are token healing's: b(t) is what spl_decode_batch_device emits for id t, and t is ordinary if it is an id of the
 * vocabulary proper and b(t) has at least one byte.  END is o->end_ids[0 .. n_end), n_end in 0 .. SPL_CHOICE_MAX_END, any ids below
 * 32 * n_words -- special tokens are the usual case (an end-of-turn id).
 *
 * The state row (SPL_CHOICE_STATE_WORDS uint64 per sequence; all zero is free and fresh, so a reset is the caller zeroing rows; every bit
 * not named is 0, so rows compare bit for bit):
 *     word 0      A: the slots that can still be spelled, bit s for slot s
 *     word 1      bits 0..6 k, the bytes spelled so far     bit 8 broken     bit 9 done     bits 16..21 hit, the slot answered (with done)
 * TO BEGIN the caller writes a candidate set into word 0 with word 1 = 0 (all slots of A share their first k bytes by construction; a
 * caller who writes k > 0 itself guarantees that: the call only reads c_s[k:]).  ON LOAD k is clamped to 64; every slot with len[s] = 0,
 * len[s] > 64 or len[s] < k leaves A; a row with done or broken set passes through with word 0 cleared (broken wins over done); a row
 * whose A is empty then, with neither bit set, is free and is written back all zero.
 *
 * THE MASK ROW: int32 [n_seqs, n_words], bit t & 31 of word t >> 5 for id t, 1 = allowed, as spl_heal_step_device writes it.  With
 * r_s = c_s[k:] for s in A:
 *   A empty   the sequence is FREE (or done, or broken): its row is all ones, in every bit of every one of its n_words words.
 *   otherwise it is CONSTRAINED: bit t is set iff (a) t is ordinary and some s in A has |b(t)| <= |r_s| with r_s starting with b(t), or
 *             (b) SPL_CHOICE_THEN_FREE is not set, t is in END and some s in A has |r_s| = 0.  Every other bit of the row is 0, up to
 *             32 * n_words.  A constrained row is NEVER ALL ZERO: where (a) and (b) yield no id -- the vocabulary lacks the single byte
 *             that comes next -- the sequence becomes `broken` in that call and its row is ones.
 *
 * STEP: per sequence the first clamp(d_len[b], 0, row_len) ids of row b of d_ids [n_seqs, row_len] (d_len NULL: all; row_len may be 0)
 * are read in order WHILE the sequence is constrained.  For an id t:
 *   1. t is ordinary and S = {s in A : r_s starts with b(t)} is not empty: A := S and k += |b(t)|.  Under SPL_CHOICE_THEN_FREE, if some
 *      s in A now has len[s] = k, the sequence is `done`, hit is the lowest such s and A becomes empty.
 *   2. otherwise, SPL_CHOICE_THEN_FREE is not set, t is in END and E = {s in A : |r_s| = 0} is not empty: the sequence is `done`,
 *      hit = min E, A becomes empty.
 *   3. otherwise -- a special that is no END id, an id of neither map, an int64 value outside 0 .. 2^32 - 1, an ordinary id no remainder
 *      starts with, an END id too early -- the sequence is `broken`, A becomes empty and k := 0.
 * Later ids of a sequence that is free, done or broken are not read.  Equivalently: an id is accepted iff its bit was set in the mask of
 * the state in front of it.  The call then writes the mask of the state it arrived at; row_len 0 only writes masks -- that is how the
 * first mask is obtained after the caller wrote candidate sets.  Of equal choices in two slots the lower one is the hit.
 *
 * WRITE-BACK, canonical: constrained (A, k); done (0, k | done | hit << 16); broken (0, 1 << 8); free zeros.  d_state_out may be
 * d_state_in.  No other output may coincide with an input or with another output.  d_live [n_seqs] uint8 (NULL ok): 1 iff the sequence
 * is constrained after the call.  There is no count over the batch: it would need a second launch or an atomic on global memory;
 * live.sum() is the caller's.  SPL_CHOICE_KEEP_FREE: the rows of sequences that are not constrained after the call are not written at
 * all -- the caller filled them with ones once.
 *
 * What the rule is NOT, as healing's: it ignores the split pattern, so the ids need not be the canonical encoding of the choice; UTF-8
 * validity is not part of it (spl_utf8_mask_device with SPL_UTF8_AND can AND its rows into these afterwards); more than 64 slots, choices
 * over 64 bytes and a table per sequence are out of scope.
 *
 * ONE launch on hip_stream, asynchronous: a wavefront owns a sequence (workgroups of 64 threads, no workgroup barrier); the step tests a
 * slot per lane; the row of a constrained sequence is a handful of ids, so it starts from zeros in LDS and the ids are SCATTERED into it
 * -- per alive slot one search of the ordinary ids sorted by their bytes for the last one that is <= r_s, then its ancestors in the prefix
 * order -- and streamed to the mask, every word of a written row stored exactly once; a free row is stored as ones.  No scratch, no
 * atomics on global memory, no wait between workgroups.  spl_choice_reserve_device uploads the decode tables and token healing's sorted
 * order, id -> rank and prefix order (shared with spl_heal_*_device; synchronises once, again after spl_add_special); after it a call
 * neither allocates nor synchronises.  The row is built in LDS a PIECE at a time: the handle option "choice_piece_words" (spl_set_option /
 * spl_get_option; a multiple of 4 in 4 .. 8192, default 8192; for tests and measuring only) is the words of a piece -- every shipped
 * vocabulary's row is one piece, a smaller value takes a toy vocabulary's row through several.  Same results.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, in, o, out, d_table, d_state_in,
 * d_state_out or d_mask; a null d_ids where there is an id to read; a struct_size shorter than a struct or above 4096; an unknown flag
 * bit; n_words * 32 below the largest vocabulary id + 1, or n_words above 2^26; n_end above SPL_CHOICE_MAX_END; an END id at or above
 * 32 * n_words; n_end = 0 without SPL_CHOICE_THEN_FREE (no sequence could ever finish); n_seqs >= 2^31; an array not aligned to its
 * element type; an output that coincides with an input (other than state out with state in) or with another output.  Arguments are
 * refused, never clamped.  A vocabulary the healing reserve refuses is refused here too. */
#define SPL_CHOICE_THEN_FREE   1u  /* a sequence is done as soon as one of its choices is spelled out; END ids play no part */
#define SPL_CHOICE_KEEP_FREE   2u  /* rows of sequences that are not constrained after the call are not written */
#define SPL_CHOICE_I64         4u  /* d_ids are int64 (torch.long); default int32 / uint32 bit patterns */
#define SPL_CHOICE_SLOTS       64
#define SPL_CHOICE_MAX_LEN     64
#define SPL_CHOICE_TABLE_BYTES (64 * 64 + 64)
#define SPL_CHOICE_STATE_WORDS 2
#define SPL_CHOICE_MAX_END     8

typedef struct spl_choice_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled */
    uint32_t flags, n_words;
    uint32_t n_end;                       /* 0 .. SPL_CHOICE_MAX_END */
    uint32_t end_ids[SPL_CHOICE_MAX_END];
} spl_choice_opts;
typedef struct spl_choice_in {
    uint32_t struct_size, row_len;        /* row_len: the columns of d_ids (may be 0) */
    uint64_t n_seqs;
    const void* d_ids; const int32_t* d_len;
    const uint64_t* d_state_in;           /* [n_seqs, SPL_CHOICE_STATE_WORDS] */
    const uint8_t* d_table;               /* SPL_CHOICE_TABLE_BYTES */
} spl_choice_in;
typedef struct spl_choice_out {
    uint32_t struct_size, reserved;
    uint64_t* d_state_out;                /* [n_seqs, SPL_CHOICE_STATE_WORDS] */
    int32_t* d_mask;                      /* [n_seqs, n_words] */
    uint8_t* d_live;                      /* NULL ok */
} spl_choice_out;

int spl_choice_reserve_device(spl_tokenizer* t);
int spl_choice_step_device(spl_tokenizer* t, const spl_choice_in* in, const spl_choice_opts* o, const spl_choice_out* out, void* hip_stream);

/* THE REGEX GUIDE for n_seqs sequences at once, everything in DEVICE memory: the answer of a sequence MATCHES A REGULAR
 * EXPRESSION -- dates, numbers, identifiers, a fixed JSON shape (vLLM's guided_regex, Outlines' regex).  The library holds no automaton
 * compiler: the calls take a deterministic automaton over BYTES as a table in the caller's device memory (splintr_amd/dfa.py compiles
 * one from a pattern; the calls do not care how the table was made).  The expensive half -- which ids may follow which state, seconds to
 * minutes on a host for 100 k to 200 k ids -- is spl_dfa_index_device, a GPU job; a step is then a row copy.
 *
 * THE TABLE (SPL_DFA_TABLE_BYTES(n_states) of device memory, the CALLER's, 2-byte aligned): uint16 trans[n_states][256], then
 * uint8 accept[n_states].  trans[q][x] is the state behind byte x in state q; ON LOAD every value >= n_states is DEAD (SPL_DFA_DEAD is
 * the one a builder writes) -- the kernels never index outside the table, whatever it holds.  accept[q] != 0: q accepts.  n_states is
 * 1 .. SPL_DFA_MAX_STATES.  One table serves a call; a sequence's start state is whatever the caller writes into its state word, so
 * several automata stacked into one table serve one batch.
 *
 * b(t) and ORDINARY are token healing's: b(t) is what spl_decode_batch_device emits for id t, and t is ordinary if it is an id of the
 * vocabulary proper and b(t) has at least one byte.  walk(q, b(t)) follows trans byte by byte and is DEAD as soon as a step is.  END is
 * o->end_ids[0 .. n_end), n_end in 1 .. SPL_DFA_MAX_END, any ids below 32 * n_words -- special tokens are the usual case.
 *
 * THE INDEX (SPL_DFA_INDEX_BYTES(n_states, n_words) of device memory, the CALLER's, 4-byte aligned), written by spl_dfa_index_device:
 * int32 rows[n_states][stride], stride = n_words rounded up to a multiple of four, then uint8 some[n_states].  Bit t & 31 of word
 * t >> 5 of row q is 1 iff t is ordinary and walk(q, b(t)) != DEAD; every other bit is 0, up to 32 * stride.  some[q] is 1 iff row q
 * has a set bit.  Every word and every some byte is stored exactly once.  The index holds ordinary ids only, so it does not depend on
 * the END ids; it belongs to (table, n_states, n_words, the handle's vocabulary) and a step must be given the n_words it was built with.
 * It is rebuilt by the caller after spl_add_special, as the reserves rebuild their tables.
 *
 * THE STATE ROW (SPL_DFA_STATE_WORDS uint64 per sequence; all zero is free, so a reset is the caller zeroing words; every bit not named
 * is 0, so rows compare bit for bit):    bits 0..15 q     bit 16 constrained     bit 17 broken     bit 18 done
 * TO BEGIN the caller writes start | 1 << 16.  ON LOAD broken wins over done and done over constrained; a constrained row with
 * q >= n_states becomes broken.
 *
 * THE MASK ROW: int32 [n_seqs, n_words], bit t & 31 of word t >> 5 for id t, 1 = allowed, as spl_heal_step_device writes it.
 *   free, done or broken   every bit of every one of the row's n_words words is 1.
 *   constrained            rows[q], ORed with the END bits if accept[q].  A constrained row is NEVER ALL ZERO: where that row is empty
 *                          (some[q] = 0 and q does not accept) the sequence becomes `broken` in that call and its row is ones.
 *
 * STEP: per sequence the first clamp(d_len[b], 0, row_len) ids of row b of d_ids [n_seqs, row_len] (d_len NULL: all; row_len may be 0)
 * are read in order WHILE the sequence is constrained.  For an id t:
 *   1. t is ordinary and walk(q, b(t)) = q' != DEAD: q := q'.
 *   2. otherwise, t is in END and accept[q]: the sequence is `done`; q stays the accepting state it ended in.
 *   3. otherwise -- a special that is no END id, an id of neither map, an int64 value outside 0 .. 2^32 - 1, an ordinary id whose walk
 *      dies, an END id in a state that does not accept -- the sequence is `broken`.
 * An END id that is ordinary and walks on is an ordinary id (rule 1 wins).  Later ids of a sequence that is free, done or broken are
 * not read.  Equivalently: an id is accepted iff its bit was set in the mask of the state in front of it.  The call then writes the mask
 * of the state it arrived at; row_len 0 only writes masks -- that is how the first mask is obtained after the caller wrote start states.
 *
 * WRITE-BACK, canonical: constrained q | 1 << 16; done q | 1 << 18; broken 1 << 17; free 0.  d_state_out may be d_state_in.  No other
 * output may coincide with an input or with another output.  d_live [n_seqs] uint8 (NULL ok): 1 iff the sequence is constrained after
 * the call.  SPL_DFA_KEEP_FREE: the rows of sequences that are not constrained after the call are not written at all -- the caller
 * filled them with ones once.  There is no "then free" flag: done at the first accepting state is not what a regular expression means.
 *
 * What the rule is NOT, as healing's: it ignores the split pattern, so the ids need not be the canonical encoding of the match; UTF-8
 * validity is not part of it -- a `.` or a negated class of the pattern admits any byte (spl_utf8_mask_device with SPL_UTF8_AND can AND
 * its rows into these afterwards); the table is assumed TRIMMED (every state reaches an accepting one, as splintr_amd/dfa.py leaves it):
 * that is what makes "the walk does not die" the right rule, an untrimmed table merely allows ids that lead nowhere.  Nested
 * brackets (JSON mode) are spl_nest_step_device's (below); general context-free grammars, more than 4096 states and a table per
 * sequence are out of scope.
 *
 * SHAPE.  spl_dfa_index_device: two launches on hip_stream, asynchronous -- a lane owns an id and tests its first byte before anything
 * else, a wavefront's ballot is two words of a row; then a wavefront per state ORs its row into some[q].  spl_dfa_step_device: ONE
 * launch -- a wavefront owns a sequence, walks the step's ids (serial, short) and copies the row, 16 bytes a lane where n_words is a
 * multiple of four and the mask and the index are 16-byte aligned, word by word otherwise, the END bits ORed into a word before its one
 * store.  No LDS, no scratch, no atomics on global memory, no wait between workgroups.  spl_dfa_reserve_device uploads the decode tables
 * and token healing's id -> rank (shared with spl_heal_*_device and spl_choice_*_device; synchronises once, again after
 * spl_add_special); after it neither call allocates nor synchronises.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null t, in, o, out, d_table, d_index,
 * d_state_in, d_state_out or d_mask; a null d_ids where there is an id to read; a struct_size shorter than a struct or above 4096; an
 * unknown flag bit; n_states 0 or above SPL_DFA_MAX_STATES; n_words * 32 below the largest vocabulary id + 1, or n_words above 2^26;
 * n_end 0 or above SPL_DFA_MAX_END; an END id at or above 32 * n_words; n_seqs >= 2^31; an array not aligned to its element type; an
 * output that coincides with an input (other than state out with state in) or with another output.  Arguments are refused, never
 * clamped.  A vocabulary the healing reserve refuses is refused here too. */
#define SPL_DFA_KEEP_FREE   2u  /* rows of sequences that are not constrained after the call are not written */
#define SPL_DFA_I64         4u  /* d_ids are int64 (torch.long); default int32 / uint32 bit patterns */
#define SPL_DFA_DEAD        0xFFFF
#define SPL_DFA_MAX_STATES  4096
#define SPL_DFA_STATE_WORDS 1
#define SPL_DFA_MAX_END     8
#define SPL_DFA_TABLE_BYTES(n_states) ((size_t)(n_states) * 512 + (size_t)(n_states))
#define SPL_DFA_INDEX_BYTES(n_states, n_words) ((size_t)(n_states) * ((((size_t)(n_words) + 3) & ~(size_t)3) * 4 + 1))

typedef struct spl_dfa_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled */
    uint32_t flags, n_words;
    uint32_t n_end;                       /* 1 .. SPL_DFA_MAX_END */
    uint32_t end_ids[SPL_DFA_MAX_END];
} spl_dfa_opts;
typedef struct spl_dfa_in {
    uint32_t struct_size, row_len;        /* row_len: the columns of d_ids (may be 0) */
    uint64_t n_seqs;
    const void* d_ids; const int32_t* d_len;
    const uint64_t* d_state_in;           /* [n_seqs, SPL_DFA_STATE_WORDS] */
    const uint8_t* d_table;               /* SPL_DFA_TABLE_BYTES(n_states) */
    const int32_t* d_index;               /* SPL_DFA_INDEX_BYTES(n_states, n_words), as spl_dfa_index_device left it */
    uint32_t n_states, reserved;
} spl_dfa_in;
typedef struct spl_dfa_out {
    uint32_t struct_size, reserved;
    uint64_t* d_state_out;                /* [n_seqs, SPL_DFA_STATE_WORDS] */
    int32_t* d_mask;                      /* [n_seqs, n_words] */
    uint8_t* d_live;                      /* NULL ok */
} spl_dfa_out;

int spl_dfa_reserve_device(spl_tokenizer* t);
int spl_dfa_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, uint32_t n_words, int32_t* d_index, void* hip_stream);
int spl_dfa_step_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out, void* hip_stream);

/* JUMP-FORWARD for the regex guide (csrc/spl_k_dfa_jump.h).  Where the automaton leaves no choice -- the fixed keys
 * and punctuation of a JSON object, the tags of a tool call -- the forced bytes are handed back AS IDS and cost no forward pass of the
 * model.  A forced run is a function of the state alone, so the runs of all n_states states are found on the GPU when the jump index
 * is built and are encoded once by this handle's own encoder; a decode step is then a row gather of ids beside the mask: no encode,
 * no trie on the host, no synchronisation.  walk, DEAD, ORDINARY, b(t) and the state word are spl_dfa_step_device's.
 *
 * FORCED BYTE.  force(q) = x iff accept[q] == 0 and exactly one byte x has trans[q][x] < n_states.  An accepting state is never forced:
 * an END id may follow it.  Like the index, this does not depend on the END ids.
 * RUN.  run(q) is the bytes x1 x2 ... with q1 = q and q(i+1) = trans[qi][xi], continued while force(qi) is defined, and capped at
 * SPL_DFA_JUMP_MAX_BYTES bytes (a table need not be trimmed: the cap also ends cycles).
 * UTF-8 TRIM.  After the cap the run is cut back to a character boundary of its own bytes: if it ends in a lead byte (>= 0xC0; C0..DF
 * announce one continuation byte, E0..EF two, F0..FF three) with fewer continuation bytes (80..BF) behind it than it announces, the run
 * is cut in front of that lead byte.  Leading continuation bytes stay: they finish a character begun before the run.  Example: (é|è)x
 * forces C3 from the start state; after the trim that run is empty -- without it the model could no longer draw the token "é".
 *
 * THE JUMP INDEX (SPL_DFA_JUMP_INDEX_BYTES(n_states) of device memory, the CALLER's, 4-byte aligned), written by
 * spl_dfa_jump_index_device: uint32 ids[n_states][64], then uint8 n_ids[n_states], then uint8 run_len[n_states], then uint8
 * run[n_states][64].  run[q][0 .. run_len[q]) is run(q); ids[q][0 .. n_ids[q]) are the ids of run(q) encoded as a text of its own by
 * this handle's encoder, with flags 0 and no specials; n_ids[q] == 0 iff the run is empty.  Every byte of the region is written, zeros
 * where nothing is meant.  Build it again after spl_add_special.
 *
 * JUMP STEP (spl_dfa_jump_device).  Everything spl_dfa_step_device does, from the same spl_dfa_in and spl_dfa_opts, and between the walk
 * of the sampler's ids and the mask: for a sequence still constrained in state q, n = min(n_ids[q], 64, row_len_out); the leading ids of
 * ids[q][0 .. n) are emitted for as long as each is ordinary and walks -- the first id that does not walk ends the emission and does NOT
 * break the sequence; q moves along what was emitted.  The emitted ids go to d_forced_ids[b][0 .. m) (int32 [n_seqs, row_len_out],
 * row_len_out in 1 .. 64) and m to d_forced_len[b]; entries at and beyond m are not written.  The mask, live, done, broken and the
 * empty-row break are spl_dfa_step_device's, for the state arrived at.  A sequence that is free, done or broken gets d_forced_len 0.
 * The kernel trusts nothing in the jump index: it walks what it emits and never indexes outside a table, whatever the index holds.
 * With every n_ids zero the call is spl_dfa_step_device bit for bit.
 *
 * What it is NOT: the ids are those of the run encoded ALONE -- the seam with the text in front of it is not re-tokenised (the known
 * caveat of jump-forward; spl_heal_*_device heals a seam, composing the two is the caller's).  A state that is still forced after a
 * jump (a run above 64 bytes, or row_len_out below n_ids[q]) is continued by the next call.
 *
 * SHAPE.  spl_dfa_jump_index_device is BUILD-TIME work: a wavefront per state finds the forced byte (the 512-byte row eight bytes a
 * lane, ballots and a popcount); a second launch follows the chains of at most 64 forced bytes and trims them; the runs are compacted
 * into a bytes CSR of n_states documents by the count-scan-write driver; the call then reads the runs' total bytes back -- its ONE
 * host synchronisation of hip_stream, because spl_encode_batch_device takes n_bytes from the host (a handle with SPL_PATTERN_CUSTOM
 * synchronises once more inside that encode, as every device encode of such a handle does) -- reserves workspace as needed and
 * encodes the documents through the handle's device encode path (the chunk memo may take the runs' chunks in, as after any encode; it
 * shares the handle's workspace with every other encode call: stream-ordered, as those); a last launch scatters the ids CSR into
 * ids[][] and n_ids[].  This call may ALLOCATE and SYNCHRONISES.  spl_dfa_jump_device does neither after spl_dfa_reserve_device: ONE
 * launch, a wavefront per sequence, no LDS, no scratch, no atomics on global memory, no polling.
 *
 * SPL_EINVAL, with the cause in spl_last_error() and before anything touches the device: a null handle; row_len_out 0 or above 64; a
 * null or misaligned d_forced_ids, d_forced_len or d_jump_index; a null jump struct or a struct_size shorter than it; d_forced_ids or
 * d_forced_len coinciding with any other array of the call; everything spl_dfa_step_device refuses. */
#define SPL_DFA_JUMP_MAX_BYTES 64
#define SPL_DFA_JUMP_MAX_IDS   64
#define SPL_DFA_JUMP_INDEX_BYTES(n_states) ((size_t)(n_states) * (64 * 4 + 1 + 1 + 64))

typedef struct spl_dfa_jump_out {
    uint32_t struct_size, row_len_out;    /* row_len_out: the columns of d_forced_ids, 1 .. SPL_DFA_JUMP_MAX_IDS */
    const void* d_jump_index;             /* SPL_DFA_JUMP_INDEX_BYTES(n_states), as spl_dfa_jump_index_device left it */
    int32_t* d_forced_ids;                /* [n_seqs, row_len_out] */
    int32_t* d_forced_len;                /* [n_seqs] */
} spl_dfa_jump_out;

int spl_dfa_jump_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, void* d_jump_index, void* hip_stream);
int spl_dfa_jump_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out, const spl_dfa_jump_out* jump,
                        void* hip_stream);

/* NESTED LANGUAGES -- JSON MODE -- for n_seqs sequences at once, everything in DEVICE memory (csrc/spl_k_nest.h): the
 * answer of a sequence is SOME valid JSON document (OpenAI's response_format json_object, vLLM's guided_json without a schema), or a
 * word of any other language made of regular pieces inside nested brackets.  A regular expression cannot say that; the regex guide's
 * byte automaton plus a small STACK per sequence can.  The library holds no builder: the calls take a table in the caller's device
 * memory (splintr_amd/nest.py builds the JSON one).  walk, ORDINARY, b(t), END ids, KEEP_FREE, I64, live and the empty-row break mean
 * what they mean for spl_dfa_step_device.
 *
 * THE TABLE (SPL_NEST_TABLE_BYTES(n_states, n_ret) of device memory, the CALLER's, 2-byte aligned), in this order: uint16
 * trans[S][256], uint16 ret[n_ret][16], uint8 op[S][256], uint8 accept[S].  S = n_states is 1 .. SPL_NEST_MAX_STATES, n_ret is
 * 0 .. SPL_NEST_MAX_RET.  A CONFIGURATION is (q, stack); the stack holds 4-bit symbols and is at most o->max_depth deep, max_depth in
 * 1 .. SPL_NEST_MAX_DEPTH.  One byte x from (q, stack), with v = trans[q][x] and o = op[q][x]:
 *   o == 0              (v, stack) if v < S, else DEAD.
 *   o == 0x10 | y       PUSH y (0..15): (v, stack + y) if v < S and depth < max_depth, else DEAD.
 *   o == 0x20           POP: with y the top symbol, (ret[v][y], stack - top) if depth > 0, v < n_ret and ret[v][y] < S, else DEAD.
 *   any other o         DEAD.
 * The kernels never index outside the table, whatever it holds.  END may follow (q, stack) iff accept[q] and the stack is empty.  The
 * return state of a pop depends on the popped symbol: a JSON table keeps "which container am I in" in the state and "which container
 * encloses it" on the stack.
 *
 * STACK-FREE AND TOUCHING PAIRS.  Walk b(t) from q and ignore the stack: the pair (q, t) TOUCHES iff the walk meets a byte with
 * op != 0 before it dies or ends -- whether or not that op then turns out to be valid.
 *
 * THE INDEX (SPL_NEST_INDEX_BYTES(n_states, n_words, dep_cap) of device memory, the CALLER's, 4-byte aligned), written by
 * spl_nest_index_device: int32 rows[S][stride] with the regex guide's stride, uint32 dep_off[S + 1], uint32 dep_ids[dep_cap], uint8
 * some[S].  Bit t of rows[q] is 1 iff t is ordinary, the walk ends alive and the pair does not touch; dep_ids[dep_off[q] ..
 * dep_off[q + 1]) are the ordinary ids that touch from q, ascending; some[q] is 1 iff the row has a bit.  The index depends on neither
 * the END ids nor max_depth.  spl_nest_index_device is BUILD-TIME work: it may ALLOCATE scratch and SYNCHRONISES hip_stream once, to
 * read the number of dependent entries, which it returns through *n_dep.  Where that is above dep_cap the call returns SPL_ECAPACITY
 * ("dep_cap is too small") with *n_dep set: rows, some and dep_off are then written, no entry of dep_ids is, and nothing behind the
 * index ever; call again with dep_cap >= *n_dep.
 *
 * THE STATE ROW (SPL_NEST_STATE_WORDS uint64 per sequence; all zero is free; every bit not named is 0, so rows compare bit for bit):
 *   word 0       bits 0..15 q, bit 16 constrained, bit 17 broken, bit 18 done -- as spl_dfa_step_device's -- and bits 24..30 the depth
 *   words 1..4   stack level i (0 = the bottom) in word 1 + i / 16, bits 4 * (i % 16) ..
 * TO BEGIN the caller writes start | 1 << 16 and zeros.  ON LOAD a constrained row with q >= S or depth > max_depth is broken; nibbles
 * at or above the depth are ignored and written back as zero.  A sequence that is done, broken or free is written with an empty stack.
 *
 * STEP AND MASK.  Per id, while the sequence is constrained: an ordinary id whose walk from the configuration lives moves the
 * configuration; otherwise an END id where END may follow makes the sequence done; anything else breaks it.  The mask of the
 * configuration arrived at is rows[q], ORed with the dependent ids of q whose walk from the REAL stack lives, ORed with the END bits
 * where END may follow.  If that is empty the sequence breaks in that call and its row is ones.  Free, done and broken rows are ones.
 * With every op zero, rows, some, the mask, live and state word 0 are spl_dfa_*'s bit for bit and every dep list is empty.
 *
 * SHAPE.  spl_nest_index_device: k_dfa_index's shape with two ballots per (state, 64 ids) -- alive and stack-free into rows, touching
 * into a scratch bitmap --, a wavefront per state that ORs and popcounts, an exclusive scan of at most 4096 counts in one workgroup,
 * and a wavefront per state that turns its scratch row into ascending ids.  spl_nest_step_device: ONE launch after
 * spl_nest_reserve_device, a wavefront per sequence, neither allocating nor synchronising; a state without dependent ids takes the
 * regex guide's row copy; otherwise the row goes out in pieces of 1024 words, the dependent ids of a piece walked a lane each against
 * a private copy of the stack and merged in 4 KB of LDS BEFORE the copy: every mask word is stored exactly once, nothing is read back.
 * No atomics on global memory, no wait between workgroups.
 *
 * SPL_EINVAL, before anything touches the device: everything spl_dfa_index_device and spl_dfa_step_device refuse; n_ret above
 * SPL_NEST_MAX_RET; max_depth 0 or above SPL_NEST_MAX_DEPTH; a null n_dep; index_bytes below
 * SPL_NEST_INDEX_BYTES(n_states, n_words, dep_cap).  JSON Schema, general context-free grammars, jump-forward for nest tables, more
 * than 16 stack symbols or 64 levels are out of scope. */
#define SPL_NEST_KEEP_FREE   2u
#define SPL_NEST_I64         4u
#define SPL_NEST_PUSH        0x10
#define SPL_NEST_POP         0x20
#define SPL_NEST_MAX_STATES  4096
#define SPL_NEST_MAX_RET     4096
#define SPL_NEST_MAX_DEPTH   64
#define SPL_NEST_STATE_WORDS 5
#define SPL_NEST_MAX_END     8
#define SPL_NEST_TABLE_BYTES(n_states, n_ret) ((size_t)(n_states) * 769 + (size_t)(n_ret) * 32)
#define SPL_NEST_INDEX_BYTES(n_states, n_words, dep_cap) \
    ((size_t)(n_states) * ((((size_t)(n_words) + 3) & ~(size_t)3) * 4 + 5) + 4 + (size_t)(dep_cap) * 4)

typedef struct spl_nest_opts {
    uint32_t struct_size;                 /* sizeof the struct as the CALLER was compiled */
    uint32_t flags, n_words;
    uint32_t n_end;                       /* 1 .. SPL_NEST_MAX_END */
    uint32_t end_ids[SPL_NEST_MAX_END];
    uint32_t max_depth, reserved;         /* max_depth: 1 .. SPL_NEST_MAX_DEPTH */
} spl_nest_opts;
typedef struct spl_nest_in {
    uint32_t struct_size, row_len;        /* row_len: the columns of d_ids (may be 0) */
    uint64_t n_seqs;
    const void* d_ids; const int32_t* d_len;
    const uint64_t* d_state_in;           /* [n_seqs, SPL_NEST_STATE_WORDS] */
    const uint8_t* d_table;               /* SPL_NEST_TABLE_BYTES(n_states, n_ret) */
    const int32_t* d_index;               /* SPL_NEST_INDEX_BYTES(n_states, n_words, dep_cap), as spl_nest_index_device left it */
    uint32_t n_states, n_ret;
    uint32_t dep_cap, reserved;           /* dep_cap: the one the index was built with */
    uint64_t index_bytes;                 /* the bytes behind d_index */
} spl_nest_in;
typedef struct spl_nest_out {
    uint32_t struct_size, reserved;
    uint64_t* d_state_out;                /* [n_seqs, SPL_NEST_STATE_WORDS]; may be d_state_in */
    int32_t* d_mask;                      /* [n_seqs, n_words] */
    uint8_t* d_live;                      /* NULL ok */
} spl_nest_out;

int spl_nest_reserve_device(spl_tokenizer* t);
int spl_nest_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, uint32_t n_ret, uint32_t n_words, int32_t* d_index,
                          uint32_t dep_cap, uint32_t* n_dep, void* hip_stream);
int spl_nest_step_device(spl_tokenizer* t, const spl_nest_in* in, const spl_nest_opts* o, const spl_nest_out* out, void* hip_stream);

/* DRAFT VERIFICATION for the regex guide and the nest guide (csrc/spl_k_draft.h): the guide behind a SPECULATIVE
 * sampler -- draft models, n-gram lookup, Medusa / EAGLE trees (xgrammar's "rollback", vLLM's structured output with spec decode).  The
 * verifier's one forward pass yields logits in front of every draft position; it needs the guide's mask in front of each of them and
 * where the draft leaves the language.  From ONE state row per sequence, which is only read, and a draft of up to SPL_DRAFT_MAX_NODES
 * ids per sequence, a chain or a tree, ONE launch writes the mask in front of the first draft id, the mask behind every draft id,
 * whether each id is acceptable, and optionally live and the state behind each.  Everything not named here -- table, index, state row,
 * END, ORDINARY, b(t), walk, settle, flags, refusals -- is spl_dfa_step_device's / spl_nest_step_device's.
 *
 * INPUT.  The step's spl_dfa_in / spl_nest_in and opts as they are.  row_len is the number of NODES, 0 .. SPL_DRAFT_MAX_NODES: row b of
 * d_ids holds the id of each.  d_len clamps as it does for the step; nodes at or beyond the clamped length are ABSENT.  d_parent NULL
 * is a CHAIN: node i hangs below node i - 1, node 0 below the root.  Otherwise int32 [row_len], one row for all sequences, or
 * [n_seqs, row_len] with SPL_DRAFT_PARENT_PER_SEQ in draft->flags: a parent is -1 (the root) or an index 0 .. i - 1, so every tree comes
 * in topological order.  A node whose parent is anything else (>= i, < -1), or whose ancestor is such a node or is absent, is an ORPHAN.
 * The kernel never follows a value it has not checked.  THE PATH of node i is the ids of its ancestors from the root down, then its own.
 *
 * OUTPUT.  d_mask int32 [n_seqs, 1 + row_len, n_words]: row 0 belongs to the root, row 1 + i to node i.  d_ok uint8 [n_seqs, row_len].
 * d_live uint8 [n_seqs, 1 + row_len] (NULL ok).  d_state_out uint64 [n_seqs, 1 + row_len, STATE_WORDS] (NULL ok).  d_state_in is only
 * read; no output may coincide with it, with another input or with another output.
 *   row 0        what the step writes for row_len 0: the mask in front of the first draft id.
 *   row 1 + i    of a node that is present and no orphan: mask row, state row and live are bit for bit what spl_*_step_device writes for
 *                this sequence from d_state_in when given the node's path as its ids.  As in the step nothing settles between the ids of
 *                a path; only the configuration arrived at is settled.
 *   ok[i]        1 iff the sequence is free on input, or every id of the path was read and accepted by the step's rule 1 or 2: after the
 *                walk and before the settle the sequence is constrained, or it became `done` at the path's LAST id.  A child of a node
 *                that ended the sequence, and anything below a rejected id, has ok 0; its row follows from the line above (done or
 *                broken: ones).
 *   absent, orphan   ok 0, live 0, a state row of 1 << 17 (broken) and zeros, a mask row of ones.
 * SPL_*_KEEP_FREE skips the mask rows of nodes that are not constrained, as the step does per sequence.  For a chain ok is monotone along
 * the row and its sum is the number of leading draft ids the guide accepts: the sampler takes min(that, what the model accepts), draws a
 * bonus id under the mask row of that position (row `accepted`), and commits with ONE ordinary step over the accepted ids and the bonus id.
 * A tree commits by copying the accepted node's state row into the sequence's (d_state_out).  Jump-forward inside a draft, drafts for
 * guided choice and token healing, and more than 64 nodes are out of scope.
 *
 * SHAPE.  ONE launch each, k_dfa_draft / k_nest_draft: a wavefront owns one (sequence, row) pair, the grid is (1 + row_len) by sequences.
 * Because a parent's index is below its child's, the ancestors of a node fit ONE 64-bit word: the wavefront climbs from the node through
 * d_parent setting bits -- every value checked against -1 <= p < the node it was read at, so the climb ends within 64 steps whatever the
 * array holds -- and walks the set bits in ascending order, which is root-to-node order; no local array, no scratch.  The walk, the
 * settle and the row write are the step's own code, handed the output row b * (1 + row_len) + r in place of the sequence.  A row re-walks
 * its prefix: at most 64 short serial walks against a row copy of tens of kilobytes.  The nest kernel keeps the step's 4 KB of LDS.  No
 * atomics on global memory, no wait between workgroups, no allocation and no synchronisation after spl_dfa_reserve_device /
 * spl_nest_reserve_device.
 *
 * SPL_EINVAL, before anything touches the device: everything the step refuses (its d_state_out may be NULL here); a null or short draft
 * struct; an unknown draft flag; row_len above SPL_DRAFT_MAX_NODES; a null d_ok or d_mask; d_parent not 4-byte aligned;
 * SPL_DRAFT_PARENT_PER_SEQ without d_parent; (1 + row_len) * n_seqs >= 2^31; any output coinciding with any input or other output. */
#define SPL_DRAFT_MAX_NODES      64
#define SPL_DRAFT_PARENT_PER_SEQ 1u  /* d_parent is [n_seqs, row_len]; default one row [row_len] for all sequences */

typedef struct spl_draft_out {
    uint32_t struct_size, flags;          /* flags: SPL_DRAFT_PARENT_PER_SEQ */
    const int32_t* d_parent;              /* NULL: a chain */
    int32_t* d_mask;                      /* [n_seqs, 1 + row_len, n_words] */
    uint8_t* d_ok;                        /* [n_seqs, row_len] */
    uint8_t* d_live;                      /* [n_seqs, 1 + row_len]; NULL ok */
    uint64_t* d_state_out;                /* [n_seqs, 1 + row_len, STATE_WORDS]; NULL ok */
} spl_draft_out;

int spl_dfa_draft_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_draft_out* draft, void* hip_stream);
int spl_nest_draft_device(spl_tokenizer* t, const spl_nest_in* in, const spl_nest_opts* o, const spl_draft_out* draft, void* hip_stream);

/* Host-side lookup of ONE id, for consumers that decode token by token on the CPU -- the streaming
 * decoders (src/core/streaming.rs, src/python/bindings.rs:465-834 take clones of Tokenizer::decoder
 * and special_tokens_decoder).  *bytes / *len = what decode_bytes emits for the id; the pointer
 * stays valid until spl_destroy or the next spl_add_special.  Returns 0 unknown id, 1 vocabulary
 * token, 2 vocabulary token of a ByteLevel vocabulary whose key is NOT ByteLevel text (the bytes
 * are the key itself), 3 special token. */
int spl_token_bytes(const spl_tokenizer* t, uint32_t id, const uint8_t** bytes, uint32_t* len);
/* 1 if the vocabulary's keys are ByteLevel text (from_bytes_byte_level / the container's flag). */
int spl_is_byte_level(const spl_tokenizer* t);

/* Per-kernel timing (HIP events on the launch stream).  While enabled every encode call records
 * events around each kernel; spl_profile_read returns the accumulated milliseconds and launch
 * counts per kernel since the last spl_profile_reset and synchronises the stream.
 * Slot order (spl_kernel_name gives the same names; a slot counts the CALLS in which its kernels ran, not the launches of a ranged call):
 *   0 memset + k_mark_docs   1 k_special_scan   2 k_pretok (every device call, an empty batch included)   3 k_deferred_wave
 *   4 k_bpe_segments   5 k_bpe_long   6 k_range_count   7 unused   8 k_range_out (queue mode) | k_tile_out (tile-owned mode); 9..15 unused.
 * Tile-owned mode fills slots 2 and 8 (0 and 1 too with SPL_WITH_SPECIAL).  Slot 8 tells the two forms of that mode apart: a call that ran
 * as ONE launch (option "fuse", splintr_amd/csrc/spl_k_fuse.h) leaves it alone, the two-launch form (k_pretok + k_tile_out) adds one -- and so does an
 * empty batch, which launches neither. */
#define SPL_MAX_KERNELS 16
int spl_profile_enable(spl_tokenizer* t, int on);
int spl_profile_reset(spl_tokenizer* t);
int spl_profile_read(spl_tokenizer* t, double ms_out[SPL_MAX_KERNELS], uint64_t launches_out[SPL_MAX_KERNELS]);
const char* spl_kernel_name(int index);   /* NULL past the last kernel */

/* The chunk memo of the handle's first context -- the GPU path's counterpart of the reference's LRU of encoded chunks
 * (src/core/tokenizer.rs:707-722; result-transparent there and here: keys are compared in full): out[0] fills run (k_memo_fill, between two
 * launches), out[1] chunks put in, out[2] chunks found to be beyond an entry (more than fourteen tokens: remembered as such), out[3] entries of
 * the table (0: off).  spl_set_option("memo", 0) turns it off; "memo_bits" (4..22, default 16) sizes it.  Synchronises the device. */
int spl_memo_stats(spl_tokenizer* t, uint64_t out[4]);
/* The memo's seed (option "memo_first"), first device: out[0] = vocabulary keys of 2..64 bytes put into the memo when it was created, out[1] = keys
 * that found neither of their two slots free (the vocabulary's own tables answer those).  Both 0 with "memo_first" or "memo" off.  Seeds are no
 * learned chunks: spl_memo_stats does not count them.  Where the memo does not exist yet (a fresh handle, behind "memo_clear") the figures are
 * those of the host's plan for the next launch's memo: a query, no device state is made. */
int spl_memo_seed_stats(spl_tokenizer* t, uint64_t out[2]);
/* Debug / tests: slot `slot` of the first device's memo as it lies in HBM: the entry's sixteen words (key[8], meta0, meta1, ids[6]), then
 * bytes 32..63 of the key for the table of 33..64-byte chunks (long_table != 0; zeros otherwise).  Synchronises the device. */
int spl_debug_memo_entry(spl_tokenizer* t, int long_table, uint32_t slot, uint32_t out[24]);

/* Counters of the last encode call on this handle (device -> host copy, synchronises):
 * [2] items of the global long-chunk queue (> 64 B, plus every miss of a deferred segment),
 * [3] deferred segments (scanner chains that outgrew a tile window); [0], [1] unused. */
int spl_last_queue_counts(spl_tokenizer* t, uint32_t counts_out[4]);

/* Development aid: when enabled (bit 0 of `enable`; -DSPL_DEBUG_STAMPS builds), one k_pretok workgroup
 * stamps the shader clock at its phase boundaries; the call returns the stamps of the previous batch
 * (synchronises).  Bits 1-3 force an execution mode for the tests (0 the size decides, 1 the small-tile geometry,
 * 4 queue mode, 5 tile-owned mode with the second geometry; 2 and 3 were the multi-pass pipeline, removed in round 4: SPL_EINVAL);
 * bits 4-6 cut the kernel off after a phase (profiling builds only). */
int spl_debug_phases(spl_tokenizer* t, int enable, unsigned long long stamps_out[16]);

/* Development aid: per-workgroup records of the last stamped k_pretok launch, 4 wall-clock ticks
 * each (start, end of the merge phase, counts done, end) for the first SPL_DEBUG_BLOCKS
 * workgroups.  Returns the count copied. */
#define SPL_DEBUG_BLOCKS 4096
int spl_debug_blocks(spl_tokenizer* t, unsigned long long* out, int max_blocks);

/* Development aid: the device side of spl_allgatherv_csr's last step WITHOUT a communicator (RCCL does not put two ranks on one GPU, so
 * the tests could not reach it at world > 1).  d_all_off (device memory) holds every rank's LOCAL offsets side by side, rank r's N_r of
 * them from index N_0 + .. + N_{r-1}; counts (HOST memory) is [world][2] = {T_r, N_r}.  Afterwards d_all_off[0 .. N_total] are the
 * offsets into the global id array, the closing entry T_total included; nothing else is written.  Runs the same code as
 * spl_allgatherv_csr, asynchronously on `hip_stream`; the handle only names the device.  SPL_EINVAL for world == 0 or world > 64 (the
 * largest communicator spl_comm_create accepts) -- checked first, before anything touches a device -- and for a null argument. */
int spl_debug_rebase_offsets(spl_tokenizer* t, uint64_t* d_all_off, const uint64_t* counts /* [world][2]: T, N */,
                             uint32_t world, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLINTR_HIP_H */
