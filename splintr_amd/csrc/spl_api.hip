// spl_api.hip -- the C ABI (include/splintr_hip.h): the root of the library's one HIP translation unit.  It includes the kernels
// (spl_kernels.hip) and the host side, one file per concern and each building on the ones before it -- spl_host_res.h (resource owners,
// pinned pool), spl_ctx.h (per-GPU context, handle, uploads), spl_streams.h (stream probe), spl_launch.h (memo, launch order, device
// splitter), spl_host_split.h, spl_pipeline.h (spl_encode_batch), spl_decode_host.h, spl_collective.h, spl_collate_host.h, spl_pair_host.h, spl_chat_host.h, spl_seqpack_host.h, spl_window_host.h, spl_decode_dev_host.h, spl_spans_host.h, spl_seqscan_host.h, spl_stream_host.h, spl_stop_host.h, spl_heal_host.h, spl_mask_host.h, spl_choice_host.h, spl_dfa_host.h, spl_dfa_jump_host.h, spl_nest_host.h, spl_draft_host.h -- and holds the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include "../../include/splintr_hip.h"
#include "spl_kernels.hip"
#include "spl_tables.h"
#include "spl_comm.h"
#include "spl_regex.h"
#include "spl_rx_split.h"

using namespace spl;

#include "spl_host_res.h"
#include "spl_ctx.h"
#include "spl_streams.h"
#include "spl_launch.h"
#include "spl_host_split.h"
#include "spl_pipeline.h"
#include "spl_decode_host.h"
#include "spl_collective.h"
#include "spl_collate_host.h"
#include "spl_pair_host.h"
#include "spl_chat_host.h"
#include "spl_seqpack_host.h"
#include "spl_window_host.h"
#include "spl_decode_dev_host.h"
#include "spl_spans_host.h"
#include "spl_seqscan_host.h"
#include "spl_stream_host.h"
#include "spl_stop_host.h"
#include "spl_heal_host.h"
#include "spl_mask_host.h"
#include "spl_choice_host.h"
#include "spl_dfa_host.h"
#include "spl_dfa_jump_host.h"
#include "spl_nest_host.h"
#include "spl_draft_host.h"

namespace {
// No exception crosses the C ABI: every entry point that allocates (std::bad_alloc), starts threads or grows
// containers runs inside this guard and reports SPL_EDEVICE instead.
template <class F> int guarded(const char* what, F f) {
    try { return f(); }
    catch (const std::exception& e) { return fail(SPL_EDEVICE, std::string(what) + ": " + e.what()); }
    catch (...) { return fail(SPL_EDEVICE, std::string(what) + ": unknown exception"); }
}
}  // namespace

extern "C" {

const char* spl_last_error(void) { return g_err.c_str(); }

int spl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

spl_tokenizer* spl_create(const void* vocab, size_t vocab_len, const void* uclass_tab, size_t uclass_len,
                          const spl_opts* opts_in) {
    if (!vocab || !uclass_tab || !opts_in) { fail(SPL_EINVAL, "spl_create: null argument"); return nullptr; }
    // the caller's struct may be older (smaller) than this library's: only the bytes it has are read
    spl_opts o{};
    const uint32_t have = opts_in->struct_size;
    if (refuse_struct_size("spl_create", "spl_opts", have, 8, nullptr) != SPL_OK) return nullptr;
    memcpy(&o, opts_in, std::min<size_t>(have, sizeof o));
    const spl_opts* opts = &o;
    try {
        std::unique_ptr<spl_tokenizer> t(new spl_tokenizer());
        std::string err;
        const bool custom = opts->pattern == SPL_PATTERN_CUSTOM;
        if (custom && (have < sizeof(spl_opts) || !opts->pattern_text || !opts->pattern_len)) {
            fail(SPL_EINVAL, "spl_create: SPL_PATTERN_CUSTOM needs spl_opts.pattern_text / pattern_len");
            return nullptr;
        }
        if (build_tables((const uint8_t*)vocab, vocab_len, (const uint8_t*)uclass_tab, uclass_len, custom ? SPL_PATTERN_CL100K : opts->pattern,
                         (opts->flags & SPL_OPT_BYTE_LEVEL) != 0, t->ht, err)) {
            fail(SPL_EINVAL, "spl_create: " + err);
            return nullptr;
        }
        if (custom) {
            // Tokenizer::new compiles the pattern (tokenizer.rs:426); a pattern this matcher cannot express is refused here
            t->regex = regex_compile(std::string(opts->pattern_text, (size_t)opts->pattern_len), t->ht, err);
            if (!t->regex) { fail(SPL_EINVAL, "spl_create: Regex error: " + err); return nullptr; }
            if (!regex_device_image(*t->regex, t->rx_image)) t->rx_image.clear();
        }
        t->ctx.emplace_back(new Ctx());
        t->ctx[0]->device = opts->device;
        if (upload_tables(*t->ctx[0], t->ht) != SPL_OK) return nullptr;      // (the context's destructor frees what was uploaded)
        return t.release();
    } catch (const std::exception& e) {                      // no exception crosses the C ABI
        fail(SPL_EDEVICE, std::string("spl_create: ") + e.what());
        return nullptr;
    }
}

static int spl_set_devices_impl(spl_tokenizer* t, const int32_t* devices, uint32_t n) {
    if (!t || !devices || n == 0 || n > 64) return fail(SPL_EINVAL, "spl_set_devices: bad argument");
    const int have = spl_device_count();
    for (uint32_t i = 0; i < n; i++)
        if (devices[i] < 0 || devices[i] >= have) return fail(SPL_EINVAL, "spl_set_devices: no such device");
    std::vector<std::unique_ptr<Ctx>> nc;
    for (uint32_t i = 0; i < n; i++) {
        nc.emplace_back(new Ctx());
        nc.back()->device = devices[i];
        int rc = upload_tables(*nc.back(), t->ht);
        if (rc) return rc;
    }
    t->ctx.swap(nc);
    return SPL_OK;
}

uint32_t spl_n_devices(const spl_tokenizer* t) { return t ? (uint32_t)t->ctx.size() : 0u; }

int spl_set_option(spl_tokenizer* t, const char* name, int64_t value) {
    if (!t || !name) return fail(SPL_EINVAL, "spl_set_option: null argument");
    const std::string k(name);
    auto memo_drop_all = [&] { for (auto& c : t->ctx) { c->memo_drop(); if (c->twin) c->twin->memo_drop(); } };      // (a new geometry, or Tokenizer::clear_cache)
    if (k == "chunk_bytes" && value >= 1) t->chunk_bytes = (uint64_t)value;
    else if (k == "single_chunk_max_bytes" && value >= 0) t->single_max = (uint64_t)value;
    else if (k == "result_estimate_div" && value >= 1) t->est_div = (uint32_t)value;
    else if (k == "subdoc_split") t->subdoc = value != 0;
    else if (k == "direct_write") t->direct_write = value != 0;
    else if (k == "device_split") t->rx_device = value != 0;
    else if (k == "small_path") t->small_path = value != 0;
    else if (k == "direct_read") t->direct_read = value != 0;
    else if (k == "chunk_ramp") t->chunk_ramp = value != 0;
    else if (k == "twin_streams") t->twin_streams = value != 0;
    else if (k == "pick_streams") t->pick_streams = value != 0;
    else if (k == "fuse") t->fuse = value != 0;
    else if (k == "group_scan_min" && value >= 0 && value < (1 << 24)) t->group_scan_min = (uint32_t)value;
    else if (k == "range_tiles" && value >= 0 && value < (1 << 24)) t->range_tiles = (uint32_t)value;
    else if (k == "range_streams" && (value == 1 || value == 2)) t->range_streams = (int)value;
    else if (k == "memo") t->memo = value != 0;
    else if (k == "memo_first") { if ((value != 0) != (t->memo_first != 0)) memo_drop_all(); t->memo_first = value != 0; }     // (the seed is part of the form: the next launch builds the memo anew)
    else if (k == "memo_clear") memo_drop_all();               // Tokenizer::clear_cache (tokenizer.rs:995-1000)
    else if (k == "memo_bits" && value >= 4 && value <= 22) { t->memo_bits = (uint32_t)value; memo_drop_all(); }
    else if (k == "memo_long_bits" && value >= 0 && value <= 20) { t->memo_long_bits = (uint32_t)value; memo_drop_all(); }
    else if (k == "memo_log_cap" && value >= 1 && value <= 65536) { t->memo_log_cap = (uint32_t)value; memo_drop_all(); }
    else if (k == "fuse_max_tiles" && value >= 0 && value <= (int64_t)FUSE_MAX_TILES) t->fuse_max_tiles = (uint32_t)value;
    else if (k == "copy_threads" && value >= 1 && value <= 64) t->copy_threads = (int)value;
    else if (k == "decode_chunk_ids" && value >= 1024) t->dec_chunk_ids = (uint64_t)value;
    else if (k == "sdma_d2h") t->sdma_d2h = value != 0;        // (where the HSA runtime or the device's agent cannot be found: hipMemcpyAsync, silently)
    else if (k == "window_totals_chunk" && value >= 1 && value <= (int64_t)WIN_CHUNK) t->win_chunk = (uint32_t)value;
    else if (k == "seqpack_lds_max" && value >= 0 && value <= (int64_t)SQP_LDS_MAX) t->seqpack_lds_max = (uint32_t)value;
    else if (k == "stream_one_max" && value >= 0 && value <= (int64_t)ST_ONE_MAX) t->stream_one_max = (uint32_t)value;
    else if (k == "stop_one_max" && value >= 0 && value <= (int64_t)SP_ONE_MAX) t->stop_one_max = (uint32_t)value;
    else if (k == "heal_phase" && value >= 0 && value <= 2) t->heal_phase = (uint32_t)value;
    else if (k == "jump_phase" && value >= 0 && value <= 3) t->jump_phase = (uint32_t)value;
    else if (k == "choice_piece_words" && value >= 4 && value <= (int64_t)CH_PIECE && value % 4 == 0) t->choice_piece = (uint32_t)value;
    else if (k == "slab_pack24") {
        if (value && std::max(t->ht.max_id, t->max_special_id) >= (1u << 24))
            return fail(SPL_EINVAL, "slab_pack24: an id of this tokenizer does not fit three bytes (vocabulary or special-token ids >= 2^24)");
        t->slab_pack24 = value != 0;
    }
    else return fail(SPL_EINVAL, "spl_set_option: unknown option or bad value: " + k);
    return SPL_OK;
}

int spl_get_option(const spl_tokenizer* t, const char* name, int64_t* value) {
    if (!t || !name || !value) return fail(SPL_EINVAL, "spl_get_option: null argument");
    const std::string k(name);
    const std::pair<const char*, int64_t> all[] = {
        {"chunk_bytes", (int64_t)t->chunk_bytes}, {"single_chunk_max_bytes", (int64_t)t->single_max}, {"result_estimate_div", t->est_div},
        {"subdoc_split", t->subdoc}, {"direct_write", t->direct_write}, {"device_split", t->rx_device}, {"small_path", t->small_path},
        {"direct_read", t->direct_read}, {"chunk_ramp", t->chunk_ramp}, {"twin_streams", t->twin_streams}, {"pick_streams", t->pick_streams},
        {"fuse", t->fuse}, {"group_scan_min", t->group_scan_min}, {"range_tiles", t->range_tiles}, {"range_streams", t->range_streams},
        {"memo", t->memo}, {"memo_first", t->memo_first}, {"memo_bits", t->memo_bits}, {"memo_long_bits", t->memo_long_bits},
        {"memo_log_cap", t->memo_log_cap}, {"fuse_max_tiles", t->fuse_max_tiles}, {"copy_threads", t->copy_threads},
        {"decode_chunk_ids", (int64_t)t->dec_chunk_ids}, {"sdma_d2h", t->sdma_d2h}, {"window_totals_chunk", t->win_chunk},
        {"seqpack_lds_max", t->seqpack_lds_max},
        {"stream_one_max", t->stream_one_max}, {"stop_one_max", t->stop_one_max}, {"heal_phase", t->heal_phase}, {"jump_phase", t->jump_phase},
        {"choice_piece_words", t->choice_piece},
        {"slab_pack24", t->slab_pack24},
    };
    for (const auto& e : all)
        if (k == e.first) { *value = e.second; return SPL_OK; }
    return fail(SPL_EINVAL, "spl_get_option: unknown option: " + k);
}

static int spl_add_special_impl(spl_tokenizer* t, const uint8_t* literal, size_t len, uint32_t id) {
    if (!t || !literal || len == 0) return fail(SPL_EINVAL, "spl_add_special: bad argument");
    if (len > 255) return fail(SPL_EINVAL, "spl_add_special: literal longer than 255 bytes");
    if (id > 0x7FFFFFFFu) return fail(SPL_EINVAL, "spl_add_special: id out of range");
    if (t->slab_pack24 && id >= (1u << 24))
        return fail(SPL_EINVAL, "spl_add_special: the all-gather slabs of this handle carry three bytes per id (slab_pack24): ids must be < 2^24");
    const std::string lit((const char*)literal, len);
    bool replaced = false;
    for (auto& sp : t->specials)
        if (sp.lit == lit) { sp.id = id; replaced = true; }       // a map: the later insert wins
    if (!replaced) {
        // The one-launch scan (k_special_scan) treats every occurrence as a match, which equals
        // Aho-Corasick's non-overlapping Standard semantics only if no two occurrences can ever overlap
        // (no literal contains another, no proper suffix of one is a prefix of another or of itself);
        // any other set -- or a literal beyond SP_MAXLEN bytes -- takes the general two-launch matcher.
        auto overlaps = [](const std::string& a, const std::string& b) {
            if (a.find(b) != std::string::npos || b.find(a) != std::string::npos) return true;
            for (size_t k = 1; k < a.size() && k < b.size(); k++) {
                if (a.compare(a.size() - k, k, b, 0, k) == 0) return true;   // suffix of a == prefix of b
                if (b.compare(b.size() - k, k, a, 0, k) == 0) return true;
            }
            return false;
        };
        bool general = len > (size_t)SP_MAXLEN;
        for (size_t k = 1; k < lit.size() && !general; k++)
            general = lit.compare(lit.size() - k, k, lit, 0, k) == 0;    // the literal can overlap itself
        for (const auto& sp : t->specials)
            if (!general && overlaps(sp.lit, lit)) general = true;
        if (general) t->special_general = true;
        t->specials.push_back(Special{lit, id});
    }
    for (auto& c : t->ctx) { c->sp_uploaded = false; c->dec_uploaded = false; c->heal_uploaded = false; c->u8_uploaded = false; if (c->twin) c->twin->sp_uploaded = false; }
    t->max_special_id = 0;
    t->max_tok_bytes = 0;
    for (const auto& sp : t->specials) t->max_special_id = std::max(t->max_special_id, sp.id);
    if (lit.find('\n') != std::string::npos) t->special_newline = true;
    return SPL_OK;
}

uint32_t spl_vocab_size(const spl_tokenizer* t) {
    if (!t) return 0;
    return std::max(t->ht.max_id, t->max_special_id) + 1;
}

void spl_destroy(spl_tokenizer* t) { delete t; }

static int spl_reserve_impl(spl_tokenizer* t, uint64_t max_bytes, uint64_t max_docs) {
    if (!t) return fail(SPL_EINVAL, "spl_reserve: null handle");
    return reserve(t->ctx[0].get(), max_bytes, max_docs);
}

static int spl_encode_batch_device_impl(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                            uint64_t n_docs, uint32_t flags, uint32_t* d_ids, uint64_t ids_capacity,
                            uint64_t* d_out_off, void* hip_stream) {
    if (!t || !d_doc_off || !d_out_off || (n_bytes && (!d_utf8 || !d_ids)))
        return fail(SPL_EINVAL, "spl_encode_batch_device: null argument");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    if (t->regex) return encode_device_custom(t, t->ctx[0].get(), d_utf8, n_bytes, d_doc_off, n_docs, flags, d_ids, ids_capacity, d_out_off, (hipStream_t)hip_stream, nullptr);
    return launch_all(t, t->ctx[0].get(), {.text = d_utf8, .n_bytes = n_bytes, .doc_off = d_doc_off, .n_docs = n_docs, .flags = flags,
                                           .ids = d_ids, .ids_cap = ids_capacity, .out_off = d_out_off, .stream = (hipStream_t)hip_stream});
}

static int spl_encode_batch_device_packed_impl(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                                   uint64_t n_docs, uint32_t flags, uint32_t* d_ids, uint64_t ids_capacity,
                                   uint64_t* d_out_off, uint32_t* d_slab, uint64_t cap_words, uint64_t max_docs,
                                   void* hip_stream) {
    if (!t || !d_doc_off || !d_out_off || !d_slab || (n_bytes && (!d_utf8 || !d_ids)))
        return fail(SPL_EINVAL, "spl_encode_batch_device_packed: null argument");
    if (cap_words < max_docs + 4 || n_docs > max_docs || cap_words > 0xFFFFFFFFull)
        return fail(SPL_EINVAL, "spl_encode_batch_device_packed: slab too small or beyond 2^32 words");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    SlabOut so;
    so.d_slab = d_slab; so.cap_words = cap_words; so.max_docs = max_docs;
    if (t->regex) return encode_device_custom(t, t->ctx[0].get(), d_utf8, n_bytes, d_doc_off, n_docs, flags, d_ids, ids_capacity, d_out_off, (hipStream_t)hip_stream, &so);
    return launch_all(t, t->ctx[0].get(), {.text = d_utf8, .n_bytes = n_bytes, .doc_off = d_doc_off, .n_docs = n_docs, .flags = flags,
                                           .ids = d_ids, .ids_cap = ids_capacity, .out_off = d_out_off, .stream = (hipStream_t)hip_stream, .slab = &so});
}

int spl_encode_batch(spl_tokenizer* t, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                     spl_result** out) {
    if (!t || !doc_off || !out) return fail(SPL_EINVAL, "spl_encode_batch: null argument");
    TRACE("spl_encode_batch: enter");
    if (doc_off[0] != 0) return fail(SPL_EINVAL, "spl_encode_batch: doc_off[0] must be 0");
    for (uint64_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] < doc_off[d]) return fail(SPL_EINVAL, "spl_encode_batch: doc_off must be non-decreasing");
    if (doc_off[n_docs] && !utf8) return fail(SPL_EINVAL, "spl_encode_batch: null text");
    try {
        std::unique_ptr<spl_result> r(new spl_result());
        if (t->small_path && !t->regex && doc_off[n_docs] > 0 && doc_off[n_docs] <= SMALL_MAX_BYTES && n_docs <= SMALL_MAX_DOCS) {
            int rcs = encode_small(t, utf8, doc_off, n_docs, flags, r.get());
            if (rcs) return rcs;
            t->small_calls++;
            *out = r.release();
            return SPL_OK;
        }
        const bool dev_split = rx_applies(t, flags);
        if (dev_split)                                      // (the status words of the contexts the batch may use: cleared, in stream order)
            for (auto& c : t->ctx) {
                HIP_TRY(hipSetDevice(c->device));
                int rcx = ensure_streams(*c);
                if (!rcx) rcx = rx_ensure(t, c.get());
                if (rcx) return rcx;
                if (!rcx) rcx = rx_next_status(c.get(), c->s_cmp.get());   // (this batch's status word: cleared by the previous batch's k_rx_mark)
                if (rcx) return rcx;
                c->h_rx_status.host()[0] = 0;
                c->h_rx_bad.host()[0] = 0;
            }
        int rc = encode_host(t, utf8, doc_off, n_docs, flags, r.get(), !dev_split);
        TRACE("spl_encode_batch: encode_host returned %d", rc);
        if (rc) return rc;
        if (dev_split) {
            // what the device splitter gave up on (a match longer than RX_REACH, a runaway attempt): the batch again, split on the host
            // (every chunk's split left the status word in the context's pinned copy, in front of the kernels whose completion
            //  encode_host has waited for: nothing to copy or wait for here)
            uint32_t gave_up = 0;
            for (auto& c : t->ctx) gave_up |= c->h_rx_status.host()[0];
            t->rx_fallbacks += gave_up ? n_docs : 0;
            if (gave_up) {
                r.reset(new spl_result());
                rc = encode_host(t, utf8, doc_off, n_docs, flags, r.get(), true);
                if (rc) return rc;
            }
        }
        *out = r.release();
        return SPL_OK;
    } catch (const std::exception& e) {                      // std::bad_alloc, std::system_error (thread creation): no exception crosses the C ABI
        return fail(SPL_EDEVICE, std::string("spl_encode_batch: ") + e.what());
    }
}

const uint32_t* spl_result_tokens(const spl_result* r) { return r ? r->ids : nullptr; }
const uint64_t* spl_result_offsets(const spl_result* r) { return r ? r->off : nullptr; }
uint64_t spl_result_n_tokens(const spl_result* r) { return r ? r->n_tokens : 0; }
uint64_t spl_result_n_docs(const spl_result* r) { return r ? r->n_docs : 0; }
void spl_result_free(spl_result* r) { delete r; }

void* spl_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable) != hipSuccess) {
        fail(SPL_EDEVICE, "spl_host_alloc: hipHostMalloc failed");
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void spl_host_free(void* p) { if (p) (void)hipHostFree(p); }

void spl_free(void* p) { if (p && !loose().release(p)) free(p); }

int spl_token_bytes(const spl_tokenizer* t, uint32_t id, const uint8_t** bytes, uint32_t* len) {
    if (!t || !bytes || !len) return 0;
    if (id <= t->ht.max_id && t->ht.tok_present[id]) {
        *bytes = t->ht.tok_bytes.data() + t->ht.tok_off[id];
        *len = t->ht.tok_off[id + 1] - t->ht.tok_off[id];
        return t->ht.tok_present[id];
    }
    for (size_t k = t->specials.size(); k-- > 0;)
        if (t->specials[k].id == id) {
            *bytes = (const uint8_t*)t->specials[k].lit.data();
            *len = (uint32_t)t->specials[k].lit.size();
            return 3;
        }
    return 0;
}
int spl_is_byte_level(const spl_tokenizer* t) { return t && t->ht.byte_level ? 1 : 0; }

int spl_profile_enable(spl_tokenizer* t, int on) {
    if (!t) return fail(SPL_EINVAL, "null handle");
    t->ctx[0]->prof = on != 0;
    return SPL_OK;
}
int spl_profile_reset(spl_tokenizer* t) {
    if (!t) return fail(SPL_EINVAL, "null handle");
    memset(t->ctx[0]->prof_ms, 0, sizeof t->ctx[0]->prof_ms);
    memset(t->ctx[0]->prof_n, 0, sizeof t->ctx[0]->prof_n);
    return SPL_OK;
}
int spl_profile_read(spl_tokenizer* t, double ms_out[SPL_MAX_KERNELS], uint64_t launches_out[SPL_MAX_KERNELS]) {
    if (!t) return fail(SPL_EINVAL, "null handle");
    memcpy(ms_out, t->ctx[0]->prof_ms, sizeof t->ctx[0]->prof_ms);
    memcpy(launches_out, t->ctx[0]->prof_n, sizeof t->ctx[0]->prof_n);
    return SPL_OK;
}
const char* spl_kernel_name(int index) { return (index >= 0 && index < KI_N) ? k_names[index] : nullptr; }

int spl_gatherv_pack(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, uint32_t* d_slab,
                     uint64_t cap_words, uint64_t max_docs, void* hip_stream) {
    if (!t || !d_ids || !d_out_off || !d_slab) return fail(SPL_EINVAL, "spl_gatherv_pack: null argument");
    if (n_docs > max_docs || cap_words < max_docs + 4 || cap_words > 0xFFFFFFFFull)
        return fail(SPL_EINVAL, "spl_gatherv_pack: slab too small for the document table");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    hipLaunchKernelGGL(k_gatherv_pack, dim3(256), dim3(256), 0, (hipStream_t)hip_stream, d_ids, d_out_off, (uint32_t)n_docs,
                       d_slab, (uint32_t)cap_words, (uint32_t)max_docs, t->slab_pack24 ? 1u : 0u, ~0ull);      // (the caller's CSR is whole)
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int spl_gatherv_unpack(spl_tokenizer* t, const uint32_t* d_slabs, uint32_t world, uint64_t cap_words, uint64_t max_docs,
                       uint32_t* d_all_ids, uint64_t all_ids_cap, uint64_t* d_all_off, uint32_t* d_status, void* hip_stream) {
    if (!t || !d_slabs || !d_all_ids || !d_all_off || !d_status || world == 0)
        return fail(SPL_EINVAL, "spl_gatherv_unpack: bad argument");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    hipLaunchKernelGGL(k_gatherv_unpack, dim3(128, world), dim3(256), 0, (hipStream_t)hip_stream, d_slabs, world,
                       (uint32_t)cap_words, (uint32_t)max_docs, d_all_ids, all_ids_cap, d_all_off, d_status,
                       (uint64_t)cap_words, (uint64_t)0, t->slab_pack24 ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int spl_gatherv_unpack_group(spl_tokenizer* t, const uint32_t* d_slabs, uint32_t world, uint32_t depth, uint32_t n_batches,
                             uint64_t cap_words, uint64_t max_docs, uint32_t* d_all_ids, uint64_t all_ids_cap,
                             uint64_t* d_all_off, uint64_t off_stride, uint32_t* d_status, void* hip_stream) {
    if (!t || !d_slabs || !d_all_ids || !d_all_off || !d_status || world == 0 || depth == 0 || n_batches > depth)
        return fail(SPL_EINVAL, "spl_gatherv_unpack_group: bad argument");
    if (n_batches == 0) return SPL_OK;
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    hipLaunchKernelGGL(k_gatherv_unpack, dim3(128, world, n_batches), dim3(256), 0, (hipStream_t)hip_stream, d_slabs, world,
                       (uint32_t)cap_words, (uint32_t)max_docs, d_all_ids, all_ids_cap, d_all_off, d_status,
                       (uint64_t)depth * cap_words, off_stride, t->slab_pack24 ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int spl_gatherv_unpack_at(spl_tokenizer* t, const uint32_t* d_slabs, uint32_t world, uint64_t cap_words, uint64_t max_docs,
                          uint32_t* d_all_ids, uint64_t all_ids_cap, uint64_t* d_all_off, uint64_t all_off_cap, uint64_t* d_run,
                          uint32_t* d_status, void* hip_stream) {
    if (!t || !d_slabs || !d_all_ids || !d_all_off || !d_run || !d_status || world == 0 || cap_words < max_docs + 4 || cap_words > 0xFFFFFFFFull)
        return fail(SPL_EINVAL, "spl_gatherv_unpack_at: bad argument");
    HIP_TRY(hipSetDevice(t->ctx[0]->device));
    hipLaunchKernelGGL(k_gatherv_unpack_at, dim3(128, world), dim3(256), 0, (hipStream_t)hip_stream, d_slabs, world, (uint32_t)cap_words,
                       (uint32_t)max_docs, d_all_ids, all_ids_cap, d_all_off, all_off_cap, (const uint64_t*)d_run, d_status, t->slab_pack24 ? 1u : 0u);
    hipLaunchKernelGGL(k_gatherv_advance, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, d_slabs, world, (uint32_t)cap_words, d_run);
    HIP_TRY(hipGetLastError());
    return SPL_OK;
}

int spl_pad_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, const spl_collate_opts* o,
                   void* d_rows, uint8_t* d_mask, int32_t* d_len, void* hip_stream) {
    return guarded("spl_pad_device", [&] { return pad_device(t, d_ids, d_out_off, n_docs, o, d_rows, d_mask, d_len, (hipStream_t)hip_stream); });
}

int spl_decode_reserve_device(spl_tokenizer* t, uint64_t max_ids) {
    return guarded("spl_decode_reserve_device", [&] { return decode_reserve_device(t, max_ids); });
}

int spl_decode_batch_device(spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap, const uint64_t* d_ids_off, const int32_t* d_len,
                            uint64_t n_docs, const spl_decode_opts* o, uint8_t* d_bytes, uint64_t bytes_capacity, uint64_t* d_out_off,
                            void* hip_stream) {
    return guarded("spl_decode_batch_device", [&] {
        return decode_batch_device(t, d_ids, n_ids_cap, d_ids_off, d_len, n_docs, o, d_bytes, bytes_capacity, d_out_off, (hipStream_t)hip_stream); });
}

uint32_t spl_max_token_bytes(const spl_tokenizer* t) { return t ? max_token_bytes(t) : 0u; }

int spl_token_spans_device(spl_tokenizer* t, const void* d_ids, uint64_t n_ids_cap, const uint64_t* d_ids_off, const int32_t* d_len,
                           uint64_t n_docs, const spl_decode_opts* o, uint32_t span_flags, void* d_byte_span, void* d_char_span,
                           uint64_t* d_byte_off, uint64_t* d_char_off, void* hip_stream) {
    return guarded("spl_token_spans_device", [&] {
        return token_spans_device(t, d_ids, n_ids_cap, d_ids_off, d_len, n_docs, o, span_flags, d_byte_span, d_char_span, d_byte_off,
                                  d_char_off, (hipStream_t)hip_stream); });
}

int spl_stream_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    return guarded("spl_stream_reserve_device", [&] { return stream_reserve_device(t, max_seqs); });
}

int spl_stream_decode_device(spl_tokenizer* t, const void* d_ids, const int32_t* d_len, uint64_t n_seqs, const spl_decode_opts* o,
                             uint32_t stream_flags, const uint8_t* d_final, const uint64_t* d_state_in, uint64_t* d_state_out, uint8_t* d_bytes,
                             uint64_t bytes_capacity, uint64_t* d_out_off, void* hip_stream) {
    return guarded("spl_stream_decode_device", [&] {
        return stream_decode_device(t, {.ids = d_ids, .len = d_len, .n_seqs = n_seqs, .o = o, .stream_flags = stream_flags, .fin = d_final,
                                        .state_in = d_state_in, .state_out = d_state_out, .bytes = d_bytes, .bytes_cap = bytes_capacity,
                                        .out_off = d_out_off, .stream = (hipStream_t)hip_stream}); });
}

int spl_stop_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    return guarded("spl_stop_reserve_device", [&] { return stop_reserve_device(t, max_seqs); });
}

int spl_stop_match_device(spl_tokenizer* t, const uint8_t* d_in_bytes, uint64_t in_capacity, const uint64_t* d_in_off, uint64_t n_seqs,
                          const uint8_t* d_table, const uint64_t* d_mask, const uint8_t* d_final, uint32_t stop_flags,
                          const uint64_t* d_state_in, uint64_t* d_state_out, uint8_t* d_out_bytes, uint64_t out_capacity, uint64_t* d_out_off,
                          int32_t* d_hit, void* hip_stream) {
    return guarded("spl_stop_match_device", [&] {
        return stop_match_device(t, {.in = d_in_bytes, .in_cap = in_capacity, .in_off = d_in_off, .n_seqs = n_seqs, .table = d_table,
                                     .mask = d_mask, .fin = d_final, .flags = stop_flags, .state_in = d_state_in, .state_out = d_state_out,
                                     .out = d_out_bytes, .out_cap = out_capacity, .out_off = d_out_off, .hit = d_hit,
                                     .stream = (hipStream_t)hip_stream}); });
}

int spl_heal_reserve_device(spl_tokenizer* t, uint64_t max_seqs) {
    return guarded("spl_heal_reserve_device", [&] { return heal_reserve_device(t, max_seqs); });
}

int spl_heal_begin_device(spl_tokenizer* t, const spl_heal_in* in, const spl_heal_opts* o, const spl_heal_out* out, void* hip_stream) {
    return guarded("spl_heal_begin_device", [&] { return heal_device(t, true, in, o, out, (hipStream_t)hip_stream); });
}

int spl_heal_step_device(spl_tokenizer* t, const spl_heal_in* in, const spl_heal_opts* o, const spl_heal_out* out, void* hip_stream) {
    return guarded("spl_heal_step_device", [&] { return heal_device(t, false, in, o, out, (hipStream_t)hip_stream); });
}

int spl_choice_reserve_device(spl_tokenizer* t) {
    return guarded("spl_choice_reserve_device", [&] { return choice_reserve_device(t); });
}

int spl_choice_step_device(spl_tokenizer* t, const spl_choice_in* in, const spl_choice_opts* o, const spl_choice_out* out, void* hip_stream) {
    return guarded("spl_choice_step_device", [&] { return choice_step_device(t, in, o, out, (hipStream_t)hip_stream); });
}

int spl_dfa_reserve_device(spl_tokenizer* t) {
    return guarded("spl_dfa_reserve_device", [&] { return dfa_reserve_device(t); });
}

int spl_dfa_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, uint32_t n_words, int32_t* d_index, void* hip_stream) {
    return guarded("spl_dfa_index_device", [&] { return dfa_index_device(t, d_table, n_states, n_words, d_index, (hipStream_t)hip_stream); });
}

int spl_dfa_step_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out, void* hip_stream) {
    return guarded("spl_dfa_step_device", [&] { return dfa_step_device(t, in, o, out, (hipStream_t)hip_stream); });
}

int spl_dfa_jump_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, void* d_jump_index, void* hip_stream) {
    return guarded("spl_dfa_jump_index_device", [&] { return dfa_jump_index_device(t, d_table, n_states, d_jump_index, (hipStream_t)hip_stream); });
}

int spl_dfa_jump_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_dfa_out* out, const spl_dfa_jump_out* jump, void* hip_stream) {
    return guarded("spl_dfa_jump_device", [&] { return dfa_jump_device(t, in, o, out, jump, (hipStream_t)hip_stream); });
}

int spl_nest_reserve_device(spl_tokenizer* t) {
    return guarded("spl_nest_reserve_device", [&] { return nest_reserve_device(t); });
}

int spl_nest_index_device(spl_tokenizer* t, const uint8_t* d_table, uint32_t n_states, uint32_t n_ret, uint32_t n_words, int32_t* d_index, uint32_t dep_cap,
                          uint32_t* n_dep, void* hip_stream) {
    return guarded("spl_nest_index_device", [&] { return nest_index_device(t, d_table, n_states, n_ret, n_words, d_index, dep_cap, n_dep, (hipStream_t)hip_stream); });
}

int spl_nest_step_device(spl_tokenizer* t, const spl_nest_in* in, const spl_nest_opts* o, const spl_nest_out* out, void* hip_stream) {
    return guarded("spl_nest_step_device", [&] { return nest_step_device(t, in, o, out, (hipStream_t)hip_stream); });
}

int spl_dfa_draft_device(spl_tokenizer* t, const spl_dfa_in* in, const spl_dfa_opts* o, const spl_draft_out* draft, void* hip_stream) {
    return guarded("spl_dfa_draft_device", [&] { return dfa_draft_device(t, in, o, draft, (hipStream_t)hip_stream); });
}

int spl_nest_draft_device(spl_tokenizer* t, const spl_nest_in* in, const spl_nest_opts* o, const spl_draft_out* draft, void* hip_stream) {
    return guarded("spl_nest_draft_device", [&] { return nest_draft_device(t, in, o, draft, (hipStream_t)hip_stream); });
}

int spl_utf8_mask_reserve_device(spl_tokenizer* t) {
    return guarded("spl_utf8_mask_reserve_device", [&] { return utf8_mask_reserve_device(t); });
}

int spl_utf8_mask_device(spl_tokenizer* t, const uint64_t* d_state, uint64_t n_seqs, const spl_decode_opts* o, uint32_t flags, uint32_t n_words,
                         int32_t* d_mask, uint8_t* d_live, void* hip_stream) {
    return guarded("spl_utf8_mask_device", [&] { return utf8_mask_device(t, d_state, n_seqs, o, flags, n_words, d_mask, d_live, (hipStream_t)hip_stream); });
}

int spl_mask_apply_device(spl_tokenizer* t, const spl_mask_apply* a, void* hip_stream) {
    return guarded("spl_mask_apply_device", [&] { return mask_apply_device(t, a, (hipStream_t)hip_stream); });
}

int spl_pack_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, const spl_collate_opts* o,
                    void* d_rows, uint64_t rows_cap, int32_t* d_doc, int32_t* d_pos, uint64_t* d_n, void* hip_stream) {
    return guarded("spl_pack_device", [&] {
        return pack_device(t, d_ids, d_out_off, n_docs, o, d_rows, rows_cap, d_doc, d_pos, d_n, (hipStream_t)hip_stream); });
}

int spl_pair_device(spl_tokenizer* t, const uint32_t* d_a_ids, const uint64_t* d_a_off, uint64_t n_a, const uint32_t* d_b_ids,
                    const uint64_t* d_b_off, uint64_t n_b, const int32_t* d_a_idx, const int32_t* d_b_idx, uint64_t n_pairs,
                    const spl_pair_opts* o, void* d_rows, uint8_t* d_mask, uint8_t* d_type, uint8_t* d_special, int32_t* d_len,
                    int32_t* d_kept, uint32_t* d_status, void* hip_stream) {
    return guarded("spl_pair_device", [&] {
        return pair_device(t, d_a_ids, d_a_off, n_a, d_b_ids, d_b_off, n_b, d_a_idx, d_b_idx, n_pairs, o, d_rows, d_mask, d_type, d_special,
                           d_len, d_kept, d_status, (hipStream_t)hip_stream); });
}

uint64_t spl_chat_work_bytes(uint64_t n_turns, uint64_t n_convs) { return chat_work_bytes(n_turns, n_convs); }

int spl_chat_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_off, uint64_t n_docs, const int32_t* d_turn_doc,
                    const uint8_t* d_turn_role, const uint8_t* d_turn_train, uint64_t n_turns, const uint64_t* d_conv_off, uint64_t n_convs,
                    const spl_chat_opts* o, void* d_rows, void* d_labels, uint8_t* d_loss, uint8_t* d_mask, uint8_t* d_role, uint8_t* d_special,
                    int32_t* d_len, int32_t* d_kept, int32_t* d_turn_col, uint32_t* d_status, void* d_work, void* hip_stream) {
    return guarded("spl_chat_device", [&] {
        return chat_device(t, d_ids, d_off, n_docs, d_turn_doc, d_turn_role, d_turn_train, n_turns, d_conv_off, n_convs, o, d_rows, d_labels,
                           d_loss, d_mask, d_role, d_special, d_len, d_kept, d_turn_col, d_status, d_work, (hipStream_t)hip_stream); });
}

uint64_t spl_seqpack_work_bytes(uint64_t n_seqs, uint64_t max_rows, uint32_t strategy) { (void)strategy; return sqp_work_bytes(n_seqs, max_rows); }

int spl_seqpack_device(spl_tokenizer* t, const spl_seqpack_in* in, const spl_seqpack_opts* o, const spl_seqpack_out* out, void* d_work,
                       void* hip_stream) {
    return guarded("spl_seqpack_device", [&] { return seqpack_device(t, in, o, out, d_work, (hipStream_t)hip_stream); });
}

uint64_t spl_window_work_bytes(uint64_t n_docs) { return window_work_bytes(n_docs); }

int spl_window_device(spl_tokenizer* t, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, const spl_collate_opts* o,
                      uint32_t overlap, void* d_rows, uint64_t rows_cap, uint8_t* d_mask, int32_t* d_len, int32_t* d_row_doc,
                      int64_t* d_row_start, uint64_t* d_row_off, uint64_t* d_n, void* d_work, void* hip_stream) {
    return guarded("spl_window_device", [&] {
        return window_device(t, d_ids, d_out_off, n_docs, o, overlap, d_rows, rows_cap, d_mask, d_len, d_row_doc, d_row_start, d_row_off, d_n,
                             d_work, (hipStream_t)hip_stream); });
}

int spl_debug_blocks(spl_tokenizer* t, unsigned long long* out, int max_blocks) {
    if (!t || !out) return fail(SPL_EINVAL, "null argument");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    if (!c->d_dbg.get()) return 0;
    const int n = max_blocks < SPL_DEBUG_BLOCKS ? max_blocks : SPL_DEBUG_BLOCKS;
    HIP_TRY(hipMemcpy(out, c->d_dbg.get() + 16, (size_t)n * 32, hipMemcpyDeviceToHost));
    return n;
}

int spl_debug_phases(spl_tokenizer* t, int enable, unsigned long long stamps_out[16]) {
    if (!t) return fail(SPL_EINVAL, "null handle");
    if (((enable >> 1) & 7) == 2 || ((enable >> 1) & 7) == 3)
        return fail(SPL_EINVAL, "spl_debug_phases: geometries 2 and 3 were the multi-pass pipeline, removed in round 4");
    for (auto& cp : t->ctx) {
        Ctx* c = cp.get();
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        if (c == t->ctx[0].get() && stamps_out && c->d_dbg.get()) HIP_TRY(hipMemcpy(stamps_out, c->d_dbg.get(), 16 * 8, hipMemcpyDeviceToHost));
        c->dbg_on = (enable & 1) != 0;
        c->stop_phase = (enable >> 4) & 7;
        c->force_tile = (enable >> 1) & 7;      // development: 1 = small tiles, 2 = large tiles, 3 = small tiles + multi-pass, 4 = queue mode, 5 = tile-owned with geometry B
    }
    return SPL_OK;
}

int spl_debug_rebase_offsets(spl_tokenizer* t, uint64_t* d_all_off, const uint64_t* counts, uint32_t world, void* hip_stream) {
    if (world == 0 || world > (uint32_t)COMM_MAX_WORLD) return fail(SPL_EINVAL, "spl_debug_rebase_offsets: world must be 1 .. 64");
    if (!t || !d_all_off || !counts) return fail(SPL_EINVAL, "spl_debug_rebase_offsets: null argument");
    return guarded("spl_debug_rebase_offsets", [&] {
        HIP_TRY(hipSetDevice(t->ctx[0]->device));
        return rebase_offsets(d_all_off, counts, 2, world, (hipStream_t)hip_stream);
    });
}

#ifdef SPL_MERGE_TIMING
int spl_debug_merge_timing(unsigned long long out[8], int reset) {
    if (reset) { unsigned long long z[8] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(spl::g_mt), z, sizeof z); return 0; }
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(spl::g_mt), 64);
    return 0;
}
#endif

int spl_memo_stats(spl_tokenizer* t, uint64_t out[4]) {
    if (!t || !out) return fail(SPL_EINVAL, "null argument");
    Ctx* c = t->ctx[0].get();
    const Memo& m = c->memo;
    out[0] = m.fills; out[1] = out[2] = 0; out[3] = m ? (uint64_t)m.mask + 1 + (m.d_tab2 ? (uint64_t)m.mask2 + 1 : 0) : 0;
    if (m) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        unsigned long long st[2] = {0, 0};
        HIP_TRY(hipMemcpy(st, m.d_stats.get(), 16, hipMemcpyDeviceToHost));
        out[1] = st[0]; out[2] = st[1];
    }
    return SPL_OK;
}

int spl_memo_seed_stats(spl_tokenizer* t, uint64_t out[2]) {
    if (!t || !out) return fail(SPL_EINVAL, "null argument");
    Ctx* c = t->ctx[0].get();
    out[0] = out[1] = 0;
    if (c->memo) { out[0] = c->memo.seed_placed; out[1] = c->memo.seed_left; }
    else if (t->memo && t->memo_first) {                        // (no memo yet: what the next launch will seed -- the host's plan, no device state)
        std::lock_guard<std::mutex> lock(t->seed_mu);
        const spl::MemoSeedPlan& plan = memo_seed_planned(t, t->memo_bits, t->memo_long_bits);
        out[0] = plan.placed; out[1] = plan.left_out;
    }
    return SPL_OK;
}

// Debug / tests: one slot of the first device's memo as it lies in HBM -- the entry's sixteen words (MemoEnt), then bytes 32..63 of the key for the
// table of 33..64-byte chunks (zeros for the other).  SPL_EINVAL where there is no such table or slot.  Synchronises the device.
int spl_debug_memo_entry(spl_tokenizer* t, int long_table, uint32_t slot, uint32_t out[24]) {
    if (!t || !out) return fail(SPL_EINVAL, "null argument");
    Ctx* c = t->ctx[0].get();
    const bool lng = long_table != 0;
    const Memo& m = c->memo;
    if (!m || (lng && !m.d_tab2) || slot > (lng ? m.mask2 : m.mask)) return fail(SPL_EINVAL, "spl_debug_memo_entry: no such table or slot");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    memset(out, 0, 24 * sizeof(uint32_t));
    if (!lng) HIP_TRY(hipMemcpy(out, m.d_tab.get() + slot, sizeof(MemoEnt), hipMemcpyDeviceToHost));
    else {
        const Memo2Parts p = m.parts2();
        HIP_TRY(hipMemcpy(out, p.ent + slot, sizeof(MemoEnt), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out + 16, p.hi + slot, sizeof(MemoHi), hipMemcpyDeviceToHost));
    }
    return SPL_OK;
}

int spl_last_queue_counts(spl_tokenizer* t, uint32_t counts_out[4]) {
    if (!t || !t->ctx[0]->d_zero.get()) return fail(SPL_EINVAL, "no batch has run");
    Ctx* c = t->ctx[0].get();
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    if (!c->last_qcount) {       // single-pass call: no global queues exist
        for (int i = 0; i < 4; i++) counts_out[i] = 0;
        return SPL_OK;
    }
    uint32_t q[8];
    HIP_TRY(hipMemcpy(q, c->last_qcount, 32, hipMemcpyDeviceToHost));
    counts_out[0] = q[0]; counts_out[1] = q[1]; counts_out[3] = q[3];
    counts_out[2] = q[2] + q[4];             // the long-chunk queue is filled from both ends
    return SPL_OK;
}

int spl_set_devices(spl_tokenizer* t, const int32_t* devices, uint32_t n) {
    return guarded("spl_set_devices", [&] { return spl_set_devices_impl(t, devices, n); });
}
int spl_add_special(spl_tokenizer* t, const uint8_t* literal, size_t len, uint32_t id) {
    return guarded("spl_add_special", [&] { return spl_add_special_impl(t, literal, len, id); });
}
int spl_reserve(spl_tokenizer* t, uint64_t max_bytes, uint64_t max_docs) {
    return guarded("spl_reserve", [&] { return spl_reserve_impl(t, max_bytes, max_docs); });
}
int spl_encode_batch_device(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                            uint64_t n_docs, uint32_t flags, uint32_t* d_ids, uint64_t ids_capacity,
                            uint64_t* d_out_off, void* hip_stream) {
    return guarded("spl_encode_batch_device", [&] {
        return spl_encode_batch_device_impl(t, d_utf8, n_bytes, d_doc_off, n_docs, flags, d_ids, ids_capacity, d_out_off, hip_stream); });
}
int spl_encode_batch_device_packed(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                                   uint64_t n_docs, uint32_t flags, uint32_t* d_ids, uint64_t ids_capacity,
                                   uint64_t* d_out_off, uint32_t* d_slab, uint64_t cap_words, uint64_t max_docs,
                                   void* hip_stream) {
    return guarded("spl_encode_batch_device_packed", [&] {
        return spl_encode_batch_device_packed_impl(t, d_utf8, n_bytes, d_doc_off, n_docs, flags, d_ids, ids_capacity, d_out_off,
                                                   d_slab, cap_words, max_docs, hip_stream); });
}
int spl_decode_batch(spl_tokenizer* t, const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs, uint8_t** out_bytes,
                     uint64_t** out_off) {
    return guarded("spl_decode_batch", [&] { return spl_decode_batch_impl(t, ids, ids_off, n_docs, out_bytes, out_off); });
}

int spl_comm_unique_id(uint8_t id_out[SPL_COMM_ID_BYTES]) {
    if (!id_out) return fail(SPL_EINVAL, "spl_comm_unique_id: null argument");
    return guarded("spl_comm_unique_id", [&] {
        Rccl& R = rccl();
        if (!R.lib) return fail(SPL_EDEVICE, "spl_comm_unique_id: " + R.err);
        ncclUniqueId uid;
        NCCL_TRY(R.GetUniqueId(&uid));
        memcpy(id_out, uid.internal, SPL_COMM_ID_BYTES);
        return SPL_OK;
    });
}
spl_comm* spl_comm_create(const uint8_t id[SPL_COMM_ID_BYTES], int rank, int world, int device) {
    if (!id || world < 1 || world > COMM_MAX_WORLD || rank < 0 || rank >= world) { fail(SPL_EINVAL, "spl_comm_create: bad argument"); return nullptr; }
    spl_comm* c = nullptr;
    if (guarded("spl_comm_create", [&] { return comm_create(id, rank, world, device, &c); }) != SPL_OK) return nullptr;
    return c;
}
void spl_comm_destroy(spl_comm* c) {
    if (!c) return;
    if (hipSetDevice(c->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (c->comm) (void)rccl().CommDestroy(c->comm);
    }
    delete c;                                 // (its buffers free themselves)
}
int spl_comm_rank(const spl_comm* c) { return c ? c->rank : -1; }
int spl_comm_world(const spl_comm* c) { return c ? c->world : 0; }
int spl_allgather_slabs(spl_comm* c, const uint32_t* d_send, uint32_t* d_recv, uint64_t words_per_rank, void* hip_stream) {
    if (!c || !d_send || !d_recv) return fail(SPL_EINVAL, "spl_allgather_slabs: null argument");
    return guarded("spl_allgather_slabs", [&] {
        HIP_TRY(hipSetDevice(c->device));
        NCCL_TRY(rccl().AllGather(d_send, d_recv, words_per_rank, ncclUint32, c->comm, (hipStream_t)hip_stream));
        return SPL_OK;
    });
}
int spl_allgather_slabs_p2p(spl_comm* c, const uint32_t* d_send, uint32_t* d_recv, uint64_t words_per_rank, void* hip_stream) {
    if (!c || !d_send || !d_recv) return fail(SPL_EINVAL, "spl_allgather_slabs_p2p: null argument");
    return guarded("spl_allgather_slabs_p2p", [&] {
        Rccl& R = rccl();
        HIP_TRY(hipSetDevice(c->device));
        NCCL_TRY(R.GroupStart());
        for (int p = 0; p < c->world; p++) {
            NCCL_TRY(R.Send(d_send, words_per_rank, ncclUint32, p, c->comm, (hipStream_t)hip_stream));
            NCCL_TRY(R.Recv(d_recv + (size_t)p * words_per_rank, words_per_rank, ncclUint32, p, c->comm, (hipStream_t)hip_stream));
        }
        NCCL_TRY(R.GroupEnd());
        return SPL_OK;
    });
}
int spl_allgatherv_csr(spl_comm* c, const uint32_t* d_ids, const uint64_t* d_out_off, uint64_t n_docs, uint32_t* d_all_ids,
                       uint64_t all_ids_cap, uint64_t* d_all_off, uint64_t all_off_cap, uint64_t* n_tokens_total,
                       uint64_t* n_docs_total, void* hip_stream) {
    if (!c || !d_out_off || !d_all_ids || !d_all_off) return fail(SPL_EINVAL, "spl_allgatherv_csr: null argument");
    return guarded("spl_allgatherv_csr", [&] {
        return allgatherv_csr(c, d_ids, d_out_off, n_docs, d_all_ids, all_ids_cap, d_all_off, all_off_cap, n_tokens_total, n_docs_total,
                              (hipStream_t)hip_stream);
    });
}

int spl_split_host(spl_tokenizer* t, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t* start_bits,
                   uint32_t* gap_bits) {
    if (!t || !doc_off || !start_bits || !gap_bits) return fail(SPL_EINVAL, "spl_split_host: null argument");
    if (!t->regex) return fail(SPL_EINVAL, "spl_split_host: the handle has no custom split pattern (its pattern runs on the GPU)");
    if (doc_off[0] != 0) return fail(SPL_EINVAL, "spl_split_host: doc_off[0] must be 0");
    for (uint64_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] < doc_off[d]) return fail(SPL_EINVAL, "spl_split_host: doc_off must be non-decreasing");
    if (doc_off[n_docs] && !utf8) return fail(SPL_EINVAL, "spl_split_host: null text");
    return guarded("spl_split_host", [&] {
        const uint64_t words = doc_off[n_docs] / 32 + 2;
        memset(start_bits, 0, words * 4);
        memset(gap_bits, 0, words * 4);
        return host_split_docs(t, utf8, doc_off, n_docs, false, start_bits, gap_bits, nullptr, 128);
    });
}

int spl_split_device(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off, uint64_t n_docs,
                     uint32_t* d_start_bits, uint32_t* d_gap_bits, uint32_t* d_status, void* hip_stream) {
    if (!t || !d_doc_off || !d_start_bits || !d_gap_bits || !d_status || (n_bytes && !d_utf8))
        return fail(SPL_EINVAL, "spl_split_device: null argument");
    if (!t->regex) return fail(SPL_EINVAL, "spl_split_device: the handle has no custom split pattern (its pattern runs inside the tile kernel)");
    if (t->rx_image.empty()) return fail(SPL_EINVAL, "spl_split_device: this pattern's program does not fit the device matcher (use spl_split_host)");
    return guarded("spl_split_device", [&] {
        HIP_TRY(hipSetDevice(t->ctx[0]->device));
        return rx_launch(t, t->ctx[0].get(), d_utf8, n_bytes, d_doc_off, n_docs, d_start_bits, d_gap_bits, d_status, (hipStream_t)hip_stream, nullptr, 0, nullptr,
                         true);      // (the public half has no per-document fallback behind it: anything given up on shows in *d_status)
    });
}

uint64_t spl_device_split_fallbacks(const spl_tokenizer* t) { return t ? t->rx_fallbacks : 0; }
uint64_t spl_small_path_calls(const spl_tokenizer* t) { return t ? t->small_calls : 0; }

int spl_pick_stream(int device, void* const* busy_hip_streams, uint32_t n_busy, void** hip_stream_out, double* conflict_us) {
    if (!hip_stream_out || (n_busy && !busy_hip_streams)) return fail(SPL_EINVAL, "spl_pick_stream: null argument");
    HIP_TRY(hipSetDevice(device));
    std::vector<hipStream_t> busy;
    for (uint32_t i = 0; i < n_busy; i++) busy.push_back((hipStream_t)busy_hip_streams[i]);
    hipStream_t s = nullptr;
    int rc = pick_stream_beside(busy, &s, conflict_us);
    if (rc) return rc;
    *hip_stream_out = (void*)s;
    return SPL_OK;
}

int spl_encode_chunks_device(spl_tokenizer* t, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                             uint64_t n_docs, const uint32_t* d_start_bits, const uint32_t* d_gap_bits, uint32_t* d_ids,
                             uint64_t ids_capacity, uint64_t* d_out_off, void* hip_stream) {
    if (!t || !d_doc_off || !d_out_off || !d_start_bits || !d_gap_bits || (n_bytes && (!d_utf8 || !d_ids)))
        return fail(SPL_EINVAL, "spl_encode_chunks_device: null argument");
    return guarded("spl_encode_chunks_device", [&] {
        HIP_TRY(hipSetDevice(t->ctx[0]->device));
        ExtIn ext;
        ext.d_starts = d_start_bits; ext.d_gaps = d_gap_bits;
        return launch_all(t, t->ctx[0].get(), {.text = d_utf8, .n_bytes = n_bytes, .doc_off = d_doc_off, .n_docs = n_docs,
                                               .ids = d_ids, .ids_cap = ids_capacity, .out_off = d_out_off, .stream = (hipStream_t)hip_stream, .ext = &ext});
    });
}

}  // extern "C"
