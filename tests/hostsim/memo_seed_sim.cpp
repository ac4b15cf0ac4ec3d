// memo_seed_sim.cpp -- TEST TOOL (not part of the product, never shipped in the package).
//
// The chunk memo's seed on a machine without a GPU: the product's host table builder and its placement of the vocabulary's keys into a new
// memo (spl_tables.cpp memo_seed_plan), with the very hash functions the tile kernel's memo_probe uses (spl_common.h), compiled with plain g++.
// The checks themselves are tests/test_memo_seed_cpu.py's; this file only hands out the plan, the candidate slots of a key, the whole-chunk
// probe (spl_lookup.h probe_chunk) and the decoder's view of the vocabulary.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../splintr_amd/csrc/spl_lookup.h"
#include "../../splintr_amd/csrc/spl_tables.h"

using namespace spl;

namespace {
struct Sim {
    HostTables ht;
    DeviceTables dt;
    MemoSeedPlan plan;
};
std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
struct KeyAcc {           // a record's zero-padded key words as probe_chunk's text
    const uint32_t* k; int words;
    uint32_t load32(int p) const {
        uint32_t w = 0;
        for (int i = 0; i < 4; i++) { const int q = p + i; if (q < 4 * words) w |= ((k[q >> 2] >> (8 * (q & 3))) & 0xFFu) << (8 * i); }
        return w;
    }
};
}  // namespace

extern "C" {

void* ms_create(const char* vocab, const char* ucls, int pattern, char* errbuf, int errlen) {
    Sim* s = new Sim();
    auto v = slurp(vocab), u = slurp(ucls);
    std::string err;
    if (build_tables(v.data(), v.size(), u.data(), u.size(), pattern, false, s->ht, err)) {
        snprintf(errbuf, errlen, "%s", err.c_str());
        delete s;
        return nullptr;
    }
    HostTables& h = s->ht;
    s->dt = DeviceTables{};
    DeviceTables& d = s->dt;
    d.short_tab = h.short_tab.data(); d.short_mask = (uint32_t)(h.short_tab.size() / SPL_SHORT_BUCKET) - 1;
    d.tiny_tab = h.tiny_tab.data(); d.tiny_mask = (uint32_t)((h.tiny_tab.size() - 4) / SPL_TINY_WORDS) - 1;
    d.t8_tab = h.t8_tab.data(); d.t8_mask = (uint32_t)((h.t8_tab.size() - 4) / SPL_T8_WORDS) - 1;
    d.long_tab = h.long_tab.data(); d.long_mask = (uint32_t)h.long_tab.size() - 1; d.key_blob = h.key_blob.data();
    d.byte_id = h.byte_id.data(); d.max_key_len = h.max_key_len; d.id_limit = h.id_limit;
    d.len_mask = h.len_mask.data(); d.tiny_free = h.tiny_free; d.t8_free = h.t8_free;
    d.pfx = h.pfx.data(); d.filt4 = h.filt4.data(); d.filt4_shift = h.filt4_shift;
    return s;
}
void ms_destroy(void* p) { delete (Sim*)p; }

// the plan for a memo of 2^bits (and 2^long_bits; 0: none) entries.  out: keys placed, keys left out, records in the first list, in the second
void ms_plan(void* p, uint32_t bits, uint32_t long_bits, uint64_t* out) {
    Sim* s = (Sim*)p;
    memo_seed_plan(s->ht, bits, long_bits, s->plan);
    out[0] = s->plan.placed; out[1] = s->plan.left_out; out[2] = s->plan.list.size() / 10; out[3] = s->plan.list2.size() / 18;
}
// the records of the last plan (10 words each; long: 18), and for each its two candidate slots as memo_probe computes them, and what the
// whole-chunk probe of the vocabulary's tables answers for its key
void ms_records(void* p, int lng, uint32_t mask, uint32_t* recs, uint32_t* first, uint32_t* second, uint32_t* probed) {
    Sim* s = (Sim*)p;
    const std::vector<uint32_t>& l = lng ? s->plan.list2 : s->plan.list;
    const size_t rw = lng ? 18 : 10, n = l.size() / rw;
    memcpy(recs, l.data(), l.size() * 4);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = l.data() + i * rw;
        const uint32_t len = r[1] >> 24;
        uint32_t h;
        if (lng) { uint32_t k[16]; memcpy(k, r + 2, sizeof k); h = hash_memo_w<16>(k, len); }
        else { uint32_t k[8]; memcpy(k, r + 2, sizeof k); h = hash_memo_w<8>(k, len); }
        first[i] = h & mask;
        second[i] = memo_slot2(h, mask);
        probed[i] = probe_chunk(s->dt, KeyAcc{r + 2, lng ? 16 : 8}, 0, (int)len);
    }
}
// the decoder's side of the vocabulary (built from the id -> bytes map, not from the seed list): tokens of max_id + 1 ids
uint32_t ms_n_ids(void* p) { return ((Sim*)p)->ht.max_id + 1; }
uint32_t ms_token_bytes_total(void* p) { return (uint32_t)((Sim*)p)->ht.tok_bytes.size(); }
void ms_tokens(void* p, uint32_t* off, uint8_t* bytes, uint8_t* present) {
    Sim* s = (Sim*)p;
    memcpy(off, s->ht.tok_off.data(), s->ht.tok_off.size() * 4);
    if (!s->ht.tok_bytes.empty()) memcpy(bytes, s->ht.tok_bytes.data(), s->ht.tok_bytes.size());
    memcpy(present, s->ht.tok_present.data(), s->ht.tok_present.size());
}

}  // extern "C"
