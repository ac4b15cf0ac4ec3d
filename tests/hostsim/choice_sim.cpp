// choice_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_choice.h (the code k_choice runs: the load of a state row, the
// step with a slot per lane, the grouped search for pred', the chain walk that ORs ids into a piece of the row in LDS, the END ids, the
// streamed stores, the state packing) evaluated on the CPU with HlHostWave.  The lanes of the wavefront are a parameter, so the grouped
// search also runs with a few lanes a group, as a plain binary search, and with the slots taken in batches; the piece is a parameter, so a
// toy vocabulary's row is built in several pieces.  The tables come from hl_build, the function the library uploads from.  The wavefront's
// registers and its LDS piece are guarded by canaries, the outputs arrive poisoned, and every store is counted per state word, mask word
// and live byte (a 16-byte store counts its four words, and its address is checked).
// Built with g++; no GPU.  -DSPL_CHOICE_MUTANT_LCP (the chain without the lcp bound) and -DSPL_CHOICE_MUTANT_EQ (|b(t)| < |r_s| in place
// of <=) build the two mutants tests/test_choice_cpu.py must see fail.  -DCHOICE_SIM_MAIN adds a main() that runs a small self-check (for
// a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_choice.h"

using namespace spl;

namespace {

const uint32_t WCANARY = 0xEEEEEEEEu;

struct SimOut {
    uint64_t* so; uint8_t* sw; uint8_t* lv; uint8_t* lw; uint32_t* mask; uint8_t* mw; uint32_t n_words; uint64_t* bad;
    void state(uint64_t b, uint32_t i, uint64_t v) const { so[b * CH_STATE_WORDS + i] = v; sw[b * CH_STATE_WORDS + i]++; }
    void alive(uint64_t b, uint32_t v) const { if (lv) { lv[b] = (uint8_t)v; lw[b]++; } }
    void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; mw[b * n_words + k]++; }
    void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        if ((b * n_words + k) % 4 || k + 4 > n_words) { (*bad)++; return; }        // (the sim's mask base stands for a 16-byte aligned one)
        for (uint32_t j = 0; j < 4; j++) put(b, k + j, v[j]);
    }
};

}  // namespace

extern "C" {

void ch_geometry(uint32_t out[8]) {
    out[0] = CH_SLOTS; out[1] = CH_MAX_LEN; out[2] = CH_TABLE_BYTES; out[3] = CH_STATE_WORDS; out[4] = CH_MAX_END; out[5] = CH_PIECE;
    out[6] = CH_WAVE; out[7] = HL_REGS;
}

int ch_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const void* ids, const int32_t* len,
           uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t piece, uint32_t v4, uint32_t n_end,
           const uint32_t* end_ids, const uint8_t* table, uint32_t lanes, const uint64_t* state_in, uint64_t* state_out, uint8_t* state_w,
           uint32_t* mask, uint8_t* mask_w, uint8_t* live, uint8_t* live_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || piece < 4 || piece > CH_PIECE || piece % 4 || n_end > CH_MAX_END) return -1;
    if (v4 && n_words % 4) return -1;
    std::vector<uint32_t> sorted, rank, parent;
    if (!hl_build(tok_off, tok_bytes, present, max_id, sorted, rank, parent)) return -2;
    if ((uint64_t)n_words * 32 < (uint64_t)max_id + 1) return -3;
    const HlTab t{tok_off, tok_bytes, max_id, sorted.data(), rank.data(), parent.data(), (uint32_t)sorted.size()};
    ChIn a{};
    a.ids = ids; a.len = len; a.state_in = state_in; a.table = table; a.n_seqs = n_seqs; a.row_len = row_len; a.flags = flags;
    a.n_words = n_words; a.piece = piece; a.v4 = v4; a.n_end = n_end;
    for (uint32_t i = 0; i < n_end; i++) a.end_ids[i] = end_ids[i];
    const uint32_t lds_n = n_words < piece ? n_words : piece;
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY), lds((size_t)lds_n + 2, WCANARY);
    uint64_t bad = 0;
    const SimOut out{state_out, state_w, live, live_w, mask, mask_w, n_words, &bad};
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, lds.data() + 1};
    for (uint64_t b = 0; b < n_seqs; b++) ch_seq(w, t, a, b, out);
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY) + (lds.front() != WCANARY) + (lds.back() != WCANARY);
    stats[1] = sorted.size();
    return 0;
}

}  // extern "C"

#ifdef CHOICE_SIM_MAIN
// y, ye, yes, n, no, s over the choices "yes" and "no": the first row allows y, ye, yes, n, no; behind "ye" only "s" (the remainder starts
// with nothing else); behind "yes" only the END id; the END id then ends the sequence with hit 0 and its row is ones
int main() {
    const char* toks[] = {"y", "ye", "yes", "n", "no", "s"};
    std::vector<uint32_t> off{0};
    std::vector<uint8_t> bytes, present;
    for (const char* s : toks) { bytes.insert(bytes.end(), s, s + strlen(s)); off.push_back((uint32_t)bytes.size()); present.push_back(1); }
    bytes.push_back(0);
    std::vector<uint8_t> table(CH_TABLE_BYTES, 0);
    memcpy(&table[0], "yes", 3); table[CH_SLOTS * CH_MAX_LEN] = 3;
    memcpy(&table[CH_MAX_LEN], "no", 2); table[CH_SLOTS * CH_MAX_LEN + 1] = 2;
    const uint32_t end_id = 9;
    int bad = 0;
    for (uint32_t lanes : {64u, 5u, 2u, 1u})
        for (uint32_t piece : {4u, CH_PIECE}) {
            // no ids: the first row; then "ye"; then "s"; then END
            const uint32_t feed[4][2] = {{0, 0}, {1, 1}, {5, 1}, {end_id, 1}};
            const uint32_t want_mask[4] = {0x1Fu, 0x20u, 1u << end_id, 0xFFFFFFFFu};
            const uint64_t want0[4] = {3, 1, 1, 0}, want1[4] = {0, 2, 3, 3 | CH_DONE};
            uint64_t st[2] = {3, 0};
            for (int k = 0; k < 4; k++) {
                uint64_t so[2] = {~0ull, ~0ull}, stats[2];
                uint8_t sw[2] = {0, 0}, mw[1] = {0}, live = 9, lw = 0;
                uint32_t mask[1] = {0xA5A5A5A5u};
                const int rc = ch_sim(off.data(), bytes.data(), present.data(), 5, &feed[k][0], nullptr, 1, feed[k][1], 0, 1, piece, 0, 1, &end_id,
                                      table.data(), lanes, st, so, sw, mask, mw, &live, &lw, stats);
                if (rc || mask[0] != want_mask[k] || mw[0] != 1 || sw[0] != 1 || sw[1] != 1 || lw != 1 || stats[0] || so[0] != want0[k] || so[1] != want1[k] ||
                    live != (want0[k] ? 1 : 0)) {
                    bad++;
                    printf("lanes %u piece %u k %d: rc %d mask %x state %llx %llx\n", lanes, piece, k, rc, mask[0], (unsigned long long)so[0], (unsigned long long)so[1]);
                }
                st[0] = so[0]; st[1] = so[1];
            }
        }
    printf(bad ? "choice_sim: FAILED\n" : "choice_sim: ok\n");
    return bad;
}
#endif
