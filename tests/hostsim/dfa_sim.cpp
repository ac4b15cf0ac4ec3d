// dfa_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_dfa.h (the code k_dfa_index, k_dfa_some and k_dfa_step run: the walk
// with its DEAD rule, the index build with a lane per id and a ballot per state, the OR over a row, the load of a state word, the serial
// step, the row copy with the END bits, the state packing) evaluated on the CPU with HlHostWave.  The lanes of the wavefront are a
// parameter, so the index build also runs with the 64 ids of a wavefront taken in turns and the states in batches of a few.  The id ->
// rank table comes from hl_build, the function the library uploads from.  The wavefront's registers are guarded by canaries, the outputs
// arrive poisoned, and every store is counted per index word, some byte, state word, mask word and live byte (a 16-byte store counts its
// four words, and its address is checked).
// Built with g++; no GPU.  -DSPL_DFA_MUTANT_FIRST (a walk that tests only the first byte for DEAD) and -DSPL_DFA_MUTANT_END (END allowed
// without accept[q]) build the two mutants tests/test_dfa_cpu.py must see fail.  -DDFA_SIM_MAIN adds a main() that runs a small
// self-check (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_dfa.h"

using namespace spl;

namespace {

const uint32_t WCANARY = 0xEEEEEEEEu;

struct SimOut {
    uint64_t* so; uint8_t* sw; uint8_t* lv; uint8_t* lw; uint32_t* mask; uint8_t* mw; uint32_t n_words; uint64_t* bad;
    void state(uint64_t b, uint64_t v) const { so[b] = v; sw[b]++; }
    void alive(uint64_t b, uint32_t v) const { if (lv) { lv[b] = (uint8_t)v; lw[b]++; } }
    void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; mw[b * n_words + k]++; }
    void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        if ((b * n_words + k) % 4 || k + 4 > n_words) { (*bad)++; return; }        // (the sim's mask base stands for a 16-byte aligned one)
        for (uint32_t j = 0; j < 4; j++) put(b, k + j, v[j]);
    }
};

DfTab tab_of(const uint8_t* table, uint32_t n_states) {
    return DfTab{reinterpret_cast<const uint16_t*>(table), table + (size_t)n_states * 512, n_states};
}

}  // namespace

extern "C" {

void df_geometry(uint32_t out[8]) {
    out[0] = DF_DEAD; out[1] = DF_MAX_STATES; out[2] = DF_STATE_WORDS; out[3] = DF_MAX_END; out[4] = DF_WAVE; out[5] = DF_INDEX_STATES;
    out[6] = DF_KEEP_FREE; out[7] = DF_I64;
}

// the grid of k_dfa_index and k_dfa_some: every wavefront of 64 ids below 32 * stride, every block of s_block states; then a wavefront a state
int df_index_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const uint8_t* table, uint32_t n_states,
                 uint32_t n_words, uint32_t lanes, uint32_t s_block, uint32_t* rows, uint8_t* rows_w, uint8_t* some, uint8_t* some_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !s_block || !n_states || n_states > DF_MAX_STATES) return -1;
    std::vector<uint32_t> sorted, rank, parent;
    if (!hl_build(tok_off, tok_bytes, present, max_id, sorted, rank, parent)) return -2;
    if ((uint64_t)n_words * 32 < (uint64_t)max_id + 1) return -3;
    const HlTab t{tok_off, tok_bytes, max_id, sorted.data(), rank.data(), parent.data(), (uint32_t)sorted.size()};
    const DfTab d = tab_of(table, n_states);
    const uint32_t stride = df_stride(n_words);
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY);
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    uint64_t bad = 0;
    for (uint64_t id0 = 0; id0 < (uint64_t)stride * 32 + 64; id0 += 64)            // (one wavefront past the end, as a grid rounded up has)
        for (uint32_t s0 = 0; s0 < n_states; s0 += s_block)
            df_index_wave(w, t, d, id0, s0, s0 + s_block < n_states ? s0 + s_block : n_states, stride, [&](uint32_t q, uint32_t k, uint32_t v) {
                if (q >= n_states || k >= stride) { bad++; return; }
                rows[(size_t)q * stride + k] = v; rows_w[(size_t)q * stride + k]++;
            });
    for (uint32_t q = 0; q < n_states; q++)
        df_some_wave(w, rows, stride, q, [&](uint32_t s, uint32_t v) { if (s >= n_states) { bad++; return; } some[s] = (uint8_t)v; some_w[s]++; });
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    stats[1] = sorted.size();
    return 0;
}

int df_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const void* ids, const int32_t* len,
           uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t v4, uint32_t n_end, const uint32_t* end_ids,
           const uint8_t* table, uint32_t n_states, const uint32_t* rows, const uint8_t* some, uint32_t lanes, const uint64_t* state_in,
           uint64_t* state_out, uint8_t* state_w, uint32_t* mask, uint8_t* mask_w, uint8_t* live, uint8_t* live_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_end || n_end > DF_MAX_END || !n_states || n_states > DF_MAX_STATES) return -1;
    if (v4 && n_words % 4) return -1;
    std::vector<uint32_t> sorted, rank, parent;
    if (!hl_build(tok_off, tok_bytes, present, max_id, sorted, rank, parent)) return -2;
    if ((uint64_t)n_words * 32 < (uint64_t)max_id + 1) return -3;
    const HlTab t{tok_off, tok_bytes, max_id, sorted.data(), rank.data(), parent.data(), (uint32_t)sorted.size()};
    const DfTab d = tab_of(table, n_states);
    // (the 16-byte loads of a row need an aligned copy of the index: numpy's buffers are, this one is made so)
    const uint32_t stride = df_stride(n_words);
    std::vector<uint32_t> copy((size_t)n_states * stride + 8);
    uint32_t* base = copy.data();
    while (reinterpret_cast<uintptr_t>(base) % 16) base++;
    memcpy(base, rows, (size_t)n_states * stride * 4);
    const DfIndex x{base, some, stride};
    DfIn a{};
    a.ids = ids; a.len = len; a.state_in = state_in; a.n_seqs = n_seqs; a.row_len = row_len; a.flags = flags;
    a.n_words = n_words; a.v4 = v4; a.n_end = n_end;
    for (uint32_t i = 0; i < n_end; i++) a.end_ids[i] = end_ids[i];
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY);
    uint64_t bad = 0;
    const SimOut out{state_out, state_w, live, live_w, mask, mask_w, n_words, &bad};
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    for (uint64_t b = 0; b < n_seqs; b++) df_seq(w, t, d, x, a, b, out);
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    stats[1] = sorted.size();
    return 0;
}

}  // extern "C"

#ifdef DFA_SIM_MAIN
// a, ab, b, c over the automaton of "a|ab" (0 -a-> 1 (accepts) -b-> 2 (accepts)), with transitions that are no states where a builder
// writes DEAD: the index rows are {a, ab}, {b}, {}; the first mask is a, ab; behind "a": b and END; behind "ab": END; END ends it
int main() {
    const char* toks[] = {"a", "ab", "b", "c"};
    std::vector<uint32_t> off{0};
    std::vector<uint8_t> bytes, present;
    for (const char* s : toks) { bytes.insert(bytes.end(), s, s + strlen(s)); off.push_back((uint32_t)bytes.size()); present.push_back(1); }
    bytes.push_back(0);
    const uint32_t S = 3, end_id = 9;
    std::vector<uint16_t> trans(S * 256 + (S + 1) / 2, 0xFFFF);
    for (uint32_t i = 0; i < S * 256; i++) trans[i] = (uint16_t)(S + i % 5);      // no state: DEAD on load
    trans[0 * 256 + 'a'] = 1; trans[1 * 256 + 'b'] = 2;
    uint8_t* table = reinterpret_cast<uint8_t*>(trans.data());
    table[S * 512 + 0] = 0; table[S * 512 + 1] = 1; table[S * 512 + 2] = 1;
    int bad = 0;
    for (uint32_t lanes : {64u, 5u, 2u, 1u}) {
        uint32_t rows[3 * 4]; uint8_t rows_w[3 * 4] = {0}, some[3] = {9, 9, 9}, some_w[3] = {0};
        uint64_t stats[2];
        for (uint32_t& r : rows) r = 0xA5A5A5A5u;
        int rc = df_index_sim(off.data(), bytes.data(), present.data(), 3, table, S, 1, lanes, 2, rows, rows_w, some, some_w, stats);
        const uint32_t want_rows[12] = {3, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0};
        if (rc || stats[0] || memcmp(rows, want_rows, sizeof rows) || some[0] != 1 || some[1] != 1 || some[2] != 0) { bad++; printf("lanes %u: index rc %d\n", lanes, rc); }
        for (int i = 0; i < 12; i++) if (rows_w[i] != 1) { bad++; printf("lanes %u: index word %d stored %u times\n", lanes, i, rows_w[i]); }
        const uint32_t feed[4][2] = {{0, 0}, {0, 1}, {2, 1}, {end_id, 1}};          // no ids | a | b | END
        const uint32_t want_mask[4] = {3u, 4u | 1u << end_id, 1u << end_id, 0xFFFFFFFFu};
        const uint64_t want[4] = {0 | DF_CON, 1 | DF_CON, 2 | DF_CON, 2 | DF_DONE};
        uint64_t st = 0 | DF_CON;
        for (int k = 0; k < 4; k++) {
            uint64_t so = ~0ull;
            uint8_t sw = 0, mw = 0, live = 9, lw = 0;
            uint32_t mask = 0xA5A5A5A5u;
            rc = df_sim(off.data(), bytes.data(), present.data(), 3, &feed[k][0], nullptr, 1, feed[k][1], 0, 1, 0, 1, &end_id, table, S, rows, some, lanes,
                        &st, &so, &sw, &mask, &mw, &live, &lw, stats);
            if (rc || mask != want_mask[k] || mw != 1 || sw != 1 || lw != 1 || stats[0] || so != want[k] || live != (k < 3 ? 1 : 0)) {
                bad++;
                printf("lanes %u k %d: rc %d mask %x state %llx\n", lanes, k, rc, mask, (unsigned long long)so);
            }
            st = so;
        }
    }
    printf(bad ? "dfa_sim: FAILED\n" : "dfa_sim: ok\n");
    return bad;
}
#endif
