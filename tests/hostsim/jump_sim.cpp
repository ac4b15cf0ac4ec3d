// jump_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_dfa_jump.h (the code k_dfa_force, k_dfa_runs, k_dfa_jump_scatter and
// k_dfa_jump run: the forced byte of a state from ballots over its row, the chain of force words with its cap and its UTF-8 trim, the ids
// CSR laid into rows of 64, and the step -- spl_k_dfa.h's walk, the jump, the settle, the row write) evaluated on the CPU with HlHostWave.
// The lanes of the wavefront are a parameter.  The wavefront's registers are guarded by canaries, the outputs arrive poisoned, and every
// store is counted per force word, run byte, length, id, count, state word, mask word, live byte, emitted id and emitted count.
// Built with g++; no GPU.  -DSPL_DFA_JUMP_MUTANT_ACCEPT (a force that ignores accept[q]) and -DSPL_DFA_JUMP_MUTANT_NOWALK (emission
// without the walk) build the two mutants tests/test_dfa_jump_cpu.py must see fail.  -DJUMP_SIM_MAIN adds a main() that runs a small
// self-check (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_dfa_jump.h"

using namespace spl;

namespace {

const uint32_t WCANARY = 0xEEEEEEEEu;

struct SimOut {
    uint64_t* so; uint8_t* sw; uint8_t* lv; uint8_t* lw; uint32_t* mask; uint8_t* mw; uint32_t n_words; uint64_t* bad;
    int32_t* fi; uint8_t* fiw; int32_t* fl; uint8_t* flw; uint32_t row_len_out; uint64_t n_seqs;
    void state(uint64_t b, uint64_t v) const { so[b] = v; sw[b]++; }
    void alive(uint64_t b, uint32_t v) const { if (lv) { lv[b] = (uint8_t)v; lw[b]++; } }
    void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; mw[b * n_words + k]++; }
    void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        if ((b * n_words + k) % 4 || k + 4 > n_words) { (*bad)++; return; }        // (the sim's mask base stands for a 16-byte aligned one)
        for (uint32_t j = 0; j < 4; j++) put(b, k + j, v[j]);
    }
    void forced(uint64_t b, uint32_t i, uint32_t id) const {
        if (b >= n_seqs || i >= row_len_out) { (*bad)++; return; }
        fi[b * row_len_out + i] = (int32_t)id; fiw[b * row_len_out + i]++;
    }
    void forced_n(uint64_t b, uint32_t m) const { fl[b] = (int32_t)m; flw[b]++; }
};

DfTab tab_of(const uint8_t* table, uint32_t n_states) {
    return DfTab{reinterpret_cast<const uint16_t*>(table), table + (size_t)n_states * 512, n_states};
}

}  // namespace

extern "C" {

void jm_geometry(uint32_t out[4]) {
    out[0] = JM_MAX_BYTES; out[1] = JM_MAX_IDS; out[2] = (uint32_t)jm_index_bytes(1); out[3] = JM_NONE;
}

// the grids of k_dfa_force and k_dfa_runs: a wavefront a state, the second launch behind the whole of the first
int jm_runs_sim(const uint8_t* table, uint32_t n_states, uint32_t lanes, uint32_t* force, uint8_t* force_w, uint8_t* run, uint8_t* run_w,
                uint8_t* run_len, uint8_t* len_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_states || n_states > DF_MAX_STATES) return -1;
    const DfTab d = tab_of(table, n_states);
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY);
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    uint64_t bad = 0;
    for (uint32_t q = 0; q < n_states; q++)
        jm_force_wave(w, d, q, [&](uint32_t s, uint32_t v) { if (s >= n_states) { bad++; return; } force[s] = v; force_w[s]++; });
    for (uint32_t q = 0; q < n_states; q++)
        jm_run_wave(w, force, n_states, q,
                    [&](uint32_t s, uint32_t i, uint32_t x) {
                        if (s >= n_states || i >= JM_MAX_BYTES || x > 255) { bad++; return; }
                        run[(size_t)s * JM_MAX_BYTES + i] = (uint8_t)x; run_w[(size_t)s * JM_MAX_BYTES + i]++;
                    },
                    [&](uint32_t s, uint32_t n) { if (s >= n_states || n > JM_MAX_BYTES) { bad++; return; } run_len[s] = (uint8_t)n; len_w[s]++; });
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    return 0;
}

// the grid of k_dfa_jump_scatter
int jm_scatter_sim(const uint32_t* csr, const uint64_t* off, uint64_t cap, uint32_t n_states, uint32_t lanes, uint32_t* ids, uint8_t* ids_w, uint8_t* n_ids,
                   uint8_t* n_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_states || n_states > DF_MAX_STATES) return -1;
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY);
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    uint64_t bad = 0;
    for (uint32_t q = 0; q < n_states; q++)
        jm_scatter_wave(w, csr, off, cap, q,
                        [&](uint32_t s, uint32_t i, uint32_t v) {
                            if (s >= n_states || i >= JM_MAX_IDS) { bad++; return; }
                            ids[(size_t)s * JM_MAX_IDS + i] = v; ids_w[(size_t)s * JM_MAX_IDS + i]++;
                        },
                        [&](uint32_t s, uint32_t n) { if (s >= n_states || n > JM_MAX_IDS) { bad++; return; } n_ids[s] = (uint8_t)n; n_w[s]++; });
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    return 0;
}

// the grid of k_dfa_jump; jump: a jump index as it lies in memory (jm_index_bytes(n_states) bytes, 4-byte aligned)
int jm_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const void* ids, const int32_t* len,
           uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t v4, uint32_t n_end, const uint32_t* end_ids,
           const uint8_t* table, uint32_t n_states, const uint32_t* rows, const uint8_t* some, uint32_t lanes, const uint64_t* state_in,
           uint64_t* state_out, uint8_t* state_w, uint32_t* mask, uint8_t* mask_w, uint8_t* live, uint8_t* live_w, void* jump, uint32_t row_len_out,
           int32_t* forced, uint8_t* forced_w, int32_t* forced_len, uint8_t* forced_len_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_end || n_end > DF_MAX_END || !n_states || n_states > DF_MAX_STATES) return -1;
    if (v4 && n_words % 4) return -1;
    if (!row_len_out || row_len_out > JM_MAX_IDS) return -1;
    std::vector<uint32_t> sorted, rank, parent;
    if (!hl_build(tok_off, tok_bytes, present, max_id, sorted, rank, parent)) return -2;
    if ((uint64_t)n_words * 32 < (uint64_t)max_id + 1) return -3;
    const HlTab t{tok_off, tok_bytes, max_id, sorted.data(), rank.data(), parent.data(), (uint32_t)sorted.size()};
    const DfTab d = tab_of(table, n_states);
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
    const JmIndex ix = jm_index(jump, n_states);
    const JmStep j{ix.ids, ix.n_ids, row_len_out};
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY);
    uint64_t bad = 0;
    const SimOut out{state_out, state_w, live, live_w, mask, mask_w, n_words, &bad, forced, forced_w, forced_len, forced_len_w, row_len_out, n_seqs};
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    for (uint64_t b = 0; b < n_seqs; b++) jm_seq(w, t, d, x, a, j, b, out);
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    stats[1] = sorted.size();
    return 0;
}

}  // extern "C"

#ifdef JUMP_SIM_MAIN
// a, ab, b, c, abc over the automaton of "abc(a|b)": 0 -a-> 1 -b-> 2 -c-> 3 -a|b-> 4 (accepts).  run(0) = abc, run(1) = bc, run(2) = c,
// nothing is forced at 3 (two bytes) or at 4 (it accepts).  With the index ids[0] = {abc}: the jump from the start state emits abc and
// arrives at 3, whose mask is a | b (not ab: it walks on into nothing).
int main() {
    const char* toks[] = {"a", "ab", "b", "c", "abc"};
    std::vector<uint32_t> off{0};
    std::vector<uint8_t> bytes, present;
    for (const char* s : toks) { bytes.insert(bytes.end(), s, s + strlen(s)); off.push_back((uint32_t)bytes.size()); present.push_back(1); }
    bytes.push_back(0);
    const uint32_t S = 5, end_id = 9;
    std::vector<uint16_t> trans(S * 256 + (S + 1) / 2, 0xFFFF);
    for (uint32_t i = 0; i < S * 256; i++) trans[i] = (uint16_t)(S + i % 5);      // no state: DEAD on load
    trans[0 * 256 + 'a'] = 1; trans[1 * 256 + 'b'] = 2; trans[2 * 256 + 'c'] = 3; trans[3 * 256 + 'a'] = 4; trans[3 * 256 + 'b'] = 4;
    uint8_t* table = reinterpret_cast<uint8_t*>(trans.data());
    for (uint32_t q = 0; q < S; q++) table[S * 512 + q] = q == 4;
    int bad = 0;
    for (uint32_t lanes : {64u, 5u, 2u, 1u}) {
        std::vector<uint32_t> index(jm_index_bytes(S) / 4 + 1, 0xA5A5A5A5u);
        const JmIndex ix = jm_index(index.data(), S);
        std::vector<uint32_t> force(S, 0xA5A5A5A5u);
        std::vector<uint8_t> force_w(S, 0), run_w(S * 64, 0), len_w(S, 0), ids_w(S * 64, 0), n_w(S, 0);
        uint64_t stats[2] = {0, 0};
        int rc = jm_runs_sim(table, S, lanes, force.data(), force_w.data(), ix.run, run_w.data(), ix.run_len, len_w.data(), stats);
        const char* want_run[5] = {"abc", "bc", "c", "", ""};
        for (uint32_t q = 0; q < S; q++)
            if (rc || stats[0] || ix.run_len[q] != strlen(want_run[q]) || memcmp(ix.run + q * 64, want_run[q], strlen(want_run[q])) || force_w[q] != 1 || len_w[q] != 1) {
                bad++; printf("lanes %u: run of state %u\n", lanes, q);
            }
        for (uint32_t i = 0; i < S * 64; i++) if (run_w[i] != 1) { bad++; printf("lanes %u: run byte %u stored %u times\n", lanes, i, run_w[i]); break; }
        const uint32_t csr[3] = {4, 2, 3};                                         // abc | b c | c
        const uint64_t coff[6] = {0, 1, 3, 3, 3, 3};
        rc = jm_scatter_sim(csr, coff, 3, S, lanes, ix.ids, ids_w.data(), ix.n_ids, n_w.data(), stats);
        if (rc || stats[0] || ix.n_ids[0] != 1 || ix.ids[0] != 4 || ix.n_ids[1] != 2 || ix.ids[64] != 2 || ix.ids[65] != 3 || ix.n_ids[2] != 0 || ix.ids[1] != 0) {
            bad++; printf("lanes %u: scatter rc %d\n", lanes, rc);
        }
        const uint32_t rows[5 * 4] = {0x13, 0, 0, 0, 0x4, 0, 0, 0, 0x8, 0, 0, 0, 0x5, 0, 0, 0, 0, 0, 0, 0};
        const uint8_t some[5] = {1, 1, 1, 1, 0};
        const uint64_t st = 0 | DF_CON;
        uint64_t so = ~0ull;
        uint8_t sw = 0, mw = 0, live = 9, lw = 0, fw[4] = {0, 0, 0, 0}, flw = 0;
        uint32_t mask = 0xA5A5A5A5u;
        int32_t forced[4] = {-7, -7, -7, -7}, flen = -7;
        rc = jm_sim(off.data(), bytes.data(), present.data(), 4, nullptr, nullptr, 1, 0, 0, 1, 0, 1, &end_id, table, S, rows, some, lanes, &st, &so, &sw, &mask,
                    &mw, &live, &lw, index.data(), 4, forced, fw, &flen, &flw, stats);
        if (rc || stats[0] || so != (3 | DF_CON) || mask != 0x5u || flen != 1 || forced[0] != 4 || forced[1] != -7 || fw[0] != 1 || fw[1] != 0 || flw != 1 ||
            sw != 1 || mw != 1 || lw != 1 || live != 1) {
            bad++; printf("lanes %u: jump rc %d state %llx mask %x len %d\n", lanes, rc, (unsigned long long)so, mask, flen);
        }
    }
    printf(bad ? "jump_sim: FAILED\n" : "jump_sim: ok\n");
    return bad;
}
#endif
