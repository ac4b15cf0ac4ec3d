// utf8mask_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_utf8mask.h (the code k_utf8_table / k_utf8_mask run: the
// automaton, the class of a state word, a token's eight runs, an id's entry, the ballots turned into the table's words, the row gather)
// evaluated on the CPU with spl_k_heal.h's HlHostWave.  The grids of both kernels are walked workgroup by workgroup and lane by lane; the
// table and the mask arrive poisoned, every store is counted per word and per live byte, the wavefront's registers are guarded by canaries.
// Built with g++; no GPU.  -DUTF8MASK_SIM_MAIN adds a main() that runs a small self-check (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_utf8mask.h"

using namespace spl;

namespace {
const uint32_t WCANARY = 0xEEEEEEEEu;
}

extern "C" {

uint32_t um_sim_step(uint32_t s, uint32_t x) { return um_step(s, x); }
uint32_t um_sim_class(uint64_t word) { return um_class(word); }
uint32_t um_sim_token_classes(const uint8_t* b, uint32_t n) { return um_token_classes(b, n); }
void um_geometry(uint32_t out[4]) { out[0] = UM_ROWS; out[1] = UM_WAVE; out[2] = UM_NT; out[3] = UM_HEAD; }

// the table: rows [UM_ROWS, stride] and the count of stores per word.  present: one BIT per id of the dense table.
int um_sim_table(const uint32_t* tok_off, const uint8_t* tok_bytes, uint32_t max_id, const uint32_t* sp_ids, const uint32_t* sp_off, uint32_t n_sp,
                 const uint32_t* sp_bits, const uint32_t* present, uint32_t stride, uint32_t* rows, uint8_t* rows_w, uint64_t* stats) {
    if (stride == 0 || stride % 4) return -1;
    const DecTab t{tok_off, tok_bytes, max_id, sp_ids, sp_off, n_sp, sp_bits};
    std::vector<uint32_t> regs(HL_WAVE * HL_REGS + 2, WCANARY);
    HlHostWave w{UM_WAVE, {nullptr, nullptr}, regs.data() + 1, nullptr};
    const uint32_t waves = stride / 2, per = UM_NT / UM_WAVE, wgs = (waves + per - 1) / per;
    for (uint32_t g = 0; g < wgs; g++)
        for (uint32_t wv = 0; wv < per; wv++) {
            const uint64_t id0 = ((uint64_t)g * per + wv) * UM_WAVE;
            um_table_wave(w, t, present, id0, stride, [&](uint32_t r, uint32_t k, uint32_t v) {
                rows[(uint64_t)r * stride + k] = v; rows_w[(uint64_t)r * stride + k]++;
            });
        }
    stats[0] = (regs.front() != WCANARY) + (regs.back() != WCANARY);
    return 0;
}

// a step over a table: k_utf8_mask's grid, a lane per word (per == 1) or per four words (per == 4: n_words a multiple of four)
int um_sim_mask(const uint32_t* rows, uint32_t stride, const uint64_t* state, uint64_t n_seqs, uint32_t skip, uint32_t flags, uint32_t n_words,
                uint32_t per, uint32_t* mask, uint8_t* mask_w, uint8_t* mask_r, uint8_t* live, uint8_t* live_w) {
    if ((per != 1 && per != 4) || (per == 4 && n_words % 4)) return -1;
    const UmTab t{rows, stride};
    const uint32_t per_wg = UM_NT * per, wgs = (n_words + per_wg - 1) / per_wg;
    for (uint64_t b = 0; b < n_seqs; b++)
        for (uint32_t g = 0; g < wgs; g++)
            for (uint32_t l = 0; l < UM_NT; l++) {
                const uint32_t k0 = (g * UM_NT + l) * per;
                if (k0 >= n_words) continue;
                um_row_words(t, state, b, skip != 0, flags, k0, per, n_words,
                             [&](uint64_t s, uint32_t k) { mask_r[s * n_words + k]++; return mask[s * n_words + k]; },
                             [&](uint64_t s, uint32_t k, uint32_t v) { mask[s * n_words + k] = v; mask_w[s * n_words + k]++; },
                             [&](uint64_t s, uint32_t v) { if (live) { live[s] = (uint8_t)v; live_w[s]++; } });
            }
    return 0;
}

}  // extern "C"

#ifdef UTF8MASK_SIM_MAIN
// ids 0 "a", 1 C3, 2 A9, 3 "é", 4 E2 82, 5 AC: behind the pending C3 only A9 and AC may follow
int main() {
    const uint8_t bytes[] = {'a', 0xC3, 0xA9, 0xC3, 0xA9, 0xE2, 0x82, 0xAC, 0};
    const uint32_t off[] = {0, 1, 2, 3, 5, 7, 8}, present[] = {0x3Fu}, sp_bits[] = {0u}, none[] = {0u, 0u};
    std::vector<uint32_t> rows(UM_ROWS * 4, 0xA5A5A5A5u);
    std::vector<uint8_t> rows_w(UM_ROWS * 4, 0);
    uint64_t stats[1] = {0};
    int bad = um_sim_table(off, bytes, 5, none, none, 0, sp_bits, present, 4, rows.data(), rows_w.data(), stats) != 0 || stats[0] != 0;
    for (uint8_t c : rows_w) bad += c != 1;
    const uint64_t state[3] = {0, 0xC3ull | (1ull << 24), 1ull << 26};
    uint32_t mask[3] = {7, 7, 7};
    uint8_t mask_w[3] = {0, 0, 0}, mask_r[3] = {0, 0, 0}, live[3] = {9, 9, 9}, live_w[3] = {0, 0, 0};
    bad += um_sim_mask(rows.data(), 4, state, 3, 0, 0, 1, 1, mask, mask_w, mask_r, live, live_w) != 0;
    bad += mask[0] != 0x1Bu || mask[1] != 0x24u || mask[2] != 0xFFFFFFFFu || live[0] != 1 || live[1] != 1 || live[2] != 0;
    printf(bad ? "utf8mask_sim: FAILED %x %x %x\n" : "utf8mask_sim: ok\n", mask[0], mask[1], mask[2]);
    return bad;
}
#endif
