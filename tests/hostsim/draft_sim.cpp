// draft_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_draft.h (the code k_dfa_draft and k_nest_draft run: the climb
// through the parents into one 64-bit word, the walk of a path in ascending order, ok, and -- unchanged -- the step's settle and row
// write handed an output row) evaluated on the CPU with HlHostWave, one wavefront per (sequence, row) pair as the grid has them.  The
// lanes of the wavefront are a parameter.  The wavefront's registers and the overlay are guarded by canaries, the outputs arrive poisoned,
// and every store is counted per state word, mask word, live byte and ok byte (a 16-byte store counts its four words, and its address is
// checked); live and the state rows may be absent, as in the call.  Built with g++; no GPU.  -DSPL_DRAFT_MUTANT_ORDER (the ancestors
// walked in descending order), -DSPL_DRAFT_MUTANT_OK (ok that ignores a rejected ancestor) and -DSPL_DRAFT_MUTANT_DONE (a child of a node
// that ended the sequence accepted) build the three mutants tests/test_draft_cpu.py must see fail.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_draft.h"

using namespace spl;

namespace {

const uint32_t WCANARY = 0xEEEEEEEEu;

// the outputs over ROWS; W: the words of a state row
template <uint32_t W> struct SimOut {
    uint64_t* so; uint8_t* sw; uint8_t* lv; uint8_t* lw; uint32_t* mask; uint8_t* mw; uint8_t* okp; uint8_t* okw; uint32_t n_words; uint64_t* bad;
    void state(uint64_t row, uint64_t v) const { if (so) { so[row] = v; sw[row]++; } }                                  // (the regex guide's)
    void state(uint64_t row, uint32_t i, uint64_t v) const { if (so) { so[row * W + i] = v; sw[row * W + i]++; } }      // (the nest guide's)
    void alive(uint64_t row, uint32_t v) const { if (lv) { lv[row] = (uint8_t)v; lw[row]++; } }
    void ok(uint64_t at, uint32_t v) const { okp[at] = (uint8_t)v; okw[at]++; }
    void put(uint64_t row, uint32_t k, uint32_t v) const { mask[row * n_words + k] = v; mw[row * n_words + k]++; }
    void put4(uint64_t row, uint32_t k, const uint32_t* v) const {
        if ((row * n_words + k) % 4 || k + 4 > n_words) { (*bad)++; return; }      // (the sim's mask base stands for a 16-byte aligned one)
        for (uint32_t j = 0; j < 4; j++) put(row, k + j, v[j]);
    }
};

struct Vocab {
    std::vector<uint32_t> sorted, rank, parent;
    HlTab t;
    int build(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, uint32_t n_words) {
        if (!hl_build(tok_off, tok_bytes, present, max_id, sorted, rank, parent)) return -2;
        if ((uint64_t)n_words * 32 < (uint64_t)max_id + 1) return -3;
        t = HlTab{tok_off, tok_bytes, max_id, sorted.data(), rank.data(), parent.data(), (uint32_t)sorted.size()};
        return 0;
    }
};

// (the 16-byte loads of a row need an aligned copy of the index: this one is made so)
struct AlignedRows {
    std::vector<uint32_t> copy; uint32_t* base;
    AlignedRows(const uint32_t* rows, size_t n) : copy(n + 8) {
        base = copy.data();
        while (reinterpret_cast<uintptr_t>(base) % 16) base++;
        memcpy(base, rows, n * 4);
    }
};

DfIn make_in(const void* ids, const int32_t* len, const uint64_t* state_in, uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t v4,
             uint32_t n_end, const uint32_t* end_ids) {
    DfIn a{};
    a.ids = ids; a.len = len; a.state_in = state_in; a.n_seqs = n_seqs; a.row_len = row_len; a.flags = flags;
    a.n_words = n_words; a.v4 = v4; a.n_end = n_end;
    for (uint32_t i = 0; i < n_end; i++) a.end_ids[i] = end_ids[i];
    return a;
}

}  // namespace

extern "C" {

void dr_geometry(uint32_t out[2]) { out[0] = DR_MAX_NODES; out[1] = DR_PARENT_PER_SEQ; }

// spl_dfa_draft_device's one launch: rows (1 + row_len) by sequences
int dr_dfa_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const void* ids, const int32_t* len,
               const int32_t* parent, uint32_t per_seq, uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t v4, uint32_t n_end,
               const uint32_t* end_ids, const uint8_t* table, uint32_t n_states, const uint32_t* rows, const uint8_t* some, uint32_t lanes,
               const uint64_t* state_in, uint64_t* state_out, uint8_t* state_w, uint32_t* mask, uint8_t* mask_w, uint8_t* live, uint8_t* live_w, uint8_t* ok,
               uint8_t* ok_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_end || n_end > DF_MAX_END || !n_states || n_states > DF_MAX_STATES || row_len > DR_MAX_NODES) return -1;
    if (v4 && n_words % 4) return -1;
    Vocab v;
    if (int rc = v.build(tok_off, tok_bytes, present, max_id, n_words)) return rc;
    const DfTab d{reinterpret_cast<const uint16_t*>(table), table + (size_t)n_states * 512, n_states};
    const uint32_t stride = df_stride(n_words);
    AlignedRows ar(rows, (size_t)n_states * stride);
    const DfIndex x{ar.base, some, stride};
    const DfIn a = make_in(ids, len, state_in, n_seqs, row_len, flags, n_words, v4, n_end, end_ids);
    const DrIn g{parent, per_seq};
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY);
    uint64_t bad = 0;
    const SimOut<1> out{state_out, state_w, live, live_w, mask, mask_w, ok, ok_w, n_words, &bad};
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    for (uint64_t b = 0; b < n_seqs; b++)
        for (uint32_t r = 0; r <= row_len; r++) dr_dfa_row(w, v.t, d, x, a, g, b, r, out);
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    stats[1] = v.sorted.size();
    return 0;
}

int dr_nest_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const void* ids, const int32_t* len,
                const int32_t* parent, uint32_t per_seq, uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t v4, uint32_t n_end,
                const uint32_t* end_ids, uint32_t max_depth, const uint8_t* table, uint32_t n_states, uint32_t n_ret, const uint32_t* rows,
                const uint32_t* dep_off, const uint32_t* dep_ids, uint32_t dep_cap, const uint8_t* some, uint32_t lanes, const uint64_t* state_in,
                uint64_t* state_out, uint8_t* state_w, uint32_t* mask, uint8_t* mask_w, uint8_t* live, uint8_t* live_w, uint8_t* ok, uint8_t* ok_w,
                uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_end || n_end > DF_MAX_END || !n_states || n_states > DF_MAX_STATES || n_ret > NS_MAX_RET) return -1;
    if (!max_depth || max_depth > NS_MAX_DEPTH || row_len > DR_MAX_NODES) return -1;
    if (v4 && n_words % 4) return -1;
    Vocab v;
    if (int rc = v.build(tok_off, tok_bytes, present, max_id, n_words)) return rc;
    const NsTab d = ns_tab(table, n_states, n_ret);
    const uint32_t stride = df_stride(n_words);
    AlignedRows ar(rows, (size_t)n_states * stride);
    const NsIndex x{ar.base, dep_off, dep_ids, some, stride, dep_cap};
    const DfIn a = make_in(ids, len, state_in, n_seqs, row_len, flags, n_words, v4, n_end, end_ids);
    const DrIn g{parent, per_seq};
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY), ov(NS_PIECE + 2, WCANARY);
    uint64_t bad = 0;
    const SimOut<NS_STATE_WORDS> out{state_out, state_w, live, live_w, mask, mask_w, ok, ok_w, n_words, &bad};
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, ov.data() + 1};
    for (uint64_t b = 0; b < n_seqs; b++)
        for (uint32_t r = 0; r <= row_len; r++) dr_nest_row(w, v.t, d, x, NsStep{max_depth}, a, g, b, r, out);
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY) + (ov.front() != WCANARY) + (ov.back() != WCANARY);
    stats[1] = v.sorted.size();
    return 0;
}

}  // extern "C"
