// nest_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_nest.h (the code k_nest_index, k_nest_count, k_nest_write and
// k_nest_step run: the walk over configurations with push and pop, the index build with two ballots per state, the count and the
// ascending write of the dependent ids, the load of a state row, the serial step, the dependent pass with a private stack per lane, the
// piecewise row write with its overlay, the state packing) evaluated on the CPU with HlHostWave.  The lanes of the wavefront are a
// parameter.  The exclusive scan over the per-state counts between count and write is a plain loop here (k_nest_scan is device code).
// The wavefront's registers and the overlay are guarded by canaries, the outputs arrive poisoned, and every store is counted per index
// word, dep entry, some byte, state word, mask word and live byte (a 16-byte store counts its four words, and its address is checked).
// Built with g++; no GPU.  -DSPL_NEST_MUTANT_POP (a pop that ignores the symbol and takes ret[v][0]), -DSPL_NEST_MUTANT_END (END allowed
// at non-zero depth) and -DSPL_NEST_MUTANT_DEP (a dependent id tested against an empty stack) build the three mutants
// tests/test_nest_cpu.py must see fail.  -DNEST_SIM_MAIN adds a main() that runs a small self-check (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_nest.h"

using namespace spl;

namespace {

const uint32_t WCANARY = 0xEEEEEEEEu;

struct SimOut {
    uint64_t* so; uint8_t* sw; uint8_t* lv; uint8_t* lw; uint32_t* mask; uint8_t* mw; uint32_t n_words; uint64_t* bad;
    void state(uint64_t b, uint32_t i, uint64_t v) const { so[b * NS_STATE_WORDS + i] = v; sw[b * NS_STATE_WORDS + i]++; }
    void alive(uint64_t b, uint32_t v) const { if (lv) { lv[b] = (uint8_t)v; lw[b]++; } }
    void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; mw[b * n_words + k]++; }
    void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        if ((b * n_words + k) % 4 || k + 4 > n_words) { (*bad)++; return; }        // (the sim's mask base stands for a 16-byte aligned one)
        for (uint32_t j = 0; j < 4; j++) put(b, k + j, v[j]);
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

}  // namespace

extern "C" {

void ns_geometry(uint32_t out[8]) {
    out[0] = NS_MAX_DEPTH; out[1] = NS_STATE_WORDS; out[2] = NS_MAX_RET; out[3] = NS_PUSH; out[4] = NS_POP; out[5] = NS_PIECE;
    out[6] = DF_MAX_STATES; out[7] = DF_MAX_END;
}

// the launches of spl_nest_index_device: the index grid, a wavefront a state for the counts, the scan, a wavefront a state for the ids.
// Returns -4 where the dependent entries do not fit dep_cap (stats[2] holds their number; no entry is written then).
int ns_index_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const uint8_t* table, uint32_t n_states,
                 uint32_t n_ret, uint32_t n_words, uint32_t lanes, uint32_t s_block, uint32_t dep_cap, uint32_t* rows, uint8_t* rows_w, uint32_t* dep_off,
                 uint8_t* dep_off_w, uint32_t* dep_ids, uint8_t* dep_w, uint8_t* some, uint8_t* some_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !s_block || !n_states || n_states > DF_MAX_STATES || n_ret > NS_MAX_RET) return -1;
    Vocab v;
    if (int rc = v.build(tok_off, tok_bytes, present, max_id, n_words)) return rc;
    const NsTab d = ns_tab(table, n_states, n_ret);
    const uint32_t stride = df_stride(n_words);
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY), touch((size_t)n_states * stride, 0x5A5A5A5Au), cnt(n_states, 0);
    std::vector<uint8_t> touch_w((size_t)n_states * stride, 0);
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, nullptr};
    uint64_t bad = 0;
    for (uint64_t id0 = 0; id0 < (uint64_t)stride * 32 + 64; id0 += 64)            // (one wavefront past the end, as a grid rounded up has)
        for (uint32_t s0 = 0; s0 < n_states; s0 += s_block)
            ns_index_wave(w, v.t, d, id0, s0, s0 + s_block < n_states ? s0 + s_block : n_states, stride,
                [&](uint32_t q, uint32_t k, uint32_t x) {
                    if (q >= n_states || k >= stride) { bad++; return; }
                    rows[(size_t)q * stride + k] = x; rows_w[(size_t)q * stride + k]++;
                },
                [&](uint32_t q, uint32_t k, uint32_t x) {
                    if (q >= n_states || k >= stride) { bad++; return; }
                    touch[(size_t)q * stride + k] = x; touch_w[(size_t)q * stride + k]++;
                });
    for (uint8_t c : touch_w) bad += c != 1;
    for (uint32_t q = 0; q < n_states; q++)
        ns_count_wave(w, rows, touch.data(), stride, q, [&](uint32_t s, uint32_t x, uint32_t n) {
            if (s >= n_states) { bad++; return; }
            some[s] = (uint8_t)x; some_w[s]++; cnt[s] = n;
        });
    uint32_t total = 0;
    for (uint32_t q = 0; q < n_states; q++) { dep_off[q] = total; dep_off_w[q]++; total += cnt[q]; }
    dep_off[n_states] = total; dep_off_w[n_states]++;
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    stats[1] = v.sorted.size();
    stats[2] = total;
    if (total > dep_cap) return -4;
    for (uint32_t q = 0; q < n_states; q++)
        ns_write_wave(w, touch.data(), stride, q, dep_off[q], dep_off[q + 1] < dep_cap ? dep_off[q + 1] : dep_cap, [&](uint32_t pos, uint32_t id) {
            if (pos >= dep_cap) { bad++; return; }
            dep_ids[pos] = id; dep_w[pos]++;
        });
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY);
    return 0;
}

int ns_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, const void* ids, const int32_t* len,
           uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t n_words, uint32_t v4, uint32_t n_end, const uint32_t* end_ids,
           uint32_t max_depth, const uint8_t* table, uint32_t n_states, uint32_t n_ret, const uint32_t* rows, const uint32_t* dep_off,
           const uint32_t* dep_ids, uint32_t dep_cap, const uint8_t* some, uint32_t lanes, const uint64_t* state_in, uint64_t* state_out,
           uint8_t* state_w, uint32_t* mask, uint8_t* mask_w, uint8_t* live, uint8_t* live_w, uint64_t* stats) {
    if (lanes == 0 || lanes > 64 || !n_end || n_end > DF_MAX_END || !n_states || n_states > DF_MAX_STATES || n_ret > NS_MAX_RET) return -1;
    if (!max_depth || max_depth > NS_MAX_DEPTH) return -1;
    if (v4 && n_words % 4) return -1;
    Vocab v;
    if (int rc = v.build(tok_off, tok_bytes, present, max_id, n_words)) return rc;
    const NsTab d = ns_tab(table, n_states, n_ret);
    // (the 16-byte loads of a row need an aligned copy of the index: numpy's buffers are, this one is made so)
    const uint32_t stride = df_stride(n_words);
    std::vector<uint32_t> copy((size_t)n_states * stride + 8);
    uint32_t* base = copy.data();
    while (reinterpret_cast<uintptr_t>(base) % 16) base++;
    memcpy(base, rows, (size_t)n_states * stride * 4);
    const NsIndex x{base, dep_off, dep_ids, some, stride, dep_cap};
    DfIn a{};
    a.ids = ids; a.len = len; a.state_in = state_in; a.n_seqs = n_seqs; a.row_len = row_len; a.flags = flags;
    a.n_words = n_words; a.v4 = v4; a.n_end = n_end;
    for (uint32_t i = 0; i < n_end; i++) a.end_ids[i] = end_ids[i];
    std::vector<uint32_t> regs((size_t)lanes * HL_REGS + 2, WCANARY), ov(NS_PIECE + 2, WCANARY);
    uint64_t bad = 0;
    const SimOut out{state_out, state_w, live, live_w, mask, mask_w, n_words, &bad};
    HlHostWave w{lanes, {nullptr, nullptr}, regs.data() + 1, ov.data() + 1};
    for (uint64_t b = 0; b < n_seqs; b++) ns_seq(w, v.t, d, x, NsStep{max_depth}, a, b, out);
    stats[0] = bad + (regs.front() != WCANARY) + (regs.back() != WCANARY) + (ov.front() != WCANARY) + (ov.back() != WCANARY);
    stats[1] = v.sorted.size();
    return 0;
}

}  // extern "C"

#ifdef NEST_SIM_MAIN
// a, (, ), )), (), a) over  0 -a-> 0, 0 -(-> 0 push 1, 0 -)-> pop ret[0][1] = 0; state 0 accepts: balanced brackets around a's
int main() {
    const char* toks[] = {"a", "(", ")", "))", "()", "a)"};
    std::vector<uint32_t> off{0};
    std::vector<uint8_t> bytes, present;
    for (const char* s : toks) { bytes.insert(bytes.end(), s, s + strlen(s)); off.push_back((uint32_t)bytes.size()); present.push_back(1); }
    bytes.push_back(0);
    const uint32_t S = 1, R = 1, end_id = 9;
    std::vector<uint16_t> tab16((S * 769 + R * 32 + 1) / 2, 0);
    uint8_t* table = reinterpret_cast<uint8_t*>(tab16.data());
    uint16_t* trans = tab16.data();
    uint16_t* ret = tab16.data() + S * 256;
    uint8_t* op = table + S * 512 + R * 32;
    for (uint32_t i = 0; i < 256; i++) trans[i] = 0xFFFF;
    for (uint32_t i = 0; i < 16; i++) ret[i] = 0xFFFF;
    trans['a'] = 0; trans['('] = 0; op['('] = NS_PUSH | 1; trans[')'] = 0; op[')'] = NS_POP; ret[1] = 0;
    op[256] = 1;                                                               // accept[0]
    int bad = 0;
    const uint32_t want_dep[5] = {1, 2, 3, 4, 5};
    for (uint32_t lanes : {64u, 5u, 3u, 1u}) {
        uint32_t rows[4], dep_off[2] = {7, 7}, dep_ids[6]; uint8_t rows_w[4] = {0}, dow[2] = {0}, dw[6] = {0}, some[1] = {9}, some_w[1] = {0};
        uint64_t stats[3];
        int rc = ns_index_sim(off.data(), bytes.data(), present.data(), 5, table, S, R, 1, lanes, 2, 5, rows, rows_w, dep_off, dow, dep_ids, dw, some, some_w, stats);
        if (rc || stats[0] || rows[0] != 1u || dep_off[1] != 5 || memcmp(dep_ids, want_dep, 20) || some[0] != 1) { bad++; printf("lanes %u: index rc %d\n", lanes, rc); }
        // ( | a) | )) with one level left: dead -> broken
        const uint32_t feed[3] = {1, 5, 3};
        const uint32_t want_mask[3] = {0b110111u, 0b010011u | 1u << end_id, 0xFFFFFFFFu};
        uint64_t st[5] = {0 | DF_CON, 0, 0, 0, 0};
        for (int k = 0; k < 3; k++) {
            uint64_t so[5]; uint8_t sw[5] = {0}, mw = 0, live = 9, lw = 0; uint32_t mask = 0xA5A5A5A5u;
            rc = ns_sim(off.data(), bytes.data(), present.data(), 5, &feed[k], nullptr, 1, 1, 0, 1, 0, 1, &end_id, 2, table, S, R, rows, dep_off, dep_ids, 5, some,
                        lanes, st, so, sw, &mask, &mw, &live, &lw, stats);
            if (rc || stats[0] || mask != want_mask[k] || mw != 1 || lw != 1) { bad++; printf("lanes %u k %d: rc %d mask %x state %llx\n", lanes, k, rc, mask, (unsigned long long)so[0]); }
            memcpy(st, so, sizeof st);
        }
    }
    printf(bad ? "nest_sim: FAILED\n" : "nest_sim: ok\n");
    return bad;
}
#endif
