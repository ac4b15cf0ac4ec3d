// heal_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_heal.h (the code k_heal_plan / k_heal_fill run: table access, the
// byte-string compare, the search with one pivot per lane, the step and begin transitions, the chain of partial ids, the state packing, the
// ballots turned into words) evaluated on the CPU with HlHostWave.  The lanes of the plan's wavefront are a parameter, so the 64-way search
// also runs 5-way, 3-way and as a plain binary search; the fill's wavefront has the hardware's 64 (its ballot is two words).  The tables
// come from hl_build, the function the library uploads from.  The wavefront's buffers and the scratch are guarded by canaries, the outputs
// arrive poisoned, and every store is counted per state word, mask word, live byte and n_back entry.
// Built with g++; no GPU.  -DSPL_HEAL_MUTANT_HI (hi = lo + 1) and -DSPL_HEAL_MUTANT_LCP (the chain without the lcp bound) build the two
// mutants tests/test_heal_cpu.py must see fail.  -DHEAL_SIM_MAIN adds a main() that runs a small self-check (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_heal.h"

using namespace spl;

namespace {

const uint8_t CANARY = 0xEE;
const uint32_t WCANARY = 0xEEEEEEEEu;

struct SimOut {
    uint64_t* so; uint8_t* sw; uint8_t* lv; uint8_t* lw; int32_t* nb; uint8_t* nw; uint32_t* scr;
    void state(uint64_t b, uint32_t i, uint64_t v) const { so[b * HL_STATE_WORDS + i] = v; sw[b * HL_STATE_WORDS + i]++; }
    void alive(uint64_t b, uint32_t v) const { if (lv) { lv[b] = (uint8_t)v; lw[b]++; } }
    void back(uint64_t b, uint32_t v) const { if (nb) { nb[b] = (int32_t)v; nw[b]++; } }
    void plan(uint64_t b, uint32_t i, uint32_t v) const { scr[b * HL_SCR + i] = v; }
};

struct Args {
    const uint32_t* tok_off; const uint8_t* tok_bytes; const uint8_t* present; uint32_t max_id;
    int begin; const void* ids; const int32_t* len; uint64_t n_seqs; uint32_t row_len, flags, max_back, min_keep, n_words, lanes, spw;
    const uint64_t* state_in; uint64_t* state_out; uint8_t* state_w; uint32_t* mask; uint8_t* mask_w; uint8_t* live; uint8_t* live_w;
    int32_t* n_back; uint8_t* nback_w; int32_t* d_n; uint64_t* stats;
};

int run(const Args& x) {
    if (x.lanes == 0 || x.lanes > 64 || x.spw == 0 || x.spw > HL_SPW_MAX) return -1;
    std::vector<uint32_t> sorted, rank, parent;
    if (!hl_build(x.tok_off, x.tok_bytes, x.present, x.max_id, sorted, rank, parent)) return -2;
    if ((uint64_t)x.n_words * 32 < (uint64_t)x.max_id + 1) return -3;
    const HlTab t{x.tok_off, x.tok_bytes, x.max_id, sorted.data(), rank.data(), parent.data(), (uint32_t)sorted.size()};
    HlIn a{};
    a.ids = x.ids; a.len = x.len; a.state_in = x.state_in; a.n_seqs = x.n_seqs; a.row_len = x.row_len; a.flags = x.flags;
    a.max_back = x.begin ? x.max_back : 0; a.min_keep = x.min_keep;
    uint64_t damage = 0;
    // the scratch: poisoned, a canary word on both sides
    std::vector<uint32_t> scr(x.n_seqs * HL_SCR + 2, 0xA5A5A5A5u);
    scr.front() = scr.back() = WCANARY;
    const SimOut out{x.state_out, x.state_w, x.live, x.live_w, x.n_back, x.nback_w, scr.data() + 1};
    {   // the plan: a wavefront of `lanes` lanes per sequence
        std::vector<uint8_t> pb(2 * HL_MAX_P + 2, CANARY);
        HlHostWave w{x.lanes, {pb.data() + 1, pb.data() + 1 + HL_MAX_P}, nullptr, nullptr};
        for (uint64_t b = 0; b < x.n_seqs; b++) hl_plan_seq(w, t, a, x.begin != 0, b, out);
        damage += (pb.front() != CANARY) + (pb.back() != CANARY);
    }
    damage += (scr.front() != WCANARY) + (scr.back() != WCANARY);
    uint64_t max_part = 0;
    for (uint64_t b = 0; b < x.n_seqs; b++)
        if (scr[1 + b * HL_SCR] != HL_NONE) max_part = std::max<uint64_t>(max_part, scr[1 + b * HL_SCR + 2] & 0x7Fu);
    {   // the fill: the grid of k_heal_fill, workgroup by workgroup and wavefront by wavefront
        std::vector<uint32_t> regs(HL_WAVE * HL_REGS + 2, WCANARY), inf(3 * HL_SPW_MAX + 2, WCANARY);
        HlHostWave w{HL_WAVE, {nullptr, nullptr}, regs.data() + 1, inf.data() + 1};
        const uint32_t cols = (x.n_words + HL_WG_WORDS - 1) / HL_WG_WORDS;
        const uint64_t groups = (x.n_seqs + x.spw - 1) / x.spw;
        for (uint64_t g = 0; g < groups; g++)
            for (uint32_t c = 0; c < cols; c++)
                for (uint32_t wv = 0; wv < HL_FILL_NT / HL_WAVE; wv++) {
                    const uint64_t s0 = g * x.spw, s1 = std::min<uint64_t>(s0 + x.spw, x.n_seqs);
                    const uint64_t id0 = (uint64_t)c * HL_WG_IDS + wv * HL_WAVE_IDS;
                    if (id0 >= (uint64_t)x.n_words * 32) continue;
                    hl_fill_wave(w, t, scr.data() + 1, (uint32_t)id0, s0, s1, x.n_words, x.flags, [&](uint64_t s, uint32_t k, uint32_t v) {
                        x.mask[s * x.n_words + k] = v; x.mask_w[s * x.n_words + k]++;
                    });
                }
        damage += (regs.front() != WCANARY) + (regs.back() != WCANARY) + (inf.front() != WCANARY) + (inf.back() != WCANARY);
    }
    if (x.d_n) {
        uint32_t c = 0, k = 0;
        for (uint64_t s = 0; s < x.n_seqs; s++) { c += scr[1 + s * HL_SCR] != HL_NONE; k += (scr[1 + s * HL_SCR + 2] & HL_BROKE) != 0; }
        x.d_n[0] = (int32_t)c; x.d_n[1] = (int32_t)k;
    }
    x.stats[0] = damage; x.stats[1] = max_part; x.stats[2] = sorted.size();
    return 0;
}

}  // namespace

extern "C" {

void hl_geometry(uint32_t out[8]) {
    out[0] = HL_WAVE; out[1] = HL_PER; out[2] = HL_WG_IDS; out[3] = HL_SCR; out[4] = HL_STATE_WORDS; out[5] = HL_MAX_P; out[6] = HL_SPW_MAX;
    out[7] = HL_MAX_PART;
}

uint32_t hl_sim_spw(uint64_t n_seqs, uint32_t n_words) { return hl_spw(n_seqs, n_words); }

int hl_sim(const uint32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* present, uint32_t max_id, int begin, const void* ids,
           const int32_t* len, uint64_t n_seqs, uint32_t row_len, uint32_t flags, uint32_t max_back, uint32_t min_keep, uint32_t n_words,
           uint32_t lanes, uint32_t spw, const uint64_t* state_in, uint64_t* state_out, uint8_t* state_w, uint32_t* mask, uint8_t* mask_w,
           uint8_t* live, uint8_t* live_w, int32_t* n_back, uint8_t* nback_w, int32_t* d_n, uint64_t* stats) {
    return run(Args{tok_off, tok_bytes, present, max_id, begin, ids, len, n_seqs, row_len, flags, max_back, min_keep, n_words, lanes, spw,
                    state_in, state_out, state_w, mask, mask_w, live, live_w, n_back, nback_w, d_n, stats});
}

}  // extern "C"

#ifdef HEAL_SIM_MAIN
// a, aa, aaa, ab, b and P = "aab": covering none, partial a and aa; then the step with "aa" leaves P = "b"
int main() {
    const char* toks[] = {"a", "aa", "aaa", "ab", "b"};
    std::vector<uint32_t> off{0};
    std::vector<uint8_t> bytes, present;
    for (const char* s : toks) { bytes.insert(bytes.end(), s, s + strlen(s)); off.push_back((uint32_t)bytes.size()); present.push_back(1); }
    int bad = 0;
    for (uint32_t lanes : {64u, 5u, 3u, 1u}) {
        uint64_t st_in[HL_STATE_WORDS] = {3, 0, 0, 0, 0, 0, 0, 0, 0}, st_out[HL_STATE_WORDS], stats[3];
        memcpy(&st_in[1], "aab", 3);
        uint8_t st_w[HL_STATE_WORDS] = {0}, mask_w[1] = {0}, live = 9, live_w = 0;
        uint32_t mask[1] = {0xA5A5A5A5u}, id = 1;
        int32_t n[2] = {-1, -1};
        for (int k = 0; k < 2; k++) {
            memset(st_w, 0, sizeof st_w); mask_w[0] = 0; live_w = 0;
            const int rc = hl_sim(off.data(), bytes.data(), present.data(), 4, 0, &id, nullptr, 1, k, 0, 0, 0, 1, lanes, 8, st_in, st_out, st_w, mask,
                                  mask_w, &live, &live_w, nullptr, nullptr, n, stats);
            const uint32_t want = k == 0 ? 0x3u : 0x10u;                       // {a, aa}, then {b}
            if (rc || mask[0] != want || mask_w[0] != 1 || stats[0] || live != 1 || n[0] != 1 || n[1] != 0) { bad++; printf("lanes %u k %d: rc %d mask %x\n", lanes, k, rc, mask[0]); }
        }
    }
    printf(bad ? "heal_sim: FAILED\n" : "heal_sim: ok\n");
    return bad;
}
#endif
