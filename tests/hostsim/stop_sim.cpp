// stop_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_stop.h (the code k_stop_one / k_stop_len / k_stop_write run:
// table access, the backward compare, the tie rule, the hold-back, the chunk walk with its front halo, the state transition, the capacity
// cut) evaluated on the CPU sequence by sequence and lane by lane.  The lanes of a wavefront (the stride of its staging and copy loops) and
// the end positions of a chunk are parameters, so that chunk and step edges can be tested exhaustively at small sizes.  The staging area,
// the tail buffer and the row are arrays guarded by canaries; every write is counted per destination byte, offset, hit and state word.
// Built with g++; no GPU.  -DSPL_STOP_HALO=62 and -DSPL_STOP_MUTANT_SHORTEST build the two mutants tests/test_stop_device_cpu.py must see fail.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_stop.h"
#include "seqscan_sim.h"

using namespace spl;

namespace {

struct Sink {
    uint8_t* out; uint64_t cap; uint8_t* out_writes;
    uint64_t* out_off; uint8_t* off_writes;
    uint64_t* state_out; uint8_t* state_writes;
    int32_t* hit; uint8_t* hit_writes;
    uint64_t canary_damage = 0;
    void put(uint64_t o, uint32_t x) { if (o < cap) { out[o] = (uint8_t)x; out_writes[o]++; } }
};

const uint8_t CANARY = 0xEE;

// the LDS of one wavefront: the row, the tail buffer and the staging area, a canary byte on both sides of each
struct Wave {
    std::vector<uint8_t> rowb, ntb, stg;
    uint32_t chunk;
    explicit Wave(uint32_t chunk_) : rowb(8 * SP_STATE_WORDS + 2, CANARY), ntb(64 + 2, CANARY), stg(chunk_ + SP_H + 2, CANARY), chunk(chunk_) {}
    uint8_t* row() { return rowb.data() + 1; }
    uint8_t* nt() { return ntb.data() + 1; }
    uint8_t* stage() { return stg.data() + 1; }
    uint64_t word(uint32_t i) { uint64_t w; memcpy(&w, row() + 8 * i, 8); return w; }
    uint64_t damage() const {
        return (rowb.front() != CANARY) + (rowb.back() != CANARY) + (ntb.front() != CANARY) + (ntb.back() != CANARY) + (stg.front() != CANARY) +
               (stg.back() != CANARY);
    }
};

SpSeq load_row(const SpIn& a, uint64_t b, Wave& L) {
    memcpy(L.row(), a.state_in + b * SP_STATE_WORDS, 8 * SP_STATE_WORDS);
    return sp_open(a, b, L.word(0), L.word(1));
}

uint64_t live_mask(const uint8_t* tab, uint64_t mask) {
    uint64_t live = 0;
    for (uint32_t lane = 0; lane < 64; lane++)
        if (sp_slot_live(tab, mask, lane)) live |= 1ull << lane;
    return live;
}

// sp_find of the header, restated: chunks of `chunk` end positions, staged `lanes` entries at a time
uint64_t find(const SpIn& a, uint64_t b, uint32_t lanes, Wave& L, uint64_t& cut, uint32_t& info) {
    const SpSeq q = load_row(a, b, L);
    const uint8_t* tab = a.table;
    const uint32_t chunk = L.chunk;
    cut = q.L0 - q.h0; info = 0;
    if (q.idle) return 0;
    const uint8_t* tail = L.row() + 16;
    const uint64_t live = live_mask(tab, q.mask);
    bool found = false;
    for (uint64_t p0 = 0; p0 < q.m && !found; p0 += chunk) {
        const uint64_t base = q.L0 + p0;
        for (uint32_t j0 = 0; j0 < chunk + SP_H; j0 += lanes)
            for (uint32_t j = j0; j < j0 + lanes && j < chunk + SP_H; j++) {
                uint64_t w;
                L.stage()[j] = sp_stage_pos(base, j, q.n, w) ? (uint8_t)sp_w(tail, q.L0, a.in, q.lo, w) : (uint8_t)0;
            }
        for (uint32_t lane = 0; lane < chunk && !found; lane++) {       // (the first lane with a match: the ballot's lowest bit)
            if (!(base + lane < q.n)) break;
            const uint32_t at = SP_H + lane, avail = sp_avail(base, lane);
            uint32_t best_l = 0, best_s = 0;
            for (uint64_t mm = live; mm; mm &= mm - 1) {
                const uint32_t s = (uint32_t)__builtin_ctzll(mm), l = sp_len(tab, s);
                if (!sp_last_eq(L.stage(), at, tab, s, l)) continue;
                if (sp_better(best_l, l) && sp_match(L.stage(), at, avail, tab, s, l)) { best_l = l; best_s = s; }
            }
            if (best_l) {
                cut = sp_cut_hit(a.flags, base + lane + 1, best_l);
                info = sp_info(true, best_s, best_l, 0);
                found = true;
            }
        }
    }
    if (!found) {
        uint32_t h = 0;
        if (!q.fin) {
            const uint32_t tl = sp_new_tail_len(false, false, q.n);
            for (uint32_t lane = 0; lane < tl; lane++) L.nt()[lane] = (uint8_t)sp_w(tail, q.L0, a.in, q.lo, q.n - tl + lane);
            for (uint32_t k = 0; k < 64; k++) {
                bool mine = false;
                for (uint64_t mm = live; mm && !mine; mm &= mm - 1) {
                    const uint32_t s = (uint32_t)__builtin_ctzll(mm), l = sp_len(tab, s);
                    if (sp_hold_first(L.nt(), tl, k, tab, s, l)) mine = sp_hold(L.nt(), tl, k, tab, s, l);
                }
                if (mine) h = k;
            }
        }
        cut = q.n - h;
        info = sp_info(false, 0, 0, h);
    }
    return sp_count(q, cut);
}

// sp_emit of the header, restated
void emit(const SpIn& a, uint64_t b, uint32_t lanes, Wave& L, uint64_t cut, uint32_t info, Sink& k, uint64_t o0) {
    const SpSeq q = load_row(a, b, L);
    uint64_t* row_out = k.state_out + b * SP_STATE_WORDS;
    uint8_t* w_out = k.state_writes + b * SP_STATE_WORDS;
    if (q.idle) {
        for (uint32_t i = 0; i < SP_STATE_WORDS; i++) { row_out[i] = L.word(i); w_out[i]++; }
        k.hit[b] = sp_hit_of(L.word(0)); k.hit_writes[b]++;
        return;
    }
    const uint8_t* tail = L.row() + 16;
    const uint64_t count = sp_count(q, cut), r0 = q.L0 - q.h0;
    for (uint32_t lane = 0; lane < lanes; lane++)
        for (uint64_t i = lane; i < count; i += lanes) k.put(o0 + i, sp_w(tail, q.L0, a.in, q.lo, r0 + i));
    const bool hit = sp_info_hit(info);
    const uint64_t end = hit ? sp_end_hit(a.flags, cut, sp_info_len(info)) : q.n;
    const uint32_t tl = sp_new_tail_len(hit, q.fin, end);
    for (uint32_t lane = 0; lane < 64; lane++) L.nt()[lane] = lane < tl ? (uint8_t)sp_w(tail, q.L0, a.in, q.lo, end - tl + lane) : (uint8_t)0;
    row_out[0] = sp_new_word0(q, info, tl); w_out[0]++;
    k.hit[b] = hit ? (int32_t)sp_info_slot(info) : -1; k.hit_writes[b]++;
    row_out[1] = q.released + count; w_out[1]++;
    for (uint32_t i = 2; i < SP_STATE_WORDS; i++) { memcpy(&row_out[i], L.nt() + 8 * (i - 2), 8); w_out[i]++; }
}

struct Carry { uint64_t cut = 0; uint32_t inf = 0; };

// the driver (seqscan_sim.h) over find and emit
int run(const SpIn& a, uint32_t lanes, uint32_t chunk, int three, Sink& k) {
    Wave L(chunk);
    seqsim::run<Carry>(a.n_seqs, three, k.out_off, k.off_writes,
                       [&](uint64_t b, Carry& c) { return find(a, b, lanes, L, c.cut, c.inf); },
                       [&](uint64_t b, const Carry& c, uint64_t o0) { emit(a, b, lanes, L, c.cut, c.inf, k, o0); });
    k.canary_damage += L.damage();
    return 0;
}

}  // namespace

extern "C" {

void sp_geometry(uint32_t out[8]) {
    out[0] = SP_WAVE; out[1] = SP_H; out[2] = SEQ_BLK; out[3] = SP_ONE_DEFAULT; out[4] = SP_NT; out[5] = SP_ONE_NT; out[6] = SP_ONE_MAX;
    out[7] = SP_TABLE_BYTES;
}

int sp_step(const uint8_t* in, uint64_t in_cap, const uint64_t* in_off, uint64_t n_seqs, const uint8_t* table, const uint64_t* mask,
            const uint8_t* fin, uint32_t flags, const uint64_t* state_in, uint32_t lanes, uint32_t chunk, int three, uint8_t* out, uint64_t cap,
            uint64_t* out_off, uint64_t* state_out, int32_t* hit, uint8_t* out_writes, uint8_t* off_writes, uint8_t* state_writes,
            uint8_t* hit_writes, uint64_t* stats) {
    if (lanes == 0 || chunk == 0) return -1;
    SpIn a{};
    a.in = in; a.in_cap = in_cap; a.in_off = in_off; a.n_seqs = n_seqs; a.table = table; a.mask = mask; a.fin = fin; a.flags = flags;
    a.state_in = state_in;
    Sink k{out, cap, out_writes, out_off, off_writes, state_out, state_writes, hit, hit_writes};
    const int rc = run(a, lanes, chunk, three, k);
    stats[0] = k.canary_damage;
    return rc;
}

}  // extern "C"
