// spans_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_spans.h (the code k_span_len / k_span_write run) evaluated on
// the CPU block by block and lane by lane, with the kernels' geometry -- DD_PER slots a lane, the in-block running sums and the marks as
// arrays guarded by canaries -- for every span entry and every offset.  The number of lanes of a workgroup is a parameter (a block is
// lanes * DD_PER slots), so that block edges can be tested exhaustively at small sizes.  Every write is counted per destination.
// `mutant` plants one of two mistakes in the driver (tests/test_spans_cpu.py names the cases that must catch each):
//   1  the carry-in is taken from the block's base instead of the document's start      2  the continuation adjustment is dropped
// Built with g++; no GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_spans.h"
#include "gather_sim.h"

using namespace spl;

// a lane's n (0 .. DD_PER) entries from slot i0 on, as sn_store writes them; cnt: writes per slot
template <bool S64>
static void store(uint32_t* out, uint8_t* cnt, uint64_t i0, uint32_t n, const uint32_t* w) {
    constexpr uint32_t W = sn_words(S64);
    for (uint32_t j = 0; j < n; j++) {
        for (uint32_t k = 0; k < W; k++) out[(i0 + j) * W + k] = w[j * W + k];
        cnt[i0 + j]++;
    }
}

// stats: [0] canary damage of the LDS arrays, [1] most rounds of one document search, [2] blocks that computed a carry-in,
//        [3] carry-ins that needed the reduction (the start not on a block's first slot), [4] blocks
template <bool I64, bool S64>
static int run(const DecIn& a, const DecTab& t, const SpanTab& s, uint32_t lanes, int mutant, uint32_t* bspan, uint32_t* cspan, uint64_t* boff,
               uint64_t* coff, uint8_t* bspan_w, uint8_t* cspan_w, uint8_t* boff_w, uint8_t* coff_w, uint64_t* stats) {
    constexpr uint32_t W = sn_words(S64);
    const uint32_t BLK = lanes * DD_PER;
    const uint64_t slots = dd_slots(a), n_blk = dd_n_blocks(slots, BLK), E = dd_end(a);
    std::vector<uint64_t> blk_b(n_blk + 1, 0), blk_c(n_blk + 1, 0);
    // k_span_len
    for (uint64_t b = 0; b < n_blk; b++) {
        const uint64_t base = b * BLK;
        uint64_t sb = 0, sc = 0;
        if (base < E)
            for (uint32_t lane = 0; lane < lanes; lane++) {
                uint32_t len[DD_PER], ent[DD_PER], mb, mc;
                sn_lane<I64>(a, t, s, base + (uint64_t)lane * DD_PER, E, len, ent, mb, mc);
                sb += mb; sc += mc;
            }
        blk_b[b] = sb; blk_c[b] = sc;
    }
    // k_decode_scan, once per array
    for (std::vector<uint64_t>* v : {&blk_b, &blk_c}) {
        uint64_t run = 0;
        for (uint64_t b = 0; b < n_blk; b++) { const uint64_t x = (*v)[b]; (*v)[b] = run; run += x; }
        (*v)[n_blk] = run;
    }
    // k_span_write
    const uint32_t CANARY = 0xC0FFEE0Du;
    std::vector<uint32_t> buf_b(BLK + 3, CANARY), buf_c(BLK + 3, CANARY), buf_m(BLK + 2, CANARY);
    uint32_t *s_b = buf_b.data() + 1, *s_c = buf_c.data() + 1, *s_mark = buf_m.data() + 1;
    std::vector<uint32_t> len(BLK), ent(BLK);
    memset(stats, 0, 5 * sizeof(uint64_t));
    for (uint64_t b = 0; b < n_blk; b++) {
        const uint64_t base = b * BLK;
        if (base > E) {
            const uint32_t zero[DD_PER * 4] = {0};
            for (uint32_t lane = 0; lane < lanes; lane++) {
                const uint64_t i0 = base + (uint64_t)lane * DD_PER;
                if (bspan) store<S64>(bspan, bspan_w, i0, sn_lane_count(i0, slots), zero);
                if (cspan) store<S64>(cspan, cspan_w, i0, sn_lane_count(i0, slots), zero);
            }
            continue;
        }
        stats[4]++;
        uint32_t rb = 0, rc = 0;
        for (uint32_t lane = 0; lane < lanes; lane++) {
            uint32_t mb, mc;
            sn_lane<I64>(a, t, s, base + (uint64_t)lane * DD_PER, E, &len[lane * DD_PER], &ent[lane * DD_PER], mb, mc);
            for (uint32_t j = 0; j < DD_PER; j++) {
                const uint32_t k = lane * DD_PER + j;
                s_b[k] = rb; s_c[k] = rc; s_mark[k] = 0;
                rb += len[k]; rc += ent[k] & (SN_CONT - 1u);
            }
        }
        s_b[BLK] = rb; s_c[BLK] = rc;
        const uint64_t B0 = blk_b[b], C0 = blk_c[b];
        uint64_t rounds = 0;
        const uint64_t first = dd_first_doc(a, base, lanes, LaneCount{lanes, &rounds});
        if (rounds > stats[1]) stats[1] = rounds;
        for (uint32_t lane = 0; lane < lanes; lane++)
            for (uint64_t d = first + lane; d <= a.n_docs; d += lanes) {
                const uint64_t st = dd_doc_start(a, d);
                if (!dd_owns(st, base, BLK)) break;
                boff[d] = B0 + s_b[st - base]; boff_w[d]++;
                if (coff) { coff[d] = C0 + s_c[st - base]; coff_w[d]++; }
                s_mark[st - base] = 1u;
            }
        uint64_t cb = 0, cc = 0;
        if (sn_has_carry(a, first, base)) {
            stats[2]++;
            const uint64_t st = dd_doc_start(a, first - 1);
            uint64_t b0; uint32_t r;
            sn_carry_place(st, BLK, b0, r);
            cb = blk_b[b0]; cc = blk_c[b0];
            if (r) {
                stats[3]++;
                for (uint32_t lane = 0; lane < lanes; lane++) {
                    uint32_t l2[DD_PER], e2[DD_PER], qb, qc;
                    sn_lane<I64>(a, t, s, b0 * BLK + (uint64_t)lane * DD_PER, st, l2, e2, qb, qc);
                    cb += qb; cc += qc;
                }
            }
            if (mutant == 1) { cb = B0; cc = C0; }
        }
        uint32_t before = 0;                              // the running maximum of (marked slot + 1) over the lanes in front
        for (uint32_t lane = 0; lane < lanes; lane++) {
            const uint64_t i0 = base + (uint64_t)lane * DD_PER;
            uint32_t wb[DD_PER * W], wc[DD_PER * W], m[DD_PER];
            const uint32_t lm = sn_lane_marks(&s_mark[lane * DD_PER], lane * DD_PER, m);
            for (uint32_t j = 0; j < DD_PER; j++) {
                const uint32_t k = lane * DD_PER + j;
                const uint32_t mm = sn_mark_at(m[j], before);
                uint64_t v[4] = {0, 0, 0, 0};
                if (i0 + j < E)
                    sn_span(B0 + s_b[k], C0 + s_c[k], sn_start_sum(mm, s_b, B0, cb), sn_start_sum(mm, s_c, C0, cc), len[k],
                            mutant == 2 ? ent[k] & (SN_CONT - 1u) : ent[k], v);
                sn_pack<S64>(v[0], v[1], wb + j * W);
                sn_pack<S64>(v[2], v[3], wc + j * W);
            }
            if (bspan) store<S64>(bspan, bspan_w, i0, sn_lane_count(i0, slots), wb);
            if (cspan) store<S64>(cspan, cspan_w, i0, sn_lane_count(i0, slots), wc);
            before = sn_mark_at(lm, before);
        }
        if (buf_b.front() != CANARY || buf_b[BLK + 2] != CANARY || buf_c.front() != CANARY || buf_c[BLK + 2] != CANARY ||
            buf_m.front() != CANARY || buf_m[BLK + 1] != CANARY) stats[0]++;
    }
    return 0;
}

extern "C" {

void sn_geometry(uint32_t out[4]) { out[0] = DD_NT; out[1] = DD_PER; out[2] = DD_BLK; out[3] = SN_MAX_TOKEN_BYTES; }

// what upload_decode stores per id: the table entries of n byte strings laid out by off[0 .. n]
void sn_entries(const uint8_t* bytes, const uint32_t* off, uint32_t n, uint16_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = sn_entry(bytes + off[k], off[k + 1] - off[k]);
}

// bspan / cspan: slots * (2 or 4) words (+ whatever canaries the caller keeps behind them), either may be null; boff / coff: n_docs + 1
int sn_spans(const void* ids, const uint64_t* ids_off, const int32_t* len, uint64_t n_docs, uint64_t n_cap, uint32_t row_len, uint32_t flags,
             const uint32_t* tok_off, uint32_t max_id, const uint32_t* sp_ids, const uint32_t* sp_off, uint32_t n_sp, const uint32_t* sp_bits,
             const uint16_t* nch, const uint16_t* sp_nch, uint32_t span_flags, uint32_t lanes, int mutant, uint32_t* bspan, uint32_t* cspan,
             uint64_t* boff, uint64_t* coff, uint8_t* bspan_w, uint8_t* cspan_w, uint8_t* boff_w, uint8_t* coff_w, uint64_t* stats) {
    DecIn a{};
    a.ids = ids; a.ids_off = ids_off; a.len = len; a.n_docs = n_docs; a.n_cap = row_len ? 0 : n_cap; a.row_len = row_len; a.flags = flags;
    const DecTab t{tok_off, nullptr, max_id, sp_ids, sp_off, n_sp, sp_bits};          // (no text: tok_bytes is never read)
    const SpanTab s{nch, sp_nch};
    if (lanes == 0) return -1;
    const bool i64 = (flags & DD_I64) != 0, s64 = (span_flags & SN_I64) != 0;
#define RUN(I, S) run<I, S>(a, t, s, lanes, mutant, bspan, cspan, boff, coff, bspan_w, cspan_w, boff_w, coff_w, stats)
    return i64 ? (s64 ? RUN(true, true) : RUN(true, false)) : (s64 ? RUN(false, true) : RUN(false, false));
#undef RUN
}

}  // extern "C"
