// decode_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_decode_dev.h (the code k_dec_len / k_dec_gather run) evaluated
// on the CPU block by block and lane by lane, with the kernels' geometry -- DD_PER slots a lane, groups of DD_W output bytes by absolute
// address, the in-block starts as an array (guarded by canaries) -- for every output byte and every offset.  The number of lanes of a
// workgroup is a parameter (a block is lanes * DD_PER slots), so that block edges can be tested exhaustively at small sizes.  Every write
// is counted per destination byte / offset.  Built with g++; no GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_decode_dev.h"
#include "gather_sim.h"

using namespace spl;

// stats: [0] wide stores, [1] byte stores, [2] canary damage of the starts array, [3] most rounds of one document search,
//        [4] wide stores at a misaligned address, [5] blocks
template <bool I64>
static int run(const DecIn& a, const DecTab& t, uint32_t lanes, uint8_t* out, uint64_t cap, uint64_t* out_off, uint8_t* out_writes,
               uint8_t* off_writes, uint64_t* stats) {
    const uint32_t BLK = lanes * DD_PER;
    const uint64_t n_blk = dd_n_blocks(dd_slots(a), BLK);
    const uint64_t E = dd_end(a);
    std::vector<uint64_t> blk(n_blk + 1, 0);
    // k_dec_len
    for (uint64_t b = 0; b < n_blk; b++) {
        const uint64_t base = b * BLK;
        uint64_t sum = 0;
        if (base < E)
            for (uint32_t lane = 0; lane < lanes; lane++) {
                uint32_t len[DD_PER], src[DD_PER];
                sum += dd_lane_lens<I64>(a, t, base + (uint64_t)lane * DD_PER, E, len, src);
            }
        blk[b] = sum;
    }
    // k_decode_scan
    uint64_t run = 0;
    for (uint64_t b = 0; b < n_blk; b++) { const uint64_t v = blk[b]; blk[b] = run; run += v; }
    blk[n_blk] = run;
    // k_dec_gather
    const uint32_t CANARY = 0xC0FFEE0Du;
    std::vector<uint32_t> sbuf(BLK + 3, CANARY), s_src(BLK, 0);
    uint32_t* s_start = sbuf.data() + 1;
    memset(stats, 0, 6 * sizeof(uint64_t));
    for (uint64_t b = 0; b < n_blk; b++) {
        const uint64_t base = b * BLK;
        if (base > E) continue;
        stats[5]++;
        uint32_t st = 0;
        for (uint32_t lane = 0; lane < lanes; lane++) {
            uint32_t len[DD_PER], src[DD_PER];
            dd_lane_lens<I64>(a, t, base + (uint64_t)lane * DD_PER, E, len, src);
            for (uint32_t j = 0; j < DD_PER; j++) { s_start[lane * DD_PER + j] = st; s_src[lane * DD_PER + j] = src[j]; st += len[j]; }
        }
        s_start[BLK] = st;
        const uint64_t b0 = blk[b], b1c = dd_cut(b0 + s_start[BLK], cap);
        if (b1c > b0) {
            const uint64_t g_last = (b1c - 1) / DD_W;
            for (uint32_t lane = 0; lane < lanes; lane++)
                for (uint64_t g = b0 / DD_W + lane; g <= g_last; g += lanes) {
                    uint64_t lo, hi;
                    dd_group_range(g, b0, b1c, lo, hi);
                    const uint32_t p = (uint32_t)(lo - b0), n = (uint32_t)(hi - lo);
                    uint32_t w[DD_W / 4];
                    dd_gather(s_start, s_src.data(), t.tok_bytes, dd_owner(s_start, BLK, p), p, n, w);
                    if (dd_group_wide(lo, hi)) {
                        stats[0]++;
                        if (lo % DD_W) stats[4]++;
                        for (uint32_t k = 0; k < DD_W; k++) { out[lo + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3))); out_writes[lo + k]++; }
                    } else {
                        for (uint32_t k = 0; k < n; k++) { out[lo + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3))); out_writes[lo + k]++; stats[1]++; }
                    }
                }
        }
        uint64_t rounds = 0;
        const uint64_t first = dd_first_doc(a, base, lanes, LaneCount{lanes, &rounds});
        if (rounds > stats[3]) stats[3] = rounds;
        for (uint32_t lane = 0; lane < lanes; lane++)
            for (uint64_t d = first + lane; d <= a.n_docs; d += lanes) {
                const uint64_t s = dd_doc_start(a, d);
                if (!dd_owns(s, base, BLK)) break;
                out_off[d] = b0 + s_start[s - base];
                off_writes[d]++;
            }
        if (sbuf.front() != CANARY || sbuf[BLK + 2] != CANARY) stats[2]++;
    }
    return 0;
}

extern "C" {

void ds_geometry(uint32_t out[4]) { out[0] = DD_NT; out[1] = DD_PER; out[2] = DD_BLK; out[3] = DD_W; }

// out / out_writes: cap bytes (+ whatever canaries the caller keeps behind them); out_off / off_writes: n_docs + 1 entries
int ds_decode(const void* ids, const uint64_t* ids_off, const int32_t* len, uint64_t n_docs, uint64_t n_cap, uint32_t row_len, uint32_t flags,
              const uint32_t* tok_off, const uint8_t* tok_bytes, uint32_t max_id, const uint32_t* sp_ids, const uint32_t* sp_off, uint32_t n_sp,
              const uint32_t* sp_bits, uint32_t lanes, uint8_t* out, uint64_t cap, uint64_t* out_off, uint8_t* out_writes, uint8_t* off_writes,
              uint64_t* stats) {
    DecIn a{};
    a.ids = ids; a.ids_off = ids_off; a.len = len; a.n_docs = n_docs; a.n_cap = row_len ? 0 : n_cap; a.row_len = row_len; a.flags = flags;
    const DecTab t{tok_off, tok_bytes, max_id, sp_ids, sp_off, n_sp, sp_bits};
    if (lanes == 0) return -1;
    return (flags & DD_I64) ? run<true>(a, t, lanes, out, cap, out_off, out_writes, off_writes, stats)
                            : run<false>(a, t, lanes, out, cap, out_off, out_writes, off_writes, stats);
}

}  // extern "C"
