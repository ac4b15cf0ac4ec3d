// window_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_window.h (the code k_window_scan / _totals / _add /
// _gather run) evaluated on the CPU with the kernels' geometry.  The scan: every lane's run by win_scan_lane, the sums over a workgroup's
// lanes restated in plain code, the spans' totals chunk by chunk, the bases added.  The gather: every output element lane by lane, the
// kernel's own two cooperative searches over row_off (col_span_docs) with the count played lane by lane (gather_sim.h), the window of
// COL_WIN row starts guarded by canaries -- and the bound that makes pack mode's global fall-back unnecessary here (a span never holds
// more than COL_WIN documents) asserted.  Built with g++; no GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_window.h"
#include "gather_sim.h"

using namespace spl;

extern "C" {

void ws_geometry(uint32_t out[6]) { out[0] = COL_NT; out[1] = COL_VEC; out[2] = COL_SPAN; out[3] = COL_WIN; out[4] = WIN_SPAN; out[5] = WIN_CHUNK; }
uint64_t ws_work_words(uint64_t n_docs) { return win_work_words(n_docs); }

// row_off [n_docs + 1], n_out [2], work [win_work_words(n_docs)] (null where that is 0); launches: how many kernels ran; returns -1 if
// the workspace would be needed and is missing.
int ws_scan(const uint64_t* off, uint64_t n_docs, uint32_t B, uint32_t step, uint32_t chunk, uint64_t rows_cap, uint64_t* row_off,
            uint64_t* n_out, uint64_t* work, uint32_t* launches) {
    const WinGeo g{B, step};
    const uint64_t spans = win_spans(n_docs), grid = spans ? spans : 1;
    if (spans > 1 && !work) return -1;
    uint64_t* tot = spans > 1 ? work : nullptr;
    // k_window_scan
    for (uint64_t b = 0; b < grid; b++) {
        std::vector<uint64_t> sum(COL_NT);
        std::vector<std::vector<uint64_t>> pre(COL_NT, std::vector<uint64_t>(WIN_PER));
        for (uint32_t lane = 0; lane < COL_NT; lane++) {
            uint64_t d0;
            const uint32_t cnt = win_scan_run(n_docs, b, lane, d0);
            sum[lane] = win_scan_lane(off, d0, cnt, g, pre[lane].data());
        }
        uint64_t base = 0;                              // (win_block_scan: the exclusive sum over the lanes in front)
        for (uint32_t lane = 0; lane < COL_NT; lane++) {
            uint64_t d0;
            const uint32_t cnt = win_scan_run(n_docs, b, lane, d0);
            for (uint32_t j = 0; j < cnt; j++) row_off[d0 + j] = base + pre[lane][j];
            base += sum[lane];
        }
        if (tot) tot[b] = base;
        else { row_off[n_docs] = base; n_out[0] = base; n_out[1] = win_min(base, rows_cap); }
    }
    *launches = 1;
    if (!tot) return 0;
    // k_window_totals
    uint64_t carry = 0;
    for (uint64_t b = 0; b < spans; b += chunk) {
        uint64_t run = 0;
        for (uint32_t lane = 0; lane < COL_NT; lane++) {
            const uint64_t i = b + lane;
            if (lane < chunk && i < spans) { const uint64_t x = tot[i]; tot[i] = carry + run; run += x; }
        }
        carry += run;
    }
    tot[spans] = carry;
    // k_window_add
    for (uint64_t b = 0; b < spans; b++) {
        const uint64_t d_end = win_min((b + 1) * WIN_SPAN, n_docs);
        for (uint64_t d = b * WIN_SPAN; d < d_end; d++) row_off[d] += tot[b];
    }
    row_off[n_docs] = tot[spans]; n_out[0] = tot[spans]; n_out[1] = win_min(tot[spans], rows_cap);
    *launches = 3;
    return 0;
}

// total = rows_cap * L elements of rows / mask are written, rows_cap entries of len / doc / start (each may be null).
// stats: [0] spans that hold rows of documents, [1] the most documents one span's window held, [2] most rounds of one search,
// [3] canary damage.  Returns -1 if a span would need more than COL_WIN window entries (the bound of spl_k_window.h's header comment).
int ws_gather(const uint32_t* ids, const uint64_t* off, const uint64_t* row_off, uint64_t n_docs, uint32_t flags, uint32_t L, uint32_t pad_id,
              uint32_t bos_id, uint32_t eos_id, uint32_t overlap, uint32_t* rows, uint64_t total, uint8_t* mask, int32_t* len,
              int32_t* row_doc, int64_t* row_start, uint32_t stats[4]) {
    const ColOpts o{flags, L, pad_id, bos_id, eos_id};
    const WinGeo g{L - col_k(flags), L - col_k(flags) - overlap};
    memset(stats, 0, 16);
    const uint64_t CANARY = 0xC0FFEE0DDF00Dull;
    std::vector<uint64_t> win_buf(COL_WIN + 2, CANARY);
    uint64_t* s_win = win_buf.data() + 1;
    const uint64_t R = row_off[n_docs];
    const uint64_t n_spans = (total + COL_SPAN - 1) / COL_SPAN;
    for (uint64_t span = 0; span < n_spans; span++) {
        const uint64_t s0 = span * COL_SPAN;
        const uint64_t s_end = s0 + COL_SPAN < total ? s0 + COL_SPAN : total;
        uint64_t r_first, r_last; uint32_t c;
        col_rowcol(s0, L, r_first, c);
        uint32_t d_lo = 0, n_win = 0;
        if (r_first < R) {
            col_rowcol(s_end - 1, L, r_last, c);
            if (r_last >= R) r_last = R - 1;
            uint32_t d_hi;
            const uint32_t r = col_span_docs(row_off, 0u, 1u, n_docs, r_first, r_last, d_lo, d_hi, LaneCount{COL_NT, nullptr});
            if (r > stats[2]) stats[2] = r;
            // the search stopped at the bound: the document behind it must start beyond the span's last row, or the bound is wrong
            const uint32_t hi = col_span_hi_bound(d_lo, n_docs, 1u);
            if (d_hi == hi && (uint64_t)hi + 1 < n_docs && row_off[(uint64_t)hi + 1] <= r_last) return -1;
            n_win = d_hi - d_lo + 1;
            if (n_win > COL_WIN) return -1;
            for (uint32_t i = 0; i < COL_WIN; i++) s_win[i] = 0;                     // (a read beyond n_win finds a start that is <= every row: a wrong document, not a lucky one)
            for (uint32_t i = 0; i < n_win; i++) s_win[i] = row_off[(uint64_t)d_lo + i];
            stats[0]++;
            if (n_win > stats[1]) stats[1] = n_win;
        }
        for (uint32_t lane = 0; lane < COL_NT; lane++) {
            const uint64_t e0 = s0 + (uint64_t)lane * COL_VEC;
            const uint32_t n = e0 >= s_end ? 0u : (s_end - e0 < COL_VEC ? (uint32_t)(s_end - e0) : COL_VEC);
            if (!n) continue;
            uint32_t v[COL_VEC], m;
            win_group(ids, off, R, e0, n, d_lo, o, g, ColLocWin{s_win, n_win, d_lo}, v, m, len, row_doc, row_start);
            for (uint32_t i = 0; i < n; i++) {
                rows[e0 + i] = v[i];
                if (mask) mask[e0 + i] = (uint8_t)((m >> (8 * i)) & 0xFF);
            }
        }
        if (win_buf.front() != CANARY || win_buf.back() != CANARY) stats[3]++;
    }
    return 0;
}

}  // extern "C"
