// spl_k_window.h -- the CSR result as SLIDING WINDOWS: every document alone and complete, as rows of L that overlap by a fixed number
// of ids (what Hugging Face calls return_overflowing_tokens with a stride).  k = BOS + EOS, B = L - k the body budget,
// step = B - overlap:
//
//   rows of document d     n_w(d) = 1 if len_d <= B, else 1 + ceil((len_d - B) / step)       (an empty document has its row too)
//   window w of d          ids [w * step, min(w * step + B, len_d)) of the document, as [BOS] body [EOS] and padding: exactly the
//                          pad-mode row of that VIRTUAL document (col_pad_elem of spl_k_collate.h, KEEP_TAIL off)
//   row_off[d]             the rows in front of document d: the exclusive prefix sum of n_w -- NOT a closed form over out_off, so
//                          a scan runs in front of the gather
//
//   k_window_scan          one workgroup per span of WIN_SPAN documents: n_w per document, the exclusive scan within the span to
//                          row_off, the span's total to the workspace.  A batch of one span (n_docs <= WIN_SPAN) is done here:
//                          the workgroup also writes row_off[n_docs] and n_out.
//   k_window_totals        (more than one span) ONE workgroup: the exclusive scan of the spans' totals, in place, chunk by chunk
//   k_window_add           (more than one span) every span adds its base to its part of row_off, in place; row_off[n_docs], n_out
//   k_window_gather        k_collate_pack's shape over ROWS instead of stream positions: flat output, COL_VEC elements a lane,
//                          COL_SPAN a workgroup; the documents of the span's first and last row by the cooperative k-ary search
//                          over row_off, the starts between them in the LDS window, each element col_pad_elem on the virtual document
//
// Reduce-then-scan over LAUNCHES: a workgroup never waits for another one -- no polling, no look-back chain, no read-modify-write on a
// shared word; the order comes from the stream.  Nothing here uses an atomic, and every output element is written once.
//
// Every document has at least one row, so row_off is STRICTLY increasing: a span of COL_SPAN elements touches at most COL_SPAN rows and
// therefore at most COL_SPAN documents -- the window (COL_WIN = COL_SPAN starts) always holds them, and pack mode's global fall-back
// (runs of empty documents that share a start) has no counterpart here.  tests/hostsim/window_sim.cpp asserts the bound.
//
// As in spl_k_collate.h the mapping is the plain C++ of the first half (values and pointers only): tests/hostsim/window_sim.cpp
// includes it in a g++ build; the kernels call exactly these functions.
#pragma once
#include "spl_k_collate.h"

namespace spl {

constexpr uint32_t WIN_PER = 16;                     // documents per lane of the scan (a run of consecutive ones)
constexpr uint32_t WIN_SPAN = COL_NT * WIN_PER;      // documents per workgroup of the scan: 4096
constexpr uint32_t WIN_CHUNK = COL_NT;               // span totals per round of k_window_totals (fewer: a test's option)

struct WinGeo { uint32_t B, step; };                 // body budget L - k (>= 1), step B - overlap (1 .. B)

SPL_HD uint64_t win_spans(uint64_t n_docs) { return (n_docs + WIN_SPAN - 1) / WIN_SPAN; }
// words of workspace: nothing for one span; else the spans' totals and, behind them, the grand total
SPL_HD uint64_t win_work_words(uint64_t n_docs) { const uint64_t s = win_spans(n_docs); return s > 1 ? s + 1 : 0; }

// ceil(a / s); the 32-bit division where the operands allow it (as col_rowcol)
SPL_HD uint64_t win_ceil_div(uint64_t a, uint32_t s) {
    const uint64_t t = a + (s - 1);                  // (a <= 2^63 here: ids counted by a byte count)
    if ((t >> 32) == 0) return (uint32_t)t / s;
    return t / s;
}
// rows of a document of len_d ids
SPL_HD uint64_t win_n_rows(uint64_t len_d, const WinGeo& g) {
    return len_d <= g.B ? 1u : 1u + win_ceil_div(len_d - g.B, g.step);
}
// the virtual document of window w (w < n_w) of the document ids[o0 .. o1): ids[v0 .. v1)
SPL_HD void win_bounds(uint64_t o0, uint64_t o1, uint64_t w, const WinGeo& g, uint64_t& v0, uint64_t& v1) {
    v0 = o0 + w * g.step;                            // (w * step < len_d for every window of the document: v0 <= o1)
    v1 = o1 - v0 > g.B ? v0 + g.B : o1;
}

// ------------------------------------------------------------------------------------------ the scan
// One lane's run: documents d0 .. d0 + cnt - 1 (cnt <= WIN_PER).  pre[j] = the rows of the run's documents in front of document
// d0 + j; returns the run's rows.
SPL_HD uint64_t win_scan_lane(const uint64_t* off, uint64_t d0, uint32_t cnt, const WinGeo& g, uint64_t pre[WIN_PER]) {
    uint64_t sum = 0, lo = cnt ? off[d0] : 0;
#pragma unroll
    for (uint32_t j = 0; j < WIN_PER; j++) {
        pre[j] = sum;
        if (j < cnt) { const uint64_t hi = off[d0 + j + 1]; sum += win_n_rows(hi - lo, g); lo = hi; }
    }
    return sum;
}
// the documents of lane `lane` of span `span`: its first one and how many (0: beyond the batch)
SPL_HD uint32_t win_scan_run(uint64_t n_docs, uint64_t span, uint32_t lane, uint64_t& d0) {
    d0 = span * WIN_SPAN + (uint64_t)lane * WIN_PER;
    if (d0 >= n_docs) return 0;
    return n_docs - d0 < WIN_PER ? (uint32_t)(n_docs - d0) : WIN_PER;
}
SPL_HD uint64_t win_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ------------------------------------------------------------------------------------------ the gather
// One lane's group: n (1..COL_VEC) flat elements from e0 on; R = row_off[n_docs], the rows that hold documents.  A row r < R belongs to
// the LARGEST d with row_off[d] <= r (loc: the window search of spl_k_collate.h, over row starts), its window is w = r - row_off[d].
// v[i]: the values; m: the mask bytes; the per-row outputs are stored by the lane that owns column 0 of the row.  Rows from R on:
// pad_id, mask 0, len 0, doc -1, start 0.
SPL_HD void win_group(const uint32_t* ids, const uint64_t* off, uint64_t R, uint64_t e0, uint32_t n, uint32_t d_first, const ColOpts& o,
                      const WinGeo& g, const ColLocWin& loc, uint32_t v[COL_VEC], uint32_t& m, int32_t* len, int32_t* row_doc,
                      int64_t* row_start) {
    uint64_t r; uint32_t c;
    col_rowcol(e0, o.L, r, c);
    uint32_t d = d_first;
    bool have = false;
    uint64_t v0 = 0, v1 = 0, w = 0;
    m = 0;
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) {
        v[i] = o.pad_id;
        if (i >= n) continue;
        if (r < R) {
            if (!have) {
                d = loc(d, r);
                w = r - loc.win[d - loc.d_lo];
                win_bounds(off[d], off[(uint64_t)d + 1], w, g, v0, v1);
                have = true;
            }
            if (c == 0) {
                if (len) len[r] = (int32_t)col_pad_used(v1 - v0, o);
                if (row_doc) row_doc[r] = (int32_t)d;
                if (row_start) row_start[r] = (int64_t)(w * g.step);
            }
            if (col_pad_elem(ids, v0, v1, c, o, v[i])) m |= 1u << (8 * i);
        } else if (c == 0) {
            if (len) len[r] = 0;
            if (row_doc) row_doc[r] = -1;
            if (row_start) row_start[r] = 0;
        }
        if (++c == o.L) { c = 0; r++; have = false; }
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// The inclusive scan of one value per lane over the workgroup (COL_NT lanes, four wavefronts): shuffles within a wavefront, the
// wavefronts' totals through LDS.  total: the sum over the workgroup.  Every lane calls it; s_wave is free again on return.
__device__ __forceinline__ uint64_t win_block_scan(uint64_t x, uint64_t* s_wave, uint64_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    x = wave_scan_incl64(x);
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint64_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < COL_NT / 64; i++) { const uint64_t t = s_wave[i]; if (i < wave) base += t; sum += t; }
    __syncthreads();
    total = sum;
    return x + base;
}

// grid: win_spans(n_docs) workgroups, at least one.  work == nullptr: the batch is one span (or empty) and this launch is all of the scan.
__global__ __launch_bounds__(COL_NT) void k_window_scan(const uint64_t* __restrict__ off, uint64_t n_docs, WinGeo g, uint64_t rows_cap,
                                                        uint64_t* __restrict__ row_off, uint64_t* __restrict__ work,
                                                        uint64_t* __restrict__ n_out) {
    __shared__ uint64_t s_wave[COL_NT / 64];
    uint64_t d0, pre[WIN_PER], total;
    const uint32_t cnt = win_scan_run(n_docs, blockIdx.x, threadIdx.x, d0);
    const uint64_t sum = win_scan_lane(off, d0, cnt, g, pre);
    const uint64_t base = win_block_scan(sum, s_wave, total) - sum;
#pragma unroll
    for (uint32_t j = 0; j < WIN_PER; j++)
        if (j < cnt) row_off[d0 + j] = base + pre[j];
    if (threadIdx.x == 0) {
        if (work) work[blockIdx.x] = total;
        else { row_off[n_docs] = total; n_out[0] = total; n_out[1] = win_min(total, rows_cap); }
    }
}

// ONE workgroup: tot[0 .. n) to their exclusive prefix sums in place, chunk (<= COL_NT) of them a round; tot[n] = the sum of all.
__global__ __launch_bounds__(COL_NT) void k_window_totals(uint64_t* __restrict__ tot, uint64_t n, uint32_t chunk) {
    __shared__ uint64_t s_wave[COL_NT / 64];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < n; b += chunk) {
        const uint64_t i = b + threadIdx.x;
        const bool mine = threadIdx.x < chunk && i < n;
        const uint64_t x = mine ? tot[i] : 0;
        uint64_t total;
        const uint64_t incl = win_block_scan(x, s_wave, total);
        if (mine) tot[i] = carry + incl - x;
        carry += total;
    }
    if (threadIdx.x == 0) tot[n] = carry;
}

// grid: win_spans(n_docs) workgroups: span b adds tot[b] to row_off[b * WIN_SPAN ..); the last one writes row_off[n_docs] and n_out
__global__ __launch_bounds__(COL_NT) void k_window_add(uint64_t n_docs, uint64_t rows_cap, uint64_t* __restrict__ row_off,
                                                       const uint64_t* __restrict__ tot, uint64_t* __restrict__ n_out) {
    const uint64_t base = tot[blockIdx.x], d_begin = (uint64_t)blockIdx.x * WIN_SPAN;
    const uint64_t d_end = win_min(d_begin + WIN_SPAN, n_docs);
    if (base)
        for (uint64_t d = d_begin + threadIdx.x; d < d_end; d += COL_NT) row_off[d] += base;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const uint64_t total = tot[gridDim.x];
        row_off[n_docs] = total; n_out[0] = total; n_out[1] = win_min(total, rows_cap);
    }
}

// (tests/hostsim/window_sim.cpp runs the mapping functions and col_span_docs -- both searches and the bound between them -- with a count
//  over its own lanes.  What it still restates of this kernel: the span loop with r_first and r_last, and the window fill; a change to
//  those here is checked by tests/test_gpu_window.py alone.)
// total = rows_cap * L: every element below it is written, nothing at or beyond it; the per-row outputs likewise below rows_cap.
template <bool I64>
__global__ __launch_bounds__(COL_NT) void k_window_gather(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ off,
                                                          const uint64_t* __restrict__ row_off, uint64_t n_docs, ColOpts o, WinGeo g,
                                                          void* __restrict__ rows, uint64_t total, uint8_t* __restrict__ mask,
                                                          int32_t* __restrict__ len, int32_t* __restrict__ row_doc,
                                                          int64_t* __restrict__ row_start) {
    __shared__ uint64_t s_win[COL_WIN];
    const uint64_t R = row_off[n_docs];
    const uint64_t n_spans = (total + COL_SPAN - 1) / COL_SPAN;
    for (uint64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
        const uint64_t s0 = span * COL_SPAN;
        const uint64_t s_end = s0 + COL_SPAN < total ? s0 + COL_SPAN : total;
        const uint64_t e0 = s0 + (uint64_t)threadIdx.x * COL_VEC;
        const uint32_t n = e0 >= s_end ? 0u : (s_end - e0 < COL_VEC ? (uint32_t)(s_end - e0) : COL_VEC);
        uint32_t v[COL_VEC], m = 0;
        uint64_t r_first, r_last; uint32_t c;
        col_rowcol(s0, o.L, r_first, c);
        uint32_t d_lo = 0, n_win = 0;
        if (r_first < R) {                              // (uniform over the workgroup: every lane takes part in every round)
            col_rowcol(s_end - 1, o.L, r_last, c);
            if (r_last >= R) r_last = R - 1;
            // the documents of the span's first and last row, over row_off (k = 0: a document's start is row_off[d] itself; the bound's
            // k = 1: every document takes a row of its own, so the span holds at most COL_SPAN of them and n_win <= COL_WIN)
            uint32_t d_hi;
            col_span_docs(row_off, 0u, 1u, n_docs, r_first, r_last, d_lo, d_hi, WgCount{});
            n_win = col_fill_window(s_win, row_off, 0u, d_lo, d_hi);
        }
        if (n) win_group(ids, off, R, e0, n, d_lo, o, g, ColLocWin{s_win, n_win, d_lo}, v, m, len, row_doc, row_start);
        if (r_first < R) __syncthreads();               // (the next span of this workgroup fills the window again)
        col_store_group<I64>(rows, e0, n, v);           // (the final group may be partial: nothing is written past rows_cap * L)
        col_store_bytes(mask, e0, n, m);                // (win_group sets a mask byte to 0 or 1: stored as it is)
    }
}
#endif  // __HIPCC__

}  // namespace spl
