// collate_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_collate.h (the code k_collate_pad / k_collate_pack run)
// evaluated on the CPU for every output element, with the kernels' geometry: workgroups of COL_NT lanes, COL_VEC elements a lane, the
// kernel's own two cooperative k-ary searches (col_span_docs) with the workgroup's count played lane by lane (gather_sim.h), the window
// of COL_WIN document starts (guarded by canaries: it must never be indexed beyond its size) and the global search for spans that hold
// more documents than the window.  Built with g++; no GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_collate.h"
#include "gather_sim.h"

using namespace spl;

extern "C" {

void cs_geometry(uint32_t out[4]) { out[0] = COL_NT; out[1] = COL_VEC; out[2] = COL_SPAN; out[3] = COL_WIN; }

// rows u32 [n_docs * L], mask u8, len i32 (mask / len may be null)
int cs_pad(const uint32_t* ids, const uint64_t* off, uint64_t n_docs, uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t bos_id,
           uint32_t eos_id, uint32_t* rows, uint8_t* mask, int32_t* len) {
    const ColOpts o{flags, L, pad_id, bos_id, eos_id};
    const uint64_t total = n_docs * L, n_spans = (total + COL_SPAN - 1) / COL_SPAN;
    for (uint64_t span = 0; span < n_spans; span++)
        for (uint32_t lane = 0; lane < COL_NT; lane++) {
            const uint64_t e0 = span * COL_SPAN + (uint64_t)lane * COL_VEC;
            if (e0 >= total) continue;
            const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
            uint32_t v[COL_VEC], m;
            col_pad_group(ids, off, e0, n, o, v, m, len);
            for (uint32_t i = 0; i < n; i++) {
                rows[e0 + i] = v[i];
                if (mask) mask[e0 + i] = (uint8_t)((m >> (8 * i)) & 0xFF);
            }
        }
    return 0;
}

// total = rows_cap * L elements of rows / doc / pos are written (doc / pos may be null); n_out[0] = rows needed, n_out[1] = S.
// stats: [0] spans that used the window, [1] spans that searched the global array, [2] most rounds of one search, [3] canary damage.
int cs_pack(const uint32_t* ids, const uint64_t* off, uint64_t n_docs, uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t bos_id,
            uint32_t eos_id, uint32_t* rows, uint64_t total, int32_t* doc_out, int32_t* pos_out, uint64_t n_out[2], uint32_t stats[4]) {
    const ColOpts o{flags, L, pad_id, bos_id, eos_id};
    const uint32_t k = col_k(flags);
    const uint64_t S = off[n_docs] + n_docs * k;
    n_out[0] = (S + L - 1) / L; n_out[1] = S;
    memset(stats, 0, 16);
    const uint64_t CANARY = 0xC0FFEE0DDF00Dull;
    std::vector<uint64_t> win_buf(COL_WIN + 2, CANARY);
    uint64_t* s_win = win_buf.data() + 1;
    const uint64_t n_spans = (total + COL_SPAN - 1) / COL_SPAN;
    for (uint64_t span = 0; span < n_spans; span++) {
        const uint64_t s0 = span * COL_SPAN;
        const uint64_t s_end = s0 + COL_SPAN < total ? s0 + COL_SPAN : total;
        const bool in_stream = s0 < S;
        uint32_t d_lo = 0, d_hi = 0, n_win = 0;
        bool use_win = false;
        if (in_stream) {
            const uint64_t p_last = (s_end < S ? s_end : S) - 1;
            const uint32_t r = col_span_docs(off, k, k, n_docs, s0, p_last, d_lo, d_hi, LaneCount{COL_NT, nullptr});
            if (r > stats[2]) stats[2] = r;
            use_win = col_use_window(d_lo, d_hi);
            if (use_win) {
                n_win = d_hi - d_lo + 1;
                if (n_win > COL_WIN) return -1;
                for (uint32_t i = 0; i < COL_WIN; i++) s_win[i] = 0;                 // (a read beyond n_win finds a start that is <= every p: a wrong document, not a lucky one)
                for (uint32_t i = 0; i < n_win; i++) s_win[i] = col_doc_start(off, (uint64_t)d_lo + i, k);
                stats[0]++;
            } else {
                stats[1]++;
            }
        }
        for (uint32_t lane = 0; lane < COL_NT; lane++) {
            const uint64_t e0 = s0 + (uint64_t)lane * COL_VEC;
            const uint32_t n = e0 >= s_end ? 0u : (s_end - e0 < COL_VEC ? (uint32_t)(s_end - e0) : COL_VEC);
            if (!n) continue;
            uint32_t v[COL_VEC], pos[COL_VEC];
            int32_t doc[COL_VEC];
            if (!in_stream) { for (uint32_t i = 0; i < COL_VEC; i++) { v[i] = pad_id; doc[i] = -1; pos[i] = 0; } }
            else if (use_win) col_pack_group(ids, off, S, e0, n, d_lo, o, ColLocWin{s_win, n_win, d_lo}, v, doc, pos);
            else col_pack_group(ids, off, S, e0, n, d_lo, o, ColLocGlobal{off, k, d_hi}, v, doc, pos);
            for (uint32_t i = 0; i < n; i++) {
                rows[e0 + i] = v[i];
                if (doc_out) doc_out[e0 + i] = doc[i];
                if (pos_out) pos_out[e0 + i] = (int32_t)pos[i];
            }
        }
        if (win_buf.front() != CANARY || win_buf.back() != CANARY) stats[3]++;
    }
    return 0;
}

}  // extern "C"
