// spl_k_collate.h -- from the CSR result (ids[T] u32, out_off[n_docs + 1] u64) to what a model reads, one launch each:
//
//   k_collate_pad    rows[n_docs, L]: row d = [BOS] + document d's ids cut to L - k + [EOS], the rest pad_id; mask, len
//   k_collate_pack   the stream  [BOS] ids_0 [EOS] [BOS] ids_1 [EOS] ...  cut into rows of L; doc and pos per element
//
// Both are pure gathers: every output element is written once, by the lane that owns it -- no atomics, no workspace, no second pass.
// Every output is a flat array; a lane owns COL_VEC consecutive flat elements (one 16-byte store of int32, two of int64, one 4-byte
// store of the mask), a workgroup COL_SPAN of them.  L need not be a multiple of COL_VEC: the elements of a lane's group are resolved one
// by one and may lie in different rows.
//
// The mapping from an output element to its source is the plain C++ of the first half of this file (values and pointers only, no
// HIP builtin): tests/hostsim/collate_sim.cpp includes it in a g++ build and evaluates it for every output element; the kernels below
// call exactly these functions.
//
// Pack mode needs, per element, the document a stream position p lies in: the LARGEST d with out_off[d] + d * k <= p (k = BOS + EOS
// tokens added per document; out_off is already the prefix sum, so the stream needs no scan).  "Largest" is what skips empty documents
// when k = 0: they add nothing to the stream and share their start with their successor.  The search over the whole offset array runs
// ONCE PER WORKGROUP: a cooperative k-ary search (every lane probes one split point per round: 2^31 documents in four rounds) for the
// document of the span's first and of its last position; the starts of the documents between them go to LDS, and a lane finishes its
// search there.  With k >= 1 a span of COL_SPAN positions holds at most COL_SPAN documents; with k = 0 a run of empty documents puts
// any number of (equal) starts into it: a span with more than COL_WIN documents leaves the window alone and its lanes search the global
// array between the span's two bounds -- the window is never indexed beyond COL_WIN entries.
#pragma once
#include "spl_common.h"

namespace spl {

// (the values of SPL_COLLATE_* in include/splintr_hip.h)
constexpr uint32_t COL_I64 = 1u, COL_PAD_LEFT = 2u, COL_KEEP_TAIL = 4u, COL_BOS = 8u, COL_EOS = 16u;
constexpr uint32_t COL_NT = 256;                    // lanes per workgroup
constexpr uint32_t COL_VEC = 4;                     // flat elements per lane
constexpr uint32_t COL_SPAN = COL_NT * COL_VEC;     // flat elements per workgroup
constexpr uint32_t COL_WIN = COL_SPAN;              // document starts the LDS window holds (8 KB)

struct ColOpts { uint32_t flags, L, pad_id, bos_id, eos_id; };

SPL_HD uint32_t col_bos(uint32_t flags) { return (flags & COL_BOS) ? 1u : 0u; }
SPL_HD uint32_t col_k(uint32_t flags) { return col_bos(flags) + ((flags & COL_EOS) ? 1u : 0u); }

// flat element -> (row, column); the 32-bit division where the index allows it
SPL_HD void col_rowcol(uint64_t e, uint32_t L, uint64_t& r, uint32_t& c) {
    if ((e >> 32) == 0) { const uint32_t e32 = (uint32_t)e; r = e32 / L; c = e32 % L; }
    else { r = e / L; c = (uint32_t)(e % L); }
}

// ------------------------------------------------------------------------------------------ pad mode
// entries of a row that are not padding: the document's ids cut to the budget L - k, plus BOS and EOS (never cut away)
SPL_HD uint32_t col_pad_used(uint64_t len_d, const ColOpts& o) {
    const uint32_t k = col_k(o.flags), budget = o.L - k;
    return (len_d < budget ? (uint32_t)len_d : budget) + k;
}
// column c of the row of a document whose ids are ids[o0 .. o1): the value; returns the mask (false: padding)
SPL_HD bool col_pad_elem(const uint32_t* ids, uint64_t o0, uint64_t o1, uint32_t c, const ColOpts& o, uint32_t& val) {
    const uint64_t len_d = o1 - o0;
    const uint32_t used = col_pad_used(len_d, o), bos = col_bos(o.flags), n_tok = used - col_k(o.flags);
    const uint32_t lead = (o.flags & COL_PAD_LEFT) ? o.L - used : 0u;
    val = o.pad_id;
    if (c < lead || c - lead >= used) return false;
    const uint32_t q = c - lead;
    if (bos && q == 0) { val = o.bos_id; return true; }
    if ((o.flags & COL_EOS) && q == used - 1) { val = o.eos_id; return true; }
    const uint64_t first = (o.flags & COL_KEEP_TAIL) ? len_d - n_tok : 0;     // KEEP_TAIL: truncation drops the FRONT of the document
    val = ids[o0 + first + (q - bos)];
    return true;
}
// One lane's group: n (1..COL_VEC) flat elements from e0 on.  v[i]: the values; m: the mask bytes, byte i for element i; len[d] is
// stored by the lane that owns column 0 of row d.
SPL_HD void col_pad_group(const uint32_t* ids, const uint64_t* off, uint64_t e0, uint32_t n, const ColOpts& o, uint32_t v[COL_VEC],
                          uint32_t& m, int32_t* len) {
    uint64_t r; uint32_t c;
    col_rowcol(e0, o.L, r, c);
    uint64_t o0 = off[r], o1 = off[r + 1];
    m = 0;
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) {
        v[i] = o.pad_id;
        if (i >= n) continue;
        if (c == 0 && len) len[r] = (int32_t)col_pad_used(o1 - o0, o);
        if (col_pad_elem(ids, o0, o1, c, o, v[i])) m |= 1u << (8 * i);
        if (++c == o.L) {
            c = 0; r++;
            if (i + 1 < n) { o0 = o1; o1 = off[r + 1]; }         // (more elements: the next row exists)
        }
    }
}

// ------------------------------------------------------------------------------------------ pack mode
SPL_HD uint64_t col_doc_start(const uint64_t* off, uint64_t d, uint32_t k) { return off[d] + d * k; }

// The cooperative k-ary search for the LARGEST d of [lo, hi] with start_d <= p (start_lo <= p holds): every round, lane i probes
// d_i = lo + (i + 1) * step; the starts are non-decreasing, so the lanes that find start_{d_i} <= p are the first cnt ones, and the
// answer lies in [lo + cnt * step, lo + (cnt + 1) * step - 1].  The kernel counts with one barrier per round.
SPL_HD uint32_t col_kary_step(uint32_t lo, uint32_t hi) { return (hi - lo + COL_NT - 1) / COL_NT; }
SPL_HD bool col_kary_pred(const uint64_t* off, uint32_t k, uint32_t lo, uint32_t hi, uint32_t step, uint32_t lane, uint64_t p) {
    const uint64_t d = (uint64_t)lo + (uint64_t)(lane + 1) * step;
    return d <= hi && col_doc_start(off, d, k) <= p;
}
SPL_HD void col_kary_narrow(uint32_t& lo, uint32_t& hi, uint32_t step, uint32_t cnt) {
    const uint64_t nlo = (uint64_t)lo + (uint64_t)cnt * step, nhi = nlo + step - 1;
    lo = (uint32_t)nlo;
    if (nhi < hi) hi = (uint32_t)nhi;
}
// the upper bound of the search for the span's last document: with k >= 1 every document takes a position of its own
SPL_HD uint32_t col_span_hi_bound(uint32_t d_lo, uint64_t n_docs, uint32_t k) {
    const uint64_t last = n_docs - 1, far = (uint64_t)d_lo + COL_SPAN - 1;
    return (uint32_t)((k && far < last) ? far : last);
}
SPL_HD bool col_use_window(uint32_t d_lo, uint32_t d_hi) { return d_hi - d_lo < COL_WIN; }
// One search: lo becomes the LARGEST d of [lo, hi] with start_d <= p; returns its rounds.  count(pred) = how many of the workgroup's
// COL_NT lanes hold pred(lane): one barrier in a kernel (WgCount of spl_k_merge.h), a loop over the lanes in a host simulation.
template <class Count>
SPL_HD uint32_t col_kary_search(const uint64_t* starts, uint32_t k, uint32_t& lo, uint32_t hi, uint64_t p, const Count& count) {
    uint32_t rounds = 0;
    for (; lo < hi; rounds++) {
        const uint32_t step = col_kary_step(lo, hi);
        const uint32_t cnt = count([&](uint32_t lane) { return col_kary_pred(starts, k, lo, hi, step, lane, p); });
        col_kary_narrow(lo, hi, step, cnt);
    }
    return rounds;
}
// The documents d_lo, d_hi of a span's first and last position (p_first <= p_last, both in a document): the search over all documents
// for the first, then from d_lo up to col_span_hi_bound for the last.  start_d = starts[d] + d * k; k_bound is the k of the bound
// (pack mode: k; windows search row_off with k = 0, and every document has a row of its own: 1).  Uniform over the workgroup: every
// lane takes part in every round.  Returns the most rounds one of the two searches took (the simulations report it, a kernel drops it).
template <class Count>
SPL_HD uint32_t col_span_docs(const uint64_t* starts, uint32_t k, uint32_t k_bound, uint64_t n_docs, uint64_t p_first, uint64_t p_last,
                              uint32_t& d_lo, uint32_t& d_hi, const Count& count) {
    d_lo = 0;
    const uint32_t r_lo = col_kary_search(starts, k, d_lo, (uint32_t)(n_docs - 1), p_first, count);
    d_hi = d_lo;
    const uint32_t r_hi = col_kary_search(starts, k, d_hi, col_span_hi_bound(d_lo, n_docs, k_bound), p_last, count);
    return r_lo > r_hi ? r_lo : r_hi;
}

// A lane's search, from the document d_prev of its previous element (of the span's first position for its first element) on: the
// LARGEST d of [d_prev, d_hi] with start_d <= p.  Nearly always the next start lies beyond p and one read settles it.
struct ColLocWin {                 // win[i] = start of document d_lo + i, i < n
    const uint64_t* win; uint32_t n, d_lo;
    SPL_HD uint32_t operator()(uint32_t d_prev, uint64_t p) const {
        uint32_t lo = d_prev - d_lo, hi = n - 1;
        if (lo == hi || win[lo + 1] > p) return d_prev;
        lo++;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (win[mid] <= p) lo = mid; else hi = mid - 1;
        }
        return d_lo + lo;
    }
};
struct ColLocGlobal {              // the span holds more documents than the window: the offset array itself, between the span's bounds
    const uint64_t* off; uint32_t k, d_hi;
    SPL_HD uint32_t operator()(uint32_t d_prev, uint64_t p) const {
        uint32_t lo = d_prev, hi = d_hi;
        if (lo == hi || col_doc_start(off, (uint64_t)lo + 1, k) > p) return d_prev;
        lo++;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (col_doc_start(off, mid, k) <= p) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
};

// stream position p of document d (ids[o0 .. o0 + len_d), stream start o0 + d * k), column c of its row: value and position.
// Positions restart at a document's start and at a row's start (a row is the attention context): p - max(start, p - c) = min(j, c).
SPL_HD void col_pack_elem(const uint32_t* ids, uint64_t o0, uint64_t len_d, uint64_t start, uint64_t p, uint32_t c, const ColOpts& o,
                          uint32_t& val, uint32_t& pos) {
    const uint64_t j = p - start;
    const uint32_t bos = col_bos(o.flags);
    pos = j < c ? (uint32_t)j : c;
    if (bos && j == 0) val = o.bos_id;
    else if ((o.flags & COL_EOS) && j == len_d + bos) val = o.eos_id;
    else val = ids[o0 + j - bos];
}
// One lane's group: n (1..COL_VEC) stream positions from p0 on; S = the stream's length; d_first = the document of the span's first position.
template <class Loc>
SPL_HD void col_pack_group(const uint32_t* ids, const uint64_t* off, uint64_t S, uint64_t p0, uint32_t n, uint32_t d_first, const ColOpts& o,
                           const Loc& loc, uint32_t v[COL_VEC], int32_t doc[COL_VEC], uint32_t pos[COL_VEC]) {
    uint64_t r; uint32_t c;
    col_rowcol(p0, o.L, r, c);
    const uint32_t k = col_k(o.flags);
    uint32_t d = d_first;
    bool have = false;
    uint64_t o0 = 0, len_d = 0;
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) {
        v[i] = o.pad_id; doc[i] = -1; pos[i] = 0;
        const uint64_t p = p0 + i;
        if (i < n && p < S) {
            const uint32_t nd = loc(d, p);
            if (!have || nd != d) { d = nd; o0 = off[d]; len_d = off[(uint64_t)d + 1] - o0; have = true; }
            col_pack_elem(ids, o0, len_d, o0 + (uint64_t)d * k, p, c, o, v[i], pos[i]);
            doc[i] = (int32_t)d;
        }
        if (++c == o.L) c = 0;
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
template <bool I64> __device__ __forceinline__ void col_store4(void* rows, uint64_t e, const uint32_t v[COL_VEC]) {
    if (I64) {                                          // ids are bit patterns: int64 ZERO-extends
        uint4* q = reinterpret_cast<uint4*>(static_cast<uint64_t*>(rows) + e);
        q[0] = make_uint4(v[0], 0u, v[1], 0u);
        q[1] = make_uint4(v[2], 0u, v[3], 0u);
    } else {
        *reinterpret_cast<uint4*>(static_cast<uint32_t*>(rows) + e) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}
template <bool I64> __device__ __forceinline__ void col_store1(void* rows, uint64_t e, uint32_t v) {
    if (I64) static_cast<uint64_t*>(rows)[e] = (uint64_t)v;
    else static_cast<uint32_t*>(rows)[e] = v;
}
// What the gather kernels of this family (here, spl_k_window.h, spl_k_pair.h, spl_k_chat.h, spl_k_seqpack.h) store of one lane's group
// of n (0..COL_VEC) flat elements from e0 on: all four in one wide store, or -- the final partial group of an output -- one by one, so
// that nothing is written past the output's end.  The partial paths index the group's registers with constants (a lane's own index
// would put the group into scratch memory: sqp_store_labels, spl_k_seqpack.h).  The rows (k_collate_chat and k_seqpack_gather keep a
// rows tail of their own and say why; their byte and int32 arrays go through the two functions below):
template <bool I64> __device__ __forceinline__ void col_store_group(void* rows, uint64_t e0, uint32_t n, const uint32_t v[COL_VEC]) {
    if (n == COL_VEC) { col_store4<I64>(rows, e0, v); return; }
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) if (i < n) col_store1<I64>(rows, e0 + i, v[i]);
}
// a byte array (null: not wanted), byte i of `bytes` for element i
__device__ __forceinline__ void col_store_bytes(uint8_t* out, uint64_t e0, uint32_t n, uint32_t bytes) {
    if (!out) return;
    if (n == COL_VEC) { *reinterpret_cast<uint32_t*>(out + e0) = bytes; return; }
    for (uint32_t i = 0; i < n; i++) out[e0 + i] = (uint8_t)(bytes >> (8 * i));
}
// an int32 array (null: not wanted)
__device__ __forceinline__ void col_store_i32(int32_t* out, uint64_t e0, uint32_t n, const int32_t x[COL_VEC]) {
    if (!out) return;
    if (n == COL_VEC) { *reinterpret_cast<int4*>(out + e0) = make_int4(x[0], x[1], x[2], x[3]); return; }
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) if (i < n) out[e0 + i] = x[i];
}

// The starts of documents d_lo .. d_hi (at most COL_WIN of them) into the LDS window, readable by every lane on return; their number.
__device__ __forceinline__ uint32_t col_fill_window(uint64_t* s_win, const uint64_t* starts, uint32_t k, uint32_t d_lo, uint32_t d_hi) {
    const uint32_t n_win = d_hi - d_lo + 1;
    for (uint32_t i = threadIdx.x; i < n_win; i += COL_NT) s_win[i] = col_doc_start(starts, (uint64_t)d_lo + i, k);
    __syncthreads();
    return n_win;
}

// grid: one workgroup per span of COL_SPAN flat elements (beyond 2^31 - 1 spans a workgroup takes several)
template <bool I64>
__global__ __launch_bounds__(COL_NT) void k_collate_pad(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ off, uint64_t n_docs,
                                                        ColOpts o, void* __restrict__ rows, uint8_t* __restrict__ mask,
                                                        int32_t* __restrict__ len) {
    const uint64_t total = n_docs * o.L, n_spans = (total + COL_SPAN - 1) / COL_SPAN;
    for (uint64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
        const uint64_t e0 = span * COL_SPAN + (uint64_t)threadIdx.x * COL_VEC;
        if (e0 >= total) continue;
        const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
        uint32_t v[COL_VEC], m;
        col_pad_group(ids, off, e0, n, o, v, m, len);
        col_store_group<I64>(rows, e0, n, v);           // (the final group may be partial: nothing is written past n_docs * L)
        col_store_bytes(mask, e0, n, m);                // (col_pad_group sets a mask byte to 0 or 1: stored as it is)
    }
}

// (tests/hostsim/collate_sim.cpp runs the mapping functions above and col_span_docs -- both searches and the bound between them -- with
//  a count over its own lanes.  What it still restates of this kernel: the span loop with p_last, the choice between window and global
//  search, and the window fill; a change to those here is checked by tests/test_gpu_collate.py alone.)
// total = rows_cap * L: every element below it is written (beyond the stream: pad_id, doc -1, pos 0), nothing at or beyond it.
// n_out[0] = the rows the stream needs, n_out[1] = its length -- always.
template <bool I64>
__global__ __launch_bounds__(COL_NT) void k_collate_pack(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ off, uint64_t n_docs,
                                                         ColOpts o, void* __restrict__ rows, uint64_t total, int32_t* __restrict__ doc_out,
                                                         int32_t* __restrict__ pos_out, uint64_t* __restrict__ n_out) {
    __shared__ uint64_t s_win[COL_WIN];
    const uint32_t k = col_k(o.flags);
    const uint64_t S = off[n_docs] + n_docs * k;
    if (blockIdx.x == 0 && threadIdx.x == 0) { n_out[0] = (S + o.L - 1) / o.L; n_out[1] = S; }
    const uint64_t n_spans = (total + COL_SPAN - 1) / COL_SPAN;
    for (uint64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
        const uint64_t s0 = span * COL_SPAN;
        const uint64_t s_end = s0 + COL_SPAN < total ? s0 + COL_SPAN : total;
        const uint64_t e0 = s0 + (uint64_t)threadIdx.x * COL_VEC;
        const uint32_t n = e0 >= s_end ? 0u : (s_end - e0 < COL_VEC ? (uint32_t)(s_end - e0) : COL_VEC);
        uint32_t v[COL_VEC], pos[COL_VEC];
        int32_t doc[COL_VEC];
        const bool in_stream = s0 < S;                  // (uniform over the workgroup)
        if (in_stream) {
            // the documents of the span's first and last stream position: uniform, every lane takes part in every round
            const uint64_t p_last = (s_end < S ? s_end : S) - 1;
            uint32_t d_lo, d_hi;
            col_span_docs(off, k, k, n_docs, s0, p_last, d_lo, d_hi, WgCount{});
            if (col_use_window(d_lo, d_hi)) {
                const uint32_t n_win = col_fill_window(s_win, off, k, d_lo, d_hi);
                if (n) col_pack_group(ids, off, S, e0, n, d_lo, o, ColLocWin{s_win, n_win, d_lo}, v, doc, pos);
                __syncthreads();                        // (the next span of this workgroup fills the window again)
            } else if (n) {
                col_pack_group(ids, off, S, e0, n, d_lo, o, ColLocGlobal{off, k, d_hi}, v, doc, pos);
            }
        } else {
            for (uint32_t i = 0; i < COL_VEC; i++) { v[i] = o.pad_id; doc[i] = -1; pos[i] = 0; }
        }
        col_store_group<I64>(rows, e0, n, v);           // (the final group may be partial: nothing is written past rows_cap * L)
        col_store_i32(doc_out, e0, n, doc);
        col_store_i32(pos_out, e0, n, reinterpret_cast<const int32_t*>(pos));       // (position ids are stored as int32)
    }
}
#endif  // __HIPCC__

}  // namespace spl
