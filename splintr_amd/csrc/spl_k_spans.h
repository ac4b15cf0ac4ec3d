// spl_k_spans.h -- spl_token_spans_device: where every id of a CSR or of rows lies in the text spl_decode_batch_device writes for the same
// input -- per slot a byte span and a character span, counted from its document's start -- and the documents' global offsets
// (DESIGN.md 4.12).  A pure function of the ids: lengths from the decode tables, character counts from a u16 table beside them, no text.
//
//   k_span_len<I64>          one workgroup per block of DD_BLK slots: the block's sums of byte lengths and of characters (two words)
//   k_decode_scan            (spl_k_decode.h, unchanged) exclusive scan of either array of sums, the total behind it: two launches
//   k_span_write<I64, S64>   one workgroup per block: the 1 024 (len, nch, cont) again, scanned into LDS as in-block running sums; the
//                            offsets of the documents that start in the block (the decode's ownership rule, "end" included), each of
//                            which also MARKS its start slot in LDS; a running maximum over the marks gives every slot the start of its
//                            document, or "before the block"; the span is the slot's running sum minus the one at that start
//
// No atomics, no polling, no wait between workgroups; every span entry and every offset is written once, by the lane that owns it.
//
// Running sums never decrease, so "the sum at the start of my document" is the sum at the LAST marked slot at or before mine: empty
// documents (several marks on one slot) and any number of documents in a block need no window and no second path.  Only ONE document can
// reach into a block from an earlier one (the last whose start lies before the block's base).  Its start sum is the scanned sum of the
// block its start lies in plus the lengths of that block's slots below the start: the workgroup recomputes those, no per-document
// workspace.  Rows mode runs the same code (a row starts at r * row_len).
//
// What a slot gets (i a slot of document d; G_b / G_c the running sums of len / nch over ALL slots below i, s the clamped start of d):
//   byte span   (G_b(i) - G_b(s), the same + len(i))
//   char span   (cs - (cont(i) && cs > 0), cs + nch(i)),  cs = G_c(i) - G_c(s)       tiktoken's decode_with_offsets rule
// A slot at or beyond the clamped end belongs to no document: both spans are (0, 0).  int32 entries saturate at INT32_MAX.
//
// The mapping is the plain C++ of the first half of this file (values and pointers only, no HIP builtin): tests/hostsim/spans_sim.cpp
// includes it in a g++ build and evaluates it block by block and lane by lane; the kernels below call exactly these functions.
#pragma once
#include "spl_k_decode_dev.h"

namespace spl {

constexpr uint32_t SN_I64 = 1u;                      // (SPL_SPANS_I64 of include/splintr_hip.h)
constexpr uint32_t SN_CONT = 0x8000u;                // a table entry: characters in 15 bits, "the first byte continues a character" on top
constexpr uint32_t SN_MAX_TOKEN_BYTES = 0x7FFFu;     // what 15 bits count (the host refuses a vocabulary with a longer token)

// characters per id, beside DecTab's arrays and indexed like them: one entry per dense id, one per entry of the side table
struct SpanTab { const uint16_t* nch; const uint16_t* sp_nch; };
// byte_span / char_span: [slots, 2] int32 or int64 (null: not wanted); byte_off (required) / char_off: [n_docs + 1]
struct SpanOut { void* byte_span; void* char_span; uint64_t* byte_off; uint64_t* char_off; };

// ------------------------------------------------------------------------------------------ a table entry, a slot's characters
// what upload_decode stores for a byte string: the bytes that START a character, and whether the first one does not
SPL_HD uint16_t sn_entry(const uint8_t* p, uint32_t n) {
    uint32_t c = 0;
    for (uint32_t k = 0; k < n; k++) c += (p[k] & 0xC0u) != 0x80u ? 1u : 0u;
    return (uint16_t)(c | ((n && (p[0] & 0xC0u) == 0x80u) ? SN_CONT : 0u));
}
// the entry of an id dd_id_span gave a length > 0 for (so: a dense id, or one the side table holds)
SPL_HD uint32_t sn_id_entry(const DecTab& t, const SpanTab& s, uint32_t id) {
    if (id <= t.max_id) return s.nch[id];
    uint32_t lo = 0, hi = t.n_sp;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (t.sp_ids[mid] < id) lo = mid + 1; else hi = mid; }
    return s.sp_nch[lo];
}
// One lane's DD_PER consecutive slots from i0 on: byte lengths and table entries (0 where the length is 0), their sums.  A slot at or
// beyond lim (the clamped end -- or, for the carry-in, the document's start) counts nothing and is not read; validity, clamping and an
// id's length are the decode's (dd_slot_valid, dd_id_span), the read in one piece is dd_lane_lens'.
template <bool I64>
SPL_HD void sn_lane(const DecIn& a, const DecTab& t, const SpanTab& s, uint64_t i0, uint64_t lim, uint32_t len[DD_PER], uint32_t ent[DD_PER],
                    uint32_t& sum_b, uint32_t& sum_c) {
    typedef typename std::conditional<I64, uint64_t, uint32_t>::type id_t;
    const id_t* ids = static_cast<const id_t*>(__builtin_assume_aligned(a.ids, sizeof(id_t) * DD_PER)) + i0;
    struct alignas(sizeof(id_t) * DD_PER) Quad { id_t a, b, c, d; };
    static_assert(DD_PER == 4, "a lane reads its slots as one Quad");
    const bool whole = i0 + DD_PER <= lim;
    Quad q{};
    if (whole) q = *reinterpret_cast<const Quad*>(ids);
    sum_b = sum_c = 0;
#pragma unroll
    for (uint32_t j = 0; j < DD_PER; j++) {
        len[j] = 0; ent[j] = 0;
        if (!dd_slot_valid(a, i0 + j, lim)) continue;
        const id_t id = !whole ? ids[j] : (j == 0 ? q.a : j == 1 ? q.b : j == 2 ? q.c : q.d);
        uint32_t src;
        len[j] = I64 ? dd_id64_span(t, a.flags, (uint64_t)id, src) : dd_id_span(t, a.flags, (uint32_t)id, src);
        if (len[j]) ent[j] = sn_id_entry(t, s, (uint32_t)id);
        sum_b += len[j];
        sum_c += ent[j] & (SN_CONT - 1u);
    }
}

// ------------------------------------------------------------------------------------------ the carry-in
// `first` is the first document whose clamped start is >= base (dd_first_doc).  Slots of the block below that start
// belong to document first - 1, which starts BEFORE the block: true where there are such slots.
SPL_HD bool sn_has_carry(const DecIn& a, uint64_t first, uint64_t base) {
    return first >= 1 && first <= a.n_docs && dd_doc_start(a, first) > base;
}
// that document's start s lies in block s / blk, r slots into it: its start sums are the block's scanned sums plus the lengths of the
// block's first r slots (sn_lane with lim = s)
SPL_HD void sn_carry_place(uint64_t s, uint32_t blk, uint64_t& b0, uint32_t& r) { b0 = s / blk; r = (uint32_t)(s - b0 * blk); }

// ------------------------------------------------------------------------------------------ a slot's spans
// A lane's part of the running maximum over the marks: mk[j] != 0 where a document starts at the lane's slot j (slot0 = the lane's first
// slot in the block) -> m[j] = 1 + the last marked slot of THIS lane at or before j (0: none); returns m[DD_PER - 1], what the lanes
// behind it take over.  sn_mark_at joins it with `before`, the maximum over the lanes in front.
SPL_HD uint32_t sn_lane_marks(const uint32_t mk[DD_PER], uint32_t slot0, uint32_t m[DD_PER]) {
    uint32_t lm = 0;
#pragma unroll
    for (uint32_t j = 0; j < DD_PER; j++) { if (mk[j]) lm = slot0 + j + 1; m[j] = lm; }
    return lm;
}
SPL_HD uint32_t sn_mark_at(uint32_t m_j, uint32_t before) { return m_j > before ? m_j : before; }
// m: 1 + the last marked slot of the block at or before this one, 0: none (the document started before the block -> the carry-in, or
// there is no document in front of the slot at all and carry is 0).  run[]: the in-block running sums; g0: the block's scanned sum.
SPL_HD uint64_t sn_start_sum(uint32_t m, const uint32_t* run, uint64_t g0, uint64_t carry) { return m ? g0 + run[m - 1] : carry; }
// (gb, gc): the running sums at the slot, (sb, sc): at its document's start -> out[0 .. 1] the byte span, out[2 .. 3] the character span
SPL_HD void sn_span(uint64_t gb, uint64_t gc, uint64_t sb, uint64_t sc, uint32_t len, uint32_t ent, uint64_t out[4]) {
    const uint64_t bs = gb - sb, cs = gc - sc;
    out[0] = bs; out[1] = bs + len;
    out[2] = cs - (((ent & SN_CONT) && cs > 0) ? 1u : 0u);      // a token that begins inside a character starts at that character
    out[3] = cs + (ent & (SN_CONT - 1u));
}
SPL_HD uint32_t sn_sat32(uint64_t v) { return v > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)v; }
// one (start, end) as it is stored: two words (int32, saturated) or four (int64, little endian)
template <bool S64> SPL_HD void sn_pack(uint64_t s, uint64_t e, uint32_t* w) {
    if (S64) { w[0] = (uint32_t)s; w[1] = (uint32_t)(s >> 32); w[2] = (uint32_t)e; w[3] = (uint32_t)(e >> 32); }
    else { w[0] = sn_sat32(s); w[1] = sn_sat32(e); }
}
constexpr uint32_t sn_words(bool s64) { return s64 ? 4u : 2u; }       // words per span entry
// how many of a lane's DD_PER slots from i0 on exist (nothing is written at or beyond `slots`)
SPL_HD uint32_t sn_lane_count(uint64_t i0, uint64_t slots) { return i0 >= slots ? 0u : (slots - i0 < DD_PER ? (uint32_t)(slots - i0) : DD_PER); }

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// blk_b / blk_c: n_blk sums each (k_decode_scan puts the total behind them).  Two words, not one packed u64: a block's sums stay below
// 2^32 (1 024 slots of at most 32 767 bytes), the scanned sums of a call need not.
template <bool I64>
__global__ __launch_bounds__(DD_NT) void k_span_len(DecIn a, DecTab t, SpanTab s, uint64_t n_blk, uint64_t* __restrict__ blk_b,
                                                    uint64_t* __restrict__ blk_c) {
    __shared__ uint32_t s_w[2][DD_NT / 64];
    const uint64_t E = dd_end(a);
    for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint64_t base = b * DD_BLK;
        if (base >= E) {                                  // (uniform) wholly beyond the clamped end
            if (threadIdx.x == 0) { blk_b[b] = 0; blk_c[b] = 0; }
            continue;
        }
        uint32_t len[DD_PER], ent[DD_PER], mb, mc;
        sn_lane<I64>(a, t, s, base + (uint64_t)threadIdx.x * DD_PER, E, len, ent, mb, mc);
        const uint32_t xb = wave_scan_incl(mb), xc = wave_scan_incl(mc);
        if ((threadIdx.x & 63) == 63) { s_w[0][threadIdx.x >> 6] = xb; s_w[1][threadIdx.x >> 6] = xc; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t sb = 0, sc = 0;
            for (uint32_t w = 0; w < DD_NT / 64; w++) { sb += s_w[0][w]; sc += s_w[1][w]; }
            blk_b[b] = sb; blk_c[b] = sc;
        }
        __syncthreads();                                  // (the next block of this workgroup fills s_w again)
    }
}

// a lane's n (0 .. DD_PER) span entries from slot i0 on: all four in wide stores, fewer one entry (8 or 16 bytes) at a time
template <bool S64>
__device__ __forceinline__ void sn_store(void* out, uint64_t i0, uint32_t n, const uint32_t* w) {
    constexpr uint32_t W = sn_words(S64);
    uint32_t* p = static_cast<uint32_t*>(out) + i0 * W;
    if (n == DD_PER) {
#pragma unroll
        for (uint32_t q = 0; q < DD_PER * W / 4; q++)
            reinterpret_cast<uint4*>(p)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < DD_PER - 1; j++) {           // (constant indices: w stays in registers)
        if (j >= n) continue;
        if (S64) reinterpret_cast<uint4*>(p)[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
        else reinterpret_cast<uint2*>(p)[j] = make_uint2(w[2 * j], w[2 * j + 1]);
    }
}

// blk_b / blk_c: the exclusive scans of k_span_len's sums.  Every span entry below dd_slots(a) and every offset is written.
// (tests/hostsim/spans_sim.cpp runs the mapping functions above and dd_first_doc with a count over its own lanes.  What it still restates
//  of this kernel: the in-block scans, the running maximum ACROSS lanes, the carry-in's reduction and the document loop; a change to
//  those here is checked by tests/test_gpu_spans.py alone.)
template <bool I64, bool S64>
__global__ __launch_bounds__(DD_NT) void k_span_write(DecIn a, DecTab t, SpanTab s, uint64_t n_blk, const uint64_t* __restrict__ blk_b,
                                                      const uint64_t* __restrict__ blk_c, SpanOut o) {
    __shared__ __attribute__((aligned(16))) uint32_t s_b[DD_BLK + 4];       // in-block running byte sums, [DD_BLK] = the block's bytes
    __shared__ __attribute__((aligned(16))) uint32_t s_c[DD_BLK + 4];       // ... of characters
    __shared__ __attribute__((aligned(16))) uint32_t s_mark[DD_BLK];        // a document starts at this slot
    __shared__ uint32_t s_w[2][DD_NT / 64], s_r[2][DD_NT / 64], s_m[DD_NT / 64];
    constexpr uint32_t W = sn_words(S64);
    const uint64_t E = dd_end(a), slots = dd_slots(a);
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint64_t base = b * DD_BLK, i0 = base + (uint64_t)tid * DD_PER;
        const uint32_t n_mine = sn_lane_count(i0, slots);
        uint32_t wb[DD_PER * W], wc[DD_PER * W];
        if (base > E) {                                   // (uniform) no slot of a document, no document, not even the end: (0, 0)
#pragma unroll
            for (uint32_t k = 0; k < DD_PER * W; k++) wb[k] = 0;
            if (o.byte_span) sn_store<S64>(o.byte_span, i0, n_mine, wb);
            if (o.char_span) sn_store<S64>(o.char_span, i0, n_mine, wb);
            continue;
        }
        // the 1 024 lengths and character counts again, scanned
        uint32_t len[DD_PER], ent[DD_PER], mb, mc;
        sn_lane<I64>(a, t, s, i0, E, len, ent, mb, mc);
        const uint32_t xb = wave_scan_incl(mb), xc = wave_scan_incl(mc);
        if ((tid & 63) == 63) { s_w[0][wave] = xb; s_w[1][wave] = xc; }
        __syncthreads();
        uint32_t rb[DD_PER + 1], rc[DD_PER + 1];          // the running sums at the lane's slots and behind them
        rb[0] = xb - mb; rc[0] = xc - mc;
        for (uint32_t w = 0; w < wave; w++) { rb[0] += s_w[0][w]; rc[0] += s_w[1][w]; }
#pragma unroll
        for (uint32_t j = 0; j < DD_PER; j++) { rb[j + 1] = rb[j] + len[j]; rc[j + 1] = rc[j] + (ent[j] & (SN_CONT - 1u)); }
        *reinterpret_cast<uint4*>(&s_b[tid * DD_PER]) = make_uint4(rb[0], rb[1], rb[2], rb[3]);
        *reinterpret_cast<uint4*>(&s_c[tid * DD_PER]) = make_uint4(rc[0], rc[1], rc[2], rc[3]);
        *reinterpret_cast<uint4*>(&s_mark[tid * DD_PER]) = make_uint4(0u, 0u, 0u, 0u);
        if (tid == DD_NT - 1) { s_b[DD_BLK] = rb[DD_PER]; s_c[DD_BLK] = rc[DD_PER]; }
        __syncthreads();
        const uint64_t B0 = blk_b[b], C0 = blk_c[b];
        // the documents whose clamped start lies in this block's slots (the end, "document" n_docs, among them): offsets and marks
        const uint64_t first = dd_first_doc(a, base, DD_NT, WgCount{});
        for (uint64_t d = first + tid; d <= a.n_docs; d += DD_NT) {
            const uint64_t st = dd_doc_start(a, d);
            if (!dd_owns(st, base, DD_BLK)) break;        // (the starts are non-decreasing)
            o.byte_off[d] = B0 + s_b[st - base];
            if (o.char_off) o.char_off[d] = C0 + s_c[st - base];
            s_mark[st - base] = 1u;                       // (empty documents: several lanes, one value)
        }
        // the start sums of the one document that reaches into the block from before it
        uint64_t cb = 0, cc = 0;
        uint32_t r = 0;
        if (sn_has_carry(a, first, base)) {               // (uniform)
            const uint64_t st = dd_doc_start(a, first - 1);
            uint64_t b0;
            sn_carry_place(st, DD_BLK, b0, r);
            cb = blk_b[b0]; cc = blk_c[b0];
            if (r) {
                uint32_t l2[DD_PER], e2[DD_PER], qb, qc;
                sn_lane<I64>(a, t, s, b0 * DD_BLK + (uint64_t)tid * DD_PER, st, l2, e2, qb, qc);
                const uint32_t yb = wave_scan_incl(qb), yc = wave_scan_incl(qc);
                if ((tid & 63) == 63) { s_r[0][wave] = yb; s_r[1][wave] = yc; }
            }
        }
        __syncthreads();                                  // the marks and the carry-in's wave sums
        if (r)
            for (uint32_t w = 0; w < DD_NT / 64; w++) { cb += s_r[0][w]; cc += s_r[1][w]; }
        // every slot's last mark at or before it: a running maximum of (slot + 1)
        uint32_t m[DD_PER];
        const uint4 mk = *reinterpret_cast<const uint4*>(&s_mark[tid * DD_PER]);
        const uint32_t mj[DD_PER] = {mk.x, mk.y, mk.z, mk.w};
        const uint32_t lm = sn_lane_marks(mj, tid * DD_PER, m);
        const uint32_t xm = wave_scan_max(lm);
        if ((tid & 63) == 63) s_m[wave] = xm;
        uint32_t before = (uint32_t)__shfl_up((int)xm, 1);
        if ((tid & 63) == 0) before = 0;
        __syncthreads();
        for (uint32_t w = 0; w < wave; w++) before = sn_mark_at(s_m[w], before);
        // the spans of the lane's slots
#pragma unroll
        for (uint32_t j = 0; j < DD_PER; j++) {
            uint64_t v[4] = {0, 0, 0, 0};
            if (i0 + j < E) {
                const uint32_t mm = sn_mark_at(m[j], before);
                sn_span(B0 + rb[j], C0 + rc[j], sn_start_sum(mm, s_b, B0, cb), sn_start_sum(mm, s_c, C0, cc), len[j], ent[j], v);
            }
            sn_pack<S64>(v[0], v[1], wb + j * W);
            sn_pack<S64>(v[2], v[3], wc + j * W);
        }
        if (o.byte_span) sn_store<S64>(o.byte_span, i0, n_mine, wb);
        if (o.char_span) sn_store<S64>(o.char_span, i0, n_mine, wc);
        __syncthreads();                                  // (the next block of this workgroup fills the LDS again)
    }
}
#endif  // __HIPCC__

}  // namespace spl
