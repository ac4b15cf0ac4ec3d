// spl_k_decode_dev.h -- spl_decode_batch_device: ids in HBM (a CSR, or rows [n_docs, row_len] with a validity predicate) to a bytes CSR in
// HBM, three launches on the caller's stream:
//
//   k_dec_len<I64>      one workgroup per block of DD_BLK id slots: every slot's byte length, summed per block
//   k_decode_scan       (spl_k_decode.h, unchanged) exclusive scan of the block sums, the total behind them
//   k_dec_gather<I64>   one workgroup per block: the 1 024 lengths again, scanned into LDS as in-block starts; then the block's output range
//                       [blk[b], blk[b + 1]) OUTPUT-centrically -- a lane owns aligned groups of DD_W consecutive output bytes (by absolute
//                       address), finds the slot of its first byte by binary search over the LDS starts, walks on from there byte by byte
//                       and issues ONE wide store; and the offsets of the documents that start in the block's slots
//
// No atomics, no polling, no wait between workgroups; every output byte and every offset is written once, by the lane that owns it.
//
// A slot's length is 0 when it lies at or beyond the clamped end, is padding (rows mode), is skipped (DD_SKIP_SPECIAL) or is an id of
// neither map.  Byte p of a block (counted from the block's first byte) belongs to the LARGEST slot i with start_i <= p: zero-length
// slots share their start with their successor and are skipped -- collate's empty-run rule.
//
// The groups at the two ends of a block's range are partial wherever the range does not begin or end on a multiple of DD_W: the
// neighbouring workgroup owns the other bytes of such a group, so they are written with byte stores (a wide store there is a race).
// The same holds for the group bytes_capacity cuts.
//
// Position "end" (the clamped id count E) is owned like a slot: the grid has E_max / DD_BLK + 1 = ceil((E_max + 1) / DD_BLK) blocks,
// E_max being the slots the call covers, so that block floor(E / DD_BLK) exists even when E is a multiple of DD_BLK; a document (or
// the closing offset, "document" n_docs) belongs to the ONE block whose slot range holds its clamped start.
//
// The mapping is the plain C++ of the first half of this file (values and pointers only, no HIP builtin): tests/hostsim/decode_sim.cpp
// includes it in a g++ build and evaluates it block by block and lane by lane; the kernels below call exactly these functions.
#pragma once
#include <type_traits>

#include "spl_common.h"

#ifndef SPL_DEC_GROUP
#define SPL_DEC_GROUP 16               /* output bytes a lane owns per step: 16 or 4 (profiles/decode_device.txt) */
#endif

namespace spl {

// (the values of SPL_DECODE_* in include/splintr_hip.h)
constexpr uint32_t DD_I64 = 1u, DD_PAD_LEFT = 2u, DD_SKIP_SPECIAL = 4u;
constexpr uint32_t DD_NT = 256;                     // lanes per workgroup
constexpr uint32_t DD_PER = 4;                      // consecutive id slots per lane
constexpr uint32_t DD_BLK = DD_NT * DD_PER;         // id slots per workgroup (== DEC_BLK: k_decode_scan's block sums)
constexpr uint32_t DD_W = SPL_DEC_GROUP;            // bytes per group
static_assert(DD_W == 4 || DD_W == 16, "a group is one 4-byte or one 16-byte store");

// id -> bytes: the dense table over the vocabulary's id range (specials fill its holes), the sorted side table of the specials beyond it
// (upload_decode), and one bit per dense id: set where ONLY the special map holds the id.
struct DecTab {
    const uint32_t* tok_off; const uint8_t* tok_bytes; uint32_t max_id;
    const uint32_t* sp_ids; const uint32_t* sp_off; uint32_t n_sp;
    const uint32_t* sp_bits;
};
// the input: CSR mode (row_len == 0: ids_off[n_docs + 1], n_cap an upper bound of the id count) or rows mode (ids [n_docs, row_len];
// len[n_docs] or null)
struct DecIn {
    const void* ids; const uint64_t* ids_off; const int32_t* len;
    uint64_t n_docs, n_cap; uint32_t row_len, flags;
};

// ------------------------------------------------------------------------------------------ slots: where they end, which are valid
SPL_HD uint64_t dd_slots(const DecIn& a) { return a.row_len ? a.n_docs * a.row_len : a.n_cap; }       // what the grid covers
SPL_HD uint64_t dd_n_blocks(uint64_t slots, uint32_t blk) { return slots / blk + 1; }                   // ceil((slots + 1) / blk): "end" has an owner
// the clamped start of document d, d = 0 .. n_docs (n_docs: the end).  CSR mode: an offset beyond n_cap is n_cap.
SPL_HD uint64_t dd_doc_start(const DecIn& a, uint64_t d) {
    if (a.row_len) return d * a.row_len;
    const uint64_t s = a.ids_off[d];
    return s < a.n_cap ? s : a.n_cap;
}
SPL_HD uint64_t dd_end(const DecIn& a) { return dd_doc_start(a, a.n_docs); }
SPL_HD void dd_rowcol(uint64_t i, uint32_t L, uint64_t& r, uint32_t& c) {
    if ((i >> 32) == 0) { const uint32_t i32 = (uint32_t)i; r = i32 / L; c = i32 % L; }
    else { r = i / L; c = (uint32_t)(i % L); }
}
// rows mode: entry c of row r counts (the first len[r] entries, with DD_PAD_LEFT the last; len[r] clamped to 0 .. row_len)
SPL_HD bool dd_row_valid(const DecIn& a, uint64_t r, uint32_t c) {
    if (!a.len) return true;
    const int32_t l = a.len[r];
    const uint32_t n = l < 0 ? 0u : ((uint32_t)l > a.row_len ? a.row_len : (uint32_t)l);
    return (a.flags & DD_PAD_LEFT) ? c >= a.row_len - n : c < n;
}
SPL_HD bool dd_slot_valid(const DecIn& a, uint64_t i, uint64_t E) {
    if (i >= E) return false;
    if (!a.row_len) return true;
    uint64_t r; uint32_t c;
    dd_rowcol(i, a.row_len, r, c);
    return dd_row_valid(a, r, c);
}

// ------------------------------------------------------------------------------------------ an id's bytes
// length and place in tok_bytes of what id decodes to (Tokenizer::decode_bytes: the vocabulary first, then the special map, else nothing)
SPL_HD uint32_t dd_id_span(const DecTab& t, uint32_t flags, uint32_t id, uint32_t& src) {
    src = 0;
    if (id <= t.max_id) {
        if ((flags & DD_SKIP_SPECIAL) && ((t.sp_bits[id >> 5] >> (id & 31)) & 1u)) return 0u;
        src = t.tok_off[id];
        return t.tok_off[id + 1] - src;
    }
    if (flags & DD_SKIP_SPECIAL) return 0u;            // every id of the side table is special by construction
    uint32_t lo = 0, hi = t.n_sp;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (t.sp_ids[mid] < id) lo = mid + 1; else hi = mid; }
    if (lo < t.n_sp && t.sp_ids[lo] == id) { src = t.sp_off[lo]; return t.sp_off[lo + 1] - src; }
    return 0u;
}
// int64 ids: a value outside 0 .. 2^32 - 1 is an id of neither map
SPL_HD uint32_t dd_id64_span(const DecTab& t, uint32_t flags, uint64_t v, uint32_t& src) {
    src = 0;
    return (v >> 32) ? 0u : dd_id_span(t, flags, (uint32_t)v, src);
}
// One lane's DD_PER consecutive slots from i0 on: lengths and sources.  Ids at or beyond E are not read: a lane whose slots all lie
// below E reads them in one piece (16 or 32 aligned bytes -- padding slots of rows mode included, they are inside the buffer).
template <bool I64>
SPL_HD uint32_t dd_lane_lens(const DecIn& a, const DecTab& t, uint64_t i0, uint64_t E, uint32_t len[DD_PER], uint32_t src[DD_PER]) {
    typedef typename std::conditional<I64, uint64_t, uint32_t>::type id_t;
    const id_t* ids = static_cast<const id_t*>(__builtin_assume_aligned(a.ids, sizeof(id_t) * DD_PER)) + i0;
    struct alignas(sizeof(id_t) * DD_PER) Quad { id_t a, b, c, d; };
    static_assert(DD_PER == 4, "a lane reads its slots as one Quad");
    const bool whole = i0 + DD_PER <= E;
    Quad q{};
    if (whole) q = *reinterpret_cast<const Quad*>(ids);
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < DD_PER; j++) {
        len[j] = 0; src[j] = 0;
        if (!dd_slot_valid(a, i0 + j, E)) continue;
        const id_t id = !whole ? ids[j] : (j == 0 ? q.a : j == 1 ? q.b : j == 2 ? q.c : q.d);
        len[j] = I64 ? dd_id64_span(t, a.flags, (uint64_t)id, src[j]) : dd_id_span(t, a.flags, (uint32_t)id, src[j]);
        sum += len[j];
    }
    return sum;
}

// ------------------------------------------------------------------------------------------ the owner rule
// starts[0 .. n]: the in-block starts of a block's n slots, starts[n] = the block's byte count.  The slot of byte p < starts[n]: the
// LARGEST i with starts[i] <= p (starts[0] == 0).  Zero-length slots share their start with their successor and never own a byte.
SPL_HD uint32_t dd_owner(const uint32_t* starts, uint32_t n, uint32_t p) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (starts[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// n (1 .. DD_W) bytes from in-block byte p on, whose owner is slot i, little endian into w: the walk is per output byte, a token may
// be of any length.  p + n <= starts[n_slots] keeps i below n_slots.
SPL_HD void dd_gather(const uint32_t* starts, const uint32_t* src, const uint8_t* tok_bytes, uint32_t i, uint32_t p, uint32_t n,
                      uint32_t w[DD_W / 4]) {
    uint32_t nxt = starts[i + 1], delta = src[i] - starts[i];
#pragma unroll
    for (uint32_t q = 0; q < DD_W / 4; q++) w[q] = 0;
#pragma unroll
    for (uint32_t k = 0; k < DD_W; k++) {
        if (k >= n) continue;
        if (p >= nxt) {
            do { i++; nxt = starts[i + 1]; } while (p >= nxt);
            delta = src[i] - starts[i];
        }
        w[k >> 2] |= (uint32_t)tok_bytes[delta + p] << (8 * (k & 3));
        p++;
    }
}

// ------------------------------------------------------------------------------------------ groups, edges, the capacity cut
// a block whose bytes are [b0, b1) writes [b0, dd_cut(b1, cap)): bytes at or beyond the capacity are dropped
SPL_HD uint64_t dd_cut(uint64_t b1, uint64_t cap) { return b1 < cap ? b1 : cap; }
// the part [lo, hi) of group g (absolute bytes [g * DD_W, g * DD_W + DD_W)) the block owns; a group it owns whole gets one wide store,
// any other one byte stores
SPL_HD void dd_group_range(uint64_t g, uint64_t b0, uint64_t b1c, uint64_t& lo, uint64_t& hi) {
    lo = g * DD_W; hi = lo + DD_W;
    if (lo < b0) lo = b0;
    if (hi > b1c) hi = b1c;
}
SPL_HD bool dd_group_wide(uint64_t lo, uint64_t hi) { return hi - lo == DD_W; }

// ------------------------------------------------------------------------------------------ which documents a block owns
SPL_HD bool dd_owns(uint64_t start, uint64_t base, uint32_t blk) { return start >= base && start - base < blk; }
// CSR mode: the FIRST d of [0, n_docs + 1] whose clamped start is >= base (n_docs + 1: none), by a cooperative k-ary search over the
// starts (non-decreasing): every round, lane i probes d_i = lo + (i + 1) * step - 1; the lanes that find start < base are the first
// cnt ones, and the answer lies in [lo + cnt * step, min(lo + (cnt + 1) * step - 1, hi)].  The kernel counts with one barrier a round.
SPL_HD uint64_t dd_kary_step(uint64_t lo, uint64_t hi, uint32_t lanes) { return (hi - lo + lanes - 1) / lanes; }
SPL_HD bool dd_kary_pred(const DecIn& a, uint64_t lo, uint64_t hi, uint64_t step, uint32_t lane, uint64_t base) {
    const uint64_t d = lo + (uint64_t)(lane + 1) * step - 1;
    return d < hi && dd_doc_start(a, d) < base;
}
SPL_HD void dd_kary_narrow(uint64_t& lo, uint64_t& hi, uint64_t step, uint32_t cnt) {
    const uint64_t nlo = lo + (uint64_t)cnt * step, nhi = nlo + step - 1;
    lo = nlo;
    if (nhi < hi) hi = nhi;
}
// rows mode: the starts are r * row_len, the first one >= base in closed form
SPL_HD uint64_t dd_first_doc_rows(const DecIn& a, uint64_t base) {
    const uint64_t d = (base + a.row_len - 1) / a.row_len;
    return d <= a.n_docs ? d : a.n_docs + 1;
}
// Either mode: the first document of the block whose slots begin at base.  lanes: the workgroup's size (DD_NT in the kernels; the host
// simulations run several); count(pred) = how many of those lanes hold pred(lane): one barrier in a kernel (WgCount of
// spl_k_merge.h), a loop over the lanes in a simulation, which also counts its calls -- the rounds.  Uniform: every lane of the
// workgroup calls it.
template <class Count>
SPL_HD uint64_t dd_first_doc(const DecIn& a, uint64_t base, uint32_t lanes, const Count& count) {
    if (a.row_len) return dd_first_doc_rows(a, base);
    uint64_t lo = 0, hi = a.n_docs + 1;
    while (lo < hi) {
        const uint64_t step = dd_kary_step(lo, hi, lanes);
        const uint32_t cnt = count([&](uint32_t lane) { return dd_kary_pred(a, lo, hi, step, lane, base); });
        dd_kary_narrow(lo, hi, step, cnt);
    }
    return lo;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// grid: one workgroup per block of DD_BLK slots, dd_n_blocks of them (beyond 2^31 - 1 blocks a workgroup takes several)
template <bool I64>
__global__ __launch_bounds__(DD_NT) void k_dec_len(DecIn a, DecTab t, uint64_t n_blk, uint64_t* __restrict__ blk) {
    __shared__ uint32_t s_w[DD_NT / 64];
    const uint64_t E = dd_end(a);
    for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint64_t base = b * DD_BLK;
        if (base >= E) {                                  // (uniform) wholly beyond the clamped end
            if (threadIdx.x == 0) blk[b] = 0;
            continue;
        }
        uint32_t len[DD_PER], src[DD_PER];
        const uint32_t x = wave_scan_incl(dd_lane_lens<I64>(a, t, base + (uint64_t)threadIdx.x * DD_PER, E, len, src));
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t sum = 0;
            for (uint32_t w = 0; w < DD_NT / 64; w++) sum += s_w[w];
            blk[b] = sum;
        }
        __syncthreads();                                  // (the next block of this workgroup fills s_w again)
    }
}

__device__ __forceinline__ void dd_store_group(uint8_t* p, const uint32_t w[DD_W / 4]) {
    if (DD_W == 16) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1 % (DD_W / 4)], w[2 % (DD_W / 4)], w[3 % (DD_W / 4)]);
    else *reinterpret_cast<uint32_t*>(p) = w[0];
}

// blk: the exclusive scan of k_dec_len's sums.  out (16-byte aligned) receives the bytes below cap, out_off all n_docs + 1 offsets.
// (tests/hostsim/decode_sim.cpp runs the mapping functions above and dd_first_doc with a count over its own lanes.  What it still
//  restates of this kernel: the in-block scan, the group loop and the document loop; a change to those here is checked by
//  tests/test_gpu_decode_device.py alone.)
template <bool I64>
__global__ __launch_bounds__(DD_NT) void k_dec_gather(DecIn a, DecTab t, uint64_t n_blk, const uint64_t* __restrict__ blk,
                                                      uint8_t* __restrict__ out, uint64_t cap, uint64_t* __restrict__ out_off) {
    __shared__ __attribute__((aligned(16))) uint32_t s_start[DD_BLK + 4];              // in-block starts, [DD_BLK] = the block's byte count
    __shared__ __attribute__((aligned(16))) uint32_t s_src[DD_BLK];                    // where a slot's bytes lie in tok_bytes
    __shared__ uint32_t s_w[DD_NT / 64];
    const uint64_t E = dd_end(a);
    const uint32_t tid = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint64_t base = b * DD_BLK;
        if (base > E) continue;                           // (uniform) no slot, no document, not even the end
        // the 1 024 lengths again, scanned
        uint32_t len[DD_PER], src[DD_PER];
        const uint32_t mine = dd_lane_lens<I64>(a, t, base + (uint64_t)tid * DD_PER, E, len, src);
        const uint32_t x = wave_scan_incl(mine);
        if ((tid & 63) == 63) s_w[tid >> 6] = x;
        __syncthreads();
        uint32_t st = x - mine;
        for (uint32_t w = 0; w < (tid >> 6); w++) st += s_w[w];
        *reinterpret_cast<uint4*>(&s_start[tid * DD_PER]) = make_uint4(st, st + len[0], st + len[0] + len[1], st + len[0] + len[1] + len[2]);
        *reinterpret_cast<uint4*>(&s_src[tid * DD_PER]) = make_uint4(src[0], src[1], src[2], src[3]);
        if (tid == DD_NT - 1) s_start[DD_BLK] = st + mine;
        __syncthreads();
        // the block's bytes, group by group
        const uint64_t b0 = blk[b], b1c = dd_cut(b0 + s_start[DD_BLK], cap);
        if (b1c > b0) {
            const uint64_t g_last = (b1c - 1) / DD_W;
            for (uint64_t g = b0 / DD_W + tid; g <= g_last; g += DD_NT) {
                uint64_t lo, hi;
                dd_group_range(g, b0, b1c, lo, hi);
                const uint32_t p = (uint32_t)(lo - b0), n = (uint32_t)(hi - lo);
                uint32_t w[DD_W / 4];
                dd_gather(s_start, s_src, t.tok_bytes, dd_owner(s_start, DD_BLK, p), p, n, w);
                if (dd_group_wide(lo, hi)) dd_store_group(out + lo, w);
                else for (uint32_t k = 0; k < n; k++) out[lo + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
        // the documents whose clamped start lies in this block's slots (the end, "document" n_docs, among them)
        const uint64_t first = dd_first_doc(a, base, DD_NT, WgCount{});
        for (uint64_t d = first + tid; d <= a.n_docs; d += DD_NT) {
            const uint64_t s = dd_doc_start(a, d);
            if (!dd_owns(s, base, DD_BLK)) break;         // (the starts are non-decreasing)
            out_off[d] = b0 + s_start[s - base];
        }
        __syncthreads();                                  // (the next block of this workgroup fills the LDS again)
    }
}
#endif  // __HIPCC__

}  // namespace spl
