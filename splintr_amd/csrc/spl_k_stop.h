// spl_k_stop.h -- spl_stop_match_device: STOP STRINGS for B streaming sequences at once.  Per sequence b the call is the
// pure function
//
//     (state_in[b], the new bytes of b, mask[b], final[b]) -> (the bytes that may leave now, hit[b], state_out[b])
//
// of the whole-text rule: T = every byte fed so far, S = the stops the mask selects (the table's slots, 1 .. 64 bytes each).  The first hit is
// the smallest end e at which some stop is a suffix of T[:e]; of the stops that end there the longest wins (start p), of equal ones the
// lowest slot; released is T[:p] (SP_INCLUDE: T[:e]) and the sequence is stopped for good.  Without a hit, released is T[:|T| - h], h the
// longest suffix of T that is a PROPER prefix of a stop (h <= 63): text that may still become a stop is held back, exactly as much as must be.
// Final (per sequence or for all), behind the call's bytes and without a hit: the held bytes leave, and the text is CLOSED -- the tail is
// emptied, so that nothing fed later can match into text already released (`released` goes on counting).  Nothing of this depends on
// where the steps cut T.
//
// The state row, SP_STATE_WORDS uint64 per sequence (all zero: fresh; every bit not named is 0, so rows compare bit for bit):
//     word 0      bits 0..6 tail_len     bits 8..14 held     bit 16 stopped     bits 24..29 the slot that hit
//     word 1      released: the bytes released so far; once stopped, where the text was cut
//     words 2..9  the tail: the last min(|T|, 63) bytes of T (of T[:e] once stopped), the first byte lowest, zero from tail_len on
//
// A WAVEFRONT owns a sequence (and strides over the sequences of its workgroup).  Its stream is W = the tail + the new bytes; position
// L0 - held of W is where the released text ends.  W's new bytes are walked in chunks of 64 END positions, one a lane, each chunk staged in
// LDS with SP_H = 63 bytes in front of it, so that a 64-byte stop may straddle any chunk or step edge.  For every live slot (a uniform loop
// over the mask's bits) a lane compares backwards from its end position -- the stop's last byte first, and the slot is skipped where the
// ballot of that is empty -- and keeps the longest match; a ballot and a count of trailing zeros give the smallest end, and the walk ends
// at the first chunk with a hit.  Without a hit lane k (1 .. 63) asks whether the last k bytes of W begin a live stop longer than k: the
// highest set bit of that ballot is h.  The table (4 160 bytes) is copied into LDS once per workgroup.
//
// The driver around a sequence is spl_k_seqscan.h's: one launch (k_stop_one) up to the handle's "stop_one_max" sequences (SP_ONE_DEFAULT), three
// beyond (k_stop_len, k_decode_scan, k_stop_write).  The count pass finds cut and hit and hands them to the write pass, which only copies:
// through LDS (a u64 and a u32 per sequence) or through the scratch (two u64).  The write pass alone writes state_out and hit, by a
// wavefront that has read state_in[b] before: the two may be one array.
//
// The first half is plain C++ (values and pointers only): tests/hostsim/stop_sim.cpp includes it in a g++ build and evaluates it sequence by
// sequence and lane by lane with a run-time lane count and chunk size; the kernels call exactly these functions.
#pragma once
#include "spl_common.h"
#include "spl_k_seqscan.h"

#ifndef SPL_STOP_HALO
#define SPL_STOP_HALO 63               /* bytes staged in front of a chunk: the longest stop less one (tests/hostsim builds a mutant with 62) */
#endif
#ifndef SPL_STOP_ONE_DEFAULT
#define SPL_STOP_ONE_DEFAULT 64        /* sequences up to which a call takes the one-launch form.  Measured (profiles/stop_match.txt, K = 1, 8 stops): one launch 8.5 / 14.3 / 19.9 / 25.8 / 31.6 / 49.3 us at 16 / 32 / 48 / 64 / 80 / 128 sequences, three launches 24.8 / 25.9 / 26.1 / 26.1 / 26.1 / 26.3 us: the medians cross between 64 and 80 */
#endif

namespace spl {

// (the values of SPL_STOP_* in include/splintr_hip.h)
constexpr uint32_t SP_INCLUDE = 1u, SP_FINAL_ALL = 2u;
constexpr uint32_t SP_SLOTS = 64, SP_MAX_LEN = 64, SP_TABLE_BYTES = 64 * 64 + 64, SP_STATE_WORDS = 10;
constexpr uint32_t SP_TAIL_MAX = SP_MAX_LEN - 1;     // bytes of T a sequence keeps: what a stop that ends in a later step can reach back
constexpr uint32_t SP_H = SPL_STOP_HALO;
constexpr uint32_t SP_WAVE = 64;                     // lanes of a wavefront: end positions of a chunk
constexpr uint32_t SP_NT = SEQ_NT, SP_ONE_NT = SEQ_ONE_NT;     // the driver's workgroups (spl_k_seqscan.h)
constexpr uint32_t SP_ONE_MAX = SEQ_ONE_MAX;         // most sequences the one-launch form can take (cut and hit are in LDS too); option "stop_one_max"
constexpr uint32_t SP_ONE_DEFAULT = SPL_STOP_ONE_DEFAULT;
static_assert(SP_ONE_DEFAULT <= SP_ONE_MAX, "the default threshold is one the kernel can take");
static_assert(SP_H <= SP_TAIL_MAX && SP_TAIL_MAX < SP_WAVE, "lane k holds the suffix of k bytes; the tail fits eight words");

struct SpIn {
    const uint8_t* in; uint64_t in_cap; const uint64_t* in_off; uint64_t n_seqs;
    const uint8_t* table; const uint64_t* mask; const uint8_t* fin; uint32_t flags; const uint64_t* state_in;
};

// ------------------------------------------------------------------------------------------ the state row
SPL_HD uint32_t sp_tail_len(uint64_t w0) { return (uint32_t)w0 & 0x7Fu; }
SPL_HD uint32_t sp_held(uint64_t w0) { return (uint32_t)(w0 >> 8) & 0x7Fu; }
SPL_HD bool sp_stopped(uint64_t w0) { return ((w0 >> 16) & 1u) != 0; }
SPL_HD uint32_t sp_slot(uint64_t w0) { return (uint32_t)(w0 >> 24) & 0x3Fu; }
SPL_HD uint64_t sp_word0(uint32_t tail_len, uint32_t held, bool stopped, uint32_t slot) {
    return (uint64_t)(tail_len & 0x7Fu) | ((uint64_t)(held & 0x7Fu) << 8) | ((uint64_t)(stopped ? 1u : 0u) << 16) | ((uint64_t)(stopped ? slot & 0x3Fu : 0u) << 24);
}
SPL_HD int32_t sp_hit_of(uint64_t w0) { return sp_stopped(w0) ? (int32_t)sp_slot(w0) : -1; }

// ------------------------------------------------------------------------------------------ the table
// slot s: bytes [64 s, 64 s + len[s]), the lengths behind the 64 slots; a length of 0 or above 64: the slot never matches
SPL_HD uint32_t sp_len(const uint8_t* tab, uint32_t s) { const uint32_t l = tab[SP_SLOTS * SP_MAX_LEN + s]; return l > SP_MAX_LEN ? 0u : l; }
SPL_HD bool sp_slot_live(const uint8_t* tab, uint64_t mask, uint32_t s) { return s < SP_SLOTS && ((mask >> s) & 1ull) && sp_len(tab, s) != 0; }

// ------------------------------------------------------------------------------------------ one sequence's call
struct SpSeq {
    uint64_t released, lo, m, n, mask;     // lo, m: where its new bytes lie in `in` and how many; n = L0 + m: the length of W
    uint32_t L0, h0, slot;                 // tail_len and held of state_in
    bool stopped, fin, idle;               // idle: the row stays as it is, bit for bit, and nothing leaves
};
// (an offset above in_cap counts as in_cap: an overflowed producer's convention; bytes beyond it are not read)
SPL_HD SpSeq sp_open(const SpIn& a, uint64_t b, uint64_t w0, uint64_t w1) {
    SpSeq q;
    const uint64_t x = a.in_off[b], y = a.in_off[b + 1];
    q.lo = x < a.in_cap ? x : a.in_cap;
    const uint64_t hi = y < a.in_cap ? y : a.in_cap;
    q.m = hi > q.lo ? hi - q.lo : 0;
    q.L0 = sp_tail_len(w0); q.h0 = sp_held(w0); q.slot = sp_slot(w0); q.stopped = sp_stopped(w0);
    if (q.L0 > SP_TAIL_MAX) q.L0 = SP_TAIL_MAX;            // (a row that is no state: stay inside the row)
    if (q.h0 > q.L0) q.h0 = q.L0;
    q.released = w1;
    q.n = q.L0 + q.m;
    q.mask = a.mask ? a.mask[b] : ~0ull;
    q.fin = (a.flags & SP_FINAL_ALL) || (a.fin && a.fin[b]);
    q.idle = q.stopped || (q.m == 0 && !q.fin);
    return q;
}
// byte q of W
SPL_HD uint32_t sp_w(const uint8_t* tail, uint32_t L0, const uint8_t* in, uint64_t lo, uint64_t q) { return q < L0 ? tail[q] : in[lo + (q - L0)]; }

// ------------------------------------------------------------------------------------------ chunks, the compare, the tie
// entry j (0 .. chunk + SP_H) of the staging area of the chunk whose first end byte is W[base] is W[base + j - SP_H]
SPL_HD bool sp_stage_pos(uint64_t base, uint32_t j, uint64_t n, uint64_t& q) {
    q = base + j - SP_H;
    return base + j >= SP_H && q < n;
}
// bytes that lie at or in front of a lane's end byte, W[base + lane], as far as the staging area shows them
SPL_HD uint32_t sp_avail(uint64_t base, uint32_t lane) {
    const uint64_t all = base + lane + 1, staged = (uint64_t)SP_H + lane + 1;
    return (uint32_t)(all < staged ? all : staged);
}
// the stop's last byte against the end byte (stage[at]): most positions are rejected here
SPL_HD bool sp_last_eq(const uint8_t* stage, uint32_t at, const uint8_t* tab, uint32_t s, uint32_t l) { return stage[at] == tab[SP_MAX_LEN * s + l - 1]; }
SPL_HD bool sp_match(const uint8_t* stage, uint32_t at, uint32_t avail, const uint8_t* tab, uint32_t s, uint32_t l) {
    if (l == 0 || l > avail) return false;
    const uint8_t* k = tab + SP_MAX_LEN * s;
    for (uint32_t i = 0; i < l; i++)
        if (stage[at - i] != k[l - 1 - i]) return false;
    return true;
}
// a match of l bytes against the best so far (0: none), the slots taken in rising order: the longest wins, of equal ones the first
SPL_HD bool sp_better(uint32_t best_l, uint32_t l) {
#ifdef SPL_STOP_MUTANT_SHORTEST
    return best_l == 0 || l < best_l;
#else
    return l > best_l;
#endif
}
// hold-back: nt = the last tl bytes of W; are its last k a proper prefix of stop s (l bytes)?
SPL_HD bool sp_hold_first(const uint8_t* nt, uint32_t tl, uint32_t k, const uint8_t* tab, uint32_t s, uint32_t l) {
    return k >= 1 && k <= tl && k < l && nt[tl - k] == tab[SP_MAX_LEN * s];
}
SPL_HD bool sp_hold(const uint8_t* nt, uint32_t tl, uint32_t k, const uint8_t* tab, uint32_t s, uint32_t l) {
    if (k == 0 || k > tl || k >= l) return false;
    const uint8_t* key = tab + SP_MAX_LEN * s;
    for (uint32_t i = 0; i < k; i++)
        if (nt[tl - k + i] != key[i]) return false;
    return true;
}

// ------------------------------------------------------------------------------------------ what the find pass hands to the write pass
// cut: the position of W where the released text ends after this call; info: bit 0 hit, bits 8..13 the slot, bits 16..22 its length,
// bits 24..30 held
SPL_HD uint32_t sp_info(bool hit, uint32_t slot, uint32_t len, uint32_t held) { return (hit ? 1u : 0u) | (slot << 8) | (len << 16) | (held << 24); }
SPL_HD bool sp_info_hit(uint32_t i) { return (i & 1u) != 0; }
SPL_HD uint32_t sp_info_slot(uint32_t i) { return (i >> 8) & 0x3Fu; }
SPL_HD uint32_t sp_info_len(uint32_t i) { return (i >> 16) & 0x7Fu; }
SPL_HD uint32_t sp_info_held(uint32_t i) { return (i >> 24) & 0x7Fu; }
SPL_HD uint64_t sp_cut_hit(uint32_t flags, uint64_t e, uint32_t l) { return (flags & SP_INCLUDE) ? e : e - l; }
SPL_HD uint64_t sp_end_hit(uint32_t flags, uint64_t cut, uint32_t l) { return (flags & SP_INCLUDE) ? cut : cut + l; }
// the bytes that leave: W[L0 - h0, cut) (the released text never shrinks; a mask that changed under a live sequence could ask for it)
SPL_HD uint64_t sp_count(const SpSeq& q, uint64_t cut) { const uint64_t r0 = q.L0 - q.h0; return cut > r0 ? cut - r0 : 0; }
// the tail the sequence keeps: of W[:end], end = the hit's end or n; none once the text is closed by a final without a hit
SPL_HD uint32_t sp_new_tail_len(bool hit, bool fin, uint64_t end) { return !hit && fin ? 0u : (uint32_t)(end < SP_TAIL_MAX ? end : SP_TAIL_MAX); }
SPL_HD uint64_t sp_new_word0(const SpSeq& q, uint32_t info, uint32_t tl) {
    const bool hit = sp_info_hit(info);
    return sp_word0(tl, hit || q.fin ? 0u : sp_info_held(info), hit, sp_info_slot(info));
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ one sequence, one wavefront
struct SpWave {
    uint64_t row[SP_STATE_WORDS];      // state_in's row; the bytes of row[2 ..] are the tail
    uint64_t nt[8];                    // the last bytes of W: what the hold-back looks at, and the tail that is kept
    uint8_t stage[SP_WAVE + 64];       // a chunk and the SP_H bytes in front of it
};

// the table into LDS, once per workgroup
__device__ __forceinline__ void sp_load_table(const uint8_t* __restrict__ table, uint8_t* s_tab) {
    if ((reinterpret_cast<uintptr_t>(table) & 15u) == 0) {
        for (uint32_t i = threadIdx.x; i < SP_TABLE_BYTES / 16; i += blockDim.x)
            reinterpret_cast<uint4*>(s_tab)[i] = reinterpret_cast<const uint4*>(table)[i];
    } else {
        for (uint32_t i = threadIdx.x; i < SP_TABLE_BYTES; i += blockDim.x) s_tab[i] = table[i];
    }
}

__device__ __forceinline__ SpSeq sp_load_row(const SpIn& a, uint64_t b, SpWave& L) {
    const uint32_t lane = threadIdx.x & 63;
    if (lane < SP_STATE_WORDS) L.row[lane] = a.state_in[b * SP_STATE_WORDS + lane];
    wave_lds_sync();
    return sp_open(a, b, L.row[0], L.row[1]);
}

// Sequence b's cut and info; returns the bytes it emits.  Every lane of the wavefront calls it.
__device__ __forceinline__ uint64_t sp_find(const SpIn& a, const uint8_t* tab, uint64_t b, SpWave& L, uint64_t& cut, uint32_t& info) {
    const uint32_t lane = threadIdx.x & 63;
    const SpSeq q = sp_load_row(a, b, L);
    cut = q.L0 - q.h0; info = 0;
    if (q.idle) { wave_lds_sync(); return 0; }                 // (uniform)
    const uint8_t* tail = reinterpret_cast<const uint8_t*>(&L.row[2]);
    const uint64_t live = __ballot(sp_slot_live(tab, q.mask, lane));
    bool found = false;
    for (uint64_t p0 = 0; p0 < q.m; p0 += SP_WAVE) {
        const uint64_t base = q.L0 + p0;
        for (uint32_t j = lane; j < SP_WAVE + SP_H; j += SP_WAVE) {
            uint64_t w;
            L.stage[j] = sp_stage_pos(base, j, q.n, w) ? (uint8_t)sp_w(tail, q.L0, a.in, q.lo, w) : (uint8_t)0;
        }
        wave_lds_sync();
        const bool active = base + lane < q.n;
        const uint32_t at = SP_H + lane, avail = sp_avail(base, lane);
        uint32_t best_l = 0, best_s = 0;
        for (uint64_t mm = live; mm; mm &= mm - 1) {           // (uniform: the mask's live slots in rising order)
            const uint32_t s = (uint32_t)__builtin_ctzll(mm), l = sp_len(tab, s);
            const bool c = active && sp_last_eq(L.stage, at, tab, s, l);
            if (!__ballot(c)) continue;
            if (c && sp_better(best_l, l) && sp_match(L.stage, at, avail, tab, s, l)) { best_l = l; best_s = s; }
        }
        const uint64_t hits = __ballot(best_l != 0);
        wave_lds_sync();                                       // (the next chunk fills the staging area again)
        if (hits) {
            const int f = __builtin_ctzll(hits);
            const uint32_t l = (uint32_t)__shfl((int)best_l, f), s = (uint32_t)__shfl((int)best_s, f);
            cut = sp_cut_hit(a.flags, base + (uint32_t)f + 1, l);
            info = sp_info(true, s, l, 0);
            found = true;
            break;
        }
    }
    if (!found) {
        uint32_t h = 0;
        if (!q.fin) {
            const uint32_t tl = sp_new_tail_len(false, false, q.n);
            uint8_t* nt = reinterpret_cast<uint8_t*>(L.nt);
            if (lane < tl) nt[lane] = (uint8_t)sp_w(tail, q.L0, a.in, q.lo, q.n - tl + lane);
            wave_lds_sync();
            bool mine = false;                                  // lane k: the last k bytes of W begin a live stop longer than k
            for (uint64_t mm = live; mm; mm &= mm - 1) {
                const uint32_t s = (uint32_t)__builtin_ctzll(mm), l = sp_len(tab, s);
                const bool c = !mine && sp_hold_first(nt, tl, lane, tab, s, l);
                if (!__ballot(c)) continue;
                if (c) mine = sp_hold(nt, tl, lane, tab, s, l);
            }
            const uint64_t hb = __ballot(mine);
            h = hb ? 63u - (uint32_t)__builtin_clzll(hb) : 0u;
            wave_lds_sync();
        }
        cut = q.n - h;
        info = sp_info(false, 0, 0, h);
    }
    return sp_count(q, cut);
}

// Sequence b's bytes from o0 on, its hit and its state row, from the cut and info sp_find gave.  Every lane of the wavefront calls it.
__device__ __forceinline__ void sp_emit(const SpIn& a, uint64_t b, SpWave& L, uint64_t cut, uint32_t info, uint8_t* __restrict__ out, uint64_t cap,
                                        uint64_t o0, uint64_t* __restrict__ state_out, int32_t* __restrict__ hit_out) {
    const uint32_t lane = threadIdx.x & 63;
    const SpSeq q = sp_load_row(a, b, L);
    uint64_t* row_out = state_out + b * SP_STATE_WORDS;
    if (q.idle) {                                               // (uniform) the row as it is
        if (lane < SP_STATE_WORDS) row_out[lane] = L.row[lane];
        if (lane == 0) hit_out[b] = sp_hit_of(L.row[0]);
        wave_lds_sync();
        return;
    }
    const uint8_t* tail = reinterpret_cast<const uint8_t*>(&L.row[2]);
    const uint64_t count = sp_count(q, cut), r0 = q.L0 - q.h0;
    for (uint64_t i = lane; i < count; i += SP_WAVE) seq_put(out, cap, o0 + i, sp_w(tail, q.L0, a.in, q.lo, r0 + i));
    const bool hit = sp_info_hit(info);
    const uint64_t end = hit ? sp_end_hit(a.flags, cut, sp_info_len(info)) : q.n;
    const uint32_t tl = sp_new_tail_len(hit, q.fin, end);
    uint8_t* nt = reinterpret_cast<uint8_t*>(L.nt);
    nt[lane] = lane < tl ? (uint8_t)sp_w(tail, q.L0, a.in, q.lo, end - tl + lane) : (uint8_t)0;
    wave_lds_sync();
    if (lane == 0) { row_out[0] = sp_new_word0(q, info, tl); hit_out[b] = hit ? (int32_t)sp_info_slot(info) : -1; }
    else if (lane == 1) row_out[1] = q.released + count;
    else if (lane < SP_STATE_WORDS) row_out[lane] = L.nt[lane - 2];
    wave_lds_sync();
}

// ------------------------------------------------------------------------------------------ the op and its kernels (spl_k_seqscan.h)
struct SpCarry { uint64_t cut; uint32_t info; };
template <class C, class I>
struct SpKeep {
    C* cut; I* inf;
    __device__ __forceinline__ void put(uint64_t b, const SpCarry& k) const { cut[b] = k.cut; inf[b] = k.info; }
    __device__ __forceinline__ SpCarry get(uint64_t b) const { return {cut[b], (uint32_t)inf[b]}; }
};
struct SpOp {
    using Wave = SpWave;
    using Carry = SpCarry;
    const SpIn& a; const uint8_t* tab; uint8_t* out; uint64_t cap; uint64_t* state_out; int32_t* hit_out;
    __device__ __forceinline__ uint64_t count(uint64_t b, SpWave& L, SpCarry& k) const { return sp_find(a, tab, b, L, k.cut, k.info); }
    __device__ __forceinline__ void write(uint64_t b, SpWave& L, const SpCarry& k, uint64_t o0) const { sp_emit(a, b, L, k.cut, k.info, out, cap, o0, state_out, hit_out); }
};

// cut[b], inf[b]: where sequence b is cut, behind the driver's cnt[b]
__global__ __launch_bounds__(SP_NT) void k_stop_len(SpIn a, uint64_t n_blk, uint64_t* __restrict__ cnt, uint64_t* __restrict__ cut,
                                                    uint64_t* __restrict__ inf, uint64_t* __restrict__ blk) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[SP_TABLE_BYTES];
    __shared__ SpWave s_wave[SP_NT / 64];
    __shared__ uint64_t s_sum[SP_NT / 64];
    sp_load_table(a.table, s_tab);
    __syncthreads();
    seq_len_body(SpOp{a, s_tab, nullptr, 0, nullptr, nullptr}, SpKeep<uint64_t, uint64_t>{cut, inf}, a.n_seqs, n_blk, s_wave, s_sum, cnt, blk);
}
__global__ __launch_bounds__(SP_NT) void k_stop_write(SpIn a, uint64_t n_blk, const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ cut,
                                                      const uint64_t* __restrict__ inf, const uint64_t* __restrict__ blk,
                                                      uint8_t* __restrict__ out, uint64_t cap, uint64_t* __restrict__ out_off,
                                                      uint64_t* __restrict__ state_out, int32_t* __restrict__ hit_out) {
    __shared__ SpWave s_wave[SP_NT / 64];
    seq_write_body(SpOp{a, nullptr, out, cap, state_out, hit_out}, SpKeep<const uint64_t, const uint64_t>{cut, inf}, a.n_seqs, n_blk, s_wave, cnt, blk, out_off);
}
__global__ __launch_bounds__(SP_ONE_NT) void k_stop_one(SpIn a, uint8_t* __restrict__ out, uint64_t cap, uint64_t* __restrict__ out_off,
                                                        uint64_t* __restrict__ state_out, int32_t* __restrict__ hit_out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[SP_TABLE_BYTES];
    __shared__ SpWave s_wave[SP_ONE_NT / 64];
    __shared__ uint64_t s_cnt[SP_ONE_MAX + 1];
    __shared__ uint64_t s_cut[SP_ONE_MAX];
    __shared__ uint32_t s_inf[SP_ONE_MAX];
    sp_load_table(a.table, s_tab);
    __syncthreads();
    seq_one_body(SpOp{a, s_tab, out, cap, state_out, hit_out}, SpKeep<uint64_t, uint32_t>{s_cut, s_inf}, (uint32_t)a.n_seqs, s_wave, s_cnt, out_off);
}
#endif  // __HIPCC__

}  // namespace spl
