// spl_k_stream.h -- spl_stream_decode_device: ONE STEP of B streaming decoders at once.  Per sequence b the call is the
// pure function
//
//     (state_in[b], ids[b, 0 .. K), len[b]) -> (the bytes that may leave now, state_out[b])
//
// of the reference's StreamingDecoder / ByteLevelStreamingDecoder (src/core/streaming.rs; find_valid_utf8_len and is_incomplete_utf8 of
// src/python/bindings.rs:591-640): token bytes go behind what is pending and only complete UTF-8 characters leave.  What the reference keeps
// in its buffer is either at most three bytes of an unfinished character or a buffer that can never emit again, so one word holds it:
//
//     bits 0..23  the pending bytes, first byte lowest      bits 24..25  their count      bit 26  stalled      bits 32..63  held
//
// (every other bit 0; a word of 0 is a fresh decoder).  The stream of a sequence is S = pending bytes + the bytes the device decode emits for
// the row's valid slots (spl_k_decode_dev.h: dd_id_span).  Hold mode (the reference): emit the longest valid prefix of S; what is left is
// nothing (state 0), the well-formed beginning of ONE character that reaches the end of S (pending), or anything else: the sequence STALLS
// (held = bytes left; from then on held only grows, saturating).  Replace mode: S is cut into units -- an ASCII byte; a lead with the
// continuation bytes that conform to its row of the Unicode table (all of them: a character, copied; the end of S first: pending; a
// non-conforming byte first: one maximal invalid subpart, EF BF BD); any other byte (EF BF BD) -- which is what Python's incremental
// decoder with errors="replace" emits.  Final (per sequence or for all): a non-stalled sequence's pending bytes leave as one EF BF BD.
//
// The cut is LOCAL: a lead always starts a unit, and a continuation byte at p is consumed iff some k in 1 .. 3 has a lead at p - k that
// wants at least k continuations and bytes p - k + 1 .. p conform to it.  So the role of a byte follows from ST_H = 3 bytes either side.
//
// A WAVEFRONT owns a sequence (and strides over the sequences of its workgroup).  It takes the row in windows of 64 slots -- one slot a
// lane, lengths scanned into LDS, slot 0 the pending bytes -- and a window's stream in chunks of 64 bytes staged in LDS with a halo of ST_H
// bytes on both sides (a byte finds its slot by dd_owner over the starts), so a character, or a 300-byte key, may straddle any chunk edge.
// A ballot gives the roles; hold mode takes the first non-copy position (count of trailing zeros), replace mode scans the per-byte output
// lengths {0, 1, 3}.  Between windows the carry is the state word itself: feeding a decoder window by window is feeding it step by step.
//
// The driver around a sequence is spl_k_seqscan.h's: one launch (k_stream_one) up to the handle's "stream_one_max" sequences (ST_ONE_DEFAULT),
// three beyond (k_stream_len, k_decode_scan, k_stream_write); the count hands the write nothing.  The write pass alone writes state_out, by
// a wavefront that has read state_in[b] before: the two may be one array.
//
// The first half is plain C++ (values and pointers only): tests/hostsim/stream_sim.cpp includes it in a g++ build and evaluates it sequence
// by sequence and lane by lane with a run-time window and chunk size; the kernels call exactly these functions.
#pragma once
#include "spl_common.h"
#include "spl_k_decode_dev.h"
#include "spl_k_seqscan.h"

#ifndef SPL_STREAM_HALO
#define SPL_STREAM_HALO 3              /* bytes either side of a byte that decide its role (tests/hostsim builds a mutant with 2) */
#endif
#ifndef SPL_STREAM_ONE_DEFAULT
#define SPL_STREAM_ONE_DEFAULT 64      /* sequences up to which a call takes the one-launch form.  Measured (profiles/stream_decode.txt, K = 1): one launch 7.1 / 11.5 / 20.6 / 25.2 / 38.5 us at 16 / 32 / 64 / 80 / 128 sequences, three launches 23.2 / 23.7 / 24.9 / 24.9 / 25.0 us: the medians cross between 64 and 80 */
#endif

namespace spl {

// (the values of SPL_STREAM_* in include/splintr_hip.h)
constexpr uint32_t ST_REPLACE = 1u, ST_FINAL_ALL = 2u;
constexpr uint32_t ST_H = SPL_STREAM_HALO;
constexpr uint32_t ST_WAVE = 64;                    // lanes of a wavefront: slots of a window, bytes of a chunk
constexpr uint32_t ST_NT = SEQ_NT, ST_ONE_NT = SEQ_ONE_NT;     // the driver's workgroups (spl_k_seqscan.h)
constexpr uint32_t ST_ONE_MAX = SEQ_ONE_MAX;        // most sequences the one-launch form can take; option "stream_one_max"
constexpr uint32_t ST_ONE_DEFAULT = SPL_STREAM_ONE_DEFAULT;
static_assert(ST_ONE_DEFAULT <= ST_ONE_MAX, "the default threshold is one the kernel can take");
static_assert(ST_H >= 1 && ST_H <= 3, "a role looks at most three bytes either way");

struct StIn {
    const void* ids; const int32_t* len; const uint8_t* fin; const uint64_t* state_in;
    uint64_t n_seqs; uint32_t row_len, dflags, sflags;
};

// ------------------------------------------------------------------------------------------ the state word
constexpr uint64_t ST_STALLED = 1ull << 26;
SPL_HD uint32_t st_count(uint64_t s) { return (uint32_t)(s >> 24) & 3u; }
SPL_HD uint32_t st_pend(uint64_t s) { return (uint32_t)s & 0xFFFFFFu; }
SPL_HD bool st_stalled(uint64_t s) { return (s & ST_STALLED) != 0; }
SPL_HD uint64_t st_held(uint64_t s) { return s >> 32; }
SPL_HD uint64_t st_make_stalled(uint64_t held) { return ST_STALLED | ((held > 0xFFFFFFFFull ? 0xFFFFFFFFull : held) << 32); }
SPL_HD uint64_t st_add_held(uint64_t s, uint64_t more) { return st_make_stalled(st_held(s) + more); }
// n (1 .. 3) pending bytes, the first one lowest in `bytes`
SPL_HD uint64_t st_make_pending(uint32_t bytes, uint32_t n) {
    if (n > 3) n = 3;
    return (uint64_t)(bytes & (0xFFFFFFu >> (8 * (3 - n)))) | ((uint64_t)n << 24);
}

// ------------------------------------------------------------------------------------------ the Unicode table (Table 3-7)
// continuation bytes a lead wants (0: not a lead -- C0, C1 and F5 .. FF never are)
SPL_HD uint32_t st_want(uint32_t x) { return x < 0xC2 ? 0u : x <= 0xDF ? 1u : x <= 0xEF ? 2u : x <= 0xF4 ? 3u : 0u; }
// byte x as the k-th (1 ..) byte behind `lead`: 80 .. BF, the second byte narrowed after E0, ED, F0 and F4
SPL_HD bool st_conf(uint32_t lead, uint32_t k, uint32_t x) {
    uint32_t lo = 0x80, hi = 0xBF;
#ifndef SPL_STREAM_MUTANT_WIDE_SECOND
    if (k == 1) {
        if (lead == 0xE0) lo = 0xA0; else if (lead == 0xED) hi = 0x9F; else if (lead == 0xF0) lo = 0x90; else if (lead == 0xF4) hi = 0x8F;
    }
#endif
    return x >= lo && x <= hi;
}

// ------------------------------------------------------------------------------------------ the role of one byte
// The neighbourhood of position p: byte p + rel (rel = -ST_H .. ST_H) is byte rel + ST_H of w, and bit rel + ST_H of `have` says that the
// position lies inside S.  A position outside the neighbourhood counts as outside S.
constexpr uint32_t ST_ABSENT = 0x100;
SPL_HD uint32_t st_at(uint64_t w, uint32_t have, int rel) {
    const int i = rel + (int)ST_H;
    if (i < 0 || i > 2 * (int)ST_H || !((have >> i) & 1u)) return ST_ABSENT;
    return (uint32_t)(w >> (8 * i)) & 0xFFu;
}
// a lead at rel: 2 every continuation is there and conforms (a character), 1 S ends first (unfinished), 0 a non-conforming byte first
SPL_HD uint32_t st_lead(uint64_t w, uint32_t have, int rel, uint32_t lead) {
    const uint32_t want = st_want(lead);
    for (uint32_t k = 1; k <= want; k++) {
        const uint32_t x = st_at(w, have, rel + (int)k);
        if (x == ST_ABSENT) return 1u;
        if (!st_conf(lead, k, x)) return 0u;
    }
    return 2u;
}
// roles: the low two bits are the bytes the position emits in replace mode
constexpr uint32_t ST_R_TAIL = 0;     // consumed by a lead that is no character: emits nothing, starts nothing
constexpr uint32_t ST_R_COPY = 1;     // an ASCII byte, or a byte of a complete character
constexpr uint32_t ST_R_BAD = 3;      // starts a maximal invalid subpart: EF BF BD; hold mode stalls here
constexpr uint32_t ST_R_PEND = 4;     // the lead of the unfinished character S ends with: pending from here on
SPL_HD uint32_t st_role(uint64_t w, uint32_t have) {
    const uint32_t x = st_at(w, have, 0);
    if (x < 0x80) return ST_R_COPY;
    if (st_want(x)) {
        const uint32_t s = st_lead(w, have, 0, x);
        return s == 2 ? ST_R_COPY : s == 1 ? ST_R_PEND : ST_R_BAD;
    }
    if (x > 0xBF) return ST_R_BAD;                       // C0, C1, F5 .. FF
    for (int k = 1; k <= 3; k++) {                        // a continuation byte: the lead that consumes it, if any
        const uint32_t y = st_at(w, have, -k);
        if (y == ST_ABSENT) break;
        const uint32_t want = st_want(y);
        if (want) {
            bool mine = want >= (uint32_t)k;
            for (int j = 1; j <= k && mine; j++) mine = st_conf(y, (uint32_t)j, st_at(w, have, -k + j));
            if (!mine) break;
            return st_lead(w, have, -k, y) == 2 ? ST_R_COPY : ST_R_TAIL;
        }
        if (y < 0x80 || y > 0xBF) break;
    }
    return ST_R_BAD;
}
// the state a sequence is left in by the FIRST position hold mode does not copy (role r, `rest` bytes from it to the end of S), or by the
// ST_R_PEND position of replace mode
SPL_HD uint64_t st_state_at(uint32_t r, uint64_t w, uint32_t rest) {
    return r == ST_R_PEND ? st_make_pending((uint32_t)(w >> (8 * ST_H)), rest) : st_make_stalled(rest);
}

// ------------------------------------------------------------------------------------------ slots, bytes, chunks
SPL_HD uint32_t st_row_valid(const StIn& a, uint64_t b) {
    if (!a.len) return a.row_len;
    const int32_t l = a.len[b];
    return l < 0 ? 0u : ((uint32_t)l > a.row_len ? a.row_len : (uint32_t)l);
}
template <bool I64>
SPL_HD uint32_t st_slot_span(const StIn& a, const DecTab& t, uint64_t b, uint32_t k, uint32_t& src) {
    const uint64_t i = b * a.row_len + k;
    if (I64) return dd_id64_span(t, a.dflags, static_cast<const uint64_t*>(a.ids)[i], src);
    return dd_id_span(t, a.dflags, static_cast<const uint32_t*>(a.ids)[i], src);
}
// byte q of a window's stream.  starts[0 .. n_slots]: slot 0 is the pending bytes (start 0), slots 1 .. the window's ids, starts[n_slots] =
// the stream's length; src[i]: where slot i's bytes lie in tok_bytes.
SPL_HD uint32_t st_fetch(const uint32_t* starts, const uint32_t* src, const uint8_t* tok_bytes, uint32_t n_slots, uint32_t pend, uint32_t q) {
    const uint32_t i = dd_owner(starts, n_slots, q);
    if (i == 0) return (pend >> (8 * q)) & 0xFFu;
    return tok_bytes[src[i] + (q - starts[i])];
}
// entry j (0 .. chunk + 2 ST_H) of a chunk's staging area is position p0 + j - ST_H
SPL_HD bool st_stage_pos(uint32_t p0, uint32_t j, uint32_t n, uint32_t& q) {
    q = p0 + j - ST_H;
    return p0 + j >= ST_H && q < n;
}
// the neighbourhood of position p0 + lane from the staging area
SPL_HD uint32_t st_nbr(const uint8_t* stage, uint32_t lane, uint32_t p0, uint32_t n, uint64_t& w) {
    uint32_t have = 0;
    w = 0;
    for (uint32_t i = 0; i <= 2 * ST_H; i++) {
        uint32_t q;
        if (!st_stage_pos(p0, lane + i, n, q)) continue;
        have |= 1u << i;
        w |= (uint64_t)stage[lane + i] << (8 * i);
    }
    return have;
}
SPL_HD bool st_final(const StIn& a, uint64_t b) { return (a.sflags & ST_FINAL_ALL) || (a.fin && a.fin[b]); }

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ one sequence, one wavefront
struct StWave {
    uint32_t start[ST_WAVE + 4];       // [0] the pending bytes' start (0), [1 .. 64] the window's slots, [65] the stream's length
    uint32_t src[ST_WAVE + 4];
    uint8_t byte[ST_WAVE + 16];        // a chunk and its two halos
};

// The bytes sequence b emits, counted (WRITE false) or written from o0 on, with its state word.  Every lane of the wavefront calls it.
template <bool I64, bool WRITE>
__device__ __forceinline__ uint64_t st_seq(const StIn& a, const DecTab& t, uint64_t b, StWave& L, uint8_t* __restrict__ out, uint64_t cap,
                                           uint64_t o0, uint64_t* __restrict__ state_out) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t state = a.state_in[b];
    const uint32_t n_valid = st_row_valid(a, b);
    const bool replace = (a.sflags & ST_REPLACE) != 0;
    uint64_t o = o0;
    for (uint64_t k0 = 0; k0 < n_valid; k0 += ST_WAVE) {
        uint32_t len = 0, src = 0;
        if (k0 + lane < n_valid) len = st_slot_span<I64>(a, t, b, (uint32_t)(k0 + lane), src);
        const uint32_t incl = wave_scan_incl(len), total = (uint32_t)__shfl((int)incl, 63);
        if (total == 0) continue;                          // (uniform) the state stays as it is, bit for bit
        if (st_stalled(state)) { state = st_add_held(state, total); continue; }
        const uint32_t c = st_count(state), pend = st_pend(state), n = c + total;
        if (lane == 0) L.start[0] = 0;
        L.start[1 + lane] = c + incl - len;
        L.src[1 + lane] = src;
        if (lane == 63) L.start[ST_WAVE + 1] = n;
        wave_lds_sync();
        uint64_t next = 0;
        for (uint32_t p0 = 0; p0 < n; p0 += ST_WAVE) {
            for (uint32_t j = lane; j < ST_WAVE + 2 * ST_H; j += ST_WAVE) {
                uint32_t q;
                L.byte[j] = st_stage_pos(p0, j, n, q) ? (uint8_t)st_fetch(L.start, L.src, t.tok_bytes, ST_WAVE + 1, pend, q) : (uint8_t)0;
            }
            wave_lds_sync();
            uint64_t w;
            const uint32_t have = st_nbr(L.byte, lane, p0, n, w);
            const bool active = p0 + lane < n;
            const uint32_t r = active ? st_role(w, have) : ST_R_TAIL;
            const uint32_t x = (uint32_t)(w >> (8 * ST_H)) & 0xFFu;
            const uint64_t mine = st_state_at(r, w, n - (p0 + lane));
            bool stop = false;
            if (!replace) {
                const uint64_t bad = __ballot(active && r >= ST_R_BAD);
                const uint32_t first = bad ? (uint32_t)__builtin_ctzll(bad) : ST_WAVE;
                const uint32_t n_copy = first < n - p0 ? first : n - p0;
                if (WRITE && lane < n_copy) seq_put(out, cap, o + lane, x);
                o += n_copy;
                if (bad) { next = (uint64_t)__shfl((unsigned long long)mine, (int)first); stop = true; }
            } else {
                const uint32_t l = r & 3u, li = wave_scan_incl(l);
                if (WRITE) {
                    const uint64_t at = o + li - l;
                    if (l == 1) seq_put(out, cap, at, x);
                    else if (l == 3) { seq_put(out, cap, at, 0xEF); seq_put(out, cap, at + 1, 0xBF); seq_put(out, cap, at + 2, 0xBD); }
                }
                o += (uint32_t)__shfl((int)li, 63);
                const uint64_t pm = __ballot(active && r == ST_R_PEND);
                if (pm) next = (uint64_t)__shfl((unsigned long long)mine, (int)__builtin_ctzll(pm));
            }
            wave_lds_sync();                               // (the next chunk, or the next window, fills the LDS again)
            if (stop) break;
        }
        state = next;
    }
    if (st_final(a, b) && !st_stalled(state) && st_count(state)) {
        if (WRITE && lane < 3) seq_put(out, cap, o + lane, lane == 0 ? 0xEFu : lane == 1 ? 0xBFu : 0xBDu);
        o += 3;
        state = 0;
    }
    if (WRITE && lane == 0) state_out[b] = state;
    return o - o0;
}

// ------------------------------------------------------------------------------------------ the op and its kernels (spl_k_seqscan.h)
template <bool I64>
struct StOp {
    using Wave = StWave;
    using Carry = SeqNoCarry;
    const StIn& a; const DecTab& t; uint8_t* out; uint64_t cap; uint64_t* state_out;
    __device__ __forceinline__ uint64_t count(uint64_t b, StWave& L, SeqNoCarry&) const { return st_seq<I64, false>(a, t, b, L, nullptr, 0, 0, nullptr); }
    __device__ __forceinline__ void write(uint64_t b, StWave& L, const SeqNoCarry&, uint64_t o0) const { st_seq<I64, true>(a, t, b, L, out, cap, o0, state_out); }
};

template <bool I64>
__global__ __launch_bounds__(ST_NT) void k_stream_len(StIn a, DecTab t, uint64_t n_blk, uint64_t* __restrict__ cnt, uint64_t* __restrict__ blk) {
    __shared__ StWave s_wave[ST_NT / 64];
    __shared__ uint64_t s_sum[ST_NT / 64];
    seq_len_body(StOp<I64>{a, t, nullptr, 0, nullptr}, SeqNoKeep{}, a.n_seqs, n_blk, s_wave, s_sum, cnt, blk);
}
template <bool I64>
__global__ __launch_bounds__(ST_NT) void k_stream_write(StIn a, DecTab t, uint64_t n_blk, const uint64_t* __restrict__ cnt,
                                                        const uint64_t* __restrict__ blk, uint8_t* __restrict__ out, uint64_t cap,
                                                        uint64_t* __restrict__ out_off, uint64_t* __restrict__ state_out) {
    __shared__ StWave s_wave[ST_NT / 64];
    seq_write_body(StOp<I64>{a, t, out, cap, state_out}, SeqNoKeep{}, a.n_seqs, n_blk, s_wave, cnt, blk, out_off);
}
template <bool I64>
__global__ __launch_bounds__(ST_ONE_NT) void k_stream_one(StIn a, DecTab t, uint8_t* __restrict__ out, uint64_t cap, uint64_t* __restrict__ out_off,
                                                          uint64_t* __restrict__ state_out) {
    __shared__ StWave s_wave[ST_ONE_NT / 64];
    __shared__ uint64_t s_cnt[ST_ONE_MAX + 1];
    seq_one_body(StOp<I64>{a, t, out, cap, state_out}, SeqNoKeep{}, (uint32_t)a.n_seqs, s_wave, s_cnt, out_off);
}
#endif  // __HIPCC__

}  // namespace spl
