// spl_k_choice.h -- spl_choice_step_device: GUIDED CHOICE for B sequences at once.  The answer of a sequence is exactly
// one of up to 64 byte strings (the choice table, laid out as the stop table: 64 slots of up to 64 bytes, uint8 len[64] behind them).  Per
// sequence there is a set A of slots that can still be spelled and the count k of bytes spelled so far (every slot of A shares them); the
// call advances both along the ids the sampler drew and writes the bitmask of the ids it may draw next.  With r_s = c_s[k:] for s in A:
//
//     A empty (free, done or broken)   every bit of the row is 1
//     constrained                       bit t is 1 iff t is ORDINARY (spl_k_heal.h) and some r_s starts with b(t), or -- without
//                                       CH_THEN_FREE -- t is an END id and some r_s is empty; every other bit of the row is 0.  A
//                                       constrained row is never all zero: a sequence whose row would be BREAKS and runs free.
//
// Step, per id while the sequence is constrained: an ordinary id some r_s starts with narrows A to those slots and adds its bytes to k
// (under CH_THEN_FREE the sequence is DONE as soon as a slot of A is spelled out, hit = the lowest such slot); otherwise an END id with
// some r_s empty ends it (done, hit = the lowest such slot); anything else breaks it.
//
// The state row, CH_STATE_WORDS uint64 per sequence (all zero: free and fresh; every bit not named is 0, so rows compare bit for bit):
//     word 0      A, bit s for slot s
//     word 1      bits 0..6 k     bit 8 broken     bit 9 done     bits 16..21 hit (with done)
// written back as (A, k) constrained, (0, k | done | hit << 16) done, (0, broken) broken, zeros free.
//
// ONE launch, k_choice: a WAVEFRONT owns a sequence, a workgroup is one wavefront -- no workgroup barrier, no scratch, no atomics on
// global memory, no polling, no wait between workgroups.  The step tests a slot per lane (the byte loop "r_s starts with b(t)", the new A
// is the ballot).  The row of a constrained sequence is a handful of ids, so it is SCATTERED, not tested id by id: the tokens that are a
// prefix of r_s (or equal to it) are pred' -- the last rank of hl_build's sorted order whose bytes are <= r_s, a prefix of r_s counting as
// below it -- and those of pred's parent ancestors that are no longer than lcp(pred', r_s).  pred' comes from ONE search per slot: with n
// slots alive the lanes split into n groups of 64 / n lanes, every group runs hl_search's multi-way rounds for its slot (one slot: three
// rounds for 200 k tokens; 64 slots: a binary search per lane).  The first lane of a group then walks the chain and ORs the ids' bits into
// a piece of the row in LDS (min(n_words, piece) words; every shipped vocabulary is one piece), the END ids go the same way, and the piece
// is streamed to the mask row, 16 bytes a lane where the row allows it: every word of a written row is stored exactly once.  The chains
// are counted while piece 0 is built, so the "never all zero" rule is decided in front of the first store.  A free row is stored as ones
// without touching LDS or any table.
//
// The first half is plain C++ over the WAVE POLICY of spl_k_heal.h (lanes(), ballot(f), each(f), sync(), reg, info() -- here the LDS piece):
// the kernel instantiates it with the hardware's wavefront, tests/hostsim/choice_sim.cpp with HlHostWave and a run-time lane count -- the
// same text runs in both (with fewer lanes than slots the slots are taken in batches of `lanes`).
#pragma once
#include "spl_common.h"
#include "spl_k_heal.h"

namespace spl {

// (the values of SPL_CHOICE_* in include/splintr_hip.h)
constexpr uint32_t CH_THEN_FREE = 1u, CH_KEEP_FREE = 2u, CH_I64 = 4u;
constexpr uint32_t CH_SLOTS = 64, CH_MAX_LEN = 64, CH_TABLE_BYTES = CH_SLOTS * CH_MAX_LEN + CH_SLOTS, CH_STATE_WORDS = 2, CH_MAX_END = 8;
constexpr uint32_t CH_WAVE = 64;
constexpr uint32_t CH_PIECE = 8192;                               // words of a row built in LDS at once ("choice_piece_words": 4 .. CH_PIECE, a multiple of 4)
constexpr uint64_t CH_BROKEN = 1ull << 8, CH_DONE = 1ull << 9;
// a lane's registers (HlHostWave / HlDevWave: HL_REGS of them): the slot its group searches for, the search's range, the chain's first rank
constexpr uint32_t CH_R_SLOT = 0, CH_R_A = 1, CH_R_B = 2, CH_R_PRED = 3;
static_assert(CH_R_PRED < HL_REGS, "the wave policy's registers hold a lane's search");

struct ChIn {
    const void* ids; const int32_t* len; const uint64_t* state_in; const uint8_t* table; uint64_t n_seqs;
    uint32_t row_len, flags, n_words, piece, v4, n_end;           // v4: n_words is a multiple of four and the mask 16-byte aligned
    uint32_t end_ids[CH_MAX_END];
};

SPL_HD const uint8_t* ch_slot(const ChIn& a, uint32_t s) { return a.table + (size_t)s * CH_MAX_LEN; }
SPL_HD uint32_t ch_len(const ChIn& a, uint32_t s) { return a.table[CH_SLOTS * CH_MAX_LEN + s]; }
SPL_HD bool ch_is_end(const ChIn& a, uint32_t id) {
    for (uint32_t i = 0; i < a.n_end; i++)
        if (a.end_ids[i] == id) return true;
    return false;
}
SPL_HD uint32_t ch_row_n(const ChIn& a, uint64_t b) {
    if (!a.len) return a.row_len;
    const int32_t l = a.len[b];
    return l < 0 ? 0u : ((uint32_t)l > a.row_len ? a.row_len : (uint32_t)l);
}
// the i-th set bit of m (i < popcount(m))
SPL_HD uint32_t ch_nth_bit(uint64_t m, uint32_t i) {
    for (; i; i--) m &= m - 1;
    return (uint32_t)__builtin_ctzll(m);
}
// an OR into the wavefront's LDS piece: lanes of one wavefront may meet in a word
SPL_HD void ch_lds_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
// the slots s with f(s), a slot per lane: the ballot of the hardware's wavefront, `lanes` slots at a time otherwise
template <class W, class F> SPL_HD uint64_t ch_slots(W& w, F f) {
    const uint32_t L = w.lanes();
    uint64_t m = 0;
    for (uint32_t s0 = 0; s0 < CH_SLOTS; s0 += L) m |= w.ballot([&](uint32_t l) { return s0 + l < CH_SLOTS && f(s0 + l); }) << s0;
    return m;
}
// rank p is ABOVE R[0 .. rl): its bytes sort behind R, a proper extension of R included; a prefix of R and R itself are not above.  Over
// the ranks the answer never goes back to false.  By ONE lane.
SPL_HD bool ch_above(const HlTab& t, uint32_t p, const uint8_t* R, uint32_t rl) {
    uint32_t tl;
    const uint8_t* tb = hl_bytes(t, p, tl);
    const uint32_t m = tl < rl ? tl : rl;
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t c = tb[i], x = R[i];
        if (c != x) return c > x;
    }
    return tl > rl;
}

// ------------------------------------------------------------------------------------------ the step
struct ChState { uint64_t A; uint32_t k, hit; bool broken, done; };

// the row as it is loaded: k clamped, done and broken rows with no slots, slots that cannot be spelled from k dropped
template <class W> SPL_HD ChState ch_load(W& w, const ChIn& a, uint64_t b) {
    const uint64_t* row = a.state_in + b * CH_STATE_WORDS;
    const uint64_t w1 = row[1];
    ChState s;
    s.A = row[0];                                                              // (state_out may be state_in: the row is read here, written once at the end)
    s.k = (uint32_t)w1 & 0x7Fu; if (s.k > CH_MAX_LEN) s.k = CH_MAX_LEN;
    s.broken = (w1 & CH_BROKEN) != 0; s.done = !s.broken && (w1 & CH_DONE) != 0; s.hit = (uint32_t)(w1 >> 16) & 63u;
    if (s.broken || s.done) s.A = 0;
    if (s.A) {
        const uint32_t k = s.k;
        s.A &= ch_slots(w, [&](uint32_t sl) { const uint32_t n = ch_len(a, sl); return n >= 1 && n <= CH_MAX_LEN && n >= k; });
    }
    if (!s.A && !s.done) s.k = 0;
    return s;
}
SPL_HD uint64_t ch_word1(const ChState& s) {
    if (s.broken) return CH_BROKEN;
    if (s.done) return (uint64_t)s.k | CH_DONE | ((uint64_t)s.hit << 16);
    return s.A ? (uint64_t)s.k : 0ull;
}
// the slots of A that are spelled out
template <class W> SPL_HD uint64_t ch_spelled(W& w, const ChIn& a, const ChState& s) {
    const uint64_t A = s.A; const uint32_t k = s.k;
    return ch_slots(w, [&](uint32_t sl) { return ((A >> sl) & 1u) && ch_len(a, sl) == k; });
}
// the row's valid ids in order, while the sequence is constrained
template <class W> SPL_HD void ch_step_seq(W& w, const HlTab& t, const ChIn& a, uint64_t b, ChState& s) {
    const uint32_t n = ch_row_n(a, b);
    const bool then_free = (a.flags & CH_THEN_FREE) != 0;
    for (uint32_t i = 0; i < n && s.A; i++) {
        uint32_t id; bool is_id = true;
        if (a.flags & CH_I64) {
            const uint64_t v = static_cast<const uint64_t*>(a.ids)[b * a.row_len + i];
            is_id = (v >> 32) == 0; id = (uint32_t)v;
        } else id = static_cast<const uint32_t*>(a.ids)[b * a.row_len + i];
        const uint32_t r = is_id ? hl_rank32(t, id) : HL_NONE;
        uint64_t S = 0;
        uint32_t tl = 0;
        if (r != HL_NONE) {
            const uint8_t* tb = hl_bytes(t, r, tl);
            const uint64_t A = s.A; const uint32_t k = s.k;
            S = ch_slots(w, [&](uint32_t sl) {
                if (!((A >> sl) & 1u) || k + tl > ch_len(a, sl)) return false;
                const uint8_t* c = ch_slot(a, sl) + k;
                for (uint32_t j = 0; j < tl; j++)
                    if (c[j] != tb[j]) return false;
                return true;
            });
        }
        if (S) {
            s.A = S; s.k += tl;
            if (then_free) {
                const uint64_t F = ch_spelled(w, a, s);
                if (F) { s.done = true; s.hit = (uint32_t)__builtin_ctzll(F); s.A = 0; }
            }
            continue;
        }
        const uint64_t E = (!then_free && is_id && ch_is_end(a, id)) ? ch_spelled(w, a, s) : 0ull;
        if (E) { s.done = true; s.hit = (uint32_t)__builtin_ctzll(E); s.A = 0; }
        else { s.broken = true; s.A = 0; s.k = 0; }
    }
}

// ------------------------------------------------------------------------------------------ the row
// Batch `bt` of the alive slots (`groups` of them a batch, g lanes a group): every group's search for the first rank above its r_s.  It
// leaves the chain's first rank -- pred', HL_NONE for none -- in the register of the group's first lane.
template <class W> SPL_HD void ch_search(W& w, const HlTab& t, const ChIn& a, const ChState& s, uint32_t n_alive, uint32_t groups, uint32_t g, uint32_t bt) {
    const uint64_t A = s.A; const uint32_t k = s.k;
    w.each([&](uint32_t l) {
        const uint32_t grp = l / g, idx = bt * groups + grp;
        const bool on = grp < groups && idx < n_alive;
        const uint32_t sl = on ? ch_nth_bit(A, idx) : CH_SLOTS;
        w.reg(l, CH_R_SLOT) = sl;
        w.reg(l, CH_R_A) = 0u;
        w.reg(l, CH_R_B) = on && ch_len(a, sl) > k ? t.n : 0u;                  // (an empty r_s has no prefix token: nothing to search)
        w.reg(l, CH_R_PRED) = HL_NONE;
    });
    const uint64_t gm = g >= 64 ? ~0ull : (1ull << g) - 1;
    while (w.ballot([&](uint32_t l) { return w.reg(l, CH_R_A) < w.reg(l, CH_R_B); })) {
        // one pivot per lane, as hl_search: the lanes of a group that say "not above" are its first c
        const uint64_t m = w.ballot([&](uint32_t l) {
            const uint32_t lo = w.reg(l, CH_R_A), hi = w.reg(l, CH_R_B);
            if (lo >= hi) return false;
            const uint32_t n = hi - lo, step = n / (g + 1) + (n % (g + 1) ? 1u : 0u), sl = w.reg(l, CH_R_SLOT);
            const uint64_t p = (uint64_t)lo + (uint64_t)(l % g + 1) * step - 1;
            return p < hi && !ch_above(t, (uint32_t)p, ch_slot(a, sl) + k, ch_len(a, sl) - k);
        });
        w.each([&](uint32_t l) {
            const uint32_t lo = w.reg(l, CH_R_A), hi = w.reg(l, CH_R_B);
            if (lo >= hi) return;
            const uint32_t n = hi - lo, step = n / (g + 1) + (n % (g + 1) ? 1u : 0u);
            const uint32_t c = (uint32_t)__builtin_popcountll((m >> (l / g * g)) & gm);
            const uint64_t nb = (uint64_t)lo + (uint64_t)(c + 1) * step - 1;
            w.reg(l, CH_R_A) = lo + c * step;
            if (c < g && nb < hi) w.reg(l, CH_R_B) = (uint32_t)nb;
        });
    }
    w.each([&](uint32_t l) {
        const uint32_t sl = w.reg(l, CH_R_SLOT);
        if (l % g == 0 && sl < CH_SLOTS && ch_len(a, sl) > k && w.reg(l, CH_R_A) > 0) w.reg(l, CH_R_PRED) = w.reg(l, CH_R_A) - 1;
    });
}
// The chains of the batch the registers hold: the ids inside words [p0, p0 + pw) are ORed into the piece; returns the lanes whose chain
// has an id at all (inside the piece or not).
template <class W> SPL_HD uint64_t ch_walk(W& w, const HlTab& t, const ChIn& a, const ChState& s, uint32_t p0, uint32_t pw) {
    uint32_t* lds = w.info();
    const uint32_t k = s.k;
    return w.ballot([&](uint32_t l) {
        uint32_t r = w.reg(l, CH_R_PRED);
        if (r == HL_NONE) return false;
        const uint32_t sl = w.reg(l, CH_R_SLOT), rl = ch_len(a, sl) - k;
        const uint8_t* R = ch_slot(a, sl) + k;
        uint32_t tl;
        const uint8_t* tb = hl_bytes(t, r, tl);
#ifdef SPL_CHOICE_MUTANT_LCP
        const uint32_t lcp = rl;
        (void)tb; (void)R;
#else
        uint32_t lcp = 0;
        for (const uint32_t m = tl < rl ? tl : rl; lcp < m && tb[lcp] == R[lcp]; lcp++) {}
#endif
        uint32_t cnt = 0;
        for (; r != HL_NONE; r = t.parent[r]) {
            (void)hl_bytes(t, r, tl);
#ifdef SPL_CHOICE_MUTANT_EQ
            if (tl > lcp || tl >= rl) continue;
#else
            if (tl > lcp) continue;
#endif
            const uint32_t id = t.sorted[r], d = (id >> 5) - p0;
            cnt++;
            if (d < pw) ch_lds_or(lds + d, 1u << (id & 31u));
        }
        return cnt != 0;
    });
}

// everything of sequence b: the transition, the row, the state row and live.  put(b, word, value) and put4(b, word, four values) store.
template <class W, class O> SPL_HD void ch_seq(W& w, const HlTab& t, const ChIn& a, uint64_t b, const O& out) {
    const uint32_t L = w.lanes();
    ChState s = ch_load(w, a, b);
    ch_step_seq(w, t, a, b, s);
    auto finish = [&](bool ones) {                                             // the state row and live; a row of ones where one is due
        const uint64_t w0 = s.A, w1 = ch_word1(s);
        w.each([&](uint32_t l) { if (l == 0) { out.state(b, 0, w0); out.state(b, 1, w1); out.alive(b, w0 ? 1u : 0u); } });
        if (!ones || (a.flags & CH_KEEP_FREE)) return;
        const uint32_t one[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        w.each([&](uint32_t l) {
            if (a.v4) for (uint32_t i = 4 * l; i < a.n_words; i += 4 * L) out.put4(b, i, one);
            else for (uint32_t i = l; i < a.n_words; i += L) out.put(b, i, 0xFFFFFFFFu);
        });
    };
    if (!s.A) { finish(true); return; }
    const uint32_t n_alive = (uint32_t)__builtin_popcountll(s.A);
    const uint32_t groups = n_alive < L ? n_alive : L, g = L / groups, batches = (n_alive + groups - 1) / groups;
    const bool ends = !(a.flags & CH_THEN_FREE) && a.n_end && ch_spelled(w, a, s) != 0;
    uint32_t* lds = w.info();
    for (uint32_t p0 = 0; p0 < a.n_words; p0 += a.piece) {
        const uint32_t pw = a.n_words - p0 < a.piece ? a.n_words - p0 : a.piece;
        w.each([&](uint32_t l) { for (uint32_t i = l; i < pw; i += L) lds[i] = 0u; });
        w.sync();
        uint64_t any = 0;
        for (uint32_t bt = 0; bt < batches; bt++) {
            if (p0 == 0 || batches > 1) ch_search(w, t, a, s, n_alive, groups, g, bt);        // (one batch: the registers keep it for every piece)
            any |= ch_walk(w, t, a, s, p0, pw);
        }
        if (p0 == 0) {
            if (!any && !ends) {                                               // the vocabulary lacks what comes next: the sequence breaks, its row is ones
                s.broken = true; s.A = 0; s.k = 0;
                finish(true);
                return;
            }
            finish(false);
        }
        if (ends)
            w.each([&](uint32_t l) {
                for (uint32_t i = l; i < a.n_end; i += L) {
                    const uint32_t id = a.end_ids[i], d = (id >> 5) - p0;
                    if (d < pw) ch_lds_or(lds + d, 1u << (id & 31u));
                }
            });
        w.sync();
        w.each([&](uint32_t l) {
            if (a.v4) for (uint32_t i = 4 * l; i < pw; i += 4 * L) out.put4(b, p0 + i, lds + i);
            else for (uint32_t i = l; i < pw; i += L) out.put(b, p0 + i, lds[i]);
        });
        w.sync();
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernel
struct ChOut {
    uint64_t* state_out; uint32_t* mask; uint8_t* live; uint32_t n_words;
    __device__ __forceinline__ void state(uint64_t b, uint32_t i, uint64_t v) const { state_out[b * CH_STATE_WORDS + i] = v; }
    __device__ __forceinline__ void alive(uint64_t b, uint32_t v) const { if (live) live[b] = (uint8_t)v; }
    __device__ __forceinline__ void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; }
    __device__ __forceinline__ void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        *reinterpret_cast<uint4*>(mask + b * n_words + k) = make_uint4(v[0], v[1], v[2], v[3]);
    }
};

// grid (1, sequences over y and z), one wavefront a workgroup; dynamic LDS: min(n_words, piece) words
__global__ __launch_bounds__(CH_WAVE) void k_choice(ChIn a, HlTab t, ChOut out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_choice[];
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    HlDevWave w{nullptr, s_choice, {}};
    ch_seq(w, t, a, b, out);
}
#endif  // __HIPCC__

}  // namespace spl
