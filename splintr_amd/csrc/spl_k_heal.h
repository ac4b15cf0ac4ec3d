// spl_k_heal.h -- spl_heal_begin_device / spl_heal_step_device: TOKEN HEALING for B sequences at once.  Per sequence there
// is a pending prefix P of 0 .. 64 bytes; the call advances it and writes the bitmask of the ids the sampler may draw next:
//
//     |P| = 0  (free)         every bit of the row is 1
//     |P| >= 1 (constrained)  bit t is 1 iff t is ORDINARY (an id of the vocabulary proper with at least one byte) and b(t) starts with P
//                             (t COVERS) or P starts with b(t) and |b(t)| < |P| (t is PARTIAL); every other bit of the row is 0
//
// Step: the row's valid ids in order -- free stays free; a covering id empties P (healed); a partial id takes its bytes off the front of P;
// anything else (a special, an unknown id, an ordinary id that disagrees) empties P and sets the sticky `broken`.  Begin: walk back from a
// prompt's last token while the limits allow (max_back, min_keep, ordinary, 64 bytes, and under HL_AUTO: some ordinary token is strictly
// longer than the candidate and starts with it), P = the bytes taken.
//
// The state row, HL_STATE_WORDS uint64 per sequence (all zero: free and fresh; every bit not named is 0 and P's bytes from |P| on are 0, so
// rows compare bit for bit):
//     word 0      bits 0..6 |P|     bit 8 broken     bit 9 healed
//     words 1..8  P, the first byte lowest
//
// Tables (spl_heal_host.h builds them): sorted[n] rank -> id, the ordinary ids by (bytes as unsigned, shorter first, id); rank[max_id + 1]
// id -> rank, HL_NONE for every id that is not ordinary; parent[n]: the rank of the longest other ordinary token that is a proper prefix of
// this one (of equal byte strings: the rank in front), HL_NONE for none.  The covering ids of P are one range of ranks [lo, hi): lo the first
// rank whose bytes are >= P, hi the first at or behind lo whose bytes do not start with P.  The partial ids need no search: a token A that is
// a proper prefix of P sorts below P, so A <= pred = rank lo - 1 < P, and a string between A and P starts with A -- A is pred or one of
// pred's parent ancestors, namely those of length <= min(lcp(pred, P), |P| - 1).
//
// Two launches.  k_heal_plan: a WAVEFRONT owns a sequence -- the transition (each compare one lane per byte and a ballot), then lo and hi by
// a search with one pivot per lane (three rounds for 200 k tokens), then the chain; it leaves lo, hi and the partial ids in the scratch.
// k_heal_fill: a workgroup owns HL_WG_IDS ids and a group of sequences; a lane holds the ranks of HL_PER ids in registers (loaded at the
// first constrained sequence, never for free ones), tests lo <= rank < hi, the 64-bit ballots become two words each (lane k keeps word k of
// the wavefront's range), the partial ids of the range are ORed in, whole words are stored.  No atomics on global memory, no polling, no wait between workgroups; every word of
// every written row is stored exactly once.
//
// The first half is plain C++ over a WAVE POLICY (lanes(), ballot(f), each(f), get(k, f), sync(), reg): the kernels instantiate it with the
// hardware's wavefront, tests/hostsim/heal_sim.cpp with HlHostWave and a run-time lane count -- the same text runs in both.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "spl_common.h"

#ifndef SPL_HEAL_PER
#define SPL_HEAL_PER 16                /* ids a lane of the fill holds in registers: a wavefront owns 64 * SPL_HEAL_PER ids, 2 * SPL_HEAL_PER words of a row */
#endif

namespace spl {

// (the values of SPL_HEAL_* in include/splintr_hip.h)
constexpr uint32_t HL_AUTO = 1u, HL_KEEP_FREE = 2u, HL_I64 = 4u, HL_PAD_LEFT = 8u;
constexpr uint32_t HL_STATE_WORDS = 9, HL_MAX_P = 64, HL_MAX_BACK = 8;
constexpr uint32_t HL_NONE = 0xFFFFFFFFu;
constexpr uint32_t HL_WAVE = 64;
constexpr uint32_t HL_PLAN_NT = 256;                             // k_heal_plan: four sequences a workgroup
constexpr uint32_t HL_FILL_NT = 256;
constexpr uint32_t HL_PER = SPL_HEAL_PER;
constexpr uint32_t HL_WAVE_IDS = HL_WAVE * HL_PER, HL_WAVE_WORDS = HL_WAVE_IDS / 32;
constexpr uint32_t HL_WG_IDS = HL_WAVE_IDS * (HL_FILL_NT / HL_WAVE), HL_WG_WORDS = HL_WG_IDS / 32;
constexpr uint32_t HL_REGS = HL_PER + 2;                             // a fill lane's registers: its ranks and two more (hl_fill_wave)
constexpr uint32_t HL_MAX_PART = 63;                             // a partial token is shorter than P
// the scratch, HL_SCR words per sequence: lo (HL_NONE: the sequence is free), hi, the count of partial ids (bit 31: it broke in this call), the ids
constexpr uint32_t HL_SCR = 3 + HL_MAX_PART, HL_BROKE = 1u << 31;
constexpr uint32_t HL_SPW_MAX = 64;                              // most sequences one fill workgroup loops over

struct HlTab {
    const uint32_t* tok_off; const uint8_t* tok_bytes; uint32_t max_id;        // the decode tables (upload_decode)
    const uint32_t* sorted; const uint32_t* rank; const uint32_t* parent; uint32_t n;
};
struct HlIn {
    const void* ids; const int32_t* len; const uint64_t* state_in; uint64_t n_seqs;
    uint32_t row_len, flags, max_back, min_keep;
};

// ------------------------------------------------------------------------------------------ the state row
SPL_HD uint32_t hl_plen(uint64_t w0) { const uint32_t l = (uint32_t)w0 & 0x7Fu; return l > HL_MAX_P ? HL_MAX_P : l; }      // (a row that is no state: stay inside the row)
SPL_HD bool hl_broken(uint64_t w0) { return ((w0 >> 8) & 1u) != 0; }
SPL_HD bool hl_healed(uint64_t w0) { return ((w0 >> 9) & 1u) != 0; }
SPL_HD uint64_t hl_word0(uint32_t plen, bool broken, bool healed) { return (uint64_t)plen | ((uint64_t)(broken ? 1u : 0u) << 8) | ((uint64_t)(healed ? 1u : 0u) << 9); }

// ------------------------------------------------------------------------------------------ table access
// the rank of an id as the rows hold it (int64: a value outside 0 .. 2^32 - 1 is no id); HL_NONE: not ordinary
SPL_HD uint32_t hl_rank32(const HlTab& t, uint32_t id) { return id <= t.max_id ? t.rank[id] : HL_NONE; }
SPL_HD uint32_t hl_rank_at(const HlTab& t, const void* ids, uint64_t i, bool i64) {
    if (!i64) return hl_rank32(t, static_cast<const uint32_t*>(ids)[i]);
    const uint64_t v = static_cast<const uint64_t*>(ids)[i];
    return (v >> 32) ? HL_NONE : hl_rank32(t, (uint32_t)v);
}
SPL_HD const uint8_t* hl_bytes(const HlTab& t, uint32_t r, uint32_t& len) {
    const uint32_t id = t.sorted[r], o = t.tok_off[id];
    len = t.tok_off[id + 1] - o;
    return t.tok_bytes + o;
}
// a row's valid entries: len clamped to 0 .. row_len (null: all of them)
SPL_HD uint32_t hl_row_n(const HlIn& a, uint64_t b) {
    if (!a.len) return a.row_len;
    const int32_t l = a.len[b];
    return l < 0 ? 0u : ((uint32_t)l > a.row_len ? a.row_len : (uint32_t)l);
}

// ------------------------------------------------------------------------------------------ byte-string compare
// rank r against P, by ONE lane: 0 its bytes are below P (a proper prefix of P included), 1 they start with P, 2 they are above P and do
// not start with it.  Over the ranks the class never decreases: lo is the first rank of class >= 1, hi the first of class 2.
SPL_HD uint32_t hl_class(const HlTab& t, uint32_t r, const uint8_t* P, uint32_t plen) {
    uint32_t tl;
    const uint8_t* tb = hl_bytes(t, r, tl);
    const uint32_t m = tl < plen ? tl : plen;
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t c = tb[i], p = P[i];
        if (c != p) return c < p ? 0u : 2u;
    }
    return tl >= plen ? 1u : 0u;
}
// the first i < n with f(i), or n: one lane per index and a ballot
template <class W, class F> SPL_HD uint32_t hl_first(W& w, uint32_t n, F f) {
    const uint32_t L = w.lanes();
    for (uint32_t i0 = 0; i0 < n; i0 += L) {
        const uint64_t m = w.ballot([&](uint32_t l) { return i0 + l < n && f(i0 + l); });
        if (m) return i0 + (uint32_t)__builtin_ctzll(m);
    }
    return n;
}
// the bytes two strings share at their fronts
template <class W> SPL_HD uint32_t hl_lcp(W& w, const uint8_t* A, uint32_t la, const uint8_t* B, uint32_t lb) {
    return hl_first(w, la < lb ? la : lb, [&](uint32_t i) { return A[i] != B[i]; });
}

// ------------------------------------------------------------------------------------------ the searches
// The first rank in [a, b] of class >= thr (b: none below it), given that every rank below a is of a lower class.  One pivot per lane:
// pivots step ranks apart, the count of lanes that say "lower" picks the piece; 64 lanes take 200 k ranks in three rounds, one lane is a
// binary search.
template <class W> SPL_HD uint32_t hl_search(W& w, const HlTab& t, const uint8_t* P, uint32_t plen, uint32_t a, uint32_t b, uint32_t thr) {
    const uint32_t L = w.lanes();
    while (a < b) {
        const uint32_t n = b - a, step = n / (L + 1) + (n % (L + 1) ? 1u : 0u);
        const uint64_t m = w.ballot([&](uint32_t l) {
            const uint64_t p = (uint64_t)a + (uint64_t)(l + 1) * step - 1;
            return p < b && hl_class(t, (uint32_t)p, P, plen) < thr;
        });
        const uint32_t c = (uint32_t)__builtin_popcountll(m);                   // (the class never decreases: the lanes that say "lower" are the first c)
        const uint64_t nb = (uint64_t)a + (uint64_t)(c + 1) * step - 1;
        a += c * step;
        if (c < L && nb < b) b = (uint32_t)nb;                                 // (lane c said "not lower" at nb)
    }
    return a;
}
struct HlRange { uint32_t lo, hi; };
// [lo, hi): the ranks whose bytes start with P.  hi is looked for next to lo first (a prefix of several bytes has few covering tokens).
template <class W> SPL_HD HlRange hl_range(W& w, const HlTab& t, const uint8_t* P, uint32_t plen) {
    HlRange g;
    g.lo = hl_search(w, t, P, plen, 0u, t.n, 1u);
#ifdef SPL_HEAL_MUTANT_HI
    g.hi = g.lo < t.n ? g.lo + 1 : g.lo;
#else
    const uint32_t L = w.lanes();
    const uint64_t m = w.ballot([&](uint32_t l) { return (uint64_t)g.lo + l < t.n && hl_class(t, g.lo + l, P, plen) < 2u; });
    const uint32_t c = (uint32_t)__builtin_popcountll(m);
    g.hi = c < L ? g.lo + c : hl_search(w, t, P, plen, g.lo + L, t.n, 2u);
#endif
    return g;
}
// HL_AUTO: some ordinary token starts with the candidate (c bytes) and is strictly longer.  The candidate itself, if it is a token, sorts
// first in [lo, hi): a last rank that is longer than c says it all.
SPL_HD bool hl_extends(const HlTab& t, HlRange g, uint32_t c) {
    if (g.hi <= g.lo) return false;
    uint32_t tl;
    (void)hl_bytes(t, g.hi - 1, tl);
    return tl > c;
}

// ------------------------------------------------------------------------------------------ one sequence: transition, range, chain
// what the plan writes.  The kernels' sink stores; the host simulation's counts every store.
struct HlOut {
    uint64_t* state_out; uint8_t* live; int32_t* n_back; uint32_t* scr;
    SPL_HD void state(uint64_t b, uint32_t i, uint64_t v) const { state_out[b * HL_STATE_WORDS + i] = v; }
    SPL_HD void alive(uint64_t b, uint32_t v) const { if (live) live[b] = (uint8_t)v; }
    SPL_HD void back(uint64_t b, uint32_t v) const { if (n_back) n_back[b] = (int32_t)v; }
    SPL_HD void plan(uint64_t b, uint32_t i, uint32_t v) const { scr[b * HL_SCR + i] = v; }
};

// P lives in one of the wavefront's two 64-byte buffers (w.pbuf(0 / 1)), zero from |P| on; a transition writes the other one
template <class W> SPL_HD void hl_p_load(W& w, uint32_t cur, const uint64_t* row, uint32_t plen) {
    const uint8_t* src = plen ? reinterpret_cast<const uint8_t*>(row + 1) : nullptr;
    uint8_t* P = w.pbuf(cur);
    w.each([&](uint32_t l) { for (uint32_t i = l; i < HL_MAX_P; i += w.lanes()) P[i] = i < plen ? src[i] : (uint8_t)0; });
    w.sync();
}
// P := P[k:]
template <class W> SPL_HD void hl_p_drop(W& w, uint32_t& cur, uint32_t plen, uint32_t k) {
    const uint8_t* P = w.pbuf(cur);
    uint8_t* Q = w.pbuf(cur ^ 1u);
    w.each([&](uint32_t l) { for (uint32_t i = l; i < HL_MAX_P; i += w.lanes()) Q[i] = i + k < plen ? P[i + k] : (uint8_t)0; });
    w.sync();
    cur ^= 1u;
}
// the other buffer := tb[0 .. tl) + P   (tl + plen <= 64)
template <class W> SPL_HD void hl_p_front(W& w, uint32_t cur, uint32_t plen, const uint8_t* tb, uint32_t tl) {
    const uint8_t* P = w.pbuf(cur);
    uint8_t* Q = w.pbuf(cur ^ 1u);
    w.each([&](uint32_t l) { for (uint32_t i = l; i < HL_MAX_P; i += w.lanes()) Q[i] = i < tl ? tb[i] : (i - tl < plen ? P[i - tl] : (uint8_t)0); });
    w.sync();
}

// the state a step arrives at: the row's valid ids applied in order
template <class W> SPL_HD void hl_step_seq(W& w, const HlTab& t, const HlIn& a, uint64_t b, uint32_t& cur, uint32_t& plen, bool& broken, bool& healed,
                                           bool& broke_now) {
    const uint32_t n = hl_row_n(a, b);
    for (uint32_t k = 0; k < n && plen; k++) {                                 // (free stays free: nothing is read)
        const uint32_t r = hl_rank_at(t, a.ids, b * a.row_len + k, (a.flags & HL_I64) != 0);
        bool agree = r != HL_NONE;
        uint32_t tl = 0;
        if (agree) {
            const uint8_t* tb = hl_bytes(t, r, tl);
            const uint8_t* P = w.pbuf(cur);
            const uint32_t m = tl < plen ? tl : plen;
            agree = hl_lcp(w, tb, m, P, m) == m;
        }
        if (!agree) { broken = true; broke_now = true; hl_p_drop(w, cur, plen, plen); plen = 0; }
        else if (tl >= plen) { healed = true; hl_p_drop(w, cur, plen, plen); plen = 0; }
        else { hl_p_drop(w, cur, plen, tl); plen -= tl; }
    }
}

// the state a begin arrives at: tokens taken off the prompt's end while the limits allow; returns how many.  Under HL_AUTO the range of
// the last candidate taken is P's own: have says that g holds it.
template <class W> SPL_HD uint32_t hl_begin_seq(W& w, const HlTab& t, const HlIn& a, uint64_t b, uint32_t& cur, uint32_t& plen, HlRange& g, bool& have) {
    const uint32_t n = hl_row_n(a, b);
    uint32_t taken = 0;
    have = false;
    for (uint32_t j = 1; j <= a.max_back; j++) {
        if ((int64_t)n - (int64_t)j < (int64_t)a.min_keep) break;
        const uint64_t pos = (a.flags & HL_PAD_LEFT) ? (uint64_t)a.row_len - j : (uint64_t)n - j;
        const uint32_t r = hl_rank_at(t, a.ids, b * a.row_len + pos, (a.flags & HL_I64) != 0);
        if (r == HL_NONE) break;
        uint32_t tl;
        const uint8_t* tb = hl_bytes(t, r, tl);
        if (tl + plen > HL_MAX_P) break;
        hl_p_front(w, cur, plen, tb, tl);
        if (a.flags & HL_AUTO) {
            const HlRange c = hl_range(w, t, w.pbuf(cur ^ 1u), tl + plen);
            if (!hl_extends(t, c, tl + plen)) break;
            g = c; have = true;
        }
        cur ^= 1u; plen += tl; taken = j;
    }
    return taken;
}

// everything of sequence b: the transition, the state row, live, the range and the partial ids into the scratch
template <class W, class O> SPL_HD void hl_plan_seq(W& w, const HlTab& t, const HlIn& a, bool begin, uint64_t b, const O& out) {
    uint32_t cur = 0, plen = 0, taken = 0;
    bool broken = false, healed = false, broke_now = false, have = false;
    HlRange g{0, 0};
    if (begin) {
        hl_p_load(w, cur, nullptr, 0);
        taken = hl_begin_seq(w, t, a, b, cur, plen, g, have);
    } else {
        const uint64_t* row = a.state_in + b * HL_STATE_WORDS;
        const uint64_t w0 = row[0];
        plen = hl_plen(w0); broken = hl_broken(w0); healed = hl_healed(w0);
        hl_p_load(w, cur, row, plen);                                          // (state_out may be state_in: the row is read here, written below)
        hl_step_seq(w, t, a, b, cur, plen, broken, healed, broke_now);
    }
    const uint8_t* P = w.pbuf(cur);
    const uint64_t w0 = hl_word0(plen, broken, healed);
    w.each([&](uint32_t l) {
        for (uint32_t i = l; i < HL_STATE_WORDS; i += w.lanes()) {
            uint64_t v = w0;
            if (i) memcpy(&v, P + 8 * (i - 1), 8);
            out.state(b, i, v);
        }
        if (l == 0) { out.alive(b, plen ? 1u : 0u); if (begin) out.back(b, taken); }
    });
    if (!plen) {
        w.each([&](uint32_t l) { if (l == 0) { out.plan(b, 0, HL_NONE); out.plan(b, 1, 0u); out.plan(b, 2, broke_now ? HL_BROKE : 0u); } });
        w.sync();
        return;
    }
    if (!have) g = hl_range(w, t, P, plen);
    // the chain: pred and its ancestors, those short enough to be a prefix of P
    uint32_t cnt = 0;
    if (g.lo > 0) {
        uint32_t r = g.lo - 1, tl;
        const uint8_t* tb = hl_bytes(t, r, tl);
#ifdef SPL_HEAL_MUTANT_LCP
        const uint32_t bound = plen - 1;
        (void)tb;
#else
        const uint32_t lcp = hl_lcp(w, tb, tl, P, plen), bound = lcp < plen - 1 ? lcp : plen - 1;
#endif
        while (r != HL_NONE && bound) {
            (void)hl_bytes(t, r, tl);
            if (tl <= bound && cnt < HL_MAX_PART) {
                const uint32_t id = t.sorted[r], at = cnt;
                w.each([&](uint32_t l) { if (l == 0) out.plan(b, 3 + at, id); });
                cnt++;
            }
            r = t.parent[r];
        }
    }
    w.each([&](uint32_t l) { if (l == 0) { out.plan(b, 0, g.lo); out.plan(b, 1, g.hi); out.plan(b, 2, cnt | (broke_now ? HL_BROKE : 0u)); } });
    w.sync();
}

// ------------------------------------------------------------------------------------------ the fill
// One wavefront, the ids [id0, id0 + HL_WAVE_IDS), the sequences [s0, s1): the words [id0 / 32, ...) of their rows below n_words.  put(s, word
// index, value) stores.  The ballot is the hardware's: 64 lanes, two words.
template <class W, class F> SPL_HD void hl_fill_wave(W& w, const HlTab& t, const uint32_t* scr, uint32_t id0, uint64_t s0, uint64_t s1, uint32_t n_words,
                                                    uint32_t flags, F put) {
    static_assert(HL_WAVE_WORDS <= HL_WAVE && HL_MAX_PART < HL_WAVE, "a lane per word of the wavefront's range, a lane per partial id");
    const uint32_t wd0 = id0 >> 5;
    if (wd0 >= n_words || s0 >= s1) return;
    const uint32_t nw = n_words - wd0 < HL_WAVE_WORDS ? n_words - wd0 : HL_WAVE_WORDS;
    // lo, hi and the count of every sequence of the group, fetched at once: the loop below waits for no load of its own
    uint32_t* inf = w.info();
    const uint32_t ns = (uint32_t)(s1 - s0);                                   // (<= HL_SPW_MAX)
    w.each([&](uint32_t l) {
        for (uint32_t i = l; i < ns; i += HL_WAVE) {
            const uint32_t* q = scr + (s0 + i) * HL_SCR;
            inf[3 * i] = q[0]; inf[3 * i + 1] = q[1]; inf[3 * i + 2] = q[2];
        }
    });
    w.sync();
    // a lane's registers: the ranks of its HL_PER ids, then R_PART lane k's k-th partial id of the sequence (loaded in front of the
    // ballots, used behind them), R_WORD the word of the row that lane k builds (word wd0 + k)
    constexpr uint32_t R_PART = HL_PER, R_WORD = HL_PER + 1;
    bool loaded = false;
    for (uint32_t i = 0; i < ns; i++) {
        const uint64_t s = s0 + i;
        const uint32_t lo = inf[3 * i], hi = inf[3 * i + 1];
        if (lo == HL_NONE) {                                                   // free: ones, and rank is not touched
            if (!(flags & HL_KEEP_FREE)) w.each([&](uint32_t l) { if (l < nw) put(s, wd0 + l, 0xFFFFFFFFu); });
            continue;
        }
        if (!loaded) {
            w.each([&](uint32_t l) {
#pragma unroll
                for (uint32_t j = 0; j < HL_PER; j++) {
                    const uint64_t id = (uint64_t)id0 + j * HL_WAVE + l;
                    w.reg(l, j) = id <= t.max_id ? t.rank[id] : HL_NONE;
                }
            });
            loaded = true;
        }
        const uint32_t span = hi - lo;                                          // (HL_NONE - lo >= span: an id that is not ordinary is never inside)
        const uint32_t cnt = inf[3 * i + 2] & 0x7Fu;
        const uint32_t* q = scr + s * HL_SCR + 3;
        w.each([&](uint32_t l) { w.reg(l, R_PART) = l < cnt ? q[l] : HL_NONE; w.reg(l, R_WORD) = 0u; });
#pragma unroll
        for (uint32_t j = 0; j < HL_PER; j++) {                                 // ballot j is words 2 j and 2 j + 1 of the range
            const uint64_t m = w.ballot([&](uint32_t l) { return w.reg(l, j) - lo < span; });
            w.each([&](uint32_t l) { if ((l >> 1) == j) w.reg(l, R_WORD) = (l & 1u) ? (uint32_t)(m >> 32) : (uint32_t)m; });
        }
        for (uint32_t k = 0; k < cnt; k++) {                                   // the partial ids that fall into the range
            const uint32_t d = w.get(k, [&](uint32_t l) { return w.reg(l, R_PART); }) - id0;
            if (d < HL_WAVE_IDS) w.each([&](uint32_t l) { if (l == (d >> 5)) w.reg(l, R_WORD) |= 1u << (d & 31u); });
        }
        w.each([&](uint32_t l) { if (l < nw) put(s, wd0 + l, w.reg(l, R_WORD)); });
    }
}
// sequences a fill workgroup loops over: as many as keep the grid at a thousand workgroups or more, 8 .. HL_SPW_MAX
SPL_HD uint32_t hl_spw(uint64_t n_seqs, uint32_t n_words) {
    const uint64_t cols = ((uint64_t)n_words + HL_WG_WORDS - 1) / HL_WG_WORDS;
    uint32_t spw = HL_SPW_MAX;
    while (spw > 8 && cols * ((n_seqs + spw - 1) / spw) < 1024) spw >>= 1;
    return spw;
}

// ------------------------------------------------------------------------------------------ the tables (host)
// sorted, rank and parent from the vocabulary proper: off[max_id + 2] and bytes as the decode tables hold them, present[id] != 0 for an id
// of the vocabulary proper.  false: more than HL_MAX_PART ids spell prefixes (of at most 63 bytes) of one string -- only a vocabulary with
// equal byte strings under many ids can do that -- and the scratch could not hold a sequence's partial ids.
inline bool hl_build(const uint32_t* off, const uint8_t* bytes, const uint8_t* present, uint32_t max_id, std::vector<uint32_t>& sorted,
                     std::vector<uint32_t>& rank, std::vector<uint32_t>& parent) {
    auto len_of = [&](uint32_t id) { return off[id + 1] - off[id]; };
    auto ptr_of = [&](uint32_t id) { return bytes + off[id]; };
    sorted.clear();
    for (uint64_t id = 0; id <= max_id; id++)
        if (present[id] && len_of((uint32_t)id) >= 1) sorted.push_back((uint32_t)id);
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) {
        const uint32_t lx = len_of(x), ly = len_of(y);
        const int k = memcmp(ptr_of(x), ptr_of(y), std::min(lx, ly));
        if (k) return k < 0;
        return lx != ly ? lx < ly : x < y;
    });
    const uint32_t n = (uint32_t)sorted.size();
    rank.assign((size_t)max_id + 1, HL_NONE);
    parent.assign(n, HL_NONE);
    std::vector<uint32_t> depth(n, 0), chain;
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t id = sorted[r], l = len_of(id);
        rank[id] = r;
        // the ranks on the stack are prefixes of one another; one that is no prefix of this token is a prefix of none that follows
        while (!chain.empty()) {
            const uint32_t top = sorted[chain.back()], lt = len_of(top);
            if (lt <= l && memcmp(ptr_of(top), ptr_of(id), lt) == 0) break;
            chain.pop_back();
        }
        if (!chain.empty()) parent[r] = chain.back();
        depth[r] = (l < HL_MAX_P ? 1u : 0u) + (parent[r] == HL_NONE ? 0u : depth[parent[r]]);
        if (depth[r] > HL_MAX_PART) return false;
        chain.push_back(r);
    }
    return true;
}

// the host's wavefront: `lanes` lanes one after the other (tests/hostsim/heal_sim.cpp owns the buffers and guards them)
struct HlHostWave {
    uint32_t n_lanes; uint8_t* pb[2]; uint32_t* regs; uint32_t* inf;
    uint32_t lanes() const { return n_lanes; }
    template <class F> uint64_t ballot(F f) const { uint64_t m = 0; for (uint32_t l = 0; l < n_lanes; l++) if (f(l)) m |= 1ull << l; return m; }
    template <class F> void each(F f) const { for (uint32_t l = 0; l < n_lanes; l++) f(l); }
    void sync() const {}
    uint8_t* pbuf(uint32_t k) const { return pb[k]; }
    uint32_t* info() const { return inf; }
    template <class F> uint32_t get(uint32_t k, F f) const { return f(k); }          // lane k's value, for all
    uint32_t& reg(uint32_t l, uint32_t j) const { return regs[l * HL_REGS + j]; }
};

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
struct HlDevWave {
    uint8_t* pb0; uint32_t* inf; uint32_t rk[HL_REGS];
    __device__ __forceinline__ uint32_t lanes() const { return HL_WAVE; }
    template <class F> __device__ __forceinline__ uint64_t ballot(F f) const { return __ballot(f(threadIdx.x & 63u)); }
    template <class F> __device__ __forceinline__ void each(F f) const { f(threadIdx.x & 63u); }
    __device__ __forceinline__ void sync() const { wave_lds_sync(); }
    __device__ __forceinline__ uint8_t* pbuf(uint32_t k) const { return pb0 + k * HL_MAX_P; }
    __device__ __forceinline__ uint32_t* info() const { return inf; }
    template <class F> __device__ __forceinline__ uint32_t get(uint32_t k, F f) const { return (uint32_t)__builtin_amdgcn_readlane((int)f(threadIdx.x & 63u), (int)k); }
    __device__ __forceinline__ uint32_t& reg(uint32_t, uint32_t j) { return rk[j]; }
};

template <bool BEGIN>
__global__ __launch_bounds__(HL_PLAN_NT) void k_heal_plan(HlIn a, HlTab t, HlOut out) {
    __shared__ __attribute__((aligned(8))) uint8_t s_p[HL_PLAN_NT / HL_WAVE][2 * HL_MAX_P];
    const uint32_t wv = threadIdx.x / HL_WAVE;
    const uint64_t b = (uint64_t)blockIdx.x * (HL_PLAN_NT / HL_WAVE) + wv;
    if (b >= a.n_seqs) return;                                                 // (a whole wavefront: nothing waits for it)
    HlDevWave w{s_p[wv], nullptr, {}};
    hl_plan_seq(w, t, a, BEGIN, b, out);
}

// grid (id ranges of HL_WG_IDS, sequence groups of spw over y and z).  Workgroup (0, 0, 0) also counts, for d_n, what the plan left: the constrained
// sequences and those that broke in this call.
__global__ __launch_bounds__(HL_FILL_NT) void k_heal_fill(HlTab t, const uint32_t* __restrict__ scr, uint64_t n_seqs, uint32_t spw, uint32_t n_words,
                                                          uint32_t flags, uint32_t* __restrict__ mask, int32_t* __restrict__ d_n) {
    __shared__ uint32_t s_inf[HL_FILL_NT / HL_WAVE][3 * HL_SPW_MAX];
    __shared__ uint32_t s_n[2];
    const uint32_t wv = threadIdx.x / HL_WAVE;
    if (d_n && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
        __syncthreads();
        uint32_t c = 0, k = 0;
        for (uint64_t s = threadIdx.x; s < n_seqs; s += HL_FILL_NT) {
            c += scr[s * HL_SCR] != HL_NONE ? 1u : 0u;
            k += (scr[s * HL_SCR + 2] & HL_BROKE) ? 1u : 0u;
        }
        if (c) atomicAdd(&s_n[0], c);
        if (k) atomicAdd(&s_n[1], k);
        __syncthreads();
        if (threadIdx.x < 2) d_n[threadIdx.x] = (int32_t)s_n[threadIdx.x];
    }
    const uint64_t s0 = ((uint64_t)blockIdx.z * gridDim.y + blockIdx.y) * spw, s1 = s0 + spw < n_seqs ? s0 + spw : n_seqs;
    const uint64_t id0 = (uint64_t)blockIdx.x * HL_WG_IDS + wv * HL_WAVE_IDS;
    if (id0 >= (uint64_t)n_words * 32) return;
    HlDevWave w{nullptr, s_inf[wv], {}};
    hl_fill_wave(w, t, scr, (uint32_t)id0, s0, s1, n_words, flags, [&](uint64_t s, uint32_t k, uint32_t v) { mask[s * n_words + k] = v; });
}
#endif  // __HIPCC__

}  // namespace spl
