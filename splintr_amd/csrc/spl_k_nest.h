// spl_k_nest.h -- spl_nest_index_device / spl_nest_step_device: NESTED LANGUAGES (JSON mode) for B sequences at once.
// The regex guide's byte automaton plus a small STACK per sequence: regular pieces inside nested brackets.  The caller's table is uint16
// trans[S][256], uint16 ret[n_ret][16], uint8 op[S][256], uint8 accept[S]; a configuration is (q, stack) with 4-bit symbols, at most
// max_depth deep.  One byte x, v = trans[q][x], o = op[q][x]:
//
//     o == 0          (v, stack) if v < S
//     o == 0x10 | y   PUSH: (v, stack + y) if v < S and depth < max_depth
//     o == 0x20       POP:  (ret[v][top], stack - top) if depth > 0, v < n_ret and ret[v][top] < S
//     anything else, and every "if" that fails: DEAD -- the kernels never index outside the table, whatever it holds.
//
// END may follow (q, stack) iff accept[q] and the stack is empty.  Walked WITHOUT the stack, a pair (q, id) TOUCHES iff the walk meets a
// byte with op != 0 before it dies or ends.
//
//     THE INDEX       int32 rows[S][stride] (bit t: ordinary, the walk ends alive and never touches), uint32 dep_off[S + 1], uint32
//                     dep_ids[dep_cap] (the touching ids of q, ascending, at dep_off[q] .. dep_off[q + 1]), uint8 some[S].
//     THE STATE ROW   NS_STATE_WORDS uint64: word 0 as spl_k_dfa.h's plus the depth in bits 24..30; words 1..4 the stack, level i (0 the
//                     bottom) in word 1 + i / 16 at bits 4 * (i % 16); nibbles at and above the depth are zero.
//     THE MASK ROW    rows[q] | the dependent ids of q whose walk from the real stack lives | the END bits where END may follow.
//
// k_nest_index has k_dfa_index's shape with two ballots per (state, 64 ids): alive-and-stack-free into rows, touching into a scratch
// bitmap of the same shape.  k_nest_count: a wavefront per state ORs its row (some) and popcounts its scratch row.  k_nest_scan: one
// workgroup, an exclusive scan of at most 4096 counts.  k_nest_write: a wavefront per state turns its scratch row into ascending ids.
// k_nest_step: ONE launch, a wavefront per sequence; the walk of the step's ids is serial and uniform with the stack in four 64-bit
// values; a state without dependent ids goes through df_write untouched (no LDS traffic); otherwise the row is written in PIECES of
// NS_PIECE words: the dependent ids that fall into a piece are walked 64 at a time, a lane an id with its own copy of the stack, the
// survivors ORed into the piece's overlay in LDS, and the piece is streamed out -- rows | overlay | END bits, every word stored once,
// nothing read back from the mask.  Nibbles are read and written by shifts and selects over the four words: no indexed local array, no
// scratch.  No atomics on global memory, no wait between workgroups.
//
// The first half is plain C++ over the WAVE POLICY of spl_k_heal.h, as spl_k_dfa.h's.
#pragma once
#include "spl_common.h"
#include "spl_k_dfa.h"

#ifndef SPL_NEST_PIECE
#define SPL_NEST_PIECE 1024            /* words of a row that one overlay in LDS covers: 32 768 ids, 4 KB -- eight wavefronts a SIMD still fit */
#endif

namespace spl {

// (the values of SPL_NEST_* in include/splintr_hip.h)
constexpr uint32_t NS_MAX_DEPTH = 64, NS_STATE_WORDS = 5, NS_MAX_RET = 4096;
constexpr uint32_t NS_PUSH = 0x10u, NS_POP = 0x20u;
constexpr uint32_t NS_PIECE = SPL_NEST_PIECE;
constexpr uint32_t NS_NT = 256, NS_SCAN_NT = 1024;
// a lane's registers in the index build, behind spl_k_dfa.h's: the two words of its state's touching row
constexpr uint32_t NS_R_TLO = 5, NS_R_THI = 6;
static_assert(NS_PIECE % 4 == 0 && NS_PIECE >= 4, "a piece is whole 16-byte accesses");
static_assert(NS_R_THI < HL_REGS && DF_R_HI < NS_R_TLO, "the wave policy's registers hold a lane's id and its four words");

struct NsTab { const uint16_t* trans; const uint16_t* ret; const uint8_t* op; const uint8_t* accept; uint32_t n_states, n_ret; };
struct NsIndex { const uint32_t* rows; const uint32_t* dep_off; const uint32_t* dep_ids; const uint8_t* some; uint32_t stride, dep_cap; };
// the stack: level i in word i / 16 at bits 4 * (i % 16); never indexed by a run-time value
struct NsStack { uint64_t w0, w1, w2, w3; uint32_t depth; };

SPL_HD NsTab ns_tab(const uint8_t* table, uint32_t n_states, uint32_t n_ret) {
    const uint8_t* ret = table + (size_t)n_states * 512;
    const uint8_t* op = ret + (size_t)n_ret * 32;
    return NsTab{reinterpret_cast<const uint16_t*>(table), reinterpret_cast<const uint16_t*>(ret), op, op + (size_t)n_states * 256, n_states, n_ret};
}
SPL_HD uint32_t ns_top(const NsStack& s) {                                    // (depth >= 1)
    const uint32_t i = s.depth - 1, k = i >> 4;
    const uint64_t w = k == 0 ? s.w0 : (k == 1 ? s.w1 : (k == 2 ? s.w2 : s.w3));
    return (uint32_t)(w >> (4 * (i & 15u))) & 15u;
}
// level `at` := y (0..15); the level held zero before
SPL_HD void ns_put(NsStack& s, uint32_t at, uint32_t y) {
    const uint32_t k = at >> 4;
    const uint64_t v = (uint64_t)y << (4 * (at & 15u));
    s.w0 |= k == 0 ? v : 0ull; s.w1 |= k == 1 ? v : 0ull; s.w2 |= k == 2 ? v : 0ull; s.w3 |= k == 3 ? v : 0ull;
}
SPL_HD void ns_clear(NsStack& s, uint32_t at) {
    const uint32_t k = at >> 4;
    const uint64_t v = ~(15ull << (4 * (at & 15u)));
    s.w0 &= k == 0 ? v : ~0ull; s.w1 &= k == 1 ? v : ~0ull; s.w2 &= k == 2 ? v : ~0ull; s.w3 &= k == 3 ? v : ~0ull;
}
// the nibbles below `depth` of a word that holds levels 16 k ..
SPL_HD uint64_t ns_keep(uint64_t w, uint32_t depth, uint32_t k) {
    if (depth <= 16 * k) return 0ull;
    const uint32_t n = depth - 16 * k;
    return n >= 16 ? w : (w & ((1ull << (4 * n)) - 1));
}

// one byte from (q, s), q < n_states: the next state (s moved with it) or DF_DEAD (s is then worthless)
SPL_HD uint32_t ns_next(const NsTab& d, uint32_t q, NsStack& s, uint32_t x, uint32_t max_depth) {
    const size_t at = (size_t)q * 256 + x;
    const uint32_t v = d.trans[at], o = d.op[at];
    if (o == 0) return v < d.n_states ? v : DF_DEAD;
    if ((o & 0xF0u) == NS_PUSH) {
        if (v >= d.n_states || s.depth >= max_depth) return DF_DEAD;
        ns_put(s, s.depth, o & 15u);
        s.depth++;
        return v;
    }
    if (o == NS_POP) {
        if (s.depth == 0 || v >= d.n_ret) return DF_DEAD;
#ifdef SPL_NEST_MUTANT_POP
        const uint32_t r = d.ret[(size_t)v * 16];
#else
        const uint32_t r = d.ret[(size_t)v * 16 + ns_top(s)];
#endif
        if (r >= d.n_states) return DF_DEAD;
        s.depth--;
        ns_clear(s, s.depth);
        return r;
    }
    return DF_DEAD;
}
// the n bytes at b from (q, s)
SPL_HD uint32_t ns_walk(const NsTab& d, uint32_t q, NsStack& s, const uint8_t* b, uint32_t n, uint32_t max_depth) {
    for (uint32_t i = 0; i < n; i++) {
        q = ns_next(d, q, s, b[i], max_depth);
        if (q == DF_DEAD) return DF_DEAD;
    }
    return q;
}
// bytes [from, n) from q WITHOUT the stack: 0 the walk dies, 1 it ends alive and touches nothing, 2 it touches
SPL_HD uint32_t ns_class_from(const NsTab& d, uint32_t q, const uint8_t* b, uint32_t from, uint32_t n) {
    for (uint32_t i = from; i < n; i++) {
        const size_t at = (size_t)q * 256 + b[i];
        if (d.op[at]) return 2u;
        const uint32_t v = d.trans[at];
        if (v >= d.n_states) return 0u;
        q = v;
    }
    return 1u;
}
// may an END id follow (q, s)
SPL_HD bool ns_ends(const NsTab& d, uint32_t q, const NsStack& s) {
#ifdef SPL_NEST_MUTANT_END
    (void)s;
    return d.accept[q] != 0;
#else
    return d.accept[q] != 0 && s.depth == 0;
#endif
}

// ------------------------------------------------------------------------------------------ the index
// df_index_wave's shape with two ballots: put(state, word, value) takes the rows, putt(state, word, value) the touching bitmap.
template <class W, class F, class G>
SPL_HD void ns_index_wave(W& w, const HlTab& t, const NsTab& d, uint64_t id0, uint32_t s0, uint32_t s1, uint32_t stride, F put, G putt) {
    const uint32_t wd0 = (uint32_t)(id0 >> 5), L = w.lanes();
    if (wd0 >= stride) return;
    for (uint32_t sb = s0; sb < s1; sb += L) {
        w.each([&](uint32_t l) { w.reg(l, DF_R_LO) = 0u; w.reg(l, DF_R_HI) = 0u; w.reg(l, NS_R_TLO) = 0u; w.reg(l, NS_R_THI) = 0u; });
        for (uint32_t i0 = 0; i0 < 64; i0 += L) {
            w.each([&](uint32_t l) {
                uint32_t len = 0;
                const uint64_t id = id0 + i0 + l;
                const uint8_t* p = (i0 + l < 64 && id <= 0xFFFFFFFFull) ? df_bytes(t, (uint32_t)id, len) : nullptr;
                w.reg(l, DF_R_LEN) = p ? len : 0u;
                w.reg(l, DF_R_OFF) = p ? (uint32_t)(p - t.tok_bytes) : 0u;
                w.reg(l, DF_R_B0) = p ? p[0] : 0u;
            });
            const uint32_t top = s1 - sb < L ? s1 - sb : L;
            for (uint32_t r = 0; r < top; r++) {
                const uint32_t q = sb + r;
                // the class of the lane's id from q: the first byte decides most pairs
                auto cls = [&](uint32_t l) -> uint32_t {
                    const uint32_t len = w.reg(l, DF_R_LEN);
                    if (!len) return 0u;
                    const size_t at = (size_t)q * 256 + w.reg(l, DF_R_B0);
                    if (d.op[at]) return 2u;
                    const uint32_t q1 = d.trans[at];
                    if (q1 >= d.n_states) return 0u;
                    return len == 1 ? 1u : ns_class_from(d, q1, t.tok_bytes + w.reg(l, DF_R_OFF), 1u, len);
                };
                w.each([&](uint32_t l) { w.reg(l, DF_R_B0) = (w.reg(l, DF_R_B0) & 0xFFu) | (cls(l) << 8); });
                const uint64_t m = w.ballot([&](uint32_t l) { return (w.reg(l, DF_R_B0) >> 8) == 1u; }) << i0;
                const uint64_t mt = w.ballot([&](uint32_t l) { return (w.reg(l, DF_R_B0) >> 8) == 2u; }) << i0;
                w.each([&](uint32_t l) {
                    w.reg(l, DF_R_B0) &= 0xFFu;
                    if (l == r) {
                        w.reg(l, DF_R_LO) |= (uint32_t)m; w.reg(l, DF_R_HI) |= (uint32_t)(m >> 32);
                        w.reg(l, NS_R_TLO) |= (uint32_t)mt; w.reg(l, NS_R_THI) |= (uint32_t)(mt >> 32);
                    }
                });
            }
        }
        w.each([&](uint32_t l) {
            if (sb + l >= s1) return;
            put(sb + l, wd0, w.reg(l, DF_R_LO));
            putt(sb + l, wd0, w.reg(l, NS_R_TLO));
            if (wd0 + 1 < stride) { put(sb + l, wd0 + 1, w.reg(l, DF_R_HI)); putt(sb + l, wd0 + 1, w.reg(l, NS_R_THI)); }
        });
    }
}
// One wavefront, state q: has its row a set bit, and how many bits has its touching row.  put(state, 0 | 1, count) by one lane.
template <class W, class F> SPL_HD void ns_count_wave(W& w, const uint32_t* rows, const uint32_t* touch, uint32_t stride, uint32_t q, F put) {
    const uint32_t L = w.lanes();
    const uint32_t* row = rows + (size_t)q * stride;
    const uint32_t* trow = touch + (size_t)q * stride;
    w.each([&](uint32_t l) {
        uint32_t v = 0, c = 0;
        for (uint32_t k = l; k < stride; k += L) { v |= row[k]; c += (uint32_t)__builtin_popcount(trow[k]); }
        w.reg(l, 0) = v; w.reg(l, 1) = c;
    });
    const uint64_t any = w.ballot([&](uint32_t l) { return w.reg(l, 0) != 0; });
    uint32_t n = 0;
    for (uint32_t k = 0; k < L; k++) n += w.get(k, [&](uint32_t l) { return w.reg(l, 1); });
    w.each([&](uint32_t l) { if (l == 0) put(q, any ? 1u : 0u, n); });
}
// One wavefront, state q: the set bits of its touching row as ascending ids at [lo, hi).  put(position, id): every entry stored once.
template <class W, class F> SPL_HD void ns_write_wave(W& w, const uint32_t* touch, uint32_t stride, uint32_t q, uint32_t lo, uint32_t hi, F put) {
    const uint32_t L = w.lanes();
    const uint32_t* trow = touch + (size_t)q * stride;
    uint32_t at = lo;
    for (uint32_t k0 = 0; k0 < stride; k0 += L) {
        uint64_t m = w.ballot([&](uint32_t l) { return k0 + l < stride && trow[k0 + l] != 0; });
        while (m) {                                                            // (most words of a touching row are zero)
            const uint32_t k = k0 + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t wv = trow[k];
            for (uint32_t j0 = 0; j0 < 32; j0 += L) {
                const uint64_t mb = w.ballot([&](uint32_t l) { return j0 + l < 32 && ((wv >> ((j0 + l) & 31u)) & 1u) != 0; });
                w.each([&](uint32_t l) {
                    if (!((mb >> l) & 1ull)) return;
                    const uint32_t pos = at + (uint32_t)__builtin_popcountll(mb & ((1ull << l) - 1));
                    if (pos < hi) put(pos, k * 32 + j0 + l);
                });
                at += (uint32_t)__builtin_popcountll(mb);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ the step
struct NsStep { uint32_t max_depth; };

// the row as it is loaded: spl_k_dfa.h's word 0; a constrained row whose depth is above max_depth is broken; nibbles at and above the depth are dropped
SPL_HD DfState ns_load(const NsTab& d, const NsStep& p, const uint64_t* row, NsStack& s) {
    const DfTab dt{d.trans, d.accept, d.n_states};
    DfState st = df_load(dt, row[0]);
    s = NsStack{0ull, 0ull, 0ull, 0ull, 0u};
    if (!st.con) return st;
    const uint32_t depth = (uint32_t)(row[0] >> 24) & 0x7Fu;
    if (depth > p.max_depth) { st.con = false; st.broken = true; st.q = 0; return st; }
    s.depth = depth;
    s.w0 = ns_keep(row[1], depth, 0); s.w1 = ns_keep(row[2], depth, 1); s.w2 = ns_keep(row[3], depth, 2); s.w3 = ns_keep(row[4], depth, 3);
    return st;
}
// word i of the row as it is written: a sequence that is not constrained has no stack
SPL_HD uint64_t ns_word(const DfState& st, const NsStack& s, uint32_t i) {
    if (i == 0) return df_word(st) | (st.con ? (uint64_t)s.depth << 24 : 0ull);
    if (!st.con) return 0ull;
    return i == 1 ? s.w0 : (i == 2 ? s.w1 : (i == 3 ? s.w2 : s.w3));
}
// one id of a constrained sequence: df_step_id's, over configurations
SPL_HD void ns_step_id(const HlTab& t, const NsTab& d, const NsStep& p, const DfIn& a, uint32_t id, bool is_id, DfState& st, NsStack& s) {
    uint32_t tl = 0;
    const uint8_t* tb = is_id ? df_bytes(t, id, tl) : nullptr;
    NsStack s1 = s;
    const uint32_t q1 = tb ? ns_walk(d, st.q, s1, tb, tl, p.max_depth) : DF_DEAD;
    if (q1 != DF_DEAD) { st.q = q1; s = s1; return; }
    st.con = false;
    if (is_id && df_is_end(a, id) && ns_ends(d, st.q, s)) st.done = true;
    else { st.broken = true; st.q = 0; }
}
// THE WALK of the step's ids, serial and the same for every lane: df_step_seq's, over configurations
SPL_HD void ns_step_seq(const HlTab& t, const NsTab& d, const NsStep& p, const DfIn& a, uint64_t b, DfState& st, NsStack& s) {
    const uint32_t n = df_row_n(a, b);
    for (uint32_t i = 0; i < n && st.con; i++) {
        uint32_t id;
        const bool is_id = df_read_id(a, b, i, id);
        ns_step_id(t, d, p, a, id, is_id, st, s);
    }
}
// does the dependent id `id` live from (q, s): a lane's own copy of the stack
SPL_HD bool ns_dep_lives(const HlTab& t, const NsTab& d, const NsStep& p, uint32_t q, const NsStack& s, uint32_t id) {
    uint32_t tl = 0;
    const uint8_t* tb = df_bytes(t, id, tl);
    if (!tb) return false;
#ifdef SPL_NEST_MUTANT_DEP
    NsStack c{0ull, 0ull, 0ull, 0ull, 0u};
    (void)s;
#else
    NsStack c = s;
#endif
    return ns_walk(d, q, c, tb, tl, p.max_depth) != DF_DEAD;
}
// the dependent ids of q as the index holds them, inside dep_cap whatever the offsets say
SPL_HD void ns_dep_range(const NsIndex& x, uint32_t q, uint32_t& lo, uint32_t& hi) {
    lo = x.dep_off[q]; hi = x.dep_off[q + 1];
    if (hi > x.dep_cap) hi = x.dep_cap;
    if (lo > hi) lo = hi;
}
// lives any dependent id of q (asked only where the row and the END bits are empty)
template <class W> SPL_HD bool ns_dep_any(W& w, const HlTab& t, const NsTab& d, const NsIndex& x, const NsStep& p, uint32_t n_words, uint32_t q, const NsStack& s) {
    uint32_t lo, hi;
    ns_dep_range(x, q, lo, hi);
    const uint32_t L = w.lanes();
    for (uint32_t c = lo; c < hi; c += L) {
        const uint64_t m = w.ballot([&](uint32_t l) {
            if (c + l >= hi) return false;
            const uint32_t id = x.dep_ids[c + l];
            return (id >> 5) < n_words && ns_dep_lives(t, d, p, q, s, id);
        });
        if (m) return true;
    }
    return false;
}
SPL_HD void ns_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);                                                            // (LDS; lanes of one wavefront may share a word)
#else
    *p |= v;
#endif
}
// THE ROW WRITE of a constrained state WITH dependent ids: piece by piece, the overlay in w.info() (NS_PIECE words)
template <class W, class O>
SPL_HD void ns_write_dep(W& w, const HlTab& t, const NsTab& d, const NsIndex& x, const NsStep& p, const DfIn& a, uint64_t b, uint32_t q, const NsStack& s,
                         bool ends, const O& out) {
    const uint32_t L = w.lanes();
    uint32_t* ov = w.info();
    const uint32_t* row = x.rows + (size_t)q * x.stride;
    uint32_t c, end;
    ns_dep_range(x, q, c, end);
    for (uint32_t p0 = 0; p0 < a.n_words; p0 += NS_PIECE) {
        const uint32_t pw = a.n_words - p0 < NS_PIECE ? a.n_words - p0 : NS_PIECE;
        const uint32_t lo = p0 * 32u, hi = (p0 + pw) * 32u;                    // (n_words <= 2^26: below 2^32)
        const bool has = c < end && x.dep_ids[c] < hi;
        if (has) {
            w.each([&](uint32_t l) { for (uint32_t i = l; i < pw; i += L) ov[i] = 0u; });
            w.sync();
            while (c < end) {
                // the lanes in front of the first id at or behind the piece's end take part; an id below the piece (no index has one) is passed over
                const uint64_t in = w.ballot([&](uint32_t l) { return c + l < end && x.dep_ids[c + l] < hi; });
                const uint32_t adv = ~in ? (uint32_t)__builtin_ctzll(~in) : 64u;
                if (!adv) break;
                w.each([&](uint32_t l) {
                    if (l >= adv) return;
                    const uint32_t id = x.dep_ids[c + l];
                    if (id >= lo && ns_dep_lives(t, d, p, q, s, id)) ns_or(ov + ((id - lo) >> 5), 1u << (id & 31u));
                });
                c += adv;
                if (adv < L) break;
            }
            w.sync();
        }
        w.each([&](uint32_t l) {
            if (a.v4) {
                for (uint32_t i = 4 * l; i < pw; i += 4 * L) {
                    const uint32_t* r = static_cast<const uint32_t*>(__builtin_assume_aligned(row + p0 + i, 16));
                    uint32_t v[4] = {r[0], r[1], r[2], r[3]};
                    if (has)
                        for (uint32_t j = 0; j < 4; j++) v[j] |= ov[i + j];
                    if (ends)
                        for (uint32_t j = 0; j < 4; j++) v[j] |= df_end_bits(a, p0 + i + j);
                    out.put4(b, p0 + i, v);
                }
            } else {
                for (uint32_t i = l; i < pw; i += L) out.put(b, p0 + i, row[p0 + i] | (has ? ov[i] : 0u) | (ends ? df_end_bits(a, p0 + i) : 0u));
            }
        });
        w.sync();                                                              // (the overlay is read before the next piece clears it)
    }
}
// df_write for the mask alone: the state row and live are this header's
template <class O> struct NsMaskOnly {
    const O& o;
    SPL_HD void state(uint64_t, uint64_t) const {}
    SPL_HD void alive(uint64_t, uint32_t) const {}
    SPL_HD void put(uint64_t b, uint32_t k, uint32_t v) const { o.put(b, k, v); }
    SPL_HD void put4(uint64_t b, uint32_t k, const uint32_t* v) const { o.put4(b, k, v); }
};
// THE SETTLE AND THE ROW WRITE of the configuration (st, s) a walk arrived at, into row b of the outputs.  out: state(b, word index,
// value), alive, put, put4.
template <class W, class O>
SPL_HD void ns_finish(W& w, const HlTab& t, const NsTab& d, const NsIndex& x, const NsStep& p, const DfIn& a, uint64_t b, DfState st, const NsStack& s,
                      const O& out) {
    bool ends = false;
    uint32_t n_dep = 0;
    if (st.con) {
        uint32_t lo, hi;
        ns_dep_range(x, st.q, lo, hi);
        n_dep = hi - lo;
        ends = a.n_end != 0 && ns_ends(d, st.q, s);
        // THE SETTLE: a constrained configuration with nothing to draw breaks
        if (!ends && !x.some[st.q] && !(n_dep && ns_dep_any(w, t, d, x, p, a.n_words, st.q, s))) { st.con = false; st.broken = true; st.q = 0; }
    }
    w.each([&](uint32_t l) {
        if (l < NS_STATE_WORDS) out.state(b, l, ns_word(st, s, l));
        if (l == 0) out.alive(b, st.con ? 1u : 0u);
    });
    if (w.lanes() < NS_STATE_WORDS)
        w.each([&](uint32_t l) { for (uint32_t i = l + w.lanes(); i < NS_STATE_WORDS; i += w.lanes()) out.state(b, i, ns_word(st, s, i)); });
    if (st.con && n_dep) { ns_write_dep(w, t, d, x, p, a, b, st.q, s, ends, out); return; }
    // no dependent id (or a row of ones): the regex guide's own row write
    const DfIndex dx{x.rows, x.some, x.stride};
    df_write(w, dx, a, b, st, st.con && ends, NsMaskOnly<O>{out});
}
// everything of sequence b: the walk, the settle and the row write
template <class W, class O>
SPL_HD void ns_seq(W& w, const HlTab& t, const NsTab& d, const NsIndex& x, const NsStep& p, const DfIn& a, uint64_t b, const O& out) {
    NsStack s;
    DfState st = ns_load(d, p, a.state_in + b * NS_STATE_WORDS, s);              // (state_out may be state_in: the row is read here, written once below)
    ns_step_seq(t, d, p, a, b, st, s);
    ns_finish(w, t, d, x, p, a, b, st, s, out);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// grid (groups of 256 ids, blocks of DF_INDEX_STATES states): a wavefront owns 64 ids
__global__ __launch_bounds__(DF_INDEX_NT) void k_nest_index(HlTab t, NsTab d, uint32_t stride, uint32_t* __restrict__ rows, uint32_t* __restrict__ touch) {
    const uint64_t id0 = ((uint64_t)blockIdx.x * (DF_INDEX_NT / DF_WAVE) + threadIdx.x / DF_WAVE) * DF_WAVE;
    const uint32_t s0 = blockIdx.y * DF_INDEX_STATES, s1 = s0 + DF_INDEX_STATES < d.n_states ? s0 + DF_INDEX_STATES : d.n_states;
    HlDevWave w{nullptr, nullptr, {}};
    ns_index_wave(w, t, d, id0, s0, s1, stride, [&](uint32_t q, uint32_t k, uint32_t v) { rows[(size_t)q * stride + k] = v; },
                  [&](uint32_t q, uint32_t k, uint32_t v) { touch[(size_t)q * stride + k] = v; });
}

// a wavefront per state, four a workgroup
__global__ __launch_bounds__(NS_NT) void k_nest_count(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ touch, uint32_t stride, uint32_t n_states,
                                                      uint8_t* __restrict__ some, uint32_t* __restrict__ cnt) {
    const uint32_t q = blockIdx.x * (NS_NT / DF_WAVE) + threadIdx.x / DF_WAVE;
    if (q >= n_states) return;                                                 // (a whole wavefront: nothing waits for it)
    HlDevWave w{nullptr, nullptr, {}};
    ns_count_wave(w, rows, touch, stride, q, [&](uint32_t s, uint32_t v, uint32_t n) { some[s] = (uint8_t)v; cnt[s] = n; });
}

// ONE workgroup: the exclusive scan of at most 4096 counts, four a thread; dep_off[n_states] is the total
__global__ __launch_bounds__(NS_SCAN_NT) void k_nest_scan(const uint32_t* __restrict__ cnt, uint32_t n_states, uint32_t* __restrict__ dep_off) {
    __shared__ uint32_t s_sum[NS_SCAN_NT];
    const uint32_t t = threadIdx.x;
    uint32_t c[4], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) { c[j] = 4 * t + j < n_states ? cnt[4 * t + j] : 0u; mine += c[j]; }
    s_sum[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < NS_SCAN_NT; d <<= 1) {
        const uint32_t v = t >= d ? s_sum[t - d] : 0u;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    uint32_t at = s_sum[t] - mine;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (4 * t + j < n_states) dep_off[4 * t + j] = at;
        at += c[j];
    }
    if (t == NS_SCAN_NT - 1) dep_off[n_states] = s_sum[t];
}

__global__ __launch_bounds__(NS_NT) void k_nest_write(const uint32_t* __restrict__ touch, uint32_t stride, uint32_t n_states, const uint32_t* __restrict__ dep_off,
                                                      uint32_t* __restrict__ dep_ids, uint32_t dep_cap) {
    const uint32_t q = blockIdx.x * (NS_NT / DF_WAVE) + threadIdx.x / DF_WAVE;
    if (q >= n_states) return;
    HlDevWave w{nullptr, nullptr, {}};
    const uint32_t lo = dep_off[q], hi = dep_off[q + 1] < dep_cap ? dep_off[q + 1] : dep_cap;
    ns_write_wave(w, touch, stride, q, lo, hi, [&](uint32_t pos, uint32_t id) { dep_ids[pos] = id; });
}

struct NsOut {
    uint64_t* state_out; uint32_t* mask; uint8_t* live; uint32_t n_words;
    __device__ __forceinline__ void state(uint64_t b, uint32_t i, uint64_t v) const { state_out[b * NS_STATE_WORDS + i] = v; }
    __device__ __forceinline__ void alive(uint64_t b, uint32_t v) const { if (live) live[b] = (uint8_t)v; }
    __device__ __forceinline__ void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; }
    __device__ __forceinline__ void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        *reinterpret_cast<uint4*>(mask + b * n_words + k) = make_uint4(v[0], v[1], v[2], v[3]);
    }
};

// grid (1, sequences over y and z), one wavefront a workgroup
__global__ __launch_bounds__(DF_WAVE) void k_nest_step(DfIn a, HlTab t, NsTab d, NsIndex x, NsStep p, NsOut out) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ov[NS_PIECE];
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    HlDevWave w{nullptr, s_ov, {}};
    ns_seq(w, t, d, x, p, a, b, out);
}
#endif  // __HIPCC__

}  // namespace spl
