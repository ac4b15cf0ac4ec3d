// spl_k_dfa.h -- spl_dfa_index_device / spl_dfa_step_device: the REGEX GUIDE for B sequences at once.  The answer of a
// sequence matches a regular expression, given as a deterministic automaton over BYTES (the caller's table: uint16 trans[S][256], then
// uint8 accept[S]; a value >= S is DEAD -- the kernels never index outside the table, whatever it holds).  With walk(q, b(t)) following
// trans byte by byte, DEAD as soon as a step is:
//
//     THE INDEX       int32 rows[S][stride], then uint8 some[S]: bit t of row q is 1 iff t is ORDINARY (spl_k_heal.h) and walk(q, b(t)) is
//                     not DEAD; every other bit is 0, up to 32 * stride; some[q] is 1 iff row q has a set bit.
//     THE STATE ROW   one uint64: bits 0..15 q, bit 16 constrained, bit 17 broken, bit 18 done; zero is free.
//     STEP            per id while the sequence is constrained: ordinary with walk(q, b(t)) = q' alive: q := q'; otherwise an END id
//                     with accept[q]: done; anything else: broken.
//     THE MASK ROW    free, done, broken: ones.  constrained: rows[q] | the END bits if accept[q]; where that is empty the sequence
//                     breaks in this call and its row is ones.
//
// k_dfa_index: a lane owns an id, a wavefront 64 ids -- two words of every row.  The id's span is loaded once per batch of 64 states; per
// state the FIRST byte is tested before anything else (most (state, id) pairs die there), the ballot is the two words, and lane r keeps the
// words of the batch's state r: every word is stored exactly once.  k_dfa_some: a wavefront per state ORs its row.  k_dfa_step: ONE launch,
// a wavefront owns a sequence; the walk of the step's ids is serial and uniform, the row is then copied by all lanes, 16 bytes a lane where
// the row width and the addresses allow it, the END bits ORed into a word's value before its one store.  No LDS, no scratch, no atomics on
// global memory, no wait between workgroups.
//
// The first half is plain C++ over the WAVE POLICY of spl_k_heal.h (lanes(), ballot(f), each(f), reg): the kernels instantiate it with the
// hardware's wavefront, tests/hostsim/dfa_sim.cpp with HlHostWave and a run-time lane count -- the same text runs in both.
#pragma once
#include "spl_common.h"
#include "spl_k_heal.h"

namespace spl {

// (the values of SPL_DFA_* in include/splintr_hip.h)
constexpr uint32_t DF_KEEP_FREE = 2u, DF_I64 = 4u;
constexpr uint32_t DF_DEAD = 0xFFFFu, DF_MAX_STATES = 4096, DF_STATE_WORDS = 1, DF_MAX_END = 8;
constexpr uint64_t DF_CON = 1ull << 16, DF_BROKEN = 1ull << 17, DF_DONE = 1ull << 18;
constexpr uint32_t DF_WAVE = 64, DF_INDEX_NT = 256;
constexpr uint32_t DF_INDEX_STATES = 256;                          // states a workgroup of k_dfa_index takes its 256 ids through
// a lane's registers in the index build: its id's byte offset, length (0: not ordinary) and first byte; the two words of its state
constexpr uint32_t DF_R_OFF = 0, DF_R_LEN = 1, DF_R_B0 = 2, DF_R_LO = 3, DF_R_HI = 4;
static_assert(DF_R_HI < HL_REGS, "the wave policy's registers hold a lane's id and words");

struct DfTab { const uint16_t* trans; const uint8_t* accept; uint32_t n_states; };
struct DfIndex { const uint32_t* rows; const uint8_t* some; uint32_t stride; };
struct DfIn {
    const void* ids; const int32_t* len; const uint64_t* state_in; uint64_t n_seqs;
    uint32_t row_len, flags, n_words, v4, n_end;                  // v4: n_words is a multiple of four, the mask and the index 16-byte aligned
    uint32_t end_ids[DF_MAX_END];
};

SPL_HD uint32_t df_stride(uint32_t n_words) { return (n_words + 3u) & ~3u; }
// one byte from state q (< n_states): the next state, DF_DEAD for every value that is no state
SPL_HD uint32_t df_next(const DfTab& d, uint32_t q, uint32_t x) {
    const uint32_t v = d.trans[(size_t)q * 256 + x];
    return v < d.n_states ? v : DF_DEAD;
}
// bytes [from, n) from state q
SPL_HD uint32_t df_walk_from(const DfTab& d, uint32_t q, const uint8_t* b, uint32_t from, uint32_t n) {
    for (uint32_t i = from; i < n; i++) {
        const uint32_t nx = df_next(d, q, b[i]);
#ifdef SPL_DFA_MUTANT_FIRST
        if (nx == DF_DEAD) { if (i == 0) return DF_DEAD; continue; }
#else
        if (nx == DF_DEAD) return DF_DEAD;
#endif
        q = nx;
    }
    return q;
}
// may an END id follow state q
SPL_HD bool df_ends(const DfTab& d, uint32_t q) {
#ifdef SPL_DFA_MUTANT_END
    (void)d; (void)q;
    return true;
#else
    return d.accept[q] != 0;
#endif
}
// the bytes of an ORDINARY id (len >= 1); nullptr for every other value
SPL_HD const uint8_t* df_bytes(const HlTab& t, uint32_t id, uint32_t& len) {
    len = 0;
    if (hl_rank32(t, id) == HL_NONE) return nullptr;
    const uint32_t o = t.tok_off[id];
    len = t.tok_off[id + 1] - o;
    return t.tok_bytes + o;
}
SPL_HD bool df_is_end(const DfIn& a, uint32_t id) {
    for (uint32_t i = 0; i < a.n_end; i++)
        if (a.end_ids[i] == id) return true;
    return false;
}
SPL_HD uint32_t df_row_n(const DfIn& a, uint64_t b) {
    if (!a.len) return a.row_len;
    const int32_t l = a.len[b];
    return l < 0 ? 0u : ((uint32_t)l > a.row_len ? a.row_len : (uint32_t)l);
}

// ------------------------------------------------------------------------------------------ the index
// One wavefront, the ids [id0, id0 + 64) and the states [s0, s1): words id0 / 32 and id0 / 32 + 1 of their rows, below `stride`.  The
// states go in batches of `lanes`; lane r collects the two words of the batch's state r over the wavefront's ids (the hardware's wavefront
// has them in one ballot; fewer lanes take the 64 ids in turns).  put(state, word, value).
template <class W, class F> SPL_HD void df_index_wave(W& w, const HlTab& t, const DfTab& d, uint64_t id0, uint32_t s0, uint32_t s1, uint32_t stride, F put) {
    const uint32_t wd0 = (uint32_t)(id0 >> 5), L = w.lanes();
    if (wd0 >= stride) return;
    for (uint32_t sb = s0; sb < s1; sb += L) {
        w.each([&](uint32_t l) { w.reg(l, DF_R_LO) = 0u; w.reg(l, DF_R_HI) = 0u; });
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
                const uint64_t m = w.ballot([&](uint32_t l) {
                    const uint32_t len = w.reg(l, DF_R_LEN);
                    if (!len) return false;
                    const uint32_t q1 = df_next(d, q, w.reg(l, DF_R_B0));             // the first byte decides most pairs
                    if (q1 == DF_DEAD) return false;
#ifdef SPL_DFA_MUTANT_FIRST
                    return df_walk_from(d, q, t.tok_bytes + w.reg(l, DF_R_OFF), 0u, len) != DF_DEAD;
#else
                    return len == 1 || df_walk_from(d, q1, t.tok_bytes + w.reg(l, DF_R_OFF), 1u, len) != DF_DEAD;
#endif
                }) << i0;
                w.each([&](uint32_t l) { if (l == r) { w.reg(l, DF_R_LO) |= (uint32_t)m; w.reg(l, DF_R_HI) |= (uint32_t)(m >> 32); } });
            }
        }
        w.each([&](uint32_t l) {
            if (sb + l >= s1) return;
            put(sb + l, wd0, w.reg(l, DF_R_LO));
            if (wd0 + 1 < stride) put(sb + l, wd0 + 1, w.reg(l, DF_R_HI));
        });
    }
}
// One wavefront, state q: has its row a set bit.  rows: the index as df_index_wave left it.  put(state, 0 | 1) by one lane.
template <class W, class F> SPL_HD void df_some_wave(W& w, const uint32_t* rows, uint32_t stride, uint32_t q, F put) {
    const uint32_t L = w.lanes();
    const uint32_t* row = rows + (size_t)q * stride;
    const uint64_t any = w.ballot([&](uint32_t l) {
        uint32_t v = 0;
        for (uint32_t k = l; k < stride; k += L) v |= row[k];
        return v != 0;
    });
    w.each([&](uint32_t l) { if (l == 0) put(q, any ? 1u : 0u); });
}

// ------------------------------------------------------------------------------------------ the step
struct DfState { uint32_t q; bool con, broken, done; };

// the row as it is loaded: broken wins over done, done over constrained; a constrained row whose q is no state is broken
SPL_HD DfState df_load(const DfTab& d, uint64_t word) {
    DfState s{(uint32_t)word & 0xFFFFu, false, (word & DF_BROKEN) != 0, false};
    s.done = !s.broken && (word & DF_DONE) != 0;
    s.con = !s.broken && !s.done && (word & DF_CON) != 0;
    if (s.con && s.q >= d.n_states) { s.con = false; s.broken = true; }
    if (!s.done && !s.con) s.q = 0;
    return s;
}
SPL_HD uint64_t df_word(const DfState& s) {
    if (s.broken) return DF_BROKEN;
    if (s.done) return (uint64_t)s.q | DF_DONE;
    return s.con ? ((uint64_t)s.q | DF_CON) : 0ull;
}
// one id of a constrained sequence: an ordinary id that walks moves q; an END id behind an accepting state ends the sequence; anything else breaks it
SPL_HD void df_step_id(const HlTab& t, const DfTab& d, const DfIn& a, uint32_t id, bool is_id, DfState& s) {
    uint32_t tl = 0;
    const uint8_t* tb = is_id ? df_bytes(t, id, tl) : nullptr;
    const uint32_t q1 = tb ? df_walk_from(d, s.q, tb, 0u, tl) : DF_DEAD;
    if (q1 != DF_DEAD) { s.q = q1; return; }
    s.con = false;
    if (is_id && df_is_end(a, id) && df_ends(d, s.q)) s.done = true;
    else { s.broken = true; s.q = 0; }
}
// entry i of row b of the ids: false for an int64 value outside 32 bits (id is then its low half, which no rule reads)
SPL_HD bool df_read_id(const DfIn& a, uint64_t b, uint32_t i, uint32_t& id) {
    if (a.flags & DF_I64) {
        const uint64_t v = static_cast<const uint64_t*>(a.ids)[b * a.row_len + i];
        id = (uint32_t)v;
        return (v >> 32) == 0;
    }
    id = static_cast<const uint32_t*>(a.ids)[b * a.row_len + i];
    return true;
}
// THE WALK: the row's valid ids in order, while the sequence is constrained (the same for every lane: a serial walk)
SPL_HD void df_step_seq(const HlTab& t, const DfTab& d, const DfIn& a, uint64_t b, DfState& s) {
    const uint32_t n = df_row_n(a, b);
    for (uint32_t i = 0; i < n && s.con; i++) {
        uint32_t id;
        const bool is_id = df_read_id(a, b, i, id);
        df_step_id(t, d, a, id, is_id, s);
    }
}
// the END bits that fall into word k
SPL_HD uint32_t df_end_bits(const DfIn& a, uint32_t k) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < a.n_end; i++)
        if ((a.end_ids[i] >> 5) == k) v |= 1u << (a.end_ids[i] & 31u);
    return v;
}

// THE SETTLE: the state a call leaves behind the state it arrived at -- a constrained state with nothing to draw breaks.  Returns whether
// the END bits belong into the row.
SPL_HD bool df_settle(const DfTab& d, const DfIndex& x, const DfIn& a, DfState& s) {
    if (!s.con) return false;
    const bool ends = a.n_end != 0 && df_ends(d, s.q);
    if (!ends && !x.some[s.q]) { s.con = false; s.broken = true; s.q = 0; }       // nothing to draw: the sequence breaks, its row is ones
    return ends;
}
// THE ROW WRITE: the state row, live and the mask row of a settled state.  put(b, word, value) and put4(b, word, four values) store.
template <class W, class O> SPL_HD void df_write(W& w, const DfIndex& x, const DfIn& a, uint64_t b, const DfState& s, bool ends, const O& out) {
    const uint32_t L = w.lanes();
    const uint64_t word = df_word(s);
    w.each([&](uint32_t l) { if (l == 0) { out.state(b, word); out.alive(b, s.con ? 1u : 0u); } });
    if (!s.con) {
        if (a.flags & DF_KEEP_FREE) return;
        const uint32_t one[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        w.each([&](uint32_t l) {
            if (a.v4) for (uint32_t i = 4 * l; i < a.n_words; i += 4 * L) out.put4(b, i, one);
            else for (uint32_t i = l; i < a.n_words; i += L) out.put(b, i, 0xFFFFFFFFu);
        });
        return;
    }
    const uint32_t* row = x.rows + (size_t)s.q * x.stride;
    w.each([&](uint32_t l) {
        if (a.v4) {
            for (uint32_t i = 4 * l; i < a.n_words; i += 4 * L) {
                const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(row + i, 16));
                uint32_t v[4] = {p[0], p[1], p[2], p[3]};
                if (ends)
                    for (uint32_t j = 0; j < 4; j++) v[j] |= df_end_bits(a, i + j);
                out.put4(b, i, v);
            }
        } else {
            for (uint32_t i = l; i < a.n_words; i += L) out.put(b, i, row[i] | (ends ? df_end_bits(a, i) : 0u));
        }
    });
}
// everything of sequence b: the walk, the settle and the row write (spl_k_dfa_jump.h puts the jump between the first two)
template <class W, class O> SPL_HD void df_seq(W& w, const HlTab& t, const DfTab& d, const DfIndex& x, const DfIn& a, uint64_t b, const O& out) {
    DfState s = df_load(d, a.state_in[b]);                                     // (state_out may be state_in: the row is read here, written once below)
    df_step_seq(t, d, a, b, s);
    const bool ends = df_settle(d, x, a, s);
    df_write(w, x, a, b, s, ends, out);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// grid (groups of 256 ids, blocks of DF_INDEX_STATES states): a wavefront owns 64 ids
__global__ __launch_bounds__(DF_INDEX_NT) void k_dfa_index(HlTab t, DfTab d, uint32_t stride, uint32_t* __restrict__ rows) {
    const uint64_t id0 = ((uint64_t)blockIdx.x * (DF_INDEX_NT / DF_WAVE) + threadIdx.x / DF_WAVE) * DF_WAVE;
    const uint32_t s0 = blockIdx.y * DF_INDEX_STATES, s1 = s0 + DF_INDEX_STATES < d.n_states ? s0 + DF_INDEX_STATES : d.n_states;
    HlDevWave w{nullptr, nullptr, {}};
    df_index_wave(w, t, d, id0, s0, s1, stride, [&](uint32_t q, uint32_t k, uint32_t v) { rows[(size_t)q * stride + k] = v; });
}

// a wavefront per state, four a workgroup
__global__ __launch_bounds__(DF_INDEX_NT) void k_dfa_some(const uint32_t* __restrict__ rows, uint32_t stride, uint32_t n_states, uint8_t* __restrict__ some) {
    const uint32_t q = blockIdx.x * (DF_INDEX_NT / DF_WAVE) + threadIdx.x / DF_WAVE;
    if (q >= n_states) return;                                                 // (a whole wavefront: nothing waits for it)
    HlDevWave w{nullptr, nullptr, {}};
    df_some_wave(w, rows, stride, q, [&](uint32_t s, uint32_t v) { some[s] = (uint8_t)v; });
}

struct DfOut {
    uint64_t* state_out; uint32_t* mask; uint8_t* live; uint32_t n_words;
    __device__ __forceinline__ void state(uint64_t b, uint64_t v) const { state_out[b] = v; }
    __device__ __forceinline__ void alive(uint64_t b, uint32_t v) const { if (live) live[b] = (uint8_t)v; }
    __device__ __forceinline__ void put(uint64_t b, uint32_t k, uint32_t v) const { mask[b * n_words + k] = v; }
    __device__ __forceinline__ void put4(uint64_t b, uint32_t k, const uint32_t* v) const {
        *reinterpret_cast<uint4*>(mask + b * n_words + k) = make_uint4(v[0], v[1], v[2], v[3]);
    }
};

// grid (1, sequences over y and z), one wavefront a workgroup
__global__ __launch_bounds__(DF_WAVE) void k_dfa_step(DfIn a, HlTab t, DfTab d, DfIndex x, DfOut out) {
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    HlDevWave w{nullptr, nullptr, {}};
    df_seq(w, t, d, x, a, b, out);
}
#endif  // __HIPCC__

}  // namespace spl
