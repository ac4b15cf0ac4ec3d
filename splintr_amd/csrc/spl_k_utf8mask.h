// spl_k_utf8mask.h -- spl_utf8_mask_device: UTF-8 CONTINUATION MASKS for B sequences at once.  Per sequence the stream
// decoder's state word (spl_k_stream.h) holds pending bytes p, the well-formed beginning of one character; the call writes the bitmask of
// the ids the sampler may draw so that the decoder neither stalls (hold mode) nor emits U+FFFD (replace mode):
//
//     bit t is 1 iff t is KNOWN (the vocabulary proper or the special map holds it) and p + e(t) is PREFIX-VALID: well-formed UTF-8,
//     optionally followed by the well-formed beginning of one character that reaches the end.  e(t): the bytes the device decode emits
//     for t -- nothing for a special id under DD_SKIP_SPECIAL; a known id with no bytes is allowed in every state.
//     Every other bit of the row is 0.  A stalled sequence (and a word that no decoder leaves: pending bytes that begin no character)
//     has nothing left to protect: its row is all ones and its live byte 0.
//
// p matters only through one of EIGHT CLASSES, the states of the automaton of Unicode's Table 3-7 that are not "dead":
//
//     0 start      1 / 2 / 3 one / two / three continuation bytes 80 .. BF owed      4 behind E0: A0 .. BF, then one      5 behind ED: 80 .. 9F,
//     then one      6 behind F0: 90 .. BF, then two      7 behind F4: 80 .. 8F, then two
//
// so a step is a ROW GATHER from a table built once per handle ON THE DEVICE (again after spl_add_special): UM_ROWS rows of `stride`
// words -- rows 0 .. 7 the ids of the vocabulary proper by class, rows 8 .. 15 the ids only the special map holds by class, row 16 those
// ids whatever the class; a row is vocabulary[class] | special[skip ? 16 : 8 + class].
//
// k_utf8_table: a lane owns an id and runs the eight starts over its bytes.  Only the first three bytes depend on the start: a run that
// began inside a character has passed the start state by then, so behind three bytes the eight runs are in at most four distinct states
// and the rest of the token is decided once per distinct state.  The wavefront's 64-bit ballots become two words each (lane k keeps word
// k & 1 of row k >> 1); whole words are stored, each exactly once.  k_utf8_mask: a lane owns a word of a row (four, as one 16-byte access,
// where the row width and the address allow it).  No atomics on global memory, no polling, no wait between workgroups.
//
// The first half is plain C++ over the WAVE POLICY of spl_k_heal.h (lanes(), ballot(f), each(f), reg): the kernels instantiate it with
// the hardware's wavefront, tests/hostsim/utf8mask_sim.cpp with HlHostWave -- the same text runs in both.
#pragma once
#include "spl_common.h"
#include "spl_k_decode_dev.h"
#include "spl_k_heal.h"
#include "spl_k_stream.h"

namespace spl {

// (the value of SPL_UTF8_AND in include/splintr_hip.h)
constexpr uint32_t UM_AND = 1u;
constexpr uint32_t UM_CLASSES = 8, UM_DEAD = 8, UM_FREE = 8;        // UM_DEAD: a run that met a byte the table forbids; UM_FREE: um_class of a stalled word
constexpr uint32_t UM_ROWS = 2 * UM_CLASSES + 1, UM_ROW_SP = UM_CLASSES, UM_ROW_SP_ANY = 2 * UM_CLASSES;
constexpr uint32_t UM_WAVE = 64, UM_NT = 256;
constexpr uint32_t UM_HEAD = 3;                                     // bytes of a token that depend on the start
static_assert(UM_ROWS * 2 <= UM_WAVE, "a lane per word of the wavefront's 64 ids in every row");

struct UmTab {                      // the table and its width: stride words a row (a multiple of four, zeros behind the largest known id)
    const uint32_t* rows; uint32_t stride;
};

// ------------------------------------------------------------------------------------------ the automaton (Table 3-7)
// one byte from state s (0 .. 7): the next state, UM_DEAD where the table forbids the byte
SPL_HD uint32_t um_step(uint32_t s, uint32_t x) {
    if (s == 0) {
        if (x < 0x80) return 0u;
        const uint32_t want = st_want(x);
        if (!want) return UM_DEAD;
        if (x == 0xE0) return 4u;
        if (x == 0xED) return 5u;
        if (x == 0xF0) return 6u;
        if (x == 0xF4) return 7u;
        return want;
    }
    if (s >= UM_DEAD) return UM_DEAD;
    uint32_t lo = 0x80, hi = 0xBF;
    if (s == 4) lo = 0xA0; else if (s == 5) hi = 0x9F; else if (s == 6) lo = 0x90; else if (s == 7) hi = 0x8F;
    if (x < lo || x > hi) return UM_DEAD;
    return s <= 3 ? s - 1 : (s <= 5 ? 1u : 2u);
}
// the class of a stream state word: its pending bytes run from the start; UM_FREE for a stalled word and for pending bytes that begin no
// character (a decoder leaves no such word)
SPL_HD uint32_t um_class(uint64_t word) {
    if (st_stalled(word)) return UM_FREE;
    const uint32_t n = st_count(word), p = st_pend(word);
    uint32_t s = 0;
    for (uint32_t i = 0; i < n; i++) {
        s = um_step(s, (p >> (8 * i)) & 0xFFu);
        if (s == UM_DEAD || s == 0) return UM_FREE;                          // (a byte the table forbids; a whole character or ASCII: no beginning)
    }
    return s;
}
// the classes from which the bytes b[0 .. n) are prefix-valid: bit c for class c.  The eight runs, four bits each, go through the first
// UM_HEAD bytes in step; the rest is run once from every distinct state they are left in.
SPL_HD uint32_t um_token_classes(const uint8_t* b, uint32_t n) {
    uint32_t runs = 0x76543210u;
    const uint32_t head = n < UM_HEAD ? n : UM_HEAD;
    for (uint32_t i = 0; i < head; i++) {
        const uint32_t x = b[i];
        uint32_t next = 0;
#pragma unroll
        for (uint32_t c = 0; c < UM_CLASSES; c++) next |= um_step((runs >> (4 * c)) & 15u, x) << (4 * c);
        runs = next;
    }
    uint32_t seen = 0, good = 0;                                   // per STATE behind the head: the rest was run from it, and survived
    uint32_t out = 0;
#pragma unroll
    for (uint32_t c = 0; c < UM_CLASSES; c++) {
        const uint32_t s = (runs >> (4 * c)) & 15u;
        if (s == UM_DEAD) continue;
        if (n > head && !((seen >> s) & 1u)) {
            seen |= 1u << s;
            uint32_t r = s;
            for (uint32_t i = head; i < n && r != UM_DEAD; i++) r = um_step(r, b[i]);
            if (r != UM_DEAD) good |= 1u << s;
        }
        if (n <= head || ((good >> s) & 1u)) out |= 1u << c;
    }
    return out;
}

// ------------------------------------------------------------------------------------------ one id's entry of the table
// bits 0 .. 7: the classes that allow the id; bit 8: only the special map holds it (bits 0 .. 7 are then those of its literal).  0: the id is
// not known.  present: one bit per id of the dense table, set for the vocabulary proper.
SPL_HD uint32_t um_id_entry(const DecTab& t, const uint32_t* present, uint64_t id) {
    if (id > 0xFFFFFFFFull) return 0u;
    uint32_t src = 0, len = 0;
    bool special = false;
    if (id <= t.max_id) {
        const uint32_t i = (uint32_t)id;
        if (!((present[i >> 5] >> (i & 31)) & 1u)) {
            if (!((t.sp_bits[i >> 5] >> (i & 31)) & 1u)) return 0u;     // a hole
            special = true;
        }
        src = t.tok_off[i];
        len = t.tok_off[i + 1] - src;
    } else {
        len = dd_id_span(t, 0u, (uint32_t)id, src);                    // (the side table: every entry is a special literal of one byte or more)
        if (!len) return 0u;
        special = true;
    }
    return um_token_classes(t.tok_bytes + src, len) | (special ? 0x100u : 0u);
}

// One wavefront, the ids [id0, id0 + 64): words id0 / 32 and id0 / 32 + 1 of every row of the table, below `stride`.  put(row, word, value).
template <class W, class F> SPL_HD void um_table_wave(W& w, const DecTab& t, const uint32_t* present, uint64_t id0, uint32_t stride, F put) {
    const uint32_t wd0 = (uint32_t)(id0 >> 5);
    if (wd0 >= stride) return;
    w.each([&](uint32_t l) { w.reg(l, 0) = um_id_entry(t, present, id0 + l); w.reg(l, 1) = 0u; });
    for (uint32_t r = 0; r < UM_ROWS; r++) {                       // ballot r is words wd0 and wd0 + 1 of row r
        const uint64_t m = w.ballot([&](uint32_t l) {
            const uint32_t e = w.reg(l, 0);
            const bool sp = (e & 0x100u) != 0;
            if (r == UM_ROW_SP_ANY) return sp;
            return (r < UM_ROW_SP ? !sp : sp) && ((e >> (r & 7u)) & 1u);
        });
        w.each([&](uint32_t l) { if ((l >> 1) == r) w.reg(l, 1) = (l & 1u) ? (uint32_t)(m >> 32) : (uint32_t)m; });
    }
    w.each([&](uint32_t l) { if (l < 2 * UM_ROWS && wd0 + (l & 1u) < stride) put(l >> 1, wd0 + (l & 1u), w.reg(l, 1)); });
}

// ------------------------------------------------------------------------------------------ a step: words of a row
// word k of the row of class c (0 .. 7); zeros behind the table's width
SPL_HD uint32_t um_row_word(const UmTab& t, uint32_t c, bool skip, uint32_t k) {
    if (k >= t.stride) return 0u;
    return t.rows[(uint64_t)c * t.stride + k] | t.rows[(uint64_t)(skip ? UM_ROW_SP_ANY : UM_ROW_SP + c) * t.stride + k];
}
// Words [k0, k0 + n) of sequence b's row and, from the lane that has k0 == 0, its live byte.  load(b, k) / store(b, k, v) reach the mask.
template <class L, class S, class V> SPL_HD void um_row_words(const UmTab& t, const uint64_t* state, uint64_t b, bool skip, uint32_t flags, uint32_t k0,
                                                            uint32_t n, uint32_t n_words, L load, S store, V alive) {
    const uint32_t c = um_class(state[b]);
    if (k0 == 0) alive(b, c != UM_FREE ? 1u : 0u);
    for (uint32_t k = k0; k < k0 + n && k < n_words; k++) {
        if (c == UM_FREE) { if (!(flags & UM_AND)) store(b, k, 0xFFFFFFFFu); continue; }      // (an AND with ones leaves the word alone: it is not touched)
        const uint32_t v = um_row_word(t, c, skip, k);
        store(b, k, (flags & UM_AND) ? (load(b, k) & v) : v);
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
__global__ __launch_bounds__(UM_NT) void k_utf8_table(DecTab t, const uint32_t* __restrict__ present, uint32_t stride, uint32_t* __restrict__ rows) {
    const uint64_t id0 = ((uint64_t)blockIdx.x * (UM_NT / UM_WAVE) + threadIdx.x / UM_WAVE) * UM_WAVE;
    HlDevWave w{nullptr, nullptr, {}};
    um_table_wave(w, t, present, id0, stride, [&](uint32_t r, uint32_t k, uint32_t v) { rows[(uint64_t)r * stride + k] = v; });
}

// grid (word groups of a row, sequences over y and z).  V4: a lane owns four words and moves them as one 16-byte access (n_words a multiple
// of four, the mask 16-byte aligned; the table's stride always is a multiple of four).
template <bool V4>
__global__ __launch_bounds__(UM_NT) void k_utf8_mask(UmTab t, const uint64_t* __restrict__ state, uint64_t n_seqs, uint32_t skip, uint32_t flags,
                                                     uint32_t n_words, uint32_t* __restrict__ mask, uint8_t* __restrict__ live) {
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= n_seqs) return;
    const uint32_t k0 = (blockIdx.x * UM_NT + threadIdx.x) * (V4 ? 4u : 1u);
    if (k0 >= n_words) return;
    auto alive = [&](uint64_t s, uint32_t v) { if (live) live[s] = (uint8_t)v; };
    if (!V4) {
        um_row_words(t, state, b, skip != 0, flags, k0, 1u, n_words, [&](uint64_t s, uint32_t k) { return mask[s * n_words + k]; },
                     [&](uint64_t s, uint32_t k, uint32_t v) { mask[s * n_words + k] = v; }, alive);
        return;
    }
    uint4* const at = reinterpret_cast<uint4*>(mask + b * n_words + k0);
    uint32_t have[4] = {0u, 0u, 0u, 0u}, v[4] = {0u, 0u, 0u, 0u};
    bool wrote = false;
    if ((flags & UM_AND) && !st_stalled(state[b])) { const uint4 m = *at; have[0] = m.x; have[1] = m.y; have[2] = m.z; have[3] = m.w; }
    um_row_words(t, state, b, skip != 0, flags, k0, 4u, n_words, [&](uint64_t, uint32_t k) { return have[k - k0]; },
                 [&](uint64_t, uint32_t k, uint32_t x) { v[k - k0] = x; wrote = true; }, alive);
    if (wrote) *at = make_uint4(v[0], v[1], v[2], v[3]);
}
#endif  // __HIPCC__

}  // namespace spl
