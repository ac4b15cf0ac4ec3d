// spl_k_pair.h -- from TWO CSRs (ids[T] u32, off[n + 1] u64 each) to one row per PAIR of documents, one launch:
//
//   k_collate_pair   rows[n_pairs, L]: row p = prefix + A' + middle + B' + suffix, the rest pad_id -- A' and B' the two documents of
//                    pair p cut to the budget L - k (k = the three fixed segments' ids), by one of three truncation rules; mask,
//                    token types, special-token mask, len, the ids kept of each side
//
// The kernel of spl_k_collate.h's family: a pure gather, every output element written once by the lane that owns it -- no atomics, no
// LDS, no workspace, no second pass.  A lane owns COL_VEC consecutive flat elements (one 16-byte store of int32, two of int64, one
// 4-byte store per byte array: col_store_group and col_store_bytes of spl_k_collate.h), a workgroup COL_SPAN of them; L need not be
// a multiple of COL_VEC: the elements of a lane's group are resolved one by one, and where the group crosses a row boundary the next
// pair is resolved again.  A side's document is named by an index array (or the pair's own number): a query that exists once in HBM
// is read by every pair that names it.
//
// The mapping from an output element to its source is the plain C++ of the first half of this file (values and pointers only; the one
// HIP builtin, CPAIR_UNIFORM, is the identity in a host build): tests/hostsim/pair_sim.cpp includes it in a g++ build and evaluates it
// for every output element; the kernel below calls exactly these functions.
//
// The options travel BY VALUE as a kernel argument (412 bytes of the kernarg segment), the three fixed segments packed one behind the
// other in ONE array.  A lane's group first resolves its elements -- a document's id, padding, or the NUMBER of a fixed entry -- and
// then walks the fixed entries once with a uniform index (cpair_fixed_pass): every entry is a scalar load of the kernel argument and a
// select per element, never an indexed read by a lane's own column and never a copy of the struct in scratch memory.
#pragma once
#include "spl_k_collate.h"

namespace spl {

// (the values of SPL_PAIR_* in include/splintr_hip.h; COL_I64 and COL_PAD_LEFT are shared with the collate family)
constexpr uint32_t CPAIR_MAX_FIXED = 32;
constexpr uint32_t CPAIR_KEEP_TAIL_A = 32u, CPAIR_KEEP_TAIL_B = 64u;
constexpr uint32_t CPAIR_LONGEST_FIRST = 0, CPAIR_ONLY_FIRST = 1, CPAIR_ONLY_SECOND = 2;

struct PairGeo {
    uint32_t flags, L, pad_id, trunc;
    uint32_t n_prefix, n_middle, n_suffix;
};
struct PairOpts {
    PairGeo g;
    uint32_t fixed[3 * CPAIR_MAX_FIXED];      // prefix, middle, suffix one behind the other: k = n_prefix + n_middle + n_suffix entries
};
// (host) the three segments of the C ABI's options into the one array the kernel walks
inline void cpair_set_fixed(PairOpts& o, const uint32_t* prefix, uint32_t n_prefix, const uint32_t* middle, uint32_t n_middle,
                            const uint32_t* suffix, uint32_t n_suffix) {
    uint32_t at = 0;
    o.g.n_prefix = n_prefix; o.g.n_middle = n_middle; o.g.n_suffix = n_suffix;
    for (uint32_t i = 0; i < 3 * CPAIR_MAX_FIXED; i++) o.fixed[i] = 0;
    for (uint32_t i = 0; i < n_prefix; i++) o.fixed[at++] = prefix[i];
    for (uint32_t i = 0; i < n_middle; i++) o.fixed[at++] = middle[i];
    for (uint32_t i = 0; i < n_suffix; i++) o.fixed[at++] = suffix[i];
}
// the two sides; a_idx / b_idx: the document of each pair (null: pair p takes document p)
struct PairSrc {
    const uint32_t* a_ids; const uint64_t* a_off;
    const uint32_t* b_ids; const uint64_t* b_off;
    const int32_t* a_idx; const int32_t* b_idx;
    uint32_t n_a, n_b;        // (document counts are below 2^31: the C ABI refuses more)
};
// one pair, resolved: where the kept ids of each side start in its ids array and how many they are
struct PairRow {
    uint64_t a0, b0;
    uint32_t na, nb;          // a', b'
    bool bad;                 // an index named no document of its side (that side is empty)
};

SPL_HD uint32_t cpair_k(const PairGeo& o) { return o.n_prefix + o.n_middle + o.n_suffix; }

// ------------------------------------------------------------------------------------------ spans and the grid
// One workgroup per span of COL_SPAN flat elements, and no loop over spans in the kernel: beyond the 2^31 - 1 workgroups of the grid's x
// the spans go on through its y and z (65 535 each), which covers every output the C ABI accepts (below 2^63 elements) in ONE launch.
// (k_collate_pad's loop over spans was tried first: the compiler hoists every flag test, null check and derived address out of it and
//  holds them all in scalar registers -- 20 to 30 spilled, whatever was done to the body.  The loop ran once for any output below
//  2^41 elements, more than a device's memory holds.)
SPL_HD void cpair_grid(uint64_t total, uint32_t& gx, uint32_t& gy, uint32_t& gz) {
    const uint64_t spans = (total + COL_SPAN - 1) / COL_SPAN, X = 0x7FFFFFFFull, YZ = 65535;
    gx = (uint32_t)(spans < X ? (spans ? spans : 1) : X);
    const uint64_t rest = (spans + gx - 1) / gx;               // (at most 2^22: spans is below 2^53)
    gy = (uint32_t)(rest < YZ ? (rest ? rest : 1) : YZ);
    gz = (uint32_t)((rest + gy - 1) / gy);
    if (gz == 0) gz = 1;
}
SPL_HD uint64_t cpair_span(uint32_t bx, uint32_t by, uint32_t bz, uint32_t gx, uint32_t gy) {
    return (uint64_t)bx + (uint64_t)gx * ((uint64_t)by + (uint64_t)gy * bz);
}

// ------------------------------------------------------------------------------------------ lengths and truncation
// (la, lb) cut to the budget B.  LONGEST_FIRST is Hugging Face's sequential rule -- while a' + b' > B remove one id from the longer
// side, from B on a tie -- in closed form: the rule never cuts a side that is shorter than its half (hA = ceil(B / 2) for A, which
// wins the ties, hB = floor(B / 2) for B), and cuts two sides that both exceed their halves down to exactly these.
SPL_HD void cpair_trunc(uint64_t la, uint64_t lb, uint32_t B, uint32_t trunc, uint32_t& na, uint32_t& nb) {
    if (la + lb <= B) { na = (uint32_t)la; nb = (uint32_t)lb; return; }       // (document lengths are far below 2^63: the sum does not wrap)
    if (trunc == CPAIR_ONLY_SECOND) { na = la < B ? (uint32_t)la : B; nb = B - na; return; }      // (lb > B - na here)
    if (trunc == CPAIR_ONLY_FIRST) { nb = lb < B ? (uint32_t)lb : B; na = B - nb; return; }
    const uint32_t hB = B / 2, hA = B - hB;
    if (la < hA) { na = (uint32_t)la; nb = B - na; }
    else if (lb <= hB) { nb = (uint32_t)lb; na = B - nb; }
    else { na = hA; nb = hB; }
}

// document i of one side: [o0, o1) of its ids; an index outside 0 .. n - 1 names the empty document and is reported
SPL_HD void cpair_doc(const uint64_t* off, uint32_t n, const int32_t* idx, uint64_t p, uint64_t& o0, uint64_t& len, bool& bad) {
    uint32_t i = (uint32_t)p;                                     // (idx == null: p < n, the host has checked n_pairs <= n; p < 2^31)
    if (idx) i = (uint32_t)idx[p];
    o0 = 0; len = 0;
    if (i >= n) { bad = true; return; }                           // (a negative index is at least 2^31 as an unsigned number, n is below that)
    o0 = off[i];
    len = off[i + 1] - o0;
}

SPL_HD PairRow cpair_resolve(const PairSrc& s, uint64_t p, const PairGeo& o) {
    PairRow r;
    uint64_t la, lb;
    r.bad = false;
    cpair_doc(s.a_off, s.n_a, s.a_idx, p, r.a0, la, r.bad);
    cpair_doc(s.b_off, s.n_b, s.b_idx, p, r.b0, lb, r.bad);
    cpair_trunc(la, lb, o.L - cpair_k(o), o.trunc, r.na, r.nb);
    r.a0 += (la - r.na) * ((o.flags / CPAIR_KEEP_TAIL_A) & 1u);     // KEEP_TAIL: truncation drops the FRONT of that side's document
    r.b0 += (lb - r.nb) * ((o.flags / CPAIR_KEEP_TAIL_B) & 1u);
    return r;
}

// ------------------------------------------------------------------------------------------ one element
constexpr uint32_t CPAIR_MASK = 1u, CPAIR_TYPE = 2u, CPAIR_SPECIAL = 4u;
constexpr uint32_t CPAIR_NOT_FIXED = 0xFFFFFFFFu;
// column c of the row of a resolved pair: returns the element's bits (mask, token type, special).  val: the value of padding and of a
// document's id; fix: for an entry of a fixed segment its number in PairOpts::fixed (val is then set by cpair_fixed_pass).
SPL_HD uint32_t cpair_elem(const PairSrc& s, const PairRow& r, uint32_t c, const PairGeo& o, uint32_t& val, uint32_t& fix) {
    const uint32_t used = cpair_k(o) + r.na + r.nb;
    const uint32_t lead = (o.L - used) * ((o.flags / COL_PAD_LEFT) & 1u);
    val = o.pad_id; fix = CPAIR_NOT_FIXED;
    const uint32_t q = c - lead;
    if (c < lead || q >= used) return CPAIR_SPECIAL;                              // padding: mask 0, type 0, special 1
    const uint32_t e1 = o.n_prefix, e2 = e1 + r.na, e3 = e2 + o.n_middle, e4 = e3 + r.nb;      // the ends of prefix, A', middle, B'
    const uint32_t type = q >= e3 ? CPAIR_TYPE : 0u;
    const bool in_a = q >= e1 && q < e2, in_b = q >= e3 && q < e4;
    if (in_a || in_b) {
        const uint32_t* src = in_a ? s.a_ids + (r.a0 + (q - e1)) : s.b_ids + (r.b0 + (q - e3));
        val = *src;
        return CPAIR_MASK | type;
    }
    fix = q < e1 ? q : (q < e3 ? q - r.na : q - r.na - r.nb);
    return CPAIR_MASK | CPAIR_SPECIAL | type;
}

// The values of a group's fixed entries: ONE walk over the k entries with an index that is uniform over the wavefront (on the device
// made so explicitly: fixed[j] is then a scalar load of the kernel argument), a select per element.
#if defined(__HIP_DEVICE_COMPILE__)
#define CPAIR_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define CPAIR_UNIFORM(x) (x)
#endif
SPL_HD void cpair_fixed_pass(const uint32_t* fixed, uint32_t k, const uint32_t fix[COL_VEC], uint32_t v[COL_VEC]) {
    if ((fix[0] & fix[1] & fix[2] & fix[3]) == CPAIR_NOT_FIXED) return;
    static_assert(COL_VEC == 4, "a group is four elements");
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t x = fixed[CPAIR_UNIFORM(j)];
#pragma unroll
        for (uint32_t i = 0; i < COL_VEC; i++) v[i] = fix[i] == j ? x : v[i];
    }
}

// One lane's group: n (1..COL_VEC) flat elements from e0 on.  v[i]: the values; m / ty / sp: the mask, token-type and special bytes,
// byte i for element i.  len[p], kept[2p], kept[2p + 1] and -- for a pair with a bad index -- status[0] = 1 are stored by the lane
// that owns column 0 of row p (len, kept: null if not wanted).
SPL_HD void cpair_group(const PairSrc& s, uint64_t e0, uint32_t n, const PairGeo& o, const uint32_t* fixed, uint32_t v[COL_VEC], uint32_t& m, uint32_t& ty,
                        uint32_t& sp, int32_t* len, int32_t* kept, uint32_t* status) {
    uint64_t p; uint32_t c;
    col_rowcol(e0, o.L, p, c);
    uint32_t fix[COL_VEC], bits = 0;              // bits: byte i holds element i's CPAIR_MASK | _TYPE | _SPECIAL
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) { v[i] = o.pad_id; fix[i] = CPAIR_NOT_FIXED; }
    // row by row (one row, or two where the group crosses a boundary; more only for rows shorter than the group): the pair is resolved
    // once per row, and elements first .. first + cnt - 1 of the group are its columns c .. c + cnt - 1
    for (uint32_t first = 0; first < n; p++, c = 0) {
        const PairRow r = cpair_resolve(s, p, o);
        const uint32_t room = o.L - c, cnt = n - first < room ? n - first : room;
        if (len) { if (c == 0) len[p] = (int32_t)(cpair_k(o) + r.na + r.nb); }          // (the uniform test first)
        if (kept) { if (c == 0) { kept[2 * p] = (int32_t)r.na; kept[2 * p + 1] = (int32_t)r.nb; } }
        if (c == 0 && r.bad) status[0] = 1u;
#pragma unroll
        for (uint32_t i = 0; i < COL_VEC; i++) {
            if (i < first || i - first >= cnt) continue;
            bits |= cpair_elem(s, r, c + (i - first), o, v[i], fix[i]) << (8 * i);
        }
        first += cnt;
    }
    m = bits & 0x01010101u; ty = (bits >> 1) & 0x01010101u; sp = (bits >> 2) & 0x01010101u;
    cpair_fixed_pass(fixed, cpair_k(o), fix, v);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernel
// grid: cpair_grid(n_pairs * L) -- one workgroup per span of COL_SPAN flat elements
template <bool I64>
__global__ __launch_bounds__(COL_NT) void k_collate_pair(PairSrc s, uint32_t n_pairs, PairOpts o, void* __restrict__ rows,
                                                         uint8_t* __restrict__ mask, uint8_t* __restrict__ type, uint8_t* __restrict__ special,
                                                         int32_t* __restrict__ len, int32_t* __restrict__ kept, uint32_t* __restrict__ status) {
    const uint64_t total = (uint64_t)n_pairs * o.g.L;
    const uint64_t e0 = cpair_span(blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y) * COL_SPAN + (uint64_t)threadIdx.x * COL_VEC;
    if (e0 >= total) return;
    const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
    uint32_t v[COL_VEC], m, ty, sp;
    cpair_group(s, e0, n, o.g, o.fixed, v, m, ty, sp, len, kept, status);
    col_store_group<I64>(rows, e0, n, v);               // (the final group may be partial: nothing is written past n_pairs * L)
    col_store_bytes(mask, e0, n, m);                    // (an output that is not wanted: one uniform test each)
    col_store_bytes(type, e0, n, ty);
    col_store_bytes(special, e0, n, sp);
}
#endif  // __HIPCC__

}  // namespace spl
