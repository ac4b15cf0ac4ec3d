// spl_k_draft.h -- spl_dfa_draft_device / spl_nest_draft_device: DRAFT VERIFICATION for the regex guide and the nest guide (DESIGN.md
// 4.21).  A speculative sampler hands the verifier a DRAFT of up to 64 ids per sequence -- a chain, or a tree given by a parent per node
// -- and the model's one forward pass yields logits in front of every one of them.  From ONE state row per sequence, which is only read,
// one launch writes the mask in front of the first id (row 0, the root), the mask behind every draft id (row 1 + i for node i), whether
// each id is acceptable (ok), and optionally live and the state behind each.
//
//     THE PATH of node i   the ids of its ancestors from the root down, then its own.  parent[i] is -1 (the root) or an index below i, so a
//                          tree arrives in topological order and the ancestors of node i are a set of indices at or below i: ONE 64-bit word.
//     ROW 1 + i            bit for bit what the step writes for this sequence when its ids are the path: the walk is the step's
//                          (df_step_id / ns_step_id through df_read_id), nothing settles between the ids, the settle and the row write are
//                          df_settle + df_write and ns_finish, unchanged, handed the output row in place of the sequence.
//     ok[i]                the sequence is free on input, or every id of the path was read and accepted: behind the walk the sequence is
//                          constrained, or it became done at the path's LAST id.
//     ABSENT, ORPHAN       a node at or beyond the clamped length is absent; a node whose parent is neither -1 nor an index below it, or
//                          that hangs below such a node, is an orphan.  Both: ok 0, live 0, a broken state row, a mask row of ones.
//
// dr_path climbs from i through the parents, setting bits; every value is checked against -1 <= p < the node it was read at before it is
// followed, so the climb takes at most 64 steps and indexes nothing outside the row, whatever the array holds.  The set bits in ascending
// order are the path in root-to-node order: no indexed local array, no scratch.  k_dfa_draft / k_nest_draft: ONE launch each, a wavefront
// owns one (sequence, row) pair, grid (1 + row_len, sequences over y and z); a row re-walks its prefix -- at most 64 short serial walks
// against a row copy of tens of kilobytes.  The nest kernel keeps k_nest_step's 4 KB overlay in LDS.  No atomics on global memory, no
// wait between workgroups.
//
// The first half is plain C++ over the WAVE POLICY of spl_k_heal.h, as spl_k_dfa.h's: tests/hostsim/draft_sim.cpp runs the same text.
#pragma once
#include "spl_common.h"
#include "spl_k_dfa.h"
#include "spl_k_nest.h"

namespace spl {

// (the values of SPL_DRAFT_* in include/splintr_hip.h)
constexpr uint32_t DR_MAX_NODES = 64, DR_PARENT_PER_SEQ = 1u;

// the draft's shape: parent NULL is a chain; one row [row_len] for all sequences, or [n_seqs, row_len] with per_seq
struct DrIn { const int32_t* parent; uint32_t per_seq; };

// the ancestors of node i of sequence b, itself included, as a bit set over the nodes; 0 for a node that is absent or an orphan
SPL_HD uint64_t dr_path(const DfIn& a, const DrIn& g, uint64_t b, uint32_t i) {
    if (i >= df_row_n(a, b)) return 0ull;
    if (!g.parent) return i >= 63u ? ~0ull : (2ull << i) - 1;
    const int32_t* row = g.parent + (g.per_seq ? b * a.row_len : 0ull);
    uint64_t m = 0;
    for (uint32_t at = i;;) {                                                  // (`at` falls with every turn: at most 64 of them)
        m |= 1ull << at;
        const int32_t p = row[at];
        if (p == -1) return m;
        if (p < -1 || (uint32_t)p >= at) return 0ull;
        at = (uint32_t)p;
    }
}
// the next node of a path in root-to-node order; the path loses it
SPL_HD uint32_t dr_next(uint64_t& path) {
#ifdef SPL_DRAFT_MUTANT_ORDER
    const uint32_t j = 63u - (uint32_t)__builtin_clzll(path);
    path &= ~(1ull << j);
#else
    const uint32_t j = (uint32_t)__builtin_ctzll(path);
    path &= path - 1;
#endif
    return j;
}
// ok behind the id that was just read: the sequence is still constrained, or this id -- the path's last -- ended it
SPL_HD bool dr_ok(const DfState& s, uint64_t rest) {
#ifdef SPL_DRAFT_MUTANT_DONE
    (void)rest;
    return s.con || s.done;
#else
    return s.con || (s.done && !rest);
#endif
}

// THE WALK of a path from the state as it was loaded -> ok.  Serial and the same for every lane, as df_step_seq.
SPL_HD bool dr_dfa_walk(const HlTab& t, const DfTab& d, const DfIn& a, uint64_t b, uint64_t path, DfState& s) {
    bool ok = !s.con && !s.done && !s.broken;                                  // free on input: nothing is read, everything is acceptable
    while (path && s.con) {
        const uint32_t j = dr_next(path);
        uint32_t id;
        const bool is_id = df_read_id(a, b, j, id);
        df_step_id(t, d, a, id, is_id, s);
        ok = dr_ok(s, path);
    }
#ifdef SPL_DRAFT_MUTANT_OK
    if (path && s.broken) ok = true;
#endif
    return ok;
}
SPL_HD bool dr_nest_walk(const HlTab& t, const NsTab& d, const NsStep& p, const DfIn& a, uint64_t b, uint64_t path, DfState& st, NsStack& s) {
    bool ok = !st.con && !st.done && !st.broken;
    while (path && st.con) {
        const uint32_t j = dr_next(path);
        uint32_t id;
        const bool is_id = df_read_id(a, b, j, id);
        ns_step_id(t, d, p, a, id, is_id, st, s);
        ok = dr_ok(st, path);
    }
#ifdef SPL_DRAFT_MUTANT_OK
    if (path && st.broken) ok = true;
#endif
    return ok;
}

// Row r of sequence b (0: the root, 1 + i: node i) of the regex guide.  out is the step's over OUTPUT ROWS -- row b * (1 + row_len) + r
// stands where the step has its sequence -- plus ok(b * row_len + i, 0 | 1), by one lane.
template <class W, class O>
SPL_HD void dr_dfa_row(W& w, const HlTab& t, const DfTab& d, const DfIndex& x, const DfIn& a, const DrIn& g, uint64_t b, uint32_t r, const O& out) {
    DfState s = df_load(d, a.state_in[b]);
    if (r) {
        const uint64_t path = dr_path(a, g, b, r - 1);
        bool ok = false;
        if (path) ok = dr_dfa_walk(t, d, a, b, path, s);
        else s = DfState{0u, false, true, false};                                // absent or orphan: a broken row
        w.each([&](uint32_t l) { if (l == 0) out.ok(b * a.row_len + (r - 1), ok ? 1u : 0u); });
    }
    const bool ends = df_settle(d, x, a, s);
    df_write(w, x, a, b * (1ull + a.row_len) + r, s, ends, out);
}
// the same of the nest guide
template <class W, class O>
SPL_HD void dr_nest_row(W& w, const HlTab& t, const NsTab& d, const NsIndex& x, const NsStep& p, const DfIn& a, const DrIn& g, uint64_t b, uint32_t r,
                        const O& out) {
    NsStack s;
    DfState st = ns_load(d, p, a.state_in + b * NS_STATE_WORDS, s);
    if (r) {
        const uint64_t path = dr_path(a, g, b, r - 1);
        bool ok = false;
        if (path) ok = dr_nest_walk(t, d, p, a, b, path, st, s);
        else st = DfState{0u, false, true, false};
        w.each([&](uint32_t l) { if (l == 0) out.ok(b * a.row_len + (r - 1), ok ? 1u : 0u); });
    }
    ns_finish(w, t, d, x, p, a, b * (1ull + a.row_len) + r, st, s, out);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// the step's outputs over rows, live and the state rows optional, and ok
struct DrDfaOut {
    uint64_t* state_out; uint32_t* mask; uint8_t* live; uint8_t* d_ok; uint32_t n_words;
    __device__ __forceinline__ void state(uint64_t row, uint64_t v) const { if (state_out) state_out[row] = v; }
    __device__ __forceinline__ void alive(uint64_t row, uint32_t v) const { if (live) live[row] = (uint8_t)v; }
    __device__ __forceinline__ void ok(uint64_t at, uint32_t v) const { d_ok[at] = (uint8_t)v; }
    __device__ __forceinline__ void put(uint64_t row, uint32_t k, uint32_t v) const { mask[row * n_words + k] = v; }
    __device__ __forceinline__ void put4(uint64_t row, uint32_t k, const uint32_t* v) const {
        *reinterpret_cast<uint4*>(mask + row * n_words + k) = make_uint4(v[0], v[1], v[2], v[3]);
    }
};
struct DrNestOut {
    uint64_t* state_out; uint32_t* mask; uint8_t* live; uint8_t* d_ok; uint32_t n_words;
    __device__ __forceinline__ void state(uint64_t row, uint32_t i, uint64_t v) const { if (state_out) state_out[row * NS_STATE_WORDS + i] = v; }
    __device__ __forceinline__ void alive(uint64_t row, uint32_t v) const { if (live) live[row] = (uint8_t)v; }
    __device__ __forceinline__ void ok(uint64_t at, uint32_t v) const { d_ok[at] = (uint8_t)v; }
    __device__ __forceinline__ void put(uint64_t row, uint32_t k, uint32_t v) const { mask[row * n_words + k] = v; }
    __device__ __forceinline__ void put4(uint64_t row, uint32_t k, const uint32_t* v) const {
        *reinterpret_cast<uint4*>(mask + row * n_words + k) = make_uint4(v[0], v[1], v[2], v[3]);
    }
};

// grid (1 + row_len, sequences over y and z), one wavefront a workgroup
__global__ __launch_bounds__(DF_WAVE) void k_dfa_draft(DfIn a, DrIn g, HlTab t, DfTab d, DfIndex x, DrDfaOut out) {
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    HlDevWave w{nullptr, nullptr, {}};
    dr_dfa_row(w, t, d, x, a, g, b, blockIdx.x, out);
}

__global__ __launch_bounds__(DF_WAVE) void k_nest_draft(DfIn a, DrIn g, HlTab t, NsTab d, NsIndex x, NsStep p, DrNestOut out) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ov[NS_PIECE];
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    HlDevWave w{nullptr, s_ov, {}};
    dr_nest_row(w, t, d, x, p, a, g, b, blockIdx.x, out);
}
#endif  // __HIPCC__

}  // namespace spl
