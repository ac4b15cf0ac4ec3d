// spl_k_dfa_jump.h -- spl_dfa_jump_index_device / spl_dfa_jump_device: JUMP-FORWARD for the regex guide.  Where the
// automaton of spl_k_dfa.h leaves no choice, the forced bytes are emitted as ids and cost no forward pass of the model.  With walk, DEAD,
// ORDINARY, b(t) and the state word of spl_k_dfa.h:
//
//     FORCED BYTE     force(q) = x iff accept[q] == 0 and exactly one byte x has trans[q][x] < S (an accepting state is never forced: an
//                     END id may follow it).
//     RUN             run(q): the bytes x1 x2 ... with q1 = q, q(i+1) = trans[qi][xi], while force(qi) is defined; at most JM_MAX_BYTES
//                     (a table need not be trimmed: the cap also ends cycles).
//     UTF-8 TRIM      the capped run is cut back to a character boundary of its own bytes: where it ends in a lead byte (>= 0xC0) with
//                     fewer continuation bytes behind it than it announces, it is cut in front of that lead byte.  Leading continuation
//                     bytes stay.
//     THE JUMP INDEX  uint32 ids[S][64], uint8 n_ids[S], uint8 run_len[S], uint8 run[S][64]: ids[q][0 .. n_ids[q]) is run(q) encoded as a
//                     text of its own; every byte of the region is written, zeros where nothing is meant.
//     JUMP STEP       spl_k_dfa.h's step, and between the walk of the sampler's ids and the settle: for a sequence still constrained in
//                     state q, n = min(n_ids[q], 64, row_len_out); the leading ids of ids[q][0 .. n) are emitted for as long as each is
//                     ordinary and walks -- the first that does not ends the emission, not the sequence; q moves along what was emitted.
//
// k_dfa_force: a wavefront per state, the 512-byte trans row eight bytes a lane, four ballots, one word a state -- (next state << 8 | byte),
// JM_NONE where nothing is forced -- into the first S words of the jump index (the scatter overwrites them).  k_dfa_runs: a launch of its
// own (it needs every force word), a wavefront per state; the chain of at most 64 dependent loads is the same for every lane, lane i keeps
// byte i, one 64-byte store a state.  k_dfa_jump_len / _write / _one: the runs compacted into a bytes CSR of S documents by the
// count-scan-write driver (spl_k_seqscan.h), which the handle's device encode then takes.  k_dfa_jump_scatter: the ids CSR into ids[S][64]
// and n_ids[S].  k_dfa_jump: the step, ONE launch, a wavefront per sequence; it trusts nothing in the jump index -- it walks what it emits
// and its indices are bounded by the state and by 64.  No LDS (but the driver's), no scratch, no atomics on global memory, no polling.
//
// The first half is plain C++ over the wave policy of spl_k_heal.h; tests/hostsim/jump_sim.cpp runs the same text with HlHostWave.
#pragma once
#include "spl_k_dfa.h"

namespace spl {

// (the values of SPL_DFA_JUMP_* in include/splintr_hip.h)
constexpr uint32_t JM_MAX_BYTES = 64, JM_MAX_IDS = 64;
constexpr uint32_t JM_NONE = 0xFFFFFFFFu;                                          // a force word: nothing is forced
constexpr uint32_t JM_NT = 256;
constexpr uint32_t JM_R_BYTE = 0;                                                  // a lane's register in the runs: its byte of the run
static_assert(JM_MAX_BYTES == DF_WAVE, "a lane of the hardware's wavefront keeps one byte of a run");

// the jump index as it lies in memory, S = n_states
SPL_HD size_t jm_index_bytes(uint32_t S) { return (size_t)S * (JM_MAX_IDS * 4 + 1 + 1 + JM_MAX_BYTES); }
struct JmIndex { uint32_t* ids; uint8_t* n_ids; uint8_t* run_len; uint8_t* run; };
SPL_HD JmIndex jm_index(void* base, uint32_t S) {
    uint8_t* p = static_cast<uint8_t*>(base);
    return JmIndex{static_cast<uint32_t*>(base), p + (size_t)S * JM_MAX_IDS * 4, p + (size_t)S * (JM_MAX_IDS * 4 + 1), p + (size_t)S * (JM_MAX_IDS * 4 + 2)};
}
// the step's part of a call: the index's ids and counts, the width of a row of emitted ids
struct JmStep { const uint32_t* ids; const uint8_t* n_ids; uint32_t row_len_out; };

// ------------------------------------------------------------------------------------------ force
// One wavefront, state q (< n_states): the live entries of its trans row, four entries a lane and a ballot per entry; put(q, word) by one lane.
template <class W, class F> SPL_HD void jm_force_wave(W& w, const DfTab& d, uint32_t q, F put) {
    const uint32_t L = w.lanes();
    const uint16_t* row = d.trans + (size_t)q * 256;
    uint32_t live = 0, at = 0;
    for (uint32_t base = 0; base < 256; base += 4 * L) {
        w.each([&](uint32_t l) {                                                  // (the row is 2-byte aligned: the compiler picks the loads)
            uint16_t v[4] = {0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu};
            if (base + 4 * l < 256) __builtin_memcpy(v, row + base + 4 * l, 8);
            w.reg(l, 0) = (uint32_t)v[0] | (uint32_t)v[1] << 16;
            w.reg(l, 1) = (uint32_t)v[2] | (uint32_t)v[3] << 16;
        });
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t m = w.ballot([&](uint32_t l) {
                const uint32_t v = (w.reg(l, j >> 1) >> (16 * (j & 1u))) & 0xFFFFu;
                return base + 4 * l < 256 && v < d.n_states;
            });
            if (m) { live += (uint32_t)__builtin_popcountll(m); at = base + 4 * (uint32_t)__builtin_ctzll(m) + j; }
        }
    }
#ifdef SPL_DFA_JUMP_MUTANT_ACCEPT
    const bool forced = live == 1;
#else
    const bool forced = live == 1 && d.accept[q] == 0;
#endif
    const uint32_t word = forced ? (df_next(d, q, at) << 8 | at) : JM_NONE;       // (one live entry: `at` is it)
    w.each([&](uint32_t l) { if (l == 0) put(q, word); });
}

// ------------------------------------------------------------------------------------------ runs
// how many continuation bytes a lead byte announces
SPL_HD uint32_t jm_lead_need(uint32_t x) { return x >= 0xF0u ? 3u : (x >= 0xE0u ? 2u : 1u); }
// One wavefront, state q: the chain of force words from q, capped and trimmed; lane i keeps byte i (fewer lanes take the 64 bytes in turns,
// the chain once a turn).  put(q, i, byte) for every i < 64 -- zeros behind the run -- and put_len(q, n) by one lane.
template <class W, class F, class G> SPL_HD void jm_run_wave(W& w, const uint32_t* force, uint32_t n_states, uint32_t q, F put, G put_len) {
    const uint32_t L = w.lanes();
    uint32_t len = 0;
    for (uint32_t i0 = 0; i0 < JM_MAX_BYTES; i0 += L) {
        w.each([&](uint32_t l) { w.reg(l, JM_R_BYTE) = 0u; });
        uint32_t cur = q, n = 0, lead = JM_NONE, need = 0;
        while (n < JM_MAX_BYTES && cur < n_states) {
            const uint32_t f = force[cur];
            if (f == JM_NONE) break;
            const uint32_t x = f & 0xFFu, at = n;
            w.each([&](uint32_t l) { if (i0 + l == at) w.reg(l, JM_R_BYTE) = x; });
            if (x >= 0xC0u) { lead = n; need = jm_lead_need(x); }
            else if (x < 0x80u) lead = JM_NONE;
            cur = f >> 8; n++;
        }
        if (lead != JM_NONE && n - 1 - lead < need) n = lead;                     // the trim: an unfinished character at the end goes
        len = n;
        w.each([&](uint32_t l) { if (i0 + l < JM_MAX_BYTES) put(q, i0 + l, i0 + l < len ? w.reg(l, JM_R_BYTE) : 0u); });
    }
    w.each([&](uint32_t l) { if (l == 0) put_len(q, len); });
}

// ------------------------------------------------------------------------------------------ scatter
// One wavefront, state q: its stretch of the ids CSR into ids[q][64], zeros behind it; put(q, i, id) for every i < 64, put_n(q, n) by one lane.
template <class W, class F, class G> SPL_HD void jm_scatter_wave(W& w, const uint32_t* csr, const uint64_t* off, uint64_t cap, uint32_t q, F put, G put_n) {
    const uint32_t L = w.lanes();
    const uint64_t o0 = off[q], o1 = off[q + 1];
    uint64_t n64 = o1 > o0 ? o1 - o0 : 0;
    if (o0 >= cap) n64 = 0; else if (n64 > cap - o0) n64 = cap - o0;             // (never behind the CSR, whatever the offsets hold)
    const uint32_t n = n64 > JM_MAX_IDS ? JM_MAX_IDS : (uint32_t)n64;
    w.each([&](uint32_t l) { for (uint32_t i = l; i < JM_MAX_IDS; i += L) put(q, i, i < n ? csr[o0 + i] : 0u); });
    w.each([&](uint32_t l) { if (l == 0) put_n(q, n); });
}

// ------------------------------------------------------------------------------------------ the step
// THE JUMP of a sequence that is constrained in s.q: the leading ids of the state's row that are ordinary and walk, q moved along them.
// Returns how many; the ids are row[0 .. m) (the caller stores them).
SPL_HD uint32_t jm_jump(const HlTab& t, const DfTab& d, const JmStep& j, DfState& s, const uint32_t*& row) {
    row = j.ids + (size_t)s.q * JM_MAX_IDS;                                       // (s.q < n_states: df_load and the walk see to it)
    uint32_t n = j.n_ids[s.q];
    if (n > JM_MAX_IDS) n = JM_MAX_IDS;
    if (n > j.row_len_out) n = j.row_len_out;
    uint32_t m = 0;
    for (; m < n; m++) {
        uint32_t tl = 0;
        const uint8_t* tb = df_bytes(t, row[m], tl);
        const uint32_t q1 = tb ? df_walk_from(d, s.q, tb, 0u, tl) : DF_DEAD;
#ifdef SPL_DFA_JUMP_MUTANT_NOWALK
        if (q1 != DF_DEAD) s.q = q1;
#else
        if (q1 == DF_DEAD) break;                                                 // the emission stops; the sequence is not broken
        s.q = q1;
#endif
    }
    return m;
}
// everything of sequence b: spl_k_dfa.h's walk, the jump, the settle and the row write.  out.forced(b, i, id) and out.forced_n(b, m) store.
template <class W, class O> SPL_HD void jm_seq(W& w, const HlTab& t, const DfTab& d, const DfIndex& x, const DfIn& a, const JmStep& j, uint64_t b, const O& out) {
    const uint32_t L = w.lanes();
    DfState s = df_load(d, a.state_in[b]);
    df_step_seq(t, d, a, b, s);
    uint32_t m = 0;
    const uint32_t* row = nullptr;
    if (s.con) m = jm_jump(t, d, j, s, row);
    w.each([&](uint32_t l) {
        for (uint32_t i = l; i < m; i += L) out.forced(b, i, row[i]);
        if (l == 0) out.forced_n(b, m);
    });
    const bool ends = df_settle(d, x, a, s);
    df_write(w, x, a, b, s, ends, out);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernels
// a wavefront per state, four a workgroup; force: the first n_states words of the jump index
__global__ __launch_bounds__(JM_NT) void k_dfa_force(DfTab d, uint32_t* __restrict__ force) {
    const uint32_t q = blockIdx.x * (JM_NT / DF_WAVE) + threadIdx.x / DF_WAVE;
    if (q >= d.n_states) return;                                               // (a whole wavefront: nothing waits for it)
    HlDevWave w{nullptr, nullptr, {}};
    jm_force_wave(w, d, q, [&](uint32_t s, uint32_t v) { force[s] = v; });
}

__global__ __launch_bounds__(JM_NT) void k_dfa_runs(const uint32_t* __restrict__ force, uint32_t n_states, uint8_t* __restrict__ run, uint8_t* __restrict__ run_len) {
    const uint32_t q = blockIdx.x * (JM_NT / DF_WAVE) + threadIdx.x / DF_WAVE;
    if (q >= n_states) return;
    HlDevWave w{nullptr, nullptr, {}};
    jm_run_wave(w, force, n_states, q, [&](uint32_t s, uint32_t i, uint32_t x) { run[(size_t)s * JM_MAX_BYTES + i] = (uint8_t)x; },
                [&](uint32_t s, uint32_t n) { run_len[s] = (uint8_t)n; });
}

// the runs as a bytes CSR of n_states documents: the op of the count-scan-write driver (spl_k_seqscan.h)
struct JmWave {};
struct JmOp {
    using Wave = JmWave;
    using Carry = SeqNoCarry;
    const uint8_t* run; const uint8_t* run_len; uint8_t* out; uint64_t cap;
    __device__ __forceinline__ uint32_t len(uint64_t q) const { const uint32_t n = run_len[q]; return n > JM_MAX_BYTES ? JM_MAX_BYTES : n; }
    __device__ __forceinline__ uint64_t count(uint64_t q, JmWave&, SeqNoCarry&) const { return len(q); }
    __device__ __forceinline__ void write(uint64_t q, JmWave&, const SeqNoCarry&, uint64_t o0) const {
        const uint32_t lane = threadIdx.x & 63u;
        if (lane < len(q)) seq_put(out, cap, o0 + lane, run[q * JM_MAX_BYTES + lane]);
    }
};
__global__ __launch_bounds__(SEQ_NT) void k_dfa_jump_len(const uint8_t* __restrict__ run_len, uint64_t n_states, uint64_t n_blk, uint64_t* __restrict__ cnt,
                                                         uint64_t* __restrict__ blk) {
    __shared__ JmWave s_wave[SEQ_NT / 64];
    __shared__ uint64_t s_sum[SEQ_NT / 64];
    seq_len_body(JmOp{nullptr, run_len, nullptr, 0}, SeqNoKeep{}, n_states, n_blk, s_wave, s_sum, cnt, blk);
}
__global__ __launch_bounds__(SEQ_NT) void k_dfa_jump_write(const uint8_t* __restrict__ run, const uint8_t* __restrict__ run_len, uint64_t n_states, uint64_t n_blk,
                                                           const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ blk, uint8_t* __restrict__ out,
                                                           uint64_t cap, uint64_t* __restrict__ out_off) {
    __shared__ JmWave s_wave[SEQ_NT / 64];
    seq_write_body(JmOp{run, run_len, out, cap}, SeqNoKeep{}, n_states, n_blk, s_wave, cnt, blk, out_off);
}
__global__ __launch_bounds__(SEQ_ONE_NT) void k_dfa_jump_one(const uint8_t* __restrict__ run, const uint8_t* __restrict__ run_len, uint32_t n_states,
                                                             uint8_t* __restrict__ out, uint64_t cap, uint64_t* __restrict__ out_off) {
    __shared__ JmWave s_wave[SEQ_ONE_NT / 64];
    __shared__ uint64_t s_cnt[SEQ_ONE_MAX + 1];
    seq_one_body(JmOp{run, run_len, out, cap}, SeqNoKeep{}, n_states, s_wave, s_cnt, out_off);
}

// a wavefront per state, four a workgroup
__global__ __launch_bounds__(JM_NT) void k_dfa_jump_scatter(const uint32_t* __restrict__ csr, const uint64_t* __restrict__ off, uint64_t cap, uint32_t n_states,
                                                            uint32_t* __restrict__ ids, uint8_t* __restrict__ n_ids) {
    const uint32_t q = blockIdx.x * (JM_NT / DF_WAVE) + threadIdx.x / DF_WAVE;
    if (q >= n_states) return;
    HlDevWave w{nullptr, nullptr, {}};
    jm_scatter_wave(w, csr, off, cap, q, [&](uint32_t s, uint32_t i, uint32_t v) { ids[(size_t)s * JM_MAX_IDS + i] = v; },
                    [&](uint32_t s, uint32_t n) { n_ids[s] = (uint8_t)n; });
}

struct JmOut : DfOut {
    int32_t* forced_ids; int32_t* forced_len; uint32_t row_len_out;
    __device__ __forceinline__ void forced(uint64_t b, uint32_t i, uint32_t id) const { forced_ids[b * row_len_out + i] = (int32_t)id; }
    __device__ __forceinline__ void forced_n(uint64_t b, uint32_t m) const { forced_len[b] = (int32_t)m; }
};

// grid (1, sequences over y and z), one wavefront a workgroup
__global__ __launch_bounds__(DF_WAVE) void k_dfa_jump(DfIn a, HlTab t, DfTab d, DfIndex x, JmStep j, JmOut out) {
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    HlDevWave w{nullptr, nullptr, {}};
    jm_seq(w, t, d, x, a, j, b, out);
}
#endif  // __HIPCC__

}  // namespace spl
