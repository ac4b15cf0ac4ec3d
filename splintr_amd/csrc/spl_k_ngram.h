// spl_k_ngram.h -- spl_ngram_draft_device: N-GRAM DRAFTING ("prompt lookup decoding").  A speculative sampler without a
// draft model proposes what followed the last time the sequence ended the way it ends now.  From the id history of every sequence, as
// it lies in HBM, ONE call appends the ids the last step committed and writes up to 8 draft branches of up to 64 ids -- the input of
// spl_dfa_draft_device / spl_nest_draft_device (spl_k_draft.h) as it is.
//
//     H, L            the history hist[:len] ++ new[:new_len] cut at cap, and its length.  An id outside [0, 2^31) is a HOLE: it equals
//                     nothing, not even itself.  Inside the kernel a hole of the history is -1 and a hole of the suffix is -2, so plain
//                     integer equality is the definition's.
//     m(e)            of an end 1 <= e <= L - 1: how many ids in front of e equal the ids in front of L, counted backwards, at most max_n
//                     (and at most e: positions below 0 are staged as holes).  H[e] may lie inside the suffix: periodic text works.
//     THE KEY         of a candidate (m(e) >= min_n, H[e] no hole): m << 24 | e, or m << 24 | (~e & 0xFFFFFF) with NG_EARLIEST; cap is at
//                     most 2^24, a key is never 0 and no two ends share one.  Branch j is the largest key whose FIRST ID H[e] differs
//                     from the first id of every branch before it.
//     TOP-W DISTINCT  the W largest keys with pairwise different first ids, kept sorted (ng_insert).  The top-W distinct of a part of the
//                     ends -- a lane's, a slice's -- hold whatever the top-W distinct of all ends takes from that part: an end that is the
//                     best of its first id anywhere is the best of it in its part, and if W other first ids crowd it out there they do
//                     so everywhere.  So ONE pass over the history suffices for every branch count.
//
// k_ngram<W>: a 256-lane workgroup per (sequence, slice).  The suffix is read once and made wavefront-uniform (scalar registers).  The
// slice streams in tiles of 1 024 ids, 16 bytes a lane and load (int64 rows: two loads, narrowed), the next tile's loads in flight
// while this one is searched; a tile is staged in LDS with 8 ids in front and one behind (two buffers: one workgroup barrier a tile, and
// only an LDS one).  A lane owns four positions: it compares each with the LAST suffix id in registers -- most ends fail there --, and only
// a survivor looks at H[e] (a register, or LDS for the fourth) and counts its run backwards through LDS, then enters the lane's top-W
// distinct: 2 W registers, every index a constant.  Positions at or beyond len are read from `new`, never from hist, and the slice that
// owns them writes them into hist: no workgroup reads what another writes.  After the stream the workgroup takes `branches` rounds: every
// lane offers its best entry whose first id is not chosen yet, max over the wavefront by shuffles, over the four wavefronts through LDS.
// With ONE slice the workgroup's first wavefront then emits (ng_emit): ONE launch.  With S > 1 slices each writes its 8 (key, first id)
// pairs to scratch and k_ngram_emit, one wavefront a sequence, merges the slices' pairs by the same rounds and emits.  ng_emit: lane i is
// node i of the row (branch i / depth, step i % depth), one ballot of the nodes that are missing or holes gives every branch its count.
// No atomics on global memory, no workgroup waits for another, and matrix instructions have no place in an integer compare-and-max.
#pragma once
#include "spl_common.h"

namespace spl {

// (the values of SPL_NGRAM_* in include/splintr_hip.h)
constexpr uint32_t NG_I64 = 1u, NG_EARLIEST = 2u;
constexpr uint32_t NG_MAX_N = 8, NG_MAX_DEPTH = 64, NG_MAX_BRANCHES = 8, NG_MAX_CAP = 1u << 24, NG_MAX_SLICES = 32;
constexpr uint32_t NG_NT = 256, NG_WAVE = 64, NG_TILE = 1024, NG_HALO = 8;
static_assert(NG_TILE == 4 * NG_NT && NG_HALO >= NG_MAX_N - 1 && NG_HALO < NG_WAVE, "a lane owns four positions; the halo holds a full run");

struct NgIn {
    void* hist; const int32_t* len; const void* tail; const int32_t* tail_len;   // tail: `new`, NULL for none
    uint64_t n_seqs;
    uint32_t cap, tail_row, flags, min_n, max_n, depth, branches, pad_id;
    uint32_t slices, slice_len;     // slice_len: a multiple of NG_TILE; slices * slice_len >= cap
    uint32_t v4;                    // hist rows may be read 16 bytes at a time
};
struct NgOut { void* ids; int32_t* count; int32_t* match; int32_t* from; int32_t* parent; int32_t* len; uint8_t* full; };

// the slice length for a wanted number of slices, and the slices that come of it
SPL_HD uint32_t ng_slice_len(uint32_t cap, uint32_t want) {
    const uint32_t per = (cap + want - 1) / want;
    return per <= NG_TILE ? NG_TILE : (per + NG_TILE - 1) / NG_TILE * NG_TILE;
}
SPL_HD uint32_t ng_slices(uint32_t cap, uint32_t slice_len) { return cap <= slice_len ? 1u : (cap + slice_len - 1) / slice_len; }
SPL_HD int32_t ng_narrow(int64_t v) { return (uint64_t)v < (1ull << 31) ? (int32_t)v : -1; }
SPL_HD uint32_t ng_key(uint32_t m, uint32_t e, uint32_t flags) { return m << 24 | ((flags & NG_EARLIEST) ? ~e & 0xFFFFFFu : e); }
SPL_HD uint32_t ng_key_end(uint32_t key, uint32_t flags) { return ((flags & NG_EARLIEST) ? ~key : key) & 0xFFFFFFu; }

#if defined(__HIPCC__)
// a sequence's clamped lengths
struct NgSeq { uint32_t len, L; bool full; };
__device__ __forceinline__ NgSeq ng_seq(const NgIn& a, uint64_t b) {
    const int32_t l = a.len[b];
    const uint32_t len = l < 0 ? 0u : min((uint32_t)l, a.cap);
    uint64_t nl = 0;
    if (a.tail) { const int32_t t = a.tail_len[b]; nl = t < 0 ? 0u : min((uint32_t)t, a.tail_row); }
    return NgSeq{len, len + nl > a.cap ? a.cap : (uint32_t)(len + nl), len + nl > a.cap};
}
// H[pos] as it was given, pos < L: hist below len, `new` from there on
__device__ __forceinline__ int64_t ng_raw(const NgIn& a, uint64_t b, const NgSeq& q, uint32_t pos) {
    const bool h = pos < q.len;
    const uint64_t at = h ? b * a.cap + pos : b * a.tail_row + (pos - q.len);
    const void* base = h ? (const void*)a.hist : a.tail;
    return (a.flags & NG_I64) ? static_cast<const int64_t*>(base)[at] : (int64_t) static_cast<const int32_t*>(base)[at];
}
// H[pos] narrowed, -1 for a hole and for every position outside 0 .. L - 1
__device__ __forceinline__ int32_t ng_at(const NgIn& a, uint64_t b, const NgSeq& q, int64_t pos) {
    return pos < 0 || pos >= (int64_t)q.L ? -1 : ng_narrow(ng_raw(a, b, q, (uint32_t)pos));
}
// A lane's four positions p .. p + 3 (p a multiple of 4).  What comes from `new` goes into hist on the way: every position of the slice
// is loaded once.
__device__ __forceinline__ int4 ng_load4(const NgIn& a, uint64_t b, const NgSeq& q, uint32_t p) {
    int32_t v[4];
    if (a.v4 && p + 4 <= q.len) {
        if (a.flags & NG_I64) {
            const longlong2* s = reinterpret_cast<const longlong2*>(static_cast<const int64_t*>(a.hist) + b * a.cap + p);
            const longlong2 x = s[0], y = s[1];
            v[0] = ng_narrow(x.x); v[1] = ng_narrow(x.y); v[2] = ng_narrow(y.x); v[3] = ng_narrow(y.y);
        } else {
            const int4 x = *reinterpret_cast<const int4*>(static_cast<const int32_t*>(a.hist) + b * a.cap + p);
            v[0] = max(x.x, -1); v[1] = max(x.y, -1); v[2] = max(x.z, -1); v[3] = max(x.w, -1);
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t pos = p + i;
            v[i] = -1;
            if (pos < q.L) {
                const int64_t raw = ng_raw(a, b, q, pos);
                if (pos >= q.len) {
                    if (a.flags & NG_I64) static_cast<int64_t*>(a.hist)[b * a.cap + pos] = raw;
                    else static_cast<int32_t*>(a.hist)[b * a.cap + pos] = (int32_t)raw;
                }
                v[i] = ng_narrow(raw);
            }
        }
    }
    return make_int4(v[0], v[1], v[2], v[3]);
}
// the tile's halo: lanes 0 .. 7 the eight positions in front of t0, lane 8 the one behind the tile
__device__ __forceinline__ int32_t ng_halo(const NgIn& a, uint64_t b, const NgSeq& q, uint32_t t0, uint32_t lane) {
    if (lane > NG_HALO) return -1;
    return ng_at(a, b, q, lane < NG_HALO ? (int64_t)t0 - NG_HALO + lane : (int64_t)t0 + NG_TILE);
}

// (key, first id) enters a top-W distinct list: sorted by key, largest first, no first id twice; key 0 is an empty place
template <int W>
__device__ __forceinline__ void ng_insert(uint32_t (&lk)[W], int32_t (&lf)[W], uint32_t key, int32_t f) {
    if (key <= lk[W - 1]) return;                       // W other first ids are better, or this one's better end is among them
    uint32_t ck = key; int32_t cf = f; bool placed = false;
#pragma unroll
    for (int i = 0; i < W; i++) {
        if (!placed && lk[i] > ck) {                    // an entry that stays in front
            if (lf[i] == f) ck = 0;                     // ... and has this first id: a better end of it is here already
        } else if (ck) {                                // the new one takes this place; what was here moves down, unless it is f's old entry
            const uint32_t tk = lk[i]; const int32_t tf = lf[i];
            lk[i] = ck; lf[i] = cf; ck = tk; cf = tf; placed = true;
            if (ck && cf == f) ck = 0;
        }
    }
}
__device__ __forceinline__ unsigned long long ng_max64(unsigned long long x, unsigned long long y) { return y > x ? y : x; }
__device__ __forceinline__ unsigned long long ng_wave_max(unsigned long long x) {
#pragma unroll
    for (int d = 1; d < (int)NG_WAVE; d <<= 1) x = ng_max64(x, __shfl_xor(x, d));
    return x;
}
__device__ __forceinline__ bool ng_chosen(const uint32_t (&wk)[NG_MAX_BRANCHES], const int32_t (&wf)[NG_MAX_BRANCHES], int j, int32_t f) {
    bool ex = false;
#pragma unroll
    for (int c = 0; c < (int)NG_MAX_BRANCHES; c++) ex |= c < j && wk[c] && wf[c] == f;
    return ex;
}

// The rows of sequence b from the winners' keys, by ONE wavefront: lane i is node i (branch i / depth, step i % depth).
__device__ __forceinline__ void ng_emit(const NgIn& a, const NgOut& o, uint64_t b, const NgSeq& q, const uint32_t (&wk)[NG_MAX_BRANCHES], uint32_t lane) {
    if (a.depth) {
        const uint32_t nodes = a.branches * a.depth, j = lane / a.depth, k = lane - j * a.depth;
        const bool node = lane < nodes;
        uint32_t key = 0;
#pragma unroll
        for (uint32_t c = 0; c < NG_MAX_BRANCHES; c++) key = node && c == j ? wk[c] : key;
        const uint32_t e = ng_key_end(key, a.flags);
        int64_t raw = 0;
        bool good = false;
        if (key && e + k < q.L) { raw = ng_raw(a, b, q, e + k); good = ng_narrow(raw) >= 0; }
        const unsigned long long bad = __ballot(!good);
        if (node) {
            const unsigned long long r = bad >> (j * a.depth);
            const uint32_t cnt = r ? min((uint32_t)__builtin_ctzll(r), a.depth) : a.depth;
            const bool have = k < cnt;
            const uint64_t at = b * nodes + lane;
            if (a.flags & NG_I64) static_cast<int64_t*>(o.ids)[at] = have ? raw : (int64_t)a.pad_id;
            else static_cast<int32_t*>(o.ids)[at] = have ? (int32_t)raw : (int32_t)a.pad_id;
            if (o.parent) o.parent[at] = have ? (k ? (int32_t)lane - 1 : -1) : -2;
            if (!k) {
                o.count[b * a.branches + j] = (int32_t)cnt;
                o.match[b * a.branches + j] = (int32_t)(key >> 24);
                o.from[b * a.branches + j] = key ? (int32_t)e : -1;
            }
        }
    }
    if (!lane) {
        o.len[b] = (int32_t)q.L;
        if (o.full) o.full[b] = q.full ? 1 : 0;
    }
}

// grid (slices, sequences over y and z).  W: the places of a top-W distinct list, at least `branches`.
template <int W>
__global__ __launch_bounds__(NG_NT) void k_ngram(NgIn a, NgOut o, uint2* scr) {
    __shared__ __attribute__((aligned(16))) int32_t s_h[2][NG_HALO + NG_TILE + NG_HALO];
    __shared__ unsigned long long s_red[NG_MAX_BRANCHES][NG_NT / NG_WAVE];
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    const NgSeq q = ng_seq(a, b);
    const uint32_t lane = threadIdx.x, s0 = blockIdx.x * a.slice_len;
    if (a.slices > 1 && s0 >= q.L) return;                                      // an empty slice leaves at once: k_ngram_emit does not read its pairs
    const uint32_t t_end = min(min(s0 + a.slice_len, a.cap), q.L);
    uint32_t t0 = a.depth ? s0 : max(s0, q.len / NG_TILE * NG_TILE);           // depth 0 appends only: the tiles that hold the tail

    int32_t suf[NG_MAX_N];                                                      // suf[k] = H[L - 1 - k], uniform; -2 for a hole and beyond max_n
#pragma unroll
    for (uint32_t k = 0; k < NG_MAX_N; k++) {
        const int32_t v = k < a.max_n && a.depth ? ng_at(a, b, q, (int64_t)q.L - 1 - k) : -1;
        suf[k] = __builtin_amdgcn_readfirstlane(v < 0 ? -2 : v);
    }
    uint32_t lk[W]; int32_t lf[W];
#pragma unroll
    for (int i = 0; i < W; i++) { lk[i] = 0; lf[i] = 0; }

    int4 cur = make_int4(-1, -1, -1, -1);
    int32_t hal = -1;
    if (t0 < t_end) { cur = ng_load4(a, b, q, t0 + 4 * lane); hal = ng_halo(a, b, q, t0, lane); }
    for (uint32_t buf = 0; t0 < t_end; t0 += NG_TILE, buf ^= 1u) {
        int32_t* h = s_h[buf];
        const int32_t* at = h + NG_HALO + 4 * lane;                            // the lane's first position in LDS
        *reinterpret_cast<int4*>(h + NG_HALO + 4 * lane) = cur;
        if (lane < NG_HALO) h[lane] = hal;
        else if (lane == NG_HALO) h[NG_HALO + NG_TILE] = hal;
        const int32_t v[5] = {cur.x, cur.y, cur.z, cur.w, 0};
        if (t0 + NG_TILE < t_end) { cur = ng_load4(a, b, q, t0 + NG_TILE + 4 * lane); hal = ng_halo(a, b, q, t0 + NG_TILE, lane); }
        lds_barrier();                                                          // (the other buffer is still being read: two tiles apart never)
        if (!a.depth) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (v[i] != suf[0]) continue;
            const uint32_t e = t0 + 4 * lane + i + 1;
            const int32_t f = i < 3 ? v[i + 1] : at[4];
            if (e >= q.L || f < 0) continue;
            uint32_t m = 1;
            bool run = true;
#pragma unroll
            for (int k = 1; k < (int)NG_MAX_N; k++) { run = run && at[i - k] == suf[k]; m += run ? 1u : 0u; }
            if (m >= a.min_n) ng_insert<W>(lk, lf, ng_key(m, e, a.flags), f);
        }
    }

    // `branches` rounds: the best entry whose first id is not chosen yet, over the workgroup
    uint32_t wk[NG_MAX_BRANCHES] = {}; int32_t wf[NG_MAX_BRANCHES] = {};
#pragma unroll
    for (int j = 0; j < (int)NG_MAX_BRANCHES; j++) {
        unsigned long long best = 0;
        if (j < W && j < (int)a.branches && a.depth) {
#pragma unroll
            for (int i = W - 1; i >= 0; i--)
                if (lk[i] && !ng_chosen(wk, wf, j, lf[i])) best = (unsigned long long)lk[i] << 32 | (uint32_t)lf[i];
            best = ng_wave_max(best);
            if (!(lane & (NG_WAVE - 1))) s_red[j][lane / NG_WAVE] = best;
            lds_barrier();
            best = ng_max64(ng_max64(s_red[j][0], s_red[j][1]), ng_max64(s_red[j][2], s_red[j][3]));
        }
        wk[j] = (uint32_t)(best >> 32); wf[j] = (int32_t)(uint32_t)best;
    }
    if (a.slices > 1) {
        if (a.depth && lane < NG_MAX_BRANCHES) {
            uint2 p = make_uint2(0u, 0u);
#pragma unroll
            for (uint32_t c = 0; c < NG_MAX_BRANCHES; c++) if (lane == c) p = make_uint2(wk[c], (uint32_t)wf[c]);
            scr[(b * a.slices + blockIdx.x) * NG_MAX_BRANCHES + lane] = p;
        }
        return;
    }
    __syncthreads();                                                            // every wavefront has read len[b]: d_len may be the same array
    if (lane < NG_WAVE) ng_emit(a, o, b, q, wk, lane);
}

// S > 1: the slices' pairs merged and the rows written, one wavefront a sequence; grid (1, sequences over y and z)
__global__ __launch_bounds__(NG_WAVE) void k_ngram_emit(NgIn a, NgOut o, const uint2* scr) {
    const uint64_t b = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= a.n_seqs) return;
    const NgSeq q = ng_seq(a, b);
    const uint32_t lane = threadIdx.x;
    const uint32_t n = a.depth ? min(a.slices, (q.L + a.slice_len - 1) / a.slice_len) * NG_MAX_BRANCHES : 0u;   // the slices that did not leave at once
    const uint2* row = scr + b * a.slices * NG_MAX_BRANCHES;
    uint32_t wk[NG_MAX_BRANCHES] = {}; int32_t wf[NG_MAX_BRANCHES] = {};
#pragma unroll
    for (int j = 0; j < (int)NG_MAX_BRANCHES; j++) {
        unsigned long long best = 0;
        if (j < (int)a.branches) {
            for (uint32_t i = lane; i < n; i += NG_WAVE) {
                const uint2 p = row[i];
                if (p.x && !ng_chosen(wk, wf, j, (int32_t)p.y)) best = ng_max64(best, (unsigned long long)p.x << 32 | p.y);
            }
            best = ng_wave_max(best);
        }
        wk[j] = (uint32_t)(best >> 32); wf[j] = (int32_t)(uint32_t)best;
    }
    ng_emit(a, o, b, q, wk, lane);
}
#endif  // __HIPCC__

}  // namespace spl
