// spl_k_seqpack.h -- WHOLE sequences binned into rows of L, none cut in two: from n sequences (rows + lengths as the
// collators leave them, or a CSR) to packed rows with labels, byte companions, mask, position ids, sequence ids and the boundaries a
// variable-length attention kernel takes.  Two launches:
//
//   k_seqpack_next_fit / k_seqpack_bfd   the PLAN, ONE workgroup of SQP_NT lanes: every sequence's (row, column), the row-major order
//                    array and the rows' starts in it, row_fill, cu_seqlens, n[4].  It leaves them in the work buffer.
//   k_seqpack_gather the rows: the gather of spl_k_chat.h's shape -- a lane owns COL_VEC consecutive flat elements, the grid is
//                    cpair_grid's, no loop over spans.  A group finds the sequence that covers its first column by a binary search over
//                    the columns of its row's sequences (ocol[row_start[r] .. row_start[r + 1])) and steps forward from there.
//
// No workgroup waits for another, no atomics on device memory (the counting sort counts with LDS atomics).  Every output element is
// written once.
//
// next_fit.  clen[i] = min(len_i, L) is scanned into P[] (P[i] = ids in front of sequence i) and the non-empty flags into K[].
// next[i] = the first j > i with P[j + 1] - P[i] > L: the first sequence that no longer fits a row that sequence i opens -- a binary
// search per lane.  EMPTY sequences need no special case: P[j + 1] - P[i] > L >= P[j] - P[i] makes sequence j non-empty, so next[] of a
// non-empty sequence is a non-empty sequence or n; the walk starts at the first non-empty sequence (K == 0) and never stands on an
// empty one.  The rows' first sequences are the orbit of that start under next[]; it is marked by pointer doubling: in round k the marked
// sequences mark A[i] (A = next^(2^k)) and A becomes A o A; ceil(log2(non-empty)) rounds, one workgroup barrier each.  The three arrays
// (A, its successor, the marks) are in LDS for n <= the "seqpack_lds_max" option (SQP_LDS_MAX = 4096 by default: 48 KB) and in the work
// buffer beyond -- the SAME loop over the same pointers, the one workgroup striding over n.  A scan of the marks is the row, P the column.
//   NOT BUILT: a multi-workgroup plan for large n (exits per block, a walk over the blocks, marks per block).  The one workgroup is
//   correct for every n, but its rounds cost n / SQP_NT iterations each; the header of the C ABI says so.
//
// best_fit_decreasing.  A stable counting sort by clen descending: LDS histogram over L + 1 buckets (all lanes), a descending scan of the
// buckets (all lanes), the stable scatter by wavefront 0 (64 sequences at a time in index order; lanes with equal keys rank themselves by
// a ballot).  Then ONE LANE walks the sorted order -- a placement depends on every placement before it: head[r] = the row that reached
// the residual r most recently, link[row] = the one before it (a LIFO per residual), a two-level bitmap of the residuals that have a row.
// head[] is L + 1 words of LDS, which bounds L for this strategy: SQP_BFD_MAX_L = 32768.  link[] and the rows' counts are in LDS too when
// L + 1 + 2 n <= SQP_POOL words (144 KB) and n <= "seqpack_lds_max", otherwise in the work buffer.  Runs of equal lengths are placed one by
// one.  The walk was measured at 0.9 us per sequence (1.2 us at L = 16 384; profiles/seqpack.txt); next_fit's plan at 0.01 us.  Beyond
// about 4 000 sequences the C ABI's header advises next_fit.
//
// The decisions are the plain C++ of the first half of this file; tests/hostsim/seqpack_sim.cpp includes it in a g++ build, evaluates
// the gather for every output element and restates the plan kernels' phases lane by lane over the same functions.
#pragma once
#include "spl_k_pair.h"
#include "spl_k_seqscan.h"

namespace spl {

// (the values of SPL_SEQPACK_* in include/splintr_hip.h; COL_I64, COL_PAD_LEFT and COL_KEEP_TAIL are shared with the collate family)
constexpr uint32_t SQP_NEXT_FIT = 0, SQP_BFD = 1;
constexpr uint32_t SQP_MASK_FIRST = 32u;
constexpr uint32_t SQP_NT = 1024;                    // lanes of the plan's one workgroup
constexpr uint32_t SQP_LDS_MAX = 4096;               // most sequences whose plan arrays are in LDS (fewer: a test's option)
constexpr uint32_t SQP_POOL = 36864;                 // words of the BFD plan's LDS pool: head[L + 1], then link[n] and count[n] if they fit
constexpr uint32_t SQP_BFD_MAX_L = 32768;            // the largest row_len best_fit_decreasing takes
constexpr uint32_t SQP_BM0 = SQP_BFD_MAX_L / 32 + 1, SQP_BM1 = SQP_BM0 / 32 + 1;
constexpr uint32_t SQP_NONE = 0xFFFFFFFFu;
static_assert(SQP_BFD_MAX_L + 1 <= SQP_POOL, "head[] fits the pool");

struct SqpIn {
    const void* ids; const int32_t* len; const uint64_t* off;          // rows form: len; CSR form: off (exactly one of the two)
    const void* labels; const uint8_t* b0; const uint8_t* b1; const uint8_t* b2; const uint8_t* b3;
    uint32_t n, L_in;                                                  // (n below 2^31: the C ABI refuses more)
};
struct SqpGeo { uint32_t flags, strategy, L, pad_id, ignore_id, fills, R, lds_max; };       // fills: byte k pads byte array k; R = max_rows
struct SqpPlanOut { int32_t* place; int32_t* row_fill; int32_t* cu; int64_t* n; uint32_t* status; };
struct SqpRowsOut { void* rows; void* labels; uint8_t* b0; uint8_t* b1; uint8_t* b2; uint8_t* b3; uint8_t* mask; int32_t* pos; int32_t* sid; };

// ------------------------------------------------------------------------------------------ the work buffer
struct SqpWork {
    uint64_t* hdr;            // [8]: n[0..3] as the call reports them, [4] = the rows written = min(rows needed, R)
    uint64_t* src0;           // [n] the flat input index of a sequence's first kept id
    uint64_t* P;              // [n + 1]
    uint32_t* clen;           // [n]
    int32_t* place;           // [2 n] (row, column); (-1, -1): empty
    uint32_t* order;          // [n] sequences row-major: row r's are order[row_start[r] .. row_start[r + 1])
    uint32_t* ocol;           // [n] their columns
    uint32_t* K;              // [n + 1] next_fit: non-empty sequences in front of i; BFD: a sequence's rank in its row
    uint32_t* x0; uint32_t* x1; uint32_t* x2; uint32_t* x3;           // [n] each: the plan's scratch
    uint32_t* row_start;      // [R + 1]
    uint32_t* pad_before;     // [R + 1] rows in front of r that end in padding
    uint32_t* fill;           // [R]
};
SPL_HD uint64_t sqp_work_bytes(uint64_t n, uint64_t R) { return (64 + 8 * n + 8 * (n + 1) + 4 * (10 * n + 1) + 4 * (3 * R + 2) + 15) / 16 * 16; }
SPL_HD SqpWork sqp_work(void* work, uint64_t n, uint64_t R) {
    SqpWork w;
    w.hdr = static_cast<uint64_t*>(work); w.src0 = w.hdr + 8; w.P = w.src0 + n;
    w.clen = reinterpret_cast<uint32_t*>(w.P + n + 1); w.place = reinterpret_cast<int32_t*>(w.clen + n);
    w.order = reinterpret_cast<uint32_t*>(w.place + 2 * n); w.ocol = w.order + n; w.K = w.ocol + n;
    w.x0 = w.K + n + 1; w.x1 = w.x0 + n; w.x2 = w.x1 + n; w.x3 = w.x2 + n;
    w.row_start = w.x3 + n; w.pad_before = w.row_start + R + 1; w.fill = w.pad_before + R + 1;
    return w;
}

// ------------------------------------------------------------------------------------------ a sequence
SPL_HD bool sqp_in_i64(const SqpIn& in, const SqpGeo& g) { return (g.flags & COL_I64) && in.len; }        // (a CSR's ids are int32 whatever the rows are)
// sequence i: src0 = the flat index of its first KEPT id, clen = min(length, L), cut = it lost ids.  Returns true for a length below 0
// or above L_in, or offsets that decrease: such a sequence is empty and is reported.
SPL_HD bool sqp_seq(const SqpIn& in, const SqpGeo& g, uint32_t i, uint64_t& src0, uint32_t& clen, bool& cut) {
    uint64_t base, l;
    bool bad = false;
    if (in.len) {
        const int32_t x = in.len[i];
        bad = x < 0 || (uint32_t)x > in.L_in;
        l = bad ? 0u : (uint32_t)x;
        base = (uint64_t)i * in.L_in + ((g.flags & COL_PAD_LEFT) ? in.L_in - l : 0u);
    } else {
        const uint64_t a = in.off[i], b = in.off[(uint64_t)i + 1];
        bad = b < a;
        l = bad ? 0u : b - a;
        base = a;
    }
    clen = l < g.L ? (uint32_t)l : g.L;
    cut = l > g.L;
    src0 = base + ((g.flags & COL_KEEP_TAIL) ? l - clen : 0u);
    return bad;
}

// ------------------------------------------------------------------------------------------ next_fit
// the first j > i with P[j + 1] - P[i] > L (the first sequence a row that i opens cannot take); n: none
SPL_HD uint32_t sqp_next(const uint64_t* P, uint32_t n, uint32_t i, uint32_t L) {
    const uint64_t lim = P[i] + L;
    uint32_t lo = i + 1, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (P[(uint64_t)mid + 1] > lim) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// phase 2, element i: A = next, the mark of the walk's start
SPL_HD void sqp_nf_init(uint32_t i, const uint64_t* P, const uint32_t* clen, const uint32_t* K, uint32_t n, uint32_t L, uint32_t* A, uint32_t* M) {
    const bool ne = clen[i] != 0;
    A[i] = ne ? sqp_next(P, n, i, L) : n;
    M[i] = ne && K[i] == 0 ? 1u : 0u;
}
// phase 3, one round, element i: a marked i marks A[i]; B = A o A.  (A mark that another lane sets in this very round may or may not be
// seen: a marked sequence's A is on the walk either way.)
SPL_HD void sqp_nf_round(uint32_t i, const uint32_t* A, uint32_t* B, uint32_t* M, uint32_t n) {
    const uint32_t a = A[i];
    if (a >= n) { B[i] = n; return; }
    if (M[i]) M[a] = 1u;
    B[i] = A[a];
}
SPL_HD uint32_t sqp_nf_rounds(uint32_t nn) { uint32_t r = 0; while (r < 31 && (1u << r) < nn) r++; return r; }
// phase 4b, element i: row = the marks at or in front of i, minus one; first[row] = the row's first sequence
SPL_HD void sqp_nf_place(uint32_t i, const SqpWork& w, const uint32_t* row_of, const uint32_t* first) {
    if (w.clen[i] == 0) { w.place[2 * (uint64_t)i] = -1; w.place[2 * (uint64_t)i + 1] = -1; return; }
    const uint32_t row = row_of[i], col = (uint32_t)(w.P[i] - w.P[first[row]]), k = w.K[i];
    w.place[2 * (uint64_t)i] = (int32_t)row; w.place[2 * (uint64_t)i + 1] = (int32_t)col;
    w.order[k] = i; w.ocol[k] = col;
}

// ------------------------------------------------------------------------------------------ best_fit_decreasing
// can the LDS pool hold link[] and count[] behind head[]?
SPL_HD bool sqp_bfd_in_pool(uint32_t n, uint32_t L, uint32_t lds_max) { return n <= lds_max && (uint64_t)L + 1 + 2 * (uint64_t)n <= SQP_POOL; }
// One placement of the walk.  head[r] (r = 1 .. L): the row that reached the residual r last, SQP_NONE: none; link[row]: the row that
// reached ITS residual before it; bm0: bit r set iff head[r] has a row, bm1: bit w iff bm0[w] != 0.  A sequence of l ids goes to the
// head of the smallest r >= l that has a row, at column L - r; none: a new row.  Returns true for a new row.
SPL_HD bool sqp_bfd_place(uint32_t* head, uint32_t* bm0, uint32_t* bm1, uint32_t* link, uint32_t L, uint32_t l, uint32_t& rows, uint32_t& row,
                         uint32_t& col) {
    const uint32_t nw0 = L / 32 + 1, nw1 = nw0 / 32 + 1;
    uint32_t w = l >> 5, m = bm0[w] & (0xFFFFFFFFu << (l & 31)), r = SQP_NONE;
    if (m) r = w * 32 + (uint32_t)__builtin_ctz(m);
    else if (w + 1 < nw0) {
        uint32_t w1 = (w + 1) >> 5, m1 = bm1[w1] & (0xFFFFFFFFu << ((w + 1) & 31));
        while (!m1 && w1 + 1 < nw1) m1 = bm1[++w1];
        if (m1) { w = w1 * 32 + (uint32_t)__builtin_ctz(m1); r = w * 32 + (uint32_t)__builtin_ctz(bm0[w]); }
    }
    const bool is_new = r == SQP_NONE;
    if (is_new) { row = rows++; r = L; }
    else {
        row = head[r];
        const uint32_t nx = link[row];
        head[r] = nx;
        if (nx == SQP_NONE) { bm0[r >> 5] &= ~(1u << (r & 31)); if (bm0[r >> 5] == 0) bm1[r >> 10] &= ~(1u << ((r >> 5) & 31)); }
    }
    col = L - r;
    const uint32_t r2 = r - l;
    if (r2) { link[row] = head[r2]; head[r2] = row; bm0[r2 >> 5] |= 1u << (r2 & 31); bm1[r2 >> 10] |= 1u << ((r2 >> 5) & 31); }
    return is_new;
}
// bucket t of the descending scan holds the length L - t
SPL_HD uint32_t sqp_bfd_len_of(uint32_t L, uint32_t t) { return L - t; }
// the last phase, element i: rs[row] = where the row's sequences start in order[], K[i] = the sequence's rank in its row
SPL_HD void sqp_bfd_order(uint32_t i, const SqpWork& w, const uint32_t* rs) {
    if (w.clen[i] == 0) { w.place[2 * (uint64_t)i] = -1; w.place[2 * (uint64_t)i + 1] = -1; return; }
    const uint32_t k = rs[(uint32_t)w.place[2 * (uint64_t)i]] + w.K[i];
    w.order[k] = i; w.ocol[k] = (uint32_t)w.place[2 * (uint64_t)i + 1];
}

// ------------------------------------------------------------------------------------------ the plan's tail (both strategies)
SPL_HD uint32_t sqp_rows_written(uint32_t rows, uint32_t R) { return rows < R ? rows : R; }
// row r's fill: the end of its last sequence (0 from the rows written on)
SPL_HD uint32_t sqp_row_fill(const SqpWork& w, uint32_t r, uint32_t rows_w) {
    if (r >= rows_w) return 0;
    const uint32_t k = w.row_start[r + 1] - 1;
    return w.ocol[k] + w.clen[w.order[k]];
}
// cu_seqlens: the start of the sequence at order[k], then the start of row r's padding tail (fill < L), then the closing entry
SPL_HD void sqp_cu_seq(const SqpWork& w, uint32_t L, uint32_t k, int32_t* cu) {
    const uint32_t row = (uint32_t)w.place[2 * (uint64_t)w.order[k]];
    cu[(uint64_t)k + w.pad_before[row]] = (int32_t)(row * L + w.ocol[k]);
}
SPL_HD void sqp_cu_pad(const SqpWork& w, uint32_t L, uint32_t r, int32_t* cu) {
    if (w.fill[r] < L) cu[(uint64_t)w.row_start[r + 1] + w.pad_before[r]] = (int32_t)(r * L + w.fill[r]);
}
SPL_HD void sqp_finish(const SqpWork& w, const SqpGeo& g, const SqpPlanOut& o, uint32_t rows, uint64_t total, uint32_t cuts, uint32_t n_pad) {
    const uint32_t rows_w = sqp_rows_written(rows, g.R), placed = w.row_start[rows_w];
    if (o.cu) o.cu[(uint64_t)placed + n_pad] = (int32_t)(rows_w * g.L);
    w.hdr[0] = rows; w.hdr[1] = total; w.hdr[2] = (uint64_t)placed + n_pad + 1; w.hdr[3] = cuts; w.hdr[4] = rows_w;
    if (o.n) { o.n[0] = rows; o.n[1] = (int64_t)total; o.n[2] = (int64_t)placed + n_pad + 1; o.n[3] = cuts; }
}

// ------------------------------------------------------------------------------------------ the gather
SPL_HD uint32_t sqp_word(const void* a, uint64_t i, bool i64) { return static_cast<const uint32_t*>(a)[i64 ? 2 * i : i]; }    // (little endian: the low word)
// the LARGEST k of [ks, ke) with ocol[k] <= c (ocol[ks] == 0: a row's first sequence is at column 0)
SPL_HD uint32_t sqp_locate(const uint32_t* ocol, uint32_t ks, uint32_t ke, uint32_t c) {
    uint32_t lo = ks, hi = ke - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (ocol[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}
struct SqpGroup {
    uint32_t v[COL_VEC], lab[COL_VEC], pos[COL_VEC]; int32_t sid[COL_VEC];
    uint32_t by[4];           // by[a]: byte array a's four bytes, byte i for element i
    uint32_t mask;
};
// a label word: ignore_id is a NUMBER (sign-extended in int64), anything else an id (zero-extended)
SPL_HD int64_t sqp_label(uint32_t x, uint32_t ignore) { return x == ignore ? (int64_t)(int32_t)x : (int64_t)(uint64_t)x; }

// One lane's group: n (1..COL_VEC) flat elements of the [R, L] outputs from e0 on
SPL_HD void sqp_group(const SqpIn& in, const SqpGeo& g, const SqpWork& w, uint32_t rows_w, uint64_t e0, uint32_t n, SqpGroup& o) {
    uint64_t p; uint32_t c;
    col_rowcol(e0, g.L, p, c);
    const bool i64 = sqp_in_i64(in, g);
    o.mask = 0;
#pragma unroll
    for (uint32_t a = 0; a < 4; a++) o.by[a] = ((g.fills >> (8 * a)) & 0xFFu) * 0x01010101u;
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) { o.v[i] = g.pad_id; o.lab[i] = g.ignore_id; o.pos[i] = 0; o.sid[i] = -1; }
    for (uint32_t first = 0; first < n; p++, c = 0) {
        const uint32_t room = g.L - c, cnt = n - first < room ? n - first : room;
        if (p < rows_w) {
            const uint32_t ke = w.row_start[p + 1];
            uint32_t k = sqp_locate(w.ocol, w.row_start[p], ke, c);
            uint32_t s = w.order[k], c0 = w.ocol[k], l = w.clen[s];
            uint64_t src = w.src0[s];
#pragma unroll
            for (uint32_t i = 0; i < COL_VEC; i++) {
                if (i < first || i - first >= cnt) continue;
                const uint32_t cc = c + (i - first);
                if (cc >= c0 + l && k + 1 < ke) { k++; s = w.order[k]; c0 = w.ocol[k]; l = w.clen[s]; src = w.src0[s]; }
                const uint32_t j = cc - c0;
                if (j >= l) continue;                                           // the row's padding tail
                const uint64_t at = src + j;
                o.v[i] = sqp_word(in.ids, at, i64);
                if (in.labels) o.lab[i] = (j == 0 && (g.flags & SQP_MASK_FIRST)) ? g.ignore_id : sqp_word(in.labels, at, i64);
                o.pos[i] = j; o.sid[i] = (int32_t)s;
                o.mask |= 1u << (8 * i);
                const uint32_t keep = ~(0xFFu << (8 * i));
                if (in.b0) o.by[0] = (o.by[0] & keep) | ((uint32_t)in.b0[at] << (8 * i));
                if (in.b1) o.by[1] = (o.by[1] & keep) | ((uint32_t)in.b1[at] << (8 * i));
                if (in.b2) o.by[2] = (o.by[2] & keep) | ((uint32_t)in.b2[at] << (8 * i));
                if (in.b3) o.by[3] = (o.by[3] & keep) | ((uint32_t)in.b3[at] << (8 * i));
            }
        }
        first += cnt;
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the plan kernels' shared parts
// the inclusive scan of v over the workgroup's SQP_NT lanes and its total; s_ws: SQP_NT / 64 + 1 words
__device__ __forceinline__ uint64_t sqp_scan(uint64_t v, uint64_t* s_ws, uint64_t& total) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t x = wave_scan_incl64(v);
    if (lane == 63) s_ws[wv] = x;
    __syncthreads();
    if (wv == 0) {
        const uint64_t y = lane < SQP_NT / 64 ? s_ws[lane] : 0ull, ys = wave_scan_incl64(y);
        if (lane < SQP_NT / 64) s_ws[lane] = ys - y;
        if (lane == SQP_NT / 64 - 1) s_ws[SQP_NT / 64] = ys;
    }
    __syncthreads();
    const uint64_t r = x + s_ws[wv];
    total = s_ws[SQP_NT / 64];
    __syncthreads();                                    // (the next scan writes s_ws again)
    return r;
}
// phase 1: src0, clen, P (the scan of clen), K (the scan of the non-empty flags), the status.  total = P[n], nn = non-empty, cuts
__device__ __forceinline__ void sqp_lengths(const SqpIn& in, const SqpGeo& g, const SqpWork& w, uint32_t* status, uint64_t* s_ws, uint64_t& total,
                                           uint32_t& nn, uint32_t& cuts) {
    uint64_t cp = 0, ck = 0;
    for (uint32_t base = 0; base < in.n; base += SQP_NT) {
        const uint32_t i = base + threadIdx.x;
        uint32_t clen = 0;
        uint64_t flags = 0;
        if (i < in.n) {
            uint64_t src0; bool cut;
            if (sqp_seq(in, g, i, src0, clen, cut)) status[0] = 1u;
            w.src0[i] = src0; w.clen[i] = clen;
            flags = (clen ? 1ull : 0ull) | (cut && clen ? 1ull << 32 : 0ull);
        }
        uint64_t tp, tk;
        const uint64_t xp = sqp_scan(clen, s_ws, tp), xk = sqp_scan(flags, s_ws, tk);
        if (i < in.n) { w.P[i] = cp + xp - clen; w.K[i] = (uint32_t)(ck + xk) - (uint32_t)(flags & 1u); }
        cp += tp; ck += tk;
    }
    if (threadIdx.x == 0) { w.P[in.n] = cp; w.K[in.n] = (uint32_t)ck; }
    total = cp; nn = (uint32_t)ck; cuts = (uint32_t)(ck >> 32);
}
// the tail: row_fill, the padded rows in front of every row, cu_seqlens, seq_place, n
__device__ __forceinline__ void sqp_tail(const SqpIn& in, const SqpGeo& g, const SqpWork& w, const SqpPlanOut& o, uint32_t rows, uint64_t total, uint32_t cuts,
                                        uint64_t* s_ws) {
    const uint32_t rows_w = sqp_rows_written(rows, g.R);
    uint64_t cpad = 0;
    for (uint32_t base = 0; base < g.R; base += SQP_NT) {
        const uint32_t r = base + threadIdx.x;
        const uint32_t f = r < g.R ? sqp_row_fill(w, r, rows_w) : 0u, pf = r < rows_w && f < g.L ? 1u : 0u;
        if (r < g.R) { w.fill[r] = f; if (o.row_fill) o.row_fill[r] = (int32_t)f; }
        uint64_t t;
        const uint64_t x = sqp_scan(pf, s_ws, t);
        if (r < rows_w) w.pad_before[r] = (uint32_t)(cpad + x) - pf;
        cpad += t;
    }
    if (threadIdx.x == 0) w.pad_before[rows_w] = (uint32_t)cpad;
    __syncthreads();
    if (o.cu) {
        const uint32_t placed = w.row_start[rows_w];
        for (uint32_t k = threadIdx.x; k < placed; k += SQP_NT) sqp_cu_seq(w, g.L, k, o.cu);
        for (uint32_t r = threadIdx.x; r < rows_w; r += SQP_NT) sqp_cu_pad(w, g.L, r, o.cu);
    }
    if (o.place) for (uint64_t j = threadIdx.x; j < 2 * (uint64_t)in.n; j += SQP_NT) o.place[j] = w.place[j];
    if (threadIdx.x == 0) sqp_finish(w, g, o, rows, total, cuts, (uint32_t)cpad);
}

// ------------------------------------------------------------------------------------------ launch 1, next_fit: ONE workgroup
// (tests/hostsim/seqpack_sim.cpp shares the functions above, NOT these drivers: the phases are restated there lane by lane.)
__global__ __launch_bounds__(SQP_NT) void k_seqpack_next_fit(SqpIn in, SqpGeo g, void* __restrict__ work, SqpPlanOut o) {
    __shared__ uint32_t s_a[SQP_LDS_MAX], s_b[SQP_LDS_MAX], s_m[SQP_LDS_MAX];
    __shared__ uint64_t s_ws[SQP_NT / 64 + 1];
    const uint32_t n = in.n;
    const SqpWork w = sqp_work(work, n, g.R);
    const bool lds = n <= g.lds_max;
    uint32_t* A = lds ? s_a : w.x0;
    uint32_t* B = lds ? s_b : w.x1;
    uint32_t* M = lds ? s_m : w.x2;
    uint64_t total; uint32_t nn, cuts;
    sqp_lengths(in, g, w, o.status, s_ws, total, nn, cuts);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += SQP_NT) sqp_nf_init(i, w.P, w.clen, w.K, n, g.L, A, M);
    __syncthreads();
    for (uint32_t r = sqp_nf_rounds(nn); r; r--) {
        for (uint32_t i = threadIdx.x; i < n; i += SQP_NT) sqp_nf_round(i, A, B, M, n);
        __syncthreads();
        uint32_t* t = A; A = B; B = t;
    }
    // rows: the scan of the marks.  B: a sequence's row; A: a row's first sequence (the jump pointers are spent)
    uint64_t rows = 0;
    for (uint32_t base = 0; base < n; base += SQP_NT) {
        const uint32_t i = base + threadIdx.x, m = i < n ? M[i] : 0u;
        uint64_t t;
        const uint32_t row = (uint32_t)(rows + sqp_scan(m, s_ws, t)) - 1;
        if (i < n) B[i] = row;
        if (m) { A[row] = i; if (row <= g.R) w.row_start[row] = w.K[i]; }
        rows += t;
    }
    if (threadIdx.x == 0 && rows <= g.R) w.row_start[rows] = nn;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += SQP_NT) sqp_nf_place(i, w, B, A);
    __syncthreads();
    sqp_tail(in, g, w, o, (uint32_t)rows, total, cuts, s_ws);
}

// ------------------------------------------------------------------------------------------ launch 1, best_fit_decreasing: ONE workgroup
__global__ __launch_bounds__(SQP_NT) void k_seqpack_bfd(SqpIn in, SqpGeo g, void* __restrict__ work, SqpPlanOut o) {
    __shared__ uint32_t s_pool[SQP_POOL];
    __shared__ uint32_t s_bm0[SQP_BM0], s_bm1[SQP_BM1];
    __shared__ uint64_t s_ws[SQP_NT / 64 + 1];
    __shared__ uint32_t s_rows;
    const uint32_t n = in.n, L = g.L, lane = threadIdx.x & 63;
    const SqpWork w = sqp_work(work, n, g.R);
    const bool pool = sqp_bfd_in_pool(n, L, g.lds_max);
    uint32_t* head = s_pool;
    uint32_t* link = pool ? s_pool + L + 1 : w.x1;
    uint32_t* count = pool ? s_pool + L + 1 + n : w.x2;
    uint32_t* sorted = w.x0;
    uint32_t* slen = w.x3;
    uint64_t total; uint32_t nn, cuts;
    for (uint32_t r = threadIdx.x; r <= L; r += SQP_NT) head[r] = 0;
    sqp_lengths(in, g, w, o.status, s_ws, total, nn, cuts);
    __syncthreads();
    // the counting sort: histogram, the buckets' starts by length descending, the stable scatter
    for (uint32_t i = threadIdx.x; i < n; i += SQP_NT) { const uint32_t l = w.clen[i]; if (l) atomicAdd(&head[l], 1u); }
    __syncthreads();
    uint64_t carry = 0;
    for (uint32_t base = 0; base < L; base += SQP_NT) {
        const uint32_t t = base + threadIdx.x, l = sqp_bfd_len_of(L, t < L ? t : 0u), c = t < L ? head[l] : 0u;
        uint64_t tt;
        const uint64_t x = sqp_scan(c, s_ws, tt);
        if (t < L) head[l] = (uint32_t)(carry + x) - c;
        carry += tt;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane, key = i < n ? w.clen[i] : 0u;
            bool todo = key != 0;
            unsigned long long left = __ballot(todo);
            while (left) {
                const uint32_t k = (uint32_t)__shfl((int)key, __ffsll((long long)left) - 1);
                const unsigned long long m = __ballot(todo && key == k);
                if (todo && key == k) {
                    const uint32_t at = head[k] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
                    sorted[at] = i; slen[at] = key;
                    todo = false;
                }
                if (lane == (uint32_t)(__ffsll((long long)m) - 1)) head[k] += (uint32_t)__popcll(m);
                left &= ~m;
            }
        }
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r <= L; r += SQP_NT) head[r] = SQP_NONE;
    for (uint32_t r = threadIdx.x; r < SQP_BM0; r += SQP_NT) s_bm0[r] = 0;
    if (threadIdx.x < SQP_BM1) s_bm1[threadIdx.x] = 0;
    __syncthreads();
    // the walk: one lane.  The next sequence and its length do not depend on the placement and are loaded one step ahead
    if (threadIdx.x == 0) {
        uint32_t rows = 0, i_nx = nn ? sorted[0] : 0u, l_nx = nn ? slen[0] : 0u;
        for (uint32_t t = 0; t < nn; t++) {
            const uint32_t i = i_nx, l = l_nx;
            if (t + 1 < nn) { i_nx = sorted[t + 1]; l_nx = slen[t + 1]; }
            uint32_t row, col;
            const bool is_new = sqp_bfd_place(head, s_bm0, s_bm1, link, L, l, rows, row, col);
            const uint32_t rank = is_new ? 0u : count[row];
            count[row] = rank + 1;
            w.place[2 * (uint64_t)i] = (int32_t)row; w.place[2 * (uint64_t)i + 1] = (int32_t)col; w.K[i] = rank;
        }
        s_rows = rows;
    }
    __syncthreads();
    const uint32_t rows = s_rows;
    uint32_t* rs = w.x0;                                 // (the sorted order is spent)
    carry = 0;
    for (uint32_t base = 0; base < rows; base += SQP_NT) {
        const uint32_t r = base + threadIdx.x, c = r < rows ? count[r] : 0u;
        uint64_t tt;
        const uint64_t x = sqp_scan(c, s_ws, tt);
        if (r < rows) { const uint32_t at = (uint32_t)(carry + x) - c; rs[r] = at; if (r <= g.R) w.row_start[r] = at; }
        carry += tt;
    }
    if (threadIdx.x == 0 && rows <= g.R) w.row_start[rows] = nn;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += SQP_NT) sqp_bfd_order(i, w, rs);
    __syncthreads();
    sqp_tail(in, g, w, o, rows, total, cuts, s_ws);
}

// ------------------------------------------------------------------------------------------ launch 2: the gather
template <bool I64> __device__ __forceinline__ void sqp_store_labels(void* labels, uint64_t e, uint32_t n, const uint32_t x[COL_VEC], uint32_t ignore) {
    if (I64) {
        int64_t* q = static_cast<int64_t*>(labels) + e;
        if (n == COL_VEC) {
            const uint64_t y0 = (uint64_t)sqp_label(x[0], ignore), y1 = (uint64_t)sqp_label(x[1], ignore), y2 = (uint64_t)sqp_label(x[2], ignore),
                           y3 = (uint64_t)sqp_label(x[3], ignore);
            reinterpret_cast<uint4*>(q)[0] = make_uint4((uint32_t)y0, (uint32_t)(y0 >> 32), (uint32_t)y1, (uint32_t)(y1 >> 32));
            reinterpret_cast<uint4*>(q)[1] = make_uint4((uint32_t)y2, (uint32_t)(y2 >> 32), (uint32_t)y3, (uint32_t)(y3 >> 32));
        } else {                                        // (a constant index into x[]: a lane's own index would put the group into scratch memory)
#pragma unroll
            for (uint32_t i = 0; i < COL_VEC; i++) if (i < n) q[i] = sqp_label(x[i], ignore);
        }
    } else {
        uint32_t* q = static_cast<uint32_t*>(labels) + e;
        if (n == COL_VEC) *reinterpret_cast<uint4*>(q) = make_uint4(x[0], x[1], x[2], x[3]);
        else {
#pragma unroll
            for (uint32_t i = 0; i < COL_VEC; i++) if (i < n) q[i] = x[i];
        }
    }
}

// grid: cpair_grid(R * L) -- one workgroup per span of COL_SPAN flat elements; every element of the [R, L] outputs is written
template <bool I64>
__global__ __launch_bounds__(COL_NT) void k_seqpack_gather(SqpIn in, SqpGeo g, void* __restrict__ work, SqpRowsOut o) {
    const uint64_t total = (uint64_t)g.R * g.L;
    const uint64_t e0 = cpair_span(blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y) * COL_SPAN + (uint64_t)threadIdx.x * COL_VEC;
    if (e0 >= total) return;
    const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
    const SqpWork w = sqp_work(work, in.n, g.R);
    SqpGroup q;
    sqp_group(in, g, w, (uint32_t)w.hdr[4], e0, n, q);
    // (The rows' tail and the copy of pos are this kernel's own, NOT col_store_group and a cast: through those the int64 gather measured
    //  1 .. 3 % slower than before -- profiles/shared_prims_ab.txt -- and as written here the kernel compiles to the code it had.)
    if (n == COL_VEC) col_store4<I64>(o.rows, e0, q.v);
    else {                                              // the final partial group: nothing is written past R * L
#pragma unroll
        for (uint32_t i = 0; i < COL_VEC; i++) if (i < n) col_store1<I64>(o.rows, e0 + i, q.v[i]);
    }
    if (o.labels) sqp_store_labels<I64>(o.labels, e0, n, q.lab, g.ignore_id);
    col_store_bytes(o.b0, e0, n, q.by[0]);
    col_store_bytes(o.b1, e0, n, q.by[1]);
    col_store_bytes(o.b2, e0, n, q.by[2]);
    col_store_bytes(o.b3, e0, n, q.by[3]);
    col_store_bytes(o.mask, e0, n, q.mask);
    int32_t pos[COL_VEC];
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) pos[i] = (int32_t)q.pos[i];
    col_store_i32(o.pos, e0, n, pos);
    col_store_i32(o.sid, e0, n, q.sid);
}
#endif  // __HIPCC__

}  // namespace spl
