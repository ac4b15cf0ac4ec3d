// seqpack_sim.cpp -- TEST TOOL: the decisions of splintr_amd/csrc/spl_k_seqpack.h (the code k_seqpack_next_fit, k_seqpack_bfd and
// k_seqpack_gather run) evaluated on the CPU.  The gather: for every output element, with the kernel's geometry -- the grid of cpair_grid,
// workgroups of COL_NT lanes, COL_VEC elements a lane, the final partial group stored element by element.  The plans: the one workgroup's
// phases are RESTATED here lane by lane (SQP_NT lanes a round, a barrier between phases, the scans as wavefront scans plus the wavefronts'
// sums, the doubling rounds, the ballot ranking of the counting sort's scatter, the one-lane walk) over the same functions; the "LDS"
// arrays are vectors of the kernel's sizes with a canary behind them, chosen by the same conditions.  A change to a driver in the kernel
// is checked by tests/test_gpu_seqpack.py alone.  Built with g++; no GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_seqpack.h"

using namespace spl;

namespace {

constexpr uint32_t CANARY = 0xC0FFEE11u;

// sqp_scan, restated: 64-lane inclusive scans, then the wavefronts' sums scanned and added
void scan(const std::vector<uint64_t>& v, std::vector<uint64_t>& x, uint64_t& total) {
    uint64_t ws[SQP_NT / 64];
    for (uint32_t wv = 0; wv < SQP_NT / 64; wv++) {
        uint64_t run = 0;
        for (uint32_t lane = 0; lane < 64; lane++) { run += v[wv * 64 + lane]; x[wv * 64 + lane] = run; }
        ws[wv] = run;
    }
    uint64_t run = 0;
    for (uint32_t wv = 0; wv < SQP_NT / 64; wv++) {
        for (uint32_t lane = 0; lane < 64; lane++) x[wv * 64 + lane] += run;
        run += ws[wv];
    }
    total = run;
}

struct Plan {
    SqpIn in; SqpGeo g; SqpWork w; SqpPlanOut o;
    std::vector<uint64_t> v = std::vector<uint64_t>(SQP_NT), x = std::vector<uint64_t>(SQP_NT), v2 = std::vector<uint64_t>(SQP_NT),
                          x2 = std::vector<uint64_t>(SQP_NT);
    uint64_t total = 0; uint32_t nn = 0, cuts = 0;

    void lengths() {                                     // sqp_lengths
        uint64_t cp = 0, ck = 0;
        for (uint32_t base = 0; base < in.n; base += SQP_NT) {
            for (uint32_t tid = 0; tid < SQP_NT; tid++) {
                const uint32_t i = base + tid;
                v[tid] = 0; v2[tid] = 0;
                if (i < in.n) {
                    uint64_t src0; uint32_t clen; bool cut;
                    if (sqp_seq(in, g, i, src0, clen, cut)) o.status[0] = 1u;
                    w.src0[i] = src0; w.clen[i] = clen;
                    v[tid] = clen; v2[tid] = (clen ? 1ull : 0ull) | (cut && clen ? 1ull << 32 : 0ull);
                }
            }
            uint64_t tp, tk;
            scan(v, x, tp); scan(v2, x2, tk);
            for (uint32_t tid = 0; tid < SQP_NT; tid++) {
                const uint32_t i = base + tid;
                if (i < in.n) { w.P[i] = cp + x[tid] - v[tid]; w.K[i] = (uint32_t)(ck + x2[tid]) - (uint32_t)(v2[tid] & 1u); }
            }
            cp += tp; ck += tk;
        }
        w.P[in.n] = cp; w.K[in.n] = (uint32_t)ck;
        total = cp; nn = (uint32_t)ck; cuts = (uint32_t)(ck >> 32);
    }

    void tail(uint32_t rows) {                           // sqp_tail
        const uint32_t rows_w = sqp_rows_written(rows, g.R);
        uint64_t cpad = 0;
        for (uint32_t base = 0; base < g.R; base += SQP_NT) {
            for (uint32_t tid = 0; tid < SQP_NT; tid++) {
                const uint32_t r = base + tid;
                const uint32_t f = r < g.R ? sqp_row_fill(w, r, rows_w) : 0u;
                v[tid] = r < rows_w && f < g.L ? 1u : 0u;
                if (r < g.R) { w.fill[r] = f; if (o.row_fill) o.row_fill[r] = (int32_t)f; }
            }
            uint64_t t;
            scan(v, x, t);
            for (uint32_t tid = 0; tid < SQP_NT; tid++) if (base + tid < rows_w) w.pad_before[base + tid] = (uint32_t)(cpad + x[tid]) - (uint32_t)v[tid];
            cpad += t;
        }
        w.pad_before[rows_w] = (uint32_t)cpad;
        if (o.cu) {
            const uint32_t placed = w.row_start[rows_w];
            for (uint32_t k = 0; k < placed; k++) sqp_cu_seq(w, g.L, k, o.cu);
            for (uint32_t r = 0; r < rows_w; r++) sqp_cu_pad(w, g.L, r, o.cu);
        }
        if (o.place) for (uint64_t j = 0; j < 2 * (uint64_t)in.n; j++) o.place[j] = w.place[j];
        sqp_finish(w, g, o, rows, total, cuts, (uint32_t)cpad);
    }

    int next_fit() {                                     // k_seqpack_next_fit
        std::vector<uint32_t> s_a(SQP_LDS_MAX + 1, CANARY), s_b(SQP_LDS_MAX + 1, CANARY), s_m(SQP_LDS_MAX + 1, CANARY);
        const uint32_t n = in.n;
        const bool lds = n <= g.lds_max;
        uint32_t* A = lds ? s_a.data() : w.x0;
        uint32_t* B = lds ? s_b.data() : w.x1;
        uint32_t* M = lds ? s_m.data() : w.x2;
        lengths();
        for (uint32_t i = 0; i < n; i++) sqp_nf_init(i, w.P, w.clen, w.K, n, g.L, A, M);
        for (uint32_t r = sqp_nf_rounds(nn); r; r--) {
            // (the lanes of a round in index order, and again in reverse order in every other round: a mark set within the round is seen
            //  by some lanes and not by others, as on the device)
            if (r & 1) for (uint32_t i = 0; i < n; i++) sqp_nf_round(i, A, B, M, n);
            else for (uint32_t i = n; i-- > 0;) sqp_nf_round(i, A, B, M, n);
            uint32_t* t = A; A = B; B = t;
        }
        uint64_t rows = 0;
        for (uint32_t base = 0; base < n; base += SQP_NT) {
            for (uint32_t tid = 0; tid < SQP_NT; tid++) v[tid] = base + tid < n ? M[base + tid] : 0u;
            uint64_t t;
            scan(v, x, t);
            for (uint32_t tid = 0; tid < SQP_NT; tid++) {
                const uint32_t i = base + tid, row = (uint32_t)(rows + x[tid]) - 1;
                if (i < n) B[i] = row;
                if (v[tid]) { A[row] = i; if (row <= g.R) w.row_start[row] = w.K[i]; }
            }
            rows += t;
        }
        if (rows <= g.R) w.row_start[rows] = nn;
        for (uint32_t i = 0; i < n; i++) sqp_nf_place(i, w, B, A);
        tail((uint32_t)rows);
        return s_a[SQP_LDS_MAX] == CANARY && s_b[SQP_LDS_MAX] == CANARY && s_m[SQP_LDS_MAX] == CANARY ? 0 : -2;
    }

    int bfd() {                                          // k_seqpack_bfd
        std::vector<uint32_t> s_pool(SQP_POOL + 1, CANARY), s_bm0(SQP_BM0 + 1, CANARY), s_bm1(SQP_BM1 + 1, CANARY);
        const uint32_t n = in.n, L = g.L;
        const bool pool = sqp_bfd_in_pool(n, L, g.lds_max);
        uint32_t* head = s_pool.data();
        uint32_t* link = pool ? head + L + 1 : w.x1;
        uint32_t* count = pool ? head + L + 1 + n : w.x2;
        uint32_t* sorted = w.x0;
        uint32_t* slen = w.x3;
        for (uint32_t r = 0; r <= L; r++) head[r] = 0;
        lengths();
        for (uint32_t i = 0; i < n; i++) if (w.clen[i]) head[w.clen[i]]++;
        uint64_t carry = 0;
        for (uint32_t base = 0; base < L; base += SQP_NT) {
            for (uint32_t tid = 0; tid < SQP_NT; tid++) { const uint32_t t = base + tid; v[tid] = t < L ? head[sqp_bfd_len_of(L, t)] : 0u; }
            uint64_t tt;
            scan(v, x, tt);
            for (uint32_t tid = 0; tid < SQP_NT; tid++) { const uint32_t t = base + tid; if (t < L) head[sqp_bfd_len_of(L, t)] = (uint32_t)(carry + x[tid]) - (uint32_t)v[tid]; }
            carry += tt;
        }
        for (uint32_t base = 0; base < n; base += 64) {  // wavefront 0: equal keys rank themselves by a ballot
            uint32_t key[64]; bool todo[64];
            uint64_t left = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                key[lane] = base + lane < n ? w.clen[base + lane] : 0u;
                todo[lane] = key[lane] != 0;
                if (todo[lane]) left |= 1ull << lane;
            }
            while (left) {
                const uint32_t k = key[__builtin_ffsll((long long)left) - 1];
                uint64_t m = 0;
                for (uint32_t lane = 0; lane < 64; lane++) if (todo[lane] && key[lane] == k) m |= 1ull << lane;
                const uint32_t start = head[k];
                for (uint32_t lane = 0; lane < 64; lane++) {
                    if (!(todo[lane] && key[lane] == k)) continue;
                    const uint32_t at = start + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1));
                    sorted[at] = base + lane; slen[at] = key[lane];
                    todo[lane] = false;
                }
                head[k] = start + (uint32_t)__builtin_popcountll(m);
                left &= ~m;
            }
        }
        for (uint32_t r = 0; r <= L; r++) head[r] = SQP_NONE;
        for (uint32_t r = 0; r < SQP_BM0; r++) s_bm0[r] = 0;
        for (uint32_t r = 0; r < SQP_BM1; r++) s_bm1[r] = 0;
        uint32_t rows = 0, i_nx = nn ? sorted[0] : 0u, l_nx = nn ? slen[0] : 0u;
        for (uint32_t t = 0; t < nn; t++) {
            const uint32_t i = i_nx, l = l_nx;
            if (t + 1 < nn) { i_nx = sorted[t + 1]; l_nx = slen[t + 1]; }
            uint32_t row, col;
            const bool is_new = sqp_bfd_place(head, s_bm0.data(), s_bm1.data(), link, L, l, rows, row, col);
            const uint32_t rank = is_new ? 0u : count[row];
            count[row] = rank + 1;
            w.place[2 * (uint64_t)i] = (int32_t)row; w.place[2 * (uint64_t)i + 1] = (int32_t)col; w.K[i] = rank;
        }
        uint32_t* rs = w.x0;
        carry = 0;
        for (uint32_t base = 0; base < rows; base += SQP_NT) {
            for (uint32_t tid = 0; tid < SQP_NT; tid++) v[tid] = base + tid < rows ? count[base + tid] : 0u;
            uint64_t tt;
            scan(v, x, tt);
            for (uint32_t tid = 0; tid < SQP_NT; tid++) {
                const uint32_t r = base + tid;
                if (r < rows) { const uint32_t at = (uint32_t)(carry + x[tid]) - (uint32_t)v[tid]; rs[r] = at; if (r <= g.R) w.row_start[r] = at; }
            }
            carry += tt;
        }
        if (rows <= g.R) w.row_start[rows] = nn;
        for (uint32_t i = 0; i < n; i++) sqp_bfd_order(i, w, rs);
        tail(rows);
        return s_pool[SQP_POOL] == CANARY && s_bm0[SQP_BM0] == CANARY && s_bm1[SQP_BM1] == CANARY ? 0 : -2;
    }
};

}  // namespace

extern "C" {

void sq_geometry(uint32_t out[8]) {
    out[0] = COL_NT; out[1] = COL_VEC; out[2] = COL_SPAN; out[3] = SQP_NT; out[4] = SQP_LDS_MAX; out[5] = SQP_POOL; out[6] = SQP_BFD_MAX_L; out[7] = 0;
}
uint64_t sq_work_bytes(uint64_t n, uint64_t R) { return sqp_work_bytes(n, R); }

// in: ids, len, off, labels, b0..b3 (the input's element type follows flags & 1 in the rows form, int32 in the CSR form); out: rows / labels of
// the rows' dtype, b0..b3, mask, pos, sid [R * L]; place [2 n]; fill [R]; cu [n + R + 1]; n [4]; status [1]; work: sq_work_bytes(n, R).  Each
// output but rows, status and work may be null.  Returns 0, or -2 if a restated LDS array was written past its end.
int sq_pack(const void* ids, const int32_t* len, const uint64_t* off, const void* labels, const uint8_t* const* bin, uint32_t n, uint32_t L_in,
            uint32_t flags, uint32_t strategy, uint32_t L, uint32_t pad_id, uint32_t ignore_id, uint32_t fills, uint32_t R, uint32_t lds_max,
            void* rows, void* labels_out, uint8_t* const* bout, uint8_t* mask, int32_t* pos, int32_t* sid, int32_t* place, int32_t* fill,
            int32_t* cu, int64_t* n_out, uint32_t* status, void* work) {
    Plan p;
    p.in = SqpIn{ids, len, off, labels, bin[0], bin[1], bin[2], bin[3], n, L_in};
    p.g = SqpGeo{flags, strategy, L, pad_id, ignore_id, fills, R, lds_max};
    p.w = sqp_work(work, n, R);
    p.o = SqpPlanOut{place, fill, cu, n_out, status};
    const int rc = strategy == SQP_BFD ? p.bfd() : p.next_fit();
    if (rc) return rc;
    const bool i64 = (flags & COL_I64) != 0;
    uint8_t* ob[4];
    for (int a = 0; a < 4; a++) ob[a] = bin[a] ? bout[a] : nullptr;
    if (!labels) labels_out = nullptr;
    const uint64_t total = (uint64_t)R * L;
    if (!total) return 0;
    uint32_t gx, gy, gz;
    cpair_grid(total, gx, gy, gz);
    for (uint32_t bz = 0; bz < gz; bz++)
        for (uint32_t by = 0; by < gy; by++)
            for (uint32_t bx = 0; bx < gx; bx++)
                for (uint32_t lane = 0; lane < COL_NT; lane++) {
                    const uint64_t e0 = cpair_span(bx, by, bz, gx, gy) * COL_SPAN + (uint64_t)lane * COL_VEC;
                    if (e0 >= total) continue;
                    const uint32_t cnt = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
                    SqpGroup q;
                    sqp_group(p.in, p.g, p.w, (uint32_t)p.w.hdr[4], e0, cnt, q);
                    for (uint32_t i = 0; i < cnt; i++) {
                        if (i64) static_cast<uint64_t*>(rows)[e0 + i] = q.v[i]; else static_cast<uint32_t*>(rows)[e0 + i] = q.v[i];
                        if (labels_out) {
                            if (i64) static_cast<int64_t*>(labels_out)[e0 + i] = sqp_label(q.lab[i], ignore_id);
                            else static_cast<uint32_t*>(labels_out)[e0 + i] = q.lab[i];
                        }
                        for (int a = 0; a < 4; a++) if (ob[a]) ob[a][e0 + i] = (uint8_t)(q.by[a] >> (8 * i));
                        if (mask) mask[e0 + i] = (uint8_t)(q.mask >> (8 * i));
                        if (pos) pos[e0 + i] = (int32_t)q.pos[i];
                        if (sid) sid[e0 + i] = q.sid[i];
                    }
                }
    return 0;
}

}  // extern "C"
