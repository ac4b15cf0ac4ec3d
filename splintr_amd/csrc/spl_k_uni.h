// spl_k_uni.h -- part of spl_kernels.hip (included there, behind spl_k_wp.h; one translation unit): Unigram mode (k_uni_match<count>,
// k_uni_match<write>, k_uni_long<count>, k_uni_long<write>), an encode path of its own beside the tile kernel.
//
// The mode is Hugging Face's pre_tokenizers.Metaspace -> models.Unigram.encode_optimized (byte_fallback off, fuse_unk on), restated in
// every 0x20 stands for U+2581, a word starts at a document start and at every U+2581, and a word becomes the path of
// highest score through the keys that tile it -- best[e] = max over keys word[s:e] of best[s] + score, ONE f64 add per proposal, a
// proposal replaces the incumbent only when strictly greater, starts visited in ascending order; a character without a key of its own
// proposes unk_id at min_score - 10, and a run of unk on the chosen path is one id.
//
// The kernels read the CALLER's text: nothing is rewritten.  A word that starts at a 0x20, or at a document start without a marker
// (prepend "always"), has a SOURCE in front of its first raw byte whose walks begin at the trie node of E2 96 81 (found on the host),
// so the virtual marker costs no probe.
//
// k_uni_match: a workgroup of UNI_NT lanes owns UNI_TB raw bytes plus a halo of UNI_H and decides every word that STARTS in the tile and
// ends within UNI_H of its start.  Phase A, a lane per character start: walk the hashed trie (WordPiece mode's layout) towards the
// word's end and append an edge {f64 score, id, end, next} to a pool in LDS at every node that carries an id, chained from the start's
// head -- the score load does not depend on the walk's next probe.  Phase B, a lane per word start: the dynamic program over the LDS
// edges (best f64, id and back pointer per raw position: words tile the text, so the arrays are shared without conflict), then the
// back-track with unk fusing.  A start whose edges did not fit the pool is walked again by the word's lane, so the result does not
// depend on the pool's size.  Counts go through a workgroup scan; the count pass leaves the tile's tokens, k_decode_scan the bases,
// the write pass -- the same body -- stores ids from each word's last slot backwards and the documents' offsets.  No atomics on ids.
//
// k_uni_long: a word longer than UNI_H is logged by its tile (at most UNI_LREC a tile) and served by a wavefront of its own: best /
// id / back arrays in a global workspace indexed by raw position, blocks of 64 starts -- the lanes walk and collect edges in LDS, lane
// 0 relaxes the block in order.  Its count is added to the tile's count before the scan; the tile's write pass leaves its slots open
// and tells it where they are.
#pragma once
#include "spl_common.h"
#include "spl_k_textspans.h"
#include "spl_k_wp.h"

namespace spl {

constexpr int UNI_TB = 512, UNI_NT = 256, UNI_H = 128;      // tile, lanes, halo: a word of up to UNI_H raw bytes is decided in LDS
constexpr int UNI_R = UNI_TB + UNI_H, UNI_PAD = 16;         // staged: UNI_PAD bytes in front (character starts look three bytes back), 16 behind
constexpr int UNI_S = UNI_PAD + UNI_R + 16;                 // positions of the staged window ("P" below: raw - tile base + UNI_PAD)
constexpr int UNI_BW = (UNI_S + 31) / 32;                   // words of a bitmap over it
constexpr int UNI_POOL = 2048;                              // edges of a tile's pool (16 bytes each)
constexpr int UNI_LREC = UNI_TB / UNI_H + 1;                // words longer than UNI_H that can START in one tile
constexpr int UNI_LB = 64, UNI_LPOOL = 1024;                // the long path: starts a block, edges of a block's pool
constexpr uint64_t UNI_MAX_BYTES = 64ull << 20;             // one device call
constexpr uint32_t UNI_FROM_S = 0xFFFFFFFEu, UNI_UNSET = 0xFFFFFFFFu;      // back pointers: the word's source; no proposal yet
constexpr uint32_t UNI_H_NONE = 0xFFFFu, UNI_H_WALK = 0xFFFEu;             // edge heads: no edge; not collected (walk the trie again)

struct UniEdge { double score; uint32_t id; uint16_t end, next; };
// best / id / back pointer per position: LDS arrays over the staged window, or the global workspace over the raw text
struct UniNodes { double* best; uint32_t* bid; uint32_t* bfrom; };

struct UniArgs {
    const uint8_t* text; uint32_t n_bytes;                   // the caller's text, 16-byte aligned, readable to the next multiple of 16
    const uint64_t* doc_off; uint32_t n_docs;
    WpTrie trie; const double* score;                        // node -> id, id -> score
    uint32_t marker_node;                                    // the node of E2 96 81 (WP_NONE: no key begins with U+2581)
    uint32_t unk_id, prepend; double unk_score;              // min_score - 10
    uint64_t* cnt;                                           // [tiles + 1]: tokens per tile; exclusive sums and the total
    uint32_t* lr_n; uint32_t* lr_start; uint32_t* lr_cnt; uint64_t* lr_slot;   // long words: [tiles], [tiles * UNI_LREC] x 3
    UniNodes g;                                              // [n_bytes + 1] each: the long path's nodes
    uint32_t* ids; uint64_t ids_cap; uint64_t* out_off;
    TextSpanOut so;                                          // the <write, span> kernels only: where the spans go
};

// ---- the per-word logic, plain C++ ---------------------------------------------------------------------------------------------------
SPL_HD bool uni_bit(const uint32_t* m, uint32_t p) { return (m[p >> 5] >> (p & 31u)) & 1u; }
// The first set bit of m in [from, to), or `to`.
SPL_HD uint32_t uni_next_bit(const uint32_t* m, uint32_t from, uint32_t to) {
    for (uint32_t p = from; p < to;) {
        const uint32_t w = m[p >> 5] >> (p & 31u);
        if (w) { const uint32_t q = p + (uint32_t)__builtin_ctz(w); return q < to ? q : to; }
        p = (p | 31u) + 1u;
    }
    return to;
}
// Bytes of the character at p[0 .. avail): a well-formed character's length, else 1 (a byte by itself, which no key covers).
SPL_HD uint32_t uni_clen(const uint8_t* p, uint32_t avail, uint32_t brk) {
    uint32_t cp = 0;
    const uint32_t n = wp_decode(p, avail, brk, cp);
    return n ? n : 1u;
}
// Is p[0] a character start?  Every byte is unless a well-formed character that starts one to `back` (at most three) bytes in front covers
// it.  brk(k): does a document start at p + k (k in -2 .. 3)?  A character does not reach across one.
template <class Brk> SPL_HD bool uni_is_start(const uint8_t* p, uint32_t back, uint32_t avail, Brk&& brk) {
    if ((p[0] & 0xC0u) != 0x80u) return true;
    for (uint32_t k = 1; k <= back && k <= 3u; k++) {
        if (brk(1 - (int)k)) return true;                    // a document starts between p - k and p, p included: nothing reaches over it
        if (p[-(int)k] < 0xC2u) continue;
        const uint32_t m = (brk(2 - (int)k) ? 4u : 0u) | (brk(3 - (int)k) ? 8u : 0u);      // (bit 1, p - k + 1, was tested above or is p's own)
        return uni_clen(p - k, avail + k, m) <= k;           // the nearest lead byte decides
    }
    return true;
}
// A proposal for position e: it replaces the incumbent only when strictly greater (the earliest start wins a tie).
SPL_HD void uni_relax(const UniNodes& n, uint32_t e, double v, uint32_t id, uint32_t from) {
    if (n.bfrom[e] == UNI_UNSET || v > n.best[e]) { n.best[e] = v; n.bid[e] = id; n.bfrom[e] = from; }
}
// The chosen path from `we` back to the word's first node b; with a source (has_vm) node b is reached from it by id_b.  A run of unk is
// one id.  Returns the tokens; WRITE stores them backwards from ids[at] (only below cap).  Every back pointer is checked to lie in
// [b, e): a node without a proposal ends the walk instead of leading it astray.  span(slot, from, e, fused): the edge (from, e] --
// from UNI_FROM_S: the source's -- belongs to the id in `slot`; fused: as one more unk at the front of the run that slot holds.
struct UniNoSpan { SPL_HD void operator()(uint64_t, uint32_t, uint32_t, bool) const {} };
template <bool WRITE, class SPAN = UniNoSpan> SPL_HD uint32_t uni_backtrack(const UniNodes& n, uint32_t b, uint32_t we, bool has_vm, uint32_t id_b, uint32_t unk_id,
                                                    uint32_t* ids, uint64_t at, uint64_t cap, SPAN&& span = SPAN()) {
    uint32_t cnt = 0, e = we;
    bool prev_unk = false;
    for (;;) {
        uint32_t id, from;
        if (e == b) { if (!has_vm) break; id = id_b; from = UNI_FROM_S; }
        else { id = n.bid[e]; from = n.bfrom[e]; if (from != UNI_FROM_S && (from < b || from >= e)) break; }
        const bool unk = id == unk_id;
        if (!(unk && prev_unk)) {
            if (WRITE) { if (at < cap) { ids[at] = id; span(at, from, e, false); } at--; }
            cnt++;
        } else if (WRITE) { if (at + 1u < cap) span(at + 1u, from, e, true); }
        prev_unk = unk;
        if (from == UNI_FROM_S) break;
        e = from;
    }
    return cnt;
}

#if defined(__HIPCC__)
// One trie walk over txt[j0 .. lim) from `node`; fn(id, end, score) at every node that carries an id (first: the start node itself is
// looked at, the marker's).  fn returns false to end the walk.
template <class F> __device__ __forceinline__ void uni_walk(const UniArgs& a, const uint8_t* txt, uint32_t node, bool first, uint32_t j0, uint32_t lim, F&& fn) {
    if (node == WP_NONE) return;
    if (first) { const uint32_t id = a.trie.node_id[node]; if (id != WP_NONE && !fn(id, j0, a.score[id])) return; }
    for (uint32_t j = j0; j < lim;) {
        node = wp_child(a.trie, node, txt[j]);
        if (node == WP_NONE) return;
        j++;
        const uint32_t id = a.trie.node_id[node];
        if (id != WP_NONE && !fn(id, j, a.score[id])) return;
    }
}
// The edges of one start: the chain from head h, or -- not collected -- the walk itself.  off: what a walk's positions are shifted by
// against the edges' (the long path's pool holds positions relative to its block).
template <class F> __device__ __forceinline__ void uni_edges(const UniArgs& a, const UniEdge* pool, uint32_t h, const uint8_t* txt, uint32_t node, bool first,
                                                             uint32_t j0, uint32_t lim, uint32_t off, F&& fn) {
    if (h == UNI_H_WALK) uni_walk(a, txt, node, first, j0, lim, [&](uint32_t id, uint32_t e, double sc) { fn(id, e, sc); return true; });
    else for (; h != UNI_H_NONE; h = pool[h].next) fn(pool[h].id, (uint32_t)pool[h].end + off, pool[h].score);
}
// The dynamic program's step for start s of a word that ends at we: every edge proposes, unk does if no key covers the one character.
__device__ __forceinline__ void uni_step(const UniArgs& a, const UniNodes& n, const UniEdge* pool, uint32_t h, const uint8_t* txt, uint32_t s, uint32_t we,
                                         uint32_t off, double from_best) {
    const uint32_t ce = s + uni_clen(txt + s, we - s, 0u);
    bool single = false;
    uni_edges(a, pool, h, txt, 0u, false, s, we, off, [&](uint32_t id, uint32_t e, double sc) {
        single |= e == ce;
        uni_relax(n, e, sc + from_best, id, s);
    });
    if (!single) uni_relax(n, ce, a.unk_score + from_best, a.unk_id, s);
}
// The source's step: its walks begin at the marker's node; the edge that is the marker alone gives node b (best_b, id_b).
__device__ __forceinline__ void uni_step_source(const UniArgs& a, const UniNodes& n, const UniEdge* pool, uint32_t h, const uint8_t* txt, uint32_t b, uint32_t we,
                                                uint32_t off, double& best_b, uint32_t& id_b) {
    best_b = a.unk_score + 0.0; id_b = a.unk_id;
    uni_edges(a, pool, h, txt, a.marker_node, true, b, we, off, [&](uint32_t id, uint32_t e, double sc) {
        if (e == b) { best_b = sc + 0.0; id_b = id; }
        else uni_relax(n, e, sc + 0.0, id, UNI_FROM_S);
    });
}

// The span of one edge of a word's chosen path, for uni_backtrack (the <write, span> kernels): raw positions are the kernel's positions
// less `shift`; the word's first key byte is at b, its document starts at raw ds with c0 characters in front of it.  An edge from the
// source begins at the space the marker stands for, or -- the virtual marker -- at the document's first character, and covers it whole.
struct UniSpanPut {
    const TextSpanOut& so; uint32_t shift, b, ds, c0, first_end; bool sp;
    __device__ __forceinline__ void operator()(uint64_t slot, uint32_t from, uint32_t e, bool fused) const {
        const uint32_t rs = (from == UNI_FROM_S ? (sp ? b - 1u : b) : from) - shift;
        const uint32_t re = (from == UNI_FROM_S && !sp ? max(e, first_end) : e) - shift;
        ts_store(so, slot, ds, c0, rs, re, fused);
    }
};

template <bool WRITE, bool SPAN = false> __global__ __launch_bounds__(UNI_NT) void k_uni_match(UniArgs a) {
    static_assert(WRITE || !SPAN, "the spans are the write pass's");
    static_assert(UNI_NT == 256 && UNI_TB == 2 * UNI_NT && UNI_S / 16 <= UNI_NT && UNI_S < 0xFFFE, "two positions a lane in phase B; one 16-byte group a lane; wp_block_excl");
    __shared__ __attribute__((aligned(16))) uint8_t s_txt[UNI_S];
    __shared__ uint32_t s_brk[UNI_BW + 1], s_bd[UNI_BW + 1], s_lit[UNI_BW + 1];       // document starts; word bounds; literal U+2581
    __shared__ __attribute__((aligned(16))) UniEdge s_pool[UNI_POOL];
    __shared__ double s_best[UNI_S];
    __shared__ uint32_t s_bid[UNI_S], s_bfrom[UNI_S];
    __shared__ uint16_t s_head[UNI_S], s_headS[UNI_S];       // per start: its edges; the edges of the source in front of it
    __shared__ uint32_t s_tc[UNI_TB], s_pre[UNI_TB];         // per word start: tokens (bit 31: a long word's); tokens in front of a position
    __shared__ uint32_t s_w[4], s_fb, s_te, s_np, s_nl;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint32_t base = tile * (uint32_t)UNI_TB, nv = min((uint32_t)UNI_TB, a.n_bytes - base);
    const uint32_t pend = (uint32_t)UNI_PAD + min(a.n_bytes - base, (uint32_t)UNI_R + 8u);       // the text's end, if the window sees it
    const uint32_t plim = min(pend, (uint32_t)(UNI_PAD + UNI_R));                                // no word of this tile ends behind it
    const uint32_t t0 = UNI_PAD, t1 = UNI_PAD + nv;                                              // the tile proper
    // the window, one 16-byte group a lane: the group in front of the tile, the tile, the halo, one group behind
    if (tid < (uint32_t)UNI_S / 16u) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        const uint64_t raw = (uint64_t)base + 16ull * tid;                                       // (+ UNI_PAD - 16 = 0)
        if ((tile > 0u || tid > 0u) && raw - 16u < a.n_bytes) v = *reinterpret_cast<const uint4*>(a.text + (raw - 16u));
        *reinterpret_cast<uint4*>(s_txt + 16u * tid) = v;
    }
    if (tid <= (uint32_t)UNI_BW) { s_brk[tid] = 0u; s_bd[tid] = 0u; s_lit[tid] = 0u; }
    if (tid == 0u) { s_np = 0u; s_nl = 0u; }
    __syncthreads();
    // document starts inside the window, from three bytes in front of the tile
    const uint32_t back = tile ? 3u : 0u;
    for (uint32_t d = sp_first_doc(a.doc_off, a.n_docs, (uint64_t)base - back) + tid; d < a.n_docs; d += UNI_NT) {
        const uint64_t p = a.doc_off[d];
        if (p + UNI_PAD >= (uint64_t)base + pend) break;
        const uint32_t P = (uint32_t)(p - base) + UNI_PAD;   // (p >= base - 3: the sum does not wrap below 13)
        atomicOr(&s_brk[P >> 5], 1u << (P & 31u));
    }
    __syncthreads();
    auto brk3 = [&](uint32_t P) { return (uni_bit(s_brk, P + 1u) ? 2u : 0u) | (uni_bit(s_brk, P + 2u) ? 4u : 0u) | (uni_bit(s_brk, P + 3u) ? 8u : 0u); };
    // word bounds: a document start, a space, a literal U+2581
    for (uint32_t P = t0 + tid; P < plim; P += UNI_NT) {
        const uint32_t b0 = s_txt[P];
        const bool lit = b0 == 0xE2u && s_txt[P + 1u] == 0x96u && s_txt[P + 2u] == 0x81u && uni_clen(s_txt + P, pend - P, brk3(P)) == 3u;
        if (lit) atomicOr(&s_lit[P >> 5], 1u << (P & 31u));
        if (lit || b0 == 0x20u || uni_bit(s_brk, P)) atomicOr(&s_bd[P >> 5], 1u << (P & 31u));
    }
    __syncthreads();
    // fb: the first word start of the tile (the bytes in front of it belong to a word of an earlier tile); te: where the last word that
    // starts in the tile ends, if the window holds it
    if (tid == 0u) { s_fb = uni_next_bit(s_bd, t0, t1); s_te = uni_next_bit(s_bd, t1, plim); }
    __syncthreads();
    const uint32_t fb = s_fb, te = s_te;
    // ---- phase A: the trie walks, a lane per character start ---------------------------------------------------------------------------
    for (uint32_t P = t0 + tid; P <= plim; P += UNI_NT) {      // (plim itself can be a word's last node)
        s_bfrom[P] = UNI_UNSET;
        uint32_t head = UNI_H_WALK, headS = UNI_H_NONE;
        if (P >= fb && P < te) {
            const uint32_t b0 = s_txt[P];
            const bool bd = uni_bit(s_bd, P), sp = b0 == 0x20u;
            const bool has_vm = bd && (sp || (!uni_bit(s_lit, P) && a.prepend));
            const uint32_t lim = uni_next_bit(s_bd, P + 1u, plim);                  // the word's end: a walk stops there
            auto collect = [&](uint32_t& h) {
                return [&](uint32_t id, uint32_t e, double sc) {
                    const uint32_t k = atomicAdd(&s_np, 1u);
                    if (k >= (uint32_t)UNI_POOL) { h = UNI_H_WALK; return false; }
                    s_pool[k] = UniEdge{sc, id, (uint16_t)e, (uint16_t)h};
                    h = k;
                    return true;
                };
            };
            if (has_vm) uni_walk(a, s_txt, a.marker_node, true, P + (sp ? 1u : 0u), lim, collect(headS));
            const bool start = uni_is_start(s_txt + P, 3u, pend - P, [&](int k) { return uni_bit(s_brk, (uint32_t)((int)P + k)); });
            if (!sp && start) { head = UNI_H_NONE; uni_walk(a, s_txt, 0u, false, P, lim, collect(head)); }
        }
        s_head[P] = (uint16_t)head; s_headS[P] = (uint16_t)headS;
    }
    __syncthreads();
    // ---- phase B: the words, a lane per word start among its two positions -----------------------------------------------------------
    const UniNodes n{s_best, s_bid, s_bfrom};
    auto word = [&](uint32_t P, uint32_t& b, uint32_t& we, bool& has_vm, uint32_t& id_b) {      // false: a long word
        const bool sp = s_txt[P] == 0x20u;
        has_vm = sp || (!uni_bit(s_lit, P) && a.prepend);
        b = P + (sp ? 1u : 0u);
        const uint32_t to = min(P + (uint32_t)UNI_H + 1u, pend);
        we = uni_next_bit(s_bd, P + 1u, to);
        if (we == to && to != pend) return false;
        double best_b = 0.0;
        id_b = 0u;
        if (has_vm) uni_step_source(a, n, s_pool, s_headS[P], s_txt, b, we, 0u, best_b, id_b);
        for (uint32_t s = b; s < we; s += uni_clen(s_txt + s, we - s, 0u))
            uni_step(a, n, s_pool, s_head[s], s_txt, s, we, 0u, s == b ? best_b : s_best[s]);
        return true;
    };
    uint32_t mine = 0u;
    for (uint32_t P = t0 + 2u * tid; P < min(t0 + 2u * tid + 2u, t1); P++) {
        uint32_t tc = 0u;
        if (uni_bit(s_bd, P)) {
            uint32_t b, we, id_b; bool has_vm;
            if (word(P, b, we, has_vm, id_b)) tc = uni_backtrack<false>(n, b, we, has_vm, id_b, a.unk_id, nullptr, 0ull, 0ull);
            else if constexpr (!WRITE) {                     // log it: k_uni_long<count> adds its tokens to this tile's
                const uint32_t k = atomicAdd(&s_nl, 1u);
                if (k < (uint32_t)UNI_LREC) a.lr_start[tile * (uint32_t)UNI_LREC + k] = base + (P - t0);
            } else {
                for (uint32_t k = 0; k < min(a.lr_n[tile], (uint32_t)UNI_LREC); k++)
                    if (a.lr_start[tile * (uint32_t)UNI_LREC + k] == base + (P - t0)) tc = 0x80000000u | (k << 28) | a.lr_cnt[tile * (uint32_t)UNI_LREC + k];
            }
        }
        s_tc[P - t0] = tc;
        mine += tc & 0x0FFFFFFFu;
    }
    uint32_t total;
    uint32_t pre = wp_block_excl(mine, s_w, total);
    if constexpr (!WRITE) { if (tid == 0u) { a.cnt[tile] = total; a.lr_n[tile] = min(s_nl, (uint32_t)UNI_LREC); } }
    else {
        const uint64_t tb = a.cnt[tile];
        for (uint32_t P = t0 + 2u * tid; P < min(t0 + 2u * tid + 2u, t1); P++) {
            s_pre[P - t0] = pre;
            const uint32_t tc = s_tc[P - t0], nt = tc & 0x0FFFFFFFu;
            if (tc & 0x80000000u) a.lr_slot[tile * (uint32_t)UNI_LREC + ((tc >> 28) & 7u)] = tb + pre;      // k_uni_long<write> fills them
            else if (nt) {                                   // (the nodes of this word are as the count left them: no other word shares them)
                uint32_t b, we, id_b; bool has_vm;
                const bool sp = s_txt[P] == 0x20u;
                has_vm = sp || (!uni_bit(s_lit, P) && a.prepend);
                b = P + (sp ? 1u : 0u);
                we = uni_next_bit(s_bd, P + 1u, min(P + (uint32_t)UNI_H + 1u, pend));
                id_b = a.unk_id;
                if (has_vm) {                                // node b again: the marker's own key, if there is one
                    const uint32_t mid = a.marker_node != WP_NONE ? a.trie.node_id[a.marker_node] : WP_NONE;
                    if (mid != WP_NONE) id_b = mid;
                }
                if constexpr (SPAN) {
                    const uint32_t shift = (uint32_t)UNI_PAD - base;           // (modulo 2^32: raw = P - UNI_PAD + base)
                    const uint32_t ds = ts_doc_start(a.so, a.n_docs, P - shift);
                    (void)uni_backtrack<true>(n, b, we, has_vm, id_b, a.unk_id, a.ids, tb + pre + nt - 1u, a.ids_cap,
                                              UniSpanPut{a.so, shift, b, ds, ts_doc_chars(a.so, ds), b + uni_clen(s_txt + b, we - b, 0u), sp});
                } else
                (void)uni_backtrack<true>(n, b, we, has_vm, id_b, a.unk_id, a.ids, tb + pre + nt - 1u, a.ids_cap);
            }
            pre += nt;
        }
        __syncthreads();
        // a document begins at the rank of its first word; the last tile closes the table
        for (uint32_t d = sp_first_doc(a.doc_off, a.n_docs, base) + tid; d < a.n_docs; d += UNI_NT) {
            const uint64_t p = a.doc_off[d];
            if (p >= (uint64_t)base + nv) break;
            a.out_off[d] = tb + s_pre[(uint32_t)(p - base)];
        }
        if (tile == gridDim.x - 1u) {
            const uint64_t all = a.cnt[gridDim.x];
            for (uint32_t d = sp_first_doc(a.doc_off, a.n_docs, a.n_bytes) + tid; d <= a.n_docs; d += UNI_NT) a.out_off[d] = all;
        }
    }
}

// ---- long words ----------------------------------------------------------------------------------------------------------------------
template <bool WRITE, bool SPAN = false> __global__ __launch_bounds__(UNI_LB) void k_uni_long(UniArgs a, uint32_t ntiles) {
    static_assert(WRITE || !SPAN, "the spans are the write pass's");
    static_assert(UNI_LB == 64, "one wavefront: the ballot covers a block");
    __shared__ __attribute__((aligned(16))) UniEdge s_pool[UNI_LPOOL];
    __shared__ uint16_t s_head[UNI_LB];
    __shared__ uint32_t s_np;
    const uint32_t lane = threadIdx.x;
    for (uint32_t r = blockIdx.x; r < ntiles * (uint32_t)UNI_LREC; r += gridDim.x) {
        const uint32_t tile = r / (uint32_t)UNI_LREC;
        if (r % (uint32_t)UNI_LREC >= a.lr_n[tile]) continue;
        const uint32_t s0 = a.lr_start[r];
        // the word: its document's end, its kind, its end
        const uint32_t dn = sp_first_doc(a.doc_off, a.n_docs, (uint64_t)s0 + 1u);
        const uint32_t de = dn < a.n_docs ? (uint32_t)min(a.doc_off[dn], (uint64_t)a.n_bytes) : a.n_bytes;
        auto lit_at = [&](uint32_t q) { return q + 3u <= de && a.text[q] == 0xE2u && a.text[q + 1u] == 0x96u && a.text[q + 2u] == 0x81u; };
        const bool sp = a.text[s0] == 0x20u, has_vm = sp || (!lit_at(s0) && a.prepend);
        const uint32_t b = s0 + (sp ? 1u : 0u);
        uint32_t we = de;
        for (uint32_t q0 = s0 + 1u; q0 < de; q0 += UNI_LB) {
            const uint32_t q = q0 + lane;
            const uint64_t m = __ballot(q < de && (a.text[q] == 0x20u || lit_at(q)));
            if (m) { we = q0 + (uint32_t)__ffsll((long long)m) - 1u; break; }
        }
        uint32_t id_b = a.unk_id;
        if (has_vm && a.marker_node != WP_NONE) { const uint32_t mid = a.trie.node_id[a.marker_node]; if (mid != WP_NONE) id_b = mid; }
        if constexpr (!WRITE) {
            for (uint32_t q = b + 1u + lane; q <= we; q += UNI_LB) a.g.bfrom[q] = UNI_UNSET;
            __syncthreads();
            double best_b = 0.0;
            if (lane == 0u && has_vm) { uint32_t idb; uni_step_source(a, a.g, s_pool, UNI_H_WALK, a.text, b, we, 0u, best_b, idb); }
            uint32_t s = b;                                  // lane 0: the next character start (a character can straddle two blocks)
            for (uint32_t blk = b; blk < we; blk += UNI_LB) {
                if (lane == 0u) s_np = 0u;
                __syncthreads();
                // the lanes walk: a lane per start of the block, its edges into the pool with ends relative to the block
                const uint32_t q = blk + lane;
                uint32_t head = UNI_H_WALK;
                if (q < we && a.text[q] != 0x20u && uni_is_start(a.text + q, min(q - b, 3u), we - q, [](int) { return false; })) {
                    head = UNI_H_NONE;
                    uni_walk(a, a.text, 0u, false, q, we, [&](uint32_t id, uint32_t e, double sc) {
                        const uint32_t k = atomicAdd(&s_np, 1u);
                        if (k >= (uint32_t)UNI_LPOOL) { head = UNI_H_WALK; return false; }
                        s_pool[k] = UniEdge{sc, id, (uint16_t)(e - blk), (uint16_t)head};
                        head = k;
                        return true;
                    });
                }
                s_head[lane] = (uint16_t)head;
                __syncthreads();
                // lane 0 relaxes the block in order
                if (lane == 0u)
                    for (; s < min(blk + (uint32_t)UNI_LB, we); s += uni_clen(a.text + s, we - s, 0u))
                        uni_step(a, a.g, s_pool, s_head[s - blk], a.text, s, we, blk, s == b ? best_b : a.g.best[s]);
                __syncthreads();
            }
            if (lane == 0u) {
                const uint32_t cnt = uni_backtrack<false>(a.g, b, we, has_vm, id_b, a.unk_id, nullptr, 0ull, 0ull);
                a.lr_cnt[r] = cnt;
                atomicAdd(reinterpret_cast<unsigned long long*>(&a.cnt[tile]), (unsigned long long)cnt);
            }
        } else if (lane == 0u) {
            const uint32_t cnt = a.lr_cnt[r];
            if constexpr (SPAN) {
                const uint32_t ds = ts_doc_start(a.so, a.n_docs, s0);
                if (cnt) (void)uni_backtrack<true>(a.g, b, we, has_vm, id_b, a.unk_id, a.ids, a.lr_slot[r] + cnt - 1u, a.ids_cap,
                                                   UniSpanPut{a.so, 0u, b, ds, ts_doc_chars(a.so, ds), b + uni_clen(a.text + b, we - b, 0u), sp});
            } else
            if (cnt) (void)uni_backtrack<true>(a.g, b, we, has_vm, id_b, a.unk_id, a.ids, a.lr_slot[r] + cnt - 1u, a.ids_cap);
        }
        __syncthreads();
    }
}
#endif  // __HIPCC__

}  // namespace spl
