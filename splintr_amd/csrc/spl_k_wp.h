// spl_k_wp.h -- part of spl_kernels.hip (included there, in this order; one translation unit): WordPiece mode (k_wp_norm<count>,
// k_wp_norm<write>, k_wp_match<count>, k_wp_match<write>), an encode path of its own beside the tile kernel.
//
// The mode is Hugging Face's BertNormalizer -> BertPreTokenizer -> WordPiece restated per code point: every input code
// point becomes up to three output code points, each PLAIN, ISOLATED (a word by itself) or SPACE; a word is a maximal run of PLAIN
// characters or one ISOLATED character; a word is matched greedily, longest key first, against word-initial keys and continuation keys.
//
// k_wp_norm: a workgroup of WPN_NT lanes owns WPN_TB input bytes, 16 a lane.  A lane decodes the characters whose LEAD byte it holds (a
// character that straddles two tiles belongs to the tile of its lead byte; three bytes behind the tile are staged), looks each up in the
// two-stage table and knows its bytes out.  What a lane cannot know alone is whether its first character starts a word: that is the state
// in front of it -- BOUND (a space, an ISOLATED character or a document start came last) or PLAIN --, a scan over (NONE | BOUND | PLAIN)
// with "the right operand unless it is NONE".  The count pass leaves the tile's bytes out and the state it ends in; k_decode_scan turns
// the bytes into bases; the write pass -- the same body -- takes the state in front of the tile from the tiles before it (one step back
// unless a whole tile emitted nothing), assembles the normalised bytes and the word-start bits in LDS, congruent to their place in HBM
// modulo 16 bytes / 32 bits, and stores them by aligned 16-byte / 4-byte stores.  No workgroup waits for another.
//
// k_wp_match: a workgroup of WPM_NT lanes owns WPM_TB bytes of normalised text plus a halo of 4 * max_word_chars + 4 bytes: a word of
// more than max_word_chars characters is unk whatever follows, so the halo decides every word that STARTS in the tile.  The vocabulary is
// a trie -- one root for word-initial keys, one for continuation keys, the prefix folded in on the host -- stored as an open-addressing
// hash of (node, byte) -> child and an array node -> id.  A lane per character start walks the trie from its position to the word's end
// and leaves the LAST node that carried an id as (length, id) in LDS.  Then a lane per word start follows next = pos + length: words of
// real text are a few characters and one to three pieces long, so the chain is shorter than the log2(tile) rounds pointer doubling would
// spend on every byte.  Only positions the chain REACHES can turn the word into unk.  Counts go through a workgroup scan; the count pass
// leaves the tile's tokens, k_decode_scan the bases, the write pass stores ids and the documents' offsets.  No atomics on the result.
#pragma once
#include "spl_common.h"
#include "spl_k_textspans.h"

namespace spl {

constexpr int WPN_TB = 4096, WPN_NT = WPN_TB / 16;          // the normaliser's tile
constexpr int WPM_TB = 2048, WPM_NT = 256;                  // the matcher's tile
constexpr int WP_MAX_WORD_CHARS = 255;                      // spl_opts.max_word_chars at most
constexpr int WPM_HALO_MAX = 4 * WP_MAX_WORD_CHARS + 4, WPM_R = WPM_TB + WPM_HALO_MAX;
constexpr uint64_t WP_MAX_BYTES = 64ull << 20;              // one device call (the normalised text is up to three times as long)
constexpr uint32_t WP_NONE = 0xFFFFFFFFu;
enum : uint32_t { WPS_NONE = 0, WPS_BOUND = 1, WPS_PLAIN = 2 };

// The normalisation table (splintr_amd/wordpiece.py build_norm_table; checked entry by entry at spl_create).
struct WpNormTab { const uint16_t* s1; const uint32_t* s2; const uint32_t* multi; uint32_t shift; };
struct WpNormArgs {
    const uint8_t* text; uint32_t n_bytes;
    const uint64_t* doc_off; uint32_t n_docs;
    WpNormTab tab;
    uint64_t* cnt;                       // [tiles + 1]: bytes out per tile (count pass); exclusive sums and the total (k_decode_scan)
    uint8_t* tstate;                     // [tiles]: the state a tile ends in (count pass)
    uint8_t* out; uint32_t* starts;      // write pass: the normalised text; word-start bits over it (zero-filled by the host)
    uint64_t* out_doc_off;               // [n_docs + 1]
    uint32_t* map;                       // k_wp_norm<write, map> only: per normalised character start, its source (wp_map_entry)
};
// The trie.  edges: {node << 8 | byte, child}, key WP_NONE for an empty slot; a probe ends at the key, an empty slot or max_probe steps.
struct WpTrie { const uint2* edges; uint32_t mask, hshift, max_probe; const uint32_t* node_id; };
struct WpMatchArgs {
    const uint8_t* text; uint32_t n_bytes;                   // the NORMALISED text
    const uint32_t* starts; const uint64_t* doc_off; uint32_t n_docs;
    WpTrie trie; uint32_t unk_id, max_chars, halo;
    uint64_t* cnt;                       // [tiles + 1]: tokens per tile; exclusive sums and the total
    uint32_t* ids; uint64_t ids_cap; uint64_t* out_off;
    const uint32_t* map; TextSpanOut so; // k_wp_match<write, span> only: the normaliser's source map; where the spans go
};
// The source map: the input character a normalised character came from, as the offset of its lead byte in the caller's text (26 bits:
// WP_MAX_BYTES) and its length in bytes above them.  All outputs of one input share it; a position that starts no character holds 0.
SPL_HD uint32_t wp_map_entry(uint32_t off, uint32_t len) { return off | len << 26; }
SPL_HD uint32_t wp_map_off(uint32_t e) { return e & 0x3FFFFFFu; }
SPL_HD uint32_t wp_map_end(uint32_t e) { return (e & 0x3FFFFFFu) + (e >> 26); }

// One well-formed UTF-8 character at p[0 .. avail): its length and code point; 0 for a byte that starts none (it is dropped).  brk: bit k
// set if a document starts at p + k -- a character does not reach across a document boundary.
SPL_HD uint32_t wp_decode(const uint8_t* p, uint32_t avail, uint32_t brk, uint32_t& cp) {
    const uint32_t b = p[0];
    if (b < 0x80u) { cp = b; return 1u; }
    if (b < 0xC2u || b > 0xF4u) return 0u;
    const uint32_t len = b < 0xE0u ? 2u : b < 0xF0u ? 3u : 4u;
    if (len > avail || (brk & ((1u << len) - 2u))) return 0u;
    const uint32_t c1 = p[1];
    const uint32_t lo = b == 0xE0u ? 0xA0u : b == 0xF0u ? 0x90u : 0x80u, hi = b == 0xEDu ? 0x9Fu : b == 0xF4u ? 0x8Fu : 0xBFu;
    if (c1 < lo || c1 > hi) return 0u;
    cp = (b & (0xFFu >> (len + 1u))) << 6 | (c1 & 0x3Fu);
    for (uint32_t i = 2; i < len; i++) {
        if ((p[i] & 0xC0u) != 0x80u) return 0u;
        cp = cp << 6 | (p[i] & 0x3Fu);
    }
    return len;
}
SPL_HD uint32_t wp_utf8_len(uint32_t cp) { return cp < 0x80u ? 1u : cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u; }
SPL_HD void wp_utf8_put(uint8_t* o, uint32_t cp) {
    if (cp < 0x80u) { o[0] = (uint8_t)cp; }
    else if (cp < 0x800u) { o[0] = (uint8_t)(0xC0u | cp >> 6); o[1] = (uint8_t)(0x80u | (cp & 0x3Fu)); }
    else if (cp < 0x10000u) { o[0] = (uint8_t)(0xE0u | cp >> 12); o[1] = (uint8_t)(0x80u | (cp >> 6 & 0x3Fu)); o[2] = (uint8_t)(0x80u | (cp & 0x3Fu)); }
    else { o[0] = (uint8_t)(0xF0u | cp >> 18); o[1] = (uint8_t)(0x80u | (cp >> 12 & 0x3Fu)); o[2] = (uint8_t)(0x80u | (cp >> 6 & 0x3Fu)); o[3] = (uint8_t)(0x80u | (cp & 0x3Fu)); }
}
// Output k of code point cp under table entry e: the code point, bit 21 ISOLATED, bit 22 SPACE.
SPL_HD uint32_t wp_norm_out(const WpNormTab& t, uint32_t e, uint32_t cp, uint32_t k) {
    if ((e & 3u) >= 2u) return t.multi[(e >> 8) + k];
    return (e & 8u) ? (0x20u | 1u << 22) : (((cp + (e >> 8)) & 0x1FFFFFu) | ((e & 4u) << 19));
}
SPL_HD uint32_t wp_norm_entry(const WpNormTab& t, uint32_t cp) {
    return t.s2[((uint32_t)t.s1[cp >> t.shift] << t.shift) | (cp & ((1u << t.shift) - 1u))];
}
SPL_HD bool wp_bit(const uint32_t* m, uint32_t p) { return (m[p >> 5] >> (p & 31u)) & 1u; }

#if defined(__HIPCC__)
// Exclusive sum of x over the workgroup's 256 lanes (s_w: 4 words; total: the sum).  Two barriers.
__device__ __forceinline__ uint32_t wp_block_excl(uint32_t x, uint32_t* s_w, uint32_t& total) {
    const uint32_t incl = wave_scan_incl(x);
    __syncthreads();
    if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t pre = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) pre += s_w[w];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return pre + incl - x;
}

// ---- the normaliser -----------------------------------------------------------------------------------------------------------------
constexpr int WPN_OUT = 3 * WPN_TB + 32;                    // staged output bytes (+ up to 15 in front, the last 16-byte group's rest behind)
constexpr int WPN_OBW = (3 * WPN_TB + 31) / 32 + 2;         // words of the staged word-start bitmap

// One lane's bytes [l0, l1) of the tile: the bytes they emit and the state behind them, from state st in front.  WRITE: the bytes go to
// s_out + o, the word-start bits to s_sb at bit bb + o, the output position of every document start to s_opos.  MAP: s_map + o takes the
// source of every character written, as its position in the tile (12 bits) and its length above them.
template <bool WRITE, bool MAP = false> __device__ __forceinline__ uint32_t wp_norm_lane(const WpNormTab& tab, const uint8_t* s_in, const uint32_t* s_brk, uint32_t l0,
                                                                       uint32_t l1, uint32_t avail, uint32_t& st, uint8_t* s_out, uint32_t o,
                                                                       uint32_t* s_sb, uint32_t bb, uint16_t* s_opos, uint16_t* s_map = nullptr) {
    const uint32_t o0 = o;
    for (uint32_t li = l0; li < l1; li++) {
        if (wp_bit(s_brk, li)) { st = WPS_BOUND; if (WRITE) s_opos[li] = (uint16_t)o; }
        const uint32_t brk = (wp_bit(s_brk, li + 1u) ? 2u : 0u) | (wp_bit(s_brk, li + 2u) ? 4u : 0u) | (wp_bit(s_brk, li + 3u) ? 8u : 0u);
        uint32_t cp = 0;
        const uint32_t slen = wp_decode(s_in + li, avail - li, brk, cp);
        if (!slen) continue;
        const uint32_t e = wp_norm_entry(tab, cp), n = e & 3u;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t v = wp_norm_out(tab, e, cp, k), oc = v & 0x1FFFFFu, len = wp_utf8_len(oc);
            const bool space = (v >> 22) & 1u, iso = (v >> 21) & 1u;
            if (WRITE) {
                if (!space && (iso || st != WPS_PLAIN)) atomicOr(&s_sb[(bb + o) >> 5], 1u << ((bb + o) & 31u));
                wp_utf8_put(s_out + o, oc);
                if constexpr (MAP) s_map[o] = (uint16_t)(li | slen << 12);
            }
            st = (space || iso) ? WPS_BOUND : WPS_PLAIN;
            o += len;
        }
    }
    return o - o0;
}

template <bool WRITE, bool MAP = false> __global__ __launch_bounds__(WPN_NT) void k_wp_norm(WpNormArgs a) {
    static_assert(WRITE || !MAP, "the map is the write pass's");
    static_assert(WPN_TB <= 4096, "a source's position in the tile is 12 bits of the staged map");
    static_assert(WPN_NT == 256, "wp_block_excl and the state scan are written for four wavefronts");
    __shared__ __attribute__((aligned(16))) uint8_t s_in[WPN_TB + 16];
    __shared__ uint32_t s_brk[WPN_TB / 32 + 2];
    __shared__ uint32_t s_w[4], s_ws[4], s_tin;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint32_t base = tile * (uint32_t)WPN_TB, nv = min((uint32_t)WPN_TB, a.n_bytes - base);
    const uint32_t avail = min(a.n_bytes - base, (uint32_t)WPN_TB + 3u);        // what a character of this tile may read
    // the tile's bytes, 16 a lane in one load (the text is 16-byte aligned and readable to the next multiple of 16), three bytes behind it
    if (16u * tid < nv) *reinterpret_cast<uint4*>(s_in + 16u * tid) = *reinterpret_cast<const uint4*>(a.text + base + 16u * tid);
    if (tid < 3u && (uint32_t)WPN_TB + tid < avail) s_in[WPN_TB + tid] = a.text[base + WPN_TB + tid];
    if (tid < (uint32_t)WPN_TB / 32u + 2u) s_brk[tid] = 0u;
    if (tid == 0u) s_tin = WPS_BOUND;
    __syncthreads();
    // document starts inside the tile and its three bytes behind
    const uint32_t d0 = sp_first_doc(a.doc_off, a.n_docs, base);
    for (uint32_t d = d0 + tid; d < a.n_docs; d += WPN_NT) {
        const uint64_t p = a.doc_off[d];
        if (p >= (uint64_t)base + avail) break;
        atomicOr(&s_brk[(uint32_t)(p - base) >> 5], 1u << ((uint32_t)(p - base) & 31u));
    }
    if (WRITE && tid == 0u)                                    // the state in front of the tile: the last tile before it that ends in one
        for (uint32_t t = tile; t-- > 0u;) { const uint32_t s = a.tstate[t]; if (s != WPS_NONE) { s_tin = s; break; } }
    __syncthreads();
    const uint32_t l0 = 16u * tid, l1 = min(l0 + 16u, nv);
    uint32_t st = WPS_NONE;
    const uint32_t mine = l0 < nv ? wp_norm_lane<false>(a.tab, s_in, s_brk, l0, l1, avail, st, nullptr, 0u, nullptr, 0u, nullptr) : 0u;
    uint32_t total;
    const uint32_t o_lane = wp_block_excl(mine, s_w, total);
    // the state behind every lane: an inclusive scan of "the right operand unless it is NONE" -- the wavefront, then the four wavefronts
    uint32_t si = st;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t s2 = (uint32_t)__shfl_up((int)si, d); if ((int)(tid & 63u) >= d && si == WPS_NONE) si = s2; }
    if ((tid & 63u) == 63u) s_ws[tid >> 6] = si;
    __syncthreads();
    if constexpr (!WRITE) {
        if (tid == 0u) {
            uint32_t s = WPS_NONE;
            for (int w = 0; w < 4; w++) if (s_ws[w] != WPS_NONE) s = s_ws[w];
            a.cnt[tile] = total; a.tstate[tile] = (uint8_t)s;
        }
    } else {
        __shared__ __attribute__((aligned(16))) uint8_t s_out[WPN_OUT];
        __shared__ uint32_t s_sb[WPN_OBW];
        __shared__ uint16_t s_opos[WPN_TB];
        for (uint32_t i = tid; i < (uint32_t)WPN_OBW; i += WPN_NT) s_sb[i] = 0u;
        // the state in front of this lane: the lane before it in the wavefront, else the wavefronts before, else the tile's
        uint32_t sin = (uint32_t)__shfl_up((int)si, 1);
        if ((tid & 63u) == 0u) sin = WPS_NONE;
        for (uint32_t w = tid >> 6; sin == WPS_NONE && w-- > 0u;) sin = s_ws[w];
        if (sin == WPS_NONE) sin = s_tin;
        const uint64_t obase = a.cnt[tile];
        const uint32_t ba = (uint32_t)(obase & 15u), bb = (uint32_t)(obase & 31u);
        __syncthreads();
        if constexpr (MAP) {
            // the source map, staged beside the bytes at the same place modulo 16 and stored as they are: four entries -- 16 bytes -- a
            // group, whole groups by one store, the groups the tile shares with its neighbours entry by entry
            __shared__ uint16_t s_map[WPN_OUT];
            if (l0 < nv) (void)wp_norm_lane<true, true>(a.tab, s_in, s_brk, l0, l1, avail, sin, s_out + ba, o_lane, s_sb, bb, s_opos, s_map + ba);
            __syncthreads();
            uint32_t* const m4 = a.map + (obase - ba);
            for (uint32_t j = tid; j * 4u < ba + total; j += WPN_NT) {
                const uint32_t lo = j * 4u;
                uint32_t v[4];
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t q = lo + k;
                    const bool cs = q >= ba && q < ba + total && (s_out[q] & 0xC0u) != 0x80u;
                    v[k] = cs ? wp_map_entry(base + (s_map[q] & 0xFFFu), (uint32_t)s_map[q] >> 12) : 0u;
                }
                if (lo >= ba && lo + 4u <= ba + total) *reinterpret_cast<uint4*>(m4 + lo) = make_uint4(v[0], v[1], v[2], v[3]);
                else for (uint32_t k = 0; k < 4u; k++) if (lo + k >= ba && lo + k < ba + total) m4[lo + k] = v[k];
            }
        } else {
            if (l0 < nv) (void)wp_norm_lane<true>(a.tab, s_in, s_brk, l0, l1, avail, sin, s_out + ba, o_lane, s_sb, bb, s_opos);
            __syncthreads();
        }
        // the documents' offsets in the normalised text; the last tile also closes the table (documents that start at the text's end)
        for (uint32_t d = d0 + tid; d < a.n_docs; d += WPN_NT) {
            const uint64_t p = a.doc_off[d];
            if (p >= (uint64_t)base + nv) break;
            a.out_doc_off[d] = obase + s_opos[(uint32_t)(p - base)];
        }
        if (tile == gridDim.x - 1u) {
            const uint64_t all = a.cnt[gridDim.x];
            for (uint32_t d = sp_first_doc(a.doc_off, a.n_docs, a.n_bytes) + tid; d <= a.n_docs; d += WPN_NT) a.out_doc_off[d] = all;
        }
        // the bytes: whole 16-byte groups by one store; the groups the tile shares with its neighbours byte by byte
        uint8_t* const o16 = a.out + (obase - ba);
        for (uint32_t j = tid; j * 16u < ba + total; j += WPN_NT) {
            const uint32_t lo = j * 16u;
            if (lo >= ba && lo + 16u <= ba + total) *reinterpret_cast<uint4*>(o16 + lo) = *reinterpret_cast<const uint4*>(s_out + lo);
            else for (uint32_t q = max(lo, ba); q < min(lo + 16u, ba + total); q++) o16[q] = s_out[q];
        }
        // the word-start bits: the words the tile has to itself by plain stores, its first and last word -- shared with its neighbours -- by an OR
        const uint32_t nw = (bb + total + 31u) >> 5;
        for (uint32_t j = tid; j < nw; j += WPN_NT) {
            const uint32_t v = s_sb[j];
            if (j == 0u || j == nw - 1u) { if (v) atomicOr(&a.starts[(obase >> 5) + j], v); }
            else a.starts[(obase >> 5) + j] = v;
        }
    }
}

// ---- the matcher --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wp_child(const WpTrie& t, uint32_t node, uint32_t b) {
    const uint32_t key = node << 8 | b;
    uint32_t h = (key * 0x9E3779B1u) >> t.hshift;
    for (uint32_t k = 0; k <= t.max_probe; k++, h++) {
        const uint2 e = t.edges[h & t.mask];
        if (e.x == key) return e.y;
        if (e.x == WP_NONE) break;
    }
    return WP_NONE;
}

template <bool WRITE, bool SPAN = false> __global__ __launch_bounds__(WPM_NT) void k_wp_match(WpMatchArgs a) {
    static_assert(WRITE || !SPAN, "the spans are the write pass's");
    static_assert(WPM_NT == 256 && WPM_TB == 8 * WPM_NT, "eight positions a lane in the chain phase; wp_block_excl");
    __shared__ __attribute__((aligned(16))) uint8_t s_txt[WPM_R + 16];
    __shared__ uint32_t s_st[WPM_R / 32 + 2];
    __shared__ uint32_t s_li[WPM_R];                         // per character start: length of the longest key from here << 24 | its id
    __shared__ uint16_t s_tc[WPM_TB], s_pre[WPM_TB];         // per word start: tokens | 0x8000 for unk; tokens in front of a position
    __shared__ uint32_t s_w[4], s_fb, s_te;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint32_t base = tile * (uint32_t)WPM_TB, nv = min((uint32_t)WPM_TB, a.n_bytes - base);
    const uint32_t nvr = min((uint32_t)WPM_TB + a.halo, a.n_bytes - base);      // the tile and its halo
    for (uint32_t j = 16u * tid; j < nvr; j += 16u * WPM_NT) *reinterpret_cast<uint4*>(s_txt + j) = *reinterpret_cast<const uint4*>(a.text + base + j);
    for (uint32_t j = tid; j < (nvr + 31u) / 32u + 1u; j += WPM_NT) s_st[j] = a.starts[(base >> 5) + j];
    __syncthreads();
    auto is_b = [&](uint32_t p) { return s_txt[p] == 0x20u || wp_bit(s_st, p); };      // a word ends in front of p
    // fb: the first boundary of the tile (the bytes in front of it continue a word of an earlier tile: that tile's halo decided it);
    // te: the first boundary at or behind the tile's end (where the last word that starts in the tile ends, if the halo holds it)
    if (tid < 128u) {
        const uint32_t lane = tid & 63u, from = tid < 64u ? 0u : (uint32_t)WPM_TB, to = tid < 64u ? nv : nvr;
        uint32_t r = to;
        for (uint32_t p0 = from; p0 < to; p0 += 64u) {
            const uint64_t m = __ballot(p0 + lane < to && is_b(p0 + lane));
            if (m) { r = p0 + (uint32_t)__ffsll((long long)m) - 1u; break; }
        }
        if (lane == 0u) { if (tid < 64u) s_fb = r; else s_te = max(r, nv); }
    }
    __syncthreads();
    const uint32_t fb = s_fb, te = s_te;
    // the trie walks: a lane per character start, from the word-initial root at a word start and the continuation root elsewhere
    for (uint32_t p = tid; p < te; p += WPM_NT) {
        uint32_t best = 0u;
        const uint32_t b0 = s_txt[p];
        if (p >= fb && b0 != 0x20u && (b0 & 0xC0u) != 0x80u) {
            uint32_t node = wp_bit(s_st, p) ? 0u : 1u, j = p;
            while (j < nvr && j - p < 255u && !(j > p && is_b(j))) {
                node = wp_child(a.trie, node, s_txt[j]);
                if (node == WP_NONE) break;
                j++;
                const uint32_t id = a.trie.node_id[node];
                if (id != WP_NONE && (j >= nvr || (s_txt[j] & 0xC0u) != 0x80u)) best = (j - p) << 24 | id;
            }
        }
        s_li[p] = best;
    }
    __syncthreads();
    // the words: a lane per word start among its eight positions
    uint32_t mine = 0u;
    for (uint32_t p = 8u * tid; p < min(8u * tid + 8u, nv); p++) {
        uint32_t tc = 0u;
        if (wp_bit(s_st, p)) {
            uint32_t q = p, nch = 0u;
            while (q < nvr && !(q > p && is_b(q)) && nch <= a.max_chars) { nch += (s_txt[q] & 0xC0u) != 0x80u ? 1u : 0u; q++; }
            if (nch > a.max_chars) tc = 0x8001u;
            else {
                const uint32_t we = q;
                uint32_t n = 0u;
                for (q = p; q < we; n++) { const uint32_t l = s_li[q] >> 24; if (!l) break; q += l; }
                tc = q < we ? 0x8001u : n;                   // a position the chain reaches has no key: the whole word is unk
            }
        }
        s_tc[p] = (uint16_t)tc;
        mine += tc & 0x7FFFu;
    }
    uint32_t total;
    uint32_t pre = wp_block_excl(mine, s_w, total);
    if constexpr (!WRITE) { if (tid == 0u) a.cnt[tile] = total; }
    else {
        const uint64_t tb = a.cnt[tile];
        for (uint32_t p = 8u * tid; p < min(8u * tid + 8u, nv); p++) {
            s_pre[p] = (uint16_t)pre;
            const uint32_t tc = s_tc[p];
            uint64_t at = tb + pre;
            if (tc & 0x8000u) { if (at < a.ids_cap) a.ids[at] = a.unk_id; }
            else for (uint32_t q = p, k = 0; k < tc; k++, at++) { const uint32_t li = s_li[q]; if (at < a.ids_cap) a.ids[at] = li & 0xFFFFFFu; q += li >> 24; }
            if constexpr (SPAN) {
                // a piece spans from the source of its first character to the end of the source of its last, an unk word from its first
                // character's to its last's: that word may end beyond the halo, so its end is looked for in the text itself
                at = tb + pre;
                if (tc && at < a.ids_cap) {
                    auto byte_at = [&](uint32_t g) { return g < nvr ? (uint32_t)s_txt[g] : (uint32_t)a.text[base + g]; };
                    auto last_char = [&](uint32_t e) { uint32_t l = e - 1u; while ((byte_at(l) & 0xC0u) == 0x80u) l--; return a.map[base + l]; };
                    const uint32_t m0 = a.map[base + p], ds = ts_doc_start(a.so, a.n_docs, wp_map_off(m0)), c0 = ts_doc_chars(a.so, ds);
                    if (tc & 0x8000u) {
                        uint32_t we = p + 1u;
                        while (base + we < a.n_bytes && !(we < nvr ? is_b(we) : (a.text[base + we] == 0x20u || wp_bit(a.starts, base + we)))) we++;
                        ts_store(a.so, at, ds, c0, wp_map_off(m0), wp_map_end(last_char(we)), false);
                    } else for (uint32_t q = p, k = 0; k < tc && at < a.ids_cap; k++, at++) {
                        const uint32_t l = s_li[q] >> 24;
                        ts_store(a.so, at, ds, c0, wp_map_off(a.map[base + q]), wp_map_end(last_char(q + l)), false);
                        q += l;
                    }
                }
            }
            pre += tc & 0x7FFFu;
        }
        __syncthreads();
        // a document begins at the rank of its first word; the last tile closes the table
        for (uint32_t d = sp_first_doc(a.doc_off, a.n_docs, base) + tid; d < a.n_docs; d += WPM_NT) {
            const uint64_t p = a.doc_off[d];
            if (p >= (uint64_t)base + nv) break;
            a.out_off[d] = tb + s_pre[(uint32_t)(p - base)];
        }
        if (tile == gridDim.x - 1u) {
            const uint64_t all = a.cnt[gridDim.x];
            for (uint32_t d = sp_first_doc(a.doc_off, a.n_docs, a.n_bytes) + tid; d <= a.n_docs; d += WPM_NT) a.out_off[d] = all;
        }
    }
}
#endif  // __HIPCC__

}  // namespace spl
