// spl_k_sp.h -- part of spl_kernels.hip (included there, in this order; one translation unit): SentencePiece mode (k_sp_rewrite<count>,
// k_sp_rewrite<write>), in front of the tile kernel.
//
// The reference's SentencePiece loop (src/core/tokenizer.rs:737-795) keeps one counter, pending_underscores, over the chunks of
// [^\s]+|\s+.  Those chunks alternate between whitespace and everything else, so the counter a chunk receives is the number of trailing
// 0x20 bytes of the whitespace chunk in front of it: a local function of the text.  The whole mode is therefore a REWRITE of the corpus --
// every 0x20 of a whitespace run whose first byte is ASCII whitespace becomes E2 96 81 (U+2581) -- plus a bitmap of chunk starts in the
// rewritten text; the merge path takes both as external chunk boundaries (Batch::ext_starts).
//
// A workgroup of SPT_NT lanes owns SPT_TB input bytes, 16 a lane.  Per byte four bits -- ws (the byte belongs to a \s character of the
// handle's class table), sp (0x20), aws (one of 20 09 0A 0C 0D: Rust's is_ascii_whitespace) and brk (a text starts here) -- are kept as
// bit vectors of 64-bit words, one word a lane of the first wavefront.  Whether a whitespace run is ASCII-led travels from the run's first
// byte through the run by an add-carry over the words (sp_word_led) and ONE wavefront scan of generate / propagate across them; a run
// that is already open at the tile's first byte is walked backwards, 64 bytes a ballot, to its first byte.  The count pass leaves the
// tile's number of converted bytes; k_decode_scan turns those into tile bases; the write pass -- the same body -- assembles the tile's
// rewritten bytes and its stretch of every bitmap in LDS, congruent to their place in HBM modulo 16 bytes / 32 bits, and stores them with
// aligned 16-byte / 4-byte stores (the two bitmap words a tile shares with its neighbours: atomicOr).  No workgroup waits for another.
#pragma once
#include "spl_common.h"

namespace spl {

constexpr int SPT_TB = 4096, SPT_NT = SPT_TB / 16;          // the device tile; the host simulation instantiates the functions below for 64 bytes
constexpr int SPT_HALO = 8;                                 // bytes staged on either side of the tile (a character's lead is at most 3 back)
constexpr uint64_t SP_MAX_BYTES = 64ull << 20;              // one device call: three times this stays below the chunks path's 256 MB

// What the rewrite reads.  tstart / tbits / skip: the special-token scan's bitmaps over THIS text (null: no SPL_WITH_SPECIAL).
struct SpText {
    const uint8_t* text; uint32_t n_bytes;
    const uint64_t* doc_off; uint32_t n_docs;
    const uint16_t* ucls1; const uint8_t* ucls2; uint32_t shift;
    const uint32_t* tstart; const uint32_t* tbits; const uint32_t* skip;
};
struct SpArgs {
    SpText t;
    uint64_t* cnt;                       // [tiles + 1]: converted bytes per tile (count pass); exclusive sums and the total (k_decode_scan)
    uint8_t* out; uint32_t* starts;      // write pass: the rewritten text; chunk-start bits over it (both zero-filled by the host)
    uint64_t* out_doc_off;               // [n_docs + 1]
    uint32_t* o_tstart; uint32_t* o_tbits; uint32_t* o_skip;     // the special scan's bitmaps at the rewritten positions (null: none)
    const uint32_t* stage_in; uint32_t* stage_out;               // ... and the literals' ids (Batch::stage)
};

// A byte of the text by position: from the tile's staged window where it covers the position, else from HBM.
struct SpRd {
    const uint8_t* g; const uint8_t* win; uint32_t w0, wn;
    SPL_HD uint32_t operator()(uint32_t p) const { const uint32_t i = p - w0; return i < wn ? win[i] : g[p]; }
};
SPL_HD bool sp_bit(const uint32_t* m, uint32_t p) { return m && ((m[p >> 5] >> (p & 31)) & 1u); }
SPL_HD bool sp_cp_ws(const SpText& a, uint32_t cp) {
    const uint32_t blk = a.ucls1[cp >> a.shift];
    return (M_S >> a.ucls2[(blk << a.shift) | (cp & ((1u << a.shift) - 1u))]) & 1u;
}
// Does byte p belong to a whitespace character?  The lead byte decides through the class table, continuation bytes inherit; a sequence
// that is not one whole well-formed character is no whitespace (the reference only ever sees a str).  A special literal's bytes are text
// of their own: never whitespace.
template <class RD> SPL_HD bool sp_byte_ws(const SpText& a, const RD& rd, uint32_t p) {
    const uint32_t b = rd(p);
    if (sp_bit(a.skip, p)) return false;
    if (b == 0x20u) return true;
    if (b < 0x80u) return b < 0x20u && sp_cp_ws(a, b);
    uint32_t q = p, back = 0;
    while ((rd(q) & 0xC0u) == 0x80u && back < 3u && q > 0u) { q--; back++; }
    const uint32_t l = rd(q);
    if (l < 0xC0u) return false;
    const uint32_t want = l < 0xE0u ? 2u : l < 0xF0u ? 3u : 4u;
    if (back >= want || q + want > a.n_bytes) return false;
    uint32_t cp = l & (0xFFu >> (want + 1u));
    for (uint32_t i = 1; i < want; i++) {
        const uint32_t c = rd(q + i);
        if ((c & 0xC0u) != 0x80u) return false;
        cp = (cp << 6) | (c & 0x3Fu);
    }
    return cp < 0x110000u && sp_cp_ws(a, cp);
}
SPL_HD bool sp_is_aws(uint32_t b) { return b == 0x20u || b == 0x09u || b == 0x0Au || b == 0x0Cu || b == 0x0Du; }

// ---- the tile's logic over the bit vectors, a 64-byte word at a time ----------------------------------------------------------------
struct SpWord { uint64_t ws, sp, aws, brk, valid; };
// The four bits of byte p (bit k of the result: ws, sp, aws, brk -- brk from the special scan's bitmaps only; document starts are OR-ed in by the caller)
template <class RD> SPL_HD uint32_t sp_byte_bits(const SpText& a, const RD& rd, uint32_t p) {
    const uint32_t b = rd(p);
    const bool lit = sp_bit(a.skip, p), ws = sp_byte_ws(a, rd, p);
    return (ws ? 1u : 0u) | ((ws && b == 0x20u) ? 2u : 0u) | ((!lit && sp_is_aws(b)) ? 4u : 0u) | ((sp_bit(a.tstart, p) || sp_bit(a.tbits, p)) ? 8u : 0u);
}
// Which whitespace bytes of the word lie in an ASCII-led run.  prev_ws: the byte in front of the word is whitespace; cin: ... and ASCII-led.
// A run starts where whitespace follows something else, or a text starts; it GENERATES the flag if that byte is ASCII whitespace, every
// further byte of the run PROPAGATES it: adding the injected bit to the propagate vector ripples it through the run.  g_out / p_out: the
// word as one generate / propagate pair for the scan across words (g_out computed for cin = 0).
SPL_HD uint64_t sp_word_led(const SpWord& w, uint32_t prev_ws, uint32_t cin, uint32_t& g_out, uint32_t& p_out) {
    const uint64_t wprev = (w.ws << 1) | prev_ws;
    const uint64_t rs = w.ws & (~wprev | w.brk);
    const uint64_t g = rs & w.aws, p = w.ws & ~rs;
    const uint64_t sum0 = p + (((g << 1)) & p), sum = p + (((g << 1) | cin) & p);
    g_out = (uint32_t)((g | (p & ~sum0)) >> 63);
    p_out = p == ~0ull ? 1u : 0u;
    return g | (p & ~sum);
}
SPL_HD uint32_t sp_carry(uint32_t g, uint32_t p, uint32_t cin) { return g | (p & cin); }
// conv: the bytes that become U+2581.  starts: chunk starts -- the first byte of each run of converted spaces; every other byte of an
// ASCII-led run; the first byte of every other run unless a converted space lies directly in front of it; every text start.
// prev_conv: the byte in front of the word is a converted space.  (One device function: a later change can feed it a pattern's bitmaps.)
struct SpOut { uint64_t conv, starts; };
SPL_HD SpOut sp_word_out(const SpWord& w, uint64_t led, uint32_t prev_ws, uint32_t prev_conv) {
    SpOut o;
    o.conv = w.sp & led;
    const uint64_t convprev = (o.conv << 1) | prev_conv, wprev = (w.ws << 1) | prev_ws;
    const uint64_t in_led = w.ws & led, runstart = (w.ws ^ wprev) | w.brk;
    o.starts = ((o.conv & ~convprev) | (in_led & ~w.sp) | (runstart & ~in_led & ~convprev) | w.brk) & w.valid;
    return o;
}
// Where the ASCII-led flag of a run that is open at position `at` (byte at - 1 is whitespace, no text starts at `at`) comes from: the
// backward walk's per-position verdict.  0 go on, 1 the run starts right behind r (r is no whitespace), 2 it starts at r (a text starts there).
template <class RD> SPL_HD uint32_t sp_back_stop(const SpText& a, const RD& rd, uint32_t r, uint32_t doc_start) {
    if (!sp_byte_ws(a, rd, r)) return 1u;
    return (r == doc_start || sp_bit(a.tstart, r) || sp_bit(a.tbits, r)) ? 2u : 0u;
}
// first document that starts at or behind position p (n_docs: none)
SPL_HD uint32_t sp_first_doc(const uint64_t* doc_off, uint32_t n_docs, uint64_t p) {
    uint32_t lo = 0, hi = n_docs;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (doc_off[mid] < p) lo = mid + 1; else hi = mid; }
    return lo;
}
SPL_HD uint64_t sp_low_mask(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

#if defined(__HIPCC__)
// ---- the kernel ---------------------------------------------------------------------------------------------------------------------
constexpr int SPT_W = SPT_TB / 64;                          // 64-bit words of a tile's bit vectors: one a lane of the first wavefront
constexpr int SPT_OUT = 3 * SPT_TB + 32;                    // staged output bytes (+ up to 15 in front, the last 16-byte group's rest behind)
constexpr int SPT_OBW = (3 * SPT_TB + 31) / 32 + 2;         // words of a staged output bitmap

template <bool WRITE> __global__ __launch_bounds__(SPT_NT) void k_sp_rewrite(SpArgs a) {
    static_assert(SPT_W == 64 && SPT_NT == 256, "one word a lane of one wavefront; four lanes a word");
    __shared__ __attribute__((aligned(16))) uint8_t s_in[SPT_HALO + SPT_TB + SPT_HALO];
    __shared__ __attribute__((aligned(8))) uint32_t s_ws[2 * SPT_W], s_sp[2 * SPT_W], s_aws[2 * SPT_W], s_brk[2 * SPT_W], s_ts[2 * SPT_W], s_tb[2 * SPT_W], s_sk[2 * SPT_W];
    __shared__ uint64_t s_conv[SPT_W], s_st[SPT_W];
    __shared__ uint32_t s_cpre[SPT_W + 1];
    const SpText& t = a.t;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint32_t base = tile * (uint32_t)SPT_TB, nv = min((uint32_t)SPT_TB, t.n_bytes - base);
    const bool special = t.tstart != nullptr;
    // the tile's bytes, 16 a lane in one load (the text is 16-byte aligned and readable to the next multiple of 16), and the halo
    if (16u * tid < nv) *reinterpret_cast<uint4*>(s_in + SPT_HALO + 16u * tid) = *reinterpret_cast<const uint4*>(t.text + base + 16u * tid);
    if (tid < (uint32_t)SPT_HALO && base) s_in[tid] = t.text[base - SPT_HALO + tid];
    if (tid >= 32u && tid < 32u + (uint32_t)SPT_HALO && base + SPT_TB + (tid - 32u) < t.n_bytes) s_in[SPT_HALO + SPT_TB + tid - 32u] = t.text[base + SPT_TB + (tid - 32u)];
    if (tid < 2u * SPT_W) {
        const uint32_t wi = (base >> 5) + tid;                 // (a word of the special scan's bitmaps exists for every 32 bytes up to the text's end)
        const bool in = special && wi * 32u < t.n_bytes;
        s_ts[tid] = in ? t.tstart[wi] : 0u; s_tb[tid] = in ? t.tbits[wi] : 0u; s_sk[tid] = in ? t.skip[wi] : 0u;
        s_brk[tid] = s_ts[tid] | s_tb[tid];
    }
    __syncthreads();
    // document starts inside the tile
    const uint32_t d0 = sp_first_doc(t.doc_off, t.n_docs, base);
    for (uint32_t d = d0 + tid; d < t.n_docs; d += SPT_NT) {
        const uint64_t p = t.doc_off[d];
        if (p >= (uint64_t)base + nv) break;
        atomicOr(&s_brk[(uint32_t)(p - base) >> 5], 1u << ((uint32_t)(p - base) & 31u));
    }
    // every position of the window beyond the valid bytes is read from HBM by SpRd only if it is below n_bytes: wn covers what was staged
    const SpRd rd{t.text, s_in, base - (uint32_t)SPT_HALO, (uint32_t)SPT_HALO + nv + min((uint32_t)SPT_HALO, t.n_bytes - base - nv)};
    {
        uint32_t m_ws = 0, m_sp = 0, m_aws = 0;
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t li = 16u * tid + k;
            if (li >= nv) break;
            const uint32_t b = s_in[SPT_HALO + li];
            if (b > 0x20u && b < 0x80u) continue;               // (printable ASCII: none of the bits)
            const uint32_t bits = sp_byte_bits(t, rd, base + li);
            m_ws |= (bits & 1u) << k; m_sp |= ((bits >> 1) & 1u) << k; m_aws |= ((bits >> 2) & 1u) << k;
        }
        reinterpret_cast<uint16_t*>(s_ws)[tid] = (uint16_t)m_ws;
        reinterpret_cast<uint16_t*>(s_sp)[tid] = (uint16_t)m_sp;
        reinterpret_cast<uint16_t*>(s_aws)[tid] = (uint16_t)m_aws;
    }
    __syncthreads();
    if (tid < 64u) {
        const uint32_t w = tid;
        SpWord x;
        x.ws = reinterpret_cast<const uint64_t*>(s_ws)[w]; x.sp = reinterpret_cast<const uint64_t*>(s_sp)[w];
        x.aws = reinterpret_cast<const uint64_t*>(s_aws)[w]; x.brk = reinterpret_cast<const uint64_t*>(s_brk)[w];
        x.valid = 64u * w >= nv ? 0ull : sp_low_mask(nv - 64u * w);
        // the byte in front of the tile: is it whitespace, a converted space -- and, if its run is still open, ASCII-led?
        uint32_t t_ws = 0, t_sp = 0, t_led = 0;
        if (base && !(s_brk[0] & 1u)) {
            t_ws = sp_byte_ws(t, rd, base - 1u) ? 1u : 0u;
            t_sp = (t_ws && rd(base - 1u) == 0x20u) ? 1u : 0u;
            if (t_ws) {
                const uint32_t ds = d0 ? (uint32_t)t.doc_off[d0 - 1u] : 0u;     // the last document start below base (document 0 starts at byte 0)
                const SpRd far{t.text, nullptr, 0u, 0u};
                for (uint32_t r0 = base - 1u;; r0 -= 64u) {           // ends at ds at the latest: the lane that holds ds stops there
                    const bool on = r0 - ds >= tid;
                    const uint32_t r = r0 - tid, v = on ? sp_back_stop(t, far, r, ds) : 0u;
                    const uint64_t any = __ballot(v != 0u), at_r = __ballot(v == 2u);
                    if (any) {
                        const uint32_t l = (uint32_t)__ffsll((long long)any) - 1u;
                        const uint32_t first = (at_r >> l) & 1ull ? r0 - l : r0 - l + 1u;
                        t_led = sp_is_aws(t.text[first]) ? 1u : 0u;
                        break;
                    }
                }
            }
        }
        uint32_t pws = (uint32_t)__shfl_up((int)(uint32_t)(x.ws >> 63), 1), psp = (uint32_t)__shfl_up((int)(uint32_t)(x.sp >> 63), 1);
        if (w == 0u) { pws = t_ws; psp = t_sp; }
        uint32_t G, P;
        (void)sp_word_led(x, pws, 0u, G, P);
        if (w == 0u) G = sp_carry(G, P, t_led);
        for (int d = 1; d < 64; d <<= 1) {                       // the carries across the words: one scan of generate / propagate
            const uint32_t g2 = (uint32_t)__shfl_up((int)G, d), p2 = (uint32_t)__shfl_up((int)P, d);
            if ((int)w >= d) { G = sp_carry(G, P, g2); P &= p2; }
        }
        uint32_t cin = (uint32_t)__shfl_up((int)G, 1);
        if (w == 0u) cin = t_led;
        uint32_t g1, p1;
        const uint64_t led = sp_word_led(x, pws, cin, g1, p1);
        const SpOut o = sp_word_out(x, led & x.valid, pws, psp & cin);
        const uint32_t c = (uint32_t)__popcll(o.conv & x.valid), incl = wave_scan_incl(c);
        s_conv[w] = o.conv & x.valid; s_st[w] = o.starts; s_cpre[w] = incl - c;
        if (w == 63u) { s_cpre[SPT_W] = incl; if (!WRITE) a.cnt[tile] = incl; }
    }
    if constexpr (WRITE) {
        __shared__ __attribute__((aligned(16))) uint8_t s_out[SPT_OUT];
        __shared__ uint32_t s_ob[4][SPT_OBW];                    // staged bitmaps: chunk starts, text starts, tokens, literal bytes
        for (uint32_t i = tid; i < 4u * SPT_OBW; i += SPT_NT) (&s_ob[0][0])[i] = 0u;
        __syncthreads();
        const uint64_t obase = (uint64_t)base + 2ull * a.cnt[tile];
        const uint32_t olen = nv + 2u * s_cpre[SPT_W], ba = (uint32_t)(obase & 15u), bb = (uint32_t)(obase & 31u);
        const uint32_t nbm = special ? 4u : 1u;
        // local output position of local input position li
        auto opos = [&](uint32_t li) { return li + 2u * (s_cpre[li >> 6] + (uint32_t)__popcll(s_conv[li >> 6] & sp_low_mask(li & 63u))); };
        if (16u * tid < nv) {
            uint32_t o = opos(16u * tid);
            const uint64_t cv = s_conv[tid >> 2] >> (16u * (tid & 3u)), st = s_st[tid >> 2] >> (16u * (tid & 3u));
            const uint32_t ts = reinterpret_cast<const uint16_t*>(s_ts)[tid], tb = reinterpret_cast<const uint16_t*>(s_tb)[tid], sk = reinterpret_cast<const uint16_t*>(s_sk)[tid];
            for (uint32_t k = 0; k < 16u && 16u * tid + k < nv; k++) {
                if ((st >> k) & 1ull) atomicOr(&s_ob[0][(bb + o) >> 5], 1u << ((bb + o) & 31u));
                if (special) {
                    if ((ts >> k) & 1u) atomicOr(&s_ob[1][(bb + o) >> 5], 1u << ((bb + o) & 31u));
                    if ((tb >> k) & 1u) { atomicOr(&s_ob[2][(bb + o) >> 5], 1u << ((bb + o) & 31u)); a.stage_out[obase + o] = a.stage_in[base + 16u * tid + k]; }
                    if ((sk >> k) & 1u) atomicOr(&s_ob[3][(bb + o) >> 5], 1u << ((bb + o) & 31u));
                }
                if ((cv >> k) & 1ull) { s_out[ba + o] = 0xE2u; s_out[ba + o + 1u] = 0x96u; s_out[ba + o + 2u] = 0x81u; o += 3u; }
                else { s_out[ba + o] = s_in[SPT_HALO + 16u * tid + k]; o += 1u; }
            }
        }
        // the documents' offsets in the rewritten text; the last tile also closes the table (documents that start at the text's end)
        for (uint32_t d = d0 + tid; d < t.n_docs; d += SPT_NT) {
            const uint64_t p = t.doc_off[d];
            if (p >= (uint64_t)base + nv) break;
            a.out_doc_off[d] = obase + opos((uint32_t)(p - base));
        }
        if (tile == gridDim.x - 1u) {
            const uint64_t total = (uint64_t)t.n_bytes + 2ull * a.cnt[gridDim.x];
            for (uint32_t d = sp_first_doc(t.doc_off, t.n_docs, t.n_bytes) + tid; d <= t.n_docs; d += SPT_NT) a.out_doc_off[d] = total;
        }
        __syncthreads();
        // the bytes: whole 16-byte groups by one store; the group the tile shares with the tile in front, and the one it shares with the next, byte by byte
        uint8_t* const o16 = a.out + (obase - ba);
        for (uint32_t j = tid; j * 16u < ba + olen; j += SPT_NT) {
            const uint32_t lo = j * 16u;
            if (lo >= ba && lo + 16u <= ba + olen) *reinterpret_cast<uint4*>(o16 + lo) = *reinterpret_cast<const uint4*>(s_out + lo);
            else for (uint32_t q = max(lo, ba); q < min(lo + 16u, ba + olen); q++) o16[q] = s_out[q];
        }
        // the bitmaps: the words the tile has to itself by plain stores, its first and last word -- shared with its neighbours -- by an OR
        const uint32_t nw = (bb + olen + 31u) >> 5;
        const uint64_t w0 = obase >> 5;
        for (uint32_t m = 0; m < nbm; m++) {
            uint32_t* const dst = m == 0u ? a.starts : m == 1u ? a.o_tstart : m == 2u ? a.o_tbits : a.o_skip;
            for (uint32_t j = tid; j < nw; j += SPT_NT) {
                const uint32_t v = s_ob[m][j];
                if (j == 0u || j == nw - 1u) { if (v) atomicOr(&dst[w0 + j], v); }
                else dst[w0 + j] = v;
            }
        }
    }
}
#endif  // __HIPCC__

}  // namespace spl
