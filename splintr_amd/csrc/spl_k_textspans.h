// spl_k_textspans.h -- part of spl_kernels.hip (included there, in front of spl_k_wp.h): what the span variants of WordPiece mode's and
// Unigram mode's write kernels share (spl_encode_batch_spans_device).  Those kernels know a token's first and
// last SOURCE in the caller's text as raw byte positions; here a pair of them becomes a row of d_byte_span and of d_char_span, relative
// to the token's document.
//
// The character unit is spl_token_spans_device's: offset p counts the bytes b with (b & 0xC0) != 0x80 in front of it.  k_text_cstarts
// counts those per TS_BLK bytes of the text, 16 bytes a lane and four lanes a block; k_decode_scan makes the counts exclusive sums;
// ts_chars_before adds the partial block's bytes -- one load of the sum, up to four 16-byte loads of text and a popcount each.
#pragma once
#include "spl_common.h"

namespace spl {

constexpr int TS_BLK = 64, TS_NT = 256;                      // bytes per counted block; lanes of k_text_cstarts (16 bytes each)

struct TextSpanOut {
    const uint8_t* text; const uint64_t* doc_off;            // the CALLER's text and offsets (WordPiece mode matches normalised text)
    const uint64_t* cblk;                                    // [n_bytes / TS_BLK + 2]: character starts in front of every block (d_char_span only)
    int32_t* bspan; int32_t* cspan;                          // [ids_cap, 2] each; either may be null
};

// Character starts among the first n (at most 16) bytes of v: a continuation byte has bit 7 set and bit 6 clear.
SPL_HD uint32_t ts_starts16(const uint32_t v[4], uint32_t n) {
    uint32_t c = 0;
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t nk = n > 4u * k ? (n - 4u * k < 4u ? n - 4u * k : 4u) : 0u;
        const uint32_t cont = v[k] & ~(v[k] << 1) & 0x80808080u & (nk >= 4u ? 0xFFFFFFFFu : (1u << (8u * nk)) - 1u);
        c += nk - (uint32_t)__builtin_popcount(cont);
    }
    return c;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(TS_NT) void k_text_cstarts(const uint8_t* text, uint32_t n_bytes, uint64_t* cblk) {
    static_assert(TS_BLK == 64, "four lanes of 16 bytes a block");
    const uint32_t i = blockIdx.x * (uint32_t)TS_NT + threadIdx.x;
    const uint64_t p = 16ull * i;
    uint32_t c = 0;
    if (p < n_bytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + p);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        c = ts_starts16(w, min(16u, n_bytes - (uint32_t)p));
    }
    c += (uint32_t)__shfl_xor((int)c, 1);
    c += (uint32_t)__shfl_xor((int)c, 2);
    if ((i & 3u) == 0u && p < n_bytes) cblk[i >> 2] = c;
}

// Character starts in text[0, p), p <= n_bytes (the text is 16-byte aligned and readable to the next multiple of 16).
__device__ __forceinline__ uint32_t ts_chars_before(const TextSpanOut& o, uint32_t p) {
    uint32_t c = (uint32_t)o.cblk[p / (uint32_t)TS_BLK];
    for (uint32_t g = p & ~((uint32_t)TS_BLK - 1u); g < p; g += 16u) {
        const uint4 v = *reinterpret_cast<const uint4*>(o.text + g);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        c += ts_starts16(w, min(16u, p - g));
    }
    return c;
}
// The start of the document that holds raw position p (the last one that starts at or in front of it: empty documents lie in front).
__device__ __forceinline__ uint32_t ts_doc_start(const TextSpanOut& o, uint32_t n_docs, uint32_t p) {
    return (uint32_t)o.doc_off[sp_first_doc(o.doc_off, n_docs, (uint64_t)p + 1u) - 1u];
}
__device__ __forceinline__ uint32_t ts_doc_chars(const TextSpanOut& o, uint32_t ds) { return o.cspan ? ts_chars_before(o, ds) : 0u; }
// Row `slot` of the spans: raw positions [rs, re) of a document that starts at ds with c0 = ts_doc_chars in front of it.  start_only: the
// row's end stands already (a fused run of unk grows towards the text's start).
__device__ __forceinline__ void ts_store(const TextSpanOut& o, uint64_t slot, uint32_t ds, uint32_t c0, uint32_t rs, uint32_t re, bool start_only) {
    if (o.bspan) {
        o.bspan[2u * slot] = (int32_t)(rs - ds);
        if (!start_only) o.bspan[2u * slot + 1u] = (int32_t)(re - ds);
    }
    if (o.cspan) {
        o.cspan[2u * slot] = (int32_t)(ts_chars_before(o, rs) - c0);
        if (!start_only) o.cspan[2u * slot + 1u] = (int32_t)(ts_chars_before(o, re) - c0);
    }
}
#endif  // __HIPCC__

}  // namespace spl
