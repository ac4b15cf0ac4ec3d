// spl_k_maskapply.h -- spl_mask_apply_device: an allowed-token BITMASK int32 [n_rows, n_words] applied to logits [n_rows, n_cols] of f32,
// f16 or bf16 in place: for every live row r and every column c < min(n_cols, 32 * n_words) whose bit (c & 31 of word
// c >> 5 of mask row r) is 0, logits[r, c] becomes -inf -- a STORE of the pattern, no arithmetic: a NaN there becomes -inf too.  Everything
// else keeps its bits: allowed columns, columns at or beyond 32 * n_words, the row_stride - n_cols elements behind a row, rows that are not
// live (whose mask rows are not read either).
//
// The logits need no alignment beyond their element's.  A row is cut into PIECES of 16 bytes by absolute address; a lane owns a piece: 8
// half-precision columns or 4 floats, whose bits come from the one or two mask words that cover them.  A piece that lies inside the row's
// masked columns with all 16 bytes is WHOLE, the pieces at the row's two ends are PARTIAL (the other bytes are a neighbouring row's, its
// padding, or columns the mask does not reach).  Per piece:
//
//     every bit 1               nothing is loaded, nothing stored
//     whole, every bit 0        one 16-byte store of -inf, no load
//     whole, mixed              one 16-byte load, select, one 16-byte store
//     partial                   an element store of -inf per 0 bit, no load (a 16-byte access there would race with the neighbour's lane)
//
// so the traffic follows the mask: a healing-constrained row is written and not read, a UTF-8 start row costs little more than its mask, a
// row that is not live costs its live byte.  No LDS, no atomics, no wait between workgroups.
//
// The first half is plain C++ (values only): the index arithmetic -- which columns a piece holds, which are the row's, where their bits
// lie -- and the lane's decision, over an IO policy (word, load16, store16, store_el).  The kernel instantiates it with global memory,
// tests/hostsim/maskapply_sim.cpp with counted host buffers: the same text runs in both.
#pragma once
#include "spl_common.h"

namespace spl {

// (the values of SPL_F32 / SPL_F16 / SPL_BF16 in include/splintr_hip.h)
constexpr uint32_t MA_F32 = 0, MA_F16 = 1, MA_BF16 = 2;
constexpr uint32_t MA_NT = 256;
constexpr uint32_t MA_PIECE = 16;                                  // bytes a lane owns

struct MaArgs {
    uint64_t logits;                    // the address of logits[0, 0]
    const uint32_t* mask; const uint8_t* live;
    uint64_t n_rows, row_stride, mask_stride;                      // row_stride in elements, mask_stride in words
    uint32_t n_cols, n_words, es;       // es: bytes an element (2 or 4)
    uint32_t ninf;                      // -inf of the dtype; a 2-byte pattern in both halves
};
struct MaQuad { uint32_t w[4]; };       // a piece as four words

SPL_HD uint32_t ma_ninf(uint32_t dtype) { return dtype == MA_F32 ? 0xFF800000u : dtype == MA_F16 ? 0xFC00FC00u : 0xFF80FF80u; }
SPL_HD uint32_t ma_elem_bytes(uint32_t dtype) { return dtype == MA_F32 ? 4u : 2u; }
// the columns of a row the mask reaches
SPL_HD uint32_t ma_n_eff(uint32_t n_cols, uint32_t n_words) { return (uint64_t)n_words * 32 < n_cols ? n_words * 32u : n_cols; }

// ------------------------------------------------------------------------------------------ the index arithmetic
// A row that begins at address A (a multiple of es) with n_eff masked columns.  Piece p (0 ..) covers the addresses [(A & ~15) + 16 p, + 16):
// its element j (0 .. E - 1, E = 16 / es) is column p E - a + j with a = (A & 15) / es, the elements in front of the row in piece 0.
struct MaPiece {
    uint64_t addr;                      // the piece's address (16-byte aligned)
    uint32_t c0;                        // the column of its first element that is the row's
    uint32_t j0, n;                     // that element's index in the piece, and how many of the piece's elements are the row's (0: none)
};
SPL_HD uint64_t ma_n_pieces(uint64_t A, uint32_t es, uint32_t n_eff) {
    if (!n_eff) return 0;
    const uint32_t E = MA_PIECE / es, a = (uint32_t)(A & (MA_PIECE - 1)) / es;
    return ((uint64_t)a + n_eff + E - 1) / E;
}
SPL_HD MaPiece ma_piece(uint64_t A, uint32_t es, uint32_t n_eff, uint64_t p) {
    const uint32_t E = MA_PIECE / es, a = (uint32_t)(A & (MA_PIECE - 1)) / es;
    MaPiece q;
    q.addr = (A & ~(uint64_t)(MA_PIECE - 1)) + p * MA_PIECE;
    const uint64_t first = p * E;                                  // element index of the piece's first element, counted from the row's first piece
    q.j0 = first < a ? a - (uint32_t)first : 0u;
    const uint64_t c0 = first + q.j0 - a;
    q.c0 = (uint32_t)c0;
    q.n = c0 >= n_eff ? 0u : (n_eff - q.c0 < E - q.j0 ? n_eff - q.c0 : E - q.j0);
    return q;
}
// the bits of columns c0 .. c0 + n - 1 (n in 1 .. 8, all below 32 * n_words), column c0 lowest: one mask word, or two where they straddle
template <class IO> SPL_HD uint32_t ma_bits(IO& io, uint64_t row_word0, uint32_t c0, uint32_t n) {
    const uint32_t k = c0 >> 5, sh = c0 & 31u;
    uint64_t v = io.word(row_word0 + k);
    if (((c0 + n - 1) >> 5) != k) v |= (uint64_t)io.word(row_word0 + k + 1) << 32;
    return (uint32_t)(v >> sh) & ((1u << n) - 1u);
}

// ------------------------------------------------------------------------------------------ one lane: piece p of row r
// a row that is not live is left alone, its mask row unread: the one byte it costs
SPL_HD bool ma_row_live(const MaArgs& a, uint64_t r) { return !a.live || a.live[r] != 0; }
// what it did, for the traffic model: 0 nothing, 1 a 16-byte store, 2 a 16-byte load and store, 3 element stores
template <class IO> SPL_HD uint32_t ma_lane(IO& io, const MaArgs& a, uint64_t r, uint64_t p) {
    const uint32_t n_eff = ma_n_eff(a.n_cols, a.n_words), E = MA_PIECE / a.es;
    const uint64_t A = a.logits + r * a.row_stride * a.es;
    if (p >= ma_n_pieces(A, a.es, n_eff)) return 0u;
    const MaPiece q = ma_piece(A, a.es, n_eff, p);
    if (!q.n) return 0u;
    const uint32_t all = (1u << q.n) - 1u;
    const uint32_t bits = ma_bits(io, r * a.mask_stride, q.c0, q.n);
    if (bits == all) return 0u;
    if (q.n < E) {                                                 // partial: the row's elements one by one
        for (uint32_t i = 0; i < q.n; i++)
            if (!((bits >> i) & 1u)) io.store_el(q.addr + (uint64_t)(q.j0 + i) * a.es, a.es, a.ninf);
        return 3u;
    }
    MaQuad x;
    if (bits == 0u) {
        x.w[0] = x.w[1] = x.w[2] = x.w[3] = a.ninf;
        io.store16(q.addr, x);
        return 1u;
    }
    x = io.load16(q.addr);
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        uint32_t z;                                                // the bits of word i that become -inf
        if (a.es == 4) z = ((bits >> i) & 1u) ? 0u : 0xFFFFFFFFu;
        else z = (((bits >> (2 * i)) & 1u) ? 0u : 0x0000FFFFu) | (((bits >> (2 * i + 1)) & 1u) ? 0u : 0xFFFF0000u);
        x.w[i] = (x.w[i] & ~z) | (a.ninf & z);
    }
    io.store16(q.addr, x);
    return 2u;
}
// pieces the grid covers per row: the most any row has (a row's own count is one less where it begins on a 16-byte boundary)
SPL_HD uint64_t ma_grid_pieces(uint32_t es, uint32_t n_eff) {
    if (!n_eff) return 0;
    const uint32_t E = MA_PIECE / es;
    return ((uint64_t)(E - 1) + n_eff + E - 1) / E;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ the kernel
struct MaDevIO {
    const uint32_t* mask;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return mask[i]; }
    __device__ __forceinline__ MaQuad load16(uint64_t addr) const {
        const uint4 v = *reinterpret_cast<const uint4*>(addr);
        return MaQuad{{v.x, v.y, v.z, v.w}};
    }
    __device__ __forceinline__ void store16(uint64_t addr, const MaQuad& x) const { *reinterpret_cast<uint4*>(addr) = make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]); }
    __device__ __forceinline__ void store_el(uint64_t addr, uint32_t es, uint32_t v) const {
        if (es == 4) *reinterpret_cast<uint32_t*>(addr) = v;
        else *reinterpret_cast<uint16_t*>(addr) = (uint16_t)v;
    }
};

// grid (pieces of a row, rows over y and z)
template <uint32_t ES>
__global__ __launch_bounds__(MA_NT) void k_mask_apply(MaArgs a) {
    const uint64_t r = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (r >= a.n_rows) return;
    if (!ma_row_live(a, r)) return;
    a.es = ES;
    MaDevIO io{a.mask};
    (void)ma_lane(io, a, r, (uint64_t)blockIdx.x * MA_NT + threadIdx.x);
}
#endif  // __HIPCC__

}  // namespace spl
