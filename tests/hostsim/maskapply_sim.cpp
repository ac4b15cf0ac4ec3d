// maskapply_sim.cpp -- TEST TOOL: the first half of splintr_amd/csrc/spl_k_maskapply.h (the code k_mask_apply runs: which columns a
// 16-byte piece of an unaligned row holds, where their bits lie in the mask, and the lane's decision -- nothing, a 16-byte store, load /
// select / store, element stores) evaluated on the CPU over an IO policy that counts: every byte of the logits buffer has a store count
// and a load count, every mask word a read count, an access outside the buffer is damage and is not made.  The kernel's grid is walked row
// by row and lane by lane.  Built with g++; no GPU.  -DMASKAPPLY_SIM_MAIN adds a main() that runs a small self-check (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_maskapply.h"

using namespace spl;

namespace {

struct SimIO {
    const uint32_t* mask; uint8_t* mask_r; uint64_t mask_words;
    uint64_t lo, hi;                    // the buffer's addresses [lo, hi)
    uint8_t* st; uint8_t* ld;           // per byte of the buffer: stores, loads
    uint64_t damage = 0, kinds[4] = {0, 0, 0, 0};
    bool inside(uint64_t a, uint64_t n) { if (a >= lo && a + n <= hi) return true; damage++; return false; }
    uint32_t word(uint64_t i) { if (i >= mask_words) { damage++; return 0; } mask_r[i]++; return mask[i]; }
    MaQuad load16(uint64_t a) {
        MaQuad q{{0, 0, 0, 0}};
        if ((a & 15) || !inside(a, 16)) { damage += (a & 15) != 0; return q; }
        memcpy(q.w, reinterpret_cast<const void*>(a), 16);
        for (int i = 0; i < 16; i++) ld[a - lo + i]++;
        return q;
    }
    void store16(uint64_t a, const MaQuad& q) {
        if ((a & 15) || !inside(a, 16)) { damage += (a & 15) != 0; return; }
        memcpy(reinterpret_cast<void*>(a), q.w, 16);
        for (int i = 0; i < 16; i++) st[a - lo + i]++;
    }
    void store_el(uint64_t a, uint32_t es, uint32_t v) {
        if ((a & (es - 1)) || !inside(a, es)) { damage += (a & (es - 1)) != 0; return; }
        memcpy(reinterpret_cast<void*>(a), &v, es);
        for (uint32_t i = 0; i < es; i++) st[a - lo + i]++;
    }
};

}  // namespace

extern "C" {

void ma_sim_piece(uint64_t A, uint32_t es, uint32_t n_eff, uint64_t p, uint64_t out[5]) {
    const MaPiece q = ma_piece(A, es, n_eff, p);
    out[0] = q.addr; out[1] = q.c0; out[2] = q.j0; out[3] = q.n; out[4] = ma_n_pieces(A, es, n_eff);
}
uint64_t ma_sim_grid_pieces(uint32_t es, uint32_t n_eff) { return ma_grid_pieces(es, n_eff); }

// buf [buf_bytes]: the logits' buffer, logits[0, 0] at buf + base_off.  stats: damage, then the lanes per kind (nothing, store, load and
// store, element stores).
int ma_sim(uint8_t* buf, uint64_t buf_bytes, uint64_t base_off, uint32_t dtype, uint64_t n_rows, uint32_t n_cols, uint64_t row_stride,
           const uint32_t* mask, uint32_t n_words, uint64_t mask_stride, uint64_t mask_words, const uint8_t* live, uint8_t* st, uint8_t* ld,
           uint8_t* mask_r, uint64_t* stats) {
    if (dtype > MA_BF16 || row_stride < n_cols || mask_stride < n_words) return -1;
    MaArgs a{};
    a.logits = reinterpret_cast<uint64_t>(buf) + base_off; a.mask = mask; a.live = live;
    a.n_rows = n_rows; a.row_stride = row_stride; a.mask_stride = mask_stride;
    a.n_cols = n_cols; a.n_words = n_words; a.es = ma_elem_bytes(dtype); a.ninf = ma_ninf(dtype);
    SimIO io{mask, mask_r, mask_words, reinterpret_cast<uint64_t>(buf), reinterpret_cast<uint64_t>(buf) + buf_bytes, st, ld};
    const uint64_t pieces = ma_grid_pieces(a.es, ma_n_eff(n_cols, n_words)), wgs = (pieces + MA_NT - 1) / MA_NT;
    for (uint64_t r = 0; r < n_rows; r++) {
        if (!ma_row_live(a, r)) continue;
        for (uint64_t g = 0; g < wgs; g++)
            for (uint32_t l = 0; l < MA_NT; l++) io.kinds[ma_lane(io, a, r, g * MA_NT + l)]++;
    }
    stats[0] = io.damage;
    for (int k = 0; k < 4; k++) stats[1 + k] = io.kinds[k];
    return 0;
}

}  // extern "C"

#ifdef MASKAPPLY_SIM_MAIN
// two bf16 rows of 9 columns, stride 9, the base one element behind a 16-byte boundary: bits 0b1_0101_0101 and all zeros
int main() {
    alignas(16) uint8_t buf[64];
    uint8_t st[64] = {0}, ld[64] = {0}, mask_r[2] = {0, 0};
    for (int i = 0; i < 64; i++) buf[i] = (uint8_t)(0x3C + (i & 1));
    const uint32_t mask[2] = {0x155u, 0u};
    uint64_t stats[5];
    int bad = ma_sim(buf, 64, 2, MA_BF16, 2, 9, 9, mask, 1, 1, 2, nullptr, st, ld, mask_r, stats) != 0 || stats[0] != 0;
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 9; c++) {
            uint16_t v;
            memcpy(&v, buf + 2 + 2 * (r * 9 + c), 2);
            const bool keep = r == 0 && !(c & 1);
            bad += keep ? v != 0x3D3C : v != 0xFF80;
        }
    bad += buf[0] != 0x3C || buf[1] != 0x3D || buf[38] != 0x3C || buf[39] != 0x3D;      // in front of row 0, behind row 1
    for (int i = 0; i < 64; i++) bad += st[i] > 1;
    printf(bad ? "maskapply_sim: FAILED\n" : "maskapply_sim: ok\n");
    return bad;
}
#endif
