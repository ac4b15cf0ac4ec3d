// sp_sim.cpp -- TEST TOOL: the per-tile logic of splintr_amd/csrc/spl_k_sp.h (what k_sp_rewrite runs: sp_byte_bits, sp_word_led, sp_carry,
// sp_word_out, sp_back_stop, sp_first_doc) driven on the CPU, tile by tile, with a tile of `tile` bytes (a multiple of 64; 64 in the tests,
// so that every seam case occurs in short inputs).  The kernel's driver is RESTATED here: the words of a tile one after the other where
// the kernel has one a lane, the carries across them by a loop over sp_carry where the kernel scans, the backward walk 64 positions a
// round as the ballots go, the count pass before the write pass.  A change to the driver in the kernel is checked by
// tests/test_gpu_sentencepiece.py alone.  Built with g++; no GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_sp.h"

using namespace spl;

namespace {

struct Tile { std::vector<uint64_t> conv, starts; uint64_t n_conv = 0; };

Tile run_tile(const SpText& t, uint32_t tile, uint32_t tb) {
    const uint32_t base = tile * tb, nv = t.n_bytes - base < tb ? t.n_bytes - base : tb, W = tb / 64;
    const SpRd rd{t.text, nullptr, 0u, 0u};
    std::vector<SpWord> x(W);
    for (uint32_t w = 0; w < W; w++) {
        x[w] = SpWord{0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < 64 && 64 * w + k < nv; k++) {
            const uint32_t bits = sp_byte_bits(t, rd, base + 64 * w + k);
            x[w].ws |= (uint64_t)(bits & 1u) << k; x[w].sp |= (uint64_t)((bits >> 1) & 1u) << k;
            x[w].aws |= (uint64_t)((bits >> 2) & 1u) << k; x[w].brk |= (uint64_t)((bits >> 3) & 1u) << k;
            x[w].valid |= 1ull << k;
        }
    }
    const uint32_t d0 = sp_first_doc(t.doc_off, t.n_docs, base);
    for (uint32_t d = d0; d < t.n_docs && t.doc_off[d] < (uint64_t)base + nv; d++) {
        const uint32_t li = (uint32_t)(t.doc_off[d] - base);
        x[li >> 6].brk |= 1ull << (li & 63);
    }
    uint32_t t_ws = 0, t_sp = 0, t_led = 0;
    if (base && !(x[0].brk & 1ull)) {
        t_ws = sp_byte_ws(t, rd, base - 1) ? 1u : 0u;
        t_sp = (t_ws && t.text[base - 1] == 0x20) ? 1u : 0u;
        if (t_ws) {
            const uint32_t ds = d0 ? (uint32_t)t.doc_off[d0 - 1] : 0u;
            for (uint32_t r0 = base - 1;; r0 -= 64) {
                bool found = false;
                for (uint32_t lane = 0; lane < 64 && !found; lane++) {        // (the first set bit of the ballot)
                    if (r0 - ds < lane) break;
                    const uint32_t v = sp_back_stop(t, rd, r0 - lane, ds);
                    if (v) { t_led = sp_is_aws(t.text[v == 2u ? r0 - lane : r0 - lane + 1]) ? 1u : 0u; found = true; }
                }
                if (found) break;
            }
        }
    }
    Tile out;
    out.conv.resize(W); out.starts.resize(W);
    uint32_t cin = t_led, pws = t_ws, psp = t_sp;
    for (uint32_t w = 0; w < W; w++) {
        uint32_t G, P, g1, p1;
        (void)sp_word_led(x[w], pws, 0u, G, P);
        const uint64_t led = sp_word_led(x[w], pws, cin, g1, p1);
        const SpOut o = sp_word_out(x[w], led & x[w].valid, pws, psp & cin);
        out.conv[w] = o.conv & x[w].valid; out.starts[w] = o.starts;
        out.n_conv += (uint64_t)__builtin_popcountll(out.conv[w]);
        cin = sp_carry(G, P, cin); pws = (uint32_t)(x[w].ws >> 63); psp = (uint32_t)(x[w].sp >> 63);
    }
    return out;
}

}  // namespace

// The whole rewrite: out (capacity 3 * n_bytes), start_bits (3 * n_bytes / 32 + 2 words, zeroed here), out_doc_off[n_docs + 1].
// ucls: the class table's two stages.  tstart / tbits / skip: the literal scan's bitmaps over the text, or null.  Returns the new length.
extern "C" uint64_t sp_sim_rewrite(const uint8_t* text, uint32_t n_bytes, const uint64_t* doc_off, uint32_t n_docs, const uint16_t* ucls1,
                                   const uint8_t* ucls2, uint32_t shift, const uint32_t* tstart, const uint32_t* tbits, const uint32_t* skip,
                                   uint32_t tile, uint8_t* out, uint32_t* start_bits, uint64_t* out_doc_off) {
    const SpText t{text, n_bytes, doc_off, n_docs, ucls1, ucls2, shift, tstart, tbits, skip};
    const uint32_t ntiles = (n_bytes + tile - 1) / tile;
    std::vector<Tile> tiles;
    std::vector<uint64_t> pre(ntiles + 1, 0);
    for (uint32_t k = 0; k < ntiles; k++) { tiles.push_back(run_tile(t, k, tile)); pre[k + 1] = pre[k] + tiles[k].n_conv; }      // count pass and scan
    const uint64_t n_out = (uint64_t)n_bytes + 2 * pre[ntiles];
    memset(start_bits, 0, (size_t)(3ull * n_bytes / 32 + 2) * 4);
    for (uint32_t k = 0; k < ntiles; k++) {                                     // write pass
        uint64_t o = (uint64_t)k * tile + 2 * pre[k];
        for (uint32_t li = 0; li < tile && k * tile + li < n_bytes; li++) {
            const uint32_t p = k * tile + li;
            for (uint32_t d = sp_first_doc(doc_off, n_docs, p); d < n_docs && doc_off[d] == p; d++) out_doc_off[d] = o;
            if ((tiles[k].starts[li >> 6] >> (li & 63)) & 1ull) start_bits[o >> 5] |= 1u << (o & 31);
            if ((tiles[k].conv[li >> 6] >> (li & 63)) & 1ull) { out[o] = 0xE2; out[o + 1] = 0x96; out[o + 2] = 0x81; o += 3; }
            else out[o++] = text[p];
        }
    }
    for (uint32_t d = sp_first_doc(doc_off, n_docs, n_bytes); d <= n_docs; d++) out_doc_off[d] = n_out;
    return n_out;
}
