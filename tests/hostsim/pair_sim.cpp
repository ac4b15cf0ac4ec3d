// pair_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_pair.h (the code k_collate_pair runs) evaluated on the CPU
// for every output element, with the kernel's geometry: the grid of cpair_grid, workgroups of COL_NT lanes, COL_VEC elements a lane,
// the final partial group stored element by element.  ps_groups evaluates single groups at any flat index (outputs no memory could
// hold: index arithmetic beyond 2^32 elements).  Built with g++; no GPU.
#include <cstdint>
#include <cstring>

#include "../../splintr_amd/csrc/spl_k_pair.h"

using namespace spl;

namespace {
PairOpts opts(uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t trunc, const uint32_t* prefix, uint32_t n_prefix, const uint32_t* middle,
              uint32_t n_middle, const uint32_t* suffix, uint32_t n_suffix) {
    PairOpts o{};
    o.g.flags = flags; o.g.L = L; o.g.pad_id = pad_id; o.g.trunc = trunc;
    cpair_set_fixed(o, prefix, n_prefix, middle, n_middle, suffix, n_suffix);
    return o;
}
}  // namespace

extern "C" {

void ps_geometry(uint32_t out[3]) { out[0] = COL_NT; out[1] = COL_VEC; out[2] = COL_SPAN; }

void ps_trunc(uint64_t la, uint64_t lb, uint32_t B, uint32_t trunc, uint32_t out[2]) { cpair_trunc(la, lb, B, trunc, out[0], out[1]); }

void ps_grid(uint64_t total, uint32_t out[3]) { cpair_grid(total, out[0], out[1], out[2]); }
uint64_t ps_span(uint32_t bx, uint32_t by, uint32_t bz, uint32_t gx, uint32_t gy) { return cpair_span(bx, by, bz, gx, gy); }

// rows u32 [n_pairs * L]; mask / type / special u8, len i32 [n_pairs], kept i32 [2 * n_pairs] (each may be null); status: one word
int ps_pair(const uint32_t* a_ids, const uint64_t* a_off, uint32_t n_a, const uint32_t* b_ids, const uint64_t* b_off, uint32_t n_b,
            const int32_t* a_idx, const int32_t* b_idx, uint32_t n_pairs, uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t trunc,
            const uint32_t* prefix, uint32_t n_prefix, const uint32_t* middle, uint32_t n_middle, const uint32_t* suffix, uint32_t n_suffix,
            uint32_t* rows, uint8_t* mask, uint8_t* type, uint8_t* special, int32_t* len, int32_t* kept, uint32_t* status) {
    const PairOpts o = opts(flags, L, pad_id, trunc, prefix, n_prefix, middle, n_middle, suffix, n_suffix);
    const PairSrc s{a_ids, a_off, b_ids, b_off, a_idx, b_idx, n_a, n_b};
    const uint64_t total = (uint64_t)n_pairs * L;
    uint32_t gx, gy, gz;
    cpair_grid(total, gx, gy, gz);
    for (uint32_t bz = 0; bz < gz; bz++)
        for (uint32_t by = 0; by < gy; by++)
            for (uint32_t bx = 0; bx < gx; bx++)
                for (uint32_t lane = 0; lane < COL_NT; lane++) {
                    const uint64_t e0 = cpair_span(bx, by, bz, gx, gy) * COL_SPAN + (uint64_t)lane * COL_VEC;
                    if (e0 >= total) continue;
                    const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
                    uint32_t v[COL_VEC], m, ty, sp;
                    cpair_group(s, e0, n, o.g, o.fixed, v, m, ty, sp, len, kept, status);
                    for (uint32_t i = 0; i < n; i++) {
                        rows[e0 + i] = v[i];
                        if (mask) mask[e0 + i] = (uint8_t)(m >> (8 * i));
                        if (type) type[e0 + i] = (uint8_t)(ty >> (8 * i));
                        if (special) special[e0 + i] = (uint8_t)(sp >> (8 * i));
                    }
                }
    return 0;
}

// The groups that start at the flat elements e0[0 .. count): v [count * COL_VEC], m / ty / sp [count] (a group's four bytes each).
// Nothing of size n_pairs * L exists: len [n_pairs] and kept [2 * n_pairs] are the only arrays a group writes to.
int ps_groups(const uint32_t* a_ids, const uint64_t* a_off, uint32_t n_a, const uint32_t* b_ids, const uint64_t* b_off, uint32_t n_b,
              const int32_t* a_idx, const int32_t* b_idx, uint32_t n_pairs, uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t trunc,
              const uint32_t* prefix, uint32_t n_prefix, const uint32_t* middle, uint32_t n_middle, const uint32_t* suffix, uint32_t n_suffix,
              const uint64_t* e0, uint32_t count, uint32_t* v, uint32_t* m, uint32_t* ty, uint32_t* sp, int32_t* len, int32_t* kept,
              uint32_t* status) {
    const PairOpts o = opts(flags, L, pad_id, trunc, prefix, n_prefix, middle, n_middle, suffix, n_suffix);
    const PairSrc s{a_ids, a_off, b_ids, b_off, a_idx, b_idx, n_a, n_b};
    const uint64_t total = (uint64_t)n_pairs * L;
    for (uint32_t g = 0; g < count; g++) {
        if (e0[g] >= total || e0[g] % COL_VEC) return -1;
        const uint32_t n = total - e0[g] < COL_VEC ? (uint32_t)(total - e0[g]) : COL_VEC;
        cpair_group(s, e0[g], n, o.g, o.fixed, v + (uint64_t)g * COL_VEC, m[g], ty[g], sp[g], len, kept, status);
    }
    return 0;
}

}  // extern "C"
