// seqscan_sim.h -- TEST TOOL: the two drivers of splintr_amd/csrc/spl_k_seqscan.h (seq_one_body; seq_len_body, k_decode_scan,
// seq_write_body) restated on the CPU, once, for stream_sim.cpp and stop_sim.cpp.  count(b, Carry&) gives the bytes sequence b emits and
// what it hands its write; write(b, const Carry&, o0) writes the sequence from o0 on.  Every write of an offset is counted.
#pragma once
#include <cstdint>
#include <vector>
#include "../../splintr_amd/csrc/spl_k_seqscan.h"

namespace seqsim {
template <class Carry, class Count, class Write>
void run(uint64_t n, int three, uint64_t* out_off, uint8_t* off_writes, Count count, Write write) {
    using namespace spl;
    std::vector<uint64_t> cnt(n + 1, 0);
    std::vector<Carry> keep(n);
    if (!three) {                                   // seq_one_body: count, scan in place, write
        for (uint64_t b = 0; b < n; b++) cnt[b] = count(b, keep[b]);
        uint64_t run = 0;
        for (uint64_t b = 0; b < n; b++) { const uint64_t v = cnt[b]; cnt[b] = run; run += v; }
        out_off[n] = run; off_writes[n]++;
        for (uint64_t b = 0; b < n; b++) { write(b, keep[b], cnt[b]); out_off[b] = cnt[b]; off_writes[b]++; }
        return;
    }
    const uint64_t n_blk = seq_n_blocks(n);
    std::vector<uint64_t> blk(n_blk + 1, 0);
    for (uint64_t g = 0; g < n_blk; g++)            // seq_len_body
        for (uint32_t i = 0; i < SEQ_BLK; i++) {
            const uint64_t b = g * SEQ_BLK + i;
            if (b >= n) break;
            cnt[b] = count(b, keep[b]);
            blk[g] += cnt[b];
        }
    uint64_t run = 0;                               // k_decode_scan
    for (uint64_t g = 0; g < n_blk; g++) { const uint64_t v = blk[g]; blk[g] = run; run += v; }
    blk[n_blk] = run;
    for (uint64_t g = 0; g < n_blk; g++) {          // seq_write_body
        uint64_t o0 = blk[g];
        for (uint32_t i = 0; i < SEQ_BLK; i++) {
            const uint64_t b = g * SEQ_BLK + i;
            if (b >= n) break;
            write(b, keep[b], o0);
            out_off[b] = o0; off_writes[b]++;
            o0 += cnt[b];
        }
        if (g == 0) { out_off[n] = blk[n_blk]; off_writes[n]++; }
    }
}
}  // namespace seqsim
