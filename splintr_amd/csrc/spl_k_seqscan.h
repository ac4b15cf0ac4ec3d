// spl_k_seqscan.h -- the count-scan-write DRIVER of the per-sequence device ops (spl_k_stream.h, spl_k_stop.h): a WAVEFRONT owns
// a sequence and counts the bytes it emits, the counts are scanned into offsets, a wavefront writes.  What a sequence does is the op's.
//
// Two shapes.  n_seqs <= the op's "*_one_max" option (64 by default, at most SEQ_ONE_MAX): ONE launch of one workgroup (seq_one_body: count
// every sequence, scan the counts in LDS, write).  Beyond: seq_len_body (counts into the scratch, their sums per SEQ_BLK sequences),
// k_decode_scan (spl_k_decode.h) over the sums, seq_write_body.  No atomics, no polling, no workgroup waits for another; every offset is
// written exactly once, out_off[n] by the scan (one launch) or by block 0 (three).
//
// An op has Wave (a wavefront's LDS), Carry (what a sequence's count hands its write), count(b, Wave&, Carry&) -> the bytes sequence b emits,
// and write(b, Wave&, const Carry&, o0); every lane of the wavefront calls them.  A keep is where the carries wait between the passes:
// put(b, carry) by lane 0, get(b) by every lane (LDS in the one-launch form, the scratch in the three-launch form; the op chooses the widths).
// The first half is plain C++: tests/hostsim/seqscan_sim.h restates the two drivers over it for the ops' simulators.  The device half
// scans with wave_scan_incl64 (spl_k_merge.h, in front of this file in the kernels' translation unit).
#pragma once
#include "spl_common.h"

namespace spl {

constexpr uint32_t SEQ_BLK = 16;                    // sequences per workgroup of the three-launch form (four per wavefront)
constexpr uint32_t SEQ_NT = 256;                    // lanes per workgroup there
constexpr uint32_t SEQ_ONE_NT = 1024;               // lanes of the one workgroup of the one-launch form
constexpr uint32_t SEQ_ONE_MAX = 1024;              // most sequences the one-launch form can take (its counts are in LDS)
static_assert(SEQ_BLK <= 64, "one wave scan gives a block's starts");

// blocks of the three-launch form: block 0 exists even for no sequence (it writes the closing offset)
SPL_HD uint64_t seq_n_blocks(uint64_t n_seqs) { const uint64_t n = (n_seqs + SEQ_BLK - 1) / SEQ_BLK; return n ? n : 1; }
// an output byte: need may exceed the capacity, and what lies beyond it is counted, not written
SPL_HD void seq_put(uint8_t* __restrict__ out, uint64_t cap, uint64_t o, uint32_t x) { if (o < cap) out[o] = (uint8_t)x; }

#if defined(__HIPCC__)
struct SeqNoCarry {};
struct SeqNoKeep {
    __device__ __forceinline__ void put(uint64_t, const SeqNoCarry&) const {}
    __device__ __forceinline__ SeqNoCarry get(uint64_t) const { return {}; }
};

// ------------------------------------------------------------------------------------------ three launches
// cnt[b]: the bytes sequence b emits; blk[g]: their sum over block g's SEQ_BLK sequences (k_decode_scan scans those).  s_sum: SEQ_NT / 64 words
// (the pointers are the kernels' __restrict__ parameters: said again here it cost k_stream_len / _write four to six SGPR spills, nothing else)
template <class Op, class Keep>
__device__ __forceinline__ void seq_len_body(const Op& op, const Keep& keep, uint64_t n_seqs, uint64_t n_blk, typename Op::Wave* s_wave, uint64_t* s_sum,
                                             uint64_t* cnt, uint64_t* blk) {
    const uint32_t wv = threadIdx.x >> 6;
    for (uint64_t g = blockIdx.x; g < n_blk; g += gridDim.x) {
        uint64_t sum = 0;
        for (uint32_t i = wv; i < SEQ_BLK; i += SEQ_NT / 64) {
            const uint64_t b = g * SEQ_BLK + i;
            if (b >= n_seqs) break;
            typename Op::Carry k;
            const uint64_t c = op.count(b, s_wave[wv], k);
            if ((threadIdx.x & 63) == 0) { cnt[b] = c; keep.put(b, k); }
            sum += c;
        }
        if ((threadIdx.x & 63) == 0) s_sum[wv] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t s = 0;
            for (uint32_t w = 0; w < SEQ_NT / 64; w++) s += s_sum[w];
            blk[g] = s;
        }
        __syncthreads();
    }
}
// blk: the exclusive scan of seq_len_body's sums, the total behind them
template <class Op, class Keep>
__device__ __forceinline__ void seq_write_body(const Op& op, const Keep& keep, uint64_t n_seqs, uint64_t n_blk, typename Op::Wave* s_wave,
                                               const uint64_t* cnt, const uint64_t* blk, uint64_t* out_off) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint64_t g = blockIdx.x; g < n_blk; g += gridDim.x) {
        const uint64_t b_lane = g * SEQ_BLK + lane;
        const uint64_t mine = lane < SEQ_BLK && b_lane < n_seqs ? cnt[b_lane] : 0ull;
        const uint64_t excl = wave_scan_incl64(mine) - mine + blk[g];
        for (uint32_t i = wv; i < SEQ_BLK; i += SEQ_NT / 64) {
            const uint64_t b = g * SEQ_BLK + i;
            if (b >= n_seqs) break;
            const uint64_t o0 = (uint64_t)__shfl((unsigned long long)excl, (int)i);
            op.write(b, s_wave[wv], keep.get(b), o0);
            if (lane == 0) out_off[b] = o0;
        }
        if (g == 0 && threadIdx.x == 0) out_off[n_seqs] = blk[n_blk];
    }
}

// ------------------------------------------------------------------------------------------ one launch (n_seqs <= SEQ_ONE_MAX; s_cnt: one word more)
template <class Op, class Keep>
__device__ __forceinline__ void seq_one_body(const Op& op, const Keep& keep, uint32_t n, typename Op::Wave* s_wave, uint64_t* s_cnt,
                                             uint64_t* out_off) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t b = wv; b < n; b += SEQ_ONE_NT / 64) {
        typename Op::Carry k;
        const uint64_t c = op.count(b, s_wave[wv], k);
        if (lane == 0) { s_cnt[b] = c; keep.put(b, k); }
    }
    __syncthreads();
    if (wv == 0) {
        uint64_t carry = 0;
        for (uint32_t base = 0; base < n; base += 64) {
            const uint64_t v = base + lane < n ? s_cnt[base + lane] : 0ull;
            const uint64_t x = wave_scan_incl64(v);
            if (base + lane < n) s_cnt[base + lane] = carry + x - v;
            carry += (uint64_t)__shfl((unsigned long long)x, 63);
        }
        if (lane == 0) { s_cnt[n] = carry; out_off[n] = carry; }
    }
    __syncthreads();
    for (uint32_t b = wv; b < n; b += SEQ_ONE_NT / 64) {
        const uint64_t o0 = s_cnt[b];
        op.write(b, s_wave[wv], keep.get(b), o0);
        if (lane == 0) out_off[b] = o0;
    }
}
#endif  // __HIPCC__

}  // namespace spl
