// spl_seqscan_host.h -- the host half of the count-scan-write driver (spl_k_seqscan.h): an op's scratch and the call that picks its form.
#pragma once
namespace {

// One call's scratch: blk, the block sums, the total behind them, then arrays of one uint64 per sequence, the counts first.
struct SeqScratch {
    uint64_t n_seqs; uint64_t* blk;
    uint64_t n_blk() const { return seq_n_blocks(n_seqs); }
    uint64_t* per_seq(uint32_t i) const { return blk + n_blk() + 1 + i * n_seqs; }      // 0: the counts; 1 ..: the op's own
};
// grow-only, a quarter more than asked for
int seq_scratch_grow(DevBuf<uint64_t>& buf, uint64_t* cap, uint64_t max_seqs, uint32_t words) {
    const uint64_t need = seq_n_blocks(max_seqs) + 1 + words * max_seqs;
    return buf.grow(cap, need, need + need / 4 + 64);
}
// Up to one_max sequences one() launches the op's one-workgroup kernel; beyond, len(grid, wg) and write(grid, wg) launch its count and write
// kernels on either side of k_decode_scan over the block sums.
template <class One, class Len, class Write>
void seq_launch(const SeqScratch& s, uint64_t one_max, hipStream_t stream, One one, Len len, Write write) {
    if (s.n_seqs <= one_max) { one(); return; }
    const dim3 grid((uint32_t)s.n_blk()), wg(SEQ_NT);            // (n_seqs < 2^31: fewer than 2^27 blocks)
    len(grid, wg);
    hipLaunchKernelGGL(k_decode_scan, dim3(1), dim3(1024), 0, stream, s.blk, s.n_blk());
    write(grid, wg);
}

}  // namespace
