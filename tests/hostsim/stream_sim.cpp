// stream_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_stream.h (the code k_stream_one / k_stream_len /
// k_stream_write run: the role rule, the hold and replace lengths, the chunk walk with its halo, the state transition, the capacity cut)
// evaluated on the CPU sequence by sequence and lane by lane.  The lanes of a wavefront (= the slots of a window) and the bytes of a chunk
// are parameters, so that window and chunk edges can be tested exhaustively at small sizes.  The starts and the staging area are arrays
// guarded by canaries; every write is counted per destination byte, offset and state word.  Built with g++; no GPU.
// -DSPL_STREAM_MUTANT_WIDE_SECOND and -DSPL_STREAM_HALO=2 build the two mutants tests/test_stream_device_cpu.py must see fail.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_k_stream.h"
#include "seqscan_sim.h"

using namespace spl;

namespace {

struct Sink {
    uint8_t* out; uint64_t cap; uint8_t* out_writes;
    uint64_t* out_off; uint8_t* off_writes;
    uint64_t* state_out; uint8_t* state_writes;
    uint64_t canary_damage = 0;
    void put(uint64_t o, uint32_t x) { if (o < cap) { out[o] = (uint8_t)x; out_writes[o]++; } }
};

const uint32_t CANARY = 0xC0FFEE0Du;

// st_seq of the header, restated: one wavefront of `lanes` lanes, chunks of `chunk` bytes
template <bool I64>
uint64_t seq(const StIn& a, const DecTab& t, uint64_t b, uint32_t lanes, uint32_t chunk, bool write, Sink& k, uint64_t o0) {
    uint64_t state = a.state_in[b];
    const uint32_t n_valid = st_row_valid(a, b);
    const bool replace = (a.sflags & ST_REPLACE) != 0;
    uint64_t o = o0;
    std::vector<uint32_t> sbuf(lanes + 4, CANARY), src(lanes + 1, 0);
    uint32_t* start = sbuf.data() + 1;                                // [0 .. lanes + 1], a canary on both sides
    std::vector<uint8_t> stg(chunk + 2 * ST_H + 2, 0xEE);
    uint8_t* stage = stg.data() + 1;
    std::vector<uint32_t> role(chunk);
    std::vector<uint64_t> nb(chunk);
    for (uint64_t k0 = 0; k0 < n_valid; k0 += lanes) {
        uint32_t total = 0;
        const uint32_t c = st_stalled(state) ? 0 : st_count(state), pend = st_pend(state);
        start[0] = 0;
        for (uint32_t lane = 0; lane < lanes; lane++) {
            uint32_t len = 0, s = 0;
            if (k0 + lane < n_valid) len = st_slot_span<I64>(a, t, b, (uint32_t)(k0 + lane), s);
            start[1 + lane] = c + total; src[1 + lane] = s;
            total += len;
        }
        if (total == 0) continue;
        if (st_stalled(state)) { state = st_add_held(state, total); continue; }
        const uint32_t n = c + total;
        start[lanes + 1] = n;
        uint64_t next = 0;
        for (uint32_t p0 = 0; p0 < n; p0 += chunk) {
            for (uint32_t j = 0; j < chunk + 2 * ST_H; j++) {
                uint32_t q;
                stage[j] = st_stage_pos(p0, j, n, q) ? (uint8_t)st_fetch(start, src.data(), t.tok_bytes, lanes + 1, pend, q) : (uint8_t)0;
            }
            uint32_t first = chunk, pend_lane = chunk;
            for (uint32_t lane = 0; lane < chunk; lane++) {
                const uint32_t have = st_nbr(stage, lane, p0, n, nb[lane]);
                role[lane] = p0 + lane < n ? st_role(nb[lane], have) : ST_R_TAIL;
                if (p0 + lane < n && role[lane] >= ST_R_BAD && first == chunk) first = lane;
                if (p0 + lane < n && role[lane] == ST_R_PEND && pend_lane == chunk) pend_lane = lane;
            }
            bool stop = false;
            if (!replace) {
                const uint32_t n_copy = first < n - p0 ? first : n - p0;
                if (write) for (uint32_t lane = 0; lane < n_copy; lane++) k.put(o + lane, (uint32_t)(nb[lane] >> (8 * ST_H)) & 0xFFu);
                o += n_copy;
                if (first < chunk) { next = st_state_at(role[first], nb[first], n - (p0 + first)); stop = true; }
            } else {
                for (uint32_t lane = 0; lane < chunk; lane++) {
                    const uint32_t l = role[lane] & 3u;
                    if (write) {
                        if (l == 1) k.put(o, (uint32_t)(nb[lane] >> (8 * ST_H)) & 0xFFu);
                        else if (l == 3) { k.put(o, 0xEF); k.put(o + 1, 0xBF); k.put(o + 2, 0xBD); }
                    }
                    o += l;
                }
                if (pend_lane < chunk) next = st_state_at(role[pend_lane], nb[pend_lane], n - (p0 + pend_lane));
            }
            if (stg.front() != 0xEE || stg.back() != 0xEE) k.canary_damage++;
            if (stop) break;
        }
        state = next;
        if (sbuf.front() != CANARY || sbuf[lanes + 3] != CANARY) k.canary_damage++;
    }
    if (st_final(a, b) && !st_stalled(state) && st_count(state)) {
        if (write) { k.put(o, 0xEF); k.put(o + 1, 0xBF); k.put(o + 2, 0xBD); }
        o += 3;
        state = 0;
    }
    if (write) { k.state_out[b] = state; k.state_writes[b]++; }
    return o - o0;
}

struct NoCarry {};

// the driver (seqscan_sim.h) over seq
template <bool I64>
int run(const StIn& a, const DecTab& t, uint32_t lanes, uint32_t chunk, int three, Sink& k) {
    seqsim::run<NoCarry>(a.n_seqs, three, k.out_off, k.off_writes,
                         [&](uint64_t b, NoCarry&) { return seq<I64>(a, t, b, lanes, chunk, false, k, 0); },
                         [&](uint64_t b, const NoCarry&, uint64_t o0) { seq<I64>(a, t, b, lanes, chunk, true, k, o0); });
    return 0;
}

}  // namespace

extern "C" {

void ss_geometry(uint32_t out[7]) { out[0] = ST_WAVE; out[1] = ST_H; out[2] = SEQ_BLK; out[3] = ST_ONE_DEFAULT; out[4] = ST_NT; out[5] = ST_ONE_NT; out[6] = ST_ONE_MAX; }

int ss_step(const void* ids, const int32_t* len, const uint8_t* fin, const uint64_t* state_in, uint64_t n_seqs, uint32_t row_len, uint32_t dflags,
            uint32_t sflags, const uint32_t* tok_off, const uint8_t* tok_bytes, uint32_t max_id, const uint32_t* sp_ids, const uint32_t* sp_off,
            uint32_t n_sp, const uint32_t* sp_bits, uint32_t lanes, uint32_t chunk, int three, uint8_t* out, uint64_t cap, uint64_t* out_off,
            uint64_t* state_out, uint8_t* out_writes, uint8_t* off_writes, uint8_t* state_writes, uint64_t* stats) {
    if (lanes == 0 || chunk == 0 || row_len == 0) return -1;
    StIn a{};
    a.ids = ids; a.len = len; a.fin = fin; a.state_in = state_in; a.n_seqs = n_seqs; a.row_len = row_len; a.dflags = dflags; a.sflags = sflags;
    const DecTab t{tok_off, tok_bytes, max_id, sp_ids, sp_off, n_sp, sp_bits};
    Sink k{out, cap, out_writes, out_off, off_writes, state_out, state_writes};
    const int rc = (dflags & DD_I64) ? run<true>(a, t, lanes, chunk, three, k) : run<false>(a, t, lanes, chunk, three, k);
    stats[0] = k.canary_damage;
    return rc;
}

}  // extern "C"
