// spl_mode.h -- how large a device call may be and which mode it runs in: the three size limits and pick_mode.  Plain C++, nothing of HIP:
// spl_kernels.hip includes it for the limits, spl_launch.h for the choice, tests/hostsim/mode_sim.cpp pins the table on the CPU.
#pragma once
#include <cstdint>

#ifndef SPL_DIRECT_A_MAX_BYTES
#define SPL_DIRECT_A_MAX_BYTES (1280u * 1024u)
#endif
#ifndef SPL_DIRECT_MAX_MB
#define SPL_DIRECT_MAX_MB 256
#endif
#ifndef SPL_QUEUE_MAX_MB
#define SPL_QUEUE_MAX_MB 2047         /* 0: queue mode off (larger batches then run the multi-pass pipeline) */
#endif

namespace spl {

constexpr uint64_t SPL_QUEUE_MAX_BYTES = (uint64_t)SPL_QUEUE_MAX_MB << 20;
constexpr uint64_t SPL_DIRECT_MAX_BYTES = (uint64_t)SPL_DIRECT_MAX_MB << 20;   // batches up to this size: small tiles, tile-owned mode

// How one device call runs.  Tile-owned: every tile finishes its own tokens (k_pretok + k_tile_out, or the one fused launch), in one of two
// geometries of the same window (spl_kernels.hip SPL_TILE_DIRECT_A / _B).  Queue: tile-owned tiles plus global queues for what is long, for
// batches beyond the tile-owned limit; it has no form with special tokens or external boundaries.  force_tile (spl_debug_phases): 0 by
// size, 1 tile-owned, 4 queue mode where it has a form, 5 geometry B at any size; anything else only runs with external boundaries.
enum class TileMode { OwnedA, OwnedB, Queue, Refuse };
inline TileMode pick_mode(int force_tile, bool ext, bool special, uint64_t n_bytes) {
    static_assert(SPL_DIRECT_MAX_BYTES <= SPL_QUEUE_MAX_BYTES, "queue mode takes over where the tile-owned mode ends");
    // (a call without a byte launches no tile at all: forced queue mode would ask for grids of ZERO workgroups -- an invalid launch -- so
    //  it takes the tile-owned branch, which only zeroes the offsets and, for a packed call, queues the pack kernel)
    if (!ext && !special && n_bytes && (force_tile == 4 || (force_tile == 0 && n_bytes > SPL_DIRECT_MAX_BYTES)) && n_bytes <= SPL_QUEUE_MAX_BYTES) return TileMode::Queue;
    const bool known = force_tile == 0 || force_tile == 1 || force_tile == 4 || force_tile == 5;
    if (n_bytes > SPL_DIRECT_MAX_BYTES || !(ext || known)) return TileMode::Refuse;
    return (force_tile == 5 || n_bytes > SPL_DIRECT_A_MAX_BYTES) ? TileMode::OwnedB : TileMode::OwnedA;
}

}  // namespace spl
