// mode_sim.cpp -- TEST TOOL: splintr_amd/csrc/spl_mode.h (the size limits of a device call and pick_mode, the code launch_all runs) behind a
// C interface.  Built with g++; no GPU, nothing of HIP.
#include "../../splintr_amd/csrc/spl_mode.h"

extern "C" {

void ms_limits(uint64_t out[3]) { out[0] = SPL_DIRECT_A_MAX_BYTES; out[1] = spl::SPL_DIRECT_MAX_BYTES; out[2] = spl::SPL_QUEUE_MAX_BYTES; }

// 0 tile-owned geometry A, 1 tile-owned geometry B, 2 queue mode, 3 refused
int ms_pick(int force_tile, int ext, int special, uint64_t n_bytes) {
    switch (spl::pick_mode(force_tile, ext != 0, special != 0, n_bytes)) {
        case spl::TileMode::OwnedA: return 0;
        case spl::TileMode::OwnedB: return 1;
        case spl::TileMode::Queue: return 2;
        case spl::TileMode::Refuse: return 3;
    }
    return -1;
}

}  // extern "C"
