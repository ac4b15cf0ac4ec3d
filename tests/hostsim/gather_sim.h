// gather_sim.h -- TEST TOOL: a workgroup's count, played lane by lane.  The cooperative searches of the gather and block kernels
// (col_span_docs of spl_k_collate.h, dd_first_doc of spl_k_decode_dev.h) take "how many lanes hold pred(lane)" as a parameter: one
// barrier in a kernel, this loop in collate_sim.cpp, window_sim.cpp, decode_sim.cpp and spans_sim.cpp -- which thereby run the kernels'
// own searches.  calls (may be null): one more per count, that is per round of a search.
#pragma once
#include <cstdint>

struct LaneCount {
    uint32_t lanes;
    uint64_t* calls;
    template <class Pred> uint32_t operator()(const Pred& pred) const {
        uint32_t cnt = 0;
        for (uint32_t lane = 0; lane < lanes; lane++) cnt += pred(lane) ? 1u : 0u;
        if (calls) ++*calls;
        return cnt;
    }
};
