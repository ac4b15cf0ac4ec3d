// spl_streams.h -- the stream probe: two tiny kernels and pick_stream_beside, which MEASURES which new stream runs beside given busy ones.
// It creates and discards candidate streams itself and hands the winner out raw (the caller's Stream owner, or spl_pick_stream's caller,
// takes it).  Needs HIP_TRY and mono_us (spl_host_res.h).
#pragma once
namespace {

// ---- streams that really run side by side -----------------------------------------------------------------------------------------------
// HIP gives a stream a hardware queue of its own only up to GPU_MAX_HW_QUEUES per priority (4 by default; streams beyond share one and run
// one behind the other), and the n-th hardware queue a process creates sits on pipe n mod 4 of the command processor: two busy queues on one
// pipe take turns -- every kernel of either waits tens of microseconds (kernel traces: profiles/r05_wave_exchange.txt, r05_host_pipeline.txt).
// Which queue a stream gets depends on what else the process has created; the API neither tells nor sets it.  It can be MEASURED: a kernel
// that spins for 150 us on one stream, a few empty kernels on the other -- 14 us until they are through when the two run side by side, 22 - 55
// on one pipe, 165 in one queue (tools/dev/queue_probe.hip).  The pipeline's streams are picked that way, once per context.
__global__ void k_probe_spin(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) { }
}
__global__ void k_probe_nop() { }
double probe_us(hipStream_t spin, hipStream_t other) {       // `spin` busy, four empty kernels on `other`: us until they are through (min of 3; spin null: alone)
    double best = 1e30;
    for (int rep = 0; rep < 3; rep++) {
        if (spin) (void)hipStreamSynchronize(spin);
        (void)hipStreamSynchronize(other);
        if (spin) hipLaunchKernelGGL(k_probe_spin, dim3(8), dim3(64), 0, spin, 12000ull);       // wall_clock64: 100 MHz
        const double t0 = mono_us();
        for (int k = 0; k < 4; k++) hipLaunchKernelGGL(k_probe_nop, dim3(1), dim3(64), 0, other);
        (void)hipStreamSynchronize(other);
        best = std::min(best, mono_us() - t0);
        if (spin) (void)hipStreamSynchronize(spin);
    }
    return best;
}
// A new stream that runs beside every stream of `busy` (each of which may be the one that is busy): up to 12 candidates over the three
// priorities (a priority has queues of its own); the first without a conflict, else the least bad.  *conflict_us: what was left.
int pick_stream_beside(const std::vector<hipStream_t>& busy, hipStream_t* out, double* conflict_us) {
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    hipStream_t best_s = nullptr;
    double best_v = 1e30;
    for (int k = 0; k < 12; k++) {
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, k % 3 == 0 ? 0 : (k % 3 == 1 ? hi : lo)));
        hipLaunchKernelGGL(k_probe_nop, dim3(1), dim3(64), 0, s);            // (its queue is created with its first use)
        (void)hipStreamSynchronize(s);
        const double alone = probe_us(nullptr, s);
        double worst = 0;
        for (hipStream_t b : busy) worst = std::max(worst, std::max(probe_us(b, s), probe_us(s, b)) - alone);
        if (worst < best_v) { if (best_s) (void)hipStreamDestroy(best_s); best_s = s; best_v = worst; }
        else (void)hipStreamDestroy(s);
        if (best_v < 5.0) break;
    }
    *out = best_s;
    if (conflict_us) *conflict_us = best_v;
    return SPL_OK;
}
}  // namespace
