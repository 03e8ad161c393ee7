// pitch_plan.h — what pitchbatch.hip uses of the pitch plan of pitch.hip.
#pragma once
#include "common.h"

struct frt_pitch;

namespace frt {

// The frame levels of a track from another source than the rows of x: fill() is called once per track, after the kernels
// that leave estimate and confidence of every frame were enqueued on `stream` and before the gate, and enqueues there
// whatever writes level_db[n_channels][n_frames] (device memory, the dBFS plane of raw).
struct PitchLevelSource {
    int (*fill)(void* ctx, double* level_db, int64_t n_frames, hipStream_t stream);
    void* ctx;
};

// frt_pitch_track (friture_hip.h); with `level` the plan's own level kernels do not run
int pitch_track_with_level(frt_pitch* h, const double* x, int64_t T, int64_t x_stride, double* f0_out, double* raw_out,
                           int64_t* n_frames_out, const PitchLevelSource* level);
void pitch_plan_shape(const frt_pitch* h, int* fft_size, int* hop, int* n_channels);

}  // namespace frt
