// pitch_plan.h — what pitchbatch.hip and pitchstream.hip use of the pitch plan of pitch.hip.
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

// The front of the chain for a few frames of a ONE-channel plan, for the live chain: what it leaves on the device.
struct PitchLiveView {
    const double* s;            // [frames / 8][Lp][8]: S of frame f, grid row l at s[((f / 8) * Lp + l) * 8 + f % 8]; rows L .. Lp are 0
    double* strength;           // [frames][Kp]
    const double* kt;           // [Lp + 4][Kp]: the kernel matrix transposed, zero padded
    const double* freqs;        // [L]
    const int* lrange;          // [Kp / cand_per_range][2]: grid rows [begin, end) outside which that range of candidates is all zero
    int N, hop, L, Lp, K, Kp, cand_per_range;
};
// x: span = fft_size + (n_frames - 1) * hop float64 samples on the device.  Puts the plan on `stream`, runs the transform
// (frt_stft_run: the instance follows from the alignment of x and x_stride) and the log-grid kernel of frt_pitch_track, with its
// summation order; the strengths are then either the caller's own kernel's or pitch_live_strength_tiled's.
int pitch_live_front(frt_pitch* h, const double* x, int64_t span, int64_t x_stride, int64_t n_frames, hipStream_t stream,
                     PitchLiveView* view);
// pitch_strength_kernel, the tiled product of frt_pitch_track, over the frames of the last pitch_live_front
int pitch_live_strength_tiled(frt_pitch* h, int64_t n_frames);

}  // namespace frt
