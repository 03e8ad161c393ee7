// pitchbatch.hip — the pitch tracker widget's chain over whole recordings (PitchTrackerWidget.handle_new_data / update_curve,
// friture/pitch_tracker.py:109-119, around PitchTracker.update / estimate_pitch, :313-428) for gfx950: what pitch.hip leaves
// open for S streams of one or two rows seen chunk by chunk.  float64 arithmetic; built with -ffp-contract=off.
//
//   level    The gate's level of a frame is the RMS over EVERY row of it (:404-407, `np.sqrt(np.mean(frame**2))` on the [rows, N]
//            frame): 20 log10(sqrt(sum over rows and samples of x^2 / (rows N)) + eps).  The samples are tail || x per row (the
//            tail: what an earlier call received and no frame consumed, float64; x: float32 or float64, widened exactly).  Where
//            the hop divides the frame, overlapping frames share hop-sized blocks: rows_block_energy_kernel forms the sum of
//            squares of every (stream, row, block) once, one wavefront each, and rows_level_from_blocks_kernel adds a frame's
//            blocks; any other hop: rows_level_kernel, one wavefront per frame.  For one row these are operation for operation
//            the level kernels of pitch.hip.  The gate itself is pitch_gate_kernel of pitch.hip, unchanged, on that level.
//   read-out A refresh shows the latest estimate and the last M estimates on the OctaveC axis, flipped and clipped
//            (coordinateTransform.py:73-83 with length 1, borders 0).  The transform is pointwise: pitch_axis_kernel maps every
//            entry of history || estimates once (and leaves the next history and the per-refresh pitch), pitch_curve_kernel
//            copies the windows that were asked for.
#include <cmath>
#include <limits>

#include "common.h"
#include "pitch_device.h"
#include "pitch_plan.h"
#include "widget_device.h"

namespace frt {
namespace {

constexpr int kThreads = 256;

struct RowsSource {
    const void* x;              // [streams][rows] rows of T samples: x[s * ld_stream + row * ld_row + t]
    const double* tail;         // [streams][rows][pending]
    long long ld_stream, ld_row, pending;
    int streams, rows;
};

// sample i of tail || x of one row
template <bool kF64>
__device__ __forceinline__ double row_sample(const RowsSource& p, int s, int row, long long i) {
    if (i < p.pending) return p.tail[((long long)s * p.rows + row) * p.pending + i];
    return load_real<kF64>(p.x, (long long)s * p.ld_stream + (long long)row * p.ld_row + (i - p.pending));
}

// eb[(s * rows + row) * n_blocks + b] = sum of squares of samples [b * hop, (b + 1) * hop).  One wavefront per block.
template <bool kF64>
__global__ void __launch_bounds__(kThreads) rows_block_energy_kernel(const RowsSource p, int hop, long long n_blocks,
                                                                    double* __restrict__ eb) {
    const int lane = threadIdx.x & 63;
    const long long gb = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gb >= n_blocks * p.streams * p.rows) return;
    const int sr = (int)(gb / n_blocks);
    const long long b = gb - (long long)sr * n_blocks;
    const int s = sr / p.rows, row = sr - s * p.rows;
    double e = 0.0;
    for (int n = lane; n < hop; n += 64) {
        const double v = row_sample<kF64>(p, s, row, b * hop + n);
        e += v * v;
    }
    e = wave_sum(e);
    if (lane == 0) eb[gb] = e;
}

// frame f of stream s covers blocks f .. f + per_frame - 1 of each of its rows
__global__ void __launch_bounds__(kThreads) rows_level_from_blocks_kernel(const double* __restrict__ eb, long long n_blocks,
                                                                         int per_frame, int streams, int rows, int N, long long F,
                                                                         double* __restrict__ level) {
    const long long gf = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gf >= (long long)streams * F) return;
    const int s = (int)(gf / F);
    const long long f = gf - (long long)s * F;
    double e = 0.0;
    for (int j = 0; j < per_frame; ++j)
        for (int row = 0; row < rows; ++row) e += eb[((long long)s * rows + row) * n_blocks + f + j];
    level[gf] = level_db(e, (double)rows * (double)N);
}

// any hop: one wavefront per frame
template <bool kF64>
__global__ void __launch_bounds__(kThreads) rows_level_kernel(const RowsSource p, int N, int hop, long long F,
                                                             double* __restrict__ level) {
    const int lane = threadIdx.x & 63;
    const long long gf = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gf >= (long long)p.streams * F) return;
    const int s = (int)(gf / F);
    const long long f = gf - (long long)s * F;
    double e = 0.0;
    for (int row = 0; row < p.rows; ++row)
        for (int n = lane; n < N; n += 64) {
            const double v = row_sample<kF64>(p, s, row, f * hop + n);
            e += v * v;
        }
    e = wave_sum(e);
    if (lane == 0) level[gf] = level_db(e, (double)p.rows * (double)N);
}

struct LevelCall {
    RowsSource src;
    int dtype, N, hop;
    double* eb;                 // [streams][rows][n_frames + N / hop - 1], or null: the hop does not divide the frame
};

int fill_level(void* ctx, double* level, int64_t F, hipStream_t stream) {
    const LevelCall& c = *static_cast<const LevelCall*>(ctx);
    const long long frames = (long long)c.src.streams * F;
    if (c.eb) {
        const int per_frame = c.N / c.hop;
        const long long n_blocks = F + per_frame - 1;
        const dim3 grid((unsigned)((n_blocks * c.src.streams * c.src.rows + 3) / 4));
        if (c.dtype)
            hipLaunchKernelGGL(rows_block_energy_kernel<true>, grid, dim3(kThreads), 0, stream, c.src, c.hop, n_blocks, c.eb);
        else
            hipLaunchKernelGGL(rows_block_energy_kernel<false>, grid, dim3(kThreads), 0, stream, c.src, c.hop, n_blocks, c.eb);
        hipLaunchKernelGGL(rows_level_from_blocks_kernel, dim3((unsigned)((frames + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           stream, c.eb, n_blocks, per_frame, c.src.streams, c.src.rows, c.N, (long long)F, level);
    } else {
        const dim3 grid((unsigned)((frames + 3) / 4));
        if (c.dtype)
            hipLaunchKernelGGL(rows_level_kernel<true>, grid, dim3(kThreads), 0, stream, c.src, c.N, c.hop, (long long)F, level);
        else
            hipLaunchKernelGGL(rows_level_kernel<false>, grid, dim3(kThreads), 0, stream, c.src, c.N, c.hop, (long long)F, level);
    }
    FRT_HIP_CHECK(hipGetLastError());
    return FRT_OK;
}

struct AxisParams {
    long long F, M, R;
    double trans_min, trans_span;       // log2(min_freq), log2(max_freq) - log2(min_freq)
};

// Per stream, index i walks history || estimates (M + F entries) and then the R refreshes:
//   y[i] = clip(1 - (log2(fmax(v, 1e-20)) - trans_min) / trans_span, 0, 1)     fmax ignores NaN: unvoiced and the zeros before the
//                                                                              first frame sit at 1, and y never holds a NaN
//   history_out = the last M entries;  pitch[r] = estimates[frame_start[r + 1] - 1]
__global__ void __launch_bounds__(kThreads) pitch_axis_kernel(const double* __restrict__ est, const double* __restrict__ history_in,
                                                              const long long* __restrict__ frame_start, AxisParams p,
                                                              double* __restrict__ y, double* __restrict__ history_out,
                                                              double* __restrict__ pitch) {
    const int s = blockIdx.y;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long n = p.M + p.F;
    if (i < n) {
        const double v = i < p.M ? history_in[s * p.M + i] : est[s * p.F + (i - p.M)];
        y[s * n + i] = axis_value(v, p.trans_min, p.trans_span);
        if (i >= p.F) history_out[s * p.M + (i - p.F)] = v;
    } else if (i < n + p.R) {
        const long long r = i - n;
        pitch[s * p.R + r] = est[s * p.F + frame_start[r + 1] - 1];
    }
}

// curve[s][ro][m] = y[s][frame_start[r + 1] + m]: the M entries that end at the refresh's last frame (r = ro, or the last
// refresh alone when only that one is kept; without any refresh, the history as it stands)
__global__ void __launch_bounds__(kThreads) pitch_curve_kernel(const double* __restrict__ y, const long long* __restrict__ frame_start,
                                                               AxisParams p, long long Ro, long long total,
                                                               double* __restrict__ curve) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= total) return;
    const long long m = g % p.M, sro = g / p.M;
    const long long s = sro / Ro, ro = sro - s * Ro;
    const long long r = Ro == p.R ? ro : p.R - 1;
    const long long first = p.R ? frame_start[r + 1] : 0;
    curve[g] = y[s * (p.M + p.F) + first + m];
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" int frt_pitch_track_rows(frt_pitch* h, const double* row0, int64_t row0_stride, const void* x, int dtype, int rows,
                                    int64_t T, int64_t ld_stream, int64_t ld_row, const double* tail, int64_t pending,
                                    double* f0_out, double* raw_out, int64_t* n_frames_out) {
    FRT_REQUIRE(h, "frt_pitch_track_rows: null handle");
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_pitch_track_rows: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(rows == 1 || rows == 2, "frt_pitch_track_rows: %d rows per stream (1, or 2 for dual channels)", rows);
    FRT_REQUIRE(T >= 0 && pending >= 0, "frt_pitch_track_rows: T %lld, pending %lld", (long long)T, (long long)pending);
    int N, hop, streams;
    pitch_plan_shape(h, &N, &hop, &streams);
    const int64_t L = pending + T;
    const int64_t F = frt_pitch_frames_for(h, L);
    if (n_frames_out) *n_frames_out = F;
    if (F == 0) return FRT_OK;
    FRT_REQUIRE(row0 && x && f0_out && (tail || pending == 0), "frt_pitch_track_rows: null buffer");
    FRT_REQUIRE((rows == 1 || ld_row >= T) && (streams == 1 || ld_stream >= (rows - 1) * ld_row + T) && row0_stride >= L,
                "frt_pitch_track_rows: strides (row0 %lld, stream %lld, row %lld) for %lld + %lld samples", (long long)row0_stride,
                (long long)ld_stream, (long long)ld_row, (long long)pending, (long long)T);
    FRT_REQUIRE(is_device_pointer(row0) && is_device_pointer(x) && is_device_pointer(f0_out) && (!tail || is_device_pointer(tail)) &&
                    (!raw_out || is_device_pointer(raw_out)),
                "frt_pitch_track_rows: every buffer is device memory");

    LevelCall lc{};
    lc.src = RowsSource{x, tail, (long long)ld_stream, (long long)ld_row, (long long)pending, streams, rows};
    lc.dtype = dtype;
    lc.N = N;
    lc.hop = hop;
    const bool blocks = N % hop == 0 && N / hop >= 2;
    StageCall call;
    call.add_in(x, 0);                                  // device memory: the call runs on the null stream
    const int ieb = blocks ? call.add_scratch((size_t)streams * rows * (size_t)(F + N / hop - 1) * sizeof(double)) : -1;
    int rc = call.begin();
    if (rc) return rc;
    lc.eb = blocks ? call.ptr<double>(ieb) : nullptr;
    if ((rc = frt_pitch_set_stream(h, call.stream()))) return rc;
    const PitchLevelSource level{fill_level, &lc};
    if ((rc = pitch_track_with_level(h, row0, L, row0_stride, f0_out, raw_out, nullptr, &level))) return rc;
    return call.finish();
}

extern "C" int frt_pitch_refresh(const double* estimates, int streams, int64_t n_frames, const int64_t* frame_start,
                                 int64_t n_refresh, const double* history_in, int64_t history_length, double min_freq,
                                 double max_freq, int keep_last, double* history_out, double* pitch_out, double* curve_out) {
    FRT_REQUIRE(streams >= 1 && streams <= 65535 && n_frames >= 0 && n_refresh >= 0 && history_length >= 1,
                "frt_pitch_refresh: %d streams x %lld frames, %lld refreshes, history of %lld", streams, (long long)n_frames,
                (long long)n_refresh, (long long)history_length);
    FRT_REQUIRE(min_freq > 0 && max_freq > min_freq, "frt_pitch_refresh: axis range [%g, %g]", min_freq, max_freq);
    if (n_refresh == 0 && !keep_last) return FRT_OK;
    FRT_REQUIRE(frame_start && !is_device_pointer(frame_start), "frt_pitch_refresh: frame_start must be host memory");
    FRT_REQUIRE(frame_start[0] == 0 && frame_start[n_refresh] == n_frames, "frt_pitch_refresh: frame_start [%lld, %lld] does not span [0, %lld]",
                (long long)frame_start[0], (long long)frame_start[n_refresh], (long long)n_frames);
    for (int64_t r = 0; r < n_refresh; ++r)      // every refresh completes a frame: frame_start[r + 1] - 1 >= 0
        FRT_REQUIRE(frame_start[r + 1] > frame_start[r], "frt_pitch_refresh: frame_start does not increase at %lld", (long long)r);
    FRT_REQUIRE((estimates || n_frames == 0) && history_in && history_out && (pitch_out || n_refresh == 0) && curve_out &&
                    history_in != history_out,
                "frt_pitch_refresh: null buffer, or the history updated in place");
    FRT_REQUIRE((n_frames == 0 || is_device_pointer(estimates)) && is_device_pointer(history_in) && is_device_pointer(history_out) &&
                    (n_refresh == 0 || is_device_pointer(pitch_out)) && is_device_pointer(curve_out),
                "frt_pitch_refresh: estimates, histories and outputs are device memory");
    const int64_t Ro = keep_last ? 1 : n_refresh;
    const long long total = (long long)streams * Ro * history_length;
    FRT_REQUIRE(total / kThreads < 0x7fffffffll, "frt_pitch_refresh: %lld curve values in one call", total);

    AxisParams p{};
    p.F = n_frames;
    p.M = history_length;
    p.R = n_refresh;
    p.trans_min = std::log2(min_freq);
    p.trans_span = std::log2(max_freq) - p.trans_min;
    const size_t n = (size_t)(p.M + p.F);
    std::vector<long long> fs(frame_start, frame_start + n_refresh + 1);
    StageCall call;
    call.add_in(history_in, 0);                         // device memory: the call runs on the null stream
    const int ifs = call.add_in(fs.data(), fs.size() * sizeof(long long));
    const int iy = call.add_scratch((size_t)streams * n * sizeof(double));
    int rc = call.begin();
    if (rc) return rc;
    const hipStream_t stream = call.stream();
    hipLaunchKernelGGL(pitch_axis_kernel, dim3((unsigned)((n + p.R + kThreads - 1) / kThreads), (unsigned)streams), dim3(kThreads), 0,
                       stream, estimates, history_in, call.ptr<const long long>(ifs), p, call.ptr<double>(iy), history_out, pitch_out);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pitch_curve_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       call.ptr<const double>(iy), call.ptr<const long long>(ifs), p, (long long)Ro, total, curve_out);
    FRT_HIP_CHECK(hipGetLastError());
    return call.finish();
}
