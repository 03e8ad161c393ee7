// pitchstream.hip — the pitch tracker's live chain (PitchTracker.update / estimate_pitch, friture/pitch_tracker.py:313-428, and what
// PitchTrackerWidget.handle_new_data / update_curve, :109-119, leave in the view model) for gfx950: one stream of one or two rows,
// one to a few frames per call, the gate's previous estimate, the estimate history and the curve resident on the device.
// float64 arithmetic; built with -ffp-contract=off.
//
// A push is: the span of samples that completes F frames through page-locked memory (every row widened to float64, rows on
// 16-byte boundaries: the transform instance PitchBatch uses), frt_stft_run and the log-grid kernel of pitch.hip
// (pitch_live_front), then
//   live_energy_kernel    sums of squares over every row, in the order of pitchbatch.hip's level kernels: per hop-sized block
//                         where the hop divides the frame (a frame adds its blocks later), else per frame; a wavefront each
//   live_strength_kernel  strengths = kernels x S for few frames: a lane owns ONE candidate of one frame and walks the grid once,
//                         acc = fma(kt[l][c], S[l], acc) in ascending l — the operation sequence pitch_strength_kernel applies
//                         to a candidate, so the bits are its bits (rows outside the candidate block's band hold exact zeros on
//                         either route).  The chain of ~1000 dependent FMAs is the serial part; the loads of a wavefront are one
//                         contiguous 512-byte row of the transposed matrix and one broadcast value of S, 16 rows per batch,
//                         the next batch in flight while the current one is consumed.  Above `crossover` frames
//                         pitch_strength_kernel takes over (pitch_live_strength_tiled): it reads the matrix once per 8 frames.
//   live_finish_kernel    ONE workgroup: arg-max + parabola per frame (a wavefront per frame, pitch_device.h), the frame levels,
//                         the gate with its carried state (sequential, one thread), the history shift and the curve.
// and one copy back (estimates, latest estimate, curve) behind one synchronisation.  Everything runs on the null stream.
#include <cmath>
#include <limits>

#include "common.h"
#include "pitch_device.h"
#include "pitch_plan.h"

namespace frt {
namespace {

constexpr int kThreads = 256;
constexpr int kLiveBatch = 16;              // grid rows per batch of loads in live_strength_kernel
constexpr int kDefaultCrossover = 16;       // frames per push up to which live_strength_kernel runs (DESIGN T1, live chain)
constexpr int kMaxCrossover = 1024;
constexpr long long kMaxFrames = 1 << 20;

// unit u < units: per_row — (row, block) = (u / per, u % per), `len` samples of that row from block * advance on;
// otherwise frame u: `len` samples from u * advance on of EVERY row, one accumulator (rows_level_kernel's order)
__global__ void __launch_bounds__(kThreads) live_energy_kernel(const double* __restrict__ x, long long stride, int rows, int len,
                                                               int advance, long long per, bool per_row, long long units,
                                                               double* __restrict__ energy) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= units) return;
    const int r0 = per_row ? (int)(u / per) : 0, r1 = per_row ? r0 + 1 : rows;
    const long long i = per_row ? u - (long long)r0 * per : u;
    double e = 0.0;
    for (int row = r0; row < r1; ++row) {
        const double* xs = x + row * stride + i * advance;
        for (int n = lane; n < len; n += 64) {
            const double v = xs[n];
            e += v * v;
        }
    }
    e = wave_sum(e);
    if (lane == 0) energy[u] = e;
}

// One wavefront = 64 candidates of one frame (grid: Kp / 64 x frames).  Rows are fetched clamped — the matrix to its zero row Lp,
// S to its last row — so the look-ahead and the batch that straddles the band's end stay in bounds and contribute exact zeros.
__global__ void __launch_bounds__(64) live_strength_kernel(const double* __restrict__ kt, const double* __restrict__ s,
                                                           double* __restrict__ strength, const int* __restrict__ lrange, int Lp,
                                                           int Kp, int cand_per_range) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int f = blockIdx.y;
    const int range = blockIdx.x * 64 / cand_per_range;
    const int l_begin = lrange[2 * range], l_end = lrange[2 * range + 1];           // 0 <= begin <= end <= Lp
    const double* __restrict__ sf = s + (long long)(f >> 3) * Lp * 8 + (f & 7);
    const double* __restrict__ kc = kt + c;
    struct Batch {
        double k[kLiveBatch], v[kLiveBatch];
    };
    auto fetch = [&](int l, Batch& b) {
#pragma unroll
        for (int u = 0; u < kLiveBatch; ++u) {
            const int lk = min(l + u, Lp), ls = min(l + u, Lp - 1);
            b.k[u] = kc[(long long)lk * Kp];
            b.v[u] = sf[(long long)ls * 8];
        }
    };
    double acc = 0.0;
    auto use = [&](const Batch& b) {
#pragma unroll
        for (int u = 0; u < kLiveBatch; ++u) acc = __builtin_fma(b.k[u], b.v[u], acc);
    };
    constexpr int kLgkm0 = 0xC07F;         // s_waitcnt lgkmcnt(0), vmcnt / expcnt untouched
    if (l_begin < l_end) {
        Batch a, b;
        fetch(l_begin, a);
        for (int l = l_begin; l < l_end; l += 2 * kLiveBatch) {
            // The values of S are wave-uniform and come through scalar loads, which return out of order: any use needs
            // lgkmcnt(0).  As in pitch_strength_kernel it is placed by hand BEFORE the next batch is requested, where only the
            // current batch is outstanding (and has had a whole batch of FMAs to arrive), not before the first use, where it
            // would drain the look-ahead as well.  sched_barrier: keep the machine scheduler from sinking the look-ahead
            // loads down to their first use.
            __builtin_amdgcn_s_waitcnt(kLgkm0);
            fetch(l + kLiveBatch, b);
            __builtin_amdgcn_sched_barrier(0);
            use(a);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(kLgkm0);
            fetch(l + 2 * kLiveBatch, a);
            __builtin_amdgcn_sched_barrier(0);
            use(b);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    strength[(long long)f * Kp + c] = acc;
}

struct FinishArgs {
    const double* strength;     // [F][Kp]
    const double* freqs;        // [L]
    const double* energy;       // [rows][n_blocks] (per_frame blocks to a frame) or [F] (per_frame == 0)
    double* raw;                // [3][F] scratch: estimate before the gate, confidence, dBFS
    double* prev;               // [1] the gate's carried estimate, NaN = none
    const double* history_in;   // [M]
    double* history_out;        // [M] (another buffer)
    double* out;                // [F] gated estimates, [1] the latest, [M] the curve
    long long F, M, n_blocks;
    int K, Kp, L, N, rows, per_frame;
    double min_db, conf, p_delta, trans_min, trans_span;
};

__global__ void __launch_bounds__(kThreads) live_finish_kernel(const FinishArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long f = wave; f < a.F; f += kThreads / 64) {
        const double* st = a.strength + f * a.Kp;
        double best;
        int bi;
        pick_argmax(st, a.K, lane, best, bi);
        if (lane != 0) continue;
        a.raw[0 * a.F + f] = pick_frequency(st, bi, a.K, a.L, a.freqs);
        a.raw[1 * a.F + f] = pick_confidence(best);
        double e = 0.0;
        if (a.per_frame) {              // rows_level_from_blocks_kernel's order: blocks outside, rows inside
            for (int j = 0; j < a.per_frame; ++j)
                for (int row = 0; row < a.rows; ++row) e += a.energy[row * a.n_blocks + f + j];
        } else {
            e = a.energy[f];
        }
        a.raw[2 * a.F + f] = level_db(e, (double)a.rows * (double)a.N);
    }
    __syncthreads();
    if (threadIdx.x == 0) {             // pitch_gate_kernel's recurrence, frame after frame
        const double carried = a.prev[0];
        const double nan = std::numeric_limits<double>::quiet_NaN();
        bool v = carried == carried;
        double last = carried;
        for (long long f = 0; f < a.F; ++f) {
            const GateFrame g = gate_frame(a.raw, 1, a.F, 0, f, f ? a.raw[f - 1] : carried, a.min_db, a.conf, a.p_delta);
            v = g.ok && (!v || g.jump_ok);
            last = v ? g.f0 : nan;
            a.out[f] = last;
        }
        a.prev[0] = last;
        a.out[a.F] = last;
    }
    __syncthreads();
    // the last M entries of history || estimates: the next history, and on the axis the curve (pitch_axis_kernel's read-out)
    for (long long i = threadIdx.x; i < a.M; i += kThreads) {
        const long long j = i + a.F;
        const double v = j < a.M ? a.history_in[j] : a.out[j - a.M];
        a.history_out[i] = v;
        a.out[a.F + 1 + i] = axis_value(v, a.trans_min, a.trans_span);
    }
}

}  // namespace
}  // namespace frt

using namespace frt;

struct frt_pitch_live {
    frt_pitch* plan = nullptr;          // not owned
    int N = 0, hop = 0, crossover = kDefaultCrossover, current = 0;
    long long M = 0;
    double trans_min = 0, trans_span = 0;
    DeviceBuffer prev, history, in, energy, raw, out;       // history: [2][M], `current` holds the state
    PinnedBuffer pin_in, pin_out;       // reserved only between pushes: every push ends in a synchronisation
};

extern "C" void frt_pitch_live_destroy(frt_pitch_live* h) {
    if (!h) return;
    DeviceBuffer* bufs[] = {&h->prev, &h->history, &h->in, &h->energy, &h->raw, &h->out};
    for (auto* b : bufs) b->release();
    h->pin_in.release();
    h->pin_out.release();
    delete h;
}

extern "C" int frt_pitch_live_reset(frt_pitch_live* h) {
    FRT_REQUIRE(h, "frt_pitch_live_reset: null handle");
    const double none = std::numeric_limits<double>::quiet_NaN();
    FRT_HIP_CHECK(hipMemcpy(h->prev.ptr, &none, sizeof(double), hipMemcpyHostToDevice));
    FRT_HIP_CHECK(hipMemset(h->history.ptr, 0, 2 * (size_t)h->M * sizeof(double)));
    FRT_HIP_CHECK(hipStreamSynchronize(nullptr));
    h->current = 0;
    return FRT_OK;
}

extern "C" int frt_pitch_live_create(frt_pitch_live** out, frt_pitch* plan, int64_t history_length, double min_freq,
                                     double max_freq) {
    FRT_REQUIRE(out, "frt_pitch_live_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(plan, "frt_pitch_live_create: null plan");
    FRT_REQUIRE(history_length >= 1 && history_length <= (1ll << 24), "frt_pitch_live_create: history of %lld", (long long)history_length);
    FRT_REQUIRE(min_freq > 0 && max_freq > min_freq, "frt_pitch_live_create: axis range [%g, %g]", min_freq, max_freq);
    int N, hop, channels;
    pitch_plan_shape(plan, &N, &hop, &channels);
    FRT_REQUIRE(channels == 1, "frt_pitch_live_create: a plan of %d channels (one stream wants one)", channels);
    frt_pitch_live* h = new frt_pitch_live();
    h->plan = plan;
    h->N = N;
    h->hop = hop;
    h->M = history_length;
    h->trans_min = std::log2(min_freq);
    h->trans_span = std::log2(max_freq) - h->trans_min;
    int rc;
    if ((rc = h->prev.reserve(sizeof(double))) || (rc = h->history.reserve(2 * (size_t)h->M * sizeof(double))) ||
        (rc = frt_pitch_live_reset(h))) {
        frt_pitch_live_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" int frt_pitch_live_set_crossover(frt_pitch_live* h, int frames) {
    FRT_REQUIRE(h && frames >= 0 && frames <= kMaxCrossover, "frt_pitch_live_set_crossover: %d frames (0 .. %d)", frames, kMaxCrossover);
    h->crossover = frames;
    return FRT_OK;
}

extern "C" int frt_pitch_live_crossover(const frt_pitch_live* h) { return h ? h->crossover : kDefaultCrossover; }

extern "C" int frt_pitch_live_get_state(frt_pitch_live* h, double* previous, double* history) {
    FRT_REQUIRE(h && previous && history, "frt_pitch_live_get_state: null argument");
    FRT_HIP_CHECK(hipMemcpy(previous, h->prev.ptr, sizeof(double), hipMemcpyDefault));
    FRT_HIP_CHECK(hipMemcpy(history, h->history.as<double>() + h->current * h->M, (size_t)h->M * sizeof(double), hipMemcpyDefault));
    return FRT_OK;
}

extern "C" int frt_pitch_live_set_state(frt_pitch_live* h, const double* previous, const double* history) {
    FRT_REQUIRE(h && previous && history, "frt_pitch_live_set_state: null argument");
    FRT_HIP_CHECK(hipMemcpy(h->prev.ptr, previous, sizeof(double), hipMemcpyDefault));
    FRT_HIP_CHECK(hipMemcpy(h->history.as<double>() + h->current * h->M, history, (size_t)h->M * sizeof(double), hipMemcpyDefault));
    return FRT_OK;
}

extern "C" int frt_pitch_live_push(frt_pitch_live* h, const void* x, int dtype, int rows, int64_t span, int64_t ld_row, double min_db,
                                   double conf, double p_delta, double* estimates_out, double* latest_out, double* curve_out,
                                   int64_t* n_frames_out) {
    FRT_REQUIRE(h, "frt_pitch_live_push: null handle");
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_pitch_live_push: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(rows == 1 || rows == 2, "frt_pitch_live_push: %d rows (1, or 2 for dual channels)", rows);
    const int N = h->N, hop = h->hop;
    FRT_REQUIRE(span >= N && (span - N) % hop == 0, "frt_pitch_live_push: a span of %lld samples completes no whole number of frames of %d every %d",
                (long long)span, N, hop);
    const long long F = (span - N) / hop + 1, M = h->M;
    FRT_REQUIRE(F <= kMaxFrames, "frt_pitch_live_push: %lld frames in one push", F);
    FRT_REQUIRE(x && estimates_out && curve_out && (rows == 1 || ld_row >= span), "frt_pitch_live_push: null buffer or row stride %lld below the span",
                (long long)ld_row);
    FRT_REQUIRE(!is_device_pointer(x) && !is_device_pointer(estimates_out) && !is_device_pointer(curve_out),
                "frt_pitch_live_push: the span and the results are host memory");
    if (n_frames_out) *n_frames_out = F;

    // every row widened into the page-locked block, rows an even number of samples apart (16-byte row starts)
    const long long stride = span + (span & 1);
    const size_t in_bytes = (size_t)rows * stride * sizeof(double), out_n = (size_t)(F + 1 + M);
    const bool blocks = N % hop == 0 && N / hop >= 2;
    const int per_frame = blocks ? N / hop : 0;
    const long long n_blocks = blocks ? F + per_frame - 1 : 0;
    const long long units = blocks ? rows * n_blocks : F;
    int rc;
    if ((rc = h->pin_in.reserve(in_bytes)) || (rc = h->pin_out.reserve(out_n * sizeof(double))) || (rc = h->in.reserve(in_bytes)) ||
        (rc = h->energy.reserve((size_t)units * sizeof(double))) || (rc = h->raw.reserve(3 * (size_t)F * sizeof(double))) ||
        (rc = h->out.reserve(out_n * sizeof(double))))
        return rc;
    double* stage = static_cast<double*>(h->pin_in.ptr);
    for (int row = 0; row < rows; ++row) {
        double* d = stage + row * stride;
        if (dtype) {
            memcpy(d, static_cast<const double*>(x) + row * ld_row, (size_t)span * sizeof(double));
        } else {
            const float* s = static_cast<const float*>(x) + row * ld_row;
            for (long long i = 0; i < span; ++i) d[i] = (double)s[i];
        }
        if (stride > span) d[span] = 0.0;           // the pad: never part of a frame
    }
    const hipStream_t stream = nullptr;
    const double* xd = h->in.as<double>();
    FRT_HIP_CHECK(hipMemcpyAsync(h->in.ptr, stage, in_bytes, hipMemcpyHostToDevice, stream));
    PitchLiveView view{};
    if ((rc = pitch_live_front(h->plan, xd, span, stride, F, stream, &view))) return rc;
    hipLaunchKernelGGL(live_energy_kernel, dim3((unsigned)((units + 3) / 4)), dim3(kThreads), 0, stream, xd, stride, rows,
                       blocks ? hop : N, hop, n_blocks, blocks, units, h->energy.as<double>());
    if (F <= h->crossover) {
        hipLaunchKernelGGL(live_strength_kernel, dim3(view.Kp / 64, (unsigned)F), dim3(64), 0, stream, view.kt, view.s, view.strength,
                           view.lrange, view.Lp, view.Kp, view.cand_per_range);
    } else if ((rc = pitch_live_strength_tiled(h->plan, F))) {
        return rc;
    }
    FinishArgs a{};
    a.strength = view.strength; a.freqs = view.freqs; a.energy = h->energy.as<double>(); a.raw = h->raw.as<double>();
    a.prev = h->prev.as<double>();
    a.history_in = h->history.as<double>() + h->current * M;
    a.history_out = h->history.as<double>() + (1 - h->current) * M;
    a.out = h->out.as<double>();
    a.F = F; a.M = M; a.n_blocks = n_blocks;
    a.K = view.K; a.Kp = view.Kp; a.L = view.L; a.N = N; a.rows = rows; a.per_frame = per_frame;
    a.min_db = min_db; a.conf = conf; a.p_delta = p_delta; a.trans_min = h->trans_min; a.trans_span = h->trans_span;
    hipLaunchKernelGGL(live_finish_kernel, dim3(1), dim3(kThreads), 0, stream, a);
    FRT_HIP_CHECK(hipGetLastError());
    h->current = 1 - h->current;
    FRT_HIP_CHECK(hipMemcpyAsync(h->pin_out.ptr, h->out.ptr, out_n * sizeof(double), hipMemcpyDeviceToHost, stream));
    FRT_HIP_CHECK(hipStreamSynchronize(stream));
    const double* res = static_cast<const double*>(h->pin_out.ptr);
    memcpy(estimates_out, res, (size_t)F * sizeof(double));
    if (latest_out) *latest_out = res[F];
    memcpy(curve_out, res + F + 1, (size_t)M * sizeof(double));
    return FRT_OK;
}
