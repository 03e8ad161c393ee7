// curves.hip — the spectrum and octave-spectrum plot curves (SpectrumPlotWidget / HistPlot setdata + compute_peaks) for gfx950:
// the screen-space signal curve, its intensity, and the peak-hold curve with its state carried across refreshes.
// float64 arithmetic; built with -ffp-contract=off so that every expression is the reference's IEEE operations, in its order.
//
// Reference semantics (friture/spectrumPlotWidget.py:122-200, friture/histplot.py:77-130), per refresh of a dB row y of B bins,
// the vertical transform being CoordinateTransform's Linear branch with length 1 and no borders over [cmin, cmax]:
//   toScreen(v) = (v - cmin) / (cmax - cmin)          (cmax == cmin: 0 + 0. * v, NaN for +-inf and NaN)
//   scaled_y    = 1. - toScreen(y)
//   z           = (y - cmin) / (|M - cmin| + 1e-3), M = max(y) (numpy: a NaN anywhere in the row makes M, hence z, NaN)
//   peak hold   (state peak, int, decay; masks on the old state): peak < y -> peak = y, decay = c, int = 1;
//               otherwise int < 0.2 -> peak = peak + decay, decay = decay + c; otherwise int = int * 0.975
//   scaled_peak = 1. - toScreen(peak), z_peak = int
// with c = 20 log10(1 - 3e-6) 5000.  (toScreen's "* 1 + 0" leaves 1. - toScreen(v) unchanged, so it is not spelt out.)
//
// Kernels of one call (all on one stream):
//   curves_rowmax_kernel  the NaN-propagating max of every row whose z is written; a group of G lanes per row (G the power of
//                         two >= min(B, 64)), 64 / G rows per wavefront
//   curves_scan_kernel    one lane per (stream, bin), consecutive bins in consecutive lanes: walks the refreshes in order with the
//                         three state values in registers; the loads of the next kU refreshes are issued before the current kU
//                         are computed, so the dependent float64 recurrence never waits on memory in steady state
#include <cmath>

#include "common.h"
#include "widget_device.h"

namespace frt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kU = 16;              // refreshes per prefetch batch of the scan

// 20 * log10(1 - 3e-6) * 5000 as numpy evaluates it (checked against numpy by tests/test_plotcurves_cpu.py)
constexpr double kDecay = -0x1.0ad4b7d2d85e6p-3;

struct CurvesParams {
    const void* y;                  // y[s * ld_stream + r * ld_refresh + b]
    long long ld_refresh, ld_stream;
    int streams;
    long long R, B;
    long long Ro;                   // output rows per stream: R, or 1 (keep_last)
    double cmin, cmax;
    int flat;                       // cmax == cmin
    int peaks;                      // run the peak-hold recurrence
    int read_state;                 // peaks or a peak output
    const double* st_in;            // [streams][3][B]: peak, int, decay
    double* st_out;
    double* rowmax;                 // [streams][Ro] (z only)
    double *sy, *z, *sp, *zp;       // [streams][Ro][B] or null
};

__device__ __forceinline__ double screen_from_top(const CurvesParams& p, double v) {   // 1. - toScreen(v)
    const double t = p.flat ? 0. + 0. * v : (v - p.cmin) / (p.cmax - p.cmin);
    return 1. - t;
}

// rows (s, j), j < Ro, refresh r = keep_last ? R - 1 : j; lanes g*G .. g*G + G - 1 of a wavefront take one row
template <bool kF64, int G>
__global__ __launch_bounds__(kThreads) void curves_rowmax_kernel(CurvesParams p) {
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)p.streams * p.Ro;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (wave * (64 / G) >= rows) return;                                      // whole wavefronts only: the shuffles below
    const long long row = wave * (64 / G) + lane / G;
    const int sub = lane % G;
    double m = -INFINITY;
    if (row < rows) {
        const long long s = row / p.Ro, j = row - s * p.Ro;
        const long long r = p.Ro == p.R ? j : p.R - 1;
        const long long off = s * p.ld_stream + r * p.ld_refresh;
#pragma unroll 8
        for (long long b = sub; b < p.B; b += G) m = nanmax(m, load_real<kF64>(p.y, off + b));
    }
    for (int o = 1; o < G; o <<= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    if (row < rows && sub == 0) p.rowmax[row] = m;
}

// kFull: every output, peaks on, every refresh written (the batch form): no branch inside a batch of kU refreshes
template <bool kF64, bool kFull>
__global__ __launch_bounds__(kThreads) void curves_scan_kernel(CurvesParams p) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (long long)p.streams * p.B) return;
    const long long s = g / p.B, b = g - s * p.B;
    const char* yb = reinterpret_cast<const char*>(p.y) + (size_t)(s * p.ld_stream + b) * (kF64 ? 8 : 4);
    const double* mrow = p.rowmax ? p.rowmax + s * p.Ro : nullptr;
    const size_t so = (size_t)s * 3 * p.B + b;
    double peak = 0., pint = 0., dec = 0.;
    if (kFull || p.read_state) {
        peak = p.st_in[so];
        pint = p.st_in[so + p.B];
        dec = p.st_in[so + 2 * p.B];
    }
    const double Mlast = (!kFull && mrow && p.Ro == 1) ? mrow[0] : 0.;
    const long long R = p.R;

    // one refresh: r its index, v its y, M its row max (z only)
    auto step = [&](long long r, double v, double M) {
        const bool out = kFull || p.Ro == R || r == R - 1;
        const size_t o = ((size_t)s * p.Ro + (p.Ro == R ? r : 0)) * p.B + b;
        if ((kFull || p.sy) && out) p.sy[o] = screen_from_top(p, v);
        if ((kFull || p.z) && out) p.z[o] = (v - p.cmin) / (fabs(M - p.cmin) + 1e-3);
        if (kFull || p.peaks) {
            if (peak < v) {
                peak = v;
                dec = kDecay;
                pint = 1.;
            } else if (pint < 0.2) {
                peak = peak + dec;
                dec = dec + kDecay;
            } else {
                pint = pint * 0.975;
            }
        }
        if ((kFull || p.sp) && out) p.sp[o] = screen_from_top(p, peak);
        if ((kFull || p.zp) && out) p.zp[o] = pint;
    };
    const bool need_m = kFull || (p.z && p.Ro == R);
    auto fetch = [&](long long r0, double* yv, double* mv) {           // clamped to the last refresh: always in bounds
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long r = r0 + u < R ? r0 + u : R - 1;
            yv[u] = load_real<kF64>(yb, r * p.ld_refresh);
            mv[u] = need_m ? mrow[r] : Mlast;
        }
    };
    double ya[kU], ma[kU], yn[kU], mn[kU];
    fetch(0, ya, ma);
    for (long long r0 = 0; r0 < R; r0 += kU) {
        fetch(r0 + kU, yn, mn);                                             // the next batch is in flight during this one
        if (r0 + kU <= R) {
#pragma unroll
            for (int u = 0; u < kU; ++u) step(r0 + u, ya[u], ma[u]);
        } else {
#pragma unroll
            for (int u = 0; u < kU; ++u)
                if (r0 + u < R) step(r0 + u, ya[u], ma[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            ya[u] = yn[u];
            ma[u] = mn[u];
        }
    }
    if (kFull || p.peaks) {
        p.st_out[so] = peak;
        p.st_out[so + p.B] = pint;
        p.st_out[so + 2 * p.B] = dec;
    }
}

template <bool kF64>
void launch_rowmax(const CurvesParams& p, hipStream_t stream) {
    const int G = p.B >= 64 ? 64 : p.B > 16 ? 32 : p.B > 4 ? 16 : 4;
    const long long rows = (long long)p.streams * p.Ro;
    const long long waves = (rows + 64 / G - 1) / (64 / G);
    const dim3 grid((unsigned)((waves + kWaves - 1) / kWaves));
    switch (G) {
        case 64: hipLaunchKernelGGL((curves_rowmax_kernel<kF64, 64>), grid, dim3(kThreads), 0, stream, p); break;
        case 32: hipLaunchKernelGGL((curves_rowmax_kernel<kF64, 32>), grid, dim3(kThreads), 0, stream, p); break;
        case 16: hipLaunchKernelGGL((curves_rowmax_kernel<kF64, 16>), grid, dim3(kThreads), 0, stream, p); break;
        default: hipLaunchKernelGGL((curves_rowmax_kernel<kF64, 4>), grid, dim3(kThreads), 0, stream, p); break;
    }
}

template <bool kF64>
void launch_scan(const CurvesParams& p, bool full, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)p.streams * p.B + kThreads - 1) / kThreads));
    if (full)
        hipLaunchKernelGGL((curves_scan_kernel<kF64, true>), grid, dim3(kThreads), 0, stream, p);
    else
        hipLaunchKernelGGL((curves_scan_kernel<kF64, false>), grid, dim3(kThreads), 0, stream, p);
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" double frt_curves_decay_step(void) { return kDecay; }

extern "C" int frt_curves_run(const void* y, int dtype, int streams, int64_t n_refresh, int64_t bins, int64_t ld_refresh,
                              int64_t ld_stream, double cmin, double cmax, double* state, int peaks, int keep_last, double* scaled_y,
                              double* z, double* scaled_peak, double* z_peak) {
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_curves_run: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(streams >= 1 && bins >= 1 && n_refresh >= 0, "frt_curves_run: %d streams x %lld refreshes x %lld bins", streams,
                (long long)n_refresh, (long long)bins);
    FRT_REQUIRE((n_refresh <= 1 || ld_refresh >= bins) && (streams == 1 || ld_stream >= (n_refresh - 1) * (n_refresh > 1 ? ld_refresh : 0) + bins),
                "frt_curves_run: bad shape (ld_refresh %lld, ld_stream %lld)", (long long)ld_refresh, (long long)ld_stream);
    FRT_REQUIRE((long long)streams * bins < (1LL << 31), "frt_curves_run: %lld lanes (split the call)", (long long)streams * bins);
    const bool peak_out = scaled_peak || z_peak;
    FRT_REQUIRE(!(peaks || peak_out) || state, "frt_curves_run: null state with peaks or a peak output");
    if (n_refresh == 0) return FRT_OK;
    FRT_REQUIRE(y, "frt_curves_run: null input");
    CurvesParams p{};
    p.streams = streams;
    p.R = n_refresh;
    p.B = bins;
    p.ld_refresh = n_refresh > 1 ? ld_refresh : bins;
    p.ld_stream = streams > 1 ? ld_stream : (n_refresh - 1) * p.ld_refresh + bins;
    p.Ro = keep_last ? 1 : n_refresh;
    p.cmin = cmin;
    p.cmax = cmax;
    p.flat = cmax == cmin;
    p.peaks = peaks ? 1 : 0;
    p.read_state = (peaks || peak_out) ? 1 : 0;
    const size_t es = dtype ? sizeof(double) : sizeof(float);
    const size_t ybytes = ((size_t)(streams - 1) * p.ld_stream + (size_t)(n_refresh - 1) * p.ld_refresh + bins) * es;
    const size_t stbytes = (size_t)streams * 3 * bins * sizeof(double);
    const size_t obytes = (size_t)streams * p.Ro * bins * sizeof(double);

    StageCall call;
    const int iy = call.add_in(y, ybytes);
    const int isi = p.read_state ? call.add_in(state, stbytes) : -1;
    const int iso = peaks ? call.add_out(state, stbytes) : -1;
    double* outs[4] = {scaled_y, z, scaled_peak, z_peak};
    int io[4];
    for (int k = 0; k < 4; ++k) io[k] = outs[k] ? call.add_out(outs[k], obytes) : -1;
    const int im = z ? call.add_scratch((size_t)streams * p.Ro * sizeof(double)) : -1;
    int rc = call.begin();
    if (rc) return rc;
    p.y = call.ptr<const void>(iy);
    p.st_in = isi >= 0 ? call.ptr<const double>(isi) : nullptr;
    p.st_out = iso >= 0 ? call.ptr<double>(iso) : nullptr;
    p.sy = io[0] >= 0 ? call.ptr<double>(io[0]) : nullptr;
    p.z = io[1] >= 0 ? call.ptr<double>(io[1]) : nullptr;
    p.sp = io[2] >= 0 ? call.ptr<double>(io[2]) : nullptr;
    p.zp = io[3] >= 0 ? call.ptr<double>(io[3]) : nullptr;
    p.rowmax = im >= 0 ? call.ptr<double>(im) : nullptr;
    const hipStream_t stream = call.stream();
    if (z) {
        if (dtype) launch_rowmax<true>(p, stream);
        else launch_rowmax<false>(p, stream);
        FRT_HIP_CHECK(hipGetLastError());
    }
    const bool full = !keep_last && peaks && scaled_y && z && scaled_peak && z_peak;
    if (dtype) launch_scan<true>(p, full, stream);
    else launch_scan<false>(p, full, stream);
    FRT_HIP_CHECK(hipGetLastError());
    return call.finish();
}
