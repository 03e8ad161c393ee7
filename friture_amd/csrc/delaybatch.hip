// delaybatch.hip — the delay estimator's chain over whole recordings (Delay_Estimator_Widget.handle_new_data,
// friture/delay_estimator.py:87-176) for gfx950: both channels of S widgets decimated time-parallel, the 50 %-overlapped
// windows of the widgets' mirror rings rebuilt from a run table that the host planned on indices alone
// (friture_amd/delay_estimator.py, delay_schedule), GCC-PHAT of all of them (frt_gcc_phat as it is) and the smoothing and
// read-out of every window.  float64 throughout; built with -ffp-contract=off; everything is enqueued on the null stream.
//
//   decimate  frt_delaybatch_decimate.  A stage is the 12th-order DF2T recurrence of lfilter.py:131-139 over n samples and
//             every other output kept.  The signal is cut into cells of kDbChunk samples on a grid anchored at the recording's
//             absolute sample index; a lane owns one cell.
//               pass 1  every cell but the last from the zero state (the first from the carried state): its end state
//               pass 2  start_(c+1) = end_c + A^kDbChunk start_c along the cells of a channel (the recurrence is linear, so
//                       this is exact in real arithmetic; A^kDbChunk is made on the host in long double)
//               pass 3  every cell again from its true start state, the even outputs kept; the last cell leaves the state
//             Passes 1 and 3 are one kernel.  A workgroup is one wavefront of 64 consecutive cells of one channel; their
//             samples come through LDS in tiles of kDbTile per cell (a row of a tile is one 128-byte line of the signal, the
//             next tile's loads are in flight while this one is filtered) and the outputs leave through LDS the same way.
//             The steps of a cell are the reference's operations in the reference's order.
//   windows   frt_delaybatch_windows.  Per window and channel at most eight runs of (source range | zeros, earlier window
//             whose mean the ring view had subtracted from them).  (a) sum, minimum and maximum of every run; (b) one lane
//             per stream walks its windows in order: effective mean and gate; (c) per slab of pairs the effective windows are
//             written out and go to frt_gcc_phat.
//   readout   frt_delaybatch_readout.  A lane owns one lag of one stream and walks the windows in order, carrying the smoothed
//             correlation; per window a workgroup leaves the partial sum / extremum of its 256 lags, combined per window in lag
//             order (the bits do not depend on the grid); a second walk leaves the squared deviations for numpy.std.
#include <cmath>
#include <mutex>

#include "common.h"

namespace frt {
namespace {

constexpr int kDbOrder = 12;          // the decimator's order (13 coefficients)
constexpr int kDbChunk = 1024;        // samples per cell
constexpr int kDbTile = 16;           // samples of a cell per LDS tile
constexpr int kDbLanes = 64;          // cells per workgroup
constexpr int kDbRuns = 8;            // runs per window in the table
constexpr int kDbSeg = 256;           // lags per workgroup of the read-out

struct DbStage {
    const void* x;             // [C][x_stride] T
    double* out;               // [C][out_stride]: sample 2 o of the stage's output at o
    const double* coef;        // b[13] then a[13]
    const double* zi;          // [C][z_stride] or null (zero state)
    double* zf;                // [C][z_stride] or null
    double* ends;              // [C][nchunks][12]
    double* starts;            // [C][nchunks + 1][12]
    const double* power;       // A^kDbChunk [12][12]
    long long x_stride, out_stride, z_stride, n, lead;      // lead: samples of cell 0 in front of the input
    int nchunks, ecells;       // ecells: cells per channel in `ends`
};

template <typename T, bool OUT>
__global__ void __launch_bounds__(kDbLanes) db_cells_kernel(const DbStage a) {
    __shared__ double tin[kDbLanes][kDbTile + 1];
    __shared__ double tout[kDbLanes][kDbTile / 2 + 1];
    const int lane = threadIdx.x, ch = blockIdx.y;
    const long long c0 = (long long)blockIdx.x * kDbLanes, c = c0 + lane;
    const bool active = c < a.nchunks;
    const T* __restrict__ x = (const T*)a.x + (size_t)ch * a.x_stride;
    double b[kDbOrder + 1], ac[kDbOrder + 1], z[kDbOrder];
#pragma unroll
    for (int k = 0; k <= kDbOrder; ++k) {
        b[k] = a.coef[k];
        ac[k] = a.coef[kDbOrder + 1 + k];
    }
#pragma unroll
    for (int k = 0; k < kDbOrder; ++k) {
        z[k] = 0.0;
        if (active) {
            if (OUT) z[k] = a.starts[((size_t)ch * (a.nchunks + 1) + c) * kDbOrder + k];
            else if (c == 0 && a.zi) z[k] = a.zi[(size_t)ch * a.z_stride + k];
        }
    }
    const long long i0 = c * kDbChunk - a.lead;               // the cell's first sample, as an index of the input
    const int par = (int)(a.lead & 1);                        // sample i0 + s is an even one where s + par is even
    const long long nout = (a.n + 1) / 2;
    const int lrow = lane / kDbTile, lcol = lane % kDbTile;   // loads: four rows of sixteen samples per trip
    const int srow = lane / (kDbTile / 2), scol = lane % (kDbTile / 2);
    double nx[kDbTile];
    auto request = [&](int t) {
#pragma unroll
        for (int k = 0; k < kDbTile; ++k) {
            const long long cc = c0 + k * (kDbLanes / kDbTile) + lrow;
            const long long i = cc * kDbChunk - a.lead + (long long)t * kDbTile + lcol;
            nx[k] = (cc < a.nchunks && i >= 0 && i < a.n) ? (double)x[i] : 0.0;
        }
    };
    request(0);
    for (int t = 0; t < kDbChunk / kDbTile; ++t) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kDbTile; ++k) tin[k * (kDbLanes / kDbTile) + lrow][lcol] = nx[k];
        __syncthreads();
        if (t + 1 < kDbChunk / kDbTile) request(t + 1);
        const long long it = i0 + (long long)t * kDbTile;
#pragma unroll
        for (int s = 0; s < kDbTile; ++s) {
            const long long i = it + s;
            const double xv = tin[lane][s];
            if (active && i >= 0 && i < a.n) {                // lfilter.py:131-139, the operations in its order
                const double y = z[0] + b[0] * xv;
#pragma unroll
                for (int k = 0; k < kDbOrder - 1; ++k) z[k] = z[k + 1] + xv * b[k + 1] - y * ac[k + 1];
                z[kDbOrder - 1] = xv * b[kDbOrder] - y * ac[kDbOrder];
                if (OUT && ((s + par) & 1) == 0) tout[lane][s >> 1] = y;
            }
        }
        if (OUT) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kDbTile / 2; ++k) {
                const int row = k * (kDbLanes / (kDbTile / 2)) + srow;
                const long long cc = c0 + row;
                const long long o = ((cc * kDbChunk - a.lead + (long long)t * kDbTile + par) >> 1) + scol;      // an even number halved
                if (cc < a.nchunks && o >= 0 && o < nout) a.out[(size_t)ch * a.out_stride + o] = tout[row][scol];
            }
        }
    }
    if (!active) return;
    if (!OUT) {
#pragma unroll
        for (int k = 0; k < kDbOrder; ++k) a.ends[((size_t)ch * a.ecells + c) * kDbOrder + k] = z[k];
    } else if (c == a.nchunks - 1 && a.zf) {
#pragma unroll
        for (int k = 0; k < kDbOrder; ++k) a.zf[(size_t)ch * a.z_stride + k] = z[k];
    }
}

// pass 2: lane r < 12 carries state r of one channel along its cells (the first cell's end state is already the true one)
__global__ void __launch_bounds__(64) db_scan_kernel(const DbStage a) {
    const int lane = threadIdx.x, ch = blockIdx.x, r = lane < kDbOrder ? lane : kDbOrder - 1;
    double m[kDbOrder];
#pragma unroll
    for (int k = 0; k < kDbOrder; ++k) m[k] = a.power[r * kDbOrder + k];
    double s = a.zi ? a.zi[(size_t)ch * a.z_stride + r] : 0.0;
    double* st = a.starts + (size_t)ch * (a.nchunks + 1) * kDbOrder;
    const double* en = a.ends + (size_t)ch * a.ecells * kDbOrder;
    if (lane < kDbOrder) st[r] = s;
    double e = a.nchunks > 1 ? en[r] : 0.0;
    for (int c = 0; c + 1 < a.nchunks; ++c) {
        const double cur = e;
        if (c + 2 < a.nchunks) e = en[(size_t)(c + 1) * kDbOrder + r];
        double acc = cur;
        if (c > 0) {
#pragma unroll
            for (int k = 0; k < kDbOrder; ++k) acc += m[k] * __shfl(s, k, 64);
        }
        s = acc;
        if (lane < kDbOrder) st[(size_t)(c + 1) * kDbOrder + r] = s;
    }
}

// ---- windows ------------------------------------------------------------------------------------------------------------

__device__ inline double db_block_sum(double v, double* red) {      // 256 lanes, a fixed tree
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// (a) stats[row][w][r] = (sum, min, max) of run r of window w in row `row` of the decimated signals
__global__ void __launch_bounds__(256) db_runstats_kernel(const double* __restrict__ dec, long long stride, const long long* __restrict__ runs,
                                                          double* __restrict__ stats) {
    __shared__ double red[4], rmin[4], rmax[4];
    const long long wr = blockIdx.x, row = blockIdx.y, nwr = gridDim.x;
    const long long src = runs[wr * 4], len = runs[wr * 4 + 1], zero = runs[wr * 4 + 2];
    double* o = stats + ((size_t)row * nwr + wr) * 3;
    if (len <= 0 || zero) {                                          // block-uniform
        if (threadIdx.x == 0) {
            o[0] = 0.0;
            o[1] = len > 0 ? 0.0 : INFINITY;
            o[2] = len > 0 ? 0.0 : -INFINITY;
        }
        return;
    }
    const double* p = dec + (size_t)row * stride + src;
    double acc = 0.0, lo = INFINITY, hi = -INFINITY;
    for (long long i = threadIdx.x; i < len; i += 256) {
        const double v = p[i];
        acc += v;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
    }
    for (int s = 32; s > 0; s >>= 1) {
        lo = fmin(lo, __shfl_down(lo, s, 64));
        hi = fmax(hi, __shfl_down(hi, s, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        rmin[threadIdx.x >> 6] = lo;
        rmax[threadIdx.x >> 6] = hi;
    }
    const double total = db_block_sum(acc, red);
    if (threadIdx.x == 0) {
        o[0] = total;
        o[1] = fmin(fmin(rmin[0], rmin[1]), fmin(rmin[2], rmin[3]));
        o[2] = fmax(fmax(rmax[0], rmax[1]), fmax(rmax[2], rmax[3]));
    }
}

// (b) a lane is a stream: the effective mean of every window and its gate, in window order
__global__ void __launch_bounds__(64) db_means_kernel(const double* __restrict__ stats, const long long* __restrict__ runs,
                                                      const double* __restrict__ means_in, double* __restrict__ means,
                                                      int* __restrict__ gated, int S, long long W, int L) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    for (long long w = 0; w < W; ++w) {
        double mean[2];
        bool silent = false;
        for (int ch = 0; ch < 2; ++ch) {
            const size_t row = (size_t)s * 2 + ch;
            double total = 0.0, lo = INFINITY, hi = -INFINITY;
            for (int r = 0; r < kDbRuns; ++r) {
                const long long* run = runs + (w * kDbRuns + r) * 4;
                const long long len = run[1], prior = run[3];
                if (len <= 0) continue;
                const double* st = stats + ((size_t)row * W * kDbRuns + w * kDbRuns + r) * 3;
                double sum = st[0], a = st[1], b = st[2];
                if (prior != -1) {
                    const double m = prior >= 0 ? means[((size_t)s * W + prior) * 2 + ch] : (means_in ? means_in[(size_t)s * 2 + ch] : 0.0);
                    sum = sum - (double)len * m;
                    a = a - m;
                    b = b - m;
                }
                total += sum;
                lo = fmin(lo, a);
                hi = fmax(hi, b);
            }
            mean[ch] = total / (double)L;
            if (lo == hi) silent = true;                             // every effective sample equal: the stream object's gate
        }
        means[((size_t)s * W + w) * 2] = silent ? 0.0 : mean[0];   // a gated window subtracts nothing
        means[((size_t)s * W + w) * 2 + 1] = silent ? 0.0 : mean[1];
        gated[(size_t)s * W + w] = silent ? 1 : 0;
    }
}

// (c) the effective windows of pairs q0 .. q0 + gridDim.y - 1 (pair q = stream q / W, window q % W): (x - m_j) rounded
__global__ void __launch_bounds__(256) db_windows_kernel(const double* __restrict__ dec, long long stride, const long long* __restrict__ runs,
                                                         const double* __restrict__ means_in, const double* __restrict__ means,
                                                         double* __restrict__ d0, double* __restrict__ d1, long long q0, long long W, int L) {
    const long long q = q0 + blockIdx.y, s = q / W, w = q - s * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    const long long* run = runs + w * kDbRuns * 4;
    long long at = 0;
    int r = 0;
    for (; r < kDbRuns - 1; ++r) {                                   // the table's lengths add up to L (checked on the host)
        if (i < at + run[r * 4 + 1]) break;
        at += run[r * 4 + 1];
    }
    const long long src = run[r * 4] + (i - at), zero = run[r * 4 + 2], prior = run[r * 4 + 3];
    for (int ch = 0; ch < 2; ++ch) {
        double v = zero ? 0.0 : dec[((size_t)s * 2 + ch) * stride + src];
        if (prior != -1) v = v - (prior >= 0 ? means[((size_t)s * W + prior) * 2 + ch] : (means_in ? means_in[(size_t)s * 2 + ch] : 0.0));
        (ch ? d1 : d0)[(size_t)blockIdx.y * L + i] = v;
    }
}

// ---- read-out -----------------------------------------------------------------------------------------------------------

struct DbRead {
    const double* xcorr;       // [S][W][L]
    const int* gated;          // [S][W]
    const double* sm_in;       // [S][L] or null
    const int* present_in;     // [S] or null
    double* sm_out;            // [S][L]
    int* present_out;          // [S]
    double* psum;              // [S][W][nseg]: sum of the smoothed lags (pass 0), of their squared deviations (pass 1)
    double* pbest;             // [S][W][nseg]: the segment's extremum (signed)
    int* pidx;                 // [S][W][nseg]
    const double* mean;        // [S][W]
    long long W;
    int L, nseg;
    double alpha;
};

template <int PASS>
__global__ void __launch_bounds__(kDbSeg) db_walk_kernel(const DbRead a) {
    __shared__ double red[4], rbest[4], rval[4];
    __shared__ int ridx[4];
    const int seg = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, i = seg * kDbSeg + tid;
    const bool mine = i < a.L;
    bool have = a.sm_in && a.present_in && a.present_in[s] != 0;     // block-uniform
    double sm = have && mine ? a.sm_in[(size_t)s * a.L + i] : 0.0;
    for (long long w = 0; w < a.W; ++w) {
        if (a.gated[(size_t)s * a.W + w]) continue;                  // keeps the carried correlation
        const double x = mine ? a.xcorr[((size_t)s * a.W + w) * a.L + i] : 0.0;
        sm = have ? a.alpha * x + (1.0 - a.alpha) * sm : x;          // delay_estimator.py:134-138
        have = true;
        const size_t po = ((size_t)s * a.W + w) * a.nseg + seg;
        if (PASS == 0) {
            double best = mine ? fabs(sm) : -1.0, val = sm;
            int idx = i;
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_down(best, o, 64), ov = __shfl_down(val, o, 64);
                const int oi = __shfl_down(idx, o, 64);
                if (ob > best || (ob == best && oi < idx)) { best = ob; val = ov; idx = oi; }
            }
            if ((tid & 63) == 0) { rbest[tid >> 6] = best; rval[tid >> 6] = val; ridx[tid >> 6] = idx; }
            const double total = db_block_sum(mine ? sm : 0.0, red);
            if (tid == 0) {
                for (int k = 1; k < 4; ++k)
                    if (rbest[k] > best || (rbest[k] == best && ridx[k] < idx)) { best = rbest[k]; val = rval[k]; idx = ridx[k]; }
                a.psum[po] = total;
                a.pbest[po] = val;
                a.pidx[po] = idx;
            }
        } else {
            const double d = sm - a.mean[(size_t)s * a.W + w];
            const double total = db_block_sum(mine ? d * d : 0.0, red);
            if (tid == 0) a.psum[po] = total;
        }
        __syncthreads();
    }
    if (PASS == 0) {
        if (mine) a.sm_out[(size_t)s * a.L + i] = sm;
        if (seg == 0 && tid == 0) a.present_out[s] = have ? 1 : 0;
    }
}

// per (stream, window): the segments' partial results in lag order
__global__ void __launch_bounds__(256) db_peak_kernel(const DbRead a, int S, double* __restrict__ mean, int* __restrict__ argmax,
                                                      double* __restrict__ extremum) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)S * a.W) return;
    if (a.gated[t]) {
        mean[t] = 0.0;
        argmax[t] = 0;
        extremum[t] = 0.0;
        return;
    }
    double sum = 0.0, best = -1.0, val = 0.0;
    int idx = 0;
    for (int g = 0; g < a.nseg; ++g) {
        sum += a.psum[(size_t)t * a.nseg + g];
        const double v = a.pbest[(size_t)t * a.nseg + g];
        if (fabs(v) > best) { best = fabs(v); val = v; idx = a.pidx[(size_t)t * a.nseg + g]; }      // numpy.argmax: the first on ties
    }
    mean[t] = sum / (double)a.L;
    argmax[t] = idx;
    extremum[t] = val;
}

__global__ void __launch_bounds__(256) db_readout_kernel(const DbRead a, int S, const int* __restrict__ argmax, const double* __restrict__ extremum,
                                                         double rate, double delayrange_s, double* __restrict__ delay_ms,
                                                         double* __restrict__ distance_m, int* __restrict__ correlation) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)S * a.W) return;
    if (a.gated[t]) {                                                // delay_estimator.py:178-182
        delay_ms[t] = 0.0;
        distance_m[t] = 0.0;
        correlation[t] = 0;
        return;
    }
    double var = 0.0;
    for (int g = 0; g < a.nseg; ++g) var += a.psum[(size_t)t * a.nseg + g];
    const double sd = sqrt(var / (double)a.L);
    const double peak_norm = fabs(extremum[t]) / (3.0 * sd);
    const double time = 2.0 * delayrange_s;
    double d = 1e3 * (double)argmax[t] / rate;
    if (d > 1e3 * time / 2.0) d -= 1e3 * time;
    delay_ms[t] = d;
    distance_m[t] = d * 1e-3 * 340.0;
    double x = peak_norm > 1.0 ? peak_norm - 1.0 : 0.0;
    x = pow(0.12 * x, 3.0);
    correlation[t] = (int)((x / (1.0 + x)) * 100.0);
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// process-level scratch, created on first use and never freed (no HIP call runs from a static destructor); calls are
// serialised by the mutex and ordered by the null stream
struct DbScratch {
    std::mutex lock;
    DeviceBuffer coef, power, stage[2], ends, starts, runs, stats, d0, d1, psum, pbest, pidx, mean;
    std::vector<double> coef_host, power_host;
};
DbScratch& scratch() {
    static DbScratch* s = new DbScratch();
    return *s;
}

// A^p of the zero-input DF2T step z' = A z (y = z0; z_k' = z_(k+1) - a_(k+1) y), in long double
void db_transition_power(const double* a, long long p, double* out) {
    constexpr int n = kDbOrder;
    std::vector<long double> base(n * n, 0.0L), acc(n * n, 0.0L), tmp(n * n);
    for (int k = 0; k < n; ++k) {
        base[k * n] = -(long double)a[k + 1];
        if (k + 1 < n) base[k * n + k + 1] += 1.0L;
        acc[k * n + k] = 1.0L;
    }
    auto mul = [&](std::vector<long double>& x, const std::vector<long double>& y) {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                long double v = 0.0L;
                for (int k = 0; k < n; ++k) v += x[i * n + k] * y[k * n + j];
                tmp[i * n + j] = v;
            }
        x = tmp;
    };
    for (; p > 0; p >>= 1) {
        if (p & 1) mul(acc, base);
        mul(base, std::vector<long double>(base));
    }
    for (int i = 0; i < n * n; ++i) out[i] = (double)acc[i];
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" int frt_delaybatch_decimate(const double* b, const double* a, int n_coef, int n_stages, const void* x, int dtype,
                                       int n_channels, int64_t n, int64_t x_stride, int64_t origin, const double* zi, double* out,
                                       int64_t out_stride, double* zf, int64_t* n_out) {
    FRT_REQUIRE(b && a && n_coef == kDbOrder + 1 && a[0] == 1.0, "frt_delaybatch_decimate: needs 13 coefficients with a[0] = 1");
    FRT_REQUIRE(n_stages >= 1 && n_stages <= 8, "frt_delaybatch_decimate: n_stages %d not in [1, 8]", n_stages);
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_delaybatch_decimate: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(n_channels >= 1 && n_channels <= 65535, "frt_delaybatch_decimate: %d channels (1 .. 65535)", n_channels);
    FRT_REQUIRE(n >= 0 && n < (1ll << 40) && origin >= 0, "frt_delaybatch_decimate: n = %lld, origin = %lld", (long long)n, (long long)origin);
    int64_t len[9];
    len[0] = n;
    for (int j = 0; j < n_stages; ++j) len[j + 1] = (len[j] + 1) / 2;
    if (n_out) *n_out = len[n_stages];
    if (n == 0) {                                                    // decimate.py:56-57: nothing in, nothing out, the states stay
        if (zf && zi) FRT_HIP_CHECK(hipMemcpyAsync(zf, zi, (size_t)n_channels * n_stages * kDbOrder * sizeof(double), hipMemcpyDeviceToDevice, 0));
        else if (zf) FRT_HIP_CHECK(hipMemsetAsync(zf, 0, (size_t)n_channels * n_stages * kDbOrder * sizeof(double), 0));
        return FRT_OK;
    }
    FRT_REQUIRE(x && out && is_device_pointer(x) && is_device_pointer(out), "frt_delaybatch_decimate: x and out are device arrays");
    FRT_REQUIRE((!zi || is_device_pointer(zi)) && (!zf || is_device_pointer(zf)), "frt_delaybatch_decimate: the states are device arrays");
    FRT_REQUIRE(x_stride >= n && out_stride >= len[n_stages], "frt_delaybatch_decimate: row strides %lld / %lld below the rows' %lld / %lld samples",
                (long long)x_stride, (long long)out_stride, (long long)n, (long long)len[n_stages]);
    DbScratch& sc = scratch();
    std::lock_guard<std::mutex> guard(sc.lock);
    int rc;
    std::vector<double> coef(2 * (kDbOrder + 1)), power(kDbOrder * kDbOrder);
    for (int k = 0; k <= kDbOrder; ++k) {
        coef[k] = b[k];
        coef[kDbOrder + 1 + k] = a[k];
    }
    if (!sc.coef.ptr || coef != sc.coef_host) {
        db_transition_power(a, kDbChunk, power.data());
        if ((rc = upload_if_changed(sc.coef, sc.coef_host, coef, 0)) || (rc = upload_if_changed(sc.power, sc.power_host, power, 0))) return rc;
    }
    const int C = n_channels;
    const long long cells_max = (len[0] + 2 * (long long)kDbChunk - 2) / kDbChunk + 1;
    FRT_REQUIRE(cells_max < (1ll << 30), "frt_delaybatch_decimate: too many cells");
    for (int j = 1; j < n_stages; ++j)
        if ((rc = sc.stage[(j - 1) & 1].reserve((size_t)C * len[j] * sizeof(double)))) return rc;
    if ((rc = sc.ends.reserve((size_t)C * cells_max * kDbOrder * sizeof(double))) ||
        (rc = sc.starts.reserve((size_t)C * (cells_max + 1) * kDbOrder * sizeof(double))))
        return rc;
    for (int j = 0; j < n_stages; ++j) {
        DbStage s{};
        s.x = j == 0 ? x : sc.stage[(j - 1) & 1].ptr;
        s.x_stride = j == 0 ? x_stride : len[j];
        s.out = j == n_stages - 1 ? out : sc.stage[j & 1].as<double>();
        s.out_stride = j == n_stages - 1 ? out_stride : len[j + 1];
        s.coef = sc.coef.as<double>();
        s.power = sc.power.as<double>();
        s.zi = zi ? zi + (size_t)j * kDbOrder : nullptr;
        s.zf = zf ? zf + (size_t)j * kDbOrder : nullptr;
        s.z_stride = (long long)n_stages * kDbOrder;
        s.ends = sc.ends.as<double>();
        s.starts = sc.starts.as<double>();
        s.n = len[j];
        s.lead = (origin >> j) % kDbChunk;                           // the grid is anchored at the recording's sample 0
        s.nchunks = (int)((s.lead + s.n + kDbChunk - 1) / kDbChunk);
        s.ecells = s.nchunks;
        const bool f32 = j == 0 && dtype == 0;
        const dim3 grid((s.nchunks + kDbLanes - 1) / kDbLanes, C);
        if (s.nchunks > 1) {
            const dim3 g1((s.nchunks - 1 + kDbLanes - 1) / kDbLanes, C);      // the last cell's end state is pass 3's
            DbStage p = s;
            p.nchunks = s.nchunks - 1;
            // pass 1 sees one cell less; every sample of its cells lies inside the input
            if (f32) hipLaunchKernelGGL((db_cells_kernel<float, false>), g1, dim3(kDbLanes), 0, 0, p);
            else hipLaunchKernelGGL((db_cells_kernel<double, false>), g1, dim3(kDbLanes), 0, 0, p);
        }
        {
            hipLaunchKernelGGL(db_scan_kernel, dim3(C), dim3(64), 0, 0, s);
        }
        if (f32) hipLaunchKernelGGL((db_cells_kernel<float, true>), grid, dim3(kDbLanes), 0, 0, s);
        else hipLaunchKernelGGL((db_cells_kernel<double, true>), grid, dim3(kDbLanes), 0, 0, s);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return FRT_OK;
}

extern "C" int frt_delaybatch_windows(const double* dec, int64_t dec_stride, int64_t n_dec, int n_streams, int length, int64_t n_windows,
                                      const int64_t* runs, const double* means_in, frt_gcc* gcc_full, int64_t pairs_full, frt_gcc* gcc_last,
                                      double* xcorr, double* means_out, int* gated_out, int* n_slabs_out) {
    if (n_slabs_out) *n_slabs_out = 0;
    FRT_REQUIRE(n_streams >= 1 && n_streams <= 32767 && length >= 4 && n_windows >= 0 && n_dec >= 0 && dec_stride >= n_dec,
                "frt_delaybatch_windows: bad shape");
    if (n_windows == 0) return FRT_OK;
    FRT_REQUIRE(dec && runs && xcorr && means_out && gated_out && gcc_full && gcc_last && pairs_full >= 1, "frt_delaybatch_windows: null argument");
    FRT_REQUIRE(is_device_pointer(dec) && is_device_pointer(xcorr) && is_device_pointer(means_out) && is_device_pointer(gated_out) &&
                    (!means_in || is_device_pointer(means_in)) && !is_device_pointer(runs),
                "frt_delaybatch_windows: the run table is a host array, everything else device arrays");
    FRT_REQUIRE(n_windows * kDbRuns < (1ll << 31) && pairs_full <= 65535, "frt_delaybatch_windows: too many windows, or more than 65535 pairs per slab");
    const int64_t W = n_windows;
    for (int64_t w = 0; w < W; ++w) {                                // nothing out of bounds, whatever the table says
        int64_t total = 0;
        for (int r = 0; r < kDbRuns; ++r) {
            const int64_t* run = runs + (w * kDbRuns + r) * 4;
            FRT_REQUIRE(run[1] >= 0 && run[1] <= length && (run[2] == 0 || run[2] == 1) && run[3] >= -2 && run[3] < w,
                        "frt_delaybatch_windows: window %lld run %d: length %lld, zero flag %lld, earlier window %lld", (long long)w, r,
                        (long long)run[1], (long long)run[2], (long long)run[3]);
            FRT_REQUIRE(run[1] == 0 || run[2] || (run[0] >= 0 && run[0] + run[1] <= n_dec),
                        "frt_delaybatch_windows: window %lld run %d reads [%lld, %lld) of %lld samples", (long long)w, r, (long long)run[0],
                        (long long)(run[0] + run[1]), (long long)n_dec);
            total += run[1];
        }
        FRT_REQUIRE(total == length, "frt_delaybatch_windows: the runs of window %lld hold %lld samples, not %d", (long long)w, (long long)total, length);
    }
    DbScratch& sc = scratch();
    std::lock_guard<std::mutex> guard(sc.lock);
    int rc;
    const int S = n_streams;
    const int64_t pairs = (int64_t)S * W, per = pairs_full < pairs ? pairs_full : pairs;
    const size_t table_bytes = (size_t)W * kDbRuns * 4 * sizeof(int64_t);
    if ((rc = sc.runs.reserve(table_bytes)) || (rc = sc.stats.reserve((size_t)2 * S * W * kDbRuns * 3 * sizeof(double))) ||
        (rc = sc.d0.reserve((size_t)per * length * sizeof(double))) || (rc = sc.d1.reserve((size_t)per * length * sizeof(double))))
        return rc;
    FRT_HIP_CHECK(hipMemcpy(sc.runs.ptr, runs, table_bytes, hipMemcpyHostToDevice));        // waits for the launches that read the last table
    const long long* d_runs = sc.runs.as<long long>();
    hipLaunchKernelGGL(db_runstats_kernel, dim3((unsigned)(W * kDbRuns), 2 * S), dim3(256), 0, 0, dec, (long long)dec_stride, d_runs,
                       sc.stats.as<double>());
    hipLaunchKernelGGL(db_means_kernel, dim3((S + 63) / 64), dim3(64), 0, 0, sc.stats.as<double>(), d_runs, means_in, means_out, gated_out, S,
                       (long long)W, length);
    FRT_HIP_CHECK(hipGetLastError());
    int slabs = 0;
    for (int64_t q0 = 0; q0 < pairs; q0 += per, ++slabs) {
        const int64_t count = pairs - q0 < per ? pairs - q0 : per;
        FRT_REQUIRE(count == per || count == pairs - q0, "frt_delaybatch_windows: slab");
        hipLaunchKernelGGL(db_windows_kernel, dim3((length + 255) / 256, (unsigned)count), dim3(256), 0, 0, dec, (long long)dec_stride, d_runs,
                           means_in, means_out, sc.d0.as<double>(), sc.d1.as<double>(), (long long)q0, (long long)W, length);
        FRT_HIP_CHECK(hipGetLastError());
        // a handle's pair count is fixed: the full slabs' handle, and the last slab's own where it is shorter
        if ((rc = frt_gcc_phat(count == per ? gcc_full : gcc_last, sc.d0.as<double>(), sc.d1.as<double>(), xcorr + (size_t)q0 * length, nullptr,
                               nullptr)))
            return rc;
    }
    if (n_slabs_out) *n_slabs_out = slabs;
    return FRT_OK;
}

extern "C" int frt_delaybatch_readout(const double* xcorr, const int* gated, int n_streams, int64_t n_windows, int length,
                                      const double* smoothed_in, const int* present_in, double alpha, double sample_rate,
                                      double delayrange_s, double* smoothed_out, int* present_out, int* argmax_out, double* delay_ms_out,
                                      double* distance_m_out, double* extremum_out, int* correlation_out) {
    FRT_REQUIRE(n_streams >= 1 && n_streams <= 65535 && n_windows >= 0 && length >= 1 && sample_rate > 0, "frt_delaybatch_readout: bad shape");
    FRT_REQUIRE(smoothed_out && present_out, "frt_delaybatch_readout: null state");
    FRT_REQUIRE(n_windows == 0 || (xcorr && gated && argmax_out && delay_ms_out && distance_m_out && extremum_out && correlation_out),
                "frt_delaybatch_readout: null argument");
    DbScratch& sc = scratch();
    std::lock_guard<std::mutex> guard(sc.lock);
    int rc;
    const int S = n_streams, nseg = (length + kDbSeg - 1) / kDbSeg;
    const size_t cells = (size_t)S * (n_windows ? n_windows : 1);
    if ((rc = sc.psum.reserve(cells * nseg * sizeof(double))) || (rc = sc.pbest.reserve(cells * nseg * sizeof(double))) ||
        (rc = sc.pidx.reserve(cells * nseg * sizeof(int))) || (rc = sc.mean.reserve(cells * sizeof(double))))
        return rc;
    DbRead a{};
    a.xcorr = xcorr;
    a.gated = gated;
    a.sm_in = smoothed_in;
    a.present_in = present_in;
    a.sm_out = smoothed_out;
    a.present_out = present_out;
    a.psum = sc.psum.as<double>();
    a.pbest = sc.pbest.as<double>();
    a.pidx = sc.pidx.as<int>();
    a.mean = sc.mean.as<double>();
    a.W = n_windows;
    a.L = length;
    a.nseg = nseg;
    a.alpha = alpha;
    const dim3 wgrid(nseg, S), tgrid((unsigned)((cells + 255) / 256));
    hipLaunchKernelGGL(db_walk_kernel<0>, wgrid, dim3(kDbSeg), 0, 0, a);
    if (n_windows) {
        hipLaunchKernelGGL(db_peak_kernel, tgrid, dim3(256), 0, 0, a, S, sc.mean.as<double>(), argmax_out, extremum_out);
        hipLaunchKernelGGL(db_walk_kernel<1>, wgrid, dim3(kDbSeg), 0, 0, a);
        hipLaunchKernelGGL(db_readout_kernel, tgrid, dim3(256), 0, 0, a, S, argmax_out, extremum_out, sample_rate, delayrange_s, delay_ms_out,
                           distance_m_out, correlation_out);
    }
    FRT_HIP_CHECK(hipGetLastError());
    return FRT_OK;
}
