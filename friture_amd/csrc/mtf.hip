// mtf.hip — X5: modulation transfer of squared impulse responses and the Speech Transmission Index from it (frt_mtf_*,
// frt_sti_run; MtfBatch, sti_from_mtf).  The definition: X5 in include/friture_hip.h.
//
// Two kernels per slab of rows and one for the index; a wavefront never talks to another one inside a launch, nothing is atomic,
// no LDS besides the index's.
//   mtf_tiles: [start, stop) once.  A tile is kTile = 4096 samples and belongs to one wavefront (a row's workgroups walk its
//     tiles from start's to stop's; which workgroup takes a tile changes nothing).  Lane l holds the 64 squares e[q] of the
//     samples t = 4096 J + 64 q + l, loaded as they lie (every load of the wavefront is 64 consecutive samples, at any alignment
//     and dtype; the dtype is a branch at the load), 0 outside [start, stop).  The phasor of sample t is the product of three
//     table entries, coarse[J] lane[l] step[q], so that a sample costs one real-times-complex multiply-add per frequency:
//       per frequency  a = sum_q e[q] step[q] (fma; the even and the odd q are two chains, added at the end), a lane[l] (products
//                      rounded, then added), the 64 lanes folded by a butterfly (xor 32 .. 1), times coarse[J] on lane 0
//     and s0 = sum_q e[q], folded the same way.  The step entries are wavefront-uniform: they come through the scalar cache (the
//     tables are restrict kernel arguments for that reason).  The tile's 1 + 2 nf doubles go to scratch, component-major.
//   mtf_finish: one workgroup of 8 wavefronts per row; a wavefront takes S0 and the frequencies j = w, w + 8, .. and never needs
//     another one.  Lane i adds the values of tiles J0 + i, J0 + i + 64, .. in order, a butterfly folds the lanes; m[j] =
//     sqrt(re^2 + im^2) / S0.  A row with a bad interval is dead: NaN everywhere.
//   sti_rows: one wavefront per response, X5 steps 1 to 4.
// The tables are made on the host in long double; F t / fs is reduced to its fractional part exactly, in integers, before
// the cosine and sine are taken.  Every order above is anchored at sample 0 of the row: a row's bits depend on nothing else.
// The translation unit is compiled without floating-point contraction: the fused multiply-adds are the ones written out.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.h"
#include "rowfront.h"

using namespace frt;

namespace {

constexpr int kPer = 64, kTile = 64 * kPer, kWaves = 4, kFinishWaves = 8;
constexpr int kMaxFreqs = 16, kBands = 7;
constexpr long long kMaxTiles = kMaxSamples / kTile;

struct Call {
    const void* x;
    int dtype, nf;                                // 0 float32, 1 float64
    long long row_stride, T, ntile;
    const long long *start, *stop;                // [rows] or null: 0, T
    double* part;                                 // scratch [rows][1 + 2 nf][ntile]
    double *m, *energy;                           // [rows][nf], [rows]
};

// e[q] = x[t0 + 64 q]^2 where lo <= t < hi, 0 elsewhere.  Every load is issued, none behind a branch: one outside the interval
// reads the interval's nearest sample instead (lo < hi <= T: always inside the row) and is dropped by the select.
template <typename T>
__device__ __forceinline__ void load_squares(const T* __restrict__ x, long long t0, long long lo, long long hi, double (&e)[kPer]) {
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const long long t = t0 + 64 * q;
        const double v = (double)x[min(max(t, lo), hi - 1)];
        e[q] = (t >= lo && t < hi) ? v * v : 0.0;
    }
}

// the interval of a row; false: the row is dead (only device arrays can carry a bad one this far)
__device__ __forceinline__ bool interval(const Call& p, long long row, long long& lo, long long& hi) {
    lo = p.start ? p.start[row] : 0;
    hi = p.stop ? p.stop[row] : p.T;
    return lo >= 0 && lo < hi && hi <= p.T;
}

// step [nf][64]: exp(-2 pi i F 64 q / fs); lanes [nf][64]: exp(-2 pi i F l / fs); coarse [kMaxTiles][nf]: exp(-2 pi i F 4096 J / fs)
__global__ __launch_bounds__(64 * kWaves) void mtf_tiles(const Call p, const double2* __restrict__ step, const double2* __restrict__ lanes,
                                                         const double2* __restrict__ coarse) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nf = p.nf;
    const long long row = blockIdx.y;
    long long lo, hi;
    if (!interval(p, row, lo, hi)) return;
    const long long J1 = (hi - 1) / kTile;
    for (long long J = lo / kTile + (long long)blockIdx.x * kWaves + wave; J <= J1; J += (long long)gridDim.x * kWaves) {
        double e[kPer], s0 = 0.0;
        const long long t0 = J * kTile + lane;
        if (p.dtype) load_squares(reinterpret_cast<const double*>(p.x) + row * p.row_stride, t0, lo, hi, e);
        else load_squares(reinterpret_cast<const float*>(p.x) + row * p.row_stride, t0, lo, hi, e);
#pragma unroll
        for (int q = 0; q < kPer; ++q) s0 += e[q];
        double* part = p.part + row * (1 + 2 * nf) * p.ntile + J;
        s0 = fold_sum(s0);
        if (lane == 0) part[0] = s0;
        for (int j = 0; j < nf; ++j) {
            const double2* w = step + j * kPer;
            double ar0 = 0.0, ai0 = 0.0, ar1 = 0.0, ai1 = 0.0;
#pragma unroll
            for (int q = 0; q < kPer; q += 2) {
                ar0 = fma(e[q], w[q].x, ar0);
                ai0 = fma(e[q], w[q].y, ai0);
                ar1 = fma(e[q + 1], w[q + 1].x, ar1);
                ai1 = fma(e[q + 1], w[q + 1].y, ai1);
            }
            const double ar = ar0 + ar1, ai = ai0 + ai1;
            const double2 u = lanes[j * 64 + lane];
            const double sr = fold_sum(ar * u.x - ai * u.y), si = fold_sum(ar * u.y + ai * u.x);
            if (lane == 0) {
                const double2 c = coarse[J * nf + j];
                part[(1 + 2 * j) * p.ntile] = sr * c.x - si * c.y;
                part[(2 + 2 * j) * p.ntile] = sr * c.y + si * c.x;
            }
        }
    }
}

// the values of one component over the row's tiles: lane i adds tiles J0 + i, J0 + i + 64, .. in order, a butterfly folds the lanes
__device__ __forceinline__ double tile_sum(const double* v, long long J0, long long J1, int lane) {
    double s = 0.0;
#pragma unroll 8
    for (long long J = J0 + lane; J <= J1; J += 64) s += v[J];      // the loads of eight trips in flight, the additions in order
    return fold_sum(s);
}

__global__ __launch_bounds__(64 * kFinishWaves) void mtf_finish(const Call p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nf = p.nf;
    const long long row = blockIdx.x;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    long long lo, hi;
    if (!interval(p, row, lo, hi)) {
        if (wave == 0 && lane < nf) p.m[row * nf + lane] = nan;
        if (wave == 0 && lane == 0) p.energy[row] = nan;
        return;
    }
    const long long J0 = lo / kTile, J1 = (hi - 1) / kTile;
    const double* part = p.part + row * (1 + 2 * nf) * p.ntile;
    const double S0 = tile_sum(part, J0, J1, lane);              // every wavefront forms it for itself, in the same order
    if (wave == 0 && lane == 0) p.energy[row] = S0;
    for (int j = wave; j < nf; j += kFinishWaves) {
        const double re = tile_sum(part + (1 + 2 * j) * p.ntile, J0, J1, lane), im = tile_sum(part + (2 + 2 * j) * p.ntile, J0, J1, lane);
        if (lane == 0) p.m[row * nf + j] = sqrt(re * re + im * im) / S0;
    }
}

// ---- the index from m: X5, steps 1 to 4 ----------------------------------------------------------------------------------------

struct StiCall {
    const double *m, *a, *b;                      // [S][7][nf]; snr_db, or level_db and noise_db (or null): [S][7]
    int nf, correction;                           // 0 none, 1 snr_db, 2 levels
    const double* consts;                         // alpha [7] | beta [6] | reception threshold, dB [7] | mask [7][nf] as 0 or 1
    double *sti, *mti, *ti;
};

__device__ __forceinline__ double intensity(double db) { return exp10(db / 10.0); }

__device__ __forceinline__ double masking_db(double L) {
    if (L < 63.0) return 0.5 * L - 65.0;
    if (L < 67.0) return 1.8 * L - 146.9;
    if (L < 100.0) return 0.5 * L - 59.8;
    return -10.0;
}

__global__ __launch_bounds__(64) void sti_rows(const StiCall p) {
    __shared__ double t[kBands * kMaxFreqs], mt[kBands];
    const int lane = threadIdx.x, nf = p.nf;
    const long long s = blockIdx.x;
    for (int at = lane; at < kBands * nf; at += 64) {
        const int k = at / nf;
        double v = p.m[s * kBands * nf + at];
        if (p.correction == 1) {
            v = v / (1.0 + intensity(-p.a[s * kBands + k]));
        } else if (p.correction == 2) {
            const double I = intensity(p.a[s * kBands + k]), In = p.b ? intensity(p.b[s * kBands + k]) : 0.0;
            double Iam = 0.0;
            if (k > 0) {
                const double below = intensity(p.a[s * kBands + k - 1]) + (p.b ? intensity(p.b[s * kBands + k - 1]) : 0.0);
                Iam = below * intensity(masking_db(10.0 * log10(below)));
            }
            v = v * I / (I + In + Iam + intensity(p.consts[2 * kBands - 1 + k]));
        }
        double snr = 10.0 * log10(v / (1.0 - v));
        if (v >= 1.0 || snr > 15.0) snr = 15.0;                  // a NaN passes every comparison by
        if (v <= 0.0 || snr < -15.0) snr = -15.0;
        const double ti = (snr + 15.0) / 30.0;
        t[at] = ti;
        p.ti[s * kBands * nf + at] = ti;
    }
    wave_sync();
    if (lane < kBands) {
        double sum = 0.0, n = 0.0;
        for (int j = 0; j < nf; ++j) {
            if (p.consts[3 * kBands - 1 + lane * nf + j] != 0.0) {
                sum += t[lane * nf + j];
                n += 1.0;
            }
        }
        mt[lane] = sum / n;
        p.mti[s * kBands + lane] = sum / n;
    }
    wave_sync();
    if (lane == 0) {
        double v = 0.0;
        for (int k = 0; k < kBands; ++k) v += p.consts[k] * mt[k];
        for (int k = 0; k + 1 < kBands; ++k) v -= p.consts[kBands + k] * sqrt(mt[k] * mt[k + 1]);
        if (v > 1.0) v = 1.0;
        p.sti[s] = v;
    }
}

// exp(-2 pi i F t / fs), rounded once from long double.  The fractional part of F t / fs is formed in integers: F = a 2^p and
// fs = b 2^q with 53-bit a and b, so F t / fs = (a t 2^(p - e)) / (b 2^(q - e)), e = min(p, q), and the remainder of that
// division is exact.  (A frequency so far below fs that the integers would leave 128 bits has F t / fs < 1 for every t.)
double2 phasor(double F, long long t, double fs) {
    int p, q;
    const long double twopi = 6.283185307179586476925286766559005768L;
    const unsigned __int128 a = (unsigned __int128)std::ldexp(std::frexp(F, &p), 53), b = (unsigned __int128)std::ldexp(std::frexp(fs, &q), 53);
    const int e = std::min(p, q);
    long double cycles;
    if (p - e <= 40 && q - e <= 70) {
        const unsigned __int128 num = (a << (p - e)) * (unsigned __int128)t, den = b << (q - e);
        cycles = (long double)(num % den) / (long double)den;
    } else {
        cycles = (long double)F * (long double)t / (long double)fs;
        cycles -= floorl(cycles);
    }
    if (cycles >= 0.5L) cycles -= 1.0L;
    return make_double2((double)cosl(twopi * cycles), (double)-sinl(twopi * cycles));
}

}  // namespace

struct frt_mtf {
    double fs = 0;
    int nf = 0;
    hipStream_t stream = nullptr;
    std::vector<double2> host;                    // step | lane | coarse
    bool uploaded = false;
    DeviceBuffer tables, xin, sin, pin, mout, eout, scratch;
};

extern "C" int frt_mtf_tile(void) { return kTile; }

extern "C" int frt_mtf_create(frt_mtf** out, double fs, const double* freqs, int nf) {
    FRT_REQUIRE(out, "frt_mtf_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(std::isfinite(fs) && fs >= 100.0 && fs <= 1e7, "frt_mtf_create: fs %g (100 .. 1e7)", fs);
    FRT_REQUIRE(freqs && nf >= 1 && nf <= kMaxFreqs, "frt_mtf_create: %d frequencies (1 .. %d)", nf, kMaxFreqs);
    for (int j = 0; j < nf; ++j)
        FRT_REQUIRE(std::isfinite(freqs[j]) && freqs[j] > 0.0 && freqs[j] < fs / 2, "frt_mtf_create: freqs[%d] = %g (above 0, below fs / 2)", j, freqs[j]);
    frt_mtf* h = new frt_mtf();
    h->fs = fs;
    h->nf = nf;
    std::vector<double2>& tab = h->host;
    tab.reserve((size_t)nf * (kPer + 64 + kMaxTiles));
    for (int j = 0; j < nf; ++j)
        for (int q = 0; q < kPer; ++q) tab.push_back(phasor(freqs[j], 64LL * q, fs));
    for (int j = 0; j < nf; ++j)
        for (int l = 0; l < 64; ++l) tab.push_back(phasor(freqs[j], l, fs));
    for (long long J = 0; J < kMaxTiles; ++J)
        for (int j = 0; j < nf; ++j) tab.push_back(phasor(freqs[j], J * kTile, fs));
    *out = h;
    return FRT_OK;
}

extern "C" void frt_mtf_destroy(frt_mtf* h) {
    if (!h) return;
    destroy_handle(h, {&h->tables, &h->xin, &h->sin, &h->pin, &h->mout, &h->eout, &h->scratch});
}

extern "C" int frt_mtf_set_stream(frt_mtf* h, void* s) {
    FRT_REQUIRE(h, "frt_mtf_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_mtf_run(frt_mtf* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, const int64_t* start,
                           const int64_t* stop, int64_t scratch_bytes, double* m, double* energy) {
    FRT_REQUIRE(h, "frt_mtf_run: null handle");
    int rc;
    if ((rc = require_rows("frt_mtf_run", x, x_dtype, rows, n, row_stride, scratch_bytes))) return rc;
    FRT_REQUIRE(m && energy, "frt_mtf_run: null output");
    const long long T = n, R = rows;
    if ((rc = require_row_integers("frt_mtf_run", "start", start, R, 0, T - 1, "0 .. n - 1"))) return rc;
    if ((rc = require_row_integers("frt_mtf_run", "stop", stop, R, 1, T, "1 .. n"))) return rc;
    if ((start || stop) && !is_device_pointer(start) && !is_device_pointer(stop))        // the host sees the intervals whole
        for (long long r = 0; r < R; ++r) {
            const long long lo = start ? start[r] : 0, hi = stop ? stop[r] : T;
            FRT_REQUIRE(lo < hi, "frt_mtf_run: start[%lld] = %lld is not below stop = %lld", r, lo, hi);
        }

    const int nf = h->nf, np = 1 + 2 * nf;
    if (!h->uploaded) {
        if ((rc = h->tables.reserve(h->host.size() * sizeof(double2)))) return rc;
        FRT_HIP_CHECK(hipMemcpyAsync(h->tables.ptr, h->host.data(), h->host.size() * sizeof(double2), hipMemcpyHostToDevice, h->stream));
        h->uploaded = true;
    }
    Call p{};
    p.x = x;
    p.dtype = x_dtype;
    p.nf = nf;
    p.row_stride = row_stride;
    p.T = T;
    p.ntile = (T + kTile - 1) / kTile;
    const double2 *step = h->tables.as<const double2>(), *lanes = step + nf * kPer, *coarse = lanes + nf * 64;

    HostIO io(h->stream);
    const size_t xsize = x_dtype ? sizeof(double) : sizeof(float);
    const long long* lo = reinterpret_cast<const long long*>(start);
    const long long* hi = reinterpret_cast<const long long*>(stop);
    if ((rc = io.in_rows(h->xin, p.x, p.row_stride, (size_t)R, T, xsize))) return rc;
    if ((rc = io.in(h->sin, lo, (size_t)R))) return rc;
    if ((rc = io.in(h->pin, hi, (size_t)R))) return rc;
    if ((rc = io.out(h->mout, m, (size_t)R * nf))) return rc;
    if ((rc = io.out(h->eout, energy, (size_t)R))) return rc;

    long long slab;
    if ((rc = reserve_slab(h->scratch, R, scratch_bytes, p.ntile * np * (long long)sizeof(double), slab))) return rc;
    p.part = h->scratch.as<double>();
    const char* x0 = reinterpret_cast<const char*>(p.x);
    for (long long r0 = 0; r0 < R; r0 += slab) {
        const unsigned nr = (unsigned)std::min(slab, R - r0);
        Call c = p;
        c.x = x0 + (size_t)r0 * (size_t)p.row_stride * xsize;
        c.start = lo ? lo + r0 : nullptr;
        c.stop = hi ? hi + r0 : nullptr;
        c.m = m + r0 * nf;
        c.energy = energy + r0;
        hipLaunchKernelGGL(mtf_tiles, dim3(tile_groups(p.ntile, nr, kWaves), nr), dim3(64 * kWaves), 0, h->stream, c, step, lanes, coarse);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mtf_finish, dim3(nr), dim3(64 * kFinishWaves), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return io.finish();
}

extern "C" int frt_sti_run(const double* m, int responses, int nf, int correction, const double* a, const double* b, const double* alpha,
                           const double* beta, const unsigned char* mask, double* sti, double* mti, double* ti, void* hip_stream) {
    FRT_REQUIRE(responses >= 1 && responses <= (1 << 24), "frt_sti_run: %d responses (1 .. 2^24)", responses);
    FRT_REQUIRE(nf >= 1 && nf <= kMaxFreqs, "frt_sti_run: %d frequencies (1 .. %d)", nf, kMaxFreqs);
    FRT_REQUIRE(correction >= 0 && correction <= 2, "frt_sti_run: correction %d (0 none, 1 snr_db, 2 levels)", correction);
    FRT_REQUIRE((correction != 0) == (a != nullptr) && (correction == 2 || !b), "frt_sti_run: correction %d with%s a first and with%s a second array",
                correction, a ? "" : "out", b ? "" : "out");
    FRT_REQUIRE(m && alpha && beta && mask && sti && mti && ti, "frt_sti_run: null buffer");
    StiCall p{};
    p.nf = nf;
    p.correction = correction;
    const double threshold[kBands] = {46.0, 27.0, 12.0, 6.5, 7.5, 8.0, 12.0};
    std::vector<double> consts(3 * kBands - 1 + kBands * nf);
    for (int k = 0; k < kBands; ++k) {
        int used = 0;
        for (int j = 0; j < nf; ++j) used += (int)(consts[3 * kBands - 1 + k * nf + j] = mask[k * nf + j] ? 1.0 : 0.0);
        FRT_REQUIRE(used > 0, "frt_sti_run: band %d has no modulation frequency in the mask", k);
        consts[k] = alpha[k];
        consts[2 * kBands - 1 + k] = threshold[k];
        if (k + 1 < kBands) consts[kBands + k] = beta[k];
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    // a stateless call: its staging blocks are allocated and freed here
    DeviceBuffer min, ain, bin, cin, sout, mout, tout;
    auto run = [&]() -> int {
        int rc;
        HostIO io(stream);
        const size_t S = (size_t)responses;
        if ((rc = io.in(min, m, S * kBands * nf))) return rc;
        if ((rc = io.in(ain, a, S * kBands))) return rc;
        if ((rc = io.in(bin, b, S * kBands))) return rc;
        p.consts = consts.data();
        if ((rc = io.in(cin, p.consts, consts.size()))) return rc;
        if ((rc = io.out(sout, sti, S))) return rc;
        if ((rc = io.out(mout, mti, S * kBands))) return rc;
        if ((rc = io.out(tout, ti, S * kBands * nf))) return rc;
        p.m = m;
        p.a = a;
        p.b = b;
        p.sti = sti;
        p.mti = mti;
        p.ti = ti;
        hipLaunchKernelGGL(sti_rows, dim3((unsigned)responses), dim3(64), 0, stream, p);
        FRT_HIP_CHECK(hipGetLastError());
        return io.finish();
    };
    const int rc = run();
    for (DeviceBuffer* buf : {&min, &ain, &bin, &cin, &sout, &mout, &tout}) buf->release();
    return rc;
}
