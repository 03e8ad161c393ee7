// decay.hip — X3: reverberation time and clarity from impulse responses (frt_decay_*, DecayBatch).  The definition: X3 in
// include/friture_hip.h.
//
// Six kernels per slab of rows; a wavefront never talks to another one inside a launch, nothing is atomic.
//   dk_front: the samples once.  A group of G lanes (64, or 8 for blocks below 64 samples) takes one block of W samples:
//     lane i adds e[k W + i], e[k W + i + G], .. in order, the G lane sums fold by a butterfly (xor G / 2 .. 1).  q[k] and
//     m[k] = max |x| of the block, +inf when it holds a sample that is not finite.  The remainder behind the last whole
//     block is block nb: it counts for the peak and the onset, not for the noise.
//   dk_plan: one wavefront per row.  Peak and onset from m (only the one block that holds each is read again), N0, the
//     truncation from q, the checks that make a row dead.
//   dk_totals: [t0, t1) once (a row's workgroups walk its tiles from the onset's to the truncation's; which workgroup takes a
//     tile changes nothing).  A tile is kTile = 512 samples, one wavefront, 8 consecutive samples per lane (loaded
//     coalesced, turned through the wavefront's LDS).  Its total is the first value of its own suffix scan (tile_suffix).
//   dk_offsets: one wavefront per row.  off[j] = the totals of the tiles behind tile j, added one by one from the row's last
//     tile down (so E is the same number on both sides of a tile seam); E[t0]; the absolute thresholds E[t0] 10^(lo / 10).
//   dk_scan: [t0, t1) a second time.  E[t] = ((e[t] + .. + e[last of the lane]) + the lanes behind, a Kogge-Stone scan) +
//     off[tile].  A sample belongs to the segment its E falls in (above -5 dB, -5 .. -10, -10 .. -15, -15 .. -25, -25 .. -35);
//     L = 10 log10(E / E[t0]) is formed only where a segment or the curve needs it.  Per tile: how many samples lie above
//     each threshold (ballots), per segment that the tile touches the sums of L, (t - t0) L and L^2, and sum (t - t0) e:
//     lane sums in sample order, folded by a butterfly.  E[t0 + n50], E[t0 + n80] and the curve samples are stored by the lane that holds them.
//   dk_finish: one wavefront per row.  Lane i adds the partials of tiles j0 + i, j0 + i + 64, .. in order, a butterfly folds
//     the lanes; then the crossings from the counts, the four fits from the segment sums (EDT = the first two segments,
//     T10 / T20 / T30 = segments two to three / four / five), the ratios, and the 15 doubles and 3 integers of the row.
// The sums run on L itself, not on L - hi: slope and r2 do not depend on the shift, and with |L| <= 35 the cancellation in
// n sum L^2 - (sum L)^2 is a factor of 6 without the shift and 4 with it.  sum k^2 - (sum k)^2 / n is the closed form
// n (n^2 - 1) / 12.  Every order above is anchored at sample 0 of the row: a row's bits depend on nothing else.
// The translation unit is compiled without floating-point contraction: e[t] is a rounded square, then added.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.h"
#include "rowfront.h"

using namespace frt;

namespace {

constexpr int kPer = 8, kTile = 64 * kPer, kWaves = 4;       // samples per lane, per tile; wavefronts per workgroup
constexpr int kLdsPerWave = kTile + kTile / 8;               // a tile of doubles, one pad behind every 8
constexpr int kParts = 21;                                   // 5 counts | 5 x (sum L, sum u L, sum L^2) | sum u e
constexpr int kParams = 15, kIndices = 3;

struct RowRec {
    long long t0, t1, peak;
    int dead;
    double N0, maxq, E0, thr[5], E50, E80;
};

struct Call {
    const void* x;
    int dtype;                                    // 0 float32, 1 float64
    long long row_stride, T;
    long long W, nb, nblk, nt, ntile;             // block; whole blocks; blocks with the remainder; noise blocks; tiles
    double c, mf, fs;                             // 10^(onset_db / 20), 10^(margin_db / 10)
    long long n50, n80;
    double f[5];                                  // 10^(lo / 10), lo = -5, -10, -15, -25, -35
    const long long* onset;                       // [rows] or null
    int trunc_mode;                               // 0: t1 = T, 1: auto, 2: given
    const long long* trunc;
    long long step, nc;                           // curve: L[t0 + j step], j < nc (step 0: no curve)
    double *q, *m, *total, *off, *part;           // scratch: [rows][nblk] x 2, [rows][ntile] x 2, [rows][ntile][kParts]
    RowRec* rec;
    double* params;                               // [rows][15]
    long long* idx;                               // [rows][3]
    double* curve;                                // [rows][nc]
};

__device__ __forceinline__ double sample_at(const Call& p, long long row, long long t) {
    const long long at = row * p.row_stride + t;
    return p.dtype ? reinterpret_cast<const double*>(p.x)[at] : (double)reinterpret_cast<const float*>(p.x)[at];
}

template <int G>
__global__ __launch_bounds__(64 * kWaves) void dk_front(const Call p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / G, i = lane % G;
    const long long row = blockIdx.y;
    const long long k = ((long long)blockIdx.x * kWaves + wave) * (64 / G) + g;
    double s = 0.0, mx = 0.0;
    bool bad = false;
    if (k < p.nblk) {
        const long long a = k * p.W, b = min(a + p.W, p.T);
        for (long long t = a + i; t < b; t += G) {
            const double v = sample_at(p, row, t), av = fabs(v);
            bad |= !(av < std::numeric_limits<double>::infinity());
            mx = fmax(mx, av);
            s += v * v;
        }
    }
    if (bad) mx = std::numeric_limits<double>::infinity();
    s = fold_sum<G>(s);
    mx = fold_max<G>(mx);
    if (k < p.nblk && i == 0) {
        p.q[row * p.nblk + k] = s;
        p.m[row * p.nblk + k] = mx;
    }
}

// the smallest k in [a, b) with v[k] >= bound (LE: v[k] <= bound), -1 if there is none; the whole wavefront calls it
template <bool LE>
__device__ __forceinline__ long long first_block(const double* v, long long a, long long b, double bound, int lane) {
    for (long long k0 = a; k0 < b; k0 += 64) {
        const long long k = k0 + lane;
        const bool hit = k < b && (LE ? v[k] <= bound : v[k] >= bound);
        const unsigned long long mask = __ballot(hit);
        if (mask) return k0 + __builtin_ctzll(mask);
    }
    return -1;
}

// the smallest t in [a, b) with |x[t]| >= bound, -1 if there is none
__device__ __forceinline__ long long first_sample(const Call& p, long long row, long long a, long long b, double bound, int lane) {
    for (long long t0 = a; t0 < b; t0 += 64) {
        const long long t = t0 + lane;
        const bool hit = t < b && fabs(sample_at(p, row, t)) >= bound;
        const unsigned long long mask = __ballot(hit);
        if (mask) return t0 + __builtin_ctzll(mask);
    }
    return -1;
}

__global__ __launch_bounds__(64) void dk_plan(const Call p) {
    const int lane = threadIdx.x;
    const long long row = blockIdx.x;
    const double* q = p.q + row * p.nblk;
    const double* m = p.m + row * p.nblk;
    const double inf = std::numeric_limits<double>::infinity();
    double M = 0.0;
    for (long long k = lane; k < p.nblk; k += 64) M = fmax(M, m[k]);
    M = fold_max(M);
    bool dead = !(M > 0.0) || M == inf;                          // all zero, or a sample that is not finite
    long long t0 = -1, t1 = -1, peak = -1;
    double N0 = 0.0, maxq = 0.0;
    if (!dead) {                                                 // the same on every lane
        const long long kp = first_block<false>(m, 0, p.nblk, M, lane);
        peak = kp < 0 ? -1 : first_sample(p, row, kp * p.W, min((kp + 1) * p.W, p.T), M, lane);
        if (p.onset) {
            t0 = p.onset[row];
        } else {
            const double bound = p.c * M;
            const long long ko = first_block<false>(m, 0, p.nblk, bound, lane);
            t0 = ko < 0 ? -1 : first_sample(p, row, ko * p.W, min((ko + 1) * p.W, p.T), bound, lane);
        }
        if (p.nb > 0) {
            double s = 0.0;
            for (long long k = p.nb - p.nt + lane; k < p.nb; k += 64) s += q[k];
            N0 = fold_sum(s) / ((double)p.nt * (double)p.W);
            for (long long k = lane; k < p.nb; k += 64) maxq = fmax(maxq, q[k]);
            maxq = fold_max(maxq);
        }
        t1 = p.T;
        if (p.trunc_mode == 2) {
            t1 = p.trunc[row];
        } else if (p.trunc_mode == 1 && peak >= 0) {
            const long long k = first_block<true>(q, peak / p.W + 1, p.nb, ((double)p.W * N0) * p.mf, lane);
            if (k >= 0) t1 = k * p.W;
        }
        dead = peak < 0 || t0 < 0 || t0 >= p.T || t1 <= t0 || t1 > p.T;
    }
    if (lane == 0) {
        RowRec& r = p.rec[row];
        r.t0 = t0;
        r.t1 = t1;
        r.peak = peak;
        r.dead = dead ? 1 : 0;
        r.N0 = N0;
        r.maxq = maxq;
        r.E0 = 0.0;
        r.E50 = r.E80 = 0.0;
#pragma unroll
        for (int j = 0; j < 5; ++j) r.thr[j] = 0.0;
    }
}

// e[j] = x[ts + 8 lane + j]^2 where lo <= t < hi, 0 elsewhere: loaded 64 consecutive samples at a time, turned through buf
__device__ __forceinline__ void load_tile(const Call& p, long long row, long long ts, long long lo, long long hi, double* buf, int lane,
                                          double (&e)[kPer]) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int s = lane + 64 * j;
        const long long t = ts + s;
        const double v = (t >= lo && t < hi) ? sample_at(p, row, t) : 0.0;
        buf[s + (s >> 3)] = v * v;
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < kPer; ++j) e[j] = buf[9 * lane + j];
    wave_sync();
}

// e[j] becomes e[j] + .. + e[7] of the lane; excl = the lanes behind this one (a Kogge-Stone scan of the lane totals)
__device__ __forceinline__ void tile_suffix(double (&e)[kPer], int lane, double& excl) {
#pragma unroll
    for (int j = kPer - 2; j >= 0; --j) e[j] += e[j + 1];
    double incl = e[0];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(incl, d);
        if (lane + d < 64) incl += o;
    }
    excl = __shfl_down(incl, 1);
    if (lane == 63) excl = 0.0;
}

__global__ __launch_bounds__(64 * kWaves) void dk_totals(const Call p) {
    __shared__ double lds[kWaves][kLdsPerWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = blockIdx.y;
    const RowRec& r = p.rec[row];
    if (r.dead) return;
    const long long t0 = r.t0, t1 = r.t1, j1 = (t1 - 1) / kTile;
    // the workgroups of a row share its tiles from the onset's to the truncation's, whatever their number
    for (long long j = t0 / kTile + (long long)blockIdx.x * kWaves + wave; j <= j1; j += (long long)gridDim.x * kWaves) {
        double e[kPer], excl;
        load_tile(p, row, j * kTile, t0, t1, lds[wave], lane, e);
        tile_suffix(e, lane, excl);
        if (lane == 0) p.total[row * p.ntile + j] = e[0] + excl;
    }
}

__global__ __launch_bounds__(64) void dk_offsets(const Call p) {
    const int lane = threadIdx.x;
    const long long row = blockIdx.x;
    RowRec& r = p.rec[row];
    if (r.dead) return;
    const long long j0 = r.t0 / kTile, j1 = (r.t1 - 1) / kTile;
    const double* total = p.total + row * p.ntile;
    double* off = p.off + row * p.ntile;
    double acc = 0.0;                                            // the same on every lane
    for (long long top = j1; top >= j0; top -= 64) {
        const long long j = top - lane;
        const double v = j >= j0 ? total[j] : 0.0;
        double mine = 0.0;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            if (lane == i) mine = acc;
            acc += __shfl(v, i);
        }
        if (j >= j0) off[j] = mine;
    }
    if (lane == 0) {
        r.E0 = acc;
#pragma unroll
        for (int j = 0; j < 5; ++j) r.thr[j] = acc * p.f[j];
    }
}

// one tile of dk_scan: tile j of `row`, buf the wavefront's LDS
__device__ __forceinline__ void scan_tile(const Call& p, RowRec& r, long long row, long long j, long long t0, long long t1, double E0,
                                          const double (&thr)[5], double* buf, int lane) {
    const long long ts = j * kTile;
    const double off = p.off[row * p.ntile + j];
    double e[kPer], suf[kPer], excl;
    load_tile(p, row, ts, t0, t1, buf, lane, e);
#pragma unroll
    for (int i = 0; i < kPer; ++i) suf[i] = e[i];
    tile_suffix(suf, lane, excl);

    // pass 1: E, the segment of every sample, the counts above each threshold (the same on every lane), L where it is needed
    int cnt[5] = {0, 0, 0, 0, 0}, seg[kPer];
    double L[kPer], ue = 0.0;
    unsigned touched = 0;
    const long long u50 = t0 + p.n50, u80 = t0 + p.n80;
    double* curve = p.curve ? p.curve + row * p.nc : nullptr;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const long long t = ts + kPer * lane + i;
        const bool valid = t >= t0 && t < t1;
        const double E = (suf[i] + excl) + off;
        seg[i] = 0;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            seg[i] += E <= thr[s] ? 1 : 0;
            cnt[s] += __popcll(__ballot(valid && E > thr[s]));
        }
        if (!valid) seg[i] = 5;
        const bool on_curve = curve && valid && (t - t0) % p.step == 0;
        L[i] = 0.0;
        if (seg[i] < 5 || on_curve) L[i] = 10.0 * log10(E / E0);
        if (on_curve) curve[(t - t0) / p.step] = L[i];
        if (valid) {
            if (seg[i] < 5) touched |= 1u << seg[i];
            ue += (double)(t - t0) * e[i];
            if (t == u50) r.E50 = E;
            if (t == u80) r.E80 = E;
        }
    }
    // pass 2: the sums of the segments that the tile touches (L is monotone: one or two of them, as a rule)
    double out[kParts];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        out[s] = (double)cnt[s];
        out[5 + 3 * s] = out[6 + 3 * s] = out[7 + 3 * s] = 0.0;
        if (__ballot((touched >> s) & 1u) != 0) {                // the same on every lane
            double sL = 0.0, sU = 0.0, sQ = 0.0;
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                if (seg[i] == s) {
                    sL += L[i];
                    sU += (double)(ts + kPer * lane + i - t0) * L[i];
                    sQ += L[i] * L[i];
                }
            }
            out[5 + 3 * s] = fold_sum(sL);
            out[6 + 3 * s] = fold_sum(sU);
            out[7 + 3 * s] = fold_sum(sQ);
        }
    }
    out[20] = fold_sum(ue);
    if (lane == 0) {
        double* part = p.part + (row * p.ntile + j) * kParts;
#pragma unroll
        for (int i = 0; i < kParts; ++i) part[i] = out[i];
    }
}

__global__ __launch_bounds__(64 * kWaves) void dk_scan(const Call p) {
    __shared__ double lds[kWaves][kLdsPerWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = blockIdx.y;
    RowRec& r = p.rec[row];
    if (r.dead) return;
    const long long t0 = r.t0, t1 = r.t1, j1 = (t1 - 1) / kTile;
    const double E0 = r.E0;
    double thr[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) thr[s] = r.thr[s];
    for (long long j = t0 / kTile + (long long)blockIdx.x * kWaves + wave; j <= j1; j += (long long)gridDim.x * kWaves)
        scan_tile(p, r, row, j, t0, t1, E0, thr, lds[wave], lane);
}

// the curve entries that no tile writes: those at or behind t1, and every entry of a dead row
__global__ void dk_curve_tail(const Call p) {
    const long long row = blockIdx.y, j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.nc) return;
    const RowRec& r = p.rec[row];
    if (r.dead || r.t0 + j * p.step >= r.t1) p.curve[row * p.nc + j] = std::numeric_limits<double>::quiet_NaN();
}

__global__ __launch_bounds__(64) void dk_finish(const Call p) {
    const int lane = threadIdx.x;
    const long long row = blockIdx.x;
    const RowRec& r = p.rec[row];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double* o = p.params + row * kParams;
    long long* ix = p.idx + row * kIndices;
    if (r.dead) {
        if (lane < kParams) o[lane] = nan;
        if (lane < kIndices) ix[lane] = -1;
        return;
    }
    const long long t0 = r.t0, t1 = r.t1, j0 = t0 / kTile, j1 = (t1 - 1) / kTile;
    double v[kParts];
#pragma unroll
    for (int i = 0; i < kParts; ++i) v[i] = 0.0;
    for (long long j = j0 + lane; j <= j1; j += 64) {
        const double* part = p.part + (row * p.ntile + j) * kParts;
#pragma unroll
        for (int i = 0; i < kParts; ++i) v[i] += part[i];
    }
#pragma unroll
    for (int i = 0; i < kParts; ++i) v[i] = fold_sum(v[i]);
    if (lane != 0) return;
    const double E0 = r.E0, span = (double)(t1 - t0);
    // crossing s: the smallest t with L[t] <= lo[s] is t0 + v[s]; reached when it lies before t1
    for (int fit = 0; fit < 4; ++fit) {
        const int first = fit ? 1 : 0, last = fit ? fit + 1 : 1;   // segments first .. last; the range ends at crossing `last`
        const double a = fit ? v[0] : 0.0, b = v[last], n = b - a;
        double rt = nan, r2 = nan;
        if (b < span && n >= 2.0) {
            double SL = 0.0, SU = 0.0, SQ = 0.0;
            for (int s = first; s <= last; ++s) {
                SL += v[5 + 3 * s];
                SU += v[6 + 3 * s];
                SQ += v[7 + 3 * s];
            }
            const double SkL = SU - a * SL, Sk = n * (n - 1.0) / 2.0;
            const double cov = n * SkL - Sk * SL, vk = n * n * (n * n - 1.0) / 12.0, vl = n * SQ - SL * SL;
            rt = -60.0 / ((cov / vk) * p.fs);
            r2 = (cov * cov) / (vk * vl);
        }
        o[fit] = rt;
        o[4 + fit] = r2;
    }
    const double E50 = r.E50, E80 = r.E80;
    o[8] = 10.0 * log10((E0 - E50) / E50);
    o[9] = 10.0 * log10((E0 - E80) / E80);
    o[10] = (E0 - E50) / E0;
    o[11] = v[20] / E0 / p.fs;
    o[12] = 10.0 * log10(E0);
    o[13] = 10.0 * log10(r.N0);
    o[14] = p.nb == 0 ? nan : (r.N0 == 0.0 ? inf : 10.0 * log10(r.maxq / ((double)p.W * r.N0)));
    ix[0] = r.peak;
    ix[1] = t0;
    ix[2] = t1;
}

}  // namespace

struct frt_decay {
    double fs = 0, c = 0, mf = 0, noise_tail = 0;
    int W = 0;
    long long n50 = 0, n80 = 0;
    hipStream_t stream = nullptr;
    DeviceBuffer xin, oin, tin, pout, iout, cout, scratch;
};

extern "C" int frt_decay_tile(void) { return kTile; }

extern "C" int frt_decay_create(frt_decay** out, double fs, int block, double onset_db, double noise_tail, double margin_db) {
    FRT_REQUIRE(out, "frt_decay_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(std::isfinite(fs) && fs >= 100.0 && fs <= 1e7, "frt_decay_create: fs %g (100 .. 1e7)", fs);
    FRT_REQUIRE(block >= 8 && block <= 65536, "frt_decay_create: block %d (8 .. 65536)", block);
    FRT_REQUIRE(std::isfinite(onset_db) && onset_db <= 0.0, "frt_decay_create: onset_db %g (at most 0)", onset_db);
    FRT_REQUIRE(noise_tail > 0.0 && noise_tail <= 1.0, "frt_decay_create: noise_tail %g (above 0, at most 1)", noise_tail);
    FRT_REQUIRE(std::isfinite(margin_db) && margin_db >= 0.0, "frt_decay_create: margin_db %g (at least 0)", margin_db);
    frt_decay* h = new frt_decay();
    h->fs = fs;
    h->W = block;
    h->c = std::pow(10.0, onset_db / 20.0);
    h->mf = std::pow(10.0, margin_db / 10.0);
    h->noise_tail = noise_tail;
    h->n50 = (long long)std::floor(0.05 * fs + 0.5);
    h->n80 = (long long)std::floor(0.08 * fs + 0.5);
    *out = h;
    return FRT_OK;
}

extern "C" void frt_decay_destroy(frt_decay* h) {
    if (!h) return;
    destroy_handle(h, {&h->xin, &h->oin, &h->tin, &h->pout, &h->iout, &h->cout, &h->scratch});
}

extern "C" int frt_decay_set_stream(frt_decay* h, void* s) {
    FRT_REQUIRE(h, "frt_decay_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_decay_run(frt_decay* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, const int64_t* onset,
                             int truncate_mode, const int64_t* truncation, int64_t curve_step, int64_t scratch_bytes, double* params,
                             int64_t* indices, double* curve) {
    FRT_REQUIRE(h, "frt_decay_run: null handle");
    int rc;
    if ((rc = require_rows("frt_decay_run", x, x_dtype, rows, n, row_stride, scratch_bytes))) return rc;
    FRT_REQUIRE(truncate_mode >= 0 && truncate_mode <= 2, "frt_decay_run: truncate_mode %d (0 none, 1 auto, 2 given)", truncate_mode);
    FRT_REQUIRE((truncate_mode == 2) == (truncation != nullptr), "frt_decay_run: truncation is given with truncate_mode 2 and only then");
    FRT_REQUIRE(curve_step >= 0 && (curve_step > 0) == (curve != nullptr), "frt_decay_run: curve_step %lld %s a curve",
                (long long)curve_step, curve ? "with" : "without");
    FRT_REQUIRE(params && indices, "frt_decay_run: null output");
    const long long T = n, W = h->W, R = rows;
    if ((rc = require_row_integers("frt_decay_run", "onset", onset, R, 0, T - 1, "0 .. n - 1"))) return rc;
    if ((rc = require_row_integers("frt_decay_run", "truncation", truncation, R, 1, T, "1 .. n"))) return rc;

    Call p{};
    p.x = x;
    p.dtype = x_dtype;
    p.row_stride = row_stride;
    p.T = T;
    p.W = W;
    p.nb = T / W;
    p.nblk = (T + W - 1) / W;
    p.nt = std::max(1LL, (long long)std::ceil(h->noise_tail * (double)p.nb));
    p.nt = std::min(p.nt, std::max(1LL, p.nb));
    p.ntile = (T + kTile - 1) / kTile;
    p.c = h->c;
    p.mf = h->mf;
    p.fs = h->fs;
    p.n50 = h->n50;
    p.n80 = h->n80;
    const double lows[5] = {-5.0, -10.0, -15.0, -25.0, -35.0};
    for (int j = 0; j < 5; ++j) p.f[j] = std::pow(10.0, lows[j] / 10.0);
    p.trunc_mode = truncate_mode;
    p.step = curve_step;
    p.nc = curve_step ? (T + curve_step - 1) / curve_step : 0;

    HostIO io(h->stream);
    const size_t xsize = x_dtype ? sizeof(double) : sizeof(float);
    const long long* on = reinterpret_cast<const long long*>(onset);
    const long long* tr = reinterpret_cast<const long long*>(truncation);
    long long* ix = reinterpret_cast<long long*>(indices);
    if ((rc = io.in_rows(h->xin, p.x, p.row_stride, (size_t)R, T, xsize))) return rc;
    if ((rc = io.in(h->oin, on, (size_t)R))) return rc;
    if ((rc = io.in(h->tin, tr, (size_t)R))) return rc;
    if ((rc = io.out(h->pout, params, (size_t)R * kParams))) return rc;
    if ((rc = io.out(h->iout, ix, (size_t)R * kIndices))) return rc;
    if ((rc = io.out(h->cout, curve, (size_t)R * p.nc))) return rc;

    const long long doubles = 2 * p.nblk + (2 + kParts) * p.ntile;
    const long long per_row = doubles * (long long)sizeof(double) + (long long)sizeof(RowRec);
    long long slab;
    if ((rc = reserve_slab(h->scratch, R, scratch_bytes, per_row, slab))) return rc;
    double* at = h->scratch.as<double>();
    p.q = at;
    p.m = (at += slab * p.nblk);
    p.total = (at += slab * p.nblk);
    p.off = (at += slab * p.ntile);
    p.part = (at += slab * p.ntile);
    p.rec = reinterpret_cast<RowRec*>(at + slab * p.ntile * kParts);
    const char* x0 = reinterpret_cast<const char*>(p.x);
    const int G = W >= 64 ? 64 : 8;
    const unsigned front_groups = (unsigned)((p.nblk + kWaves * (64 / G) - 1) / (kWaves * (64 / G)));
    for (long long r0 = 0; r0 < R; r0 += slab) {
        const unsigned nr = (unsigned)std::min(slab, R - r0);
        const unsigned groups = tile_groups(p.ntile, nr, kWaves);        // dk_totals, dk_scan: the workgroups of a row loop over its live tiles
        Call c = p;
        c.x = x0 + (size_t)r0 * (size_t)p.row_stride * xsize;
        c.onset = on ? on + r0 : nullptr;
        c.trunc = tr ? tr + r0 : nullptr;
        c.params = params + r0 * kParams;
        c.idx = ix + r0 * kIndices;
        c.curve = curve ? curve + r0 * p.nc : nullptr;
        if (G == 64) hipLaunchKernelGGL(dk_front<64>, dim3(front_groups, nr), dim3(64 * kWaves), 0, h->stream, c);
        else hipLaunchKernelGGL(dk_front<8>, dim3(front_groups, nr), dim3(64 * kWaves), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(dk_plan, dim3(nr), dim3(64), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(dk_totals, dim3(groups, nr), dim3(64 * kWaves), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(dk_offsets, dim3(nr), dim3(64), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        if (c.curve) {
            hipLaunchKernelGGL(dk_curve_tail, dim3((unsigned)((p.nc + 255) / 256), nr), dim3(256), 0, h->stream, c);
            FRT_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(dk_scan, dim3(groups, nr), dim3(64 * kWaves), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(dk_finish, dim3(nr), dim3(64), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return io.finish();
}
