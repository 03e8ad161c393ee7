// spatial.hip — X8: inter-aural cross-correlation and lateral energy from pairs of responses (frt_spatial_*, SpatialBatch).  The
// definition: X8 in include/friture_hip.h.
//
// Five kernels per slab of pairs; a workgroup never talks to another one inside a launch, nothing is atomic.
//   sp_front: both rows once, [0, e).  One wavefront per block of kFront = 1024 samples: m[k] = max(|l|, |r|) of the block, +inf
//     when it holds a sample that is not finite.
//   sp_plan: one wavefront per pair.  Peak and onset from m (only the one block that holds each is read again), the windows
//     [A_w, B_w), their distinct ends sorted into cut points, the live segments between them (a segment that no window covers is
//     not summed) and the tiles of each, counted from the segment's start.
//   sp_corr<NGW>: the work.  A workgroup of four wavefronts takes one tile of kTile = 2048 samples of one segment at a time
//     (a pair's workgroups share its tiles, whatever their number).  The tile of l (zero behind the tile's end) and the tile of r
//     with Mp samples in front and what the lags reach behind it (zero outside [0, e)) are staged in LDS in blocks of 8
//     doubles with 2 doubles of padding behind each (80 bytes: the 16-byte reads of 16 lanes at that stride fall on 16
//     different groups of four banks).  Mp = 8 ceil(M / 8), so that lag 0 opens a group of 8 lags: group g holds the lags
//     -Mp + 8 g .. -Mp + 8 g + 7 (those below -M are computed and dropped).  Wavefront w owns the groups w, w + 4, ..; lane i
//     walks the blocks i, i + 64, i + 128, i + 192 of the tile in that order.  Per block and group: 8 doubles of l (read once per
//     block), 16 of r (the blocks i + g and i + g + 1: aligned, whatever M), 64 fused multiply-adds acc[lag] = fma(l[j], r[j + lag],
//     acc[lag]), j ascending.  The group of lag 0 carries El = fma(l, l, El), Er = fma(r, r, Er) (r masked to the tile) and
//     X += |l r|, the product rounded first.  The 64 lane sums of a group's 8 lags fold in one pass (fold8): the lanes trade
//     halves of their lags over xor 32, 16, 8 and end with one lag each, then a butterfly over xor 4, 2, 1.
//   sp_corr0: M = 0 reads no halo and stages nothing: thread i of 256 adds the samples i, i + 256, .. of the tile in order, the
//     lanes fold by a butterfly, the four wavefronts are added in order.
//   sp_fold: per segment and value, strand i of 16 adds the partials of the tiles i, i + 16, .. in order; the strands are added
//     in order.
//   sp_finish: one wavefront per pair.  A window's sums are those of its segments in ascending time, added one by one; then the
//     division, the largest |IACF| and the smallest index that attains it, and the pair's outputs.
// The translation unit is compiled without floating-point contraction: the fused multiply-adds are the ones written out.
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>

#include "common.h"
#include "rowfront.h"

using namespace frt;

namespace {

constexpr int kTile = 2048, kThreads = 256, kWaves = 4, kFront = 1024;
constexpr int kMaxLag = 128, kMaxWin = 4, kMaxSeg = 2 * kMaxWin - 1;
constexpr int kMaxGroups = 2 * (kMaxLag / 8) + 1;            // 33 groups of 8 lags at M = 128
constexpr int kLBlocks = kTile / 8;                          // blocks of 8 samples per tile
constexpr int kRBlocks = kLBlocks + kMaxGroups;              // lane block 255 of group NG - 1 reads the blocks 255 + NG - 1 and 255 + NG
constexpr int kPad = 10;                                     // doubles from one block of 8 to the next
constexpr int kStrands = 16, kFoldWidth = 64;
constexpr int kParams = 5;                                   // iacc, tau, cross_abs, El, Er

struct PairRec {
    long long e, t0, peak;
    int dead, nseg;
    long long segA[kMaxSeg], segB[kMaxSeg];
    int tile0[kMaxSeg + 1], mask[kMaxSeg];                   // the first tile of every segment (and the end); the windows that hold it
};

struct Call {
    const void* x;
    int dtype;                                    // 0 float32, 1 float64
    long long row_stride, pair_stride, T;
    int M, Mp, NG, g0, W, K, nlag, lagoff;        // lags kept; groups; the group of lag 0; windows; doubles per partial; lags summed; where -M lies
    long long a[kMaxWin], b[kMaxWin];             // the windows in samples behind the onset, b = -1: to the end
    double c, fs;
    const long long *onset, *stop;                // [pairs] or null
    long long nblk, maxt;                         // blocks of the front; the most tiles a pair can have
    double *m, *part, *seg;                       // scratch: [pairs][nblk], [pairs][maxt][K], [pairs][kMaxSeg][K]
    PairRec* rec;
    double* params;                               // [pairs][W][5]
    long long* idx;                               // [pairs][W + 2]
    double* iacf;                                 // [pairs][W][2 M + 1] or null
};

__device__ __forceinline__ double sample_at(const Call& p, long long pair, int row, long long t) {
    const long long at = pair * p.pair_stride + row * p.row_stride + t;
    return p.dtype ? reinterpret_cast<const double*>(p.x)[at] : (double)reinterpret_cast<const float*>(p.x)[at];
}

__device__ __forceinline__ long long pair_end(const Call& p, long long pair) {
    const long long e = p.stop ? p.stop[pair] : p.T;
    return e >= 1 && e <= p.T ? e : 0;            // 0: a dead pair (only a device array can carry a bad end this far)
}

__global__ __launch_bounds__(64 * kWaves) void sp_front(const Call p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long pair = blockIdx.y, k = (long long)blockIdx.x * kWaves + wave;
    if (k >= p.nblk) return;
    const long long e = pair_end(p, pair), a = k * kFront, b = min(a + kFront, e);
    double mx = 0.0;
    bool bad = false;
    for (long long t = a + lane; t < b; t += 64) {
        const double al = fabs(sample_at(p, pair, 0, t)), ar = fabs(sample_at(p, pair, 1, t));
        bad |= !(al < std::numeric_limits<double>::infinity()) || !(ar < std::numeric_limits<double>::infinity());
        mx = fmax(mx, fmax(al, ar));
    }
    if (__ballot(bad) != 0) mx = std::numeric_limits<double>::infinity();
    mx = fold_max(mx);
    if (lane == 0) p.m[pair * p.nblk + k] = mx;
}

// the smallest k in [a, b) with v[k] >= bound, -1 if there is none; the whole wavefront calls it
__device__ __forceinline__ long long first_block(const double* v, long long a, long long b, double bound, int lane) {
    for (long long k0 = a; k0 < b; k0 += 64) {
        const long long k = k0 + lane;
        const unsigned long long mask = __ballot(k < b && v[k] >= bound);
        if (mask) return k0 + __builtin_ctzll(mask);
    }
    return -1;
}

// the smallest t in [a, b) with max(|l[t]|, |r[t]|) >= bound, -1 if there is none
__device__ __forceinline__ long long first_sample(const Call& p, long long pair, long long a, long long b, double bound, int lane) {
    for (long long t0 = a; t0 < b; t0 += 64) {
        const long long t = t0 + lane;
        const bool hit = t < b && fmax(fabs(sample_at(p, pair, 0, t)), fabs(sample_at(p, pair, 1, t))) >= bound;
        const unsigned long long mask = __ballot(hit);
        if (mask) return t0 + __builtin_ctzll(mask);
    }
    return -1;
}

__global__ __launch_bounds__(64) void sp_plan(const Call p) {
    const int lane = threadIdx.x;
    const long long pair = blockIdx.x;
    const double* m = p.m + pair * p.nblk;
    const double inf = std::numeric_limits<double>::infinity();
    const long long e = pair_end(p, pair), nb = (e + kFront - 1) / kFront;
    double P = 0.0;
#pragma unroll 8
    for (long long k = lane; k < nb; k += 64) P = fmax(P, m[k]);
    P = fold_max(P);
    bool dead = e == 0 || !(P > 0.0) || P == inf;                // a bad end, all zero, or a sample that is not finite
    long long t0 = -1, peak = -1;
    if (!dead) {                                                 // the same on every lane
        const long long kp = first_block(m, 0, nb, P, lane);
        peak = kp < 0 ? -1 : first_sample(p, pair, kp * kFront, min((kp + 1) * kFront, e), P, lane);
        if (p.onset) {
            t0 = p.onset[pair];
        } else {
            const double bound = p.c * P;
            const long long ko = first_block(m, 0, nb, bound, lane);
            t0 = ko < 0 ? -1 : first_sample(p, pair, ko * kFront, min((ko + 1) * kFront, e), bound, lane);
        }
        dead = peak < 0 || t0 < 0 || t0 >= e;
    }
    if (lane != 0) return;
    PairRec& r = p.rec[pair];
    r.e = e;
    r.t0 = dead ? -1 : t0;
    r.peak = dead ? -1 : peak;
    r.dead = dead ? 1 : 0;
    r.nseg = 0;
    r.tile0[0] = 0;
    if (dead) return;
    long long A[kMaxWin], B[kMaxWin], cut[2 * kMaxWin];
    int nc = 0;
    for (int w = 0; w < p.W; ++w) {
        A[w] = min(t0 + p.a[w], e);
        B[w] = p.b[w] < 0 ? e : min(t0 + p.b[w], e);
        cut[nc++] = A[w];
        cut[nc++] = B[w];
    }
    for (int i = 1; i < nc; ++i) {                               // insertion sort of at most 8 cut points
        const long long v = cut[i];
        int j = i;
        for (; j > 0 && cut[j - 1] > v; --j) cut[j] = cut[j - 1];
        cut[j] = v;
    }
    int ns = 0;
    for (int i = 0; i + 1 < nc; ++i) {
        const long long lo = cut[i], hi = cut[i + 1];
        if (hi <= lo) continue;
        int mask = 0;
        for (int w = 0; w < p.W; ++w)
            if (A[w] <= lo && hi <= B[w]) mask |= 1 << w;
        if (!mask) continue;                                     // between two windows: nobody's samples
        r.segA[ns] = lo;
        r.segB[ns] = hi;
        r.mask[ns] = mask;
        r.tile0[ns + 1] = r.tile0[ns] + (int)((hi - lo + kTile - 1) / kTile);
        ++ns;
    }
    r.nseg = ns;
}

// tile q of a live pair: its segment's index, its first sample and its end
__device__ __forceinline__ void tile_span(const PairRec& r, int q, long long& ts, long long& te) {
    int s = 0;
    while (q >= r.tile0[s + 1]) ++s;
    ts = r.segA[s] + (long long)(q - r.tile0[s]) * kTile;
    te = min(ts + kTile, r.segB[s]);
}

// The 64 lane sums of 8 values in one pass: over xor 32, 16 and 8 a lane keeps one half of what it holds and gets its partner's
// sums of that half (both add own + partner's: the same number), so that lane i ends with value (i >> 3) & 7 summed over the 8
// lanes that differ from it in bits 3 .. 5; a butterfly over xor 4, 2, 1 adds the rest.  Every lane with the same i >> 3 ends
// with the same total.
__device__ __forceinline__ double fold8(const double (&a)[8], int lane) {
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    double b4[4], b2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double keep = h5 ? a[4 + i] : a[i], send = h5 ? a[i] : a[4 + i];
        b4[i] = keep + __shfl_xor(send, 32);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double keep = h4 ? b4[2 + i] : b4[i], send = h4 ? b4[i] : b4[2 + i];
        b2[i] = keep + __shfl_xor(send, 16);
    }
    const double keep = h3 ? b2[1] : b2[0], send = h3 ? b2[0] : b2[1];
    double v = keep + __shfl_xor(send, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

__device__ __forceinline__ void read_block(const double* buf, int block, double* out) {
    const double2* q = reinterpret_cast<const double2*>(buf + kPad * block);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double2 v = q[i];
        out[2 * i] = v.x;
        out[2 * i + 1] = v.y;
    }
}

// The tile of l and the tile of r with its halo into LDS.  Every load is issued before the first value is used: a sample outside
// its range is loaded from the tile's first sample (always a valid address) and replaced by zero, so no load hangs on a branch.
template <typename T>
__device__ __forceinline__ void stage_tile(const T* x, const Call& p, long long pair, long long ts, int len, long long e, int nr, int tid,
                                           double* lbuf, double* rbuf) {
    constexpr int kL = kTile / kThreads, kR = (8 * kRBlocks + kThreads - 1) / kThreads;
    const T* l = x + pair * p.pair_stride;
    const T* r = l + p.row_stride;
    double lv[kL], rv[kR];
#pragma unroll
    for (int j = 0; j < kL; ++j) {
        const int i = tid + kThreads * j;
        lv[j] = (double)l[ts + (i < len ? i : 0)];
    }
#pragma unroll
    for (int j = 0; j < kR; ++j) {
        const long long t = ts - p.Mp + tid + kThreads * j;
        rv[j] = (double)r[(t >= 0 && t < e) ? t : ts];
    }
#pragma unroll
    for (int j = 0; j < kL; ++j) {
        const int i = tid + kThreads * j;
        lbuf[i + 2 * (i >> 3)] = i < len ? lv[j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kR; ++j) {
        const int i = tid + kThreads * j;
        const long long t = ts - p.Mp + i;
        if (i < nr) rbuf[i + 2 * (i >> 3)] = (t >= 0 && t < e) ? rv[j] : 0.0;
    }
}

template <int NGW>                                              // the most groups of 8 lags that a wavefront owns
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(NGW <= 4 ? 3 : 2))) void sp_corr(const Call p) {   // the LDS lets three workgroups share a CU
    __shared__ __attribute__((aligned(16))) double lbuf[kLBlocks * kPad];
    __shared__ __attribute__((aligned(16))) double rbuf[kRBlocks * kPad];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long pair = blockIdx.y;
    const PairRec& r = p.rec[pair];
    if (r.dead) return;
    const int ntile = r.tile0[r.nseg], nr = 8 * (kLBlocks + p.NG);
    const long long e = r.e;
    for (int q = blockIdx.x; q < ntile; q += gridDim.x) {
        long long ts, te;
        tile_span(r, q, ts, te);
        const int len = (int)(te - ts), nstep = (len + 511) / 512;
        if (p.dtype) stage_tile(reinterpret_cast<const double*>(p.x), p, pair, ts, len, e, nr, tid, lbuf, rbuf);
        else stage_tile(reinterpret_cast<const float*>(p.x), p, pair, ts, len, e, nr, tid, lbuf, rbuf);
        __syncthreads();
        double acc[NGW][8], el = 0.0, er = 0.0, xs = 0.0;
#pragma unroll
        for (int sl = 0; sl < NGW; ++sl)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[sl][i] = 0.0;
        for (int k = 0; k < nstep; ++k) {
            const int b = lane + 64 * k;
            double l[8];
            read_block(lbuf, b, l);
#pragma unroll
            for (int sl = 0; sl < NGW; ++sl) {
                const int g = wave + kWaves * sl;
                if (g < p.NG) {                                  // the same on every lane
                    double rr[16];
                    read_block(rbuf, b + g, rr);
                    read_block(rbuf, b + g + 1, rr + 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[sl][i] = fma(l[j], rr[i + j], acc[sl][i]);
                    if (g == p.g0) {                             // lag 0 is this group's first
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const double rv = 8 * b + j < len ? rr[j] : 0.0;
                            el = fma(l[j], l[j], el);
                            er = fma(rv, rv, er);
                            xs += fabs(l[j] * rv);
                        }
                    }
                }
            }
        }
        double* part = p.part + (pair * p.maxt + q) * p.K;
#pragma unroll
        for (int sl = 0; sl < NGW; ++sl) {
            const int g = wave + kWaves * sl;
            if (g < p.NG) {
                const double v = fold8(acc[sl], lane);
                if ((lane & 7) == 0) part[8 * g + (lane >> 3)] = v;
                if (g == p.g0) {
                    el = fold_sum(el);
                    er = fold_sum(er);
                    xs = fold_sum(xs);
                    if (lane == 0) {
                        part[p.nlag] = el;
                        part[p.nlag + 1] = er;
                        part[p.nlag + 2] = xs;
                    }
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void sp_corr0(const Call p) {
    __shared__ double sums[kWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long pair = blockIdx.y;
    const PairRec& r = p.rec[pair];
    if (r.dead) return;
    const int ntile = r.tile0[r.nseg];
    for (int q = blockIdx.x; q < ntile; q += gridDim.x) {
        long long ts, te;
        tile_span(r, q, ts, te);
        double c = 0.0, el = 0.0, er = 0.0, xs = 0.0;
        for (long long t = ts + tid; t < te; t += kThreads) {
            const double l = sample_at(p, pair, 0, t), rv = sample_at(p, pair, 1, t);
            c = fma(l, rv, c);
            el = fma(l, l, el);
            er = fma(rv, rv, er);
            xs += fabs(l * rv);
        }
        c = fold_sum(c);
        el = fold_sum(el);
        er = fold_sum(er);
        xs = fold_sum(xs);
        if (lane == 0) {
            sums[wave][0] = c;
            sums[wave][1] = el;
            sums[wave][2] = er;
            sums[wave][3] = xs;
        }
        __syncthreads();
        if (tid < 4) p.part[(pair * p.maxt + q) * p.K + tid] = ((sums[0][tid] + sums[1][tid]) + sums[2][tid]) + sums[3][tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kStrands * kFoldWidth) void sp_fold(const Call p) {
    __shared__ double sh[kStrands][kFoldWidth];
    const int kk = threadIdx.x % kFoldWidth, strand = threadIdx.x / kFoldWidth, k = blockIdx.x * kFoldWidth + kk, s = blockIdx.z;
    const long long pair = blockIdx.y;
    const PairRec& r = p.rec[pair];
    if (r.dead || s >= r.nseg) return;                            // the same on every thread
    double v = 0.0;
    if (k < p.K) {
#pragma unroll 8
        for (int j = r.tile0[s] + strand; j < r.tile0[s + 1]; j += kStrands) v += p.part[(pair * p.maxt + j) * p.K + k];
    }
    sh[strand][kk] = v;
    __syncthreads();
    if (strand == 0 && k < p.K) {
        double t = sh[0][kk];
#pragma unroll
        for (int i = 1; i < kStrands; ++i) t += sh[i][kk];
        p.seg[(pair * kMaxSeg + s) * p.K + k] = t;
    }
}

__global__ __launch_bounds__(64) void sp_finish(const Call p) {
    const int lane = threadIdx.x, nl = 2 * p.M + 1;
    const long long pair = blockIdx.x;
    const PairRec& r = p.rec[pair];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double* par = p.params + pair * p.W * kParams;
    long long* ix = p.idx + pair * (p.W + 2);
    double* cf = p.iacf ? p.iacf + pair * p.W * nl : nullptr;
    if (r.dead) {
        for (int i = lane; i < p.W * kParams; i += 64) par[i] = nan;
        for (int i = lane; i < p.W + 2; i += 64) ix[i] = -1;
        if (cf)
            for (int i = lane; i < p.W * nl; i += 64) cf[i] = nan;
        return;
    }
    const double* seg = p.seg + pair * kMaxSeg * p.K;
    for (int w = 0; w < p.W; ++w) {
        double El = 0.0, Er = 0.0, X = 0.0;
        for (int s = 0; s < r.nseg; ++s) {
            if ((r.mask[s] >> w) & 1) {
                El += seg[s * p.K + p.nlag];
                Er += seg[s * p.K + p.nlag + 1];
                X += seg[s * p.K + p.nlag + 2];
            }
        }
        const double den = El * Er, root = sqrt(den);
        const bool live = den > 0.0;
        double best = -1.0;
        int bi = INT_MAX;
        for (int k = lane; k < nl; k += 64) {
            double C = 0.0;
            for (int s = 0; s < r.nseg; ++s)
                if ((r.mask[s] >> w) & 1) C += seg[s * p.K + p.lagoff + k];
            const double v = live ? C / root : nan;
            if (cf) cf[w * nl + k] = v;
            if (live && fabs(v) > best) {
                best = fabs(v);
                bi = k;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m);
            const int oi = __shfl_xor(bi, m);
            if (ob > best || (ob == best && oi < bi)) {
                best = ob;
                bi = oi;
            }
        }
        if (lane == 0) {
            par[w * kParams] = live ? best : nan;
            par[w * kParams + 1] = live ? (double)(bi - p.M) / p.fs : nan;
            par[w * kParams + 2] = X;
            par[w * kParams + 3] = El;
            par[w * kParams + 4] = Er;
            ix[w] = live ? bi : -1;
        }
    }
    if (lane == 0) {
        ix[p.W] = r.peak;
        ix[p.W + 1] = r.t0;
    }
}

template <int NGW>
void launch_corr(const Call& c, unsigned groups, unsigned nr, hipStream_t stream) {
    hipLaunchKernelGGL(sp_corr<NGW>, dim3(groups, nr), dim3(kThreads), 0, stream, c);
}

}  // namespace

struct frt_spatial {
    double fs = 0, c = 0;
    int M = 0, W = 0;
    long long a[kMaxWin] = {0, 0, 0, 0}, b[kMaxWin] = {0, 0, 0, 0};
    hipStream_t stream = nullptr;
    DeviceBuffer xin, oin, ein, pout, iout, cout, scratch;
};

extern "C" int frt_spatial_tile(void) { return kTile; }

extern "C" int frt_spatial_create(frt_spatial** out, double fs, int max_lag, const int64_t* starts, const int64_t* stops, int windows,
                                  double onset_db) {
    FRT_REQUIRE(out, "frt_spatial_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(std::isfinite(fs) && fs >= 100.0 && fs <= 1e7, "frt_spatial_create: fs %g (100 .. 1e7)", fs);
    FRT_REQUIRE(max_lag >= 0 && max_lag <= kMaxLag, "frt_spatial_create: max_lag %d (0 .. %d)", max_lag, kMaxLag);
    FRT_REQUIRE(windows >= 1 && windows <= kMaxWin && starts && stops, "frt_spatial_create: %d windows (1 .. %d, not null)", windows, kMaxWin);
    for (int w = 0; w < windows; ++w) {
        const long long a = starts[w], b = stops[w];
        FRT_REQUIRE(a >= 0 && a < (1LL << 31) && (b == -1 || (b > a && b <= (1LL << 31))),
                    "frt_spatial_create: window %d = [%lld, %lld) (0 <= start < stop <= 2^31, stop -1: to the end)", w, a, b);
    }
    FRT_REQUIRE(std::isfinite(onset_db) && onset_db <= 0.0, "frt_spatial_create: onset_db %g (at most 0)", onset_db);
    frt_spatial* h = new frt_spatial();
    h->fs = fs;
    h->M = max_lag;
    h->W = windows;
    for (int w = 0; w < windows; ++w) {
        h->a[w] = starts[w];
        h->b[w] = stops[w];
    }
    h->c = std::pow(10.0, onset_db / 20.0);
    *out = h;
    return FRT_OK;
}

extern "C" void frt_spatial_destroy(frt_spatial* h) {
    if (!h) return;
    destroy_handle(h, {&h->xin, &h->oin, &h->ein, &h->pout, &h->iout, &h->cout, &h->scratch});
}

extern "C" int frt_spatial_set_stream(frt_spatial* h, void* s) {
    FRT_REQUIRE(h, "frt_spatial_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_spatial_run(frt_spatial* h, const void* x, int x_dtype, int pairs, int64_t n, int64_t row_stride, int64_t pair_stride,
                               const int64_t* onset, const int64_t* stop, int64_t scratch_bytes, double* params, int64_t* indices,
                               double* iacf) {
    FRT_REQUIRE(h, "frt_spatial_run: null handle");
    int rc;
    if ((rc = require_rows("frt_spatial_run", x, x_dtype, pairs, n, row_stride, scratch_bytes))) return rc;
    FRT_REQUIRE(row_stride >= n, "frt_spatial_run: bad stride (n %lld, row stride %lld)", (long long)n, (long long)row_stride);
    FRT_REQUIRE(pairs == 1 || pair_stride >= n, "frt_spatial_run: bad stride (n %lld, pair stride %lld)", (long long)n, (long long)pair_stride);
    FRT_REQUIRE(params && indices, "frt_spatial_run: null output");
    const long long T = n, S = pairs;
    if ((rc = require_row_integers("frt_spatial_run", "stop", stop, S, 1, T, "1 .. n"))) return rc;
    if ((rc = require_row_integers("frt_spatial_run", "onset", onset, S, 0, T - 1, "0 .. n - 1"))) return rc;
    if (onset && stop && !is_device_pointer(onset) && !is_device_pointer(stop))
        for (long long r = 0; r < S; ++r)
            FRT_REQUIRE(onset[r] < stop[r], "frt_spatial_run: onset[%lld] = %lld lies at or behind stop %lld", r, (long long)onset[r], (long long)stop[r]);

    Call p{};
    p.x = x;
    p.dtype = x_dtype;
    p.row_stride = row_stride;
    p.pair_stride = pairs == 1 ? 0 : pair_stride;
    p.T = T;
    p.M = h->M;
    p.W = h->W;
    p.Mp = 8 * ((h->M + 7) / 8);
    p.NG = h->M ? p.Mp / 8 + h->M / 8 + 1 : 0;
    p.g0 = p.Mp / 8;
    p.nlag = h->M ? 8 * p.NG : 1;
    p.lagoff = p.Mp - h->M;
    p.K = p.nlag + 3;
    for (int w = 0; w < kMaxWin; ++w) {
        p.a[w] = h->a[w];
        p.b[w] = h->b[w];
    }
    p.c = h->c;
    p.fs = h->fs;
    p.nblk = (T + kFront - 1) / kFront;
    p.maxt = T / kTile + kMaxSeg + 1;             // sum of ceil(len / kTile) over at most kMaxSeg disjoint segments

    HostIO io(h->stream);
    const size_t xsize = x_dtype ? sizeof(double) : sizeof(float);
    const long long* on = reinterpret_cast<const long long*>(onset);
    const long long* st = reinterpret_cast<const long long*>(stop);
    long long* ix = reinterpret_cast<long long*>(indices);
    const long long nl = 2 * p.M + 1;
    if ((rc = io.in_rows(h->xin, p.x, p.row_stride, p.pair_stride, (size_t)S, 2, T, xsize))) return rc;
    if ((rc = io.in(h->oin, on, (size_t)S))) return rc;
    if ((rc = io.in(h->ein, st, (size_t)S))) return rc;
    if ((rc = io.out(h->pout, params, (size_t)S * p.W * kParams))) return rc;
    if ((rc = io.out(h->iout, ix, (size_t)S * (p.W + 2)))) return rc;
    if ((rc = io.out(h->cout, iacf, (size_t)S * p.W * nl))) return rc;

    const long long doubles = p.nblk + p.maxt * p.K + (long long)kMaxSeg * p.K;
    const long long per_pair = doubles * (long long)sizeof(double) + (long long)sizeof(PairRec);
    long long slab;
    if ((rc = reserve_slab(h->scratch, S, scratch_bytes, per_pair, slab))) return rc;
    double* at = h->scratch.as<double>();
    p.m = at;
    p.part = (at += slab * p.nblk);
    p.seg = (at += slab * p.maxt * p.K);
    p.rec = reinterpret_cast<PairRec*>(at + slab * kMaxSeg * p.K);
    const char* x0 = reinterpret_cast<const char*>(p.x);
    const unsigned front_groups = (unsigned)((p.nblk + kWaves - 1) / kWaves);
    const unsigned fold_groups = (unsigned)((p.K + kFoldWidth - 1) / kFoldWidth);
    const int ngw = (p.NG + kWaves - 1) / kWaves;
    for (long long r0 = 0; r0 < S; r0 += slab) {
        const unsigned nr = (unsigned)std::min(slab, S - r0);
        const unsigned groups = tile_groups(p.maxt, nr, 1);       // sp_corr: the workgroups of a pair loop over its tiles, one at a time
        Call c = p;
        c.x = x0 + (size_t)r0 * (size_t)p.pair_stride * xsize;
        c.onset = on ? on + r0 : nullptr;
        c.stop = st ? st + r0 : nullptr;
        c.params = params + r0 * p.W * kParams;
        c.idx = ix + r0 * (p.W + 2);
        c.iacf = iacf ? iacf + r0 * p.W * nl : nullptr;
        hipLaunchKernelGGL(sp_front, dim3(front_groups, nr), dim3(64 * kWaves), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(sp_plan, dim3(nr), dim3(64), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        switch (ngw) {
            case 0: hipLaunchKernelGGL(sp_corr0, dim3(groups, nr), dim3(kThreads), 0, h->stream, c); break;
            case 1: launch_corr<1>(c, groups, nr, h->stream); break;
            case 2: launch_corr<2>(c, groups, nr, h->stream); break;
            case 3: launch_corr<3>(c, groups, nr, h->stream); break;
            case 4: launch_corr<4>(c, groups, nr, h->stream); break;
            case 5: launch_corr<5>(c, groups, nr, h->stream); break;
            case 6: launch_corr<6>(c, groups, nr, h->stream); break;
            case 7: launch_corr<7>(c, groups, nr, h->stream); break;
            case 8: launch_corr<8>(c, groups, nr, h->stream); break;
            default: launch_corr<9>(c, groups, nr, h->stream); break;
        }
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(sp_fold, dim3(fold_groups, nr, kMaxSeg), dim3(kStrands * kFoldWidth), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(sp_finish, dim3(nr), dim3(64), 0, h->stream, c);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return io.finish();
}
