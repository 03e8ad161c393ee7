// soundlevel.hip — X7: the detector of a sound level meter over whole recordings: squared samples through 1 .. 4 first-order
// exponential averages (the time weightings of IEC 61672-1), and per logging interval the energy, the peak and each average's
// end value, maximum and minimum, with a carried state (frt_spl_*, SoundLevelBatch).  The definition: X7 in include/friture_hip.h.
//
// e' = a e + g q is affine in e, so a row is cut into cells of `cell` samples on a grid anchored at the recording's absolute
// sample index and run time-parallel, as sosfilter.hip does with its 2K states; here the state is one scalar per time constant:
//   spl_cells_kernel<NT, false>  pass 1: every cell from e = 0 (the call's first cell resumes the carried partial run): its end
//                                value P_c per time constant.
//   spl_scan_kernel<0>           scan level 1a: Q_r = the cells of run r (64 consecutive cells on the absolute grid) chained from
//                                zero, q' = A q + P_c (the call's first run resumes the carried q).
//   spl_scan_kernel<1>           scan level 2: U_{r+1} = A^64 U_r + Q_r along the runs of a row, from the carried U.
//   spl_scan_kernel<2>           scan level 1b: S_{c+1} = A S_c + P_c inside every run from its true start U_r (the call's first
//                                run from the carried S_c); a run's first cell starts from U_r itself.
//   spl_cells_kernel<NT, true>   pass 2: every cell again from its true start S_c (the call's first from the carried running
//                                value): per cell the sum of q, max |w|, and per time constant the end value, maximum and minimum.
//   spl_fold_kernel              a lane per (row, interval): the interval's cells in ascending order, behind the carried open
//                                interval; emits complete intervals (and with flush the partial last one), leaves the open one.
//   spl_state_kernel             a wavefront per row: the state behind the call's last sample, the stream totals over the
//                                emitted intervals, their energies added in ascending order.
// a, g, A = a^cell and A^64 are made on the host in long double and rounded once (spl_tables).  A scan step is P + A s, the
// product rounded on its own.  A cells workgroup is four wavefronts; a lane owns one cell, a wavefront 64 consecutive cells.
// Samples come through LDS in tiles of 16 per cell (a padded row per cell: conflict-free for the lane that reads its own row; a
// load instruction covers four cells' rows of 16 consecutive samples), the next tile's loads in flight while this one is
// averaged; a wavefront's tile is its own, so the wavefronts of a workgroup never wait for each other.  A NaN stays in e for
// good, so fmax and fmin run bare in the sample loop and a cell whose end value (or energy) is NaN gets NaN extrema (peak)
// behind it; the folds over cells and intervals keep a NaN explicitly.  No atomics, nothing waits on another workgroup, every
// order is fixed by the absolute grid: the bits of a row's results depend on its own samples, the settings and the absolute
// index alone.  The translation unit is compiled without floating-point contraction: every product rounds on its own.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "rowfront.h"

using namespace frt;

namespace {

constexpr int kMaxTau = 4;
constexpr int kTileW = 16, kPitch = kTileW + 1;      // samples of a cell per LDS tile; doubles per padded LDS row
constexpr int kWaves = 4, kRun = 64;                 // wavefronts per cells workgroup; cells per run of the scan
constexpr int kMinCell = 16, kMaxCell = 1024, kMaxInterval = 1 << 20;
constexpr int kTargetCell = 400;                     // the default cell: the largest admissible one up to this; measured:
                                                     // tools/bench_soundlevel.py --cells (DESIGN X7)
constexpr int kAhead = 16;                           // runs whose Q the level-two walk holds in registers ahead of its steps
// the state of a row: nine vectors of ntau doubles, then five scalars
enum { kVz, kVp, kVs, kVq, kVu, kVimax, kVimin, kVtmax, kVtmin, kStateVecs };
enum { kScellE, kSintE, kSintPeak, kStotE, kStotPeak, kStateScalars };

struct Call {
    const void* x;              // [rows][x_stride]
    int xdt;                    // 0 float32, 1 float64
    long long x_stride, T, n0;  // x[0] is absolute sample n0
    int ntau, cell, ipc, flush; // ipc: cells per interval
    long long interval;
    long long c0, c1, r0;       // the first cell; the cell that holds n0 + T; the first run
    long long j0, j1;           // the first interval; the interval that holds n0 + T
    int nc, ncp, nr;            // cells of the call, their pitch (nc + 1), runs
    long long jt, jout;         // intervals the call touches; intervals it emits
    double a[kMaxTau], g[kMaxTau], A[kMaxTau], A64[kMaxTau];
    const double* st_in;        // [rows][9 ntau + 5] or null
    double* st_out;
    double *E, *St, *Q, *U, *C; // scratch: [rows][ntau][ncp] x 2, [rows][ntau][nr] x 2, [rows][2 + 3 ntau][ncp]
    double* vals;               // [rows][jout][2 + 3 ntau]: energy, peak, last_i, max_i, min_i
    long long* count;           // [jout]
};

__device__ __forceinline__ int state_len(int ntau) { return kStateVecs * ntau + kStateScalars; }

// max and min that keep a NaN
__device__ __forceinline__ double keep_max(double a, double b) { return a != a ? a : (b != b ? b : fmax(a, b)); }
__device__ __forceinline__ double keep_min(double a, double b) { return a != a ? a : (b != b ? b : fmin(a, b)); }

template <int NT, bool OUT>
__global__ __launch_bounds__(64 * kWaves) void spl_cells_kernel(const Call p) {
    constexpr int NF = 2 + 3 * NT;
    __shared__ double tin[kWaves][64 * kPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = blockIdx.y;
    const long long k0 = ((long long)blockIdx.x * kWaves + wave) * 64, k = k0 + lane;
    if (k0 >= p.nc) return;                                      // the whole wavefront: it shares nothing with the others
    const bool active = k < p.nc;
    double* tb = tin[wave];
    const long long base = (p.c0 + k0) * p.cell - p.n0;          // the cell group's first sample as an index of x (may be negative)
    const long long mine = base + (long long)lane * p.cell;      // this lane's cell
    const int ntile = p.cell / kTileW;
    const size_t xrow = (size_t)row * (size_t)p.x_stride;

    double nx[kTileW];
    auto request = [&](int t) {
#pragma unroll
        for (int j = 0; j < kTileW; ++j) {
            const int flat = j * 64 + lane;
            const long long i = base + (long long)(flat / kTileW) * p.cell + (long long)t * kTileW + flat % kTileW;
            double v = 0.0;
            if (i >= 0 && i < p.T) {
                const size_t at = xrow + (size_t)i;
                v = p.xdt ? reinterpret_cast<const double*>(p.x)[at] : (double)reinterpret_cast<const float*>(p.x)[at];
            }
            nx[j] = v;
        }
    };

    const int SL = state_len(NT);
    const double* carried = p.st_in ? p.st_in + (size_t)row * SL : nullptr;
    double a[NT], g[NT], e[NT], mx[NT], mn[NT], en = 0.0, pk = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        a[i] = p.a[i];
        g[i] = p.g[i];
        e[i] = 0.0;
        mx[i] = -INFINITY;
        mn[i] = INFINITY;
        if (active) {
            if (OUT) {
                if (k > 0) e[i] = p.St[((size_t)row * NT + i) * p.ncp + k];
                else if (carried) e[i] = carried[kVz * NT + i];
            } else if (k == 0 && carried) {
                e[i] = carried[kVp * NT + i];
            }
        }
    }
    if (OUT && active && k == 0 && carried) en = carried[kStateVecs * NT + kScellE];

    request(0);
    for (int t = 0; t < ntile; ++t) {
        wave_sync();
#pragma unroll
        for (int j = 0; j < kTileW; ++j) {
            const int flat = j * 64 + lane;
            tb[(flat / kTileW) * kPitch + flat % kTileW] = nx[j];
        }
        wave_sync();
        if (t + 1 < ntile) request(t + 1);
        // the samples lo <= s < hi of this tile lie inside the call
        const long long it = mine + (long long)t * kTileW;
        const int lo = active ? (int)std::min<long long>(kTileW, std::max<long long>(0, -it)) : kTileW;
        const int hi = active ? (int)std::min<long long>(kTileW, std::max<long long>(0, p.T - it)) : 0;
#pragma unroll
        for (int s = 0; s < kTileW; ++s) {
            if (s >= lo && s < hi) {
                const double v = tb[lane * kPitch + s];
                const double q = v * v;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    e[i] = a[i] * e[i] + g[i] * q;
                    if (OUT) {
                        mx[i] = fmax(mx[i], e[i]);
                        mn[i] = fmin(mn[i], e[i]);
                    }
                }
                if (OUT) {
                    en += q;
                    pk = fmax(pk, fabs(v));
                }
            }
        }
    }
    if (!active) return;
    if (!OUT) {
#pragma unroll
        for (int i = 0; i < NT; ++i) p.E[((size_t)row * NT + i) * p.ncp + k] = e[i];
        return;
    }
    double* rec = p.C + (size_t)row * NF * p.ncp + k;
    if (en != en) pk = en;                                       // a NaN sample: fmax dropped it
    rec[0] = en;
    rec[(size_t)p.ncp] = pk;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (e[i] != e[i]) mx[i] = mn[i] = e[i];                  // e went NaN inside the cell and stayed so
        rec[(size_t)(2 + i) * p.ncp] = e[i];
        rec[(size_t)(2 + NT + i) * p.ncp] = mx[i];
        rec[(size_t)(2 + 2 * NT + i) * p.ncp] = mn[i];
    }
}

// A lane walks one chain.  LEVEL 0 and 2: one chain per (row, time constant, run), at most 64 steps; LEVEL 1: one chain per
// (row, time constant) along its runs.
template <int LEVEL>
__global__ __launch_bounds__(256) void spl_scan_kernel(const Call p, long long items) {
    const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= items) return;
    const long long plane = LEVEL == 1 ? item : item / p.nr;     // (row, time constant)
    const int lr = LEVEL == 1 ? 0 : (int)(item % p.nr);
    const int i = (int)(plane % p.ntau);
    const long long row = plane / p.ntau;
    const double* E = p.E + (size_t)plane * p.ncp;
    double* St = p.St + (size_t)plane * p.ncp;
    double* Q = p.Q + (size_t)plane * p.nr;
    double* U = p.U + (size_t)plane * p.nr;
    const double* carried = p.st_in ? p.st_in + (size_t)row * state_len(p.ntau) + i : nullptr;

    if (LEVEL == 1) {
        const double A64 = p.A64[i];
        double u = carried ? carried[kVu * p.ntau] : 0.0;
        U[0] = u;
        // one dependent chain: the Q of the next kAhead runs are in flight while these kAhead steps are made
        const int steps = p.nr - 1;
        double cur[kAhead], nxt[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) cur[j] = j < steps ? Q[j] : 0.0;
        for (int r = 0; r < steps; r += kAhead) {
#pragma unroll
            for (int j = 0; j < kAhead; ++j) nxt[j] = r + kAhead + j < steps ? Q[r + kAhead + j] : 0.0;
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                if (r + j < steps) {
                    u = cur[j] + A64 * u;
                    U[r + j + 1] = u;
                }
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) cur[j] = nxt[j];
        }
        return;
    }
    // the whole cells of run r0 + lr inside the call, as cell indices of the call
    const double A = p.A[i];
    const long long run = p.r0 + lr;
    const long long ka = std::max(run * kRun, p.c0) - p.c0, kb = std::min(run * kRun + kRun, p.c1) - p.c0;
    double s = 0.0;
    if (lr > 0) s = LEVEL == 2 ? U[lr] : 0.0;
    else if (carried) s = carried[(LEVEL == 2 ? kVs : kVq) * p.ntau];
    if (LEVEL == 2) St[ka] = s;
    for (long long kc = ka; kc < kb; ++kc) {
        s = E[kc] + A * s;
        if (LEVEL == 2 && (p.c0 + kc + 1) % kRun != 0) St[kc + 1] = s;      // a run's first cell starts from U_r
    }
    if (LEVEL == 0) Q[lr] = s;
}

__global__ __launch_bounds__(256) void spl_fold_kernel(const Call p, long long rows) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * p.jt) return;
    const long long row = idx / p.jt, jj = idx % p.jt, j = p.j0 + jj;
    const int NT = p.ntau, NF = 2 + 3 * NT, SL = state_len(NT);
    const long long ca = j * p.ipc, cb = ca + p.ipc;
    const long long ka = std::max(ca, p.c0) - p.c0, kb = std::min(cb, p.c1) - p.c0;      // the interval's complete cells
    const bool part = (p.n0 + p.T) % p.cell != 0 && p.c1 >= ca && p.c1 < cb;             // and its cell that the stream ends in
    const bool complete = j < p.j1;
    const double* rec = p.C + (size_t)row * NF * p.ncp;
    const double* carried = jj == 0 && p.st_in ? p.st_in + (size_t)row * SL : nullptr;
    double en = 0.0, pk = 0.0, mx[kMaxTau], mn[kMaxTau];
    if (carried) {
        en = carried[kStateVecs * NT + kSintE];
        pk = carried[kStateVecs * NT + kSintPeak];
    }
    for (int i = 0; i < kMaxTau; ++i) {
        mx[i] = carried && i < NT ? carried[kVimax * NT + i] : -INFINITY;
        mn[i] = carried && i < NT ? carried[kVimin * NT + i] : INFINITY;
    }
    const long long kend = part ? (long long)p.nc : kb;          // the partial cell is the call's last, nc - 1
    for (long long k = ka; k < kend; ++k) {
        if (k < kb) en += rec[k];
        pk = keep_max(pk, rec[(size_t)p.ncp + k]);
        for (int i = 0; i < kMaxTau; ++i) {
            if (i < NT) {
                mx[i] = keep_max(mx[i], rec[(size_t)(2 + NT + i) * p.ncp + k]);
                mn[i] = keep_min(mn[i], rec[(size_t)(2 + 2 * NT + i) * p.ncp + k]);
            }
        }
    }
    if (complete || p.flush) {
        double* o = p.vals + ((size_t)row * p.jout + jj) * NF;
        o[0] = part ? en + rec[p.nc - 1] : en;
        o[1] = pk;
        for (int i = 0; i < kMaxTau; ++i) {
            if (i < NT) {
                o[2 + i] = rec[(size_t)(2 + i) * p.ncp + kend - 1];
                o[2 + NT + i] = mx[i];
                o[2 + 2 * NT + i] = mn[i];
            }
        }
        if (row == 0) p.count[jj] = complete ? p.interval : p.n0 + p.T - j * p.interval;
    }
    if (!complete && p.st_out) {
        double* so = p.st_out + (size_t)row * SL;
        so[kStateVecs * NT + kSintE] = en;
        so[kStateVecs * NT + kSintPeak] = pk;
        for (int i = 0; i < kMaxTau; ++i) {
            if (i < NT) {
                so[kVimax * NT + i] = mx[i];
                so[kVimin * NT + i] = mn[i];
            }
        }
    }
}

// a butterfly over the wavefront with the NaN-keeping extrema; every lane ends with lane 0's value
__device__ __forceinline__ double wave_keep_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = keep_max(v, __shfl_xor(v, m));
    return __shfl(v, 0);
}
__device__ __forceinline__ double wave_keep_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = keep_min(v, __shfl_xor(v, m));
    return __shfl(v, 0);
}

// A wavefront per row.  The emitted intervals come in 64 at a time, a lane each; their energies are added in ascending order
// (lane after lane, every lane making the same sum), the extrema fold in any order.  Lane 0 writes the state.
__global__ __launch_bounds__(64) void spl_state_kernel(const Call p) {
    const long long row = blockIdx.x;
    const int lane = threadIdx.x;
    const int NT = p.ntau, NF = 2 + 3 * NT, SL = state_len(NT);
    const bool inside = (p.n0 + p.T) % p.cell != 0;              // the call ends inside a cell
    const bool open = (p.n0 + p.T) % p.interval != 0;            // and inside an interval: spl_fold_kernel left its accumulators
    const double* rec = p.C + (size_t)row * NF * p.ncp;
    const double* carried = p.st_in ? p.st_in + (size_t)row * SL : nullptr;
    double* so = p.st_out + (size_t)row * SL;
    double te = carried ? carried[kStateVecs * NT + kStotE] : 0.0, tp = carried ? carried[kStateVecs * NT + kStotPeak] : 0.0;
    double tmx[kMaxTau], tmn[kMaxTau];
    for (int i = 0; i < kMaxTau; ++i) {
        tmx[i] = carried && i < NT ? carried[kVtmax * NT + i] : -INFINITY;
        tmn[i] = carried && i < NT ? carried[kVtmin * NT + i] : INFINITY;
    }
    for (long long j0 = 0; j0 < p.jout; j0 += 64) {
        const bool have = j0 + lane < p.jout;
        const double* o = p.vals + ((size_t)row * p.jout + (have ? j0 + lane : 0)) * NF;
        const double en = o[0];
        const int n = (int)std::min<long long>(64, p.jout - j0);
        for (int l = 0; l < n; ++l) te += __shfl(en, l);
        tp = keep_max(tp, wave_keep_max(have ? o[1] : 0.0));
        for (int i = 0; i < kMaxTau; ++i) {
            if (i < NT) {
                tmx[i] = keep_max(tmx[i], wave_keep_max(have ? o[2 + NT + i] : -INFINITY));
                tmn[i] = keep_min(tmn[i], wave_keep_min(have ? o[2 + 2 * NT + i] : INFINITY));
            }
        }
    }
    if (lane != 0) return;
    for (int i = 0; i < kMaxTau; ++i) {
        if (i >= NT) break;
        const size_t plane = (size_t)row * NT + i;
        const double st = p.St[plane * p.ncp + (p.c1 - p.c0)];
        so[kVz * NT + i] = inside ? rec[(size_t)(2 + i) * p.ncp + p.nc - 1] : st;
        so[kVp * NT + i] = inside ? p.E[plane * p.ncp + p.nc - 1] : 0.0;
        so[kVs * NT + i] = st;
        so[kVq * NT + i] = p.Q[plane * p.nr + p.nr - 1];
        so[kVu * NT + i] = p.U[plane * p.nr + p.nr - 1];
        so[kVtmax * NT + i] = tmx[i];
        so[kVtmin * NT + i] = tmn[i];
        if (!open) {
            so[kVimax * NT + i] = -INFINITY;
            so[kVimin * NT + i] = INFINITY;
        }
    }
    so[kStateVecs * NT + kScellE] = inside ? rec[p.nc - 1] : 0.0;
    so[kStateVecs * NT + kStotE] = te;
    so[kStateVecs * NT + kStotPeak] = tp;
    if (!open) {
        so[kStateVecs * NT + kSintE] = 0.0;
        so[kStateVecs * NT + kSintPeak] = 0.0;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

struct Settings {
    double fs = 0;
    int ntau = 0, interval = 0, cell = 0;
    double tau[kMaxTau], a[kMaxTau], g[kMaxTau], A[kMaxTau], A64[kMaxTau];
};

int default_cell(int interval) {
    if (interval < kMinCell || interval > kMaxInterval || interval % kTileW) return 0;
    int best = kMinCell;
    for (int c = kMinCell; c <= std::min(kTargetCell, interval); c += kTileW)
        if (interval % c == 0) best = c;
    return best;
}

// a = exp(-1 / (fs tau)) and g = -expm1(-1 / (fs tau)) in long double, rounded once; A = a^cell and A^64 by stepping the rounded
// a in long double, one product per sample, rounded once
int check_settings(const char* who, double fs, const double* taus, int ntau, int interval, int cell, Settings& s) {
    FRT_REQUIRE(std::isfinite(fs) && fs >= 100.0 && fs <= 1e7, "%s: fs %g (100 .. 1e7)", who, fs);
    FRT_REQUIRE(ntau >= 1 && ntau <= kMaxTau && taus, "%s: %d time constants (1 .. %d)", who, ntau, kMaxTau);
    FRT_REQUIRE(interval >= kMinCell && interval <= kMaxInterval && interval % kTileW == 0,
                "%s: interval %d (a multiple of 16 in 16 .. 2^20)", who, interval);
    if (cell == 0) cell = default_cell(interval);
    FRT_REQUIRE(cell >= kMinCell && cell <= kMaxCell && cell % kTileW == 0 && interval % cell == 0,
                "%s: cell %d (a multiple of 16 in 16 .. 1024 that divides the interval %d)", who, cell, interval);
    s.fs = fs;
    s.ntau = ntau;
    s.interval = interval;
    s.cell = cell;
    for (int i = 0; i < kMaxTau; ++i) s.tau[i] = s.a[i] = s.g[i] = s.A[i] = s.A64[i] = 0.0;
    for (int i = 0; i < ntau; ++i) {
        FRT_REQUIRE(std::isfinite(taus[i]) && taus[i] > 0.0, "%s: time constant %d is %g s (> 0)", who, i, taus[i]);
        const long double x = -1.0L / ((long double)fs * (long double)taus[i]);
        s.tau[i] = taus[i];
        s.a[i] = (double)expl(x);
        s.g[i] = (double)-expm1l(x);
        FRT_REQUIRE(s.a[i] > 0.0 && s.a[i] < 1.0 && s.g[i] > 0.0, "%s: time constant %d (%g s at fs %g) leaves no average: a = %g", who, i,
                    taus[i], fs, s.a[i]);
        long double z = 1.0L;
        for (int n = 0; n < kRun * cell; ++n) {
            if (n == cell) s.A[i] = (double)z;
            z *= (long double)s.a[i];
        }
        s.A64[i] = (double)z;
    }
    return FRT_OK;
}

}  // namespace

struct frt_spl {
    Settings s;
    hipStream_t stream = nullptr;
    DeviceBuffer xin, sin, sout, vout, cout, scratch;
};

extern "C" int frt_spl_default_cell(int interval) { return default_cell(interval); }

extern "C" int frt_spl_state_length(int ntau) { return ntau >= 1 && ntau <= kMaxTau ? kStateVecs * ntau + kStateScalars : 0; }

extern "C" int frt_spl_tables(double fs, const double* taus, int ntau, int interval, int cell, double* a, double* g, double* A, double* A64) {
    Settings s;
    int rc = check_settings("frt_spl_tables", fs, taus, ntau, interval, cell, s);
    if (rc) return rc;
    for (int i = 0; i < ntau; ++i) {
        if (a) a[i] = s.a[i];
        if (g) g[i] = s.g[i];
        if (A) A[i] = s.A[i];
        if (A64) A64[i] = s.A64[i];
    }
    return FRT_OK;
}

extern "C" int frt_spl_create(frt_spl** out, double fs, const double* taus, int ntau, int interval, int cell) {
    FRT_REQUIRE(out, "frt_spl_create: null handle pointer");
    *out = nullptr;
    Settings s;
    int rc = check_settings("frt_spl_create", fs, taus, ntau, interval, cell, s);
    if (rc) return rc;
    frt_spl* h = new frt_spl();
    h->s = s;
    *out = h;
    return FRT_OK;
}

extern "C" void frt_spl_destroy(frt_spl* h) {
    if (!h) return;
    destroy_handle(h, {&h->xin, &h->sin, &h->sout, &h->vout, &h->cout, &h->scratch});
}

extern "C" int frt_spl_set_stream(frt_spl* h, void* s) {
    FRT_REQUIRE(h, "frt_spl_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

namespace {

template <int NT>
int launch_slab(const Call& c, unsigned rows, hipStream_t stream) {
    const unsigned groups = (unsigned)((c.nc + 63) / 64);
    const dim3 cells_grid((groups + kWaves - 1) / kWaves, rows), cells_block(64 * kWaves);
    hipLaunchKernelGGL((spl_cells_kernel<NT, false>), cells_grid, cells_block, 0, stream, c);
    FRT_HIP_CHECK(hipGetLastError());
    const long long planes = (long long)rows * NT, chains = planes * c.nr;
    hipLaunchKernelGGL((spl_scan_kernel<0>), dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, stream, c, chains);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((spl_scan_kernel<1>), dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, stream, c, planes);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((spl_scan_kernel<2>), dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, stream, c, chains);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((spl_cells_kernel<NT, true>), cells_grid, cells_block, 0, stream, c);
    FRT_HIP_CHECK(hipGetLastError());
    const long long folds = (long long)rows * c.jt;
    hipLaunchKernelGGL(spl_fold_kernel, dim3((unsigned)((folds + 255) / 256)), dim3(256), 0, stream, c, (long long)rows);
    FRT_HIP_CHECK(hipGetLastError());
    if (c.st_out) {
        hipLaunchKernelGGL(spl_state_kernel, dim3(rows), dim3(64), 0, stream, c);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return FRT_OK;
}

}  // namespace

extern "C" int64_t frt_spl_intervals_for(int interval, int64_t n_before, int64_t n, int flush) {
    if (interval < 1 || n_before < 0 || n < 0) return -1;
    const long long end = n_before + n;
    return end / interval - n_before / interval + (flush && end % interval != 0 ? 1 : 0);
}

extern "C" int frt_spl_run(frt_spl* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, int64_t n_before,
                           const double* state_in, double* state_out, int flush, int64_t scratch_bytes, double* vals, int64_t* count,
                           int64_t* n_intervals) {
    FRT_REQUIRE(h, "frt_spl_run: null handle");
    int rc;
    if ((rc = require_rows("frt_spl_run", x, x_dtype, rows, n, row_stride, scratch_bytes))) return rc;
    FRT_REQUIRE(flush == 0 || flush == 1, "frt_spl_run: flush %d (0 or 1)", flush);
    FRT_REQUIRE(n_before >= 0 && n_before <= (1LL << 60), "frt_spl_run: n_before %lld (0 .. 2^60)", (long long)n_before);
    FRT_REQUIRE(state_in || n_before == 0, "frt_spl_run: n_before %lld without a state", (long long)n_before);
    const Settings& s = h->s;
    const long long R = rows, T = n;
    const int NF = 2 + 3 * s.ntau, SL = kStateVecs * s.ntau + kStateScalars;

    Call p{};
    p.x = x;
    p.xdt = x_dtype;
    p.x_stride = row_stride;
    p.T = T;
    p.n0 = n_before;
    p.ntau = s.ntau;
    p.cell = s.cell;
    p.ipc = s.interval / s.cell;
    p.flush = flush;
    p.interval = s.interval;
    p.c0 = p.n0 / s.cell;
    p.c1 = (p.n0 + T) / s.cell;
    p.r0 = p.c0 / kRun;
    p.j0 = p.n0 / s.interval;
    p.j1 = (p.n0 + T) / s.interval;
    p.nc = (int)((p.n0 + T - 1) / s.cell - p.c0 + 1);
    p.ncp = p.nc + 1;
    p.nr = (int)(p.c1 / kRun - p.r0 + 1);
    p.jt = (p.n0 + T - 1) / s.interval - p.j0 + 1;
    p.jout = frt_spl_intervals_for(s.interval, n_before, n, flush);
    for (int i = 0; i < kMaxTau; ++i) {
        p.a[i] = s.a[i];
        p.g[i] = s.g[i];
        p.A[i] = s.A[i];
        p.A64[i] = s.A64[i];
    }
    p.st_in = state_in;
    p.st_out = state_out;
    p.vals = vals;
    p.count = reinterpret_cast<long long*>(count);
    FRT_REQUIRE(p.jout == 0 || (vals && count), "frt_spl_run: null output for %lld intervals", p.jout);
    if (n_intervals) *n_intervals = p.jout;

    HostIO io(h->stream);
    const size_t xsize = x_dtype ? sizeof(double) : sizeof(float);
    if ((rc = io.in_rows(h->xin, p.x, p.x_stride, (size_t)R, T, xsize))) return rc;
    if ((rc = io.in(h->sin, p.st_in, (size_t)R * SL))) return rc;
    if ((rc = io.out(h->vout, p.vals, (size_t)R * p.jout * NF))) return rc;
    if ((rc = io.out(h->cout, p.count, (size_t)p.jout))) return rc;
    if ((rc = io.out(h->sout, p.st_out, (size_t)R * SL))) return rc;

    const long long per_row = (long long)s.ntau * (2LL * p.ncp + 2LL * p.nr) + (long long)NF * p.ncp;
    long long slab;
    if ((rc = reserve_slab(h->scratch, R, scratch_bytes, per_row * (long long)sizeof(double), slab))) return rc;
    double* at = h->scratch.as<double>();
    p.E = at;
    p.St = (at += slab * s.ntau * p.ncp);
    p.Q = (at += slab * s.ntau * p.ncp);
    p.U = (at += slab * s.ntau * p.nr);
    p.C = (at += slab * s.ntau * p.nr);
    const char* x0 = reinterpret_cast<const char*>(p.x);
    for (long long r0 = 0; r0 < R; r0 += slab) {
        const unsigned nr = (unsigned)std::min(slab, R - r0);
        Call c = p;
        c.x = x0 + (size_t)r0 * (size_t)p.x_stride * xsize;
        c.st_in = p.st_in ? p.st_in + (size_t)r0 * SL : nullptr;
        c.st_out = p.st_out ? p.st_out + (size_t)r0 * SL : nullptr;
        c.vals = p.vals ? p.vals + (size_t)r0 * p.jout * NF : nullptr;
        switch (s.ntau) {
            case 1: rc = launch_slab<1>(c, nr, h->stream); break;
            case 2: rc = launch_slab<2>(c, nr, h->stream); break;
            case 3: rc = launch_slab<3>(c, nr, h->stream); break;
            default: rc = launch_slab<4>(c, nr, h->stream); break;
        }
        if (rc) return rc;
    }
    return io.finish();
}
