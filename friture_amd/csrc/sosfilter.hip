// sosfilter.hip — X6: cascades of second-order sections over whole recordings, one filter per row or a bank of filters per
// row, forward or reversed in time, with a carried state (frt_sos_*, SosBatch).  The definition: X6 in include/friture_hip.h.
//
// The joint recurrence of K sections is affine in its 2K states, s' = A s + b x, so a row is cut into cells of `cell` samples
// on a grid anchored at the recording's absolute sample index and run time-parallel:
//   sos_cells_kernel<K, false>  pass 1: every cell from the zero state (the call's first cell resumes the carried partial run P):
//                               its end state P_c.
//   sos_scan_kernel<K, 0>       scan level 1a: Q_r = the cells of run r (64 consecutive cells on the absolute grid) chained from
//                               zero, q' = M q + P_c (the call's first run resumes the carried q).
//   sos_scan_kernel<K, 1>       scan level 2: U_{r+1} = M^64 U_r + Q_r along the runs of an output row, from the carried U.
//   sos_scan_kernel<K, 2>       scan level 1b: S_{c+1} = M S_c + P_c inside every run from its true start U_r (the call's first
//                               run from the carried S_c); a run's first cell starts from U_r itself.
//   sos_cells_kernel<K, true>   pass 3: every cell again from its true start state S_c (the call's first from the carried running
//                               state), writing y; the last cell leaves the running state.
//   sos_state_kernel            the five vectors of the state behind the call's last sample.
// M = A^cell and M^64 are made on the host in long double by stepping unit vectors through the section code (sos_tables) and
// rounded once.  A matrix-vector step is P_i, then + M[i][0] s_0, + M[i][1] s_1, .. in that order, every product rounded on its own.
// A cells workgroup is four wavefronts; a lane owns one cell, a wavefront 64 consecutive cells.  Samples come through LDS in
// tiles of 16 per cell (a padded row per cell: conflict-free for the lane that reads its own row; a load instruction covers
// four cells' rows of 16 consecutive samples, as db_cells_kernel's does), the next tile's loads in flight while this one is
// filtered; y leaves through a tile of the wavefront's own in the same way.  Tiles of 32 and of 8 were measured slower: X6.  Row mode: the four
// wavefronts take four cell groups of one row.  Bank mode: they share ONE staged tile of one cell group and take filters
// w, w + 4, ..; the samples are staged once per four filters.  reverse is the reflection t <-> T - 1 - t where x is loaded
// and y is stored, nothing else.  No atomics, nothing waits on another workgroup, every order is fixed by the absolute grid:
// the bits of an output row depend on its own samples, its filter, the cell size and the absolute index alone.
// The translation unit is compiled without floating-point contraction: every product of a section rounds on its own.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "rowfront.h"

using namespace frt;

namespace {

constexpr int kMaxSections = 8, kMaxStates = 2 * kMaxSections, kMaxFilters = 64;
constexpr int kTileW = 16, kPitch = kTileW + 1;      // samples of a cell per LDS tile; doubles per padded LDS row
constexpr int kWaves = 4, kRun = 64;                 // wavefronts per cells workgroup; cells per run of the scan
constexpr int kStateVecs = 5;                        // z (running), p (partial zero-state run), s (S_c), q (partial Q), u (U_r)
constexpr int kDefaultCell = 256;                    // measured: tools/bench_sos.py --cells (DESIGN X6)
constexpr int kAhead = 16;                           // runs whose Q the level-two walk holds in registers ahead of its steps

struct Call {
    const void* x;              // [rows][x_stride]
    void* y;                    // [orows][T]
    int xdt, ydt;               // 0 float32, 1 float64
    long long x_stride, T, n0;  // x[0] is absolute sample n0
    int reverse, fan, F, cell;
    long long row0;             // the slab's first input row (row mode: row r uses filter (row0 + r) % F)
    long long c0, c1, r0;       // the first cell; the cell that holds n0 + T; the first run
    int nc, ncp, nr;            // cells of the call, their pitch (nc + 1), runs
    const double* coef;         // [F][K][5]: b0 b1 b2 a1 a2
    const double *M, *M64;      // [F][16][16], row i = the weights of new state i
    const double* st_in;        // [orows][5][2K] or null
    double* st_out;
    double *E, *St, *Q, *U, *Z; // scratch: [orows][2K][ncp] x 2, [orows][2K][nr] x 2, [orows][2K]
};

template <int K, bool OUT, bool FAN>
__global__ __launch_bounds__(64 * kWaves) void sos_cells_kernel(const Call p) {
    constexpr int NS = 2 * K;
    constexpr int kLoaders = FAN ? 64 * kWaves : 64;             // lanes that fill one tile
    constexpr int kLoads = 64 * kTileW / kLoaders;               // loads per lane and tile
    __shared__ double tin[FAN ? 1 : kWaves][64 * kPitch];
    __shared__ double tout[OUT ? kWaves : 1][OUT ? 64 * kPitch : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = blockIdx.y;
    const long long k0 = (FAN ? (long long)blockIdx.x : (long long)blockIdx.x * kWaves + wave) * 64, k = k0 + lane;
    const bool active = k < p.nc;
    double* tb = tin[FAN ? 0 : wave];
    const int li = FAN ? (int)threadIdx.x : lane;
    const long long base = (p.c0 + k0) * p.cell - p.n0;          // the cell group's first sample as an index of x (may be negative)
    const long long mine = base + (long long)lane * p.cell;      // this lane's cell
    const int ntile = p.cell / kTileW;
    const size_t xrow = (size_t)row * (size_t)p.x_stride;

    double nx[kLoads];
    auto request = [&](int t) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int flat = j * kLoaders + li;
            const long long i = base + (long long)(flat / kTileW) * p.cell + (long long)t * kTileW + flat % kTileW;
            double v = 0.0;
            if (i >= 0 && i < p.T) {
                const size_t at = xrow + (size_t)(p.reverse ? p.T - 1 - i : i);
                v = p.xdt ? reinterpret_cast<const double*>(p.x)[at] : (double)reinterpret_cast<const float*>(p.x)[at];
            }
            nx[j] = v;
        }
    };

    const int nf = FAN ? p.F : 1;
    for (int fg = 0; fg < nf; fg += kWaves) {
        const int f = FAN ? fg + wave : (int)((p.row0 + row) % p.F);
        const bool on = active && f < p.F;
        const size_t orow = FAN ? (size_t)row * p.F + (f < p.F ? f : 0) : (size_t)row;
        const double* cf = p.coef + (size_t)(f < p.F ? f : 0) * K * 5;
        double b0[K], b1[K], b2[K], a1[K], a2[K], z[NS];
#pragma unroll
        for (int s = 0; s < K; ++s) {
            b0[s] = cf[5 * s];
            b1[s] = cf[5 * s + 1];
            b2[s] = cf[5 * s + 2];
            a1[s] = cf[5 * s + 3];
            a2[s] = cf[5 * s + 4];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            z[s] = 0.0;
            if (on) {
                if (OUT) {
                    if (k > 0) z[s] = p.St[(orow * NS + s) * p.ncp + k];
                    else if (p.st_in) z[s] = p.st_in[(orow * kStateVecs + 0) * NS + s];
                } else if (k == 0 && p.st_in) {
                    z[s] = p.st_in[(orow * kStateVecs + 1) * NS + s];
                }
            }
        }
        request(0);
        for (int t = 0; t < ntile; ++t) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kLoads; ++j) {
                const int flat = j * kLoaders + li;
                tb[(flat / kTileW) * kPitch + flat % kTileW] = nx[j];
            }
            __syncthreads();
            if (t + 1 < ntile) request(t + 1);
            // the samples lo <= s < hi of this tile lie inside the call
            const long long it = mine + (long long)t * kTileW;
            const int lo = on ? (int)std::min<long long>(kTileW, std::max<long long>(0, -it)) : kTileW;
            const int hi = on ? (int)std::min<long long>(kTileW, std::max<long long>(0, p.T - it)) : 0;
#pragma unroll 8
            for (int s = 0; s < kTileW; ++s) {
                if (s >= lo && s < hi) {
                    double v = tb[lane * kPitch + s];
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        const double y = b0[q] * v + z[2 * q];
                        z[2 * q] = (b1[q] * v - a1[q] * y) + z[2 * q + 1];
                        z[2 * q + 1] = b2[q] * v - a2[q] * y;
                        v = y;
                    }
                    if (OUT) tout[wave][lane * kPitch + s] = v;
                }
            }
            if (OUT) {
                wave_sync();
                if (f < p.F) {
#pragma unroll 8
                    for (int j = 0; j < kTileW; ++j) {
                        const int flat = j * 64 + lane;
                        const long long i = base + (long long)(flat / kTileW) * p.cell + (long long)t * kTileW + flat % kTileW;
                        if (i >= 0 && i < p.T) {
                            const size_t at = orow * (size_t)p.T + (size_t)(p.reverse ? p.T - 1 - i : i);
                            const double v = tout[wave][(flat / kTileW) * kPitch + flat % kTileW];
                            if (p.ydt) reinterpret_cast<double*>(p.y)[at] = v;
                            else reinterpret_cast<float*>(p.y)[at] = (float)v;
                        }
                    }
                }
                wave_sync();
            }
        }
        if (on) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (!OUT) p.E[(orow * NS + s) * p.ncp + k] = z[s];
                else if (k == p.nc - 1) p.Z[orow * NS + s] = z[s];
            }
        }
    }
}

__device__ __forceinline__ int filter_of(const Call& p, long long orow) {
    return (int)((p.fan ? orow : p.row0 + orow) % p.F);
}

// A group of 16 lanes walks one chain; lane i < 2K carries state i and holds row i of the matrix.  LEVEL 0 and 2: one chain per
// (output row, run), at most 64 steps; LEVEL 1: one chain per output row along its runs.
template <int K, int LEVEL>
__global__ __launch_bounds__(64) void sos_scan_kernel(const Call p, long long items) {
    constexpr int NS = 2 * K;
    const int lane = threadIdx.x, i = lane & 15;
    const long long item = (long long)blockIdx.x * 4 + (lane >> 4);
    const bool live = item < items, own = live && i < NS;
    const long long orow = !live ? 0 : (LEVEL == 1 ? item : item / p.nr);
    const int lr = !live || LEVEL == 1 ? 0 : (int)(item % p.nr);
    const double* mat = (LEVEL == 1 ? p.M64 : p.M) + (size_t)filter_of(p, orow) * kMaxStates * kMaxStates + i * kMaxStates;
    double m[NS];
#pragma unroll
    for (int kk = 0; kk < NS; ++kk) m[kk] = own ? mat[kk] : 0.0;
    const size_t plane = (size_t)orow * NS + (own ? i : 0);
    const double* E = p.E + plane * p.ncp;
    double* St = p.St + plane * p.ncp;
    double* Q = p.Q + plane * p.nr;
    double* U = p.U + plane * p.nr;
    const double* carried = p.st_in ? p.st_in + (size_t)orow * kStateVecs * NS + (own ? i : 0) : nullptr;

    if (LEVEL == 1) {
        double u = own && carried ? carried[4 * NS] : 0.0;
        if (own) U[0] = u;
        // one dependent chain per output row: the Q of the next kAhead runs are in flight while these kAhead steps are made
        const int steps = p.nr - 1;
        double cur[kAhead], nxt[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) cur[j] = own && j < steps ? Q[j] : 0.0;
        for (int r = 0; r < steps; r += kAhead) {
#pragma unroll
            for (int j = 0; j < kAhead; ++j) nxt[j] = own && r + kAhead + j < steps ? Q[r + kAhead + j] : 0.0;
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                if (r + j < steps) {                     // the same on every lane
                    double acc = cur[j];
#pragma unroll
                    for (int kk = 0; kk < NS; ++kk) acc += m[kk] * __shfl(u, kk, 16);
                    u = acc;
                    if (own) U[r + j + 1] = u;
                }
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) cur[j] = nxt[j];
        }
        return;
    }
    // the whole cells of run r0 + lr inside the call, as cell indices of the call
    const long long run = p.r0 + lr;
    const long long ka = std::max(run * kRun, p.c0) - p.c0, kb = std::min(run * kRun + kRun, p.c1) - p.c0;
    double s = 0.0;
    if (own) {
        if (lr > 0) s = LEVEL == 2 ? U[lr] : 0.0;
        else if (carried) s = carried[(LEVEL == 2 ? 2 : 3) * NS];
    }
    if (LEVEL == 2 && own) St[ka] = s;
    double e = own && ka < kb ? E[ka] : 0.0;
    for (int j = 0; j < kRun; ++j) {                     // the same trip count on every lane: the shuffles stay whole
        const long long kc = ka + j;
        const bool step = kc < kb;
        double acc = e;
        if (own && kc + 1 < kb) e = E[kc + 1];
#pragma unroll
        for (int kk = 0; kk < NS; ++kk) acc += m[kk] * __shfl(s, kk, 16);
        if (step) s = acc;
        if (LEVEL == 2 && own && step && (p.c0 + kc + 1) % kRun != 0) St[kc + 1] = s;      // a run's first cell starts from U_r
    }
    if (LEVEL == 0 && own) Q[lr] = s;
}

__global__ void sos_state_kernel(const Call p, long long orows, int NS) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= orows * NS) return;
    const size_t orow = (size_t)(idx / NS), plane = (size_t)idx;
    const int i = (int)(idx % NS);
    const bool inside = (p.n0 + p.T) % p.cell != 0;              // the call ends inside a cell
    const double st = p.St[plane * p.ncp + (p.c1 - p.c0)];
    double* o = p.st_out + orow * kStateVecs * NS + i;
    o[0] = inside ? p.Z[plane] : st;
    o[NS] = inside ? p.E[plane * p.ncp + p.nc - 1] : 0.0;
    o[2 * NS] = st;
    o[3 * NS] = p.Q[plane * p.nr + p.nr - 1];
    o[4 * NS] = p.U[plane * p.nr + p.nr - 1];
}

// ---- host --------------------------------------------------------------------------------------------------------------------

struct Design {
    int F = 0, K = 0, cell = 0;
    std::vector<double> coef;      // [F][K][5]
};

int check_design(const char* who, const double* sos, int filters, int sections, int cell, Design& d) {
    FRT_REQUIRE(sos, "%s: null sos", who);
    FRT_REQUIRE(filters >= 1 && filters <= kMaxFilters, "%s: %d filters (1 .. %d)", who, filters, kMaxFilters);
    FRT_REQUIRE(sections >= 1 && sections <= kMaxSections, "%s: %d sections (1 .. %d)", who, sections, kMaxSections);
    if (cell == 0) cell = kDefaultCell;
    FRT_REQUIRE(cell >= 32 && cell <= 1024 && (cell & (cell - 1)) == 0, "%s: cell %d (a power of two in 32 .. 1024)", who, cell);
    d.F = filters;
    d.K = sections;
    d.cell = cell;
    d.coef.resize((size_t)filters * sections * 5);
    for (int f = 0; f < filters; ++f) {
        for (int k = 0; k < sections; ++k) {
            const double* s = sos + ((size_t)f * sections + k) * 6;
            for (int j = 0; j < 6; ++j) FRT_REQUIRE(std::isfinite(s[j]), "%s: filter %d section %d: coefficient %d is not finite", who, f, k, j);
            const double a0 = s[3];
            FRT_REQUIRE(a0 != 0.0, "%s: filter %d section %d: a0 is 0", who, f, k);
            double* c = d.coef.data() + ((size_t)f * sections + k) * 5;
            c[0] = s[0] / a0;
            c[1] = s[1] / a0;
            c[2] = s[2] / a0;
            c[3] = s[4] / a0;
            c[4] = s[5] / a0;
            for (int j = 0; j < 5; ++j) FRT_REQUIRE(std::isfinite(c[j]), "%s: filter %d section %d: not finite after the division by a0", who, f, k);
            // both roots of z^2 + a1 z + a2 inside the unit circle
            FRT_REQUIRE(std::fabs(c[4]) < 1.0 && std::fabs(c[3]) < 1.0 + c[4], "%s: filter %d section %d has a pole with |p| >= 1 (a1 %g, a2 %g)",
                        who, f, k, c[3], c[4]);
        }
    }
    return FRT_OK;
}

// M [F][2K][2K] (M[i][j]: state i after `cell` steps of silence from the unit state j) and M^64 likewise, in long double by
// stepping the section code, rounded once
void sos_tables(const Design& d, double* M, double* M64) {
    const int NS = 2 * d.K;
    for (int f = 0; f < d.F; ++f) {
        const double* c = d.coef.data() + (size_t)f * d.K * 5;
        for (int j = 0; j < NS; ++j) {
            long double z[kMaxStates] = {0};
            z[j] = 1.0L;
            for (long long n = 0; n < (long long)kRun * d.cell; ++n) {
                if (n == d.cell && M)
                    for (int i = 0; i < NS; ++i) M[((size_t)f * NS + i) * NS + j] = (double)z[i];
                long double v = 0.0L;
                for (int q = 0; q < d.K; ++q) {
                    const long double y = (long double)c[5 * q] * v + z[2 * q];
                    z[2 * q] = ((long double)c[5 * q + 1] * v - (long double)c[5 * q + 3] * y) + z[2 * q + 1];
                    z[2 * q + 1] = (long double)c[5 * q + 2] * v - (long double)c[5 * q + 4] * y;
                    v = y;
                }
            }
            if (M64)
                for (int i = 0; i < NS; ++i) M64[((size_t)f * NS + i) * NS + j] = (double)z[i];
        }
    }
}

}  // namespace

struct frt_sos {
    Design d;
    hipStream_t stream = nullptr;
    DeviceBuffer coef, M, M64, xin, sin, sout, yout, scratch;
};

extern "C" int frt_sos_default_cell(void) { return kDefaultCell; }

extern "C" int frt_sos_state_length(int sections) { return sections >= 1 && sections <= kMaxSections ? kStateVecs * 2 * sections : 0; }

extern "C" int frt_sos_tables(const double* sos, int filters, int sections, int cell, double* coef, double* M, double* M64) {
    Design d;
    int rc = check_design("frt_sos_tables", sos, filters, sections, cell, d);
    if (rc) return rc;
    if (coef) std::copy(d.coef.begin(), d.coef.end(), coef);
    sos_tables(d, M, M64);
    return FRT_OK;
}

extern "C" int frt_sos_create(frt_sos** out, const double* sos, int filters, int sections, int cell) {
    FRT_REQUIRE(out, "frt_sos_create: null handle pointer");
    *out = nullptr;
    Design d;
    int rc = check_design("frt_sos_create", sos, filters, sections, cell, d);
    if (rc) return rc;
    const int NS = 2 * d.K;
    std::vector<double> M((size_t)d.F * NS * NS), M64(M.size());
    sos_tables(d, M.data(), M64.data());
    // the device copies: rows padded to 16 x 16 per filter
    std::vector<double> P((size_t)d.F * kMaxStates * kMaxStates, 0.0), P64(P.size(), 0.0);
    for (int f = 0; f < d.F; ++f)
        for (int i = 0; i < NS; ++i)
            for (int j = 0; j < NS; ++j) {
                P[((size_t)f * kMaxStates + i) * kMaxStates + j] = M[((size_t)f * NS + i) * NS + j];
                P64[((size_t)f * kMaxStates + i) * kMaxStates + j] = M64[((size_t)f * NS + i) * NS + j];
            }
    frt_sos* h = new frt_sos();
    h->d = d;
    if ((rc = upload(h->coef, d.coef)) || (rc = upload(h->M, P)) || (rc = upload(h->M64, P64))) {
        for (DeviceBuffer* b : {&h->coef, &h->M, &h->M64}) b->release();
        delete h;
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_sos_destroy(frt_sos* h) {
    if (!h) return;
    destroy_handle(h, {&h->coef, &h->M, &h->M64, &h->xin, &h->sin, &h->sout, &h->yout, &h->scratch});
}

extern "C" int frt_sos_set_stream(frt_sos* h, void* s) {
    FRT_REQUIRE(h, "frt_sos_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

namespace {

template <int K>
int launch_slab(const Call& c, unsigned rows, long long orows, hipStream_t stream) {
    const unsigned groups = (unsigned)((c.nc + 63) / 64);
    const dim3 cells_grid(c.fan ? groups : (groups + kWaves - 1) / kWaves, rows), cells_block(64 * kWaves);
    if (c.fan) hipLaunchKernelGGL((sos_cells_kernel<K, false, true>), cells_grid, cells_block, 0, stream, c);
    else hipLaunchKernelGGL((sos_cells_kernel<K, false, false>), cells_grid, cells_block, 0, stream, c);
    FRT_HIP_CHECK(hipGetLastError());
    const long long chains = orows * c.nr;
    hipLaunchKernelGGL((sos_scan_kernel<K, 0>), dim3((unsigned)((chains + 3) / 4)), dim3(64), 0, stream, c, chains);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((sos_scan_kernel<K, 1>), dim3((unsigned)((orows + 3) / 4)), dim3(64), 0, stream, c, orows);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((sos_scan_kernel<K, 2>), dim3((unsigned)((chains + 3) / 4)), dim3(64), 0, stream, c, chains);
    FRT_HIP_CHECK(hipGetLastError());
    if (c.fan) hipLaunchKernelGGL((sos_cells_kernel<K, true, true>), cells_grid, cells_block, 0, stream, c);
    else hipLaunchKernelGGL((sos_cells_kernel<K, true, false>), cells_grid, cells_block, 0, stream, c);
    FRT_HIP_CHECK(hipGetLastError());
    if (c.st_out) {
        const long long n = orows * 2 * K;
        hipLaunchKernelGGL(sos_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c, orows, 2 * K);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return FRT_OK;
}

}  // namespace

extern "C" int frt_sos_run(frt_sos* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, int fan, int reverse,
                           int64_t n_before, const double* state_in, double* state_out, int64_t scratch_bytes, void* y, int y_dtype) {
    FRT_REQUIRE(h, "frt_sos_run: null handle");
    int rc;
    if ((rc = require_rows("frt_sos_run", x, x_dtype, rows, n, row_stride, scratch_bytes))) return rc;
    FRT_REQUIRE(y_dtype == 0 || y_dtype == 1, "frt_sos_run: y_dtype %d (0 float32, 1 float64)", y_dtype);
    FRT_REQUIRE((fan == 0 || fan == 1) && (reverse == 0 || reverse == 1), "frt_sos_run: fan %d, reverse %d (0 or 1)", fan, reverse);
    FRT_REQUIRE(n_before >= 0 && n_before <= (1LL << 60), "frt_sos_run: n_before %lld (0 .. 2^60)", (long long)n_before);
    FRT_REQUIRE(!reverse || (!state_in && !state_out && n_before == 0), "frt_sos_run: reverse runs whole rows from the zero state: no state");
    FRT_REQUIRE(state_in || n_before == 0, "frt_sos_run: n_before %lld without a state", (long long)n_before);
    FRT_REQUIRE(y, "frt_sos_run: null output");
    const Design& d = h->d;
    const int NS = 2 * d.K, opr = fan ? d.F : 1;
    const long long R = rows, T = n, OR = R * opr;

    Call p{};
    p.x = x;
    p.y = y;
    p.xdt = x_dtype;
    p.ydt = y_dtype;
    p.x_stride = row_stride;
    p.T = T;
    p.n0 = n_before;
    p.reverse = reverse;
    p.fan = fan;
    p.F = d.F;
    p.cell = d.cell;
    p.c0 = p.n0 / d.cell;
    p.c1 = (p.n0 + T) / d.cell;
    p.r0 = p.c0 / kRun;
    p.nc = (int)((p.n0 + T - 1) / d.cell - p.c0 + 1);
    p.ncp = p.nc + 1;
    p.nr = (int)(p.c1 / kRun - p.r0 + 1);
    p.coef = h->coef.as<const double>();
    p.M = h->M.as<const double>();
    p.M64 = h->M64.as<const double>();
    p.st_in = state_in;
    p.st_out = state_out;

    HostIO io(h->stream);
    const size_t xsize = x_dtype ? sizeof(double) : sizeof(float), ysize = y_dtype ? sizeof(double) : sizeof(float);
    long long y_ld = T;
    if ((rc = io.in_rows(h->xin, p.x, p.x_stride, (size_t)R, T, xsize))) return rc;
    if ((rc = io.in(h->sin, p.st_in, (size_t)OR * kStateVecs * NS))) return rc;
    if ((rc = io.out_rows(h->yout, p.y, y_ld, (size_t)OR, T, ysize))) return rc;
    if ((rc = io.out(h->sout, p.st_out, (size_t)OR * kStateVecs * NS))) return rc;

    const long long per_orow = (long long)NS * (2LL * p.ncp + 2LL * p.nr + 1);
    long long slab;
    if ((rc = reserve_slab(h->scratch, R, scratch_bytes, per_orow * opr * (long long)sizeof(double), slab))) return rc;
    const long long so = slab * opr;
    double* at = h->scratch.as<double>();
    p.E = at;
    p.St = (at += so * NS * p.ncp);
    p.Q = (at += so * NS * p.ncp);
    p.U = (at += so * NS * p.nr);
    p.Z = (at += so * NS * p.nr);
    const char* x0 = reinterpret_cast<const char*>(p.x);
    char* y0 = reinterpret_cast<char*>(p.y);
    for (long long r0 = 0; r0 < R; r0 += slab) {
        const unsigned nr = (unsigned)std::min(slab, R - r0);
        Call c = p;
        c.row0 = r0;
        c.x = x0 + (size_t)r0 * (size_t)p.x_stride * xsize;
        c.y = y0 + (size_t)r0 * opr * (size_t)T * ysize;
        c.st_in = p.st_in ? p.st_in + (size_t)r0 * opr * kStateVecs * NS : nullptr;
        c.st_out = p.st_out ? p.st_out + (size_t)r0 * opr * kStateVecs * NS : nullptr;
        const long long orows = (long long)nr * opr;
        switch (d.K) {
            case 1: rc = launch_slab<1>(c, nr, orows, h->stream); break;
            case 2: rc = launch_slab<2>(c, nr, orows, h->stream); break;
            case 3: rc = launch_slab<3>(c, nr, orows, h->stream); break;
            case 4: rc = launch_slab<4>(c, nr, orows, h->stream); break;
            case 5: rc = launch_slab<5>(c, nr, orows, h->stream); break;
            case 6: rc = launch_slab<6>(c, nr, orows, h->stream); break;
            case 7: rc = launch_slab<7>(c, nr, orows, h->stream); break;
            default: rc = launch_slab<8>(c, nr, orows, h->stream); break;
        }
        if (rc) return rc;
    }
    return io.finish();
}
