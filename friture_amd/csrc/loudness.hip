// loudness.hip — ITU-R BS.1770-4 / EBU R 128 programme loudness and true peak (frt_loudness_*; the definition: L2 in
// include/friture_hip.h).
//
// The K-weighting is a 4-state linear recurrence, s' = A s + b x.  A sub-block (kB = 4800 samples, on the absolute grid of the
// stream) is cut into kCells = 64 cells of kCell = 75 samples, and the recurrence becomes parallel over cells in four launches:
//   ld_cells_kernel    one workgroup per (stream, sub-block): four wavefronts fetch the samples into LDS (coalesced reads), lane c
//                      of the first runs cell c from the zero state (z_c), lane 0 chains them, P_0 = 0, P_{c+1} = A^75 P_c + z_c:
//                      P_c is the state at the start of cell c of a sub-block entered with the zero state, Z = P_64 the one at its end
//   ld_scan_kernel     one wavefront per stream: s_{b+1} = A^4800 s_b + Z_b over the call's sub-blocks, from the carried state,
//                      Z fetched 64 sub-blocks at a time and handed from lane to lane
//   ld_block_kernel    one workgroup of four wavefronts per (stream, sub-block), the samples and their tp_zeros halo on both sides
//                      in LDS: wavefront 0 runs cell c from its true start state A^(75 c) s_b + P_c and sums y^2 along it (the
//                      sub-block's energy is the 64 cell sums added in ascending order); wavefronts 1 .. 3 form the four
//                      interpolated outputs of every sample, each ONE chain acc = fma(h[..], x[kb + j], acc), j ascending, the
//                      coefficients uniform across the lanes, and keep max |u|; all four keep max |x|
//   ld_readout_kernel  one workgroup per programme: the new 400 ms and 3 s blocks from the sub-block energies (the last 29 of
//                      the calls before are carried), momentary and short-term loudness, both gates over the whole series
//   ld_carry_kernel    the samples and energies the next call needs
// Every matrix A^(75 c), c = 0 .. 64, is formed on the host by running the definition on the four unit states.  Nothing
// depends on the grid, the stream count or where a call was cut: cells sit on the absolute grid, every chain of additions
// is ordered by the position in the sub-block, and the gates are a function of the whole series.
// This translation unit is compiled with -ffp-contract=off: the biquads are the operation order of the definition, and the only
// fused multiply-adds are the fma() calls of the interpolator, which are part of ITS definition (R1).
#include "common.h"
#include "hostio.h"

#include <algorithm>
#include <cmath>

namespace {

using namespace frt;

constexpr int kB = 4800;                 // samples per sub-block (100 ms)
constexpr int kCells = 64;               // cells per sub-block: one per lane of a wavefront
constexpr int kCell = kB / kCells;       // 75 samples
constexpr int kTail = 29;                // sub-block energies carried: a 3 s block spans 30
constexpr int kMaxZeros = 512;           // tp_zeros: (kB + 2 * 512) float64 slots and the reduction rows stay under 64 KB of LDS
constexpr int kFirThreads = 192;         // wavefronts 1 .. 3 of ld_block_kernel
constexpr int kGroup = 5;                // samples a thread interpolates side by side: kB = kFirThreads * kGroup * 5
constexpr int kBlockThreads = 256;

// stage 1 (shelf) and stage 2 (high-pass) of the K-weighting at 48 kHz, a[0] = 1
constexpr double kB10 = 1.53512485958697, kB11 = -2.69169618940638, kB12 = 1.19839281085285;
constexpr double kA11 = -1.69065929318241, kA12 = 0.73248077421585;
constexpr double kB20 = 1.0, kB21 = -2.0, kB22 = 1.0;
constexpr double kA21 = -1.99004745483398, kA22 = 0.99007225036621;

// one sample through both biquads, direct form II transposed: y = z0 + b0 x; z0 = (z1 + x b1) - y a1; z1 = x b2 - y a2
__host__ __device__ inline double kw_step(double x, double* s) {
    const double y1 = s[0] + kB10 * x;
    s[0] = (s[1] + x * kB11) - y1 * kA11;
    s[1] = x * kB12 - y1 * kA12;
    const double y2 = s[2] + kB20 * y1;
    s[2] = (s[3] + y1 * kB21) - y2 * kA21;
    s[3] = y1 * kB22 - y2 * kA22;
    return y2;
}

// out = M v + z, M [4][4] row-major, each row one ascending chain
__device__ inline void affine(const double* M, const double* v, const double* z, double* out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = (((M[4 * i] * v[0] + M[4 * i + 1] * v[1]) + M[4 * i + 2] * v[2]) + M[4 * i + 3] * v[3]) + z[i];
}

inline long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct Counts {                          // of a stream after n_in samples, `blocks` sub-blocks with an energy
    long long energies, peaks;
};
inline Counts counts(long long n_in, int R, bool flush) {
    if (flush) return {n_in / kB, (n_in + kB - 1) / kB};
    const long long e = std::max<long long>(0, floor_div(n_in - R, kB));
    return {e, e};
}
inline long long n400(long long e) { return std::max<long long>(0, e - 3); }
inline long long n3s(long long e) { return std::max<long long>(0, e - kTail); }

struct Params {
    const void* x;           // [S][ld], the call's samples first_in ..
    const double* carry;     // [S][carry_len], the samples carry_pos .. first_in - 1 (nullptr: zeros)
    long long n, ld, first_in, carry_pos, carry_len, total;
    long long b0;            // the first sub-block of the call
    int ne, npk;             // sub-blocks with an energy, with peaks
    int R, S, C, true_peak;
    const double* pw;        // [kCells + 1][16]: A^(75 c)
    const double* filt_in;   // [S][4] or nullptr
    double *pref, *zb, *start;      // [S][ne][kCells][4], [S][ne][4], [S][ne][4]
    double *energy, *tpk, *spk;     // [S][ne], [S][npk], [S][npk]
};

// sample k of the stream (absolute index): this call's x, the carried samples behind it, zeros elsewhere
template <typename Tin>
__device__ inline double sample(const Params& p, const Tin* xs, const double* cs, long long k) {
    long long r = k - p.first_in;
    if (r >= 0) return r < p.n ? (double)xs[r] : 0.0;
    r = k - p.carry_pos;
    return (r >= 0 && r < p.carry_len && cs) ? cs[r] : 0.0;
}

// dst[i] = sample k_first + i, i < count, by the whole workgroup; a span inside this call's samples (the usual case, uniform
// over the workgroup) is a plain coalesced copy whose loads the compiler can issue together
template <typename Tin>
__device__ inline void stage(const Params& p, const Tin* xs, const double* cs, long long k_first, int count, double* dst) {
    const long long r0 = k_first - p.first_in;
    const int tid = threadIdx.x, step = blockDim.x;
    if (r0 >= 0 && r0 + count <= p.n) {
        const Tin* __restrict__ src = xs + r0;
#pragma unroll 8
        for (int i = tid; i < count; i += step) dst[i] = (double)src[i];
    } else {
        for (int i = tid; i < count; i += step) dst[i] = sample(p, xs, cs, k_first + i);
    }
}

template <typename Tin>
__global__ __launch_bounds__(kBlockThreads) void ld_cells_kernel(Params p) {
    __shared__ double sx[kB];
    __shared__ double sz[kCells * 4];
    __shared__ double sp[(kCells + 1) * 4];
    const int s = blockIdx.y, b = blockIdx.x, lane = threadIdx.x;
    const Tin* xs = reinterpret_cast<const Tin*>(p.x) + (long long)s * p.ld;
    const double* cs = p.carry ? p.carry + (long long)s * p.carry_len : nullptr;
    const long long k0 = (p.b0 + b) * kB;
    stage(p, xs, cs, k0, kB, sx);                       // four wavefronts fetch, the first one computes
    __syncthreads();
    if (lane < kCells) {
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        const double* mine = sx + lane * kCell;
        for (int i = 0; i < kCell; ++i) (void)kw_step(mine[i], st);
#pragma unroll
        for (int r = 0; r < 4; ++r) sz[lane * 4 + r] = st[r];
    }
    __syncthreads();
    if (lane == 0) {
        double A[16], v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 16; ++r) A[r] = p.pw[16 + r];
        for (int c = 0; c < kCells; ++c) {
            double nv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) sp[c * 4 + r] = v[r];
            affine(A, v, sz + c * 4, nv);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = nv[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sp[kCells * 4 + r] = v[r];
    }
    __syncthreads();
    if (lane >= kCells) return;
    const long long blk = (long long)s * p.ne + b;
#pragma unroll
    for (int r = 0; r < 4; ++r) p.pref[(blk * kCells + lane) * 4 + r] = sp[lane * 4 + r];
    if (lane < 4) p.zb[blk * 4 + lane] = sp[kCells * 4 + lane];
}

// the value lane j holds, in every lane (j uniform)
__device__ inline double lane_value(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// One wavefront per stream.  Lane l fetches Z of sub-block base + l (one coalesced read per 64 sub-blocks), the chain then
// runs on values handed from lane to lane, every lane computing the same states: no memory access sits inside the chain.
// Lane j keeps the state at the start of sub-block base + j and writes it when the 64 are done.
__global__ __launch_bounds__(64) void ld_scan_kernel(Params p, double* filt_out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    double A[16], v[4];
#pragma unroll
    for (int r = 0; r < 16; ++r) A[r] = p.pw[kCells * 16 + r];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = p.filt_in ? p.filt_in[(long long)s * 4 + r] : 0.0;
    for (int base = 0; base < p.ne; base += 64) {
        const int mine = base + lane, steps = p.ne - base < 64 ? p.ne - base : 64;
        const long long blk = (long long)s * p.ne + mine;
        double z[4] = {0.0, 0.0, 0.0, 0.0}, keep[4] = {0.0, 0.0, 0.0, 0.0};
        if (mine < p.ne) {
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = p.zb[blk * 4 + r];
        }
        for (int j = 0; j < steps; ++j) {
            double zj[4], nv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                zj[r] = lane_value(z[r], j);
                if (lane == j) keep[r] = v[r];
            }
            affine(A, v, zj, nv);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = nv[r];
        }
        if (mine < p.ne) {
#pragma unroll
            for (int r = 0; r < 4; ++r) p.start[blk * 4 + r] = keep[r];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) filt_out[(long long)s * 4 + r] = v[r];
    }
}

// coef: [2 R + 1][4], row j the j-th tap of the four outputs of a sample: column 0 (the output AT the sample) reads the samples
// from R before it on, columns 1 .. 3 from R - 1 before it on and have 2 R taps (their last row is not read)
template <typename Tin>
__global__ __launch_bounds__(kBlockThreads) void ld_block_kernel(Params p, const double* __restrict__ coef) {
    extern __shared__ __align__(16) double lds[];
    const int R = p.R, span = kB + 2 * R;
    double* sx = lds;                                   // sx[i]: sample k0 - R + i
    double* se = lds + span;                            // [kCells] cell energies
    double* rt = se + kCells;                           // [kBlockThreads] max |u|
    double* rs = rt + kBlockThreads;                    // [kBlockThreads] max |x|
    const int s = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const Tin* xs = reinterpret_cast<const Tin*>(p.x) + (long long)s * p.ld;
    const double* cs = p.carry ? p.carry + (long long)s * p.carry_len : nullptr;
    const long long k0 = (p.b0 + b) * kB;
    double ms = 0.0, mt = 0.0;
    stage(p, xs, cs, k0 - R, span, sx);
    __syncthreads();
    for (int i = tid; i < kB; i += kBlockThreads) ms = fmax(ms, fabs(sx[R + i]));
    if (tid < kCells) {
        if (b < p.ne) {
            const long long blk = (long long)s * p.ne + b;
            double M[16], v[4], z[4], st[4];
#pragma unroll
            for (int r = 0; r < 16; ++r) M[r] = p.pw[tid * 16 + r];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = p.start[blk * 4 + r];
                z[r] = p.pref[(blk * kCells + tid) * 4 + r];
            }
            affine(M, v, z, st);
            const double* mine = sx + R + tid * kCell;
            double e = 0.0;
            for (int i = 0; i < kCell; ++i) {
                const double y = kw_step(mine[i], st);
                e = e + y * y;
            }
            se[tid] = e;
        }
    } else if (p.true_peak) {
        const long long left = p.total - k0;            // samples of the stream from k0 on: outputs exist for those alone
        const int valid = left < kB ? (int)left : kB;
        for (int g0 = tid - kCells; g0 < kB; g0 += kFirThreads * kGroup) {
            double acc[kGroup][4], xa[kGroup];
            const double* w[kGroup];
#pragma unroll
            for (int g = 0; g < kGroup; ++g) {
                w[g] = sx + g0 + g * kFirThreads;
                xa[g] = w[g][0];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[g][q] = 0.0;
            }
            for (int j = 0; j < 2 * R; ++j) {
                const double c0 = coef[4 * j], c1 = coef[4 * j + 1], c2 = coef[4 * j + 2], c3 = coef[4 * j + 3];
#pragma unroll
                for (int g = 0; g < kGroup; ++g) {
                    const double xb = w[g][j + 1];
                    acc[g][0] = fma(c0, xa[g], acc[g][0]);
                    acc[g][1] = fma(c1, xb, acc[g][1]);
                    acc[g][2] = fma(c2, xb, acc[g][2]);
                    acc[g][3] = fma(c3, xb, acc[g][3]);
                    xa[g] = xb;
                }
            }
            const double cl = coef[8 * R];
#pragma unroll
            for (int g = 0; g < kGroup; ++g) {
                acc[g][0] = fma(cl, xa[g], acc[g][0]);
                if (g0 + g * kFirThreads < valid)
                    mt = fmax(mt, fmax(fmax(fabs(acc[g][0]), fabs(acc[g][1])), fmax(fabs(acc[g][2]), fabs(acc[g][3]))));
            }
        }
    }
    rt[tid] = mt;
    rs[tid] = ms;
    __syncthreads();
    for (int half = kBlockThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            rt[tid] = fmax(rt[tid], rt[tid + half]);
            rs[tid] = fmax(rs[tid], rs[tid + half]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const long long at = (long long)s * p.npk + b;
        p.tpk[at] = rt[0];
        p.spk[at] = rs[0];
        if (b < p.ne) {
            double e = 0.0;
            for (int c = 0; c < kCells; ++c) e = e + se[c];
            p.energy[(long long)s * p.ne + b] = e;
        }
    }
}

struct Readout {
    const double *tail, *energy;        // [S][tl] the energies of the sub-blocks e0 - tl .. e0 - 1, [S][ne] those from e0 on
    const double *z400_in, *z3s_in;     // [P][n400(e0)], [P][n3s(e0)]
    double *z400, *z3s;                 // [P][n400(e1)], [P][n3s(e1)]
    double *momentary, *short_term, *integrated;      // [P][new 400 ms blocks], [P][new 3 s blocks], [P]
    const double* weights;              // [C]
    long long e0, e1;
    int tl, ne, C;
};

__device__ inline double lkfs(double z) { return z > 0.0 ? -0.691 + 10.0 * log10(z) : -INFINITY; }

__device__ inline double energy_at(const Readout& r, int s, long long b) {
    return b < r.e0 ? r.tail[(long long)s * r.tl + (b - (r.e0 - r.tl))] : r.energy[(long long)s * r.ne + (b - r.e0)];
}

// z of the block of `len` sub-blocks from j on: per channel one ascending chain of energies, times its weight, channels ascending
__device__ inline double block_power(const Readout& r, int p, long long j, int len, double norm) {
    double z = 0.0;
    for (int c = 0; c < r.C; ++c) {
        double inner = energy_at(r, p * r.C + c, j);
        for (int i = 1; i < len; ++i) inner = inner + energy_at(r, p * r.C + c, j + i);
        z = z + r.weights[c] * inner;
    }
    return z / norm;
}

// (sum, count) over the workgroup of the entries each thread gathered, in an order fixed by the thread index
__device__ inline void reduce_pair(double* rsum, double* rcnt, int tid, double& sum, double& cnt) {
    __syncthreads();
    rsum[tid] = sum;
    rcnt[tid] = cnt;
    __syncthreads();
    for (int half = kBlockThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            rsum[tid] = rsum[tid] + rsum[tid + half];
            rcnt[tid] = rcnt[tid] + rcnt[tid + half];
        }
        __syncthreads();
    }
    sum = rsum[0];
    cnt = rcnt[0];
}

__global__ __launch_bounds__(kBlockThreads) void ld_readout_kernel(Readout r) {
    __shared__ double rsum[kBlockThreads], rcnt[kBlockThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long a0 = r.e0 > 3 ? r.e0 - 3 : 0, a1 = r.e1 > 3 ? r.e1 - 3 : 0;
    const long long s0 = r.e0 > kTail ? r.e0 - kTail : 0, s1 = r.e1 > kTail ? r.e1 - kTail : 0;
    for (long long j = tid; j < a1; j += kBlockThreads) {
        if (j < a0) {
            r.z400[p * a1 + j] = r.z400_in[p * a0 + j];
        } else {
            const double z = block_power(r, p, j, 4, 4.0 * kB);
            r.z400[p * a1 + j] = z;
            r.momentary[p * (a1 - a0) + (j - a0)] = lkfs(z);
        }
    }
    for (long long j = tid; j < s1; j += kBlockThreads) {
        if (j < s0) {
            r.z3s[p * s1 + j] = r.z3s_in[p * s0 + j];
        } else {
            const double z = block_power(r, p, j, kTail + 1, (kTail + 1.0) * kB);
            r.z3s[p * s1 + j] = z;
            r.short_term[p * (s1 - s0) + (j - s0)] = lkfs(z);
        }
    }
    __syncthreads();                     // each thread reads back below what itself and others wrote: same workgroup, global memory
    __threadfence_block();
    const double* z = r.z400 + p * a1;
    double sum = 0.0, cnt = 0.0;
    for (long long j = tid; j < a1; j += kBlockThreads)
        if (lkfs(z[j]) > -70.0) {
            sum = sum + z[j];
            cnt = cnt + 1.0;
        }
    reduce_pair(rsum, rcnt, tid, sum, cnt);
    double result = -INFINITY;
    if (cnt > 0.0) {                     // uniform: every thread holds the same totals
        const double gate = lkfs(sum / cnt) - 10.0;
        sum = 0.0;
        cnt = 0.0;
        for (long long j = tid; j < a1; j += kBlockThreads) {
            const double l = lkfs(z[j]);
            if (l > -70.0 && l > gate) {
                sum = sum + z[j];
                cnt = cnt + 1.0;
            }
        }
        reduce_pair(rsum, rcnt, tid, sum, cnt);
        if (cnt > 0.0) result = lkfs(sum / cnt);
    }
    if (tid == 0) r.integrated[p] = result;
}

// what the next call needs: the samples from R before its first sub-block on, the last kTail energies
template <typename Tin>
__global__ void ld_carry_kernel(Params p, Readout r, double* samples, long long pos, long long len, double* tail, int tl) {
    const int s = blockIdx.y;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const Tin* xs = reinterpret_cast<const Tin*>(p.x) + (long long)s * p.ld;
    const double* cs = p.carry ? p.carry + (long long)s * p.carry_len : nullptr;
    if (i < len) samples[(long long)s * len + i] = sample(p, xs, cs, pos + i);
    if (i < tl) tail[(long long)s * tl + i] = energy_at(r, s, r.e1 - tl + i);
}

}  // namespace

struct frt_loudness {
    int S = 0, C = 0, P = 0, R = 0;
    hipStream_t stream = nullptr;
    frt::DeviceBuffer pw, coef, weights, xin, sin, sout, out, pref, zb, start;
};

extern "C" int frt_loudness_create(frt_loudness** out, int streams, int channels_per_programme, const double* weights, int tp_zeros,
                                   const double* prototype) {
    FRT_REQUIRE(out, "frt_loudness_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(channels_per_programme >= 1 && channels_per_programme <= 64, "frt_loudness_create: %d channels per programme (1 .. 64)",
                channels_per_programme);
    FRT_REQUIRE(streams >= 1 && streams <= 65535 && streams % channels_per_programme == 0,
                "frt_loudness_create: %d streams (1 .. 65535, whole programmes of %d channels)", streams, channels_per_programme);
    FRT_REQUIRE(tp_zeros >= 1 && tp_zeros <= kMaxZeros, "frt_loudness_create: tp_zeros %d (1 .. %d)", tp_zeros, kMaxZeros);
    FRT_REQUIRE(weights && !is_device_pointer(weights), "frt_loudness_create: the weights are a host array of %d doubles", channels_per_programme);
    for (int c = 0; c < channels_per_programme; ++c)
        FRT_REQUIRE(std::isfinite(weights[c]) && weights[c] >= 0.0, "frt_loudness_create: weight %d is %g (finite, not negative)", c, weights[c]);
    FRT_REQUIRE(prototype && !is_device_pointer(prototype), "frt_loudness_create: the prototype is a host array of 8 tp_zeros + 1 doubles");
    const int R = tp_zeros;
    for (int i = 0; i <= 8 * R; ++i) FRT_REQUIRE(std::isfinite(prototype[i]), "frt_loudness_create: prototype[%d] is not finite", i);
    frt_loudness* h = new frt_loudness();
    h->S = streams;
    h->C = channels_per_programme;
    h->P = streams / channels_per_programme;
    h->R = R;
    // A^(75 c): column j is the state 75 c zero samples after the unit state e_j
    std::vector<double> pw((size_t)(kCells + 1) * 16);
    for (int j = 0; j < 4; ++j) {
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        st[j] = 1.0;
        for (int c = 0; c <= kCells; ++c) {
            for (int i = 0; i < 4; ++i) pw[(size_t)c * 16 + i * 4 + j] = st[i];
            for (int i = 0; i < kCell; ++i) (void)kw_step(0.0, st);
        }
    }
    std::vector<double> coef((size_t)(2 * R + 1) * 4, 0.0);
    for (int j = 0; j <= 2 * R; ++j) {
        coef[(size_t)4 * j] = prototype[8 * R - 4 * j];
        if (j < 2 * R)
            for (int q = 1; q < 4; ++q) coef[(size_t)4 * j + q] = prototype[8 * R + q - 4 - 4 * j];
    }
    std::vector<double> w(weights, weights + channels_per_programme);
    int rc = upload(h->pw, pw);
    if (!rc) rc = upload(h->coef, coef);
    if (!rc) rc = upload(h->weights, w);
    if (rc) {
        frt_loudness_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_loudness_destroy(frt_loudness* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->pw, &h->coef, &h->weights, &h->xin, &h->sin, &h->sout, &h->out, &h->pref, &h->zb, &h->start}) b->release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_loudness_set_stream(frt_loudness* h, void* s) {
    FRT_REQUIRE(h, "frt_loudness_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int64_t frt_loudness_state_length(const frt_loudness* h, int64_t n_in, int64_t blocks) {
    if (!h || n_in < 0 || blocks < 0 || blocks * kB > n_in) {
        set_last_error("frt_loudness_state_length: bad arguments (%lld samples, %lld sub-blocks)", (long long)n_in, (long long)blocks);
        return FRT_ERR_INVALID;
    }
    return (int64_t)h->S * (4 + (n_in - blocks * kB + h->R) + std::min<long long>(kTail, blocks)) + (int64_t)h->P * (n400(blocks) + n3s(blocks));
}

namespace {

template <typename Tin>
int launch(frt_loudness* h, Params& p, Readout& r, double* filt_out, double* samples, long long pos, long long len, double* tail, int tl) {
    if (p.ne > 0) {
        hipLaunchKernelGGL(ld_cells_kernel<Tin>, dim3(p.ne, h->S), dim3(kBlockThreads), 0, h->stream, p);
        FRT_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ld_scan_kernel, dim3(h->S), dim3(64), 0, h->stream, p, filt_out);
    FRT_HIP_CHECK(hipGetLastError());
    if (p.npk > 0) {
        const size_t lds = (size_t)(kB + 2 * p.R + kCells + 2 * kBlockThreads) * sizeof(double);
        hipLaunchKernelGGL(ld_block_kernel<Tin>, dim3(p.npk, h->S), dim3(kBlockThreads), lds, h->stream, p, h->coef.as<const double>());
        FRT_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ld_readout_kernel, dim3(h->P), dim3(kBlockThreads), 0, h->stream, r);
    FRT_HIP_CHECK(hipGetLastError());
    const long long most = std::max<long long>(len, tl);
    hipLaunchKernelGGL(ld_carry_kernel<Tin>, dim3((unsigned)((most + 255) / 256), h->S), dim3(256), 0, h->stream, p, r, samples, pos, len, tail, tl);
    FRT_HIP_CHECK(hipGetLastError());
    return FRT_OK;
}

}  // namespace

extern "C" int frt_loudness_run(frt_loudness* h, const void* x, int x_dtype, int64_t n, int64_t ld, const double* state_in, double* state_out,
                                int64_t first_in, int flush, int true_peak, double* out) {
    FRT_REQUIRE(h, "frt_loudness_run: null handle");
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "frt_loudness_run: dtype %d (0 float32, 1 float64)", x_dtype);
    FRT_REQUIRE(n >= 0 && ld >= n && (n == 0 || x), "frt_loudness_run: bad input (n %lld, ld %lld)", (long long)n, (long long)ld);
    FRT_REQUIRE(first_in >= 0 && first_in + n <= ((int64_t)1 << 40), "frt_loudness_run: bad position (%lld + %lld samples)", (long long)first_in,
                (long long)n);
    FRT_REQUIRE((flush == 0 || flush == 1) && (true_peak == 0 || true_peak == 1), "frt_loudness_run: flush %d, true_peak %d (0 or 1)", flush, true_peak);
    FRT_REQUIRE(state_in || first_in == 0, "frt_loudness_run: a stream continued without its state");
    FRT_REQUIRE(state_out && out, "frt_loudness_run: null state_out or out");
    FRT_REQUIRE(state_out != state_in, "frt_loudness_run: the state cannot be updated in place");
    const int S = h->S, P = h->P, R = h->R;
    const long long N = first_in + n;
    const Counts before = counts(first_in, R, false), after = counts(N, R, flush);
    const long long e0 = before.energies, e1 = after.energies, ne = e1 - e0, npk = after.peaks - e0;
    FRT_REQUIRE(npk <= 0x7fffffffLL, "frt_loudness_run: %lld sub-blocks in one call", npk);
    const long long len_in = first_in - e0 * kB + R, len_out = N - e1 * kB + R;
    const int tl_in = (int)std::min<long long>(kTail, e0), tl_out = (int)std::min<long long>(kTail, e1);
    const long long a0 = n400(e0), a1 = n400(e1), s0 = n3s(e0), s1 = n3s(e1);
    const size_t in_len = (size_t)S * (4 + len_in + tl_in) + (size_t)P * (a0 + s0);
    const size_t out_state_len = (size_t)S * (4 + len_out + tl_out) + (size_t)P * (a1 + s1);
    const size_t out_len = (size_t)S * (ne + 2 * npk) + (size_t)P * ((a1 - a0) + (s1 - s0) + 1);
    const size_t esize = x_dtype ? sizeof(double) : sizeof(float);
    int rc;
    Params p{};
    p.x = x;
    p.n = n;
    p.ld = ld;
    HostIO io(h->stream);
    if ((rc = io.in_rows(h->xin, p.x, p.ld, S, n, esize))) return rc;
    const double* din = state_in;
    if ((rc = io.in(h->sin, din, in_len))) return rc;
    double *dso = state_out, *dout = out;
    if ((rc = io.out(h->sout, dso, out_state_len))) return rc;
    if ((rc = io.out(h->out, dout, out_len))) return rc;
    if (ne > 0) {
        if ((rc = h->pref.reserve((size_t)S * ne * kCells * 4 * sizeof(double)))) return rc;
        if ((rc = h->zb.reserve((size_t)S * ne * 4 * sizeof(double)))) return rc;
        if ((rc = h->start.reserve((size_t)S * ne * 4 * sizeof(double)))) return rc;
    }
    // the state: filter states [S][4] | samples [S][len] | energy tail [S][tl] | z400 [P][a] | z3s [P][s]
    const double *filt_in = nullptr, *carry = nullptr, *tail_in = nullptr, *z400_in = nullptr, *z3s_in = nullptr;
    if (din) {
        filt_in = din;
        carry = filt_in + (size_t)S * 4;
        tail_in = carry + (size_t)S * len_in;
        z400_in = tail_in + (size_t)S * tl_in;
        z3s_in = z400_in + (size_t)P * a0;
    }
    double* filt_out = dso;
    double* samples_out = filt_out + (size_t)S * 4;
    double* tail_out = samples_out + (size_t)S * len_out;
    double* z400_out = tail_out + (size_t)S * tl_out;
    double* z3s_out = z400_out + (size_t)P * a1;
    // the results: energy [S][ne] | true peak [S][npk] | sample peak [S][npk] | momentary [P][..] | short-term [P][..] | integrated [P]
    p.carry = carry;
    p.first_in = first_in;
    p.carry_pos = e0 * kB - R;
    p.carry_len = len_in;
    p.total = N;
    p.b0 = e0;
    p.ne = (int)ne;
    p.npk = (int)npk;
    p.R = R;
    p.S = S;
    p.C = h->C;
    p.true_peak = true_peak;
    p.pw = h->pw.as<const double>();
    p.filt_in = filt_in;
    p.pref = h->pref.as<double>();
    p.zb = h->zb.as<double>();
    p.start = h->start.as<double>();
    p.energy = dout;
    p.tpk = p.energy + (size_t)S * ne;
    p.spk = p.tpk + (size_t)S * npk;
    Readout r{};
    r.tail = tail_in;
    r.energy = p.energy;
    r.z400_in = z400_in;
    r.z3s_in = z3s_in;
    r.z400 = z400_out;
    r.z3s = z3s_out;
    r.momentary = p.spk + (size_t)S * npk;
    r.short_term = r.momentary + (size_t)P * (a1 - a0);
    r.integrated = r.short_term + (size_t)P * (s1 - s0);
    r.weights = h->weights.as<const double>();
    r.e0 = e0;
    r.e1 = e1;
    r.tl = tl_in;
    r.ne = (int)ne;
    r.C = h->C;
    if ((rc = x_dtype ? launch<double>(h, p, r, filt_out, samples_out, e1 * kB - R, len_out, tail_out, tl_out)
                      : launch<float>(h, p, r, filt_out, samples_out, e1 * kB - R, len_out, tail_out, tl_out)))
        return rc;
    return io.finish();
}
