// deconvolve.hip — X4: the float64 real transform of whole rows of n = 2^13 .. 2^24 samples (frt_rfft_long_rows,
// frt_irfft_long_rows) and deconvolution by regularised spectral division built on it (frt_deconvolve_*, DeconvolveBatch).
// The definition: X4 in include/friture_hip.h.
//
// A real n-point transform is one complex transform of Mc = n / 2 points of z[m] = x[2 m] + i x[2 m + 1] and the unpack of
// rfft64.h's users.  Mc does not fit one workgroup's LDS: Mc = N1 N2, N1 = 2^floor(log2 Mc / 2) <= N2, both in 64 .. 4096, and
// with m = n1 N2 + n2, k = k1 + N1 k2 the transform runs in four steps over two scratch rows A and Z of complex128:
//   lf_column_kernel<log2 N1>: G adjacent columns n2 per workgroup.  The points are read in runs of G (from the caller's row:
//     float32 or float64, zeros behind its T samples; or complex from scratch) into the frames' LDS, each frame goes through
//     fft_core.h's N1-point transform (8 points per thread), is multiplied by exp(-2 pi i k1 n2 / Mc) and leaves through the
//     LDS again in runs of G: A[k1 N2 + n2].
//   lf_row_kernel<log2 N2>: G adjacent rows k1 per workgroup, read along the row, N2-point transform, stored transposed in
//     runs of G through the LDS: Z[k1 + N1 k2]; as the last pass of an inverse it stores the reals r[2 m] = Re, r[2 m + 1] = -Im
//     up to `keep` instead.
//   lf_pair_kernel: one thread per pair (k, Mc - k): the unpack X[k] = Ze + w^k Zo, X[Mc - k] = conj(Ze - w^k Zo) (w =
//     exp(-i pi / Mc)), the product with G[k], and the pack for the inverse W[k] = conj(((A + B) + i conj(w^k) (A - B)) / n),
//     A = H[k], B = conj H[Mc - k].  The pack stores the conjugate, so the inverse IS the forward passes on W followed by the
//     conjugating real store: no second set of instances.
// exp(-2 pi i j / M) for the step between the passes and for the pair kernel is the product of a coarse entry (j / 4096) and a
// fine entry (j mod 4096) of two host-made tables (long double, rounded once): one more complex product, no device sincos.
// The translation unit is compiled without floating-point contraction; nothing is atomic; a row's bits depend on the row, n,
// and the reference alone.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "hostio.h"
#include "rfft64.h"

using namespace frt;

namespace {

using rfft64::C;

constexpr int kMinLog2 = 13, kMaxLog2 = 24;
constexpr int kFineBits = 12, kFine = 1 << kFineBits;            // entries of a fine twiddle table
constexpr long long kMaxTableBytes = 1LL << 30;
constexpr long long kDefaultScratch = 1LL << 28;                 // the reference's transform at frt_deconvolve_create

// One pass kernel's workgroup: G frames of N points, N / 8 threads each.  G >= 4 wherever G N <= 8192 points fit the LDS
// (N = 4096: 2).  Frame g starts SKEW slots behind a multiple of the padded frame, so that the 16-byte LDS accesses of the
// staging (8 lanes: 8 / G consecutive points of each of G frames) fall on 8 different bank groups.
template <int LOG2>
struct Geo {
    static constexpr int N = 1 << LOG2, TPF = N / 8;
    static constexpr bool WAVE_LOCAL = rfft64::Plan<LOG2>::WAVE_LOCAL;
    static constexpr int G = N >= 4096 ? 2 : N >= 512 ? 4 : 8;
    static constexpr int BLOCK = G * TPF;
    static constexpr int STRIDE = lds_padded_size(N) + 8 / G;
    static constexpr size_t LDS = (size_t)G * STRIDE * sizeof(C);
};

struct PassParams {
    const void* in;                               // rows of reals (kind 0 float32, 1 float64) or of complex128 (kind 2)
    int kind;
    long long in_stride, T;                       // elements between rows; live samples of a row of reals
    C* out;                                       // complex rows
    long long out_stride;
    double* real_out;                             // row pass only: not null: the reals, scaled already, up to keep
    long long real_stride, keep;
    int other;                                    // the other factor: N2 for the column pass, N1 for the row pass
    const C *tw, *twc, *twf;                      // exp(-2 pi i n / N); column pass: exp(-2 pi i 4096 c / Mc), exp(-2 pi i f / Mc)
};

template <int LOG2>
__global__ __launch_bounds__(Geo<LOG2>::BLOCK) void lf_column_kernel(const PassParams p) {
    using R = Geo<LOG2>;
    constexpr int TPF = R::TPF, G = R::G;
    constexpr bool WL = R::WAVE_LOCAL;
    extern __shared__ __attribute__((aligned(16))) char lf_smem[];
    C* all = reinterpret_cast<C*>(lf_smem);
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = all + item * R::STRIDE;
    const long long s = blockIdx.y;
    const int N2 = p.other, col0 = blockIdx.x * G;

#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = tid + it * R::BLOCK, g = idx & (G - 1), r = idx / G;
        const long long m = (long long)r * N2 + col0 + g;
        C z = C{0.0, 0.0};
        if (p.kind == 2) {
            z = reinterpret_cast<const C*>(p.in)[s * p.in_stride + m];
        } else if (p.kind == 1) {
            const double* xs = reinterpret_cast<const double*>(p.in) + s * p.in_stride;
            if (2 * m < p.T) z.x = xs[2 * m];
            if (2 * m + 1 < p.T) z.y = xs[2 * m + 1];
        } else {
            const float* xs = reinterpret_cast<const float*>(p.in) + s * p.in_stride;
            if (2 * m < p.T) z.x = (double)xs[2 * m];
            if (2 * m + 1 < p.T) z.y = (double)xs[2 * m + 1];
        }
        all[g * R::STRIDE + lds_pad(r)] = z;
    }
    __syncthreads();
    C v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = buf[lds_pad(i + j * TPF)];
    pass_sync<WL>();                                             // the frame is read: the transform may scatter into buf
    TwTable<double, LOG2> tw{p.tw, 0};
    fft_pow2_forward<double, LOG2, WL>(v, buf, i, tw);
    pass_sync<WL>();                                             // the last gathers of the transform are done
    const int n2 = col0 + item;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k1 = i + j * TPF, at = k1 * n2;                // < Mc <= 2^23
        const C w = cmul(p.twc[at >> kFineBits], p.twf[at & (kFine - 1)]);
        buf[lds_pad(k1)] = cmul(v[j], w);
    }
    __syncthreads();
    C* out = p.out + s * p.out_stride;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = tid + it * R::BLOCK, g = idx & (G - 1), r = idx / G;
        out[(long long)r * N2 + col0 + g] = all[g * R::STRIDE + lds_pad(r)];
    }
}

template <int LOG2>
__global__ __launch_bounds__(Geo<LOG2>::BLOCK) void lf_row_kernel(const PassParams p) {
    using R = Geo<LOG2>;
    constexpr int N = R::N, TPF = R::TPF, G = R::G;
    constexpr bool WL = R::WAVE_LOCAL;
    extern __shared__ __attribute__((aligned(16))) char lf_smem[];
    C* all = reinterpret_cast<C*>(lf_smem);
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = all + item * R::STRIDE;
    const long long s = blockIdx.y;
    const int N1 = p.other, row0 = blockIdx.x * G;

    const C* in = reinterpret_cast<const C*>(p.in) + s * p.in_stride + (long long)(row0 + item) * N;
    C v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = in[i + j * TPF];
    TwTable<double, LOG2> tw{p.tw, 0};
    fft_pow2_forward<double, LOG2, WL>(v, buf, i, tw);
    pass_sync<WL>();
#pragma unroll
    for (int j = 0; j < 8; ++j) buf[lds_pad(i + j * TPF)] = v[j];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = tid + it * R::BLOCK, g = idx & (G - 1), r = idx / G;
        const C z = all[g * R::STRIDE + lds_pad(r)];
        const long long m = row0 + g + (long long)N1 * r;
        if (!p.real_out) {
            p.out[s * p.out_stride + m] = z;
        } else {
            double* y = p.real_out + s * p.real_stride;
            if (2 * m < p.keep) y[2 * m] = z.x;
            if (2 * m + 1 < p.keep) y[2 * m + 1] = -z.y;
        }
    }
}

enum PairMode { kUnpack = 0, kDivide = 1, kPack = 2 };

struct PairParams {
    int mode;
    long long Mc;
    const C* Z;                                   // kUnpack, kDivide: the complex transform [rows][z_stride]
    long long z_stride;
    const C* spec_in;                             // kPack: half spectra [rows][Mc + 1]
    C* spec_out;                                  // kUnpack: X; kDivide: H, or null; [rows][Mc + 1]
    const C* G;                                   // kDivide: [refs][Mc + 1]
    long long g_stride;                           // 0: one reference for all rows
    C* W;                                         // kDivide, kPack: the packed conjugate [rows][w_stride]
    long long w_stride;
    const C *pc, *pf;                             // exp(-2 pi i 4096 c / n), exp(-2 pi i f / n)
    double scale;                                 // 1 / n
};

__global__ __launch_bounds__(256) void lf_pair_kernel(const PairParams p) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x, Mc = p.Mc, s = blockIdx.y;
    if (k > Mc / 2) return;
    const long long kk = Mc - k;                                 // k = 0: bin Mc; k = Mc / 2: the bin itself
    const C w = cmul(p.pc[k >> kFineBits], p.pf[k & (kFine - 1)]);
    C xa, xb;
    if (p.mode != kPack) {
        const C* Z = p.Z + s * p.z_stride;
        const C a = Z[k], b = cconj(Z[kk & (Mc - 1)]);
        const C ze = {(a.x + b.x) * 0.5, (a.y + b.y) * 0.5};
        const C zo = mul_mi(C{(a.x - b.x) * 0.5, (a.y - b.y) * 0.5});
        const C t = cmul(w, zo);
        xa = ze + t;
        xb = ze - t;
        if (k != 0) xb = cconj(xb);
        if (kk == k) xb = xa;                                    // bin Mc / 2 is its own partner: one value
    } else {
        const C* X = p.spec_in + s * (Mc + 1);
        xa = X[k];
        xb = X[kk];
    }
    if (p.mode == kDivide) {
        const C* G = p.G + s * p.g_stride;
        xa = cmul(xa, G[k]);
        xb = cmul(xb, G[kk]);
    }
    if (p.mode != kPack && p.spec_out) {
        C* X = p.spec_out + s * (Mc + 1);
        X[k] = xa;
        if (kk != k) X[kk] = xb;
    }
    if (p.mode == kUnpack) return;
    if (k == 0) xa.y = xb.y = 0.0;                               // the imaginary parts of bins 0 and n / 2 do not count
    const C a = xa, b = cconj(xb);
    const C sum = a + b, t = cmul(cconj(w), a - b);
    C* W = p.W + s * p.w_stride;
    W[k] = C{(sum.x - t.y) * p.scale, -((sum.y + t.x) * p.scale)};             // conj((sum + i t) / n)
    if (k != 0 && kk != k) W[kk] = C{(sum.x + t.y) * p.scale, -((t.x - sum.y) * p.scale)};      // conj((conj sum + i conj t) / n)
}

// Pmax[ref] = max_k |X[k]|^2 over the bins 0 .. Mc (a maximum has no order): kPmaxParts workgroups per reference leave
// partial maxima (X = the spectra, `from` = null), then one workgroup per reference folds them (`from` = the partials)
constexpr int kPmaxParts = 256;

__global__ __launch_bounds__(256) void dc_pmax_kernel(const C* X, long long Mc, const double* from, double* to) {
    __shared__ double part[256];
    double m = 0.0;
    if (from) {
        m = from[(long long)blockIdx.y * kPmaxParts + threadIdx.x];
    } else {
        const C* row = X + (long long)blockIdx.y * (Mc + 1);
        for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k <= Mc; k += 256LL * kPmaxParts)
            m = fmax(m, row[k].x * row[k].x + row[k].y * row[k].y);
    }
    part[threadIdx.x] = m;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) to[(long long)blockIdx.y * gridDim.x + blockIdx.x] = part[0];
}

// in place X -> G = conj(X) / (P + r Pmax), 0 where the denominator is 0
__global__ __launch_bounds__(256) void dc_inverse_kernel(C* X, long long Mc, const double* pmax, double reg, const double* reg_bins) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k > Mc) return;
    C* at = X + (long long)blockIdx.y * (Mc + 1) + k;
    const C x = *at;
    const double r = reg_bins ? reg_bins[k] : reg;
    const double den = (x.x * x.x + x.y * x.y) + r * pmax[blockIdx.y];
    *at = den == 0.0 ? C{0.0, 0.0} : C{x.x / den, -x.y / den};
}

typedef void (*PassKernel)(const PassParams);

struct PassLaunch {
    PassKernel kernel = nullptr;
    int block = 0, group = 0;
    size_t lds = 0;
};

// exp(-2 pi i step j / M), j < count
std::vector<C> roots(long long M, long long step, long long count) {
    std::vector<C> t((size_t)count);
    const long double unit = -2.0L * 3.14159265358979323846264338327950288L / (long double)M;
    for (long long j = 0; j < count; ++j) t[(size_t)j] = C{(double)cosl(unit * (long double)(step * j)), (double)sinl(unit * (long double)(step * j))};
    return t;
}

// the transform of n real points: the factors, the two pass kernels and the tables (one device block)
struct LongPlan {
    long long n = 0, Mc = 0;
    int N1 = 0, N2 = 0;
    PassLaunch col, row;
    DeviceBuffer tables;
    const C *tw1 = nullptr, *tw2 = nullptr, *twc = nullptr, *twf = nullptr, *pc = nullptr, *pf = nullptr;

    int init(long long n_, const char* who) {
        n = n_;
        Mc = n / 2;
        const int l = rfft64::log2_of(Mc), l1 = l / 2, l2 = l - l1;
        N1 = 1 << l1;
        N2 = 1 << l2;
        const bool found = rfft64::dispatch<6, 11>(l1, [&](auto v) {
            using R = Geo<decltype(v)::value>;
            col = PassLaunch{lf_column_kernel<decltype(v)::value>, R::BLOCK, R::G, R::LDS};
        }) && rfft64::dispatch<6, 12>(l2, [&](auto v) {
            using R = Geo<decltype(v)::value>;
            row = PassLaunch{lf_row_kernel<decltype(v)::value>, R::BLOCK, R::G, R::LDS};
        });
        if (!found) {
            set_last_error("%s: no kernel for n %lld", who, n);
            return FRT_ERR_UNSUPPORTED;
        }
        int rc = rfft64::allow_lds((const void*)col.kernel, col.lds, who, "n", (int)n);
        if (!rc) rc = rfft64::allow_lds((const void*)row.kernel, row.lds, who, "n", (int)n);
        if (rc) return rc;
        std::vector<C> t = rfft64::twiddles(N1, false);
        const size_t o2 = t.size();
        for (const std::vector<C>& part : {rfft64::twiddles(N2, false), roots(Mc, kFine, std::max(1LL, Mc / kFine)), roots(Mc, 1, kFine),
                                           roots(n, kFine, Mc / 2 / kFine + 1), roots(n, 1, kFine)})
            t.insert(t.end(), part.begin(), part.end());
        if ((rc = upload(tables, t))) return rc;
        tw1 = tables.as<const C>();
        tw2 = tw1 + o2;
        twc = tw2 + N2;
        twf = twc + std::max(1LL, Mc / kFine);
        pc = twf + kFine;
        pf = pc + (Mc / 2 / kFine + 1);
        return FRT_OK;
    }

    int launch(const PassLaunch& k, int frames, int rows, hipStream_t stream, const PassParams& p) const {
        hipLaunchKernelGGL(k.kernel, dim3((unsigned)(frames / k.group), (unsigned)rows), dim3(k.block), k.lds, stream, p);
        FRT_HIP_CHECK(hipGetLastError());
        return FRT_OK;
    }

    // `rows` rows of T live reals -> their complex transforms Z [rows][Mc + 1] (A: scratch of the same shape)
    int forward(const void* x, int dtype, long long stride, long long T, int rows, C* A, C* Z, hipStream_t stream) const {
        PassParams p{};
        p.in = x;
        p.kind = dtype;
        p.in_stride = stride;
        p.T = T;
        p.out = A;
        p.out_stride = Mc + 1;
        p.other = N2;
        p.tw = tw1;
        p.twc = twc;
        p.twf = twf;
        int rc = launch(col, N2, rows, stream, p);
        if (rc) return rc;
        PassParams q{};
        q.in = A;
        q.kind = 2;
        q.in_stride = Mc + 1;
        q.out = Z;
        q.out_stride = Mc + 1;
        q.other = N1;
        q.tw = tw2;
        return launch(row, N1, rows, stream, q);
    }

    // the packed rows W [rows][Mc + 1] -> the first `keep` reals of every row (Z: scratch)
    int inverse(const C* W, C* Z, int rows, double* out, long long out_stride, long long keep, hipStream_t stream) const {
        PassParams p{};
        p.in = W;
        p.kind = 2;
        p.in_stride = Mc + 1;
        p.out = Z;
        p.out_stride = Mc + 1;
        p.other = N2;
        p.tw = tw1;
        p.twc = twc;
        p.twf = twf;
        int rc = launch(col, N2, rows, stream, p);
        if (rc) return rc;
        PassParams q{};
        q.in = Z;
        q.kind = 2;
        q.in_stride = Mc + 1;
        q.real_out = out;
        q.real_stride = out_stride;
        q.keep = keep;
        q.other = N1;
        q.tw = tw2;
        return launch(row, N1, rows, stream, q);
    }

    int pair(PairParams p, int rows, hipStream_t stream) const {
        p.Mc = Mc;
        p.pc = pc;
        p.pf = pf;
        p.scale = 1.0 / (double)n;
        hipLaunchKernelGGL(lf_pair_kernel, dim3((unsigned)((Mc / 2 + 1 + 255) / 256), (unsigned)rows), dim3(256), 0, stream, p);
        FRT_HIP_CHECK(hipGetLastError());
        return FRT_OK;
    }

    long long row_bytes() const { return 2 * (Mc + 1) * (long long)sizeof(C); }        // A and Z of one row
    long long slab_rows(long long rows, long long scratch_bytes) const {
        return std::min(rows, std::max(1LL, scratch_bytes / row_bytes()));
    }
};

bool long_size(long long n) { return n >= (1LL << kMinLog2) && n <= (1LL << kMaxLog2) && (n & (n - 1)) == 0; }

// What the two stateless entries keep between calls: the plan of every n they have served, the staging of host arrays and
// one scratch block, all grow-only.  Allocating and freeing them per call cost 1 ms beside 30 us of kernels.  A process-level
// object made on first use and never destroyed (no HIP call runs from a static destructor at exit); the calls hold its mutex
// and synchronise their stream before they return, so no launch outlives the call that owns the blocks.  A block above
// kKeepBytes (more than one row of the top size needs) is released when its call ends.
struct Stateless {
    std::mutex lock;
    LongPlan* plans[kMaxLog2 + 1] = {};
    DeviceBuffer in, out, scratch;

    int plan(long long n, const char* who, const LongPlan** found) {
        LongPlan*& p = plans[rfft64::log2_of(n)];
        if (!p) {
            LongPlan* made = new LongPlan();
            const int rc = made->init(n, who);
            if (rc) {
                made->tables.release();
                delete made;
                return rc;
            }
            p = made;
        }
        *found = p;
        return FRT_OK;
    }
    void end(int rc, hipStream_t stream) {
        if (rc) (void)hipStreamSynchronize(stream);
        for (DeviceBuffer* b : {&in, &out, &scratch})
            if (b->bytes > kKeepBytes) b->release();
    }
    static constexpr size_t kKeepBytes = (size_t)1 << 29;
};

Stateless& stateless() {
    static Stateless* s = new Stateless();
    return *s;
}

}  // namespace

extern "C" int frt_rfft_long_rows(const void* x, int x_dtype, int rows, int64_t T, int64_t row_stride, int64_t n, int64_t scratch_bytes,
                                  double* spec, void* hip_stream) {
    FRT_REQUIRE(x && spec, "frt_rfft_long_rows: null buffer");
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "frt_rfft_long_rows: x_dtype %d (0 float32, 1 float64)", x_dtype);
    FRT_REQUIRE(long_size(n), "frt_rfft_long_rows: n %lld (a power of two, 2^13 .. 2^24)", (long long)n);
    FRT_REQUIRE(T >= 1 && T <= n, "frt_rfft_long_rows: T %lld (1 .. n)", (long long)T);
    FRT_REQUIRE(rows >= 1 && rows <= 65535, "frt_rfft_long_rows: %d rows (1 .. 65535)", rows);
    FRT_REQUIRE(rows == 1 || row_stride >= T, "frt_rfft_long_rows: bad stride (T %lld, row stride %lld)", (long long)T, (long long)row_stride);
    FRT_REQUIRE(scratch_bytes >= 0, "frt_rfft_long_rows: scratch_bytes %lld", (long long)scratch_bytes);
    hipStream_t stream = (hipStream_t)hip_stream;
    Stateless& kept = stateless();
    std::lock_guard<std::mutex> guard(kept.lock);
    auto run = [&]() -> int {
        const LongPlan* found = nullptr;
        int rc = kept.plan(n, "frt_rfft_long_rows", &found);
        if (rc) return rc;
        const LongPlan& plan = *found;
        const long long Mc = plan.Mc, per = plan.slab_rows(rows, scratch_bytes);
        HostIO io(stream);
        const void* xs = x;
        long long ld = row_stride;
        if ((rc = io.in_rows(kept.in, xs, ld, (size_t)rows, T, x_dtype ? sizeof(double) : sizeof(float)))) return rc;
        double* X = spec;
        if ((rc = io.out(kept.out, X, (size_t)rows * (Mc + 1) * 2))) return rc;
        if ((rc = kept.scratch.reserve((size_t)(per * plan.row_bytes())))) return rc;
        C *A = kept.scratch.as<C>(), *Z = A + per * (Mc + 1);
        const size_t esize = x_dtype ? sizeof(double) : sizeof(float);
        for (long long r0 = 0; r0 < rows; r0 += per) {
            const int nr = (int)std::min<long long>(per, rows - r0);
            if ((rc = plan.forward(reinterpret_cast<const char*>(xs) + r0 * ld * esize, x_dtype, ld, T, nr, A, Z, stream))) return rc;
            PairParams q{};
            q.mode = kUnpack;
            q.Z = Z;
            q.z_stride = Mc + 1;
            q.spec_out = reinterpret_cast<C*>(X) + r0 * (Mc + 1);
            if ((rc = plan.pair(q, nr, stream))) return rc;
        }
        return io.finish();
    };
    const int rc = run();
    kept.end(rc, stream);
    return rc;
}

extern "C" int frt_irfft_long_rows(const double* spec, int rows, int64_t n, int64_t keep, int64_t scratch_bytes, double* out,
                                   int64_t out_stride, void* hip_stream) {
    FRT_REQUIRE(spec && out, "frt_irfft_long_rows: null buffer");
    FRT_REQUIRE(long_size(n), "frt_irfft_long_rows: n %lld (a power of two, 2^13 .. 2^24)", (long long)n);
    FRT_REQUIRE(keep >= 1 && keep <= n, "frt_irfft_long_rows: keep %lld (1 .. n)", (long long)keep);
    FRT_REQUIRE(rows >= 1 && rows <= 65535, "frt_irfft_long_rows: %d rows (1 .. 65535)", rows);
    FRT_REQUIRE(rows == 1 || out_stride >= keep, "frt_irfft_long_rows: bad stride (keep %lld, out stride %lld)", (long long)keep,
                (long long)out_stride);
    FRT_REQUIRE(scratch_bytes >= 0, "frt_irfft_long_rows: scratch_bytes %lld", (long long)scratch_bytes);
    hipStream_t stream = (hipStream_t)hip_stream;
    Stateless& kept = stateless();
    std::lock_guard<std::mutex> guard(kept.lock);
    auto run = [&]() -> int {
        const LongPlan* found = nullptr;
        int rc = kept.plan(n, "frt_irfft_long_rows", &found);
        if (rc) return rc;
        const LongPlan& plan = *found;
        const long long Mc = plan.Mc, per = plan.slab_rows(rows, scratch_bytes);
        HostIO io(stream);
        const double* X = spec;
        if ((rc = io.in(kept.in, X, (size_t)rows * (Mc + 1) * 2))) return rc;
        void* y = out;
        long long ld = out_stride;
        if ((rc = io.out_rows(kept.out, y, ld, (size_t)rows, keep, sizeof(double)))) return rc;
        if ((rc = kept.scratch.reserve((size_t)(per * plan.row_bytes())))) return rc;
        C *A = kept.scratch.as<C>(), *Z = A + per * (Mc + 1);
        for (long long r0 = 0; r0 < rows; r0 += per) {
            const int nr = (int)std::min<long long>(per, rows - r0);
            PairParams q{};
            q.mode = kPack;
            q.spec_in = reinterpret_cast<const C*>(X) + r0 * (Mc + 1);
            q.W = A;
            q.w_stride = Mc + 1;
            if ((rc = plan.pair(q, nr, stream))) return rc;
            if ((rc = plan.inverse(A, Z, nr, reinterpret_cast<double*>(y) + r0 * ld, ld, keep, stream))) return rc;
        }
        return io.finish();
    };
    const int rc = run();
    kept.end(rc, stream);
    return rc;
}

struct frt_deconvolve {
    LongPlan plan;
    int refs = 0;
    long long Lx = 0;
    hipStream_t stream = nullptr;
    DeviceBuffer G, xin, hout, sout, scratch;
};

extern "C" int frt_deconvolve_create(frt_deconvolve** out, const double* x, int64_t Lx, int refs, int64_t n, double reg,
                                     const double* reg_bins) {
    FRT_REQUIRE(out, "frt_deconvolve_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(x, "frt_deconvolve_create: null reference");
    FRT_REQUIRE(long_size(n), "frt_deconvolve_create: n %lld (a power of two, 2^13 .. 2^24)", (long long)n);
    FRT_REQUIRE(Lx >= 1 && Lx <= n, "frt_deconvolve_create: Lx %lld (1 .. n)", (long long)Lx);
    FRT_REQUIRE(refs >= 1 && refs <= 65535, "frt_deconvolve_create: %d references (1 .. 65535)", refs);
    FRT_REQUIRE(std::isfinite(reg) && reg >= 0.0, "frt_deconvolve_create: reg %g (finite, >= 0)", reg);
    const long long Mc = n / 2, table = (long long)refs * (Mc + 1) * (long long)sizeof(C);
    FRT_REQUIRE_CODE(table <= kMaxTableBytes, FRT_ERR_UNSUPPORTED,
                     "frt_deconvolve_create: the inverse spectra of %d references at n %lld take %lld bytes: not supported (at most 2^30)", refs,
                     (long long)n, table);
    FRT_REQUIRE(!is_device_pointer(x) && !(reg_bins && is_device_pointer(reg_bins)),
                "frt_deconvolve_create: the reference and reg_bins are host arrays of doubles");
    for (long long i = 0; i < (long long)refs * Lx; ++i) FRT_REQUIRE(std::isfinite(x[i]), "frt_deconvolve_create: x[%lld] is not finite", i);
    if (reg_bins)
        for (long long k = 0; k <= Mc; ++k)
            FRT_REQUIRE(std::isfinite(reg_bins[k]) && reg_bins[k] >= 0.0, "frt_deconvolve_create: reg_bins[%lld] %g (finite, >= 0)", k, reg_bins[k]);
    frt_deconvolve* h = new frt_deconvolve();
    h->refs = refs;
    h->Lx = Lx;
    auto fill = [&]() -> int {
        int rc = h->plan.init(n, "frt_deconvolve_create");
        if (rc) return rc;
        const LongPlan& plan = h->plan;
        const long long per = plan.slab_rows(refs, kDefaultScratch);
        if ((rc = h->G.reserve((size_t)table))) return rc;
        if ((rc = h->xin.reserve((size_t)refs * Lx * sizeof(double)))) return rc;
        if ((rc = h->scratch.reserve((size_t)(per * plan.row_bytes())))) return rc;
        DeviceBuffer aux;                                        // Pmax [refs] | its partials [refs][kPmaxParts] | reg_bins [Mc + 1]
        if ((rc = aux.reserve(((size_t)refs * (1 + kPmaxParts) + (reg_bins ? (size_t)Mc + 1 : 0)) * sizeof(double)))) return rc;
        auto work = [&]() -> int {
            FRT_HIP_CHECK(hipMemcpy(h->xin.ptr, x, (size_t)refs * Lx * sizeof(double), hipMemcpyHostToDevice));
            double *pmax = aux.as<double>(), *parts = pmax + refs, *bins = nullptr;
            if (reg_bins) {
                bins = parts + (size_t)refs * kPmaxParts;
                FRT_HIP_CHECK(hipMemcpy(bins, reg_bins, (size_t)(Mc + 1) * sizeof(double), hipMemcpyHostToDevice));
            }
            C *A = h->scratch.as<C>(), *Z = A + per * (Mc + 1);
            for (long long r0 = 0; r0 < refs; r0 += per) {
                const int nr = (int)std::min<long long>(per, refs - r0);
                int r = plan.forward(h->xin.as<double>() + r0 * Lx, 1, Lx, Lx, nr, A, Z, nullptr);
                if (r) return r;
                PairParams q{};
                q.mode = kUnpack;
                q.Z = Z;
                q.z_stride = Mc + 1;
                q.spec_out = h->G.as<C>() + r0 * (Mc + 1);
                if ((r = plan.pair(q, nr, nullptr))) return r;
            }
            hipLaunchKernelGGL(dc_pmax_kernel, dim3(kPmaxParts, (unsigned)refs), dim3(256), 0, nullptr, h->G.as<const C>(), Mc,
                               (const double*)nullptr, parts);
            FRT_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(dc_pmax_kernel, dim3(1, (unsigned)refs), dim3(256), 0, nullptr, (const C*)nullptr, Mc, (const double*)parts, pmax);
            FRT_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(dc_inverse_kernel, dim3((unsigned)((Mc + 1 + 255) / 256), (unsigned)refs), dim3(256), 0, nullptr, h->G.as<C>(), Mc,
                               pmax, reg, bins);
            FRT_HIP_CHECK(hipGetLastError());
            FRT_HIP_CHECK(hipStreamSynchronize(nullptr));
            return FRT_OK;
        };
        rc = work();
        if (rc) (void)hipDeviceSynchronize();
        aux.release();
        return rc;
    };
    const int rc = fill();
    if (rc) {
        frt_deconvolve_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_deconvolve_destroy(frt_deconvolve* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->plan.tables, &h->G, &h->xin, &h->hout, &h->sout, &h->scratch}) b->release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_deconvolve_set_stream(frt_deconvolve* h, void* s) {
    FRT_REQUIRE(h, "frt_deconvolve_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_deconvolve_run(frt_deconvolve* h, const void* y, int y_dtype, int rows, int64_t T, int64_t row_stride, int64_t keep,
                                  int64_t scratch_bytes, double* out, int64_t out_stride, double* spectrum) {
    FRT_REQUIRE(h, "frt_deconvolve_run: null handle");
    FRT_REQUIRE(y && out, "frt_deconvolve_run: null buffer");
    FRT_REQUIRE(y_dtype == 0 || y_dtype == 1, "frt_deconvolve_run: y_dtype %d (0 float32, 1 float64)", y_dtype);
    const LongPlan& plan = h->plan;
    const long long n = plan.n, Mc = plan.Mc;
    FRT_REQUIRE(rows >= 1 && rows <= 65535, "frt_deconvolve_run: %d rows (1 .. 65535)", rows);
    FRT_REQUIRE(h->refs == 1 || h->refs == rows, "frt_deconvolve_run: %d references for %d rows (one for all, or one per row)", h->refs, rows);
    FRT_REQUIRE(T >= 1 && T <= n, "frt_deconvolve_run: T %lld (1 .. n = %lld)", (long long)T, n);
    FRT_REQUIRE(keep >= 1 && keep <= n, "frt_deconvolve_run: keep %lld (1 .. n = %lld)", (long long)keep, n);
    FRT_REQUIRE(rows == 1 || (row_stride >= T && out_stride >= keep), "frt_deconvolve_run: bad stride (T %lld, row stride %lld; keep %lld, out stride %lld)",
                (long long)T, (long long)row_stride, (long long)keep, (long long)out_stride);
    FRT_REQUIRE(scratch_bytes >= 0, "frt_deconvolve_run: scratch_bytes %lld", (long long)scratch_bytes);
    int rc;
    HostIO io(h->stream);
    const size_t esize = y_dtype ? sizeof(double) : sizeof(float);
    const void* ys = y;
    long long ld = row_stride, old = out_stride;
    if ((rc = io.in_rows(h->xin, ys, ld, (size_t)rows, T, esize))) return rc;
    void* hs = out;
    if ((rc = io.out_rows(h->hout, hs, old, (size_t)rows, keep, sizeof(double)))) return rc;
    double* S = spectrum;
    if ((rc = io.out(h->sout, S, (size_t)rows * (Mc + 1) * 2))) return rc;
    const long long per = plan.slab_rows(rows, scratch_bytes);
    if ((rc = h->scratch.reserve((size_t)(per * plan.row_bytes())))) return rc;
    C *A = h->scratch.as<C>(), *Z = A + per * (Mc + 1);
    for (long long r0 = 0; r0 < rows; r0 += per) {
        const int nr = (int)std::min<long long>(per, rows - r0);
        if ((rc = plan.forward(reinterpret_cast<const char*>(ys) + r0 * ld * esize, y_dtype, ld, T, nr, A, Z, h->stream))) return rc;
        PairParams q{};
        q.mode = kDivide;
        q.Z = Z;
        q.z_stride = Mc + 1;
        q.spec_out = S ? reinterpret_cast<C*>(S) + r0 * (Mc + 1) : nullptr;
        q.g_stride = h->refs == 1 ? 0 : Mc + 1;
        q.G = h->G.as<const C>() + r0 * q.g_stride;
        q.W = A;
        q.w_stride = Mc + 1;
        if ((rc = plan.pair(q, nr, h->stream))) return rc;
        if ((rc = plan.inverse(A, Z, nr, reinterpret_cast<double*>(hs) + r0 * old, old, keep, h->stream))) return rc;
    }
    return io.finish();
}
