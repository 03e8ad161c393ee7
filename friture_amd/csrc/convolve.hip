// convolve.hip — X2: uniformly partitioned FFT convolution of recordings with a caller's FIR (frt_convolve_*, ConvolveBatch),
// and the inverse real transform of rows of half spectra (frt_irfft_rows, impulse_response).  The definition: X2 in
// include/friture_hip.h.
//
// Two kernels per time slab, one code path per block size B (64 .. 4096); a frame of B complex points is served by B / 8
// threads (fft_core.h, float64, 8 points per thread: wave-local up to B = 512, one workgroup of B / 8 threads above).
//   cv_window_kernel<LOG2B>: one window of 2 B real samples per frame group.  z[n] = x[2 n] + i x[2 n + 1] goes through ONE
//     B-point complex transform; Z goes once more through the frame's LDS so that the owner of bin k reads Z[B - k], and the
//     unpack X[k] = Ze[k] + w^k Zo[k] (Ze = (Z[k] + conj Z[B - k]) / 2, Zo = -i (Z[k] - conj Z[B - k]) / 2, w = exp(-i pi / B))
//     writes the B + 1 bins to the slab's scratch.  The same kernel makes the tap spectra H_p at frt_convolve_create (windows
//     that start at p B with B live samples).  Samples come from the carried tail, from the call's rows in place (float32 or
//     float64, strided), or are zeros (before the stream, and behind its end for a flushed stream).
//   cv_block_kernel<LOG2B>: one tile of kTile = 2 consecutive output blocks per frame group.  Step p loads H_p[k] and the one
//     window spectrum X_{j0 - p}[k] that the tile has not seen yet (the tile's windows stay in a register ring whose slots are
//     static because p is unrolled by kTile), and every block of the tile adds X_{j - p} H_p to ITS OWN accumulators with
//     explicit fused multiply-adds, p = 0 .. P - 1 in order: a block's bits do not depend on its place in a tile.  Then per
//     block the pack Z[k] = ((A + B) + i conj(w^k) (A - B)) / (2 B) (A = Y[k], B = conj Y[B - k]) through the frame's LDS, the
//     inverse transform (the forward one on conjugates) and the store of its second half: B real samples.
// The translation unit is compiled without floating-point contraction; nothing is atomic and nothing depends on how the
// blocks were cut into tiles, launches, slabs or calls.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "hostio.h"
#include "rfft64.h"

using namespace frt;

namespace {

constexpr int kTile = 2;                          // J of X2: output blocks per tile
constexpr long long kMaxTaps = 1LL << 18, kMaxPartitions = 4096, kMaxSamples = 1LL << 40;
constexpr long long kMaxTableBytes = 1LL << 30;
constexpr long long kMaxWindows = 1LL << 24;      // windows per launch (the grid's x extent)

using rfft64::C;
using rfft64::Plan;                               // Plan<LOG2B>: N = B, IPB frame groups per workgroup

// where the samples of a row are: positions t0 .. first_in - 1 in the carried tail, first_in .. end - 1 in the call's rows,
// zeros elsewhere
struct Source {
    const void* x;
    int dtype;                                    // 0 float32, 1 float64
    long long row_stride, first_in, end;
    const double* tail;                           // [S][lt]
    long long t0, lt;
};

__device__ __forceinline__ double sample_at(const Source& src, long long s, long long pos) {
    if (pos < src.t0 || pos >= src.end) return 0.0;
    if (pos < src.first_in) return src.tail[s * src.lt + (pos - src.t0)];
    const long long at = s * src.row_stride + (pos - src.first_in);
    return src.dtype ? reinterpret_cast<const double*>(src.x)[at] : (double)reinterpret_cast<const float*>(src.x)[at];
}

struct WindowParams {
    Source src;
    long long w0, nw;                             // the windows w0 .. w0 + nw - 1 of every row
    long long shift;                              // window w starts at (w + shift) B: -1 for the streams, 0 for the taps
    int live;                                     // samples of a window that are read (2 B; B for the taps), even
    C* out;                                       // [S][nw][B + 1]
    const C *tw, *tw2;                            // exp(-2 pi i n / B), exp(-i pi n / B), n < B
};

template <int LOG2B>
__global__ __launch_bounds__(Plan<LOG2B>::BLOCK) void cv_window_kernel(const WindowParams p) {
    using R = Plan<LOG2B>;
    constexpr int B = R::N, TPF = R::TPF;
    constexpr bool WL = R::WAVE_LOCAL;
    extern __shared__ __attribute__((aligned(16))) char cv_smem[];
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = reinterpret_cast<C*>(cv_smem) + item * lds_padded_size(B);
    const long long s = blockIdx.y;
    const long long slot = (long long)blockIdx.x * R::IPB + item;
    const bool on = slot < p.nw;
    const long long start = (p.w0 + slot + p.shift) * (long long)B;

    C v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = C{0.0, 0.0};
    if (on && p.live == 2 * B && start >= p.src.first_in && start + 2 * B <= p.src.end) {      // the whole window in the call's rows
        const long long at = s * p.src.row_stride + (start - p.src.first_in) + 2 * i;
        if (p.src.dtype) {
            const double* xs = reinterpret_cast<const double*>(p.src.x) + at;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = C{xs[2 * j * TPF], xs[2 * j * TPF + 1]};
        } else {
            const float* xs = reinterpret_cast<const float*>(p.src.x) + at;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = C{(double)xs[2 * j * TPF], (double)xs[2 * j * TPF + 1]};
        }
    } else if (on) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = 2 * (i + j * TPF);
            if (m < p.live) v[j] = C{sample_at(p.src, s, start + m), sample_at(p.src, s, start + m + 1)};
        }
    }
    TwTable<double, LOG2B> tw{p.tw, 0};
    fft_pow2_forward<double, LOG2B, WL>(v, buf, i, tw);
    pass_sync<WL>();                                             // the last gathers of the transform are done
#pragma unroll
    for (int j = 0; j < 8; ++j) buf[lds_pad(i + j * TPF)] = v[j];
    pass_sync<WL>();
    if (!on) return;
    C* out = p.out + (s * p.nw + slot) * (long long)(B + 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = i + j * TPF;
        const C a = v[j], b = cconj(buf[lds_pad((B - k) & (B - 1))]);
        const C ze = {(a.x + b.x) * 0.5, (a.y + b.y) * 0.5};
        const C zo = mul_mi(C{(a.x - b.x) * 0.5, (a.y - b.y) * 0.5});
        const C t = cmul(p.tw2[k], zo);
        out[k] = ze + t;
        if (k == 0) out[B] = ze - t;
    }
}

// The inverse real 2 B-point transform of the half spectrum Y[0 .. B]: the thread holds Y[i + j TPF] in y[j] and thread 0
// Y[B] in ynyq.  On return y[j] = (r[2 n], -r[2 n + 1]) at n = i + j TPF, r the real sequence (scaled by 1 / (2 B)).
template <int LOG2B>
__device__ __forceinline__ void inverse_real(C (&y)[8], C ynyq, C* buf, int i, const C* tw, const C* tw2) {
    using R = Plan<LOG2B>;
    constexpr int B = R::N, TPF = R::TPF;
    constexpr bool WL = R::WAVE_LOCAL;
    const double scale = 0.5 / (double)B;                        // a power of two: exact wherever it is applied
    pass_sync<WL>();                                             // whoever used buf before is done with it
#pragma unroll
    for (int j = 0; j < 8; ++j) buf[lds_pad(i + j * TPF)] = y[j];
    pass_sync<WL>();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = i + j * TPF;
        const C a = y[j];
        const C b = cconj(k == 0 ? ynyq : buf[lds_pad((B - k) & (B - 1))]);
        const C sum = a + b, t = cmul(cconj(tw2[k]), a - b);
        const C z = {(sum.x - t.y) * scale, (sum.y + t.x) * scale};     // (sum + i t) / (2 B)
        y[j] = cconj(z);
    }
    pass_sync<WL>();                                             // the partners are read: the transform may scatter into buf
    TwTable<double, LOG2B> table{tw, 0};
    fft_pow2_forward<double, LOG2B, WL>(y, buf, i, table);
}

struct BlockParams {
    const C* spec;                                // [S][nw][B + 1]: the windows w0 .. w0 + nw - 1
    long long w0, nw;
    const C* H;                                   // [filters][P][B + 1]
    long long filter_stride;                      // entries between the filters of two streams (0: one filter for all)
    int P;
    long long ja, jb;                             // the output blocks of this launch
    void* y;
    int y_dtype;
    long long y_stride, out_begin, out_end;       // y[s][0] is output out_begin; outputs from out_end on are not stored
    const C *tw, *tw2;
};

__device__ __forceinline__ void cfma(C& acc, C x, C h) {
    acc.x = __builtin_fma(x.x, h.x, acc.x);
    acc.x = __builtin_fma(-x.y, h.y, acc.x);
    acc.y = __builtin_fma(x.x, h.y, acc.y);
    acc.y = __builtin_fma(x.y, h.x, acc.y);
}

template <int LOG2B>
__global__ __launch_bounds__(Plan<LOG2B>::BLOCK) void cv_block_kernel(const BlockParams p) {
    using R = Plan<LOG2B>;
    constexpr int B = R::N, TPF = R::TPF, J = kTile;
    extern __shared__ __attribute__((aligned(16))) char cv_smem[];
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = reinterpret_cast<C*>(cv_smem) + item * lds_padded_size(B);
    // Neighbouring tiles read the same window spectra, and workgroups are handed to the eight XCDs (one L2 each) in turn:
    // workgroup ids are remapped (a bijection) so that the ids that share an XCD cover one contiguous run of (stream, tiles).
    // A choice of speed alone: nothing depends on where a tile runs.
    const unsigned long long gx = gridDim.x, nwg = gx * gridDim.y, orig = blockIdx.y * gx + blockIdx.x;
    const unsigned long long q8 = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
    const unsigned long long wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
    const long long s = (long long)(wg / gx);
    const long long tile = (long long)(wg % gx) * R::IPB + item;
    const long long j0 = p.ja + tile * J;                        // may lie behind jb: such a frame group computes and stores nothing
    const bool nyq = i == 0;
    const C* spec = p.spec + s * p.nw * (long long)(B + 1);
    const C* H = p.H + s * p.filter_stride;
    const C zero = C{0.0, 0.0};

    // window w of the tile lives in ring slot (w - j0) mod J; rn: bin B, thread 0's
    C acc[J][8], an[J], ring[J][8], rn[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        an[jj] = zero;
        rn[jj] = zero;
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[jj][q] = ring[jj][q] = zero;
    }
#pragma unroll
    for (int jj = 1; jj < J; ++jj) {
        if (j0 + jj < p.jb) {
            const C* X = spec + (j0 + jj - p.w0) * (long long)(B + 1);
#pragma unroll
            for (int q = 0; q < 8; ++q) ring[jj][q] = X[i + q * TPF];
            if (nyq) rn[jj] = X[B];
        }
    }
    const bool live = j0 < p.jb;
    for (int p0 = 0; p0 < p.P; p0 += J) {
#pragma unroll
        for (int r = 0; r < J; ++r) {
            const int pp = p0 + r;
            if (pp < p.P) {
                const int fresh = (J - r) % J;                   // the slot of window j0 - pp
                C h[8], hn = zero;
                const C* Hp = H + (long long)pp * (B + 1);
#pragma unroll
                for (int q = 0; q < 8; ++q) h[q] = Hp[i + q * TPF];
                if (nyq) hn = Hp[B];
                if (live) {                                      // j0 - pp >= ja - P + 1 = w0
                    const C* X = spec + (j0 - pp - p.w0) * (long long)(B + 1);
#pragma unroll
                    for (int q = 0; q < 8; ++q) ring[fresh][q] = X[i + q * TPF];
                    if (nyq) rn[fresh] = X[B];
                }
#pragma unroll
                for (int jj = 0; jj < J; ++jj) {
                    const int slot = (jj - r + J) % J;           // window j0 + jj - pp
#pragma unroll
                    for (int q = 0; q < 8; ++q) cfma(acc[jj][q], ring[slot][q], h[q]);
                    cfma(an[jj], rn[slot], hn);
                }
            }
        }
    }

#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        inverse_real<LOG2B>(acc[jj], an[jj], buf, i, p.tw, p.tw2);
        const long long j = j0 + jj;
        if (j < p.jb) {
            const long long pos = j * (long long)B;              // of the block's first output
            const long long row = s * p.y_stride + (pos - p.out_begin);
#pragma unroll
            for (int q = 4; q < 8; ++q) {                        // the second half of the 2 B samples
                const int m = 2 * (i + q * TPF) - B;
                const double a = acc[jj][q].x, b = -acc[jj][q].y;
                if (p.y_dtype) {
                    double* y = reinterpret_cast<double*>(p.y) + row + m;
                    if (pos + m < p.out_end) y[0] = a;
                    if (pos + m + 1 < p.out_end) y[1] = b;
                } else {
                    float* y = reinterpret_cast<float*>(p.y) + row + m;
                    if (pos + m < p.out_end) y[0] = (float)a;
                    if (pos + m + 1 < p.out_end) y[1] = (float)b;
                }
            }
        }
    }
}

// the samples the next call needs: positions nt0 .. nt0 + nlt - 1 of every row
__global__ void cv_tail_kernel(const Source src, double* out, long long nt0, long long nlt) {
    const long long s = blockIdx.y, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nlt) out[s * nlt + i] = sample_at(src, s, nt0 + i);
}

struct IrfftParams {
    const double* spec;                           // [rows][B + 1][2]
    double* out;                                  // [rows][2 B]
    long long rows;
    const C *tw, *tw2;
};

template <int LOG2B>
__global__ __launch_bounds__(Plan<LOG2B>::BLOCK) void cv_irfft_kernel(const IrfftParams p) {
    using R = Plan<LOG2B>;
    constexpr int B = R::N, TPF = R::TPF;
    extern __shared__ __attribute__((aligned(16))) char cv_smem[];
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = reinterpret_cast<C*>(cv_smem) + item * lds_padded_size(B);
    const long long row = (long long)blockIdx.x * R::IPB + item;
    const bool on = row < p.rows;
    C y[8], yn = C{0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = C{0.0, 0.0};
    if (on) {
        const C* Y = reinterpret_cast<const C*>(p.spec) + row * (long long)(B + 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = Y[i + j * TPF];
        if (i == 0) {                                            // the imaginary parts of bins 0 and B do not count (numpy's irfft)
            y[0].y = 0.0;
            yn = C{Y[B].x, 0.0};
        }
    }
    inverse_real<LOG2B>(y, yn, buf, i, p.tw, p.tw2);
    if (on) {
        C* out = reinterpret_cast<C*>(p.out) + row * (long long)B;
#pragma unroll
        for (int j = 0; j < 8; ++j) out[i + j * TPF] = C{y[j].x, -y[j].y};
    }
}

typedef void (*WindowKernel)(const WindowParams);
typedef void (*BlockKernel)(const BlockParams);
typedef void (*IrfftKernel)(const IrfftParams);

}  // namespace

struct frt_convolve {
    int B = 0, P = 0, filters = 0;
    long long L = 0;
    WindowKernel window = nullptr;
    BlockKernel block = nullptr;
    rfft64::Launch launch{};
    hipStream_t stream = nullptr;
    DeviceBuffer H, tw, xin, sin, sout, yout, spec;
};

namespace {

long long tail_start(const frt_convolve* h, long long n) { return std::max(0LL, (n / h->B - h->P) * (long long)h->B); }

int launch_windows(const frt_convolve* h, const WindowParams& p, int S, hipStream_t stream) {
    const unsigned blocks = (unsigned)((p.nw + h->launch.ipb - 1) / h->launch.ipb);
    hipLaunchKernelGGL(h->window, dim3(blocks, S), dim3(h->launch.block), h->launch.lds, stream, p);
    FRT_HIP_CHECK(hipGetLastError());
    return FRT_OK;
}

}  // namespace

extern "C" int frt_convolve_create(frt_convolve** out, const double* taps, int64_t L, int filters, int block) {
    FRT_REQUIRE(out, "frt_convolve_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(taps, "frt_convolve_create: null taps");
    FRT_REQUIRE(L >= 1 && L <= kMaxTaps, "frt_convolve_create: L %lld taps (1 .. 2^18)", (long long)L);
    FRT_REQUIRE(filters >= 1 && filters <= 65535, "frt_convolve_create: %d filters (1 .. 65535)", filters);
    FRT_REQUIRE(block == 0 || (block >= 64 && block <= 4096 && (block & (block - 1)) == 0),
                "frt_convolve_create: block %d (0: the default, or a power of two in 64 .. 4096)", block);
    int B = block;
    if (!B) B = (int)std::min<long long>(4096, std::max<long long>(64, 1LL << rfft64::log2_of(L)));
    const long long P = (L + B - 1) / B;
    FRT_REQUIRE(P <= kMaxPartitions, "frt_convolve_create: %lld partitions of block %d for L %lld (at most 4096)", P, B, (long long)L);
    const long long table = (long long)filters * P * (B + 1) * (long long)sizeof(C);
    FRT_REQUIRE_CODE(table <= kMaxTableBytes, FRT_ERR_UNSUPPORTED,
                     "frt_convolve_create: the spectra of %d filters of %lld taps take %lld bytes: not supported (at most 2^30)", filters,
                     (long long)L, table);
    FRT_REQUIRE(!is_device_pointer(taps), "frt_convolve_create: the taps are a host array of %d x %lld doubles", filters, (long long)L);
    for (long long i = 0; i < (long long)filters * L; ++i)
        FRT_REQUIRE(std::isfinite(taps[i]), "frt_convolve_create: taps[%lld] is not finite", i);
    frt_convolve* h = new frt_convolve();
    h->B = B;
    h->P = (int)P;
    h->L = L;
    h->filters = filters;
    const bool found = rfft64::dispatch<6, 12>(rfft64::log2_of(B), [&](auto log2b) {
        h->window = cv_window_kernel<decltype(log2b)::value>;
        h->block = cv_block_kernel<decltype(log2b)::value>;
        h->launch = rfft64::launch_of<decltype(log2b)::value>();
    });
    if (!found) {
        delete h;
        set_last_error("frt_convolve_create: no kernel for block %d", B);
        return FRT_ERR_UNSUPPORTED;
    }
    int rc = upload(h->tw, rfft64::twiddles(B, true));
    if (!rc) rc = h->H.reserve((size_t)table);
    if (!rc) rc = h->xin.reserve((size_t)filters * L * sizeof(double));
    for (const void* k : {(const void*)h->window, (const void*)h->block})
        if (!rc) rc = rfft64::allow_lds(k, h->launch.lds, "frt_convolve_create", "block", B);
    if (!rc) {
        // H_p: the transform of h[p B .. p B + B), zeros behind it, by the kernel that transforms the streams' windows
        WindowParams p{};
        p.src = Source{h->xin.ptr, 1, L, 0, L, nullptr, 0, 0};
        p.w0 = 0;
        p.nw = P;
        p.shift = 0;
        p.live = B;
        p.out = h->H.as<C>();
        p.tw = h->tw.as<const C>();
        p.tw2 = p.tw + B;
        auto fill = [&]() -> int {
            FRT_HIP_CHECK(hipMemcpy(h->xin.ptr, taps, (size_t)filters * L * sizeof(double), hipMemcpyHostToDevice));
            int r = launch_windows(h, p, filters, nullptr);
            if (r) return r;
            FRT_HIP_CHECK(hipStreamSynchronize(nullptr));
            return FRT_OK;
        };
        rc = fill();
    }
    if (rc) {
        frt_convolve_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_convolve_destroy(frt_convolve* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->H, &h->tw, &h->xin, &h->sin, &h->sout, &h->yout, &h->spec}) b->release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_convolve_set_stream(frt_convolve* h, void* s) {
    FRT_REQUIRE(h, "frt_convolve_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int64_t frt_convolve_state_length(const frt_convolve* h, int streams, int64_t n_in) {
    FRT_REQUIRE(h, "frt_convolve_state_length: null handle");
    FRT_REQUIRE(streams >= 1 && n_in >= 0, "frt_convolve_state_length: %d streams after %lld samples", streams, (long long)n_in);
    return (int64_t)streams * (n_in - tail_start(h, n_in));
}

extern "C" int frt_convolve_run(frt_convolve* h, const void* x, int x_dtype, int streams, int64_t n, int64_t row_stride, const double* state_in,
                                double* state_out, int64_t first_in, int flush, int64_t scratch_bytes, void* y, int y_dtype, int64_t y_stride,
                                int64_t* n_out_ptr) {
    FRT_REQUIRE(h, "frt_convolve_run: null handle");
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "frt_convolve_run: x_dtype %d (0 float32, 1 float64)", x_dtype);
    FRT_REQUIRE(y_dtype == 0 || y_dtype == 1, "frt_convolve_run: y_dtype %d (0 float32, 1 float64)", y_dtype);
    FRT_REQUIRE(streams >= 1 && streams <= 65535, "frt_convolve_run: %d streams (1 .. 65535)", streams);
    FRT_REQUIRE(h->filters == 1 || h->filters == streams, "frt_convolve_run: %d filters for %d streams (one for all, or one per stream)",
                h->filters, streams);
    FRT_REQUIRE(n >= 0 && (n == 0 || x), "frt_convolve_run: bad input (n %lld)", (long long)n);
    FRT_REQUIRE(n == 0 || streams == 1 || row_stride >= n, "frt_convolve_run: bad stride (n %lld, row stride %lld)", (long long)n,
                (long long)row_stride);
    FRT_REQUIRE(first_in >= 0 && first_in + n <= kMaxSamples, "frt_convolve_run: bad position (%lld + %lld samples)", (long long)first_in,
                (long long)n);
    FRT_REQUIRE(state_in || first_in == 0, "frt_convolve_run: a stream continued without its state");
    FRT_REQUIRE(flush == 0 || flush == 1, "frt_convolve_run: flush %d (0 or 1)", flush);
    FRT_REQUIRE(!state_out || state_out != state_in, "frt_convolve_run: the state cannot be updated in place");
    FRT_REQUIRE(scratch_bytes >= 0, "frt_convolve_run: scratch_bytes %lld", (long long)scratch_bytes);
    const int S = streams, B = h->B, P = h->P;
    const long long n0 = first_in, n1 = first_in + n;
    const long long ja = n0 / B, out_begin = ja * B;
    const long long out_end = flush ? n1 + h->L - 1 : (n1 / B) * B;
    const long long jb = (out_end + B - 1) / B;
    const long long n_out = std::max(0LL, out_end - out_begin);
    FRT_REQUIRE(n_out == 0 || (y && (S == 1 || y_stride >= n_out)), "frt_convolve_run: bad output (%lld outputs, y stride %lld)", n_out,
                (long long)y_stride);
    if (n_out_ptr) *n_out_ptr = n_out;
    const long long t0 = tail_start(h, n0), lt = n0 - t0;
    const long long nt0 = tail_start(h, n1), nlt = flush ? 0 : n1 - nt0;
    FRT_REQUIRE(nlt == 0 || state_out, "frt_convolve_run: null state_out for %lld carried samples", nlt);
    const size_t xsize = x_dtype ? sizeof(double) : sizeof(float), ysize = y_dtype ? sizeof(double) : sizeof(float);
    int rc;
    Source src{x, x_dtype, row_stride, n0, n1, nullptr, t0, lt};          // behind n1: zeros (a flushed stream reads them)
    HostIO io(h->stream);
    if ((rc = io.in_rows(h->xin, src.x, src.row_stride, S, n, xsize))) return rc;
    if (state_in && lt > 0) {
        src.tail = state_in;
        if ((rc = io.in(h->sin, src.tail, (size_t)S * lt))) return rc;
    } else {
        src.t0 = n0;                                             // nothing carried
        src.lt = 0;
    }
    if ((rc = io.out(h->sout, state_out, (size_t)S * nlt))) return rc;
    if ((rc = io.out_rows(h->yout, y, y_stride, S, n_out, ysize))) return rc;

    // time slabs: the spectra of one launch (the windows of its blocks and the P - 1 before them, transformed again) stay
    // within scratch_bytes, at least one block per launch
    const long long win_bytes = (long long)S * (B + 1) * (long long)sizeof(C);
    const long long max_w = std::min(kMaxWindows, std::max<long long>(P, scratch_bytes / win_bytes));
    const long long per_slab = max_w - (P - 1);
    for (long long a = ja; a < jb; a += per_slab) {
        const long long b = std::min(jb, a + per_slab);
        WindowParams w{};
        w.src = src;
        w.w0 = a - P + 1;
        w.nw = b - w.w0;
        w.shift = -1;
        w.live = 2 * B;
        if ((rc = h->spec.reserve((size_t)(w.nw * win_bytes)))) return rc;
        w.out = h->spec.as<C>();
        w.tw = h->tw.as<const C>();
        w.tw2 = w.tw + B;
        if ((rc = launch_windows(h, w, S, h->stream))) return rc;
        BlockParams k{};
        k.spec = w.out;
        k.w0 = w.w0;
        k.nw = w.nw;
        k.H = h->H.as<const C>();
        k.filter_stride = h->filters == 1 ? 0 : (long long)P * (B + 1);
        k.P = P;
        k.ja = a;
        k.jb = b;
        k.y = y;
        k.y_dtype = y_dtype;
        k.y_stride = y_stride;
        k.out_begin = out_begin;
        k.out_end = out_end;
        k.tw = w.tw;
        k.tw2 = w.tw2;
        const long long tiles = (b - a + kTile - 1) / kTile;
        hipLaunchKernelGGL(h->block, dim3((unsigned)((tiles + h->launch.ipb - 1) / h->launch.ipb), S), dim3(h->launch.block), h->launch.lds,
                           h->stream, k);
        FRT_HIP_CHECK(hipGetLastError());
    }
    if (nlt > 0) {
        hipLaunchKernelGGL(cv_tail_kernel, dim3((unsigned)((nlt + 255) / 256), S), dim3(256), 0, h->stream, src, state_out, nt0, nlt);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return io.finish();
}

extern "C" int frt_irfft_rows(const double* spec, int64_t rows, int n, double* out, void* hip_stream) {
    FRT_REQUIRE(n >= 64 && n <= 8192 && (n & (n - 1)) == 0, "frt_irfft_rows: n %d (a power of two, 64 .. 8192)", n);
    FRT_REQUIRE(rows >= 0 && rows <= (1LL << 30), "frt_irfft_rows: %lld rows", (long long)rows);
    FRT_REQUIRE(rows == 0 || (spec && out), "frt_irfft_rows: null buffer");
    if (rows == 0) return FRT_OK;
    const int B = n / 2;
    IrfftKernel kernel = nullptr;
    rfft64::Launch launch{};
    const bool found = rfft64::dispatch<5, 12>(rfft64::log2_of(B), [&](auto log2b) {
        kernel = cv_irfft_kernel<decltype(log2b)::value>;
        launch = rfft64::launch_of<decltype(log2b)::value>();
    });
    if (!found) {
        set_last_error("frt_irfft_rows: no kernel for n %d", n);
        return FRT_ERR_UNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    const bool in_dev = is_device_pointer(spec), out_dev = is_device_pointer(out);
    const size_t tw_bytes = (size_t)2 * B * sizeof(C), in_bytes = (size_t)rows * (B + 1) * sizeof(C), out_bytes = (size_t)rows * n * sizeof(double);
    // a stateless call: one device block per call (twiddles | staged spectra | staged rows), allocated and freed here
    DeviceBuffer work;
    int rc = work.reserve(tw_bytes + (in_dev ? 0 : in_bytes) + (out_dev ? 0 : out_bytes));
    if (rc) return rc;
    auto run = [&]() -> int {
        const std::vector<C> tw = rfft64::twiddles(B, true);
        FRT_HIP_CHECK(hipMemcpyAsync(work.ptr, tw.data(), tw_bytes, hipMemcpyHostToDevice, stream));
        FRT_HIP_CHECK(hipStreamSynchronize(stream));             // tw leaves scope; pageable copies are staged, this keeps it plain
        char* at = work.as<char>() + tw_bytes;
        IrfftParams p{};
        p.spec = spec;
        if (!in_dev) {
            FRT_HIP_CHECK(hipMemcpyAsync(at, spec, in_bytes, hipMemcpyHostToDevice, stream));
            p.spec = reinterpret_cast<const double*>(at);
            at += in_bytes;
        }
        p.out = out_dev ? out : reinterpret_cast<double*>(at);
        p.rows = rows;
        p.tw = work.as<const C>();
        p.tw2 = p.tw + B;
        int r = rfft64::allow_lds((const void*)kernel, launch.lds, "frt_irfft_rows", "n", n);
        if (r) return r;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + launch.ipb - 1) / launch.ipb)), dim3(launch.block), launch.lds, stream, p);
        FRT_HIP_CHECK(hipGetLastError());
        if (!out_dev) FRT_HIP_CHECK(hipMemcpyAsync(out, p.out, out_bytes, hipMemcpyDeviceToHost, stream));
        FRT_HIP_CHECK(hipStreamSynchronize(stream));
        return FRT_OK;
    };
    rc = run();
    work.release();
    return rc;
}
