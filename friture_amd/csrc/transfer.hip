// transfer.hip — X1: Welch cross-spectra, transfer function and coherence of a reference row and a measured row
// (frt_transfer_*, TransferBatch; the definition: X1 in include/friture_hip.h).
//
// Two kernels per time slab.
//   tf_run_kernel<LOG2N>: one (pair, run of <= kRun frames) per frame group of N / 8 threads.  A frame is packed as
//     z = x w + i y w and transformed by ONE N-point complex transform (fft_core.h, float64, 8 points per thread: wave-local
//     up to N = 512, one workgroup of N / 8 threads above); Z goes once more through the frame's LDS so that the owner of
//     bin k = i + q N/8 (q < 4; thread 0 also owns N/2) reads Z[N - k]; X = (Z[k] + conj Z[N-k]) / 2, Y = -i (Z[k] - conj
//     Z[N-k]) / 2, which also holds at k = 0 and k = N/2 (Z[N - k] is Z[k] itself there).  |X|^2, |Y|^2 and conj(X) Y are
//     summed in registers in frame order, from the carried partial when the run was opened by an earlier launch, and leave
//     as one [bins][4] partial per run.  The complex spectra never reach memory.
//     Unpacked this way a row's spectrum carries the rounding of the louder row (about 1e-16 of it); a row whose windowed
//     frame is all zeros is found by a vote per frame and gets the spectrum 0 exactly, as its transform alone would.
//   tf_finish_kernel: per (pair, estimate, bin) the carried sum and the run partials in run order, the division by the frame
//     count, h1 and the coherence, and the sums of the estimate that stays open.
// Nothing is atomic and no sum depends on how the frames were cut into launches, slabs or calls.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "common.h"
#include "hostio.h"
#include "rfft64.h"

using namespace frt;

namespace {

constexpr int kRun = 16;                          // RUN of X1: frames per run
constexpr long long kRunning = 1LL << 60;         // frames per estimate of a running estimate (average = 0)
constexpr int kMaxDelay = 96000;
constexpr long long kMaxHop = 1LL << 30, kMaxSamples = 1LL << 40;
constexpr int kFinishThreads = 256;

// where the frames fa .. fb - 1 of a launch lie on the run grid of their estimates
struct Grid {
    long long K, rpe;                             // frames and runs per estimate
    long long fa, fb;
    long long ga;                                 // the run of frame fa
};

__host__ __device__ __forceinline__ long long run_of(const Grid& g, long long f) {
    const long long e = f / g.K;
    return e * g.rpe + (f - e * g.K) / kRun;
}

__host__ __device__ __forceinline__ void run_frames(const Grid& g, long long r, long long& start, long long& end) {
    const long long e = r / g.rpe;
    start = e * g.K + (r - e * g.rpe) * kRun;
    end = start + kRun < (e + 1) * g.K ? start + kRun : (e + 1) * g.K;
}

struct Params {
    const void* x;                                // the call's samples, positions first_in .. first_in + n - 1 of each row
    int dtype;                                    // 0 float32, 1 float64
    long long row_stride, pair_stride, first_in;
    const double *tail_x, *tail_y;                // carried samples [S][lx], [S][ly]: positions tx0 .. first_in - 1, ty0 .. first_in - 1
    long long tx0, ty0, lx, ly;
    long long a, b, hop;                          // frame f: x from a + f hop, y from b + f hop
    const double* window;                         // [N]
    const cpx<double>* tw;                        // exp(-2 pi i n / N)
    const double* open_in;                        // [S][bins][4]: the partial of the run an earlier launch left open
    double* part;                                 // [S][nruns][bins][4]
    long long nruns;
    Grid g;
};

__device__ __forceinline__ double sample_at(const Params& p, long long row, const double* tail, long long t0, long long pos) {
    if (pos < p.first_in) return tail[pos - t0];
    const long long at = row + (pos - p.first_in);
    return p.dtype ? reinterpret_cast<const double*>(p.x)[at] : (double)reinterpret_cast<const float*>(p.x)[at];
}

struct alignas(16) Sum4 {            // one bin of a partial or a state block: sxx, syy, Re sxy, Im sxy
    double x, y, z, w;
};

struct Sums {
    double xx, yy, re, im;
    // A = Z[k], B = conj Z[N - k] of the packed transform; a row whose windowed frame is all zeros has the spectrum 0 exactly
    // (unpacked, it would carry the other row's rounding)
    __device__ __forceinline__ void add(cpx<double> A, cpx<double> B, double scale, bool on, bool nzx, bool nzy) {
        cpx<double> X = {(A.x + B.x) * scale, (A.y + B.y) * scale};
        cpx<double> Y = {(A.y - B.y) * scale, (B.x - A.x) * scale};
        if (!nzx) X = cpx<double>{0.0, 0.0};
        if (!nzy) Y = cpx<double>{0.0, 0.0};
        if (on) {
            xx = xx + (X.x * X.x + X.y * X.y);
            yy = yy + (Y.x * Y.x + Y.y * Y.y);
            re = re + (X.x * Y.x + X.y * Y.y);
            im = im + (X.x * Y.y - X.y * Y.x);
        }
    }
};

template <int LOG2N>
__global__ __launch_bounds__(rfft64::Plan<LOG2N>::BLOCK) void tf_run_kernel(const Params p) {
    using R = rfft64::Plan<LOG2N>;                               // R::IPB runs per workgroup
    using C = cpx<double>;
    constexpr int N = R::N, TPF = R::TPF, BINS = N / 2 + 1;
    constexpr bool WL = R::WAVE_LOCAL;
    extern __shared__ __attribute__((aligned(16))) char tf_smem[];
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = reinterpret_cast<C*>(tf_smem) + item * lds_padded_size(N);
    const long long s = blockIdx.y;
    const long long w = (long long)blockIdx.x * R::IPB + item;

    long long f0 = 0, f1 = 0;
    bool carried = false;
    if (w < p.nruns) {
        long long start, end;
        run_frames(p.g, p.g.ga + w, start, end);
        carried = start < p.g.fa && p.open_in;
        f0 = start > p.g.fa ? start : p.g.fa;
        f1 = end < p.g.fb ? end : p.g.fb;
    }
    const int nfr = (int)(f1 - f0);
    int nmax = nfr;                                              // the trip count is uniform over the wavefront
    if constexpr (R::IPB > 1) {
#pragma unroll
        for (int off = TPF; off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off));
    }

    Sums acc[4], nyq;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = Sums{0.0, 0.0, 0.0, 0.0};
        if (carried) {
            const double* o = p.open_in + (s * BINS + (i + q * TPF)) * 4;
            acc[q] = Sums{o[0], o[1], o[2], o[3]};
        }
    }
    nyq = Sums{0.0, 0.0, 0.0, 0.0};
    if (carried && i == 0) {
        const double* o = p.open_in + (s * BINS + N / 2) * 4;
        nyq = Sums{o[0], o[1], o[2], o[3]};
    }

    const long long row_x = s * p.pair_stride, row_y = row_x + p.row_stride;
    const double* tail_x = p.tail_x ? p.tail_x + s * p.lx : nullptr;
    const double* tail_y = p.tail_y ? p.tail_y + s * p.ly : nullptr;
    const double scale = 0.5 / (double)N;                        // a power of two: exact wherever it is applied

    using TW = typename std::conditional<WL, TwRegs<double, LOG2N>, TwTable<double, LOG2N>>::type;
    TW tw;
    if constexpr (WL) tw.load(p.tw, i);

    for (int g = 0; g < nmax; ++g) {
        const bool on = g < nfr;
        if constexpr (!WL) {
            int zero = 0;
            asm volatile("s_mov_b32 %0, 0" : "=s"(zero));      // keeps the twiddle loads inside the loop
            tw.tw = p.tw;
            tw.zero = zero;
        }
        const long long px = p.a + (f0 + g) * p.hop, py = p.b + (f0 + g) * p.hop;
        C v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = C{0.0, 0.0};
        if (on && px >= p.first_in && py >= p.first_in) {        // the whole frame lies in the call's samples
            const long long ax = row_x + (px - p.first_in) + i, ay = row_y + (py - p.first_in) + i;
            if (p.dtype) {
                const double *xs = reinterpret_cast<const double*>(p.x) + ax, *ys = reinterpret_cast<const double*>(p.x) + ay;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = C{xs[j * TPF], ys[j * TPF]};
            } else {
                const float *xs = reinterpret_cast<const float*>(p.x) + ax, *ys = reinterpret_cast<const float*>(p.x) + ay;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = C{(double)xs[j * TPF], (double)ys[j * TPF]};
            }
        } else if (on) {                                         // part of it in the carried samples
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = i + j * TPF;
                v[j] = C{sample_at(p, row_x, tail_x, p.tx0, px + n), sample_at(p, row_y, tail_y, p.ty0, py + n)};
            }
        }
        bool fx = false, fy = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double wn = p.window[i + j * TPF];
            v[j] = C{v[j].x * wn, v[j].y * wn};
            fx = fx || v[j].x != 0.0;
            fy = fy || v[j].y != 0.0;
        }
        // is either row's windowed frame all zeros?  (the votes are also the barrier behind the previous frame's reads of buf)
        bool nzx, nzy;
        if constexpr (WL) {
            constexpr unsigned long long lanes = TPF >= 64 ? ~0ull : (1ull << (TPF & 63)) - 1ull;
            const unsigned long long mine = lanes << (item * TPF);
            nzx = (__ballot(fx) & mine) != 0;
            nzy = (__ballot(fy) & mine) != 0;
            pass_sync<true>();
        } else {
            nzx = __syncthreads_or(fx);
            nzy = __syncthreads_or(fy);
        }
        fft_pow2_forward<double, LOG2N, WL>(v, buf, i, tw);
        pass_sync<WL>();                                         // the last gathers of the transform are done
#pragma unroll
        for (int j = 0; j < 8; ++j) buf[lds_pad(i + j * TPF)] = v[j];
        pass_sync<WL>();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = i + q * TPF;
            acc[q].add(v[q], cconj(buf[lds_pad((N - k) & (N - 1))]), scale, on, nzx, nzy);
        }
        nyq.add(v[4], cconj(v[4]), scale, on, nzx, nzy);         // thread 0: Z[N/2]
    }

    if (w < p.nruns) {
        Sum4* out = reinterpret_cast<Sum4*>(p.part) + (s * p.nruns + w) * BINS;
#pragma unroll
        for (int q = 0; q < 4; ++q) out[i + q * TPF] = Sum4{acc[q].xx, acc[q].yy, acc[q].re, acc[q].im};
        if (i == 0) out[N / 2] = Sum4{nyq.xx, nyq.yy, nyq.re, nyq.im};
    }
}

struct Finish {
    const double* part;                           // [S][nruns][bins][4]
    long long nruns;
    const double *sum_in, *open_in;               // [S][bins][4] each; null: zeros
    double *sum_out, *open_out;
    Grid g;
    long long ea, n_est;                          // the estimate of frame fa; estimates this launch touches
    long long e_first, E;                         // the estimate in output slot 0; slots per pair
    int bins, emit_open;                          // emit_open: the estimate that stays open is written too (running estimate)
    double *sxy, *h1, *sxx, *syy, *coh;
};

__device__ __forceinline__ Sum4 plus(Sum4 a, Sum4 b) { return Sum4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
// member by member: a choice between two objects would put both in scratch memory
__device__ __forceinline__ Sum4 pick(bool c, Sum4 a, Sum4 b) { return Sum4{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w}; }

__global__ __launch_bounds__(kFinishThreads) void tf_finish_kernel(const Finish f) {
    const int k = blockIdx.y * kFinishThreads + threadIdx.x;
    if (k >= f.bins) return;
    const Grid g = Grid{f.g.K, f.g.rpe, f.g.fa, f.g.fb, f.g.ga};
    const long long s = blockIdx.z, e = f.ea + blockIdx.x;
    const long long es = e * g.K, ee = es + g.K;
    const long long lo = es > g.fa ? es : g.fa, hi = ee < g.fb ? ee : g.fb;
    const long long cell = s * f.bins + k;
    const Sum4 zero4 = Sum4{0.0, 0.0, 0.0, 0.0};
    Sum4 acc = zero4, open = zero4;
    bool has_open = false;
    if (es < g.fa && f.sum_in) acc = reinterpret_cast<const Sum4*>(f.sum_in)[cell];
    if (lo < hi) {
        const Sum4* part = reinterpret_cast<const Sum4*>(f.part) + (s * f.nruns) * f.bins + k;
        const long long r_lo = run_of(g, lo), r_hi = run_of(g, hi - 1);
        long long start, end;
        run_frames(g, r_hi, start, end);
        has_open = end > g.fb;                    // only the last run can be short of its end
        const long long n = r_hi - r_lo + (has_open ? 0 : 1);
        part += (r_lo - g.ga) * f.bins;
        long long j = 0;
        for (; j + 8 <= n; j += 8) {             // eight partials requested together, added in run order
            Sum4 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = part[(j + u) * f.bins];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = plus(acc, t[u]);
        }
        for (; j < n; ++j) acc = plus(acc, part[j * f.bins]);
        if (has_open) open = part[n * f.bins];
    } else if (f.open_in && (g.fb - es) % kRun != 0) {         // a launch without frames: the open run stays as it came
        open = reinterpret_cast<const Sum4*>(f.open_in)[cell];
        has_open = true;
    }
    const bool complete = hi == ee;
    if (complete || (f.emit_open && hi > es)) {
        const Sum4 total = pick(has_open, plus(acc, open), acc);
        const double count = (double)(hi - es);
        const double xx = total.x / count, yy = total.y / count, re = total.z / count, im = total.w / count;
        const long long at = (s * f.E + (e - f.e_first)) * f.bins + k;
        f.sxx[at] = xx;
        f.syy[at] = yy;
        f.sxy[2 * at] = re;
        f.sxy[2 * at + 1] = im;
        const double den = xx * yy;
        f.h1[2 * at] = xx != 0.0 ? re / xx : 0.0;
        f.h1[2 * at + 1] = xx != 0.0 ? im / xx : 0.0;
        f.coh[at] = den != 0.0 ? (re * re + im * im) / den : 0.0;
    }
    if (blockIdx.x == f.n_est - 1) {              // the estimate that stays open (zeros when the last one closed here)
        reinterpret_cast<Sum4*>(f.sum_out)[cell] = pick(complete, zero4, acc);
        reinterpret_cast<Sum4*>(f.open_out)[cell] = pick(complete, zero4, open);
    }
}

// the samples the next call needs: positions nx0 .. of row 0 and ny0 .. of row 1, up to the end of the call's samples
__global__ void tf_tail_kernel(const Params p, double* out_x, long long nx0, long long nlx, double* out_y, long long ny0, long long nly) {
    const long long s = blockIdx.y, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row_x = s * p.pair_stride, row_y = row_x + p.row_stride;
    if (i < nlx) out_x[s * nlx + i] = sample_at(p, row_x, p.tail_x ? p.tail_x + s * p.lx : nullptr, p.tx0, nx0 + i);
    if (i < nly) out_y[s * nly + i] = sample_at(p, row_y, p.tail_y ? p.tail_y + s * p.ly : nullptr, p.ty0, ny0 + i);
}

typedef void (*RunKernel)(const Params);

}  // namespace

struct frt_transfer {
    int N = 0, bins = 0, d = 0;
    long long hop = 0, K = 0, rpe = 0, a = 0, b = 0;
    RunKernel kernel = nullptr;
    rfft64::Launch launch{};
    hipStream_t stream = nullptr;
    DeviceBuffer window, tw, xin, sin, sout, out, part, sums[2];
};

namespace {

long long frames_after(const frt_transfer* h, long long n) {
    const long long usable = n - std::abs(h->d) - h->N;
    return usable < 0 ? 0 : usable / h->hop + 1;
}

// the first carried position of a row whose frames start at `lead` + f hop, after n samples and F frames
long long tail_start(const frt_transfer* h, long long lead, long long n, long long F) { return std::min(n, lead + F * h->hop); }

}  // namespace

extern "C" int frt_transfer_create(frt_transfer** out, int fft_size, int64_t hop, const double* window, int64_t average, int delay) {
    FRT_REQUIRE(out, "frt_transfer_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(fft_size >= 64 && (fft_size & (fft_size - 1)) == 0, "frt_transfer_create: fft_size %d (a power of two, 64 .. 8192)", fft_size);
    FRT_REQUIRE_CODE(fft_size <= 8192, FRT_ERR_UNSUPPORTED, "frt_transfer_create: fft_size %d is not supported (64 .. 8192)", fft_size);
    FRT_REQUIRE(hop >= 1 && hop <= kMaxHop, "frt_transfer_create: hop %lld (1 .. 2^30)", (long long)hop);
    FRT_REQUIRE(average >= 0 && average <= kMaxSamples, "frt_transfer_create: average %lld (frames per estimate, 0: one running estimate)",
                (long long)average);
    FRT_REQUIRE(delay >= -kMaxDelay && delay <= kMaxDelay, "frt_transfer_create: delay %d (-%d .. %d samples)", delay, kMaxDelay, kMaxDelay);
    FRT_REQUIRE(window && !is_device_pointer(window), "frt_transfer_create: the window is a host array of %d doubles", fft_size);
    for (int i = 0; i < fft_size; ++i) FRT_REQUIRE(std::isfinite(window[i]), "frt_transfer_create: window[%d] is not finite", i);
    frt_transfer* h = new frt_transfer();
    h->N = fft_size;
    h->bins = fft_size / 2 + 1;
    h->d = delay;
    h->hop = hop;
    h->K = average ? average : kRunning;
    h->rpe = (h->K + kRun - 1) / kRun;
    h->a = delay < 0 ? -delay : 0;
    h->b = delay > 0 ? delay : 0;
    const bool found = rfft64::dispatch<6, 13>(rfft64::log2_of(fft_size), [&](auto log2n) {
        h->kernel = tf_run_kernel<decltype(log2n)::value>;
        h->launch = rfft64::launch_of<decltype(log2n)::value>();
    });
    if (!found) {
        delete h;
        set_last_error("frt_transfer_create: no kernel for fft_size %d", fft_size);
        return FRT_ERR_UNSUPPORTED;
    }
    std::vector<double> w(window, window + fft_size);
    int rc = upload(h->window, w);
    if (!rc) rc = upload(h->tw, rfft64::twiddles(fft_size, false));
    if (!rc) rc = rfft64::allow_lds((const void*)h->kernel, h->launch.lds, "frt_transfer_create", "fft_size", fft_size);
    if (rc) {
        frt_transfer_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_transfer_destroy(frt_transfer* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->window, &h->tw, &h->xin, &h->sin, &h->sout, &h->out, &h->part, &h->sums[0], &h->sums[1]}) b->release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_transfer_set_stream(frt_transfer* h, void* s) {
    FRT_REQUIRE(h, "frt_transfer_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_transfer_run(frt_transfer* h, const void* x, int x_dtype, int pairs, int64_t n, int64_t row_stride, int64_t pair_stride,
                                const double* state_in, double* state_out, int64_t first_in, int64_t scratch_bytes, double* out,
                                int64_t* n_estimates_out) {
    FRT_REQUIRE(h, "frt_transfer_run: null handle");
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "frt_transfer_run: dtype %d (0 float32, 1 float64)", x_dtype);
    FRT_REQUIRE(pairs >= 1 && pairs <= 65535, "frt_transfer_run: %d pairs (1 .. 65535)", pairs);
    FRT_REQUIRE(n >= 0 && (n == 0 || x), "frt_transfer_run: bad input (n %lld)", (long long)n);
    FRT_REQUIRE(n == 0 || (row_stride >= n && pair_stride >= 0), "frt_transfer_run: bad strides (n %lld, row stride %lld, pair stride %lld)",
                (long long)n, (long long)row_stride, (long long)pair_stride);
    FRT_REQUIRE(first_in >= 0 && first_in + n <= kMaxSamples, "frt_transfer_run: bad position (%lld + %lld samples)", (long long)first_in,
                (long long)n);
    FRT_REQUIRE(state_in || first_in == 0, "frt_transfer_run: a stream continued without its state");
    FRT_REQUIRE(state_out, "frt_transfer_run: null state_out");
    FRT_REQUIRE(state_out != state_in, "frt_transfer_run: the state cannot be updated in place");
    FRT_REQUIRE(scratch_bytes >= 0, "frt_transfer_run: scratch_bytes %lld", (long long)scratch_bytes);
    const int S = pairs, bins = h->bins;
    const long long n0 = first_in, n1 = first_in + n;
    const long long F0 = frames_after(h, n0), F1 = frames_after(h, n1);
    const bool running = h->K == kRunning;
    const long long e_first = running ? 0 : F0 / h->K;
    const long long E = running ? (F1 > 0 ? 1 : 0) : F1 / h->K - e_first;
    FRT_REQUIRE(E == 0 || out, "frt_transfer_run: null out for %lld estimates", E);
    if (n_estimates_out) *n_estimates_out = E;
    const long long tx0 = tail_start(h, h->a, n0, F0), ty0 = tail_start(h, h->b, n0, F0), lx = n0 - tx0, ly = n0 - ty0;
    const long long nx0 = tail_start(h, h->a, n1, F1), ny0 = tail_start(h, h->b, n1, F1), nlx = n1 - nx0, nly = n1 - ny0;
    const size_t head = (size_t)S * bins * 4;                 // entries of one [S][bins][4] block
    const size_t in_len = 2 * head + (size_t)S * (lx + ly), out_state_len = 2 * head + (size_t)S * (nlx + nly);
    const size_t seb = (size_t)S * E * bins, out_len = 7 * seb;
    const size_t esize = x_dtype ? sizeof(double) : sizeof(float);
    int rc;
    Params p{};
    p.x = x;
    p.dtype = x_dtype;
    p.row_stride = row_stride;
    p.pair_stride = pair_stride;
    HostIO io(h->stream);
    if ((rc = io.in_rows(h->xin, p.x, p.row_stride, p.pair_stride, S, 2, n, esize))) return rc;      // pairs of rows; as one copy when evenly spaced
    const double* din = state_in;
    if ((rc = io.in(h->sin, din, in_len))) return rc;
    double *dso = state_out, *dout = out;
    if ((rc = io.out(h->sout, dso, out_state_len))) return rc;
    if ((rc = io.out(h->out, dout, out_len))) return rc;
    // the state: estimate sums [S][bins][4] | open run [S][bins][4] | row 0 from tx0 [S][lx] | row 1 from ty0 [S][ly]
    p.first_in = n0;
    p.tail_x = din ? din + 2 * head : nullptr;
    p.tail_y = din ? p.tail_x + (size_t)S * lx : nullptr;
    p.tx0 = tx0;
    p.ty0 = ty0;
    p.lx = lx;
    p.ly = ly;
    p.a = h->a;
    p.b = h->b;
    p.hop = h->hop;
    p.window = h->window.as<const double>();
    p.tw = h->tw.as<const cpx<double>>();
    // time slabs of whole runs (the first and the last may be part of one): their partials stay within scratch_bytes
    const size_t run_bytes = (size_t)S * bins * 4 * sizeof(double);
    const long long max_runs = std::max<long long>(1, std::min<long long>((long long)(scratch_bytes / run_bytes), 0x7fffffffLL));
    Grid g{h->K, h->rpe, F0, F0, 0};
    const double *sum_in = din, *open_in = din ? din + head : nullptr;
    int flip = 0;
    long long fa = F0;
    do {
        long long fb = fa;
        long long nruns = 0;
        if (fa < F1) {
            g.fa = fa;
            g.ga = run_of(g, fa);
            const long long g_last = std::min(run_of(g, F1 - 1), g.ga + max_runs - 1);
            long long start, end;
            run_frames(g, g_last, start, end);
            fb = std::min(end, F1);
            nruns = g_last - g.ga + 1;
        }
        g.fa = fa;
        g.fb = fb;
        g.ga = run_of(g, fa);
        const bool last = fb == F1;
        double *sum_out, *open_out;
        if (last) {
            sum_out = dso;
            open_out = dso + head;
        } else {
            if ((rc = h->sums[flip].reserve(2 * head * sizeof(double)))) return rc;
            sum_out = h->sums[flip].as<double>();
            open_out = sum_out + head;
        }
        p.g = g;
        p.nruns = nruns;
        p.open_in = open_in;
        if (nruns > 0) {
            if ((rc = h->part.reserve((size_t)nruns * run_bytes))) return rc;
            p.part = h->part.as<double>();
            const unsigned blocks = (unsigned)((nruns + h->launch.ipb - 1) / h->launch.ipb);
            hipLaunchKernelGGL(h->kernel, dim3(blocks, S), dim3(h->launch.block), h->launch.lds, h->stream, p);
            FRT_HIP_CHECK(hipGetLastError());
        }
        Finish f{};
        f.part = h->part.as<const double>();
        f.nruns = nruns;
        f.sum_in = sum_in;
        f.open_in = open_in;
        f.sum_out = sum_out;
        f.open_out = open_out;
        f.g = g;
        f.ea = fa / h->K;
        f.n_est = fb > fa ? (fb - 1) / h->K - f.ea + 1 : 1;
        f.e_first = e_first;
        f.E = E;
        f.bins = bins;
        f.emit_open = running && last;
        f.sxy = dout;
        f.h1 = dout + 2 * seb;
        f.sxx = dout + 4 * seb;
        f.syy = dout + 5 * seb;
        f.coh = dout + 6 * seb;
        FRT_REQUIRE(f.n_est <= 0x7fffffffLL, "frt_transfer_run: %lld estimates in one slab", f.n_est);
        hipLaunchKernelGGL(tf_finish_kernel, dim3((unsigned)f.n_est, (bins + kFinishThreads - 1) / kFinishThreads, S), dim3(kFinishThreads), 0,
                           h->stream, f);
        FRT_HIP_CHECK(hipGetLastError());
        sum_in = sum_out;
        open_in = open_out;
        flip ^= 1;
        fa = fb;
    } while (fa < F1);
    const long long most = std::max(nlx, nly);
    if (most > 0) {
        double* out_x = dso + 2 * head;
        hipLaunchKernelGGL(tf_tail_kernel, dim3((unsigned)((most + 255) / 256), S), dim3(256), 0, h->stream, p, out_x, nx0, nlx,
                           out_x + (size_t)S * nlx, ny0, nly);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return io.finish();
}
