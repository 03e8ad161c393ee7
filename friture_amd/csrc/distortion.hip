// distortion.hip — X9: the fundamental, the harmonics and the residual of tone recordings, frame by frame
// (frt_tone_*, ToneBatch; the definition: X9 in include/friture_hip.h).
//
// Two kernels per time slab.
//   tone_frame_kernel<LOG2>: one frame per frame group of N / 16 threads, N = 2^(LOG2 + 1).  The frame's N real samples are
//     windowed on load and packed as N / 2 complex points z[n] = x[2 n] w[2 n] + i x[2 n + 1] w[2 n + 1]; ONE N/2-point
//     complex transform (fft_core.h, float64, 8 points per thread: wave-local up to N = 1024, one workgroup above) and the
//     unpack of convolve.hip's window kernel give X[k]; Q[k] stays in the owner's registers and goes to the frame's LDS
//     buffer.  In the same kernel: the arg-max over the search range as a (value, lowest index) reduction; the lobe sums, lane
//     h - 1 of the group for order h, ascending k; the lobes are then zeroed in LDS (Q >= 0, so adding a zero is skipping the
//     bin) and the residual is each thread's bins in ascending k, a butterfly over the lanes of a wavefront and the wavefronts
//     in order.  3 + H doubles per frame leave the kernel: kappa, P1, R, P_2 .. P_H and a code (-1 dead, else 2 c1 + valid).
//   tone_fold_kernel: one wavefront per stream, lane q for quantity q: the frames of the slab in frame order from the carried
//     totals, and the record's values to the planes of the result.
// Nothing is atomic and no sum depends on how the frames were cut into launches, slabs or calls.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "hostio.h"
#include "rfft64.h"

using namespace frt;

namespace {

constexpr long long kMaxHop = 1LL << 30, kMaxSamples = 1LL << 40;
constexpr int kMaxLobe = 16, kMaxOrder = 32;

using rfft64::C;
using rfft64::Plan;                               // Plan<LOG2>: N / 2 complex points, IPB frame groups per workgroup

struct Params {
    const void* x;                                // the call's samples, positions first_in .. first_in + n - 1 of each row
    int dtype;                                    // 0 float32, 1 float64
    long long row_stride, first_in;
    const double* tail;                           // carried samples [S][lt]: positions t0 .. first_in - 1
    long long t0, lt;
    long long hop, fa, nf;                        // the frames fa .. fa + nf - 1 of every stream
    const C* window;                              // [N / 2]: (w[2 n], w[2 n + 1])
    const C *tw, *tw2;                            // exp(-2 pi i n / (N/2)), exp(-2 pi i n / N), n < N / 2
    const int* search;                            // [n_search][2]: klo, khi
    int n_search;
    int L, H, ka, kb;
    double qscale, gate;                          // 1 / (N sum w^2); a live frame with P1 < gate is gated
    double* rec;                                  // [S][nf][3 + H]
};

__device__ __forceinline__ double sample_at(const Params& p, long long s, long long pos) {
    if (pos < p.first_in) return p.tail[s * p.lt + (pos - p.t0)];
    const long long at = s * p.row_stride + (pos - p.first_in);
    return p.dtype ? reinterpret_cast<const double*>(p.x)[at] : (double)reinterpret_cast<const float*>(p.x)[at];
}

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

template <int LOG2>
__global__ __launch_bounds__(Plan<LOG2>::BLOCK) void tone_frame_kernel(const Params p) {
    using R = Plan<LOG2>;
    constexpr int M = R::N, TPF = R::TPF;                        // M = N / 2 complex points, TPF = N / 16 threads per frame
    constexpr bool WL = R::WAVE_LOCAL;
    constexpr int GL = TPF < 64 ? TPF : 64, NW = TPF / GL;       // a frame group's lanes in one wavefront; its wavefronts
    extern __shared__ __attribute__((aligned(16))) char tone_smem[];
    const int tid = threadIdx.x, item = tid / TPF, i = tid - item * TPF;
    C* buf = reinterpret_cast<C*>(tone_smem) + item * lds_padded_size(M);
    double* Q = reinterpret_cast<double*>(buf);                  // [M + 1], then the reductions' slots
    double* red = Q + M + 2;                                     // [NW][2] of the arg-max, [NW] of the residual behind it
    const long long s = blockIdx.y;
    const long long slot = (long long)blockIdx.x * R::IPB + item;
    const bool on = slot < p.nf;
    const long long start = (p.fa + slot) * p.hop;
    const int* range = p.search + (p.n_search > 1 ? 2 * s : 0);
    const int klo = range[0], khi = range[1];
    const int L = p.L, H = p.H, ka = p.ka, kb = p.kb;

    C v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = C{0.0, 0.0};
    if (on && start >= p.first_in) {                             // the whole frame lies in the call's samples
        const long long at = s * p.row_stride + (start - p.first_in) + 2 * i;
        if (p.dtype) {
            const double* xs = reinterpret_cast<const double*>(p.x) + at;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = C{xs[2 * j * TPF], xs[2 * j * TPF + 1]};
        } else {
            const float* xs = reinterpret_cast<const float*>(p.x) + at;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = C{(double)xs[2 * j * TPF], (double)xs[2 * j * TPF + 1]};
        }
    } else if (on) {                                             // part of it in the carried samples
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = 2 * (i + j * TPF);
            v[j] = C{sample_at(p, s, start + m), sample_at(p, s, start + m + 1)};
        }
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bad = bad || !is_finite(v[j].x) || !is_finite(v[j].y);
        const C wn = p.window[i + j * TPF];
        v[j] = C{v[j].x * wn.x, v[j].y * wn.y};
    }
    // does the frame hold a sample that is not finite?
    if constexpr (WL) {
        constexpr unsigned long long lanes = TPF >= 64 ? ~0ull : (1ull << (TPF & 63)) - 1ull;
        bad = (__ballot(bad) & (lanes << (item * TPF))) != 0;
    } else {
        bad = __syncthreads_or(bad);
    }

    TwTable<double, LOG2> tw{p.tw, 0};
    fft_pow2_forward<double, LOG2, WL>(v, buf, i, tw);
    pass_sync<WL>();                                             // the last gathers of the transform are done
#pragma unroll
    for (int j = 0; j < 8; ++j) buf[lds_pad(i + j * TPF)] = v[j];
    pass_sync<WL>();
    // X[k] = E[k] + exp(-2 pi i k / N) O[k], E and O the transforms of the even and of the odd samples; X[N/2] = E[0] - O[0]
    double q[8], qn = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = i + j * TPF;
        const C a = v[j], b = cconj(buf[lds_pad((M - k) & (M - 1))]);
        const C ze = {(a.x + b.x) * 0.5, (a.y + b.y) * 0.5};
        const C zo = mul_mi(C{(a.x - b.x) * 0.5, (a.y - b.y) * 0.5});
        const C t = cmul(p.tw2[k], zo);
        const C X = ze + t;
        q[j] = (X.x * X.x + X.y * X.y) * (k == 0 ? p.qscale : 2.0 * p.qscale);
        if (k == 0) {
            const C Y = ze - t;
            qn = (Y.x * Y.x + Y.y * Y.y) * p.qscale;
        }
    }
    pass_sync<WL>();                                             // everyone has read Z: the buffer becomes Q
#pragma unroll
    for (int j = 0; j < 8; ++j) Q[i + j * TPF] = q[j];
    if (i == 0) Q[M] = qn;

    // the arg-max over klo .. khi, lowest index on ties: the thread's bins ascend with j
    double best = -1.0;
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = i + j * TPF;
        if (k >= klo && k <= khi && q[j] > best) {
            best = q[j];
            bi = k;
        }
    }
#pragma unroll
    for (int off = 1; off < GL; off <<= 1) {
        const double ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    if constexpr (NW > 1) {
        if ((i & 63) == 0) {
            red[2 * (i >> 6)] = best;
            red[2 * (i >> 6) + 1] = (double)bi;
        }
    }
    pass_sync<WL>();                                             // Q and the wavefronts' winners are written
    if constexpr (NW > 1) {
        best = red[0];
        bi = (int)red[1];
        for (int w = 1; w < NW; ++w) {
            const double ov = red[2 * w];
            const int oi = (int)red[2 * w + 1];
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
    }
    const bool dead = bad || !(best > 0.0);
    const int c1 = dead ? klo : bi;                              // a dead frame goes through the same steps on a bin that exists

    // lane h - 1 takes order h; every one of them sums the fundamental's lobe for kappa
    double P1 = 0.0, kappa = 0.0, Ph = 0.0;
    int lo = 0, hi = -1;
    bool present = false;
    if (i < H) {
        double num = 0.0;
        for (int k = c1 - L; k <= c1 + L; ++k) {
            const double qv = Q[k];
            P1 = P1 + qv;
            num = num + (double)k * qv;
        }
        kappa = num / P1;
        if (i == 0) {
            lo = c1 - L;
            hi = c1 + L;
        } else if (!dead) {
            const double ch = rint((double)(i + 1) * kappa);
            const double cp = i == 1 ? (double)c1 : rint((double)i * kappa);
            if (cp >= 0.0 && ch + (double)L <= (double)kb) {     // present; false for a kappa that is not finite
                const int c = (int)ch, below = (int)cp + L + 1;
                present = true;
                lo = c - L > below ? c - L : below;
                hi = c + L;
                for (int k = lo; k <= hi; ++k) Ph = Ph + Q[k];
            }
        }
    }
    pass_sync<WL>();                                             // the lobe sums have read Q
    for (int k = lo; k <= hi; ++k) Q[k] = 0.0;                   // the lobes are disjoint
    pass_sync<WL>();

    double r = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = i + j * TPF;
        if (k >= ka && k <= kb) r = r + Q[k];
    }
    if (i == 0 && kb == M) r = r + Q[M];
#pragma unroll
    for (int off = 1; off < GL; off <<= 1) r = r + __shfl_xor(r, off);
    if constexpr (NW > 1) {
        double* rr = red + 2 * NW;
        if ((i & 63) == 0) rr[i >> 6] = r;
        __syncthreads();
        r = rr[0];
        for (int w = 1; w < NW; ++w) r = r + rr[w];
    }

    if (on && i < H) {
        const double nan = __builtin_nan("");
        double* rec = p.rec + (s * p.nf + slot) * (long long)(3 + H);
        if (i == 0) {
            const bool valid = !dead && !(P1 < p.gate);
            rec[0] = dead ? nan : kappa;
            rec[1] = dead ? nan : P1;
            rec[2] = dead ? nan : r;
            rec[2 + H] = dead ? -1.0 : (double)(2 * c1 + (valid ? 1 : 0));
        } else {
            rec[2 + i] = present ? Ph : nan;                     // an absent order, and every order of a dead frame
        }
    }
}

struct Fold {
    const double* rec;                            // [S][nf][3 + H]
    long long nf, f_at, F;                        // the slab's frames are the call's frames f_at .. f_at + nf - 1 of F
    const double* tot_in;                         // [S][3 + H]: the sums of kappa, P1, R, P_2 .. P_H, then n_valid; null: zeros
    double* tot_out;
    int H;
    double *kappa, *fund, *resid, *harm, *code;   // the planes of the result
};

__global__ __launch_bounds__(64) void tone_fold_kernel(const Fold f) {
    const int q = threadIdx.x, RW = 3 + f.H;
    if (q >= RW) return;
    const long long s = blockIdx.x;
    const bool counts = q == RW - 1;
    double acc = f.tot_in ? f.tot_in[s * RW + q] : 0.0;
    const double* rec = f.rec + s * f.nf * RW;
    const long long at = s * f.F + f.f_at;
    double* plane;
    long long step = 1;
    if (q == 0) plane = f.kappa + at;
    else if (q == 1) plane = f.fund + at;
    else if (q == 2) plane = f.resid + at;
    else if (counts) plane = f.code + at;
    else {
        plane = f.harm + at * (f.H - 1) + (q - 3);
        step = f.H - 1;
    }
    auto take = [&](double v, double code) {
        const bool valid = code >= 0.0 && ((long long)code & 1);
        const double add = counts ? 1.0 : (v != v ? 0.0 : v);     // an absent order adds 0
        if (valid) acc = acc + add;
    };
    long long j = 0;
    for (; j + 8 <= f.nf; j += 8) {                              // eight records requested together, added in frame order
        double v[8], c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            v[u] = rec[(j + u) * RW + q];
            c[u] = rec[(j + u) * RW + RW - 1];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            plane[(j + u) * step] = v[u];
            take(v[u], c[u]);
        }
    }
    for (; j < f.nf; ++j) {
        const double v = rec[j * RW + q], c = rec[j * RW + RW - 1];
        plane[j * step] = v;
        take(v, c);
    }
    f.tot_out[s * RW + q] = acc;
}

// the samples the next call needs: positions nt0 .. of every row, up to the end of the call's samples
__global__ void tone_tail_kernel(const Params p, double* out, long long nt0, long long nlt) {
    const long long s = blockIdx.y, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nlt) out[s * nlt + i] = sample_at(p, s, nt0 + i);
}

typedef void (*FrameKernel)(const Params);

}  // namespace

struct frt_tone {
    int N = 0, L = 0, H = 0, ka = 0, kb = 0, n_search = 0;
    long long hop = 0;
    double qscale = 0.0, gate = 0.0;
    FrameKernel kernel = nullptr;
    rfft64::Launch launch{};
    hipStream_t stream = nullptr;
    DeviceBuffer window, tw, search, xin, sin, sout, out, rec, tot[2];
};

namespace {

long long frames_after(const frt_tone* h, long long n) { return n < h->N ? 0 : (n - h->N) / h->hop + 1; }

}  // namespace

extern "C" int frt_tone_create(frt_tone** out, int fft_size, int64_t hop, const double* window, int lobe, int harmonics, int ka, int kb,
                               const int* klo, const int* khi, int n_search, double gate) {
    FRT_REQUIRE(out, "frt_tone_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(fft_size >= 512 && fft_size <= 16384 && (fft_size & (fft_size - 1)) == 0,
                "frt_tone_create: fft_size %d (a power of two, 512 .. 16384)", fft_size);
    FRT_REQUIRE(hop >= 1 && hop <= kMaxHop, "frt_tone_create: hop %lld (1 .. 2^30)", (long long)hop);
    FRT_REQUIRE(lobe >= 1 && lobe <= kMaxLobe, "frt_tone_create: lobe %d (1 .. %d bins)", lobe, kMaxLobe);
    FRT_REQUIRE(harmonics >= 2 && harmonics <= kMaxOrder, "frt_tone_create: harmonics %d (2 .. %d)", harmonics, kMaxOrder);
    FRT_REQUIRE(ka >= lobe + 1 && kb <= fft_size / 2 && ka <= kb, "frt_tone_create: band ka %d .. kb %d (lobe + 1 .. fft_size / 2)", ka, kb);
    FRT_REQUIRE(n_search >= 1 && n_search <= 65535 && klo && khi, "frt_tone_create: n_search %d ranges (1 .. 65535, klo and khi given)", n_search);
    for (int s = 0; s < n_search; ++s)
        FRT_REQUIRE(klo[s] >= ka + lobe && khi[s] <= kb - lobe && klo[s] <= khi[s],
                    "frt_tone_create: search range %d: klo %d .. khi %d is empty or outside ka + lobe %d .. kb - lobe %d", s, klo[s], khi[s],
                    ka + lobe, kb - lobe);
    FRT_REQUIRE(gate >= 0.0 && std::isfinite(gate), "frt_tone_create: gate %g (a power >= 0)", gate);
    FRT_REQUIRE(window && !is_device_pointer(window), "frt_tone_create: the window is a host array of %d doubles", fft_size);
    double sum2 = 0.0;
    for (int i = 0; i < fft_size; ++i) {
        FRT_REQUIRE(std::isfinite(window[i]), "frt_tone_create: window[%d] is not finite", i);
        sum2 = sum2 + window[i] * window[i];
    }
    FRT_REQUIRE(sum2 > 0.0 && std::isfinite(sum2), "frt_tone_create: the window is all zero");
    frt_tone* h = new frt_tone();
    h->N = fft_size;
    h->hop = hop;
    h->L = lobe;
    h->H = harmonics;
    h->ka = ka;
    h->kb = kb;
    h->n_search = n_search;
    h->gate = gate;
    h->qscale = 1.0 / ((double)fft_size * sum2);
    const bool found = rfft64::dispatch<8, 13>(rfft64::log2_of(fft_size) - 1, [&](auto log2m) {
        h->kernel = tone_frame_kernel<decltype(log2m)::value>;
        h->launch = rfft64::launch_of<decltype(log2m)::value>();
    });
    if (!found) {
        delete h;
        set_last_error("frt_tone_create: no kernel for fft_size %d", fft_size);
        return FRT_ERR_UNSUPPORTED;
    }
    std::vector<double> w(window, window + fft_size);
    std::vector<int> search((size_t)2 * n_search);
    for (int s = 0; s < n_search; ++s) {
        search[2 * s] = klo[s];
        search[2 * s + 1] = khi[s];
    }
    int rc = upload(h->window, w);
    if (!rc) rc = upload(h->tw, rfft64::twiddles(fft_size / 2, true));
    if (!rc) rc = upload(h->search, search);
    if (!rc) rc = rfft64::allow_lds((const void*)h->kernel, h->launch.lds, "frt_tone_create", "fft_size", fft_size);
    if (rc) {
        frt_tone_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_tone_destroy(frt_tone* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->window, &h->tw, &h->search, &h->xin, &h->sin, &h->sout, &h->out, &h->rec, &h->tot[0], &h->tot[1]}) b->release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_tone_set_stream(frt_tone* h, void* s) {
    FRT_REQUIRE(h, "frt_tone_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_tone_run(frt_tone* h, const void* x, int x_dtype, int streams, int64_t n, int64_t row_stride, const double* state_in,
                            double* state_out, int64_t first_in, int64_t scratch_bytes, double* out, int64_t* n_frames_out) {
    FRT_REQUIRE(h, "frt_tone_run: null handle");
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "frt_tone_run: dtype %d (0 float32, 1 float64)", x_dtype);
    FRT_REQUIRE(streams >= 1 && streams <= 65535, "frt_tone_run: %d streams (1 .. 65535)", streams);
    FRT_REQUIRE(h->n_search == 1 || h->n_search == streams, "frt_tone_run: %d streams for %d search ranges", streams, h->n_search);
    FRT_REQUIRE(n >= 0 && (n == 0 || x), "frt_tone_run: bad input (n %lld)", (long long)n);
    FRT_REQUIRE(n == 0 || row_stride >= n, "frt_tone_run: bad stride (n %lld, row stride %lld)", (long long)n, (long long)row_stride);
    FRT_REQUIRE(first_in >= 0 && first_in + n <= kMaxSamples, "frt_tone_run: bad position (%lld + %lld samples)", (long long)first_in,
                (long long)n);
    FRT_REQUIRE(state_in || first_in == 0, "frt_tone_run: a stream continued without its state");
    FRT_REQUIRE(state_out, "frt_tone_run: null state_out");
    FRT_REQUIRE(state_out != state_in, "frt_tone_run: the state cannot be updated in place");
    FRT_REQUIRE(scratch_bytes >= 0, "frt_tone_run: scratch_bytes %lld", (long long)scratch_bytes);
    const int S = streams, H = h->H, RW = 3 + H;
    const long long n0 = first_in, n1 = first_in + n;
    const long long F0 = frames_after(h, n0), F1 = frames_after(h, n1), F = F1 - F0;
    FRT_REQUIRE(F == 0 || out, "frt_tone_run: null out for %lld frames", F);
    if (n_frames_out) *n_frames_out = F;
    const long long t0 = std::min(n0, F0 * h->hop), lt = n0 - t0;
    const long long nt0 = std::min(n1, F1 * h->hop), nlt = n1 - nt0;
    const size_t head = (size_t)S * RW;
    const size_t in_len = head + (size_t)S * lt, out_state_len = head + (size_t)S * nlt;
    const size_t sf = (size_t)S * F, out_len = sf * (size_t)(3 + H);
    const size_t esize = x_dtype ? sizeof(double) : sizeof(float);
    int rc;
    Params p{};
    p.x = x;
    p.dtype = x_dtype;
    p.row_stride = row_stride;
    HostIO io(h->stream);
    if ((rc = io.in_rows(h->xin, p.x, p.row_stride, S, n, esize))) return rc;
    const double* din = state_in;
    if ((rc = io.in(h->sin, din, in_len))) return rc;
    double *dso = state_out, *dout = out;
    if ((rc = io.out(h->sout, dso, out_state_len))) return rc;
    if ((rc = io.out(h->out, dout, out_len))) return rc;
    // the state: totals [S][3 + H] | the row from t0 on [S][lt]
    p.first_in = n0;
    p.tail = din ? din + head : nullptr;
    p.t0 = t0;
    p.lt = lt;
    p.hop = h->hop;
    p.window = h->window.as<const C>();
    p.tw = h->tw.as<const C>();
    p.tw2 = p.tw + h->N / 2;
    p.search = h->search.as<const int>();
    p.n_search = h->n_search;
    p.L = h->L;
    p.H = H;
    p.ka = h->ka;
    p.kb = h->kb;
    p.qscale = h->qscale;
    p.gate = h->gate;
    // time slabs of whole frame groups: their records stay within scratch_bytes
    const size_t frame_bytes = (size_t)S * RW * sizeof(double);
    const long long max_frames = std::max<long long>(1, std::min<long long>((long long)(scratch_bytes / frame_bytes), 1LL << 24));
    const double* tot_in = din;
    int flip = 0;
    long long fa = F0;
    do {
        const long long fb = std::min(F1, fa + max_frames), nf = fb - fa;
        const bool last = fb == F1;
        double* tot_out = dso;
        if (!last) {
            if ((rc = h->tot[flip].reserve(head * sizeof(double)))) return rc;
            tot_out = h->tot[flip].as<double>();
        }
        if (nf > 0) {
            if ((rc = h->rec.reserve((size_t)nf * frame_bytes))) return rc;
            p.rec = h->rec.as<double>();
            p.fa = fa;
            p.nf = nf;
            const unsigned blocks = (unsigned)((nf + h->launch.ipb - 1) / h->launch.ipb);
            hipLaunchKernelGGL(h->kernel, dim3(blocks, S), dim3(h->launch.block), h->launch.lds, h->stream, p);
            FRT_HIP_CHECK(hipGetLastError());
        }
        Fold f{};
        f.rec = h->rec.as<const double>();
        f.nf = nf;
        f.f_at = fa - F0;
        f.F = F;
        f.tot_in = tot_in;
        f.tot_out = tot_out;
        f.H = H;
        f.kappa = dout;
        f.fund = dout + sf;
        f.resid = dout + 2 * sf;
        f.harm = dout + 3 * sf;
        f.code = dout + (size_t)(2 + H) * sf;
        hipLaunchKernelGGL(tone_fold_kernel, dim3(S), dim3(64), 0, h->stream, f);
        FRT_HIP_CHECK(hipGetLastError());
        tot_in = tot_out;
        flip ^= 1;
        fa = fb;
    } while (fa < F1);
    if (nlt > 0) {
        hipLaunchKernelGGL(tone_tail_kernel, dim3((unsigned)((nlt + 255) / 256), S), dim3(256), 0, h->stream, p, dso + head, nt0, nlt);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return io.finish();
}
