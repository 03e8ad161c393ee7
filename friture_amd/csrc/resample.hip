// resample.hip — rational-ratio polyphase sample-rate converter (frt_resample_*; the definition: include/friture_hip.h).
//
// Output m sits at position q = m mod L of period P = m div L.  Its K taps are the inputs kb(m) .. kb(m) + K - 1,
// kb(m) = ceil((m M - C) / L) = kb(q) + P M, and its coefficients depend on q alone: the table is [K][L], column q holding
// h[C + q M - (kb(q) + j) L] for j = 0 .. K - 1 (0 where the index leaves [0, 2C]), so that the lanes of a wavefront, which
// own adjacent positions, load a contiguous row.  A thread owns one position of kPeriods periods, np periods apart: one
// coefficient load serves kPeriods fused multiply-adds, each with its own sample from LDS.  A workgroup stages the input span
// of its kPeriods * np periods (the periods' advance plus K - 1 samples) in LDS as float64, read once from memory, and
// stages it twice, the second copy one sample later: whatever the parity of a thread's first tap, one of the two copies has it
// 16-byte aligned, and two taps come with one ds_read_b128 (two ds_read_b64 merge into a ds_read2_b64 at half that rate).
// Every output is ONE chain acc = fma(c[j], x[kb + j], acc), j ascending from acc = 0: the order is fixed by the position in
// the period and by nothing else (not the tile, the grid, the stream count or where a call was cut).  L = 1 and M = 1 are the
// same code with one column, or with kb advancing by less than a sample per output.
#include "common.h"
#include "hostio.h"

#include <algorithm>
#include <numeric>

struct frt_resample {
    long long L = 0, M = 0, C = 0;
    int K = 0, S = 0;
    // launch shape, fixed at create: np periods side by side in a workgroup, `direct` when even one does not fit LDS
    int np = 1, threads = 64, span = 0, direct = 0;
    hipStream_t stream = nullptr;
    frt::DeviceBuffer coef, xin, tin, tout, yout;
};

namespace {

using namespace frt;

constexpr int kPeriods = 4;              // outputs per thread, L apart times np: they share every coefficient
constexpr int kTapBlock = 8;            // coefficient loads in flight ahead of their multiply-adds
constexpr int kCap = 8190;               // float64 slots of LDS per workgroup, both copies (just under 64 KB)
constexpr long long kMaxCoef = 1 << 20;  // L * K

__host__ __device__ inline long long floor_div(long long a, long long b) {      // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

struct Params {
    const void* x;           // [S][ld], this call's samples
    const double* tail;      // [S][K - 1], the samples before them (nullptr: zeros)
    void* y;                 // [S][ldy]
    const double* coef;      // [K][L]
    long long n, ld, ldy, first_in, first_out, n_out, M, C, Pbase;
    int L, K, np, span, copy, direct;       // copy: slots between the two LDS copies of the span (even)
};

// sample k of the stream (absolute index): this call's x, the carried tail behind it, zeros elsewhere
template <typename Tin>
__device__ inline double sample(const Params& p, const Tin* xs, const double* ts, long long k) {
    long long r = k - p.first_in;
    if (r >= 0) return r < p.n ? (double)xs[r] : 0.0;
    r += p.K - 1;
    return (r >= 0 && ts) ? ts[r] : 0.0;
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(512) void resample_kernel(Params p) {
    extern __shared__ __align__(16) double sx[];
    const int s = blockIdx.y, L = p.L, K = p.K, np = p.np;
    const Tin* xs = reinterpret_cast<const Tin*>(p.x) + (long long)s * p.ld;
    const double* ts = p.tail ? p.tail + (long long)s * (K - 1) : nullptr;
    Tout* ys = reinterpret_cast<Tout*>(p.y) + (long long)s * p.ldy;
    const long long P0 = p.Pbase + (long long)blockIdx.x * (kPeriods * np);
    const long long klo = ceil_div(P0 * L * p.M - p.C, L);                       // kb of the tile's first output
    if (!p.direct) {
        double* shifted = sx + p.copy;                                           // sample i at shifted[i + 1]
        for (int i = threadIdx.x; i < p.span; i += blockDim.x) sx[i] = shifted[i + 1] = sample(p, xs, ts, klo + i);
        __syncthreads();
    }
    const long long step = (long long)np * p.M;                                  // input distance of a thread's outputs
    for (int it = threadIdx.x; it < np * L; it += blockDim.x) {
        const int pt = it / L, q = it - pt * L;
        const long long P = P0 + pt;
        const long long kbq = ceil_div((long long)q * p.M - p.C, L), kb = kbq + P * p.M;
        const double* c = p.coef + q;
        double acc[kPeriods];
#pragma unroll
        for (int r = 0; r < kPeriods; ++r) acc[r] = 0.0;
        // the last tap of a column may fall off the prototype's end (its index below 0): the sum leaves it out
        const int Kq = (int)((p.C + (long long)q * p.M - kbq * L) / L) + 1;     // K or K - 1
        if (!p.direct) {
            const double* w[kPeriods];                                          // each 16-byte aligned, in one copy or the other
#pragma unroll
            for (int r = 0; r < kPeriods; ++r) {
                const int first = (int)(kb - klo) + r * (int)step;
                w[r] = (first & 1) ? sx + p.copy + first + 1 : sx + first;
            }
            int j = 0;
            for (; j + kTapBlock < K; j += kTapBlock) {                         // whole blocks within the K - 1 taps every column has
                double cj[kTapBlock];
#pragma unroll
                for (int u = 0; u < kTapBlock; ++u) cj[u] = c[(long long)(j + u) * L];
#pragma unroll
                for (int u = 0; u < kTapBlock; u += 2) {
                    double2 v[kPeriods];
#pragma unroll
                    for (int r = 0; r < kPeriods; ++r) v[r] = *reinterpret_cast<const double2*>(w[r] + j + u);
#pragma unroll
                    for (int r = 0; r < kPeriods; ++r) acc[r] = fma(cj[u], v[r].x, acc[r]);
#pragma unroll
                    for (int r = 0; r < kPeriods; ++r) acc[r] = fma(cj[u + 1], v[r].y, acc[r]);
                }
            }
            for (; j < Kq; ++j) {
                const double cj = c[(long long)j * L];
#pragma unroll
                for (int r = 0; r < kPeriods; ++r) acc[r] = fma(cj, w[r][j], acc[r]);
            }
        } else {
            for (int j = 0; j < Kq; ++j) {
                const double cj = c[(long long)j * L];
#pragma unroll
                for (int r = 0; r < kPeriods; ++r) acc[r] = fma(cj, sample(p, xs, ts, kb + r * step + j), acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kPeriods; ++r) {
            const long long rel = (P + (long long)r * np) * L + q - p.first_out;
            if (rel >= 0 && rel < p.n_out) ys[rel] = (Tout)acc[r];
        }
    }
}

// the last K - 1 samples of tail || x
template <typename Tin>
__global__ void resample_tail_kernel(Params p, double* out) {
    const int s = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.K - 1) return;
    const Tin* xs = reinterpret_cast<const Tin*>(p.x) + (long long)s * p.ld;
    const double* ts = p.tail ? p.tail + (long long)s * (p.K - 1) : nullptr;
    out[(long long)s * (p.K - 1) + i] = sample(p, xs, ts, p.first_in + p.n - (p.K - 1) + i);
}

template <typename Tin>
int launch(const frt_resample* h, const Params& p, int y_dtype, unsigned tiles, double* tail_out) {
    if (tiles) {
        const dim3 grid(tiles, h->S), block(h->threads);
        const size_t lds = p.direct ? 0 : (size_t)2 * p.copy * sizeof(double);
        if (y_dtype) hipLaunchKernelGGL((resample_kernel<Tin, double>), grid, block, lds, h->stream, p);
        else hipLaunchKernelGGL((resample_kernel<Tin, float>), grid, block, lds, h->stream, p);
        FRT_HIP_CHECK(hipGetLastError());
    }
    if (tail_out) {
        hipLaunchKernelGGL(resample_tail_kernel<Tin>, dim3((p.K - 1 + 255) / 256, h->S), dim3(256), 0, h->stream, p, tail_out);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return FRT_OK;
}

}  // namespace

extern "C" int frt_resample_create(frt_resample** out, int64_t L, int64_t M, int64_t C, const double* prototype, int streams) {
    FRT_REQUIRE(out, "frt_resample_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(L >= 1 && M >= 1 && L <= kMaxCoef && M <= ((int64_t)1 << 40), "frt_resample_create: L %lld, M %lld (positive integers)",
                (long long)L, (long long)M);
    FRT_REQUIRE(L != M, "frt_resample_create: L == M == %lld (rate_in == rate_out: nothing to resample)", (long long)L);
    FRT_REQUIRE(std::gcd((long long)L, (long long)M) == 1, "frt_resample_create: L %lld and M %lld share a factor", (long long)L, (long long)M);
    FRT_REQUIRE(C >= 1 && C <= ((int64_t)1 << 40), "frt_resample_create: C %lld (the prototype has 2C + 1 >= 3 points)", (long long)C);
    const long long K = (2 * C + L) / L;                                         // ceil((2C + 1) / L)
    FRT_REQUIRE(L * K <= kMaxCoef, "frt_resample_create: L * K = %lld * %lld coefficients (at most %lld)", (long long)L, K, kMaxCoef);
    FRT_REQUIRE(K >= 2, "frt_resample_create: %lld tap per output", K);
    FRT_REQUIRE(streams >= 1 && streams <= 65535, "frt_resample_create: %d streams", streams);
    FRT_REQUIRE(prototype && !is_device_pointer(prototype), "frt_resample_create: the prototype is a host array of 2C + 1 doubles");
    frt_resample* h = new frt_resample();
    h->L = L;
    h->M = M;
    h->C = C;
    h->K = (int)K;
    h->S = streams;
    std::vector<double> coef((size_t)(L * K));
    for (long long q = 0; q < L; ++q) {
        const long long i0 = C + q * M - ceil_div(q * M - C, L) * L;            // in (2C - L, 2C]
        for (long long j = 0; j < K; ++j) coef[(size_t)(j * L + q)] = i0 - j * L >= 0 ? prototype[i0 - j * L] : 0.0;
    }
    // np periods side by side: enough for 256 threads, as far as their span fits LDS
    const long long dq = ceil_div((L - 1) * M - C, L) - ceil_div(-C, L);        // kb(L - 1) - kb(0) <= M
    const long long want = (256 + L - 1) / L, room = (kCap / 2 - 2) - K - dq;       // per copy, the shifted one starts a slot later
    const long long fit = room < 0 ? 0 : (room / M + 1) / kPeriods;
    h->direct = fit < 1;
    h->np = (int)(h->direct ? want : std::min(want, fit));
    h->span = h->direct ? 0 : (int)((kPeriods * h->np - 1) * M + dq + K);
    const long long items = h->np * L, passes = (items + 511) / 512;
    h->threads = (int)(((items + passes - 1) / passes + 63) / 64 * 64);
    int rc = upload(h->coef, coef);
    if (rc) {
        frt_resample_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_resample_destroy(frt_resample* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->coef, &h->xin, &h->tin, &h->tout, &h->yout}) b->release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_resample_set_stream(frt_resample* h, void* s) {
    FRT_REQUIRE(h, "frt_resample_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_resample_run(frt_resample* h, const void* x, int x_dtype, int64_t n, int64_t ld, const double* tail_in, double* tail_out,
                                int64_t first_in, int64_t first_out, int64_t n_out, void* y, int y_dtype, int64_t ldy) {
    FRT_REQUIRE(h, "frt_resample_run: null handle");
    FRT_REQUIRE((x_dtype == 0 || x_dtype == 1) && (y_dtype == 0 || y_dtype == 1), "frt_resample_run: dtypes %d, %d (0 float32, 1 float64)",
                x_dtype, y_dtype);
    FRT_REQUIRE(n >= 0 && ld >= n && (n == 0 || x), "frt_resample_run: bad input (n %lld, ld %lld)", (long long)n, (long long)ld);
    FRT_REQUIRE(first_in >= 0 && first_out >= 0 && n_out >= 0 && first_in + n <= ((int64_t)1 << 40),
                "frt_resample_run: bad position (input %lld, output %lld, %lld outputs)", (long long)first_in, (long long)first_out, (long long)n_out);
    // nothing before the carried tail is needed, nothing after a flushed stream's last output exists
    const long long emitted = std::max<long long>(0, ceil_div(first_in * h->L - h->C, h->M)), most = ceil_div((first_in + n) * h->L, h->M);
    FRT_REQUIRE(first_out >= emitted && first_out + n_out <= most,
                "frt_resample_run: outputs %lld .. %lld of a stream of %lld + %lld inputs (%lld .. %lld can be formed)", (long long)first_out,
                (long long)(first_out + n_out), (long long)first_in, (long long)n, emitted, most);
    FRT_REQUIRE(n_out == 0 || (y && ldy >= n_out), "frt_resample_run: bad output (ldy %lld)", (long long)ldy);
    FRT_REQUIRE(tail_in || first_in == 0, "frt_resample_run: a stream continued without its tail");
    FRT_REQUIRE(!tail_out || tail_out != tail_in, "frt_resample_run: the tail cannot be updated in place");
    const int Kt = h->K - 1;
    const size_t esize = x_dtype ? sizeof(double) : sizeof(float), osize = y_dtype ? sizeof(double) : sizeof(float);
    const size_t tcount = (size_t)h->S * Kt;
    Params p{};
    p.x = x;
    p.tail = tail_in;
    p.y = y;
    p.coef = h->coef.as<const double>();
    p.n = n;
    p.ld = ld;
    p.ldy = ldy;
    p.first_in = first_in;
    p.first_out = first_out;
    p.n_out = n_out;
    p.M = h->M;
    p.C = h->C;
    p.L = (int)h->L;
    p.K = h->K;
    p.np = h->np;
    p.span = h->span;
    p.copy = (h->span + 2) / 2 * 2;
    p.direct = h->direct;
    HostIO io(h->stream);
    int rc;
    if ((rc = io.in_rows(h->xin, p.x, p.ld, h->S, n, esize))) return rc;
    if ((rc = io.in(h->tin, p.tail, tcount))) return rc;
    if ((rc = io.out(h->tout, tail_out, tcount))) return rc;
    if ((rc = io.out_rows(h->yout, p.y, p.ldy, h->S, n_out, osize))) return rc;
    long long tiles = 0;
    if (n_out > 0) {
        p.Pbase = first_out / h->L;
        const long long periods = (first_out + n_out - 1) / h->L - p.Pbase + 1;
        tiles = (periods + kPeriods * h->np - 1) / (kPeriods * h->np);
        FRT_REQUIRE(tiles <= 0x7fffffffLL, "frt_resample_run: %lld outputs in one call", (long long)n_out);
    }
    if ((rc = x_dtype ? launch<double>(h, p, y_dtype, (unsigned)tiles, tail_out) : launch<float>(h, p, y_dtype, (unsigned)tiles, tail_out))) return rc;
    return io.finish();
}
