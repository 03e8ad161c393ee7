// levels.hip — the level meters and the long-time level history, for gfx950.  float64 arithmetic; built with
// -ffp-contract=off so that every value is produced by the reference's IEEE operations in the reference's order.
//
// Reference semantics (per channel; the reference widgets handle one or two channels):
//   Levels_Widget.handle_new_data: peak hold/decay, exp_smoothed_value of y^2, 10 log10 / 20 log10, dB_to_IEC,
//   BallisticPeak                  friture/levels.py:47-77,85-124, iec.py, ballistic_peak.py:21-66,
//                                  signal/exp_smoothing.py:40-56
//   LongLevelWidget.handle_new_data: per block of 2^Ndec samples y^2 -> Ndec x (11-tap gauss(11, 2) FIR, [::2]) ->
//   41-tap gauss(41, 8) FIR -> 10 log10(max(level, 1e-150))      friture/longlevels.py:31-91,138-171,195-209
//
// The decimation FIRs have a = [1, 0, ...] and non-negative taps and inputs, so the DF2T loop of
// signal/lfilter.py:131-139 returns the same bits as the left-to-right tap sum over raw inputs
//   acc = x[n-10] b10; acc = acc + x[n-9] b9; ...; y = acc + x[n] b0
// (every "- yk a[k]" subtracts +0 and the partial sums of z are the same additions in the same order).  Every output is
// therefore computed independently (time-parallel) and the carried state is the last 10 (40) INPUTS of each stage.
//
// Kernels of one call (all on the object's stream):
//   levels_front_kernel  one read of the input: per chunk max|x| (NaN when a sample is, as numpy's max) and the RMS dot
//                        (exp_smooth_rows_kernel's products and order: 64 strided lanes, then a __shfl_down tree); the
//                        squaring and the first S decimation stages in LDS, with a halo of 10 (2^S - 1) samples; the
//                        stage-S signal to HBM
//   levels_tail_kernel   stages S .. Ndec-1 on the stage-S signal, the same way (one value per block)
//   levels_fir_kernel    the 41-tap FIR and the dB per block, the history ring, and the carried state of the call
//   levels_scan_kernel   one lane per channel walks the chunks in order: peak hold/decay, the RMS recurrence, both dB
//                        values, dB_to_IEC and BallisticPeak (sequential in the reference, kept sequential here)
#include <algorithm>
#include <cmath>

#include "common.h"
#include "hostio.h"

namespace frt {
namespace {

constexpr int kMaxNdec = 13;                      // the settings allow rt 1 .. 20 s: Ndec 8 .. 13
constexpr int kMeta = 8;                          // old_max, old_rms, peak_iec, hold counter, decay factor, (3 unused)
constexpr int kTailOff = kMeta;                   // last 10 inputs of stage s at kTailOff + 10 s
constexpr int kFirOff = kTailOff + 10 * kMaxNdec; // last 40 inputs of the 41-tap FIR
constexpr int kPendOff = kFirOff + 40;            // squared samples: the 2^13 before old_index, then the unconsumed ones
constexpr int kHist = 1 << kMaxNdec;
constexpr int kPendCap = 2 * kHist;
constexpr int kChan = kPendOff + kPendCap;        // doubles of carried state per channel
constexpr int kHeader = 2;                        // get/set_state: pending count, Ndec, then C x kChan
constexpr int kFrontJ = 64;                       // stage-S outputs per front workgroup
constexpr int kFrontS = 5;                        // stages done in the front
constexpr int kThreads = 256;
constexpr int kFields = FRT_LEVELS_METER_FIELDS;

struct LvParams {
    const void* x;              // input rows (device), x[c * ld + i]
    long long ld, n;            // row stride, samples per channel in this call
    int dtype;                  // 0 float32, 1 float64
    int nch;                    // channels processed by this call
    int C;                      // channels of the object
    int ndec, S;                // stages, of which the front does S
    int square;                 // 1: the long-level path squares its input (levels), 0: raw (Subsampler)
    int decim;                  // 1: the decimation stages run in this call
    int fir;                    // 1: the 41-tap FIR, dB and ring run (levels mode)
    int meters;                 // 1: the meter scan runs in this call
    long long r;                // squared samples carried from earlier calls, in front of x (levels mode)
    long long skip;             // carried samples in front of the first block (kHist - 2^Ndec; 0 for the Subsampler)
    long long E[kMaxNdec + 1];  // samples of stage input s consumed in this call (E[s+1] = ceil(E[s] / 2))
    long long ntile_front, ntile_tail;
    int Bt;                     // blocks per tail workgroup
    int capA, capB;             // LDS doubles of the two level buffers (front: kFrontS, tail: its own L)
    // meters
    long long chunk, nchunks;
    int K;                      // chunks per front workgroup
    int nk;                     // taps of the smoothing kernel
    const double* kern;         // [nk]
    // state (double-buffered: read old, write new)
    const double* old_state;    // [C][kChan]
    double* new_state;
    double* us;                 // stage-S signal [nch][E[S]]
    double* ud;                 // stage-Ndec signal [nch][E[ndec]] (== us when S == ndec)
    double* mt;                 // per chunk {max|x|, dot} [nch][nchunks][2]
    double* long_out;           // [nch][E[ndec]][2] {level, dB}
    double* ring;               // [C][H]
    long long H, ring_head;
    double* meters_out;         // [nch][nchunks][kFields]
    double alpha, one_m_alpha2, peak_rate, decay_full, decay_last;
    double b11[11];
    double b41[41];
};

__device__ inline double load_x(const LvParams& p, int c, long long i) {
    if (p.dtype == 0) return (double)(static_cast<const float*>(p.x))[(size_t)c * p.ld + i];
    return (static_cast<const double*>(p.x))[(size_t)c * p.ld + i];
}

// np.abs(y).max() (levels.py:97): NaN when either is NaN (fmax would drop it), so that a chunk holding a NaN fails
// `value_max > old_max (1 - alpha2)` and the peak decays, whatever else the chunk holds
__device__ inline double nan_max(double m, double a) { return (a > m || a != a) ? a : m; }

// sample j of the carried squared samples followed by this call's input
__device__ inline double carried_or_input(const LvParams& p, const double* oldc, int c, long long j) {
    if (j < p.r) return oldc[kPendOff + j];
    const double v = load_x(p, c, j - p.r);
    return p.square ? v * v : v;
}

// sample i >= 0 of the stage-0 input
__device__ inline double stage0_input(const LvParams& p, const double* oldc, int c, long long i) {
    return carried_or_input(p, oldc, c, i + p.skip);
}

// One workgroup computes outputs [o0, o1) of relative level L from relative level 0 (absolute level base), all levels in
// LDS (even levels in A, odd in B).  Level l covers [lo[l], hi[l]); indices -10 .. -1 are the carried inputs of that stage.
// Level l's owned part — (2^(L-l) (o0 - 1), hi[l]) — partitions the indices among the tiles; an owner writes the entries
// of its level that become the carried inputs of the next call.
template <class Src>
__device__ void run_stages(const LvParams& p, int c, int base, int L, long long o0, long long o1, bool last, double* A, double* B,
                           Src src, double* out) {
    long long lo[kMaxNdec + 1], hi[kMaxNdec + 1];
    lo[L] = o0;
    hi[L] = o1;
    for (int l = L; l > 0; --l) {
        lo[l - 1] = max(2 * lo[l] - 10, -10LL);
        hi[l - 1] = last ? p.E[base + l - 1] : 2 * hi[l] - 1;
    }
    const double* oldc = p.old_state + (size_t)c * kChan;
    double* newc = p.new_state + (size_t)c * kChan;
    const int tid = threadIdx.x;
    for (int l = 0; l <= L; ++l) {
        double* cur = (l & 1) ? B : A;
        const double* prev = (l & 1) ? A : B;
        const double* told = oldc + kTailOff + 10 * (base + l);
        for (long long i = lo[l] + tid; i < hi[l]; i += blockDim.x) {
            double v;
            if (i < 0) {
                v = told[i + 10];
            } else if (l == 0) {
                v = src(i);
            } else {
                const double* q = prev + (2 * i - 10 - lo[l - 1]);
                double acc = q[0] * p.b11[10];
#pragma unroll
                for (int k = 1; k <= 10; ++k) acc = acc + q[k] * p.b11[10 - k];
                v = acc;
            }
            cur[i - lo[l]] = v;
        }
        __syncthreads();
        if (l < L) {           // carried inputs of stage base + l
            const long long E = p.E[base + l];
            const long long own_lo = max(0LL, (o0 - 1) * (1LL << (L - l)) + 1);
            const long long a = max(own_lo, E - 10), b = hi[l];
            for (long long i = a + tid; i < b; i += blockDim.x) newc[kTailOff + 10 * (base + l) + (i - (E - 10))] = cur[i - lo[l]];
        }
    }
    const double* res = (L & 1) ? B : A;
    for (long long i = o0 + tid; i < o1; i += blockDim.x) out[i] = res[i - lo[L]];
}

__global__ void __launch_bounds__(kThreads) levels_front_kernel(LvParams p) {
    extern __shared__ double lds[];
    const int c = blockIdx.y;
    const long long t = blockIdx.x;
    if (t < p.ntile_front) {
        const long long o0 = t * kFrontJ, o1 = min(o0 + kFrontJ, p.E[p.S]);
        const double* oldc = p.old_state + (size_t)c * kChan;
        run_stages(p, c, 0, p.S, o0, o1, o1 == p.E[p.S], lds, lds + p.capA,
                   [&](long long i) { return stage0_input(p, oldc, c, i); }, p.us + (size_t)c * p.E[p.S]);
    }
    if (!p.meters) return;
    // per chunk max|x| and sum_t (x_t x_t) kern[nk - used + t]: exp_smooth_rows_kernel's products and summation order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long k_end = min((t + 1) * p.K, p.nchunks);
    for (long long k = t * p.K + wave; k < k_end; k += kThreads / 64) {
        const long long start = k * p.chunk;
        const long long len = min(p.chunk, p.n - start);
        const long long used = min(len, (long long)p.nk);
        const double* kern = p.kern + (p.nk - used);
        double acc = 0.0, m = 0.0;
        for (long long i = lane; i < len; i += 64) {
            const double v = load_x(p, c, start + i);
            m = nan_max(m, fabs(v));
            if (i < used) acc += (v * v) * kern[i];
        }
        for (int o = 32; o > 0; o >>= 1) {
            acc += __shfl_down(acc, o, 64);
            m = nan_max(m, __shfl_down(m, o, 64));
        }
        if (lane == 0) {
            double* d = p.mt + ((size_t)c * p.nchunks + k) * 2;
            d[0] = m;
            d[1] = acc;
        }
    }
}

__global__ void __launch_bounds__(kThreads) levels_tail_kernel(LvParams p) {
    extern __shared__ double lds[];
    const int c = blockIdx.y;
    const long long t = blockIdx.x;
    const long long En = p.E[p.ndec];
    const long long o0 = t * p.Bt, o1 = min(o0 + p.Bt, En);
    const double* us = p.us + (size_t)c * p.E[p.S];
    run_stages(p, c, p.S, p.ndec - p.S, o0, o1, o1 == En, lds, lds + p.capA, [&](long long i) { return us[i]; },
               p.ud + (size_t)c * En);
}

// one thread per (block, channel): the 41-tap FIR + dB + ring; and per (state entry, channel) the carried state
__global__ void __launch_bounds__(kThreads) levels_fir_kernel(LvParams p) {
    const int c = blockIdx.y;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const double* oldc = p.old_state + (size_t)c * kChan;
    double* newc = p.new_state + (size_t)c * kChan;
    const bool active = c < p.nch;
    const long long En = p.E[p.ndec];
    const double* ud = p.ud + (size_t)c * En;
    if (p.fir && active && g < En) {
        const double* fold = oldc + kFirOff;
        const long long b = g;
        auto v = [&](long long i) { return i < 0 ? fold[i + 40] : ud[i]; };
        double acc = v(b - 40) * p.b41[40];
        for (int k = 1; k <= 40; ++k) acc = acc + v(b - 40 + k) * p.b41[40 - k];
        const double clipped = 1e-150 > acc ? 1e-150 : acc;          // max(level, 1e-150)
        const double db = 10.0 * log10(clipped);
        double* o = p.long_out + ((size_t)c * En + b) * 2;
        o[0] = acc;
        o[1] = db;
        if (b >= En - p.H) p.ring[(size_t)c * p.H + (p.ring_head + b) % p.H] = db;
    }
    if (g >= kChan) return;
    const int e = (int)g;
    double v;
    if (e < kMeta) {
        if (p.meters) return;                                          // the scan writes them
        v = oldc[e];
    } else if (e < kFirOff) {
        const int s = (e - kTailOff) / 10, q = (e - kTailOff) % 10;
        if (active && p.decim && s < p.ndec) {
            const long long i = p.E[s] - 10 + q;
            if (i >= 0) return;                                        // the tile owning index i wrote it
            v = oldc[kTailOff + 10 * s + q + p.E[s]];
        } else {
            v = oldc[e];
        }
    } else if (e < kPendOff) {
        const int q = e - kFirOff;
        if (active && p.fir) {
            const long long i = En - 40 + q;
            v = i < 0 ? oldc[kFirOff + q + En] : ud[i];
        } else {
            v = oldc[e];
        }
    } else {
        const long long k = e - kPendOff;
        if (active && p.fir) {
            const long long rest = p.r + p.n - p.E[0];
            v = k < rest ? carried_or_input(p, oldc, c, p.E[0] + k) : 0.0;      // (zeros past the end: a state is one value)
        } else {
            v = oldc[e];
        }
    }
    newc[e] = v;
}

__device__ inline double db_to_iec(double dB) {                       // iec.py
    if (dB < -70.0) return 0.0;
    if (dB < -60.0) return (dB + 70.0) * 0.0025;
    if (dB < -50.0) return (dB + 60.0) * 0.005 + 0.025;
    if (dB < -40.0) return (dB + 50.0) * 0.0075 + 0.075;
    if (dB < -30.0) return (dB + 40.0) * 0.015 + 0.15;
    if (dB < -20.0) return (dB + 30.0) * 0.02 + 0.3;
    return (dB + 20.0) * 0.025 + 0.5;
}

__global__ void __launch_bounds__(64) levels_scan_kernel(LvParams p) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.C) return;
    const double* oldc = p.old_state + (size_t)c * kChan;
    double* newc = p.new_state + (size_t)c * kChan;
    if (c >= p.nch) {
        for (int e = 0; e < kMeta; ++e) newc[e] = oldc[e];
        return;
    }
    double old_max = oldc[0], old_rms = oldc[1], peak = oldc[2], hold = oldc[3], factor = oldc[4];
    for (long long k = 0; k < p.nchunks; ++k) {
        const long long len = min(p.chunk, p.n - k * p.chunk);
        const double* d = p.mt + ((size_t)c * p.nchunks + k) * 2;
        if (len > 0) {                                                 // levels.py:95-101
            const double value_max = d[0];
            if (value_max > old_max * p.one_m_alpha2) old_max = value_max;
            else old_max *= p.one_m_alpha2;
            const double decay = len == p.chunk ? p.decay_full : p.decay_last;
            old_rms = p.alpha * d[1] + old_rms * decay;                // exp_smoothing.py:51-54
        }
        const double level_rms = 10.0 * log10(old_rms);
        const double level_max = 20.0 * log10(old_max);
        const double in = db_to_iec(level_rms > level_max ? level_rms : level_max);    // Python max(level_max, level_rms)
        double next;                                                   // ballistic_peak.py:40-62
        double branch;
        if (in > peak) {
            next = in;
            hold = 0.0;
            factor = p.peak_rate;
            branch = FRT_LEVELS_FOLLOW;
        } else if (hold + 1.0 <= 32.0) {
            next = peak;
            hold += 1.0;
            branch = FRT_LEVELS_HOLD;
        } else {
            next = factor * peak;
            if (next < in) {
                next = in;
                hold = 0.0;
                factor = p.peak_rate;
                branch = FRT_LEVELS_DECAY_FLOOR;
            } else {
                factor *= factor;
                branch = FRT_LEVELS_DECAY;
            }
        }
        peak = next;
        double* o = p.meters_out + ((size_t)c * p.nchunks + k) * kFields;
        o[0] = old_rms;
        o[1] = old_max;
        o[2] = level_rms;
        o[3] = level_max;
        o[4] = peak;
        o[5] = branch;
    }
    newc[0] = old_max;
    newc[1] = old_rms;
    newc[2] = peak;
    newc[3] = hold;
    newc[4] = factor;
    for (int e = 5; e < kMeta; ++e) newc[e] = oldc[e];
}

__global__ void levels_history_kernel(const double* __restrict__ ring, long long H, long long total, long long count, int C,
                                      double* __restrict__ out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (j >= count || c >= C) return;
    const long long idx = total - count + j;
    out[(size_t)c * count + j] = idx < 0 ? 0.0 : ring[(size_t)c * H + idx % H];
}

}  // namespace
}  // namespace frt

using namespace frt;

struct frt_levels {
    int C = 0, ndec = 0, nk = 0;
    long long H = 0;
    hipStream_t stream = nullptr;
    double alpha = 0, alpha2 = 0, peak_rate = 0;
    double b11[11], b41[41];
    std::vector<double> kern_host;
    DeviceBuffer kern, state[2], ring, xin, us, ud, mt, outs, hist;
    int cur = 0;
    long long r = 0, ring_total = 0;
    PinnedBuffer pin;
};

namespace {

// the initial state of one channel: levels.py:66-69,76 (old_rms = old_max = 1e-30), ballistic_peak.py:27-29
void initial_meta(double* m, double rate) {
    for (int e = 0; e < kMeta; ++e) m[e] = 0.0;
    m[0] = 1e-30;
    m[1] = 1e-30;
    m[2] = 0.0;
    m[3] = 0.0;
    m[4] = rate;
}

// Every call: x (device) [nch][ld], meters into dm [nch][nchunks][kFields] (or none), long levels into dl [nch][nb][2]
// (or none) / the Subsampler's outputs into dl [nch][E[ndec]] (subsample mode).
int run_device(frt_levels* h, const void* x, int dtype, long long n, long long ld, int nch, long long chunk, long long nchunks,
               double* dm, double* dl, bool subsample, long long* nout) {
    LvParams p{};
    p.x = x;
    p.ld = ld;
    p.n = n;
    p.dtype = dtype;
    p.nch = nch;
    p.C = h->C;
    p.ndec = h->ndec;
    p.S = std::min(kFrontS, h->ndec);
    p.square = subsample ? 0 : 1;
    p.meters = dm != nullptr && nchunks > 0;
    p.fir = !subsample && dl != nullptr;
    // longlevels.py:150-160: each block is audiobuffer.data_indexed(old_index, 2^Ndec), the 2^Ndec samples ENDING at
    // old_index (zeros before the stream's start); the carried samples start kHist before old_index, so that a new Ndec
    // (setresptime keeps old_index) finds them too
    p.r = p.fir ? h->r : 0;
    const long long block = 1LL << h->ndec;
    p.skip = p.fir ? kHist - block : 0;
    const long long nb = p.fir ? (p.r - kHist + n) / block : 0;
    p.E[0] = subsample ? n : nb * block;                          // 0 when the long levels are not asked for
    p.decim = p.E[0] > 0;
    for (int s = 0; s < kMaxNdec; ++s) p.E[s + 1] = (p.E[s] + 1) / 2;
    const long long En = p.E[h->ndec];
    if (nout) *nout = subsample ? En : nb;
    p.chunk = chunk;
    p.nchunks = p.meters ? nchunks : 0;
    p.K = (int)std::max<long long>(kThreads / 64, (kFrontJ << kFrontS) / std::max<long long>(chunk, 1));
    p.nk = h->nk;
    p.kern = h->kern.as<const double>();
    p.old_state = h->state[h->cur].as<const double>();
    p.new_state = h->state[1 - h->cur].as<double>();
    p.ring = h->ring.as<double>();
    p.H = h->H;
    p.ring_head = h->ring_total % h->H;
    p.alpha = h->alpha;
    p.one_m_alpha2 = 1.0 - h->alpha2;                                                  // levels.py:97,101
    p.peak_rate = h->peak_rate;
    // exp_smoothing.py:47-50: a = (1 - alpha)^N, or 0 when the chunk is longer than the kernel
    const long long last_len = nchunks > 0 ? n - (nchunks - 1) * chunk : 0;
    p.decay_full = chunk > h->nk ? 0.0 : std::pow(1.0 - h->alpha, (double)chunk);
    p.decay_last = last_len > h->nk ? 0.0 : std::pow(1.0 - h->alpha, (double)last_len);
    memcpy(p.b11, h->b11, sizeof(p.b11));
    memcpy(p.b41, h->b41, sizeof(p.b41));
    int rc;
    if (p.decim) {
        if ((rc = h->us.reserve((size_t)nch * p.E[p.S] * sizeof(double)))) return rc;
        p.us = h->us.as<double>();
        if (p.S < h->ndec) {
            if ((rc = h->ud.reserve((size_t)nch * En * sizeof(double)))) return rc;
            p.ud = h->ud.as<double>();
        } else {
            p.ud = p.us;
        }
        if (subsample) p.ud = dl;                                       // the last stage writes the caller's buffer
        if (subsample && p.S == h->ndec) p.us = dl;
    } else {
        p.ud = p.us = h->us.as<double>();
    }
    if (p.meters) {
        if ((rc = h->mt.reserve((size_t)nch * nchunks * 2 * sizeof(double)))) return rc;
        p.mt = h->mt.as<double>();
        p.meters_out = dm;
    }
    p.long_out = subsample ? nullptr : dl;
    const long long ngroups = p.meters ? (nchunks + p.K - 1) / p.K : 0;
    p.ntile_front = p.decim ? (p.E[p.S] + kFrontJ - 1) / kFrontJ : 0;
    const long long gx = std::max(p.ntile_front, ngroups);
    if (gx > 0) {
        p.capA = (kFrontJ + 10) << p.S;
        p.capB = (kFrontJ + 10) << (p.S - 1);
        const size_t lds = (size_t)(p.capA + p.capB) * sizeof(double);
        hipLaunchKernelGGL(levels_front_kernel, dim3((unsigned)gx, nch), dim3(kThreads), lds, h->stream, p);
        FRT_HIP_CHECK(hipGetLastError());
    }
    if (p.decim && p.S < h->ndec) {
        const int L = h->ndec - p.S;
        p.Bt = std::max(8, 2048 >> L);
        p.ntile_tail = (En + p.Bt - 1) / p.Bt;
        p.capA = (p.Bt + 10) << L;
        p.capB = (p.Bt + 10) << (L - 1);
        const size_t lds = (size_t)(p.capA + p.capB) * sizeof(double);
        hipLaunchKernelGGL(levels_tail_kernel, dim3((unsigned)p.ntile_tail, nch), dim3(kThreads), lds, h->stream, p);
        FRT_HIP_CHECK(hipGetLastError());
    }
    if (p.meters) {
        hipLaunchKernelGGL(levels_scan_kernel, dim3((h->C + 63) / 64), dim3(64), 0, h->stream, p);
        FRT_HIP_CHECK(hipGetLastError());
    }
    const long long items = std::max<long long>(kChan, p.fir ? En : 0);
    hipLaunchKernelGGL(levels_fir_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads), h->C), dim3(kThreads), 0, h->stream, p);
    FRT_HIP_CHECK(hipGetLastError());
    h->cur = 1 - h->cur;
    if (p.fir) {
        h->r = p.r + n - p.E[0];                                      // kHist .. kHist + 2^Ndec - 1
        h->ring_total += nb;
    }
    return FRT_OK;
}

int write_state(frt_levels* h, const std::vector<double>& s) {
    FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    FRT_HIP_CHECK(hipMemcpy(h->state[h->cur].ptr, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice));
    return FRT_OK;
}

int read_state(frt_levels* h, std::vector<double>& s) {
    s.resize((size_t)h->C * kChan);
    FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    FRT_HIP_CHECK(hipMemcpy(s.data(), h->state[h->cur].ptr, s.size() * sizeof(double), hipMemcpyDeviceToHost));
    return FRT_OK;
}

}  // namespace

extern "C" int frt_levels_create(frt_levels** out, int channels, int ndec, int64_t history_len, const double* kernel, int nk,
                                 double alpha, double alpha2, const double* gauss11, const double* gauss41, double peak_decay_rate) {
    FRT_REQUIRE(out, "frt_levels_create: null handle pointer");
    *out = nullptr;
    FRT_REQUIRE(channels >= 1 && channels <= 65535, "frt_levels_create: %d channels", channels);
    FRT_REQUIRE(ndec >= 1 && ndec <= kMaxNdec, "frt_levels_create: Ndec %d (1 .. %d supported)", ndec, kMaxNdec);
    FRT_REQUIRE(history_len >= 1, "frt_levels_create: history of %lld entries", (long long)history_len);
    FRT_REQUIRE(kernel && nk >= 1 && gauss11 && gauss41, "frt_levels_create: null table");
    FRT_REQUIRE(!is_device_pointer(kernel) && !is_device_pointer(gauss11) && !is_device_pointer(gauss41),
                "frt_levels_create: host tables");
    frt_levels* h = new frt_levels();
    h->C = channels;
    h->ndec = ndec;
    h->nk = nk;
    h->H = history_len;
    h->alpha = alpha;
    h->alpha2 = alpha2;
    h->peak_rate = peak_decay_rate;
    memcpy(h->b11, gauss11, sizeof(h->b11));
    memcpy(h->b41, gauss41, sizeof(h->b41));
    h->kern_host.assign(kernel, kernel + nk);
    int rc = upload(h->kern, h->kern_host);
    for (int i = 0; i < 2 && !rc; ++i) rc = h->state[i].reserve((size_t)channels * kChan * sizeof(double));
    if (!rc) rc = h->ring.reserve((size_t)channels * history_len * sizeof(double));
    if (!rc) rc = frt_levels_reset(h);
    if (rc) {
        frt_levels_destroy(h);
        return rc;
    }
    *out = h;
    return FRT_OK;
}

extern "C" void frt_levels_destroy(frt_levels* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : {&h->kern, &h->state[0], &h->state[1], &h->ring, &h->xin, &h->us, &h->ud, &h->mt, &h->outs, &h->hist}) b->release();
    h->pin.release();
    delete h;
    free_retired_allocations(true);
}

extern "C" int frt_levels_set_stream(frt_levels* h, void* s) {
    FRT_REQUIRE(h, "frt_levels_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_levels_reset(frt_levels* h) {
    FRT_REQUIRE(h, "frt_levels_reset: null handle");
    std::vector<double> s((size_t)h->C * kChan, 0.0);
    for (int c = 0; c < h->C; ++c) initial_meta(&s[(size_t)c * kChan], h->peak_rate);
    h->r = kHist;                                                       // zeros before the stream's start
    h->ring_total = 0;
    int rc = write_state(h, s);
    if (rc) return rc;
    FRT_HIP_CHECK(hipMemset(h->ring.ptr, 0, (size_t)h->C * h->H * sizeof(double)));
    return FRT_OK;
}

extern "C" int frt_levels_set_ndec(frt_levels* h, int ndec) {
    FRT_REQUIRE(h, "frt_levels_set_ndec: null handle");
    FRT_REQUIRE(ndec >= 1 && ndec <= kMaxNdec, "frt_levels_set_ndec: Ndec %d (1 .. %d supported)", ndec, kMaxNdec);
    std::vector<double> s;
    int rc = read_state(h, s);
    if (rc) return rc;
    // longlevels.py:212-229: a new Subsampler and zf = 0; the samples not yet consumed stay in the audio buffer
    for (int c = 0; c < h->C; ++c) std::fill(s.begin() + (size_t)c * kChan + kTailOff, s.begin() + (size_t)c * kChan + kPendOff, 0.0);
    h->ndec = ndec;
    return write_state(h, s);
}

extern "C" int64_t frt_levels_state_length(const frt_levels* h) { return h ? kHeader + (int64_t)h->C * kChan : 0; }

extern "C" int frt_levels_get_state(frt_levels* h, double* out) {
    FRT_REQUIRE(h && out, "frt_levels_get_state: null argument");
    std::vector<double> s;
    int rc = read_state(h, s);
    if (rc) return rc;
    out[0] = (double)h->r;
    out[1] = (double)h->ndec;
    memcpy(out + kHeader, s.data(), s.size() * sizeof(double));
    return FRT_OK;
}

extern "C" int frt_levels_set_state(frt_levels* h, const double* in) {
    FRT_REQUIRE(h && in, "frt_levels_set_state: null argument");
    const long long r = (long long)in[0];
    const int ndec = (int)in[1];
    FRT_REQUIRE(ndec >= 1 && ndec <= kMaxNdec && r >= kHist && r < kPendCap && (double)r == in[0],
                "frt_levels_set_state: bad header (%g pending, Ndec %g)", in[0], in[1]);
    std::vector<double> s(in + kHeader, in + kHeader + (size_t)h->C * kChan);
    int rc = write_state(h, s);
    if (rc) return rc;
    h->r = r;
    h->ndec = ndec;
    return FRT_OK;
}

extern "C" int64_t frt_levels_blocks_for(const frt_levels* h, int64_t n) {
    if (!h || n < 0) return 0;
    return (h->r - kHist + n) >> h->ndec;
}

extern "C" int64_t frt_levels_pending(const frt_levels* h) { return h ? h->r - kHist : 0; }

extern "C" int frt_levels_run(frt_levels* h, const void* x, int dtype, int64_t n, int64_t ld, int64_t chunk, double* meters_out,
                              double* long_out, int64_t* nblocks) {
    FRT_REQUIRE(h, "frt_levels_run: null handle");
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_levels_run: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(n >= 0 && ld >= n && chunk >= 1, "frt_levels_run: bad shape (n %lld, ld %lld, chunk %lld)", (long long)n, (long long)ld,
                (long long)chunk);
    FRT_REQUIRE(n == 0 || x, "frt_levels_run: null input");
    const long long nchunks = (n + chunk - 1) / chunk;
    const long long nb = long_out ? (h->r - kHist + n) >> h->ndec : 0;
    if (nblocks) *nblocks = nb;
    const size_t esize = dtype ? sizeof(double) : sizeof(float);
    const size_t mcount = meters_out ? (size_t)h->C * nchunks * kFields : 0, lcount = long_out ? (size_t)h->C * nb * 2 : 0;
    HostIO io(h->stream);
    int rc;
    if ((rc = io.in_rows(h->xin, x, ld, h->C, n, esize))) return rc;
    // one block for both outputs; a host output has its twin in it even when it has no elements: null means "not asked for"
    if ((rc = h->outs.reserve(std::max<size_t>((mcount + lcount) * sizeof(double), 64)))) return rc;
    if ((rc = io.out_at(meters_out, h->outs.as<double>(), mcount))) return rc;
    if ((rc = io.out_at(long_out, h->outs.as<double>() + mcount, lcount))) return rc;
    if ((rc = run_device(h, x, dtype, n, ld, h->C, chunk, nchunks, meters_out, long_out, false, nullptr))) return rc;
    return io.finish();
}

extern "C" int frt_levels_push(frt_levels* h, const double* x_host, int nch, int64_t n, double* meters_out, double* long_out,
                               int64_t* nblocks) {
    FRT_REQUIRE(h, "frt_levels_push: null handle");
    FRT_REQUIRE(nch >= 1 && nch <= h->C && n >= 0, "frt_levels_push: %d channels x %lld samples", nch, (long long)n);
    FRT_REQUIRE(!long_out || nch == h->C, "frt_levels_push: the long levels need all %d channels", h->C);
    FRT_REQUIRE(n == 0 || x_host, "frt_levels_push: null input");
    const long long nb = long_out ? (h->r - kHist + n) >> h->ndec : 0;
    if (nblocks) *nblocks = nb;
    const size_t xbytes = (size_t)nch * n * sizeof(double);
    const size_t mbytes = meters_out ? (size_t)nch * kFields * sizeof(double) : 0;
    const size_t lbytes = long_out ? (size_t)nch * nb * 2 * sizeof(double) : 0;
    const size_t xround = (xbytes + 255) / 256 * 256;
    int rc;
    const size_t pin_need = xround + mbytes + lbytes;
    if (h->pin.ptr && h->pin.grows(pin_need)) FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    if ((rc = h->pin.reserve(pin_need, std::max(pin_need, (size_t)1 << 16)))) return rc;
    if ((rc = h->xin.reserve(std::max<size_t>(pin_need, 64)))) return rc;
    // one upload, the launches, one download
    if (xbytes) {
        FRT_HIP_CHECK(hipStreamSynchronize(h->stream));      // the pinned block may still be the source of the previous upload
        memcpy(h->pin.ptr, x_host, xbytes);
        FRT_HIP_CHECK(hipMemcpyAsync(h->xin.ptr, h->pin.ptr, xbytes, hipMemcpyHostToDevice, h->stream));
    }
    double* dm = meters_out ? reinterpret_cast<double*>(h->xin.as<char>() + xround) : nullptr;
    double* dl = long_out ? reinterpret_cast<double*>(h->xin.as<char>() + xround + mbytes) : nullptr;
    if ((rc = run_device(h, h->xin.ptr, 1, n, n, nch, n > 0 ? n : 1, 1, dm, dl, false, nullptr))) return rc;
    if (mbytes + lbytes) {
        char* back = h->pin.as<char>() + xround;
        FRT_HIP_CHECK(hipMemcpyAsync(back, h->xin.as<char>() + xround, mbytes + lbytes, hipMemcpyDeviceToHost, h->stream));
        FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (mbytes) memcpy(meters_out, back, mbytes);
        if (lbytes) memcpy(long_out, back + mbytes, lbytes);
    } else {
        FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    return FRT_OK;
}

extern "C" int64_t frt_levels_subsample_length(const frt_levels* h, int64_t n) {
    if (!h || n < 0) return 0;
    for (int s = 0; s < h->ndec; ++s) n = (n + 1) / 2;
    return n;
}

extern "C" int frt_levels_subsample(frt_levels* h, const void* x, int dtype, int64_t n, int64_t ld, double* out, int64_t* nout) {
    FRT_REQUIRE(h, "frt_levels_subsample: null handle");
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_levels_subsample: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(n >= 0 && ld >= n, "frt_levels_subsample: bad shape");
    const long long m = frt_levels_subsample_length(h, n);
    if (nout) *nout = m;
    if (n == 0) return FRT_OK;                                          // longlevels.py:74-75: an empty push returns it
    FRT_REQUIRE(x && out, "frt_levels_subsample: null buffer");
    const size_t esize = dtype ? sizeof(double) : sizeof(float);
    HostIO io(h->stream);
    int rc;
    if ((rc = io.in_rows(h->xin, x, ld, h->C, n, esize))) return rc;
    if ((rc = io.out(h->outs, out, (size_t)h->C * m))) return rc;
    if ((rc = run_device(h, x, dtype, n, ld, h->C, 1, 0, nullptr, out, true, nullptr))) return rc;
    return io.finish();
}

extern "C" int frt_levels_history(frt_levels* h, int64_t count, double* out) {
    FRT_REQUIRE(h && out, "frt_levels_history: null argument");
    FRT_REQUIRE(count >= 0 && count <= h->H, "frt_levels_history: %lld entries of a ring of %lld", (long long)count, h->H);
    if (count == 0) return FRT_OK;
    HostIO io(h->stream);
    int rc;
    if ((rc = io.out(h->hist, out, (size_t)h->C * count))) return rc;
    hipLaunchKernelGGL(levels_history_kernel, dim3((unsigned)((count + 255) / 256), h->C), dim3(256), 0, h->stream, h->ring.as<const double>(),
                       h->H, h->ring_total, (long long)count, h->C, out);
    FRT_HIP_CHECK(hipGetLastError());
    return io.finish();
}
