// pitch_device.h — device code shared by pitch.hip, pitchbatch.hip and pitchstream.hip: the pieces of the pitch chain that
// must mean one instruction sequence wherever they run (all three files are built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

namespace frt {

__device__ __forceinline__ double wave_sum(double v) {
    // fixed-order butterfly: every lane ends with the same, scheduling-independent sum
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// dBFS of `count` samples whose squares add up to `energy`   (pitch_tracker.py:399-400, 407-408)
__device__ __forceinline__ double level_db(double energy, double count) {
    return 20.0 * log10(sqrt(energy / count) + std::numeric_limits<double>::epsilon());
}

// np.argmax ordering: the first NaN wins, otherwise the first maximum
__device__ __forceinline__ bool argmax_before(double va, int ia, double vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

// arg-max over the K strengths of one frame by one wavefront: every lane ends with the winner
__device__ __forceinline__ void pick_argmax(const double* st, int K, int lane, double& best, int& bi) {
    best = st[lane < K ? lane : 0];
    bi = lane < K ? lane : 0;
    for (int c = lane + 64; c < K; c += 64) {
        const double v = st[c];
        if (argmax_before(v, c, best, bi)) { best = v; bi = c; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (argmax_before(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
}

// parabolic vertex around the winner and index -> Hz   (:392-402, fastParabolicInterp :187-191); one lane
__device__ __forceinline__ double pick_frequency(const double* st, int bi, int K, int L, const double* freqs) {
    double shift = 0.0;
    if (bi > 0 && bi < K - 1) {
        const double y1 = st[bi - 1], y2 = st[bi], y3 = st[bi + 1];
        const double pa = (y1 - 2 * y2 + y3) / 2;
        const double pb = (y3 - y1) / 2;
        shift = -pb / (2 * pa + std::numeric_limits<double>::epsilon());
    }
    // np.interp(idx + shift, arange(L), freqs)   (:402)
    const double xq = (double)bi + shift;
    double f0;
    if (xq != xq) {
        f0 = xq;
    } else if (xq < 0.0) {
        f0 = freqs[0];
    } else if (xq >= (double)(L - 1)) {
        f0 = freqs[L - 1];
    } else {
        const int j = (int)floor(xq);
        const double fj = freqs[j];
        if ((double)j == xq) {
            f0 = fj;
        } else {
            const double slope = (freqs[j + 1] - fj) / ((double)(j + 1) - (double)j);
            f0 = slope * (xq - (double)j) + fj;
        }
    }
    return f0;
}

__device__ __forceinline__ double pick_confidence(double best) { return best / 2.56; }          // :412

// One frame of the voiced / unvoiced gate (:405-428) on raw[3][C][F] = (estimate, confidence, dBFS); `before` is the raw
// estimate of the frame before (or the carried one).
struct GateFrame {
    bool ok, jump_ok;
    double f0;
};

__device__ __forceinline__ GateFrame gate_frame(const double* raw, int C, long long F, int chan, long long f, double before,
                                                double min_db, double conf, double p_delta) {
    GateFrame g;
    g.f0 = raw[(0ll * C + chan) * F + f];
    const double cf = raw[(1ll * C + chan) * F + f];
    const double db = raw[(2ll * C + chan) * F + f];
    g.ok = !((db < min_db) || (cf < conf));
    g.jump_ok = !(12.0 * fabs(log2(g.f0 / before)) > p_delta);
    return g;
}

// update_curve, :114-117: an estimate on the OctaveC axis, flipped and clipped.  fmax ignores NaN: unvoiced estimates and the
// zeros before the first frame sit at 1, and the result is never NaN.
__device__ __forceinline__ double axis_value(double v, double trans_min, double trans_span) {
    const double t = (log2(fmax(v, 1e-20)) - trans_min) / trans_span;
    return fmin(fmax(1.0 - t, 0.0), 1.0);
}

}  // namespace frt
