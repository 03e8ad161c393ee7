// screen_interp.h — np.interp onto the screen rows, shared by specgram.hip and specgrambatch.hip (both compiled with
// -ffp-contract=off): the interval search on the host and the per-row evaluation on the device
// (friture/signal/frequency_resampler.py:67-83).
#pragma once
#include <hip/hip_runtime.h>

namespace frt {

// np.interp with the interval index found on the host (frequency_resampler.py:80; same branches as freq_resample_kernel).
__device__ __forceinline__ double freq_interp(const double* __restrict__ col, int nb, int j, double dx, double den) {
    if (j < 0) return col[0];
    if (j >= nb - 1) return col[nb - 1];
    const double f0 = col[j];
    if (dx == 0.0) return f0;
    const double slope = (col[j + 1] - f0) / den;
    return slope * dx + f0;
}

// numpy.interp's interval search for the screen rows (largest j with freq[j] <= x; -1 / nb outside the table)
static inline void interval_search(const double* freq, int nb, const double* targets, int height, int* j, double* dx, double* den) {
    for (int r = 0; r < height; ++r) {
        const double x = targets[r];
        dx[r] = 0.0;
        den[r] = 1.0;
        if (!(x >= freq[0])) { j[r] = -1; continue; }
        if (x > freq[nb - 1]) { j[r] = nb; continue; }
        int lo = 0, hi = nb;
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (freq[mid] <= x) lo = mid; else hi = mid;
        }
        j[r] = lo;
        if (lo < nb - 1) {
            dx[r] = x - freq[lo];
            den[r] = freq[lo + 1] - freq[lo];
        }
    }
}

}  // namespace frt
