// widget_device.h — device helpers shared by the widget translation units (spectrum.hip, spectrumbatch.hip, curves.hip,
// scope.hip).  spectrum.hip is built with floating-point contraction on and the others with it off: nothing here
// may hold a multiply next to an add, or one source line would mean two instruction sequences.
#pragma once
#include <hip/hip_runtime.h>

namespace frt {

// element i of a float32 or float64 array, as float64 (float32 widens exactly)
template <bool kF64>
__device__ __forceinline__ double load_real(const void* base, long long i) {
    return kF64 ? reinterpret_cast<const double*>(base)[i] : (double)reinterpret_cast<const float*>(base)[i];
}

__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }   // numpy.max: NaN wins

__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

struct ArgMax {
    double v;
    int i;
};

__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {          // first index wins ties (numpy.argmax)
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ ArgMax wave_argmax(ArgMax m) {
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax other = {__shfl_xor(m.v, o, 64), __shfl_xor(m.i, o, 64)};
        m = better(m, other);
    }
    return m;
}

}  // namespace frt
