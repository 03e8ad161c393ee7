// rfft64.h — the float64 real-FFT frame that transfer.hip (X1) and convolve.hip (X2) are built on: a frame of N complex points
// goes through fft_core.h's transform with 8 points per thread, N / 8 threads per frame; wave-local (several frames per
// wavefront of 64) up to N = 512, one workgroup of N / 8 threads above.  Here: the plan's constants, the choice of an
// instantiation by log2 N, the twiddle table and the LDS allowance.  The kernels stay in their files: each translation unit
// has its own floating-point contraction.
#pragma once
#include <cmath>
#include <type_traits>
#include <vector>

#include "common.h"
#include "fft_core.h"

namespace frt {
namespace rfft64 {

using C = cpx<double>;

template <int LOG2>
struct Plan {
    static constexpr int N = 1 << LOG2, TPF = N / 8;
    static constexpr bool WAVE_LOCAL = TPF <= 64;
    static constexpr int BLOCK = WAVE_LOCAL ? 64 : TPF;
    static constexpr int IPB = BLOCK / TPF;                     // frames (frame groups) per workgroup
    static constexpr size_t LDS = (size_t)IPB * lds_padded_size(N) * sizeof(C);
};

struct Launch {                                   // what the host needs of a Plan
    int block, ipb;
    size_t lds;
};

template <int LOG2>
constexpr Launch launch_of() {
    return Launch{Plan<LOG2>::BLOCK, Plan<LOG2>::IPB, Plan<LOG2>::LDS};
}

// f(std::integral_constant<int, LOG2>) for LOG2 == log2 in LO .. HI; false outside
template <int LO, int HI, typename F>
bool dispatch(int log2, F&& f) {
    if constexpr (LO > HI) {
        return false;
    } else {
        if (log2 != LO) return dispatch<LO + 1, HI>(log2, f);
        f(std::integral_constant<int, LO>{});
        return true;
    }
}

inline int log2_of(long long v) {
    int l = 0;
    while ((1LL << l) < v) ++l;
    return l;
}

// t[n] = exp(-2 pi i n / N), n < N; with `half` behind it t[N + n] = exp(-i pi n / N), n < N
inline std::vector<C> twiddles(int N, bool half) {
    std::vector<C> t((size_t)(half ? 2 : 1) * N);
    const long double step = -3.14159265358979323846264338327950288L / (long double)N;
    for (int n = 0; n < N; ++n) {
        t[n] = C{(double)cosl(2.0L * step * n), (double)sinl(2.0L * step * n)};
        if (half) t[N + n] = C{(double)cosl(step * n), (double)sinl(step * n)};
    }
    return t;
}

// the kernel may use `lds` bytes of dynamic LDS per workgroup
inline int allow_lds(const void* kernel, size_t lds, const char* who, const char* what, int size) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) return FRT_OK;
    set_last_error("%s: %zu bytes of LDS per workgroup refused for %s %d", who, lds, what, size);
    return FRT_ERR_HIP;
}

}  // namespace rfft64
}  // namespace frt
