// rowfront.h — what the entries over rows of samples share (frt_decay_run, frt_mtf_run, frt_sos_run, frt_spl_run): the wavefront folds of
// their kernels, the opening of the entry, the row slabs that keep a launch's scratch within scratch_bytes, the workgroups per
// row of a tile loop, and the end of a handle.  (convolve.hip, deconvolve.hip, transfer.hip and loudness.hip cut their scratch
// into windows and runs, not rows.)
#pragma once
#include <algorithm>
#include <initializer_list>

#include "hostio.h"

namespace frt {

constexpr long long kMaxSamples = 1LL << 24;      // per row and call
static_assert(sizeof(long long) == sizeof(int64_t), "int64_t is long long here");

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a butterfly (xor G / 2 .. 1) over groups of G lanes: every lane of a group ends with the same value
template <int G = 64>
__device__ __forceinline__ double fold_sum(double v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int G = 64>
__device__ __forceinline__ double fold_max(double v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// what every entry over rows of samples requires of x, its rows and scratch_bytes; `who` is the entry's name
inline int require_rows(const char* who, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, int64_t scratch_bytes) {
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "%s: x_dtype %d (0 float32, 1 float64)", who, x_dtype);
    FRT_REQUIRE(rows >= 1 && rows <= 65535, "%s: %d rows (1 .. 65535)", who, rows);
    FRT_REQUIRE(n >= 1 && n <= kMaxSamples && x, "%s: bad input (n %lld, 1 .. 2^24)", who, (long long)n);
    FRT_REQUIRE(rows == 1 || row_stride >= n, "%s: bad stride (n %lld, row stride %lld)", who, (long long)n, (long long)row_stride);
    FRT_REQUIRE(scratch_bytes >= 0, "%s: scratch_bytes %lld", who, (long long)scratch_bytes);
    return FRT_OK;
}

// v [rows] (or null) on the host lies within lo .. hi, which the message spells as `range`; a device array passes: the kernel
// that reads it makes a row with a bad value dead
inline int require_row_integers(const char* who, const char* name, const int64_t* v, long long rows, long long lo, long long hi,
                                const char* range) {
    if (!v || is_device_pointer(v)) return FRT_OK;
    for (long long r = 0; r < rows; ++r)
        FRT_REQUIRE(v[r] >= lo && v[r] <= hi, "%s: %s[%lld] = %lld (%s)", who, name, r, (long long)v[r], range);
    return FRT_OK;
}

// row slabs: the scratch of one launch stays within scratch_bytes, at least one row per launch; `scratch` holds one slab
inline int reserve_slab(DeviceBuffer& scratch, long long rows, long long scratch_bytes, long long per_row, long long& slab) {
    slab = std::min(rows, std::max(1LL, scratch_bytes / per_row));
    return scratch.reserve((size_t)(slab * per_row));
}

// The workgroups (of `waves` wavefronts, a tile each) per row of a launch whose wavefronts loop over a row's live tiles, so that
// a short live span in a long row costs no launch of idle workgroups: enough of them to fill the device when the rows are few.
// tests/decay_helpers.py restates this formula (tile_groups), and tests/test_decay_edges_gpu.py and tests/test_sti_edges_gpu.py
// (the tile loops' second trip) derive their shapes from it: change them together.
inline unsigned tile_groups(long long ntile, unsigned rows_in_launch, int waves) {
    const long long all_groups = (ntile + waves - 1) / waves, nr = rows_in_launch;
    return (unsigned)std::min(all_groups, std::max(16LL, (8192 + nr - 1) / nr));
}

// the end of a handle (not null): whatever its stream still runs, its buffers, the handle, the blocks its buffers had parked
template <typename Handle>
void destroy_handle(Handle* h, std::initializer_list<DeviceBuffer*> buffers) {
    (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer* b : buffers) b->release();
    delete h;
    free_retired_allocations(true);
}

}  // namespace frt
