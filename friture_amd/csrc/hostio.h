// hostio.h — the host boundary of the recording entries (frt_levels_run / _subsample / _history, frt_resample_run,
// frt_loudness_run, frt_transfer_run, frt_convolve_run): every array argument is a host array or a device array, in any mix.
//
// A HostIO lives for one call.  A host input is copied to a DeviceBuffer of the handle on the call's stream and the site's
// pointer (and stride) is repointed to it; a host output gets a device twin, which the kernels write and finish() copies
// back.  A device array, a null pointer and an array of no elements pass through as they are.  The order on the stream is
// the sites': uploads, the launches, then in finish() the downloads in the order the outputs were named and ONE
// synchronisation.  (The live entries with double-buffered pinned slots, PinnedSlot, and the widget entries, StageCall, are
// other designs: common.h.)
#pragma once
#include "common.h"

namespace frt {

class HostIO {
  public:
    explicit HostIO(hipStream_t stream) : stream_(stream) {}

    // `groups` groups of `rows` rows of n elements of esize bytes: row stride ld, group stride group_ld, both in elements.
    // Staged, the rows lie densely: ld = n, group_ld = rows n.  A single row's stride is not read (sites leave it unchecked).
    template <typename I>
    int in_rows(DeviceBuffer& buf, const void*& x, I& ld, I& group_ld, size_t groups, size_t rows, long long n, size_t esize) {
        if (n <= 0 || is_device_pointer(x)) return FRT_OK;
        const size_t width = (size_t)n * esize, pitch = (size_t)(groups * rows == 1 ? n : ld) * esize;
        int rc = buf.reserve(groups * rows * width);
        if (rc) return rc;
        if (groups == 1 || group_ld == (long long)rows * ld) {
            FRT_HIP_CHECK(hipMemcpy2DAsync(buf.ptr, width, x, pitch, width, groups * rows, hipMemcpyHostToDevice, stream_));
        } else {
            for (size_t g = 0; g < groups; ++g)
                FRT_HIP_CHECK(hipMemcpy2DAsync(buf.as<char>() + g * rows * width, width, reinterpret_cast<const char*>(x) + g * group_ld * esize,
                                               pitch, width, rows, hipMemcpyHostToDevice, stream_));
        }
        x = buf.ptr;
        ld = n;
        group_ld = (I)rows * n;
        return FRT_OK;
    }
    template <typename I>
    int in_rows(DeviceBuffer& buf, const void*& x, I& ld, size_t rows, long long n, size_t esize) {
        I all = 0;
        return in_rows(buf, x, ld, all, 1, rows, n, esize);
    }

    // a flat block of `count` elements
    template <typename T>
    int in(DeviceBuffer& buf, const T*& p, size_t count) {
        if (!p || !count || is_device_pointer(p)) return FRT_OK;
        int rc = buf.reserve(count * sizeof(T));
        if (rc) return rc;
        FRT_HIP_CHECK(hipMemcpyAsync(buf.ptr, p, count * sizeof(T), hipMemcpyHostToDevice, stream_));
        p = buf.as<const T>();
        return FRT_OK;
    }

    // Outputs: p becomes the address to hand to the kernels.  out_at is for a site that placed the twin itself (`staged`, inside
    // a block it reserved): a host array is staged whatever its count, and only the copy back of no elements is left out.
    template <typename T>
    int out_at(T*& p, T* staged, size_t count) {
        if (!p || is_device_pointer(p)) return FRT_OK;
        int rc = back(p, 0, staged, count * sizeof(T), 1);
        p = staged;
        return rc;
    }
    template <typename T>
    int out(DeviceBuffer& buf, T*& p, size_t count) {
        if (!p || !count || is_device_pointer(p)) return FRT_OK;
        int rc = buf.reserve(count * sizeof(T));
        return rc ? rc : out_at(p, buf.as<T>(), count);
    }
    template <typename I>
    int out_rows(DeviceBuffer& buf, void*& y, I& ld, size_t rows, long long n, size_t esize) {
        if (!y || n <= 0 || is_device_pointer(y)) return FRT_OK;
        int rc = buf.reserve(rows * n * esize);
        if (!rc) rc = back(y, (size_t)(rows == 1 ? n : ld) * esize, buf.ptr, (size_t)n * esize, rows);
        y = buf.ptr;
        ld = n;
        return rc;
    }

    int finish() {
        for (int i = 0; i < n_; ++i) {
            const Back& b = back_[i];
            if (b.rows == 1) FRT_HIP_CHECK(hipMemcpyAsync(b.dst, b.src, b.width, hipMemcpyDeviceToHost, stream_));
            else FRT_HIP_CHECK(hipMemcpy2DAsync(b.dst, b.pitch, b.src, b.width, b.width, b.rows, hipMemcpyDeviceToHost, stream_));
        }
        n_ = 0;
        FRT_HIP_CHECK(hipStreamSynchronize(stream_));
        return FRT_OK;
    }

  private:
    struct Back {
        void* dst;
        size_t pitch;
        const void* src;
        size_t width, rows;
    };
    int back(void* dst, size_t pitch, const void* src, size_t width, size_t rows) {
        if (!width) return FRT_OK;
        FRT_REQUIRE(n_ < kMost, "HostIO: more than %d staged outputs in one call", kMost);
        back_[n_++] = Back{dst, pitch, src, width, rows};
        return FRT_OK;
    }
    static constexpr int kMost = 4;
    hipStream_t stream_;
    Back back_[kMost];
    int n_ = 0;
};

}  // namespace frt
