// scope.hip — the oscilloscope (Scope_Widget) for gfx950: rising-edge trigger on row 0, traces, many refreshes per call.
// float64 comparisons and arithmetic; built with -ffp-contract=off so that scaled_y is the reference's three IEEE operations.
//
// Reference semantics (friture/scope.py:78-135), per refresh k of stream s, the stream seen up to e = ends[k] (zeros before 0):
//   trigger mode (timerange <= 500 ms): window = x[e - 2w, e); region = window[w//2 : -(w//2 rounded up)], w samples starting
//     at r0 = e - 2w + w//2; level = (max(region) * 2.) / 3. (numpy max: a NaN anywhere makes the level NaN, so no trigger);
//     trigger = the first i with region[i] < level and region[i + 1] >= level; the trace is window[:, i : i + 2 (w//2)],
//     every row cut at the same place, i.e. it starts at absolute index e - 2w + i.  No crossing: no trace (the widget keeps
//     its previous curves).
//   scrolling mode (timerange > 500 ms): the trace is x[:, e - w, e), always.
//   scaled_y = 1. - (y + 1) / 2.
//
// Kernels of one call (all on one stream):
//   scope_block_max_kernel  one read of row 0: the NaN-propagating max of every aligned sub-block of kSub samples and of every
//                           aligned block of kBlock samples (trigger mode, widths that can hold a whole sub-block)
//   scope_trigger_kernel    one wavefront per refresh: the region's max from the whole blocks it covers (one load of up to 64
//                           block maxima), the whole sub-blocks at its two ends (< 8 each, one load) and the samples at its two
//                           ends (< kSub each, one load each), so the cost of the max does not grow with the width; then the
//                           crossing search from the region's start, 64 samples per step (the first step's samples are loaded
//                           together with the max's), a ballot per step, exit at the first crossing
//   scope_trace_kernel      the traces of the refreshes that triggered (raw and/or scaled), 1024 samples per workgroup
#include <cmath>

#include "common.h"
#include "widget_device.h"

namespace frt {
namespace {

constexpr int kBlock = 512;                 // samples per block maximum (the widget's chunk)
constexpr int kSub = 64;                    // samples per sub-block maximum: 8 per block
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTraceTile = 4 * kThreads;    // trace samples per workgroup
constexpr int kInlineEnds = 4;              // this many refreshes or fewer: the ends travel in the kernel arguments

struct ScopeParams {
    const void* x;                  // device: x[s * ld_stream + r * ld_row + t]
    long long ld_row, ld_stream, n;
    int dtype;                      // 0 float32, 1 float64
    int streams, rows;
    long long K;                    // refreshes
    const long long* ends;          // device [K], or null: ends_inline
    long long ends_inline[kInlineEnds];
    long long w, h;                 // width, width // 2
    int scrolling;
    long long nb, ns;               // blocks and sub-blocks of row 0 per stream: ceil(n / kBlock), ceil(n / kSub)
    double* bmax;                   // [streams][nb]
    double* smax;                   // [streams][ns]
    long long* start;               // [streams][K]
    long long L;                    // trace length: 2h (trigger) or w (scrolling)
    double* raw;                    // [streams][rows][K][L] or null
    double* scaled;                 // [streams][rows][K][L] or null
    const double* keep_raw;         // host-staged outputs: what the caller's buffers held, copied where nothing triggered
    const double* keep_scaled;
};

__device__ __forceinline__ double load(const ScopeParams& p, const char* row, long long t) {
    if (t < 0) return 0.0;                                          // before the stream's start: a fresh ring's zeros
    return p.dtype ? load_real<true>(row, t) : load_real<false>(row, t);
}

__device__ __forceinline__ const char* row_ptr(const ScopeParams& p, int s, int r) {
    const size_t es = p.dtype ? sizeof(double) : sizeof(float);
    return reinterpret_cast<const char*>(p.x) + ((size_t)s * p.ld_stream + (size_t)r * p.ld_row) * es;
}

__device__ __forceinline__ long long end_of(const ScopeParams& p, long long k) {
    return p.ends ? p.ends[k] : p.ends_inline[k];
}

// one wavefront per block of kBlock samples: lane l takes the 8 samples 8l .. 8l + 7 (16-byte loads when the row allows them),
// lanes 8q .. 8q + 7 make sub-block q
template <bool kVec>
__global__ __launch_bounds__(kThreads) void scope_block_max_kernel(ScopeParams p) {
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int s = blockIdx.y;
    if (j >= p.nb) return;
    const char* row = row_ptr(p, s, 0);
    const long long t0 = j * kBlock;
    double m = -INFINITY;
    if (kVec && t0 + kBlock <= p.n) {
        if (p.dtype) {
            const double2* q = reinterpret_cast<const double2*>(reinterpret_cast<const double*>(row) + t0) + 4 * lane;
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = q[u];
#pragma unroll
            for (int u = 0; u < 4; ++u) m = nanmax(nanmax(m, v[u].x), v[u].y);
        } else {
            const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(row) + t0) + 2 * lane;
            float4 v[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) v[u] = q[u];
#pragma unroll
            for (int u = 0; u < 2; ++u)
                m = nanmax(nanmax(nanmax(nanmax(m, (double)v[u].x), (double)v[u].y), (double)v[u].z), (double)v[u].w);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long t = t0 + 8 * lane + u;
            if (t < p.n) m = nanmax(m, load(p, row, t));
        }
    }
    for (int o = 1; o < 8; o <<= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    const long long sj = j * (kBlock / kSub) + (lane >> 3);
    if ((lane & 7) == 0 && sj * kSub < p.n) p.smax[(size_t)s * p.ns + sj] = m;
    for (int o = 8; o < 64; o <<= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) p.bmax[(size_t)s * p.nb + j] = m;
}

__device__ __forceinline__ long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

__global__ __launch_bounds__(kThreads) void scope_trigger_kernel(ScopeParams p) {
    const int lane = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (idx >= (long long)p.streams * p.K) return;
    const int s = (int)(idx / p.K);
    const long long k = idx - (long long)s * p.K;
    const long long e = end_of(p, k);
    long long start = FRT_SCOPE_NO_TRIGGER;
    if (p.scrolling) {
        start = e - p.w;
    } else {
        const char* row = row_ptr(p, s, 0);
        const long long r0 = e - 2 * p.w + p.h, r1 = r0 + p.w;         // the search region [r0, r1), r1 <= e <= n
        // the first scan step's samples do not depend on the level: loaded together with the max's
        const bool first = lane < p.w - 1;
        const double v0 = first ? load(p, row, r0 + lane) : 0.0, v1 = first ? load(p, row, r0 + lane + 1) : 0.0;
        const long long s0 = -floor_div(-r0, kSub), s1 = floor_div(r1, kSub);        // whole sub-blocks [s0, s1)
        double m = -INFINITY;
        if (s0 < s1) {
            if (r0 + lane < s0 * kSub) m = nanmax(m, load(p, row, r0 + lane));       // < kSub samples at each end
            if (s1 * kSub + lane < r1) m = nanmax(m, load(p, row, s1 * kSub + lane));
            constexpr int kPer = kBlock / kSub;
            const long long b0 = -floor_div(-s0, kPer), b1 = floor_div(s1, kPer);   // whole blocks [b0, b1)
            const double* sm = p.smax + (size_t)s * p.ns;
            long long js;
            bool take;
            if (b0 < b1) {                                                         // < 8 sub-blocks at each end
                js = lane < kPer ? s0 + lane : b1 * kPer + (lane - kPer);
                take = lane < kPer ? js < b0 * kPer : (lane < 2 * kPer && js < s1);
                const double* bm = p.bmax + (size_t)s * p.nb;
                for (long long jb = b0 + lane; jb < b1; jb += 64) m = nanmax(m, jb < 0 ? 0.0 : bm[jb]);   // before 0: zeros
            } else {                                                               // < 16 sub-blocks, no whole block
                js = s0 + lane;
                take = js < s1;
            }
            if (take) m = nanmax(m, js < 0 ? 0.0 : sm[js]);
        } else {                                                                   // < 2 kSub samples
            for (long long t = r0 + lane; t < r1; t += 64) m = nanmax(m, load(p, row, t));
        }
        m = wave_max(m);
        const double level = (m * 2.) / 3.;                              // scope.py:109, in this order
        if (level == level) {
            for (long long i0 = 0; i0 < p.w - 1; i0 += 64) {
                const long long i = i0 + lane;
                bool c = false;
                if (i0 == 0)
                    c = first && v0 < level && v1 >= level;
                else if (i < p.w - 1)
                    c = load(p, row, r0 + i) < level && load(p, row, r0 + i + 1) >= level;
                const unsigned long long mask = __ballot(c);
                if (mask) {
                    start = r0 + i0 + (__ffsll((long long)mask) - 1) - p.h;
                    break;
                }
            }
        }
    }
    if (lane == 0) p.start[idx] = start;
}

// one workgroup per (stream, row, refresh, tile of kTraceTile samples)
__global__ __launch_bounds__(kThreads) void scope_trace_kernel(ScopeParams p, long long tiles) {
    long long b = blockIdx.x;
    const long long tile = b % tiles;
    b /= tiles;
    const long long k = b % p.K;
    b /= p.K;
    const int r = (int)(b % p.rows);
    const int s = (int)(b / p.rows);
    const long long start = p.start[(size_t)s * p.K + k];
    const size_t base = (((size_t)s * p.rows + r) * p.K + k) * p.L;
    if (start == FRT_SCOPE_NO_TRIGGER) {
        if (!p.keep_raw && !p.keep_scaled) return;
        for (int u = 0; u < 4; ++u) {
            const long long j = tile * kTraceTile + u * kThreads + threadIdx.x;
            if (j >= p.L) break;
            if (p.raw && p.keep_raw) p.raw[base + j] = p.keep_raw[base + j];
            if (p.scaled && p.keep_scaled) p.scaled[base + j] = p.keep_scaled[base + j];
        }
        return;
    }
    const char* row = row_ptr(p, s, r);
    for (int u = 0; u < 4; ++u) {
        const long long j = tile * kTraceTile + u * kThreads + threadIdx.x;
        if (j >= p.L) break;
        const double y = load(p, row, start + j);                       // start + j < e <= n
        if (p.raw) p.raw[base + j] = y;
        if (p.scaled) p.scaled[base + j] = 1. - (y + 1) / 2.;           // scope.py:129
    }
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" int64_t frt_scope_trace_length(int64_t width, int scrolling) {
    if (width < 1) return 0;
    return scrolling ? width : 2 * (width / 2);
}

extern "C" int frt_scope_run(const void* x, int dtype, int streams, int rows, int64_t n, int64_t ld_row, int64_t ld_stream,
                             const int64_t* ends, int64_t n_refresh, int64_t width, int scrolling, int64_t* start_out,
                             double* trace_out, int trace_kind) {
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_scope_run: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(streams >= 1 && streams <= 65535 && rows >= 1 && rows <= 65535, "frt_scope_run: %d streams x %d rows", streams, rows);
    FRT_REQUIRE(n >= 0 && (rows == 1 || ld_row >= n) && (streams == 1 || ld_stream >= (rows - 1) * ld_row + n),
                "frt_scope_run: bad shape (n %lld, ld_row %lld, ld_stream %lld)", (long long)n, (long long)ld_row, (long long)ld_stream);
    FRT_REQUIRE(width >= 1, "frt_scope_run: width %lld (the trigger region would be empty)", (long long)width);
    FRT_REQUIRE(n_refresh >= 0 && (n_refresh == 0 || (ends && start_out)), "frt_scope_run: null ends or start_out");
    FRT_REQUIRE(n == 0 || x, "frt_scope_run: null input");
    FRT_REQUIRE(trace_kind >= 0 && trace_kind <= (FRT_SCOPE_TRACE_RAW | FRT_SCOPE_TRACE_SCALED) && (!trace_out || trace_kind),
                "frt_scope_run: trace_kind %d", trace_kind);
    if (n_refresh == 0) return FRT_OK;
    FRT_REQUIRE(!is_device_pointer(ends), "frt_scope_run: ends must be host memory");
    for (int64_t k = 0; k < n_refresh; ++k) {
        FRT_REQUIRE(ends[k] >= 0 && ends[k] <= n, "frt_scope_run: ends[%lld] = %lld outside [0, %lld]", (long long)k, (long long)ends[k],
                    (long long)n);
        FRT_REQUIRE(k == 0 || ends[k] >= ends[k - 1], "frt_scope_run: ends not sorted at %lld", (long long)k);
    }
    ScopeParams p{};
    p.dtype = dtype;
    p.streams = streams;
    p.rows = rows;
    p.n = n;
    p.ld_row = rows > 1 ? ld_row : n;
    p.ld_stream = streams > 1 ? ld_stream : (long long)(rows - 1) * p.ld_row + n;
    p.K = n_refresh;
    p.w = width;
    p.h = width / 2;
    p.scrolling = scrolling ? 1 : 0;
    p.L = frt_scope_trace_length(width, p.scrolling);
    p.nb = (n + kBlock - 1) / kBlock;
    p.ns = (n + kSub - 1) / kSub;
    const bool traces = trace_out && p.L > 0;
    const int nkind = traces ? ((trace_kind & FRT_SCOPE_TRACE_RAW) ? 1 : 0) + ((trace_kind & FRT_SCOPE_TRACE_SCALED) ? 1 : 0) : 0;
    const size_t es = dtype ? sizeof(double) : sizeof(float);
    const size_t xbytes = n ? ((size_t)(streams - 1) * p.ld_stream + (size_t)(rows - 1) * p.ld_row + n) * es : 0;
    const size_t sbytes = (size_t)streams * n_refresh * sizeof(int64_t);
    const size_t tbytes = (size_t)streams * rows * n_refresh * p.L * sizeof(double);
    const bool need_bmax = !p.scrolling && width >= kSub && p.nb > 0;        // a region of < kSub samples holds no sub-block
    const bool inline_ends = n_refresh <= kInlineEnds;
    const long long tiles = (p.L + kTraceTile - 1) / kTraceTile;
    FRT_REQUIRE(!traces || (long long)streams * rows * n_refresh * tiles < (1LL << 31),
                "frt_scope_run: %lld trace workgroups (split the call)", (long long)streams * rows * n_refresh * tiles);

    StageCall call;
    const int ix = call.add_in(n ? x : nullptr, xbytes);
    const int is = call.add_out(start_out, sbytes);
    const bool trace_host = traces && !is_device_pointer(trace_out);
    // staged (host) traces: what the caller's buffer holds goes up too, so that refreshes without a trigger leave it as it was
    const int ik = trace_host ? call.add_in(trace_out, nkind * tbytes) : -1;
    const int it = traces ? call.add_out(trace_out, nkind * tbytes) : -1;
    const int ib = need_bmax ? call.add_scratch((size_t)streams * (p.nb + p.ns) * sizeof(double)) : -1;
    const int ie = inline_ends ? -1 : call.add_scratch(n_refresh * sizeof(int64_t));
    int rc = call.begin();
    if (rc) return rc;
    p.x = n ? call.ptr<const void>(ix) : nullptr;
    p.start = call.ptr<long long>(is);
    if (traces) {
        double* t = call.ptr<double>(it);
        const double* kp = ik >= 0 ? call.ptr<const double>(ik) : nullptr;
        const size_t step = tbytes / sizeof(double);
        int slot = 0;
        if (trace_kind & FRT_SCOPE_TRACE_RAW) {
            p.raw = t;
            p.keep_raw = kp;
            ++slot;
        }
        if (trace_kind & FRT_SCOPE_TRACE_SCALED) {
            p.scaled = t + slot * step;
            p.keep_scaled = kp ? kp + slot * step : nullptr;
        }
    }
    if (need_bmax) {
        p.bmax = call.ptr<double>(ib);
        p.smax = p.bmax + (size_t)streams * p.nb;
    }
    const hipStream_t stream = call.stream();
    if (inline_ends) {
        for (int64_t k = 0; k < n_refresh; ++k) p.ends_inline[k] = ends[k];
    } else {
        p.ends = call.ptr<const long long>(ie);
        FRT_HIP_CHECK(hipMemcpyAsync(const_cast<long long*>(p.ends), ends, n_refresh * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    }
    if (need_bmax) {
        const bool vec = ((uintptr_t)p.x % 16 == 0) && (p.ld_stream * es) % 16 == 0;
        const dim3 grid((unsigned)((p.nb + kWaves - 1) / kWaves), streams);
        if (vec)
            hipLaunchKernelGGL(scope_block_max_kernel<true>, grid, dim3(kThreads), 0, stream, p);
        else
            hipLaunchKernelGGL(scope_block_max_kernel<false>, grid, dim3(kThreads), 0, stream, p);
        FRT_HIP_CHECK(hipGetLastError());
    }
    const long long waves = (long long)streams * n_refresh;
    hipLaunchKernelGGL(scope_trigger_kernel, dim3((unsigned)((waves + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, p);
    FRT_HIP_CHECK(hipGetLastError());
    if (traces) {
        const long long blocks = (long long)streams * rows * n_refresh * tiles;
        hipLaunchKernelGGL(scope_trace_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, p, tiles);
        FRT_HIP_CHECK(hipGetLastError());
    }
    return call.finish();
}
