// spectrumbatch.hip — the spectrum widget's chain over whole recordings (Spectrum_Widget.handle_new_data, friture/spectrum.py:
// 125-184) for gfx950: S streams x R refreshes x B bins in one call, between the float64 STFT engine and frt_curves_run.
// float64 arithmetic; built with -ffp-contract=off: every value is a fixed sequence of IEEE operations, whichever lane forms it.
//
// Per refresh r of stream s, its n = frame_start[r + 1] - frame_start[r] PSD frames in frame order (exp_smoothing.py:91-107):
//   sp   = alpha * sum_t psd[t] * kernel[nk - n + t] + previous * (1 - alpha)^n       (n > nk: the first nk frames, decay 0)
//   dB   = 10 log10(sp + 1e-30) + w            (two rows: 10 log10(sp2 + 1e-30) - 10 log10(sp1 + 1e-30))
//   peak = argmax(dB);  pitch = argmax(sp1[k] * sp1[2k] * sp1[3k], k < B / 3);  the first index wins ties
//
// Kernels of one call (all on one stream):
//   spectrum_batch_scan_kernel    one lane per (stream, bin), consecutive bins in consecutive lanes (frames are read as whole
//                                 rows): walks the refreshes in time order with the smoothed values in registers.  A lane of the
//                                 lower third also carries the recurrences of bins 2k and 3k of the first row — the same operations
//                                 on the same data as their own lanes run, so the same bits — and forms the harmonic product
//                                 without any exchange between workgroups.  Each wavefront leaves its (value, index) maxima of dB
//                                 and of the product per refresh in scratch: no barrier anywhere, a wavefront never waits for
//                                 another.  The refresh table, the decays and the smoothing kernel are read at wave-uniform addresses.
//   spectrum_batch_argmax_kernel  one lane per (stream, output refresh): the first maximum over the wavefronts' partials
#include <cmath>
#include <map>
#include <vector>

#include "common.h"
#include "widget_device.h"

namespace frt {
namespace {

constexpr int kThreads = 256;
constexpr int kNone = 0x7fffffff;

struct BatchParams {
    long long ld_frame, ld_row;     // psd[(s * rows + row) * ld_row + f * ld_frame + b]
    int rows;                       // 1, or 2 (dual channels)
    int B, K;                       // bins, B / 3
    int W, Wh;                      // wavefronts per row of dB, of the harmonic product
    long long R, Ro;                // refreshes; output rows per stream: R, or 1 (keep_last)
    long long ld_db;                // db[s * ld_db + ro * B + b]
    int nk;
    double alpha;
    const double* st_in;            // [streams][rows][B]
    double* st_out;
    double* db;
    double* part_v;                 // [streams][Ro][W] then [streams][Ro][Wh]
    int* part_i;
};

// one refresh of one bin: frames f0 .. f0 + n - 1 of `col` (the bin's column of one row), taps kt[0 .. n - 1]
template <bool kF64>
__device__ __forceinline__ double smooth(const void* col, long long ld_frame, long long f0, int n, const double* __restrict__ kt,
                                         double alpha, double previous, double decay) {
    double acc = 0.0;
#pragma unroll 4
    for (int t = 0; t < n; ++t) acc += load_real<kF64>(col, (f0 + t) * ld_frame) * kt[t];
    return alpha * acc + previous * decay;
}

template <bool kF64>
__global__ __launch_bounds__(kThreads) void spectrum_batch_scan_kernel(const void* __restrict__ psd, const long long* __restrict__ frame_start,
                                                                       const double* __restrict__ decay, const double* __restrict__ kern,
                                                                       const double* __restrict__ weight, BatchParams p) {
    const int s = blockIdx.y;
    const int k = blockIdx.x * kThreads + threadIdx.x;
    const int wave = k >> 6;                                         // of the row; k & ~63 is the wavefront's first bin
    if ((k & ~63) >= p.B) return;                                    // whole wavefronts only: the shuffles below
    const bool live = k < p.B, hlive = k < p.K;
    const bool dual = p.rows == 2;
    const size_t esz = kF64 ? 8 : 4;
    const char* row0 = reinterpret_cast<const char*>(psd) + (size_t)s * p.rows * p.ld_row * esz;
    const char* row1 = row0 + (size_t)p.ld_row * esz;
    const double* st = p.st_in + (size_t)s * p.rows * p.B;
    double sp0 = 0., sp1 = 0., h2 = 0., h3 = 0.;
    if (live) {
        sp0 = st[k];
        if (dual) sp1 = st[p.B + k];
    }
    if (hlive) {
        h2 = st[2 * k];
        h3 = st[3 * k];
    }
    const double wk = (live && weight) ? weight[k] : 0.;
    for (long long r = 0; r < p.R; ++r) {
        const long long f0 = frame_start[r];
        long long nn = frame_start[r + 1] - f0;
        const double dec = decay[r];                                 // 0 where nn > nk
        if (nn > p.nk) nn = p.nk;                                    // data[:, :nk]: the refresh's first nk frames
        const int n = (int)nn;
        const double* kt = kern + (p.nk - n);
        if (live) {
            sp0 = smooth<kF64>(row0 + (size_t)k * esz, p.ld_frame, f0, n, kt, p.alpha, sp0, dec);
            if (dual) sp1 = smooth<kF64>(row1 + (size_t)k * esz, p.ld_frame, f0, n, kt, p.alpha, sp1, dec);
        }
        if (hlive) {
            h2 = smooth<kF64>(row0 + (size_t)(2 * k) * esz, p.ld_frame, f0, n, kt, p.alpha, h2, dec);
            h3 = smooth<kF64>(row0 + (size_t)(3 * k) * esz, p.ld_frame, f0, n, kt, p.alpha, h3, dec);
        }
        if (p.Ro != p.R && r != p.R - 1) continue;                   // keep_last: only the state walks
        const long long ro = p.Ro == p.R ? r : 0;
        const size_t orow = (size_t)s * p.Ro + ro;
        ArgMax best = {-INFINITY, kNone};
        if (live) {
            double d;
            if (dual) d = 10.0 * log10(sp1 + 1e-30) - 10.0 * log10(sp0 + 1e-30);
            else d = 10.0 * log10(sp0 + 1e-30) + wk;
            p.db[(size_t)s * p.ld_db + (size_t)ro * p.B + k] = d;
            if (!(d != d)) best = ArgMax{d, k};
        }
        best = wave_argmax(best);
        if ((threadIdx.x & 63) == 0) {
            p.part_v[orow * p.W + wave] = best.v;
            p.part_i[orow * p.W + wave] = best.i;
        }
        if ((k & ~63) < p.K) {                                       // wave-uniform
            ArgMax hb = {-INFINITY, kNone};
            if (hlive) {
                const double h = sp0 * h2 * h3;
                if (!(h != h)) hb = ArgMax{h, k};
            }
            hb = wave_argmax(hb);
            if ((threadIdx.x & 63) == 0) {
                const size_t o = (size_t)gridDim.y * p.Ro * p.W + orow * p.Wh + wave;
                p.part_v[o] = hb.v;
                p.part_i[o] = hb.i;
            }
        }
    }
    if (live) {
        double* so = p.st_out + (size_t)s * p.rows * p.B;
        so[k] = sp0;
        if (dual) so[p.B + k] = sp1;
    }
}

// rows = streams * Ro; the partials of a row are in ascending bin order
__global__ __launch_bounds__(kThreads) void spectrum_batch_argmax_kernel(const double* __restrict__ part_v, const int* __restrict__ part_i,
                                                                         long long rows, int W, int Wh, int* __restrict__ peak,
                                                                         int* __restrict__ pitch) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= rows) return;
    ArgMax m = {-INFINITY, kNone};
    for (int w = 0; w < W; ++w) m = better(m, ArgMax{part_v[g * W + w], part_i[g * W + w]});
    peak[g] = m.i == kNone ? 0 : m.i;
    const size_t o = (size_t)rows * W + (size_t)g * Wh;
    ArgMax h = {-INFINITY, kNone};
    for (int w = 0; w < Wh; ++w) h = better(h, ArgMax{part_v[o + w], part_i[o + w]});
    pitch[g] = h.i == kNone ? 0 : h.i;
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" int frt_spectrum_batch(const void* psd, int dtype, int streams, int rows, int64_t n_frames, int64_t bins, int64_t ld_frame,
                                  int64_t ld_row, const int64_t* frame_start, int64_t n_refresh, const double* kernel, int nk,
                                  double alpha, const double* weight_db, double* state, int keep_last, double* db_out,
                                  int64_t ld_db_stream, int* peak_index_out, int* pitch_index_out) {
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_spectrum_batch: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(rows == 1 || rows == 2, "frt_spectrum_batch: %d rows per stream (1, or 2 for dual channels)", rows);
    FRT_REQUIRE(streams >= 1 && streams <= 65535 && bins >= 3 && bins < (1 << 30) && n_frames >= 0 && n_refresh >= 0,
                "frt_spectrum_batch: %d streams x %lld frames x %lld bins, %lld refreshes", streams, (long long)n_frames,
                (long long)bins, (long long)n_refresh);
    FRT_REQUIRE((n_frames <= 1 || ld_frame >= bins) &&
                    (streams * rows == 1 || n_frames == 0 || ld_row >= (n_frames - 1) * (n_frames > 1 ? ld_frame : 0) + bins),
                "frt_spectrum_batch: bad shape (ld_frame %lld, ld_row %lld)", (long long)ld_frame, (long long)ld_row);
    FRT_REQUIRE(nk >= 1 && kernel && !is_device_pointer(kernel), "frt_spectrum_batch: kernel is a host table of nk >= 1 taps");
    FRT_REQUIRE(state, "frt_spectrum_batch: null state");
    if (n_refresh == 0) return FRT_OK;
    FRT_REQUIRE(frame_start && !is_device_pointer(frame_start), "frt_spectrum_batch: frame_start must be host memory");
    FRT_REQUIRE(db_out && peak_index_out && pitch_index_out, "frt_spectrum_batch: null output");
    FRT_REQUIRE(frame_start[0] >= 0 && frame_start[n_refresh] <= n_frames, "frt_spectrum_batch: frame_start [%lld, %lld] outside [0, %lld]",
                (long long)frame_start[0], (long long)frame_start[n_refresh], (long long)n_frames);
    for (int64_t r = 0; r < n_refresh; ++r)
        FRT_REQUIRE(frame_start[r + 1] >= frame_start[r], "frt_spectrum_batch: frame_start not sorted at %lld", (long long)r);
    FRT_REQUIRE(n_frames == 0 || psd, "frt_spectrum_batch: null input");
    const int64_t Ro = keep_last ? 1 : n_refresh;
    const int64_t ld_db = streams > 1 && ld_db_stream ? ld_db_stream : Ro * bins;
    FRT_REQUIRE(ld_db >= Ro * bins && (ld_db == Ro * bins || is_device_pointer(db_out)),
                "frt_spectrum_batch: ld_db_stream %lld (at least %lld; padded streams need a device output)", (long long)ld_db_stream,
                (long long)(Ro * bins));

    // (1 - alpha)^n per distinct n, as frt_spectrum_post forms it (exp_smoothing.py:94-101)
    std::vector<long long> fs(frame_start, frame_start + n_refresh + 1);
    std::vector<double> decay((size_t)n_refresh);
    std::map<long long, double> pow_of;
    for (int64_t r = 0; r < n_refresh; ++r) {
        const long long n = fs[r + 1] - fs[r];
        auto it = pow_of.find(n);
        if (it == pow_of.end()) it = pow_of.emplace(n, n > nk ? 0.0 : std::pow(1.0 - alpha, (double)n)).first;
        decay[r] = it->second;
    }

    BatchParams p{};
    p.rows = rows;
    p.B = (int)bins;
    p.K = (int)bins / 3;
    p.W = (p.B + 63) / 64;
    p.Wh = (p.K + 63) / 64;
    p.R = n_refresh;
    p.Ro = Ro;
    p.ld_db = ld_db;
    p.nk = nk;
    p.alpha = alpha;
    p.ld_frame = n_frames > 1 ? ld_frame : bins;
    p.ld_row = streams * rows > 1 ? ld_row : (n_frames > 0 ? (n_frames - 1) * p.ld_frame + bins : bins);
    const size_t es = dtype ? sizeof(double) : sizeof(float);
    const size_t pbytes = n_frames ? ((size_t)(streams * rows - 1) * p.ld_row + (size_t)(n_frames - 1) * p.ld_frame + bins) * es : 0;
    const size_t stbytes = (size_t)streams * rows * bins * sizeof(double);
    const size_t orows = (size_t)streams * Ro;
    const size_t parts = orows * (p.W + p.Wh);

    StageCall call;
    const double zero = 0.0;
    const int ipsd = pbytes ? call.add_in(psd, pbytes) : call.add_in(&zero, sizeof(double));
    const int ifs = call.add_in(fs.data(), fs.size() * sizeof(long long));
    const int idec = call.add_in(decay.data(), decay.size() * sizeof(double));
    const int ikern = call.add_in(kernel, (size_t)nk * sizeof(double));
    const int iw = weight_db ? call.add_in(weight_db, (size_t)bins * sizeof(double)) : -1;
    // a lane reads the state of bins 2k and 3k, which other workgroups write at their end: a state in device memory is read
    // from a copy (a host state is staged into a block of its own anyway)
    const bool st_dev = is_device_pointer(state);
    const int isi = st_dev ? call.add_scratch(stbytes) : call.add_in(state, stbytes);
    const int iso = call.add_out(state, stbytes);
    const int idb = call.add_out(db_out, ((size_t)(streams - 1) * ld_db + (size_t)Ro * bins) * sizeof(double));
    const int ipk = call.add_out(peak_index_out, orows * sizeof(int));
    const int ipt = call.add_out(pitch_index_out, orows * sizeof(int));
    const int ipv = call.add_scratch(parts * sizeof(double));
    const int ipi = call.add_scratch(parts * sizeof(int));
    int rc = call.begin();
    if (rc) return rc;
    const hipStream_t stream = call.stream();
    if (st_dev) FRT_HIP_CHECK(hipMemcpyAsync(call.ptr<void>(isi), state, stbytes, hipMemcpyDeviceToDevice, stream));
    p.st_in = call.ptr<const double>(isi);
    p.st_out = call.ptr<double>(iso);
    p.db = call.ptr<double>(idb);
    p.part_v = call.ptr<double>(ipv);
    p.part_i = call.ptr<int>(ipi);
    const dim3 grid((unsigned)((bins + kThreads - 1) / kThreads), (unsigned)streams);
    const double* d_w = iw >= 0 ? call.ptr<const double>(iw) : nullptr;
    if (dtype)
        hipLaunchKernelGGL(spectrum_batch_scan_kernel<true>, grid, dim3(kThreads), 0, stream, call.ptr<const void>(ipsd),
                           call.ptr<const long long>(ifs), call.ptr<const double>(idec), call.ptr<const double>(ikern), d_w, p);
    else
        hipLaunchKernelGGL(spectrum_batch_scan_kernel<false>, grid, dim3(kThreads), 0, stream, call.ptr<const void>(ipsd),
                           call.ptr<const long long>(ifs), call.ptr<const double>(idec), call.ptr<const double>(ikern), d_w, p);
    FRT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(spectrum_batch_argmax_kernel, dim3((unsigned)((orows + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       p.part_v, p.part_i, (long long)orows, p.W, p.Wh, call.ptr<int>(ipk), call.ptr<int>(ipt));
    FRT_HIP_CHECK(hipGetLastError());
    return call.finish();
}
