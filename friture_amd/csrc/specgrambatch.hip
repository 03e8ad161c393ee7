// specgrambatch.hip — the spectrogram widget's screen stages over whole recordings (Spectrogram_Widget.handle_new_data,
// friture/spectrogram.py:161-173) for gfx950: S streams x a time slab of normalised frames -> pixel columns in one call, behind
// the float64 STFT engine (FRT_STFT_NORM).  Built with -ffp-contract=off; the arithmetic is screen_columns_kernel's
// (specgram.hip), operation for operation:
//   Frequency_Resampler.push: np.interp per frame           friture/signal/frequency_resampler.py:67-83    (freq_interp)
//   Online_Linear_2D_resampler.push: cur (1 - a) + prev a   friture/signal/online_linear_2D_resampler.py:61-97, linear_interp.py:57-60
//   Color_Transform.push: lut[int(clip(v, 0, 1) * 255)]     friture/signal/color_tranform.py:48-51
//   addData: frequency axis flipped                         friture/spectrogram_image.py:82-92
// The scalar recurrence that decides which frame feeds which column with which weight stays with the caller (the column table).
//
// specgram_batch_kernel: a workgroup owns one stream, a block of kRows screen rows and a tile of kTile consecutive frames plus
// the frame before the tile (the first tile's is the carried column).
//   phase 1  lanes run along the screen rows of one frame: neighbouring rows have neighbouring interval indices, so a wavefront's
//            loads of a frame fall into few cache lines, and a row block reads only its own part of the spectrum.  The
//            frequency-resampled value of (frame, row) is formed ONCE, into LDS (screen_columns_kernel forms it twice per pixel).
//            Frames that no column of the tile reads are skipped (pixel rate below the STFT rate).
//   phase 2  lanes run along the output columns of the tile: a pixel row of the tile leaves as one contiguous run of uint32.
// LDS: (kTile + 1) x (kRows + 1) doubles = 34 056 bytes, four workgroups per CU; the odd row pitch spreads the lanes of phase 2,
// which read one row of different frames, over the banks.  Any height: the row blocks are the grid's y axis.
#include <cmath>
#include <vector>

#include "common.h"
#include "screen_interp.h"

namespace frt {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 128;              // screen rows per workgroup
constexpr int kTile = 32;               // frames per tile
constexpr int kPitch = kRows + 1;       // doubles per frame in LDS

struct SpecgramBatchParams {
    const double* norm;                 // norm[s * ld_stream + f * ld_frame + b]
    long long ld_frame, ld_stream;
    int nb, height;
    long long n_frames;
    const int* jidx;                    // [height] interval tables of the screen rows
    const double* dx;
    const double* den;
    const int* src;                     // [n_cols] source frame of the slab, < 0: a column the resampler allocated and never wrote
    const double* a;                    // [n_cols]
    const long long* tile_col;          // [n_tiles + 1] the columns whose source frame lies in each tile
    const double* old_in;               // [streams][height]
    double* old_out;
    const uint32_t* lut;
    uint32_t* pixels;                   // pixels[s * height * ld_pixel + (height - 1 - h) * ld_pixel + col_offset + c]
    long long ld_pixel, col_offset;
};

__global__ __launch_bounds__(kThreads) void specgram_batch_kernel(const SpecgramBatchParams p) {
    __shared__ double col[(kTile + 1) * kPitch];
    __shared__ uint32_t lut[256];
    __shared__ int need[kTile + 1];
    const int tid = threadIdx.x;
    const int s = blockIdx.z;
    const int r0 = blockIdx.y * kRows;
    const long long f0 = (long long)blockIdx.x * kTile;
    const int nf = (int)(p.n_frames - f0 < kTile ? p.n_frames - f0 : kTile);
    const long long c0 = p.tile_col[blockIdx.x], c1 = p.tile_col[blockIdx.x + 1];
    const bool has_last = f0 + nf == p.n_frames;                      // this tile leaves the carried column
    if (c0 == c1 && !has_last) return;
    const int rows = p.height - r0 < kRows ? p.height - r0 : kRows;

    lut[tid] = p.lut[tid];
    if (tid <= kTile) need[tid] = 0;
    __syncthreads();
    for (long long c = c0 + tid; c < c1; c += kThreads) {
        const int sc = p.src[c];
        if (sc >= 0) {                                               // slot 0 is frame f0 - 1
            need[sc - f0] = 1;
            need[sc - f0 + 1] = 1;
        }
    }
    if (tid == 0 && has_last) need[nf] = 1;
    __syncthreads();

    // ---- phase 1: np.interp of the tile's frames onto this block's rows -----------------------------------------------
    {
        const int r = tid % kRows;
        if (r < rows) {
            const int h = r0 + r;
            const int j = p.jidx[h];
            const double dx = p.dx[h], den = p.den[h];
            const double* base = p.norm + (size_t)s * p.ld_stream;
            for (int fl = tid / kRows; fl <= nf; fl += kThreads / kRows) {
                if (!need[fl]) continue;
                const long long f = f0 - 1 + fl;
                col[fl * kPitch + r] = f < 0 ? p.old_in[(size_t)s * p.height + h] : freq_interp(base + (size_t)f * p.ld_frame, p.nb, j, dx, den);
            }
        }
    }
    __syncthreads();
    if (has_last && tid < rows) p.old_out[(size_t)s * p.height + r0 + tid] = col[nf * kPitch + tid];

    // ---- phase 2: time lerp, clip, LUT; lanes along the columns --------------------------------------------------------
    const int nc = (int)(c1 - c0);
    uint32_t* out = p.pixels + (size_t)s * p.height * p.ld_pixel + p.col_offset + c0;
    for (int i = tid; i < rows * nc; i += kThreads) {
        const int r = i / nc, k = i - r * nc;
        const int sc = p.src[c0 + k];
        uint32_t px = lut[0];                                        // np.zeros of the resampler's block -> lut[0]
        if (sc >= 0) {
            const int fl = (int)(sc - f0);
            const double cur = col[(fl + 1) * kPitch + r], prev = col[fl * kPitch + r];
            const double w = p.a[c0 + k];
            double v = cur * (1.0 - w) + prev * w;                   // linear_interp.py:57-60
            v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);                 // numpy.clip (NaN falls through to the cast like numpy's)
            px = lut[(int)(v * 255.0)];
        }
        out[(size_t)(p.height - 1 - (r0 + r)) * p.ld_pixel + k] = px;
    }
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" int frt_specgram_batch(const double* norm, int streams, int64_t n_frames, int nb, int64_t ld_frame, int64_t ld_stream,
                                  const double* freq, const double* targets, int height, const int* src, const double* a,
                                  int64_t n_cols, const double* old_in, double* old_out, const uint32_t* lut256, uint32_t* pixels,
                                  int64_t col_offset, int64_t ld_pixel) {
    FRT_REQUIRE(streams >= 1 && streams <= 65535 && n_frames >= 1 && n_frames < ((int64_t)1 << 40) && nb >= 1 && height >= 1 && n_cols >= 0,
                "frt_specgram_batch: %d streams x %lld frames x %d bins, height %d, %lld columns", streams, (long long)n_frames, nb,
                height, (long long)n_cols);
    FRT_REQUIRE(norm && freq && targets && old_in && old_out && lut256, "frt_specgram_batch: null argument");
    FRT_REQUIRE(!is_device_pointer(freq) && !is_device_pointer(targets) && !is_device_pointer(lut256),
                "frt_specgram_batch: freq, targets and lut256 are host tables");
    FRT_REQUIRE((n_frames == 1 || ld_frame >= nb) && (streams == 1 || ld_stream >= (n_frames - 1) * (n_frames > 1 ? ld_frame : 0) + nb),
                "frt_specgram_batch: bad shape (ld_frame %lld, ld_stream %lld)", (long long)ld_frame, (long long)ld_stream);
    FRT_REQUIRE(old_in != old_out || !is_device_pointer(old_out), "frt_specgram_batch: old_in and old_out must not overlap");
    const long long ldf = n_frames > 1 ? ld_frame : nb;
    const long long lds = streams > 1 ? ld_stream : (n_frames - 1) * ldf + nb;
    const long long n_tiles = (n_frames + kTile - 1) / kTile;
    FRT_REQUIRE(n_tiles <= 0x7fffffffLL, "frt_specgram_batch: %lld frames in one call", (long long)n_frames);
    const long long row_blocks = (height + kRows - 1) / kRows;
    FRT_REQUIRE(row_blocks <= 65535, "frt_specgram_batch: height %d", height);
    if (n_cols > 0) {
        FRT_REQUIRE(src && a && pixels && !is_device_pointer(src) && !is_device_pointer(a), "frt_specgram_batch: src and a are host tables of n_cols entries");
        FRT_REQUIRE(col_offset >= 0 && ld_pixel >= col_offset + n_cols, "frt_specgram_batch: columns [%lld, %lld) in rows of %lld pixels",
                    (long long)col_offset, (long long)(col_offset + n_cols), (long long)ld_pixel);
        FRT_REQUIRE(is_device_pointer(pixels) || (col_offset == 0 && ld_pixel == n_cols),
                    "frt_specgram_batch: a host pixel block is written whole (col_offset 0, ld_pixel = n_cols)");
    }
    // the columns of each tile: the source frames ascend (a filler column stays with the frame before it)
    std::vector<long long> tile_col((size_t)n_tiles + 1, n_cols);
    {
        long long t = 0, eff = 0;
        tile_col[0] = 0;
        for (int64_t c = 0; c < n_cols; ++c) {
            if (src[c] >= 0) {
                FRT_REQUIRE(src[c] < n_frames && src[c] >= eff, "frt_specgram_batch: source frame %d of column %lld (ascending, below %lld)",
                            src[c], (long long)c, (long long)n_frames);
                eff = src[c];
            }
            while (t < eff / kTile) tile_col[(size_t)++t] = c;
        }
    }
    std::vector<int> j((size_t)height);
    std::vector<double> dx((size_t)height), den((size_t)height);
    interval_search(freq, nb, targets, height, j.data(), dx.data(), den.data());

    const size_t old_bytes = (size_t)streams * height * sizeof(double);
    const size_t cols_alloc = n_cols > 0 ? (size_t)n_cols : 1;
    const int zero_src = 0;
    const double zero_a = 0.0;
    StageCall call;
    const int i_norm = call.add_in(norm, ((size_t)(streams - 1) * lds + (size_t)(n_frames - 1) * ldf + nb) * sizeof(double));
    const int i_j = call.add_in(j.data(), (size_t)height * sizeof(int));
    const int i_dx = call.add_in(dx.data(), (size_t)height * sizeof(double));
    const int i_den = call.add_in(den.data(), (size_t)height * sizeof(double));
    const int i_src = call.add_in(n_cols > 0 ? src : &zero_src, cols_alloc * sizeof(int));
    const int i_a = call.add_in(n_cols > 0 ? a : &zero_a, cols_alloc * sizeof(double));
    const int i_tc = call.add_in(tile_col.data(), tile_col.size() * sizeof(long long));
    const int i_old = call.add_in(old_in, old_bytes);
    const int i_lut = call.add_in(lut256, 256 * sizeof(uint32_t));
    const int i_oldo = call.add_out(old_out, old_bytes);
    const int i_pix = n_cols > 0 ? call.add_out(pixels, (size_t)streams * height * ld_pixel * sizeof(uint32_t)) : call.add_scratch(sizeof(uint32_t));
    int rc = call.begin();
    if (rc) return rc;
    SpecgramBatchParams p{};
    p.norm = call.ptr<const double>(i_norm);
    p.ld_frame = ldf;
    p.ld_stream = lds;
    p.nb = nb;
    p.height = height;
    p.n_frames = n_frames;
    p.jidx = call.ptr<const int>(i_j);
    p.dx = call.ptr<const double>(i_dx);
    p.den = call.ptr<const double>(i_den);
    p.src = call.ptr<const int>(i_src);
    p.a = call.ptr<const double>(i_a);
    p.tile_col = call.ptr<const long long>(i_tc);
    p.old_in = call.ptr<const double>(i_old);
    p.old_out = call.ptr<double>(i_oldo);
    p.lut = call.ptr<const uint32_t>(i_lut);
    p.pixels = call.ptr<uint32_t>(i_pix);
    p.ld_pixel = n_cols > 0 ? ld_pixel : 1;
    p.col_offset = n_cols > 0 ? col_offset : 0;
    hipLaunchKernelGGL(specgram_batch_kernel, dim3((unsigned)n_tiles, (unsigned)row_blocks, (unsigned)streams), dim3(kThreads), 0, call.stream(), p);
    FRT_HIP_CHECK(hipGetLastError());
    return call.finish();
}
