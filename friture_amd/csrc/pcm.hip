// pcm.hip — PCM ingest: interleaved integer / float recordings to the planar float rows of the chains (frt_pcm_*; the
// definition: include/friture_hip.h).
//
// A workgroup takes one tile of F = frt_pcm_tile_frames(format, channels) frames, F a multiple of 64 with F * C * width <= 32 KB,
// tiles counted from frame 0 of the buffer: F * C * width is a multiple of 16, so every tile starts at the buffer's own
// address mod 16.  The tile's bytes are read ONCE, all channels of them — one contiguous span, whatever `select` keeps; a
// channel that is not selected costs its bytes and nothing else — as aligned 16-byte loads (kFill in flight per thread: a whole
// tile in one trip), the partial granules at the two ends of the requested range byte by byte: no byte outside the requested
// frames is touched.  The LDS image keeps the address mod 16 (byte A of the buffer sits at logical byte A - base16, base16 the
// tile's start rounded down to 16), so that a global granule is four whole logical dwords, and logical dword D is stored at
//
//     pcm_phys(D) = D + (D >> 5) + (D >> 10)
//
// one pad dword behind every 32 and one more behind every 1024.  After the barrier the lanes of a wavefront run along 64
// consecutive frames of one output row: lane stride C * width bytes in LDS, which for a frame of 128 B (s32 x 32), 256 B
// (f64 x 32) or any other power of two would put a lane group on one bank; with the pads, strides of 2 .. 32 dwords step one
// bank per 32 dwords and strides of 64 and 128 dwords one bank per 1024 (the degrees per format and channel count:
// tools/exp/lds_layout_model.py).  A lane assembles its sample from aligned dwords — one where the buffer's
// address is a multiple of the width, otherwise (and always for s24) two or three joined by a byte shift: no LDS access is
// off its natural alignment for any address of the buffer — converts it and stores it: one frame per lane, 4 or 8 bytes, 256
// or 512 contiguous bytes per wavefront and store.
#include "common.h"

#include <algorithm>

struct frt_pcm {
    hipStream_t stream = nullptr;
    frt::PinnedSlot in[2], out[2];          // raw slabs on their way up, decoded slabs on their way back
    frt::DeviceBuffer raw, rows, sel;
    std::vector<int32_t> sel_host;
    bool used = false;                      // a decode got as far as the device: destroying an unused handle makes no device call
};

namespace {

using namespace frt;

constexpr int kFormats = 6;
constexpr int kWidth[kFormats] = {1, 2, 3, 4, 4, 8};
constexpr int kTileBytes = 32768;                         // raw bytes of a tile at most
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFill = 8;                                  // 16-byte loads in flight per thread while the image is filled
constexpr int kItems = 4;                                 // LDS reads in flight per lane while it is decoded
constexpr size_t kDefaultSlab = (size_t)64 << 20;

__host__ __device__ constexpr unsigned pcm_phys(unsigned D) { return D + (D >> 5) + (D >> 10); }
// logical bytes: up to 15 in front of the tile, the tile, 8 behind it for the second and third dword of an unaligned sample
constexpr unsigned kLdsDwords = pcm_phys((15 + kTileBytes + 8) / 4 + 1) + 1;

int tile_frames(int format, int channels) { return kTileBytes / (channels * kWidth[format]) / 64 * 64; }

struct Params {
    unsigned long long src;      // address of the first byte of frame src_frame
    long long src_frame;
    long long first, last;       // the frames to decode
    long long tile0;             // the tile of block 0
    void* y;                     // row s, frame f at y[s * ldy + f - y_frame]
    long long ldy, y_frame;
    const int32_t* select;
    int n_select, C, F, aligned;
};

__device__ inline unsigned join(unsigned lo, unsigned hi, unsigned shift) {      // bytes shift / 8 .. of hi:lo
    return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> shift);
}

// the W bytes at logical byte L of the image, little-endian, in lo (and hi for W = 8)
template <int W, bool aligned>
__device__ inline void fetch(const unsigned* lds, unsigned L, unsigned& lo, unsigned& hi) {
    const unsigned D = L >> 2, shift = (L & 3) * 8;
    hi = 0;
    if (W == 1) {
        lo = (lds[pcm_phys(D)] >> shift) & 0xffu;
    } else if (W == 2 && aligned) {
        lo = (lds[pcm_phys(D)] >> shift) & 0xffffu;
    } else if (W == 4 && aligned) {
        lo = lds[pcm_phys(D)];
    } else if (W == 8 && aligned) {
        lo = lds[pcm_phys(D)];
        hi = lds[pcm_phys(D + 1)];
    } else if (W <= 4) {
        lo = join(lds[pcm_phys(D)], lds[pcm_phys(D + 1)], shift);
        if (W < 4) lo &= (1u << (8 * (W & 3))) - 1u;
    } else {
        const unsigned a = lds[pcm_phys(D)], b = lds[pcm_phys(D + 1)], c = lds[pcm_phys(D + 2)];
        lo = join(a, b, shift);
        hi = join(b, c, shift);
    }
}

// one rounding of the exact value at most: every integer format is exact in float64, u8 / s16 / s24 in float32 too
template <int FMT, typename Tout>
__device__ inline Tout value(unsigned lo, unsigned hi) {
    if (FMT == 0) return (Tout)((int)lo - 128) * (Tout)0x1p-7;
    if (FMT == 1) return (Tout)(int)(short)lo * (Tout)0x1p-15;
    if (FMT == 2) return (Tout)((int)(lo ^ 0x800000u) - 0x800000) * (Tout)0x1p-23;
    if (FMT == 3) return (Tout)((double)(int)lo * 0x1p-31);
    if (FMT == 4) return (Tout)__uint_as_float(lo);
    return (Tout)__longlong_as_double((long long)((((unsigned long long)hi) << 32) | lo));
}

struct Tile {
    unsigned mis, ra, rb, frame;      // the image's offset in its first granule, the frames [ra, rb) of the tile to decode, bytes per frame
    long long col0;                   // output column of the tile's frame 0
};

// A wavefront per 64 frames of a row, the wavefronts of the workgroup on consecutive chunks of it.  The item index is wave-uniform,
// and said to be: row and channel are scalar, the channel a scalar load.  kItems items per trip — their channels loaded first,
// then every LDS read, then the stores: an item past the end reads the last one again, a frame outside the range its nearest
// frame inside, and neither is stored.
template <int FMT, typename Tout, bool ALIGNED>
__device__ inline void decode_rows(const unsigned* lds, const Params& p, const Tile& t) {
    constexpr int W = kWidth[FMT];
    const unsigned lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned c0 = t.ra >> 6, chunks = ((t.rb + 63) >> 6) - c0, items = chunks * (unsigned)p.n_select;
    Tout* y = reinterpret_cast<Tout*>(p.y);
    for (unsigned it0 = wave; it0 < items; it0 += kItems * kWaves) {
        unsigned lo[kItems], hi[kItems], r[kItems], s[kItems], ch[kItems];
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const unsigned it = it0 + u * kWaves < items ? it0 + u * kWaves : items - 1;
            s[u] = it / chunks;
            r[u] = ((c0 + it - s[u] * chunks) << 6) + lane;
            ch[u] = (unsigned)p.select[s[u]];
        }
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            const unsigned rr = r[u] < t.ra ? t.ra : r[u] >= t.rb ? t.rb - 1 : r[u];
            fetch<W, ALIGNED>(lds, t.mis + rr * t.frame + ch[u] * W, lo[u], hi[u]);
        }
#pragma unroll
        for (int u = 0; u < kItems; ++u)
            if (it0 + u * kWaves < items && r[u] >= t.ra && r[u] < t.rb)
                y[(long long)s[u] * p.ldy + (t.col0 + r[u])] = value<FMT, Tout>(lo[u], hi[u]);
    }
}

template <int FMT, typename Tout>
__global__ __launch_bounds__(kThreads) void pcm_decode_kernel(Params p) {
    constexpr int W = kWidth[FMT];
    __shared__ __align__(16) unsigned lds[kLdsDwords];
    const long long tile = p.tile0 + blockIdx.x, t0 = tile * p.F;
    const long long fa = t0 > p.first ? t0 : p.first, fb = t0 + p.F < p.last ? t0 + p.F : p.last;
    if (fa >= fb) return;
    const unsigned frame = (unsigned)p.C * W;
    const unsigned long long base = p.src + (unsigned long long)((t0 - p.src_frame) * (long long)frame);      // may lie before src: never read
    const unsigned long long base16 = base & ~15ull;
    const unsigned ra = (unsigned)(fa - t0), rb = (unsigned)(fb - t0);
    {   // the bytes [lo, hi) of frames fa .. fb - 1: whole 16-byte granules inside them, the ends byte by byte
        const unsigned long long lo = base + (unsigned long long)ra * frame, hi = base + (unsigned long long)rb * frame;
        unsigned long long ga = (lo + 15) & ~15ull;
        if (ga > hi) ga = hi;
        unsigned long long gb = hi & ~15ull;
        if (gb < ga) gb = ga;
        const unsigned granules = (unsigned)((gb - ga) >> 4);
        // kFill loads in flight per thread (a whole tile in one trip); a thread past the end loads the last granule again
        for (unsigned g0 = threadIdx.x; g0 < granules; g0 += kFill * kThreads) {
            uint4 v[kFill];
#pragma unroll
            for (int u = 0; u < kFill; ++u) {
                const unsigned g = g0 + u * kThreads;
                v[u] = *reinterpret_cast<const uint4*>(ga + 16ull * (g < granules ? g : granules - 1));
            }
#pragma unroll
            for (int u = 0; u < kFill; ++u) {
                const unsigned g = g0 + u * kThreads;
                if (g >= granules) break;
                const unsigned q = pcm_phys((unsigned)(ga + 16ull * g - base16) >> 2);       // four dwords never cross a pad
                lds[q] = v[u].x;
                lds[q + 1] = v[u].y;
                lds[q + 2] = v[u].z;
                lds[q + 3] = v[u].w;
            }
        }
        unsigned char* image = reinterpret_cast<unsigned char*>(lds);
        const unsigned head = (unsigned)(ga - lo), tail = (unsigned)(hi - gb);      // < 16 each
        if (threadIdx.x < head + tail) {
            const unsigned long long a = threadIdx.x < head ? lo + threadIdx.x : gb + (threadIdx.x - head);
            const unsigned L = (unsigned)(a - base16);
            image[4 * pcm_phys(L >> 2) + (L & 3)] = *reinterpret_cast<const unsigned char*>(a);
        }
    }
    __syncthreads();
    const Tile part{(unsigned)(base - base16), ra, rb, frame, t0 - p.y_frame};
    if (p.aligned) decode_rows<FMT, Tout, true>(lds, p, part);
    else decode_rows<FMT, Tout, false>(lds, p, part);
}

template <int FMT>
void launch_format(const Params& p, int y_dtype, unsigned tiles, hipStream_t stream) {
    if (y_dtype) hipLaunchKernelGGL((pcm_decode_kernel<FMT, double>), dim3(tiles), dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL((pcm_decode_kernel<FMT, float>), dim3(tiles), dim3(kThreads), 0, stream, p);
}

int launch(const Params& p, int format, int y_dtype, unsigned tiles, hipStream_t stream) {
    switch (format) {
        case 0: launch_format<0>(p, y_dtype, tiles, stream); break;
        case 1: launch_format<1>(p, y_dtype, tiles, stream); break;
        case 2: launch_format<2>(p, y_dtype, tiles, stream); break;
        case 3: launch_format<3>(p, y_dtype, tiles, stream); break;
        case 4: launch_format<4>(p, y_dtype, tiles, stream); break;
        default: launch_format<5>(p, y_dtype, tiles, stream); break;
    }
    FRT_HIP_CHECK(hipGetLastError());
    return FRT_OK;
}

// rows [n_select][nf] of a decoded slab, back from the device in `slot`, into the caller's y at column `col`
int drain(PinnedSlot& slot, void* y, int n_select, long long ldy, long long col, long long nf, size_t osize) {
    if (int rc = slot.wait()) return rc;
    for (int s = 0; s < n_select; ++s)
        memcpy((char*)y + ((size_t)s * ldy + col) * osize, slot.as<char>() + (size_t)s * nf * osize, (size_t)nf * osize);
    return FRT_OK;
}

}  // namespace

extern "C" int frt_pcm_create(frt_pcm** out) {
    FRT_REQUIRE(out, "frt_pcm_create: null handle pointer");
    *out = new frt_pcm();
    return FRT_OK;
}

extern "C" void frt_pcm_destroy(frt_pcm* h) {
    if (!h) return;
    if (h->used) (void)hipStreamSynchronize(h->stream);
    for (PinnedSlot* s : {&h->in[0], &h->in[1], &h->out[0], &h->out[1]}) s->release();
    for (DeviceBuffer* b : {&h->raw, &h->rows, &h->sel}) b->release();
    const bool used = h->used;
    delete h;
    if (used) free_retired_allocations(true);
}

extern "C" int frt_pcm_set_stream(frt_pcm* h, void* s) {
    FRT_REQUIRE(h, "frt_pcm_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_pcm_tile_frames(int format, int channels) {
    FRT_REQUIRE(format >= 0 && format < kFormats, "frt_pcm_tile_frames: format %d (0 u8, 1 s16, 2 s24, 3 s32, 4 f32, 5 f64)", format);
    FRT_REQUIRE(channels >= 1 && channels <= 64, "frt_pcm_tile_frames: %d channels (1 .. 64)", channels);
    return tile_frames(format, channels);
}

extern "C" int frt_pcm_decode(frt_pcm* h, const void* data, int format, int channels, int64_t n_frames_total, int64_t first_frame,
                              int64_t n_frames, const int32_t* select, int n_select, void* y, int y_dtype, int64_t ldy, int64_t slab_bytes) {
    FRT_REQUIRE(h, "frt_pcm_decode: null handle");
    FRT_REQUIRE(format >= 0 && format < kFormats, "frt_pcm_decode: format %d (0 u8, 1 s16, 2 s24, 3 s32, 4 f32, 5 f64)", format);
    FRT_REQUIRE(y_dtype == 0 || y_dtype == 1, "frt_pcm_decode: y_dtype %d (0 float32, 1 float64)", y_dtype);
    FRT_REQUIRE(channels >= 1 && channels <= 64, "frt_pcm_decode: %d channels (1 .. 64)", channels);
    FRT_REQUIRE(n_select >= 1 && n_select <= 65535 && select, "frt_pcm_decode: %d selected channels (1 .. 65535, a host array)", n_select);
    for (int s = 0; s < n_select; ++s)
        FRT_REQUIRE(select[s] >= 0 && select[s] < channels, "frt_pcm_decode: select[%d] = %d of %d channels", s, (int)select[s], channels);
    FRT_REQUIRE(n_frames_total >= 0 && n_frames_total <= ((int64_t)1 << 50) && first_frame >= 0 && n_frames >= 0 &&
                    first_frame <= n_frames_total && n_frames <= n_frames_total - first_frame,
                "frt_pcm_decode: frames %lld .. %lld of %lld", (long long)first_frame, (long long)(first_frame + n_frames),
                (long long)n_frames_total);
    FRT_REQUIRE(ldy >= n_frames, "frt_pcm_decode: ldy %lld for %lld frames", (long long)ldy, (long long)n_frames);
    FRT_REQUIRE(slab_bytes >= 0, "frt_pcm_decode: slab_bytes %lld", (long long)slab_bytes);
    if (n_frames == 0) return FRT_OK;
    FRT_REQUIRE(data && y, "frt_pcm_decode: null buffer");
    h->used = true;
    const int W = kWidth[format], F = tile_frames(format, channels);
    const size_t frame = (size_t)channels * W, osize = y_dtype ? sizeof(double) : sizeof(float);
    const bool data_dev = is_device_pointer(data), y_dev = is_device_pointer(y);
    int rc;
    if ((rc = upload_if_changed(h->sel, h->sel_host, std::vector<int32_t>(select, select + n_select), h->stream))) return rc;
    // slabs of whole tiles; buffers that are on the device already need none
    const long long last = first_frame + n_frames, tile_a = first_frame / F, tile_b = (last + F - 1) / F;
    long long per_slab = tile_b - tile_a;
    if (!data_dev || !y_dev) {
        const size_t limit = slab_bytes ? (size_t)slab_bytes : kDefaultSlab;
        per_slab = std::max<long long>(1, std::min<long long>(per_slab, (long long)(limit / ((size_t)F * frame))));
    }
    FRT_REQUIRE(per_slab <= 0x7fffffffLL, "frt_pcm_decode: %lld tiles in one launch", per_slab);
    const size_t slab_frames = (size_t)std::min<long long>(per_slab * F, n_frames + F);       // a first slab starts inside its tile
    Params p{};
    p.last = last;
    p.select = h->sel.as<const int32_t>();
    p.n_select = n_select;
    p.C = channels;
    p.F = F;
    long long prev_col = 0, prev_nf = 0;
    int k = 0;
    for (long long t = tile_a; t < tile_b; t += per_slab, ++k) {
        const long long fa = std::max<long long>(first_frame, t * F), fb = std::min<long long>(last, (t + per_slab) * F), nf = fb - fa;
        p.first = fa;
        p.tile0 = t;
        if (data_dev) {
            p.src = (unsigned long long)(uintptr_t)data;
            p.src_frame = 0;
        } else {
            PinnedSlot& s = h->in[k & 1];
            if ((rc = s.wait())) return rc;
            if (s.grows(nf * frame)) FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
            if ((rc = s.reserve(nf * frame, slab_frames * frame))) return rc;
            if ((rc = h->raw.reserve(slab_frames * frame))) return rc;
            memcpy(s.ptr, (const char*)data + (size_t)fa * frame, nf * frame);       // while the slab before is on its way
            FRT_HIP_CHECK(hipMemcpyAsync(h->raw.ptr, s.ptr, nf * frame, hipMemcpyHostToDevice, h->stream));
            if ((rc = s.mark(h->stream))) return rc;
            p.src = (unsigned long long)(uintptr_t)h->raw.ptr;
            p.src_frame = fa;
        }
        p.aligned = p.src % (W == 3 ? 1 : W) == 0;
        if (y_dev) {
            p.y = y;
            p.ldy = ldy;
            p.y_frame = first_frame;
        } else {
            if ((rc = h->rows.reserve((size_t)n_select * slab_frames * osize))) return rc;
            p.y = h->rows.ptr;
            p.ldy = nf;
            p.y_frame = fa;
        }
        if ((rc = launch(p, format, y_dtype, (unsigned)std::min<long long>(per_slab, tile_b - t), h->stream))) return rc;
        if (!y_dev) {
            PinnedSlot& o = h->out[k & 1];                 // drained one slab ago
            const size_t bytes = (size_t)n_select * nf * osize;
            if (o.grows(bytes)) FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
            if ((rc = o.reserve(bytes, (size_t)n_select * slab_frames * osize))) return rc;
            FRT_HIP_CHECK(hipMemcpyAsync(o.ptr, h->rows.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
            if ((rc = o.mark(h->stream))) return rc;
            if (k > 0 && (rc = drain(h->out[(k - 1) & 1], y, n_select, ldy, prev_col, prev_nf, osize))) return rc;
            prev_col = fa - first_frame;
            prev_nf = nf;
        }
    }
    if (!y_dev && (rc = drain(h->out[(k - 1) & 1], y, n_select, ldy, prev_col, prev_nf, osize))) return rc;
    FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    for (PinnedSlot* s : {&h->in[0], &h->in[1], &h->out[0], &h->out[1]}) s->forget();
    return FRT_OK;
}
