// pcmenc.hip — PCM export: the planar float rows of the chains to interleaved integer / float PCM (frt_pcmenc_*; the definition:
// include/friture_hip.h, R3).  The mirror of pcm.hip.
//
// A workgroup takes one tile of F = frt_pcm_tile_frames(format, channels) frames, tiles counted from frame 0 of the output:
// F * C * width is a multiple of 16, so every tile starts at the destination's own address mod 16.  Phase 1: a wavefront per 64
// consecutive frames of one output channel, lane i on frame i of row route[c] — 256 or 512 contiguous bytes per load, kItems of
// them in flight per lane; every row element is read once per channel that carries it.  The lane quantises its sample and
// writes its `width` bytes into an LDS image of the tile's interleaved bytes.  The image keeps the address mod 16 (byte A of the
// destination sits at logical byte A - base16, base16 the tile's start rounded down to 16), and logical dword D is stored at
//
//     pcmenc_phys(D) = D + (D >> 5) + (D >> 10)
//
// pcm.hip's pads, for pcm.hip's reason with the two sides exchanged: the writes run at lane stride C * width bytes, which for a
// frame of 128 B, 256 B or any other power of two would put a lane group on one bank, and the pads step a bank per 32 (per
// 1024) dwords; the reads of phase 2 are four consecutive dwords per thread at a 16-byte lane stride, which the pad behind every
// 32 dwords spreads over all 32 banks (the degrees per format and channel count: tools/exp/lds_layout_model.py pcm_encode,
// DESIGN.md R3).  A sample is written at its natural width where the destination's address is a multiple of min(width, 4), an
// s24 sample as a 16-bit store at the even address of its three bytes and a byte store at the other end, any other sample byte
// by byte: no LDS access is off its natural alignment for any address of the destination.
// Phase 2, after the barrier: the image leaves as aligned 16-byte stores, consecutive threads on consecutive granules; the
// partial granules at the two ends of the tile's range leave byte by byte: no byte outside the requested frames is written.
//
// The clip counts: one ballot per 64 samples, summed in a scalar while the wavefront stays on one channel, then one LDS atomicAdd
// per wavefront and channel into the workgroup's counters, and after the barrier one global atomicAdd per workgroup and channel
// (none for a count of zero) into row blockIdx mod kClipSlots of a [kClipSlots][64] table that the host sums: with one global
// atomic per wavefront and channel on a single [channels] row, 0.1 % of clipped samples made the adds on 2 (8) addresses the
// whole of the kernel's time.
#include "common.h"

#include <algorithm>

struct frt_pcmenc {
    hipStream_t stream = nullptr;
    frt::PinnedSlot in[2], out[2];          // row slabs on their way up, encoded slabs on their way back
    frt::PinnedBuffer counts;
    frt::DeviceBuffer rows, bytes, route, clip;
    std::vector<int32_t> route_host;
    bool used = false;                      // an encode got as far as the device: destroying an unused handle makes no device call
};

namespace {

using namespace frt;

constexpr int kFormats = 6;
constexpr int kWidth[kFormats] = {1, 2, 3, 4, 4, 8};
constexpr int kBits[kFormats] = {8, 16, 24, 32, 0, 0};
constexpr int kMaxChannels = 64;
constexpr int kTileBytes = 32768;                         // encoded bytes of a tile at most: frt_pcm_tile_frames' budget
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kItems = 8;                                 // row loads in flight per lane while the image is filled
constexpr int kDrain = 4;                                 // granules in flight per thread while the image leaves
constexpr size_t kDefaultSlab = (size_t)64 << 20;
constexpr long long kMaxFrames = 1ll << 50;
constexpr int kClipSlots = 16;                            // rows of the clip-count table: consecutive workgroups add to different rows
constexpr size_t kClipBytes = (size_t)kClipSlots * kMaxChannels * sizeof(unsigned long long);

__host__ __device__ constexpr unsigned pcmenc_phys(unsigned D) { return D + (D >> 5) + (D >> 10); }
// logical bytes: up to 15 in front of the tile, then the tile
constexpr unsigned kLdsDwords = pcmenc_phys((15 + kTileBytes) / 4 + 1) + 1;

struct Params {
    const void* x;               // row r, frame f of the call at x[r * ldx + f - x_frame]
    long long ldx, x_frame;
    unsigned long long dst;      // address of the first byte of frame dst_frame, a multiple of F
    long long dst_frame;
    long long last;              // the call encodes frames [0, last)
    long long tile0;             // the tile of block 0
    long long frame0;            // absolute index of the call's frame 0: the dither counter
    unsigned long long seed;
    const int32_t* route;
    unsigned long long* clipped; // [kClipSlots][kMaxChannels]
    int C, F, aligned, player;
};

// Philox4x32-10 on counter (f lo, f hi, c, 0) and key (seed lo, seed hi); d = ((o0 >> 8) - (o1 >> 8)) 2^-24: triangular on (-1, 1)
__device__ inline double dither_lsb(unsigned long long f, unsigned c, unsigned long long seed) {
    unsigned c0 = (unsigned)f, c1 = (unsigned)(f >> 32), c2 = c, c3 = 0, k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (double)((int)(c0 >> 8) - (int)(c1 >> 8)) * 0x1p-24;
}

// the stored bytes of one sample, little-endian, in lo (and hi for f64); clip: the rounded value lay outside the range or was NaN
template <int FMT, typename Tin, bool DITHER>
__device__ inline void encode_value(Tin v, double d, bool player, unsigned& lo, unsigned& hi, bool& clip) {
    hi = 0;
    clip = false;
    if constexpr (FMT == 4) {
        lo = __float_as_uint((float)v);                     // float32: the bits; float64: one round-to-nearest-even
    } else if constexpr (FMT == 5) {
        const unsigned long long b = (unsigned long long)__double_as_longlong((double)v);
        lo = (unsigned)b;
        hi = (unsigned)(b >> 32);
    } else {
        constexpr int B = kBits[FMT];
        constexpr double full = (double)(1ll << (B - 1));
        const double w = (double)v;
        int q;
        if (FMT == 1 && player) {                           // friture/playback/player.py:173-177
            const double c = fmin(fmax(w, -1.0), 1.0);      // of a NaN: -1.0, replaced below
            clip = !(w == c);
            q = w != w ? 0 : (int)(32767.0 * c);
        } else {
            const double t = w * full;                      // exact
            const double r = rint(DITHER ? t + d : t);
            const double c = fmin(fmax(r, -full), full - 1.0);
            clip = !(r == c);
            q = r != r ? 0 : (int)c;
        }
        lo = FMT == 0 ? (unsigned)(q + 128) & 0xffu : FMT == 1 ? (unsigned)q & 0xffffu : FMT == 2 ? (unsigned)q & 0xffffffu : (unsigned)q;
    }
}

// the W bytes of a sample to logical byte L of the image
template <int W, bool ALIGNED>
__device__ inline void put(unsigned* lds, unsigned L, unsigned lo, unsigned hi) {
    unsigned char* image = reinterpret_cast<unsigned char*>(lds);
    const unsigned D = L >> 2;
    if (W == 1) {
        image[4 * pcmenc_phys(D) + (L & 3)] = (unsigned char)lo;
    } else if (W == 2 && ALIGNED) {
        *reinterpret_cast<unsigned short*>(image + 4 * pcmenc_phys(D) + (L & 3)) = (unsigned short)lo;
    } else if (W == 3) {                                    // a 16-bit store at the even address of the three, a byte at the other end
        const unsigned odd = L & 1, a16 = L + odd, a8 = L + 2 - 2 * odd;
        *reinterpret_cast<unsigned short*>(image + 4 * pcmenc_phys(a16 >> 2) + (a16 & 3)) = (unsigned short)(lo >> (8 * odd));
        image[4 * pcmenc_phys(a8 >> 2) + (a8 & 3)] = (unsigned char)(odd ? lo : lo >> 16);
    } else if (W == 4 && ALIGNED) {
        lds[pcmenc_phys(D)] = lo;
    } else if (W == 8 && ALIGNED) {
        lds[pcmenc_phys(D)] = lo;
        lds[pcmenc_phys(D + 1)] = hi;
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const unsigned a = L + i;
            image[4 * pcmenc_phys(a >> 2) + (a & 3)] = (unsigned char)((i < 4 ? lo : hi) >> (8 * (i & 3)));
        }
    }
}

// A wavefront per 64 frames of an output channel, the wavefronts of the workgroup on consecutive chunks of it: item `it` is chunk
// it mod chunks of channel it / chunks, kept as the pair (c, k) and stepped without a division.  Everything about an item but
// the lane is wave-uniform, and said to be: channel, row (a scalar load), the row's address and the image's are scalar.  kItems
// items per trip — their rows looked up first, then every global load, then the LDS writes — and the items left over one by
// one.  A frame past the tile's range loads its last frame and is neither written nor counted; a silent channel (row -1) loads
// nothing.
template <int FMT, typename Tin, bool DITHER, bool ALIGNED>
struct RowEncoder {
    static constexpr int W = kWidth[FMT];
    unsigned* lds;
    unsigned* block_clip;                  // [channels] in LDS, zeroed before the first wavefront arrives
    const Params& p;
    const Tin* x;                          // of the tile's frame 0 in row 0
    unsigned rb, chunks, lane, lane_byte, image0, count = 0, count_c = 0;
    unsigned long long frame_abs;          // absolute index of the tile's frame 0

    struct Item { unsigned c, k; };
    __device__ void step(Item& s, unsigned n) const {
        s.k += n;
        while (s.k >= chunks) {
            s.k -= chunks;
            ++s.c;
        }
    }
    __device__ Tin load_row(const Item& s, int row) const {             // row >= 0
        const unsigned r0 = s.k << 6, off = lane < rb - 1 - r0 ? lane : rb - 1 - r0;
        return x[(long long)row * p.ldx + r0 + off];
    }
    __device__ Tin load(const Item& s, int row) const { return row < 0 ? (Tin)0 : load_row(s, row); }
    __device__ void flush() {
        if (lane == 0 && count) atomicAdd(&block_clip[count_c], count);
        count = 0;
    }
    __device__ void finish(const Item& s, int row, Tin v) {
        const unsigned r0 = s.k << 6;
        const bool live = r0 + lane < rb;
        double d = 0.0;
        if (DITHER && row >= 0) d = dither_lsb(frame_abs + r0 + lane, s.c, p.seed);
        unsigned lo, hi;
        bool clip;
        encode_value<FMT, Tin, DITHER>(v, d, p.player != 0, lo, hi, clip);
        if (live) put<W, ALIGNED>(lds, image0 + r0 * ((unsigned)p.C * W) + s.c * W + lane_byte, lo, hi);
        if (FMT < 4 && row >= 0) {
            if (s.c != count_c) {
                flush();
                count_c = s.c;
            }
            count += (unsigned)__popcll(__ballot(live && clip));
        }
    }
    __device__ void run(unsigned wave, unsigned items) {
        Item s{0, 0};
        step(s, wave);
        unsigned it = wave;
        for (; it + (kItems - 1) * kWaves < items; it += kItems * kWaves) {
            Tin v[kItems];
            Item at[kItems];
            int row[kItems];
#pragma unroll
            for (int u = 0; u < kItems; ++u) {
                at[u] = s;
                row[u] = p.route[s.c];
                step(s, kWaves);
            }
            // a trip without a silent channel issues its loads back to back; the branch around a silent channel's load would
            // otherwise put a wait behind every one of them
            bool silent = false;
#pragma unroll
            for (int u = 0; u < kItems; ++u) silent |= row[u] < 0;
            if (!silent) {
#pragma unroll
                for (int u = 0; u < kItems; ++u) v[u] = load_row(at[u], row[u]);
            } else {
#pragma unroll
                for (int u = 0; u < kItems; ++u) v[u] = load(at[u], row[u]);
            }
#pragma unroll
            for (int u = 0; u < kItems; ++u) finish(at[u], row[u], v[u]);
        }
        for (; it < items; it += kWaves) {
            const int row = p.route[s.c];
            finish(s, row, load(s, row));
            step(s, kWaves);
        }
        if (FMT < 4) flush();
    }
};

template <int FMT, typename Tin, bool DITHER>
__global__ __launch_bounds__(kThreads) void pcm_encode_kernel(Params p) {
    constexpr int W = kWidth[FMT];
    __shared__ __align__(16) unsigned lds[kLdsDwords];
    __shared__ unsigned block_clip[kMaxChannels];
    const long long tile = p.tile0 + blockIdx.x, t0 = tile * p.F;
    const long long fb = t0 + p.F < p.last ? t0 + p.F : p.last;
    if (t0 >= fb) return;
    const unsigned frame = (unsigned)p.C * W, rb = (unsigned)(fb - t0);
    const unsigned long long base = p.dst + (unsigned long long)((t0 - p.dst_frame) * (long long)frame);
    const unsigned long long base16 = base & ~15ull;
    if (FMT < 4) {
        if (threadIdx.x < kMaxChannels) block_clip[threadIdx.x] = 0;
        __syncthreads();
    }
    {
        const unsigned lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), chunks = (rb + 63) >> 6;
        const Tin* x = reinterpret_cast<const Tin*>(p.x) + (t0 - p.x_frame);
        const unsigned long long frame_abs = (unsigned long long)(p.frame0 + t0);
        if (p.aligned) RowEncoder<FMT, Tin, DITHER, true>{lds, block_clip, p, x, rb, chunks, lane, lane * frame, (unsigned)(base - base16), 0, 0, frame_abs}.run(wave, chunks * (unsigned)p.C);
        else RowEncoder<FMT, Tin, DITHER, false>{lds, block_clip, p, x, rb, chunks, lane, lane * frame, (unsigned)(base - base16), 0, 0, frame_abs}.run(wave, chunks * (unsigned)p.C);
    }
    __syncthreads();
    if (FMT < 4 && threadIdx.x < (unsigned)p.C && block_clip[threadIdx.x])
        atomicAdd(&p.clipped[(blockIdx.x % kClipSlots) * kMaxChannels + threadIdx.x], (unsigned long long)block_clip[threadIdx.x]);
    // the bytes [lo, hi) of the tile's frames: whole 16-byte granules inside them, the ends byte by byte
    const unsigned long long lo = base, hi = base + (unsigned long long)rb * frame;
    unsigned long long ga = (lo + 15) & ~15ull;
    if (ga > hi) ga = hi;
    unsigned long long gb = hi & ~15ull;
    if (gb < ga) gb = ga;
    const unsigned granules = (unsigned)((gb - ga) >> 4);
    for (unsigned g0 = threadIdx.x; g0 < granules; g0 += kDrain * kThreads) {
        uint4 v[kDrain];
#pragma unroll
        for (int u = 0; u < kDrain; ++u) {
            const unsigned g = g0 + u * kThreads < granules ? g0 + u * kThreads : granules - 1;
            const unsigned q = pcmenc_phys((unsigned)(ga + 16ull * g - base16) >> 2);       // four dwords never cross a pad
            v[u] = make_uint4(lds[q], lds[q + 1], lds[q + 2], lds[q + 3]);
        }
#pragma unroll
        for (int u = 0; u < kDrain; ++u) {
            const unsigned g = g0 + u * kThreads;
            if (g >= granules) break;
            *reinterpret_cast<uint4*>(ga + 16ull * g) = v[u];
        }
    }
    const unsigned char* image = reinterpret_cast<const unsigned char*>(lds);
    const unsigned head = (unsigned)(ga - lo), tail = (unsigned)(hi - gb);      // < 16 each
    if (threadIdx.x < head + tail) {
        const unsigned long long a = threadIdx.x < head ? lo + threadIdx.x : gb + (threadIdx.x - head);
        const unsigned L = (unsigned)(a - base16);
        *reinterpret_cast<unsigned char*>(a) = image[4 * pcmenc_phys(L >> 2) + (L & 3)];
    }
}

template <int FMT, bool DITHER>
void launch_format(const Params& p, int x_dtype, unsigned tiles, hipStream_t stream) {
    if (x_dtype) hipLaunchKernelGGL((pcm_encode_kernel<FMT, double, DITHER>), dim3(tiles), dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL((pcm_encode_kernel<FMT, float, DITHER>), dim3(tiles), dim3(kThreads), 0, stream, p);
}

int launch(const Params& p, int format, int x_dtype, bool dither, unsigned tiles, hipStream_t stream) {
    switch (format) {
        case 0: dither ? launch_format<0, true>(p, x_dtype, tiles, stream) : launch_format<0, false>(p, x_dtype, tiles, stream); break;
        case 1: dither ? launch_format<1, true>(p, x_dtype, tiles, stream) : launch_format<1, false>(p, x_dtype, tiles, stream); break;
        case 2: dither ? launch_format<2, true>(p, x_dtype, tiles, stream) : launch_format<2, false>(p, x_dtype, tiles, stream); break;
        case 3: dither ? launch_format<3, true>(p, x_dtype, tiles, stream) : launch_format<3, false>(p, x_dtype, tiles, stream); break;
        case 4: launch_format<4, false>(p, x_dtype, tiles, stream); break;
        default: launch_format<5, false>(p, x_dtype, tiles, stream); break;
    }
    FRT_HIP_CHECK(hipGetLastError());
    return FRT_OK;
}

// the bytes of an encoded slab, back from the device in `slot`, into the caller's dst at byte `at`
int drain(PinnedSlot& slot, void* dst, size_t at, size_t bytes) {
    if (int rc = slot.wait()) return rc;
    memcpy((char*)dst + at, slot.ptr, bytes);
    return FRT_OK;
}

}  // namespace

extern "C" int frt_pcmenc_create(frt_pcmenc** out) {
    FRT_REQUIRE(out, "frt_pcmenc_create: null handle pointer");
    *out = new frt_pcmenc();
    return FRT_OK;
}

extern "C" void frt_pcmenc_destroy(frt_pcmenc* h) {
    if (!h) return;
    if (h->used) (void)hipStreamSynchronize(h->stream);
    for (PinnedSlot* s : {&h->in[0], &h->in[1], &h->out[0], &h->out[1]}) s->release();
    h->counts.release();
    for (DeviceBuffer* b : {&h->rows, &h->bytes, &h->route, &h->clip}) b->release();
    const bool used = h->used;
    delete h;
    if (used) free_retired_allocations(true);
}

extern "C" int frt_pcmenc_set_stream(frt_pcmenc* h, void* s) {
    FRT_REQUIRE(h, "frt_pcmenc_set_stream: null handle");
    h->stream = (hipStream_t)s;
    return FRT_OK;
}

extern "C" int frt_pcmenc_encode(frt_pcmenc* h, const void* x, int x_dtype, int n_rows, int64_t ldx, int64_t n_frames, int64_t frame0,
                                 const int32_t* route, int channels, int format, int mode, int dither, uint64_t seed, void* dst,
                                 int64_t* clipped, int64_t slab_bytes) {
    FRT_REQUIRE(h, "frt_pcmenc_encode: null handle");
    FRT_REQUIRE(format >= 0 && format < kFormats, "frt_pcmenc_encode: format %d (0 u8, 1 s16, 2 s24, 3 s32, 4 f32, 5 f64)", format);
    FRT_REQUIRE(x_dtype == 0 || x_dtype == 1, "frt_pcmenc_encode: x_dtype %d (0 float32, 1 float64)", x_dtype);
    FRT_REQUIRE(mode == 0 || mode == 1, "frt_pcmenc_encode: mode %d (0 nearest, 1 player)", mode);
    FRT_REQUIRE(dither == 0 || dither == 1, "frt_pcmenc_encode: dither %d (0 or 1)", dither);
    FRT_REQUIRE(channels >= 1 && channels <= kMaxChannels, "frt_pcmenc_encode: %d channels (1 .. 64)", channels);
    FRT_REQUIRE(n_rows >= 1 && n_rows <= 65535, "frt_pcmenc_encode: %d rows (1 .. 65535)", n_rows);
    FRT_REQUIRE(route, "frt_pcmenc_encode: null route (a host array of `channels` row indices)");
    for (int c = 0; c < channels; ++c)
        FRT_REQUIRE(route[c] >= -1 && route[c] < n_rows, "frt_pcmenc_encode: route[%d] = %d of %d rows (-1: silence)", c, (int)route[c], n_rows);
    FRT_REQUIRE(n_frames >= 0 && frame0 >= 0 && frame0 <= kMaxFrames && n_frames <= kMaxFrames - frame0,
                "frt_pcmenc_encode: frames %lld .. %lld (0 .. 2^50)", (long long)frame0, (long long)frame0 + (long long)n_frames);
    FRT_REQUIRE(ldx >= n_frames, "frt_pcmenc_encode: ldx %lld for %lld frames", (long long)ldx, (long long)n_frames);
    FRT_REQUIRE(slab_bytes >= 0, "frt_pcmenc_encode: slab_bytes %lld", (long long)slab_bytes);
    FRT_REQUIRE(mode == 0 || (format == 1 && !dither), "frt_pcmenc_encode: mode 1 (player) is for s16 without dither, got format %d, dither %d",
                format, dither);
    FRT_REQUIRE(!dither || format < 4, "frt_pcmenc_encode: dither with the float format %d", format);
    if (n_frames == 0) return FRT_OK;
    FRT_REQUIRE(x && dst, "frt_pcmenc_encode: null buffer");
    h->used = true;
    const int W = kWidth[format], F = kTileBytes / (channels * W) / 64 * 64;
    const size_t frame = (size_t)channels * W, isize = x_dtype ? sizeof(double) : sizeof(float);
    const bool x_dev = is_device_pointer(x), d_dev = is_device_pointer(dst);
    int rc;
    // a host x goes up as the rows the route names, once each: the device's route then counts those
    std::vector<int32_t> rt(route, route + channels), staged;
    if (!x_dev) {
        std::vector<int32_t> slot_of(n_rows, -1);
        for (int32_t& r : rt) {
            if (r < 0) continue;
            if (slot_of[r] < 0) {
                slot_of[r] = (int32_t)staged.size();
                staged.push_back(r);
            }
            r = slot_of[r];
        }
    }
    if ((rc = upload_if_changed(h->route, h->route_host, rt, h->stream))) return rc;
    if ((rc = h->clip.reserve(kClipBytes))) return rc;
    if (format < 4) FRT_HIP_CHECK(hipMemsetAsync(h->clip.ptr, 0, kClipBytes, h->stream));      // the float formats count nothing
    // slabs of whole tiles; buffers that are on the device already need none
    const long long tiles = (n_frames + F - 1) / F;
    long long per_slab = tiles;
    if (!x_dev || !d_dev) {
        const size_t limit = slab_bytes ? (size_t)slab_bytes : kDefaultSlab;
        per_slab = std::max<long long>(1, std::min<long long>(per_slab, (long long)(limit / ((size_t)F * frame))));
    }
    FRT_REQUIRE(per_slab <= 0x7fffffffLL, "frt_pcmenc_encode: %lld tiles in one launch", per_slab);
    const size_t slab_frames = (size_t)std::min<long long>(per_slab * F, n_frames);
    Params p{};
    p.last = n_frames;
    p.frame0 = frame0;
    p.seed = seed;
    p.route = h->route.as<const int32_t>();
    p.clipped = h->clip.as<unsigned long long>();
    p.C = channels;
    p.F = F;
    p.player = mode;
    long long prev_fa = 0, prev_nf = 0;
    int k = 0;
    for (long long t = 0; t < tiles; t += per_slab, ++k) {
        const long long fa = t * F, fb = std::min<long long>(n_frames, (t + per_slab) * F), nf = fb - fa;
        p.tile0 = t;
        if (x_dev) {
            p.x = x;
            p.ldx = ldx;
            p.x_frame = 0;
        } else {
            PinnedSlot& s = h->in[k & 1];
            const size_t need = staged.size() * (size_t)nf * isize, most = staged.size() * slab_frames * isize;
            if (need) {
                if ((rc = s.wait())) return rc;
                if (s.grows(need)) FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
                if ((rc = s.reserve(need, most))) return rc;
                if ((rc = h->rows.reserve(most))) return rc;
                for (size_t j = 0; j < staged.size(); ++j)                  // while the slab before is on its way
                    memcpy(s.as<char>() + j * (size_t)nf * isize, (const char*)x + ((size_t)staged[j] * ldx + fa) * isize, (size_t)nf * isize);
                FRT_HIP_CHECK(hipMemcpyAsync(h->rows.ptr, s.ptr, need, hipMemcpyHostToDevice, h->stream));
                if ((rc = s.mark(h->stream))) return rc;
            }
            p.x = h->rows.ptr;               // every channel silent: never read
            p.ldx = nf;
            p.x_frame = fa;
        }
        if (d_dev) {
            p.dst = (unsigned long long)(uintptr_t)dst;
            p.dst_frame = 0;
        } else {
            if ((rc = h->bytes.reserve(slab_frames * frame))) return rc;
            p.dst = (unsigned long long)(uintptr_t)h->bytes.ptr;
            p.dst_frame = fa;
        }
        p.aligned = W != 3 && p.dst % (W < 4 ? W : 4) == 0;          // every tile starts at p.dst's address mod 16
        if ((rc = launch(p, format, x_dtype, dither != 0, (unsigned)std::min<long long>(per_slab, tiles - t), h->stream))) return rc;
        if (!d_dev) {
            PinnedSlot& o = h->out[k & 1];                 // drained one slab ago
            const size_t bytes = (size_t)nf * frame;
            if (o.grows(bytes)) FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
            if ((rc = o.reserve(bytes, slab_frames * frame))) return rc;
            FRT_HIP_CHECK(hipMemcpyAsync(o.ptr, h->bytes.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
            if ((rc = o.mark(h->stream))) return rc;
            if (k > 0 && (rc = drain(h->out[(k - 1) & 1], dst, (size_t)prev_fa * frame, (size_t)prev_nf * frame))) return rc;
            prev_fa = fa;
            prev_nf = nf;
        }
    }
    if (h->counts.grows(kClipBytes)) FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    if ((rc = h->counts.reserve(kClipBytes, kClipBytes))) return rc;
    if (format < 4) FRT_HIP_CHECK(hipMemcpyAsync(h->counts.ptr, h->clip.ptr, kClipBytes, hipMemcpyDeviceToHost, h->stream));
    if (!d_dev && (rc = drain(h->out[(k - 1) & 1], dst, (size_t)prev_fa * frame, (size_t)prev_nf * frame))) return rc;
    FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    for (PinnedSlot* s : {&h->in[0], &h->in[1], &h->out[0], &h->out[1]}) s->forget();
    if (clipped && format < 4)
        for (int slot = 0; slot < kClipSlots; ++slot)
            for (int c = 0; c < channels; ++c) clipped[c] += (int64_t)h->counts.as<unsigned long long>()[slot * kMaxChannels + c];
    return FRT_OK;
}
