// octspecbatch.hip — the octave-spectrum widget's chain over whole recordings (OctaveSpectrum_Widget.handle_new_data,
// friture/octavespectrum.py:91-122) for gfx950: Octave_Filters.filter, per-band exponential smoothing of y^2 and
// 10 log10(sp + 1e-30) + weighting at every refresh of S widgets fed chunk by chunk.  float64 throughout; built with
// -ffp-contract=off.
//
//   bank     frt_ola_filter_batch (ola.hip, K3) over the consumed samples with energy blocks of 256 = 2^(kNOctave - 1) input
//            samples: band k of stage j gets the zero-state energy E_b = alpha sum_i (1 - alpha)^(m-1-i) y_i^2 of its
//            m = 256 >> j samples of sub-block b.  A widget's chunk of 256 c samples (c = 1..4) is c whole sub-blocks at every
//            stage, so the reference's per-chunk decimation y[:N:2] lies on one uniform grid.
//   walk     sp_b = E_b + sp_(b-1) (1 - alpha)^m over the sub-blocks (exp_smoothing.py:52-54 holds for any partition of the
//            samples into consecutive blocks), emitting sp and / or dB at the sub-blocks that end a refresh.  A thread is one
//            band of one stream, consecutive threads consecutive bands: its loads of [sub-block][band] and its stores of
//            [refresh][band] are contiguous over the wavefront.  The walk is sequential in time, so from 4 x 64 sub-blocks on
//            it is split: octspec_local_kernel leaves the zero-carry end value of every run of 64 sub-blocks,
//            octspec_walk_kernel chains the runs in front of its own (a few dozen steps) and walks its run from that carry.
//            Shorter inputs are one launch of octspec_walk_kernel, one run per stream.  Which sub-block ends which refresh
//            comes from the device form of the caller's table of ends: row_of[b] = the output row, or -1.
//   slabs    The block energies ([streams][n / 256][bands] doubles), the bank's stage signals and the staged samples grow with
//            n: a call walks the recording in time slabs of whole refreshes under the caller's scratch budget; the bank's
//            tails (in the handle) and sp (two small buffers taking turns) carry from slab to slab.  Scratch is the handle's own
//            staging and plan buffers, which hold nothing between calls: xin the staged samples, eblock / eseg the block
//            energies and the runs' ends, eout the call's tables, ypacked sp between two slabs.
#include <cmath>

#include "octbank.h"

namespace frt {
namespace {

constexpr int kOsBlock = 1 << (kNOctave - 1);     // input samples per sub-block
constexpr int kOsSplit = 64;                      // sub-blocks per run of the two-level walk (energy_local_kernel's, iir.hip)
constexpr int kOsBatch = 8;                       // values a thread requests per trip: the next trip's before this trip's are used
static_assert(kOsSplit % kOsBatch == 0, "a run is walked in whole trips");

// end[c][run][band]: the last value of sp over run `run` from a zero carry (the last run's is never needed: not launched)
__global__ void __launch_bounds__(256) octspec_local_kernel(const double* __restrict__ eblock, const double* __restrict__ decay,
                                                            double* __restrict__ end, int nb, int nbands) {
    const int band = threadIdx.x, run = blockIdx.x, c = blockIdx.y, nruns = gridDim.x;
    if (band >= nbands) return;
    const double d = decay[band];
    const double* p = eblock + ((size_t)c * nb + (size_t)run * kOsSplit) * nbands + band;      // a whole run: nruns = full runs only
    double nx[kOsBatch], local = 0.0;
#pragma unroll
    for (int j = 0; j < kOsBatch; ++j) nx[j] = p[(size_t)j * nbands];
#pragma unroll                                                   // straight-line: as a loop the requests end up behind the steps and are waited for at once
    for (int i = 0; i < kOsSplit; i += kOsBatch) {
        double e[kOsBatch];
#pragma unroll
        for (int j = 0; j < kOsBatch; ++j) e[j] = nx[j];
        if (i + kOsBatch < kOsSplit) {
#pragma unroll
            for (int j = 0; j < kOsBatch; ++j) nx[j] = p[(size_t)(i + kOsBatch + j) * nbands];
        }
#pragma unroll
        for (int j = 0; j < kOsBatch; ++j) local = e[j] + local * d;
    }
    end[((size_t)c * nruns + run) * nbands + band] = local;
}

struct OsWalk {
    const double* eblock;      // [C][nb][nbands]
    const double* decay;       // [nbands] (1 - alpha)^m
    const double* weight;      // [nbands] dB or null
    const int* row_of;         // [nb] output row of the refresh a sub-block ends, -1: none
    const double* end;         // [C][nruns - 1][nbands] of octspec_local_kernel (nruns > 1)
    const double* sp_in;       // [C][nbands]
    double* sp_out;            // [C][nbands], not sp_in
    double* db;                // [C][rows][nbands]
    double* energy;            // the same shape or null
    int nb, nb_held, nbands, run_len;   // nb_held: sub-blocks per stream in eblock (nb, but see frt_octspec_run)
    long long rows;
};

// row_of is wave-uniform and written before the launch: read through the constant address space, its entries come through the
// scalar cache and are waited for where they are used (as a global load the compiler moves each one to a scalar register
// right behind its request, which serialises the trip's loads)
typedef const int __attribute__((address_space(4))) * os_rows;

// DB / EN are instances, not branches: a float64 log10 between the steps of an instance that does not want it costs its
// instruction-cache lines (energy_finish_kernel, iir.hip).
template <bool DB, bool EN>
__global__ void __launch_bounds__(256) octspec_walk_kernel(const OsWalk a) {
    const int band = threadIdx.x, run = blockIdx.x, c = blockIdx.y, nruns = gridDim.x;
    if (band >= a.nbands) return;
    const int nbands = a.nbands;
    const int b0 = run * a.run_len, count = (a.nb - b0) < a.run_len ? (a.nb - b0) : a.run_len;
    const double d = a.decay[band];
    const double w = (DB && a.weight) ? a.weight[band] : 0.0;
    const double* p = a.eblock + ((size_t)c * a.nb_held + b0) * nbands + band;
    const os_rows rp = (os_rows)(uintptr_t)(a.row_of + b0);
    double nx[kOsBatch];                                         // the run's first values travel while the chain is formed
    int nr[kOsBatch];
    auto request = [&](int i) {                                  // branch-free: an entry past the run's end re-reads its last one
#pragma unroll
        for (int j = 0; j < kOsBatch; ++j) {
            const int at = i + j < count ? i + j : count - 1;
            nx[j] = p[(size_t)at * nbands];
            nr[j] = rp[at];
        }
    };
    request(0);
    double sp = a.sp_in[(size_t)c * nbands + band];
    if (run > 0) {                                               // every run in front of this one is whole: sp = end_g + sp d^run_len
        double dlen = 1.0;
        for (int i = 0; i < a.run_len; ++i) dlen *= d;
        const double* se = a.end + (size_t)c * (nruns - 1) * nbands + band;
        for (int g = 0; g < run; g += kOsBatch) {
            double e[kOsBatch];
#pragma unroll
            for (int j = 0; j < kOsBatch; ++j) e[j] = se[(size_t)(g + j < run ? g + j : run - 1) * nbands];
#pragma unroll
            for (int j = 0; j < kOsBatch; ++j)
                if (g + j < run) sp = e[j] + sp * dlen;
        }
    }
    const size_t obase = (size_t)c * a.rows * nbands + band;
    for (int i = 0; i < count; i += kOsBatch) {
        double e[kOsBatch];
        int r[kOsBatch];
#pragma unroll
        for (int j = 0; j < kOsBatch; ++j) {
            e[j] = nx[j];
            r[j] = nr[j];
        }
        if (i + kOsBatch < count) request(i + kOsBatch);
        asm volatile("" ::: "memory");                           // the next trip's requests stay in front of this trip's stores
#pragma unroll
        for (int j = 0; j < kOsBatch; ++j) {
            if (i + j < count) {
                sp = e[j] + sp * d;
                if (r[j] >= 0) {                                 // wave-uniform: the sub-block ends a refresh
                    const size_t o = obase + (size_t)r[j] * nbands;
                    if (EN) a.energy[o] = sp;
                    if (DB) a.db[o] = 10.0 * log10(sp + 1e-30) + w;
                }
            }
        }
    }
    if (run == nruns - 1) a.sp_out[(size_t)c * nbands + band] = sp;
}

// user [C][9][nfilt][511] <-> handle [9][C][nfilt][511]
__global__ void __launch_bounds__(256) octspec_tails_kernel(double* __restrict__ user, double* __restrict__ held, int C, int per_stage,
                                                            int to_user) {
    const size_t total = (size_t)kNOctave * C * per_stage;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;             // index in the user's layout
    if (i >= total) return;
    const size_t c = i / ((size_t)kNOctave * per_stage), rest = i - c * kNOctave * per_stage;
    const size_t j = rest / per_stage, e = rest - j * per_stage;
    const size_t hi = (j * C + c) * per_stage + e;
    if (to_user) user[i] = held[hi];
    else held[hi] = user[i];
}

int tails_copy(frt_octbank* h, double* user, bool to_user, const char* who) {
    FRT_REQUIRE(h && h->mode == 1 && h->ola && user, "%s: needs a mode-1 handle and a buffer", who);
    const int per_stage = h->nfilt * kTail;
    const size_t total = (size_t)kNOctave * h->n_channels * per_stage, bytes = total * sizeof(double);
    const bool dev = is_device_pointer(user);
    double* d_user = user;
    if (!dev) {
        int rc = h->xin.reserve(bytes);
        if (rc) return rc;
        d_user = h->xin.as<double>();
        if (!to_user) FRT_HIP_CHECK(hipMemcpyAsync(d_user, user, bytes, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(octspec_tails_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, d_user,
                       h->ola->pending.as<double>(), h->n_channels, per_stage, (int)to_user);
    FRT_HIP_CHECK(hipGetLastError());
    if (!dev) {
        if (to_user) FRT_HIP_CHECK(hipMemcpyAsync(user, d_user, bytes, hipMemcpyDeviceToHost, h->stream));
        FRT_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    return FRT_OK;
}

}  // namespace
}  // namespace frt

using namespace frt;

extern "C" int64_t frt_octbank_tails_length(const frt_octbank* h) {
    return h && h->mode == 1 ? (int64_t)kNOctave * h->nfilt * kTail : 0;
}

extern "C" int frt_octbank_get_tails(frt_octbank* h, double* tails) { return tails_copy(h, tails, true, "frt_octbank_get_tails"); }

extern "C" int frt_octbank_set_tails(frt_octbank* h, const double* tails) {
    return tails_copy(h, const_cast<double*>(tails), false, "frt_octbank_set_tails");
}

extern "C" int frt_octspec_run(frt_octbank* h, const void* x, int dtype, int64_t n, int64_t x_stride, const int64_t* ends,
                               int64_t n_refresh, const double* alphas, const double* weight_db, const double* energies_in,
                               double* energies_out, double* db_out, double* energy_out, int keep_last, int64_t scratch_bytes,
                               int* n_slabs_out) {
    FRT_REQUIRE(h && h->mode == 1 && h->ola && h->bpo >= 1, "frt_octspec_run: needs a mode-1 handle with bands");
    FRT_REQUIRE(dtype == 0 || dtype == 1, "frt_octspec_run: dtype %d (0 float32, 1 float64)", dtype);
    FRT_REQUIRE(n >= 0 && n < (1ll << 31), "frt_octspec_run: n = %lld must be below 2^31", (long long)n);
    FRT_REQUIRE(n_refresh >= 0 && (n_refresh == 0 || ends), "frt_octspec_run: n_refresh %lld without ends", (long long)n_refresh);
    FRT_REQUIRE(alphas && energies_in && energies_out && energies_in != energies_out, "frt_octspec_run: null or aliased energies");
    FRT_REQUIRE(n_refresh == 0 || (x && db_out), "frt_octspec_run: null buffer");
    FRT_REQUIRE(h->n_channels == 1 || x_stride >= n, "frt_octspec_run: the handle has %d channels: x_stride %lld below n", h->n_channels,
                (long long)x_stride);
    if (n_slabs_out) *n_slabs_out = 0;
    const int C = h->n_channels, nbands = h->nbands;
    const size_t sp_bytes = (size_t)C * nbands * sizeof(double);
    if (n_refresh == 0) {
        FRT_HIP_CHECK(hipMemcpyAsync(energies_out, energies_in, sp_bytes, hipMemcpyDeviceToDevice, h->stream));
        return FRT_OK;
    }
    for (int64_t r = 0; r < n_refresh; ++r) {
        const int64_t len = ends[r] - (r ? ends[r - 1] : 0);
        FRT_REQUIRE(len >= kOsBlock && len <= 1024 && len % kOsBlock == 0 && ends[r] <= n,
                    "frt_octspec_run: refresh %lld ends at %lld, %lld samples after the one before (multiples of 256 in [256, 1024], within n = %lld)",
                    (long long)r, (long long)ends[r], (long long)len, (long long)n);
    }
    const int64_t used = ends[n_refresh - 1], nb_all = used / kOsBlock, rows = keep_last ? 1 : n_refresh;
    // slabs of whole refreshes: per sample and stream 8 bytes of staged input (none where the samples are read in place), 8 of
    // stage signals (n / 2 + n / 4 + ... doubles) and nbands / 32 of block energies
    const double per_sample = C * (16.0 + nbands / 32.0);
    int64_t slab_max = scratch_bytes > 0 ? (int64_t)((double)scratch_bytes / per_sample) : used;
    if (slab_max < 1024) slab_max = 1024;                        // one refresh at least
    std::vector<int64_t> cut{0};                                 // refresh indices the slabs start at, then n_refresh
    for (int64_t r = 0, start = 0; r < n_refresh; ++r) {
        if (ends[r] - start > slab_max) {
            cut.push_back(r);
            start = ends[r - 1];
        }
    }
    cut.push_back(n_refresh);
    const int n_slabs = (int)cut.size() - 1;
    int64_t nb_max = 0, n_max = 0;
    for (int s = 0; s < n_slabs; ++s) {
        const int64_t a = cut[s] ? ends[cut[s] - 1] : 0, len = ends[cut[s + 1] - 1] - a;
        if (len > n_max) n_max = len;
    }
    nb_max = n_max / kOsBlock;
    // the call's tables in one upload: decay [nbands], weight [nbands], then row_of [nb_all] ints
    std::vector<double> tab((size_t)2 * nbands + (nb_all + 1) / 2, 0.0);
    for (int k = 0; k < nbands; ++k) {
        const int j = kNOctave - 1 - k / h->bpo;
        tab[k] = std::pow(1.0 - alphas[k], (double)(kOsBlock >> j));
        tab[nbands + k] = weight_db ? weight_db[k] : 0.0;
    }
    int* row_of = (int*)(tab.data() + 2 * nbands);
    for (int64_t b = 0; b < nb_all; ++b) row_of[b] = -1;
    for (int64_t r = keep_last ? n_refresh - 1 : 0; r < n_refresh; ++r) row_of[ends[r] / kOsBlock - 1] = keep_last ? 0 : (int)r;
    int rc;
    FRT_HIP_CHECK(hipStreamSynchronize(h->stream));              // an earlier call's launches may still read the tables
    if ((rc = upload(h->eout, tab))) return rc;
    const int runs_max = (int)((nb_max + kOsSplit - 1) / kOsSplit);
    if ((rc = h->eblock.reserve((size_t)C * (nb_max + 1) * nbands * sizeof(double))) || (rc = h->ypacked.reserve(2 * sp_bytes)) ||
        (rc = h->eseg.reserve((size_t)C * runs_max * nbands * sizeof(double))))
        return rc;
    const double* d_decay = h->eout.as<double>();
    const int* d_row_of = (const int*)(d_decay + 2 * nbands);
    const size_t esz = dtype ? sizeof(double) : sizeof(float);
    const double* sp_in = energies_in;
    for (int s = 0; s < n_slabs; ++s) {
        const int64_t a = cut[s] ? ends[cut[s] - 1] : 0, len = ends[cut[s + 1] - 1] - a;
        const int nb = (int)(len / kOsBlock);
        const void* xs = (const char*)x + (size_t)a * esz;
        if (C > 1 && x_stride != len) {                          // the bank reads rows of exactly its n samples
            if ((rc = h->xin.reserve((size_t)C * n_max * esz))) return rc;
            FRT_HIP_CHECK(hipMemcpy2DAsync(h->xin.ptr, (size_t)len * esz, xs, (size_t)x_stride * esz, (size_t)len * esz, C,
                                           hipMemcpyDeviceToDevice, h->stream));
            xs = h->xin.ptr;
        }
        // A call of ONE energy block that is the whole input belongs to the bank's chunk kernels, which smooth on their own: a slab
        // of a single sub-block asks for two.  The bank fills every block index below the count it is given — the second from the
        // outputs behind the samples, the new tails' — and the walk reads the first only.
        const int nb_held = nb == 1 ? 2 : nb;
        if ((rc = frt_ola_filter_batch(h, xs, dtype == 0, len, nullptr, 0, h->eblock.as<double>(), kOsBlock, nb_held, alphas))) return rc;
        double* sp_out = s == n_slabs - 1 ? energies_out : h->ypacked.as<double>() + (size_t)(s & 1) * C * nbands;
        OsWalk w{};
        w.eblock = h->eblock.as<double>();
        w.decay = d_decay;
        w.weight = weight_db ? d_decay + nbands : nullptr;
        w.row_of = d_row_of + a / kOsBlock;
        w.end = h->eseg.as<double>();
        w.sp_in = sp_in;
        w.sp_out = sp_out;
        // keep_last: the one row belongs to the last slab; db / energy of row r of the call otherwise
        w.db = db_out;
        w.energy = energy_out;
        w.nb = nb;
        w.nb_held = nb_held;
        w.nbands = nbands;
        w.rows = rows;
        const int threads = (nbands + 63) / 64 * 64;
        int nruns = 1;
        w.run_len = nb;
        if (nb >= 4 * kOsSplit) {
            nruns = (nb + kOsSplit - 1) / kOsSplit;
            w.run_len = kOsSplit;
            hipLaunchKernelGGL(octspec_local_kernel, dim3(nruns - 1, C), dim3(threads), 0, h->stream, w.eblock, w.decay,
                               h->eseg.as<double>(), nb, nbands);
        }
        auto walk = energy_out ? octspec_walk_kernel<true, true> : octspec_walk_kernel<true, false>;
        hipLaunchKernelGGL(walk, dim3(nruns, C), dim3(threads), 0, h->stream, w);
        FRT_HIP_CHECK(hipGetLastError());
        sp_in = sp_out;
    }
    if (n_slabs_out) *n_slabs_out = n_slabs;
    return FRT_OK;
}
