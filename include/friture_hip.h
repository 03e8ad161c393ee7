/* friture_hip.h — C ABI of libfriture_hip.so, the MI355X (gfx950) backend for Friture's
 * spectral-analysis hot path.
 *
 * The reference (tlecomte/friture) has no FFI: its boundary is a set of duck-typed Python
 * classes and functions.  Every entry point below names the reference interface
 * it replaces (paths relative to the reference checkout); the ctypes bindings that present the
 * reference's own names on top of this ABI live in friture_amd/ and are shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success and a negative status on failure, never throws;
 *     frt_last_error() returns a thread-local description of the last failure;
 *   - handles are opaque and own all device memory; one handle per Python object, used from
 *     one thread at a time (the reference calls everything from the Qt GUI thread);
 *   - buffers are caller owned.  A buffer argument may be a host pointer (staged through an
 *     internal device buffer, call returns after the result is back on the host) or a device
 *     pointer (kernels are enqueued on the handle's stream and the call returns immediately);
 *     inputs and outputs of one call must live on the same side;
 *   - audio is channel-major: x[c][t].
 */
#ifndef FRITURE_HIP_H
#define FRITURE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define FRT_OK 0
#define FRT_ERR_INVALID (-1)
#define FRT_ERR_HIP (-2)
#define FRT_ERR_NO_DEVICE (-3)
#define FRT_ERR_UNSUPPORTED (-4)
#define FRT_ERR_TOO_SMALL (-5)

/* ---- library ---------------------------------------------------------------------------- */

/* Binds the calling process to HIP device `device` (one process per GPU) and verifies that it is
 * a gfx950 part.  n_cus_out / hbm_bytes_out may be NULL. */
int frt_init(int device, int* n_cus_out, int64_t* hbm_bytes_out);
/* The same two figures for any visible device WITHOUT binding the process to it (the current device is untouched). */
int frt_device_properties(int device, int* n_cus_out, int64_t* hbm_bytes_out);
const char* frt_last_error(void);
const char* frt_version(void);
/* 1 if `p` is device memory, 0 if host memory. */
int frt_is_device_pointer(const void* p);
/* Path selection for tests and A/B runs.  The library never reads the environment; where one entry point has two product
 * code paths chosen by the shape of the call, this forces one of them for the whole process (value < 0: back to the shape
 * rule).  Both paths of every option compute the same reference function and are held to the same parity bar:
 *   "gcc_one_workgroup"    frt_gcc_phat: 1 = one workgroup per window pair whatever the batch size, 0 = a pair as launches
 *                          of its phases (default: by batch size)
 *                          (also read by frt_gcc_create: a handle of at most CUs / 8 pairs of the default window made while the
 *                          option is 1 gets the two-way plan of the large batches instead of the four-way plan of the small ones;
 *                          a handle made by frt_gcc_create_fixed with one_workgroup >= 0 uses that value in both places for its
 *                          whole life and never reads this option)
 *   "gcc_resident"         frt_gcc_phat, default window (24000 samples), one workgroup per pair: 0 = the kernel that parks the
 *                          sub-spectra in a scratch slab in HBM instead of the one that keeps them in registers and LDS
 *   "ola_defer"            frt_octbank_filter / _energies (mode 1, batched, >= 6 bands per octave): 0 = every stage's band filters in the
 *                          stage's own launch instead of one deferred launch over the low-rate stages
 *   "iir_lookback"         frt_octbank_energies (mode 0, time-parallel): 0 = every stage's chunk start states from a scan launch
 *                          instead of the output pass's own look-back over its predecessors' end states at the high-rate stages
 *   "iir_lane_columns"     frt_octbank_energies (mode 0, time-parallel): the output pass with the filter groups of 64 chunks in one
 *                          workgroup and their samples staged through LDS — 1 = at every stage it serves, 0 = at none (default:
 *                          where the launch has a workgroup per compute unit and the groups share enough samples)
 *   "gcc_any_length"       frt_gcc_create: 1 = the chirp-z transform also for lengths the mixed-radix plan serves
 *   "ola_chunk_kernels"    frt_octbank_filter (mode 1, one block of <= 1024 host samples): 0 = per-stage transform launches
 *                          instead of the two running-convolution launches
 *   "pitch_grid_two_pass"  frt_pitch_track: 1 = the two-pass log-grid kernel also on the widget's 1023-point grid
 * Unknown names: FRT_ERR_INVALID. */
int frt_set_option(const char* name, int value);
int frt_get_option(const char* name, int* value_out);

/* ---- K1: STFT -> power spectrum ( -> dB / normalised / colour pixels) -------------------------
 * Replaces audioproc.analyzelive + norm_square (friture/audioproc.py:42-50) looped by the STFT
 * drivers Spectrum_Widget.handle_new_data (friture/spectrum.py:144-155) and
 * Spectrogram_Widget.handle_new_data (friture/spectrogram.py:149-159), and the dB / weighting /
 * normalise / colour-LUT steps that follow (friture/spectrogram.py:119-129,161-162,
 * friture/signal/color_tranform.py:48-51, friture/signal/lookup_table.py:50-52).
 *
 * Frame f of channel c covers x[c][f*hop .. f*hop + fft_size); n_frames = (T - fft_size)/hop + 1.
 * Outputs are frame-major: out[c][f][k], k = 0..fft_size/2 (the reference's (N/2+1, frames)
 * array is the transpose of one channel's slab). */
typedef struct frt_stft frt_stft;

/* output kinds for frt_stft_run */
#define FRT_STFT_PSD 0   /* float: |rfft(x*w)|^2 / N^2                      audioproc.py:44-50  */
#define FRT_STFT_DB 1    /* float: 10 log10(psd + 1e-30) + weight[k]        spectrum.py:95-101  */
#define FRT_STFT_NORM 2  /* float: (dB - spec_min)/(spec_max - spec_min)    spectrogram.py:128  */
#define FRT_STFT_IMAGE 3 /* uint32: lut[int(clip(norm,0,1)*255)]            lookup_table.py:50  */

/* fft_size: power of two in [32, 16384] (spectrum_settings.py:61-70); hop in [1, ...);
 * precision: 32 (float in, float arithmetic) or 64 (double in, double arithmetic, double out). */
int frt_stft_create(frt_stft** h, int fft_size, int hop, int n_channels, int precision);
void frt_stft_destroy(frt_stft* h);
/* hipStream_t used for device-pointer calls (NULL = default stream). */
int frt_stft_set_stream(frt_stft* h, void* hip_stream);
/* weight_db: fft_size/2+1 values added to the dB spectrum or NULL (no weighting);
 * lut256: 256 colour words or NULL. */
int frt_stft_set_epilogue(frt_stft* h, const double* weight_db, double spec_min, double spec_max,
                          const uint32_t* lut256);
/* x: [n_channels][x_stride] samples (float for precision 32, double for 64), T valid per channel.
 * out: [n_channels][n_frames][fft_size/2+1] elements of the output kind (4 bytes each at
 * precision 32; at precision 64 PSD/DB/NORM are doubles and IMAGE stays uint32).
 * x and out: both host (returns with the result), both device (enqueued on the handle's stream), or x host and out
 * device (the samples go up through page-locked memory, the call returns without waiting: order consumers on the stream). */
int frt_stft_run(frt_stft* h, int kind, const void* x, int64_t T, int64_t x_stride, void* out,
                 int64_t* n_frames_out);
/* The same transform with SPLIT output rows (fft_size <= 1024; FRT_ERR_UNSUPPORTED above): out_rows[c][f][k] holds
 * bins k = 0..fft_size/2-1 — rows of fft_size/2 values, so that every row is a whole number of 64-byte lines when
 * out_rows is 64-byte aligned — and out_nyquist[c][f] holds bin fft_size/2 of every frame (element types as for
 * frt_stft_run).  Values are bit-identical to frt_stft_run's; only their addresses differ.  The reference's own array is
 * (N/2+1, frames), frequency-major (friture/spectrogram.py:149-159, friture/spectrum.py:144-155), so neither layout is
 * its transpose-free image: the packed rows of frt_stft_run are what the drop-in classes hand on, the split rows are for
 * batch consumers — a row store of the packed layout starts on a 4-byte boundary and touches five 64-byte lines where
 * this one touches four.  Same host / device pointer rules as frt_stft_run; out_rows and out_nyquist
 * on the same side. */
int frt_stft_run_split(frt_stft* h, int kind, const void* x, int64_t T, int64_t x_stride, void* out_rows,
                       void* out_nyquist, int64_t* n_frames_out);
/* survey-named conveniences (precision-32 handles): */
int frt_stft_psd(frt_stft* h, const float* x, int64_t T, float* psd_out, int64_t* n_frames_out);
int frt_stft_image(frt_stft* h, const float* x, int64_t T, uint32_t* rgba_out, int64_t* n_frames_out);
/* Exact drop-in for audioproc.analyzelive (audioproc.py:42-47): one double frame of fft_size
 * samples -> fft_size/2+1 doubles.  Requires a precision-64 handle. */
int frt_stft_analyzelive_f64(frt_stft* h, const double* frame, double* psd_out);
/* Number of frames frt_stft_run produces for T samples per channel. */
int64_t frt_stft_frames_for(const frt_stft* h, int64_t T);
/* Tuning hook (bench / tests): frames a workgroup lane-group processes back to back; 0 = auto.  A negative
 * value sets the run length to its magnitude and, for fft_size >= 2048, selects the generic workgroup-wide
 * kernel instead of the radix-16 + wave-local one (A/B runs). */
int frt_stft_set_run_length(frt_stft* h, int frames_per_run);

/* The walk (float32, fft_size 1024, hop 512 or 256): a grid of as many workgroups as are resident on the device, whose
 * wavefronts load their constants once and stride over runs of 16 frames.  Same values, bit for bit, as the launch of
 * one run per lane group.  mode -1 = automatic (default: large batches with no run length set), 0 = never, 1 = always when
 * such an instance exists (then a run length set with frt_stft_set_run_length is the walk's; in the other modes a set run
 * length keeps the launch of one run per lane group).  blocks 0 = the resident count queried at create time, > 0 = this
 * grid (tests). */
int frt_stft_set_persistent(frt_stft* h, int mode, int blocks);

/* ---- K2 / K4: octave filter bank with decimation, band energies -------------------------------
 * mode 0 replaces the exact IIR bank octave_filter_bank_decimation (friture/filter.py:86-118) built
 * on lfilter_float64_1D (friture/signal/lfilter.py:85-147) and decimate
 * (friture/signal/decimate.py:27-42): 9 octaves, `bands_per_octave` 4th-order band-passes per
 * octave on the j-times decimated signal, 12th-order elliptic decimator between octaves, carried
 * state.  Sequential mode is bit-identical to the reference; the time-parallel mode
 * (frt_octbank_set_chunk) evaluates the same recurrences chunk-wise and agrees to rounding.
 * mode 1 is the FFT overlap-add bank of Octave_Filters.filter (friture/octavefilters.py:49-58 /
 * friture/filter.py:136-247): 512-tap minimum-phase FIR of every IIR, 511-sample tails carried across calls; the same
 * frt_octbank_filter / frt_octbank_energies entry points.  Up to 1024 samples a call is one overlap-add block at the
 * reference's FFT sizes; a longer input is processed as if fed in 1024-sample blocks, every octave stage as one launch
 * over all blocks (the reference itself would crop such an input to its first stage's FFT size).
 *
 * Band order everywhere is the reference's list order: band k = 0 is the lowest band
 * (dec = 256), band 9*bpo-1 the highest (dec = 1); dec[k] = 2^(8 - k / bpo). */
typedef struct frt_octbank frt_octbank;

/* boct/aoct: [bands_per_octave][5]; bdec/adec: [13] (friture/generated_filters.py PARAMS);
 * boct_fir/bdec_fir are only used by mode 1 and may be NULL.  bands_per_octave = 0 creates a
 * decimator-only handle for frt_decimate_multiple. */
int frt_octbank_create(frt_octbank** h, int bands_per_octave, int n_channels, int mode, const double* boct,
                       const double* aoct, const double* bdec, const double* adec, const double* boct_fir,
                       const double* bdec_fir);
void frt_octbank_destroy(frt_octbank* h);
int frt_octbank_set_stream(frt_octbank* h, void* hip_stream);
/* zero every carried state (octave_filter_bank_decimation_filtic, friture/filter.py:121-133) */
int frt_octbank_reset(frt_octbank* h);
/* 0 (default): sequential in time, bit-identical to the reference.  chunk0 > 0 (multiple of 64, >= 256; for
 * frt_octbank_energies a multiple of the energy block, or a divisor of it — the latter for 16-byte aligned device
 * input in whole chunks only): batches of at least 2*chunk0 samples are
 * processed time-parallel, octave stage j in chunks of max(64, chunk0 / 2^j) of its own samples.  The two modes
 * agree to ~1e-10 of the input scale (same recurrences, other association order).  A negative value selects
 * the same chunking with the zero-state pass run as a second recurrence instead of a table product (A/B runs). */
int frt_octbank_set_chunk(frt_octbank* h, int chunk0);
/* doubles per channel in the packed output for n input samples: sum over bands of ceil(n / dec) */
int64_t frt_octbank_packed_length(const frt_octbank* h, int n);
/* x: [n_channels][n]; y_packed: [n_channels][packed_length], band k stored after band k-1;
 * dec_out: [9*bpo] or NULL.  n = 0 -> FRT_ERR_TOO_SMALL ("Filter input is too small",
 * friture/signal/decimate.py:33-34). */
int frt_octbank_filter(frt_octbank* h, const double* x, int n, double* y_packed, int* dec_out);
/* carried filter states per channel in the reference's zis/zfs order (friture/filter.py:121-133):
 * per octave the band states i = bpo-1..0 (4 doubles each) then the decimator's 12. */
int frt_octbank_state_length(const frt_octbank* h);
int frt_octbank_get_state(frt_octbank* h, double* z /* [n_channels][state_length] */);
int frt_octbank_set_state(frt_octbank* h, const double* z);
/* Band energies of OctaveSpectrum_Widget.handle_new_data (friture/octavespectrum.py:101-121) for a
 * whole batch: x float [n_channels][n] is cut in blocks of `block` samples (power of two >= 256, the
 * widget's chunk), per block and band sp = alpha*sum_i (1-alpha)^(m-1-i) y_i^2 + sp_prev*(1-alpha)^m
 * (friture/signal/exp_smoothing.py:40-56; m = block/dec), carried across blocks and calls.
 * energy_out: float [n_channels][n/block][9*bpo]; as_db != 0 stores 10 log10(sp + 1e-30) + weight_db[k]
 * (weight_db may be NULL) instead of sp.  The band signals themselves are not written.  Mode 1: block <= 1024. */
int frt_octbank_energies(frt_octbank* h, const float* x, int64_t n, int block, const double* alphas,
                         const double* weight_db, int as_db, float* energy_out);
/* The pending tails of a mode-1 handle — the FFT bank's whole carried state (friture/filter.py:213-245) — read and set.
 * tails: [n_channels][9][bands_per_octave + 1][511] doubles: per channel, per octave stage j = 0 (full rate) .. 8, per filter
 * of the stage (the band-passes i = 0..bpo-1 as in boct_fir, then the decimator), the 511 outputs still to be added to the
 * stage's next samples.  frt_octbank_tails_length: doubles per channel (0 for a mode-0 handle).  Host pointers (the call
 * returns with the copy done) or device pointers (enqueued on the handle's stream).  frt_octbank_get_state / _set_state
 * remain the exact IIR bank's. */
int64_t frt_octbank_tails_length(const frt_octbank* h);
int frt_octbank_get_tails(frt_octbank* h, double* tails);
int frt_octbank_set_tails(frt_octbank* h, const double* tails);
/* The octave-spectrum widget's chain over a recording (OctaveSpectrum_Widget.handle_new_data, friture/octavespectrum.py:91-122)
 * as widgets fed chunk by chunk would have seen it; mode-1 handle, float64 results.  x: DEVICE samples [n_channels] rows of n
 * samples x_stride elements apart, float32 (dtype 0) or float64 (dtype 1), n < 2^31.  ends: [n_refresh] HOST int64, the sample
 * counts at which the widgets refresh, counted from x[0]: increasing, every chunk (ends[r] - ends[r-1], ends[0]) a multiple of
 * 256 in [256, 1024], ends[n_refresh-1] <= n — 256 = 2^8 keeps the per-chunk decimation y[:N:2] of all nine stages on one grid,
 * 1024 is where the reference's first-stage rfft(x, 1536) would start to crop.  Samples behind the last end are not consumed.
 * alphas, weight_db (may be NULL): [9*bpo] HOST doubles.  energies_in / energies_out: [n_channels][9*bpo] DEVICE doubles, the
 * smoothed energies sp before and after (two different buffers); the filters' state is the handle's tails (above), read and
 * left behind.  Per refresh r and band: sp after the chunk by sp = E_b + sp (1 - alpha)^(256 / dec) over the chunk's 256-sample
 * sub-blocks b, E_b the sub-block's zero-state energy alpha sum_i (1 - alpha)^(m-1-i) y_i^2 — the chunk's own
 * exp_smoothed_value (friture/signal/exp_smoothing.py:40-56) to rounding.  db_out: [n_channels][R'][9*bpo] DEVICE doubles,
 * 10 log10(sp + 1e-30) + weight_db, R' = n_refresh or 1 with keep_last (the final refresh); energy_out: sp itself in the same
 * shape, or NULL.  The recording is walked in time slabs of whole refreshes whose scratch (staged samples, stage signals,
 * block energies) stays within scratch_bytes (<= 0: one slab; a refresh at least); n_slabs_out (may be NULL) receives their
 * number.  Launches and copies per call depend on the number of slabs only.  Enqueued on the handle's stream. */
int frt_octspec_run(frt_octbank* h, const void* x, int dtype, int64_t n, int64_t x_stride, const int64_t* ends, int64_t n_refresh,
                    const double* alphas, const double* weight_db, const double* energies_in, double* energies_out,
                    double* db_out, double* energy_out, int keep_last, int64_t scratch_bytes, int* n_slabs_out);
/* decimate_multiple (friture/signal/decimate.py:45-71) with carried state: n_stages chained
 * decimations by 2 of x [n_channels][n] -> out [n_channels][*n_out].  Needs a bands_per_octave = 0 handle. */
int frt_decimate_multiple(frt_octbank* h, int n_stages, const double* x, int n, double* out, int* n_out);
/* the same with the reference's functional interface (the states are arguments and results, decimate.py:45-71) as ONE call
 * on HOST arrays: x [n_channels][n] -> out [n_channels][*n_out], zi / zf [n_channels][n_stages][order] (order = the handle's
 * decimator order: 12 for the bank's) or NULL (zero state / not wanted); the handle's carried state is not touched.  Every
 * channel of the handle rides in the same n_stages launches (the delay estimator's two channels, delay_estimator.py:97-98).
 * The samples are read and the result written in place in page-locked memory: roundup(8 n channels, 256) + 128 n_stages
 * channels bytes must fit 256 KB, i.e. n <= 32 639 for one channel and two stages (FRT_ERR_INVALID above that: use
 * frt_octbank_set_state + frt_decimate_multiple). */
int frt_decimate_multiple_state(frt_octbank* h, int n_stages, const double* x, int n, const double* zi, double* out, int* n_out,
                                double* zf);
/* lfilter_float64_1D (friture/signal/lfilter.py:85-147): direct form II transposed IIR of one host
 * signal with explicit state; len(b) = len(a) = n_coef <= 16, zi/zf hold n_coef-1 doubles. */
int frt_lfilter_f64(const double* b, const double* a, int n_coef, const double* x, int n, const double* zi,
                    double* y, double* zf);

/* ---- the delay estimator's per-chunk part, device resident (SURVEY.md §8 row 5 caller) -----------------------------
 * Delay_Estimator_Widget.handle_new_data (friture/delay_estimator.py:87-131) without its GCC-PHAT call: per chunk of both
 * channels, n_stages chained decimations by 2 with carried state (:97-98, decimate_multiple) and a push into two private
 * mirror rings of the decimated signals (:99-100, friture/ringbuffer.py:39-63), all in HBM.  frt_delay_push is
 * asynchronous (a pinned slot, the decimation stages and one ring-write launch on the object's stream; nothing comes back
 * per chunk).  Windows are handed out as device pointers into the rings (RingBuffer.data_indexed, ringbuffer.py:87-99; the
 * rings grow by the reference's rule, ringbuffer.py:102-130) and go to frt_gcc_phat / frt_gcc_readout as they are. */
typedef struct frt_delay frt_delay;
int frt_delay_create(frt_delay** out, const double* bdec, const double* adec, int n_stages, int ring_length /* 10000 */);
void frt_delay_destroy(frt_delay* h);
void* frt_delay_stream(frt_delay* h);                 /* the hipStream_t the pushes are enqueued on */
/* x: float64 [2][n] in HOST memory; *offset_out = decimated samples pushed so far (RingBuffer.offset), may be NULL */
int frt_delay_push(frt_delay* h, const double* x, int n, int64_t* offset_out);
/* the rings hold at least `length` samples from now on (RingBuffer.grow_if_needed) */
int frt_delay_reserve(frt_delay* h, int length);
/* device pointers of the `length` samples of each ring that end at absolute index `end` (<= offset); valid until the
 * rings grow.  Enqueued pushes may still be in flight: order consumers on frt_delay_stream or call frt_delay_window_std. */
int frt_delay_window(frt_delay* h, int64_t end, int length, double** d0, double** d1);
/* numpy.std of both windows (the gate of delay_estimator.py:127) -> std_out[2] on the host; waits for the object's stream */
int frt_delay_window_std(frt_delay* h, const double* d0, const double* d1, int length, double* std_out);
/* d0 -= means[0], d1 -= means[1] in place (generalized_cross_correlation does this to its views, correlation.py:27-28);
 * means: two doubles in DEVICE memory (frt_gcc_phat's means_out); stream: the stream frt_gcc_phat ran on, NULL = the object's */
int frt_delay_demean(frt_delay* h, double* d0, double* d1, int length, const double* means, void* stream);

/* ---- device-resident streaming spectrogram ------------------------------------------------
 * One object does what Spectrogram_Widget.handle_new_data does per chunk (friture/spectrogram.py:131-177) and hands back
 * the block CanvasScaledSpectrogram.addData draws (friture/spectrogram_image.py:82-129): a mirror ring of the samples in
 * HBM (friture/ringbuffer.py:39-63; only the new chunk crosses PCIe), the realizable frames through the float64 STFT with
 * the dB / weighting / normalise epilogue, np.interp onto the screen rows (friture/signal/frequency_resampler.py:67-83),
 * the online time resampler with its carried column on the device (friture/signal/online_linear_2D_resampler.py:45-97),
 * clip + LUT (friture/signal/color_tranform.py:48-51) and the flip of the frequency axis.  Float64, the reference's
 * operations in the reference's order: the pixels are the reference's pixels.
 * overlap as in the widget (0.75 default): needed = fft_size (1 - overlap), hop = int(needed).  ring_length >= 2 fft_size. */
typedef struct frt_specgram frt_specgram;
int frt_specgram_create(frt_specgram** h, int fft_size, double overlap, int ring_length);
void frt_specgram_destroy(frt_specgram* h);
/* weight_db [fft_size/2+1] or NULL, dB range, 256 colour words */
int frt_specgram_set_epilogue(frt_specgram* h, const double* weight_db, double spec_min, double spec_max, const uint32_t* lut256);
/* freq [fft_size/2+1] bin frequencies, targets [height] screen-row frequencies (Frequency_Resampler.xscaled).  A changed
 * height Fourier-resamples the carried column (Online_Linear_2D_resampler.set_height). */
int frt_specgram_set_screen(frt_specgram* h, const double* freq, const double* targets, int height);
/* Online_Linear_2D_resampler.set_ratio: STFT rate / pixel rate as the two numbers the widget passes */
int frt_specgram_set_ratio(frt_specgram* h, double interp_factor_L, double decim_factor_M);
/* chunk: n new samples (host, float64).  pixels_out: [height][max_cols] uint32 (host or device), row 0 = highest frequency;
 * *n_cols_out columns are written (often 0), *n_frames_out (nullable) spectra were computed. */
int frt_specgram_push(frt_specgram* h, const double* chunk, int n, uint32_t* pixels_out, int max_cols, int* n_cols_out,
                      int* n_frames_out);
int frt_specgram_reset(frt_specgram* h);

/* ---- K5: GCC-PHAT cross-correlation and the delay read-out --------------------------------------
 * frt_gcc_phat replaces generalized_cross_correlation (friture/signal/correlation.py:24-43): mean
 * removal, numpy.hanning window, two real FFTs, conj(D0) D1, PHAT weight 1/(1e-10 max|G| + |G|),
 * inverse real FFT.  length must be even with length/2 = R * M2, R in {1, 2, 4}, M2 <= 6144 and
 * 5-smooth (the default window of 24000 samples, friture/delay_estimator.py:114-115, qualifies).
 * The reference subtracts the means in place on its arguments; means_out lets a binding reproduce
 * that side effect. */
typedef struct frt_gcc frt_gcc;
int frt_gcc_create(frt_gcc** h, int length, int n_pairs);
/* The same with the handle's own value of "gcc_one_workgroup": 1 or 0 pins it, -1 leaves it to the process option (frt_gcc_create). */
int frt_gcc_create_fixed(frt_gcc** h, int length, int n_pairs, int one_workgroup);
void frt_gcc_destroy(frt_gcc* h);
int frt_gcc_set_stream(frt_gcc* h, void* hip_stream);
/* d0, d1, xcorr_out: [n_pairs][length] doubles; argmax_out: [n_pairs] index of max |xcorr| or NULL;
 * means_out: [n_pairs][2] or NULL. */
int frt_gcc_phat(frt_gcc* h, const double* d0, const double* d1, double* xcorr_out, int* argmax_out, double* means_out);

/* Peak read-out of Delay_Estimator_Widget.handle_new_data (friture/delay_estimator.py:134-176). */
typedef struct frt_delay_readout {
    int argmax;           /* index of max |smoothed|                                   :141-142 */
    int correlation_pct;  /* int(100 x/(1+x)), x = (0.12 max(0, peak/(3 std) - 1))^3    :171-176 */
    double delay_ms;      /* 1e3 argmax / rate, minus the window when past its half     :148-152 */
    double distance_m;    /* delay * 340 m/s                                            :167-168 */
    double extremum;      /* smoothed[argmax] (its sign is the polarity)                :146     */
} frt_delay_readout;
/* smoothed_out = alpha * xcorr + (1 - alpha) * old_smoothed (or xcorr when old_smoothed is NULL),
 * [n_pairs][length]; readout: [n_pairs] host structs. */
int frt_gcc_readout(frt_gcc* h, const double* xcorr, const double* old_smoothed, double alpha, double sample_rate,
                    double delayrange_s, double* smoothed_out, frt_delay_readout* readout);

/* ---- the delay estimator's chain over whole recordings (delaybatch.hip) -----------------------------------------------
 * Three steps of DelayEstimatorBatch (friture_amd/delay_estimator.py); everything is enqueued on the null stream, every
 * array is DEVICE memory unless said otherwise, float64 unless said otherwise.
 *
 * frt_delaybatch_decimate: decimate_multiple (friture/signal/decimate.py:45-71) of x [n_channels][n] (rows x_stride elements
 * apart; dtype 0 float32, widened exactly, 1 float64), time-parallel: every stage cuts its input into cells of 1024 samples
 * on a grid anchored at sample `origin` >> stage of the recording (origin: the absolute index of x's first sample), runs the
 * cells from the zero state, chains their end states with the exact transition A^1024 and runs them again from their true
 * start states.  b, a: the decimator's 13 + 13 coefficients (HOST, a[0] = 1).  zi / zf: [n_channels][n_stages][12] DF2T
 * states in decimate_multiple's order, NULL = zero state / not wanted.  out: [n_channels][*n_out], rows out_stride apart,
 * *n_out = n halved n_stages times, rounding up. */
int frt_delaybatch_decimate(const double* b, const double* a, int n_coef, int n_stages, const void* x, int dtype, int n_channels,
                            int64_t n, int64_t x_stride, int64_t origin, const double* zi, double* out, int64_t out_stride,
                            double* zf, int64_t* n_out);
/* The windows of n_streams delay estimators and their GCC-PHAT.  dec: [n_streams][2][n_dec] decimated signals behind the
 * carried tail, rows dec_stride apart.  runs: HOST [n_windows][8][4] int64 (delay_schedule): per window up to eight runs of
 * (first source index in a row of dec, length, 1 = zeros instead, earlier window whose mean the ring view had subtracted: its
 * index in this call, -1 none, -2 the window before this call's first: means_in [n_streams][2], NULL = zeros); the lengths of
 * a window add up to `length`.  means_out: [n_streams][n_windows][2] the effective windows' means (0 where gated); gated_out:
 * [n_streams][n_windows] 1 where every effective sample of a channel is equal.  xcorr: [n_streams][n_windows][length], pair
 * q = stream * n_windows + window.  The pairs go to frt_gcc_phat in slabs of pairs_full (<= 65535) on gcc_full, a handle of
 * that many pairs, and a shorter last slab on gcc_last, a handle of its size (both on the null stream). */
int frt_delaybatch_windows(const double* dec, int64_t dec_stride, int64_t n_dec, int n_streams, int length, int64_t n_windows,
                           const int64_t* runs, const double* means_in, frt_gcc* gcc_full, int64_t pairs_full, frt_gcc* gcc_last,
                           double* xcorr, double* means_out, int* gated_out, int* n_slabs_out);
/* Smoothing and read-out of every window in order (friture/delay_estimator.py:134-182): smoothed = alpha xcorr + (1 - alpha)
 * smoothed from the first ungated window on (itself where no correlation is carried: smoothed_in [n_streams][length] with
 * present_in [n_streams] != 0, either may be NULL); gated windows keep it and read 0.  Per window [n_streams][n_windows]:
 * argmax of |smoothed| (the first on ties), delay_ms, distance_m, extremum, correlation as frt_delay_readout has them.
 * smoothed_out / present_out: the correlation carried out.  Partial sums are combined in lag order. */
int frt_delaybatch_readout(const double* xcorr, const int* gated, int n_streams, int64_t n_windows, int length,
                           const double* smoothed_in, const int* present_in, double alpha, double sample_rate, double delayrange_s,
                           double* smoothed_out, int* present_out, int* argmax_out, double* delay_ms_out, double* distance_m_out,
                           double* extremum_out, int* correlation_out);

/* ---- K6: screen-space stages of the spectrogram, and block-wise exponential smoothing -------------
 * Stateless float64 kernels, one per block of the reference's Transform_Pipeline
 * (friture/signal/transform_pipeline.py:23-34); the stateful bookkeeping of the online resampler
 * (which pixel columns a pushed column produces) is scalar arithmetic that stays with the caller.
 * Matrices are row-major; data/out buffers may be host or device memory. */
/* P5 Frequency_Resampler.push (friture/signal/frequency_resampler.py:67-83):
 * out[h][c] = numpy.interp(targets[h], freq, data[:, c]); data [n_bins][n_cols], out [height][n_cols]. */
int frt_freq_resample(const double* freq, int n_bins, const double* targets, int height, const double* data,
                      int n_cols, double* out);
/* P6 linear_interp_2D (friture/signal/linear_interp.py:57-60) for all pixel columns a push emits:
 * out[h][p] = data[h][src_col[p]] * (1 - a[p]) + prev * a[p], prev = data[h][src_col[p]-1] or old[h]
 * for column 0; data [height][n_cols], out [height][n_out]. */
int frt_time_resample(const double* data, const double* old, int height, int n_cols, const int* src_col,
                      const double* a, int n_out, double* out);
/* Fourier resampling of `count` real vectors x [count][n] -> y [count][m] (friture/signal/scipy_resample.py:51-141 with
 * window = None, axis = the vector): the N = min(n, m) lowest frequencies of fft(x) are kept, y = ifft(Y) * m / n.  Any
 * lengths (screen heights are arbitrary integers).  Used by Online_Linear_2D_resampler.set_height
 * (friture/signal/online_linear_2D_resampler.py:45-55) for the carried column when the plot is resized. */
int frt_fourier_resample(const double* x, int n, int count, double* y, int m);
/* P7 Color_Transform.push (friture/signal/color_tranform.py:48-51): out[i] = lut[int(clip(v[i],0,1)*255)] */
int frt_colour_map(const uint32_t* lut256, const double* values, int64_t count, uint32_t* out);
/* P5 + P6 + P7 in one call: Transform_Pipeline.push (friture/signal/transform_pipeline.py:29-34) over the spectrogram's three
 * blocks (friture/spectrogram.py:62-68) — np.interp onto the screen rows (frequency_resampler.py:67-83), the online time
 * resampler's lerp against its carried column (online_linear_2D_resampler.py:61-97, linear_interp.py:47-60), clip + LUT
 * (color_tranform.py:48-51) — the reference's operations in the reference's order, host arrays in and out.
 * norm [n_cols][nb] frame-major; freq [nb], targets [height]: Frequency_Resampler's freq and xscaled; old_in / old_out
 * [height]: the time resampler's carried column before / after; src, a [n_out]: its (source column, weight) pairs;
 * pixels_out [height][n_out] uint32, row 0 = lowest frequency. */
int frt_screen_columns(const double* norm, int nb, int n_cols, const double* freq, const double* targets, int height,
                       const double* old_in, const int* src, const double* a, int n_out, const uint32_t* lut256,
                       uint32_t* pixels_out, double* old_out);
/* P8 exp_smoothed_value_2d (friture/signal/exp_smoothing.py:91-107); nf = 1 gives exp_smoothed_value:
 * out[r] = alpha * dot(data[r][:n], kernel[nk-n:]) + previous[r] * (1-alpha)^n, n = min(nt, nk)
 * (previous is dropped when nt > nk). */
int frt_exp_smooth_2d(const double* kernel, int nk, double alpha, const double* data, int nf, int nt, int64_t row_stride,
                      const double* previous, double* out);
/* The octave-spectrum widget's smoothing of one chunk in ONE call (friture/octavespectrum.py:103-112 calls exp_smoothed_value
 * once per band, friture/signal/exp_smoothing.py:40-56): group g = the nf[g] bands of one octave, which share kernel
 * (kernels[g], nk[g] taps), alpha and length nt[g]; data[g] points at the group's rows (row_stride[g] doubles apart — the packed
 * band signals frt_octbank_filter returns are laid out like this).  square != 0: every datum is squared first (the widget smooths
 * y^2).  previous / out: one value per row, groups concatenated.  Every row equals its own frt_exp_smooth_2d call bit for bit.
 * Host arrays only (one chunk of the widget). */
int frt_exp_smooth_groups(int n_groups, const double* const* kernels, const int* nk, const double* alphas,
                          const double* const* data, const int* nf, const int* nt, const int64_t* row_stride, int square,
                          const double* previous, double* out);

/* ---- spectrum widget post-processing (Spectrum_Widget.handle_new_data, friture/spectrum.py:156-182) --
 * psd: the n_frames new PSD frames [n_frames][frame_stride] (float when psd_is_f32, else double; the
 * frame-major slab frt_stft_run writes).  smoothed = exp_smoothed_value_2d(kernel, alpha, psd^T, previous);
 * db = 10 log10(smoothed + 1e-30) + weight_db (or - 10 log10(ref_smoothed + 1e-30) in dual-channel mode);
 * *peak_index_out = argmax(db); *pitch_index_out = argmax of the harmonic product spectrum
 * s[:K] s[::2][:K] s[::3][:K], K = n_bins / 3, of smoothed (of ref_smoothed in dual-channel mode).
 * psd / previous / weight_db / ref_smoothed / smoothed_out: all host or all device; db_out may be a host array either way.
 * STREAM ORDER of device-resident arguments (this call and the other stateless entry points that accept device pointers:
 * frt_freq_resample, frt_time_resample, frt_colour_map, frt_exp_smooth_2d, frt_screen_columns): the kernel is launched on
 * the NULL stream, which is ordered behind every BLOCKING stream of the process and behind nothing else.  Whatever
 * produced `psd` must therefore have been enqueued on the null stream or a blocking stream (the default of
 * frt_stft_create; torch's current stream unless the caller made it a non-blocking side stream) — or be complete
 * (hipStreamSynchronize / an event wait) before the call.  A handle whose stream was set to a hipStreamNonBlocking one with
 * frt_stft_set_stream gives no such order. */
int frt_spectrum_post(const void* psd, int psd_is_f32, int n_frames, int n_bins, int64_t frame_stride,
                      const double* kernel, int nk, double alpha, const double* previous, const double* weight_db,
                      const double* ref_smoothed, double* smoothed_out, double* db_out, int* peak_index_out,
                      int* pitch_index_out);

/* ---- T1: pitch tracker (PitchTracker.estimate_pitch / update, friture/pitch_tracker.py:313-428) ---------
 * Per frame of fft_size samples (hop apart): |rfft(frame * hann)| -> np.interp onto the log-spaced grid
 * log_freqs[n_log] -> divide by its RMS -> strengths = kernels[n_candidates][n_log] @ grid spectrum ->
 * arg-max, parabolic vertex (fastParabolicInterp :160-193), index -> Hz, confidence = strength / 2.56,
 * frame level 20 log10(rms + eps); then the sequential gate: unvoiced (NaN) when level < min_db,
 * confidence < conf, or the estimate jumps more than p_delta semitones from the previous voiced one.
 * The grid and the kernel matrix are the caller's tables (_init_swipe :334-355, calcCosineKernel :195-264);
 * the gate's "previous estimate" is carried in the handle, per channel, across calls. */
typedef struct frt_pitch frt_pitch;
int frt_pitch_create(frt_pitch** h, int fft_size, int hop, int n_channels, double sample_rate, const double* log_freqs,
                     int n_log, const double* kernels, int n_candidates, double min_db, double conf, double p_delta);
void frt_pitch_destroy(frt_pitch* h);
int frt_pitch_set_stream(frt_pitch* h, void* hip_stream);
/* forget the previous estimates (prev_f0 = None, :292) */
int frt_pitch_reset(frt_pitch* h);
/* the gate's carried state: previous[n_channels] (host or device), NaN = no previous estimate */
int frt_pitch_set_previous(frt_pitch* h, const double* previous);
int frt_pitch_get_previous(frt_pitch* h, double* previous);
/* the widget changes the thresholds at run time (pitch_tracker.py:142-146) */
int frt_pitch_set_gate(frt_pitch* h, double min_db, double conf, double p_delta);
/* device scratch (spectra, grid spectra, strengths) a call may hold; longer runs go through it in chunks
 * of frames.  Default 1 GiB. */
int frt_pitch_set_scratch_limit(frt_pitch* h, int64_t bytes);
int64_t frt_pitch_frames_for(const frt_pitch* h, int64_t T);
/* x: [n_channels][x_stride] doubles, T valid samples per channel.  f0_out: [n_channels][n_frames], NaN =
 * unvoiced.  raw_out (or NULL): [3][n_channels][n_frames] = estimate before gating, confidence, dBFS. */
int frt_pitch_track(frt_pitch* h, const double* x, int64_t T, int64_t x_stride, double* f0_out, double* raw_out,
                    int64_t* n_frames_out);

/* ---- P3: the pitch tracker widget's chain over whole recordings (PitchBatch) --------------------------------------------
 * frt_pitch_track for streams of one or two rows behind a carried tail: estimate and confidence from row 0, the gate's level
 * from EVERY row of the frame (pitch_tracker.py:404-407: the RMS of the [rows, N] frame), then the gate of frt_pitch_track on
 * that level, with the handle's previous estimates.  The handle has one channel per stream.
 *   row0: [streams][row0_stride] doubles, pending + T valid samples: row 0 of tail || x per stream
 *   x: sample t of row `row` of stream s at x[s * ld_stream + row * ld_row + t], dtype 0 float32 / 1 float64 (widened exactly)
 *   tail: [streams][rows][pending] doubles, the samples received before x that no frame has consumed (NULL when pending == 0)
 * Frame g is samples [g * hop, g * hop + fft_size) of tail || x; n_frames = frames_for(pending + T).  f0_out, raw_out: as
 * frt_pitch_track.  Every buffer is device memory; launched on the null stream (which the handle is left on), one
 * synchronisation at the end. */
int frt_pitch_track_rows(frt_pitch* h, const double* row0, int64_t row0_stride, const void* x, int dtype, int rows, int64_t T,
                         int64_t ld_stream, int64_t ld_row, const double* tail, int64_t pending, double* f0_out, double* raw_out,
                         int64_t* n_frames_out);
/* What the widget shows at each refresh (PitchTrackerWidget.handle_new_data / update_curve, :109-119).  estimates:
 * [streams][n_frames]; frame_start: [n_refresh + 1] HOST int64, increasing from 0 to n_frames: refresh r completes frames
 * frame_start[r] .. frame_start[r + 1] - 1; history_in: [streams][history_length], the estimates before these (zeros before the
 * first).  pitch_out[s][r] = estimates[s][frame_start[r + 1] - 1]; curve_out: [streams][R'][history_length] with R' = n_refresh, or
 * 1 with keep_last (the final refresh; with n_refresh == 0 the history as it stands): the last history_length entries of history || estimates up to the refresh, as
 * clip(1 - (log2(fmax(f, 1e-20)) - log2(min_freq)) / (log2(max_freq) - log2(min_freq)), 0, 1) (fmax ignores NaN: unvoiced = 1);
 * history_out (not history_in): the last history_length entries after the call.  Device buffers, null stream, one
 * synchronisation at the end. */
int frt_pitch_refresh(const double* estimates, int streams, int64_t n_frames, const int64_t* frame_start, int64_t n_refresh,
                      const double* history_in, int64_t history_length, double min_freq, double max_freq, int keep_last,
                      double* history_out, double* pitch_out, double* curve_out);

/* ---- T1 live: the pitch tracker's chain for one stream fed chunk by chunk (PitchTrackerStream) ---------------------------------
 * A small object on top of a ONE-channel frt_pitch plan (not owned; it must outlive the object and is left on the null stream):
 * the gate's previous estimate, the last history_length estimates (zeros before the first) and the axis range
 * [min_freq, max_freq] of the curve live on the device.  frt_pitch_live_push takes the HOST samples that complete
 * n_frames >= 1 frames — span = fft_size + (n_frames - 1) * hop samples per row, row r at x + r * ld_row, dtype 0 float32 /
 * 1 float64 (widened exactly), rows 1 or 2 — and runs the chain of frt_pitch_track_rows + frt_pitch_refresh on them: spectrum
 * and estimate from row 0, the gate's level from every row, the gate with the thresholds given here, then the history shifted
 * by the new estimates.  estimates_out: [n_frames] (NaN = unvoiced); latest_out: the last of them; curve_out: [history_length],
 * the curve of frt_pitch_refresh after this push.  One copy back and one synchronisation per push, null stream.  The same
 * samples give the bits of frt_pitch_track_rows / frt_pitch_refresh however the frames are spread over pushes: up to
 * `crossover` frames per push (default 16) the strengths come from a kernel with one candidate per lane, above it from the
 * tiled kernel of frt_pitch_track, with equal bits. */
typedef struct frt_pitch_live frt_pitch_live;
int frt_pitch_live_create(frt_pitch_live** h, frt_pitch* plan, int64_t history_length, double min_freq, double max_freq);
void frt_pitch_live_destroy(frt_pitch_live* h);
/* no previous estimate, a history of zeros */
int frt_pitch_live_reset(frt_pitch_live* h);
int frt_pitch_live_push(frt_pitch_live* h, const void* x, int dtype, int rows, int64_t span, int64_t ld_row, double min_db,
                        double conf, double p_delta, double* estimates_out, double* latest_out, double* curve_out,
                        int64_t* n_frames_out);
/* previous: [1] (NaN = none), history: [history_length]; host or device memory */
int frt_pitch_live_get_state(frt_pitch_live* h, double* previous, double* history);
int frt_pitch_live_set_state(frt_pitch_live* h, const double* previous, const double* history);
/* frames per push (0 .. 1024) up to which the one-candidate-per-lane kernel forms the strengths */
int frt_pitch_live_set_crossover(frt_pitch_live* h, int frames);
int frt_pitch_live_crossover(const frt_pitch_live* h);

/* ---- L1: level meters and long-time levels (Levels_Widget, LongLevelWidget) -----------------------------
 * Per channel and per chunk (friture/levels.py:85-124, iec.py, ballistic_peak.py:21-66,
 * signal/exp_smoothing.py:40-56): value_max = max|y| (chunks of length > 0); old_max = value_max if
 * value_max > old_max (1 - alpha2), else old_max *= (1 - alpha2); rms = alpha (kernel tail . y^2) +
 * rms (1 - alpha)^len (an empty chunk keeps rms); level_rms = 10 log10(rms), level_max = 20 log10(old_max);
 * peak_iec = BallisticPeak(dB_to_IEC(max(level_max, level_rms))), the hold-then-decay machine whose decay
 * factor squares itself on every decay step.  Per complete block of 2^Ndec samples (friture/longlevels.py:
 * 31-91,138-171,195-209; a block is the 2^Ndec samples ending where the previous one ended plus 2^Ndec, i.e. the
 * widget's data_indexed(old_index, 2^Ndec): one block behind the stream, zeros before its start): y^2 -> Ndec x (FIR gauss11 with a = [1, 0, ...], then [::2]) -> FIR gauss41 with
 * carried state -> 10 log10(max(level, 1e-150)) -> a history ring of history_len entries.
 * kernel[nk], alpha, alpha2, gauss11[11], gauss41[41] and peak_decay_rate are the reference's own host values
 * (levels.py:57-74, longlevels.py:49-51,61,220-221, ballistic_peak.py:22); the handle carries every state
 * across calls, per channel.  Ndec 1 .. 13. */
typedef struct frt_levels frt_levels;
#define FRT_LEVELS_METER_FIELDS 6  /* rms, old_max, level_rms, level_max, peak_iec, branch                  */
#define FRT_LEVELS_FOLLOW 0        /* ballistic_peak.py:43-47  the input is above the peak                  */
#define FRT_LEVELS_HOLD 1          /* ballistic_peak.py:48-51  hold                                         */
#define FRT_LEVELS_DECAY 2         /* ballistic_peak.py:52-62  decay; the factor squares itself             */
#define FRT_LEVELS_DECAY_FLOOR 3   /* ballistic_peak.py:55-58  decay below the input: follow it, reset hold */
int frt_levels_create(frt_levels** h, int channels, int ndec, int64_t history_len, const double* kernel, int nk, double alpha,
                      double alpha2, const double* gauss11, const double* gauss41, double peak_decay_rate);
void frt_levels_destroy(frt_levels* h);
int frt_levels_set_stream(frt_levels* h, void* hip_stream);
/* every state to its initial value (levels.py:66-69, ballistic_peak.py:27-29, longlevels.py:225-229), ring zeroed */
int frt_levels_reset(frt_levels* h);
/* LongLevelWidget.setresptime (longlevels.py:212-229): new Ndec, zero subsampler and FIR state; the samples not
 * yet consumed, the meters and the ring are kept */
int frt_levels_set_ndec(frt_levels* h, int ndec);
/* the carried state as doubles: [pending count, Ndec, channels x (meters, stage inputs, FIR inputs, pending)] */
int64_t frt_levels_state_length(const frt_levels* h);
int frt_levels_get_state(frt_levels* h, double* state);
int frt_levels_set_state(frt_levels* h, const double* state);
/* blocks a call with n more samples per channel produces; samples received and not yet consumed (< 2^Ndec) */
int64_t frt_levels_blocks_for(const frt_levels* h, int64_t n);
int64_t frt_levels_pending(const frt_levels* h);
/* Batch form.  x: [channels][ld] float32 (dtype 0) or float64 (dtype 1), host or device; cut into chunks of
 * `chunk` samples (a short last chunk is a short chunk).  meters_out (or NULL: no meters):
 * [channels][ceil(n / chunk)][FRT_LEVELS_METER_FIELDS]; long_out (or NULL: no long levels, nothing carried):
 * [channels][nblocks][2] = {level, level dB}.  Host or device outputs. */
int frt_levels_run(frt_levels* h, const void* x, int dtype, int64_t n, int64_t ld, int64_t chunk, double* meters_out,
                   double* long_out, int64_t* nblocks);
/* Interactive form: one handle_new_data of channels [0, nch) — the whole push is one chunk, n = 0 is the
 * reference's empty chunk.  x_host: [nch][n] float64; meters_out [nch][FRT_LEVELS_METER_FIELDS] or NULL;
 * long_out [nch][nblocks][2] or NULL (needs nch = channels).  One upload, the launches, one download. */
int frt_levels_push(frt_levels* h, const double* x_host, int nch, int64_t n, double* meters_out, double* long_out,
                    int64_t* nblocks);
/* Subsampler.push (longlevels.py:54-91): x through the Ndec stages as given (no squaring), [::2] keeping index 0
 * of THIS call at every stage; out [channels][nout] (host or device).  Uses the stage state only. */
int64_t frt_levels_subsample_length(const frt_levels* h, int64_t n);
int frt_levels_subsample(frt_levels* h, const void* x, int dtype, int64_t n, int64_t ld, double* out, int64_t* nout);
/* the last `count` <= history_len ring entries per channel, oldest first, 0 where nothing was pushed yet:
 * out [channels][count] (host or device) */
int frt_levels_history(frt_levels* h, int64_t count, double* out);

/* ---- S1: oscilloscope (Scope_Widget) ----------------------------------------------------------------------------------
 * Per refresh k of stream s, the stream seen up to e = ends[k] (samples before index 0 are zeros, as in a fresh ring), width w
 * (int(timerange * 1e-3 * SAMPLING_RATE), host arithmetic), h = w / 2 (friture/scope.py:78-135):
 *   trigger mode (scrolling = 0, timerange <= 500 ms): the region is the w samples x[r0, r0 + w) of row 0, r0 = e - 2w + h;
 *     level = (max(region) * 2.) / 3. in float64 (a NaN in the region: no trigger); the trigger is the first i with
 *     region[i] < level && region[i + 1] >= level; the trace is x[:, e - 2w + i, e - 2w + i + 2h) of every row.
 *   scrolling mode (scrolling = 1, timerange > 500 ms): the trace is x[:, e - w, e), always.
 * Float32 input is compared in float64 (a float32 sample widens exactly; the level is never rounded to float32). */
#define FRT_SCOPE_NO_TRIGGER (-9223372036854775807LL - 1) /* start_out of a refresh without a crossing             */
#define FRT_SCOPE_TRACE_RAW 1                              /* trace_kind bit: the samples y                          */
#define FRT_SCOPE_TRACE_SCALED 2                           /* trace_kind bit: scaled_y = 1. - (y + 1) / 2. (scope.py:129) */
/* samples per trace row: 2 (width / 2) in trigger mode, width in scrolling mode */
int64_t frt_scope_trace_length(int64_t width, int scrolling);
/* x: streams x rows x n samples, x[s * ld_stream + r * ld_row + t], float32 (dtype 0) or float64 (dtype 1), host or device
 * (a host input is staged as the whole span it covers).  ends: [n_refresh] HOST int64, sorted, each in [0, n].  Only row 0
 * of each stream triggers; the other rows are cut at the same place.
 * start_out: [streams][n_refresh] absolute index of the trace's first sample (may be negative), FRT_SCOPE_NO_TRIGGER when no
 * crossing was found.  trace_out (or NULL): for each bit set in trace_kind, raw first, a block of
 * [streams][rows][n_refresh][frt_scope_trace_length] doubles; written only for the refreshes that triggered.  Host or device
 * outputs; one synchronisation at the end.  width < 1: FRT_ERR_INVALID (the reference raises on an empty region). */
int frt_scope_run(const void* x, int dtype, int streams, int rows, int64_t n, int64_t ld_row, int64_t ld_stream, const int64_t* ends,
                  int64_t n_refresh, int64_t width, int scrolling, int64_t* start_out, double* trace_out, int trace_kind);

/* ---- P1: spectrum / octave-spectrum plot curves with peak hold (SpectrumPlotWidget, HistPlot) ----------------------------
 * Per refresh r of stream s, y the row of `bins` dB values (friture/spectrumPlotWidget.py:122-200, friture/histplot.py:77-130):
 *   toScreen(v) = (v - cmin) / (cmax - cmin), or 0 + 0. * v when cmax == cmin (NaN for +-inf and NaN)
 *   scaled_y = 1. - toScreen(y);  z = (y - cmin) / (|M - cmin| + 1e-3), M = max(y) with NaN propagating
 *   peak hold on the old state (peak, int, decay): peak < y -> (y, 1, c); else int < 0.2 -> peak += decay, decay += c;
 *     else int *= 0.975;  c = frt_curves_decay_step() = 20 log10(1 - 3e-6) 5000
 *   scaled_peak = 1. - toScreen(peak);  z_peak = int
 * All in float64; float32 input is widened first.  The caller swaps a reversed range and resets the state on a bin-count
 * change (peak -500, int 0, decay c), as the widgets do. */
double frt_curves_decay_step(void);
/* y: y[s * ld_stream + r * ld_refresh + b], float32 (dtype 0) or float64 (dtype 1), host or device (a host input is staged as
 * the whole span it covers).  state: [streams][3][bins] doubles (peak, int, decay), read, and written back when peaks != 0;
 * peaks == 0 leaves it as it is (peak outputs then show it unchanged); may be NULL when peaks == 0 and no peak output is asked.
 * scaled_y, z, scaled_peak, z_peak (each may be NULL): [streams][n_refresh][bins] doubles, or [streams][1][bins] with
 * keep_last (the final refresh only; the state still walks every refresh).  Host or device inputs and outputs in any mix;
 * one synchronisation at the end. */
int frt_curves_run(const void* y, int dtype, int streams, int64_t n_refresh, int64_t bins, int64_t ld_refresh, int64_t ld_stream,
                   double cmin, double cmax, double* state, int peaks, int keep_last, double* scaled_y, double* z,
                   double* scaled_peak, double* z_peak);

/* ---- P2: the spectrum widget's chain over whole recordings (Spectrum_Widget.handle_new_data, friture/spectrum.py:125-184) ----
 * Between the float64 STFT engine and frt_curves_run: per refresh r of stream s, which owns the PSD frames
 * frame_start[r] .. frame_start[r + 1] - 1 (n of them, accumulated in frame order; friture/signal/exp_smoothing.py:91-107):
 *   sp = alpha * sum_t psd[t] * kernel[nk - n + t] + previous * (1 - alpha)^n      (n > nk: the first nk frames, decay 0)
 *   dB = 10 log10(sp + 1e-30) + weight_db   (rows == 2, dual channels: 10 log10(sp2 + 1e-30) - 10 log10(sp1 + 1e-30), no weight)
 *   peak = argmax(dB);  pitch = argmax(sp1[k] sp1[2k] sp1[3k], k < bins / 3)   (spectrum.py:103-123); first index wins ties; NaNs
 *   are skipped (PSD >= 0 is the precondition)
 * Refreshes are walked in time order and each (stream, row, bin) is a fixed sequence of IEEE operations: a recording cut into
 * several calls with the state carried gives the same bits as one call.
 * psd: psd[(s * rows + row) * ld_row + f * ld_frame + b], float32 (dtype 0) or float64 (dtype 1), host or device — the slab
 * frt_stft_run leaves (ld_frame = bins, ld_row = n_frames * bins).  frame_start: [n_refresh + 1] HOST int64, sorted, within
 * [0, n_frames].  kernel: [nk] HOST doubles, (1 - alpha)^(nk - 1 .. 0).  weight_db: [bins] or NULL.  state: [streams][rows][bins]
 * smoothed spectra, read and written.  db_out: [streams][R'][bins] with R' = n_refresh, or 1 with keep_last (the final refresh;
 * the state still walks every refresh); stream s starts at s * ld_db_stream (0 = packed; a padded layout needs a device
 * output).  peak_index_out, pitch_index_out: [streams][R'].  Host or device buffers in any mix; launched on the null stream when
 * any buffer is in device memory (STREAM ORDER as for frt_spectrum_post); one synchronisation at the end. */
int frt_spectrum_batch(const void* psd, int dtype, int streams, int rows, int64_t n_frames, int64_t bins, int64_t ld_frame,
                       int64_t ld_row, const int64_t* frame_start, int64_t n_refresh, const double* kernel, int nk, double alpha,
                       const double* weight_db, double* state, int keep_last, double* db_out, int64_t ld_db_stream,
                       int* peak_index_out, int* pitch_index_out);

/* ---- P3: the spectrogram widget's screen stages over whole recordings (Spectrogram_Widget.handle_new_data,
 * friture/spectrogram.py:161-173) ----
 * One time slab of S streams behind frt_stft_run(FRT_STFT_NORM): per output column c with source frame f = src[c] and weight a[c]
 *   cur, prev = np.interp(targets, freq, frame f), np.interp(targets, freq, frame f - 1)   (friture/signal/frequency_resampler.py:67-83;
 *     frame -1 is old_in, the column the time resampler carried into the slab)
 *   v = cur (1 - a) + prev a                                  (friture/signal/online_linear_2D_resampler.py:61-97, linear_interp.py:57-60)
 *   pixel = lut256[int(clip(v, 0, 1) * 255)]                  (friture/signal/color_tranform.py:48-51)
 * written with the frequency axis flipped (friture/spectrogram_image.py:82-92: row 0 = highest frequency).  src[c] < 0 marks a
 * column the resampler allocated and never wrote (online_linear_2D_resampler.py:66-68): lut256[0].  The operations and their
 * order are those of frt_screen_columns and frt_specgram_push, so the pixels are theirs bit for bit; the scalar recurrence that
 * yields (src, a) stays with the caller.  Every frame is frequency-resampled once, whatever the number of columns that read it,
 * and frames no column reads are not touched.
 * norm: norm[s * ld_stream + f * ld_frame + b], n_frames >= 1 frames of nb bins, host or device.  freq [nb], targets [height],
 * lut256 [256], src, a [n_cols]: HOST tables; the source frames ascend.  old_in, old_out: [streams][height], host or device,
 * distinct buffers; old_out receives the frequency-resampled last frame of the slab.  pixels: pixels[s * height * ld_pixel + row *
 * ld_pixel + col_offset + c], so that the slabs of a recording fill one image; a host block is written whole (col_offset 0,
 * ld_pixel = n_cols).  n_cols = 0 only carries the column.  Any height (screen rows are processed in blocks).  Launched on the
 * null stream (STREAM ORDER as for frt_spectrum_post); one synchronisation at the end. */
int frt_specgram_batch(const double* norm, int streams, int64_t n_frames, int nb, int64_t ld_frame, int64_t ld_stream,
                       const double* freq, const double* targets, int height, const int* src, const double* a, int64_t n_cols,
                       const double* old_in, double* old_out, const uint32_t* lut256, uint32_t* pixels, int64_t col_offset,
                       int64_t ld_pixel);

/* ---- R1: rational-ratio polyphase sample-rate converter (Resampler: recordings at other rates for the 48 kHz chains) -----
 * The reference has no such component; this is the definition.  With g = gcd(rate_in, rate_out): L = rate_out / g,
 * M = rate_in / g, Q = max(L, M), C = zeros * Q.  The prototype h[0 .. 2C] (host, float64) is a Kaiser-windowed sinc:
 *   beta = 0.1102 (A - 8.7), dw = (A - 8) / (2.285 * 2C) rad/sample, fc = 0.5 / Q - dw / (4 pi) cycles/sample (the stop band
 *   begins at the narrower Nyquist, so nothing folds back), h[n] = 2 fc sinc(2 fc (n - C)) kaiser(2C + 1, beta)[n], h *= L / sum(h)
 * The output is zero-phase:
 *   y[m] = sum_k h[C + m M - k L] x[k]   over every k with 0 <= C + m M - k L <= 2C;  x[k] = 0 outside the stream
 * i.e. K = ceil((2C + 1) / L) taps per output, the first input being kb(m) = ceil((m M - C) / L), in 64-bit index arithmetic.
 * After N inputs in total a stream that is not flushed has emitted max(0, ceil((N L - C) / M)) outputs (every tap of theirs has
 * arrived), a flushed one ceil(N L / M) (later inputs are zeros).  The carried tail is the last K - 1 inputs: kb of the next
 * output never reaches behind it.
 * Arithmetic is float64 throughout (a float32 sample widens exactly, a float32 output is one rounding of the float64 sum), with
 * fused multiply-adds.  One output is one chain acc = fma(h[..], x[kb + j], acc), j = 0 .. K - 1 from acc = 0: its order is
 * fixed by the position in the period (m mod L) and by nothing else, so a stream cut into calls, run beside other streams or in
 * another grid gives the same bits. */
typedef struct frt_resample frt_resample;
/* prototype: [2C + 1] HOST doubles; the handle keeps the table [K][L] (column q: the coefficients of the outputs m = q mod L) on
 * the device.  FRT_ERR_INVALID, before any device call: L, M or C not positive, L == M (rate_in == rate_out), L and M with a
 * common factor, L * K > 2^20 coefficients, streams outside 1 .. 65535. */
int frt_resample_create(frt_resample** h, int64_t L, int64_t M, int64_t C, const double* prototype, int streams);
void frt_resample_destroy(frt_resample* h);
int frt_resample_set_stream(frt_resample* h, void* hip_stream);
/* One call over all streams.  x: [streams][ld] float32 (x_dtype 0) or float64 (1), the n inputs first_in .. first_in + n - 1 of
 * every stream (n = 0: x may be NULL).  tail_in: [streams][K - 1] doubles, the inputs before first_in, zeros before the stream's
 * start (NULL: zeros, for first_in = 0 only); tail_out (or NULL): the same for the next call, a buffer distinct from tail_in.
 * y: [streams][ldy] float32 (y_dtype 0) or float64 (1), the n_out outputs first_out .. first_out + n_out - 1; inputs from
 * first_in + n on are zeros.  FRT_ERR_INVALID unless max(0, ceil((first_in L - C) / M)) <= first_out and first_out + n_out <=
 * ceil((first_in + n) L / M): the caller chooses between the flushed and the unflushed count.  Host or device buffers in any
 * mix (host ones are staged); one synchronisation at the end. */
int frt_resample_run(frt_resample* h, const void* x, int x_dtype, int64_t n, int64_t ld, const double* tail_in, double* tail_out,
                     int64_t first_in, int64_t first_out, int64_t n_out, void* y, int y_dtype, int64_t ldy);

/* ---- R2: PCM ingest (recording.py: interleaved integer / float recordings, the data chunk of a WAV file) ------------------
 * The reference has no such component (its audio arrives as float32 already); this is the definition.  A PCM buffer is
 * n_frames_total frames of `channels` interleaved little-endian samples:
 *   format  name  bytes                          value of a sample
 *   0       u8    1                              (b - 128) * 2^-7
 *   1       s16   2                              v * 2^-15
 *   2       s24   3, packed, bit 23 the sign     v * 2^-23
 *   3       s32   4                              v * 2^-31
 *   4       f32   4                              the value itself
 *   5       f64   8                              the value itself
 * Full scale is [-1, 1).  Output row s, sample t is the value of channel select[s] of frame first_frame + t, as float32
 * (y_dtype 0) or float64 (1).  Every value is exact in float64, those of u8, s16 and s24 in float32 too, so the output is
 * defined to the bit: float64 is the exact value, float32 ONE round-to-nearest-even of it (s32: int -> float64 -> scale ->
 * float32; f64: one conversion); float32 subnormals are kept; a NaN stays a NaN (its payload is not specified).
 * One workgroup decodes a tile of frt_pcm_tile_frames(format, channels) frames — a multiple of 64 whose raw bytes are at
 * most 32 KB, tiles counted from frame 0 — reading the tile's bytes once, every channel of them: channels that `select`
 * leaves out are still read (one contiguous span is the point), and no byte outside the requested frames is. */
typedef struct frt_pcm frt_pcm;
int frt_pcm_create(frt_pcm** h);
void frt_pcm_destroy(frt_pcm* h);
int frt_pcm_set_stream(frt_pcm* h, void* hip_stream);
/* pure host: frames per workgroup, or FRT_ERR_INVALID (format outside 0 .. 5, channels outside 1 .. 64) */
int frt_pcm_tile_frames(int format, int channels);
/* data: n_frames_total * channels * width bytes, host or device, at ANY byte address.  select: HOST array of n_select channel
 * indices (repeats and any order allowed).  y: [n_select][ldy], host or device; columns from n_frames on are left alone.
 * Buffers in any mix.  Host data goes up in slabs of whole tiles of at most slab_bytes (0: 64 MB) through two page-locked
 * blocks, slab k + 1 being copied while slab k is in flight; a host y comes back through two more, slab k - 1 being copied
 * out while slab k runs (the handle owns four page-locked blocks); data and y both on the device: one launch.  A handle serves
 * one call at a time.  The result is the same to the bit for every slab_bytes.  One synchronisation at the end.
 * FRT_ERR_INVALID, before any device call: an unknown format or y_dtype, channels outside 1 .. 64, n_select outside
 * 1 .. 65535, a select entry outside [0, channels), frames outside [0, n_frames_total], ldy < n_frames.  n_frames = 0 does
 * nothing. */
int frt_pcm_decode(frt_pcm* h, const void* data, int format, int channels, int64_t n_frames_total, int64_t first_frame,
                   int64_t n_frames, const int32_t* select, int n_select, void* y, int y_dtype, int64_t ldy, int64_t slab_bytes);

/* ---- R3: PCM export (recording.py encode_pcm / save_wav: planar float rows to interleaved PCM, the mirror of R2) ---------
 * Input: x[n_rows][ldx], float32 (x_dtype 0) or float64 (1), host or device.  Output: n_frames frames of `channels`
 * interleaved little-endian samples of one of R2's six formats, n_frames * channels * width bytes at ANY byte address, host
 * or device.  route[c], c in [0, channels), a HOST array: the row that output channel c carries, -1 for silence; repeats
 * and any order allowed (the mirror of `select`).
 * An integer format of b bits (u8 8, s16 16, s24 24, s32 32), v the sample converted exactly to float64 (mode 0):
 *   t = v * 2^(b-1)                      exact in float64
 *   t = t + d                            with dither only: one float64 addition, d below
 *   r = rint(t)                          round half to even
 *   q = clamp(r, -2^(b-1), 2^(b-1) - 1)  a NaN encodes as q = 0
 * u8 stores q + 128, s24 the low three bytes of q.  A silent channel stores 0 (u8: 128).  clipped[c], an int64 HOST array of
 * `channels` entries (or NULL): the call ADDS, per output channel, the number of samples whose r lay outside the range or was
 * NaN; silent channels and the float formats add nothing.
 * f32 from float32 and f64 from float64 are bit copies (a NaN stays a NaN, its payload is not specified), f64 from float32
 * the exact widening, f32 from float64 ONE round-to-nearest-even (subnormals kept, overflow to infinity); silence is +0.0.
 * This inverts R2's scale: encode(decode(raw)) == raw for every byte string of an integer format with float64 rows, and
 * with float32 rows for u8, s16 and s24 (s32 through float32 does not round-trip).
 * mode 1 ("player", s16 only, no dither): q = (int16) trunc(32767 * min(max(v, -1), 1)), the float64 product truncated toward
 * zero — the statements of friture/playback/player.py:173-177; a NaN gives 0; clipped[c] counts |v| > 1 and NaN.
 * Dither (integer formats, mode 0): Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85) on the counter (f & 0xffffffff, f >> 32, c, 0), f = frame0 + i the absolute frame index and c the OUTPUT
 * channel, with the key (seed & 0xffffffff, seed >> 32).  With outputs o0 .. o3,
 *   d = ((int)(o0 >> 8) - (int)(o1 >> 8)) * 2^-24
 * a triangular density on (-1, 1) LSB, exact in float64.  The bytes depend on (x, route, format, seed, frame0) only: not on
 * tile, slab, launch shape or how a recording is cut into calls.
 * One workgroup encodes a tile of frt_pcm_tile_frames(format, channels) frames, tiles counted from frame 0 of the output;
 * no byte outside the n_frames * channels * width bytes of dst is written. */
typedef struct frt_pcmenc frt_pcmenc;
int frt_pcmenc_create(frt_pcmenc** h);             /* allocates nothing on the device */
void frt_pcmenc_destroy(frt_pcmenc* h);            /* no device call for a handle that never reached the device */
int frt_pcmenc_set_stream(frt_pcmenc* h, void* hip_stream);
/* A host x (the rows the route names, once each) or a host dst goes through the handle's page-locked blocks in slabs of whole
 * tiles of at most slab_bytes encoded bytes (0: 64 MB): the host copy of slab k + 1's rows and of slab k - 1's bytes run while
 * slab k is in flight (uploads, kernels and downloads share the handle's one stream and run one after the other there); x and
 * dst both on the device: one launch.  The clip counts are added up on the device per workgroup and then, with atomic adds, into
 * a [16][64] int64 table (row: workgroup mod 16) that the call zeroes, reads back once at the end (8 KB) and sums on the host.
 * A handle serves one call at a time.  The result is the same to the bit for every slab_bytes.  One synchronisation
 * at the end.  FRT_ERR_INVALID, before any device call: a null handle, an unknown format, x_dtype, mode or dither, channels
 * outside 1 .. 64, n_rows outside 1 .. 65535, a route entry outside [-1, n_rows), n_frames < 0, frame0 < 0, frame0 + n_frames
 * > 2^50, ldx < n_frames, slab_bytes < 0, mode 1 with a format other than s16 or with dither, dither with a float format.
 * n_frames = 0 does nothing. */
int frt_pcmenc_encode(frt_pcmenc* h, const void* x, int x_dtype, int n_rows, int64_t ldx, int64_t n_frames, int64_t frame0,
                      const int32_t* route, int channels, int format, int mode, int dither, uint64_t seed, void* dst,
                      int64_t* clipped, int64_t slab_bytes);

/* ---- L2: programme loudness (ITU-R BS.1770-4 / EBU R 128) and true peak (LoudnessBatch) -------------------------------
 * The reference has no such component; this is the definition.  Samples x[s][k] at 48 kHz, the one rate for which BS.1770
 * states its coefficients; float64 arithmetic whatever the input dtype (a float32 sample widens exactly).
 * K-weighting: two biquads in series, each in direct form II transposed in the operation order of lfilter_float64_1D
 * (y = z0 + b0 x; z0 = (z1 + x b1) - y a1; z1 = x b2 - y a2), no fused multiply-add, zero state at the start of a stream:
 *   stage 1  b = 1.53512485958697, -2.69169618940638, 1.19839281085285   a = 1, -1.69065929318241, 0.73248077421585
 *   stage 2  b = 1, -2, 1                                                 a = 1, -1.99004745483398, 0.99007225036621
 * Sub-blocks of B = 4800 samples (100 ms) on the absolute grid of the stream; only whole sub-blocks have an energy
 * e[s][b] = sum of y^2.  Its order of additions is fixed by the position in the sub-block: 64 cells of 75 samples, each cell
 * one ascending chain from 0, the 64 cell sums added in ascending order from 0.  The filter state at the start of cell c of
 * sub-block b is A^(75 c) s_b + P_c with P_0 = 0, P_(c+1) = A^75 P_c + z_c (z_c: the state after cell c entered with the zero
 * state) and s_(b+1) = A^4800 s_b + P_64; A^n is the 4x4 matrix whose column j is the state n zero samples after the unit
 * state e_j, formed by running the biquads; every matrix-vector product is per row (((m0 v0 + m1 v1) + m2 v2) + m3 v3) + z.
 * This is the sequential recurrence up to rounding (distance measured: DESIGN L2) and the same bits for every grid, stream
 * count and cut of a recording into calls.
 * Peaks per sub-block: the sample peak max |x|; the true peak max |u| over the outputs u[m], 4 B b <= m < 4 B (b + 1), that
 * exist (m < 4 N for a flushed stream of N samples), u being R1's output for L = 4, M = 1, C = 4 tp_zeros and the given
 * prototype (R1's definition as it stands: one ascending fma chain per output, x = 0 outside the stream; K = 2 tp_zeros + 1).
 * A stream that is not flushed has emitted max(0, floor((N - tp_zeros) / B)) sub-blocks after N samples (the last true-peak tap
 * of a sub-block arrives tp_zeros samples past its end); a flushed one has floor(N / B) energies and ceil(N / B) peak entries
 * (a partial last sub-block has peaks and no energy).
 * Programmes: P = streams / C programmes of C channels with weights G[c] >= 0:
 *   z400[p][j] = (sum_c G[c] (((e[j] + e[j+1]) + e[j+2]) + e[j+3])) / 19200, channels ascending from 0
 *   z3s[p][j]  = the same over the 30 sub-blocks from j on, / 144000
 *   l(z) = -0.691 + 10 log10 z, -inf for z = 0;  momentary = l(z400), short-term = l(z3s)
 * Integrated: over the blocks with l(z400) > -70, Gamma = l(their mean) - 10; the result is l(mean of the z400 with l > -70
 * and l > Gamma) over EVERY block of the stream so far, -inf when none passes the absolute gate.  (Loudness range, EBU Tech
 * 3342, is a sort of the short-term series: friture_amd/loudness.py.)
 * The state after n_in samples and E sub-blocks with an energy is one array of doubles,
 *   filter states [S][4] at the start of sub-block E | samples E B - tp_zeros .. n_in - 1 [S][n_in - E B + tp_zeros] (zeros
 *   before the stream) | the last min(29, E) energies [S][..] | z400 [P][max(0, E - 3)] | z3s [P][max(0, E - 29)]
 * of frt_loudness_state_length(h, n_in, E) entries, and the results of a call that takes the stream from (first_in, E) to
 * (first_in + n, E') with K' peak entries are another,
 *   energy [S][E' - E] | true peak [S][K' - E] | sample peak [S][K' - E] | momentary [P][new z400] | short-term [P][new z3s] |
 *   integrated [P]
 * (linear values; with true_peak = 0 the interpolator is skipped and the true-peak entries are 0). */
typedef struct frt_loudness frt_loudness;
/* weights: [channels_per_programme] HOST doubles; prototype: [8 tp_zeros + 1] HOST doubles.  FRT_ERR_INVALID, before any
 * device call: streams outside 1 .. 65535 or no multiple of channels_per_programme (1 .. 64), a negative or non-finite weight,
 * tp_zeros outside 1 .. 512, a non-finite prototype. */
int frt_loudness_create(frt_loudness** h, int streams, int channels_per_programme, const double* weights, int tp_zeros,
                        const double* prototype);
void frt_loudness_destroy(frt_loudness* h);
int frt_loudness_set_stream(frt_loudness* h, void* hip_stream);
/* pure host: the entries of a state; FRT_ERR_INVALID for a null handle, negative counts or blocks * 4800 > n_in */
int64_t frt_loudness_state_length(const frt_loudness* h, int64_t n_in, int64_t blocks);
/* One call over all streams.  x: [streams][ld] float32 (x_dtype 0) or float64 (1), the samples first_in .. first_in + n - 1
 * (n = 0: x may be NULL).  state_in: the state after first_in samples of a stream that was NOT flushed (NULL: a new stream,
 * first_in = 0 only); state_out: the state after the call, a buffer distinct from state_in (after flush = 1 it is laid out for
 * E' = floor(N / B) and is final); out: the results.  Host or device buffers in any mix (host ones are staged); one
 * synchronisation at the end. */
int frt_loudness_run(frt_loudness* h, const void* x, int x_dtype, int64_t n, int64_t ld, const double* state_in, double* state_out,
                     int64_t first_in, int flush, int true_peak, double* out);

/* ---- X1: Welch cross-spectra, transfer function and coherence of two rows (TransferBatch) ----------------------------
 * The reference has no such component; this is the definition.  A stream is a pair of rows at one sample rate (nothing here
 * depends on it): x = row 0, the reference, and y = row 1, the measured signal; float64 arithmetic whatever the input dtype
 * (a float32 sample widens exactly).
 * Parameters: fft_size N, a power of two in 64 .. 8192; hop >= 1, which may exceed N; a window w of N doubles; average = K >= 1
 * frames per estimate, or 0 for one running estimate over everything seen; delay d, |d| <= 96000 samples.
 * Frames: frame f is x[a + f hop .. + N) and y[b + f hop .. + N) with a = max(0, -d), b = max(0, d): a positive delay means
 * that the measured row lags.  After n samples in total there are F(n) = max(0, floor((n - |d| - N) / hop) + 1) frames.  Per
 * frame X = rfft(x w) / N and Y = rfft(y w) / N over the bins 0 .. N/2 (with this scale |X|^2 is K1's FRT_STFT_PSD).
 * Estimates: estimate e is the mean over its frames of |X|^2 (sxx), |Y|^2 (syy) and conj(X) Y (sxy, the convention of
 * scipy.signal.csd(x, y)).  With average = K it covers the frames e K .. e K + K - 1 and is emitted by the call in which its
 * last frame completes; a running estimate covers every frame so far and is emitted by every call after which F >= 1.
 * Derived, written by the device: h1 = sxy / sxx and coherence = |sxy|^2 / (sxx syy); where the denominator is 0 (a silent
 * row) h1 = 0 and coherence = 0.  Both rows of a frame share one transform, so a row's spectrum is accurate to about 1e-16 of
 * the LOUDER row's; a row whose windowed frame is all zeros has the spectrum 0 exactly.
 * Summation order, part of the definition: within an estimate the frames are grouped into runs of RUN = 16 consecutive frames
 * on the estimate's own frame grid (the last run of an estimate may be short); a run's sum is sequential in frame order from
 * 0; the run sums are added sequentially in run order from 0, then divided by the frame count.  No atomics: the same bits
 * for every cut of a recording into calls, every slab size and every batch.
 * The state after n samples is one array of doubles, S the number of pairs,
 *   the sum over the complete runs of the open estimate [S][N/2 + 1][4] (sxx, syy, Re sxy, Im sxy) | the sum of the open run
 *   [S][N/2 + 1][4] | row 0 from min(n, a + F(n) hop) on [S][..] | row 1 from min(n, b + F(n) hop) on [S][..]
 * (at most N + |d| samples per row), and the results of a call that emits E estimates are another,
 *   sxy [S][E][N/2 + 1][2] | h1 [S][E][N/2 + 1][2] | sxx [S][E][N/2 + 1] | syy [S][E][N/2 + 1] | coherence [S][E][N/2 + 1]
 * (complex values as re, im).  Out of scope: N = 16384, fractional delays, exponential averaging.  The impulse response
 * behind an h1 and its use on a signal: X2. */
typedef struct frt_transfer frt_transfer;
/* window: [fft_size] HOST doubles.  FRT_ERR_INVALID, before any device call: fft_size below 64 or no power of two, hop outside
 * 1 .. 2^30, average < 0, |delay| > 96000, a non-finite window; FRT_ERR_UNSUPPORTED: a power of two above 8192. */
int frt_transfer_create(frt_transfer** h, int fft_size, int64_t hop, const double* window, int64_t average, int delay);
void frt_transfer_destroy(frt_transfer* h);
/* Launches go to the null stream unless another one is set here. */
int frt_transfer_set_stream(frt_transfer* h, void* hip_stream);
/* One call over `pairs` streams.  x: float32 (x_dtype 0) or float64 (1); sample t of row r of pair s is x[s pair_stride +
 * r row_stride + t] (strides in elements, row_stride >= n), the samples first_in .. first_in + n - 1 of the streams (n = 0: x
 * may be NULL).  state_in: the state after first_in samples (NULL: new streams, first_in = 0 only); state_out: the state
 * after the call, a buffer distinct from state_in; out: the results (may be NULL when no estimate is emitted);
 * n_estimates_out (may be NULL): E.  The run partials of one launch stay within scratch_bytes (at least one run per launch):
 * the frames are cut into time slabs, and the result does not depend on it.  Host or device buffers in any mix (host ones are
 * staged); one synchronisation at the end.  FRT_ERR_INVALID, before any device call: a null handle, an unknown x_dtype,
 * pairs outside 1 .. 65535, n < 0, a bad stride, first_in < 0 or first_in + n > 2^40, first_in > 0 without state_in, a null
 * state_out or one equal to state_in, scratch_bytes < 0, a null out when estimates are emitted. */
int frt_transfer_run(frt_transfer* h, const void* x, int x_dtype, int pairs, int64_t n, int64_t row_stride, int64_t pair_stride,
                     const double* state_in, double* state_out, int64_t first_in, int64_t scratch_bytes, double* out,
                     int64_t* n_estimates_out);

/* ---- X2: uniformly partitioned FFT convolution of rows with a caller's FIR (ConvolveBatch) ----------------------------
 * The reference has no such component; this is the definition.  A stream is one row x[s][t], t counted from the start of the
 * stream across calls, x = 0 before it.  The taps h are L doubles, 1 <= L <= 2^18: one filter for all streams, or one per
 * stream.  The output is y[s][t] = sum_{l < L} h[s][l] x[s][t - l]; float64 arithmetic whatever the input dtype (a float32
 * sample widens exactly), and a float32 output is one rounding of the float64 value.
 * Block size: B, a power of two in 64 .. 4096; by default the smallest power of two >= L, clamped to 64 .. 4096.
 * P = ceil(L / B) <= 4096 partitions; H_p = the real 2 B-point transform of h[p B .. p B + B) followed by B zeros, bins
 * 0 .. B.  X_w = the real 2 B-point transform of the window x[(w - 1) B .. (w + 1) B) (overlap-save).
 * Output blocks: block j is y[j B .. j B + B), on the grid of absolute sample indices, which depends on nothing but B.  It is
 * the last B samples of the inverse real 2 B-point transform of Y_j = sum_{p = 0 .. P - 1} X_{j - p} H_p.
 * Order of the arithmetic, part of the definition: a real 2 B-point transform is one B-point complex transform of
 * z[n] = x[2 n] + i x[2 n + 1] and the unpack X[k] = Ze[k] + w^k Zo[k], Ze = (Z[k] + conj Z[B - k]) / 2, Zo = -i (Z[k] - conj
 * Z[B - k]) / 2, w = exp(-i pi / B); Y_j[k] starts at 0 and takes the terms p = 0, 1, .. in order, each as four fused
 * multiply-adds (re += Xr Hr; re -= Xi Hi; im += Xr Hi; im += Xi Hr); the inverse is the pack Z[k] = ((A + B') + i conj(w^k)
 * (A - B')) / (2 B), A = Y[k], B' = conj Y[B - k], and one B-point complex transform.  No atomics.
 * Bit identity: a block's bits depend on its whole window, so a call that does not flush emits complete blocks only: after n
 * samples in total a stream has emitted floor(n / B) B outputs.  A flushed stream continues with zeros and has emitted
 * n + L - 1 outputs; after a flush the state is final (none is written).  A recording cut into calls at any sample, any
 * scratch_bytes, and a stream alone or in a batch give the same bits as one whole call.
 * The state after n samples is the input samples max(0, (floor(n / B) - P) B) .. n - 1 as doubles [S][..] (at most
 * (P + 1) B - 1 per stream: frt_convolve_state_length); n itself travels beside it (first_in).
 * Out of scope: fractional or time-varying filters, non-uniform partitions, a low-latency live object, a direct time-domain
 * path for short L.  Deconvolution by spectral division: X4. */
typedef struct frt_convolve frt_convolve;
/* taps: [filters][L] HOST doubles; block: 0 for the default.  The tap spectra H [filters][P][B + 1] are made once, on the
 * device.  FRT_ERR_INVALID, before any device call: a null handle pointer or null taps, L outside 1 .. 2^18, filters outside
 * 1 .. 65535, a block that is neither 0 nor a power of two in 64 .. 4096, P > 4096, non-finite taps; FRT_ERR_UNSUPPORTED: H
 * would exceed 1 GiB. */
int frt_convolve_create(frt_convolve** h, const double* taps, int64_t L, int filters, int block);
void frt_convolve_destroy(frt_convolve* h);
/* Launches go to the null stream unless another one is set here. */
int frt_convolve_set_stream(frt_convolve* h, void* hip_stream);
/* pure host: the doubles of the state of `streams` streams after n_in samples; negative for a null handle or bad counts */
int64_t frt_convolve_state_length(const frt_convolve* h, int streams, int64_t n_in);
/* One call over `streams` rows.  x: float32 (x_dtype 0) or float64 (1), sample t of row s is x[s row_stride + t] (stride in
 * elements, >= n), the samples first_in .. first_in + n - 1 of the streams (n = 0: x may be NULL).  state_in: the state
 * after first_in samples of streams that were not flushed (NULL: new streams, first_in = 0 only); state_out: the state after
 * the call, a buffer distinct from state_in (flush = 1: not written, may be NULL).  y: float32 (y_dtype 0) or float64 (1),
 * y[s y_stride + i] is output floor(first_in / B) B + i; *n_out (may be NULL): the outputs per row, floor((first_in + n) / B) B
 * - floor(first_in / B) B, or with flush = 1 first_in + n + L - 1 - floor(first_in / B) B.  The window spectra of one launch
 * stay within scratch_bytes (at least one block per launch): the blocks are cut into time slabs, each transforming the P - 1
 * windows before its first block again, and the result does not depend on it.  Host or device buffers in any mix (host ones
 * are staged); one synchronisation at the end.  FRT_ERR_INVALID, before any device call: a null handle, an unknown dtype,
 * streams outside 1 .. 65535, a handle of neither 1 nor `streams` filters, n < 0, a bad stride, first_in < 0 or first_in + n
 * > 2^40, first_in > 0 without state_in, a null state_out when samples are carried or one equal to state_in, scratch_bytes < 0,
 * a null y when outputs are emitted. */
int frt_convolve_run(frt_convolve* h, const void* x, int x_dtype, int streams, int64_t n, int64_t row_stride, const double* state_in,
                     double* state_out, int64_t first_in, int flush, int64_t scratch_bytes, void* y, int y_dtype, int64_t y_stride,
                     int64_t* n_out);
/* out[r] = the inverse real n-point transform of the half spectrum spec[r] (bins 0 .. n/2 as re, im; the imaginary parts of
 * bins 0 and n/2 do not count), scaled by 1 / n as numpy.fft.irfft: the impulse response behind X1's h1.  n: a power of two
 * in 64 .. 8192.  Host or device buffers in any mix; launched on hip_stream (NULL: the null stream), synchronised. */
int frt_irfft_rows(const double* spec, int64_t rows, int n, double* out, void* hip_stream);

/* ---- X3: reverberation time and clarity from impulse responses (DecayBatch) -----------------------------------------------
 * The reference has no such component; this is the definition (the ISO 3382 quantities by Schroeder's backward integration).
 * A row x[0 .. T) is float32 or float64, 1 <= T <= 2^24; fs defaults to 48000.  All arithmetic is float64: e[t] = (double)x[t]^2.
 * Parameters: block W = 480 samples (any integer in 8 .. 65536), onset_db = -20, noise_tail = 0.1, margin_db = 10.
 * 1. Peak: p is the smallest t with |x[t]| = max |x|.  A row that is all zero, or that holds a sample that is not finite, is
 *    a dead row: NaN in every float output, -1 in every index output; it never faults and never affects its neighbours.  (A
 *    row whose given onset or truncation lies outside its range, which only device arrays can carry this far, is dead too.)
 * 2. Onset: t0 is the smallest t with |x[t]| >= c |x[p]|, c the double nearest 10^(onset_db / 20), made on the host, the
 *    product rounded to double: the test is exact.  Or t0 is given per row, 0 <= t0 < T (the bands of one response share
 *    the broadband onset).
 * 3. Noise: nb = floor(T / W) blocks, q[k] = the sum of e over [k W, (k + 1) W); nt = max(1, ceil(noise_tail nb));
 *    N0 = (the sum of the last nt block sums) / (nt W), 0 when nb = 0.
 * 4. Truncation: auto: t1 = k W for the smallest k > floor(p / W) with q[k] <= W N0 10^(margin_db / 10), T if there is none;
 *    none: t1 = T; or given per row, t0 < t1 <= T.  A row whose given onset lies at or behind its automatic truncation
 *    (t1 <= t0) is a dead row.
 * 5. Schroeder integral and decay curve, t0 <= t < t1: E[t] = e[t] + .. + e[t1 - 1], L[t] = 10 log10(E[t] / E[t0]).
 * 6. Decay times over the ranges (hi, lo): EDT (0, -10), T10 (-5, -15), T20 (-5, -25), T30 (-5, -35).  a = the smallest t
 *    with L[t] <= hi (EDT: a = t0), b = the smallest t with L[t] <= lo; a least-squares line of L[t] over k = t - a, a <= t < b
 *    (the sums of k and k^2 are closed forms); RT = -60 / (slope fs) seconds, r2 the squared correlation coefficient of the
 *    same fit; NaN when lo is not reached before t1 or b - a < 2.
 * 7. Energy ratios, n50 = round(0.05 fs), n80 = round(0.08 fs), E[u] = 0 for u >= t1: C50 = 10 log10((E[t0] - E[t0 + n50]) /
 *    E[t0 + n50]), C80 the same with n80, D50 = (E[t0] - E[t0 + n50]) / E[t0] (a short response: C = +inf, D50 = 1);
 *    Ts = sum (t - t0) e[t] / E[t0] / fs over [t0, t1).
 * 8. level_db = 10 log10 E[t0]; noise_db = 10 log10 N0; dynamic_range = 10 log10(max_k q[k] / (W N0)), NaN when nb = 0 and
 *    +inf when N0 = 0; the integers peak, onset, truncation.
 * 9. On request the curve L[t0 + j step], j < ceil(T / step); entries at or behind t1 are NaN.
 * Order of the sums, per row and anchored at its sample 0 (so the bits of a row depend on no other row, on no slab size, row
 * stride or input dtype): q[k] by 64 lanes (8 for W < 64), lane i adding e[k W + i], e[k W + i + 64], .. in order, the lanes
 * folded by a butterfly.  E[t]: tiles of frt_decay_tile() = 512 samples, 8 consecutive samples per lane; E[t] = ((e[t] + ..
 * + e[last of the lane], added from the back) + a Kogge-Stone scan of the totals of the lanes behind) + the totals of the
 * tiles behind, added one by one from the row's last tile.  The crossings are counts (a = t0 + the number of t with L[t] >
 * hi), a sample belongs to the range its own L falls in, and the comparisons are made on E against E[t0] 10^(lo / 10), those
 * factors made on the host: L is monotone up to the last bit of E, and an input whose crossing hangs on that bit has no
 * defined index.  The regression sums: per tile lane sums in sample order folded by a butterfly, tile sums 64 apart added
 * in order and folded by a butterfly.  No atomics.
 * There is no carried state: a decay is integrated from its end, so a response is given whole.  Out of scope as well:
 * Lundeby's iteration, the tail-compensation term, noise subtraction, sample rates handled in any way other than the fs
 * argument.  IIR band filters in front of it (Butterworth band-passes on the same band edges) are X6. */
typedef struct frt_decay frt_decay;
/* pure host: the tile length of the scan */
int frt_decay_tile(void);
/* FRT_ERR_INVALID, before any device call: a null handle pointer, fs outside 100 .. 1e7, block outside 8 .. 65536, onset_db
 * above 0, noise_tail outside (0, 1], margin_db below 0, anything not finite. */
int frt_decay_create(frt_decay** h, double fs, int block, double onset_db, double noise_tail, double margin_db);
void frt_decay_destroy(frt_decay* h);
/* Launches go to the null stream unless another one is set here. */
int frt_decay_set_stream(frt_decay* h, void* hip_stream);
/* One call over `rows` rows of n samples.  x: float32 (x_dtype 0) or float64 (1), sample t of row r is x[r row_stride + t]
 * (stride in elements, >= n).  onset: [rows] or NULL (step 2 finds it).  truncate_mode 0: t1 = n; 1: auto; 2: truncation
 * [rows] gives t1.  params [rows][15]: edt, t10, t20, t30 | r2 of the four | c50, c80, d50, ts | level_db, noise_db,
 * dynamic_range.  indices [rows][3]: peak, onset, truncation.  curve [rows][ceil(n / curve_step)], or NULL with curve_step 0.
 * The rows are cut into slabs whose scratch stays within scratch_bytes (at least one row per launch); the result does not
 * depend on it.  Host or device buffers in any mix (host ones are staged); one synchronisation at the end.
 * FRT_ERR_INVALID, before any launch: a null handle, an unknown x_dtype, rows outside 1 .. 65535, n outside 1 .. 2^24, a null
 * x, a bad stride, an unknown truncate_mode, truncation without mode 2 or mode 2 without it, curve_step < 0, a curve without
 * a step or a step without a curve, scratch_bytes < 0, null params or indices, and in host arrays an onset outside 0 .. n - 1
 * or a truncation outside 1 .. n. */
int frt_decay_run(frt_decay* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, const int64_t* onset,
                  int truncate_mode, const int64_t* truncation, int64_t curve_step, int64_t scratch_bytes, double* params,
                  int64_t* indices, double* curve);

/* ---- X4: long real transforms and deconvolution by spectral division (rfft_rows, irfft_rows, DeconvolveBatch) ---------------
 * The reference has no such component; this is the definition.  n is a power of two in 2^13 .. 2^24, Mc = n / 2; all
 * arithmetic is float64 (a float32 sample widens exactly).
 * 1. Long real transform: X[k] = sum_{t < n} x[t] exp(-2 pi i k t / n), k = 0 .. n/2, as numpy.fft.rfft(x, n); a row of T <= n
 *    samples (float32 or float64, strided rows read in place) is continued with zeros.  The inverse is numpy.fft.irfft(spec, n):
 *    the imaginary parts of bins 0 and n/2 do not count, the scale 1 / n is a power of two, and only the first keep <= n
 *    samples are stored.
 * 2. Deconvolution: a reference x of 1 <= Lx <= n doubles, one for all rows or one per row.  At creation the device forms
 *    P[k] = Re X[k]^2 + Im X[k]^2, Pmax = max_k P[k] per reference, and G[k] = conj(X[k]) / (P[k] + r[k] Pmax) (two real
 *    divisions), 0 where the denominator is 0; r is the scalar reg >= 0 or one value >= 0 per bin (a frequency-dependent,
 *    Kirkeby-style regularisation).  Per measured row y of T <= n samples: H[k] = Y[k] G[k], one complex product in which every
 *    multiplication rounds on its own, and h = irfft(H, n)[0 .. keep).  The division is circular: with n >= T the acausal
 *    part (the harmonic-distortion responses of a sweep) sits at the end of h.  On request H itself is returned.
 * Order of the arithmetic, part of the definition: the complex transform of z[m] = x[2 m] + i x[2 m + 1] has Mc = N1 N2 points,
 *    N1 = 2^floor(log2 Mc / 2) <= N2.  With m = n1 N2 + n2 and k = k1 + N1 k2: N1-point transforms over n1 (X1's transform of
 *    8 points per thread), the product with exp(-2 pi i k1 n2 / Mc), N2-point transforms over n2; then the unpack X[k] = Ze + t,
 *    X[Mc - k] = conj(Ze - t), t = w^k Zo, Ze = (Z[k] + conj Z[Mc - k]) / 2, Zo = -i (Z[k] - conj Z[Mc - k]) / 2, w = exp(-i pi
 *    / Mc), for k <= Mc / 2.  The inverse packs W[k] = conj(((A + B) + i conj(w^k) (A - B)) / n), A = H[k], B = conj H[Mc - k],
 *    runs the same forward transform on W and stores r[2 m] = Re, r[2 m + 1] = -Im.  exp(-2 pi i j / M) between the passes
 *    (M = Mc) and in the unpack (M = n) is the rounded product of the table entries exp(-2 pi i 4096 floor(j / 4096) / M) and
 *    exp(-2 pi i (j mod 4096) / M), both made on the host in long double and rounded once.  No atomics, no fused
 *    multiply-adds.
 * 3. Bits: a row's bits depend on its own samples, n, the reference and r only: not on the other rows of the call, on
 *    scratch_bytes, on a row stride, or on host versus device buffers; a float32 row gives the bits of the same values given
 *    as float64.  A row that holds a non-finite sample gives no finite promise for itself; it never faults and it leaves its
 *    neighbours' bits alone.
 * 4. There is no carried state: a division needs the whole spectrum.  Out of scope: n that is no power of two, n < 2^13
 *    (frt_irfft_rows' range), multi-channel (MIMO) inversion, time-domain windowing of the result, minimum-phase or
 *    inverse-filter design.
 * Scratch: two rows of Mc + 1 complex128 per row in flight (256 MB at n = 2^24); the rows are cut into slabs whose scratch
 * stays within scratch_bytes, at least one row per launch, and the result does not depend on it. */
/* spec[r] = the bins 0 .. n/2 (re, im) of row r: x float32 (x_dtype 0) or float64 (1), sample t of row r is x[r row_stride + t]
 * (stride in elements, >= T).  Host or device buffers in any mix; launched on hip_stream (NULL: the null stream), synchronised.
 * The two stateless entries keep the tables of every n they have served and one grow-only scratch block per process (a block
 * above 512 MB is released when its call ends); their calls are serialised.
 * FRT_ERR_INVALID, before any device call: a null buffer, an unknown x_dtype, n no power of two in 2^13 .. 2^24, T outside
 * 1 .. n, rows outside 1 .. 65535, a bad stride, scratch_bytes < 0. */
int frt_rfft_long_rows(const void* x, int x_dtype, int rows, int64_t T, int64_t row_stride, int64_t n, int64_t scratch_bytes,
                       double* spec, void* hip_stream);
/* out[r out_stride + t], t < keep = the inverse real n-point transform of spec[r] ([rows][n/2 + 1] as re, im).  Buffers,
 * stream and errors as above; keep outside 1 .. n is FRT_ERR_INVALID. */
int frt_irfft_long_rows(const double* spec, int rows, int64_t n, int64_t keep, int64_t scratch_bytes, double* out, int64_t out_stride,
                        void* hip_stream);
typedef struct frt_deconvolve frt_deconvolve;
/* x: [refs][Lx] HOST doubles; reg_bins: NULL (reg holds for every bin) or [n/2 + 1] HOST doubles that replace reg.  G
 * [refs][n/2 + 1] is made once, on the device.  FRT_ERR_INVALID, before any device call: a null handle pointer or null x, n no
 * power of two in 2^13 .. 2^24, Lx outside 1 .. n, refs outside 1 .. 65535, a negative or non-finite reg or reg_bins value, a
 * non-finite reference; FRT_ERR_UNSUPPORTED: G would exceed 1 GiB. */
int frt_deconvolve_create(frt_deconvolve** h, const double* x, int64_t Lx, int refs, int64_t n, double reg, const double* reg_bins);
void frt_deconvolve_destroy(frt_deconvolve* h);
/* Launches go to the null stream unless another one is set here. */
int frt_deconvolve_set_stream(frt_deconvolve* h, void* hip_stream);
/* One call over `rows` measured rows of T samples: y float32 (y_dtype 0) or float64 (1), sample t of row r is y[r row_stride + t].
 * out[r out_stride + t], t < keep: h.  spectrum: NULL, or H [rows][n/2 + 1] (re, im).  Host or device buffers in any mix
 * (host ones are staged); one synchronisation at the end.  FRT_ERR_INVALID, before any device call: a null handle, null y or
 * out, an unknown y_dtype, rows outside 1 .. 65535, a handle of neither 1 nor `rows` references, T or keep outside 1 .. n, a
 * bad stride, scratch_bytes < 0. */
int frt_deconvolve_run(frt_deconvolve* h, const void* y, int y_dtype, int rows, int64_t T, int64_t row_stride, int64_t keep,
                       int64_t scratch_bytes, double* out, int64_t out_stride, double* spectrum);

/* ---- X5: modulation transfer of impulse responses and the Speech Transmission Index (MtfBatch, sti_from_mtf) ---------------
 * The reference has no such component; this is the definition (IEC 60268-16:2011, Schroeder's indirect method).
 * Modulation transfer.  A row x[0 .. T) is float32 or float64, 1 <= T <= 2^24; all arithmetic is float64, e[t] = (double)x[t]^2.
 * A handle holds fs (default 48000, 100 .. 1e7) and nf modulation frequencies F_j in Hz, 1 <= nf <= 16, 0 < F_j < fs / 2.  Per
 * row, over the interval [start, stop) with 0 <= start < stop <= T (default 0, T):
 *    S0 = sum e[t];  S_j = sum e[t] exp(-2 pi i F_j t / fs), t counted from the row's sample 0;  m_j = |S_j| / S0.
 * Outputs per row: m [nf] and energy = S0.  A row that is all zero over the interval, or holds a sample there that is not
 * finite, gives NaN in m (energy is then 0, NaN or inf); it never faults and never affects its neighbours.  A row whose
 * interval is not one (which only device arrays can carry this far) is dead: NaN in m and in energy.
 * Order of the sums, per row and anchored at its sample 0 (so the bits of a row depend on its own samples, start, stop and
 * the frequencies: on no other row, on no slab size, row stride or input dtype, and not on host against device buffers):
 * tiles of frt_mtf_tile() = 4096 samples; lane l of a 64-lane wavefront holds the samples t = 4096 J + 64 q + l, q = 0 .. 63, of
 * tile J, and exp(-2 pi i F_j t / fs) is never evaluated: it is the product coarse_j[J] lane_j[l] step_j[q] of three table
 * entries, each exp(-2 pi i F_j u / fs) at u = 4096 J, l, 64 q, made on the host in long double from the exactly reduced
 * fractional part of F_j u / fs and rounded once.  Samples outside [start, stop) count as e = 0.  Per lane and frequency a =
 * sum_q e[q] step[q] as fused multiply-adds onto 0, real and imaginary part each, the even q and the odd q as two chains (q
 * ascending) whose sums are added at the end; s0 = s0 + e[q], q ascending.  Per tile: a lane[l] as a complex product whose
 * four products round on their own (re: a.re u.re - a.im u.im, im: a.re u.im + a.im u.re), the 64 lanes folded by a butterfly
 * (v += v of lane xor 32, 16, .. 1), the sum times coarse[J] in the same way; s0 folded likewise.  Per row: lane i of a
 * wavefront adds the tile values of tiles J0 + i, J0 + i + 64, .. in order, J0 = floor(start / 4096), the lanes folded by the
 * same butterfly; m_j = sqrt(re^2 + im^2) / S0.  No atomics, no contraction besides the fma above.
 * Index from m [S][7][nf], the octave bands 1000 G^k, k = -3 .. 3, G = 10^0.3 (125 Hz .. 8 kHz), one wavefront per response:
 * 1. Corrections, at most one: snr_db [S][7]: m' = m / (1 + 10^(-snr / 10)).  Or absolute octave-band levels level_db [S][7]
 *    with noise_db [S][7] (or none: In = 0): I_k = 10^(L_k / 10), In_k = 10^(N_k / 10), Irt_k = 10^(A_k / 10) with the reception
 *    thresholds A = 46, 27, 12, 6.5, 7.5, 8, 12 dB; Iam_1 = 0 and for k > 1 Iam_k = (I_{k-1} + In_{k-1}) 10^(amdB(Ltot_{k-1}) / 10),
 *    Ltot = 10 log10(I + In), amdB(L) = 0.5 L - 65 below 63 dB, 1.8 L - 146.9 below 67 dB, 0.5 L - 59.8 below 100 dB, -10 from
 *    there; m' = m I_k / (I_k + In_k + Iam_k + Irt_k).
 * 2. snr_eff = 10 log10(m' / (1 - m')) clipped to [-15, 15] (m' >= 1: 15, m' <= 0: -15); TI = (snr_eff + 15) / 30.
 * 3. MTI_k = the mean of TI over the columns of band k that the mask [7][nf] names, added with j ascending.
 * 4. STI = sum alpha_k MTI_k - sum beta_k sqrt(MTI_k MTI_{k+1}), k ascending, at most 1.  A NaN in a used m makes that
 *    response's STI NaN and no other's.
 * Out of scope: the direct method (STIPA test-signal generation and the analysis of a recording of it; IIR octave band-passes
 * in front of the kernel are X6), the changes of the standard's revision 5, absolute levels from an uncalibrated response, a
 * carried state, sample rates handled in any way other than the fs argument. */
typedef struct frt_mtf frt_mtf;
/* pure host: the tile length of the sums */
int frt_mtf_tile(void);
/* freqs: [nf] HOST doubles.  The tables are made here, on the host.  FRT_ERR_INVALID, before any device call: a null handle
 * pointer or null freqs, fs outside 100 .. 1e7, nf outside 1 .. 16, a frequency outside (0, fs / 2), anything not finite. */
int frt_mtf_create(frt_mtf** h, double fs, const double* freqs, int nf);
void frt_mtf_destroy(frt_mtf* h);
/* Launches go to the null stream unless another one is set here. */
int frt_mtf_set_stream(frt_mtf* h, void* hip_stream);
/* One call over `rows` rows of n samples.  x: float32 (x_dtype 0) or float64 (1), sample t of row r is x[r row_stride + t]
 * (stride in elements, >= n).  start, stop: [rows] or NULL (0, n).  m [rows][nf], energy [rows].  The rows are cut into slabs
 * whose scratch ((1 + 2 nf) doubles per tile) stays within scratch_bytes (at least one row per launch); the result does not
 * depend on it.  Host or device buffers in any mix (host ones are staged); one synchronisation at the end.
 * FRT_ERR_INVALID, before any launch: a null handle, an unknown x_dtype, rows outside 1 .. 65535, n outside 1 .. 2^24, a null
 * x, a bad stride, scratch_bytes < 0, a null output, and in host arrays a start outside 0 .. n - 1, a stop outside 1 .. n or
 * (with both known on the host) a start that is not below its stop. */
int frt_mtf_run(frt_mtf* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, const int64_t* start,
                const int64_t* stop, int64_t scratch_bytes, double* m, double* energy);
/* Steps 1 to 4 over `responses` responses.  correction 0: a and b are NULL; 1: a = snr_db; 2: a = level_db, b = noise_db or
 * NULL.  alpha [7], beta [6] and mask [7][nf] (bytes, non-zero: the column counts) are HOST arrays.  sti [responses], mti
 * [responses][7], ti [responses][7][nf].  m, a, b and the outputs: host or device buffers in any mix; launched on hip_stream
 * (NULL: the null stream), synchronised.  FRT_ERR_INVALID, before any device call: responses outside 1 .. 2^24, nf outside
 * 1 .. 16, an unknown correction, arrays that do not fit it, a null buffer, a band without a column in the mask. */
int frt_sti_run(const double* m, int responses, int nf, int correction, const double* a, const double* b, const double* alpha,
                const double* beta, const unsigned char* mask, double* sti, double* mti, double* ti, void* hip_stream);

/* ---- X6: IIR filters as cascades of second-order sections, and banks of them (SosBatch) ---------------------------------------
 * The reference has no such component; this is the definition.
 * A filter is K sections, 1 <= K <= 8, each [b0 b1 b2 a0 a1 a2]; the host divides by a0 (each quotient rounded once) and refuses
 * a section with a pole |p| >= 1 (|a2| < 1 and |a1| < 1 + a2 must hold) or a coefficient that is not finite.  A handle holds F
 * filters, 1 <= F <= 64, of the same K, and the cell size (below).  One sample x through one section, in float64, every product
 * rounded on its own (no fused multiply-add):
 *    y = b0 x + z0;   z0 = (b1 x - a1 y) + z1;   z1 = b2 x - a2 y
 * and the sections run in order, y of one being x of the next: the operation order of scipy.signal.sosfilt.  float32 input
 * widens exactly.  Output rows are (input row, filter):
 *    bank mode (fan = 1): x [S][T] gives y [S][F][T], every input row through all F filters;
 *    row mode  (fan = 0): x [R][T] gives y [R][T], row r through filter r mod F.
 * reverse = 1 is flip(forward(flip(x))) from the zero state on whole rows: the index reflection t <-> T - 1 - t where x is read
 * and y is written, nothing else; it takes and returns no state.  y is float64, or float32 as the one rounding of the float64 value.
 * Time-parallel order.  A row is cut into cells of `cell` samples (a power of two in 32 .. 1024, chosen at creation) on a grid
 * anchored at the stream's absolute sample index; 64 consecutive cells on that grid are a run.  With s the 2K states (z0, z1 of
 * section 0, then of section 1, ..), M[i][j] = state i after `cell` samples of silence from the unit state j, and M^64 the same
 * after 64 cells, both made on the host in long double by stepping the section code and rounded once:
 *    P_c = the state behind cell c run from the zero state;
 *    Q_r = the cells of run r chained from zero: q <- M q + P_c, c ascending;
 *    U_0 = 0, U_(r+1) = M^64 U_r + Q_r: the true state in front of run r + 1;
 *    S_c = U_r for a run's first cell, otherwise S_(c+1) = M S_c + P_c: the true state in front of cell c;
 *    y over cell c = the sections stepped sample by sample from S_c.
 * A matrix-vector step is new_i = ((P_i + M[i][0] s_0) + M[i][1] s_1) + .., every product rounded on its own.  A stream of at
 * most `cell` samples is therefore the sequential filter, bit for bit.  The bits of an output row depend on its own samples, its
 * filter, the cell size and the absolute sample index: on no other row, slab size, row stride, input dtype, or host against
 * device buffers, and not on how the stream was cut into calls.  The state behind n samples is, per output row, five vectors of
 * 2K doubles (frt_sos_state_length): the running state at n (S_c itself when n lies on the grid), the partial zero-state run of
 * the cell that holds n, S_c of that cell, the partial q of its run, U_r of its run; n itself travels beside it (n_before).
 * A NaN or infinity in a row makes that row's outputs not finite from that sample on and leaves the other rows' bits alone.
 * Out of scope: design families other than Butterworth band-passes (friture_amd/sosfilter.py), padding or steady-state initial
 * conditions for zero-phase use, decimating banks, a live chunk object. */
typedef struct frt_sos frt_sos;
/* pure host: the cell size that cell = 0 stands for; the doubles of a state per output row (0: sections outside 1 .. 8) */
int frt_sos_default_cell(void);
int frt_sos_state_length(int sections);
/* pure host: what a handle of this design would hold.  coef [filters][sections][5] (b0 b1 b2 a1 a2 after the division), M and
 * M64 [filters][2 sections][2 sections]; each may be NULL.  The checks are those of frt_sos_create. */
int frt_sos_tables(const double* sos, int filters, int sections, int cell, double* coef, double* M, double* M64);
/* sos: [filters][sections][6] HOST doubles.  cell: 0 for the default.  FRT_ERR_INVALID, before any device call: a null
 * pointer, filters outside 1 .. 64, sections outside 1 .. 8, a cell that is no power of two in 32 .. 1024, a coefficient that
 * is not finite, a0 = 0, a pole with |p| >= 1. */
int frt_sos_create(frt_sos** h, const double* sos, int filters, int sections, int cell);
void frt_sos_destroy(frt_sos* h);
/* Launches go to the null stream unless another one is set here. */
int frt_sos_set_stream(frt_sos* h, void* hip_stream);
/* One call over `rows` input rows of n samples, 1 <= n <= 2^24.  x: float32 (x_dtype 0) or float64 (1), sample t of row r is
 * x[r row_stride + t] (stride in elements, >= n).  y: dense, [rows][n] (fan 0) or [rows][filters][n] (fan 1), float32 (y_dtype
 * 0) or float64 (1).  n_before: the samples the streams have seen; state_in [output rows][frt_sos_state_length] or NULL (fresh
 * streams, n_before 0); state_out likewise or NULL.  The rows are cut into slabs whose scratch stays within scratch_bytes (at
 * least one row per launch); the result does not depend on it.  Host or device buffers in any mix (host ones are staged); one
 * synchronisation at the end.  FRT_ERR_INVALID, before any launch: a null handle, x or y, an unknown dtype, rows outside
 * 1 .. 65535, n outside 1 .. 2^24, a bad stride, fan or reverse other than 0 or 1, reverse with a state or n_before, n_before
 * without state_in or negative, scratch_bytes < 0. */
int frt_sos_run(frt_sos* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, int fan, int reverse,
                int64_t n_before, const double* state_in, double* state_out, int64_t scratch_bytes, void* y, int y_dtype);

/* ---- X7: the detector of a sound level meter (IEC 61672-1 time weightings, interval logging) (SoundLevelBatch) --------------------
 * The reference has no such component; this is the definition.
 * Input: rows w [R][T] of float32 or float64 samples that are ALREADY frequency weighted (the A and C weightings and band filters
 * are X6 cascades: friture_amd/soundlevel.py); float32 widens exactly.  Settings, fixed at creation: fs; 1 .. 4 time constants
 * tau_i (Fast 0.125 s, Slow 1 s); the logging interval I, a multiple of 16 in 16 .. 2^20 samples; the cell size, a multiple of
 * 16 in 16 .. 1024 that divides I.  All arithmetic is float64, every product rounded on its own (no fused multiply-add).
 * Per sample n of the stream (n counts from the stream's first sample, over all calls):
 *    q[n] = w[n] w[n];   e_i[n] = a_i e_i[n-1] + g_i q[n],  e_i[-1] = 0
 * a_i = exp(-1 / (fs tau_i)) and g_i = -expm1(-1 / (fs tau_i)), both made on the host in long double (-1 / (fs tau_i) too) and
 * rounded once.
 * Time-parallel order.  A row is cut into cells of `cell` samples on a grid anchored at the stream's absolute sample index; 64
 * consecutive cells on that grid are a run.  A_i = a_i^cell, made on the host in long double as the product 1 a a .. a (cell
 * factors of the rounded a_i, left to right) and rounded once; A64_i = the same product of 64 cell factors.  Per time constant:
 *    P_c = e behind cell c stepped sample by sample from e = 0;
 *    Q_r = the cells of run r chained from zero: q <- P_c + A q, c ascending;
 *    U_0 = 0, U_(r+1) = Q_r + A64 U_r: the true value in front of run r + 1;
 *    S_c = U_r for a run's first cell, otherwise S_(c+1) = P_c + A S_c: the true value in front of cell c;
 *    e over cell c = the recurrence stepped sample by sample from S_c (second pass).
 * A stream of at most `cell` samples is therefore the sequential recurrence, bit for bit.
 * Per interval j, the samples [j I, (j + 1) I) of the stream:
 *    energy[j] = the sums of its cells added in ascending order from 0, a cell's sum being its q added in ascending order from 0;
 *    peak[j]   = max |w|;
 *    last_i[j] = e_i at the interval's last sample;  max_i[j], min_i[j] = the extrema of e_i over the interval's samples.
 * Without flush a call emits the intervals that its last sample completes; flush = 1 also emits the partial last interval (its
 * partial last cell's sum is added last) with count[j] < I, and the state is then final.  Stream totals cover the emitted
 * intervals: the energies added in ascending order, the peak, the extrema per time constant.
 * A NaN sample makes e_i NaN from that sample on: last, max and min are NaN from its interval on (maxima and minima keep a NaN
 * explicitly), energy and peak are NaN in its own interval only; earlier intervals and other rows keep their bits.  An infinite
 * sample makes the averages not finite from there on.  An all-zero row gives exact zeros.
 * The bits of a row's results depend on its own samples, the settings and the absolute sample index: on no other row, slab
 * size, row stride, input dtype, or host against device buffers, and not on how the stream was cut into calls.  The state behind
 * n samples is, per row, nine vectors of ntau doubles and five scalars (frt_spl_state_length = 9 ntau + 5): the running e at n
 * (S_c itself when n lies on the cell grid), the partial zero-state run of the cell that holds n, S_c of that cell, the partial q
 * of its run, U_r of its run, the open interval's maximum and minimum, the totals' maximum and minimum; then the open cell's
 * sum of q, the open interval's energy (its complete cells) and peak, the totals' energy and peak.  n itself travels beside it
 * (n_before); the totals' sample count is n_before rounded down to the interval grid, or all of it after a flush.
 * Out of scope: the Impulse time weighting; class conformity claims for a whole instrument; sample rates at which the bilinear
 * transform of the A and C weightings deviates more (the deviation is documented, not corrected: soundlevel.py); fusing the
 * weighting cascade into the detector pass; a live chunk object; percentiles carried in the state. */
typedef struct frt_spl frt_spl;
/* pure host: the cell size that cell = 0 stands for, the largest admissible one up to 400 (0: a bad interval); the doubles of a
 * state per row (0: ntau outside 1 .. 4); the intervals a call of n samples behind n_before emits (-1: a bad argument) */
int frt_spl_default_cell(int interval);
int frt_spl_state_length(int ntau);
int64_t frt_spl_intervals_for(int interval, int64_t n_before, int64_t n, int flush);
/* pure host: a, g, A and A64 [ntau] as a handle of these settings holds them; each may be NULL.  The checks are those of
 * frt_spl_create. */
int frt_spl_tables(double fs, const double* taus, int ntau, int interval, int cell, double* a, double* g, double* A, double* A64);
/* taus: [ntau] HOST doubles, seconds.  cell: 0 for the default.  FRT_ERR_INVALID, before any device call: a null pointer, fs
 * outside 100 .. 1e7, ntau outside 1 .. 4, a time constant that is not finite and positive or whose a rounds to 0 or 1, an
 * interval that is no multiple of 16 in 16 .. 2^20, a cell that is no multiple of 16 in 16 .. 1024 or does not divide it. */
int frt_spl_create(frt_spl** h, double fs, const double* taus, int ntau, int interval, int cell);
void frt_spl_destroy(frt_spl* h);
/* Launches go to the null stream unless another one is set here. */
int frt_spl_set_stream(frt_spl* h, void* hip_stream);
/* One call over `rows` rows of n samples, 1 <= n <= 2^24: sample t of row r is x[r row_stride + t] (stride in elements, >= n),
 * float32 (x_dtype 0) or float64 (1).  n_before: the samples the streams have seen; state_in [rows][frt_spl_state_length] or
 * NULL (fresh streams, n_before 0); state_out likewise or NULL, not overlapping state_in.  J = frt_spl_intervals_for(I, n_before,
 * n, flush) intervals are emitted (also returned in *n_intervals, a HOST pointer or NULL): vals [rows][J][2 + 3 ntau] = energy,
 * peak, last_0 .., max_0 .., min_0 ..; count [J] = the samples of each.  The rows are cut into slabs whose scratch stays within
 * scratch_bytes (at least one row per launch); the result does not depend on it.  Host or device buffers in any mix (host
 * ones are staged); one synchronisation at the end.  FRT_ERR_INVALID, before any launch: a null handle or x, vals or count
 * null with J > 0, an unknown dtype, rows outside 1 .. 65535, n outside 1 .. 2^24, a bad stride, flush other than 0 or 1,
 * n_before without state_in or negative, scratch_bytes < 0. */
int frt_spl_run(frt_spl* h, const void* x, int x_dtype, int rows, int64_t n, int64_t row_stride, int64_t n_before,
                const double* state_in, double* state_out, int flush, int64_t scratch_bytes, double* vals, int64_t* count,
                int64_t* n_intervals);

/* ---- X8: inter-aural cross-correlation and lateral energy from pairs of responses (SpatialBatch) ----------------------------
 * The reference has no such component; this is the definition (the two-channel quantities of ISO 3382-1: Annex B's IACC of a
 * binaural pair, and the sums behind Annex A's lateral energy fractions of an omnidirectional / figure-of-eight pair).
 * A pair is two rows of T samples, 1 <= T <= 2^24, float32 or float64: row 0 is l (the left ear, or the omnidirectional
 * microphone), row 1 is r (the right ear, or the figure-of-eight).  All arithmetic is float64 on samples converted to double.
 * Parameters: fs; M = max_lag, an integer in 0 .. 128 (the standard's +-1 ms is round(fs / 1000)); 1 to 4 windows (a_w, b_w) in
 * samples behind the onset, 0 <= a_w < b_w, b_w = -1 for "to the end"; onset_db = -20.
 * 1. End: e per pair, 1 <= e <= T (default T).  A sample of either row at an index outside [0, e) counts as zero and is never
 *    read into a result, whatever it holds.
 * 2. Dead pair: [0, e) holds a sample that is not finite in either row, or both rows are all zero there (or, in device arrays,
 *    an end outside 1 .. T or an onset outside 0 .. e - 1).  Every float output is NaN, every index output -1; a dead pair never
 *    faults and never changes its neighbours' bits.
 * 3. Peak and onset: P = max over both rows and [0, e) of |x|; peak is the smallest t with max(|l[t]|, |r[t]|) = P; t0 is the
 *    smallest t with max(|l[t]|, |r[t]|) >= c P, c the double nearest 10^(onset_db / 20), made on the host, the product rounded
 *    to double: the test is exact.  Or t0 is given per pair, 0 <= t0 < e (the bands of one response share the broadband onset).
 * 4. Windows: [A_w, B_w) = [min(t0 + a_w, e), min(t0 + b_w, e)), B_w = e for b_w = -1.  An empty window is legal.
 * 5. Sums over t in [A_w, B_w): El_w = sum l[t]^2, Er_w = sum r[t]^2, X_w = sum |l[t] r[t]|, C_w[tau] = sum l[t] r[t + tau] for
 *    tau = -M .. M, where r[t + tau] may lie outside the window but not outside [0, e) (the integration runs over t).
 * 6. IACF_w[tau] = C_w[tau] / sqrt(El_w Er_w); iacc_w = max |IACF_w[tau]|; k_w = the smallest index tau + M in 0 .. 2 M that
 *    attains it; tau_w = (k_w - M) / fs seconds.  When El_w Er_w = 0 (an empty or a silent window) iacc, tau and IACF are NaN and
 *    k_w = -1; the sums are still returned.
 * Order of the sums.  Every sample contributes its 2 M + 1 products once, however the windows overlap: the distinct A_w, B_w of
 * a pair cut [0, e) into disjoint segments (a segment that no window covers is not summed); a segment is summed in tiles of
 * frt_spatial_tile() = 2048 samples counted from the segment's start; a window's sum is the sum of its segments in ascending
 * time, added one by one to 0.  So a window's bits depend on the cut points that other windows put inside it, and with the
 * windows (0, n80), (n80, end), (0, end) the whole-response window is exactly early + late.  Inside a tile, for M > 0: the tile
 * is blocks of 8 samples; lane i of 64 takes the blocks i, i + 64, i + 128, i + 192 in that order and inside a block the samples
 * in order, C[tau] = fma(l[t], r[t + tau], C[tau]), El = fma(l, l, El), Er = fma(r, r, Er), X = X + |l r| with the product
 * rounded first; the lane sums fold pairwise over the lane distances 32, 16, 8, 4, 2, 1 (C), and by the butterfly xor 32 .. 1
 * (El, Er, X); both give every lane the same sum.  For M = 0: thread i of 256 takes the samples i, i + 256, .. in order, with the
 * same four operations, a butterfly folds each wavefront's 64 lanes and the four wavefronts are added in order.  Across the
 * tiles of a segment: strand i of 16 adds the tiles i, i + 16, .. in order to 0, the strands are added in order.  The
 * divisions, the square root, the maximum and its index are made on the device.  No atomics.  A pair's bits do not depend on
 * the other pairs of the call, on scratch_bytes, on any stride, on the input's dtype or on where the buffers live; they do
 * depend on M (the order of El, Er and X differs between M = 0 and M > 0).
 * Out of scope: fractional lags, M > 128, a carried state (the onset anchors everything, so a response is given whole), L_J's
 * 10 m free-field reference (the caller supplies a reference energy), head-related or microphone calibration of any kind. */
typedef struct frt_spatial frt_spatial;
/* pure host: the tile length of the correlation */
int frt_spatial_tile(void);
/* starts, stops: [windows] HOST integers, samples behind the onset; a stop of -1 is "to the end".  FRT_ERR_INVALID, before any
 * device call: a null pointer, fs outside 100 .. 1e7, max_lag outside 0 .. 128, windows outside 1 .. 4, a start below 0, a stop
 * that is neither -1 nor above its start, either above 2^31, onset_db above 0 or not finite. */
int frt_spatial_create(frt_spatial** h, double fs, int max_lag, const int64_t* starts, const int64_t* stops, int windows,
                       double onset_db);
void frt_spatial_destroy(frt_spatial* h);
/* Launches go to the null stream unless another one is set here. */
int frt_spatial_set_stream(frt_spatial* h, void* hip_stream);
/* One call over `pairs` pairs of rows of n samples.  x: float32 (x_dtype 0) or float64 (1); sample t of row c (0: l, 1: r) of
 * pair s is x[s pair_stride + c row_stride + t] (strides in elements, >= n; the pair stride of a single pair is not read).
 * onset: [pairs] or NULL (step 3 finds it); stop: [pairs] ends e or NULL (e = n).  With W windows: params [pairs][W][5] = iacc,
 * tau, X, El, Er; indices [pairs][W + 2] = k_0 .. k_(W-1), peak, onset; iacf [pairs][W][2 max_lag + 1] or NULL.  The pairs are
 * cut into slabs whose scratch stays within scratch_bytes (at least one pair per launch); the result does not depend on it.
 * Host or device buffers in any mix (host ones are staged); one synchronisation at the end.  FRT_ERR_INVALID, before any
 * launch: a null handle, an unknown x_dtype, pairs outside 1 .. 65535, n outside 1 .. 2^24, a null x, a bad stride,
 * scratch_bytes < 0, null params or indices, and in host arrays a stop outside 1 .. n, an onset outside 0 .. n - 1 or an onset
 * at or behind its pair's stop. */
int frt_spatial_run(frt_spatial* h, const void* x, int x_dtype, int pairs, int64_t n, int64_t row_stride, int64_t pair_stride,
                    const int64_t* onset, const int64_t* stop, int64_t scratch_bytes, double* params, int64_t* indices,
                    double* iacf);

/* ---- X9: total harmonic distortion, noise and harmonic levels of tone recordings (ToneBatch) ----------------------------
 * The reference has no such component; this is the definition.  A stream is one row of samples of a system driven by a sine;
 * float64 arithmetic whatever the input dtype (a float32 sample widens exactly).
 * Settings: fft_size N, a power of two in 512 .. 16384; hop, 1 .. 2^30, which may exceed N; a window w of N doubles; the
 * half-width of a spectral line L = lobe, 1 .. 16 bins; the highest order H = harmonics, 2 .. 32; the band ka .. kb in bins,
 * L + 1 <= ka <= kb <= N/2; one search range klo .. khi for all streams or one per stream, ka + L <= klo <= khi <= kb - L; a
 * gate g >= 0, a power.  (ToneBatch derives them from Hz and dB on the host: ka = max(L + 1, ceil(f_lo N / fs)), kb =
 * min(N/2, floor(f_hi N / fs)), klo = ka + L and khi = kb - L intersected with rint(f0 N / fs) +- L when f0 is given, g the
 * double nearest 10^(gate_db / 10); an empty range is an error there.)
 * Frames: frame f of a stream is its samples [f hop, f hop + N); only complete frames count: F(n) = 0 for n < N, else
 * floor((n - N) / hop) + 1.
 * Spectrum: X = rfft(x w); Q[k] = c_k |X[k]|^2 / (N sum_n w[n]^2), c_k = 2 except c_0 = c_(N/2) = 1: a unit sine's line sums
 * to 0.5.  (The device multiplies |X[k]|^2 by the double nearest c_k / (N sum w^2), the sum made in index order on the host.)
 * Fundamental: c1 = the arg-max of Q over klo .. khi, the lowest index on ties; P1 = sum of Q[c1 - L .. c1 + L], ascending k
 * from 0; kappa = (sum k Q[k]) / P1 over the same bins, each product rounded and added in the same order.
 * Harmonics h = 2 .. H: c_h = rint((double)h * kappa), half to even, and c_1 = c1.  Order h is present when c_h + L <= kb; its
 * lobe is [max(c_h - L, c_(h-1) + L + 1), c_h + L], so a bin counts once, for the lowest order that holds it; P_h is the sum
 * over the lobe, ascending k from 0.  An absent order has no lobe: it is NaN in the output and adds 0 to the totals.
 * Residual: R = the sum of Q[k] over ka <= k <= kb outside every lobe of the orders 1 .. H.  No power is obtained by
 * subtraction.  Its order: thread i of N/16 sums the bins i, i + N/16, .. , i + 7 N/16 in that order from 0 (thread 0 then
 * adds bin N/2), a bin outside the band or inside a lobe counting as +0; the thread sums of each 64 consecutive threads (32
 * for N = 512) fold as a balanced binary tree over neighbours ((t0 + t1) + (t2 + t3) ..); the groups of 64 are added in order.
 * Dead frame: it holds a sample that is not finite, or Q is all zero over klo .. khi.  kappa, P1, R and every P_h are NaN,
 * peak_bin = -1, not valid.  Gated frame: a live frame with P1 < g; it keeps its values and is not valid.
 * A frame of finite samples whose Q overflows (samples near 1e154 and above) is live: its values are inf or NaN as the sums give
 * them, it is valid unless gated, and the totals of its stream become inf or NaN with it; no order of such a frame is present.
 * Totals per stream: n_valid and the left folds from 0, in frame order over the valid frames, of kappa, P1, R and each P_h.
 * They do not depend on how a recording is cut into calls, slabs or batches.  No atomics.
 * The state after n samples is one array of doubles, S the number of streams,
 *   totals [S][3 + H] (sum kappa, sum P1, sum R, sum P_2 .. sum P_H, n_valid) | the row from min(n, F(n) hop) on [S][..]
 * (at most N - 1 samples per row), and the results of a call that completes F frames are another,
 *   kappa [S][F] | P1 [S][F] | R [S][F] | P_h [S][F][H - 1] | code [S][F], code = -1 for a dead frame, else 2 c1 + valid.
 * Out of scope: frames above 16384, weighting curves on Q, spurs, two-tone intermodulation, harmonic phases, notch-filter
 * time-domain THD+N, multi-tone signals. */
typedef struct frt_tone frt_tone;
/* window: [fft_size] HOST doubles; klo, khi: [n_search] HOST integers, n_search = 1 or the number of streams of every run.
 * FRT_ERR_INVALID, before any device call: fft_size outside 512 .. 16384 or no power of two, hop outside 1 .. 2^30, lobe
 * outside 1 .. 16, harmonics outside 2 .. 32, a band outside lobe + 1 .. fft_size / 2 or empty, n_search outside 1 .. 65535, a
 * search range that is empty or outside ka + lobe .. kb - lobe, a gate that is negative or not finite, a null, non-finite or
 * all-zero window. */
int frt_tone_create(frt_tone** h, int fft_size, int64_t hop, const double* window, int lobe, int harmonics, int ka, int kb,
                    const int* klo, const int* khi, int n_search, double gate);
void frt_tone_destroy(frt_tone* h);
/* Launches go to the null stream unless another one is set here. */
int frt_tone_set_stream(frt_tone* h, void* hip_stream);
/* One call over `streams` rows.  x: float32 (x_dtype 0) or float64 (1); sample t of stream s is x[s row_stride + t] (stride in
 * elements, >= n; a single stream's is not read), the samples first_in .. first_in + n - 1 of the streams (n = 0: x may be
 * NULL).  state_in: the state after first_in samples (NULL: new streams, first_in = 0 only); state_out: the state after the
 * call, a buffer distinct from state_in; out: the results (may be NULL when no frame completes); n_frames_out (may be NULL): F.
 * The frame records of one launch, 3 + H doubles per frame and stream, stay within scratch_bytes (at least one frame per
 * launch): the frames are cut into time slabs, and the result does not depend on it.  Host or device buffers in any mix (host
 * ones are staged); one synchronisation at the end.  FRT_ERR_INVALID, before any device call: a null handle, an unknown
 * x_dtype, streams outside 1 .. 65535 or not the handle's n_search when that is above 1, n < 0, a bad stride, first_in < 0 or
 * first_in + n > 2^40, first_in > 0 without state_in, a null state_out or one equal to state_in, scratch_bytes < 0, a null out
 * when frames complete. */
int frt_tone_run(frt_tone* h, const void* x, int x_dtype, int streams, int64_t n, int64_t row_stride, const double* state_in,
                 double* state_out, int64_t first_in, int64_t scratch_bytes, double* out, int64_t* n_frames_out);

#ifdef __cplusplus
}
#endif
#endif /* FRITURE_HIP_H */
