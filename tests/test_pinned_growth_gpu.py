"""Growth and reuse of the page-locked staging blocks (PinnedBuffer / PinnedSlot, csrc/common.h): on one handle a small
host-array call, a larger one that makes the block reallocate, then the small one again.

Stateless entry points must give, bit for bit, what the same call gives on a fresh handle.  Stateful ones are held to the
oracle with the tolerance of their family's own test.  Sizes are the smallest that cross each route's thresholds.

Blocks whose regrowth other tests already see, and which are therefore not repeated here:
  frt_specgram_push (chunk and pixel blocks)   test_widgets_gpu.py::test_spectrogram_stream_equals_host_chain (512 .. 3000 .. 512 .. 1)
  frt_delay_push (the four slots, delay.hip)   test_gcc_gpu.py::test_delay_object_rings_equal_host_rings (512 .. 4096 .. 511, 12 rounds)
  frt_levels_push                              test_levels_gpu.py, the "irregular" case (512 .. 8192 .. 20000, 255: above the 64 KB floor)
  frt_pitch_live_push                          test_pitchstream_gpu.py::test_ragged_chunks_and_a_stall (1-2 frames, 19 at once, 1-2)
"""
import ctypes

import numpy as np
import pytest

from conftest import synth
from oracle import dsp

pytestmark = pytest.mark.gpu

_DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def tabs(hip):
    return dsp.load_filter_tables()


def small_large_small(call, make, sizes):
    """call(handle, size) on ONE handle for every size in turn, each against the same call on a handle of its own."""
    shared = make()
    for step, size in enumerate(sizes):
        got, want = call(shared, size), call(make(), size)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), (step, size)


# fft_size 32, hop 16, one float32 channel: T = 64 is served in place from the pinned block (in + out under 256 KB), T = 2^17 by
# copies through it (512 KB in + 544 KB out, under the 4 MB above which the caller's own memory is used)
STFT_SIZES = (64, 1 << 17, 64)


def test_stft_host_to_host():
    from friture_amd.stft import StftEngine
    x = synth("noise", max(STFT_SIZES), 3)
    small_large_small(lambda eng, T: (eng.psd(x[:T]),), lambda: StftEngine(32, 16, 1, 32), STFT_SIZES)


def test_stft_host_to_device(hip):
    """Host samples, spectra left on the device: the call returns before its copy has read the pinned block, so the next
    call waits on the slot's event — the large call's block is reallocated while nothing is pending, the last small call
    overwrites a block the large copy has just been reading."""
    import torch

    from friture_amd import _lib
    from friture_amd.stft import StftEngine
    x = synth("noise", max(STFT_SIZES), 4)

    def run(eng, T):
        out = torch.empty((1, eng.frames_for(T), eng.n_bins), dtype=torch.float32, device="cuda")
        nf = ctypes.c_int64(0)
        _lib.check(hip.frt_stft_run(eng._h, _lib.FRT_STFT_PSD, x.ctypes.data, T, T, ctypes.c_void_p(out.data_ptr()), ctypes.byref(nf)))
        return out

    shared = StftEngine(32, 16, 1, 32)
    got = [run(shared, T) for T in STFT_SIZES]                    # back to back: nothing waits between the calls
    torch.cuda.synchronize()
    for step, T in enumerate(STFT_SIZES):
        want = run(StftEngine(32, 16, 1, 32), T)
        torch.cuda.synchronize()
        assert torch.equal(got[step], want), (step, T)
        assert np.array_equal(got[step].cpu().numpy(), StftEngine(32, 16, 1, 32).psd(x[:T])), (step, T)


def test_iir_bank_filter_from_host_arrays(tabs):
    """IirBank.filter on host arrays (filter_host: blocks of exactly the call's size), from zero state every time."""
    from friture_amd.filter import IirBank
    boct, aoct = list(tabs["boct_3"]), list(tabs["aoct_3"])
    x = synth("noise", 1 << 16, 5).astype(np.float64)

    def call(bank, n):
        bank.reset()
        return bank.filter(x[:n])[0][0]

    small_large_small(call, lambda: IirBank(tabs["bdec"], tabs["adec"], boct, aoct, 1), (1024, 1 << 16, 1024))


def test_iir_bank_graph_goes_when_only_the_pinned_blocks_move(tabs):
    """The captured graph of filter_host (csrc/iir.hip) carries the addresses of both pinned blocks besides the device buffers'.
    The device buffers grow geometrically, the pinned blocks to exactly the call's need, so a call can move the pinned blocks
    alone; the graph of an earlier length must then be dropped, not replayed on the freed blocks.  One channel, 3 bands per
    octave (packed length: 3 x the sum of the nine stage lengths), float64, sequential mode:

      step 0  energies of [1, 2048] device samples: xbuf[1..8] hold 1024 .. 8 samples, more than the 550 .. 5 of a
              1100-sample call (from 1024 samples alone xbuf[5] holds 32 and would move for 35, dropping the graph by the
              device-buffer rule); xin, ypacked and the pinned blocks are not touched by a device-array call
      1000    eager    xin 8000 B, ypacked 3 x 1998 = 5994 doubles, pin_in 8000 B, pin_out 47952 B
      1024    eager    xin 8192 > 8000: grows to 1.5 x 8000 = 12000 B; ypacked 3 x 2044 = 6132 > 5994: grows to 1.5 x 5994 =
                       8991 doubles; pin_in 8192 B, pin_out 49056 B (exactly the need)
      1024    captured, launched
      1024    replayed
      1100    eager    xin 8800 <= 12000 B and ypacked 3 x 2199 = 6597 <= 8991 doubles stay; pin_in 8800 > 8192 B and
                       pin_out 52776 > 49056 B are reallocated
      1024    the graph of step 3 names the old pinned blocks: dropped, the call runs eagerly

    Every call from zero state, against the same call on a handle of its own, bit for bit."""
    import torch

    from friture_amd.filter import IirBank
    boct, aoct = list(tabs["boct_3"]), list(tabs["aoct_3"])
    x = synth("noise", 1100, 10).astype(np.float64)

    def make():
        return IirBank(tabs["bdec"], tabs["adec"], boct, aoct, 1)

    bank = make()
    alphas, _ = dsp.band_smoothing_setup(3, 0.125)
    bank.energies(torch.from_numpy(synth("noise", 2048, 11)[None, :]).cuda(), 1024, alphas)
    torch.cuda.synchronize()
    for step, n in enumerate((1000, 1024, 1024, 1024, 1100, 1024)):
        bank.reset()
        got, want = bank.filter(x[:n])[0][0], make().filter(x[:n])[0][0]
        assert len(got) == len(want) == 27
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), (step, n)


def test_decimate_multiple_state(hip, tabs):
    """frt_decimate_multiple_state: samples and states in one block, the decimated signal in the other.  The in-place call takes
    at most 256 KB, so the large call is 2^14 samples (128 KB against the 16 KB block the 1024-sample call left)."""
    from friture_amd import _lib
    bdec, adec = np.ascontiguousarray(tabs["bdec"], np.float64), np.ascontiguousarray(tabs["adec"], np.float64)
    x = synth("noise", 1 << 14, 6).astype(np.float64)
    zi = 1e-3 * np.random.default_rng(6).standard_normal((2, 12))
    made = []

    def make():
        h = ctypes.c_void_p()
        _lib.check(hip.frt_octbank_create(ctypes.byref(h), 0, 1, 0, None, None, bdec.ctypes.data_as(_DP), adec.ctypes.data_as(_DP), None, None))
        made.append(h)
        return h

    def call(h, n):
        out, zf, n_out = np.empty(n // 4), np.empty((2, 12)), ctypes.c_int(0)
        _lib.check(hip.frt_decimate_multiple_state(h, 2, x.ctypes.data, n, zi.ctypes.data, out.ctypes.data, ctypes.byref(n_out), zf.ctypes.data))
        assert n_out.value == n // 4
        return out, zf

    try:
        small_large_small(call, make, (1024, 1 << 14, 1024))
        ref, zr = dsp.decimate_multiple(2, bdec, adec, x[:1024], [zi[0], zi[1]])
        got, zf = call(made[0], 1024)
        assert np.array_equal(got, ref) and np.array_equal(zf, np.stack(zr))
    finally:
        for h in made:
            hip.frt_octbank_destroy(h)


def test_stage_call_arena():
    """frt_exp_smooth_2d, an entry point on the process-wide StageCall arena (no handle to make afresh): the small call before
    and after a 2.6 MB one, which reallocates the arena's pinned block unless an earlier call of the process has already
    made it that large.  The large call is held to the oracle at the 1e-13 of test_pipeline_gpu.py."""
    from friture_amd.signal.exp_smoothing import exp_smoothed_value_2d
    rng = np.random.default_rng(7)
    kern, big_kern = dsp.smoothing_kernel(0.02, 64), dsp.smoothing_kernel(0.001, 8192)
    d, prev = rng.random((4, 64)), rng.random(4)
    big, big_prev = rng.random((40, 8192)), rng.random(40)
    before = exp_smoothed_value_2d(kern, 0.02, d, prev)
    large = exp_smoothed_value_2d(big_kern, 0.001, big, big_prev)
    after = exp_smoothed_value_2d(kern, 0.02, d, prev)
    assert np.array_equal(before, after)
    assert np.max(np.abs(before / dsp.exp_smoothed_value_2d(kern, 0.02, d, prev) - 1)) < 1e-13
    assert np.max(np.abs(large / dsp.exp_smoothed_value_2d(big_kern, 0.001, big, big_prev) - 1)) < 1e-13


def test_bank_energies_carry_their_state_across_a_regrowth(tabs):
    """frt_octbank_energies on host arrays, one channel, 3 bands per octave, 1024 / 2^16 / 1024 samples in blocks of 1024:
    filter states and smoothed energies carried from call to call while both pinned blocks are reallocated in between.
    Against the oracle fed block by block, at the 1e-5 of test_iir_gpu.py::test_band_energies."""
    from friture_amd.filter import IirBank
    bpo = 3
    boct, aoct = list(tabs[f"boct_{bpo}"]), list(tabs[f"aoct_{bpo}"])
    sizes = (1024, 1 << 16, 1024)
    x32 = synth("noise", sum(sizes), 8)
    alphas, kernels = dsp.band_smoothing_setup(bpo, 0.125)
    bank = IirBank(tabs["bdec"], tabs["adec"], boct, aoct, 1)
    got, pos = [], 0
    for n in sizes:
        got.append(bank.energies(x32[None, pos:pos + n], 1024, alphas)[0])
        pos += n
    got = np.concatenate(got)
    assert got.shape == (sum(sizes) // 1024, 9 * bpo)
    zs, prev = dsp.iir_bank_filtic(tabs["bdec"], tabs["adec"], boct, aoct), [0.0] * (9 * bpo)
    for blk in range(got.shape[0]):
        y, _, zs = dsp.iir_bank(tabs["bdec"], tabs["adec"], boct, aoct, x32[blk * 1024:(blk + 1) * 1024].astype(np.float64), zs)
        prev = dsp.band_energies(y, kernels, alphas, prev)
        assert np.max(np.abs(got[blk] / np.array(prev) - 1)) <= 1e-5, blk


def test_octave_spectrum_stream_chunks_that_regrow(hip):
    """The FFT bank's chunk handler (frt_octbank_energies in mode 1, the kernels read and write the pinned blocks in place) takes
    at most 1024 samples a call: 256 / 1024 / 256 is the regrowth it can see.  Against OctaveSpectrum at the 4.4e-5 dB of
    test_widgets_gpu.py::test_octave_spectrum_stream_equals_host_chain."""
    from friture_amd.octavespectrum import OctaveSpectrum, OctaveSpectrumStream
    a, b = OctaveSpectrum(3, weighting=1, response_time=0.125), OctaveSpectrumStream(3, weighting=1, response_time=0.125)
    x = synth("noise", 256 + 1024 + 256, 9).astype(np.float64)
    pos = 0
    for n in (256, 1024, 256):
        ra, rb = a.handle_new_data(x[None, pos:pos + n]), b.handle_new_data(x[None, pos:pos + n])
        pos += n
        assert np.max(np.abs(ra[3] - rb[3])) <= 4.4e-5, n
