"""Record tests/golden/spectrogrambatch/<case>.npz from the reference's own spectrogram classes.

Driven by oracle/make_golden.py (needs the reference checkout).  The reference's own classes do the work: audioproc, RingBuffer
(behind refshim.AudioBuffer), Frequency_Resampler, Online_Linear_2D_resampler, Color_Transform and Transform_Pipeline, set up as
Spectrogram_Widget.__init__ sets them up and driven by the statements of Spectrogram_Widget.handle_new_data
(friture/spectrogram.py:131-173) with the widget's Qt parts (the image item, the settings dialog) left out.  The column table is
read off the reference, not restated: the time resampler calls linear_interp_2D once per frame that emits columns, and a
wrapper around that function notes the frame (orig_index counts them) and obtains the weights from the function itself (old = 1,
new = 0 gives `a`); columns of a push's block beyond what those calls wrote are the fillers.

Per case of oracle.spectrogrambatch.GOLDEN_CASES one file holds x (float32 PCM), ends, norm [F, B], frame_start, refresh_chunk,
pixels [H, P] (flipped as the image item flips them), src, a, filler, column_refresh, targets, weight and lut.  One file per case,
in a folder of their own, keeps each below 1 MiB.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import refshim
from . import spectrogrambatch as H


def record_case(case):
    from numpy import floor, float64, log10, tile, zeros

    import friture.plotting.frequency_scales as fscales
    import friture.signal.online_linear_2D_resampler as time_module
    from friture.audiobackend import SAMPLING_RATE
    from friture.audioproc import audioproc
    from friture.signal.color_tranform import Color_Transform
    from friture.signal.frequency_resampler import Frequency_Resampler
    from friture.signal.online_linear_2D_resampler import Online_Linear_2D_resampler
    from friture.signal.transform_pipeline import Transform_Pipeline

    scale = {"linear": fscales.Linear, "log": fscales.Logarithmic, "mel": fscales.Mel, "erb": fscales.Erb, "octave": fscales.Octave}[case["scale"]]
    fft_size, height, width = case["fft_size"], case["screen_height"], case["screen_width"]
    overlap_frac = Fraction(case["overlap"])
    overlap = float(overlap_frac)
    spec_min, spec_max = case["spec_min"], case["spec_max"]

    # ---- Spectrogram_Widget.__init__ and its setters, without Qt -------------------------------------------------------------
    audiobuffer = refshim.AudioBuffer()
    proc = audioproc()
    frequency_resampler = Frequency_Resampler()
    screen_resampler = Online_Linear_2D_resampler()
    audio_pipeline = Transform_Pipeline([frequency_resampler, screen_resampler, Color_Transform()])
    proc.set_fftsize(fft_size)
    A, B, C = proc.get_freq_weighting()
    w = {0: np.array([0.]), 1: A, 2: B}.get(case["weighting"], C)
    w = w.reshape(len(w), 1)
    freq = proc.get_freq_scale()
    frequency_resampler.setfreq(freq)
    frequency_resampler.setfreqscale(scale)
    frequency_resampler.setfreqrange(case["minfreq"], case["maxfreq"])
    sfft_rate_frac = Fraction(SAMPLING_RATE, fft_size) / (Fraction(1) - overlap_frac) / 1000
    old_index = audiobuffer.ringbuffer.offset

    # ---- the column table, from the reference's own calls --------------------------------------------------------------------
    calls = []
    inner = time_module.linear_interp_2D

    def noting(resampled_buffer, data, old_data, orig_index, resampled_index, resampling_ratio, n):
        weights = np.zeros((1, n))
        inner(weights, np.zeros(1), np.ones(1), orig_index, resampled_index, resampling_ratio, n)
        calls.append((int(orig_index) - 1, weights[0].copy()))
        return inner(resampled_buffer, data, old_data, orig_index, resampled_index, resampling_ratio, n)

    time_module.linear_interp_2D = noting
    x = H.synth(case["kind"], case["n"], case["seed"])
    ends = H.case_ends(case)
    norms, pixels, frame_start, refresh_chunk = [], [], [0], []
    src, a, filler, column_refresh = [], [], [], []
    try:
        pos = 0
        for c, e in enumerate(ends):
            audiobuffer.push(x[None, pos:e].astype(float64))
            pos = int(e)
            # ---- handle_new_data ------------------------------------------------------------------------------------------
            index = audiobuffer.ringbuffer.offset
            available = index - old_index
            if available < 0:
                available = 0
                old_index = index
            needed = fft_size * (1. - overlap)
            realizable = int(floor(available / needed))
            if realizable > 0:
                spn = zeros((len(freq), realizable), dtype=float64)
                for i in range(realizable):
                    floatdata = audiobuffer.data_indexed(old_index, fft_size)
                    floatdata = floatdata[0, :]
                    spn[:, i] = proc.analyzelive(floatdata)
                    old_index += int(needed)
                wt = tile(w, (1, realizable))
                norm_spectrogram = ((10. * log10(spn + 1e-30) + wt) - spec_min) / (spec_max - spec_min)
                screen_resampler.set_height(height)
                screen_rate_frac = Fraction(max(width, 1), int(case["timerange_s"] * 1000))
                screen_resampler.set_ratio(sfft_rate_frac, screen_rate_frac)
                frequency_resampler.setnsamples(height)
                calls.clear()
                data = audio_pipeline.push(norm_spectrogram)
                # ---- what the test keeps ------------------------------------------------------------------------------------
                r = len(refresh_chunk)
                written = sum(len(wts) for _, wts in calls)
                assert written <= data.shape[1]
                for f, wts in calls:
                    src += [f] * len(wts)
                    a += wts.tolist()
                spare = data.shape[1] - written
                src += [frame_start[-1] + realizable - 1] * spare
                a += [0.] * spare
                filler += [False] * written + [True] * spare
                column_refresh += [r] * data.shape[1]
                norms.append(norm_spectrogram.T.copy())
                pixels.append(data[::-1].copy())                     # spectrogram_image.py:82-92 flips the frequency axis
                frame_start.append(frame_start[-1] + realizable)
                refresh_chunk.append(c)
    finally:
        time_module.linear_interp_2D = inner
    lut = audio_pipeline.blocks[2].colors.copy()
    return dict(x=x, ends=ends, norm=np.concatenate(norms), frame_start=np.array(frame_start, np.int64),
                refresh_chunk=np.array(refresh_chunk, np.int64), pixels=np.concatenate(pixels, axis=1).astype(np.uint32),
                src=np.array(src, np.int64), a=np.array(a, np.float64), filler=np.array(filler, bool),
                column_refresh=np.array(column_refresh, np.int64), targets=np.array(frequency_resampler.xscaled, np.float64),
                weight=np.broadcast_to(w[:, 0], freq.shape).astype(np.float64)), lut


def spectrogrambatch(out_dir):
    refshim.install()
    folder = out_dir / H.GOLDEN_FOLDER
    folder.mkdir(exist_ok=True)
    for name, case in H.GOLDEN_CASES.items():
        got, lut = record_case(case)
        got["lut"] = np.asarray(lut, np.uint32)
        print(f"{name}: {got['norm'].shape[0]} frames, {got['pixels'].shape[1]} columns, {int(got['filler'].sum())} fillers")
        np.savez_compressed(folder / f"{name}.npz", **got)
