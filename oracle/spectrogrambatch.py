"""Shared by the SpectrogramBatch tests and their recorder (oracle/golden_spectrogrambatch.py): the case list and the
spectrogram widget's body replayed chunk by chunk over oracle.dsp and plain numpy, in the reference's operation order
(friture/spectrogram.py:131-173, signal/frequency_resampler.py:67-83, signal/online_linear_2D_resampler.py:57-97,
signal/linear_interp.py:51-60, signal/color_tranform.py:48-51, signal/lookup_table.py:50-52).  Nothing here touches the GPU or the
package under test."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import dsp
from .cases import FS, chunk_ends, synth  # noqa: F401 (synth: the cases' input, for the tests and the recorder)

GOLDEN_FOLDER = "spectrogrambatch"      # under tests/golden/: one file per case

# The recorded cases (tests/golden/spectrogrambatch/<case>.npz).  `overlap` is a Fraction as in the widget (overlap_frac); the float the
# widget divides with is float(overlap).
GOLDEN_CASES = {
    # one second of the seeded chirp in chunks of 512: the pixel rate far below the STFT rate (18.75 frames per column)
    "chirp_1024": dict(fft_size=1024, overlap=Fraction(3, 4), spec_min=-140., spec_max=0., weighting=0, scale="mel", minfreq=20.,
                       maxfreq=20000., screen_width=100, screen_height=48, timerange_s=10., kind="chirp", n=48000, seed=11, chunk=512),
    # `needed` = 1000 * (1 - 2/3) is not a whole number (333.33...; hop 333), A weighting, log scale, 1.8 frames per column in
    # floats that are not exact: the reference allocates one column more than it writes in one refresh (a filler)
    "thirds_1000": dict(fft_size=1000, overlap=Fraction(2, 3), spec_min=-120., spec_max=-10., weighting=1, scale="log", minfreq=50.,
                        maxfreq=16000., screen_width=800, screen_height=33, timerange_s=10., kind="noise", n=12000, seed=12, chunk=512),
    # several columns per frame (0.5625 frames per column), C weighting, ERB scale, ragged chunks
    "up_512": dict(fft_size=512, overlap=Fraction(1, 2), spec_min=-100., spec_max=-20., weighting=3, scale="erb", minfreq=20.,
                   maxfreq=22000., screen_width=1000, screen_height=20, timerange_s=3., kind="tone", n=16000, seed=13, chunk=None),
}
# the reference raises in its fifth refresh with these settings: the time resampler writes more columns than it allocated
OVER_EMISSION = dict(fft_size=1000, overlap=Fraction(2, 3), screen_width=640, screen_height=8, timerange_s=2., n=40000, chunk=512, refresh=5)


def load_golden(folder):
    """{case: {array name: array}} of the recorded files in `folder` (tests/golden/spectrogrambatch)."""
    out = {}
    for name in GOLDEN_CASES:
        with np.load(folder / f"{name}.npz", allow_pickle=False) as z:
            out[name] = {k: z[k] for k in z.files}
    return out


def case_ends(case):
    if case["chunk"] is not None:
        return chunk_ends(case["n"], case["chunk"])
    rng = np.random.default_rng(case["seed"])
    ends = np.cumsum(rng.choice([1, 100, 512, 512, 640, 3000], size=400))
    return np.concatenate([ends[ends < case["n"]], [case["n"]]]).astype(np.int64)


def settings(fft_size=4096, overlap=Fraction(3, 4), spec_min=-140., spec_max=0., weighting=0, scale="mel", minfreq=20., maxfreq=20000.,
             screen_width=800, screen_height=400, timerange_s=10., **_):
    """What the widget derives from its settings (spectrogram.py:93-101,143,165-167; audioproc.py:86-96)."""
    needed = fft_size * (1. - float(overlap))
    freq = dsp.frequency_axis(fft_size)
    curves = dsp.weighting_curves(freq)
    weight = np.zeros(freq.shape) if weighting == 0 else curves[min(weighting, 3) - 1]
    sfft_rate = Fraction(FS, fft_size) / (Fraction(1) - Fraction(overlap)) / 1000
    screen_rate = Fraction(max(screen_width, 1), int(timerange_s * 1000))
    return dict(fft_size=fft_size, needed=needed, hop=int(needed), freq=freq, weight=weight, spec_min=spec_min, spec_max=spec_max,
                targets=dsp.frequency_targets(scale, minfreq, maxfreq, screen_height), height=screen_height,
                ratio=float(sfft_rate) / float(screen_rate), lut=dsp.colour_lut(dsp.cmrmap()))


class Resampler:
    """Online_Linear_2D_resampler.push with its bookkeeping made visible: besides the block it returns, per allocated column, the
    pushed column that fed it, its weight and whether it was left unwritten.  Raises ValueError where the reference's block
    assignment does (more columns emitted than allocated)."""

    def __init__(self, ratio, height, old=None, orig_index=0., resampled_index=0.):
        self.ratio, self.height = ratio, height
        self.orig_index, self.resampled_index = orig_index, resampled_index
        self.old = np.zeros(height) if old is None else np.array(old, np.float64)

    def processable(self, m):
        return int(np.ceil((self.orig_index + m - (self.resampled_index + self.ratio)) / self.ratio))

    def push(self, data):
        cols = data.shape[1]
        total = self.processable(cols)
        out = np.zeros((self.height, total))
        src, a_all, w = [], [], 0
        for j in range(cols):
            self.orig_index += 1.
            n = self.processable(0)
            if n > 0:
                idx = self.resampled_index + self.ratio * np.arange(1, n + 1, dtype=np.float64)
                a = self.orig_index - idx
                block = data[:, j][:, None] * (1.0 - a)[None, :] + self.old[:, None] * a[None, :]
                if w + n > total:
                    raise ValueError(f"could not broadcast: {w + n} columns into {total}")
                out[:, w:w + n] = block
                self.resampled_index = float(idx[-1])
                src += [j] * n
                a_all += a.tolist()
                w += n
            self.old = data[:, j]
        filler = [False] * w + [True] * (total - w)
        src += [cols - 1] * (total - w)
        a_all += [0.] * (total - w)
        return out, np.array(src, np.int64), np.array(a_all), np.array(filler, bool)


def colour(values, lut):
    """Color_Transform.push: (pixels, v * 255 before the truncation)."""
    v255 = np.clip(values, 0., 1.) * 255
    return lut[v255.astype(np.intp)], v255


def screen_replay(norm, frame_start, st, old=None, orig_index=0., resampled_index=0.):
    """The three pipeline blocks on given normalised frames norm [F, B] of one stream, pushed refresh by refresh.  Returns
    dict(pixels [H, P] uint32 flipped, v255 [H, P] flipped, src (global frame), a, filler, column_refresh [P], old_column [H],
    orig_index, resampled_index)."""
    rs = Resampler(st["ratio"], st["height"], old, orig_index, resampled_index)
    pix, v255, src, a, filler, cref = [], [], [], [], [], []
    for r in range(len(frame_start) - 1):
        f0, f1 = int(frame_start[r]), int(frame_start[r + 1])
        try:
            block, s, w, fl = rs.push(dsp.frequency_resample(st["targets"], st["freq"], np.asarray(norm[f0:f1], np.float64).T))
        except ValueError as e:
            raise ValueError(f"refresh {r}: {e}") from None
        p, v = colour(block, st["lut"])
        pix.append(p[::-1])
        v255.append(v[::-1])
        src.append(s + f0)
        a.append(w)
        filler.append(fl)
        cref.append(np.full(len(s), r, np.int64))
    H = st["height"]
    cat = lambda parts, shape, dt: np.concatenate(parts, axis=-1) if parts else np.zeros(shape, dt)
    return dict(pixels=cat(pix, (H, 0), np.uint32), v255=cat(v255, (H, 0), np.float64), src=cat(src, (0,), np.int64),
                a=cat(a, (0,), np.float64), filler=cat(filler, (0,), bool), column_refresh=cat(cref, (0,), np.int64),
                old_column=np.array(rs.old, np.float64), orig_index=rs.orig_index, resampled_index=rs.resampled_index)


def frames_replay(x, ends, st):
    """The widget's frame loop (dsp.widget_frames): one stream x [T] float64 -> psd_frame -> dB + weighting -> normalisation, chunk
    by chunk.  Returns (norm [F, B], frame_start [R + 1], refresh_chunk [R])."""
    window = dsp.hann_symmetric(st["fft_size"])
    norm, frame_start, refresh_chunk = [], [0], []
    for c, frames in dsp.widget_frames(np.asarray(x, np.float64)[None], ends, st["fft_size"], st["needed"]):
        realizable = len(frames)
        spn = np.zeros((len(st["freq"]), realizable))
        for i in range(realizable):
            spn[:, i] = dsp.psd_frame(frames[i, 0], window)
        w = np.tile(st["weight"][:, None], (1, realizable))
        norm.append(dsp.normalise(dsp.log_spectrum(spn) + w, st["spec_min"], st["spec_max"]).T)
        frame_start.append(frame_start[-1] + realizable)
        refresh_chunk.append(c)
    norm = np.concatenate(norm) if norm else np.zeros((0, len(st["freq"])))
    return norm, np.array(frame_start, np.int64), np.array(refresh_chunk, np.int64)


def replay(x, ends, st):
    """One stream through the whole chain.  screen_replay's dict plus norm, frame_start, refresh_chunk."""
    norm, frame_start, refresh_chunk = frames_replay(x, ends, st)
    out = screen_replay(norm, frame_start, st)
    out.update(norm=norm, frame_start=frame_start, refresh_chunk=refresh_chunk)
    return out


def near_edge(v255, eps=1e-9):
    """Where v * 255 lies within eps of an integer: the truncation there may fall either way when the frames differ in the last bits."""
    return np.abs(v255 - np.rint(v255)) <= eps
