"""The octave-spectrum widget's processing chain (friture/octavespectrum.py:91-156) without Qt:
Octave_Filters.filter (FFT overlap-add bank on the GPU), per-band exponential smoothing of y^2
(frt_exp_smooth_groups: all bands of a chunk in one launch) and 10 log10(sp + 1e-30) + weighting.

`OctaveSpectrumBatch` runs the same chain over whole recordings, many streams at a time, in device calls
(frt_octspec_run, octspecbatch.hip); its dB rows are what `plotcurves.CurveBatch` reads."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._batchio import carried, check_keep, check_samples, null_stream, source, to_host
from .constants import NOCTAVE, SAMPLING_RATE
from .octavefilters import Octave_Filters
from .signal.exp_smoothing import exp_smoothed_value_groups

DEFAULT_BANDSPEROCTAVE = 3      # octavespectrum_settings.py:25-31
DEFAULT_RESPONSE_TIME = 1.


class OctaveSpectrum:
    def __init__(self, bandsperoctave: int = DEFAULT_BANDSPEROCTAVE, weighting: int = 1,
                 response_time: float = DEFAULT_RESPONSE_TIME):
        self.filters = Octave_Filters(bandsperoctave)
        self.weighting = weighting
        self.dispbuffers = [0] * bandsperoctave * NOCTAVE
        self.setresponsetime(response_time)

    def setresponsetime(self, response_time):
        self.response_time = response_time
        w = 0.65
        decs = self.filters.get_decs()
        ns = [response_time * SAMPLING_RATE / dec for dec in decs]
        Ns = [2 * 4096 / dec for dec in decs]
        self.alphas = [1. - (1. - w) ** (1. / (n + 1)) for n in ns]
        self.kernels = [(1. - alpha) ** np.arange(N - 1, -1, -1) for alpha, N in zip(self.alphas, Ns)]

    def setbandsperoctave(self, bandsperoctave):
        self.filters.setbandsperoctave(bandsperoctave)
        self.dispbuffers = [0] * bandsperoctave * NOCTAVE
        self.setresponsetime(self.response_time)

    def handle_new_data(self, floatdata):
        if floatdata.shape[1] == 0:
            return None
        y, _ = self.filters.filter(floatdata[0, :])
        bpo = self.filters.bandsperoctave
        # The reference smooths band by band (octavespectrum.py:103-112); bands of one octave share kernel, alpha and length and lie
        # back to back in the bank's packed output, so the chunk's 9 x bpo values are ONE call (frt_exp_smooth_groups, y^2 formed on
        # the device; until round 4: one call per octave, nine device round trips per chunk).
        blocks = []
        if getattr(self.filters, "_packed", None) is not None and y[0].base is self.filters._packed:
            blocks = [(y[octave * bpo], bpo) for octave in range(NOCTAVE)]      # this call's packed output: octaves are [bpo, m] blocks
        else:
            for octave in range(NOCTAVE):
                lo = octave * bpo
                row, m = y[lo], y[lo].shape[0]
                packed = all(y[lo + i].ctypes.data == row.ctypes.data + i * m * 8 and y[lo + i].shape[0] == m for i in range(1, bpo))
                blocks.append((row, bpo) if packed and row.flags.c_contiguous else np.stack(y[lo:lo + bpo]))
        sp = exp_smoothed_value_groups([self.kernels[o * bpo] for o in range(NOCTAVE)], [self.alphas[o * bpo] for o in range(NOCTAVE)],
                                       blocks, np.asarray(self.dispbuffers, np.float64), square=True)
        self.dispbuffers = list(sp)
        w = {0: 0., 1: self.filters.A, 2: self.filters.B}.get(self.weighting, self.filters.C)
        db_spectrogram = 10 * np.log10(sp + 1e-30) + w
        return self.filters.flow, self.filters.fhigh, self.filters.f_nominal, db_spectrogram


class OctaveSpectrumStream(OctaveSpectrum):
    """The same chain with everything between the chunk and the 9 x bpo dB values on the device: the FIR bank's tails, the
    smoothed energies and the weighting live in the bank object (frt_octbank_energies in mode 1, one block = the chunk);
    a chunk costs one upload of its samples and one download of the band vector.  Values are float32 on the way out
    (1e-7 relative; the north star's band-energy tolerance is 1e-5)."""

    def __init__(self, bandsperoctave: int = DEFAULT_BANDSPEROCTAVE, weighting: int = 1,
                 response_time: float = DEFAULT_RESPONSE_TIME):
        super().__init__(bandsperoctave, weighting, response_time)
        from .filter import FirBank
        self._bank = FirBank(bandsperoctave, 1)

    def setbandsperoctave(self, bandsperoctave):
        super().setbandsperoctave(bandsperoctave)
        from .filter import FirBank
        self._bank = FirBank(bandsperoctave, 1)

    def handle_new_data(self, floatdata):
        n = floatdata.shape[1]
        if n == 0:
            return None
        w = {0: np.zeros(len(self.alphas)), 1: self.filters.A, 2: self.filters.B}.get(self.weighting, self.filters.C)
        x = np.ascontiguousarray(floatdata[0:1, :], np.float32)
        db = self._bank.energies(x, n, np.asarray(self.alphas), weight_db=w, as_db=True)[0, 0]
        return self.filters.flow, self.filters.fhigh, self.filters.f_nominal, db.astype(np.float64)


# ---- the same chain over whole recordings ---------------------------------------------------------------------------------

SUBBLOCK = 2 ** (NOCTAVE - 1)       # 256: the chunk lengths' unit
MAX_CHUNK = 1024


def octave_schedule(n_samples, chunk=512, ends=None, pending=0):
    """ends [R] int64 of a stream of n_samples behind `pending` received and not consumed samples, counted from the stream's
    first sample (an end inside the pending samples is negative): refresh r is the chunk that ends at ends[r], chunk lengths are
    the differences of [-pending, ends...].  Default: multiples of `chunk` (256, 512, 768 or 1024) from -pending, up to
    n_samples.  Every chunk length must be a multiple of 256 in [256, 1024]: ValueError otherwise."""
    n_samples, pending = int(n_samples), int(pending)
    if ends is None:
        if chunk not in (256, 512, 768, 1024):
            raise ValueError(f"chunk {chunk} (256, 512, 768 or 1024)")
        return np.arange(chunk - pending, n_samples + 1, chunk, dtype=np.int64)
    ends = np.asarray(ends, np.int64).reshape(-1)
    lengths = np.diff(ends, prepend=-pending)
    bad = np.flatnonzero((lengths < SUBBLOCK) | (lengths > MAX_CHUNK) | (lengths % SUBBLOCK != 0))
    if bad.size:
        raise ValueError(f"chunk {int(bad[0])} has {int(lengths[bad[0]])} samples: chunk lengths must be multiples of {SUBBLOCK} in "
                         f"[{SUBBLOCK}, {MAX_CHUNK}] and ends sorted")
    if ends.size and ends[-1] > n_samples:
        raise ValueError(f"end {int(ends[-1])} beyond the {n_samples} samples")
    return ends


class OctaveSpectrumState(NamedTuple):
    """What an octave-spectrum widget carries between two calls."""
    energies: object        # [S, 9 * bpo] float64: the smoothed band energies sp (the reference's dispbuffers)
    tails: object           # [S, 9, bpo + 1, 511] float64: the bank's pending tails per stage and filter, the decimator last
    samples: object         # [S, pending] float64: received and not consumed (float32 input widened exactly)
    pending: int


class OctaveSpectrumResult(NamedTuple):
    db: object              # [S, R', 9 * bpo] float64 (R' = R, or 1 with keep="last"); [R', 9 * bpo] for one stream given without its axis
    energy: object          # the smoothed sp in the same shape with with_energy, else None
    flow: object            # [9 * bpo] band edges and labels, as OctaveSpectrum.handle_new_data returns them
    fhigh: object
    f_nominal: object
    ends: object            # [R] int64 (host): the refreshes' ends, counted from this call's first sample
    state: OctaveSpectrumState


class OctaveSpectrumBatch:
    """S streams of a whole recording through the octave-spectrum widget's chain in device calls, as widgets fed chunk by chunk
    would have seen it (one stream = row 0 of one widget: the reference filters floatdata[0, :] only): the FFT overlap-add bank
    over the consumed samples with block energies per 256 samples, then per (stream, band) the walk sp = E + sp (1 - alpha)^m
    over the sub-blocks, read out as sp and 10 log10(sp + 1e-30) + weighting where a chunk ends (frt_octspec_run).  Fixed
    settings, no pause.

    run(x, chunk=512 | ends=..., state=None, keep="all" | "last", with_energy=False) takes [S, T] (the stream axis may be left
    out for one stream), float32 or float64, numpy array or CUDA tensor.  Results are numpy for numpy input and CUDA tensors
    for CUDA input; a CUDA `db` is contiguous [S, R, 9 * bpo]: what CurveBatch.run reads in place.

    Chunk lengths are multiples of 256 in [256, 1024].  256 = 2^(NOCTAVE - 1): the reference decimates every chunk on its own
    (y[:N:2] at each of the eight decimations), which lies on one uniform grid across chunks only where every chunk is a whole
    number of 2^8 samples.  1024 is the reference's own limit: its first stage transforms np.fft.rfft(x, 1536), which crops
    anything longer (and frt_octbank_energies refuses it).  Ragged chunk lengths stay with OctaveSpectrumStream.  Samples behind
    the last chunk end are not consumed: they are carried in the state and stand in front of the next call's samples.

    The state is the truth, the bank handle (one FirBank per number of streams) a cache: every run loads tails and energies
    from `state` (None: a fresh widget, zeros) and reads them out afterwards; the caller's state is never modified.  A recording
    fed in pieces equals the recording fed whole to rounding, not bit for bit: the bank's overlap-add sets of 3072 outputs start
    with each call (and each slab), so the same products are summed in another order.  Block energies, stage signals and staged
    samples live in at most `scratch_bytes` of device memory (or one chunk's): longer recordings go through in time slabs of
    whole refreshes; the number of launches and copies of a run depends on the number of slabs only."""

    def __init__(self, bandsperoctave: int = DEFAULT_BANDSPEROCTAVE, weighting: int = 1,
                 response_time: float = DEFAULT_RESPONSE_TIME):
        from . import filter_design, tables
        from .filter import octave_frequencies
        from .octavefilters import nominal_labels
        if "boct_%d" % bandsperoctave not in filter_design.load_tables():
            raise Exception("Unknown bandsperoctave: %d" % (bandsperoctave))
        self.bandsperoctave = int(bandsperoctave)
        self.nbands = NOCTAVE * self.bandsperoctave
        self.weighting = weighting
        self.response_time = response_time
        self.fi, self.flow, self.fhigh = octave_frequencies(self.nbands, self.bandsperoctave)
        self.f_nominal = nominal_labels(self.fi, self.bandsperoctave)
        A, B, C = tables.weighting_db(self.fi)
        self.w = {0: np.zeros(self.nbands), 1: A, 2: B}.get(weighting, C)
        decs = [2 ** j for j in range(NOCTAVE)[::-1] for _ in range(self.bandsperoctave)]
        self.alphas = np.array([1. - (1. - 0.65) ** (1. / (response_time * SAMPLING_RATE / dec + 1)) for dec in decs])
        self.last_slabs = 0             # time slabs of the latest run
        self._banks = {}

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def schedule(self, n_samples, chunk=512, ends=None, state=None):
        """octave_schedule from a carried state's pending samples on."""
        return octave_schedule(n_samples, chunk, ends, 0 if state is None else state.pending)

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _bank(self, streams):
        if streams not in self._banks:
            from .filter import FirBank
            self._banks[streams] = FirBank(self.bandsperoctave, streams)
        return self._banks[streams]

    def _check_input(self, x, state):
        x, is_np, squeeze, pending = check_samples("OctaveSpectrumBatch", x, state)
        if state is not None:
            S = x.shape[0]
            want = {"energies": (S, self.nbands), "tails": (S, NOCTAVE, self.bandsperoctave + 1, 511), "samples": (S, pending)}
            got = {name: tuple(getattr(state, name).shape) for name in want}
            if pending < 0 or got != want:
                raise ValueError(f"state of another shape: {got} (want {want}), pending {pending}")
        return x, is_np, squeeze, pending

    def run(self, x, chunk=512, ends=None, state=None, keep="all", with_energy=False, scratch_bytes=1 << 30):
        check_keep(keep, "all", "last")
        x, is_np, squeeze, pending = self._check_input(x, state)
        ends = self.schedule(x.shape[-1], chunk, ends, state)
        import torch
        lib = _lib.init()
        S, T, B, R = x.shape[0], x.shape[-1], self.nbands, len(ends)
        f64, vp = torch.float64, ctypes.c_void_p
        last = int(ends[-1]) if R else -pending                      # the consumed samples end here
        held, sp_in, tails_in = (None, None, None) if state is None else (state.samples, state.energies, state.tails)
        with null_stream(x, is_np) as dev:
            x0 = xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev) if is_np else x
            held, sp_in = carried(dev, held, (S, pending)), carried(dev, sp_in, (S, B))
            Ro = R if keep == "all" else min(R, 1)
            db = torch.empty((S, Ro, B), dtype=f64, device=dev)
            energy = torch.empty((S, Ro, B), dtype=f64, device=dev) if with_energy else None
            self.last_slabs = 0
            if R:
                bank = self._bank(S)
                _lib.check(lib.frt_octbank_set_stream(bank._h, None))
                if state is None:
                    bank.reset()
                else:
                    bank.set_tails(carried(dev, tails_in, (S, NOCTAVE, self.bandsperoctave + 1, 511)))
                if pending:                                          # the pending samples stand in front: one float64 buffer
                    xd = torch.cat([held, xd[:, :max(last, 0)].to(f64)], dim=1)[:, :pending + last]
                xd, x_ptr, code, strides = source(xd, True)
                table = np.ascontiguousarray(ends + pending)
                sp_out = torch.empty((S, B), dtype=f64, device=dev)
                slabs = ctypes.c_int(0)
                _lib.check(lib.frt_octspec_run(
                    bank._h, vp(x_ptr), code, pending + last, strides[0], table.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), R,
                    self.alphas.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                    np.ascontiguousarray(self.w, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), vp(sp_in.data_ptr()),
                    vp(sp_out.data_ptr()), vp(db.data_ptr()), vp(energy.data_ptr()) if with_energy else None, int(keep == "last"),
                    int(scratch_bytes), ctypes.byref(slabs)))
                self.last_slabs = slabs.value
                tails = bank.get_tails(torch.empty((S, NOCTAVE, self.bandsperoctave + 1, 511), dtype=f64, device=dev))
                rest = x0[:, max(last, 0):].to(f64)                  # behind the last end (inside the pending samples: last < 0)
                if last < 0:
                    rest = torch.cat([held[:, pending + last:], rest], dim=1)
                new_state = OctaveSpectrumState(sp_out, tails, rest.clone(memory_format=torch.contiguous_format), 0)
            else:
                tails = carried(dev, tails_in, (S, NOCTAVE, self.bandsperoctave + 1, 511))
                new_state = OctaveSpectrumState(sp_in, tails, torch.cat([held, xd.to(f64)], dim=1), 0)
            new_state = new_state._replace(pending=int(new_state.samples.shape[1]))
            if is_np:
                db, energy, new_state = to_host((db, energy, new_state))
        if squeeze:
            db = db[0]
            energy = energy[0] if with_energy else None
        return OctaveSpectrumResult(db, energy, self.flow, self.fhigh, self.f_nominal, ends, new_state)
