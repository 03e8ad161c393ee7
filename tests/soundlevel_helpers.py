"""References for SoundLevelBatch's detector (X7), numpy only: (i) the sequential recurrence e = a e + g q in np.longdouble, (ii)
the same in float64, (iii) a float64 restatement of the cell form (the tables rounded from long double, pass 1, the two-level
scan, pass 2, the folds over cells and intervals), the accuracy bar made from (i) and (ii) as tests/sos_helpers.py makes it, and
the inputs that the CPU and the GPU tests share.  Everything is vectorised over the rows and the time constants."""
import functools
from collections import namedtuple

import numpy as np

from sos_helpers import decaying_noise

RUN = 64
FS = 48000.0

# energy, peak [R, J]; last, max, min [R, J, ntau]; count [J]
Fields = namedtuple("Fields", "energy peak last max min count")
FIELD_NAMES = ("energy", "peak", "last", "max", "min")


def tables(fs, taus, cell):
    """(a, g, A, A64) [ntau] float64 as X7 makes them: x = -1 / (fs tau), a = exp(x) and g = -expm1(x) in long double, rounded
    once; A = the product 1 a a .. a of `cell` factors of the rounded a in long double, left to right, A64 of 64 cell factors."""
    ld = np.longdouble
    x = -ld(1) / (ld(fs) * np.asarray(taus, np.float64).astype(ld))
    a, g = np.exp(x).astype(np.float64), (-np.expm1(x)).astype(np.float64)
    z, al = np.ones(len(a), ld), a.astype(ld)
    A = None
    for n in range(RUN * cell):
        if n == cell:
            A = z.astype(np.float64)
        z = z * al
    return a, g, A, z.astype(np.float64)


def sequential(w, a, g, dtype=np.float64):
    """References (i) (dtype=np.longdouble) and (ii) (np.float64): e [R, ntau, T] of that dtype, from e = 0."""
    w = np.atleast_2d(np.asarray(w)).astype(np.float64).astype(dtype)
    a, g = np.asarray(a, np.float64).astype(dtype)[None], np.asarray(g, np.float64).astype(dtype)[None]
    R, T = w.shape
    e = np.zeros((R, a.shape[1]), dtype)
    out = np.empty((R, a.shape[1], T), dtype)
    q = w * w
    for t in range(T):
        e = a * e + g * q[:, t:t + 1]
        out[:, :, t] = e
    return out


def fields(w, e, interval):
    """The per-interval results of a flushed stream from the samples w [R, T] and the averages e [R, ntau, T], in e's dtype: the
    energy as the sequential sum of q, extrema that keep a NaN."""
    dtype = e.dtype
    w = np.atleast_2d(np.asarray(w)).astype(np.float64)
    R, T = w.shape
    J = -(-T // interval)
    q = w.astype(dtype) ** 2
    energy, peak = np.empty((R, J), dtype), np.empty((R, J))
    last, mx, mn = (np.empty((R, J, e.shape[1]), dtype) for _ in range(3))
    for j in range(J):
        s = slice(j * interval, min(T, (j + 1) * interval))
        energy[:, j] = np.cumsum(q[:, s], axis=1)[:, -1]
        peak[:, j] = np.abs(w[:, s]).max(axis=1)
        last[:, j], mx[:, j], mn[:, j] = e[:, :, s][:, :, -1], e[:, :, s].max(axis=2), e[:, :, s].min(axis=2)
    count = np.minimum(interval, T - np.arange(J) * interval).astype(np.int64)
    return Fields(energy, peak, last, mx, mn, count)


def cell_form(w, fs, taus, cell, interval):
    """Reference (iii): X7's order of operations in float64, one flushed call from the zero state.  P_c from zero; Q_r: q <- P_c
    + A q; U_(r+1) = Q_r + A64 U_r; S_c = U_r at a run's first cell, else S_(c+1) = P_c + A S_c; pass 2 from S_c; a cell's sum of q
    ascending from 0, an interval's cell sums ascending from 0 (the partial last cell last)."""
    w = np.atleast_2d(np.asarray(w)).astype(np.float64)
    a, g, A, A64 = tables(fs, taus, cell)
    R, T = w.shape
    nt = len(a)
    ipc = interval // cell
    J = -(-T // interval)
    C = -(-T // cell)
    runs = -(-C // RUN)
    Cp = max(runs * RUN, J * ipc)
    Cp = -(-Cp // RUN) * RUN
    runs = Cp // RUN
    pad = np.zeros((R, Cp * cell))
    pad[:, :T] = w
    live = (np.arange(Cp * cell) < T).reshape(1, Cp, cell)
    cells = pad.reshape(R, Cp, cell)
    q = cells * cells
    a_, g_, A_, A64_ = (v.reshape(1, nt, 1) for v in (a, g, A, A64))

    def step(e, t):
        return np.where(live[:, None, :, t], a_ * e + g_ * q[:, None, :, t], e)

    P = np.zeros((R, nt, Cp))
    for t in range(cell):
        P = step(P, t)
    Pr = P.reshape(R, nt, runs, RUN)
    Q = np.zeros((R, nt, runs))
    for k in range(RUN):
        Q = Pr[..., k] + A_ * Q
    U = np.zeros((R, nt, runs))
    for r in range(runs - 1):
        U[..., r + 1] = Q[..., r] + A64_[..., 0] * U[..., r]
    S = np.zeros((R, nt, runs, RUN))
    S[..., 0] = U
    for k in range(RUN - 1):
        S[..., k + 1] = Pr[..., k] + A_ * S[..., k]
    e = S.reshape(R, nt, Cp).copy()
    mx, mn = np.full(e.shape, -np.inf), np.full(e.shape, np.inf)
    en, pk = np.zeros((R, Cp)), np.zeros((R, Cp))
    for t in range(cell):
        e = step(e, t)
        on = live[:, None, :, t]
        mx, mn = np.where(on, np.maximum(mx, e), mx), np.where(on, np.minimum(mn, e), mn)
        en = en + q[:, :, t]                                      # behind the end q is +0: the sum keeps its bits
        pk = np.maximum(pk, np.abs(cells[:, :, t]))
    nci = J * ipc
    energy = np.zeros((R, J))
    enj = en[:, :nci].reshape(R, J, ipc)
    for k in range(ipc):
        energy = energy + enj[:, :, k]
    peak = pk[:, :nci].reshape(R, J, ipc).max(axis=2)
    peak = np.where(np.isnan(enj).any(axis=2), np.nan, peak)
    last_cell = np.minimum((np.arange(J) + 1) * ipc, C) - 1
    last = np.moveaxis(e[:, :, last_cell], 1, 2)
    with np.errstate(invalid="ignore"):
        vmax = np.moveaxis(mx[:, :, :nci].reshape(R, nt, J, ipc).max(axis=3), 1, 2)
        vmin = np.moveaxis(mn[:, :, :nci].reshape(R, nt, J, ipc).min(axis=3), 1, 2)
    count = np.minimum(interval, T - np.arange(J) * interval).astype(np.int64)
    return Fields(energy, peak, last, vmax, vmin, count)


def distance(y, ref, scale):
    """max |y - ref| per (row, time constant) over the intervals, relative to scale [R, ntau], in long double."""
    d = np.abs(np.asarray(y, np.longdouble) - np.asarray(ref, np.longdouble)).max(axis=1)
    return (d / np.where(scale > 0, scale, 1)).astype(np.float64)


def bar(e64, eld):
    """Per (row, time constant) max(64 e_seq, 1e-13), e_seq the distance of the float64 sequential recurrence from the long
    double one relative to the row's maximum: the rule of tests/sos_helpers.py.  Returns (bar, the maxima)."""
    peak = np.abs(eld).max(axis=2)
    e_seq = (np.abs(e64.astype(np.longdouble) - eld).max(axis=2) / np.where(peak > 0, peak, 1)).astype(np.float64)
    return np.maximum(64 * e_seq, 1e-13), peak


def check_fields(got, ref, seq_bar, e_peak, w, interval):
    """Asserts a detector result (Fields of float64 arrays) against the long double reference: count and peak exact, the
    averages' fields within the bar, the energy within 1e-10 interval max w^2 (the form of the loudness tests)."""
    np.testing.assert_array_equal(got.count, ref.count)
    np.testing.assert_array_equal(got.peak, ref.peak)
    for name in ("last", "max", "min"):
        d = distance(getattr(got, name), getattr(ref, name), e_peak)
        assert np.all(d <= seq_bar), (name, d.max(), seq_bar.min())
    w = np.atleast_2d(w).astype(np.float64)
    ebar = 1e-10 * interval * (w * w).max(axis=1, keepdims=True)
    de = np.abs(got.energy.astype(np.longdouble) - ref.energy).astype(np.float64)
    assert np.all(de <= np.maximum(ebar, 0)), ("energy", de.max(), ebar.min())


# ---- the inputs that the CPU and the GPU tests share -----------------------------------------------------------------------------

SEAM = dict(interval=480, cell=32, taus=(0.002, 0.02), fs=FS)       # the smallest configuration in which every seam exists
SEAM_LENGTHS = (1, 31, 32, 33, 479, 480, 481, 2047, 2048, 2049)
LONG_LENGTH = 64 * 64 * 32 + 3                                   # three runs of level two at cell 32
SEAM_KINDS = ("f64x3", "f32x65")


def seam_input(kind, T):
    seed = T * 5 + SEAM_KINDS.index(kind)
    if kind == "f64x3":
        return decaying_noise(3, T, seed, rt=1.0)
    return decaying_noise(65, T, seed, dtype=np.float32)


def long_input():
    return decaying_noise(2, LONG_LENGTH, 23, rt=1.0)


@functools.lru_cache(maxsize=None)
def cached(kind, T):
    """The references of one shared input at the SEAM settings, made once per process: (w, Fields in long double, Fields in
    float64 sequential, bar [R, ntau], the averages' maxima [R, ntau])."""
    w = long_input() if kind == "long" else seam_input(kind, T)
    a, g, _, _ = tables(SEAM["fs"], SEAM["taus"], SEAM["cell"])
    eld, e64 = sequential(w, a, g, np.longdouble), sequential(w, a, g, np.float64)
    b, peak = bar(e64, eld)
    return w, fields(w, eld, SEAM["interval"]), fields(w, e64, SEAM["interval"]), b, peak
