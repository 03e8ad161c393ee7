"""References for SoundLevelBatch's detector (X7), numpy only: (i) the sequential recurrence e = a e + g q in np.longdouble, (ii)
the same in float64, (iii) a float64 restatement of the cell form (the tables rounded from long double, pass 1, the two-level
scan, pass 2, the folds over cells and intervals), the accuracy bar made from (i) and (ii) as tests/sos_helpers.py makes it, and
the inputs and settings that the CPU and the GPU tests share (the seams, and the edge settings of test_soundlevel_edges_*.py), and the
comparisons that the GPU test files share.  Everything is vectorised over the rows and the time constants."""
import functools
from collections import namedtuple

import numpy as np

from sos_helpers import decaying_noise, led  # noqa: F401 (led: for the GPU test files)

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


UNIT_AT = 703


def unit_and_noise(T):
    """Three rows: a unit sample followed by silence, decaying noise, and silence around a unit sample at UNIT_AT (the last sample
    of cell 0 at cell 704, so that cell 2 starts from A times a normal number)."""
    w = decaying_noise(3, T, 3 * T + 1, rt=1.0)
    w[[0, 2]] = 0.0
    w[0, 0] = w[2, UNIT_AT] = 1.0
    return w


INPUTS = {"f64x3": lambda T: seam_input("f64x3", T), "f32x65": lambda T: seam_input("f32x65", T), "long": lambda T: long_input(),
          "f64x1": lambda T: decaying_noise(1, T, 3 * T + 2, rt=1.0), "f64x2": lambda T: decaying_noise(2, T, 3 * T + 3, rt=1.0),
          "unit+noise": unit_and_noise}


def cached(kind, T, fs, taus, cell, interval):
    """The references of one named input at the given settings, made once per process and keyed by (kind, T, fs, taus, cell,
    interval): (w, Fields in long double, Fields in float64 sequential, bar [R, ntau], the averages' maxima [R, ntau])."""
    return _cached(kind, int(T), float(fs), tuple(float(t) for t in taus), int(cell), int(interval))


@functools.lru_cache(maxsize=None)
def _cached(kind, T, fs, taus, cell, interval):
    w = INPUTS[kind](T)
    a, g, _, _ = tables(fs, taus, cell)
    eld, e64 = sequential(w, a, g, np.longdouble), sequential(w, a, g, np.float64)
    b, peak = bar(e64, eld)
    return w, fields(w, eld, interval), fields(w, e64, interval), b, peak


def worst_ratio(got, ref, seq_bar, e_peak):
    """The largest distance / bar over last, max and min: the figure the parity tests print."""
    return max(float((distance(getattr(got, n), getattr(ref, n), e_peak) / seq_bar).max()) for n in ("last", "max", "min"))


# ---- the edge settings: every number of time constants, cell and interval extremes, walk lengths, table extremes ------------------
# (test_soundlevel_edges_cpu.py / _gpu.py); a case is (kind, T, settings)

def edge(kind, T, taus, cell, interval, fs=FS):
    return kind, T, dict(interval=interval, cell=cell, taus=taus, fs=fs)


EDGE_TAUS = {1: (0.002,), 3: (0.002, 0.02, 0.035), 4: (0.002, 0.02, 0.125, 1.0)}
TAUS_LENGTHS = (2049, 64 * 32 + 33, 2 * 64 * 32 + 33)                # the last: three runs, so that A64 meets a U that is not 0
PIECES_LENGTH = 64 * 32 + 33
PIECE_CUTS = (1, 31, 32, 33, 480, 1000, 2049)                      # of the longer row
LONG_INTERVAL_LENGTH = 3 * 1280 + 5                                # cell 16, interval 1280: 80 cells per interval, more than a run
LONG_INTERVAL_CUTS = (1024, 1280, 1281)                            # a run seam inside interval 0, the interval's end, one behind it
WALK_RUNS = (17, 18, 33, 34)                                       # 16, 17, 32 and 33 steps of level two


def run_edge_length(cell):
    """65 cells and 17 samples: one run seam, one step of level two, a partial last cell."""
    return 65 * cell + 17


TAUS_CASES = [edge("f64x3", T, EDGE_TAUS[n], 32, 480) for n in EDGE_TAUS for T in TAUS_LENGTHS]
EXTREME_CASES = [edge("f64x2", LONG_INTERVAL_LENGTH if cell == 16 else run_edge_length(cell), (0.002, 0.125), cell, interval)
                 for cell, interval in ((16, 16), (16, 48), (48, 96), (80, 480), (1024, 1024), (1024, 2048))]
LONG_INTERVAL_CASE = edge("f64x2", LONG_INTERVAL_LENGTH, (0.002, 0.125), 16, 1280)
WALK_CASES = [edge("f64x1", (nr - 1) * 1024 + 5, EDGE_TAUS[3], 16, 16 * 64) for nr in WALK_RUNS]
# a = 1 - 5.2e-6; A = a^1024 and A64 exactly 0; A = 3.3e-15 and A64 = 0
TABLE_CASES = [edge("f64x2", run_edge_length(1024), (1.0, 0.125), 1024, 1024, fs=192000.0),
               edge("f64x2", run_edge_length(1024), (20e-6, 0.125), 1024, 1024), edge("f64x2", run_edge_length(32), (20e-6, 0.125), 32, 480)]
DENORMAL_CASE = edge("unit+noise", run_edge_length(704), (20e-6,), 704, 704)       # A = a^704 = e^-733: a denormal double
EDGE_CASES = TAUS_CASES + EXTREME_CASES + [LONG_INTERVAL_CASE] + WALK_CASES + TABLE_CASES + [DENORMAL_CASE]


def edge_id(case):
    kind, T, s = case
    return f"{kind}-{T}-fs{s['fs']:g}-ntau{len(s['taus'])}-tau{min(s['taus']):g}-cell{s['cell']}-int{s['interval']}"


# ---- what the GPU test files share -------------------------------------------------------------------------------------------------

def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same_bits(a, b):
    a, b = host(a), host(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


RESULT_FIELDS = "leq lmax lmin level peak_db energy peak count total_leq sel total_lmax total_lmin total_peak_db".split()
DETECTOR_FIELDS = "energy peak last max min count total_energy total_peak total_max total_min".split()


def same_result(a, b, fields=None):
    for name in fields or (RESULT_FIELDS if hasattr(a, "leq") else DETECTOR_FIELDS):
        same_bits(getattr(a, name), getattr(b, name))


def same_detector_state(a, b):
    assert (a.rows, a.n, a.final, a.settings) == (b.rows, b.n, b.final, b.settings)
    same_bits(a.data, b.data)


def as_fields(d):
    return Fields(*(host(getattr(d, n)) for n in ("energy", "peak", "last", "max", "min", "count")))


def in_pieces(batch, x, cuts, method="detect", **kw):
    """The calls over x[..., a:b] for consecutive cuts, the last one flushed: (the results, the last state)."""
    state, parts = None, []
    ends = list(cuts) + [x.shape[-1]]
    for a, b in zip([0] + list(cuts), ends):
        r = getattr(batch, method)(x[..., a:b], state=state, flush=b == x.shape[-1], **kw)
        state = r.state
        parts.append(r)
    return parts, state


def joined(parts, name):
    axis = 0 if name == "count" else (-2 if name in ("last", "max", "min", "lmax", "lmin", "level") else -1)
    return np.concatenate([host(getattr(p, name)) for p in parts], axis=axis)


def pieces_equal_whole(batch, x, cuts, method="detect", **kw):
    whole = getattr(batch, method)(x)
    parts, state = in_pieces(batch, x, cuts, method, **kw)
    names = ("energy peak last max min count" if method == "detect" else "leq lmax lmin level peak_db energy peak count").split()
    for name in names:
        same_bits(joined(parts, name), getattr(whole, name))
    for name in (DETECTOR_FIELDS[6:] if method == "detect" else RESULT_FIELDS[8:]):
        same_bits(getattr(parts[-1], name), getattr(whole, name))
    return whole, state
