"""The loudness tests' numpy restatement of the definition in include/friture_hip.h (L2).  The product does not import it and
it does not import the product.  The K-weighting as a sequential sample loop over all streams at once, in float64 and in
np.longdouble (the reference of the error bounds), and row by row on Python floats for long recordings (the same float64
operations); the sub-block energies; the peaks, the true peak through resample_helpers.gather with the prototype as an
argument; the programme blocks, both gates and the loudness range; the cell decomposition that loudness.hip computes, which
tests/test_loudness_cpu.py pins to the sequential loop."""
from __future__ import annotations

import math

import numpy as np

import resample_helpers as rh

B = 4800
CELLS, CELL = 64, 75
STAGE1 = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -1.69065929318241, 0.73248077421585))
STAGE2 = ((1.0, -2.0, 1.0), (1.0, -1.99004745483398, 0.99007225036621))
PRESETS = {"mono": (1.0,), "stereo": (1.0, 1.0), "5.0": (1.0, 1.0, 1.0, 1.41, 1.41), "5.1": (1.0, 1.0, 1.0, 0.0, 1.41, 1.41)}


# ---- K-weighting ------------------------------------------------------------------------------------------------------------------

def step(x, s, dtype=np.float64):
    """One sample x [...] through both biquads, the state s = [z0, z1, z0', z1'] (arrays like x) updated in place; returns y.
    Direct form II transposed in lfilter's order: y = z0 + b0 x; z0 = (z1 + x b1) - y a1; z1 = x b2 - y a2."""
    y = x
    for k, (b, a) in enumerate((STAGE1, STAGE2)):
        b0, b1, b2, a1, a2 = dtype(b[0]), dtype(b[1]), dtype(b[2]), dtype(a[1]), dtype(a[2])
        x = y
        y = s[2 * k] + b0 * x
        s[2 * k] = (s[2 * k + 1] + x * b1) - y * a1
        s[2 * k + 1] = x * b2 - y * a2
    return y


def kweight(x, dtype=np.float64, state=None):
    """y [S, T] in `dtype`: the sequential recurrence over the samples, all streams at once, from the zero state."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    xe = x.astype(dtype)
    s = [np.zeros(x.shape[0], dtype) for _ in range(4)] if state is None else state
    y = np.empty(x.shape, dtype)
    for k in range(x.shape[1]):
        y[:, k] = step(xe[:, k], s, dtype)
    return y


def kweight_row(x, dtype=float):
    """y [T] of one stream x [T], sample by sample on scalars: Python floats (the same float64 operations as kweight, a long
    recording in a second) or np.longdouble scalars."""
    (b10, b11, b12), (_, a11, a12) = [[dtype(v) for v in c] for c in STAGE1]
    (b20, b21, b22), (_, a21, a22) = [[dtype(v) for v in c] for c in STAGE2]
    z0 = z1 = w0 = w1 = dtype(0.0)
    out = []
    values = np.asarray(x, np.float64).tolist()
    for v in (values if dtype is float else [dtype(v) for v in values]):
        y1 = z0 + b10 * v
        z0 = (z1 + v * b11) - y1 * a11
        z1 = v * b12 - y1 * a12
        y2 = w0 + b20 * y1
        w0 = (w1 + y1 * b21) - y2 * a21
        w1 = y1 * b22 - y2 * a22
        out.append(y2)
    return np.array(out, np.float64 if dtype is float else dtype)


def energies(y):
    """e [S, T // B]: the sum of y^2 over every whole sub-block, in y's dtype."""
    nb = y.shape[1] // B
    return np.sum(y[:, :nb * B].reshape(y.shape[0], nb, B) ** 2, axis=2)


# ---- the cell decomposition of loudness.hip -----------------------------------------------------------------------------------------

def powers():
    """A^(75 c), c = 0 .. 64, [65, 4, 4]: column j is the state 75 c zero samples after the unit state e_j."""
    pw = np.empty((CELLS + 1, 4, 4))
    for j in range(4):
        s = [np.float64(i == j) for i in range(4)]
        for c in range(CELLS + 1):
            pw[c, :, j] = s
            for _ in range(CELL):
                step(np.float64(0.0), s)
    return pw


def affine(M, v, z):
    """M v + z per row as (((m0 v0 + m1 v1) + m2 v2) + m3 v3) + z; M [..., 4, 4], v and z [..., 4]."""
    return (((M[..., 0] * v[..., None, 0] + M[..., 1] * v[..., None, 1]) + M[..., 2] * v[..., None, 2]) + M[..., 3] * v[..., None, 3]) + z


def cell_energies(x, state=None):
    """(e [S, T // B], the filter state [S, 4] at the start of sub-block T // B) as loudness.hip forms them, float64."""
    x = np.asarray(x, np.float64)
    S, nb = x.shape[0], x.shape[1] // B
    pw = powers()
    cells = x[:, :nb * B].reshape(S, nb, CELLS, CELL)
    s = [np.zeros((S, nb, CELLS)) for _ in range(4)]
    for i in range(CELL):
        step(cells[..., i], s)
    z = np.stack(s, axis=-1)                                        # [S, nb, 64, 4]
    P = np.zeros((S, nb, CELLS + 1, 4))
    for c in range(CELLS):
        P[:, :, c + 1] = affine(pw[1], P[:, :, c], z[:, :, c])
    start = np.zeros((S, nb + 1, 4))
    if state is not None:
        start[:, 0] = state
    for b in range(nb):
        start[:, b + 1] = affine(pw[CELLS], start[:, b], P[:, b, CELLS])
    first = affine(pw[None, None, :CELLS], start[:, :nb, None, :], P[:, :, :CELLS])      # [S, nb, 64, 4]
    s = [first[..., r].copy() for r in range(4)]
    e = np.zeros((S, nb, CELLS))
    for i in range(CELL):
        y = step(cells[..., i], s)
        e = e + y * y
    total = np.zeros((S, nb))
    for c in range(CELLS):
        total = total + e[:, :, c]
    return total, start[:, nb]


# ---- peaks ------------------------------------------------------------------------------------------------------------------------

def emitted(n_in, R, flush):
    """(sub-blocks with an energy, sub-blocks with peaks) after n_in samples in total."""
    if flush:
        return n_in // B, -(-n_in // B)
    e = max(0, (n_in - R) // B)
    return e, e


def sample_peaks(x, n_blocks):
    x = np.asarray(x, np.float64)
    pad = np.zeros((x.shape[0], n_blocks * B))
    n = min(x.shape[1], n_blocks * B)
    pad[:, :n] = x[:, :n]
    return np.max(np.abs(pad.reshape(x.shape[0], n_blocks, B)), axis=2) if n_blocks else np.zeros((x.shape[0], 0))


def true_peaks(x, R, h, n_blocks):
    """max |u| per sub-block over the outputs 4 B b .. 4 B (b + 1) - 1 that the flushed stream x [S, N] has (m < 4 N)."""
    x = np.asarray(x, np.float64)
    out = np.zeros((x.shape[0], n_blocks))
    for b in range(n_blocks):
        m0, m1 = 4 * B * b, min(4 * B * (b + 1), 4 * x.shape[1])
        out[:, b] = np.max(np.abs(rh.gather(x, 4, 1, 4 * R, h, m0, m1)), axis=1)
    return out


# ---- programmes ---------------------------------------------------------------------------------------------------------------------

def lkfs(z):
    z = np.asarray(z)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def block_powers(e, weights, length):
    """z [P, max(0, nb - length + 1)]: sum_c G[c] (e[j] + .. + e[j + length - 1]) / (length B), in e's dtype."""
    C = len(weights)
    S, nb = e.shape
    n = max(0, nb - length + 1)
    z = np.zeros((S // C, n), e.dtype)
    ep = e.reshape(S // C, C, nb)
    for c in range(C):
        inner = np.zeros((S // C, n), e.dtype)
        for i in range(length):
            inner = inner + ep[:, c, i:i + n]
        z = z + e.dtype.type(weights[c]) * inner
    return z / e.dtype.type(length * B)


def gated(z, offset):
    """(the blocks above -70, Gamma = l(their mean) - offset, the blocks above both) of one programme's powers z [n]."""
    l = lkfs(z)
    absolute = l > -70.0
    if not absolute.any():
        return absolute, -np.inf, absolute
    gamma = lkfs(np.mean(z[absolute])) - offset
    return absolute, gamma, absolute & (l > gamma)


def integrated(z400):
    out = np.full(z400.shape[0], -np.inf)
    for p in range(z400.shape[0]):
        _, _, keep = gated(z400[p], 10.0)
        if keep.any():
            out[p] = lkfs(np.mean(z400[p][keep]))
    return out


def loudness_range(z3s):
    out = np.zeros(z3s.shape[0])
    for p in range(z3s.shape[0]):
        _, _, keep = gated(z3s[p], 20.0)
        v = np.sort(lkfs(z3s[p][keep]))
        n = len(v)
        if n >= 2:
            out[p] = v[int(math.floor((n - 1) * 0.95 + 0.5))] - v[int(math.floor((n - 1) * 0.10 + 0.5))]
    return out


def gate_margin(z, offset):
    """The smallest distance in LU of a block's loudness from the thresholds it is compared with (-70 and Gamma), over the
    programmes of z [P, n]; inf when there is nothing to compare."""
    worst = np.inf
    for p in range(z.shape[0]):
        l = lkfs(z[p]).astype(np.float64)
        absolute, gamma, _ = gated(z[p], offset)
        finite = l[np.isfinite(l)]
        if finite.size:
            worst = min(worst, float(np.min(np.abs(finite + 70.0))))
        if absolute.any():
            worst = min(worst, float(np.min(np.abs(l[absolute] - float(gamma)))))
    return worst


def reference(x, weights, R, h, flush=True, dtype=np.longdouble, y=None):
    """Everything a whole recording x [S, N] gives in one call, from the sequential recurrence in `dtype`: a dict of energy,
    sample_peak, true_peak (None without h), z400, z3s, momentary, short_term, integrated, loudness_range (float64 where
    they are results) and the gate margins."""
    x = np.asarray(x)
    ne, npk = emitted(x.shape[1], R, flush)
    y = kweight(x, dtype) if y is None else y
    e = energies(y)[:, :ne]
    z400, z3s = block_powers(e, weights, 4), block_powers(e, weights, 30)
    return dict(energy=e, sample_peak=sample_peaks(x, npk), true_peak=None if h is None else true_peaks(x, R, h, npk),
                z400=z400, z3s=z3s, momentary=lkfs(z400).astype(np.float64), short_term=lkfs(z3s).astype(np.float64),
                integrated=integrated(z400).astype(np.float64), loudness_range=loudness_range(z3s).astype(np.float64),
                margin=min(gate_margin(z400, 10.0), gate_margin(z3s, 20.0)))


def dbfs(amp_db):
    return 10.0 ** (amp_db / 20.0)


def sine(f, n, amp=1.0, phase=0.0):
    return amp * np.sin(2 * np.pi * f * np.arange(n) / 48000.0 + phase)
