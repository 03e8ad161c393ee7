"""References for SosBatch (X6), numpy only: (i) the sequential recurrence in np.longdouble, (ii) the same in float64, (iii) a
float64 restatement of the cell form (M rounded from long double, then passes 1, 2 and 3), the accuracy bar made from (i) and (ii),
the closed-form impulse response of a cascade, the inputs that the CPU and the GPU tests share (the seams, the banks, and the
edge inputs of test_sos_edges_*.py behind the sections(K) / bank(F, K) builders), and the comparisons that the GPU test files
share.  Everything is vectorised over the output rows (input row, filter)."""
import functools

import numpy as np

RUN = 64


def normalise(sos):
    """[F, K, 6] float64 with a0 = 1, each quotient rounded once."""
    s = np.asarray(sos, np.float64)
    s = s.reshape((-1,) + s.shape[-2:])
    s = s / s[..., 3:4]
    s[..., 3] = 1.0
    return s


def layout(x, sos, fan):
    """(xx [N, T] float64, coef [N, K, 6]) per output row: bank mode (row, filter) row-major, row mode filter r % F."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    s = normalise(sos)
    R, F = x.shape[0], s.shape[0]
    if fan:
        return np.repeat(x, F, axis=0), np.tile(s, (R, 1, 1))
    return x, s[np.arange(R) % F]


def _steps(xx, coef, z, dtype):
    """Step every row of xx [N, n] through its sections from the states z [N, 2K] (changed in place): y [N, n]."""
    K = coef.shape[1]
    c = coef.astype(dtype)
    y = np.empty(xx.shape, dtype)
    for t in range(xx.shape[1]):
        v = xx[:, t].astype(dtype)
        for k in range(K):
            o = c[:, k, 0] * v + z[:, 2 * k]
            z[:, 2 * k] = (c[:, k, 1] * v - c[:, k, 4] * o) + z[:, 2 * k + 1]
            z[:, 2 * k + 1] = c[:, k, 2] * v - c[:, k, 5] * o
            v = o
        y[:, t] = v
    return y


def sequential(x, sos, fan=False, dtype=np.float64, reverse=False):
    """References (i) (dtype=np.longdouble) and (ii) (np.float64): y [N, T] of that dtype."""
    xx, coef = layout(x, sos, fan)
    if reverse:
        xx = xx[:, ::-1]
    y = _steps(xx, coef, np.zeros((xx.shape[0], 2 * coef.shape[1]), dtype), dtype)
    return y[:, ::-1] if reverse else y


def transition(coef, steps):
    """M [N, 2K, 2K] float64: state i after `steps` samples of silence from the unit state j, stepped in long double (all the
    unit states of all rows in one walk)."""
    N, K = coef.shape[:2]
    S2 = 2 * K
    z = np.tile(np.eye(S2, dtype=np.longdouble), (N, 1))         # row n * 2K + j: filter n from the unit state j
    _steps(np.zeros((N * S2, steps)), np.repeat(coef, S2, axis=0), z, np.longdouble)
    return np.ascontiguousarray(z.reshape(N, S2, S2).transpose(0, 2, 1).astype(np.float64))


def _matvec(M, s, p):
    acc = p.copy()
    for k in range(M.shape[-1]):
        acc += M[..., :, k] * s[..., k:k + 1]
    return acc


def cell_form(x, sos, cell, fan=False):
    """Reference (iii): passes 1, 2 (two levels, runs of 64 cells) and 3 in float64, from the zero state: y [N, T]."""
    xx, coef = layout(x, sos, fan)
    N, T = xx.shape
    S2 = 2 * coef.shape[1]
    C = -(-T // cell)
    runs = -(-C // RUN)
    Cp = runs * RUN
    pad = np.zeros((N, Cp * cell))
    pad[:, :T] = xx
    cells = pad.reshape(N * Cp, cell)
    ccoef = np.repeat(coef, Cp, axis=0)
    M, M64 = transition(coef, cell), transition(coef, RUN * cell)
    P = np.zeros((N * Cp, S2))
    _steps(cells, ccoef, P, np.float64)
    P = P.reshape(N, runs, RUN, S2)
    Mr = M[:, None]                                              # [N, 1, 2K, 2K] against [N, runs, 2K]
    q = np.zeros((N, runs, S2))
    for j in range(RUN):
        q = _matvec(Mr, q, P[:, :, j])
    U = np.zeros((N, runs, S2))
    for r in range(runs - 1):
        U[:, r + 1] = _matvec(M64, U[:, r], q[:, r])
    S = np.zeros((N, runs, RUN, S2))
    S[:, :, 0] = U
    for j in range(RUN - 1):
        S[:, :, j + 1] = _matvec(Mr, S[:, :, j], P[:, :, j])
    y = _steps(cells, ccoef, S.reshape(N * Cp, S2).copy(), np.float64)
    return y.reshape(N, Cp * cell)[:, :T]


def distance(y, ref):
    """max |y - ref| per row relative to the row's max |ref|, in long double."""
    ref = np.asarray(ref, np.longdouble)
    peak = np.abs(ref).max(axis=1)
    return (np.abs(np.asarray(y, np.longdouble) - ref).max(axis=1) / np.where(peak > 0, peak, 1)).astype(np.float64)


def bar(y64, yld):
    """Per output row max(64 e_seq, 1e-13), e_seq the distance of the float64 sequential filter from the long double one."""
    return np.maximum(64 * distance(y64, yld), 1e-13)


def decaying_noise(rows, T, seed, rt=0.25, fs=48000, dtype=np.float64):
    """Gaussian noise under an exponential decay of 60 dB in rt seconds."""
    rng = np.random.default_rng(seed)
    env = 10.0 ** (-3.0 * np.arange(T) / (rt * fs))
    return (rng.standard_normal((rows, T)) * env).astype(dtype)


@functools.lru_cache(maxsize=None)
def cached(name, *args):
    """The references of one named test input, made once per process: (x, sos, fan, y_longdouble, y_float64)."""
    x, sos, fan = INPUTS[name](*args)
    return x, sos, fan, sequential(x, sos, fan, np.longdouble), sequential(x, sos, fan, np.float64)


INPUTS = {}


def impulse_response(sos, n):
    """h[0 .. n) of one cascade [K, 6] in closed form, long double: h[m] = c0 [m = 0] + sum_i r_i p_i^m over its 2K distinct poles."""
    s = normalise(sos)[0].astype(np.longdouble)
    cl = np.clongdouble
    poles = []
    for b0, b1, b2, _, a1, a2 in s:
        d = np.sqrt((a1 * a1 - 4 * a2).astype(cl))
        poles += [(-a1 + d) / 2, (-a1 - d) / 2]
    poles = np.array(poles, cl)

    def H_without(u, skip):                                      # prod B_k(u) / prod_{j != skip} (1 - p_j u), u = z^-1
        num = np.prod([b0 + b1 * u + b2 * u * u for b0, b1, b2, *_ in s])
        den = np.prod([1 - p * u for j, p in enumerate(poles) if j != skip])
        return num / den

    res = np.array([H_without(1 / p, i) for i, p in enumerate(poles)], cl)
    c0 = np.prod([b2 / a2 for _, _, b2, _, _, a2 in s])            # the value at u -> infinity
    m = np.arange(n)
    h = np.zeros(n, cl)
    for r, p in zip(res, poles):
        h += r * np.exp(m * np.log(p))
    h[0] += c0
    return h.real


# ---- the inputs that the CPU and the GPU tests share -----------------------------------------------------------------------------

SEAM_CELL = 32
SEAM_LENGTHS = (31, 32, 33, 64 * 32 - 1, 64 * 32, 64 * 32 + 1)
LONG_LENGTH = 64 * 64 * 32 + 3                                   # three runs of level two at cell 32
SEAM_KINDS = ("bank6", "one", "perrow", "mod3")


def _seam(T, kind):
    from friture_amd import sosfilter
    seed = T * 7 + SEAM_KINDS.index(kind)
    if kind == "bank6":                                          # 3 float64 rows into six octave bands, K = 3
        return decaying_noise(3, T, seed, rt=1.0), sosfilter.band_sos("octave", 48000, 3)[1], True
    if kind == "one":                                            # 65 float32 rows through one filter, K = 1
        return decaying_noise(65, T, seed, dtype=np.float32), sosfilter.butter_band_sos(500.0, 2000.0, 48000, 1), False
    if kind == "perrow":                                         # one filter per row, K = 8
        sos = np.stack([sosfilter.butter_band_sos(f / 2 ** 0.5, f * 2 ** 0.5, 48000, 8) for f in (250.0, 1000.0, 4000.0)])
        return decaying_noise(3, T, seed), sos, False
    thirds = sosfilter.band_sos("third", 48000, 3)[1]            # "mod3": 7 float32 rows, row r through filter r % 3
    return decaying_noise(7, T, seed, dtype=np.float32), thirds[[0, 7, 15]], False


def _bank(bands):
    from friture_amd import sosfilter
    return decaying_noise(2, 1 << 14, 11), sosfilter.band_sos(bands, 48000, 3)[1], True


INPUTS.update(seam=_seam, bank=_bank)


# ---- the edge inputs: every section count, cell size, walk length and bank width (test_sos_edges_cpu.py / _gpu.py) ----------------

EDGE_CELL = 32
SECTION_COUNTS = tuple(range(1, 9))
SECTIONS_LENGTH = 64 * 32 + 33                                   # two runs at cell 32: one step of level two, from U_0 = 0
THREE_RUNS_LENGTH = 2 * 64 * 32 + 33                             # three runs: the second step multiplies M^64 by a U that is not 0
WALK_CENTRE = 16.0                                               # an octave whose state outlives a run of 2048 samples: M^64 has entries of 85
CELLS = (64, 128, 256, 512, 1024)
WALK_RUNS = (17, 18, 33, 34)                                     # 16, 17, 32 and 33 steps of level two: whole rounds of 16 and one more
WIDTHS = (1, 4, 64)
STIFF_KINDS = ("band20", "A", "C")
STIFF_CELLS = (32, 256)
CENTRES = {1: (1000.0,), 3: (125.0, 1000.0, 8000.0), 4: (125.0, 500.0, 2000.0, 8000.0), 5: (125.0, 500.0, 1000.0, 4000.0, 8000.0),
           64: tuple(np.geomspace(100.0, 10000.0, 64).tolist())}


def sections(K, centre=1000.0):
    """The Butterworth band-pass of order K (K sections) one octave wide around `centre` at 48 kHz: [K, 6]."""
    from friture_amd import sosfilter
    return sosfilter.butter_band_sos(centre / 2 ** 0.5, centre * 2 ** 0.5, 48000, K)


def bank(F, K):
    """F such filters on the centres CENTRES[F]: [F, K, 6]."""
    return np.stack([sections(K, f) for f in CENTRES[F]])


def run_edge_length(cell):
    """65 cells and 17 samples: one run seam, one step of level two, a partial last cell."""
    return 65 * cell + 17


def walk_length(nr):
    """nr runs at cell 32, the last one of five samples: nr - 1 steps of level two."""
    return (nr - 1) * 64 * EDGE_CELL + 5


def _sections(K, mode):
    seed = 100 + 2 * K + (mode == "bank")
    if mode == "bank":                                           # 2 rows into five bands: the second filter group has three idle waves
        return decaying_noise(2, SECTIONS_LENGTH, seed), bank(5, K), True
    return decaying_noise(3, SECTIONS_LENGTH, seed), bank(5, K)[[0, 3]], False       # row r through filter r % 2


def _three_runs(K):
    return decaying_noise(1, THREE_RUNS_LENGTH, 150 + K), bank(5, K), True


def _cells(cell):
    return decaying_noise(1, run_edge_length(cell), 200 + cell), bank(3, 3), True


def _walk(nr):
    return decaying_noise(1, walk_length(nr), 300 + nr), sections(1, WALK_CENTRE)[None], False


def _width(F):
    return decaying_noise(1, 2 * EDGE_CELL + 1, 400 + F), bank(F, 1), True


def stiff_sos(kind):
    """The 20 Hz third-octave of order 4, the A weighting (K = 3) and the C weighting (K = 2), both weightings with a double real
    pole at 20.6 Hz: [K, 6]."""
    from friture_amd import sosfilter, soundlevel
    return sosfilter.butter_band_sos(17.8, 22.4, 48000, 4) if kind == "band20" else soundlevel.weighting_sos(kind)


def _stiff(kind, cell):
    x = decaying_noise(2, run_edge_length(cell), 500 + cell + STIFF_KINDS.index(kind), rt=2.0)
    return x, stiff_sos(kind)[None], False


INPUTS.update(sections=_sections, three_runs=_three_runs, cells=_cells, walk=_walk, width=_width, stiff=_stiff)

# (name, args, cell) of every edge input that has a long double reference
EDGE_INPUTS = ([("sections", (K, mode), EDGE_CELL) for K in SECTION_COUNTS for mode in ("bank", "row")]
               + [("three_runs", (K,), EDGE_CELL) for K in SECTION_COUNTS]
               + [("cells", (cell,), cell) for cell in CELLS] + [("walk", (nr,), EDGE_CELL) for nr in WALK_RUNS]
               + [("width", (F,), EDGE_CELL) for F in WIDTHS] + [("stiff", (kind, cell), cell) for kind in STIFF_KINDS for cell in STIFF_CELLS])


# ---- what the GPU test files share -------------------------------------------------------------------------------------------------

def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def same_bits(a, b):
    a, b = host(a), host(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_state(a, b):
    assert a.rows == b.rows and a.n == b.n and a.settings == b.settings
    same_bits(a.data, b.data)


def led(x, lead):
    """x as a view that starts `lead` elements into a buffer."""
    buf = np.zeros(lead + x.size, x.dtype)
    buf[lead:] = x.reshape(-1)
    return buf[lead:].reshape(x.shape)


def run_pieces(batch, x, cuts, fan):
    state, parts = None, []
    for a, b in zip([0] + list(cuts), list(cuts) + [x.shape[-1]]):
        r = batch.run(x[..., a:b], fan=fan, state=state)
        state = r.state
        parts.append(host(r.y))
    return np.concatenate(parts, axis=-1), state


def parity(y, name, args, label):
    """Prints and asserts the distance of y from the long double reference of the named input; returns the worst distance / bar."""
    x, sos, fan, yld, y64 = cached(name, *args)
    y = host(y).astype(np.float64).reshape(yld.shape)
    e, d, b = distance(y64, yld), distance(y, yld), bar(y64, yld)
    print(f"{label}: e_seq {e.max():.2e}, device {d.max():.2e}, largest device / e_seq {(d / np.maximum(e, 1e-300)).max():.1f}, "
          f"bar {b.min():.2e} .. {b.max():.2e}, worst device / bar {(d / b).max():.3f}")
    assert np.all(d <= b)
    return float((d / b).max())
