"""What the DecayBatch tests share: the numpy restatement of X3 (include/friture_hip.h, steps 1 to 9) in float64 or
np.longdouble, seeded responses, the gap condition on the reference and the two distances."""
import functools
import math

import numpy as np

RANGES = ((0.0, -10.0), (-5.0, -15.0), (-5.0, -25.0), (-5.0, -35.0))          # EDT, T10, T20, T30
FLOATS = ("edt", "t10", "t20", "t30", "c50", "c80", "d50", "ts", "level_db", "noise_db", "dynamic_range")
DB_FIELDS = ("c50", "c80", "level_db", "noise_db", "dynamic_range")            # bar: 1e-9 dB
REL_FIELDS = ("edt", "t10", "t20", "t30", "ts", "d50")                         # bar: 1e-8 relative (and r2)
INDICES = ("peak", "onset", "truncation")


def response(T, rt, seed, lead=0, floor_db=-70.0, fs=48000, dtype=np.float64):
    """A zero lead-in, then Gaussian noise times 10^(-3 t / rt) (t in seconds from the lead-in's end) plus a stationary noise
    floor at floor_db."""
    rng = np.random.default_rng(seed)
    n = T - lead
    t = np.arange(n) / fs
    x = np.zeros(T)
    x[lead:] = rng.standard_normal(n) * 10.0 ** (-3.0 * t / rt) + 10.0 ** (floor_db / 20.0) * rng.standard_normal(n)
    return x.astype(dtype)


def closed_form_row(T=8192, rt=0.0517, fs=48000, A=0.5):
    """x[t] = A r^t with alternating signs, r^2 = 10^(-6 / (rt fs)): E[t] = A^2 r^(2 t) (1 - r^(2 (T - t))) / (1 - r^2)."""
    r = 10.0 ** (-3.0 / (rt * fs))
    return A * r ** np.arange(T) * (-1.0) ** np.arange(T), r


def _dead(T, step):
    out = {k: math.nan for k in FLOATS}
    out.update({k: -1 for k in INDICES})
    out["r2"] = np.full(4, math.nan)
    out["curve"] = None if not step else np.full(-(-T // step), math.nan)
    out["gap_at"], out["gap_db"], out["gap_q"] = {}, math.inf, math.inf
    return out


def restate(x, fs=48000, block=480, onset_db=-20.0, noise_tail=0.1, margin_db=10.0, onset=None, truncate="auto", curve_step=0,
            real=np.float64):
    """One row by the text of X3, sums in `real`.  Besides the results: gap_at, per threshold the smallest distance in dB of the
    L[a - 1], L[a] or L[b - 1], L[b] around its crossing (of min L where it is not reached), gap_db, the smallest of them, and
    gap_q, the smallest relative distance of q[k] from the truncation threshold over the blocks that were tested."""
    x = np.asarray(x, np.float64)                                    # a float32 sample widens exactly
    T, W = len(x), int(block)
    if not np.all(np.isfinite(x)) or not np.any(x):
        return _dead(T, curve_step)
    ax = np.abs(x)
    p = int(np.argmax(ax))
    c = 10.0 ** (onset_db / 20.0)
    t0 = int(np.argmax(ax >= c * ax[p])) if onset is None else int(onset)      # the product is a float64 product: step 2
    e = x.astype(real) ** 2
    nb = T // W
    q = e[:nb * W].reshape(nb, W).sum(axis=1)
    nt = max(1, math.ceil(noise_tail * nb))
    N0 = q[nb - nt:].sum() / real(nt * W) if nb else real(0)
    gap_q = math.inf
    if truncate is None:
        t1 = T
    elif isinstance(truncate, str):
        bound = real(W) * N0 * real(10.0 ** (margin_db / 10.0))
        first = p // W + 1
        hit = np.nonzero(q[first:] <= bound)[0]
        last = first + int(hit[0]) if len(hit) else nb - 1
        t1 = last * W if len(hit) else T
        if last >= first and bound > 0:
            gap_q = float(np.min(np.abs(q[first:last + 1] - bound) / bound))
    else:
        t1 = int(truncate)
    if onset is not None and isinstance(truncate, str) and t1 <= t0:
        return _dead(T, curve_step)                                  # step 4: a given onset at or behind the automatic truncation
    assert 0 <= t0 < t1 <= T
    seg = e[t0:t1]
    E = np.cumsum(seg[::-1])[::-1]
    E0 = E[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = real(10) * np.log10(E / E0)
        out = {"peak": p, "onset": t0, "truncation": t1, "r2": np.full(4, math.nan)}
        gap_at = {}                                                  # threshold in dB -> the distance of the L around its crossing

        def note(level, *values):
            gap_at[level] = min([gap_at.get(level, math.inf), *(abs(float(v - level)) for v in values)])

        for i, (hi, lo) in enumerate(RANGES):
            name = ("edt", "t10", "t20", "t30")[i]
            out[name] = math.nan
            below_hi, below_lo = np.nonzero(L <= hi)[0], np.nonzero(L <= lo)[0]
            a = 0 if hi == 0.0 else (int(below_hi[0]) if len(below_hi) else None)
            if a is not None and hi != 0.0:
                note(hi, *L[max(a - 1, 0):a + 1])
            if not len(below_lo):
                note(lo, np.min(L))
                continue
            b = int(below_lo[0])
            note(lo, *L[max(b - 1, 0):b + 1])
            n = b - a
            if n < 2:
                continue
            k, Lr, n_ = np.arange(n).astype(real), L[a:b], real(n)
            Sk, Skk = n_ * (n_ - 1) / 2, (n_ - 1) * n_ * (2 * n_ - 1) / 6
            SL, SkL, SLL = Lr.sum(), (k * Lr).sum(), (Lr * Lr).sum()
            cov, vk, vl = n_ * SkL - Sk * SL, n_ * Skk - Sk * Sk, n_ * SLL - SL * SL
            out[name] = -60 / (cov / vk * real(fs))
            out["r2"][i] = cov * cov / (vk * vl)
        n50, n80 = math.floor(0.05 * fs + 0.5), math.floor(0.08 * fs + 0.5)
        E50 = E[n50] if t0 + n50 < t1 else real(0)
        E80 = E[n80] if t0 + n80 < t1 else real(0)
        out["c50"] = real(10) * np.log10((E0 - E50) / E50)
        out["c80"] = real(10) * np.log10((E0 - E80) / E80)
        out["d50"] = (E0 - E50) / E0
        out["ts"] = (np.arange(t1 - t0).astype(real) * seg).sum() / E0 / real(fs)
        out["level_db"] = real(10) * np.log10(E0)
        out["noise_db"] = real(10) * np.log10(N0)
        out["dynamic_range"] = math.nan if nb == 0 else (math.inf if N0 == 0 else real(10) * np.log10(q.max() / (real(W) * N0)))
    out["curve"] = None
    if curve_step:
        out["curve"] = np.full(-(-T // curve_step), math.nan, real)
        picked = L[::curve_step]
        out["curve"][:len(picked)] = picked
    out["gap_at"], out["gap_db"], out["gap_q"] = gap_at, min(gap_at.values()), gap_q
    return out


def restate_rows(rows, onset=None, truncate="auto", **settings):
    """restate() per row; onset and integer truncations are per row."""
    refs = []
    for i, x in enumerate(rows):
        t0 = None if onset is None else int(np.asarray(onset).reshape(-1)[i])
        t1 = truncate if truncate is None or isinstance(truncate, str) else int(np.asarray(truncate).reshape(-1)[i])
        refs.append(restate(x, onset=t0, truncate=t1, **settings))
    return refs


def check_gaps(refs, least=1e-6):
    """The condition on the inputs, asserted on the reference alone: no index decision sits within `least` of an edge."""
    for i, ref in enumerate(refs):
        assert ref["gap_db"] >= least, f"row {i}: a crossing lies {ref['gap_db']:.3g} dB from its threshold: pick another seed"
        assert ref["gap_q"] >= least, f"row {i}: a block sum lies {ref['gap_q']:.3g} (relative) from the truncation threshold: pick another seed"


def db_distance(got, want):
    """|got - want| in dB; equal infinities and a NaN on both sides are at distance 0, on one side at inf."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = np.where(same, 0, np.where(np.isnan(d), np.inf, d))
    return float(np.max(d)) if d.size else 0.0


def rel_distance(got, want):
    """|got - want| / |want|, with the same conventions."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d = np.where(same, 0, np.where(np.isnan(d), np.inf, d))
    return float(np.max(d)) if d.size else 0.0


def column(refs, name):
    return np.array([r[name] for r in refs], np.longdouble if name not in INDICES else np.int64)


def compare(res, refs, label, db_bar=1e-9, rel_bar=1e-8, curve_bar=1e-9):
    """Prints the distances of a DecayResult (numpy fields) from the reference rows, then asserts the bars."""
    worst_db = max(db_distance(getattr(res, f), column(refs, f)) for f in DB_FIELDS)
    worst_rel = max(rel_distance(getattr(res, f), column(refs, f)) for f in REL_FIELDS)
    worst_r2 = rel_distance(res.r2, np.array([r["r2"] for r in refs], np.longdouble))
    line = f"{label}: dB fields {worst_db:.3g} dB (bar {db_bar:g}), decay times / Ts / D50 {worst_rel:.3g}, r2 {worst_r2:.3g} relative (bar {rel_bar:g})"
    worst_curve = 0.0
    if res.curve is not None:
        worst_curve = max(db_distance(res.curve[i], r["curve"]) for i, r in enumerate(refs))
        line += f", curve {worst_curve:.3g} dB (bar {curve_bar:g})"
    print(line)
    for f in INDICES:
        assert np.array_equal(np.asarray(getattr(res, f)), column(refs, f)), f"{label}: {f} {getattr(res, f)} != {column(refs, f)}"
    assert worst_db <= db_bar and worst_rel <= rel_bar and worst_r2 <= rel_bar and worst_curve <= curve_bar, line


# ---- the cases of test_decay_edges_gpu.py, proven on the reference alone by test_decay_edges_cpu.py ------------------------------

TILE = 512                                  # decay.TILE
LEADS = (0, TILE - 1, TILE)
EDGE_T = 5 * TILE + 17
EDGE_BLOCKS = (8, 9, 63, 64, 65, 100, 512, 513, 1000, 2577, 65536)
EDGE_FS = (8000, 11025, 44100, 96000, 192000)
EDGE_SETTINGS = tuple([("onset_db", v) for v in (0.0, -6.0, -40.0, -60.0)] + [("noise_tail", v) for v in (0.001, 0.5, 1.0)] +
                      [("margin_db", v) for v in (0.0, 3.0, 25.0)])
def strided_shape(tile):
    """(T, the lead-ins) of the probes whose tile loops take a second trip in a launch of STRIDED_ROWS rows; sti_helpers.py's too."""
    return 66 * tile + 5, (0, tile - 1, tile, 3)


STRIDED_T, STRIDED_LEADS = strided_shape(TILE)
STRIDED_ROWS = 520


def tile_groups(rows, tiles):
    """csrc/rowfront.h's tile_groups restated: the workgroups of 4 wavefronts per row in a launch of `rows` rows of `tiles` tiles."""
    return min(-(-tiles // 4), max(16, -(-8192 // rows)))


def strided(live_tiles, rows):
    """Whether a wavefront of dk_totals / dk_scan (mtf_tiles) takes a second tile in a launch of `rows` rows (4 ceil(ntile / 4)
    wavefronts cover every tile, so the row's own tile count does not matter)."""
    return live_tiles > 4 * tile_groups(rows, live_tiles)


def _frozen(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def block_case(W, f32):
    """(x [rows, EDGE_T], the longdouble references at block=W, curve_step=7): the lead-ins 0, 511, 512 in turn, a decay of 60 dB
    over half of what the lead-in leaves; 3 float64 rows or 65 float32 rows."""
    rows = 65 if f32 else 3
    x = np.stack([response(EDGE_T, 0.5 * (EDGE_T - LEADS[i % 3]) / 48000, 1000 * W + (100 if f32 else 0) + i, LEADS[i % 3],
                           dtype=np.float32 if f32 else np.float64) for i in range(rows)])
    refs = restate_rows(x, block=W, curve_step=7, real=np.longdouble)
    check_gaps(refs)
    return _frozen(x), refs


def clarity_samples(fs):
    return math.floor(0.05 * fs + 0.5), math.floor(0.08 * fs + 0.5)


@functools.lru_cache(maxsize=None)
def fs_case(fs, f32):
    """(x [rows, 4 TILE + 100], the longdouble references at that fs, block=16, truncate="auto"): the lead-ins 37, 511, 512."""
    T, rows, leads = 4 * TILE + 100, 65 if f32 else 3, (37, TILE - 1, TILE)
    x = np.stack([response(T, 0.3 * T / fs, fs + (100 if f32 else 0) + i, leads[i % 3], fs=fs, dtype=np.float32 if f32 else np.float64)
                  for i in range(rows)])
    refs = restate_rows(x, fs=fs, block=16, real=np.longdouble)
    check_gaps(refs)
    return _frozen(x), refs


@functools.lru_cache(maxsize=None)
def fs_long_case(fs):
    """(x [3, T], the onsets, the longdouble references at truncate=None): one float64 row three times, long enough for n80, with
    the onset that step 2 finds, the next one that puts t0 + n50 on a multiple of TILE, and the next that puts it one before."""
    n50, n80 = clarity_samples(fs)
    T = n80 + 3 * TILE + 100
    row = response(T, 0.3 * T / fs, fs, 37, fs=fs)
    t0 = restate(row, fs=fs, block=16, truncate=None)["onset"]
    on_seam = t0 + (-(t0 + n50)) % TILE
    before_seam = t0 + (TILE - 1 - (t0 + n50)) % TILE
    onset = np.array([t0, on_seam, before_seam], np.int64)
    x = np.stack([row] * 3)
    refs = restate_rows(x, onset=onset, truncate=None, fs=fs, block=16, real=np.longdouble)
    check_gaps(refs)
    return _frozen(x), _frozen(onset), refs


@functools.lru_cache(maxsize=None)
def setting_case(name, value, f32):
    """(x [3, EDGE_T], the longdouble references at block=16 and that one setting): a lead-in of 300; the seeds are 5, 15, 25
    for onset_db, 6, 16, 26 for noise_tail (at noise_tail = 1 seed 5 ends on a sample small enough to reach -35 dB) and 7, 17, 27
    for margin_db."""
    first = {"onset_db": 5, "noise_tail": 6, "margin_db": 7}[name]
    x = np.stack([response(EDGE_T, 0.5 * EDGE_T / 48000, first + 10 * i, 300, dtype=np.float32 if f32 else np.float64) for i in range(3)])
    refs = restate_rows(x, block=16, real=np.longdouble, **{name: value})
    check_gaps(refs)
    return _frozen(x), refs


@functools.lru_cache(maxsize=None)
def strided_case():
    """(the probes [4, 66 TILE + 5] float32, their longdouble references at block=16, truncate=None, curve_step=7): live spans
    of 67 and 66 tiles."""
    T = STRIDED_T
    x = np.stack([response(T, 0.8 * T / 48000, 9000 + i, lead, dtype=np.float32) for i, lead in enumerate(STRIDED_LEADS)])
    refs = restate_rows(x, block=16, truncate=None, curve_step=7, real=np.longdouble)
    check_gaps(refs)
    return _frozen(x), refs


def live_tiles(onset, truncation, tile=TILE):
    return (np.asarray(truncation) - 1) // tile - np.asarray(onset) // tile + 1


@functools.lru_cache(maxsize=None)
def live_span_case():
    """(x [6, STRIDED_T], onsets, truncations, references): probe rows with given onsets and truncations that leave exactly 64 and
    65 live tiles, starting in tile 0 and in tile 1, on a tile's first sample and inside it."""
    probes, _ = strided_case()
    pairs = [(1, TILE, 65 * TILE), (1, TILE, 65 * TILE + 1), (0, 0, 64 * TILE), (0, 0, 64 * TILE + 1), (3, 3, 64 * TILE - 5),
             (2, TILE + 7, 65 * TILE + 9)]
    x = np.stack([probes[i] for i, _, _ in pairs])
    onset, truncation = (np.array([p[k] for p in pairs], np.int64) for k in (1, 2))
    refs = restate_rows(x, onset=onset, truncate=truncation, block=16, curve_step=7, real=np.longdouble)
    check_gaps(refs)
    return _frozen(x), _frozen(onset), _frozen(truncation), refs


@functools.lru_cache(maxsize=None)
def dead_index_case():
    """(x [7, 2 TILE + 3] of one response, onsets, truncations, the good row's number, its reference): six rows whose given onset
    or truncation lies outside its range around one good row."""
    T = 2 * TILE + 3
    row = response(T, 0.5 * T / 48000, 4242)
    onset = np.array([-1, T, 5, 5, 5, 700, 700], np.int64)
    truncation = np.array([T, T, 0, T - 100, T + 1, 700, 100], np.int64)
    good = 3
    ref = restate(row, onset=5, truncate=T - 100, block=16, curve_step=7, real=np.longdouble)
    check_gaps([ref])
    return _frozen(np.stack([row] * 7)), _frozen(onset), _frozen(truncation), good, ref


@functools.lru_cache(maxsize=None)
def late_onset_case():
    """(x [5, EDGE_T], onsets, references at block=16, truncate="auto", curve_step=7): rows 1 and 3 are given an onset at and
    behind their automatic truncation and are dead; rows 0, 2 and 4 are given the onset that step 2 finds."""
    x = np.stack([response(EDGE_T, 0.5 * (EDGE_T - LEADS[i % 3]) / 48000, 777 + i, LEADS[i % 3]) for i in range(5)])
    found = restate_rows(x, block=16, real=np.longdouble)
    onset = np.array([r["onset"] for r in found], np.int64)
    onset[1], onset[3] = found[1]["truncation"], found[3]["truncation"] + 5
    refs = restate_rows(x, onset=onset, block=16, curve_step=7, real=np.longdouble)
    check_gaps([refs[i] for i in (0, 2, 4)])
    return _frozen(x), _frozen(onset), refs
