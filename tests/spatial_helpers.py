"""What the SpatialBatch tests share: the numpy restatement of X8 (include/friture_hip.h, steps 1 to 6) with sums in np.longdouble
(the sequential definition, not the device's order), seeded pairs, the gap conditions on the reference alone, and the distances
with their bars."""
import functools
import math

import numpy as np

TILE = 2048                                 # spatial.TILE
FLOATS = ("iacc", "tau", "cross_abs", "energy")
INDICES = ("lag_index", "peak", "onset")
ENERGY_BAR, IACF_BAR, C_BAR = 1e-10, 1e-9, 1e-10
HALO_RATIO = 4.0                            # Er' / Er at most, in every live window


def pair(T, seed, lead=0, weight=0.7, delay=5, rt=None, fs=48000, dtype=np.float64, direct=1.5):
    """[2, T]: a zero lead-in, then two rows of Gaussian noise times 10^(-3 t / rt) (t in seconds from the lead-in's end; by
    default rt is three times what the lead-in leaves, 20 dB of decay in all, so that a halo of 128 samples in front of a window
    never outweighs the window) that share a common component of `weight` (their own noise has 1 - weight); the
    common component reaches row 1 `delay` samples later than row 0.  The first sample behind the lead-in is the direct sound,
    `direct` in row 0 and 0.8 direct in row 1, so that the onset is the lead-in's end (direct=None: noise there too)."""
    rng = np.random.default_rng(seed)
    n, d = T - lead, abs(int(delay))
    assert n >= 1
    rt = 3.0 * n / fs if rt is None else rt
    env = 10.0 ** (-3.0 * (np.arange(n) / fs) / rt)
    common = rng.standard_normal(n + 2 * d)
    x = np.zeros((2, T))
    x[0, lead:] = env * (weight * common[d:d + n] + (1 - weight) * rng.standard_normal(n))
    x[1, lead:] = env * (weight * common[d - delay:d - delay + n] + (1 - weight) * rng.standard_normal(n))
    if direct is not None:
        x[:, lead] = direct, 0.8 * direct
    return x.astype(dtype)


def window_seconds(windows, fs=48000):
    """Windows in samples ((a, b), b = None or -1 for "to the end") as the seconds that SpatialBatch takes: k / fs rounds back to k."""
    out = tuple((a / fs, None if b is None or b < 0 else b / fs) for a, b in windows)
    for (a, b), (sa, sb) in zip(windows, out):
        assert math.floor(sa * fs + 0.5) == a and (sb is None or math.floor(sb * fs + 0.5) == b)
    return out


def _dead(W, M):
    return {"dead": True, "iacc": np.full(W, math.nan), "tau": np.full(W, math.nan), "cross_abs": np.full(W, math.nan),
            "energy": np.full((W, 2), math.nan), "lag_index": np.full(W, -1, np.int64), "peak": -1, "onset": -1,
            "iacf": np.full((W, 2 * M + 1), math.nan), "C": np.full((W, 2 * M + 1), math.nan), "halo_energy": np.full(W, math.nan),
            "gap_iacf": math.inf, "gap_onset": math.inf, "halo_ratio": 0.0}


def restate(x, fs=48000, max_lag=48, windows=((0, 3840), (3840, -1), (0, -1)), onset_db=-20.0, onset=None, stop=None, real=np.longdouble):
    """One pair x [2, T] by the text of X8, windows in samples, sums in `real`, every window on its own from its first sample to
    its last.  Besides the results: C [W, 2 M + 1], halo_energy [W] = Er' (the energy of r over [A - M, B + M)), halo_ratio = the
    largest Er' / Er of a live window, gap_iacf = the smallest lead of a live window's largest |IACF| over the other lags',
    gap_onset = the relative distance from the onset threshold of the sample that reaches it and of the largest before it."""
    x = np.asarray(x, np.float64)                                    # a float32 sample widens exactly
    T, M, W = x.shape[1], int(max_lag), len(windows)
    e = T if stop is None else int(stop)
    assert 1 <= e <= T
    l, r = x[0, :e], x[1, :e]
    if not (np.all(np.isfinite(l)) and np.all(np.isfinite(r))) or not (np.any(l) or np.any(r)):
        return _dead(W, M)
    ax = np.maximum(np.abs(l), np.abs(r))
    peak = int(np.argmax(ax))
    bound = 10.0 ** (onset_db / 20.0) * ax[peak]                     # a float64 product: step 3
    gap_onset = math.inf
    if onset is None:
        t0 = int(np.argmax(ax >= bound))
        before = float(np.max(ax[:t0])) if t0 else 0.0
        gap_onset = float(min((np.longdouble(ax[t0]) - bound) / bound, (bound - np.longdouble(before)) / bound))
    else:
        t0 = int(onset)
    assert 0 <= t0 < e
    lr = l.astype(real)
    rz = np.zeros(e + 2 * M, real)                                   # r[u] = rz[u + M], zero outside [0, e)
    rz[M:M + e] = r
    out = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in _dead(W, M).items()}
    out.update(dead=False, peak=peak, onset=t0, gap_onset=gap_onset)
    out["energy"], out["cross_abs"], out["C"] = np.zeros((W, 2), real), np.zeros(W, real), np.zeros((W, 2 * M + 1), real)
    out["iacc"], out["tau"], out["iacf"] = out["iacc"].astype(real), out["tau"].astype(real), out["iacf"].astype(real)
    out["halo_energy"] = np.zeros(W, real)
    for w, (a, b) in enumerate(windows):
        A, B = min(t0 + a, e), e if b is None or b < 0 else min(t0 + b, e)
        B = max(A, B)
        lw, rw = lr[A:B], rz[A + M:B + M]
        El, Er = np.dot(lw, lw), np.dot(rw, rw)
        out["energy"][w] = El, Er
        out["cross_abs"][w] = np.abs(lw * rw).sum() if B > A else 0
        for k in range(2 * M + 1):                                   # tau = k - M: r[t + tau] = rz[t + k]
            out["C"][w, k] = np.dot(lw, rz[A + k:B + k])
        halo = rz[A:B + 2 * M]
        out["halo_energy"][w] = np.dot(halo, halo)
        if El * Er == 0:
            continue
        f = out["C"][w] / np.sqrt(El * Er)
        mag = np.abs(f)
        k = int(np.argmax(mag))
        out["iacf"][w], out["iacc"][w], out["lag_index"][w], out["tau"][w] = f, mag[k], k, real(k - M) / real(fs)
        if M:
            out["gap_iacf"] = min(out["gap_iacf"], float(mag[k] - np.max(np.delete(mag, k))))
        out["halo_ratio"] = max(out["halo_ratio"], float(out["halo_energy"][w] / Er))
    return out


def restate_pairs(pairs, onset=None, stop=None, **settings):
    refs = []
    for i, x in enumerate(pairs):
        t0 = None if onset is None else int(np.asarray(onset).reshape(-1)[i])
        e = None if stop is None else int(np.asarray(stop).reshape(-1)[i])
        refs.append(restate(x, onset=t0, stop=e, **settings))
    return refs


def check_gaps(refs, least=1e-6):
    """The conditions on the inputs, asserted on the reference alone: no index decision sits within `least` of an edge, and no
    live window's halo carries more than HALO_RATIO times its own energy of r (the bar on IACF is derived for that)."""
    for i, ref in enumerate(refs):
        assert ref["gap_iacf"] >= least, f"pair {i}: the largest |IACF| leads by {ref['gap_iacf']:.3g}: pick another seed"
        assert ref["gap_onset"] >= least, f"pair {i}: the onset lies {ref['gap_onset']:.3g} (relative) from its threshold: pick another seed"
        assert ref["halo_ratio"] <= HALO_RATIO, f"pair {i}: Er' / Er = {ref['halo_ratio']:.3g}: pick another seed"


def column(refs, name):
    return np.array([r[name] for r in refs], np.int64 if name in INDICES else np.longdouble)


def abs_distance(got, want):
    """max |got - want|; a NaN on both sides is at distance 0, on one side at inf."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = np.where(both, 0, np.where(np.isnan(d), np.inf, d))
    return float(np.max(d)) if d.size else 0.0


def rel_distance(got, want):
    """max |got - want| / |want| with the same conventions; equal values (0 against 0) are at distance 0."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d = np.where(same, 0, np.where(np.isnan(d), np.inf, d))
    return float(np.max(d)) if d.size else 0.0


def compare(res, refs, label, fs=48000):
    """Prints the distances of a SpatialResult with numpy fields ([S, ..]) from the reference pairs, then asserts X8's bars:
    energy and cross_abs 1e-10 relative, iacc and iacf 1e-9 absolute, tau to the last bits, C = IACF sqrt(El Er) within
    1e-10 sqrt(El Er'), the indices equal."""
    d_energy = max(rel_distance(res.energy, column(refs, "energy")), rel_distance(res.cross_abs, column(refs, "cross_abs")))
    d_iacc, d_tau = abs_distance(res.iacc, column(refs, "iacc")), rel_distance(res.tau, column(refs, "tau"))
    line = f"{label}: energy / cross_abs {d_energy:.3g} relative (bar {ENERGY_BAR:g}), iacc {d_iacc:.3g} (bar {IACF_BAR:g}), tau {d_tau:.3g} relative"
    d_iacf = d_c = 0.0
    if res.iacf is not None:
        d_iacf = abs_distance(res.iacf, column(refs, "iacf"))
        El, Er = (np.asarray(res.energy[..., k], np.longdouble) for k in (0, 1))
        got_c = np.asarray(res.iacf, np.longdouble) * np.sqrt(El * Er)[..., None]
        scale = np.sqrt(column(refs, "energy")[..., 0] * column(refs, "halo_energy"))[..., None]
        live = ~np.isnan(column(refs, "iacf"))
        with np.errstate(invalid="ignore", divide="ignore"):
            d_c = float(np.max(np.where(live, np.abs(got_c - column(refs, "C")) / scale, 0), initial=0.0))
        line += f", iacf {d_iacf:.3g} (bar {IACF_BAR:g}), C {d_c:.3g} sqrt(El Er') (bar {C_BAR:g})"
    print(line)
    for f in INDICES:
        assert np.array_equal(np.asarray(getattr(res, f)), column(refs, f)), f"{label}: {f} {getattr(res, f)} != {column(refs, f)}"
    assert d_energy <= ENERGY_BAR and d_iacc <= IACF_BAR and d_iacf <= IACF_BAR and d_c <= C_BAR and d_tau <= 1e-14, line


# ---- the cases of test_spatial_gpu.py, proven on the reference alone by test_spatial_cpu.py ---------------------------------------

SEAM_T = (TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 5 * TILE + 17)
SEAM_LAGS = (0, 1, 48, 128)
LEADS = (0, TILE - 1, TILE)
ROOM = 1200                                 # a lead-in leaves at least this many samples (the lead-ins that do not fit are cut to T - ROOM)


def seam_windows(M):
    """Four windows in samples: (0, TILE + 5) starts at the onset (with no lead-in t0 is 0 or nearly, and the halo reaches below
    sample 0) and crosses a tile of its second segment; (150, end) ends at e (the halo reaches past the end) and overlaps it;
    (0, M - 1) is shorter than M where M allows (24 samples below M = 25: a window of a handful of samples of noise cannot keep Er'
    / Er under 4), at the onset so that half of its halo lies in the lead-in; (50 TILE, ..) is empty."""
    return ((0, TILE + 5), (150, -1), (0, M - 1 if M >= 25 else 24), (50 * TILE, 50 * TILE + 9))


def _frozen(x):
    x.setflags(write=False)
    return x


def seam_lead(i, T):
    return min(LEADS[i % 3], T - ROOM)


@functools.lru_cache(maxsize=None)
def seam_case(T, M, f32):
    """(x [pairs, 2, T], the longdouble references with seam_windows(M)): the lead-ins 0, TILE - 1, TILE in turn, inter-row delays
    -min(M, 5) .. min(M, 5) in turn; 3 float64 pairs or 65 float32 pairs."""
    pairs, d = 65 if f32 else 3, min(M, 5)
    x = np.stack([pair(T, 100000 * M + 10 * T + (5 if f32 else 0) + 1000003 * i, seam_lead(i, T), delay=(i % (2 * d + 1)) - d,
                       dtype=np.float32 if f32 else np.float64) for i in range(pairs)])
    refs = restate_pairs(x, max_lag=M, windows=seam_windows(M))
    check_gaps(refs)
    return _frozen(x), refs


def tile_groups(pairs, tiles):
    """csrc/rowfront.h's tile_groups restated for sp_corr, whose workgroups take one tile at a time: the workgroups per pair in a
    launch of `pairs` pairs that can have `tiles` tiles at the most."""
    return min(tiles, max(16, -(-8192 // pairs)))


def most_tiles(T):
    """frt_spatial_run's bound on the tiles of a pair of T samples."""
    return T // TILE + 8


SECOND_TRIP_PAIRS = 512                     # the fewest pairs at which tile_groups is down at its floor of 16
SECOND_TRIP_T = 16 * TILE + 1               # one window from the onset at sample 0 to the end: 17 tiles, the fewest above 16
SECOND_TRIP_LAG = 8


@functools.lru_cache(maxsize=None)
def second_trip_case():
    """(the probes [4, 2, 16 TILE + 1] float32 with no lead-in, their given onsets (0), the references with the one window (0,
    end)): 17 tiles per pair."""
    x = np.stack([pair(SECOND_TRIP_T, 31000 + i, 0, delay=i - 2, dtype=np.float32) for i in range(4)])
    onset = np.zeros(4, np.int64)
    refs = restate_pairs(x, onset=onset, max_lag=SECOND_TRIP_LAG, windows=((0, -1),))
    check_gaps(refs)
    return _frozen(x), _frozen(onset), refs
