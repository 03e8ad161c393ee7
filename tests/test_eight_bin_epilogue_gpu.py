"""The colour epilogue of the split-row N = 1024 instances evaluates EIGHT values per lane and frame: lane 0's descending slots
hold the bins its stores write (448, 384, 320 and the self-paired bin M/2 = 256), and the Nyquist bin's POWER waits in a register
for one colour evaluation per run (stft_wave.h).  Everything here is checked against oracle/dsp.py with the project's accounting
(dsp.image_parity: no pixel differs from the float64 epilogue of the kernel's own power outside an index edge, and every pixel
that differs from the reference's image is explained by the float32 transform's error in the power).

The input drives exactly those bins to index edges.  Per half-frame h the signal carries a (-1)^n component of amplitude a_h (the
Nyquist bin M) and a cos(pi n / 2) component of amplitude b_h (bin M/2).  The symmetric Hann window weighs both halves of a frame
alike, so frame f sees the effective amplitude (a_f + a_(f+1)) / 2: the amplitudes follow a_(f+1) = 2 A_f - a_f for the wanted
A_f.  A_f is placed so that the ORACLE's float64 index value of the bin is n_f + d_f, n_f an integer walking one index per frame,
d_f on the grid +-1e-5, +-3e-5, ..., +-9e-5 — inside EDGE = 1e-4, narrower than the zone the kernel decides in float64 (twice its
float32 error bound, 1.6e-4 for these tables), on both sides of the edge.  A few multiplicative corrections against the oracle
remove what the other components (tones on lane 0's other bins 64 j, noise) leak into the two bins.  The first frames are silent
(everything clamps to index 0), the last carry amplitude 64 (both bins clamp to 255).  The counts are asserted on the CPU; a grid
that misses them fails the module as mis-built."""
import numpy as np
import pytest

from oracle import dsp

N, HOP, M = 1024, 512, 512
F_ALL, C = 65, 2
SPEC_MIN, SPEC_MAX = -140.0, 0.0
EDGE = 1e-4
WALK = range(12, 52)                       # frames whose two bins are placed at an edge
SILENT_HALVES, LOUD_FROM = 10, 56          # half-frames [0, 10) are zero; half-frames 56.. carry amplitude 64
TOL32 = 1e-5


def index_value(p, w):
    return 255.0 * (10.0 * np.log10(p + 1e-30) + w - SPEC_MIN) / (SPEC_MAX - SPEC_MIN)


def power_for(q, w):
    return 10.0 ** ((q * (SPEC_MAX - SPEC_MIN) / 255.0 + SPEC_MIN - w) / 10.0) - 1e-30


def _targets():
    """wanted index values [C][2 bins: M, M/2][F_ALL] (NaN outside the walk)"""
    q = np.full((C, 2, F_ALL), np.nan)
    for f in WALK:
        d = ((f % 10) - 4.5) * 2e-5
        q[0, 0, f], q[0, 1, f] = 100 + f + d, 107 + f - d
        q[1, 0, f], q[1, 1, f] = 230 - f - d, 223 - f + d
    return q


def _signal(eff, rng_noise):
    """eff [C][2][F_ALL]: effective amplitudes of the walk frames -> float32 samples [C][T]"""
    T = N + HOP * (F_ALL - 1)
    n = np.arange(T)
    alt, quarter = np.where(n % 2 == 0, 1.0, -1.0), np.cos(np.pi * n / 2)
    tones = sum(0.01 * np.cos(2 * np.pi * (64 * j) * n / N + j) for j in (1, 2, 3, 5, 6, 7)) + 0.003
    x = np.zeros((C, T))
    for c in range(C):
        halves = np.zeros((2, F_ALL + 1))
        for b in range(2):
            a = halves[b]
            a[SILENT_HALVES:WALK[0] + 1] = eff[c, b, WALK[0]]
            for f in WALK:
                a[f + 1] = 2 * eff[c, b, f] - a[f]
            assert np.all(a[WALK[0]:WALK[-1] + 2] > 0)
            a[WALK[-1] + 2:LOUD_FROM] = 1.0
            a[LOUD_FROM:] = 64.0
        live = np.repeat((np.arange(F_ALL + 1) >= SILENT_HALVES).astype(float), HOP)
        x[c] = np.repeat(halves[0], HOP) * alt + np.repeat(halves[1], HOP) * quarter + live * (tones + rng_noise[c])
    return x.astype(np.float32)


def build_case():
    from friture_amd import tables
    weight = tables.weighting_db(tables.rfft_frequencies(N), 1e-50)[0]
    lut = dsp.colour_lut(dsp.cmrmap())
    qt = _targets()
    bins = (M, M // 2)
    pt = np.stack([np.stack([power_for(qt[c, b], weight[bins[b]]) for b in range(2)]) for c in range(C)])
    # first guess: |X[M]| / N = a / 2 and |X[M/2]| / N = b / 4 for a Hann window (sum N / 2)
    eff = np.stack([np.stack([np.sqrt(pt[c, 0]) * 2, np.sqrt(pt[c, 1]) * 4]) for c in range(C)])
    noise = 1e-3 * np.random.default_rng(7).standard_normal((C, N + HOP * (F_ALL - 1)))
    walk = list(WALK)
    for _ in range(8):
        x = _signal(eff, noise)
        for c in range(C):
            ref = dsp.stft_psd(x[c].astype(np.float64), N, HOP)
            for b in range(2):
                eff[c, b, walk] *= np.sqrt(pt[c, b, walk] / ref[walk, bins[b]])
    x = _signal(eff, noise)
    ref = np.stack([dsp.stft_psd(x[c].astype(np.float64), N, HOP) for c in range(C)])
    # ---- the input is what the docstring says, or the module is mis-built --------------------------------------------
    for b in range(2):
        q = index_value(ref[:, :, bins[b]], weight[bins[b]])
        dist = q - np.rint(q)
        inside = (np.abs(dist) < EDGE) & (q > 0.5) & (q < 254.5)
        counts = (int(inside.sum()), int((inside & (dist < 0)).sum()), int((inside & (dist > 0)).sum()), int((q <= 0).sum()), int((q >= 255).sum()))
        print(f"bin {bins[b]}: within {EDGE} of an edge {counts[0]} (below {counts[1]}, above {counts[2]}), clamped at 0: {counts[3]}, at 255: {counts[4]}")
        assert counts[0] >= 32 and counts[1] >= 8 and counts[2] >= 8 and counts[3] >= 8 and counts[4] >= 8, (
            f"mis-built input: bin {bins[b]} {counts}")
    return {"x": x, "ref": ref, "weight": weight, "lut": lut}


@pytest.fixture(scope="module")
def case():
    return build_case()


def test_input_reaches_the_edges(case):
    assert case["x"].dtype == np.float32 and case["ref"].shape == (C, F_ALL, M + 1)


def frames_of(x, first, count, n_fft=N, hop=HOP, origin_hop=HOP):
    s = first * origin_hop
    return np.ascontiguousarray(x[:, s:s + n_fft + hop * (count - 1)])


def run_engine(x, n_fft, hop, weight, lut, run=0, precision=32):
    """-> (split image [C, F, n_fft/2 + 1], packed image, split PSD, packed PSD) as numpy"""
    import torch

    from friture_amd import _lib
    from friture_amd.stft import StftEngine
    eng = StftEngine(n_fft, hop, x.shape[0], precision)
    eng.set_epilogue(weight, SPEC_MIN, SPEC_MAX, lut)
    eng.set_run_length(run)
    xd = torch.from_numpy(x.astype(np.float32 if precision == 32 else np.float64)).cuda()
    out = []
    for kind in (_lib.FRT_STFT_IMAGE, _lib.FRT_STFT_PSD):
        rows, nyq = eng.run_split(kind, xd)
        packed = eng.run(kind, xd)
        torch.cuda.synchronize()
        split = torch.cat([rows, nyq[..., None]], dim=-1).cpu().numpy()
        packed = packed.cpu().numpy()
        if kind == _lib.FRT_STFT_IMAGE:
            split, packed = split.view(np.uint32), packed.view(np.uint32)
        out += [split, packed]
    eng.close()
    return out[0], out[1], out[2], out[3]


def assert_parity(img, psd, ref, weight, lut):
    for c in range(img.shape[0]):
        rep = dsp.image_parity(img[c], psd[c], ref[c], weight, SPEC_MIN, SPEC_MAX, lut)
        print(rep)
        assert rep["epilogue_mismatch_outside_edge"] == 0, rep
        assert rep["mismatch_unaccounted"] == 0, rep


def assert_psd(psd, ref):
    psd = np.asarray(psd, np.float64)
    mx = np.max(ref, axis=-1)
    live = mx > 0
    assert np.all(psd[~live] == 0)
    err = np.max(np.abs(psd - ref), axis=-1)[live] / mx[live]
    print("PSD per-frame relative error", float(err.max()))
    assert err.max() <= TOL32


@pytest.mark.gpu
@pytest.mark.parametrize("first,count,run", [(30, 1, 0), (20, 16, 16), (20, 17, 16), (0, 65, 64), (0, 65, 0)])
def test_headline_split_image(hip, case, first, count, run):
    """F = 1, one whole run, one frame more than a run, and 65 frames with 64-frame runs (every lane of the Nyquist register and
    one frame beyond) and with the shape rule's run length; two channels."""
    x = frames_of(case["x"], first, count)
    ref = case["ref"][:, first:first + count]
    img, img_packed, psd, psd_packed = run_engine(x, N, HOP, case["weight"], case["lut"], run)
    assert img.shape == (C, count, M + 1)
    assert_parity(img, psd, ref, case["weight"], case["lut"])
    # the eight-value path (split rows) against the nine-value path (packed rows): pixel for pixel
    assert np.array_equal(img, img_packed)
    # PSD kind: split rows bit-identical to the packed rows, and within the bar of the oracle
    assert np.array_equal(psd, psd_packed)
    assert_psd(psd, ref)


@pytest.mark.gpu
def test_float64_instance_split_image(hip, case):
    """float64 instance, split rows, same input: pixel-exact outside 1e-9 of an edge (the bar of bench.py's configs1_f64_image)"""
    x = frames_of(case["x"], 0, F_ALL)
    img, img_packed, psd, psd_packed = run_engine(x, N, HOP, case["weight"], case["lut"], 64, precision=64)
    for c in range(C):
        rep = dsp.image_parity(img[c], case["ref"][c], None, case["weight"], SPEC_MIN, SPEC_MAX, case["lut"], edge=1e-9)
        print(rep)
        assert rep["epilogue_mismatch_outside_edge"] == 0, rep
    assert np.array_equal(img, img_packed)
    assert np.array_equal(psd, psd_packed)
    live = np.max(case["ref"], axis=-1) > 0
    assert np.max(np.max(np.abs(psd - case["ref"]), axis=-1)[live] / np.max(case["ref"], axis=-1)[live]) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop", [(512, 256), (1024, 256)])
def test_neighbouring_instances(hip, case, n_fft, hop):
    """N = 512 (two frames per wavefront: the nine-value path) and N = 1024 at hop N/4 (register window of two slots per hop)"""
    from friture_amd import tables
    count = 21
    x = frames_of(case["x"], 20, count, n_fft, hop)
    weight = tables.weighting_db(tables.rfft_frequencies(n_fft), 1e-50)[0]
    ref = np.stack([dsp.stft_psd(x[c].astype(np.float64), n_fft, hop) for c in range(C)])
    assert ref.shape[1] == count
    img, img_packed, psd, psd_packed = run_engine(x, n_fft, hop, weight, case["lut"], 8)
    assert_parity(img, psd, ref, weight, case["lut"])
    assert np.array_equal(img, img_packed)
    assert np.array_equal(psd, psd_packed)
    assert_psd(psd, ref)
