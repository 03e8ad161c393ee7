"""MtfBatch, sti_from_mtf and speech_transmission on the GPU against the numpy restatement of X5 in np.longdouble
(tests/sti_helpers.py), and against themselves for everything the definition says does not matter: the other rows of a call,
the slab size, a row stride, the input's dtype and kind.

The bar on m, derived for T <= 2^17.  S0 and the two parts of S_j are float64 sums of n <= 2^17 terms of magnitude at most
e[t]: each is within n 2^-53 sum e = 1.5e-11 S0 of exact in any order (the device's order, 64 per lane, 64 lanes, then tiles,
stays orders of magnitude inside that).  The phasor of a sample is a product of three table entries that are each rounded
once, 2^-53, and two rounded complex products: below 2e-15 per term.  |S_j| moves by at most sqrt(2) 1.5e-11 S0, the
division by S0 adds m 1.5e-11: below 4e-11 on m, so 1e-10 absolute.  energy = S0: 1e-10 relative.  The far positions (T = 2^20,
2^24) hold two samples: their sums have two terms and only the tables' accuracy shows, under the same bar.  The index: 10
log10(m / (1 - m)) / 30 has a derivative of at most 0.145 / (m (1 - m)) <= 4.9 inside the clip range (m in 0.0307 .. 0.9693),
the corrections are a handful of float64 operations, and sqrt(MTI_k MTI_{k+1}) has a derivative of at most 0.5 sqrt(1000)
= 16 once every MTI is 0 or at least 1e-3 (asserted on the reference): a float64 evaluation stays below 1e-13, the bar is 1e-9
on ti, mti and sti.  speech_transmission composes ConvolveBatch, whose own bar (1e-12 max |x| sum |h|) is about 1e-10 relative
on a band's energy: m within 1e-8, sti within 1e-7, as room_acoustics holds for the same composition.  Every parity test prints
its distances before it asserts.  Inputs and references are made once and shared."""
import ctypes
import functools
import math

import numpy as np
import pytest

import decay_helpers as dh
import sti_helpers as sh

pytestmark = pytest.mark.gpu

FS = 48000
TL = 4096                                   # sti.TILE
LANES = 64                                  # the seam inside a tile: samples 64 apart belong to one lane
FREQS = {1: (3.15,), 14: sh.MOD_FREQS, 16: sh.MOD_FREQS + (16.0, 20.0)}


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import sti
    assert sti.TILE == TL and hip.frt_mtf_tile() == TL
    return sti


def host(res):
    """A result tuple with numpy fields."""
    return type(res)(*[v.cpu().numpy() if hasattr(v, "cpu") else v for v in res])


def same_bits(a, b):
    a, b = host(a), host(b)
    for f in a._fields:
        u, v = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f


def pick(res, rows):
    res = host(res)
    return type(res)(*[v[rows] for v in res])


@functools.lru_cache(maxsize=None)
def seam_case(T, rows, f32, nf=14):
    """(x [rows, T], the longdouble reference) with the lead-ins 0, TL - 1, TL in turn (those that leave a sample) and decays that
    fall 60 dB over what the lead-in leaves."""
    leads = [lead for lead in (0, TL - 1, TL) if lead < T]
    x = np.stack([sh.response(T, max(T - leads[i % len(leads)], 8) / FS, 1000 * T + i, leads[i % len(leads)],
                              dtype=np.float32 if f32 else np.float64) for i in range(rows)])
    ref = sh.restate_mtf(x, FREQS[nf], FS, real=np.longdouble)
    x.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("T", [TL - 1, TL, TL + 1, 2 * TL + 3, 5 * TL + 17])
def test_parity_on_the_tile_seams(mod, T):
    """The sizes at which the tile seam can go wrong, with a lead-in that ends on it or one sample before it; a last tile of 4095,
    1, 3 or 17 samples leaves lanes and whole loads empty."""
    mb = mod.MtfBatch()
    x, ref = seam_case(T, 3, False)
    sh.compare(host(mb.run(x)), ref, f"T {T} float64 x 3")
    x, ref = seam_case(T, 65, True)
    sh.compare(host(mb.run(x)), ref, f"T {T} float32 x 65")
    assert np.all(np.isfinite(ref[0])) and ref[0].min() < 0.95


@pytest.mark.parametrize("nf", [1, 16])
def test_parity_at_other_frequency_counts(mod, nf):
    T = 2 * TL + 3
    x, ref = seam_case(T, 3, False, nf)
    res = host(mod.MtfBatch(FREQS[nf]).run(x))
    assert res.m.shape == (3, nf)
    sh.compare(res, ref, f"nf {nf}")
    x, ref = seam_case(T, 65, True, nf)
    sh.compare(host(mod.MtfBatch(FREQS[nf]).run(x)), ref, f"nf {nf} float32 x 65")


@functools.lru_cache(maxsize=None)
def interval_case():
    """One slowly decaying row, once per interval: one-sample intervals and intervals whose ends sit at and beside the lane and
    tile seams."""
    T = 2 * TL + 3
    ones = [0, 1, LANES - 1, LANES, LANES + 1, TL - 1, TL, TL + LANES, 2 * TL - 1, 2 * TL, T - 1]
    pairs = [(t, t + 1) for t in ones]
    pairs += [(0, LANES), (1, TL), (LANES, TL + 1), (LANES - 1, TL + LANES), (2 * LANES, 2 * TL), (TL - 1, TL + 1), (TL, T), (3, T - 3),
              (TL + 1, 2 * TL - 1), (LANES - 1, LANES + 1), (TL - LANES, TL + LANES + 1), (2 * TL, T), (0, T), (5, 5 + LANES)]
    start, stop = (np.array(v, np.int64) for v in zip(*pairs))
    x = np.repeat(sh.response(T, 4 * T / FS, 77)[None], len(pairs), axis=0)
    ref = sh.restate_mtf(x, start=start, stop=stop, real=np.longdouble)
    x.setflags(write=False)
    return x, start, stop, ref, len(ones)


def test_parity_of_intervals_on_the_seams(mod):
    import torch
    x, start, stop, ref, n_ones = interval_case()
    assert np.all(np.isfinite(ref[0])) and sh.distance(ref[0][:n_ones], 1.0) <= 1e-15          # one sample: m = 1
    mb = mod.MtfBatch()
    res = mb.run(x, start=start, stop=stop)
    sh.compare(host(res), ref, f"{len(start)} intervals")
    on_device = mb.run(torch.from_numpy(np.array(x)).cuda(), start=torch.from_numpy(start).cuda(), stop=torch.from_numpy(stop).cuda())
    same_bits(on_device, res)
    same_bits(mb.run(x, start=start), mb.run(x, start=start, stop=np.full(len(start), x.shape[1])))
    same_bits(mb.run(x, stop=stop), mb.run(x, start=np.zeros(len(start), np.int64), stop=stop))


@functools.lru_cache(maxsize=None)
def default_case(T, f32):
    x = np.stack([sh.response(T, rt * T / FS, 7 * T + i, lead, dtype=np.float32 if f32 else np.float64)
                  for i, (rt, lead) in enumerate([(0.2, 0), (0.35, 1234), (0.5, 4001)])])
    ref = sh.restate_mtf(x, real=np.longdouble)
    x.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("T,f32", [(1 << 14, False), (1 << 17, True)])
def test_parity_at_the_defaults(mod, T, f32):
    x, ref = default_case(T, f32)
    sh.compare(host(mod.MtfBatch().run(x)), ref, f"T {T} {'float32' if f32 else 'float64'}")


@pytest.mark.parametrize("T", [1 << 20, 1 << 24])
def test_far_positions_against_the_two_sample_form(mod, T):
    """Two unit samples, the second near the row's end: |1 + exp(-2 pi i F a / fs)| / 2 at every frequency, which only holds if the
    coarse table is right out there."""
    import torch
    first, second = 5, T - 2
    x = torch.zeros((1, T), dtype=torch.float32, device="cuda")
    x[0, first] = x[0, second] = 1.0
    res = host(mod.MtfBatch().run(x))
    want = np.array([sh.two_sample_m(F, second - first, 1.0, FS) for F in sh.MOD_FREQS])
    sh.compare(res, (want[None], np.array([2.0])), f"T 2^{T.bit_length() - 1}")
    assert want.min() < 0.9                                          # the form is not 1 everywhere


@functools.lru_cache(maxsize=None)
def index_case():
    """m [5, 7, 14] over both clip ranges and beyond them, levels that reach every piece of the masking function."""
    rng = np.random.default_rng(2011)
    m = rng.uniform(0.0, 1.0, (5, 7, 14))
    m[0, :, :4], m[1, :, -4:] = 0.01, 0.99
    m[2, 0, 0], m[2, 1, 1], m[2, 2, 2], m[2, 3, 3] = 1.2, -0.1, 1.0, 0.0
    m[4] = 0.02                                                      # every MTI exactly 0
    level = np.array(sh.SPEECH_DB["male"])[None] + np.array([48.0, 61.5, 65.0, 75.0, 112.0])[:, None]
    noise = rng.uniform(30.0, 64.0, (5, 7))
    m.setflags(write=False)
    return m, level, noise


INDEX_KW = {"plain": {}, "snr": {"snr_db": "noise7"}, "levels": {"level_db": "level"}, "levels and noise": {"level_db": "level", "noise_db": "noise"},
            "female": {"weights": "female"}, "stipa": {"scheme": "stipa"}, "female stipa with snr": {"weights": "female", "scheme": "stipa", "snr_db": "snr57"}}


@pytest.mark.parametrize("name", list(INDEX_KW))
def test_index_on_the_device(mod, name):
    import torch
    m, level, noise = index_case()
    values = {"level": level, "noise": noise, "noise7": noise[0] - 45.0, "snr57": noise - 45.0}
    kw = {k: values.get(v, v) if isinstance(v, str) and v in values else v for k, v in INDEX_KW[name].items()}
    ref = sh.restate_sti(m, real=np.longdouble, **kw)
    mti = ref["mti"].astype(np.float64)
    assert np.all((mti == 0) | (mti >= 1e-3)), "an MTI between 0 and 1e-3: pick another seed"
    assert all(min(abs(L - seam) for seam in (63.0, 67.0, 100.0)) >= 1e-6 for L in ref["levels"]), "a level on a seam of the masking function"
    if "level_db" in kw:
        assert min(ref["levels"]) < 63 < 64 < max(L for L in ref["levels"] if L < 67) and max(ref["levels"]) > 100
        assert any(67 < L < 100 for L in ref["levels"])
    res = host(mod.sti_from_mtf(m, **kw))
    d = {f: sh.distance(getattr(res, f), ref[f]) for f in ("ti", "mti", "sti")}
    print(name, d)
    assert res.sti.shape == (5,) and res.mti.shape == (5, 7) and res.ti.shape == (5, 7, 14)
    assert all(v <= 1e-9 for v in d.values()), d
    clipped = (ref["ti"] == 0) | (ref["ti"] == 1)
    assert clipped.any() and np.array_equal(res.ti[clipped], ref["ti"][clipped].astype(np.float64))
    assert (ref["ti"] == 0).any() and (ref["ti"] == 1).any() and res.sti[4] == 0.0
    on_device = mod.sti_from_mtf(torch.from_numpy(np.array(m)).cuda(), **kw)
    assert all(v.is_cuda for v in on_device)
    same_bits(on_device, res)
    same_bits(pick(res, 1), mod.sti_from_mtf(m[1], **{k: v[1] if getattr(v, "ndim", 0) == 2 else v for k, v in kw.items()}))


def test_index_of_a_nan_is_its_response_s_alone(mod):
    m, _, _ = index_case()
    hurt = np.array(m)
    hurt[1, 3, 5] = math.nan
    base, res = host(mod.sti_from_mtf(m)), host(mod.sti_from_mtf(hurt))
    assert np.isnan(res.sti[1]) and np.isnan(res.mti[1, 3]) and np.isnan(res.ti[1, 3, 5])
    keep = np.ones(5, bool)
    keep[1] = False
    same_bits(pick(res, keep), pick(base, keep))
    mask = np.ones((7, 14), bool)
    mask[:, 5] = False
    unused = host(mod.sti_from_mtf(hurt, scheme=mask))
    assert np.all(np.isfinite(unused.sti)) and np.isnan(unused.ti[1, 3, 5])
    clean = host(mod.sti_from_mtf(m, scheme=mask))
    assert unused.sti.tobytes() == clean.sti.tobytes() and unused.mti.tobytes() == clean.mti.tobytes()


def test_bit_identity(mod):
    import torch
    T = 5 * TL + 17
    x, _ = seam_case(T, 65, True)
    i = np.arange(65)
    kw = dict(start=(i * 37) % 600, stop=T - (i * 11) % 300)
    mb = mod.MtfBatch()
    whole = mb.run(x, **kw)
    assert np.all(np.isfinite(host(whole).m))
    same_bits(mb.run(x[17:18], start=kw["start"][17:18], stop=kw["stop"][17:18]), pick(whole, slice(17, 18)))   # a row alone
    same_bits(mb.run(x, scratch_bytes=1, **kw), whole)                                   # one row per launch
    same_bits(mb.run(x, scratch_bytes=7 * 6 * 29 * 8, **kw), whole)                      # seven rows per launch
    big = np.zeros((65, T + 11), np.float32)
    big[:, 5:5 + T] = x
    same_bits(mb.run(big[:, 5:5 + T], **kw), whole)                                      # a strided view, numpy
    same_bits(mb.run(torch.from_numpy(big).cuda()[:, 5:5 + T], **kw), whole)             # read in place on the device
    alone = mb.run(x[3], start=kw["start"][3], stop=kw["stop"][3])                       # [T] against [1, T]
    same_bits(pick(whole, 3), alone)
    assert host(alone).m.shape == (14,) and host(alone).energy.shape == ()
    same_bits(mb.run(x.astype(np.float64), **kw), whole)                                 # float32 against the same values as float64
    on_device = mb.run(torch.from_numpy(np.array(x)).cuda(), **kw)                       # numpy against a CUDA tensor
    assert all(v.is_cuda for v in on_device)
    same_bits(on_device, whole)
    same_bits(mod.MtfBatch().run(x, **kw), whole)                                        # another handle


def test_dead_rows_between_live_ones(mod):
    import torch
    T = 2 * TL + 3
    live, ref = seam_case(T, 4, False)
    x = np.zeros((8, T))
    x[0::2] = live
    x[3, 100], x[5, T - 1] = math.nan, math.inf
    x[3, :50], x[5, :50] = 0.25, -0.25
    x[7] = live[0]
    x[7, 5000:5100] = 0.0                                            # a live row with a silent interval
    start, stop = np.zeros(8, np.int64), np.full(8, T, np.int64)
    start[7], stop[7] = 5000, 5100
    mb = mod.MtfBatch()
    res = host(mb.run(x, start=start, stop=stop))
    assert np.all(np.isnan(res.m[1::2]))
    assert res.energy[1] == 0 and math.isnan(res.energy[3]) and res.energy[5] == math.inf and res.energy[7] == 0
    alone = mb.run(live)
    same_bits(pick(res, slice(0, None, 2)), alone)
    sh.compare(host(alone), ref, "the live rows")
    # intervals that are none, which only device arrays can carry to the kernel: those rows are dead, NaN in m and energy
    lo, hi = torch.zeros(8, dtype=torch.int64, device="cuda"), torch.full((8,), T, dtype=torch.int64, device="cuda")
    lo[1], hi[1] = 700, 700
    lo[3], hi[3] = 900, 100
    lo[5] = -1
    hi[7] = T + 1
    dead = host(mb.run(torch.from_numpy(live[[0, 0, 1, 1, 2, 2, 3, 3]]).cuda(), start=lo, stop=hi))
    assert np.all(np.isnan(dead.m[1::2])) and np.all(np.isnan(dead.energy[1::2]))
    same_bits(pick(dead, slice(0, None, 2)), alone)


@functools.lru_cache(maxsize=None)
def speech_case():
    from friture_amd import decay, sti
    T, rts = 1 << 15, (0.12, 0.3)
    ir = np.stack([dh.response(T, rt, 90 + s, lead=200 + 60 * s) for s, rt in enumerate(rts)])
    broadband = dh.restate_rows(ir, real=np.longdouble)
    dh.check_gaps(broadband)
    start, stop = (np.array([r[name] for r in broadband]) for name in ("onset", "truncation"))
    centres, edges = decay.band_edges(sti.octave_bands())
    m, share = [], []
    whole = sh.restate_mtf(ir, start=start, stop=stop, real=np.longdouble)[1]
    for f_lo, f_hi in edges:
        h = decay.band_filter(f_lo, f_hi, FS)
        M = (len(h) - 1) // 2
        y = np.stack([np.convolve(row, h)[M:M + T] for row in ir])
        band_m, band_energy = sh.restate_mtf(y, start=start, stop=stop, real=np.longdouble)
        m.append(band_m)
        share.append(band_energy / whole)
    ir.setflags(write=False)
    return ir, rts, start, stop, centres, np.stack(m, axis=1), np.stack(share, axis=1)


def test_speech_transmission_against_the_numpy_pipeline(mod):
    """Two decaying white-noise responses; the reference: the restated onset and truncation, band_filter, a float64 convolution, the
    restatement of m and of the index."""
    ir, rts, start, stop, centres, ref_m, share = speech_case()
    print("the bands' shares of the broadband energy:", share.astype(np.float64).min(axis=0))
    assert share.min() >= 1e-3
    ref = sh.restate_sti(ref_m, real=np.longdouble)
    assert np.all((ref["mti"] == 0) | (ref["mti"] >= 1e-3))
    res = host(mod.speech_transmission(ir))
    assert res.m.shape == (2, 7, 14) and res.ti.shape == (2, 7, 14) and res.mti.shape == (2, 7) and res.sti.shape == (2,)
    assert np.allclose(res.centres, centres, rtol=1e-12) and len(res.centres) == 7
    d_m, d_sti, d_mti = sh.distance(res.m, ref_m), sh.distance(res.sti, ref["sti"]), sh.distance(res.mti, ref["mti"])
    print(f"m {d_m:.3g} (bar 1e-08), sti {d_sti:.3g} (bar 1e-07), mti {d_mti:.3g}; STI {res.sti} at rt {rts}")
    assert d_m <= 1e-8 and d_sti <= 1e-7
    assert rts[0] < rts[1] and res.sti[0] > res.sti[1]              # the longer reverberation is the less intelligible
    halved = host(mod.speech_transmission(ir, snr_db=np.zeros(7)))
    same_bits(type(halved)(halved.centres, halved.sti, halved.mti, halved.ti, halved.m), type(res)(res.centres, *host(mod.sti_from_mtf(0.5 * res.m)), res.m))
    assert np.all(halved.sti < res.sti)
    one = host(mod.speech_transmission(ir[1]))
    assert one.sti.shape == () and one.m.shape == (7, 14)
    same_bits(one, pick(type(res)(np.broadcast_to(res.centres, (2, 7)), *res[1:]), 1))


def test_recovered_response_as_a_view(mod):
    """DeconvolveBatch recovers a response that ConvolveBatch applied; MtfBatch reads the view h[:, :Lh] in place and gives the
    bits it gives on a copy.  Against m of the applied response: a recovery error dx moves each of S_j and S0 by at most
    2 sum |x| max |dx|, so m by at most 4 max |dx| sum |x| / sum x^2."""
    import torch
    from friture_amd import convolve, deconvolve
    Lx, Lh, n = 1 << 15, 1 << 13, 1 << 17
    x = np.random.default_rng(7).standard_normal(Lx)
    h_true = np.stack([np.random.default_rng(20 + r).standard_normal(Lh) * np.exp(-np.arange(Lh) / (Lh / 8)) for r in range(2)])
    y = convolve.ConvolveBatch(h_true).run(torch.from_numpy(np.stack([x, x])).cuda()).y
    h = deconvolve.DeconvolveBatch(x, n=n, reg=0.0).run(y).h
    view = h[:, :Lh]
    assert view.is_cuda and not view.is_contiguous()
    mb = mod.MtfBatch()
    a, b = mb.run(view), mb.run(view.contiguous())
    same_bits(a, b)
    ref = sh.restate_mtf(h_true, real=np.longdouble)
    dx = float(np.abs(h.cpu().numpy()[:, :Lh] - h_true).max())
    bound = 4 * dx * float((np.abs(h_true).sum(axis=1) / (h_true ** 2).sum(axis=1)).max()) + 1e-10
    d = sh.distance(host(a).m, ref[0])
    print(f"recovery error {dx:.3g}; m of the recovered response against m of the applied one: {d:.3g} (bound {bound:.3g})")
    assert d <= bound <= 1e-7


def test_a_bad_argument_through_the_c_entry_points(mod):
    from friture_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    freqs = np.array(sh.MOD_FREQS)
    h = _lib.Handle("mtf", 48000.0, freqs.ctypes.data_as(dp), 14)
    x = np.ones((2, 64))
    m, energy = np.full((2, 14), 7.0), np.full(2, 7.0)
    vp = ctypes.c_void_p

    def run(rows=2, n=64, dtype=1, stride=64, start=None, stop=None, scratch=1 << 20, out=m):
        return h.lib.frt_mtf_run(h.h, vp(x.ctypes.data), dtype, rows, n, stride, start, stop, scratch, vp(out.ctypes.data) if out is not None else None,
                                 vp(energy.ctypes.data))

    ints = {name: np.array(v, np.int64) for name, v in (("neg", [0, -1]), ("late", [0, 64]), ("zero", [1, 0]), ("long", [64, 65]), ("ten", [10, 10]))}
    for kw in (dict(rows=0), dict(n=0), dict(n=(1 << 24) + 1), dict(dtype=2), dict(stride=63), dict(scratch=-1), dict(out=None),
               dict(start=vp(ints["neg"].ctypes.data)), dict(start=vp(ints["late"].ctypes.data)), dict(stop=vp(ints["zero"].ctypes.data)),
               dict(stop=vp(ints["long"].ctypes.data)), dict(start=vp(ints["ten"].ctypes.data), stop=vp(ints["ten"].ctypes.data))):
        assert run(**kw) == -1, kw
        assert b"frt_mtf_run" in h.lib.frt_last_error(), kw
    assert np.all(m == 7.0) and np.all(energy == 7.0)                # nothing was launched
    for args in ((48000.0, freqs.ctypes.data_as(dp), 17), (48000.0, freqs.ctypes.data_as(dp), 0), (10.0, freqs.ctypes.data_as(dp), 14),
                 (48000.0, np.array([1.0, 24000.0]).ctypes.data_as(dp), 2)):
        with pytest.raises(_lib.FritureHipError, match="frt_mtf_create"):
            _lib.Handle("mtf", *args)
    assert run() == 0 and not np.any(m == 7.0) and np.all(energy == 64.0)
    alpha, beta = (np.array(v) for v in mod.WEIGHTS["male"])
    mask, mm = np.ones((7, 14), np.uint8), np.full((1, 7, 14), 0.5)
    out = [np.full(s, 7.0) for s in ((1,), (1, 7), (1, 7, 14))]

    def index(S=1, nf=14, correction=0, a=None, b=None, mask=mask):
        return h.lib.frt_sti_run(vp(mm.ctypes.data), S, nf, correction, a, b, alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), vp(mask.ctypes.data),
                                 *[vp(o.ctypes.data) for o in out], None)

    levels = np.zeros((1, 7))
    empty = np.array(mask)
    empty[4] = 0
    for kw in (dict(S=0), dict(nf=0), dict(nf=17), dict(correction=3), dict(correction=1), dict(a=vp(levels.ctypes.data)),
               dict(correction=1, a=vp(levels.ctypes.data), b=vp(levels.ctypes.data)), dict(mask=empty)):
        assert index(**kw) == -1, kw
        assert b"frt_sti_run" in h.lib.frt_last_error(), kw
    assert all(np.all(o == 7.0) for o in out)
    assert index() == 0 and out[0][0] == pytest.approx(0.5, abs=1e-12)
