"""rfft_rows, irfft_rows and DeconvolveBatch on the GPU against closed forms and the numpy restatement of X4 in np.longdouble
(tests/deconvolve_helpers.py), and against themselves for everything the definition says does not matter: the other rows of a
call, the slab size, a row stride, the input's dtype and kind, a shared reference given per row.

The bars: spectra within 1e-12 max |X_ref| (X1's bar; numpy's own float64 transform sits at 3e-16 .. 4.5e-16 from the
longdouble one at n = 2^13 .. 2^22), h within 1e-12 of the maximum of the longdouble restatement.  H = Y G spans the dynamic
range of 1 / X, where a bar relative to max |H| is one that numpy's own float64 misses (1.3e-12 for a noise reference at
n = 2^20, reg = 0): H is held per bin to what the spectral bar on X and Y allows (deconvolve_helpers.spectrum_bound), and
irfft_rows of the returned H must give the bits of h.  Every parity case
first asserts, on the reference alone, that numpy's float64 restatement stays within 1e-13 of the longdouble one: a case whose
division is so badly conditioned that float64 itself cannot hold that (a sweep reference with reg = 0) is no parity case.
Recovery of a known response through ConvolveBatch at reg = 0: 1e-9 max |h_true|, for a reference whose min P / max P >= 1e-7
(the conditioning bounds the amplification of the transform error by about 1.5e3).  Every parity test prints its distance
before it asserts.  Inputs and references are made once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import deconvolve_helpers as dh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import deconvolve
    return deconvolve


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def same_bits(a, b):
    a, b = host(a), host(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. closed forms at every size ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log2n", range(13, 25))
def test_unit_samples_and_a_bin_cosine_at_every_size(mod, log2n):
    """Every (N1, N2) pair: both wave-local plans, both workgroup plans, the 512 / 1024 boundary and the two-frame workgroup of
    N2 = 4096.  A unit sample at p transforms to exp(-2 pi i k p / n); a cosine on bin b to n / 2 at b and zeros elsewhere."""
    n = 1 << log2n
    k = np.arange(n // 2 + 1, dtype=np.int64)
    T = n - 37
    for p, dtype in (((n // 3) | 1, np.float32), (T - 1, np.float64)):
        x = np.zeros(T, dtype)
        x[p] = 1.0
        ref = np.exp(-2j * np.pi * (((k * p) % n) / n))
        got = mod.rfft_rows(x, n)
        d = dh.distance(got, ref)
        print(f"n 2^{log2n}, unit sample at {p}: {d:.2e}")
        assert got.shape == (n // 2 + 1,) and got.dtype == np.complex128 and d <= dh.SPEC_BAR
    back = mod.irfft_rows(ref, n, keep=T)
    d = float(np.abs(back - x).max())
    print(f"n 2^{log2n}, the unit sample back: {d:.2e}")
    assert back.shape == (T,) and back.dtype == np.float64 and d <= 1e-12
    b = n // 8 + 3
    x = np.cos(2 * np.pi * (((b * np.arange(n, dtype=np.int64)) % n) / n))
    ref = np.zeros(n // 2 + 1, complex)
    ref[b] = n / 2
    got = mod.rfft_rows(x, n)
    d = dh.distance(got, ref)
    print(f"n 2^{log2n}, cosine on bin {b}: {d:.2e}")
    assert d <= dh.SPEC_BAR
    d = float(np.abs(mod.irfft_rows(got, n) - x).max())
    print(f"n 2^{log2n}, the cosine back: {d:.2e}")
    assert d <= 1e-12


# ---- 2. noise against the longdouble transform ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noise_rows(log2n):
    x = dh.noise(log2n, 3, 1 << log2n)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("cut", ["whole", "odd", "one"])
@pytest.mark.parametrize("log2n", [13, 14, 20, 21])
def test_noise_against_the_longdouble_transform(mod, log2n, cut):
    """64 x 64, 64 x 128 (the first non-square), 512 x 1024 (wave-local beside workgroup), 1024 x 1024; T = n, T = n - 37 (odd:
    the last complex point holds one sample; given as float32), T = 1."""
    n = 1 << log2n
    T = {"whole": n, "odd": n - 37, "one": 1}[cut]
    x = noise_rows(log2n)[:, :T]
    if cut == "odd":
        x = x.astype(np.float32)
    got = mod.rfft_rows(x, n)
    ref = dh.rfft(x, n)
    d = max(dh.distance(got[r], ref[r]) for r in range(3))
    print(f"n 2^{log2n}, T {T}: {d:.2e}")
    assert got.shape == (3, n // 2 + 1) and d <= dh.SPEC_BAR


# ---- 3. round trip --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log2n, cuda", [(14, False), (20, True)])
def test_round_trip_and_keep(mod, log2n, cuda):
    import torch
    n = 1 << log2n
    x = noise_rows(log2n)[:2]
    xin = torch.from_numpy(x.copy()).cuda() if cuda else x
    spec = mod.rfft_rows(xin, n)
    back = mod.irfft_rows(spec, n)
    assert (type(back) is type(xin)) and tuple(back.shape) == (2, n)
    d = dh.distance(host(back), x)
    print(f"n 2^{log2n}: irfft_rows(rfft_rows(x)) {d:.2e}")
    assert d <= 1e-12
    for keep in (1, 4097, n - 1):
        part = mod.irfft_rows(spec, n, keep=keep)
        assert tuple(part.shape) == (2, keep)
        same_bits(part, host(back)[:, :keep].copy())
    same_bits(mod.rfft_rows(xin[0], n), host(spec)[0].copy())
    cube = mod.rfft_rows(xin.reshape(2, 1, n), n)
    assert tuple(cube.shape) == (2, 1, n // 2 + 1)
    same_bits(cube.reshape(2, -1), spec)


# ---- 4. deconvolution parity ----------------------------------------------------------------------------------------------------

def reg_of(name, n):
    return {"scalar": 1e-6, "band": dh.band_reg(n), "zero": 0.0}[name]


@pytest.mark.parametrize("kind, regname", [("sweep", "scalar"), ("sweep", "band"), ("noise", "scalar"), ("noise", "band"), ("noise", "zero")])
@pytest.mark.parametrize("log2n, rows", [(14, 5), (20, 2)])
def test_parity_with_the_longdouble_restatement(mod, log2n, rows, kind, regname):
    n = 1 << log2n
    x, y = dh.measurement(kind, n // 4, rows, n // 2 + 5, n)
    reg = reg_of(regname, n)
    ref_h, ref_H = dh.restate(x, y, n, reg)
    d = dh.distance(dh.restate(x, y, n, reg, real=np.float64)[0], ref_h)
    print(f"n 2^{log2n}, {kind}, reg {regname}: numpy float64 against longdouble {d:.2e}")
    assert d <= dh.REF_BAR
    res = mod.DeconvolveBatch(x, n=n, reg=reg).run(y, spectrum=True)
    d_h = dh.distance(res.h, ref_h)
    err, bound = np.abs(res.spectrum - ref_H).astype(np.float64), dh.spectrum_bound(x, y, n, reg)
    d_H = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"n 2^{log2n}, {kind}, reg {regname}: h {d_h:.2e}; H {dh.distance(res.spectrum, ref_H):.2e} of max |H|, {d_H:.2e} of its bound")
    assert res.h.shape == (rows, n) and res.spectrum.shape == (rows, n // 2 + 1) and res.spectrum.dtype == np.complex128
    assert d_h <= dh.H_BAR and d_H <= 1.0 and not err[bound == 0].any()
    same_bits(mod.irfft_rows(res.spectrum, n), res.h)             # h IS the inverse transform of the H that is returned


def test_a_zero_bin_gives_zero_not_a_division(mod):
    """x = [1, 0, -1, 0, ..] over all of n lives on bin n / 4 alone: with reg = 0 every other bin has the denominator 0, G = 0
    there, and h is the measured row's component at that bin; an all-zero reference gives h = 0."""
    n = 1 << 13
    x = np.tile([1.0, 0.0, -1.0, 0.0], n // 4)
    y = dh.noise(5, 2, n - 3)
    res = mod.DeconvolveBatch(x, n=n, reg=0.0).run(y, spectrum=True)
    assert np.all(np.isfinite(res.h)) and np.all(np.isfinite(res.spectrum.view(np.float64)))
    ref_H = np.zeros((2, n // 2 + 1), np.result_type(dh.LD, np.complex64))
    ref_H[:, n // 4] = dh.rfft(y, n)[:, n // 4] / (n // 2)
    d_h, d_H = dh.distance(res.h, dh.irfft(ref_H, n)), dh.distance(res.spectrum, ref_H)
    print(f"one live bin: h {d_h:.2e}, H {d_H:.2e}")
    assert d_h <= dh.H_BAR and d_H <= dh.H_BAR
    live = np.zeros(n // 2 + 1, bool)
    live[n // 4] = True
    assert not res.spectrum[:, ~live].any()
    res = mod.DeconvolveBatch(np.zeros(100), n=n, reg=0.0).run(y, spectrum=True)
    assert not res.h.any() and not res.spectrum.any()


# ---- 5. recovery of a response that ConvolveBatch applied -----------------------------------------------------------------------

def test_recovery_and_the_decay_of_a_view(mod):
    import torch
    from friture_amd import convolve, decay
    Lx, Lh, n = 1 << 15, 1 << 13, 1 << 17
    x = dh.noise(7, Lx)
    P = np.abs(np.fft.rfft(x, n)) ** 2
    print(f"min P / max P of the reference: {P.min() / P.max():.2e}")
    assert P.min() / P.max() >= 1e-7
    h_true = np.stack([dh.response(20 + r, Lh) for r in range(2)])
    y = convolve.ConvolveBatch(h_true).run(torch.from_numpy(np.stack([x, x])).cuda()).y
    assert y.is_cuda and tuple(y.shape) == (2, Lx + Lh - 1)
    res = mod.DeconvolveBatch(x, n=n, reg=0.0).run(y)
    assert res.h.is_cuda and tuple(res.h.shape) == (2, n) and res.spectrum is None
    d = dh.distance(host(res.h)[:, :Lh], h_true)
    print(f"recovered against the applied response: {d:.2e}")
    assert d <= 1e-9
    view = res.h[:, :Lh]
    assert not view.is_contiguous()
    a, b = decay.DecayBatch().run(view), decay.DecayBatch().run(view.contiguous())
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            same_bits(u, v)
    assert np.all(np.isfinite(host(a.t20)))


# ---- 6. harmonics ---------------------------------------------------------------------------------------------------------------

def test_harmonic_responses_sit_at_their_offsets(mod):
    L, n = 1 << 16, 1 << 17
    x = mod.exp_sweep(50.0, 5000.0, L, fade=960)
    y = x + 0.1 * x ** 2 + 0.05 * x ** 3
    h = mod.DeconvolveBatch(x, n=n, reg=1e-4).run(y).h
    assert h.shape == (n,) and int(np.argmax(np.abs(h[:100]))) == 0
    floor = float(np.abs(h[n - 3000:n - 2000]).max())
    for order, off in zip((2, 3), mod.harmonic_offsets(L, 50.0, 5000.0, orders=(2, 3))):
        centre = n - int(round(off))
        window = np.abs(h[centre - 200:centre + 201])
        at = centre - 200 + int(np.argmax(window))
        print(f"order {order}: expected {n - off:.1f}, found {at}, peak {window.max():.3e}, floor {floor:.3e}")
        assert abs(at - (n - off)) <= 8 and window.max() >= 100 * floor


# ---- 7. identities --------------------------------------------------------------------------------------------------------------

def test_what_does_not_matter_leaves_the_bits_alone(mod):
    import torch
    n, rows = 1 << 14, 5
    x, y = dh.measurement("sweep", n // 4, rows, n // 2 + 5, n)
    T = y.shape[1]
    db = mod.DeconvolveBatch(x, n=n, reg=1e-6)
    base = db.run(y, spectrum=True)

    def same(res, pick=slice(None)):
        same_bits(res.h, base.h[pick])
        same_bits(res.spectrum, base.spectrum[pick])

    same(db.run(y[2:3], spectrum=True), slice(2, 3))                              # a row alone
    same(db.run(y, spectrum=True, scratch_bytes=1))                                # one row per launch
    same(db.run(y, spectrum=True, scratch_bytes=3 * 2 * (n // 2 + 1) * 16))        # slabs of 3 and 2 rows
    wide = np.zeros((rows, T + 11))
    wide[:, 3:3 + T] = y
    same(db.run(wide[:, 3:3 + T], spectrum=True))                                  # a strided view, rows 8 bytes off a 16-byte grid
    same(db.run(torch.from_numpy(wide).cuda()[:, 3:3 + T], spectrum=True))         # the same on the device
    res = db.run(torch.from_numpy(y.copy()).cuda(), spectrum=True)                 # numpy against CUDA
    assert res.h.is_cuda and res.spectrum.is_cuda
    same(res)
    one = db.run(y[1], spectrum=True)                                              # [T] against [1, T]
    assert one.h.shape == (n,) and one.spectrum.shape == (n // 2 + 1,)
    same_bits(one.h, base.h[1])
    same_bits(one.spectrum, base.spectrum[1])
    same(mod.DeconvolveBatch(np.tile(x, (rows, 1)), n=n, reg=1e-6).run(y, spectrum=True))      # one reference, given per row
    same_bits(db.run(y, keep=1000).h, base.h[:, :1000].copy())
    y32 = y.astype(np.float32)
    a, b = db.run(y32, spectrum=True), db.run(y32.astype(np.float64), spectrum=True)          # float32 against the same values
    same_bits(a.h, b.h)
    same_bits(a.spectrum, b.spectrum)
    sick = y.copy()
    sick[1, 100] = np.nan
    res = db.run(sick, spectrum=True)
    same_bits(res.h[[0, 2, 3, 4]], base.h[[0, 2, 3, 4]])
    same_bits(res.spectrum[[0, 2, 3, 4]], base.spectrum[[0, 2, 3, 4]])


# ---- 8. the top size ------------------------------------------------------------------------------------------------------------

def test_the_top_size_against_an_analytic_answer(mod):
    """n = 2^24, 2048 x 4096: the reference is a unit sample at p1, the measured row 0.5 at p2 (float32), reg = 0: h is 0.5 at
    p2 - p1 and zero elsewhere."""
    import torch
    n, p1, p2 = 1 << 24, 12345, (1 << 23) + 54321
    x = np.zeros(p1 + 1)
    x[p1] = 1.0
    y = torch.zeros(p2 + 1, dtype=torch.float32, device="cuda")
    y[p2] = 0.5
    h = mod.DeconvolveBatch(x, n=n, reg=0.0).run(y).h
    assert h.is_cuda and tuple(h.shape) == (n,)
    peak = float(h[p2 - p1])
    h[p2 - p1] = 0.0
    rest = float(h.abs().max())
    print(f"n 2^24: h[p2 - p1] - 0.5 = {peak - 0.5:.2e}, max |h| elsewhere {rest:.2e}")
    assert abs(peak - 0.5) <= 1e-12 and rest <= 1e-12


# ---- the C entry point with a handle ----------------------------------------------------------------------------------------------

def test_run_rejects_bad_arguments_before_any_device_call(mod, hip):
    n = 1 << 13
    db = mod.DeconvolveBatch(np.ones((2, 8)), n=n)
    h = db._handle()
    vp = ctypes.c_void_p
    y, out = np.zeros((2, 64)), np.zeros((2, n))
    yp, op = vp(y.ctypes.data), vp(out.ctypes.data)
    # frt_deconvolve_run(h, y, y_dtype, rows, T, row_stride, keep, scratch_bytes, out, out_stride, spectrum)
    for args, word in (((None, 1, 2, 64, 64, n, 0, op, n, None), b"null buffer"), ((yp, 1, 2, 64, 64, n, 0, None, n, None), b"null buffer"),
                       ((yp, 2, 2, 64, 64, n, 0, op, n, None), b"y_dtype 2"), ((yp, 1, 0, 64, 64, n, 0, op, n, None), b"rows"),
                       ((yp, 1, 3, 64, 64, n, 0, op, n, None), b"2 references for 3 rows"), ((yp, 1, 2, 0, 64, n, 0, op, n, None), b"T 0"),
                       ((yp, 1, 2, n + 1, n + 1, n, 0, op, n, None), b"T 8193"), ((yp, 1, 2, 64, 64, 0, 0, op, n, None), b"keep 0"),
                       ((yp, 1, 2, 64, 64, n + 1, 0, op, n + 1, None), b"keep 8193"), ((yp, 1, 2, 64, 63, n, 0, op, n, None), b"bad stride"),
                       ((yp, 1, 2, 64, 64, n, 0, op, n - 1, None), b"bad stride"), ((yp, 1, 2, 64, 64, n, -1, op, n, None), b"scratch_bytes")):
        assert hip.frt_deconvolve_run(h.h, *args) == -1, args[1:]
        assert b"frt_deconvolve_run" in hip.frt_last_error() and word in hip.frt_last_error(), hip.frt_last_error()
