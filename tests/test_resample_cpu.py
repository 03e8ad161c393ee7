"""Resampler without a GPU: the design of the prototype, the numpy restatement the GPU tests compare with (checked three
independent ways), the output counts, the carried-state bookkeeping and the refusals."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import resample_helpers as H
from friture_amd.resample import MAX_COEFFICIENTS, Resampler, ResampleState, to_48k

ROOT = Path(__file__).resolve().parents[1]
FOUR = (44100, 96000, 32000, 8000)


@pytest.fixture(scope="module")
def designs():
    return {rate: Resampler(rate) for rate in H.RATES}


# ---- design ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", H.RATES)
def test_design_parameters(designs, rate):
    r = designs[rate]
    L, M, K = H.DESIGN[rate]
    assert (r.L, r.M, r.K, r.C, r.Q) == (L, M, K, 64 * max(L, M), max(L, M))
    assert r.prototype.dtype == np.float64 and r.prototype.shape == (2 * r.C + 1,)
    assert r.K == H.taps(r.L, r.C) and r.latency_in == r.C / r.L
    assert np.max(np.abs(r.prototype - r.prototype[::-1])) <= 1e-15                              # zero phase


@pytest.mark.parametrize("rate", H.RATES)
def test_prototype_response(designs, rate):
    """From a 2^22-point FFT: stop band (f >= 0.5 / Q) at or below -99 dB, pass-band ripple at most 2e-4 dB up to
    0.5 / Q - dw / (2 pi), every phase h[p::L] sums to 1 within 2e-6."""
    r = designs[rate]
    n = 1 << 22
    gain = np.abs(np.fft.rfft(r.prototype, n)) / r.L
    f = np.arange(n // 2 + 1) / n
    stop = 20 * np.log10(np.max(gain[f >= 0.5 / r.Q]))
    ripple = np.max(np.abs(20 * np.log10(gain[f <= 0.5 / r.Q - r.dw / (2 * np.pi)])))
    phases = max(abs(np.sum(r.prototype[p::r.L]) - 1) for p in range(r.L))
    print(f"{rate}: stop band {stop:.2f} dB, ripple {ripple:.2e} dB, phase sums within {phases:.2e}")
    assert stop <= -99.0
    assert ripple <= 2e-4
    assert phases <= 2e-6


# ---- the helper, three ways -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", FOUR)
def test_helper_against_convolution_of_the_zero_stuffed_signal(rate):
    r = Resampler(rate, zeros=8)
    x = np.random.default_rng(rate).standard_normal(300)
    u = np.zeros(len(x) * r.L)
    u[::r.L] = x
    full = np.convolve(u, r.prototype)
    n_out = r.n_out(len(x))
    ref = full[r.C + np.arange(n_out) * r.M]
    got = H.resample(x, r.L, r.M, r.C, r.prototype)
    assert got.shape == (n_out,)
    err = np.max(np.abs(got - ref))
    print(f"{rate}: helper - convolution {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("rate,zeros", [(rate, 8) for rate in FOUR] + [(rate, 64) for rate in H.RATES])
def test_helper_against_resample_poly(rate, zeros):
    from scipy.signal import resample_poly
    r = Resampler(rate, zeros=zeros)
    x = np.random.default_rng(rate + zeros).standard_normal((2, 500))
    ref = resample_poly(x, r.L, r.M, axis=-1, window=r.prototype / r.L)
    got = H.resample(x, r.L, r.M, r.C, r.prototype)
    assert got.shape == ref.shape == (2, r.n_out(500))
    err = np.max(np.abs(got - ref))
    print(f"{rate}, zeros {zeros}: helper - resample_poly {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("rate", H.RATES)
def test_helper_resamples_a_sine_to_the_analytic_sine(designs, rate):
    r = designs[rate]
    y = H.resample(H.sine(rate), r.L, r.M, r.C, r.prototype)
    err = H.sine_error(y, r.L, r.M, r.C)
    print(f"{rate}: helper - analytic sine {err:.2e}")
    assert err <= 2e-6


# ---- counts and carried state ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", FOUR)
def test_output_counts_against_a_brute_force_count(designs, rate):
    r = designs[rate]
    L, M, C = r.L, r.M, r.C
    for N in range(401):
        flushed = sum(1 for m in range(N * L // M + 2) if m * M < N * L)                       # outputs before the stream's end
        whole = sum(1 for m in range(N * L // M + 2) if (C + m * M) // L < N)                  # their last tap has arrived
        assert r.n_out(N, True) == H.count(N, L, M, C, True) == flushed, N
        assert r.n_out(N, False) == H.count(N, L, M, C, False) == whole, N
    assert r.n_out(0) == 0 and r.n_out(1) == -(-L // M)


@pytest.mark.parametrize("rate", FOUR)
def test_carried_state_bookkeeping_gives_the_whole_bit_for_bit(designs, rate):
    r = designs[rate]
    x = np.random.default_rng(7).standard_normal(H.CUTS[-1])
    whole = H.resample(x, r.L, r.M, r.C, r.prototype)
    out, slack = H.pieces(x, r.L, r.M, r.C, r.prototype, H.CUTS)
    assert slack is not None and slack >= 0, "kb reaches behind the carried tail"
    assert [len(o) for o in out] == list(np.diff([r.n_out(c, c == H.CUTS[-1]) for c in H.CUTS]))
    assert len(out[0]) == 0 and len(out[1]) == 0                                                  # shorter than the latency
    assert np.array_equal(np.concatenate(out), whole)


# ---- the design table of the GPU suite: which branches of the kernel each row reaches ----------------------------------------------

def constants():
    return H.kernel_constants((ROOT / "friture_amd" / "csrc" / "resample.hip").read_text())


@pytest.mark.parametrize("row", H.ROWS, ids=lambda row: "-".join(map(str, row[0])))
def test_design_row_reaches_its_class_at_the_kernels_constants(row):
    """launch_plan restates frt_resample_create with kPeriods, kTapBlock and kCap read from resample.hip.  A retuned constant
    that moves a row out of the branch it is in the table for fails here, naming the row and the entry: the row then needs
    another (L, M, C), the GPU tests must not go on passing on a shape that no longer gets there."""
    (L, M, C), want = row
    periods, tap_block, cap = constants()
    plan = H.launch_plan(L, M, C, periods, tap_block, cap)
    print(f"L {L}, M {M}, C {C}: {plan}")
    assert np.gcd(L, M) == 1 and L != M and plan["K"] == H.taps(L, C) >= 2 and L * plan["K"] <= MAX_COEFFICIENTS
    for key, value in want.items():
        assert plan[key] == value, (f"design row L {L}, M {M}, C {C} no longer reaches its class at kPeriods {periods}, kTapBlock "
                                    f"{tap_block}, kCap {cap}: {key} is {plan[key]}, the row is there for {value}")
    if not plan["direct"]:
        assert 2 * ((plan["span"] + 2) // 2 * 2) <= cap, "the two LDS copies overrun kCap"
    # the rows' input length: at least two whole tiles and a ragged third, whose last period is ragged too
    n = H.row_length(L, M, plan["np"], periods)
    outputs, tile = H.count(n, L, M, C, True), periods * plan["np"] * L
    assert outputs > 2 * tile and outputs % tile and (L == 1 or outputs % L), (n, outputs, tile)
    cuts = H.piece_cuts(n, plan["K"])
    assert cuts[0] == 0 and cuts[-1] == n and list(cuts) == sorted(cuts) and len(cuts) == 8


def test_the_classes_are_distinct_and_the_default_designs_reach_none_of_them():
    """What the table adds: at the defaults (zeros 64, 48 kHz out) every design has K >= 129, the direct one has L = 1 and the
    L = 1 designs read one LDS copy only."""
    periods, tap_block, cap = constants()
    for rate in H.RATES + (352800, 3840000):
        r = Resampler(rate)
        plan = H.launch_plan(r.L, r.M, r.C, periods, tap_block, cap)
        assert plan["K"] == r.K >= 129 and plan["blocks"] >= 16 and plan["passes"] <= 2
        assert not (plan["direct"] and r.L > 1) and (r.L > 1 or plan["parities"] <= {0})
    assert len({row[0] for row in H.ROWS}) == len(H.ROWS) == 13
    assert sum(1 for _, want in H.ROWS if want["direct"]) == 3


def as_fraction(v):
    """A long double (or Fraction) exactly."""
    from fractions import Fraction
    if isinstance(v, Fraction):
        return v
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - hi))


@pytest.mark.parametrize("L,M,C", ((3, 2, 12), (5, 3, 3), (7, 9, 20)))
def test_reference_and_bound(L, M, C):
    """The extended-precision reference equals the exact rational one far inside the bound; the promised chain
    acc = fma(c, x, acc), every fma rounded once (emulated in exact rationals), is within the bound; so is `gather`; a
    mirrored prototype, a dropped edge tap and a duplicated one are far outside."""
    from fractions import Fraction
    rng = np.random.default_rng(L * 100 + M)
    x, h, K = rng.standard_normal((2, 41)), rng.standard_normal(2 * C + 1), H.taps(L, C)
    m1 = H.count(41, L, M, C, True)
    ref, B = H.reference_and_bound(x, L, M, C, h, 0, m1)
    exact, Bx = H.reference_and_bound(x, L, M, C, h, 0, m1, exact=True)
    assert ref.shape == B.shape == exact.shape == (2, m1) and exact.dtype == object and isinstance(exact[0, 0], Fraction)
    if H.EXTENDED:
        assert ref.dtype == np.longdouble
        for a, b, bound in zip(ref.ravel(), exact.ravel(), Bx.ravel()):
            assert abs(as_fraction(a) - b) <= bound / 512               # 11 more bits, K + 1 roundings against K
    for a, b in zip(B.ravel(), Bx.ravel()):
        assert abs(as_fraction(a) - b) <= b / 2 ** 50               # 0 where every tap lies past the stream's end
    assert Bx[0, 0] == Fraction(K, 2 ** 53 - K) * sum(abs(Fraction(h[C - k * L])) * abs(Fraction(x[0, k])) for k in range(C // L + 1))

    def chain(hh, m, row, js):
        kb, acc = -(-(m * M - C) // L), 0.0
        for j in js:
            k, i = kb + j, C + m * M - (kb + j) * L
            if 0 <= i <= 2 * C and 0 <= k < x.shape[1]:
                acc = float(Fraction(hh[i]) * Fraction(x[row, k]) + Fraction(acc))      # one rounding: a fused multiply-add
        return acc

    def chains(hh, js):
        return np.array([[chain(hh, m, row, js) for m in range(m1)] for row in range(2)])

    for kw in ({}, {"exact": True}):
        r, b = (exact, Bx) if kw else (ref, B)
        assert H.excess(chains(h, range(K)), r, b, **kw) <= 1.0
        assert H.excess(chains(h, range(K - 1, -1, -1)), r, b, **kw) <= 1.0                 # any order of the K terms
        assert H.excess(H.gather(x, L, M, C, h, 0, m1), r, b, **kw) <= 1.0
        assert H.excess(chains(h[::-1], range(K)), r, b, **kw) > 1e6                        # mirrored
        assert H.excess(chains(h, range(K - 1)), r, b, **kw) > 1e6                          # the last tap dropped
        assert H.excess(chains(h, [0] + list(range(K))), r, b, **kw) > 1e6                  # the first tap twice
        y32 = chains(h, range(K)).astype(np.float32)
        assert H.excess(y32, r, b, **kw) <= 1.0
        assert H.excess(np.nextafter(np.nextafter(y32, np.float32(np.inf)), np.float32(np.inf)), r, b, **kw) > 1.0
    # a shifted stream: the same outputs from the samples behind k0 alone
    part, Bp = H.reference_and_bound(x[:, 11:], L, M, C, h, m1 - 5, m1, k0=11)
    full, _ = H.reference_and_bound(np.concatenate([np.zeros((2, 11)), x[:, 11:]], axis=1), L, M, C, h, m1 - 5, m1)
    assert np.array_equal(part, full) and part.shape == Bp.shape == (2, 5)
    assert H.reference_and_bound(x[:, :0], L, M, C, h, 0, 3)[0].shape == (2, 3)


# ---- refusals, without a device -------------------------------------------------------------------------------------------------

def test_refusals_are_raised_on_the_host():
    for bad in (0, -44100, 44100.0, "44100", None, True):
        with pytest.raises(ValueError):
            Resampler(bad)
        with pytest.raises(ValueError):
            Resampler(44100, bad)
    with pytest.raises(ValueError, match="rate_in == rate_out"):
        Resampler(48000)
    with pytest.raises(ValueError, match="rate_in == rate_out"):
        Resampler(44100, 44100)
    with pytest.raises(ValueError, match="coefficients"):
        Resampler(48001)
    r = Resampler(44100)
    assert r.L * r.K <= MAX_COEFFICIENTS
    x = np.zeros((3, 100))
    with pytest.raises(ValueError, match="another shape"):
        r.run(x, state=ResampleState(np.zeros((2, r.K - 1)), 0, 0))
    with pytest.raises(ValueError, match="another shape"):
        r.run(x, state=ResampleState(np.zeros((3, r.K)), 0, 0))
    with pytest.raises(ValueError, match="final"):
        r.run(x, state=ResampleState(np.zeros((3, r.K - 1)), 1000, r.n_out(1000, True)))
    with pytest.raises(ValueError):
        r.run(x, state=ResampleState(np.zeros((3, r.K - 1)), 1000, 5))
    with pytest.raises(ValueError):
        to_48k(x, 0)
    assert to_48k(x, 48000) is x


def test_c_refusals_come_before_any_device_call():
    from friture_amd import _lib
    lib = _lib.load()
    h, proto = ctypes.c_void_p(), (ctypes.c_double * 3)(0.25, 0.5, 0.25)
    for (L, M, C, S), word in (((1, 1, 64, 1), b"rate_in == rate_out"), ((0, 2, 64, 1), b"positive"), ((2, -1, 64, 1), b"positive"),
                               ((4, 2, 64, 1), b"share a factor"), ((48000, 48001, 64 * 48001, 1), b"coefficients"),
                               ((1, 2, 0, 1), b"C 0"), ((1, 2, 128, 0), b"streams"), ((1, 2, 128, 70000), b"streams")):
        rc = lib.frt_resample_create(ctypes.byref(h), L, M, C, proto, S)
        assert rc == -1 and h.value is None, (L, M, C, S)
        assert b"frt_resample_create" in lib.frt_last_error() and word in lib.frt_last_error(), lib.frt_last_error()
    assert lib.frt_resample_run(None, None, 0, 0, 0, None, None, 0, 0, 0, None, 0, 0) == -1
    assert b"frt_resample_run" in lib.frt_last_error()


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_resample_entry_points():
    from friture_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "friture_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(frt_resample_[a-z0-9_]+)\s*\(", text))
    want = {"frt_resample_create", "frt_resample_destroy", "frt_resample_set_stream", "frt_resample_run"}
    assert declared == want
    assert want <= set(_lib.SIGNATURES)
