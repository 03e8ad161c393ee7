"""The host boundary of the recording entries, through ctypes against the C ABI: every array argument of frt_convolve_run,
frt_transfer_run, frt_loudness_run, frt_resample_run, frt_levels_run, frt_levels_subsample, frt_levels_history and
frt_irfft_rows may be a host array or a device array, in any mix (the Python wrappers only ever pass all-host or all-device).

Per entry, every placement of its array arguments (numpy array: host, CUDA tensor: device) at one tiny shape; outputs and the
new state must have the bits of the all-device run.  Input rows have ld > n, so the 2-D copies are exercised; stateful
entries run as two calls, so state_in is live in the second.  The all-device run is made once per entry and shared."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VP, DP = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
PAD = 7                                     # ld - n of every input and output row


@pytest.fixture(scope="module")
def lib(hip):
    from friture_amd import _lib
    return _lib.init()


def check(status):
    from friture_amd import _lib
    _lib.check(status)


def placements(k):
    return list(itertools.product((False, True), repeat=k))


def name(place):
    return "".join("d" if p else "h" for p in place)


def put(a, dev):
    """A copy of `a` as a host array or as a device tensor."""
    if not dev:
        return np.array(a)
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def empty(count, dtype, dev):
    """`count` elements of NaN: whatever a call does not write shows."""
    return put(np.full(count, np.nan, dtype), dev)


def addr(a, offset=0):
    """The address of element `offset` of a flat array (None stays None)."""
    if a is None:
        return None
    base = a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
    return VP(base + offset * (a.itemsize if isinstance(a, np.ndarray) else a.element_size()))


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def rows(flat, n_rows, ld, n):
    """Columns 0 .. n - 1 of `n_rows` rows at stride ld of a flat array, on the host."""
    return np.array(host(flat)[:n_rows * ld].reshape(n_rows, ld)[:, :n])


def same_bits(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


def samples(seed, shape, dtype):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def handle(create, destroy, *args):
    h = VP()
    check(create(ctypes.byref(h), *args))
    return h, lambda: destroy(h)


def table(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(DP)


# ---- frt_convolve_run: block 64, L = 200 (4 partitions), S = 2, T = 300 cut at 130, unflushed then flushed ------------------------

def convolve_run(lib, place):
    x_dev, sin_dev, sout_dev, y_dev = place
    S, B, L, T, cut = 2, 64, 200, 300, 130
    taps, taps_p = table(samples(1, (L,), np.float64))
    ld = T + PAD
    x = put(samples(2, (S * ld,), np.float32), x_dev)
    h, destroy = handle(lib.frt_convolve_create, lib.frt_convolve_destroy, taps_p, L, 1, B)
    try:
        out, state, emitted = [], None, 0
        for a, b, flush in ((0, cut, 0), (cut, T, 1)):
            n_out = (b + L - 1 if flush else b // B * B) - emitted
            n_state = 0 if flush else int(lib.frt_convolve_state_length(h, S, b))
            ldy = n_out + PAD
            y = empty(S * ldy, np.float64, y_dev)
            new = None if flush else empty(n_state, np.float64, sout_dev)
            old = None if state is None else put(state, sin_dev)
            got = ctypes.c_int64(0)
            check(lib.frt_convolve_run(h, addr(x, a), 0, S, b - a, ld, addr(old), addr(new), a, flush, 1 << 28, addr(y), 1, ldy,
                                       ctypes.byref(got)))
            assert got.value == n_out
            out.append(rows(y, S, ldy, n_out))
            state = None if flush else host(new)
            if not flush:
                out.append(state)
            emitted += n_out
        assert emitted == T + L - 1
        return out
    finally:
        destroy()


# ---- frt_transfer_run: N = 64, hop 32, average 2, delay 3, S = 2, T = 300 cut at 130 ------------------------------------------------

def transfer_run(lib, wide, place):
    from friture_amd import transfer, tables
    x_dev, sin_dev, sout_dev, out_dev = place
    S, N, hop, K, delay, T, cut = 2, 64, 32, 2, 3, 300, 130
    bins = N // 2 + 1
    ld = T + PAD
    pair = 2 * ld + (11 if wide else 0)
    win, win_p = table(tables.hann_symmetric(N))
    x = put(samples(3, (S * pair,), np.float64), x_dev)
    h, destroy = handle(lib.frt_transfer_create, lib.frt_transfer_destroy, N, hop, win_p, K, delay)
    try:
        out, state = [], None
        for a, b in ((0, cut), (cut, T)):
            E = transfer.frames_after(b, N, hop, delay) // K - transfer.frames_after(a, N, hop, delay) // K
            assert E > 0
            n_state = transfer.state_layout(S, N, hop, delay, b)[1]
            res, new = empty(7 * S * E * bins, np.float64, out_dev), empty(n_state, np.float64, sout_dev)
            old = None if state is None else put(state, sin_dev)
            got = ctypes.c_int64(0)
            check(lib.frt_transfer_run(h, addr(x, a), 1, S, b - a, ld, pair, addr(old), addr(new), a, 1 << 28, addr(res), ctypes.byref(got)))
            assert got.value == E
            state = host(new)
            out += [host(res), state]
        return out
    finally:
        destroy()


# ---- frt_loudness_run: stereo, S = 2, three sub-blocks plus a fraction, cut inside the second, flushed at the end, true peak on --------

def loudness_run(lib, place):
    from friture_amd import loudness
    x_dev, sin_dev, sout_dev, out_dev = place
    b = loudness.LoudnessBatch("stereo")
    S, P, R, SB = 2, 1, b.tp_zeros, loudness.SUB_BLOCK
    T, cut = 3 * SB + 1234, SB + 2000
    ld = T + PAD
    _, weights_p = table(b.weights)
    _, proto_p = table(b.prototype)
    x = put(0.1 * samples(4, (S * ld,), np.float32), x_dev)
    h, destroy = handle(lib.frt_loudness_create, lib.frt_loudness_destroy, S, 2, weights_p, R, proto_p)
    try:
        out, state, e0 = [], None, 0
        for lo, hi, flush in ((0, cut, 0), (cut, T, 1)):
            e1, k1 = loudness.emitted(hi, R, flush)
            n_state = loudness.state_layout(S, P, R, hi, e1)[1]
            n_res = (S * ((e1 - e0) + 2 * (k1 - e0)) + P * (loudness.n_blocks_400ms(e1) - loudness.n_blocks_400ms(e0)
                                                             + loudness.n_blocks_3s(e1) - loudness.n_blocks_3s(e0) + 1))
            res, new = empty(n_res, np.float64, out_dev), empty(n_state, np.float64, sout_dev)
            old = None if state is None else put(state, sin_dev)
            check(lib.frt_loudness_run(h, addr(x, lo), 0, hi - lo, ld, addr(old), addr(new), lo, flush, 1, addr(res)))
            state, e0 = host(new), e1
            out += [host(res), state]
        return out
    finally:
        destroy()


# ---- frt_resample_run: 44100 -> 48000, default design, S = 2, T = 500 cut at 200 ---------------------------------------------------------

def resample_run(lib, place):
    from friture_amd import resample
    x_dev, tin_dev, tout_dev, y_dev = place
    r = resample.Resampler(44100)
    S, T, cut = 2, 500, 200
    ld = T + PAD
    _, proto_p = table(r.prototype)
    x = put(samples(5, (S * ld,), np.float64), x_dev)
    h, destroy = handle(lib.frt_resample_create, lib.frt_resample_destroy, r.L, r.M, r.C, proto_p, S)
    try:
        out, tail, emitted = [], None, 0
        for a, b, flush in ((0, cut, False), (cut, T, True)):
            n_new = r.n_out(b, flush) - emitted
            assert n_new > 0
            ldy = n_new + PAD
            y, new = empty(S * ldy, np.float32, y_dev), empty(S * (r.K - 1), np.float64, tout_dev)
            old = None if tail is None else put(tail, tin_dev)
            check(lib.frt_resample_run(h, addr(x, a), 1, b - a, ld, addr(old), addr(new), a, emitted, n_new, addr(y), 0, ldy))
            tail = host(new)
            out += [rows(y, S, ldy, n_new), tail]
            emitted += n_new
        return out
    finally:
        destroy()


# ---- frt_levels_run, frt_levels_subsample, frt_levels_history: S = 2, n = 1000, chunk 512 ---------------------------------------------------

LEVELS_S, LEVELS_N, LEVELS_NDEC, LEVELS_HISTORY = 2, 1000, 3, 64


def levels_handle(lib):
    from friture_amd import levels, longlevels
    alpha, kernel, alpha2 = levels.meter_coefficients()
    kernel, kernel_p = table(kernel)
    _, g11 = table(longlevels.gauss(11, 2.))
    _, g41 = table(longlevels.gauss(10 * 4 + 1, 2. * 4))
    return handle(lib.frt_levels_create, lib.frt_levels_destroy, LEVELS_S, LEVELS_NDEC, LEVELS_HISTORY, kernel_p, kernel.shape[0], float(alpha),
                  float(alpha2), g11, g41, levels.PEAK_DECAY_RATE)


def levels_run(lib, place):
    from friture_amd import levels
    x_dev, m_dev, l_dev, hist_dev = place
    S, n, chunk = LEVELS_S, LEVELS_N, 512
    ld = n + PAD
    x = put(samples(6, (S * ld,), np.float32), x_dev)
    h, destroy = levels_handle(lib)
    try:
        nchunks, nb = -(-n // chunk), int(lib.frt_levels_blocks_for(h, n))
        assert nb > 0
        m, lo = empty(S * nchunks * levels.FIELDS, np.float64, m_dev), empty(S * nb * 2, np.float64, l_dev)
        got = ctypes.c_int64(0)
        check(lib.frt_levels_run(h, addr(x), 0, n, ld, chunk, addr(m), addr(lo), ctypes.byref(got)))
        assert got.value == nb
        hist = empty(S * LEVELS_HISTORY, np.float64, hist_dev)
        check(lib.frt_levels_history(h, LEVELS_HISTORY, addr(hist)))
        state = np.empty(lib.frt_levels_state_length(h), np.float64)
        check(lib.frt_levels_get_state(h, state.ctypes.data_as(DP)))
        return [host(m), host(lo), host(hist), state]
    finally:
        destroy()


def levels_subsample(lib, place):
    x_dev, out_dev = place
    S, n = LEVELS_S, LEVELS_N
    ld = n + PAD
    x = put(samples(7, (S * ld,), np.float64), x_dev)
    h, destroy = levels_handle(lib)
    try:
        m = int(lib.frt_levels_subsample_length(h, n))
        out = empty(S * m, np.float64, out_dev)
        got = ctypes.c_int64(0)
        check(lib.frt_levels_subsample(h, addr(x), 1, n, ld, addr(out), ctypes.byref(got)))
        assert got.value == m > 0
        return [host(out)]
    finally:
        destroy()


# ---- frt_irfft_rows: n = 64, 3 rows ----------------------------------------------------------------------------------------------------

def irfft_rows(lib, place):
    spec_dev, out_dev = place
    n, n_rows = 64, 3
    spec = put(samples(8, (n_rows * (n // 2 + 1) * 2,), np.float64), spec_dev)
    out = empty(n_rows * n, np.float64, out_dev)
    check(lib.frt_irfft_rows(addr(spec), n_rows, n, addr(out), None))
    return [host(out)]


ENTRIES = {"convolve": (convolve_run, 4), "transfer": (functools.partial(transfer_run, wide=False), 4),
           "transfer_wide": (functools.partial(transfer_run, wide=True), 4), "loudness": (loudness_run, 4), "resample": (resample_run, 4),
           "levels": (levels_run, 4), "subsample": (levels_subsample, 2), "irfft": (irfft_rows, 2)}
_all_device = {}


def all_device(lib, entry):
    if entry not in _all_device:
        run, k = ENTRIES[entry]
        out = run(lib, place=(True,) * k)
        for a in out:
            assert not np.any(np.isnan(a)), entry              # every element of every output was written
            a.setflags(write=False)
        _all_device[entry] = out
    return _all_device[entry]


@pytest.mark.parametrize("entry,place", [pytest.param(e, p, id=f"{e}-{name(p)}") for e, (_, k) in ENTRIES.items() for p in placements(k)])
def test_any_placement_gives_the_all_device_bits(lib, entry, place):
    same_bits(ENTRIES[entry][0](lib, place=place), all_device(lib, entry), (entry, name(place)))
