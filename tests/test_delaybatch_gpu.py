"""DelayEstimatorBatch on the GPU against the numpy replay of the widget (oracle/delaybatch.py), against
DelayEstimatorStream, and against itself (pieces, slabs, keep); frt_delaybatch_decimate alone against oracle.dsp.

The rounding bars were measured on an MI355X against the replay ("P5"): the next power of ten at or above ten
times the worst case seen, and never looser than the 1e-9 that the per-chunk chain holds against the same oracle
(tests/test_gcc_gpu.py, test_delay_estimator_chain_against_oracle)."""
import ctypes
import functools

import numpy as np
import pytest

from friture_amd.delay_estimator import DelayEstimatorBatch, DelayEstimatorStream, delay_schedule
from oracle import delaybatch as H
from oracle import dsp

pytestmark = pytest.mark.gpu

BAR = 1e-9           # read-outs, smoothed correlation and xcorr relative to the window's max |ref|: worst seen 1.9e-10; held at the per-chunk chain's 1e-9
DEC_BAR = 1e-10      # decimated samples relative to the row's max |ref|: worst seen 5.8e-12
STATE_BAR = 1e-9     # the decimators' end states relative to the stage's max |ref|: worst seen 9.9e-11
FIELDS = ("delay_ms", "distance_m", "extremum")


case = H.case        # (x [S, 2, T] of a dtype, the replay of every stream of it): shared with tests/test_gcc_gpu.py


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def worst_of(res, refs, what=""):
    """Compares a result of S streams with the replays; returns the worst relative error of the float fields."""
    worst = 0.0
    for s, r in enumerate(refs):
        W = len(r["gated"])
        assert np.array_equal(host(res.gated)[s], r["gated"]), f"{what} stream {s}: gate"
        doubt = [w for w in range(W) if H.doubtful(r, w)]
        assert len(doubt) <= 1
        sure = np.array([w not in doubt for w in range(W)])
        assert np.array_equal(host(res.correlation)[s][sure], r["correlation"][sure]), f"{what} stream {s}: correlation"
        assert np.array_equal(host(res.argmax)[s][sure], r["argmax"][sure]), f"{what} stream {s}: arg-max"
        for k in FIELDS:
            got, ref = host(getattr(res, k))[s], r[k]
            worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0), initial=0.0)))
        if res.xcorr is not None:
            for w in range(W):
                if not r["gated"][w]:
                    worst = max(worst, float(np.max(np.abs(host(res.xcorr)[s, w] - r["xcorr"][w])) / np.max(np.abs(r["xcorr"][w]))))
        if r["smoothed"] is not None:
            assert int(host(res.state.present)[s]) == 1
            worst = max(worst, float(np.max(np.abs(host(res.state.smoothed)[s] - r["smoothed"])) / np.max(np.abs(r["smoothed"]))))
    return worst


@pytest.mark.parametrize("kind", ["numpy", "cuda"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(H.CASES))
def test_batch_against_replay(hip, name, dtype, kind):
    import torch
    x, refs = case(name, dtype)
    delayrange, T = H.CASES[name][:2]
    xin = np.array(x) if kind == "numpy" else torch.from_numpy(np.array(x)).cuda()
    batch = DelayEstimatorBatch(delayrange)
    res = batch.run(xin, keep="all", with_xcorr=True)
    assert isinstance(res.delay_ms, np.ndarray) == (kind == "numpy") and isinstance(res.state.smoothed, np.ndarray) == (kind == "numpy")
    assert len(res.window_end) == {"r0.1": 13, "r0.5": 5, "r1.0": 5, "r2.0": 5}[name]
    assert np.array_equal(res.window_end, refs[0]["window_end"]) and np.array_equal(res.refresh_chunk, np.unique(refs[0]["window_chunk"]))
    worst = worst_of(res, refs, name)
    for s, r in enumerate(refs):                                     # what the widget shows after the chunks that completed a window
        rows = r["shown"][res.refresh_chunk]
        for k, column in enumerate(("shown_delay_ms", "shown_distance_m", "shown_extremum")):
            got = host(getattr(res, column))[s]
            worst = max(worst, float(np.max(np.abs(got - rows[:, k]) / np.maximum(np.abs(rows[:, k]), 1.0))))
    print(f"{name} {np.dtype(dtype).name} {kind}: worst {worst:.3e} (bar {BAR})")
    assert worst <= BAR


def run_decimate(hip, x, zi, n_stages=2, origin=0):
    """frt_delaybatch_decimate on a CUDA tensor x [C, n] (a strided row view is read in place) -> (out [C, n_out], zf)."""
    import torch
    t = dsp.load_filter_tables()
    b, a = np.ascontiguousarray(t["bdec"], np.float64), np.ascontiguousarray(t["adec"], np.float64)
    C, n = x.shape
    n_out = n
    for _ in range(n_stages):
        n_out = (n_out + 1) // 2
    out = torch.full((C, n_out + 3), np.nan, dtype=torch.float64, device=x.device)      # three guard columns
    zf = torch.empty((C, n_stages, 12), dtype=torch.float64, device=x.device)
    zin = None if zi is None else torch.from_numpy(np.ascontiguousarray(zi)).to(x.device)
    got = ctypes.c_int64(0)
    DP, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    from friture_amd import _lib
    _lib.check(hip.frt_delaybatch_decimate(b.ctypes.data_as(DP), a.ctypes.data_as(DP), 13, n_stages, vp(x.data_ptr()),
                                           int(x.dtype == torch.float64), C, n, x.stride(0), origin,
                                           None if zin is None else vp(zin.data_ptr()), vp(out.data_ptr()), out.stride(0), vp(zf.data_ptr()),
                                           ctypes.byref(got)))
    torch.cuda.synchronize()
    assert got.value == n_out and bool(torch.isnan(out[:, n_out:]).all())
    return out[:, :n_out].cpu().numpy(), zf.cpu().numpy()


def decimate_reference(x, zi):
    t = dsp.load_filter_tables()
    b, a = np.array(t["bdec"], np.float64), np.array(t["adec"], np.float64)
    ys, zs = [], []
    for c in range(x.shape[0]):
        z = dsp.decimate_multiple_filtic(2, b, a) if zi is None else [zi[c, 0].copy(), zi[c, 1].copy()]
        y, zf = dsp.decimate_multiple(2, b, a, x[c].astype(np.float64), z)
        ys.append(y)
        zs.append(np.array(zf))
    return np.array(ys), np.array(zs)


@functools.lru_cache(maxsize=None)
def carried_states():
    """DF2T states [4, 2, 12] as a running decimator has them: after 5000 samples of noise."""
    rng = np.random.default_rng(5)
    return decimate_reference(0.25 * rng.standard_normal((4, 5000)) + 0.01, None)[1]


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [4, 8, 252, 4096 + 4, 1 << 16])
def test_decimate_alone(hip, n, dtype, carry):
    import torch
    rng = np.random.default_rng(n)
    x = (0.25 * rng.standard_normal((4, n)) + 0.01).astype(dtype)
    zi = carried_states() if carry else None
    ref, zref = decimate_reference(x, zi)
    got, zgot = run_decimate(hip, torch.from_numpy(x).cuda(), zi, origin=0 if not carry else 20000)
    assert got.shape == ref.shape
    scale = np.max(np.abs(ref), axis=1, keepdims=True)
    worst = float(np.max(np.abs(got - ref) / scale))
    worst_z = float(np.max(np.abs(zgot - zref) / np.max(np.abs(zref), axis=2, keepdims=True)))
    print(f"n {n} {np.dtype(dtype).name} carry {carry}: samples {worst:.3e} (bar {DEC_BAR}), states {worst_z:.3e} (bar {STATE_BAR})")
    assert worst <= DEC_BAR and worst_z <= STATE_BAR


def test_decimate_reads_strided_rows_and_keeps_zeros(hip):
    import torch
    rng = np.random.default_rng(3)
    n = 4096 + 4
    wide = torch.from_numpy(0.25 * rng.standard_normal((4, n + 37))).cuda()
    view = wide[:, 5:5 + n]                                          # rows n + 37 apart, starting 5 in
    ref, zref = decimate_reference(view.cpu().numpy(), None)
    got, zgot = run_decimate(hip, view, None)
    assert float(np.max(np.abs(got - ref) / np.max(np.abs(ref)))) <= DEC_BAR
    assert float(np.max(np.abs(zgot - zref) / np.max(np.abs(zref)))) <= STATE_BAR
    got, zgot = run_decimate(hip, torch.zeros((4, n), dtype=torch.float32).cuda(), None)
    assert not got.any() and not zgot.any()                          # zeros in, exact zeros out


@pytest.mark.parametrize("name,cut", [("r0.1", 100 * 512), ("r0.1", 8 * 4800), ("r1.0", 100 * 512), ("r1.0", 2 * 48000)])
def test_two_pieces_equal_the_whole(hip, name, cut):
    """Cut inside a window and on a window's end, the chunks the same on both sides."""
    delayrange, T = H.CASES[name][:2]
    x = np.array(case(name, np.float32)[0])
    ends = H.ends_with_cut(T, cut)
    batch = DelayEstimatorBatch(delayrange)
    whole = batch.run(x, ends=ends, keep="all", with_xcorr=True)
    a = batch.run(x[..., :cut], ends=ends[ends <= cut], keep="all", with_xcorr=True)
    held = [np.array(v) for v in (a.state.zi, a.state.tail, a.state.smoothed, a.state.means, a.state.ring.cells)]
    b = batch.run(x[..., cut:], ends=ends[ends > cut] - cut, state=a.state, keep="all", with_xcorr=True)
    for before, after in zip(held, (a.state.zi, a.state.tail, a.state.smoothed, a.state.means, a.state.ring.cells)):
        assert np.array_equal(before, after)                         # the caller's state is not written to
    assert np.array_equal(np.concatenate([a.window_end, b.window_end]), whole.window_end)
    assert np.array_equal(np.concatenate([a.refresh_chunk, b.refresh_chunk + int((ends <= cut).sum())]), whole.refresh_chunk)
    assert np.array_equal(b.state.ring.cells, whole.state.ring.cells) and b.state.pending == whole.state.pending
    assert b.state.seen == whole.state.seen == T
    for k in ("gated", "correlation", "argmax"):
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)], axis=1), getattr(whole, k)), k
    worst = 0.0
    for k in FIELDS + ("shown_delay_ms", "shown_distance_m", "shown_extremum"):
        got, ref = np.concatenate([getattr(a, k), getattr(b, k)], axis=1), getattr(whole, k)
        worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))))
    got = np.concatenate([a.xcorr, b.xcorr], axis=1)
    live = whole.gated == 0
    scale = np.max(np.abs(whole.xcorr), axis=2)
    worst = max(worst, float(np.max((np.max(np.abs(got - whole.xcorr), axis=2) / np.where(live, scale, 1.0))[live])))
    for k in ("smoothed", "tail", "zi", "readout"):
        u, v = getattr(b.state, k), getattr(whole.state, k)
        worst = max(worst, float(np.max(np.abs(u - v)) / np.max(np.abs(v))))
    print(f"{name} cut at {cut}: worst {worst:.3e} (bar {BAR})")
    assert worst <= BAR


def test_slabs_do_not_change_a_bit(hip):
    x = np.array(case("r0.1", np.float32)[0])
    batch = DelayEstimatorBatch(0.1)
    one = batch.run(x, keep="all", with_xcorr=True)
    assert batch.last_slabs == 1
    many = batch.run(x, keep="all", with_xcorr=True, scratch_bytes=1)          # a pair per slab
    assert batch.last_slabs == 26
    some = batch.run(x, keep="all", with_xcorr=True, scratch_bytes=7 * 2 * 2400 * 8)      # slabs of 7 pairs and a last one of 5
    assert batch.last_slabs == 4
    for other in (many, some):
        for k in FIELDS + ("correlation", "gated", "argmax", "xcorr", "shown_extremum"):
            assert np.array_equal(getattr(one, k), getattr(other, k)), k
        assert np.array_equal(one.state.smoothed, other.state.smoothed) and np.array_equal(one.state.means, other.state.means)


def test_run_leaves_the_process_option_alone_and_is_unmoved_by_it(hip, monkeypatch, option):
    """The batch's GCC-PHAT handles carry their own dispatch: run() neither sets nor reads "gcc_one_workgroup", and a run while
    the option forces the launches of phases equals one at the shape rule bit for bit."""
    from friture_amd import _lib

    def refuse(*args):
        raise AssertionError("DelayEstimatorBatch.run touched a process option")
    x = np.array(case("r0.1", np.float32)[0])
    batch = DelayEstimatorBatch(0.1)
    with monkeypatch.context() as m:
        m.setattr(_lib, "set_option", refuse)
        m.setattr(_lib, "get_option", refuse)
        first = batch.run(x, keep="all", with_xcorr=True)
    assert _lib.get_option("gcc_one_workgroup") == -1
    option("gcc_one_workgroup", 0)
    for other in (batch, DelayEstimatorBatch(0.1)):                  # handles made before the option was forced, and after
        second = other.run(x, keep="all", with_xcorr=True)
        assert _lib.get_option("gcc_one_workgroup") == 0
        for k in ("xcorr",) + FIELDS + ("correlation", "gated", "argmax"):
            assert np.array_equal(getattr(first, k), getattr(second, k)), k
        assert np.array_equal(first.state.smoothed, second.state.smoothed) and np.array_equal(first.state.means, second.state.means)


@pytest.mark.parametrize("name", list(H.CASES))
def test_refreshes_equal_the_stream_object(hip, name):
    delayrange, T = H.CASES[name][:2]
    x = np.array(case(name, np.float64)[0][0])
    res = DelayEstimatorBatch(delayrange).run(x, keep="all")
    stream = DelayEstimatorStream(delayrange)
    rows = []
    for c in range(T // 512):
        stream.handle_new_data(x[:, c * 512:(c + 1) * 512])
        rows.append((stream.delay_ms, stream.distance_m, stream.Xcorr_extremum, stream.correlation))
    rows = np.array(rows, np.float64)[res.refresh_chunk]
    assert res.shown_delay_ms.shape == (len(res.refresh_chunk),)
    worst = 0.0
    for k, column in enumerate(("shown_delay_ms", "shown_distance_m", "shown_extremum")):
        worst = max(worst, float(np.max(np.abs(getattr(res, column) - rows[:, k]) / np.maximum(np.abs(rows[:, k]), 1.0))))
    print(f"{name} against DelayEstimatorStream: worst {worst:.3e} (bar {BAR})")
    assert worst <= BAR and np.array_equal(res.shown_correlation, rows[:, 3])


def test_keep_last_squeeze_and_short_recordings(hip):
    import torch
    x = np.array(case("r0.1", np.float32)[0])
    batch = DelayEstimatorBatch(0.1)
    every, last = batch.run(x, keep="all"), batch.run(x)
    for k in ("shown_delay_ms", "shown_distance_m", "shown_extremum", "shown_correlation"):
        assert getattr(last, k).shape == (2,) and np.array_equal(getattr(last, k), getattr(every, k)[:, -1]), k
    assert last.xcorr is None and np.array_equal(last.delay_ms, every.delay_ms)
    one = batch.run(x[0], keep="all", with_xcorr=True)               # the stream axis left out
    assert one.delay_ms.shape == (13,) and one.xcorr.shape == (13, 2400) and one.shown_correlation.shape == (13,)
    assert one.state.zi.shape == (1, 2, 2, 12)
    assert np.array_equal(one.delay_ms, every.delay_ms[0]) and np.array_equal(one.correlation, every.correlation[0])
    # too short for any window: nothing per window, the carried read-out, and a state to go on from
    short = batch.run(x[..., :2048], keep="last")
    assert len(short.window_end) == 0 and short.delay_ms.shape == (2, 0) and short.shown_delay_ms.shape == (2,)
    assert not short.shown_delay_ms.any() and not short.state.present.any() and short.state.pending == 512
    rest = batch.run(x[..., 2048:], state=short.state, keep="all")
    assert np.array_equal(rest.window_end, every.window_end) and np.array_equal(rest.gated, every.gated)
    assert np.array_equal(rest.correlation, every.correlation)
    assert float(np.max(np.abs(rest.extremum - every.extremum))) <= BAR
    carried = batch.run(x[..., :1024], state=rest.state, keep="last")      # no window: the read-out is the carried one
    assert np.array_equal(carried.shown_extremum, rest.shown_extremum[:, -1])
    with pytest.raises(ValueError):
        DelayEstimatorBatch(0.5).run(x, state=rest.state)
    cuda = batch.run(torch.from_numpy(x).cuda(), keep="last")
    assert cuda.shown_extremum.is_cuda and np.array_equal(cuda.shown_extremum.cpu().numpy(), last.shown_extremum)


def test_readout_alone_keeps_the_correlation_across_gated_windows(hip):
    """frt_delaybatch_readout on made-up correlations with gated windows in the middle, against the reference's lines."""
    import torch
    rng = np.random.default_rng(9)
    S, W, L = 3, 7, 2400
    xc = rng.standard_normal((S, W, L)) * 0.01
    for s in range(S):
        for w in range(W):
            xc[s, w, (37 * (w + 1) + 1000 * s) % L] = 0.5 * (-1) ** w
    gated = np.zeros((S, W), np.int32)
    gated[0, 2:4] = 1
    gated[1, 0] = 1
    gated[2, :] = 1
    old = rng.standard_normal((S, L)) * 0.01
    present = np.array([1, 0, 1], np.int32)
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(xc=xc, gated=gated, old=old, present=present).items()}
    sm, pres = torch.empty((S, L), dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    am, corr = (torch.empty((S, W), dtype=torch.int32, device=dev) for _ in range(2))
    d, m, e = (torch.empty((S, W), dtype=torch.float64, device=dev) for _ in range(3))
    vp = ctypes.c_void_p
    from friture_amd import _lib
    _lib.check(hip.frt_delaybatch_readout(vp(t["xc"].data_ptr()), vp(t["gated"].data_ptr()), S, W, L, vp(t["old"].data_ptr()),
                                          vp(t["present"].data_ptr()), 0.3, 12000.0, 0.1, vp(sm.data_ptr()), vp(pres.data_ptr()),
                                          vp(am.data_ptr()), vp(d.data_ptr()), vp(m.data_ptr()), vp(e.data_ptr()), vp(corr.data_ptr())))
    torch.cuda.synchronize()
    for s in range(S):
        carried = old[s] if present[s] else None
        for w in range(W):
            if gated[s, w]:
                assert (am[s, w].item(), d[s, w].item(), m[s, w].item(), e[s, w].item(), corr[s, w].item()) == (0, 0.0, 0.0, 0.0, 0)
                continue
            ro = dsp.delay_readout(xc[s, w], carried, 12000.0, 0.1)
            carried = ro["smoothed"]
            assert am[s, w].item() == ro["argmax"] and corr[s, w].item() == ro["correlation_pct"]
            assert abs(e[s, w].item() - ro["extremum"]) <= BAR and abs(d[s, w].item() - ro["delay_ms"]) <= BAR
            assert abs(m[s, w].item() - ro["distance_m"]) <= BAR
        assert pres[s].item() == int(carried is not None)
        if carried is not None:
            assert float(np.max(np.abs(sm[s].cpu().numpy() - carried))) <= BAR
