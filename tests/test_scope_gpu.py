"""The oscilloscope on the GPU (scope.hip) against tests/golden/scope.npz (the reference Scope_Widget) and against itself
(device ring vs host ring, batch vs widget, streams, dtypes, host vs device memory)."""
from pathlib import Path

import numpy as np
import pytest

from oracle import scope as H

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "scope.npz"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _chunk(name, x, s, n, rows):
    c = x[:rows, s:s + n]
    return c.astype(np.float32) if name == "exact_level_f32" else c


def _drive(name, ring):
    """Scope fed the case chunk by chunk through `ring`; yields (k, scope, window length) after every refresh."""
    from friture_amd.scope import Scope, width_for
    x = H.signal(name)
    sc = Scope()
    sc.set_buffer(ring)
    for k, (s, n, rows, tr) in enumerate(H.schedule(name)):
        c = _chunk(name, x, s, n, rows)
        if hasattr(ring, "_zeros") and not isinstance(ring.buffer, np.ndarray):
            import torch
            c = torch.from_numpy(np.ascontiguousarray(c, np.float64)).cuda()
        ring.push(c)
        sc.set_timerange(tr)
        sc.handle_new_data(c)
        w = width_for(tr)
        yield k, sc, (w if tr > 500.0 else 2 * w)


@pytest.mark.parametrize("name", H.CASES)
def test_scope_matches_reference(g, name):
    from friture_amd.ringbuffer import RingBuffer
    trig, start, length, ok, dig = (g[f"{name}_{f}"] for f in ("trig", "start", "len", "ok", "dig"))
    ring = RingBuffer()
    prev = None
    for k, sc, n_win in _drive(name, ring):
        assert sc.triggered == bool(trig[k]), k
        assert sc.y.shape[0] == length[k], k
        assert H.digest(sc.scaled_y) == dig[k, 0] and H.digest(sc.scaled_y2) == dig[k, 1], k
        if not sc.triggered:
            if prev is not None:                               # the previous curves stay
                assert sc.scaled_y is prev[0] and sc.scaled_t is prev[1]
            continue
        prev = (sc.scaled_y, sc.scaled_t)
        assert ring.offset - n_win + sc.trace_start == start[k], k
        tr = H.schedule(name)[k][3]
        w = H.width_for(tr)
        assert np.array_equal(sc.scaled_t, H.scaled_t(w, tr, sc.y.shape[0]))
        assert np.array_equal(sc.scaled_y, 1. - (sc.y + 1) / 2., equal_nan=True)
        if ok[k]:
            win = H.expected_window(name, k, n_win)
            L = sc.y.shape[0]
            assert np.array_equal(sc.y, win[0, sc.trace_start:sc.trace_start + L], equal_nan=True), k
            if win.shape[0] > 1:
                assert np.array_equal(sc.y2, win[1, sc.trace_start:sc.trace_start + L], equal_nan=True), k
            else:
                assert sc.y2 is None
        if k in H.FULL_REFRESHES.get(name, ()):
            assert np.array_equal(sc.y, g[f"{name}_full{k}_raw"])
            assert np.array_equal(sc.scaled_y, g[f"{name}_full{k}_y"])
            if f"{name}_full{k}_y2" in g.files:
                assert np.array_equal(sc.scaled_y2, g[f"{name}_full{k}_y2"])


@pytest.mark.parametrize("name", ["stereo", "nan_burst", "change", "switch", "irregular", "tr_2000"])
def test_device_ring_equals_host_ring(name):
    from friture_amd.ringbuffer import DeviceRingBuffer, RingBuffer
    host = list((k, sc.triggered, sc.trace_start, sc.y.copy(), None if sc.y2 is None else sc.y2.copy(), sc.scaled_y.copy(),
                 sc.scaled_y2.copy(), sc.scaled_t.copy()) for k, sc, _ in _drive(name, RingBuffer()))
    dev = list((k, sc.triggered, sc.trace_start, sc.y.copy(), None if sc.y2 is None else sc.y2.copy(), sc.scaled_y.copy(),
                sc.scaled_y2.copy(), sc.scaled_t.copy()) for k, sc, _ in _drive(name, DeviceRingBuffer()))
    assert len(host) == len(dev)
    for a, b in zip(host, dev):
        assert a[:3] == b[:3]
        for u, v in zip(a[3:], b[3:]):
            assert (u is None and v is None) or np.array_equal(u, v, equal_nan=True)


REGULAR = ["stereo", "noise", "silence_tone", "impulses", "nan_burst", "exact_level", "exact_level_f32"] + \
          [f"tr_{t}" for t in H.TIMERANGES]


@pytest.mark.parametrize("name", REGULAR + ["irregular"])
def test_batch_equals_widget(g, name):
    """ScopeBatch at a fixed timerange computes what the widget fed chunk by chunk computed: starts, traces, and what the curves
    show after every refresh (the last trace carried forward)."""
    from friture_amd.scope import ScopeBatch
    x = H.signal(name)
    if name == "exact_level_f32":
        x = x.astype(np.float32)
    sched = H.schedule(name)
    tr = sched[0][3]
    ends = np.array([s + n for s, n, _, _ in sched], np.int64)
    res = ScopeBatch(tr).run(x, ends=ends, traces="scaled")
    assert np.array_equal(res.starts, g[f"{name}_start"])
    assert np.array_equal(res.triggered, g[f"{name}_trig"])
    src, shown = res.carry_forward()
    for k in range(len(sched)):
        for c in range(x.shape[0]):
            want = g[f"{name}_dig"][k, c]
            assert H.digest(shown[c, k] if src[k] >= 0 else np.zeros(10)) == want, (k, c)
    raw = ScopeBatch(tr).run(x, ends=ends, traces="raw")
    assert np.array_equal(raw.starts, res.starts)
    assert np.array_equal(res.traces[:, raw.triggered], 1. - (raw.traces[:, raw.triggered] + 1) / 2., equal_nan=True)


def test_batch_default_chunks_equal_explicit_ends():
    from friture_amd.scope import ScopeBatch
    x = H.signal("stereo")[:, :20000]
    a = ScopeBatch(50).run(x)
    b = ScopeBatch(50).run(x, ends=H.chunk_ends(20000))
    assert np.array_equal(a.starts, b.starts) and a.traces is None


def test_streams_are_independent():
    from friture_amd.scope import ScopeBatch
    names = ["stereo", "noise", "silence_tone", "impulses", "nan_burst"]
    xs = np.stack([np.broadcast_to(H.signal(nm)[:, :40000], (2, 40000)) for nm in names])
    sb = ScopeBatch(50)
    many = sb.run(xs, traces="raw")
    for s in range(len(names)):
        one = sb.run(np.ascontiguousarray(xs[s]), traces="raw")
        assert np.array_equal(many.starts[s], one.starts)
        assert np.array_equal(many.traces[s], one.traces, equal_nan=True)


@pytest.mark.parametrize("tr", [10.9, 50, 500, 2000])
def test_float32_equals_float64_of_same_values(tr):
    from friture_amd.scope import ScopeBatch
    x32 = H.tone_noise(60000, 21).astype(np.float32)
    sb = ScopeBatch(tr)
    a = sb.run(x32, traces="raw")
    b = sb.run(x32.astype(np.float64), traces="raw")
    assert np.array_equal(a.starts, b.starts) and np.array_equal(a.traces, b.traces)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_host_and_device_memory_agree(dtype):
    import torch
    from friture_amd.scope import ScopeBatch
    x = np.stack([H.tone_noise(50000, 30 + s) for s in range(3)]).astype(dtype)
    sb = ScopeBatch(50)
    a = sb.run(x, traces="scaled")
    xd = torch.from_numpy(x).cuda()
    b = sb.run(xd, traces="scaled")
    assert np.array_equal(a.starts, b.starts.cpu().numpy())
    assert np.array_equal(a.triggered, b.triggered.cpu().numpy())
    assert np.array_equal(a.traces, b.traces.cpu().numpy())
    # strided rows: every other row of a wider device tensor
    wide = torch.zeros((3, 4, 50000), dtype=xd.dtype, device="cuda")
    wide[:, ::2] = xd
    c = sb.run(wide[:, ::2], traces="scaled")
    assert np.array_equal(a.starts, c.starts.cpu().numpy()) and np.array_equal(a.traces, c.traces.cpu().numpy())


def test_host_traces_untouched_without_trigger():
    """Slots of refreshes without a trigger keep what the caller's buffer held (host outputs are staged both ways)."""
    import ctypes
    from friture_amd import _lib
    x = np.zeros((1, 8000))
    x[0, 5000] = 1.0
    ends = np.array([3000, 6000, 8000], np.int64)
    starts = np.empty(3, np.int64)
    tr = np.full((1, 3, 2400), 7.0)
    lib = _lib.init()
    _lib.check(lib.frt_scope_run(x.ctypes.data, 1, 1, 1, 8000, 8000, 0, ends.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 3,
                                 2400, 0, starts.ctypes.data, tr.ctypes.data, 1))
    assert np.array_equal(starts, H.batch_np(x[0], ends, 2400, False))
    for k in range(3):
        if starts[k] == H.NO_TRIGGER:
            assert np.all(tr[0, k] == 7.0)
        else:
            assert not np.all(tr[0, k] == 7.0)
    assert (starts == H.NO_TRIGGER).sum() >= 1


@pytest.mark.parametrize("where", ["left_edge", "left_sub", "middle", "right_sub", "right_edge", "nan_left", "nan_left_sub",
                                   "nan_middle", "nan_right_sub", "nan_right", "before_start"])
def test_500ms_whole_blocks_and_partial_edges(where):
    """w = 24 000: regions of 46 whole 512-blocks plus partial edges on both sides (whole 64-sample sub-blocks, then single
    samples).  The peak (or a NaN) is put in the samples or the sub-blocks at either end, or in a whole block, of one refresh's
    region; irregular ends, some before 2w (zeros in front)."""
    from friture_amd.scope import ScopeBatch
    w, T = 24000, 200000
    rng = np.random.default_rng(7)
    x = 0.1 * rng.standard_normal(T)
    ends = np.unique(np.concatenate([rng.integers(0, T + 1, 300), [100004, 60001, 48000, 47999, 700, T]]))
    e = 100004
    r0, r1 = e - 2 * w + w // 2, e - w + w // 2
    assert r0 % 512 and r1 % 512
    pos = {"left_edge": r0 + 3, "left_sub": r0 + 100, "middle": r0 + 5000, "right_sub": r1 - 40, "right_edge": r1 - 2,
           "nan_left": r0 + 1, "nan_left_sub": r0 + 200, "nan_middle": r0 + 9000, "nan_right_sub": r1 - 100, "nan_right": r1 - 1,
           "before_start": None}[where]
    if pos is not None:
        x[pos] = np.nan if where.startswith("nan") else 3.0
        x[pos - 1] = -1.0
    sb = ScopeBatch(500)
    assert sb.width == w and not sb.scrolling
    res = sb.run(x[None], ends=ends, traces="raw")
    want = H.batch_np(x, ends, w, False)
    assert np.array_equal(res.starts, want)
    k = int(np.nonzero(ends == e)[0][0])
    if where.startswith("nan"):
        assert not res.triggered[k]
    elif pos is not None:
        assert res.starts[k] == pos - 1 - w // 2
    for j in np.nonzero(res.triggered)[0]:
        s = res.starts[j]
        seg = np.concatenate([np.zeros(max(0, -s)), x[max(s, 0):s + 2 * (w // 2)]])
        assert np.array_equal(res.traces[0, j], seg, equal_nan=True)


@pytest.mark.parametrize("width", [1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1100])
def test_widths_around_the_block_sizes(width):
    """Regions that hold no, one or a few 64-sample sub-blocks and 512-sample blocks, at every alignment (ends 0 .. 3000),
    over noise with spikes and a NaN: the starts and traces of the numpy restatement."""
    from friture_amd import _lib
    from friture_amd.scope import NO_TRIGGER
    rng = np.random.default_rng(width)
    T = 3000
    x = 0.1 * rng.standard_normal(T)
    x[rng.integers(0, T, 12)] = 2.0 * rng.random(12)
    x[1700] = np.nan
    ends = np.arange(0, T + 1, dtype=np.int64)
    import ctypes
    L = 2 * (width // 2)
    starts = np.empty(ends.shape[0], np.int64)
    tr = np.zeros((1, ends.shape[0], max(L, 1)))
    lib = _lib.init()
    _lib.check(lib.frt_scope_run(x.ctypes.data, 1, 1, 1, T, T, 0, ends.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                 ends.shape[0], width, 0, starts.ctypes.data, tr.ctypes.data if L else None, 1 if L else 0))
    assert np.array_equal(starts, H.batch_np(x, ends, width, False))
    for k in np.nonzero(starts != NO_TRIGGER)[0][::7]:
        s = starts[k]
        seg = np.concatenate([np.zeros(max(0, -s)), x[max(s, 0):s + L]])
        assert np.array_equal(tr[0, k, :L], seg, equal_nan=True)


def test_bad_arguments_are_rejected_with_a_message():
    import ctypes
    from friture_amd import _lib
    lib = _lib.init()
    x = np.zeros(1000)
    st = np.empty(4, np.int64)
    P = ctypes.POINTER(ctypes.c_int64)

    def call(ends, width=100, n=1000, dtype=1, kind=0, trace=None):
        ends = np.asarray(ends, np.int64)
        return lib.frt_scope_run(x.ctypes.data, dtype, 1, 1, n, n, 0, ends.ctypes.data_as(P), ends.shape[0], width, 0,
                                 st.ctypes.data, trace, kind)
    for kwargs, msg in [({"ends": [500], "width": 0}, b"width"), ({"ends": [600, 500]}, b"not sorted"),
                        ({"ends": [1001]}, b"outside"), ({"ends": [-1]}, b"outside"), ({"ends": [500], "dtype": 2}, b"dtype"),
                        ({"ends": [500], "kind": 4}, b"trace_kind"), ({"ends": [500], "n": -1}, b"bad shape")]:
        assert call(**kwargs) == -1, kwargs
        assert msg in lib.frt_last_error(), (kwargs, lib.frt_last_error())
    from friture_amd.scope import ScopeBatch
    with pytest.raises(_lib.FritureHipError) as err:
        ScopeBatch(0.01).run(np.zeros((1, 100)))
    assert err.value.status == -1
