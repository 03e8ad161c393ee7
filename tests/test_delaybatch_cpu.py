"""DelayEstimatorBatch without a GPU: delay_schedule's run table against oracle.dsp.MirrorRing, the numpy replay of the widget
(oracle/delaybatch.py) against the reference widget's recorded read-outs, and the input checks."""
import numpy as np
import pytest

from friture_amd.delay_estimator import DelayEstimatorBatch, DelayRing, delay_lengths, delay_schedule
from oracle import delaybatch as H
from oracle import dsp


def mark(k):
    """The 'mean' of window k: distinct, and exact when subtracted from a sample index."""
    return 0.25 + k / 1024.0


def ring_views(sizes, delayrange, gate=()):
    """dsp.MirrorRing fed decimated chunks of `sizes` samples whose values are their own index + 1; every window's view is
    recorded and then has its mark subtracted in place, as GCC-PHAT does with the mean (not for the windows in `gate`)."""
    length, needed = delay_lengths(delayrange)
    ring, old_index, views, offset = dsp.MirrorRing(), 0, [], 0
    for m in sizes:
        ring.push(np.arange(offset + 1, offset + m + 1, dtype=np.float64).reshape(1, -1))
        offset += m
        for _ in range(int((ring.offset - old_index) / needed)):
            old_index += needed
            view = ring.data_indexed(old_index, length).reshape(-1)
            views.append(view.copy())
            if len(views) - 1 not in gate:
                view -= mark(len(views) - 1)
    return views


def rebuild(plan, first_window, base, gate=()):
    """The windows that plan.runs describes, for a stream whose sample at decimated index i is i + 1; base: the absolute index
    of the carried tail's first sample; first_window: the count of the call's first window."""
    out = []
    for w, rows in enumerate(plan.runs):
        parts = []
        for first, n, zero, prior in rows.tolist():
            if n == 0:
                continue
            v = np.zeros(n) if zero else np.arange(first + base + 1, first + base + n + 1, dtype=np.float64)
            k = first_window + prior if prior >= 0 else first_window - 1      # -2: the last window before this call
            if prior != -1 and k not in gate:
                v = v - mark(k)
            parts.append(v)
        out.append(np.concatenate(parts))
    return out


RAGGED = [512, 1024, 1028, 4100, 124100, 124612, 154612, 155124, 200000, 424000, 424512, 500000]


@pytest.mark.parametrize("delayrange,ends,gate", [(0.1, None, ()), (0.4, None, ()), (0.5, None, ()), (1.0, None, ()),
                                                  (0.1, RAGGED, ()), (1.0, RAGGED, ()), (0.1, None, (3, 4, 9)), (1.0, None, (1, 2))])
def test_runs_rebuild_every_ring_view(delayrange, ends, gate):
    T = 500000 if ends else 1 << 19
    plan = delay_schedule(T, delayrange, 512, ends)
    sizes = np.diff(ends, prepend=0) // 4 if ends else [128] * (T // 512)
    views = ring_views(sizes, delayrange, gate)
    assert len(views) == len(plan.window_end) > 8
    assert plan.runs.shape == (len(views), 8, 4) and plan.runs.dtype == np.int64
    mine = rebuild(plan, 0, -plan.tail, gate)
    for w, (a, b) in enumerate(zip(views, mine)):
        assert np.array_equal(a, b), f"window {w}"
    length, needed = delay_lengths(delayrange)
    assert np.array_equal(plan.window_end, needed * np.arange(1, len(views) + 1))
    assert plan.window_start[-1] == len(views) and len(plan.window_start) == len(plan.refresh_chunk) + 1
    kinds = {(int(z), int(p >= 0)) for z, p, n in zip(plan.runs[:, :, 2].ravel(), plan.runs[:, :, 3].ravel(), plan.runs[:, :, 1].ravel()) if n}
    assert (0, 1) in kinds and (0, 0) in kinds                # carried means and untouched mirror copies both occur
    if length > 10000:
        assert (1, 0) in kinds                                  # zeros where samples were lost before the ring grew


@pytest.mark.parametrize("delayrange,cut", [(0.1, 100 * 512), (0.1, 8 * 4800), (1.0, 100 * 512), (1.0, 2 * 48000)])
def test_a_cut_recording_plans_like_the_whole(delayrange, cut):
    """Cut inside a window and on a window's end.  The ring's growth depends on the chunks, so whole and pieces see the same
    chunks: those of 512 samples, and one that ends at the cut."""
    T = 1 << 18
    ends = H.ends_with_cut(T, cut)
    whole = delay_schedule(T, delayrange, ends=ends)
    a = delay_schedule(cut, delayrange, ends=ends[ends <= cut])
    b = delay_schedule(T - cut, delayrange, ends=ends[ends > cut] - cut, state=a.ring)
    assert (cut // 4) % delay_lengths(delayrange)[1] == 0 or a.ring.offset > a.ring.old_index
    assert np.array_equal(np.concatenate([a.window_end, b.window_end]), whole.window_end)
    assert np.array_equal(b.ring.cells, whole.ring.cells) and b.ring[:4] == whole.ring[:4] and b.ring.length == whole.ring.length
    assert np.array_equal(np.concatenate([a.refresh_chunk, b.refresh_chunk + int((ends <= cut).sum())]), whole.refresh_chunk)
    views = ring_views(np.diff(ends, prepend=0) // 4, delayrange)
    mine = rebuild(a, 0, -a.tail) + rebuild(b, len(a.window_end), a.ring.offset - b.tail)
    assert len(mine) == len(views) > 4
    for w, (u, v) in enumerate(zip(views, mine)):
        assert np.array_equal(u, v), f"window {w}"


def test_schedule_refuses_what_it_cannot_plan():
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.1, chunk=510)                # not a multiple of 4
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.1, ends=[512, 1022, 1 << 16])
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.1, ends=[1024, 512, 1 << 16])     # unsorted
    with pytest.raises(ValueError):
        delay_schedule((1 << 16) + 2, 0.1)                      # a short last chunk of 2 samples
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.1, ends=[512, 1024])          # the chunks do not cover the recording
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 1.0 / 24000 * 1.5)              # windows of 3 samples: GCC-PHAT takes even lengths from 4 on
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 1e-5)
    ring = delay_schedule(1 << 16, 0.1).ring
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.5, state=ring)                # another delay range
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.1, state=ring._replace(cells=ring.cells[:, :-2]))
    with pytest.raises(ValueError):
        delay_schedule(1 << 16, 0.1, state=(1, 2, 3))
    assert isinstance(ring, DelayRing)


def test_batch_checks_its_input_before_the_device():
    batch = DelayEstimatorBatch(0.1)
    with pytest.raises(ValueError):
        batch.run(np.zeros((2, 3, 1024), np.float32))           # not two channels
    with pytest.raises(TypeError):
        batch.run(np.zeros((2, 1024), np.int16))
    with pytest.raises(ValueError):
        batch.run(np.zeros((2, 1024), np.float32), keep="some")
    with pytest.raises(ValueError):
        batch.run(np.zeros((2, 1022), np.float32))


def test_batch_refuses_a_state_of_another_shape():
    """Every array of a DelayState is checked against the input before anything reaches the device."""
    from friture_amd.delay_estimator import DelayState
    batch, S, L = DelayEstimatorBatch(0.1), 2, 2400
    ring = delay_schedule(2048, 0.1).ring                      # 512 decimated samples pending, no window yet
    good = dict(zi=np.zeros((S, 2, 2, 12)), samples=np.zeros((S, 2, 0)), tail=np.zeros((S, 2, L + 512)), pending=512, ring=ring,
                means=np.zeros((S, 2)), gated=np.zeros(S, np.int32), smoothed=np.zeros((S, L)), present=np.zeros(S, np.int32),
                readout=np.zeros((S, 4)), seen=2048)
    x = np.zeros((S, 2, 1024), np.float32)
    wrong = dict(zi=np.zeros((S, 2, 2, 11)), samples=np.zeros((S, 2, 4)), tail=np.zeros((S, 2, L)), means=np.zeros((S, 3)),
                 gated=np.zeros(S + 1, np.int32), smoothed=np.zeros((S, L + 2)), present=np.zeros(1, np.int32), readout=np.zeros((S, 3)),
                 pending=100)
    for name, value in wrong.items():
        with pytest.raises(ValueError):
            batch.run(x, state=DelayState(**{**good, name: value}))
    with pytest.raises(ValueError):
        batch.run(x[:1], state=DelayState(**good))              # a state of two streams, one stream of samples
    with pytest.raises(ValueError):
        DelayEstimatorBatch(0.5).run(x, state=DelayState(**good))      # another delay range


@pytest.mark.parametrize("name", list(H.GOLDEN))
def test_replay_equals_the_reference_widget(golden, name):
    """The numpy replay is built from pieces that tests/test_oracle_golden.py holds to the reference bit for bit (decimation,
    ring, gcc_phat), so it equals the widget's recorded read-outs bit for bit."""
    g = golden("delaybatch")
    case, stream, _ = H.GOLDEN[name]
    r = H.replay(H.signal(case)[stream], H.CASES[case][0], H.golden_ends(name))
    for k, column in enumerate(H.COLUMNS):
        assert np.array_equal(r["shown"][:, k], g[f"{name}_{column}"]), column
    assert np.array_equal(r["smoothed"], g[f"{name}_old_Xcorr"])
    assert len(r["gated"]) >= 5


@pytest.mark.parametrize("name", list(H.CASES))
def test_replay_cases_decide_clearly(name):
    """What the GPU tests rely on: in every case the reference's gate (numpy.std > 0) and the stream object's (all samples
    equal) agree, the last stream's first three windows are gated, and at most one window per stream is
    decided by less than rounding can move."""
    delayrange, T, _, S = H.CASES[name]
    x = H.signal(name)
    for s in range(S):
        r = H.replay(x[s], delayrange, H.chunk_ends(T))
        assert np.array_equal(r["gated"].astype(bool), r["silent"])
        assert sum(H.doubtful(r, w) for w in range(len(r["gated"])) if not r["gated"][w]) <= 1
        if s == S - 1:
            assert r["gated"][:3].all() and not r["gated"][3:].any()        # gated from the zero state on, live afterwards
        else:
            assert not r["gated"].any()
