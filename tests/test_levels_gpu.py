"""Level meters and long-time levels on the GPU (levels.hip) against tests/golden/levels.npz (the reference widgets) and
against themselves (streaming vs batch, channels, dtypes, state)."""
from pathlib import Path

import numpy as np
import pytest

from oracle import levels as H

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "levels.npz"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _ballistic_replay(levels_rms, levels_max):
    """BallisticPeak (ballistic_peak.py:21-66) on the host, fed dB values."""
    from friture_amd.iec import dB_to_IEC
    from friture_amd.levels import PEAK_DECAY_RATE, PEAK_FALLOFF
    peak, hold, factor, out = 0.0, 0, PEAK_DECAY_RATE, []
    for r, m in zip(levels_rms, levels_max):
        v = dB_to_IEC(max(m, r))
        if v > peak:
            new, hold, factor = v, 0, PEAK_DECAY_RATE
        elif hold + 1 <= PEAK_FALLOFF:
            new, hold = peak, hold + 1
        else:
            new = factor * float(peak)
            if new < v:
                new, hold, factor = v, 0, PEAK_DECAY_RATE
            else:
                factor *= factor
        peak = new
        out.append(peak)
    return np.array(out)


@pytest.mark.parametrize("name", ["noise", "bursts", "impulse", "stereo", "irregular"])
def test_meters_match_reference(g, name):
    from friture_amd.levels import Levels
    x = H.signal(name)
    ref = g[f"meters_{name}"]
    lv = Levels()
    got = []
    for s, n in H.chunks(x.shape[1], H.IRREGULAR_CHUNKS if name == "irregular" else None):
        got.append(lv.handle_new_data(x[:, s:s + n]).copy())
    got = np.stack(got, axis=1)                       # [C, steps, 6]
    assert got.shape[:2] == ref.shape[:2]
    assert np.array_equal(got[..., 1], ref[..., 1])                                       # old_max
    assert np.max(np.abs(got[..., 3] - ref[..., 3])) <= 1e-12                              # level_max
    assert np.max(np.abs(got[..., 0] / ref[..., 0] - 1)) <= 1e-13                          # rms
    assert np.max(np.abs(got[..., 2] - ref[..., 2])) <= 1e-12
    assert np.array_equal(got[..., 5], ref[..., 5])                                       # ballistic branches
    assert np.max(np.abs(got[..., 4] - ref[..., 4])) <= 1e-12
    for c in range(x.shape[0]):
        assert np.array_equal(got[c, :, 4], _ballistic_replay(got[c, :, 2], got[c, :, 3]))


def test_rms_equals_exp_smooth_2d_bits():
    """Each chunk's smoothed RMS equals frt_exp_smooth_2d on the same chunk and previous value, bit for bit."""
    from friture_amd.levels import LevelsBatch
    from friture_amd.signal.exp_smoothing import exp_smoothed_value_2d
    x = H.signal("stereo")[:, :40 * H.CHUNK + 100]
    lb = LevelsBatch(2, 20)
    m, _ = lb.run(x, long=False)
    prev = np.full(2, 1e-30)
    for k, (s, n) in enumerate(H.chunks(x.shape[1])):
        want = exp_smoothed_value_2d(lb.kernel, lb.alpha, x[:, s:s + n] ** 2, prev)
        assert np.array_equal(m[:, k, 0], want), k
        prev = want


@pytest.mark.parametrize("name,rt", [("noise", 1), ("noise", 4), ("noise", 20), ("bursts", 4), ("impulse", 1), ("stereo", 20)])
def test_long_levels_match_reference(g, name, rt):
    from friture_amd.levels import LevelsBatch
    x = H.signal(name)[:1]
    lb = LevelsBatch(1, rt)
    _, lo = lb.run(x, meters=False)
    ref_lin, ref_db = g[f"long_{name}_rt{rt}_lin"], g[f"long_{name}_rt{rt}_db"]
    assert lo.shape[1] == ref_lin.shape[0]
    assert np.array_equal(lo[0, :, 0], ref_lin)
    assert np.max(np.abs(lo[0, :, 1] - ref_db)) <= 1e-12
    hist = lb.history(10)[0]
    assert np.array_equal(hist, lo[0, -10:, 1])


def test_long_levels_irregular_chunks(g):
    from friture_amd.longlevels import LongLevels
    x = H.signal("irregular")
    ll = LongLevels(1)
    db = [ll.handle_new_data(x[:, s:s + n])[0, :, 1] for s, n in H.chunks(x.shape[1], H.IRREGULAR_CHUNKS)]
    assert np.max(np.abs(np.concatenate(db) - g["long_irregular_rt1_db"])) <= 1e-12


@pytest.mark.parametrize("ndec", [8, 13])
def test_subsampler_matches_reference(g, ndec):
    from friture_amd.longlevels import Subsampler
    xs = H.signal("subsampler")
    sub = Subsampler(ndec)
    outs, pos = [], 0
    for n in H.SUBSAMPLER_PUSHES:
        outs.append(sub.push(xs[pos:pos + n]))
        pos += n
    assert [o.shape[0] for o in outs] == list(g[f"subsampler_{ndec}_lengths"])
    assert np.array_equal(np.concatenate(outs), g[f"subsampler_{ndec}"])


def test_curve_matches_reference(g):
    from friture_amd.longlevels import LongLevels
    x = H.signal("curve")
    ll = LongLevels(4)
    ll.setduration(30)
    pos, k = 0, 0
    for step, v in H.CURVE_STEPS:
        if step == "push":
            for _ in range(v):
                ll.handle_new_data(x[:, pos:pos + H.CHUNK])
                pos += H.CHUNK
            t, y = ll.curve()
            assert np.array_equal(t, g[f"curve_{k}_t"]), k
            assert np.max(np.abs(y - g[f"curve_{k}_y"])) <= 1e-12, k
            k += 1
        else:
            getattr(ll, step)(v)


def test_streaming_equals_batch():
    from friture_amd.levels import LevelsBatch
    rng = np.random.default_rng(7)
    x = 0.1 * rng.standard_normal((3, 200000))
    one = LevelsBatch(3, 1)
    m1, l1 = one.run(x)
    st = LevelsBatch(3, 1)
    ms, ls, pos = [], [], 0
    while pos < x.shape[1]:
        n = int(rng.integers(1, 20)) * H.CHUNK if rng.random() < 0.8 else int(rng.integers(0, 9000))
        n = min(n, x.shape[1] - pos)
        if n % H.CHUNK and pos + n < x.shape[1]:
            n -= n % H.CHUNK                       # meters: chunk boundaries must line up with the one-call run
        m, lo = st.run(x[:, pos:pos + n])
        ms.append(m)
        ls.append(lo)
        pos += n
    assert np.array_equal(np.concatenate(ms, axis=1), m1)
    assert np.array_equal(np.concatenate(ls, axis=1), l1)
    assert np.array_equal(st.get_state(), one.get_state())


def test_channels_independent_and_dtypes():
    from friture_amd.levels import LevelsBatch
    x = (0.2 * np.random.default_rng(8).standard_normal((64, 70000))).astype(np.float32)
    mb, lb = LevelsBatch(64, 4).run(x)
    md, ld = LevelsBatch(64, 4).run(x.astype(np.float64))
    assert np.array_equal(mb, md) and np.array_equal(lb, ld)
    for c in (0, 17, 63):
        m1, l1 = LevelsBatch(1, 4).run(x[c:c + 1])
        assert np.array_equal(m1[0], mb[c]) and np.array_equal(l1[0], lb[c])


def test_state_round_trip_mid_stream():
    from friture_amd.levels import LevelsBatch
    x = 0.1 * np.random.default_rng(9).standard_normal((2, 120000))
    a = LevelsBatch(2, 1)
    a.run(x[:, :50000])
    s = a.get_state()
    ma, la = a.run(x[:, 50000:])
    b = LevelsBatch(2, 1)
    b.set_state(s)
    mb, lb = b.run(x[:, 50000:])
    assert np.array_equal(ma, mb) and np.array_equal(la, lb)


def test_full_size_batch_matches_cpu():
    import torch
    from friture_amd.levels import LevelsBatch
    x = (0.1 * np.random.default_rng(10).standard_normal((8, 1 << 22)))
    lb = LevelsBatch(8, 20)
    m, lo = lb.run(torch.from_numpy(x).cuda())
    m, lo = m.cpu().numpy(), lo.cpu().numpy()
    for c in range(8):
        cpu = H.LongLevelsCPU(13)
        want = np.array([v for v, _ in cpu.push(x[c])])
        assert np.array_equal(lo[c, :, 0], want)
    peak = np.array([np.abs(x[0, s:s + n]).max() for s, n in H.chunks(x.shape[1])])
    om, prev = [], 1e-30
    for p in peak:
        prev = p if p > prev * (1. - lb.alpha2) else prev * (1. - lb.alpha2)
        om.append(prev)
    assert np.array_equal(m[0, :, 1], np.array(om))
