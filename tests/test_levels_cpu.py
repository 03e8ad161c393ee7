"""The level meters and long-time levels without a GPU: the raw-input tap-sum form the kernels rest on, dB_to_IEC, and the
host coefficient derivation, against tests/golden/levels.npz (recorded from the reference widgets)."""
import hashlib
from pathlib import Path

import numpy as np
import pytest

from oracle import levels as H

GOLDEN = Path(__file__).resolve().parent / "golden" / "levels.npz"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,rt", [("noise", 1), ("noise", 4), ("noise", 20), ("bursts", 4), ("impulse", 1), ("stereo", 20)])
def test_tapsum_long_levels_equal_reference_bits(g, name, rt):
    """y^2 -> Ndec x (tap sum, [::2]) -> 41-tap tap sum equals the reference's DF2T lfilter chain bit for bit."""
    from friture_amd.levels import ndec_for
    x = H.signal(name)[0]
    ll = H.LongLevelsCPU(ndec_for(rt))
    B = 1 << ll.ndec
    got = []
    for s in range(0, x.shape[0] - B + 1, B):
        got += ll.push(x[s:s + B])
    lin = np.array([v for v, _ in got])
    db = np.array([d for _, d in got])
    assert np.array_equal(lin, g[f"long_{name}_rt{rt}_lin"])
    assert np.array_equal(db, g[f"long_{name}_rt{rt}_db"])


def test_tapsum_long_levels_irregular_chunks(g):
    x = H.signal("irregular")[0]
    ll = H.LongLevelsCPU(8)
    got = []
    for s, n in H.chunks(x.shape[0], H.IRREGULAR_CHUNKS):
        got += ll.push(x[s:s + n])
    assert np.array_equal(np.array([d for _, d in got]), g["long_irregular_rt1_db"])


@pytest.mark.parametrize("ndec", [8, 13])
def test_tapsum_subsampler_equals_reference_bits(g, ndec):
    """Pushes of irregular sizes (0, fewer than 11, odd): [::2] keeps index 0 of each push at every stage."""
    xs = H.signal("subsampler")
    sub = H.SubsamplerCPU(ndec)
    outs, pos = [], 0
    for n in H.SUBSAMPLER_PUSHES:
        outs.append(sub.push(xs[pos:pos + n]))
        pos += n
    assert [o.shape[0] for o in outs] == list(g[f"subsampler_{ndec}_lengths"])
    assert np.array_equal(np.concatenate(outs), g[f"subsampler_{ndec}"])


def _iec_ref(dB):      # friture/iec.py restated branch by branch
    for lo, off, k, c in [(-70.0, None, None, None), (-60.0, 70.0, 0.0025, 0.0), (-50.0, 60.0, 0.005, 0.025),
                          (-40.0, 50.0, 0.0075, 0.075), (-30.0, 40.0, 0.015, 0.15), (-20.0, 30.0, 0.02, 0.3)]:
        if dB < lo:
            return 0.0 if off is None else ((dB + off) * k + c if c else (dB + off) * k)
    return (dB + 20.0) * 0.025 + 0.5


def test_db_to_iec_breakpoints():
    from friture_amd.iec import dB_to_IEC
    pts = []
    for b in (-70.0, -60.0, -50.0, -40.0, -30.0, -20.0, 0.0):
        pts += [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf), b - 0.5, b + 0.5]
    pts += [-np.inf, -300.0, 6.0]
    for p in pts:
        assert dB_to_IEC(p) == _iec_ref(p), p
    assert np.array_equal(dB_to_IEC(np.array(pts)), np.array([_iec_ref(p) for p in pts]))
    # the curve is continuous at every breakpoint to within a few ulps
    for b in (-70.0, -60.0, -50.0, -40.0, -30.0, -20.0):
        assert abs(dB_to_IEC(b) - dB_to_IEC(np.nextafter(b, -np.inf))) < 1e-12
    assert dB_to_IEC(-60.0) == 0.025 and dB_to_IEC(-20.0) == 0.5 and dB_to_IEC(-70.5) == 0.0


def test_coefficients_equal_reference_bits(g):
    from friture_amd.levels import meter_coefficients, ndec_for
    from friture_amd.longlevels import gauss
    alpha, kernel, alpha2 = meter_coefficients()
    assert alpha == g["alpha"] and alpha2 == g["alpha2"]
    assert kernel.shape[0] == int(g["kernel_len"])
    assert hashlib.sha256(kernel.tobytes()).hexdigest() == str(g["kernel_sha256"])
    assert np.array_equal(kernel[:16], g["kernel_head"]) and np.array_equal(kernel[-600:], g["kernel_tail"])
    assert np.array_equal(np.array(gauss(11, 2.)), g["gauss11"]) and np.array_equal(np.array(gauss(41, 8.)), g["gauss41"])
    assert [ndec_for(rt) for rt in range(1, 21)] == list(g["ndec_rt1_20"])


def test_levels_entry_points_bound():
    from friture_amd import _lib
    for name in ("frt_levels_create", "frt_levels_run", "frt_levels_push", "frt_levels_subsample", "frt_levels_history",
                 "frt_levels_get_state", "frt_levels_set_state", "frt_levels_state_length"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
