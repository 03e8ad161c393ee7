"""Record tests/golden/pitchbatch.npz: the unmodified reference's PitchTracker behind a reference RingBuffer, fed chunk by chunk
as the pitch widget feeds it, and oracle/pitchbatch.py's replay checked against it.  Driven by oracle/make_golden.py (needs the
reference checkout).

Per case of oracle.pitchbatch.golden_inputs and chunking of GOLDEN_CHUNKINGS, under `<case>_<chunking>_`: ends, fresh [chunks]
(what update() returned), windows [chunks, M] (get_estimates(duration) after every chunk), latest [refreshes]
(get_latest_estimate() after every refresh) and estimates [F] (the new tail of the window of every refresh, joined).  The one-row
inputs lie in pitch.npz: `<case>_x_key` names the array; the two-row inputs come from the seeded makers.
"""
from pathlib import Path

import numpy as np

from . import pitchbatch as H
from .golden_pitch import import_reference_pitch_tracker

GOLD = Path(__file__).resolve().parents[1] / "tests" / "golden"

TOL_F0 = 1e-9       # tests/test_pitch_gpu.py's rule (H.close): the voiced pattern identical, the rest within 1e-9 relative


def worst_of(a, b):
    """H.close's measure where the voiced patterns agree."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    m = ~np.isnan(a)
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m])), initial=0.0))


def record_case(pt, RingBuffer, x, ends):
    s = H.GOLDEN_SETTINGS
    ring = RingBuffer()
    tracker = pt.PitchTracker(ring, fft_size=s["fft_size"], overlap=s["overlap"])
    mine = H.WidgetReplay(**s)
    start, worst = 0, 0.0
    fresh, windows, latest, estimates = [], [], [], []
    for e in ends.tolist():
        ring.push(x[:, start:e], 0.)
        fresh.append(tracker.update())
        assert mine.push(x[:, start:e]) == fresh[-1], e
        windows.append(np.array(tracker.get_estimates(s["duration"]), np.float64))
        assert H.close(mine.get_estimates(), windows[-1], TOL_F0), e
        worst = max(worst, worst_of(mine.get_estimates(), windows[-1]))
        if fresh[-1]:
            latest.append(tracker.get_latest_estimate())
            assert H.close(mine.pitch[-1], latest[-1], TOL_F0), e
            estimates.append(windows[-1][len(windows[-1]) - (mine.frame_start[-1] - mine.frame_start[-2]):])
        start = e
    estimates = np.concatenate(estimates)
    assert H.close(np.array(mine.estimates), estimates, TOL_F0)
    assert len(estimates) == (x.shape[1] - s["fft_size"]) // mine.step + 1
    return dict(ends=ends.astype(np.int64), fresh=np.array(fresh, bool), windows=np.array(windows), latest=np.array(latest, np.float64),
                estimates=estimates), worst


def pitchbatch(out_dir):
    pt = import_reference_pitch_tracker()
    from friture.ringbuffer import RingBuffer
    out, worst = {}, 0.0
    with np.load(GOLD / "pitch.npz", allow_pickle=False) as z:
        inputs = H.golden_inputs({key: z[key] for key in H.GOLDEN_KEYS.values()})
    for name, x in inputs.items():
        if name in H.GOLDEN_KEYS:
            out[f"{name}_x_key"] = np.array(H.GOLDEN_KEYS[name])
        for chunking, ends_of in H.GOLDEN_CHUNKINGS.items():
            got, w = record_case(pt, RingBuffer, x, ends_of(x.shape[1]))
            worst = max(worst, w)
            out.update({f"{name}_{chunking}_{k}": v for k, v in got.items()})
    print(f"pitch replay vs the reference tracker fed chunk by chunk: worst relative difference {worst:.3e} (bound {TOL_F0})")
    np.savez_compressed(out_dir / "pitchbatch.npz", **out)
