"""Record tests/golden/octavespectrumbatch.npz: the unmodified reference's OctaveSpectrum_Widget.handle_new_data
(friture/octavespectrum.py:91-122) fed chunks of mixed lengths from {256, 512, 768, 1024}, and oracle/octavespectrumbatch.py's
replay checked against it.  Driven by oracle/make_golden.py (needs the reference checkout).

Per (bpo, weighting) of oracle.octavespectrumbatch.GOLDEN_CASES, under `bpo<b>_w<w>_`: sp [chunks, 9 bpo] (the widget's dispbuffers
after every chunk) and db [chunks, 9 bpo] (what it hands to setdata); `ends` once.  The input is the seeded golden_input().
"""
import numpy as np

from . import octavespectrumbatch as H
from . import refshim

SP_BOUND, DB_BOUND = 8.3e-13, 1e-11     # sp relative (measured 8.3e-14, one decade over it); dB absolute (10 / ln 10 times it, rounded up)


def octavespectrumbatch(out_dir):
    refshim.install()
    refshim.blank("friture.histplot")
    refshim.module("friture.octavespectrum_settings", OctaveSpectrum_Settings_Dialog=refshim.Any, DEFAULT_SPEC_MIN=-80,
                   DEFAULT_SPEC_MAX=-20, DEFAULT_WEIGHTING=1, DEFAULT_BANDSPEROCTAVE=3, DEFAULT_RESPONSE_TIME=1.)
    from friture.octavespectrum import OctaveSpectrum_Widget
    x, ends = H.golden_input(), H.golden_ends()
    out, worst, worst_db = {"ends": ends}, 0.0, 0.0
    for bpo, weighting in H.GOLDEN_CASES:
        widget = OctaveSpectrum_Widget(None)
        widget.setbandsperoctave(bpo)
        widget.setweighting(weighting)
        shown, sps = [], []
        widget.PlotZoneSpect = type("Recorder", (), {"setdata": lambda self, flow, fhigh, f_nominal, db: shown.append(np.array(db))})()
        mine = H.WidgetReplay(bpo, weighting)
        start = 0
        for e in ends.tolist():
            widget.handle_new_data(x[None, start:e])
            sp, db = mine.push(x[start:e])
            start = e
            sps.append(np.array(widget.dispbuffers, np.float64))
            assert np.all(sps[-1] > 0)
            worst = max(worst, float(np.max(np.abs(sp - sps[-1]) / sps[-1])))
            worst_db = max(worst_db, float(np.max(np.abs(db - shown[-1]))))
        assert len(shown) == len(ends)
        out[f"bpo{bpo}_w{weighting}_sp"], out[f"bpo{bpo}_w{weighting}_db"] = np.array(sps), np.array(shown, np.float64)
    print(f"octave replay vs the reference widget: sp {worst:.3e} relative (bound {SP_BOUND}), dB {worst_db:.3e} (bound {DB_BOUND})")
    assert worst <= SP_BOUND and worst_db <= DB_BOUND
    np.savez_compressed(out_dir / "octavespectrumbatch.npz", **out)
