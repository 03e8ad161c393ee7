"""Record tests/golden/delaybatch.npz: the unmodified reference's Delay_Estimator_Widget.handle_new_data
(friture/delay_estimator.py:87-176) fed the seeded cases of oracle/delaybatch.py chunk by chunk, and that module's replay checked
against it.  Driven by oracle/make_golden.py (needs the reference checkout).

Per case of oracle.delaybatch.GOLDEN, under `<name>_`: delay_ms, distance_m, extremum (the widget's Xcorr_extremum) and correlation
[chunks] float64 (what the widget shows after every chunk), and old_Xcorr [L] (its smoothed correlation after the last one).
"""
import numpy as np

from . import delaybatch as H
from . import refshim


def delaybatch(out_dir):
    refshim.install()
    refshim.module("friture.delay_estimator_view_model", Delay_Estimator_View_Model=refshim.Any)
    from friture.delay_estimator import Delay_Estimator_Widget
    out = {}
    for name, (case, stream, _) in H.GOLDEN.items():
        delayrange = H.CASES[case][0]
        x, ends = H.signal(case)[stream], H.golden_ends(name)
        widget = Delay_Estimator_Widget(None)
        widget.set_delayrange(delayrange)
        rows, start = [], 0
        for e in ends.tolist():
            widget.handle_new_data(np.array(x[:, start:e]))
            start = e
            rows.append((widget.delay_ms, widget.distance_m, widget.Xcorr_extremum, widget.correlation))
        rows = np.array(rows, np.float64)
        old = np.array(widget.old_Xcorr, np.float64)
        mine = H.replay(x, delayrange, ends)
        assert np.array_equal(mine["shown"], rows) and np.array_equal(mine["smoothed"], old), name
        out.update({f"{name}_{column}": rows[:, k] for k, column in enumerate(H.COLUMNS)})
        out[f"{name}_old_Xcorr"] = old
    print(f"delay replay vs the reference widget: {len(H.GOLDEN)} cases identical")
    np.savez_compressed(out_dir / "delaybatch.npz", **out)
