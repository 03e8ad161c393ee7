"""The plot-curve tests' comparison of a widget with tests/golden/plotcurves.npz, over the cases of oracle/plotcurves.py."""
from __future__ import annotations

import numpy as np

from oracle import plotcurves as H


def check_case(g, name, w, full_arrays=True):
    """Replay `name` on the widget-like `w` and compare with the recorded reference, refresh by refresh."""
    from friture_amd.plotting import frequency_scales as fscales
    hist = name.startswith("hist_")
    dig, drew, peakset, base = g[f"{name}_dig"], g[f"{name}_drew"], g[f"{name}_peakset"], g[f"{name}_baseline"]
    prev = (None, None)
    for k in H.replay(name, w, fscales):
        sig, pk = w.signal, w.peak
        assert (sig is not prev[0]) == bool(drew[k]), (name, k)
        assert (pk is not prev[1] and pk is not None) == bool(peakset[k]), (name, k)
        prev = (sig, pk)
        peak, pint, pdec = w.peak_state()
        got = [H.digest(sig[0]), H.digest(sig[1]), H.digest(sig[2]), H.digest(sig[3]),
               H.digest(pk[2] if pk else None), H.digest(pk[3] if pk else None), H.digest(peak), H.digest(pint),
               H.digest(pdec), H.digest(w.bar_labels[0] if hist else None)]
        assert got == list(dig[k]), (name, k, [f for f, a, b in zip(g["dig_fields"], got, dig[k]) if a != b])
        assert sig[4] == base[k] and type(sig[4]) is float
        if hist:
            assert np.array_equal(w.bar_labels[1], H.bands(int(name[len("hist_bpo"):]))[2]) and w.bar_labels[2] is sig[2]
        else:
            assert w.fmax_label[0] == g[f"{name}_fmax_text"][k] and w.fpitch_label[0] == g[f"{name}_fpitch_text"][k], (name, k)
            assert np.array_equal(w.fmax_label[1], g[f"{name}_fmax_pos"][k])
            assert np.array_equal(w.fpitch_label[1], g[f"{name}_fpitch_pos"][k])
        if full_arrays and k in H.FULL_REFRESHES.get(name, ()):
            for i, key in enumerate(("sxl", "sxr", "sy", "z")):
                assert np.array_equal(sig[i], g[f"{name}_full{k}_{key}"], equal_nan=True), (name, k, key)
            if f"{name}_full{k}_sp" in g.files:
                assert np.array_equal(pk[2], g[f"{name}_full{k}_sp"], equal_nan=True)
                assert np.array_equal(pk[3], g[f"{name}_full{k}_zp"])
            assert np.array_equal(np.array([peak, pint, pdec]), g[f"{name}_full{k}_state"], equal_nan=True)
