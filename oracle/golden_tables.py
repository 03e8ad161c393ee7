"""Extract the reference's published filter-design numbers: octave_filters.npz and filter_tables.sha256.

The octave-bank coefficients are part of the reference's contract: every parity target is defined
with exactly these numbers (friture/generated_filters.py JSON, friture/data/generated_fft.npz).
friture_amd/filter_design.py re-derives the same designs, but scipy's elliptic design routines
changed between the version upstream used and the one installed here, so the re-derived values
differ by 1e-5 .. 3e-3 (relative) — far more than the 1e-5 parity tolerance on band energies.
The shipped table (friture_amd/data/octave_filters.npz) therefore holds the reference's numbers
verbatim (values only, no code), its per-array digest sits next to the golden fixtures
(tests/golden/filter_tables.sha256), and tests/test_filter_tables.py keeps the re-derivation honest.

Driven by oracle/make_golden.py (needs the reference checkout, see oracle/refshim.py).
"""
import hashlib
import json
import re
from pathlib import Path

import numpy as np

from . import dsp, refshim
from .golden_dsp import same


def filter_tables(out_dir):
    ref = Path(refshim.REFERENCE_ROOT) / "friture"
    text = (ref / "generated_filters.py").read_text()
    params = json.loads(re.search(r'JSON_PARAMS = """(.*?)"""', text, re.S).group(1))
    fft = np.load(ref / "data" / "generated_fft.npz")

    out = {
        "bdec": np.asarray(params["dec"][0], float),
        "adec": np.asarray(params["dec"][1], float),
        "bdec_fir": np.asarray(fft["bdec_fir"], float),
    }
    sizes = None
    for bpo in (1, 3, 6, 12, 24):
        boct, aoct, fi, flow, fhigh = params[str(bpo)]
        out[f"boct_{bpo}"] = np.asarray(boct, float)
        out[f"aoct_{bpo}"] = np.asarray(aoct, float)
        out[f"boct_fir_{bpo}"] = np.asarray(fft[f"{bpo}_boct_fir"], float)
        s = np.asarray(fft[f"{bpo}_fft_sizes"], np.int64)
        assert sizes is None or (s == sizes).all()
        sizes = s
    out["fft_sizes"] = sizes
    np.savez_compressed(out_dir / "octave_filters.npz", **out)
    digest = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(out.items())}
    (out_dir / "filter_tables.sha256").write_text("".join(f"{v}  {k}\n" for k, v in digest.items()))

    # the table the oracle loads against the reference's design artefacts
    tabs = dsp.load_filter_tables()
    for bpo in (1, 3, 6, 12, 24):
        same(f"boct_fir table {bpo}", tabs[f"boct_fir_{bpo}"], fft[f"{bpo}_boct_fir"])
        H = np.fft.rfft(tabs[f"boct_fir_{bpo}"], int(tabs["fft_sizes"][0]), axis=1)
        same(f"H_oct stage 0 {bpo}", H, fft[f"{bpo}_fft_H_oct"][0][:, :H.shape[1]], tol=1e-13)
    same("bdec_fir table", tabs["bdec_fir"], fft["bdec_fir"])
