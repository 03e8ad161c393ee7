"""Record tests/golden/delaybatch.npy: the unmodified reference Delay_Estimator_Widget (friture/delay_estimator.py:87-176) fed
the seeded cases of tests/delaybatch_replay.py chunk by chunk.  Needs the reference checkout (oracle/refshim.py).

Per case of delaybatch_replay.GOLDEN, under `<name>_`: delay_ms, distance_m, Xcorr_extremum (as `extremum`) and correlation
after every chunk, and the final old_Xcorr, packed into one float64 vector (delaybatch_replay.golden_layout).  --check writes
nothing and compares with the committed file instead.

    python tools/record_delaybatch_golden.py [--check]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import delaybatch_replay as H  # noqa: E402
from oracle import refshim  # noqa: E402

TARGET = ROOT / "tests" / "golden" / "delaybatch.npy"


def record():
    refshim.install()
    refshim.module("friture.delay_estimator_view_model", Delay_Estimator_View_Model=refshim.Any)
    from friture.delay_estimator import Delay_Estimator_Widget
    out = {}
    for name, (case, stream, ends) in H.GOLDEN.items():
        delayrange, T = H.CASES[case][:2]
        x = H.signal(case)[stream]
        ends = H.golden_ends(name)
        widget = Delay_Estimator_Widget(None)
        widget.set_delayrange(delayrange)
        rows, start = [], 0
        for e in ends.tolist():
            widget.handle_new_data(np.array(x[:, start:e]))
            start = e
            rows.append((widget.delay_ms, widget.distance_m, widget.Xcorr_extremum, widget.correlation))
        rows = np.array(rows, np.float64)
        for k, column in enumerate(("delay_ms", "distance_m", "extremum", "correlation")):
            out[f"{name}_{column}"] = rows[:, k]
        out[f"{name}_old_Xcorr"] = np.array(widget.old_Xcorr, np.float64)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    out = record()
    if args.check:
        held = H.golden_unpack(np.load(TARGET, allow_pickle=False))
        bad = [k for k in held if not np.array_equal(out[k], held[k])]
        print(f"{TARGET.name}: {len(held)} arrays, {len(bad)} differ {bad}")
        return 1 if bad else 0
    np.save(TARGET, H.golden_pack(out))
    print(f"wrote {TARGET} ({TARGET.stat().st_size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
