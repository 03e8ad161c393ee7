"""oracle/make_golden.py — record the golden fixtures from the unmodified reference, or check the committed ones.

Run in the build container (needs the reference checkout, see oracle/refshim.py):

    python -m oracle.make_golden [name ...]            # record into tests/golden/ (and friture_amd/data/ for the filter tables)
    python -m oracle.make_golden --check [name ...]    # record into a temporary directory, compare with the committed files

Without names: every fixture of RECORDERS.  A recorder is a function `name(out_dir)` of one of the oracle/golden_*.py
modules; it runs the reference's own code, checks oracle/dsp.py against it where the oracle restates it, and writes
`name.npz` into out_dir, or, where one file would be too large, one file per case into out_dir/name/ (`files(name)`).  The stand-ins that the recorders put into sys.modules conflict with each other, so every module
runs in a child process of its own (`--into`), all of them at once.  --check compares arrays, not file bytes (an .npz is a
zip with time stamps): the same array names, and per array the same dtype, the same shape and equal values (NaNs equal NaNs);
it prints one line per fixture (`name (K files): ...` for a folder of case files) and exits non-zero on any difference, on a
recorder that fails, and on an .npz under tests/golden/, subfolders included, that no recorder writes.
"""
from __future__ import annotations

import argparse
import importlib
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import refshim

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
RECORDERS = {       # module -> the fixtures it records
    "golden_dsp": ("psd", "image", "pipeline", "exp_smoothing", "spectrum", "iir", "ola", "gcc", "ring"),
    "golden_pitch": ("pitch",),
    "golden_levels": ("levels",),
    "golden_scope": ("scope",),
    "golden_plotcurves": ("plotcurves",),
    "golden_spectrogrambatch": ("spectrogrambatch",),
    "golden_pitchbatch": ("pitchbatch",),
    "golden_octavespectrumbatch": ("octavespectrumbatch",),
    "golden_delaybatch": ("delaybatch",),
    "golden_tables": ("filter_tables",),
}


def files(name):
    """Where the files that recorder `name` writes are committed."""
    if name == "filter_tables":
        return [ROOT / "friture_amd" / "data" / "octave_filters.npz", GOLD / "filter_tables.sha256"]
    if name == "spectrogrambatch":      # one file per case: together they would pass the size limit of a committed file
        from .spectrogrambatch import GOLDEN_CASES, GOLDEN_FOLDER
        return [GOLD / GOLDEN_FOLDER / f"{case}.npz" for case in GOLDEN_CASES]
    return [GOLD / f"{name}.npz"]


def recorded(f, out_dir):
    """Where the recorder leaves committed file f below its out_dir: by name, a file of a subfolder of tests/golden/ in that subfolder."""
    return Path(out_dir) / (f.relative_to(GOLD) if GOLD in f.parents else f.name)


def load(path):
    if path.suffix == ".npz":
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    return {k: np.array(v) for v, k in (line.split("  ") for line in path.read_text().splitlines())}      # sha256 lines


def difference(new, old):
    """The first difference between the recorded and the committed arrays, None if there is none."""
    if set(new) != set(old):
        return f"array names differ: recorded only {sorted(set(new) - set(old))}, committed only {sorted(set(old) - set(new))}"
    for k in sorted(old):
        a, b = new[k], old[k]
        if (a.dtype, a.shape) != (b.dtype, b.shape):
            return f"{k}: recorded {a.dtype} {a.shape}, committed {b.dtype} {b.shape}"
        if not np.array_equal(a, b, equal_nan=a.dtype.kind in "fc"):
            return f"{k}: values differ"
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of replacing them")
    ap.add_argument("--into", type=Path, metavar="DIR", help="record in this process into DIR (names of one module only)")
    ap.add_argument("names", nargs="*")
    args = ap.parse_args()
    module_of = {name: module for module, names in RECORDERS.items() for name in names}
    names = args.names or list(module_of)
    if set(names) - set(module_of):
        ap.error(f"no recorder for {sorted(set(names) - set(module_of))}; there are {list(module_of)}")
    if not refshim.available():
        sys.exit(f"reference checkout not found at {refshim.REFERENCE_ROOT}")
    if args.into:
        for name in names:
            getattr(importlib.import_module(f"oracle.{module_of[name]}"), name)(args.into)
        return 0

    def record(module):
        mine = [n for n in names if module_of[n] == module]
        return mine, subprocess.run([sys.executable, "-m", "oracle.make_golden", "--into", tmp, *mine], cwd=ROOT, text=True,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT)

    failed = []
    if not args.names:
        owned = {f for name in module_of for f in files(name)}
        failed = sorted(str(p.relative_to(GOLD).with_suffix("")) for p in GOLD.rglob("*.npz") if p not in owned)
        for name in failed:
            print(f"{name}: committed, but no recorder writes it")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor() as pool:
        for mine, child in pool.map(record, dict.fromkeys(module_of[n] for n in names)):
            if child.returncode or not args.check:
                print(child.stdout, end="")
            for name in mine:
                pairs = [(recorded(f, tmp), f) for f in files(name)]
                problem = None
                if child.returncode or not all(new.exists() for new, _ in pairs):
                    problem = f"recorder failed (exit status {child.returncode})"
                elif args.check:
                    problem = next((f"{old.name}: {d}" for new, old in pairs if (d := difference(load(new), load(old)))), None)
                    done = f"{sum(len(load(old)) for _, old in pairs if old.suffix == '.npz')} arrays identical"
                else:
                    for new, old in pairs:
                        shutil.copyfile(new, old)
                    done = "written to " + ", ".join(str(old.relative_to(ROOT)) for _, old in pairs)
                label = name if pairs[0][1].parent.parent != GOLD else f"{name} ({len(pairs)} files)"      # a folder of case files
                print(f"{label}: {problem or done}")
                if problem:
                    failed.append(name)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
