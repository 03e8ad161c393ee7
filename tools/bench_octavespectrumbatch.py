"""OctaveSpectrumBatch (octspecbatch.hip): whole recordings through the octave-spectrum widget's chain.

Shapes: (a) 8 streams x 2^22 float32 samples at 3 bands per octave; (b) 64 streams x 2^20 at 3; (c) 8 streams x 2^20 at 24; all at
512-sample chunks.  Per shape, in one session on the same data: the batch call (device events around OctaveSpectrumBatch.run on a
CUDA tensor after a warm-up, median / min / max of --reps) and what the bank offered before it, FirBank.energies(x, 512, alphas,
weight_db, as_db=True) — float32 in and out, blocks of 512, the state inside the handle.  `ratio` is batch median over energies
median, `energies_spread` is (max - min) / median of the energies call: the expectation under test is ratio - 1 <= that spread
(the batch costs that call plus a block axis twice as fine and float64 rows).  Prints one JSON line and writes it to --out when
given.  A per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool with --batch-only."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from benchutil import emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("a", 8, 1 << 22, 3), ("b", 64, 1 << 20, 3), ("c", 8, 1 << 20, 24)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.filter import FirBank
    from friture_amd.octavespectrum import OctaveSpectrumBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_octavespectrumbatch", "chunk": 512, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, bpo in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, T), device="cuda", dtype=torch.float32, generator=g)
        ob = OctaveSpectrumBatch(bpo)
        r = ob.run(x)
        torch.cuda.synchronize()
        R = r.db.shape[1]
        del r
        med, tmin, tmax = time_call(lambda: ob.run(x), a.reps)
        row = {"shape": label, "streams": S, "samples": T, "bands_per_octave": bpo, "refreshes": R, "slabs": ob.last_slabs,
               "batch_median_ms": med * 1e3, "batch_min_ms": tmin * 1e3, "batch_max_ms": tmax * 1e3, "reps": a.reps}
        if not a.batch_only:
            bank = FirBank(bpo, S)
            out = torch.empty((S, T // 512, 9 * bpo), dtype=torch.float32, device="cuda")
            call = lambda: bank.energies(x, 512, ob.alphas, weight_db=ob.w, as_db=True, out=out)       # noqa: E731
            call()
            torch.cuda.synchronize()
            emed, emin, emax = time_call(call, a.reps)
            row.update({"energies_median_ms": emed * 1e3, "energies_min_ms": emin * 1e3, "energies_max_ms": emax * 1e3,
                        "ratio": med / emed, "energies_spread": (emax - emin) / emed,
                        "within_spread": bool(med / emed - 1.0 <= (emax - emin) / emed)})
            del bank, out
        res["shapes"].append(row)
        del x, ob
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
