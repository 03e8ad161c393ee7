"""ToneBatch (distortion.hip): THD, THD+N and harmonic levels of whole batches of tone recordings.

Shapes: (a) 8 x 2^22 float32, N 8192; (b) 64 x 2^20 float32, N 1024; (c) 1 x 2^24 float64, N 16384; hop N / 2, Kaiser 20, L = 8,
H = 10.  The recordings are unit sines (a different fundamental per stream) with harmonics 2, 3, 5 at 1e-3, 1e-5, 1e-4 and white
noise at 1e-8, made on the device.  Per shape: ToneBatch.run on a CUDA tensor between device events after a warm-up, median /
min / max of --reps calls, and one read of the samples as a share of the 8 TB/s HBM peak (a whole-call figure: two kernels per
slab, the tail copy and the staging of the outputs).  Beside it, same session, same data: what a user writes without the class,
torch.stft in float64 with the same window, then the scaling to Q, the arg-max over the search range, the lobe sums by gathers
and the residual through a scattered lobe mask, in torch on the device (its largest distance from the class's thdn_db is
reported).  Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FS = 48000
SHAPES = [("a", 8, 1 << 22, "float32", 8192), ("b", 64, 1 << 20, "float32", 1024), ("c", 1, 1 << 24, "float64", 16384)]


def torch_route(x, tb):
    """(P1, P_h with NaN for absent orders, R, kappa) [S, F, ..] of the rows x with the settings of the ToneBatch tb."""
    import torch
    N, L, H, ka, kb = tb.fft_size, tb.lobe, tb.harmonics, tb.ka, tb.kb
    klo, khi = int(tb.klo[0]), int(tb.khi[0])
    dev = x.device
    w = torch.as_tensor(tb.window, device=dev)
    X = torch.stft(x.double(), N, tb.hop, window=w, center=False, return_complex=True)
    Q = (X.real.square() + X.imag.square()).transpose(1, 2) * (2.0 / (N * float((tb.window ** 2).sum())))
    del X
    Q[..., 0] *= 0.5
    Q[..., -1] *= 0.5
    bins = Q.shape[-1]
    span = torch.arange(-L, L + 1, device=dev)
    c1 = klo + Q[..., klo:khi + 1].argmax(-1)
    idx = c1[..., None] + span
    lobe = Q.gather(-1, idx)
    P1 = lobe.sum(-1)
    kappa = (lobe * idx).sum(-1) / P1
    c = torch.round(torch.arange(2, H + 1, device=dev) * kappa[..., None]).long()
    below = torch.cat([c1[..., None], c[..., :-1]], -1) + L + 1
    idx_h = c[..., None] + span                                         # [S, F, H - 1, 2 L + 1]
    own = (idx_h >= below[..., None]) & ((c + L <= kb)[..., None])
    safe = idx_h.clamp(max=bins - 1)
    Ph = (Q[..., None, :].expand(*c.shape, bins).gather(-1, safe) * own).sum(-1)
    Ph = torch.where(c + L <= kb, Ph, torch.full_like(Ph, float("nan")))
    outside = torch.ones_like(Q, dtype=torch.bool)
    outside[..., :ka] = False
    outside[..., kb + 1:] = False
    outside.scatter_(-1, idx, False)
    # a bin that no present order owns is pointed at bin 0, which is outside the band anyway
    outside.scatter_(-1, torch.where(own, safe, torch.zeros_like(safe)).flatten(-2), False)
    R = (Q * outside).sum(-1)
    return P1, Ph, R, kappa


def thdn_db(P1, Ph, R):
    import torch
    return 10.0 * torch.log10((torch.nansum(Ph, -1) + R) / P1)


def recording(S, T, N, dtype, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(T, device=dev, dtype=torch.float64)
    kappa = (40.37 + 3.0 * torch.arange(S, device=dev, dtype=torch.float64))[:, None]
    x = torch.sin(2 * torch.pi * kappa / N * t + 0.3)
    for h, a in ((2, 1e-3), (3, 1e-5), (5, 1e-4)):
        x += a * torch.sin(2 * torch.pi * h * kappa / N * t + 0.7 * h)
    x += 1e-8 * torch.randn((S, T), device=dev, dtype=torch.float64, generator=g)
    return x.to(getattr(torch, dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--no-routes", action="store_true", help="ToneBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.distortion import ToneBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_tone", "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": []}
    for label, S, T, dtype, N in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = recording(S, T, N, dtype, "cuda")
        tb = ToneBatch(fft_size=N)
        out = tb.run(x)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: tb.run(x), a.reps)
        samples = x.numel() * x.element_size()
        row = {"shape": label, "streams": S, "samples": T, "dtype": dtype, "fft_size": N, "hop": tb.hop, "frames": int(out.fund.shape[1]),
               "reps": a.reps,
               "run": {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "algorithmic_bytes": samples,
                       "hbm_share": samples / med / HBM_PEAK},
               "thdn_db": [float(out.total.thdn_db.min()), float(out.total.thdn_db.max())], "n_valid": int(out.total.n_valid.sum())}
        if not a.no_routes:
            theirs = thdn_db(*torch_route(x, tb)[:3])
            torch.cuda.synchronize()
            row["torch_route_distance"] = {"thdn_db": float((theirs - out.thdn_db).abs().max())}
            del theirs
            med2, tmin, tmax = time_call(lambda: torch_route(x, tb), a.reps)
            row["torch_route"] = {"what": "torch.stft in float64 with the same window, then the scaling, the arg-max, the lobe sums by gathers and "
                                          "the residual through a scattered mask, in torch on the device",
                                  "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
            row["torch_route_over_tone_batch"] = med2 / med
        res["shapes"].append(row)
        del x, out
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
