"""The level tests' numpy restatement of what levels.hip computes, held to the reference's recorded values by
test_levels_edges_cpu.py before the GPU is held to it (test_levels_edges_gpu.py).  The product does not import it.

MetersCPU: one channel of Levels_Widget.handle_new_data, chunk by chunk (friture/levels.py:93-110, signal/exp_smoothing.py:40-56,
iec.py, ballistic_peak.py:41-66), NaN and Inf treated as numpy and Python treat them; rms_step, the same smoothing step with the
dot summed in extended precision.  LongLevelsRef: oracle.levels.LongLevelsCPU with setresptime's change of Ndec
(friture/longlevels.py:212-229).  seam_lengths: the tile plan of run_device restated from the constants levels.hip declares, and
the row lengths that put a seam of that plan where a test wants it."""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np

from oracle import levels as O

LEVELS_HIP = Path(__file__).resolve().parents[1] / "friture_amd" / "csrc" / "levels.hip"
PEAK_DECAY_RATE = (1.0 - 3E-6/500.)        # ballistic_peak.py:22
PEAK_FALLOFF = 32                          # ballistic_peak.py:24
FOLLOW, HOLD, DECAY, DECAY_FLOOR = 0, 1, 2, 3
EXTENDED = np.finfo(np.longdouble).nmant >= 63          # an 80-bit (or wider) long double; otherwise exact rationals


# ---- the meters -------------------------------------------------------------------------------------------------------------------

def ballistic_replay(levels_rms, levels_max):
    """(peak_iec, branch) per step of a fresh BallisticPeak fed dB_to_IEC(max(level_max, level_rms)) of each pair of dB values."""
    m = MetersCPU(0.0, np.zeros(1), 0.0)
    out = [m.ballistic(float(r), float(x)) for r, x in zip(levels_rms, levels_max)]
    return np.array([p for p, _ in out]), np.array([b for _, b in out], np.float64)


class MetersCPU:
    """One channel of the meters.  step(y) takes a chunk and returns [rms, old_max, level_rms, level_max, peak_iec, branch],
    the fields of FRT_LEVELS_METER_FIELDS."""

    def __init__(self, alpha, kernel, alpha2):
        self.alpha, self.kernel, self.alpha2 = float(alpha), np.asarray(kernel, np.float64), float(alpha2)
        self.old_rms = 1e-30
        self.old_max = 1e-30
        self.peak, self.hold, self.factor = 0, 0, PEAK_DECAY_RATE

    def decay(self, N):
        """exp_smoothing.py:43-47: (samples used, a)."""
        Nk = self.kernel.shape[0]
        return (Nk, 0.0) if N > Nk else (N, (1.0 - self.alpha) ** N)

    def exp_smoothed_value(self, data, previous):
        N, a = self.decay(data.shape[0])
        if N == 0:
            return previous
        Nk = self.kernel.shape[0]
        conv = np.dot(self.kernel[Nk - N:Nk], data[:N])
        return float(self.alpha * conv + previous * a)

    def rms_step(self, prev, y):
        """alpha S + prev a with S = sum_t y_t^2 kernel[Nk - N + t] in extended precision (exact products of exact squares when
        long double is no wider than double), the sum and the two products of the last line included; returned in that
        precision.  N == 0 returns prev."""
        y = np.asarray(y, np.float64)
        N, a = self.decay(y.shape[0])
        if N == 0:
            return prev
        k = self.kernel[self.kernel.shape[0] - N:]
        if EXTENDED:
            q = y[:N].astype(np.longdouble)
            p = (q * q) * k.astype(np.longdouble)
            hi = p.astype(np.float64)                                  # fsum is exact over doubles: the products in two parts
            lo = (p - hi.astype(np.longdouble)).astype(np.float64)
            S = np.longdouble(math.fsum(hi)) + np.longdouble(math.fsum(lo))
            return np.longdouble(self.alpha) * S + np.longdouble(prev) * np.longdouble(a)
        from fractions import Fraction
        S = sum((Fraction(float(v)) ** 2 * Fraction(float(c)) for v, c in zip(y[:N], k)), Fraction(0))
        return Fraction(self.alpha) * S + Fraction(float(prev)) * Fraction(a)

    def ballistic(self, level_rms, level_max):
        """One BallisticPeak step on the two dB values: (peak_iec, branch)."""
        from friture_amd.iec import dB_to_IEC
        v = dB_to_IEC(max(level_max, level_rms))
        if v > self.peak:
            new, self.hold, self.factor, branch = v, 0, PEAK_DECAY_RATE, FOLLOW
        elif self.hold + 1 <= PEAK_FALLOFF:
            new, self.hold, branch = self.peak, self.hold + 1, HOLD
        else:
            new = self.factor * float(self.peak)
            if new < v:
                new, self.hold, self.factor, branch = v, 0, PEAK_DECAY_RATE, DECAY_FLOOR
            else:
                self.factor *= self.factor
                branch = DECAY
        self.peak = new
        return float(new), float(branch)

    def step(self, y):
        y = np.asarray(y, np.float64)
        with np.errstate(all="ignore"):
            if len(y) > 0:
                value_max = float(np.abs(y).max())                     # NaN when any sample is: the comparison is then false
                if value_max > self.old_max * (1. - self.alpha2):
                    self.old_max = value_max
                else:
                    self.old_max *= (1. - self.alpha2)
            self.old_rms = self.exp_smoothed_value(y ** 2, self.old_rms)
            level_rms = float(10. * np.log10(self.old_rms + 0. * 1e-80))
            level_max = float(20. * np.log10(self.old_max + 0. * 1e-80))
            peak, branch = self.ballistic(level_rms, level_max)
        return np.array([self.old_rms, self.old_max, level_rms, level_max, peak, branch])

    def run(self, x, sizes):
        """[steps, 6] of the chunks of x [T] of the given sizes, one after the other."""
        rows, pos = [], 0
        for n in sizes:
            rows.append(self.step(x[pos:pos + n]))
            pos += n
        return np.array(rows).reshape(-1, 6)


def chunk_sizes(T, chunk):
    """The sizes of the chunks LevelsBatch cuts T samples into: a short last chunk is a short chunk."""
    return [min(chunk, T - s) for s in range(0, T, chunk)]


def db_close(got, want, tol=1e-12):
    """dB values agree: within tol where both are finite, the same infinity or both NaN elsewhere."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(got) & np.isfinite(want)
    return bool(got.shape == want.shape and np.array_equal(got[~fin], want[~fin], equal_nan=True) and
                np.all(np.abs(got[fin] - want[fin]) <= tol))


# ---- the long levels ----------------------------------------------------------------------------------------------------------------

class LongLevelsRef:
    """oracle.levels.LongLevelsCPU of one channel; set_ndec is setresptime: a new Subsampler, a zero FIR state, and the samples
    not yet consumed kept (they stay in the widget's audio buffer, and old_index with them)."""

    def __init__(self, ndec):
        self.cpu = O.LongLevelsCPU(ndec)

    @property
    def ndec(self):
        return self.cpu.ndec

    def set_ndec(self, ndec):
        self.cpu.ndec = int(ndec)
        self.cpu.sub = O.SubsamplerCPU(int(ndec))
        self.cpu.tail41 = np.zeros(40)

    def push(self, x):
        """x [n] raw samples -> [nb, 2] {level, dB} of the blocks they complete."""
        with np.errstate(all="ignore"):
            out = self.cpu.push(np.asarray(x, np.float64))
        return np.array(out, np.float64).reshape(-1, 2)

    def pending(self):
        return self.cpu.pending.shape[0] - (1 << 13)


# ---- the tile plan ------------------------------------------------------------------------------------------------------------------

def kernel_constants(text=None):
    """What levels.hip declares: kMaxNdec, kFrontJ (stage-S outputs per front workgroup), kFrontS (stages of the front), kThreads,
    and the two numbers of the tail's blocks per workgroup, Bt = max(bt_min, bt_span >> L)."""
    text = LEVELS_HIP.read_text() if text is None else text
    found = {name: int(v) for name, v in re.findall(r"constexpr\s+int\s+(kMaxNdec|kFrontJ|kFrontS|kThreads)\s*=\s*(\d+)\s*;", text)}
    assert set(found) == {"kMaxNdec", "kFrontJ", "kFrontS", "kThreads"}, f"levels.hip declares {sorted(found)}"
    bt = re.findall(r"p\.Bt\s*=\s*std::max\(\s*(\d+)\s*,\s*(\d+)\s*>>\s*L\s*\)\s*;", text)
    assert len(bt) == 1, "levels.hip: the tail's blocks per workgroup are no longer max(a, b >> L)"
    assert re.search(r"p\.S\s*=\s*std::min\(kFrontS,\s*h->ndec\)", text), "levels.hip: S is no longer min(kFrontS, Ndec)"
    found["bt_min"], found["bt_span"] = int(bt[0][0]), int(bt[0][1])
    return found


# the values the lengths below were worked out for: a retune has to come back here
EXPECTED_CONSTANTS = dict(kMaxNdec=13, kFrontJ=64, kFrontS=5, kThreads=256, bt_min=8, bt_span=2048)


def tile_plan(ndec, n_stage0):
    """run_device's plan for n_stage0 stage-0 inputs at Ndec: E (the stage lengths, E[s + 1] = ceil(E[s] / 2)), S, J, the front
    tiles and the outputs of the last one, and for Ndec > S: Bt, the tail tiles and the outputs of the last one."""
    k = kernel_constants()
    S = min(k["kFrontS"], ndec)
    E = [int(n_stage0)]
    for _ in range(ndec):
        E.append((E[-1] + 1) // 2)
    J = k["kFrontJ"]
    plan = dict(E=E, S=S, J=J, front_tiles=-(-E[S] // J), front_last=E[S] - (-(-E[S] // J) - 1) * J, Bt=None, tail_tiles=0,
                tail_last=0)
    if ndec > S:
        Bt = max(k["bt_min"], k["bt_span"] >> (ndec - S))
        plan.update(Bt=Bt, tail_tiles=-(-E[ndec] // Bt), tail_last=E[ndec] - (-(-E[ndec] // Bt) - 1) * Bt)
    return plan


def seam_lengths(ndec):
    """Row lengths in samples for Ndec, by the class each is named for (W = 2 Bt outputs, or 2 J at Ndec <= S where the front is
    the last kernel: two full tiles of the last kernel):
      levels      W + 2 blocks through frt_levels_run (a block is 2^Ndec samples; the first one is the zeros before the stream):
                  two full tiles of the last kernel and a third holding two blocks
      levels_one  one block less: the third tile holds one block
      odd         W 2^Ndec + 1 Subsampler inputs: every stage length is odd, the last tile of each kernel holds one output
      even        W 2^Ndec: every stage length is even, every tile is full
      short       W 2^Ndec - 1: only the stage-0 length is odd (E[s + 1] = ceil(E[s] / 2) gives back the even lengths from stage
                  1 on), so the first stage's carried inputs end one sample early and every tile is still full
      ragged      (W 2^(Ndec - S) - 1) 2^S: the front's last tile is one output short of full (E[S] = 63 mod J), the tail's
                  first stage has an odd length and its tiles are full"""
    k = kernel_constants()
    S = min(k["kFrontS"], ndec)
    W = 2 * k["kFrontJ"] if ndec <= S else 2 * max(k["bt_min"], k["bt_span"] >> (ndec - S))
    return dict(levels=((W + 1) << ndec) + (1 << ndec), levels_one=(W + 1) << ndec, odd=(W << ndec) + 1, even=W << ndec,
                short=(W << ndec) - 1, ragged=((W << (ndec - S)) - 1) << S)
