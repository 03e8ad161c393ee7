"""friture/iec.py: dB -> IEC 60268-18 meter deflection, scalar (the reference's branches) and vectorised (np.select over
the same branches, the same operations per element)."""
from __future__ import annotations

import numpy as np


def dB_to_IEC(dB):
    if np.ndim(dB) != 0:
        return dB_to_IEC_array(dB)
    if dB < -70.0:
        return 0.0
    elif dB < -60.0:
        return (dB + 70.0) * 0.0025
    elif dB < -50.0:
        return (dB + 60.0) * 0.005 + 0.025
    elif dB < -40.0:
        return (dB + 50.0) * 0.0075 + 0.075
    elif dB < -30.0:
        return (dB + 40.0) * 0.015 + 0.15
    elif dB < -20.0:
        return (dB + 30.0) * 0.02 + 0.3
    else:
        return (dB + 20.0) * 0.025 + 0.5


def dB_to_IEC_array(dB):
    d = np.asarray(dB, np.float64)
    conds = [d < -70.0, d < -60.0, d < -50.0, d < -40.0, d < -30.0, d < -20.0]
    vals = [np.zeros_like(d), (d + 70.0) * 0.0025, (d + 60.0) * 0.005 + 0.025, (d + 50.0) * 0.0075 + 0.075,
            (d + 40.0) * 0.015 + 0.15, (d + 30.0) * 0.02 + 0.3]
    return np.select(conds, vals, (d + 20.0) * 0.025 + 0.5)
