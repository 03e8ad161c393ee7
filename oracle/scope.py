"""The oscilloscope's cases and CPU restatement, shared by oracle/golden_scope.py and the scope tests: the fixture's cases (signals regenerated from seeds, never stored;
chunk schedules; timerange schedules) and a numpy restatement of Scope_Widget.handle_new_data (friture/scope.py:78-135) over
the zero-padded stream, the form the kernels compute (friture_amd/csrc/scope.hip)."""
from __future__ import annotations

import hashlib

import numpy as np

from .cases import CHUNK, FS, chunk_ends  # noqa: F401  (chunk_ends: used by the tests)

NO_TRIGGER = -(1 << 63)
IRREGULAR_CHUNKS = [512, 0, 7, 1, 10, 513, 2048, 0, 300, 4099, 1, 8192, 65, 11, 9000, 512, 0, 3, 255, 1024, 333, 6000, 2,
                    512, 777, 5000, 64, 128, 3000]
TIMERANGES = [0.1, 1, 10.9, 25.3, 50, 500, 500.1, 2000]
# timerange changes mid-stream: (refresh index, timerange); at refresh 38 the stream is at 20 000 samples and data(2 w = 19 200)
# grows the ring from 10 000 to 28 800, after which the window is not the zero-padded stream for a while
CHANGE_SCHEDULE = [(0, 50), (10, 10.9), (20, 25.3), (38, 200), (46, 500.1), (52, 50), (60, 1)]
CHANGE_CHUNKS = [CHUNK] * 38 + [544] + [CHUNK] * 40               # 38 x 512 + 544 = 20 000 at refresh 38
# channels of each chunk of the mono -> stereo -> mono case
SWITCH_ROWS = [1] * 30 + [2] * 40 + [1] * 20


def width_for(timerange):
    time = timerange * 1e-3
    return int(time * FS)


def trace_length(width, scrolling):
    return width if scrolling else 2 * (width // 2)


def scaled_t(width, timerange, length):
    time = (np.arange(length) - width // 2) / float(FS)
    return (time * 1e3 + timerange / 2.) / timerange


def tone_noise(T, seed, rows=2):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / FS
    x = np.stack([0.5 * np.sin(2 * np.pi * 441. * t + 0.3) + 0.05 * rng.standard_normal(T),
                  0.3 * np.sin(2 * np.pi * 660. * t) + 0.05 * rng.standard_normal(T)])
    return x[:rows]


def exact_level_values(f32=False):
    """(m, a, b): a peak m and a rising pair a -> b that crosses the reference's level (m * 2.) / 3. in float64 and not a
    level rounded otherwise.  float64: a = m * (2. / 3.) < b = (m * 2.) / 3., so the other rounding crosses one sample
    earlier (0 -> a).  float32 (every value a float32 number): a < (m * 2.) / 3. < b are the float32 neighbours of the level
    and the level rounded to float32 is a, so a float32 level crosses one sample earlier too."""
    for k in range(1, 1 << 16):
        if f32:
            m = float(np.float32(0.5 + k / 131072.))
            lev = (m * 2.) / 3.
            a = float(np.float32(lev))
            if a < lev:
                return m, a, float(np.nextafter(np.float32(a), np.float32(1)))
        else:
            m = 0.5 + k / 131072. + 1e-9
            lev, other = (m * 2.) / 3., m * (2. / 3.)
            if other < lev:
                return m, other, lev
    raise AssertionError("no such peak")


def exact_level_signal(f32=False, T=24 * CHUNK, period=300):
    """Zeros, then per period the rising pair a -> b and later the peak m."""
    m, a, b = exact_level_values(f32)
    x = np.zeros((1, T))
    for p in range(0, T - period, period):
        x[0, p + 50] = a
        x[0, p + 51] = b
        x[0, p + 150] = m
    return x


def signal(name):
    """[rows, T] float64 of one case's signal (the float32 case's values are float32 numbers)."""
    if name == "stereo":
        return tone_noise(96 * CHUNK, 11)
    if name == "noise":
        return 0.2 * np.random.default_rng(12).standard_normal((1, 96 * CHUNK))
    if name == "silence_tone":
        x = np.zeros((1, 96 * CHUNK))
        x[0, 48 * CHUNK:] = tone_noise(48 * CHUNK, 13, 1)[0]
        return x
    if name == "impulses":
        x = np.zeros((1, 96 * CHUNK))
        for pos, a in [(3000, 0.8), (17000, 0.8), (17005, 0.4), (30000, 0.9), (40000, -0.5)]:
            x[0, pos] = a
        return x
    if name == "nan_burst":
        x = tone_noise(96 * CHUNK, 14, 1)
        x[0, 20000:20005] = np.nan
        return x
    if name == "exact_level":
        return exact_level_signal()
    if name == "exact_level_f32":
        return exact_level_signal(True)
    if name.startswith("tr_"):
        return tone_noise(112 * CHUNK, 15)
    if name == "change":
        return tone_noise(sum(CHANGE_CHUNKS), 16)
    if name == "switch":
        return tone_noise(CHUNK * len(SWITCH_ROWS), 17)
    if name == "irregular":
        return tone_noise(sum(IRREGULAR_CHUNKS), 18)
    raise KeyError(name)


CASES = ["stereo", "noise", "silence_tone", "impulses", "nan_burst", "exact_level", "exact_level_f32"] + \
        [f"tr_{t}" for t in TIMERANGES] + ["change", "switch", "irregular"]
# refreshes whose setData arrays are stored whole: change 38 is the refresh whose data(19 200) grows the ring (its region is
# zeros: no trigger), 46 scrolls over a window the growth left apart from the stream
FULL_REFRESHES = {"stereo": [5], "exact_level": [5], "exact_level_f32": [5], "tr_25.3": [7], "change": [38, 46]}


def schedule(name):
    """[(start, length, rows, timerange)] of the refreshes of a case: a chunk of `length` samples of `rows` channels from
    `start` is pushed, the timerange is set, then handle_new_data runs."""
    x = signal(name)
    if name == "change":
        sizes = CHANGE_CHUNKS
    elif name == "irregular":
        sizes = IRREGULAR_CHUNKS
    else:
        sizes = [CHUNK] * (x.shape[1] // CHUNK)
    out, s, tr = [], 0, 50
    changes = dict(CHANGE_SCHEDULE) if name == "change" else {}
    for k, n in enumerate(sizes):
        rows = SWITCH_ROWS[k] if name == "switch" else x.shape[0]
        tr = changes.get(k, tr)
        if name.startswith("tr_"):
            tr = float(name[3:]) if "." in name[3:] else int(name[3:])
        out.append((s, n, rows, tr))
        s += n
    return out


def expected_window(name, k, length):
    """The zero-padded stream's last `length` samples at refresh k ([rows, length]): what a ring that lost nothing holds.
    A change of the channel count starts the ring afresh (ringbuffer.py:40-42): zeros before it."""
    sched = schedule(name)
    x = signal(name)
    s, n, rows, _ = sched[k]
    e = s + n
    first = k
    while first > 0 and sched[first - 1][2] == rows:
        first -= 1
    reset = sched[first][0]
    out = np.zeros((rows, length))
    lo = max(e - length, reset)
    if e > lo:
        out[:, length - (e - lo):] = x[:rows, lo:e]
    return out


def refresh_np(window, width, scrolling):
    """scope.py:78-112 on a [rows, 2w] (trigger) or [rows, w] (scrolling) window: the start of the trace in the window, or
    NO_TRIGGER."""
    if scrolling:
        return 0
    triggerdata = window[0, width // 2:-width // 2]
    trigger_level = triggerdata.max() * 2. / 3.
    pos = np.where((triggerdata[:-1] < trigger_level) * (triggerdata[1:] >= trigger_level))[0]
    if len(pos) == 0:
        return NO_TRIGGER
    return int(pos[0])


def batch_np(row0, ends, width, scrolling):
    """Absolute trace starts of refreshes at `ends` over one zero-padded stream row."""
    n = 2 * width if not scrolling else width
    out = []
    for e in ends:
        win = np.zeros((1, n))
        lo = max(e - n, 0)
        if e > lo:
            win[0, n - (e - lo):] = row0[lo:e]
        r = refresh_np(win, width, scrolling)
        out.append(NO_TRIGGER if r == NO_TRIGGER else int(e) - n + r)
    return np.array(out, np.int64)


def digest(a):
    """First 8 bytes of the SHA-256 of a float64 array's bytes, as uint64."""
    b = hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).digest()
    return np.frombuffer(b[:8], np.uint64)[0]
