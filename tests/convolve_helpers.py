"""The numpy restatement of X2 (include/friture_hip.h): the convolution itself, the emitted counts and the state layout.
Nothing here knows about partitions or transforms: y[t] = sum_l h[l] x[t - l], by np.convolve in float64 and, for the small
shapes, as a direct sum in np.longdouble."""
import numpy as np

MIN_BLOCK, MAX_BLOCK = 64, 4096


def default_block(L):
    b = MIN_BLOCK
    while b < L and b < MAX_BLOCK:
        b *= 2
    return b


def partitions(L, block):
    return -(-L // block)


def emitted_after(n, L, block, flushed=False):
    """The outputs a stream has emitted after n samples in total."""
    return n + L - 1 if flushed else (n // block) * block


def state_start(n, L, block):
    return max(0, (n // block - partitions(L, block)) * block)


def state_after(x, L, block):
    """The carried samples after all of x [S, n]: float64 [S, ..]."""
    x = np.atleast_2d(x)
    return np.asarray(x[:, state_start(x.shape[1], L, block):], np.float64)


def rows_of(x, h):
    x = np.atleast_2d(np.asarray(x))
    h = np.asarray(h, np.float64)
    h = np.broadcast_to(h, (x.shape[0], h.shape[-1])) if h.ndim == 1 else h
    assert h.shape[0] == x.shape[0]
    return x, h


def restate(x, h):
    """np.convolve per row in float64: [S, T + L - 1]."""
    x, h = rows_of(x, h)
    return np.stack([np.convolve(xs.astype(np.float64), hs) for xs, hs in zip(x, h)])


def restate_long(x, h):
    """The direct sum per row in np.longdouble: [S, T + L - 1] (small shapes: T L multiplications per row)."""
    x, h = rows_of(x, h)
    S, T = x.shape
    L = h.shape[1]
    out = np.zeros((S, T + L - 1), np.longdouble)
    xl, hl = x.astype(np.longdouble), h.astype(np.longdouble)
    for l in range(L):
        out[:, l:l + T] += hl[:, l:l + 1] * xl
    return out


def scale(x, h):
    """max|x| sum|h| per row [S, 1]: the natural scale of a convolution's rounding error."""
    x, h = rows_of(x, h)
    return (np.max(np.abs(x.astype(np.float64)), axis=1, initial=0.0) * np.sum(np.abs(h), axis=1))[:, None]


def distance(y, x, h, ref=None):
    """max |y - ref| / (max|x| sum|h|) over all rows (rows of scale 0 must be exact zeros)."""
    ref = restate(x, h) if ref is None else ref
    y = np.atleast_2d(np.asarray(y)).astype(ref.dtype)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    sc = scale(x, h)
    err = np.max(np.abs(y - ref), axis=1, initial=0.0)[:, None]
    assert np.all(err[sc == 0] == 0)
    return float(np.max(np.where(sc > 0, err / np.where(sc > 0, sc, 1), 0.0), initial=0.0))


BAR = 1e-12          # of max|x| sum|h| per row: the package's float64 bar on the natural scale of a convolution


def signal(seed, S, T, dtype=np.float64):
    x = np.random.default_rng(seed).standard_normal((S, T)).astype(dtype)
    x.setflags(write=False)
    return x


def taps(seed, L, S=None):
    """A decaying random response: [L], or [S, L]."""
    rng = np.random.default_rng(1000 + seed)
    h = rng.standard_normal((S or 1, L)) * np.exp(-4.0 * np.arange(L) / L)
    h = h if S else h[0]
    h.setflags(write=False)
    return h
