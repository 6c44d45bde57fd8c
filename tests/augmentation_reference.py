"""float64 numpy reference of the waveform augmentation (include/cpc_hip.h, cpc_wave_power / cpc_wave_augment), given the per-clip
scalars: what tests/test_augmentation_gpu.py holds the kernels to and tests/test_augmentation_host.py checks against its own
definition.  It applies the definition as written, not the kernel's order of operations."""
import numpy as np

Q_ONE = 65536
POWER_CHUNK = 4096


def catmull_rom(t):
    """(w_-1, w_0, w_1, w_2) at the fraction t, as the definition writes them."""
    t = np.asarray(t, dtype=np.float64)
    return (((-t + 2.0) * t - 1.0) * t / 2.0, ((3.0 * t - 5.0) * t * t + 2.0) / 2.0, ((-3.0 * t + 4.0) * t + 1.0) * t / 2.0,
            (t - 1.0) * t * t / 2.0)


def catmull_rom_factored(t):
    """The same four polynomials in the factored forms the kernel evaluates."""
    t = np.asarray(t, dtype=np.float64)
    u = 1.0 - t
    return -t * u * u / 2.0, u * (2.0 + t * (2.0 - 3.0 * t)) / 2.0, t * (1.0 + t * (4.0 - 3.0 * t)) / 2.0, -u * t * t / 2.0


def power_partials(x, n):
    """[ceil(n / 4096)] float64: the sum of squares of every chunk of x[0 .. n)."""
    x = np.asarray(x, dtype=np.float64)[:n]
    return np.array([np.sum(x[c:c + POWER_CHUNK] ** 2) for c in range(0, n, POWER_CHUNK)])


def resample(x, a, q):
    """(v, mag) for the outputs n < a of one clip at the rate q (Q16): v = sum_j w_j x[i + j] and mag = sum_j |w_j x[i + j]|, with
    pos = a 65536 - (a - n) q in exact integers, i = pos >> 16, t = (pos & 0xFFFF) / 65536 and x = 0 outside the clip."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    n = np.arange(a, dtype=np.int64)
    pos = np.int64(a) * Q_ONE - (np.int64(a) - n) * np.int64(q)
    i = pos >> 16
    t = (pos & 0xFFFF).astype(np.float64) / 65536.0
    v = np.zeros(a)
    mag = np.zeros(a)
    for j, w in zip((-1, 0, 1, 2), catmull_rom(t)):
        idx = i + j
        inside = (idx >= 0) & (idx < L)
        tap = np.where(inside, x[np.clip(idx, 0, L - 1)], 0.0)
        v += w * tap
        mag += np.abs(w * tap)
    return v, mag


def augment(x, a, q=Q_ONE, drops=(), sigma=0.0, g=None, gain=1.0):
    """(y, mag) of one clip x[L] (float64): the stages in the definition's order on n < a, x itself on n >= a.  drops: (start, len)
    pairs; g: the noise variates of n < a (None: no noise); gain: the signed gain.  mag[n] = sum_j |w_j x[i + j]| + sigma |g[n]|
    (0 from the signal inside a dropped span), the magnitude the kernel's rounding error scales with; 0 on n >= a."""
    x = np.asarray(x, dtype=np.float64)
    y, mag = x.copy(), np.zeros_like(x)
    if a == 0:
        return y, mag
    if q != Q_ONE:
        v, m = resample(x, a, q)
    else:
        v, m = x[:a].copy(), np.abs(x[:a])
    for start, length in drops:
        v[start:start + length] = 0.0
        m[start:start + length] = 0.0
    if g is not None:
        v = v + float(sigma) * np.asarray(g, dtype=np.float64)
        m = m + abs(float(sigma)) * np.abs(g)
    y[:a] = v * float(gain)
    mag[:a] = m
    return y, mag
