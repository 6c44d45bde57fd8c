"""Float64 restatement of cpc_resample (include/cpc_hip.h) and of the filter design of cpc_audio_amd.resampling, written from the
formulas and sharing no code with the package: the downmix, the taps, the zero extension at a segment's ends, the output count, and
the per-output magnitude sum that the rounding-error bound of the GPU tests is made of."""
import math

import numpy as np

RATE_PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (16000, 44100), (3, 2), (2, 3)]
SHAPES = {(44100, 16000): (160, 441, 47), (48000, 16000): (1, 3, 51), (8000, 16000): (2, 1, 17), (22050, 16000): (320, 441, 24),
          (16000, 44100): (441, 160, 17), (3, 2): (2, 3, 26), (2, 3): (3, 2, 17)}          # (L, M, W)
AUDIO_PAIRS = RATE_PAIRS[:5]


def bessel_i0(x):
    """The power series sum_k ((x / 2)^k / k!)^2, to float64 precision for |x| < 20."""
    x = np.asarray(x, dtype=np.float64)
    total, term = np.ones_like(x), np.ones_like(x)
    for k in range(1, 100):
        term = term * (x / (2.0 * k)) ** 2
        total = total + term
    return total


def prototype(L, M, zeros=16, rolloff=0.945, beta=14.769656459379492):
    """(h float64 [2 W L + 1] with sum L, W)."""
    c = rolloff * min(1.0, L / M)
    W = int(math.ceil(zeros / c))
    d = (np.arange(2 * W * L + 1, dtype=np.float64) - W * L) / L
    h = c * np.sinc(c * d) * bessel_i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (d / W) ** 2))) / bessel_i0(beta)
    return h * (L / h.sum()), W


def resample_taps(orig_rate, new_rate, **filter):
    """(taps float32 [L, 2 W + 1], L, M, W), taps[p][t] = h[p - (t - W) L + W L] where that index exists."""
    g = math.gcd(orig_rate, new_rate)
    L, M = new_rate // g, orig_rate // g
    if L == M:
        return np.ones((1, 1), np.float32), 1, 1, 0
    h, W = prototype(L, M, **filter)
    taps = np.zeros((L, 2 * W + 1))
    for p in range(L):
        for t in range(2 * W + 1):
            j = p - (t - W) * L + W * L
            if 0 <= j <= 2 * W * L:
                taps[p][t] = h[j]
    return taps.astype(np.float32), L, M, W


def output_count(N, L, M):
    return (N * L + M - 1) // M


def resample(frames, taps, L, M, W, mix="first", in_scale=1.0, out_scale=1.0):
    """One segment.  frames: [N] or [N, C]; taps: the float32 table [L, 2 W + 1].  (y, bound) in float64, ceil(N L / M) outputs each:
    y[n] = out_scale sum_t taps[p][t] x[i0 + t - W] over the t whose frame lies in [0, N), with x the downmixed frame times in_scale;
    bound[n] = sum_t |taps[p][t]| (sum_c |s_c| / C or |s_0|) |in_scale| |out_scale|."""
    s = np.asarray(frames, dtype=np.float64)
    s = s.reshape(len(s), -1)
    N, C = s.shape
    if mix == "mean":
        x, mag = np.zeros(N), np.zeros(N)
        for c in range(C):
            x, mag = x + s[:, c], mag + np.abs(s[:, c])
        x, mag = x / C, mag / C
    else:
        x, mag = s[:, 0].copy(), np.abs(s[:, 0])
    taps = np.asarray(taps, dtype=np.float64)
    n_out = output_count(N, L, M)
    y, bound = np.zeros(n_out), np.zeros(n_out)
    for n in range(n_out):
        i0, p = divmod(n * M, L)
        lo, hi = max(0, W - i0), min(2 * W, N - 1 - i0 + W)          # the t whose frame i0 + t - W lies in [0, N)
        if hi >= lo:
            row = taps[p][lo:hi + 1]
            y[n] = float(np.dot(row, x[i0 + lo - W:i0 + hi - W + 1]))
            bound[n] = float(np.dot(np.abs(row), mag[i0 + lo - W:i0 + hi - W + 1]))
    return y * in_scale * out_scale, bound * abs(in_scale) * abs(out_scale)


def interior(n_out, L, M, W):
    """The slice of outputs that drops ceil(W L / M) + 2 at each end."""
    edge = (W * L + M - 1) // M + 2
    return slice(edge, n_out - edge)


def square_wave(n=6000, period=80, amplitude=32767):
    i = np.arange(n)
    return np.where((i // (period // 2)) % 2 == 0, amplitude, -amplitude).astype(np.int16)
