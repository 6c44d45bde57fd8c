"""Float64 restatement of the log-mel front end ("Log-mel front end"), independent of the package: numpy only.

Frames: no centring, no padding, Tn = (L - n_fft) // hop + 1, frame t covers samples [t hop, t hop + n_fft).
Window: periodic Hann of win_length points, 0.5 - 0.5 cos(2 pi n / win_length), centred in the n_fft frame with
(n_fft - win_length) // 2 zeros on the left (torch.stft's convention).
Spectrum: X[t, k] = sum_n w[n] x[t hop + n] exp(-2 pi i k n / n_fft), k = 0 .. n_fft / 2; power p = re^2 + im^2.
Mel bank: HTK scale mel(f) = 2595 log10(1 + f / 700), n_mels + 2 points equally spaced in mel between f_min and f_max, triangles
without area normalisation W[m, k] = max(0, min((f_k - l_m) / (c_m - l_m), (r_m - f_k) / (r_m - c_m))), f_k = k sr / n_fft.
Output: M[t, m] = sum_k W[m, k] p[t, k], A[t, m] = scaling log(M[t, m] + log_offset); with delta, channel 0 at frame w is A[w + 1, m]
and channel 1 is delta_scaling (A[w + 1, m] - A[w, m]) / scaling.
"""
import numpy as np


def frames(length, n_fft, hop):
    return (length - n_fft) // hop + 1


def window(n_fft, win_length):
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    n = np.arange(win_length, dtype=np.float64)
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    return w


def dft_basis(n_fft):
    """complex128 [n_fft / 2 + 1][n_fft]: exp(-2 pi i k n / n_fft), the angle reduced in integers first."""
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    ang = (2.0 * np.pi / n_fft) * ((k * n) % n_fft).astype(np.float64)
    return np.cos(ang) - 1j * np.sin(ang)


def spectrum(x, n_fft, win_length, hop):
    """x float64 (B, L) -> complex128 (B, Tn, n_fft / 2 + 1)."""
    x = np.asarray(x, dtype=np.float64)
    Tn = frames(x.shape[1], n_fft, hop)
    idx = np.arange(Tn)[:, None] * hop + np.arange(n_fft)[None, :]
    fr = x[:, idx] * window(n_fft, win_length)                       # (B, Tn, n_fft)
    return fr @ dft_basis(n_fft).T


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_points(n_mels, f_min, f_max):
    """The n_mels + 2 corner frequencies in Hz."""
    return mel_to_hz(np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2))


def mel_filterbank(sr, n_fft, n_mels, f_min=0.0, f_max=None):
    f_max = sr / 2.0 if f_max is None else f_max
    pts = mel_points(n_mels, f_min, f_max)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    l, c, r = pts[:-2, None], pts[1:-1, None], pts[2:, None]
    return np.maximum(0.0, np.minimum((f[None, :] - l) / (c - l), (r - f[None, :]) / (r - c)))


def mel_power(x, sr, n_fft, win_length, hop, n_mels, f_min=0.0, f_max=None):
    """(B, L) -> (M float64 (B, Tn, n_mels), p float64 (B, Tn, n_freq), X complex128)."""
    X = spectrum(x, n_fft, win_length, hop)
    p = X.real ** 2 + X.imag ** 2
    return p @ mel_filterbank(sr, n_fft, n_mels, f_min, f_max).T, p, X


def log_mel(M, delta=False, log_offset=1e-6, scaling=1.0, delta_scaling=1.0):
    """M (B, Tn, n_mels) -> (B, {1, 2}, n_mels, frames) in the module's NCHW layout."""
    A = scaling * np.log(M + log_offset)
    if not delta:
        return A.transpose(0, 2, 1)[:, None]
    d = delta_scaling * (np.log(M[:, 1:] + log_offset) - np.log(M[:, :-1] + log_offset))
    return np.stack([A[:, 1:].transpose(0, 2, 1), d.transpose(0, 2, 1)], axis=1)


def expand_bands(band_lo, band_n, band_off, band_w, n_freq):
    """Band tables back to the dense (n_mels, n_freq) matrix, in band_w's dtype."""
    out = np.zeros((len(band_lo), n_freq), dtype=np.asarray(band_w).dtype)
    for m, (lo, n, off) in enumerate(zip(band_lo, band_n, band_off)):
        out[m, lo:lo + n] = band_w[off:off + n]
    return out


def band_sums(p, band_lo, band_n, band_off, band_w, n_freq):
    """What cpc_mel_pointwise(take_log = 0) defines, in float64: band ranges clamped to [0, n_freq).  p (..., n_freq)."""
    out = np.zeros(p.shape[:-1] + (len(band_lo),), dtype=np.float64)
    for m, (lo, n, off) in enumerate(zip(band_lo, band_n, band_off)):
        k0 = min(max(int(lo), 0), n_freq)
        k1 = min(max(int(lo) + int(n), k0), n_freq)
        w = np.asarray(band_w[off + k0 - lo:off + k1 - lo], dtype=np.float64)
        out[..., m] = p[..., k0:k1].astype(np.float64) @ w
    return out
