"""Log-mel spectrogram front end on the HIP path (not in the reference; DESIGN.md, "Log-mel front end").

``MelSpectrogram`` is a framed, Hann-windowed DFT without centring or padding -- one ``cpc_gemm_nt`` over overlapped waveform rows
(row t of clip b = x[b, t*hop : t*hop + n_fft]) against the windowed DFT basis, rows (re_k, im_k) interleaved -- and an HTK mel
filter bank of unnormalised triangles kept as per-band bin ranges.  ``MelPreprocessingModule`` adds ``cpc_mel_pointwise`` (power ->
mel bands -> log -> optional delta channel) and returns the permuted view of the channels-last buffer the scalogram engine reads in
place, like ``PreprocessingModule``.  Every coefficient is computed in float64 on the host and rounded to float32 once.
"""
import math

import numpy as np

import torch
import torch.nn as nn

from . import _hip

mel_default_dict = {'sr': 16000,
                    'n_fft': 512,
                    'win_length': 400,
                    'hop_length': 160,
                    'n_mels': 80,
                    'f_min': 0.0,
                    'f_max': None}

MAX_N_FFT, MAX_N_MELS = 8192, 1024          # cpc_mel_pointwise: n_freq <= 4097, n_mels <= 1024


def hz_to_mel(f):
    """HTK scale."""
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_filterbank(sr, n_fft, n_mels, f_min, f_max):
    """Dense (n_mels, n_fft/2 + 1) float64 bank of triangles without area normalisation over n_mels + 2 points equally spaced in mel:
    W[m, k] = max(0, min((f_k - l_m) / (c_m - l_m), (r_m - f_k) / (r_m - c_m))), f_k = k sr / n_fft."""
    pts = mel_to_hz(np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2))
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    l, c, r = pts[:-2, None], pts[1:-1, None], pts[2:, None]
    return np.maximum(0.0, np.minimum((f[None, :] - l) / (c - l), (r - f[None, :]) / (r - c)))


def band_tables(bank):
    """Dense bank -> (band_lo, band_n, band_off int32 [n_mels], band_w float64 [sum band_n]): band m is bins [lo, lo + n) with weights
    band_w[off : off + n].  Raises ValueError for a band without a bin of non-zero weight or with a gap in its support."""
    lo, cnt, off, ws, total = [], [], [], [], 0
    for m, row in enumerate(bank):
        nz = np.flatnonzero(row)
        if nz.size == 0:
            raise ValueError(f"mel band {m} has no bin of non-zero weight (too many bands for this n_fft and frequency range)")
        a, b = int(nz[0]), int(nz[-1]) + 1
        if nz.size != b - a:
            raise ValueError(f"mel band {m}: the support is not one contiguous bin range")
        lo.append(a), cnt.append(b - a), off.append(total), ws.append(row[a:b])
        total += b - a
    return (np.asarray(lo, dtype=np.int32), np.asarray(cnt, dtype=np.int32), np.asarray(off, dtype=np.int32),
            np.concatenate(ws).astype(np.float64))


class MelSpectrogram(nn.Module):
    def __init__(self, sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=80, f_min=0.0, f_max=None):
        super().__init__()
        if f_max is None:
            f_max = sr / 2.0
        # (the alignment rules are launch_gemm_nt's: K and lda multiples of 8 bf16 / 4 f32 elements, and the fast kernels' K stages)
        if n_fft % 64 or not 64 <= n_fft <= MAX_N_FFT:
            raise ValueError(f"n_fft must be a multiple of 64 in [64, {MAX_N_FFT}], got {n_fft}")
        if not 1 <= win_length <= n_fft:
            raise ValueError(f"win_length must be in [1, n_fft], got {win_length}")
        if hop_length < 8 or hop_length % 8:
            raise ValueError(f"hop_length must be a multiple of 8 (at least 8), got {hop_length}")
        if not 0 <= f_min < f_max <= sr / 2.0:
            raise ValueError(f"need 0 <= f_min < f_max <= sr / 2, got f_min {f_min}, f_max {f_max}, sr {sr}")
        if not 1 <= n_mels <= MAX_N_MELS:
            raise ValueError(f"n_mels must be in [1, {MAX_N_MELS}], got {n_mels}")
        self.sr, self.n_fft, self.win_length, self.hop_length, self.n_mels = sr, n_fft, win_length, hop_length, n_mels
        self.f_min, self.f_max = float(f_min), float(f_max)
        self.n_freq = n_fft // 2 + 1
        self.lds = 2 * self.n_freq + 6              # a multiple of 8 floats; the GEMM's pad columns land inside
        self.band_lo, self.band_n, self.band_off, self.band_w64 = band_tables(self.mel_filterbank())
        self.band_w = self.band_w64.astype(np.float32)          # what is uploaded
        # "fp32": exact-f32 MFMA GEMM;  "bf16x3": waveform and basis split into bf16 (hi, lo) pairs, three bf16 products per tap
        # accumulated in f32, as the CQT's
        self.precision = "fp32"
        self._operands = None
        self._tables = None

    def frames(self, length):
        return (length - self.n_fft) // self.hop_length + 1

    def window(self):
        """Periodic Hann window of win_length points centred in the n_fft frame (torch.stft's convention), float64."""
        w = np.zeros(self.n_fft, dtype=np.float64)
        left = (self.n_fft - self.win_length) // 2
        w[left:left + self.win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(self.win_length, dtype=np.float64) / self.win_length)
        return w

    def mel_filterbank(self):
        return mel_filterbank(self.sr, self.n_fft, self.n_mels, self.f_min, self.f_max)

    def dft_operand(self, rows):
        """f32 [rows][n_fft]: row 2k = w[n] cos(2 pi k n / n_fft), row 2k + 1 = -w[n] sin(2 pi k n / n_fft), k = 0 .. n_fft/2; zero rows
        behind.  The angle is reduced exactly ((k n) mod n_fft in integers) before the float64 cos / sin."""
        n_fft, w = self.n_fft, self.window()
        out = torch.zeros(rows, n_fft, dtype=torch.float32)
        n = np.arange(n_fft, dtype=np.int64)
        for k0 in range(0, self.n_freq, 256):
            k = np.arange(k0, min(self.n_freq, k0 + 256), dtype=np.int64)
            ang = (2.0 * np.pi / n_fft) * ((k[:, None] * n[None, :]) % n_fft).astype(np.float64)
            out[2 * k0:2 * k0 + 2 * len(k):2] = torch.from_numpy((w * np.cos(ang)).astype(np.float32))
            out[2 * k0 + 1:2 * k0 + 2 * len(k):2] = torch.from_numpy((-w * np.sin(ang)).astype(np.float32))
        return out

    # ------------------------------------------------------------------ device operands
    def _prepare(self, device):
        key = (str(device), self.precision)
        if self._operands is not None and self._operands[0] == key:
            return self._operands[1]
        if self.precision == "bf16x3":
            npad = (2 * self.n_freq + 7) // 8 * 8
            full = self.dft_operand(npad).to(device)
            wh = full.to(torch.bfloat16)
            wl = (full - wh.float()).to(torch.bfloat16)
            op = torch.stack([wh, wh, wl], dim=-1).reshape(npad, 3 * self.n_fft).contiguous()
        elif self.precision == "fp32":
            npad = (2 * self.n_freq + 3) // 4 * 4
            op = self.dft_operand(npad).to(device).contiguous()
        else:
            raise ValueError("MelSpectrogram.precision must be 'fp32' or 'bf16x3'")
        self._operands = (key, (op, npad))
        return op, npad

    def tables(self, device):
        """(band_lo, band_n, band_off int32, band_w f32) on the device, uploaded once per device."""
        key = str(device)
        if self._tables is None or self._tables[0] != key:
            self._tables = (key, tuple(torch.from_numpy(a).to(device) for a in (self.band_lo, self.band_n, self.band_off, self.band_w)))
        return self._tables[1]

    def transform(self, x):
        """x (B, 1, L) or (B, L) f32 on the GPU -> (spec f32 [B][Tn][lds] with (re, im) interleaved per bin, Tn, lds)."""
        if x.dim() == 3:
            x = x[:, 0, :]
        if x.device.type != "cuda":
            raise RuntimeError("the mel spectrogram runs on the GPU only (no CPU fallback)")
        x = x.detach().float().contiguous()
        B, L = x.shape
        Tn = self.frames(L)
        if Tn < 1:
            raise ValueError(f"clip of {L} samples is shorter than one frame (n_fft = {self.n_fft})")
        if L % 8:
            x = torch.nn.functional.pad(x, (0, 8 - L % 8))
        Lp, n_fft, hop, lds = x.shape[1], self.n_fft, self.hop_length, self.lds
        op, npad = self._prepare(x.device)
        spec = torch.empty(B, Tn, lds, device=x.device, dtype=torch.float32)
        if self.precision == "bf16x3":
            x3 = torch.empty(B, 3 * Lp, device=x.device, dtype=torch.bfloat16)
            _hip.call("cpc_split3_bf16", _hip.ptr(x), _hip.ptr(x3), x.numel())
            _hip.gemm_nt(_hip.ptr(x3), _hip.ptr(op), _hip.ptr(spec), B * Tn, npad, 3 * n_fft, 3 * hop, 3 * n_fft, lds, _hip.BF16,
                         a_rpi=Tn, a_item=3 * Lp, flags=_hip.GEMM_OUT_F32, a_extent=x3.numel(), b_extent=op.numel())
        else:
            _hip.gemm_nt(_hip.ptr(x), _hip.ptr(op), _hip.ptr(spec), B * Tn, npad, n_fft, hop, n_fft, lds, _hip.F32,
                         a_rpi=Tn, a_item=Lp, a_extent=x.numel(), b_extent=op.numel())
        return spec, Tn, lds

    def pointwise(self, spec, Tn, delta=False, take_log=True, log_offset=1e-6, scaling=1.0, delta_scaling=1.0):
        """cpc_mel_pointwise on a spectrum of transform(): f32 [B][W][n_mels][Cc], (W, Cc) = (Tn - 1, 2) with delta, (Tn, 1) without;
        take_log=False gives the mel power itself."""
        B = spec.shape[0]
        W, Cc = (Tn - 1, 2) if delta else (Tn, 1)
        if W < 1:
            raise ValueError("clip too short for a delta channel (needs at least two frames)")
        lo, cnt, off, w = self.tables(spec.device)
        out = torch.empty(B, W, self.n_mels, Cc, device=spec.device, dtype=torch.float32)
        _hip.call("cpc_mel_pointwise", _hip.ptr(spec), spec.shape[2], _hip.ptr(lo), _hip.ptr(cnt), _hip.ptr(off), _hip.ptr(w), _hip.ptr(out),
                  B, Tn, self.n_freq, self.n_mels, 1 if delta else 0, 1 if take_log else 0, float(log_offset), float(scaling),
                  float(delta_scaling))
        return out

    def forward(self, x):
        """(B, 1, L) -> (B, n_freq, frames, 2) complex spectrum as (re, im), a strided view of the interleaved buffer (like CQT.forward)."""
        spec, Tn, lds = self.transform(x)
        return spec[:, :, :2 * self.n_freq].view(spec.shape[0], Tn, self.n_freq, 2).permute(0, 2, 1, 3)


class MelPreprocessingModule(nn.Module):
    """(B, 1, L) waveform -> (B, {1,2}, n_mels, frames) log-mel spectrogram, float32: A[t, m] = scaling * log(M[t, m] + log_offset);
    with ``delta`` channel 0 at frame w is A[w + 1, m] and channel 1 is delta_scaling * (A[w + 1, m] - A[w, m]) / scaling (the layout of
    PreprocessingModule's phase variant).  The result is a strided NCHW view of a channels-last buffer [B][frames][n_mels][channels] that
    ScalogramResidualEncoder consumes without a copy.  Not differentiable.  Without ``mel_dict`` it is the identity."""

    def __init__(self, mel_dict=None, delta=False, log_offset=1e-6, scaling=1.0, delta_scaling=1.0):
        super().__init__()
        if not (math.isfinite(log_offset) and log_offset > 0):
            raise ValueError(f"log_offset must be positive and finite, got {log_offset}")
        if not (math.isfinite(scaling) and math.isfinite(delta_scaling)):
            raise ValueError("scaling and delta_scaling must be finite")
        self.downsampling_factor = 1
        self.receptive_field = 1
        self.mel = None
        if mel_dict is not None:
            self.mel = MelSpectrogram(**mel_dict)
            self.downsampling_factor = self.mel.hop_length
            self.receptive_field = self.mel.n_fft
        self.delta = bool(delta)
        self.log_offset, self.scaling, self.delta_scaling = float(log_offset), float(scaling), float(delta_scaling)
        self.output = None

    def forward(self, x):
        if self.mel is None:
            return x
        spec, Tn, _ = self.mel.transform(x)
        out = self.mel.pointwise(spec, Tn, delta=self.delta, log_offset=self.log_offset, scaling=self.scaling,
                                 delta_scaling=self.delta_scaling)
        x = out.permute(0, 3, 2, 1)              # (B, channels, n_mels, frames) view
        self.output = x
        return x
