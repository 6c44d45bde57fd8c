"""Waveform augmentation in the time domain on the HIP path (include/cpc_hip.h, cpc_wave_power / cpc_wave_augment; DESIGN.md,
"Waveform augmentation"): speed change, time drop, additive noise, gain and polarity on the part of every clip in front of
``protect_from``, after Kharitonov et al., "Data augmenting contrastive learning of speech representations in the time domain".

The batch stays on the device and the host only enqueues two launches.  Every random number is a pure function of (seed, step, clip,
field or sample index): ``parameters`` and ``noise`` restate on the host, in numpy uint64 arithmetic (which wraps modulo 2^64), what
the device draws, as sampled_negatives.sampled_negative_keys does for the sampled loss."""
import ctypes as C
import math

import numpy as np
import torch

from . import _hip
from .sampled_negatives import _DRAW, _IDX, _M64, _MIX1, _MIX2, _STEP

Q_ONE = 65536                      # the rate 1 in Q16
POWER_CHUNK = 4096                 # samples per partial sum of cpc_wave_power
MAX_DROPS = 8
MAX_LENGTH = 1 << 24               # sample indices travel as f32 in params_out
_NOISE_FIELD = 32                  # per-sample hashes start behind the per-clip fields
_F_SPEED, _F_SNR, _F_GAIN, _F_POLARITY, _F_DROP = 1, 2, 3, 4, 8


def _mix(z):
    u = np.uint64
    with np.errstate(over="ignore"):
        z = (z ^ (z >> u(30))) * u(_MIX1)
        z = (z ^ (z >> u(27))) * u(_MIX2)
        return z ^ (z >> u(31))


def _clip_keys(seed, step, clips):
    """kb of the clips (uint64 array)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        return _mix(u((int(seed) + _DRAW * int(step)) & _M64) + u(_STEP) * (np.asarray(clips, dtype=np.uint64) + u(1)))


def _field(kb, f):
    """u_f of every clip: uint32 values in a uint64 array."""
    with np.errstate(over="ignore"):
        return _mix(kb + np.uint64((_IDX * int(f)) & _M64)) >> np.uint64(32)


def _draw_int(u, lo, hi):
    """lo + ((u (hi - lo + 1)) >> 32); lo, hi: ints or int64 arrays with hi - lo + 1 <= 2^32 (the product fits 64 bits)."""
    span = (np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64) + 1).astype(np.uint64)
    return np.asarray(lo, dtype=np.int64) + ((u * span) >> np.uint64(32)).astype(np.int64)


def _draw_real(u, lo, hi):
    """lo + (hi - lo) u 2^-32 in float64, lo and hi as the f32 values the device is given."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + (hi - lo) * u.astype(np.float64) * 2.0 ** -32


def _pair(value, what):
    try:
        lo, hi = value
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a pair (lo, hi), got {value!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"{what} must be finite with lo <= hi, got {value!r}")
    return lo, hi


class WaveAugmentation:
    """speed: None, or s in (0, 0.5] — the rate is drawn from [1 - s, 1 + s] (rounded to Q16); no low-pass filter is applied in front
        of a speed-up, so it is meant for s <= 0.25;
    time_drop: None, or (count, max_len) with count in [1, 8] and max_len >= 1 — count spans of 1 .. max_len samples become zero;
    noise_snr_db: None, or (lo, hi) — noise at a signal-to-noise ratio drawn from [lo, hi] dB against the clip's own mean square;
    gain_db: None, or (lo, hi) — a gain drawn from [lo, hi] dB;
    polarity: the probability in [0, 1] of flipping the sign;
    seed: an int in [0, 2^64).
    Out-of-range values raise ValueError.  The instance owns the workspace of its power pass: use it from one stream at a time."""

    def __init__(self, speed=None, time_drop=None, noise_snr_db=None, gain_db=None, polarity=0.0, seed=0):
        self.q_lo = self.q_hi = Q_ONE
        if speed is not None:
            s = float(speed)
            if not 0.0 < s <= 0.5:
                raise ValueError(f"speed must be in (0, 0.5] (the rate is drawn from [1 - speed, 1 + speed]), got {speed!r}")
            self.q_lo, self.q_hi = int(round((1.0 - s) * Q_ONE)), int(round((1.0 + s) * Q_ONE))
        self.drop_count, self.drop_max_len = 0, 0
        if time_drop is not None:
            try:
                count, max_len = time_drop
            except (TypeError, ValueError):
                raise ValueError(f"time_drop must be a pair (count, max_len), got {time_drop!r}") from None
            if int(count) != count or int(max_len) != max_len or not 1 <= int(count) <= MAX_DROPS or not 1 <= int(max_len) <= MAX_LENGTH:
                raise ValueError(f"time_drop needs count in [1, {MAX_DROPS}] and max_len in [1, 2^24], got {time_drop!r}")
            self.drop_count, self.drop_max_len = int(count), int(max_len)
        self.noise_snr_db = None if noise_snr_db is None else _pair(noise_snr_db, "noise_snr_db")
        self.gain_db = None if gain_db is None else _pair(gain_db, "gain_db")
        p = float(polarity)
        if not 0.0 <= p <= 1.0:          # (NaN fails the range)
            raise ValueError(f"polarity must be a probability in [0, 1], got {polarity!r}")
        self.polarity_threshold = int(round(p * 2.0 ** 32))
        if int(seed) != seed or not 0 <= int(seed) <= _M64:
            raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
        self.seed = int(seed)
        self._workspace = None

    # ------------------------------------------------------------------------------------------ what is on
    @property
    def speed_on(self):
        return not (self.q_lo == Q_ONE and self.q_hi == Q_ONE)

    @property
    def noise_on(self):
        return self.noise_snr_db is not None

    @staticmethod
    def _protect(protect_from, L):
        a = int(L) if protect_from is None else int(protect_from)
        if not 0 <= a <= int(L):
            raise ValueError(f"protect_from must be in [0, L] = [0, {int(L)}], got {protect_from!r}")
        return a

    def config(self, step, clip_offset, protect_from):
        """The C ABI's configuration block of one call."""
        snr = self.noise_snr_db or (0.0, 0.0)
        gain = self.gain_db or (0.0, 0.0)
        return _hip.CpcWaveAugment(self.seed, int(step) & _M64, int(clip_offset) & _M64, int(protect_from), self.q_lo, self.q_hi,
                                   self.drop_count, self.drop_max_len, int(self.noise_on), snr[0], snr[1],
                                   int(self.gain_db is not None), gain[0], gain[1], self.polarity_threshold)

    # ------------------------------------------------------------------------------------------ the device call
    def __call__(self, batch, step, clip_offset=0, protect_from=None, out=None, params_out=None):
        """batch: (B, L) f32 device tensor, unit stride along L (rows may be strided).  Returns the augmented batch in ``out`` (a
        (B, L) f32 device tensor that does not overlap batch; a fresh tensor when None); batch itself is never written.  params_out:
        None or a contiguous (B, 8) f32 device tensor that receives what the device drew (q, sigma, signed gain, mean square, and the
        first two (start, len) spans)."""
        if not isinstance(batch, torch.Tensor) or batch.dim() != 2 or batch.dtype != torch.float32:
            raise ValueError("WaveAugmentation takes a (B, L) float32 tensor")
        if not batch.is_cuda:
            raise RuntimeError("WaveAugmentation runs on the GPU only (libcpc_hip.so; there is no CPU fallback): move the tensors to "
                               "the device")
        B, L = int(batch.shape[0]), int(batch.shape[1])
        if B < 1 or not 1 <= L <= MAX_LENGTH:
            raise ValueError(f"WaveAugmentation needs B >= 1 and 1 <= L <= 2^24, got {(B, L)}")
        a = self._protect(protect_from, L)
        if batch.stride(1) != 1 or (B > 1 and batch.stride(0) < L):
            batch = batch.contiguous()
        ldx = max(int(batch.stride(0)), L)
        if out is None:
            out = torch.empty((B, L), device=batch.device, dtype=torch.float32)
        elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, L) or out.dtype != torch.float32 or out.device != batch.device
              or out.stride(1) != 1 or (B > 1 and out.stride(0) < L)):
            raise ValueError("out must be a (B, L) float32 tensor on the batch's device with unit stride along L and rows that do not overlap")
        ldy = max(int(out.stride(0)), L)
        if params_out is not None and (tuple(params_out.shape) != (B, 8) or params_out.dtype != torch.float32
                                       or params_out.device != batch.device or not params_out.is_contiguous()):
            raise ValueError("params_out must be a contiguous (B, 8) float32 tensor on the batch's device")
        partial = None
        if self.noise_on:
            need = B * max(1, -(-a // POWER_CHUNK))
            ws = self._workspace
            if ws is None or ws.device != batch.device or ws.numel() < need:
                ws = self._workspace = torch.empty(need, device=batch.device, dtype=torch.float32)
            partial = ws
            if a >= 1:
                _hip.call("cpc_wave_power", _hip.ptr(batch), _hip.ptr(partial), B, L, C.c_longlong(ldx), a)
        cfg = self.config(step, clip_offset, a)
        _hip.call("cpc_wave_augment", _hip.ptr(batch), _hip.ptr(out), _hip.ptr(partial), _hip.ptr(params_out), B, L, C.c_longlong(ldx),
                  C.c_longlong(ldy), C.byref(cfg))
        return out

    # ------------------------------------------------------------------------------------------ the host restatements
    def parameters(self, step, B, L, clip_offset=0, protect_from=None):
        """What the device draws for the B clips clip_offset .. clip_offset + B - 1 of ``step``, as numpy arrays: q (int64 [B]),
        snr_db and gain_db (float64 [B]; NaN where the stage is off), flip (bool [B]), drop_start and drop_len (int64 [B, count]).
        With protect_from = 0 no stage applies: q = 65536, no flip, spans of length 0."""
        B, L = int(B), int(L)
        a = self._protect(protect_from, L)
        with np.errstate(over="ignore"):
            kb = _clip_keys(self.seed, step, np.uint64(int(clip_offset) & _M64) + np.arange(B, dtype=np.uint64))
        live = a > 0
        q = np.full(B, Q_ONE, dtype=np.int64)
        if self.speed_on and live:
            q = _draw_int(_field(kb, _F_SPEED), self.q_lo, self.q_hi)
        snr_db = np.full(B, np.nan)
        if self.noise_on and live:
            snr_db = _draw_real(_field(kb, _F_SNR), *self.noise_snr_db)
        gain_db = np.full(B, np.nan)
        if self.gain_db is not None and live:
            gain_db = _draw_real(_field(kb, _F_GAIN), *self.gain_db)
        flip = (_field(kb, _F_POLARITY) < np.uint64(self.polarity_threshold)) & live
        start = np.zeros((B, self.drop_count), dtype=np.int64)
        length = np.zeros((B, self.drop_count), dtype=np.int64)
        if live:
            for d in range(self.drop_count):
                length[:, d] = _draw_int(_field(kb, _F_DROP + 2 * d), 1, min(self.drop_max_len, a))
                start[:, d] = _draw_int(_field(kb, _F_DROP + 1 + 2 * d), 0, a - length[:, d])
        return {"q": q, "snr_db": snr_db, "gain_db": gain_db, "flip": flip, "drop_start": start, "drop_len": length}

    def noise(self, step, clip, n0, n1):
        """g(n) for the samples n0 <= n < n1 of one clip (float64): the sum of the four 16-bit fields of the sample's hash, centred
        and scaled to unit variance."""
        u = np.uint64
        kb = _clip_keys(self.seed, step, [int(clip)])[0]
        n = np.arange(int(n0), int(n1), dtype=np.uint64)
        with np.errstate(over="ignore"):
            h = _mix(kb + u(_IDX) * (n + u(_NOISE_FIELD)))
        m = u(0xFFFF)
        s = ((h & m) + ((h >> u(16)) & m) + ((h >> u(32)) & m) + (h >> u(48))).astype(np.int64)
        return (s - 131070).astype(np.float64) * (math.sqrt(3.0) / 65536.0)
