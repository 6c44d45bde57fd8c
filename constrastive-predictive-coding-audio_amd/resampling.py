"""Sampling-rate conversion on the device: the filter design on the host (a Kaiser-windowed sinc cut into L phases), and the launch of
cpc_resample, which downmixes, resamples by L / M and stores a list of segments (files) in one launch.

``resample_taps`` is the filter; ``resample`` is the public function for tensors that already lie in HBM; ``ResamplePlan`` and
``convert_segments`` are what ``DeviceAudioDataset(convert=True)`` loads its files through.  There is no host fallback: the HIP path
resamples on the device or not at all.
"""
from __future__ import annotations

import math

import numpy as np
import torch

TILE = 1024                       # the tile of cpc_resample (include/cpc_hip.h): outputs per workgroup, the unit of the tile prefix table
MAX_TABLE_FLOATS = 1 << 20        # L (2 W + 1): 4 MB of taps; rate pairs beyond it (a large L from an awkward ratio) are refused
MAX_SPAN_FLOATS = 16384           # the LDS budget of cpc_resample for the input span of one tile
F32, INT16 = 0, 1                 # the sample codes of the C ABI
MIX_FIRST, MIX_MEAN = 0, 1


def rate_ratio(orig_rate, new_rate):
    """(L, M) with new / orig = L / M in lowest terms."""
    orig_rate, new_rate = int(orig_rate), int(new_rate)
    if orig_rate < 1 or new_rate < 1:
        raise ValueError(f"sampling rates must be positive, not {orig_rate} and {new_rate}")
    g = math.gcd(orig_rate, new_rate)
    return new_rate // g, orig_rate // g


def output_length(frames, L, M):
    """ceil(frames L / M): the outputs n whose centre (n M) div L lies inside the input."""
    return -((-int(frames) * L) // M)


def resample_taps(orig_rate, new_rate, zeros=16, rolloff=0.945, beta=14.769656459379492):
    """(taps float32 [L, 2 W + 1], L, M, W): y[n] = sum_t taps[p][t] x[i0 + t - W] with i0 = (n M) div L and p = (n M) mod L.

    The prototype, in float64, is a sinc with its cut-off at ``rolloff`` times the lower Nyquist rate under a Kaiser window of
    ``zeros`` zero crossings a side: h[j] = c sinc(c d) I0(beta sqrt(1 - (d / W)^2)) / I0(beta), d = (j - W L) / L, j = 0 .. 2 W L,
    c = rolloff min(1, L / M), W = ceil(zeros / c), scaled to sum(h) = L.  Equal rates give the identity table (W = 0)."""
    L, M = rate_ratio(orig_rate, new_rate)
    if L == M:
        return np.ones((1, 1), np.float32), 1, 1, 0
    c = float(rolloff) * min(1.0, L / M)
    if not (c > 0.0 and zeros >= 1):
        raise ValueError("rolloff must be positive and zeros at least 1")
    W = int(math.ceil(zeros / c))
    if L * (2 * W + 1) > MAX_TABLE_FLOATS:
        raise ValueError(f"resampling {orig_rate} -> {new_rate}: the tap table has {L} x {2 * W + 1} floats, more than the limit of "
                         f"{MAX_TABLE_FLOATS} (L (2 W + 1)); choose rates with a smaller ratio in lowest terms")
    d = (np.arange(2 * W * L + 1, dtype=np.float64) - W * L) / L
    h = c * np.sinc(c * d) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (d / W) ** 2))) / np.i0(beta)
    h *= L / h.sum()
    index = np.arange(L)[:, None] - (np.arange(2 * W + 1)[None, :] - W) * L + W * L
    inside = (index >= 0) & (index <= 2 * W * L)
    taps = np.where(inside, h[np.clip(index, 0, 2 * W * L)], 0.0).astype(np.float32)
    return taps, L, M, W


class ResamplePlan:
    """The taps of one rate pair with their device copy (transposed, [2 W + 1][L], what cpc_resample reads), made once per device."""

    def __init__(self, orig_rate, new_rate, **filter):
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.taps, self.L, self.M, self.W = resample_taps(orig_rate, new_rate, **filter)
        span = ((TILE - 1) * self.M) // self.L + 2 * self.W + 2
        if span > MAX_SPAN_FLOATS:
            raise ValueError(f"resampling {orig_rate} -> {new_rate}: a tile of {TILE} outputs spans {span} input frames, more than the "
                             f"{MAX_SPAN_FLOATS} floats of LDS cpc_resample stages")
        self._device_taps = {}

    def output_length(self, frames):
        return output_length(frames, self.L, self.M)

    def device_taps(self, device):
        device = torch.device(device)
        if device not in self._device_taps:
            self._device_taps[device] = torch.from_numpy(np.ascontiguousarray(self.taps.T)).to(device)
        return self._device_taps[device]


_PLANS = {}


def plan_for(orig_rate, new_rate, **filter):
    key = (int(orig_rate), int(new_rate), tuple(sorted(filter.items())))
    if key not in _PLANS:
        _PLANS[key] = ResamplePlan(orig_rate, new_rate, **filter)
    return _PLANS[key]


def _code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.int16:
        return INT16
    raise ValueError(f"samples are float32 or int16, not {t.dtype}")


def convert_segments(src, channels, mix, plan, segments, dst, in_scale=1.0, out_scale=1.0):
    """One cpc_resample launch.  src: a device tensor of interleaved frames ([frames] or [frames, channels], f32 or int16); segments:
    an int64 array [nseg, 4] of (first source frame, source frames, first output in dst, output count); dst: a 1-D device tensor,
    f32 or int16, on the same device.  The table is checked here; the kernel's guard is not relied on."""
    from . import _hip
    if not (src.is_cuda and dst.is_cuda and src.device == dst.device):
        raise RuntimeError("resampling runs on the device: the HIP path has no CPU fallback")
    if not (src.is_contiguous() and dst.is_contiguous() and dst.dim() == 1):
        raise ValueError("src and dst must be contiguous, dst 1-D")
    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.int64).reshape(-1, 4))
    frames_total = src.numel() // channels
    if len(seg) < 1 or seg.min() < 0 or int((seg[:, 0] + seg[:, 1]).max()) > frames_total or int((seg[:, 2] + seg[:, 3]).max()) > dst.numel():
        raise ValueError("segment table out of range")
    tiles = -(-seg[:, 3] // TILE)
    ntiles = int(tiles.sum())
    if ntiles == 0:
        return
    tile_first = np.concatenate([np.zeros(1, np.int64), np.cumsum(tiles)[:-1]])
    with torch.cuda.device(src.device):
        tables = torch.from_numpy(np.concatenate([seg.reshape(-1), tile_first])).to(src.device)
        _hip.call("cpc_resample", _hip.ptr(src), _code(src), frames_total, int(channels), int(mix), float(in_scale),
                  _hip.ptr(plan.device_taps(src.device)), plan.L, plan.M, plan.W, _hip.ptr(tables), _hip.ptr(tables, 4 * len(seg)),
                  len(seg), ntiles, _hip.ptr(dst), _code(dst), dst.numel(), float(out_scale))


def resample(x, orig_rate, new_rate, **filter):
    """x, a device tensor (N,) or (B, N) of float32 or int16 with one segment per row, at ``new_rate``: the same dtype with
    ceil(N L / M) columns, from one launch.  int16 results are rounded half to even and saturated.  ``filter``: resample_taps' keywords."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("x is a tensor of shape (N,) or (B, N)")
    if not x.is_cuda:
        raise RuntimeError("resample runs on the device: the HIP path has no CPU fallback; move x to the GPU")
    _code(x)
    plan = plan_for(orig_rate, new_rate, **filter)
    rows, N = (1, x.shape[0]) if x.dim() == 1 else x.shape
    n_out = plan.output_length(N)
    out = torch.empty((rows, n_out) if x.dim() == 2 else (n_out,), device=x.device, dtype=x.dtype)
    if rows and n_out:
        r = np.arange(rows, dtype=np.int64)
        segments = np.stack([r * N, np.full(rows, N), r * n_out, np.full(rows, n_out)], axis=1)
        convert_segments(x.contiguous(), 1, MIX_FIRST, plan, segments, out.view(-1))
    return out
