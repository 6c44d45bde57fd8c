"""Masking augmentation on the input grid of the scalogram engine on the HIP path (include/cpc_hip.h, cpc_grid_sum / cpc_grid_mask;
DESIGN.md, "Grid masking"): frequency bands and time spans of the scalogram or log-mel grid of every clip are filled with zero, a
constant or the clip's own per-channel mean, after Park et al., "SpecAugment: A Simple Data Augmentation Method for Automatic Speech
Recognition" (without its time warping).

The grid stays on the device and the host only enqueues one launch (two with the mean fill).  Every random number is a pure function
of (seed, step, clip, field) with the arithmetic of augmentation.WaveAugmentation at fields of its own: ``spans`` restates on the host,
in numpy uint64 arithmetic, what the device draws."""
import ctypes as C
import math

import numpy as np
import torch

from . import _hip
from .augmentation import _M64, _clip_keys, _draw_int, _field

MAX_MASKS = 8
SUM_CHUNK = 4096                   # elements per partial sum of cpc_grid_sum
MASK_FIELD = 0x4D41534B            # the mask fields start here: no field or noise index of the waveform augmentation reaches it
_F_FREQ, _F_TIME = 0, 16
FILL_ZERO, FILL_CONSTANT, FILL_MEAN = 0, 1, 2


def _masks(value, what):
    if value is None:
        return 0, 0
    try:
        count, width = value
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be None or a pair (count, max_width), got {value!r}") from None
    try:
        ok = int(count) == count and int(width) == width and 1 <= int(count) <= MAX_MASKS and 1 <= int(width) < 2 ** 31
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{what} needs count in [1, {MAX_MASKS}] and max_width in [1, 2^31), got {value!r}")
    return int(count), int(width)


class GridMasking:
    """freq_masks: None, or (count, max_width) with count in [1, 8] — count bands of 0 .. min(max_width, H) bins are filled in every
        frame in front of the protected ones;
    time_masks: None, or (count, max_width) — count spans of 0 .. min(max_width, floor(time_fraction Wa), Wa) frames are filled,
        Wa = W - protect_last;
    time_fraction: in [0, 1], the share of the Wa frames one time mask may cover at most;
    fill: "zero", "mean" (the clip's own mean of the channel over all its W H cells) or a finite float;
    protect_last: the last protect_last frames of every clip are never changed (the frames the targets are made of, say);
    seed: an int in [0, 2^64).
    Out-of-range values raise ValueError.  The instance owns the workspace of its sum pass: use it from one stream at a time."""

    def __init__(self, freq_masks=None, time_masks=None, time_fraction=1.0, fill="zero", protect_last=0, seed=0):
        self.freq_count, self.freq_max = _masks(freq_masks, "freq_masks")
        self.time_count, self.time_max = _masks(time_masks, "time_masks")
        try:
            fraction = float(time_fraction)
        except (TypeError, ValueError):
            raise ValueError(f"time_fraction must be a number in [0, 1], got {time_fraction!r}") from None
        if not 0.0 <= fraction <= 1.0:          # (NaN fails the range)
            raise ValueError(f"time_fraction must be in [0, 1], got {time_fraction!r}")
        self.time_fraction = fraction
        self.fill_value = 0.0
        if isinstance(fill, str):
            if fill not in ("zero", "mean"):
                raise ValueError(f"fill must be 'zero', 'mean' or a finite float, got {fill!r}")
            self.fill_mode = FILL_ZERO if fill == "zero" else FILL_MEAN
        else:
            try:
                value = float(fill)
            except (TypeError, ValueError):
                raise ValueError(f"fill must be 'zero', 'mean' or a finite float, got {fill!r}") from None
            if isinstance(fill, bool) or not abs(value) <= float(np.finfo(np.float32).max):          # (NaN fails too)
                raise ValueError(f"fill must be 'zero', 'mean' or a finite float (in float32), got {fill!r}")
            self.fill_mode, self.fill_value = FILL_CONSTANT, value
        if isinstance(protect_last, bool) or not isinstance(protect_last, (int, np.integer)) or not 0 <= int(protect_last) < 2 ** 31:
            raise ValueError(f"protect_last must be an int in [0, 2^31), got {protect_last!r}")
        self.protect_last = int(protect_last)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _M64:
            raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
        self.seed = int(seed)
        self._workspace = None

    # ------------------------------------------------------------------------------------------ the configuration of one call
    def _visible(self, W):
        """Wa: the frames in front of the protected ones."""
        if self.protect_last > int(W):
            raise ValueError(f"protect_last = {self.protect_last} exceeds the grid's {int(W)} frames")
        return int(W) - self.protect_last

    def time_cap(self, W):
        """The widest time mask on a grid of W frames: min(max_width, floor(time_fraction Wa), Wa)."""
        Wa = self._visible(W)
        return min(self.time_max, int(math.floor(self.time_fraction * Wa)), Wa) if self.time_count else 0

    def config(self, step, clip_offset, W):
        """The C ABI's configuration block of one call."""
        return _hip.CpcGridMask(self.seed, int(step) & _M64, int(clip_offset) & _M64, self.protect_last, self.freq_count, self.freq_max,
                                self.time_count, self.time_cap(W), self.fill_mode, self.fill_value)

    # ------------------------------------------------------------------------------------------ the device call
    @staticmethod
    def _buffer(t, what):
        """The channels-last (B, W, H, Cc) tensor behind ``t``: t itself, or t.permute(0, 3, 2, 1) for the NCHW view the front ends
        return.  Clips may be further apart than W H Cc elements; inside a clip the elements are dense."""
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype != torch.float32:
            raise ValueError(f"{what} must be a 4-D float32 tensor: (B, W, H, Cc) channels-last, or the (B, Cc, H, W) view of one")
        if not t.is_cuda:
            raise RuntimeError("GridMasking runs on the GPU only (libcpc_hip.so; there is no CPU fallback): move the tensors to the device")
        for cand in (t, t.permute(0, 3, 2, 1)):
            B, W, H, Cc = (int(s) for s in cand.shape)
            if B >= 1 and W >= 1 and H >= 1 and Cc in (1, 2, 4) and cand[0].is_contiguous() and (B == 1 or cand.stride(0) >= W * H * Cc):
                return cand
        raise ValueError(f"{what} must be a dense channels-last (B, W, H, Cc) tensor with Cc in {{1, 2, 4}}, or the (B, Cc, H, W) view of "
                         f"one as the preprocessing modules return it; got shape {tuple(t.shape)}, strides {tuple(t.stride())}")

    def __call__(self, grid, step, clip_offset=0, out=None, spans_out=None, fill_out=None):
        """grid: the (B, Cc, H, W) view the preprocessing modules return (grid.permute(0, 3, 2, 1) contiguous) or a contiguous
        (B, W, H, Cc) tensor, f32, on the device; where a shape reads both ways, the (B, W, H, Cc) reading holds.  out = None masks
        grid in place (only the masked cells are written) and returns grid; an ``out`` of the same layout that does not overlap grid
        receives the masked copy and is returned, grid is left as it is.  spans_out: None or a contiguous (B, 32) int32 device tensor
        (eight (f0, w) pairs, then eight (t0, w) pairs); fill_out: None or a contiguous (B, 4) f32 device tensor (the fill per channel)."""
        x = self._buffer(grid, "grid")
        B, W, H, Cc = (int(s) for s in x.shape)
        n = W * H * Cc
        if n > 2 ** 31 - 1 or B > 65535:
            raise ValueError(f"GridMasking needs W H Cc <= 2^31 - 1 and B <= 65535, got {(B, W, H, Cc)}")
        y = x
        if out is not None:
            y = self._buffer(out, "out")
            if tuple(y.shape) != (B, W, H, Cc) or y.device != x.device or tuple(out.shape) != tuple(grid.shape):
                raise ValueError("out must have grid's shape, layout and device")
        ldbx = int(x.stride(0)) if B > 1 else n
        ldby = int(y.stride(0)) if B > 1 else n
        for name, t, shape, dt in (("spans_out", spans_out, (B, 32), torch.int32), ("fill_out", fill_out, (B, 4), torch.float32)):
            if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or t.device != x.device
                                  or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {shape} {dt} tensor on the grid's device")
        cfg = self.config(step, clip_offset, W)
        partial = None
        if self.fill_mode == FILL_MEAN:
            need = B * (-(-n // SUM_CHUNK)) * Cc
            ws = self._workspace
            if ws is None or ws.device != x.device or ws.numel() < need:
                ws = self._workspace = torch.empty(need, device=x.device, dtype=torch.float32)
            partial = ws
            _hip.call("cpc_grid_sum", _hip.ptr(x), _hip.ptr(partial), B, n, C.c_longlong(ldbx), Cc)
        _hip.call("cpc_grid_mask", _hip.ptr(x), _hip.ptr(y), _hip.ptr(partial), _hip.ptr(spans_out), _hip.ptr(fill_out), B, W, H, Cc,
                  C.c_longlong(ldbx), C.c_longlong(ldby), C.byref(cfg))
        return grid if out is None else out

    # ------------------------------------------------------------------------------------------ the host restatement
    def spans(self, step, B, W, H, clip_offset=0):
        """What the device draws for the B clips clip_offset .. clip_offset + B - 1 of ``step`` on grids of W frames and H bins:
        (spans, mask) — spans int32 [B, 32] as cpc_grid_mask's spans_out (eight (f0, w) pairs, then eight (t0, w) pairs, 0 where not
        drawn) and mask bool [B, W, H], True for the masked cells."""
        B, W, H = int(B), int(W), int(H)
        Wa = self._visible(W)
        spans = np.zeros((B, 32), dtype=np.int32)
        mask = np.zeros((B, W, H), dtype=bool)
        if Wa == 0:
            return spans, mask
        with np.errstate(over="ignore"):
            kb = _clip_keys(self.seed, step, np.uint64(int(clip_offset) & _M64) + np.arange(B, dtype=np.uint64))
        bins, frames = np.arange(H)[None, :], np.arange(W)[None, :]
        for d in range(self.freq_count):
            w = _draw_int(_field(kb, MASK_FIELD + _F_FREQ + 2 * d), 0, min(self.freq_max, H))
            f0 = _draw_int(_field(kb, MASK_FIELD + _F_FREQ + 2 * d + 1), 0, H - w)
            spans[:, 2 * d], spans[:, 2 * d + 1] = f0, w
            mask[:, :Wa, :] |= ((bins >= f0[:, None]) & (bins < (f0 + w)[:, None]))[:, None, :]
        cap = self.time_cap(W)
        for d in range(self.time_count):
            w = _draw_int(_field(kb, MASK_FIELD + _F_TIME + 2 * d), 0, cap)
            t0 = _draw_int(_field(kb, MASK_FIELD + _F_TIME + 2 * d + 1), 0, Wa - w)
            spans[:, 16 + 2 * d], spans[:, 17 + 2 * d] = t0, w
            mask |= ((frames >= t0[:, None]) & (frames < (t0 + w)[:, None]))[:, :, None]
        return spans, mask
