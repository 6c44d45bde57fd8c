"""Host-side plan of the CPC train step: buffers in HBM + the launch sequence over the C ABI.

One ``CPCEngine`` = one (batch size, clip length, storage dtype) instance of the path
    AudioEncoder.forward -> context network -> prediction_model -> score/InfoNCE -> backward -> Adam
(reference: audio_model.py:193-211 and contrastive_estimation_training.py:97-162).  The context network is pluggable
(contexts.py: the context classes, and ContextHost, the part of an engine they may read); scalogram_engine.ScalogramCPCEngine
swaps the encoder for the 2-D residual encoder.  PyTorch is used for
device memory, streams and a few strided copies only; every arithmetic step is a HIP kernel behind libcpc_hip.so.

Data layout (all per GPU, resident for the life of the engine):
  act[l], dact[l]   storage dtype, channels-last [B][L_alloc[l]][C_l], zero pad rows, zero guards front/back
  L_alloc[l-1] = stride_l * L_alloc[l]  so that a strided conv is a GEMM whose A rows overlap uniformly
  flat parameters / gradients / Adam moments: f32, one contiguous buffer each (owned by the model)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import numbers
from types import SimpleNamespace
from typing import List, Optional, Sequence

import torch

from . import _hip, switches
from .contexts import ContextHost, GRUContext, _ceil_div, make_context
from .sampled_negatives import check_group_negatives, check_negatives, group_mode


SCORE_KINDS = ("softplus", "linear", "difference", "normalized")
NORM_EPS = 1e-8          # F.normalize's clamp under the norms of the "normalized" score (cosine similarity / temperature)


def score_kind(softplus: bool, score: Optional[str] = None) -> str:
    """The score function a loss call runs: ``score`` ("softplus" | "linear" | "difference" | "normalized") when given, else the
    ``softplus`` flag's choice between the two dot-product scores (contrastive_estimation_training.py:12-33)."""
    if score is None:
        return "softplus" if softplus else "linear"
    if score not in SCORE_KINDS:
        raise ValueError(f"score must be one of {SCORE_KINDS}, got {score!r}")
    return score


def check_temperature(temperature, kind: Optional[str] = None):
    """The temperature of the "normalized" score as a float: ValueError unless it is finite and > 0.  With ``kind`` also the pairing:
    the "normalized" kind needs one, and every other kind refuses one (returns None there)."""
    if kind is not None and kind != "normalized":
        if temperature is not None:
            raise ValueError(f"temperature belongs to score='normalized'; score {kind!r} has none")
        return None
    if temperature is None:
        raise ValueError("score='normalized' needs a temperature (finite and > 0)")
    if isinstance(temperature, DeviceTemperature):          # checked when it was built; the float checks below are for floats
        return temperature
    try:
        value = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"temperature must be a positive finite number, got {temperature!r}") from None
    if not math.isfinite(value) or value <= 0.0:
        raise ValueError(f"temperature must be a positive finite number, got {temperature!r}")
    return value


def check_temperature_range(min_temperature, max_temperature):
    """(min_temperature, max_temperature) as floats: ValueError unless both are finite and > 0 and in order."""
    out = []
    for value, what in ((min_temperature, "min_temperature"), (max_temperature, "max_temperature")):
        try:
            number = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a positive finite number, got {value!r}") from None
        if isinstance(value, bool) or not math.isfinite(number) or number <= 0.0:
            raise ValueError(f"{what} must be a positive finite number, got {value!r}")
        out.append(number)
    lo, hi = out
    if lo > hi:
        raise ValueError(f"min_temperature ({lo!r}) must not exceed max_temperature ({hi!r})")
    return lo, hi


def check_temperature_bounds(temperature, min_temperature, max_temperature):
    """(temperature, min_temperature, max_temperature) as floats: check_temperature_range's checks, and ValueError unless the
    temperature is finite and > 0 and lies inside the pair."""
    lo, hi = check_temperature_range(min_temperature, max_temperature)
    tau = check_temperature(temperature)
    if not lo <= tau <= hi:
        raise ValueError(f"temperature {tau!r} lies outside [min_temperature, max_temperature] = [{lo!r}, {hi!r}]")
    return tau, lo, hi


class TemperatureSchedule:
    """An annealed temperature: step ``s`` (0-based) scores at ``value(s)``, with q = min(s / total_steps, 1):
    'linear': start + (end - start) q;  'cosine': end + (start - end) * 0.5 (1 + cos(pi q)).  From step ``total_steps`` on it stays at
    ``end``.  cpc_temperature_set evaluates the same function on the device, in double."""

    KINDS = ("linear", "cosine")

    def __init__(self, kind, start, end, total_steps):
        if kind not in self.KINDS:
            raise ValueError(f"TemperatureSchedule kind must be one of {self.KINDS}, got {kind!r}")
        if isinstance(total_steps, bool) or not isinstance(total_steps, int) or total_steps < 1:
            raise ValueError(f"TemperatureSchedule total_steps must be an integer >= 1, got {total_steps!r}")
        self.kind, self.total_steps = kind, total_steps
        self.start, self.end = check_temperature(start), check_temperature(end)

    def value(self, step):
        """The temperature of the step with 0-based index ``step``, in Python floats (the tick's expressions)."""
        if isinstance(step, bool) or not isinstance(step, int) or step < 0:
            raise ValueError(f"the step index must be an integer >= 0, got {step!r}")
        q = min(step / self.total_steps, 1.0)
        if self.kind == "linear":
            return self.start + (self.end - self.start) * q
        return self.end + (self.start - self.end) * (0.5 * (1.0 + math.cos(math.pi * q)))

    def abi_args(self):
        """(kind, start, end, total_steps) as cpc_temperature_set takes them."""
        return self.KINDS.index(self.kind), C.c_double(self.start), C.c_double(self.end), C.c_longlong(self.total_steps)

    def __repr__(self):
        return f"TemperatureSchedule({self.kind!r}, start={self.start!r}, end={self.end!r}, total_steps={self.total_steps})"


class DeviceTemperature:
    """The temperature of the "normalized" score as device state (include/cpc_hip.h, cpc_temperature_step / cpc_temperature_set;
    DESIGN.md, "Learnable and scheduled temperature"): ``tstate`` f32[8] = {s = log(1 / tau), scale = exp(s), Adam's m and v of s, the
    latest d loss / d s, tau, 0, 0}.  The normalise kernels read the scale from it, so a captured step can change it.
      mode "learnable": FusedAdam(temperature=this) updates s behind every parameter update, at lr * ``lr_scale``, and clamps tau to
        [min_temperature, max_temperature];
      mode "scheduled": every loss call sets tau = ``schedule``.value(step) in front of its normalise launches; ``step`` is this object's
        0-based count (the trainer sets it to its training step, FusedAdam advances it), or the device's own under a captured step
        (``bind``).
    Passed as ``temperature=`` wherever a float is; an evaluation (nce_eval) reads the value as it stands."""

    MODES = ("learnable", "scheduled")

    def __init__(self, temperature=0.1, mode="learnable", min_temperature=0.01, max_temperature=1.0, lr_scale=1.0, schedule=None,
                 device=None):
        if mode not in self.MODES:
            raise ValueError(f"DeviceTemperature mode must be one of {self.MODES}, got {mode!r}")
        if mode == "scheduled":
            if not isinstance(schedule, TemperatureSchedule):
                raise ValueError(f"mode 'scheduled' needs a TemperatureSchedule, got {schedule!r}")
            temperature = schedule.value(0)
            self.min_temperature = self.max_temperature = None
        else:
            if schedule is not None:
                raise ValueError("a learnable temperature takes no schedule")
            temperature, self.min_temperature, self.max_temperature = check_temperature_bounds(temperature, min_temperature,
                                                                                                max_temperature)
        try:
            self.lr_scale = float(lr_scale)
        except (TypeError, ValueError):
            raise ValueError(f"lr_scale must be a finite number >= 0, got {lr_scale!r}") from None
        if isinstance(lr_scale, bool) or not math.isfinite(self.lr_scale) or self.lr_scale < 0.0:
            raise ValueError(f"lr_scale must be a finite number >= 0, got {lr_scale!r}")
        self.mode, self.schedule = mode, schedule
        self.device = torch.device("cuda" if device is None else device)
        self.tstate = torch.zeros(8, device=self.device, dtype=torch.float32)
        self.step = 0                 # scheduled: the 0-based index of the step the next loss call belongs to
        self.dots = None              # the per-row dots of the latest backward (the engine's scratch): what cpc_temperature_step adds up
        self._adam_state, self._step_offset = None, 0
        self._fill(temperature)

    @staticmethod
    def host_state(temperature):
        """(s, scale, tau) as float32 values: scale = float32(1 / tau) — the bits the constant path passes as its launch argument —,
        s = log of that value, tau rounded once."""
        import numpy as np
        scale = np.float32(1.0 / float(temperature))
        return float(np.float32(math.log(float(scale)))), float(scale), float(np.float32(float(temperature)))

    def _fill(self, temperature, m=0.0, v=0.0, g=0.0, s=None, scale=None, tau=None):
        s0, scale0, tau0 = self.host_state(temperature)
        if s is not None:          # a saved s: the derived values as saved, else as the kernel forms them (double, rounded once)
            import numpy as np
            s0 = float(np.float32(s))
            scale0 = float(np.float32(math.exp(s0))) if scale is None else float(scale)
            tau0 = float(np.float32(math.exp(-s0))) if tau is None else float(tau)
        self.tstate.copy_(torch.tensor([s0, scale0, m, v, g, tau0, 0.0, 0.0], dtype=torch.float32))

    @property
    def bounds(self):
        """(s_min, s_max) = (log(1 / max_temperature), log(1 / min_temperature)) of the learnable mode."""
        return math.log(1.0 / self.max_temperature), math.log(1.0 / self.min_temperature)

    def bind(self, adam_state, step_offset=0):
        """Scheduled mode inside a captured step: the tick takes its step from the device (``adam_state``, the f32[4] of FusedAdam under
        device_step, whose count is the number of steps finished) plus ``step_offset``.  bind(None) goes back to this object's ``step``."""
        self._adam_state, self._step_offset = adam_state, int(step_offset)

    def scale_ptr(self):
        return _hip.ptr(self.tstate, 1)

    def tick(self):
        """Scheduled mode: queues cpc_temperature_set for the step at hand on the current stream (nothing in learnable mode)."""
        if self.mode != "scheduled":
            return
        bound = self._adam_state is not None
        _hip.call("cpc_temperature_set", _hip.ptr(self.tstate), *self.schedule.abi_args(), C.c_longlong(0 if bound else self.step),
                  _hip.ptr(self._adam_state), C.c_longlong(self._step_offset if bound else 0))

    def value(self):
        """The temperature as it stands (tstate[5]); waits for the device."""
        return float(self.tstate[5].item())

    def state_dict(self):
        """{'mode', 's', 'm', 'v', 'step'} and the derived 'scale', 'tau' and latest gradient 'g', with one synchronous read."""
        row = self.tstate.detach().cpu().tolist()
        return {"mode": self.mode, "s": row[0], "scale": row[1], "m": row[2], "v": row[3], "g": row[4], "tau": row[5],
                "step": int(self.step)}

    def load_state_dict(self, state):
        """Takes s, m and v (and the schedule's step); ValueError for another mode or a missing or non-finite entry.  In scheduled mode
        the next tick overwrites the value from ``step``."""
        if not isinstance(state, dict) or state.get("mode") != self.mode:
            raise ValueError(f"the saved temperature has mode {state.get('mode') if isinstance(state, dict) else state!r}, "
                             f"this one is {self.mode!r}")
        try:
            s, m, v = (float(state[k]) for k in ("s", "m", "v"))
        except (KeyError, TypeError, ValueError):
            raise ValueError("the saved temperature needs finite numbers 's', 'm' and 'v'") from None
        if not all(math.isfinite(x) for x in (s, m, v)):
            raise ValueError("the saved temperature needs finite numbers 's', 'm' and 'v'")
        extra = {k: float(state[k]) for k in ("scale", "tau") if isinstance(state.get(k), float) and math.isfinite(state[k])}
        g = float(state["g"]) if isinstance(state.get("g"), float) and math.isfinite(state["g"]) else 0.0
        self._fill(math.exp(-s), m, v, g, s=s, **extra)
        self.step = int(state.get("step", self.step))

    def __repr__(self):
        return f"DeviceTemperature(mode={self.mode!r}, schedule={self.schedule!r}, lr_scale={self.lr_scale})"


def check_negatives_supported(negatives, all_timesteps=False, global_negatives=None, gradient_penalty=None, negative_groups=None):
    """Sampled negatives (``negatives = (n_neg, seed, draw)``) and grouped negatives (``negative_groups = (groups, mode)``) exist for
    the default loss branch on one process's own batch; what they do not cover is refused here, before any launch."""
    if negatives is None and negative_groups is None:
        return
    if negatives is None:
        if all_timesteps:
            raise NotImplementedError("grouped negatives are defined for score_over_all_timesteps=False only: the all-timesteps "
                                      "branch contrasts every (item, step) pair, and no selection over that set exists")
        if global_negatives is not None:
            raise NotImplementedError("grouped negatives are chosen from the process's own batch; with a global_negatives object the "
                                      "candidates would span the gathered batches of all ranks, whose group ids this rank does not hold")
        if gradient_penalty is not None:
            raise NotImplementedError("the gradient penalty's tangent passes run the dense loss kernels; grouped negatives are not "
                                      "carried through them")
        return
    if all_timesteps:
        raise NotImplementedError("sampled negatives are defined for score_over_all_timesteps=False only: the all-timesteps branch "
                                  "contrasts every (item, step) pair, and no sampler over that set exists")
    if global_negatives is not None:
        raise NotImplementedError("sampled negatives draw from the process's own batch; with a global_negatives object the candidates "
                                  "would span the gathered batches of all ranks, which the sampler does not index")
    if gradient_penalty is not None:
        raise NotImplementedError("the gradient penalty's tangent passes run the dense loss kernels; sampled negatives are not "
                                  "carried through them")


def normalize_negatives(negatives, B):
    """(n_neg, seed, draw) as Python ints the C ABI takes (seed and draw modulo 2^64); ValueError unless 1 <= n_neg <= B - 1."""
    n_neg, seed, draw = negatives
    return check_negatives(B, n_neg), int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)


def normalize_negative_groups(negative_groups, B, negatives=None):
    """(groups, mode, n_neg, seed, draw) as cpc_nce_loss_grouped takes them: ``negative_groups = (groups, mode)`` with groups an int32
    tensor [B] and mode "same" / "other"; ``negatives`` None (n_neg = 0: every eligible row) or (n_neg, seed, draw).  ValueError /
    TypeError for anything else."""
    groups, mode = negative_groups
    mode = group_mode(mode)
    n_neg, seed, draw = (0, 0, 0) if negatives is None else normalize_negatives(negatives, B)
    if not isinstance(groups, torch.Tensor) or groups.dtype != torch.int32:
        raise TypeError("negative_groups: groups must be an int32 tensor")
    if tuple(groups.shape) != (int(B),) or not groups.is_contiguous():
        raise ValueError(f"negative_groups: groups must be a contiguous tensor of shape [{int(B)}], got {tuple(groups.shape)}")
    return groups, mode, check_group_negatives(B, n_neg), seed, draw


MAX_BANK_SLOTS = 64          # the valid mask of cpc_nce_loss_banked is one 64-bit word


def check_slots_back(slots_back):
    """M, the number of earlier steps a negative bank keeps, as an int; ValueError unless it is an integer in [1, MAX_BANK_SLOTS - 1]."""
    if isinstance(slots_back, bool) or not isinstance(slots_back, int) or not 1 <= slots_back <= MAX_BANK_SLOTS - 1:
        raise ValueError(f"a negative bank keeps 1 .. {MAX_BANK_SLOTS - 1} earlier steps, got {slots_back!r}")
    return slots_back


class NegativeBank:
    """Cross-batch memory of the InfoNCE loss ("Negative bank"): a ring of ``slots_back`` + 1 slots of B prediction rows,
    ring[slot B + b][k][:] in the engine's storage dtype.  Every banked loss call copies its score operands (predicted_z; the
    normalised, 1 / temperature-scaled rows of "normalized" scores) into slot ``cur``, contrasts the targets against the rows of all
    slots whose bit is set in ``valid`` — the earlier steps' rows as constants — and then moves ``cur`` on.  The ring is allocated by
    the first call from that engine's (B, K, E, dtype, device); host state only (cur, valid), so not for a captured step."""

    def __init__(self, slots_back):
        self.slots = check_slots_back(slots_back) + 1
        self.cur, self.valid = 0, 1
        self.ring = self.sizes = None

    @property
    def filled(self):
        """How many slots hold an earlier step's rows."""
        return bin(self.valid).count("1") - 1

    def reset(self):
        """Forgets the earlier steps: the next banked call is the in-batch loss again.  The rows are zeroed, so that the score GEMM
        over the whole ring never meets what an abandoned run left (0 x NaN in the target contraction)."""
        self.valid = 1 << self.cur
        if self.ring is not None:
            self.ring.zero_()

    def bind(self, B, K, E, dtype, device):
        """Allocates the ring on first use; ValueError (naming both) when a later caller has other sizes."""
        sizes = (int(B), int(K), int(E), dtype, torch.device(device))
        if self.ring is None:
            self.sizes = sizes
            self.ring = torch.zeros(self.slots * sizes[0], sizes[1], sizes[2], dtype=dtype, device=device)
        elif sizes != self.sizes:
            raise ValueError(f"this negative bank holds rows of (B, K, E, dtype, device) = {self.sizes}, the call has {sizes}: "
                             "a bank belongs to one engine (reset() does not change its sizes; make a new NegativeBank)")

    def slot(self, i):
        """The [B][K][E] rows of slot i (a view)."""
        B = self.sizes[0]
        return self.ring[i * B:(i + 1) * B]

    def advance(self):
        """After a step: the slot just written becomes an earlier step's, the next one (whose bit is set at once: it is filled before
        any score is formed) takes the coming step's rows."""
        self.cur = (self.cur + 1) % self.slots
        self.valid |= 1 << self.cur


def check_negative_bank_supported(negative_bank, all_timesteps=False, global_negatives=None, gradient_penalty=None, negatives=None,
                                  negative_groups=None, kind=None, temperature=None, graphed=False):
    """A negative bank exists for the default loss branch of one process's own step with dot-product scores and a constant
    temperature; what it does not cover is refused here, before any launch."""
    if negative_bank is None:
        return
    if not isinstance(negative_bank, NegativeBank):
        raise TypeError(f"negative_bank must be None or a NegativeBank, got {negative_bank!r}")
    if all_timesteps:
        raise NotImplementedError("a negative bank is defined for score_over_all_timesteps=False only: its rows are the predictions "
                                  "of one step k each, and the all-timesteps branch contrasts every (item, step) pair")
    if global_negatives is not None:
        raise NotImplementedError("a negative bank holds the process's own earlier predictions; with a global_negatives object the "
                                  "candidates span the gathered batches of all ranks, whose loss kernels know no bank")
    if gradient_penalty is not None:
        raise NotImplementedError("the gradient penalty's tangent passes run the dense loss kernels; a negative bank is not carried "
                                  "through them")
    if graphed:
        raise NotImplementedError("a negative bank keeps its cursor and its mask of filled slots on the host and changes them every "
                                  "step, which a captured graph cannot replay")
    if negatives is not None or negative_groups is not None:
        raise NotImplementedError("a negative bank together with sampled or grouped negatives: no selection over the rows of earlier "
                                  "steps exists (their group ids and draws are gone)")
    if kind == "difference":
        raise NotImplementedError("a negative bank with difference scores: the banked scores come from the score GEMM, and "
                                  "cpc_diff_scores takes no ring of earlier predictions")
    if isinstance(temperature, DeviceTemperature):
        raise NotImplementedError("a negative bank with a learnable or scheduled temperature: the rows of earlier steps carry the "
                                  "1 / temperature of their own step and are constants, so neither the scale nor its gradient "
                                  "would be the current one")


def select_negatives(B, negatives, negative_groups, all_timesteps=False, global_negatives=None, negative_bank=None, kind=None,
                     temperature=None):
    """The negative selection of a loss call, checked (check_negatives_supported, check_negative_bank_supported) and normalised once
    for every score kind, as the loss-kernel stage takes it: None (the whole batch), ("sampled", n_neg, seed, draw),
    ("grouped", groups, mode, n_neg, seed, draw) or ("banked", bank)."""
    if negative_bank is not None:
        check_negative_bank_supported(negative_bank, all_timesteps, global_negatives, None, negatives, negative_groups, kind, temperature)
        return ("banked", negative_bank)
    if negative_groups is not None:
        check_negatives_supported(negatives, all_timesteps, global_negatives, negative_groups=negative_groups)
        return ("grouped",) + normalize_negative_groups(negative_groups, B, negatives)
    if negatives is not None:
        check_negatives_supported(negatives, all_timesteps, global_negatives)
        return ("sampled",) + normalize_negatives(negatives, B)
    return None


class EncoderGeometry:
    """Valid and allocated lengths of every encoder layer for clips of ``length`` samples."""

    def __init__(self, length: int, strides: Sequence[int], kernel_sizes: Sequence[int]):
        self.strides = [int(s) for s in strides]
        self.kernels = [int(k) for k in kernel_sizes]
        n = len(self.strides)
        cur = int(length)
        self.valid: List[int] = []
        for s, k in zip(self.strides, self.kernels):
            cur = (cur - k) // s + 1
            if cur <= 0:
                raise ValueError(f"clips of {length} samples are shorter than the encoder's receptive field")
            self.valid.append(cur)
        self.taps = [_ceil_div(k, s) for s, k in zip(self.strides, self.kernels)]    # D_l: output rows per input position
        pad_top = 1
        while True:
            alloc = [0] * n
            alloc[n - 1] = self.valid[n - 1] + pad_top
            for l in range(n - 1, 0, -1):
                alloc[l - 1] = self.strides[l] * alloc[l]
            if all(alloc[l] - self.valid[l] >= max(self.taps[l] - 1, 0) for l in range(n)):
                break
            pad_top += 1
            if pad_top > 4096:
                raise ValueError("could not find a padded layout for this encoder configuration")
        self.alloc = alloc
        self.frames = self.valid[-1]


ANCHOR_LOSS_REASON = ("prediction_anchors > 1 runs the equal-step InfoNCE loss over the whole batch with softplus or linear scores: "
                      "score_over_all_timesteps, sampled / grouped / banked / global negatives and difference / normalized scores index "
                      "K heads per item and are not stacked over anchors")


def check_anchor_context(model, scalogram=False):
    """prediction_anchors > 1 needs every hidden state of a recurrence: AudioGRUModel / AudioLSTMModel in the waveform engine."""
    A = int(getattr(model, "prediction_anchors", 1))
    if A <= 1:
        return
    from .audio_model import AudioGRUModel, AudioLSTMModel
    ar = model.autoregressive_model
    if scalogram:
        raise NotImplementedError(f"prediction_anchors = {A}: the scalogram / grid engines expose the context c at the last position only; "
                                  "anchors are on the waveform engine with an AudioGRUModel or AudioLSTMModel")
    if not isinstance(ar, (AudioGRUModel, AudioLSTMModel)):
        raise NotImplementedError(f"prediction_anchors = {A}: {type(ar).__name__} exposes the context c at the last position only (no "
                                  "hidden state per visible step to predict from); anchors need an AudioGRUModel or AudioLSTMModel")


class CPCEngine(ContextHost):
    A, s = 1, 1                 # prediction anchors and their stride (set by __init__; ScalogramCPCEngine keeps 1)

    @property
    def AK(self):
        """Heads of the loss: K prediction steps of each of the A anchors."""
        return self.A * self.K

    def __init__(self, model, batch_size: int, length: int, device, dtype: torch.dtype):
        enc, ar = model.encoder, model.autoregressive_model
        check_anchor_context(model)          # (refused before anything is allocated or launched)
        super().__init__(model, device, dtype, batch_size, enc.channel_count[-1], model.ar_size, model.prediction_steps, model.visible_steps)
        # prediction anchors ("Prediction anchors"): A hidden states of the one recurrence predict, s steps apart; AK heads
        self.A, self.s = int(getattr(model, "prediction_anchors", 1)), int(getattr(model, "anchor_stride", 1))
        self.L = int(length)
        self.strides = list(enc.strides)
        self.kernels = list(enc.kernel_sizes)
        self.channels = list(enc.channel_count)
        self.n = len(self.strides)
        full = EncoderGeometry(self.L, self.strides, self.kernels)
        if full.frames < self.V + self.K:
            raise ValueError(f"clips give {full.frames} encoder frames, need visible+prediction = {self.V + self.K}")
        # The model only consumes the last V+K encoder frames (audio_model.py:197-198); frame t depends on samples
        # >= t * downsampling only, so the leading frames the reference computes and discards are never computed here:
        # the encoder runs on the clip from sample x_off on.  Results (outputs, loss, gradients) are unchanged.
        self.frames_full = full.frames
        skip = full.frames - (self.V + self.K) if (self.V + self.K) > 0 else 0
        self.x_off = skip * int(enc.downsampling_factor)
        self.L_eff = self.L - self.x_off
        self.geo = EncoderGeometry(self.L_eff, self.strides, self.kernels)
        self.T = self.geo.frames
        assert self.T == full.frames - skip
        if model.enc_size != self.E:
            raise ValueError("enc_size does not match the encoder's last channel count")
        self._check_supported()
        self.ctx = make_context(self, ar) if (self.V + self.K) > 0 else None
        self._alloc()

    # Step-control state with its defaults, beside those a context may read (ContextHost: use_aux, _gp_phase, gp_capable)
    _deferred_side = ()         # calls backward() put off the main stream, for the encoder backward's first side-stream block
    _bl_active = None           # the backward target lane (_bwd_lane) of the pass in flight, or None
    fuse_c1 = False             # layer 2's data gradient fused with layer 1's weight / bias gradient (_alloc_encoder)

    # ------------------------------------------------------------------------------------------ setup
    def _check_supported(self):
        ch = 8 if self.dt == torch.bfloat16 else 4
        for l in range(1, self.n):
            if (self.kernels[l] * self.channels[l - 1]) % ch or self.channels[l] % 8:
                raise NotImplementedError("HIP conv path needs channel counts that are multiples of 8")
        c0 = self.channels[0]
        if c0 % 8 or 256 % (c0 // 8) or self.kernels[0] > 16 or self.strides[0] > 8:
            raise NotImplementedError("HIP layer-1 kernel: channels in {8,16,...,2048}, kernel <= 16, stride <= 8")
        if self.E % ch:
            raise NotImplementedError("enc_size must be a multiple of 8")

    def _alloc(self):
        need = self._alloc_encoder()
        self._alloc_head(need)

    def _alloc_encoder(self):
        """Activation / gradient buffers and weight operands of the AudioEncoder stack; returns the slab sizes it needs."""
        dev, dt = self.device, self.dt
        B, n = self.B, self.n
        La = self.geo.alloc
        self.act, self.dact = [], []
        self._keep = []
        # guard rows: act[l] is read (kernel - stride) rows past its end by layer l+1's forward / weight gradient, dact[l] is
        # read (taps - 1) rows before its start by layer l's data gradient
        self.guard_rows = max([16] + [self.kernels[l] - self.strides[l] for l in range(1, n)] + [t - 1 for t in self.geo.taps[1:]])
        self.guard = []
        for l in range(n):
            for store in (self.act, self.dact):
                full, view, g_el = self._buf(B * La[l], self.channels[l], self.guard_rows)
                self._keep.append(full)
                store.append(view)
            self.guard.append(g_el)
        # Sign-bit mask of layer 1's output (include/cpc_hip.h, cpc_sign_bits): act[0] > 0 as one byte per 8 elements, written by the
        # layer-1 forward kernel and read by the data gradient of layer 2 (the fused one) in place of act[0]: the tile's 8 KiB of
        # bits arrive by LDS-DMA before its K loop, so the epilogue of a tile reads no mask from memory (it used to end in a 32 MB
        # burst per round of tiles; 0.96 GB of the launch's traffic).  Measured (tools/bits_ab.py, B = 256): that launch 1 035 ->
        # 950 us, layer-1 forward +20 us.  For the deeper layers the same trade is even (the forward GEMMs' epilogues pay 2-6 % for
        # writing the bits — one workgroup per CU, nothing to hide an epilogue instruction behind — and a separate kernel costs what
        # the data gradients gain — also when that kernel runs on the side stream while the GRU leaves 240 CUs idle: 4.52 -> 4.57 ms per
        # step), so they keep reading their masks from the activations.
        self.act_bits: List[Optional[torch.Tensor]] = [None] * n
        if (dt == torch.bfloat16 and n >= 2 and self.channels[0] == 512
                and _hip.nt_tile(self.code, B * La[1], self.strides[1] * 512, self.geo.taps[1] * self.channels[1]) == 256
                and self.guard[0] % 128 == 0):
            full = torch.zeros((2 * self.guard[0] + B * La[0] * 512) // 8, device=dev, dtype=torch.uint8)
            self._keep.append(full)
            self.act_bits[0] = full[self.guard[0] // 8:]
        # Bias gradients of layers 2 .. n-1 (indices 1 .. n-2) from the data gradient of the layer above: its epilogue leaves the
        # column sums of every 256-row tile it stores (include/cpc_hip.h, dx_colsum_slabs), and a small reduction replaces the
        # column-sum pass over the 0.06-0.24 GB gradient (beside the main-stream GEMMs those passes cost the step 58 us,
        # CPC_PROBE runs).  bf16 and 256 x 256 tiles only; the top layer's gradient comes from other kernels and keeps its pass.
        self.cs_slabs: List[Optional[torch.Tensor]] = [None] * n       # cs_slabs[l]: sums of dact[l], written by layer l+1's data gradient
        if dt == torch.bfloat16:
            for l in range(2, n):
                cin, cout, s = self.channels[l - 1], self.channels[l], self.strides[l]
                if _hip.nt_tile(self.code, B * La[l], s * cin, self.geo.taps[l] * cout) == 256 and (s * cin) % 8 == 0:
                    nf = int(_hip.lib().cpc_conv_dgrad_colsum_floats(B, cin, s, La[l]))
                    self.cs_slabs[l - 1] = torch.zeros(nf, device=dev, dtype=torch.float32)
        # weight operand layouts (storage dtype)
        self.w_fwd: List[Optional[torch.Tensor]] = [None] * n
        self.w_dgrad: List[Optional[torch.Tensor]] = [None] * n
        self._w_dgrad_alt: List[Optional[torch.Tensor]] = [None] * n      # see prepare_ahead
        for l in range(1, n):
            cin, cout, kw, s = self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l]
            self.w_fwd[l] = torch.empty(cout * kw * cin, device=dev, dtype=dt)
            self.w_dgrad[l] = torch.empty(s * cin * self.geo.taps[l] * cout, device=dev, dtype=dt)
        need = [1]
        self.nsplit = [1] * n
        for l in range(1, n):
            I, J, M = self.kernels[l] * self.channels[l - 1], self.channels[l], B * La[l]
            self.nsplit[l] = self._pick_split(I, J, M)
            need.append(self.nsplit[l] * I * J)
        self.c1_blocks = max(1, min(8, _ceil_div(self.geo.valid[0], 512)))
        self.c1_item_blocks = min(B, 128)
        need.append(self.c1_item_blocks * self.c1_blocks * (self.kernels[0] + 1) * self.channels[0])
        need.append(self.colsum_blocks * max(self.channels))
        # bf16, wide first layer: the data gradient of layer 2 is fused with the weight / bias gradient of layer 1
        # (cpc_conv_dgrad_conv1): the 1 GB gradient of layer 1's output is neither written nor read back
        if n >= 2 and dt == torch.bfloat16 and self.channels[0] % 256 == 0 and self.kernels[0] <= 15:
            s1, c0, c1 = self.strides[1], self.channels[0], self.channels[1]
            if _hip.nt_tile(self.code, B * La[1], s1 * c0, self.geo.taps[1] * c1) == 256 and (self.geo.taps[1] * c1) % 64 == 0:
                nf = [int(_hip.lib().cpc_conv_dgrad_conv1_floats(B, c0, s1, La[1], self.kernels[0], w)) for w in (0, 1)]
                self.c1_slabs = torch.empty(nf[0], device=dev, dtype=torch.float32)
                self.c1_tmp = torch.empty(nf[1], device=dev, dtype=torch.float32)
                self.fuse_c1 = True
        # Side stream for the short, latency-bound kernels of the weight-gradient path (bias column sums, slab reductions): they run beside the large GEMMs of the main stream instead of between them.  The big
        # GEMMs all stay on the main stream.  Each layer's weight-gradient slabs get their own buffer so that the next layer's
        # GEMM never waits for the previous reduction.
        self.wslab = [None] + [torch.empty(need[l], device=dev, dtype=torch.float32) for l in range(1, n)]
        self.aux_slabs = torch.empty(self.colsum_blocks * max(self.channels), device=dev, dtype=torch.float32)
        self._ev_d = [torch.cuda.Event() for _ in range(n)]
        self._ev_w = [torch.cuda.Event() for _ in range(n)]
        return need

    def _alloc_head(self, need):
        """Predictor / loss state, the context network's buffers and the shared split-reduction workspace."""
        dev, dt, f32 = self.device, self.dt, torch.float32
        B, H, E, K = self.B, self.H, self.E, self.K
        self.w_p = torch.empty(K * E * H, device=dev, dtype=dt)           # [K*E][H]
        self.w_p_t = torch.empty(H * K * E, device=dev, dtype=dt)         # [H][K*E]
        self.c = torch.empty(B, H, device=dev, dtype=f32)
        self.pred = torch.empty(B * K * E, device=dev, dtype=dt)
        self.ldS = _ceil_div(B, 8) * 8
        self.S = torch.zeros(K * B * self.ldS, device=dev, dtype=f32)
        self.dS = torch.zeros(K * B * self.ldS, device=dev, dtype=dt)
        self.dST = torch.zeros(K * B * self.ldS, device=dev, dtype=dt)
        self.nce_out = torch.zeros(8, device=dev, dtype=f32)
        self.nce_ws = torch.empty(int(_hip.lib().cpc_nce_workspace_floats(B, K)), device=dev, dtype=f32)
        self.dpred = torch.zeros(B * K * E, device=dev, dtype=dt)
        self.dc = torch.zeros(B, H, device=dev, dtype=f32)
        need = list(need)
        need.append(_ceil_div(max(K * E, 1), 256) * B * H)               # split-K slabs of the dc GEMM
        if self.ctx is not None:
            self.ctx.allocate()
            need.append(self.ctx.slab_floats())
        if self.A > 1:
            need.append(self._alloc_anchors())
        self.slabs = torch.empty(max(need), device=dev, dtype=f32)

    def _alloc_anchors(self):
        """Prediction anchors: the head's buffers again for AK heads ([B][AK][E] predictions, AK score blocks), every anchor's target
        gradients dT f32 [A][B][K][E], the B A rows of dc, and the top recurrent layer's dHs [B][V][H] — zeroed once here; the same A - 1
        rows per item are rewritten every step.  Returns the floats the split-K slabs of the dc GEMM need."""
        dev, dt, f32 = self.device, self.dt, torch.float32
        B, H, E, K, V, A, AK = self.B, self.H, self.E, self.K, self.V, self.A, self.AK
        if self.ctx is None or not self.ctx.anchors_ok:
            raise NotImplementedError(f"prediction_anchors = {A}: {type(self.ctx).__name__} exposes c at the last position only")
        self.pred = torch.empty(B * AK * E, device=dev, dtype=dt)
        self.dpred = torch.zeros(B * AK * E, device=dev, dtype=dt)
        self.S = torch.zeros(AK * B * self.ldS, device=dev, dtype=f32)
        self.dS = torch.zeros(AK * B * self.ldS, device=dev, dtype=dt)
        self.dST = torch.zeros(AK * B * self.ldS, device=dev, dtype=dt)
        self.nce_ws = torch.empty(int(_hip.lib().cpc_nce_workspace_floats(B, AK)), device=dev, dtype=f32)
        self.dT = torch.zeros(A * B * K * E, device=dev, dtype=f32)
        self.dcA = torch.zeros(B * A, H, device=dev, dtype=f32)
        self.ctx.anchor_dHs = torch.zeros(B * V * H, device=dev, dtype=dt)
        # step index t of dHs that anchor a < A - 1 writes: its context is h_{V - d_a} = the state after step t = V - d_a - 1
        self._anchor_steps = torch.tensor([V - (A - 1 - a) * self.s - 1 for a in range(A - 1)], device=dev, dtype=torch.long)
        return _ceil_div(max(K * E, 1), 256) * B * A * H

    # ---------------------------------------------------------------------------------- weight layouts
    def prepare_weights(self):
        """f32 master parameters (reference state_dict shapes) -> storage-dtype GEMM operand layouts.  Skipped when
        prepare_ahead() already rebuilt every operand copy after the last parameter update and nothing has touched the
        parameters since."""
        token, self._ahead_token = getattr(self, "_ahead_token", None), None
        ev = getattr(self, "_ahead_ev", None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev[1])      # a side-stream rebuild (_prepare_all_ahead), current or stale, has finished
        if token is not None and token == self._param_state():
            return
        self._prepare_encoder_weights()
        self._prepare_head_weights()

    def _prepare_all_ahead(self):
        """Every operand copy of the next step rebuilt on the side stream, behind everything issued so far (the step's last Adam launch):
        the layout kernels then run beside the head of the next step instead of in front of its first convolution.  prepare_weights()
        waits for their event."""
        if getattr(self, "_ahead_ev", None) is None:
            self._ahead_ev = (torch.cuda.Event(), torch.cuda.Event())
        with self.side(self._ahead_ev[0]):
            self._prepare_encoder_weights()
            self._prepare_head_weights()
            self._ahead_ev[1].record(self.aux)
        self._ahead_token = self._param_state()

    def _prepare_head_weights(self):
        p, code = self.model._param, self.code
        H, E, K = self.H, self.E, self.K
        if self.ctx is None:          # encoder-only engine (stand-alone AudioEncoder call)
            return
        self.ctx.prepare_weights()
        w_p = p["prediction_model.weight"]
        _hip.call("cpc_cast2d", _hip.ptr(w_p), _hip.ptr(self.w_p), K * E, H, H, 1, code)
        _hip.call("cpc_cast2d", _hip.ptr(w_p), _hip.ptr(self.w_p_t), H, K * E, 1, H, code)

    def _prepare_encoder_weights(self):
        for l in range(1, self.n):
            self._prepare_conv(l, True, True)

    def _prepare_conv(self, l, fwd, dgrad, alt=False):
        w = self.model._param[f"encoder.layers.{l}.weight"]
        wd = None
        if dgrad:
            wd = self.w_dgrad[l]
            if alt:          # the current copy is still being read: build the next one in a second buffer (swapped in later)
                if self._w_dgrad_alt[l] is None:
                    self._w_dgrad_alt[l] = torch.empty_like(self.w_dgrad[l])
                wd = self._w_dgrad_alt[l]
        _hip.call("cpc_conv_w_prep", _hip.ptr(w), _hip.ptr(self.w_fwd[l]) if fwd else None, _hip.ptr(wd), self.channels[l],
                  self.channels[l - 1], self.kernels[l], self.strides[l], self.code)

    # Operand copies for the NEXT step, rebuilt as soon as the optimizer has updated their parameters (single-process training):
    # the ten layout kernels (0.1 ms at B = 256) then run on the side stream beside the remaining backward GEMMs instead of in
    # front of the next step's first convolution.
    supports_prepare_ahead = True

    def _param_state(self):
        """Changes whenever the parameters may have changed: torch's version counters catch in-place torch ops on the
        parameters (load_state_dict, torch optimizers), model._raw_updates counts the fused optimizer's raw-pointer updates."""
        m = self.model
        return (sum(p._version for p in m.parameters()) + m._flat_param._version, getattr(m, "_raw_updates", 0),
                m._flat_param.data_ptr())

    def prepare_ahead(self, lo, hi, final):
        """FusedAdam calls this right after it updated flat_param[lo:hi): from the backward pass's grad_ready_hook (on the
        side stream; ``final`` False) and from step() for the head of the buffer (``final`` True, main stream, backward
        complete).  In a hook call the lowest updated encoder layer's data-gradient operand is still being read by that
        layer's data-gradient GEMM on the main stream: its next copy is built in a second buffer, swapped in by the final call."""
        if not self.supports_prepare_ahead or self.ctx is None or not self.ctx.ahead_ok or not switches.prepare_ahead():
            return
        st = getattr(self, "_ahead", None)
        # (one Adam launch over everything, no gradient-ready pieces: the copies are rebuilt here, on the main stream behind Adam.  Doing that on
        # the side stream instead -- _prepare_all_ahead, as the scalogram engine does beside its CQT GEMMs -- was measured SLOWER for this
        # engine: the next step opens with the HBM-bound layer-1 kernel and the layer-2 GEMM, and eleven small high-priority layout kernels
        # beside them cost more than they save: conv_ar 4.202 against 4.186 ms, attention 4.674 against 4.625, interleaved runs on one box)
        if st is None:
            st = self._ahead = {"conv": set(), "head": False, "swap": []}
        off = self.model._offset
        updated = [l for l in range(1, self.n) if lo <= off[f"encoder.layers.{l}.weight"] < hi]
        for l in updated:
            busy = (not final) and l == min(updated)
            self._prepare_conv(l, True, True, alt=busy)
            st["conv"].add(l)
            if busy:
                st["swap"].append(l)
        if lo <= off["prediction_model.weight"] < hi:
            self._prepare_head_weights()
            st["head"] = True
        if final:
            for l in st["swap"]:
                self.w_dgrad[l], self._w_dgrad_alt[l] = self._w_dgrad_alt[l], self.w_dgrad[l]
            complete = st["head"] and st["conv"] == set(range(1, self.n))
            self._ahead = None
            self._ahead_token = self._param_state() if complete else None

    # ------------------------------------------------------------------------------------------ forward
    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("the CPC hot path runs on the GPU only (no CPU fallback): move the batch to the device")
        if x.dtype != torch.float32 or tuple(x.shape) != (self.B, self.L) or not x.is_contiguous():
            raise ValueError(f"expected a contiguous float32 batch of shape ({self.B}, {self.L}), got {tuple(x.shape)} {x.dtype}")

    # ---- the rows only the TARGETS need, beside the GRU recurrence -------------------------------------------------------------
    # The context network reads the first V of the V + K top-layer frames; frames V .. V+K-1 are the targets (audio_model.py:197-198).
    # With unpadded causal convolutions top rows [0, V) need rows [0, n_l) of layer l, n_{l-1} = s_l (n_l - 1) + k_l — a prefix of every
    # layer.  The GRU occupies 16 of the 256 CUs for 0.27 ms (100 dependent steps): the remaining rows of every layer (11 % of the encoder's
    # forward work at V = 100, K = 12) are computed on the side stream while it runs, and the main stream's forward launches are
    # that much shorter.  Same kernels on row ranges, identical results (_tl_rows = None: one launch per layer).
    def _target_lane_rows(self):
        """n_l per layer (rows of layer l that the context network's frames depend on), or None when the split does not apply."""
        if getattr(self, "_tl_rows", 0) != 0:
            return self._tl_rows
        self._tl_rows = None
        if (not self.use_aux or not isinstance(self.ctx, GRUContext) or self.K <= 0
                or self.V <= 0 or self.n < 2 or self.T != self.V + self.K):
            return None
        La = self.geo.alloc
        n = [0] * self.n
        n[-1] = self.V
        for l in range(self.n - 1, 0, -1):
            n[l - 1] = self.strides[l] * (n[l] - 1) + self.kernels[l]
        if any(n[l] >= La[l] or n[l] <= 0 for l in range(self.n)):
            return None
        # (worth it only where the side lane is small and the main lane still fills the chip)
        if n[-1] * 4 < La[-1] * 3 or self.B * n[-1] < 4096:
            return None
        self._tl_rows = n
        self._tl_ev = (torch.cuda.Event(), torch.cuda.Event())
        return n

    def _row_launch_tile(self, M, N):
        """CPC_GEMM_BIG_TILE for a row-range launch that is ONE nearly full round of 256 x 256 tiles (the launcher's own rule takes the
        256-wide tile from 200 tiles on): layer 2's target rows at the headline size are 196 such tiles — 0.11 ms in one round against
        0.135 ms as 784 128-wide tiles on 512 slots."""
        tiles = _ceil_div(M, 256) * _ceil_div(N, 256)
        return _hip.GEMM_BIG_TILE if (self.dt == torch.bfloat16 and 160 <= tiles < 200 and N % 256 == 0) else 0

    def _encoder_rows(self, x, lo, hi):
        """Layers 1 .. n on rows [lo[l], hi[l]) of every item (hi[l] = L_alloc[l]: to the end, pad rows included)."""
        p, code, B, La, Lv = self.model._param, self.code, self.B, self.geo.alloc, self.geo.valid
        _hip.call("cpc_conv1_fwd_rows", _hip.ptr(x, self.x_off), _hip.ptr(p["encoder.layers.0.weight"]), _hip.ptr(p.get("encoder.layers.0.bias")),
                  _hip.ptr(self.act[0]), B, self.channels[0], self.strides[0], self.kernels[0], self.L, Lv[0], La[0],
                  1 if self.n > 1 else 0, code, _hip.ptr(self.act_bits[0]), lo[0], hi[0],
                  key="cpc_conv1_fwd" if lo[0] == 0 else "cpc_conv1_fwd_target_rows")
        for l in range(1, self.n):
            cin, cout, kw, s = self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l]
            r0, rows = lo[l], hi[l] - lo[l]
            M = B * rows
            _hip.gemm_nt(_hip.ptr(self.act[l - 1], r0 * s * cin), _hip.ptr(self.w_fwd[l]), _hip.ptr(self.act[l], r0 * cout), M, cout, kw * cin,
                         s * cin, kw * cin, cout, code, bias=_hip.ptr(p.get(f"encoder.layers.{l}.bias")),
                         a_rpi=rows, a_item=La[l - 1] * cin, c_rpi=rows, c_item=La[l] * cout, c_valid=max(0, min(Lv[l], hi[l]) - r0),
                         flags=(_hip.GEMM_RELU if l < self.n - 1 else 0) | self._row_launch_tile(M, cout))

    def encoder_forward(self, x):
        """AudioEncoder.forward (audio_model.py:36-44): relu(conv) x (n-1), then a bare conv."""
        self._check_input(x)
        p, code, B, La, Lv = self.model._param, self.code, self.B, self.geo.alloc, self.geo.valid
        # (only inside forward(), which joins the lanes again; not under a hipGraph capture, which runs on one stream)
        nrows = self._target_lane_rows() if (self._tl_in_forward and self.use_aux) else None
        if nrows is not None:
            self._encoder_rows(x, [0] * self.n, nrows)                       # what the context network needs: main stream
            ev0, ev1 = self._tl_ev
            ev0.record(torch.cuda.current_stream())
            with torch.cuda.stream(self.aux):
                self.aux.wait_event(ev0)
                self._encoder_rows(x, nrows, list(La))                      # what only the targets need: side stream, beside the GRU
                ev1.record(self.aux)
            self._tl_pending = ev1
            return
        _hip.call("cpc_conv1_fwd", _hip.ptr(x, self.x_off), _hip.ptr(p["encoder.layers.0.weight"]), _hip.ptr(p.get("encoder.layers.0.bias")),
                  _hip.ptr(self.act[0]), B, self.channels[0], self.strides[0], self.kernels[0], self.L, Lv[0], La[0],
                  1 if self.n > 1 else 0, code, _hip.ptr(self.act_bits[0]))
        for l in range(1, self.n):
            _hip.call("cpc_conv_fwd", _hip.ptr(self.act[l - 1]), _hip.ptr(self.w_fwd[l]), _hip.ptr(p.get(f"encoder.layers.{l}.bias")),
                      _hip.ptr(self.act[l]), B, self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l],
                      La[l], Lv[l], 1 if l < self.n - 1 else 0, C.c_longlong(self.guard[l - 1]), code,
                      key="gemm_nt" + _hip._variant(code, 0, _hip.nt_tile(code, B * La[l], self.channels[l], self.kernels[l] * self.channels[l - 1])),
                      work=2.0 * B * La[l] * self.channels[l] * self.kernels[l] * self.channels[l - 1],
                      shape=("fwd", B * La[l], self.channels[l], self.kernels[l] * self.channels[l - 1]))

    def context_forward(self):
        """c = autoregressive_model(z) over z = frames [T-K-V, T-K) (audio_model.py:198-204), then prediction_model (:208)."""
        code, B, H, E, K = self.code, self.B, self.H, self.E, self.K
        self.ctx.forward()
        ct, coff, cstride = self.ctx.c_operand()
        if self.A > 1:          # B A rows straight out of the hidden states: row (b, a) = h_{V - (A-1-a) s}; pred [B][AK][E]
            A, s = self.A, self.s
            _hip.gemm_nt(_hip.ptr(ct, coff - (A - 1) * s * H), _hip.ptr(self.w_p), _hip.ptr(self.pred), B * A, K * E, H, s * H, H, K * E,
                         code, a_rpi=A, a_item=cstride)
        else:
            _hip.gemm_nt(_hip.ptr(ct, coff), _hip.ptr(self.w_p), _hip.ptr(self.pred), B, K * E, H, H, H, K * E, code,
                         a_rpi=1, a_item=cstride)
        ev = getattr(self, "_tl_pending", None)
        if ev is not None:          # the target rows of the encoder (side stream, see encoder_forward) are complete from here on
            torch.cuda.current_stream().wait_event(ev)
            self._tl_pending = None

    def forward(self, x):
        self.prepare_weights()
        self._nbt_batch = []          # BatchNorm `num_batches_tracked` counters of this pass: ONE multi-tensor add instead of a launch each
        self._tl_in_forward = True
        try:
            self.encoder_forward(x)
            self.context_forward()
        finally:
            self._tl_in_forward = False
            batch, self._nbt_batch = self._nbt_batch, None
            if batch:
                torch._foreach_add_(batch, 1)

    _tl_in_forward = False

    def _anchor_rows(self):
        """First target row of every anchor: T - K - d_a, d_a = (A - 1 - a) s."""
        return [self.T - self.K - (self.A - 1 - a) * self.s for a in range(self.A)]

    # views of the forward results in the reference's shapes (storage dtype, no copies)
    def view_top(self):
        return self.act[-1].view(self.B, self.geo.alloc[-1], self.E)

    def outputs(self):
        """(predicted_z (B,K,E), targets (B,E,K), z (B,E,V), c (B,H)) as float32 tensors in the reference's shapes."""
        top = self.view_top()
        T, K, V = self.T, self.K, self.V
        pred = self.pred.view(self.B, self.AK, self.E).float()
        if self.A > 1:          # head a K + k: frame T - K - d_a + k
            targets = torch.cat([top[:, r:r + K, :] for r in self._anchor_rows()], 1).float().transpose(1, 2)
        else:
            targets = top[:, T - K:T, :].float().transpose(1, 2)
        z = top[:, T - K - V:T - K, :].float().transpose(1, 2)
        zs = self.ctx.z_scale       # AttentionModel rescales z in place (attention_model.py:30)
        if zs != 1.0:
            z = z * zs
        return pred, targets, z, self.ctx.c_float().clone()

    # ------------------------------------------------------------------------------------------ loss
    # One chain for every score kind and both branches (_loss_chain); each stage below is written once.
    @property
    def ldS_all(self):
        """Leading dimension of the (B K) x (B K) matrices of the all-timesteps branch."""
        R = self.B * self.K
        return _ceil_div(R, 8) * 8

    def _all_scores(self):
        """S_all, allocated on first use: all that score_gemm_all and nce_eval need of the all-timesteps buffers."""
        if getattr(self, "S_all", None) is None:
            self.S_all = torch.zeros(self.B * self.K * self.ldS_all, device=self.device, dtype=torch.float32)
        return self.S_all

    def _all_buffers(self):
        """(S_all, ST_all, dS_all, dST_all) of the unfused all-timesteps loss, and its workspace nce_all_ws (allocated on first use)."""
        S = self._all_scores()
        if getattr(self, "ST_all", None) is None:
            self.ST_all = torch.zeros_like(S)
            self.dS_all = torch.zeros(S.numel(), device=self.device, dtype=self.dt)
            self.dST_all = torch.zeros(S.numel(), device=self.device, dtype=self.dt)
            self.nce_all_ws = torch.empty(int(_hip.lib().cpc_nce_all_workspace_floats(self.B, self.K)), device=self.device,
                                          dtype=torch.float32)
        return S, self.ST_all, self.dS_all, self.dST_all

    def _loss_buffers(self, all_timesteps: bool, transposed: bool):
        """(S, ST, dS, dST) of a branch.  The default branch's transposed scores ST exist only for the kinds whose fix-up reads them
        (``transposed``; allocated on first use, else None): its loss kernels write dST from S themselves."""
        if all_timesteps:
            return self._all_buffers()
        if transposed and getattr(self, "ST", None) is None:
            self.ST = torch.zeros_like(self.S)
        return self.S, (self.ST if transposed else None), self.dS, self.dST

    def score_gemm(self, pred=None, top=None, out=None):
        """The score contraction of the default branch (contrastive_estimation_training.py:12-22 restricted to equal steps,
        :116): K batched B x E x B products S[k] = predicted_z[:, k, :] targets[:, :, k]^T.  Returns its algorithmic FLOPs."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T, ld = self.geo.alloc[-1], self.T, self.ldS
        pred = self.pred if pred is None else pred
        top = self.act[-1] if top is None else top
        out = self.S if out is None else out
        if self.A > 1:
            # heads a K + k against rows T - K - d_a + k.  Stride == K: the windows tile rows [T - AK, T), one launch over AK heads;
            # otherwise today's launch per anchor at its head offset into pred (ld = AK E) and its own first target row
            AK = self.AK
            if self.s == K:
                _hip.gemm_nt(_hip.ptr(pred), _hip.ptr(top, (T - AK) * E), _hip.ptr(out), B, B, E, AK * E, Ltop * E, ld,
                             code, a_batch=E, b_batch=E, c_batch=B * ld, batch=AK, flags=_hip.GEMM_OUT_F32)
            else:
                for a, r in enumerate(self._anchor_rows()):
                    _hip.gemm_nt(_hip.ptr(pred, a * K * E), _hip.ptr(top, r * E), _hip.ptr(out, a * K * B * ld), B, B, E, AK * E, Ltop * E,
                                 ld, code, a_batch=E, b_batch=E, c_batch=B * ld, batch=K, flags=_hip.GEMM_OUT_F32)
            return 2.0 * AK * B * B * E
        _hip.gemm_nt(_hip.ptr(pred), _hip.ptr(top, (T - K) * E), _hip.ptr(out), B, B, E, K * E, Ltop * E, ld,
                     code, a_batch=E, b_batch=E, c_batch=B * ld, batch=K, flags=_hip.GEMM_OUT_F32)
        return 2.0 * K * B * B * E

    def score_gemm_all(self, pred=None, top=None, out=None):
        """The full (B K) x E x (B K) score contraction of score_over_all_timesteps=True (:12-22, :108-114).  Returns its FLOPs."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T = self.geo.alloc[-1], self.T
        R = B * K
        S = self._all_scores()
        pred = self.pred if pred is None else pred
        top = self.act[-1] if top is None else top
        _hip.gemm_nt(_hip.ptr(pred), _hip.ptr(top, (T - K) * E), _hip.ptr(S if out is None else out), R, R, E, E, E, self.ldS_all, code,
                     b_rpi=K, b_item=Ltop * E, flags=_hip.GEMM_OUT_F32)
        return 2.0 * R * R * E

    def nce_forward_backward(self, softplus: bool, regularization: float, score: Optional[str] = None, negatives=None,
                             negative_groups=None, temperature=None, negative_bank=None):
        """Equal-step scores, InfoNCE loss + regulariser, and d loss / d (predicted_z, targets).

        contrastive_estimation_training.py:106-122,141 with score_over_all_timesteps=False.  Only the K diagonal
        (B x B) blocks of the reference's (B K)^2 score tensor are ever formed (12x fewer FLOPs).
        ``score``: see score_kind; every kind (with the ``temperature`` of "normalized") runs _loss_chain.
        ``negatives``: None, or (n_neg, seed, draw) — every target is contrasted against n_neg seeded negatives instead of the
        whole batch (cpc_nce_loss_sampled behind the same dense score GEMM; sampled_negatives.sampled_negative_mask).
        ``negative_groups``: None, or (groups, mode) — groups an int32 device tensor [B], mode "same" / "other": a target's candidates
        are the rows of its own group / of the other groups, all of them or, with ``negatives``, n_neg seeded ones
        (cpc_nce_loss_grouped; sampled_negatives.grouped_negative_mask).
        ``negative_bank``: None, or a NegativeBank — the predictions of the steps it remembers are further candidates of every target
        (cpc_nce_loss_banked); the call writes this step's into it and moves its cursor on."""
        kind = score_kind(softplus, score)
        self._loss_chain(kind, False, regularization, check_temperature(temperature, kind), negatives, negative_groups, negative_bank)

    def nce_all_forward_backward(self, softplus: bool, regularization: float, score: Optional[str] = None, temperature=None):
        """score_over_all_timesteps=True (contrastive_estimation_training.py:108-114, :141): the full (B K) x (B K) score
        matrix (and its transpose, as a second tiny GEMM, so that both gradient layouts are written coalesced), the
        log-sum-exp over ALL predictions for every (target item, step), and d loss / d (predicted_z, targets): _loss_chain.
        bf16 storage and tile-sized problems take the fused route (_nce_all_fused) instead, "normalized" scores (with their
        ``temperature``) on the normalised operands; difference scores never do (cpc_score_lse is a dot-product kernel)."""
        kind = score_kind(softplus, score)
        self._loss_chain(kind, True, regularization, check_temperature(temperature, kind))

    def _loss_chain(self, kind: str, all_timesteps: bool, regularization: float, temperature=None, negatives=None,
                    negative_groups=None, negative_bank=None):
        """InfoNCE loss + regulariser on the scores of ``kind`` and d loss / d (predicted_z, targets), into dpred and rows [T-K, T) of
        the top-layer gradient.  The stages, in order:
          selection   select_negatives: checked and normalised before anything of the engine but B is read
          operands    as they are; "normalized": the rows over their norms, predictions also over the temperature (_norm_operands)
          bank        ("banked") the operands go into the bank's slot cur (_bank_store); a bank without earlier steps is then the
                      whole-batch selection: that step runs the very launches of a call without a bank
          scores      _scores: score GEMM(s) or cpc_diff_scores; "banked": one score GEMM over the ring's rows (_bank_scores)
          loss        _nce_loss: dense, sampled, grouped, banked or all-timesteps kernel ("linear" scores for every kind but "softplus", as
                      contrastive_estimation_training._InfoNCE does, over the same selection); or scores and loss in one, _nce_all_fused, where
                      fused_scores_ok() holds
          fix-up      "difference": _diff_coefficients
          gradients   the linear score's two contractions, _score_grads / _score_grads_all ("banked": the second one reduces over the
                      ring's rows, and nothing flows into the bank)
          operands'   "difference": the rank-1 terms (_diff_rank1); "normalized": cpc_norm_rows_bwd, in place (_norm_backward)
          backward
        All on the current stream: the target-row lane of backward() starts from those rows behind the event it records there.
        ``temperature``: already checked by the caller (nce_forward_backward / nce_all_forward_backward)."""
        selection = select_negatives(self.B, negatives, negative_groups, all_timesteps, None, negative_bank, kind, temperature)
        if self.A > 1 and (all_timesteps or selection is not None or kind not in ("softplus", "linear")):
            raise NotImplementedError(ANCHOR_LOSS_REASON)
        pred, top, dpred, dtop = self.pred, self.act[-1], self.dpred, self.dact[-1]
        if kind == "normalized":
            if isinstance(temperature, DeviceTemperature):
                temperature.dots = self._norm_dots()
            pred, top = self._norm_operands(temperature, tick=True)
        softplus = 1 if kind == "softplus" else 0
        bank = None
        if selection is not None and selection[0] == "banked":
            bank = selection[1]
            self._bank_store(bank, pred)
            if bank.filled == 0:
                selection = None
        if all_timesteps and kind != "difference" and self.fused_scores_ok():
            self._nce_all_fused(softplus, regularization, pred, top)
        elif selection is not None and selection[0] == "banked":
            S, dS = self._bank_buffers(bank)
            self._bank_scores(bank, top, S)
            self._nce_loss(S, None, dS, self.dST, softplus, regularization, selection, False)
            rows = bank.slots * self.B
            self._score_grads(dS, self.dST, bank.ring, top, dpred, dtop, rows=rows, nsplit=self._bank_nsplit(rows))
        else:
            S, ST, dS, dST = self._loss_buffers(all_timesteps, transposed=kind == "difference")
            self._scores(kind, all_timesteps, pred, top, S, ST)
            self._nce_loss(S, ST, dS, dST, softplus, regularization, selection, all_timesteps)
            if kind == "difference":
                self._diff_coefficients(S, ST, dS, dST, all_timesteps)
            (self._score_grads_all if all_timesteps else self._score_grads)(dS, dST, pred, top, dpred, dtop)
        if kind == "difference":
            self._diff_rank1(pred, top, dpred, dtop)
        elif kind == "normalized":
            self._norm_backward(temperature, pred, top, dpred, dtop)
        if bank is not None:
            bank.advance()

    # ---- negative bank (NegativeBank; include/cpc_hip.h, cpc_nce_loss_banked) ----
    def _bank_store(self, bank, pred):
        """This step's score operands (shaped like self.pred) into slot cur of the bank, which is allocated here on first use."""
        bank.bind(self.B, self.K, self.E, self.dt, self.device)
        bank.slot(bank.cur).view(-1).copy_(pred.view(-1))

    def _bank_buffers(self, bank):
        """(S, dS) [K][slots B][ldS] of the banked loss and its workspace nce_banked_ws, allocated on first use per ring size."""
        b = getattr(self, "_bank_bufs", None)
        if b is None or b.slots != bank.slots:
            n = self.K * bank.slots * self.B * self.ldS
            b = self._bank_bufs = SimpleNamespace(
                slots=bank.slots, S=torch.zeros(n, device=self.device, dtype=torch.float32),
                dS=torch.zeros(n, device=self.device, dtype=self.dt))
            self.nce_banked_ws = torch.empty(int(_hip.lib().cpc_nce_banked_workspace_floats(self.B, self.K, bank.slots)),
                                             device=self.device, dtype=torch.float32)
        return b.S, b.dS

    def _bank_nsplit(self, rows):
        """Slabs of the target contraction over the ring's ``rows``: its output is B x E per step k (96 tiles at the headline size),
        so a reduction of thousands of rows sits on few workgroups.  Measured on an MI355X at B = 256, K = 12, E = 512 (DESIGN.md,
        "Negative bank"): bf16 storage gains from 1280 rows on with slabs of about 512 rows (direct 35.8 / 95.8 us at 1280 / 4352 rows,
        slabs 20.0 / 37.9 us + the cast) and loses at 512 rows; f32 storage gains from 512 rows on, most with eight slabs.  No slab
        is ever empty: _chunk rounds a slab's rows up, so the count comes down until the last slab still starts inside the rows."""
        if self.dt == torch.bfloat16:
            n = rows // 512 if rows >= 1024 else 1
        else:
            n = rows // 64 if rows >= 512 else 1
        n = max(1, min(8, n))
        while n > 1 and (n - 1) * self._chunk(rows, n) >= rows:
            n -= 1
        return n

    def _bank_scores(self, bank, top, S):
        """score_gemm with the ring as the left operand: S[k][slot B + b][b'] = <ring[slot B + b][k], targets[b'][:, k]>."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T, ld, N = self.geo.alloc[-1], self.T, self.ldS, bank.slots * self.B
        _hip.gemm_nt(_hip.ptr(bank.ring), _hip.ptr(top, (T - K) * E), _hip.ptr(S), N, B, E, K * E, Ltop * E, ld, code,
                     a_batch=E, b_batch=E, c_batch=N * ld, batch=K, flags=_hip.GEMM_OUT_F32)

    def _scores(self, kind: str, all_timesteps: bool, pred, top, S, ST=None):
        """The scores of a kind and a branch into S and, unless None, their transpose into ST, from operands in the layouts of
        self.pred / the top-layer buffer: one cpc_diff_scores pass for "difference"; else the score GEMM, and for the ST of the
        all-timesteps branch a second one with the operands swapped."""
        if kind == "difference":
            (self.diff_scores_all if all_timesteps else self.diff_scores)(S, ST, pred, top)
            return
        (self.score_gemm_all if all_timesteps else self.score_gemm)(pred, top, S)
        if ST is not None:
            assert all_timesteps, "the default branch's dot-product scores have no transposed GEMM"
            code, B, E, K = self.code, self.B, self.E, self.K
            Ltop, T, R = self.geo.alloc[-1], self.T, B * K
            _hip.gemm_nt(_hip.ptr(top, (T - K) * E), _hip.ptr(pred), _hip.ptr(ST), R, R, E, E, E, self.ldS_all, code,
                         a_rpi=K, a_item=Ltop * E, flags=_hip.GEMM_OUT_F32)

    def _nce_loss(self, S, ST, dS, dST, softplus: int, regularization: float, selection, all_timesteps: bool):
        """Exactly one loss kernel on formed scores: cpc_nce_loss_all, or by ``selection`` (select_negatives) cpc_nce_loss,
        cpc_nce_loss_sampled, cpc_nce_loss_grouped — same buffers and layouts; the workspaces of the last two are allocated on
        first use — or cpc_nce_loss_banked (S, dS over the ring's rows from _bank_buffers, dST the current slot's).  Leaves the loss
        values in nce_out and the coefficients g = d loss / d score in dS and, transposed, dST."""
        B, K, code, P, U = self.B, self.K, self.code, _hip.ptr, C.c_ulonglong
        out, reg = P(self.nce_out), C.c_float(regularization)
        if all_timesteps:
            _hip.call("cpc_nce_loss_all", P(S), P(ST), P(dS), P(dST), out, P(self.nce_all_ws), B, K, self.ldS_all, softplus, reg, code)
        elif selection is None:
            _hip.call("cpc_nce_loss", P(S), P(dS), P(dST), out, P(self.nce_ws), B, self.AK, self.ldS, softplus, reg, code)
        elif selection[0] == "sampled":
            if getattr(self, "nce_sampled_ws", None) is None:
                self.nce_sampled_ws = torch.empty(int(_hip.lib().cpc_nce_sampled_workspace_floats(B, K)), device=self.device,
                                                  dtype=torch.float32)
            _, n_neg, seed, draw = selection
            _hip.call("cpc_nce_loss_sampled", P(S), P(dS), P(dST), out, P(self.nce_sampled_ws), B, K, self.ldS, softplus, reg,
                      n_neg, U(seed), U(draw), code)
        elif selection[0] == "banked":
            bank = selection[1]
            _hip.call("cpc_nce_loss_banked", P(S), P(dS), P(dST), out, P(self.nce_banked_ws), B, K, self.ldS, bank.slots, bank.cur,
                      U(bank.valid), softplus, reg, code)
        else:
            if getattr(self, "nce_grouped_ws", None) is None:
                self.nce_grouped_ws = torch.empty(int(_hip.lib().cpc_nce_grouped_workspace_floats(B, K)), device=self.device,
                                                  dtype=torch.float32)
            _, groups, mode, n_neg, seed, draw = selection
            _hip.call("cpc_nce_loss_grouped", P(S), P(dS), P(dST), out, P(self.nce_grouped_ws), B, K, self.ldS, softplus, reg,
                      P(groups), mode, n_neg, U(seed), U(draw), code)

    def _score_grads(self, W, WT, pred, top, out_pred, out_top, rows=None, nsplit=1):
        """The two contractions behind d loss / d (predicted_z, targets) of the default branch, for any coefficients W[k][b][b']
        (WT: its transpose per k) and operands in the layouts of ``self.pred`` / the top-layer buffer.  ``rows``: the prediction rows
        of W and ``pred`` where they are more than B (the banked loss: W [k][rows][b'], ``pred`` the ring, WT of the current slot);
        ``nsplit`` > 1 (_bank_nsplit) splits that long reduction into f32 slabs [nsplit][B][K][E], summed in slab order by one
        cpc_reduce_slabs — straight into the target rows in f32 storage, through an f32 [B][K][E] sum and one strided cast in bf16."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T, ld = self.geo.alloc[-1], self.T, self.ldS
        rows = B if rows is None else rows
        if self.A > 1:
            self._score_grads_anchors(W, WT, pred, top, out_pred)
            return
        # out_pred[b][k][:] = sum_b' W[k][b][b'] * targets[b'][k][:]
        _hip.gemm_tn(_hip.ptr(WT), _hip.ptr(top, (T - K) * E), _hip.ptr(out_pred), B, B, E, ld, Ltop * E, K * E, code,
                     a_batch=B * ld, b_batch=E, c_batch=E, batch=K)
        # out_top rows T-K+k of item b' = sum_b W[k][b][b'] * predicted_z[b][k][:]
        if nsplit == 1:
            _hip.gemm_tn(_hip.ptr(W), _hip.ptr(pred), _hip.ptr(out_top, (T - K) * E), rows, B, E, ld, K * E, Ltop * E, code,
                         a_batch=rows * ld, b_batch=E, c_batch=E, batch=K)
            return
        n = B * K * E
        if getattr(self, "_tn_slabs", None) is None or self._tn_slabs.numel() < (nsplit + 1) * n:
            self._tn_slabs = torch.empty((nsplit + 1) * n, device=self.device, dtype=torch.float32)          # slabs + their sum
        slabs, L = self._tn_slabs, C.c_longlong
        _hip.gemm_tn(_hip.ptr(W), _hip.ptr(pred), _hip.ptr(slabs), rows, B, E, ld, K * E, K * E, code, a_batch=rows * ld, b_batch=E,
                     c_batch=E, batch=K, nsplit=nsplit, m_chunk=self._chunk(rows, nsplit), slab_stride=n, flags=_hip.GEMM_OUT_F32)
        if self.dt == torch.float32:
            _hip.call("cpc_reduce_slabs", _hip.ptr(slabs), _hip.ptr(out_top, (T - K) * E), B, K * E, nsplit, L(n), 1, L(1), L(Ltop * E), L(0))
        else:
            _hip.call("cpc_reduce_slabs", _hip.ptr(slabs), _hip.ptr(slabs, nsplit * n), B, K * E, nsplit, L(n), 1, L(1), L(K * E), L(0))
            out_top[:B * Ltop * E].view(B, Ltop, E)[:, T - K:T, :].copy_(slabs[nsplit * n:(nsplit + 1) * n].view(B, K, E))

    def _score_grads_anchors(self, W, WT, pred, top, out_pred):
        """_score_grads over AK heads.  The prediction side is the same contraction per anchor (one launch where the windows tile);
        the target side goes to dT f32 [A][B][K][E], because the windows of different anchors may share top rows: one gather
        (cpc_anchor_target_grad) then makes rows [T-K, T) of the top-layer gradient final, before backward() is issued — the invariant
        both target lanes rest on (_bwd_lane); backward() adds the rows below T-K behind the context network's dz."""
        code, B, E, K, AK = self.code, self.B, self.E, self.K, self.AK
        Ltop, T, ld = self.geo.alloc[-1], self.T, self.ldS
        if self.s == K:
            _hip.gemm_tn(_hip.ptr(WT), _hip.ptr(top, (T - AK) * E), _hip.ptr(out_pred), B, B, E, ld, Ltop * E, AK * E, code,
                         a_batch=B * ld, b_batch=E, c_batch=E, batch=AK)
        for a, r in enumerate(self._anchor_rows()):
            if self.s != K:
                _hip.gemm_tn(_hip.ptr(WT, a * K * B * ld), _hip.ptr(top, r * E), _hip.ptr(out_pred, a * K * E), B, B, E, ld, Ltop * E,
                             AK * E, code, a_batch=B * ld, b_batch=E, c_batch=E, batch=K)
            _hip.gemm_tn(_hip.ptr(W, a * K * B * ld), _hip.ptr(pred, a * K * E), _hip.ptr(self.dT, a * B * K * E), B, B, E, ld, AK * E,
                         K * E, code, a_batch=B * ld, b_batch=E, c_batch=E, batch=K, flags=_hip.GEMM_OUT_F32)
        self._anchor_target_rows(T - K, T, 0)

    def _anchor_target_rows(self, lo, hi, accumulate):
        """Rows [lo, hi) of the top-layer gradient from dT (cpc_anchor_target_grad): written, or added to what is there."""
        _hip.call("cpc_anchor_target_grad", _hip.ptr(self.dT), _hip.ptr(self.dact[-1]), C.c_longlong(self.geo.alloc[-1] * self.E),
                  self.A, self.B, self.K, self.E, self._anchor_rows()[0], self.s, lo, hi, accumulate, self.code)

    def anchor_bridge_grads(self, d_pred, d_targets):
        """The autograd bridge with anchors: d predicted_z (B, AK, E) into dpred, d targets (B, E, AK) into dT, and rows [T-K, T) of the
        top-layer gradient from it; backward() does the rest.  None: zeros."""
        B, E, K, A = self.B, self.E, self.K, self.A
        if d_pred is None:
            self.dpred.zero_()
        else:
            self.dpred.view(B, self.AK, E).copy_(d_pred)
        if d_targets is None:
            self.dT.zero_()
        else:
            self.dT.view(A, B, K, E).copy_(d_targets.reshape(B, E, A, K).permute(2, 0, 3, 1))
        self._anchor_target_rows(self.T - K, self.T, 0)

    def _score_grads_all(self, W, WT, pred, top, out_pred, out_top):
        """The same for the all-timesteps branch: W [(b,k)][(b',k')] and its transpose.
        d predicted_z[(b,k)][:] = sum_c dS[(b,k)][c] * targets[c][:]  and  d targets[c][:] = sum_r dS[r][c] * predicted_z[r][:]
        (the latter into rows T-K+k' of item b' of the top-layer gradient).  As NT GEMMs over the long axis — the reduction
        form would put a 3072-row reduction on 24 workgroups — with the small right-hand operands transposed once (3 MB each)."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T = self.geo.alloc[-1], self.T
        R, ld = B * K, self.ldS_all
        tg = (T - K) * E
        if getattr(self, "targT", None) is None:
            self.targT = torch.zeros(E, ld, device=self.device, dtype=self.dt)
            self.predT = torch.zeros(E, ld, device=self.device, dtype=self.dt)
        self.targT[:, :R].copy_(top.view(B, Ltop, E)[:, T - K:T, :].reshape(R, E).t())
        self.predT[:, :R].copy_(pred.view(R, E).t())
        _hip.gemm_nt(_hip.ptr(W), _hip.ptr(self.targT), _hip.ptr(out_pred), R, E, ld, ld, ld, E, code)
        _hip.gemm_nt(_hip.ptr(WT), _hip.ptr(self.predT), _hip.ptr(out_top, tg), R, E, ld, ld, ld, E, code,
                     c_rpi=K, c_item=Ltop * E, c_valid=K)

    # ---- score_over_all_timesteps=True with the column pass fused into the score GEMM (bf16; include/cpc_hip.h, cpc_score_lse) ----
    def fused_scores_ok(self, rows=None, cols=None):
        """The fused path needs bf16 storage, 256-row / 256-column tiles, E a multiple of 64 and an even K <= 24
        (switches.fused_score off: the unfused kernels)."""
        R = self.B * self.K
        rows, cols = (R if rows is None else rows), (R if cols is None else cols)
        return (self.dt == torch.bfloat16 and switches.fused_score() and rows % 256 == 0 and cols % 256 == 0
                and self.E % 64 == 0 and self.E >= 128 and self.K % 2 == 0 and self.K <= 24)

    def _nce_all_fused(self, softplus: bool, regularization: float, pred=None, top=None):
        """One persistent MFMA launch forms the (B K) x (B K) scores tile by tile and leaves the f32 scores + per-tile column
        (max, sum-exp) pairs + the diagonal; a merge, one gradient pass (dS and its transpose) and the loss scalars follow.  Replaces: the second (transposed) score GEMM, two f32 score matrices, the 16-way split column pass and the
        two element-wise gradient passes of the unfused route.  ``pred`` / ``top``: the score operands in the layouts of
        self.pred / the top-layer buffer (None: those two)."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T = self.geo.alloc[-1], self.T
        pred = self.pred if pred is None else pred
        top, dtop = (self.act[-1] if top is None else top), self.dact[-1]
        R = B * K
        f = getattr(self, "_fs", None)
        if f is None:
            dev, f32 = self.device, torch.float32
            f = self._fs = SimpleNamespace(
                targ=torch.empty(R, E, device=dev, dtype=self.dt), Sb=torch.empty(R, R, device=dev, dtype=f32),
                pm=torch.empty(R // 256, R, device=dev, dtype=f32), ps=torch.empty(R // 256, R, device=dev, dtype=f32),
                valid=torch.zeros(R, device=dev, dtype=f32), lse=torch.empty(R, device=dev, dtype=f32),
                colp=torch.empty(_ceil_div(R, 256), 2, device=dev, dtype=f32),
                gradp=torch.empty(int(_hip.lib().cpc_nce_fused_grad_blocks(B, R)), device=dev, dtype=f32),
                dS=torch.empty(R, R, device=dev, dtype=self.dt), dST=torch.empty(R, R, device=dev, dtype=self.dt))
        P = _hip.ptr
        f.targ.view(B, K, E).copy_(top.view(B, Ltop, E)[:, T - K:T, :])
        _hip.call("cpc_score_lse", P(pred), P(f.targ), P(f.Sb), P(f.pm), P(f.ps), P(f.valid), R, R, E, C.c_longlong(E), C.c_longlong(E),
                  C.c_longlong(R), 0, key="score_lse<bf16,256>", work=2.0 * R * R * E)
        _hip.call("cpc_nce_lse_merge", P(f.pm), P(f.ps), R // 256, R, 1 if softplus else 0, C.c_float(R), P(f.lse), P(f.colp))
        _hip.call("cpc_nce_fused_grad", P(f.Sb), P(f.lse), P(f.dS), P(f.dST), P(f.gradp), B, K, R, C.c_longlong(R), C.c_longlong(R), 0,
                  1 if softplus else 0, C.c_float(regularization), C.c_float(R), C.c_float(B))
        _hip.call("cpc_nce_fused_finalize", P(f.colp), f.colp.shape[0], P(f.valid), R, P(f.gradp), f.gradp.numel(), None, 0, C.c_float(R),
                  C.c_float(B), K, C.c_float(regularization), 1 if softplus else 0, P(self.nce_out))
        self._score_grads_all(f.dS, f.dST, pred, top, self.dpred, dtop)

    def nce_eval(self, softplus: bool, all_timesteps: bool, sums, workspace, score: Optional[str] = None, temperature=None):
        """Adds this batch's validation quantities (per-step losses, per-step accuracies, mean score: include/cpc_hip.h,
        cpc_nce_eval) to ``sums`` (2 K + 1 floats) — from the score matrices of the train step (forward() must have run).
        ``score``: see score_kind (difference scores are formed by cpc_diff_scores, "normalized" scores by the score GEMM on the
        operands cpc_norm_rows leaves for ``temperature``; both are then read as linear scores)."""
        kind = score_kind(softplus, score)
        temperature = check_temperature(temperature, kind)
        pred, top = self._norm_operands(temperature) if kind == "normalized" else (self.pred, self.act[-1])
        S, ld = (self._all_scores(), self.ldS_all) if all_timesteps else (self.S, self.ldS)
        if self.A > 1:          # the last anchor's K heads (today's model): the numbers stay comparable across anchor settings
            if all_timesteps or kind not in ("softplus", "linear"):
                raise NotImplementedError(ANCHOR_LOSS_REASON)
            code, B, E, K, T = self.code, self.B, self.E, self.K, self.T
            _hip.gemm_nt(_hip.ptr(pred, (self.A - 1) * K * E), _hip.ptr(top, (T - K) * E), _hip.ptr(S), B, B, E, self.AK * E,
                         self.geo.alloc[-1] * E, ld, code, a_batch=E, b_batch=E, c_batch=B * ld, batch=K, flags=_hip.GEMM_OUT_F32)
        else:
            self._scores(kind, all_timesteps, pred, top, S)
        _hip.call("cpc_nce_eval", _hip.ptr(S), _hip.ptr(sums), _hip.ptr(workspace), self.B, self.K, ld, 1 if kind == "softplus" else 0,
                  1 if all_timesteps else 0, 1)

    # ---- difference scores (contrastive_estimation_training.py:25-33; include/cpc_hip.h, cpc_diff_scores) ----
    # The loss kernels take them as linear scores; with d = |p - t|^2 and s = 1 / d, d loss / d d = -g s^2 for g = d loss / d s, so the
    # gradient is the linear score's two contractions with G = 2 g s^2 minus the rank-1 terms (row / column sums of G) * (p / t).
    def diff_scores(self, S, ST, pred=None, top=None):
        """Default branch: S[k][b][b'] = 1 / |predicted_z[b, k] - targets[b', :, k]|^2 (and ST[k][b'][b], unless None) from operands
        in the engine's own layouts (None: self.pred / the top layer).  Returns the launch's algorithmic FLOPs (one sub + one fma per
        feature and pair)."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T, ld = self.geo.alloc[-1], self.T, self.ldS
        pred = self.pred if pred is None else pred
        top = self.act[-1] if top is None else top
        work = 2.0 * K * B * B * E
        _hip.call("cpc_diff_scores", _hip.ptr(pred), _hip.ptr(top, (T - K) * E), _hip.ptr(S), _hip.ptr(ST), B, B, E,
                  C.c_longlong(K * E), C.c_longlong(Ltop * E), 0, C.c_longlong(0), C.c_longlong(E), C.c_longlong(E),
                  C.c_longlong(B * ld), K, ld, code, work=work)
        return work

    def diff_scores_all(self, S, ST, pred=None, top=None):
        """score_over_all_timesteps=True: the (B K) x (B K) difference scores S (and ST, unless None) from one pass."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T = self.geo.alloc[-1], self.T
        pred = self.pred if pred is None else pred
        top = self.act[-1] if top is None else top
        R = B * K
        work = 2.0 * R * R * E
        _hip.call("cpc_diff_scores", _hip.ptr(pred), _hip.ptr(top, (T - K) * E), _hip.ptr(S), _hip.ptr(ST), R, R, E,
                  C.c_longlong(E), C.c_longlong(E), K, C.c_longlong(Ltop * E), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), 1,
                  self.ldS_all, code, work=work)
        return work

    def _diff_coefficients(self, S, ST, dS, dST, all_timesteps: bool):
        """cpc_diff_scores_bwd: G = 2 g s^2 in place of g in dS / dST, and its row / column sums in _diff_mu (allocated on first use;
        indexed like predicted_z's and the targets' (b, k) rows in both branches).  In bf16 storage G is rounded to bf16 (the operand
        type of the contractions) and its sums are taken of the rounded values."""
        B, K, P = self.B, self.K, _hip.ptr
        R = B * K
        if getattr(self, "_diff_mu", None) is None:
            self._diff_mu = torch.empty(2, R, device=self.device, dtype=torch.float32)
        mu, nu = self._diff_mu[0], self._diff_mu[1]
        n, ld, stride, batch = (R, self.ldS_all, 0, 1) if all_timesteps else (B, self.ldS, B * self.ldS, K)
        _hip.call("cpc_diff_scores_bwd", P(dS), P(S), P(mu), P(dST), P(ST), P(nu), n, n, ld, C.c_longlong(stride), batch, self.code)

    def _diff_rank1(self, pred, top, dpred, dtop):
        """cpc_diff_scores_rank1: dpred -= mu * predicted_z and the K target rows of dtop -= nu * targets (_diff_coefficients' sums)."""
        code, E, K, P, L = self.code, self.E, self.K, _hip.ptr, C.c_longlong
        Ltop, R, tg = self.geo.alloc[-1], self.B * K, (self.T - K) * E
        mu, nu = self._diff_mu[0], self._diff_mu[1]
        _hip.call("cpc_diff_scores_rank1", P(mu), P(pred), P(dpred), R, E, 0, L(0), L(E), code)
        _hip.call("cpc_diff_scores_rank1", P(nu), P(top, tg), P(dtop, tg), R, E, K, L(Ltop * E), L(E), code)

    # ---- cosine similarity / temperature ("normalized"; include/cpc_hip.h, cpc_norm_rows) ----
    def _norm_scratch(self):
        """Scratch of the "normalized" kind, allocated on first use (GraphedStep asks for it in front of its capture, so that the
        zero fill of tn is not replayed with every step)."""
        n = getattr(self, "_norm", None)
        if n is None:
            R = self.B * self.K
            n = self._norm = SimpleNamespace(pn=torch.empty_like(self.pred), tn=torch.zeros_like(self.act[-1]),
                                             inv_p=torch.empty(R, device=self.device, dtype=torch.float32),
                                             inv_t=torch.empty(R, device=self.device, dtype=torch.float32), dots=None)
        return n

    def _norm_dots(self):
        """dots (R floats) of the scratch, allocated when a DeviceTemperature first comes by (a float temperature never needs it)."""
        n = self._norm_scratch()
        if n.dots is None:
            n.dots = torch.zeros(self.B * self.K, device=self.device, dtype=torch.float32)
        return n.dots

    def _norm_operands(self, temperature, tick: bool = False):
        """The score operands of the "normalized" kind, from the engine's own layouts: pn = predicted_z rows / max(norm, eps) /
        temperature (shaped like self.pred) and tn = the K target rows of every item / max(norm, eps) inside a zero buffer shaped like
        the top layer (only rows [T-K, T) are ever written).  Scratch allocated on first use; 1 / max(norm, eps) per row stays in
        inv_p / inv_t (f32) for the backward.  ``temperature``: a float (the launch argument), or a DeviceTemperature: the prediction
        rows then go through cpc_norm_rows_dev, which reads the scale from its tstate, and with ``tick`` a scheduled one is set for the
        step at hand first (cpc_temperature_set; an evaluation leaves the value as it stands)."""
        code, B, E, K = self.code, self.B, self.E, self.K
        Ltop, T = self.geo.alloc[-1], self.T
        R = B * K
        n = self._norm_scratch()
        P, L, tg = _hip.ptr, C.c_longlong, (T - K) * E
        nbytes = 2.0 * R * E * self.pred.element_size()
        if isinstance(temperature, DeviceTemperature):
            if tick:
                temperature.tick()
            _hip.call("cpc_norm_rows_dev", P(self.pred), P(n.pn), P(n.inv_p), R, E, 0, L(0), L(E), temperature.scale_ptr(),
                      C.c_float(NORM_EPS), code, work=nbytes)
        else:
            _hip.call("cpc_norm_rows", P(self.pred), P(n.pn), P(n.inv_p), R, E, 0, L(0), L(E), C.c_float(1.0 / temperature),
                      C.c_float(NORM_EPS), code, work=nbytes)
        _hip.call("cpc_norm_rows", P(self.act[-1], tg), P(n.tn, tg), P(n.inv_t), R, E, K, L(Ltop * E), L(E), C.c_float(1.0),
                  C.c_float(NORM_EPS), code, work=nbytes)
        return n.pn, n.tn

    def _norm_backward(self, temperature, pn, tn, dpred, dtop):
        """cpc_norm_rows_bwd turns the gradients with respect to the normalised rows (_norm_operands' pn / tn) into those with respect
        to the rows, in place in dpred and in rows [T-K, T) of dtop.  A DeviceTemperature takes the _dev kernel for the prediction rows:
        the scale comes from its tstate, and dots[row] = <pn[row], d loss / d pn[row]> is left in the scratch, whose sum is
        d loss / d log(1 / tau) for every loss kernel of the chain — FusedAdam(temperature=...) adds them up (cpc_temperature_step)."""
        code, E, K = self.code, self.E, self.K
        Ltop, R, n = self.geo.alloc[-1], self.B * K, self._norm
        P, L, tg = _hip.ptr, C.c_longlong, (self.T - K) * E
        nbytes = 3.0 * R * E * self.pred.element_size()
        if isinstance(temperature, DeviceTemperature):
            _hip.call("cpc_norm_rows_bwd_dev", P(pn), P(n.inv_p), P(dpred), P(n.dots), R, E, 0, L(0), L(E), temperature.scale_ptr(),
                      C.c_float(NORM_EPS), code, work=nbytes)
        else:
            _hip.call("cpc_norm_rows_bwd", P(pn), P(n.inv_p), P(dpred), R, E, 0, L(0), L(E), C.c_float(1.0 / temperature),
                      C.c_float(NORM_EPS), code, work=nbytes)
        _hip.call("cpc_norm_rows_bwd", P(tn, tg), P(n.inv_t), P(dtop, tg), R, E, K, L(Ltop * E), L(E), C.c_float(1.0),
                  C.c_float(NORM_EPS), code, work=nbytes)

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, x, add_dc: Optional[torch.Tensor] = None, add_dz: Optional[torch.Tensor] = None, grad_ready_hook=None):
        """Gradients of everything upstream of (predicted_z, targets, z, c) into the model's flat gradient buffer.

        Expects ``dpred`` and rows [T-K, T) of the top-layer gradient to be filled (by nce_forward_backward or by the
        autograd bridge).  Rows [T-K-V, T-K) are overwritten here with the GRU's input gradient (+ add_dz (B,E,V)).
        ``grad_ready_hook(lo, hi)`` is called as soon as the flat-gradient range [lo, hi) is final, so that a caller can
        start reducing it across ranks while the remaining layers are still being differentiated."""
        g, code = self.model._grad, self.code
        B, V, H, E, K, n = self.B, self.V, self.H, self.E, self.K, self.n
        La, Lv = self.geo.alloc, self.geo.valid
        Ltop, T = La[-1], self.T
        t0 = T - K - V
        self._ahead = None          # prepare_ahead state of a step whose optimizer step never came (nothing was swapped in yet)
        top, dtop = self.act[-1], self.dact[-1]
        # predictor: dW_p = dpred^T c ;  dc = dpred W_p.  Only dc is on the path to the context network's backward pass: the weight
        # gradient is issued later, inside the first side-stream block of the encoder's backward pass (no event of its own)
        ct, coff, cstride = self.ctx.c_operand()

        A, s = self.A, self.s

        def dwp_call():
            if A > 1:          # over the B A rows (b, a): dpred [B A][K E], c_a straight out of the hidden states
                _hip.gemm_tn(_hip.ptr(self.dpred), _hip.ptr(ct, coff - (A - 1) * s * H), _hip.ptr(g["prediction_model.weight"]), B * A,
                             K * E, H, K * E, s * H, H, code, b_rpi=A, b_item=cstride, flags=_hip.GEMM_OUT_F32)
                return
            _hip.gemm_tn(_hip.ptr(self.dpred), _hip.ptr(ct, coff), _hip.ptr(g["prediction_model.weight"]), B, K * E, H,
                         K * E, H, H, code, b_rpi=1, b_item=cstride, flags=_hip.GEMM_OUT_F32)
        if self.use_aux and n > 1:
            self._deferred_side = [dwp_call]
        else:
            dwp_call()
        # (a B x H output with a K*E-long reduction: split the reduction over workgroups, sum the slabs in fixed order)
        ke = K * E
        R = B * A              # rows of dc: one per (item, anchor)
        dc_rows = self.dcA if A > 1 else self.dc
        ksplit = ke // 256 if (ke % 256 == 0 and ke >= 1024 and self.slabs.numel() >= (ke // 256) * R * H) else 1
        if ksplit > 1:
            _hip.gemm_nt(_hip.ptr(self.dpred), _hip.ptr(self.w_p_t), _hip.ptr(self.slabs), R, H, 256, ke, ke, H, code,
                         a_batch=256, b_batch=256, c_batch=R * H, batch=ksplit, flags=_hip.GEMM_OUT_F32)
            _hip.call("cpc_reduce_slabs", _hip.ptr(self.slabs), _hip.ptr(dc_rows), R, H, ksplit, R * H, 1, 1, H, 0)
        else:
            _hip.gemm_nt(_hip.ptr(self.dpred), _hip.ptr(self.w_p_t), _hip.ptr(dc_rows), R, H, ke, ke, ke, H, code,
                         flags=_hip.GEMM_OUT_F32)
        if A > 1:
            # the last anchor's row stays the f32 dc; the earlier anchors' rows go, rounded to the storage type, into the rows of the top
            # recurrent layer's dHs they own (two strided copies; every other row of dHs stays zero)
            rows = self.dcA.view(B, A, H)
            self.dc.copy_(rows[:, A - 1, :])
            self.ctx.anchor_dHs.view(B, V, H).index_copy_(1, self._anchor_steps, rows[:, :A - 1, :].to(self.dt))
        if add_dc is not None:
            self.dc.add_(add_dc)
        lanes_ok = self.use_aux and self.fuse_c1 and switches.wgrad_stream() and self._gp_phase == 0
        self._bl_active = self._bwd_lane() if lanes_ok else None
        if self._bl_active is not None:
            self._backward_target_rows(x, self._bl_active)
        self.ctx.backward(self.dc)      # parameter gradients of the context network + dz into rows [t0, t0+V) of dtop
        if A > 1:          # the earlier anchors' target gradients below row T-K, added to the dz just written there
            self._anchor_target_rows(T - K - (A - 1) * s, T - K, 1)
        if add_dz is not None:
            dtop.view(B, Ltop, E)[:, t0:t0 + V, :].add_(add_dz.transpose(1, 2), alpha=self.ctx.z_scale)
        self._backward_encoder(x, grad_ready_hook)
        for fn in self._deferred_side:           # an encoder backward without that side block (scalogram engine)
            fn()
        self._deferred_side = ()
        if self.use_aux:
            torch.cuda.current_stream().wait_stream(self.aux)

    def _bwd_lane(self):
        """The row split of the encoder's backward pass that mirrors encoder_forward's target lane, or None.  With kernel = 2 stride in
        every layer above the first, the data gradient at positions >= n_(l-1) of layer l-1 depends on output-gradient rows >= n_l only
        (n_l as in _target_lane_rows): GEMM rows [n_l + 1, L_alloc) of every data gradient — the part of the backward pass behind the TARGET
        frames, whose top-layer gradient is final once the loss kernels are — run on the side stream beside the GRU's backward recurrence
        (_backward_target_rows); the main stream's launches after the recurrence cover rows [0, n_l + 1).
        INVARIANT both target lanes rest on: rows >= T-K of the top-layer gradient are final before the context network's backward pass
        is issued.  Prediction anchors keep it: the loss chain (or the autograd bridge) ends with the gather of every anchor's target
        gradient into rows [T-K, T) (_anchor_target_rows, overwrite), and what the earlier anchors add lies below row T-K and is added
        on the main stream behind the context network's dz (backward()), in front of the main lane's data gradients.  The weight gradients stay
        one launch per layer: split at row n_l the same way (two slab sets, one reduction) they cost the step 0.37 ms — the chip is full
        once the recurrence has ended, and the second slab set is pure extra traffic (round 4, A/B of this lane: 4.52 off, 4.49 on,
        4.89 with the weight gradients split).  Tried on top of this and removed again: the recurrence itself in two step
        ranges with the encoder rows of the later frames beside the first (forward) / the earlier steps beside the encoder's backward pass
        over the late rows (backward) — bit-identical, and 0.0 - 0.1 ms SLOWER: what the hidden recurrence saves, the split launches lose."""
        bl = getattr(self, "_bl", 0)
        if bl != 0:
            return bl
        self._bl = None
        nr = self._target_lane_rows()
        n, B, La = self.n, self.B, self.geo.alloc
        if (nr is None or self.dt != torch.bfloat16 or not self.fuse_c1
                or type(self)._backward_encoder is not CPCEngine._backward_encoder
                or any(self.kernels[l] != 2 * self.strides[l] for l in range(1, n))
                or any(B * (La[l] - nr[l] - 1) < 256 for l in range(1, n))):
            return None
        dev, f32 = self.device, torch.float32
        bl = SimpleNamespace(n=nr, ev0=torch.cuda.Event(), ev=[torch.cuda.Event() for _ in range(n)], cs=[None] * n, tiles=[None] * n)
        for l in range(1, n):
            cin, cout, kw, s = self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l]
            bl.tiles[l] = (_ceil_div(B * (nr[l] + 1), 256), _ceil_div(B * (La[l] - nr[l] - 1), 256))
            if l >= 2 and self.cs_slabs[l - 1] is not None:        # (per-tile column sums: where the one-launch path has them)
                bl.cs[l - 1] = torch.zeros(sum(bl.tiles[l]) * s * cin, device=dev, dtype=f32)
        bl.c1_tile = (self.strides[1] * self.channels[0] // 256) * (self.kernels[0] + 1) * 256          # slab floats of one 256-row tile
        bl.c1 = torch.empty(sum(bl.tiles[1]) * bl.c1_tile, device=dev, dtype=f32)
        self._bl = bl
        return bl

    def _lane_dgrad(self, bl, l, part, x):
        """Data gradient of layer l: GEMM rows [0, n_l + 1) (part 0) or [n_l + 1, L_alloc) (part 1); layer 2's is fused with layer 1's
        weight gradient (cpc_conv_dgrad_conv1_rows)."""
        B, code, La, Lv = self.B, self.code, self.geo.alloc, self.geo.valid
        cin, cout, kw, s = self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l]
        lo, hi = (0, bl.n[l] + 1) if part == 0 else (bl.n[l] + 1, La[l])
        M = B * (hi - lo)
        tile = 256 if (l == 1 or bl.cs[l - 1] is not None) else _hip.nt_tile(code, M, s * cin, self.geo.taps[l] * cout)
        # (the side stream's launches, a fraction of a round of tiles each beside the recurrence, are booked under their own key)
        tkey = dict(key="gemm_nt" + _hip._variant(code, 0, tile) + ("@target_rows" if part else ""), work=2.0 * M * s * cin * self.geo.taps[l] * cout,
                    shape=("dgrad", M, s * cin, self.geo.taps[l] * cout))
        if l == 1:
            _hip.call("cpc_conv_dgrad_conv1_rows", _hip.ptr(self.dact[1]), _hip.ptr(self.w_dgrad[1]), _hip.ptr(self.act[0]),
                      _hip.ptr(x, self.x_off), _hip.ptr(bl.c1, part * bl.tiles[1][0] * bl.c1_tile), B, cin, cout, kw, s, La[1], self.L,
                      self.kernels[0], self.strides[0], Lv[0], C.c_longlong(self.guard[1]), code, _hip.ptr(self.act_bits[0]), lo, hi,
                      **dict(tkey, key=tkey["key"].replace("gemm_nt", "gemm_nt_conv1")))
        else:
            _hip.call("cpc_conv_dgrad_rows", _hip.ptr(self.dact[l]), _hip.ptr(self.w_dgrad[l]), _hip.ptr(self.act[l - 1]),
                      _hip.ptr(self.dact[l - 1]), B, cin, cout, kw, s, La[l], C.c_longlong(self.guard[l]), code,
                      _hip.ptr(self.act_bits[l - 1]), _hip.ptr(bl.cs[l - 1], part * bl.tiles[l][0] * s * cin), lo, hi, **tkey)

    def _backward_target_rows(self, x, bl):
        """Side stream, issued before the context network's backward pass: everything of the encoder's backward pass that hangs on the
        target frames alone (see _bwd_lane): the data-gradient chain; the main stream's launches wait for its events layer by layer."""
        bl.ev0.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.aux):
            self.aux.wait_event(bl.ev0)
            for l in range(self.n - 1, 0, -1):
                self._lane_dgrad(bl, l, 1, x)
                bl.ev[l].record(self.aux)

    def _backward_encoder(self, x, grad_ready_hook=None):
        """Encoder part of the backward pass: consumes the top-layer gradient, fills the encoder's parameter gradients."""
        g, code = self.model._grad, self.code
        B, n = self.B, self.n
        La, Lv = self.geo.alloc, self.geo.valid
        bl, self._bl_active = self._bl_active, None      # target lane (_bwd_lane): this pass covers rows [0, n_l + 1) only
        # Target lane invariant: every main-stream reader of rows the side stream's lane wrote (rows >= n_l of dact[l], the second slab
        # set of bl.c1) first waits on that layer's lane event bl.ev[l + 1] (bl.ev[1] for bl.c1).  Side-stream readers are ordered behind
        # the lane by their stream alone.
        cs_slabs = self.cs_slabs if bl is None else bl.cs
        # encoder, top layer down to layer 2.  Main stream: weight-gradient GEMM, data-gradient GEMM.  Side stream, after the
        # weight-gradient GEMM: the bias column sum (needs dact[l]) and the slab reduction, see _alloc_encoder.
        for l in range(n - 1, 0, -1):
            cin, cout, kw, s = self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l]
            bname = f"encoder.layers.{l}.bias"
            flops = 2.0 * B * La[l] * cout * kw * cin
            side_wgrad = switches.wgrad_stream()

            # The weight-gradient GEMM of layer l and the data-gradient GEMM of layer l both read dact[l] and are independent: the
            # weight gradient is issued on the side stream, beside the data-gradient chain (the tiles of the two kernels interleave on
            # the CUs, the partial last rounds of tiles of one launch are filled by the other, and both read dact[l] while it is in the
            # caches): 4.61 -> 4.55 ms per step at the end of round 2 (4.72 -> 4.69 before the side stream was cleared of the
            # column-sum passes).  Every kernel then runs longer BY ITSELF: bench.py reports the dominant kernel's roofline both as
            # it runs in the step and alone (switches.wgrad_stream off: everything on the main stream, the round-1 arrangement).
            def wgrad_call():
                _hip.call("cpc_conv_wgrad", _hip.ptr(self.act[l - 1]), _hip.ptr(self.dact[l]), _hip.ptr(self.wslab[l]), B, cin, cout, kw, s,
                          La[l], self.nsplit[l], C.c_longlong(self.guard[l - 1]), code,
                          key="gemm_tn" + _hip._variant(code, _hip.GEMM_OUT_F32, _hip.tn_tile(code, B * La[l], kw * cin, cout, self.nsplit[l],
                                                                                                 self._chunk(B * La[l], self.nsplit[l]))),
                          work=flops,
                          shape=("wgrad", B * La[l], kw * cin, cout, self.nsplit[l]))
            if not side_wgrad:
                if bl is not None and l < n - 1:
                    torch.cuda.current_stream().wait_event(bl.ev[l + 1])     # wgrad reads rows >= n_l of dact[l] (see below)
                wgrad_call()
            with self.side(self._ev_w[l]):
                for fn in self._deferred_side:       # work backward() put off the main stream (see there)
                    fn()
                self._deferred_side = ()
                if side_wgrad:
                    wgrad_call()
                # (ONE event per layer on the main stream: a recorded event between two GEMMs costs ~6 us of idle queue)
                if bname in g:
                    if cs_slabs[l] is not None:           # per-tile sums left by layer l+1's data gradient
                        _hip.call("cpc_reduce_slabs", _hip.ptr(cs_slabs[l]), _hip.ptr(g[bname]), 1, cout, cs_slabs[l].numel() // cout,
                                  cout, 1, 1, 0, 0)
                    else:
                        self._colsum_to_grad(_hip.ptr(self.dact[l]), g[bname], B * La[l], cout, scratch=self.aux_slabs)
                _hip.call("cpc_reduce_conv_w", _hip.ptr(self.wslab[l]), _hip.ptr(g[f"encoder.layers.{l}.weight"]), cin, cout, kw,
                          self.nsplit[l], kw * cin * cout)
                if grad_ready_hook is not None and l <= 2:
                    # everything from this encoder layer upwards (+ context network, predictor: later in the flat buffer) is final
                    # once the side stream gets here (its wait on _ev_w covers all earlier main-stream work): layers >= 3 and the
                    # head travel under the backward of layers 2 and 1, layer 2 (index 1) under the last data-gradient GEMM
                    off = self.model._offset
                    hi = off[f"encoder.layers.{l + 1}.weight"] if (l == 1 and n > 2) else self.model._flat_grad.numel()
                    grad_ready_hook(off[f"encoder.layers.{l}.weight"], hi)
            tkey = dict(key="gemm_nt" + _hip._variant(code, 0, _hip.nt_tile(code, B * La[l], s * cin, self.geo.taps[l] * cout)),
                        work=2.0 * B * La[l] * s * cin * self.geo.taps[l] * cout,
                        shape=("dgrad", B * La[l], s * cin, self.geo.taps[l] * cout))
            if bl is not None:
                if l < n - 1:
                    torch.cuda.current_stream().wait_event(bl.ev[l + 1])     # rows >= n_l of dact[l]: the side stream's data gradient of layer l+1
                self._lane_dgrad(bl, l, 0, x)
            elif l == 1 and self.fuse_c1:
                _hip.call("cpc_conv_dgrad_conv1", _hip.ptr(self.dact[1]), _hip.ptr(self.w_dgrad[1]), _hip.ptr(self.act[0]),
                          _hip.ptr(x, self.x_off), _hip.ptr(self.c1_slabs), B, cin, cout, kw, s, La[1], self.L, self.kernels[0],
                          self.strides[0], Lv[0], C.c_longlong(self.guard[1]), code, _hip.ptr(self.act_bits[0]),
                          **dict(tkey, key=tkey["key"].replace("gemm_nt", "gemm_nt_conv1")))
            else:
                _hip.call("cpc_conv_dgrad", _hip.ptr(self.dact[l]), _hip.ptr(self.w_dgrad[l]), _hip.ptr(self.act[l - 1]),
                          _hip.ptr(self.dact[l - 1]), B, cin, cout, kw, s, La[l], Lv[l - 1], C.c_longlong(self.guard[l]), code,
                          _hip.ptr(self.act_bits[l - 1]), _hip.ptr(self.cs_slabs[l - 1]), **tkey)
        # layer 1
        c0, k0, s0 = self.channels[0], self.kernels[0], self.strides[0]
        if bl is not None:
            torch.cuda.current_stream().wait_event(bl.ev[1])                 # the side stream's slab tiles of bl.c1 (part 1 of layer 1)
            _hip.call("cpc_conv1_fused_reduce_tiles", _hip.ptr(bl.c1), _hip.ptr(self.c1_tmp), _hip.ptr(g["encoder.layers.0.weight"]),
                      _hip.ptr(g.get("encoder.layers.0.bias")), sum(bl.tiles[1]), c0, self.strides[1], k0)
            return
        if self.fuse_c1:
            _hip.call("cpc_conv1_fused_reduce", _hip.ptr(self.c1_slabs), _hip.ptr(self.c1_tmp), _hip.ptr(g["encoder.layers.0.weight"]),
                      _hip.ptr(g.get("encoder.layers.0.bias")), B, c0, self.strides[1], La[1], k0)
            return
        nblk, nbb = self.c1_blocks, self.c1_item_blocks
        _hip.call("cpc_conv1_bwd", _hip.ptr(x, self.x_off), _hip.ptr(self.dact[0]), _hip.ptr(self.slabs), B, c0, s0, k0, self.L, Lv[0], La[0],
                  nblk, nbb, code)
        stride = (k0 + 1) * c0
        _hip.call("cpc_reduce_slabs", _hip.ptr(self.slabs), _hip.ptr(g["encoder.layers.0.weight"]), k0, c0, nbb * nblk, stride, 1, k0, 1, 0)
        if "encoder.layers.0.bias" in g:
            _hip.call("cpc_reduce_slabs", _hip.ptr(self.slabs, k0 * c0), _hip.ptr(g["encoder.layers.0.bias"]), 1, c0, nbb * nblk, stride,
                      1, 1, 0, 0)

    def input_gradient(self):
        """d / d x (B, L) float32 of whatever _backward_encoder() has just differentiated — the transposed convolution of layer 1
        (audio_model.py:38: nn.Conv1d(1, C, k, s), its autograd with respect to the input), for stand-alone encoder calls whose input
        requires grad.  Needs layer 1's output gradient in memory (the unfused route: dact[0]).  With D = ceil(k / s) taps,
          dx[b][t s + r] = sum_{d < D} sum_c dY[b][t - (D - 1 - d)][c] * w[c][r + (D - 1 - d) s]          (r < s; taps beyond k are zero)
        is ONE overlapped-row GEMM over dact[0]: row (b, t) = the D rows ending at t, K = D C, N = s (padded to 8).  Samples in front of
        x_off (frames the model never consumes, not computed at all) and behind the last window get zero."""
        B, C0, k0, s0, D = self.B, self.channels[0], self.kernels[0], self.strides[0], self.geo.taps[0]
        La0, dev = self.geo.alloc[0], self.device
        w = self.model._param["encoder.layers.0.weight"].detach().float().view(C0, k0)
        Bt = torch.zeros(8, D, C0, device=dev, dtype=torch.float32)
        for d in range(D):
            j0 = (D - 1 - d) * s0
            n = max(0, min(s0, k0 - j0))
            if n > 0:
                Bt[:n, d, :] = w[:, j0:j0 + n].t()
        Bt = Bt.view(8, D * C0).to(self.dt).contiguous()
        out = torch.empty(B * La0, 8, device=dev, dtype=torch.float32)
        if s0 > 8 or self.guard[0] < (D - 1) * C0:
            raise NotImplementedError("input gradient: layer-1 stride <= 8")
        _hip.gemm_nt(_hip.ptr(self.dact[0], -(D - 1) * C0), _hip.ptr(Bt), _hip.ptr(out), B * La0, 8, D * C0, C0, D * C0, 8, self.code,
                     flags=_hip.GEMM_OUT_F32)
        dx = torch.zeros(B, self.L, device=dev, dtype=torch.float32)
        n = min(self.L_eff, La0 * s0)
        dx[:, self.x_off:self.x_off + n] = out.view(B, La0, 8)[:, :, :s0].reshape(B, La0 * s0)[:, :n]
        return dx

    # ------------------------------------------------------------------------------------------ whole step
    def loss_and_grads(self, x, softplus: bool, regularization: float, all_timesteps: bool = False, grad_ready_hook=None,
                       global_negatives=None, after_loss=None, score: Optional[str] = None, negatives=None, negative_groups=None,
                       temperature=None, negative_bank=None):
        """Forward + loss + backward; returns the device tensor [loss, max_score, -mean valid, mean lse, reg, NaN indicator of
        this step, sticky NaN flag, -] (no sync; include/cpc_hip.h, cpc_nce_loss).
        ``global_negatives``: a GlobalNegatives object — the loss is then taken over the batches of ALL ranks.
        ``after_loss(nce_out)`` is called once the loss kernels are queued and before the backward pass is: data-parallel runs
        start the reduction of the NaN flag over the ranks there (GradAllReduce.reduce_flag).
        ``score``: "softplus" | "linear" | "difference" | "normalized" (score_kind; None: the ``softplus`` flag decides).
        ``temperature``: the temperature of "normalized" scores (finite and > 0; required there, a ValueError with any other kind).
        ``negatives``: None, or (n_neg, seed, draw): n_neg seeded negatives per target (nce_forward_backward); default branch only.
        ``negative_groups``: None, or (groups, mode): candidates by group id (nce_forward_backward); default branch only.
        ``negative_bank``: None, or a NegativeBank: earlier steps' predictions as further candidates (nce_forward_backward); default
        branch only."""
        kind = score_kind(softplus, score)
        temperature = check_temperature(temperature, kind)
        select_negatives(self.B, negatives, negative_groups, all_timesteps, global_negatives, negative_bank, kind,
                         temperature)          # refused before forward() runs
        if kind == "difference" and global_negatives is not None:
            raise NotImplementedError("difference scores under global negatives are not on the HIP path: the trainer takes the generic "
                                      "route there (contrastive_estimation_training.difference_score_function)")
        if kind == "normalized" and global_negatives is not None:
            raise NotImplementedError("normalized scores under global negatives are not on the HIP path: the trainer takes the generic "
                                      "route there (contrastive_estimation_training.NormalizedScoreFunction)")
        if self.A > 1 and (all_timesteps or global_negatives is not None or negatives is not None or negative_groups is not None
                           or negative_bank is not None or kind not in ("softplus", "linear")):
            raise NotImplementedError(ANCHOR_LOSS_REASON)
        tkw = {} if temperature is None else {"temperature": temperature}
        self.forward(x)
        if global_negatives is not None:
            global_negatives.forward_backward(softplus, regularization, all_timesteps)
        elif all_timesteps:
            self.nce_all_forward_backward(softplus, regularization, score=kind, **tkw)
        else:
            if negative_bank is not None:          # (without one nce_forward_backward is called as before the keyword existed)
                tkw["negative_bank"] = negative_bank
            self.nce_forward_backward(softplus, regularization, score=kind, negatives=negatives, negative_groups=negative_groups, **tkw)
        if after_loss is not None:
            after_loss(self.nce_out)
        self.backward(x, grad_ready_hook=grad_ready_hook)
        return self.nce_out

    def nan_flag(self):
        """One-element view of the sticky NaN flag (nce_out[6]): FusedAdam.skip_flag; zero it when a run starts."""
        return self.nce_out[6:7]

    def nan_pair(self):
        """Two-element view (nce_out[5:7]): the step's NaN indicator and the sticky flag, FusedAdam.nan_pair — what cpc_grad_norm
        raises when the gradient norm is not finite."""
        return self.nce_out[5:7]


class GlobalNegatives:
    """InfoNCE over the GLOBAL batch under one process per GPU — the loss the reference's nn.DataParallel wrap computes
    (setup_functions.py:112-115: outputs gathered to one device, scores and loss over all B x N items; SURVEY.md 8a13 / 8f
    rank 3).  Every rank all-gathers predicted_z and targets (2 x B K E storage-dtype elements per rank), computes the same
    global loss and its gradient with respect to all predictions / targets, and back-propagates the slice that belongs to
    its own clips; the parameter gradients of the ranks then ADD UP to the gradient of the global loss (all-reduce sum, no
    division).  The default data-parallel mode keeps per-GPU negatives (BASELINE.json's north star); this one is opt-in
    (``ContrastiveEstimationTrainer.global_negatives``).  Both loss branches."""

    def __init__(self, eng):
        import torch.distributed as dist
        self.dist, self.eng = dist, eng
        self.world, self.rank = dist.get_world_size(), dist.get_rank()
        B, K, E, dev, dt, f32 = eng.B, eng.K, eng.E, eng.device, eng.dt, torch.float32
        GB = B * self.world
        self.GB, self.ld = GB, _ceil_div(GB, 8) * 8
        self.local_targ = torch.empty(B * K * E, device=dev, dtype=dt)
        self.pred_all = torch.empty(GB * K * E, device=dev, dtype=dt)
        self.targ_all = torch.empty(GB * K * E, device=dev, dtype=dt)
        self.dpred_all = torch.empty(GB * K * E, device=dev, dtype=dt)
        self.dtarg_all = torch.empty(GB * K * E, device=dev, dtype=dt)
        self.S = torch.zeros(K * GB * self.ld, device=dev, dtype=f32)
        self.dS = torch.zeros(K * GB * self.ld, device=dev, dtype=dt)
        self.dST = torch.zeros(K * GB * self.ld, device=dev, dtype=dt)
        self.out = eng.nce_out          # loss values and NaN flags go straight to the engine's result cell
        self.ws = torch.empty(int(_hip.lib().cpc_nce_workspace_floats(GB, K)), device=dev, dtype=f32)

    def _all_timesteps(self, softplus: bool, regularization: float):
        """The full (GB K) x (GB K) score matrix over the gathered predictions / targets: the unfused all-timesteps
        stages of CPCEngine._loss_chain (scores, cpc_nce_loss_all, the two contractions) restated on the global batch."""
        e = self.eng
        code, E, K, GB = e.code, e.E, e.K, self.GB
        R = GB * K
        ld = _ceil_div(R, 8) * 8
        if getattr(self, "S_all", None) is None:
            dev, dt, f32 = e.device, e.dt, torch.float32
            self.S_all = torch.zeros(R * ld, device=dev, dtype=f32)
            self.ST_all = torch.zeros(R * ld, device=dev, dtype=f32)
            self.dS_all = torch.zeros(R * ld, device=dev, dtype=dt)
            self.dST_all = torch.zeros(R * ld, device=dev, dtype=dt)
            self.ws_all = torch.empty(int(_hip.lib().cpc_nce_all_workspace_floats(GB, K)), device=dev, dtype=f32)
            self.targT = torch.zeros(E, ld, device=dev, dtype=dt)
            self.predT = torch.zeros(E, ld, device=dev, dtype=dt)
        P = _hip.ptr
        _hip.gemm_nt(P(self.pred_all), P(self.targ_all), P(self.S_all), R, R, E, E, E, ld, code, flags=_hip.GEMM_OUT_F32)
        _hip.gemm_nt(P(self.targ_all), P(self.pred_all), P(self.ST_all), R, R, E, E, E, ld, code, flags=_hip.GEMM_OUT_F32)
        _hip.call("cpc_nce_loss_all", P(self.S_all), P(self.ST_all), P(self.dS_all), P(self.dST_all), P(self.out), P(self.ws_all), GB, K,
                  ld, 1 if softplus else 0, C.c_float(regularization), code)
        self.targT[:, :R].copy_(self.targ_all.view(R, E).t())
        self.predT[:, :R].copy_(self.pred_all.view(R, E).t())
        _hip.gemm_nt(P(self.dS_all), P(self.targT), P(self.dpred_all), R, E, ld, ld, ld, E, code)
        _hip.gemm_nt(P(self.dST_all), P(self.predT), P(self.dtarg_all), R, E, ld, ld, ld, E, code)

    def _all_timesteps_strips(self, softplus: bool, regularization: float):
        """The all-timesteps loss over the global batch WITHOUT the global score matrix on every rank: rank r forms two strips of it,
        (all predictions) x (its own targets) and (its own predictions) x (all targets) — 2 / world of the matrix instead of all of it.
        The column strip holds every row of its columns, so the column log-sum-exps, the regulariser's pair means and this rank's part of
        the loss are complete there (three partial sums + a maximum are all-reduced); its gradient gives d loss / d (own targets).  The row
        strip needs the log-sum-exps of ALL columns (one all-gather of R floats) and gives d loss / d (own predictions).  Fused kernels
        (cpc_score_lse / cpc_nce_fused_*): no f32 score matrix, no second (transposed) GEMM.  At 8 x 256 clips x 12 steps a rank computes
        4 x 77 GFLOP instead of 4 x 618."""
        e, dist = self.eng, self.dist
        code, E, K, B, GB, W = e.code, e.E, e.K, e.B, self.GB, self.world
        Rl, Rg = B * K, GB * K
        lo = self.rank * Rl
        s = getattr(self, "_strips", None)
        if s is None:
            dev, dt, f32 = e.device, e.dt, torch.float32
            s = self._strips = SimpleNamespace(
                Sc=torch.empty(Rg, Rl, device=dev, dtype=f32), dSc=torch.empty(Rg, Rl, device=dev, dtype=dt),
                dScT=torch.empty(Rl, Rg, device=dev, dtype=dt), Sr=torch.empty(Rl, Rg, device=dev, dtype=f32),
                dSr=torch.empty(Rl, Rg, device=dev, dtype=dt),
                pm=torch.empty(Rg // 256, Rl, device=dev, dtype=f32), ps=torch.empty(Rg // 256, Rl, device=dev, dtype=f32),
                pm2=torch.empty(Rl // 256, Rg, device=dev, dtype=f32), ps2=torch.empty(Rl // 256, Rg, device=dev, dtype=f32),
                valid=torch.zeros(Rg, device=dev, dtype=f32), lse_loc=torch.empty(Rl, device=dev, dtype=f32),
                lse_all=torch.empty(Rg, device=dev, dtype=f32), colp=torch.empty(_ceil_div(Rl, 256), 2, device=dev, dtype=f32),
                gradp=torch.empty(int(_hip.lib().cpc_nce_fused_grad_blocks(GB, Rl)), device=dev, dtype=f32),
                sums=torch.zeros(4, device=dev, dtype=f32),
                targT=torch.zeros(E, Rg, device=dev, dtype=dt), predT=torch.zeros(E, Rg, device=dev, dtype=dt))
        P, L, F = _hip.ptr, C.c_longlong, C.c_float
        sp = 1 if softplus else 0
        pred_all, targ_all = self.pred_all.view(Rg, E), self.targ_all.view(Rg, E)
        # column strip: every prediction against this rank's targets
        _hip.call("cpc_score_lse", P(pred_all), P(targ_all, lo * E), P(s.Sc), P(s.pm), P(s.ps), P(s.valid), Rg, Rl, E, L(E), L(E), L(Rl), -lo,
                  key="score_lse<bf16,256>", work=2.0 * Rg * Rl * E)
        _hip.call("cpc_nce_lse_merge", P(s.pm), P(s.ps), Rg // 256, Rl, sp, F(Rg), P(s.lse_loc), P(s.colp))
        _hip.call("cpc_nce_fused_grad", P(s.Sc), P(s.lse_loc), P(s.dSc), P(s.dScT), P(s.gradp), GB, K, Rl, L(Rl), L(Rg), -lo, sp,
                  F(regularization), F(Rg), F(GB))
        _hip.call("cpc_nce_fused_finalize", P(s.colp), s.colp.shape[0], P(s.valid, lo), Rl, P(s.gradp), s.gradp.numel(), P(s.sums), 1, F(Rg),
                  F(GB), K, F(regularization), sp, None)
        dist.all_reduce(s.sums[0:3])
        dist.all_reduce(s.sums[3:4], op=dist.ReduceOp.MAX)
        _hip.call("cpc_nce_fused_finalize", None, 0, None, 0, None, 0, P(s.sums), 2, F(Rg), F(GB), K, F(regularization), sp, P(self.out))
        dist.all_gather([s.lse_all[r * Rl:(r + 1) * Rl] for r in range(W)], s.lse_loc)
        # d loss / d own targets [c][:] = sum over ALL predictions r of dS[r][c] pred[r][:]
        s.predT.copy_(pred_all.t())
        _hip.gemm_nt(P(s.dScT), P(s.predT), P(self.dtarg_all, lo * E), Rl, E, Rg, Rg, Rg, E, code)
        # row strip: this rank's predictions against every target (the same kernel: identical accumulators; its column pairs are not used)
        _hip.call("cpc_score_lse", P(pred_all, lo * E), P(targ_all), P(s.Sr), P(s.pm2), P(s.ps2), None, Rl, Rg, E, L(E), L(E), L(Rg), lo,
                  key="score_lse<bf16,256>", work=2.0 * Rl * Rg * E)
        _hip.call("cpc_nce_fused_grad", P(s.Sr), P(s.lse_all), P(s.dSr), None, None, B, K, Rg, L(Rg), L(0), lo, sp, F(regularization), F(Rg),
                  F(GB))
        s.targT.copy_(targ_all.t())
        _hip.gemm_nt(P(s.dSr), P(s.targT), P(self.dpred_all, lo * E), Rl, E, Rg, Rg, Rg, E, code)

    # ---- Wasserstein gradient penalty with softplus scores under global negatives (scalogram_engine._gp_step): the summed scores run over
    # the GLOBAL score matrix, so the seeds of the penalty's passes are contractions with W1 = sigmoid(s) and W2 = softplus''(s) * (tangent
    # of s) over all ranks' predictions and targets.  Every rank forms the whole matrix (a parity path: the penalty costs three passes
    # through the network anyway) and keeps the rows / columns of its own clips.
    def _gp_sizes(self, all_timesteps):
        K, GB = self.eng.K, self.GB
        if all_timesteps:
            R = GB * K
            return 1, R, _ceil_div(R, 8) * 8
        return K, GB, self.ld

    def _gp_state(self, all_timesteps):
        g = getattr(self, "_gp", None)
        if g is not None and g.key == bool(all_timesteps):
            return g
        e = self.eng
        nb, R, ld = self._gp_sizes(all_timesteps)
        n = nb * R * ld
        f32 = dict(device=e.device, dtype=torch.float32)
        st = dict(device=e.device, dtype=e.dt)
        g = self._gp = SimpleNamespace(key=bool(all_timesteps), S=torch.zeros(n, **f32), St1=torch.zeros(n, **f32), St2=torch.zeros(n, **f32),
                                       W1=torch.zeros(n, **f32), W1T=torch.zeros(n, **f32), W2=torch.zeros(n, **f32), W2T=torch.zeros(n, **f32),
                                       pred_t_all=torch.zeros_like(self.pred_all), targ_t_all=torch.zeros_like(self.targ_all),
                                       local=torch.zeros_like(self.local_targ), out_p=torch.zeros_like(self.pred_all),
                                       out_t=torch.zeros_like(self.targ_all), out_p2=torch.zeros_like(self.pred_all),
                                       out_t2=torch.zeros_like(self.targ_all))
        for name in ("W1", "W1T", "W2", "W2T"):          # GEMM operands in the storage dtype
            setattr(g, name + "s", getattr(g, name) if e.dt == torch.float32 else torch.zeros(n, **st))
        if all_timesteps:
            g.aT, g.bT = torch.zeros(e.E, ld, **st), torch.zeros(e.E, ld, **st)
        return g

    def _gp_gather(self, pred, top, pred_all, targ_all, local):
        e = self.eng
        B, K, E, T, Ltop = e.B, e.K, e.E, e.T, e.geo.alloc[-1]
        n = B * K * E
        local.view(B, K, E).copy_(top.view(B, Ltop, E)[:, T - K:T, :])
        self.dist.all_gather([pred_all[r * n:(r + 1) * n] for r in range(self.world)], pred.contiguous())
        self.dist.all_gather([targ_all[r * n:(r + 1) * n] for r in range(self.world)], local)

    def _gp_scores(self, pa, ta, out, all_timesteps):
        e = self.eng
        P, code, E, K, GB = _hip.ptr, e.code, e.E, e.K, self.GB
        nb, R, ld = self._gp_sizes(all_timesteps)
        if all_timesteps:
            _hip.gemm_nt(P(pa), P(ta), P(out), R, R, E, E, E, ld, code, flags=_hip.GEMM_OUT_F32)
        else:
            _hip.gemm_nt(P(pa), P(ta), P(out), GB, GB, E, K * E, K * E, ld, code, a_batch=E, b_batch=E, c_batch=GB * ld, batch=K,
                         flags=_hip.GEMM_OUT_F32)

    def _gp_contract(self, W, WT, pa, ta, out_p, out_t, all_timesteps):
        """out_p[r] = sum_c W[r][c] ta[c],  out_t[c] = sum_r W[r][c] pa[r]  (W, WT in the storage dtype; all global rows / columns)."""
        e, g = self.eng, self._gp
        P, code, E, K, GB = _hip.ptr, e.code, e.E, e.K, self.GB
        nb, R, ld = self._gp_sizes(all_timesteps)
        if all_timesteps:
            g.aT[:, :R].copy_(ta.view(R, E).t())
            g.bT[:, :R].copy_(pa.view(R, E).t())
            _hip.gemm_nt(P(W), P(g.aT), P(out_p), R, E, ld, ld, ld, E, code)
            _hip.gemm_nt(P(WT), P(g.bT), P(out_t), R, E, ld, ld, ld, E, code)
        else:
            _hip.gemm_tn(P(WT), P(ta), P(out_p), GB, GB, E, ld, K * E, K * E, code, a_batch=GB * ld, b_batch=E, c_batch=E, batch=K)
            _hip.gemm_tn(P(W), P(pa), P(out_t), GB, GB, E, ld, K * E, K * E, code, a_batch=GB * ld, b_batch=E, c_batch=E, batch=K)

    def _gp_coeff(self, g, second, all_timesteps):
        nb, R, ld = self._gp_sizes(all_timesteps)
        P = _hip.ptr
        if second:
            _hip.call("cpc_gp_score_coeff", P(g.S), P(g.St1), P(g.St2), P(g.W2), P(g.W2T), nb, R, R, ld, ld, 1)
            names = ("W2", "W2T")
        else:
            _hip.call("cpc_gp_score_coeff", P(g.S), None, None, P(g.W1), P(g.W1T), nb, R, R, ld, ld, 0)
            names = ("W1", "W1T")
        for name in names:
            dst, src = getattr(g, name + "s"), getattr(g, name)
            if dst is not src:
                dst.copy_(src)

    def gp_softplus_seed(self, all_timesteps):
        """Pass 1: (adjoint of the local predictions [B K E], adjoint of the local targets [B, K, E]) of the summed global scores."""
        e = self.eng
        g = self._gp_state(all_timesteps)
        n = e.B * e.K * e.E
        self._gp_gather(e.pred, e.act[-1], self.pred_all, self.targ_all, self.local_targ)
        self._gp_scores(self.pred_all, self.targ_all, g.S, all_timesteps)
        self._gp_coeff(g, False, all_timesteps)
        self._gp_contract(g.W1s, g.W1Ts, self.pred_all, self.targ_all, g.out_p, g.out_t, all_timesteps)
        lo = self.rank * n
        return g.out_p[lo:lo + n], g.out_t[lo:lo + n].view(e.B, e.K, e.E)

    def gp_softplus_second(self, pred_t, top_t, all_timesteps):
        """Last pass: what the local predictions / targets gain from the tangent pass, nu_p = W1 (tangent targets) + W2 targets and
        nu_t = W1^T (tangent predictions) + W2^T predictions over the global batch (pred_all / targ_all / S are pass 1's)."""
        e = self.eng
        g = self._gp_state(all_timesteps)
        n = e.B * e.K * e.E
        self._gp_gather(pred_t, top_t, g.pred_t_all, g.targ_t_all, g.local)
        self._gp_scores(g.pred_t_all, self.targ_all, g.St1, all_timesteps)
        self._gp_scores(self.pred_all, g.targ_t_all, g.St2, all_timesteps)
        self._gp_coeff(g, True, all_timesteps)
        self._gp_contract(g.W1s, g.W1Ts, g.pred_t_all, g.targ_t_all, g.out_p, g.out_t, all_timesteps)
        self._gp_contract(g.W2s, g.W2Ts, self.pred_all, self.targ_all, g.out_p2, g.out_t2, all_timesteps)
        lo = self.rank * n
        add_p = g.out_p[lo:lo + n].view(e.B, e.K, e.E) + g.out_p2[lo:lo + n].view(e.B, e.K, e.E)
        add_t = g.out_t[lo:lo + n].view(e.B, e.K, e.E) + g.out_t2[lo:lo + n].view(e.B, e.K, e.E)
        return add_p, add_t

    def forward_backward(self, softplus: bool, regularization: float, all_timesteps: bool = False):
        e, dist = self.eng, self.dist
        code, B, E, K, GB, ld = e.code, e.B, e.E, e.K, self.GB, self.ld
        Ltop, T = e.geo.alloc[-1], e.T
        top, dtop = e.act[-1].view(B, Ltop, E), e.dact[-1].view(B, Ltop, E)
        n = B * K * E
        self.local_targ.view(B, K, E).copy_(top[:, T - K:T, :])
        dist.all_gather([self.pred_all[r * n:(r + 1) * n] for r in range(self.world)], e.pred)
        dist.all_gather([self.targ_all[r * n:(r + 1) * n] for r in range(self.world)], self.local_targ)
        P = _hip.ptr
        if all_timesteps:
            if e.fused_scores_ok(rows=B * K, cols=B * K):
                self._all_timesteps_strips(softplus, regularization)
            else:
                self._all_timesteps(softplus, regularization)
            lo = self.rank * n
            e.dpred.copy_(self.dpred_all[lo:lo + n])
            dtop[:, T - K:T, :].copy_(self.dtarg_all[lo:lo + n].view(B, K, E))
            return
        _hip.gemm_nt(P(self.pred_all), P(self.targ_all), P(self.S), GB, GB, E, K * E, K * E, ld, code, a_batch=E, b_batch=E,
                     c_batch=GB * ld, batch=K, flags=_hip.GEMM_OUT_F32)
        _hip.call("cpc_nce_loss", P(self.S), P(self.dS), P(self.dST), P(self.out), P(self.ws), GB, K, ld, 1 if softplus else 0,
                  C.c_float(regularization), code)
        _hip.gemm_tn(P(self.dST), P(self.targ_all), P(self.dpred_all), GB, GB, E, ld, K * E, K * E, code, a_batch=GB * ld, b_batch=E,
                     c_batch=E, batch=K)
        _hip.gemm_tn(P(self.dS), P(self.pred_all), P(self.dtarg_all), GB, GB, E, ld, K * E, K * E, code, a_batch=GB * ld, b_batch=E,
                     c_batch=E, batch=K)
        lo = self.rank * n
        e.dpred.copy_(self.dpred_all[lo:lo + n])
        dtop[:, T - K:T, :].copy_(self.dtarg_all[lo:lo + n].view(B, K, E))


class GradAllReduce:
    """Data-parallel gradient exchange: ONE sum over ranks of the model's flat f32 gradient buffer per step (RCCL over
    xGMI with backend "nccl"), issued in pieces as the backward pass completes them: encoder layers >= 3 + GRU + predictor
    (63 % of the bytes) travel while layers 2 and 1 are still being differentiated, layer 2 (28 %) under the last
    data-gradient GEMM, and only layer 1's 22 KB is left for finish().
    The mean is taken by FusedAdam's ``grad_scale = 1 / world``."""

    def __init__(self, model, optimizer=None, grad_scale=None):
        import torch.distributed as dist
        self.dist = dist
        self.model = model
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        self.pending = []
        self.split = None
        # With a FusedAdam given, a piece's parameters are updated (and their operand copies for the next step rebuilt, see
        # CPCEngine.prepare_ahead) as soon as its reduction has finished: at the next hook call, on the side stream beside the
        # remaining backward GEMMs, instead of after the whole backward pass.  grad_scale: 1 / world for the mean of the shard
        # gradients (default), 1 where the shard gradients add up (global negatives).
        self.optimizer = optimizer
        self.grad_scale = (1.0 / self.world) if grad_scale is None else float(grad_scale)
        self._plan, self.last_plan = [], []       # flat-gradient ranges in the order their reductions were issued (this step / last finished step)

    def describe(self):
        """The bucket plan of the last finished step, for a run's report (bench.py `data_parallel`): every range of the flat gradient buffer
        with its bytes and where its reduction is issued; ``covers_once`` says that the ranges tile the buffer exactly once."""
        flat = self.model._flat_grad
        esz, total = flat.element_size(), flat.numel()
        plan = list(self.last_plan)
        edges, ok = 0, True
        for lo, hi, _ in sorted(plan):
            ok = ok and lo == edges and hi > lo
            edges = hi
        return {"grad_bytes": total * esz, "world": self.world,
                "buckets": [{"lo": lo, "hi": hi, "bytes": (hi - lo) * esz, "issued": where} for lo, hi, where in plan],
                "covers_once": bool(ok and edges == total)}

    def reduce_flag(self, nce_out):
        """Pass as ``after_loss``: the sticky NaN flag (nce_out[6]) becomes the MAXIMUM over the ranks (and the step's indicator
        nce_out[5] with it), asynchronously, before any Adam piece of this step reads it — so that with per-GPU negatives, where
        every rank has its own loss, all ranks skip the same update and all of them leave train() at the same step."""
        if self.world > 1:
            self.flag_work = self.dist.all_reduce(nce_out[5:7], op=self.dist.ReduceOp.MAX, async_op=True)

    def _apply_finished(self):
        """Adam on every piece whose all-reduce has been issued: the current stream waits for the reduction first."""
        work = getattr(self, "flag_work", None)
        if work is not None:
            work.wait()
            self.flag_work = None
        for work, lo, hi in self.pending:
            work.wait()
            if self.optimizer is not None:
                self.optimizer.update_range(lo, hi, self.grad_scale)
        self.pending = []

    def hook(self, lo, hi):
        """Pass as ``grad_ready_hook``: starts the asynchronous all-reduce of flat_grad[lo:hi]."""
        if self.optimizer is not None:
            self._apply_finished()          # pieces issued at earlier hook calls (reduced while the backward pass went on)
        self.split = lo if self.split is None else min(self.split, lo)
        self._plan.append((lo, hi, "backward hook (overlapped)"))
        self.pending.append((self.dist.all_reduce(self.model._flat_grad[lo:hi], async_op=True), lo, hi))

    def finish(self):
        """Reduces what the hook has not covered and makes the current stream wait for all pieces.  With an optimizer attached
        the caller still calls ``optimizer.step(grad_scale)`` afterwards: it updates what is left (the head of the buffer)."""
        flat = self.model._flat_grad
        rest = flat if self.split is None else flat[:self.split]
        self._apply_finished()
        if rest.numel():
            self._plan.append((0, rest.numel(), "finish() (after the backward pass)"))
            self.dist.all_reduce(rest, async_op=True).wait()
        self.split = None
        self.last_plan, self._plan = self._plan, []


def check_max_grad_norm(max_grad_norm):
    """None, or the value as a float: ValueError unless it is finite and > 0 (what cpc_grad_norm admits)."""
    if max_grad_norm is None:
        return None
    try:
        value = float(max_grad_norm)
    except (TypeError, ValueError):
        raise ValueError(f"max_grad_norm must be None or a positive finite number, got {max_grad_norm!r}") from None
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"max_grad_norm must be None or a positive finite number, got {max_grad_norm!r}")
    return value


def check_weight_decay(weight_decay, decay_filter=None):
    """The decay as a float: ValueError unless it is finite and >= 0 (what cpc_adamw admits) and the filter None or callable."""
    try:
        value = float(weight_decay)
    except (TypeError, ValueError):
        raise ValueError(f"weight_decay must be a finite number >= 0, got {weight_decay!r}") from None
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f"weight_decay must be a finite number >= 0, got {weight_decay!r}")
    if decay_filter is not None and not callable(decay_filter):
        raise ValueError(f"weight_decay_filter must be None or callable(name, parameter) -> bool, got {decay_filter!r}")
    return value


def default_decay_filter(name, parameter):
    """Matrices and convolution kernels decay; biases and BatchNorm's weight and bias do not."""
    return parameter.dim() >= 2


def check_trust(trust_ratio, trust_clip=None):
    """(trust_ratio, trust_clip as a float or None): ValueError unless trust_ratio is a bool and trust_clip None or finite and > 0
    (what cpc_lamb admits)."""
    if not isinstance(trust_ratio, bool):
        raise ValueError(f"trust_ratio must be True or False, got {trust_ratio!r}")
    if trust_clip is None:
        return trust_ratio, None
    try:
        value = float(trust_clip)
    except (TypeError, ValueError):
        raise ValueError(f"trust_clip must be None or a positive finite number, got {trust_clip!r}") from None
    if isinstance(trust_clip, bool) or not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"trust_clip must be None or a positive finite number, got {trust_clip!r}")
    return trust_ratio, value


def check_ema(ema_decay, ema_warmup=False):
    """(ema_decay as a float or None, ema_warmup): ValueError unless ema_decay is None or a number (no bool) in [0, 1) — what cpc_ema
    admits —, ema_warmup a bool, and ema_warmup False without a decay."""
    if not isinstance(ema_warmup, bool):
        raise ValueError(f"ema_warmup must be True or False, got {ema_warmup!r}")
    if ema_decay is None:
        if ema_warmup:
            raise ValueError("ema_warmup=True needs an ema_decay")
        return None, False
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, numbers.Real):
        raise ValueError(f"ema_decay must be None or a number in [0, 1), got {ema_decay!r}")
    value = float(ema_decay)
    if not (math.isfinite(value) and 0.0 <= value < 1.0):
        raise ValueError(f"ema_decay must be None or a number in [0, 1), got {ema_decay!r}")
    return value, ema_warmup


def ema_weight(decay, warmup, t):
    """w = 1 - d of update number ``t`` (1-based) in Python floats: d = decay, or min(decay, (1 + t) / (10 + t)) under warmup
    ("EMA of the weights"; cpc_ema's host route computes the same double and rounds it once to float)."""
    if isinstance(t, bool) or not isinstance(t, int) or t < 1:
        raise ValueError(f"the number of the update being averaged must be an integer >= 1, got {t!r}")
    return 1.0 - (min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay)


class TorchEma:
    """The exponential moving average of the weights in torch ops, the definition of DESIGN.md, "EMA of the weights" (include/cpc_hip.h,
    cpc_ema, is the same on the flat buffer): after update number t, shadow <- shadow + (p - shadow) * (1 - d), d = ``decay`` or, with
    ``warmup``, min(decay, (1 + t) / (10 + t)); 1 - d == 1 copies the parameter.  Takes ``model.named_parameters()``; CPU or GPU tensors
    of any float dtype, nothing is read back to the host.  The shadow starts as a copy of the parameters (no bias correction), or is
    ``shadow`` = {name: tensor of the parameter's shape}, which is then updated in place.  Buffers (BatchNorm's running statistics) are
    not averaged."""

    def __init__(self, named_parameters, decay, warmup=False, shadow=None):
        self.decay, self.warmup = check_ema(decay, warmup)
        if self.decay is None:
            raise ValueError("TorchEma needs a decay in [0, 1)")
        self.named = [(n, p) for n, p in named_parameters]
        if shadow is None:
            shadow = {n: p.detach().clone() for n, p in self.named}
        self._check(shadow, "shadow")
        self.shadow = {n: shadow[n] for n, _ in self.named}
        self.updates = 0          # the number of the latest update averaged
        self._swapped = False

    def _check(self, tensors, what):
        if not isinstance(tensors, dict) or set(tensors) != {n for n, _ in self.named}:
            raise ValueError(f"{what} must be a dict with one tensor per parameter name")
        for n, p in self.named:
            if tuple(tensors[n].shape) != tuple(p.shape):
                raise ValueError(f"{what} of {n} has shape {tuple(tensors[n].shape)}, expected {tuple(p.shape)}")

    @torch.no_grad()
    def update(self, t):
        """Averages the parameters as they stand, as update number ``t`` (1-based: right behind the t-th optimizer.step())."""
        if self._swapped:
            raise RuntimeError("TorchEma.update inside weights(): the model holds the averaged weights")
        w = ema_weight(self.decay, self.warmup, t)
        for n, p in self.named:
            e = self.shadow[n]
            if w == 1.0:
                e.copy_(p)
            else:
                e.add_((p - e) * w)
        self.updates = t

    @torch.no_grad()
    def swap(self):
        """Exchanges parameters and shadow (in-place copies: every engine rebuilds its operand copies)."""
        for n, p in self.named:
            e = self.shadow[n]
            raw = p.detach().clone()
            p.copy_(e)
            e.copy_(raw)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def weights(self):
        """The model holds the averaged weights inside the block and the raw ones after it, also on an exception; does not nest."""
        if self._swapped:
            raise RuntimeError("TorchEma.weights() does not nest")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def state_dict(self):
        if self._swapped:
            raise RuntimeError("TorchEma.state_dict inside weights(): the shadow holds the raw weights")
        return {"decay": self.decay, "warmup": self.warmup, "ema": {n: e.detach().clone() for n, e in self.shadow.items()}}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Takes the shadow ('ema': {name: tensor}); decay and warmup stay the constructor's.  ValueError for a missing or misshapen entry."""
        if self._swapped:
            raise RuntimeError("TorchEma.load_state_dict inside weights()")
        self._check(state_dict.get("ema") if isinstance(state_dict, dict) else None, "state_dict['ema']")
        for n, e in self.shadow.items():
            e.copy_(state_dict["ema"][n])


class TorchLamb(torch.optim.Optimizer):
    """LAMB in torch ops, the definition of DESIGN.md, "LAMB trust ratios" (include/cpc_hip.h, cpc_lamb, is the same on the flat
    buffer): Adam's moments and bias-corrected direction r; u = r + weight_decay * p on the parameters
    ``decay_filter(name, parameter)`` selects (default: dim() >= 2), u = r on the others; trust = ||p|| / ||u|| where the parameter is
    selected and both norms are finite and > 0, else 1, at most ``trust_clip``; p <- p - lr * trust * u.  Takes
    ``model.named_parameters()``; CPU or GPU tensors of any float dtype, nothing is read back to the host.  The state is
    torch.optim.Adam's (step, exp_avg, exp_avg_sq), and ``load_state_dict`` takes a dict written by torch.optim.Adam / AdamW or
    FusedAdam; ``last_trust`` = {name: (w_norm, u_norm, ratio)} of the latest step."""

    def __init__(self, named_parameters, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay_filter=None, trust_clip=None):
        named = [(n, p) for n, p in named_parameters]
        weight_decay = check_weight_decay(weight_decay, decay_filter)
        _, trust_clip = check_trust(True, trust_clip)
        chosen = decay_filter or default_decay_filter
        self.names = {id(p): n for n, p in named}
        self.selected = {id(p): bool(chosen(n, p)) for n, p in named}
        self.last_trust = {}
        super().__init__([p for _, p in named], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, trust_clip=trust_clip))

    def load_state_dict(self, state_dict):
        """Takes the moments and step counts; the hyper-parameters stay the constructor's, as in FusedAdam.load_state_dict (torch
        replaces the param groups by the saved ones, which carry another optimizer's weight_decay and no trust_clip)."""
        own = [{k: group[k] for k in self.defaults} for group in self.param_groups]
        super().load_state_dict(state_dict)
        for group, kept in zip(self.param_groups, own):
            group.update(kept)

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            (b1, b2), eps, wd, clip = group["betas"], group["eps"], group["weight_decay"], group["trust_clip"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st.update(step=torch.tensor(0.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                st["step"] += 1
                t, m, v, g = int(st["step"]), st["exp_avg"], st["exp_avg_sq"], p.grad
                m.add_((g - m) * (1 - b1))
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                u = (m / (1 - b1 ** t)) / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
                selected = self.selected[id(p)]
                if selected:
                    u = u + wd * p
                w_norm, u_norm = p.norm(), u.norm()
                trust = torch.ones_like(w_norm)
                if selected:
                    usable = (w_norm > 0) & (u_norm > 0) & torch.isfinite(w_norm) & torch.isfinite(u_norm)
                    trust = torch.where(usable, w_norm / u_norm, trust)
                if clip is not None:
                    trust = trust.clamp(max=clip)
                self.last_trust[self.names[id(p)]] = (w_norm, u_norm, trust)
                p.sub_((group["lr"] * trust) * u)


class LRSchedule:
    """Warm-up, then a constant, linearly or cosine-decaying learning rate: step ``s`` (0-based) runs at ``lr * factor(s)``, what
    ``torch.optim.lr_scheduler.LambdaLR(optimizer, schedule.factor)`` with ``scheduler.step()`` behind every ``optimizer.step()``
    gives.  ``kind``: 'constant', 'linear' or 'cosine'; the factor rises as (s + 1) / warmup_steps over the first
    ``warmup_steps`` steps and falls from 1 to ``min_lr_ratio`` between step ``warmup_steps`` and step ``total_steps``, where it
    stays.  cpc_lr_factors / cpc_adamw_dev evaluate the same function on the device."""

    KINDS = ("constant", "linear", "cosine")

    def __init__(self, kind, warmup_steps=0, total_steps=None, min_lr_ratio=0.0):
        if kind not in self.KINDS:
            raise ValueError(f"LRSchedule kind must be one of {self.KINDS}, got {kind!r}")

        def whole(value, what):
            if isinstance(value, bool) or not isinstance(value, int):
                raise ValueError(f"LRSchedule {what} must be an integer, got {value!r}")
            return value
        self.kind = kind
        self.warmup_steps = whole(warmup_steps, "warmup_steps")
        if self.warmup_steps < 0:
            raise ValueError(f"LRSchedule warmup_steps must be >= 0, got {warmup_steps!r}")
        if total_steps is None:
            if kind != "constant":
                raise ValueError(f"LRSchedule('{kind}') needs total_steps")
        elif whole(total_steps, "total_steps") <= self.warmup_steps:
            raise ValueError(f"LRSchedule total_steps ({total_steps!r}) must be greater than warmup_steps ({warmup_steps!r})")
        self.total_steps = total_steps
        try:
            self.min_lr_ratio = float(min_lr_ratio)
        except (TypeError, ValueError):
            raise ValueError(f"LRSchedule min_lr_ratio must be a number in [0, 1], got {min_lr_ratio!r}") from None
        if not 0.0 <= self.min_lr_ratio <= 1.0:
            raise ValueError(f"LRSchedule min_lr_ratio must be in [0, 1], got {min_lr_ratio!r}")

    def factor(self, s):
        """The factor of the step with 0-based index ``s`` (trainer.training_step), in Python floats."""
        W, T, r = self.warmup_steps, self.total_steps, self.min_lr_ratio
        if s < W:
            return (s + 1) / W
        if self.kind == "constant":
            return 1.0
        q = min((s - W) / (T - W), 1.0)
        if self.kind == "linear":
            return r + (1.0 - r) * (1.0 - q)
        return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q))

    def abi_args(self):
        """(kind, warmup_steps, total_steps, min_ratio) as cpc_lr_factors / cpc_adamw_dev take them."""
        total = self.total_steps if self.total_steps is not None else self.warmup_steps + 1
        return self.KINDS.index(self.kind), C.c_longlong(self.warmup_steps), C.c_longlong(total), C.c_float(self.min_lr_ratio)

    def __repr__(self):
        return (f"LRSchedule({self.kind!r}, warmup_steps={self.warmup_steps}, total_steps={self.total_steps}, "
                f"min_lr_ratio={self.min_lr_ratio})")


class FusedAdam:
    """torch.optim.Adam (default betas / eps) over the model's flat f32 parameter buffer as one kernel; with ``weight_decay`` > 0
    torch.optim.AdamW on the parameters ``decay_filter`` selects, with ``schedule`` at the learning rate lr * schedule.factor(step);
    with ``trust_ratio`` LAMB (TorchLamb's definition): the decay joins Adam's direction and every selected parameter's update is
    scaled by ||p|| / ||direction||, at most ``trust_clip``."""

    def __init__(self, model, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, device_step: bool = False, max_grad_norm=None,
                 weight_decay: float = 0.0, decay_filter=None, schedule=None, step_offset: int = 0, trust_ratio: bool = False,
                 trust_clip=None, ema_decay=None, ema_warmup: bool = False, ema=None, temperature=None):
        self.model = model
        # temperature ("Learnable and scheduled temperature"): a DeviceTemperature.  In learnable mode step() issues one
        # cpc_temperature_step behind its final update — the same stream, step number and skip flag — at lr * temperature.lr_scale: the
        # scalar's gradient is no part of cpc_grad_norm, is not scaled by the clipping coefficient and gets no trust ratio and no decay.
        # In scheduled mode step() only advances the object's step index.  None: no launch is added.
        if temperature is not None and not isinstance(temperature, DeviceTemperature):
            raise ValueError(f"temperature must be None or a DeviceTemperature, got {temperature!r}")
        self.temperature = temperature
        # ema_decay / ema_warmup / ema ("EMA of the weights"): every update issued by _update is followed by a cpc_ema launch
        # over the same range, stream, step number and skip flag.  self.ema is the shadow, a flat f32 tensor shaped like the parameter
        # buffer: the caller's ``ema`` (updated in place) or a copy of the parameters as they stand.  Without a decay it is None: nothing
        # is allocated and no launch is added.
        self.ema_decay, self.ema_warmup = check_ema(ema_decay, ema_warmup)
        if ema is not None:
            if self.ema_decay is None:
                raise ValueError("ema given without an ema_decay")
            flat_ = model._flat_param
            if (not isinstance(ema, torch.Tensor) or ema.dtype != torch.float32 or tuple(ema.shape) != tuple(flat_.shape)
                    or ema.device != flat_.device or not ema.is_contiguous()):
                raise ValueError(f"ema must be a contiguous float32 tensor of shape {tuple(flat_.shape)} on {flat_.device}")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        # weight_decay / decay_filter / schedule / step_offset ("AdamW and the learning-rate schedule").  Step number i of
        # this object (0-based, counted from construction or from load_state_dict) has the schedule index step_offset + i and runs at
        # self.lr = base_lr * schedule.factor(index): set here before the step's first launch, on the device under device_step.
        # decay_bits: one bit per 64-float block of the flat buffer, set for the blocks of the parameters that decay (their
        # alignment padding included), 32 blocks per int32 word.  Without decay and schedule none of this is allocated or reached.
        self.weight_decay = check_weight_decay(weight_decay, decay_filter)
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise ValueError(f"schedule must be None or an LRSchedule, got {schedule!r}")
        if isinstance(step_offset, bool) or not isinstance(step_offset, int) or step_offset < 0:
            raise ValueError(f"step_offset must be an integer >= 0, got {step_offset!r}")
        self.base_lr, self.schedule, self.step_offset, self._t0 = self.lr, schedule, step_offset, 0
        # trust_ratio / trust_clip ("LAMB trust ratios"): every update is a cpc_lamb call over whole parameters.  The
        # bitmap then also selects who gets a ratio and is built for weight_decay == 0 too; the parameter table, its inverse, the
        # block sums' workspace and trust f32[3][parameters] are built once, here.  With trust_ratio=False none of them exists.
        self.trust_ratio, self.trust_clip = check_trust(trust_ratio, trust_clip)
        if self.trust_ratio and device_step:
            raise NotImplementedError("trust_ratio with device_step=True: the three launches of a LAMB update take the step's bias "
                                      "corrections and learning rate from the host; no captured LAMB step exists")
        decays = self.weight_decay > 0.0 or self.trust_ratio
        self.decay_bits = self._decay_bitmap(decay_filter or default_decay_filter) if decays else None
        flat = model._flat_param
        if self.trust_ratio:
            self._lamb_tables()
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.ema = None if self.ema_decay is None else (ema if ema is not None else flat.detach().clone())
        self._ema_in = False          # True inside ema_weights(): the model holds the averaged weights, self.ema the raw ones
        self.t = 0
        self._done_lo = None
        self._piece_scale = 1.0
        # after_update(lo, hi, final): called right after flat_param[lo:hi) was updated; set it to the engine's prepare_ahead in
        # single-process training so that the operand copies of the next step are rebuilt off the critical path
        self.after_update = None
        # skip_flag: one-element device tensor (CPCEngine.nan_flag()); while it is non-zero every update is a no-op on the device
        # — the reference's NaN guard returns before backward() / optimizer.step() (contrastive_estimation_training.py:124-133).
        # Every launch that owns state takes it: _update, _update_lamb, _update_ema, _update_temperature (learnable); a launch added
        # here without it is what tests/test_nan_guard_routes_gpu.py's controls stand for.  self.lr and self.t are host values: the
        # trainer's _NanRollback puts them back
        self.skip_flag = None
        # device_step: the step count lives on the device (cpc_adam_dev), so the call's arguments never change and the step
        # can be part of a captured hipGraph
        self.state = torch.zeros(4, device=flat.device, dtype=torch.float32) if device_step else None
        # max_grad_norm: torch.nn.utils.clip_grad_norm_ in front of the update ("Gradient clipping").  The norm needs the
        # WHOLE gradient, so hook() / update_range() only record their range and step() runs cpc_grad_norm and one cpc_adam_clip
        # over the buffer.  clip_state (device f32[4]) = {norm before clipping, coefficient applied, 1 if the norm is not finite,
        # max_grad_norm}; nan_pair: two-element device tensor (CPCEngine.nan_pair()) raised when the norm is not finite.
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self.nan_pair = None
        if self.max_grad_norm is not None:
            if device_step:
                raise NotImplementedError("max_grad_norm with device_step=True: clipped steps are not captured into a hipGraph")
            self.clip_state = torch.zeros(4, device=flat.device, dtype=torch.float32)
            self._clip_ws = torch.empty(int(_hip.lib().cpc_grad_norm_workspace_floats(flat.numel())), device=flat.device,
                                        dtype=torch.float32)

    def hook(self, lo, hi):
        """Single-process use as ``grad_ready_hook``: updates flat_param[lo:hi] as soon as the backward pass reports that range
        of the gradient final (the engine calls it from its side stream, beside the remaining data-gradient GEMMs); step()
        then updates what is left.  Nothing the backward pass still runs reads the f32 master parameters of a finished range
        (the GEMMs use the storage-dtype operand copies made at the start of the step).  Not for data-parallel runs, where the
        update has to follow the all-reduce."""
        if self.state is not None:
            raise ValueError("FusedAdam.hook needs the host-side step count (device_step=False)")
        self.update_range(lo, hi, 1.0)

    def update_range(self, lo, hi, grad_scale=1.0):
        """Data-parallel use (GradAllReduce): Adam on flat_param[lo:hi) once that range of the gradient has been reduced over
        the ranks, with the step count of the step in progress; step(grad_scale) then updates the head of the buffer."""
        if self.state is not None:
            raise ValueError("piecewise updates need the host-side step count (device_step=False)")
        self._not_swapped_in()
        self._done_lo = lo if self._done_lo is None else min(self._done_lo, lo)
        self._piece_scale = float(grad_scale)
        if self.max_grad_norm is not None:          # the update waits for the norm of the whole gradient: step()
            return
        self._scheduled_lr(self.t)
        self._update(lo, hi, self.t + 1, grad_scale)
        if self.after_update is not None:
            self.after_update(lo, hi, False)

    def _update(self, lo, hi, t, grad_scale, coef=None):
        """The one place that issues the update of flat_param[lo:hi) as step ``t``.  Host-side step count: cpc_adamw when a decay
        bitmap is set, else cpc_adam_clip when ``coef`` (device pointer to the clipping coefficient) is given, else cpc_adam.
        device_step: cpc_adamw_dev when decay or a schedule is set (the device evaluates the schedule from the base rate), else
        cpc_adam_dev; both keep the count themselves and ignore ``t``."""
        if hi <= lo:
            return
        if self.trust_ratio:
            self._update_lamb(lo, hi, t, grad_scale, coef)
            return self._update_ema(lo, hi, t)
        model, dev, decayed = self.model, self.state is not None, self.decay_bits is not None
        model._raw_updates = getattr(model, "_raw_updates", 0) + 1
        dev_schedule = dev and (decayed or self.schedule is not None)
        head = [_hip.ptr(x, lo) for x in (model._flat_param, model._flat_grad, self.m, self.v)]
        head += [C.c_longlong(hi - lo), C.c_float(self.base_lr if dev_schedule else self.lr), C.c_float(self.betas[0]),
                 C.c_float(self.betas[1]), C.c_float(self.eps), _hip.ptr(self.state) if dev else t, C.c_float(grad_scale)]
        if dev_schedule:
            # the device evaluates the schedule at (its step count - 1) + offset: the count starts at _t0 where step_offset does
            offset = self.step_offset - self._t0
            if offset < 0:
                raise ValueError(f"device_step: the loaded step count {self._t0} lies beyond step_offset {self.step_offset}")
            sched = self.schedule.abi_args() if self.schedule is not None else LRSchedule("constant").abi_args()
            name, tail = "cpc_adamw_dev", [C.c_float(self.weight_decay), _hip.ptr(self.decay_bits), *sched, C.c_longlong(offset), None]
        elif dev:
            name, tail = "cpc_adam_dev", []
        elif decayed:          # a range starts at a parameter: a 64-float block of the bitmap
            assert lo % 64 == 0, f"a decayed range has to start at a 64-float boundary, got {lo}"
            name, tail = "cpc_adamw", [C.c_float(self.weight_decay), _hip.ptr(self.decay_bits), C.c_longlong(lo // 64), coef]
        elif coef is not None:
            name, tail = "cpc_adam_clip", [coef]
        else:
            name, tail = "cpc_adam", []
        _hip.call(name, *head, *tail, _hip.ptr(self.skip_flag))
        self._update_ema(lo, hi, t)

    def _update_ema(self, lo, hi, t):
        """The average of flat_param[lo:hi) behind its update as step ``t``: one cpc_ema launch on the update's stream, under its skip
        flag; under device_step the step count is the device's (self.state, which the update has advanced).  Every range starts at a
        parameter, a 64-float boundary, so the pieces carry the whole buffer's bits."""
        if self.ema is None:
            return
        dev = self.state is not None
        _hip.call("cpc_ema", _hip.ptr(self.model._flat_param, lo), _hip.ptr(self.ema, lo), C.c_longlong(hi - lo), C.c_float(self.ema_decay),
                  1 if self.ema_warmup else 0, 0 if dev else t, _hip.ptr(self.state) if dev else None, _hip.ptr(self.skip_flag))

    def _update_temperature(self, t, grad_scale):
        """The temperature behind the step's final update, as step ``t``.  Learnable: Adam on s = log(1 / tau) from the dots the latest
        backward left (cpc_temperature_step), with the run's betas and eps; under device_step the step size comes from self.state, which
        the update has advanced (state[1] carries lr * schedule factor / (1 - beta1^t)), times lr_scale.  Scheduled: the step index moves on."""
        temp = self.temperature
        if temp is None:
            return
        if temp.mode == "scheduled":
            temp.step = self.step_offset + t - self._t0
            return
        if temp.dots is None:
            raise ValueError("FusedAdam(temperature=...): no backward pass has run with this DeviceTemperature (pass it as temperature= of "
                             "the loss call)")
        dev = self.state is not None
        s_min, s_max = temp.bounds
        _hip.call("cpc_temperature_step", _hip.ptr(temp.tstate), _hip.ptr(temp.dots), int(temp.dots.numel()),
                  C.c_float(temp.lr_scale if dev else self.lr * temp.lr_scale), C.c_float(self.betas[0]), C.c_float(self.betas[1]),
                  C.c_float(self.eps), 0 if dev else t, _hip.ptr(self.state) if dev else None, C.c_float(grad_scale), C.c_float(s_min),
                  C.c_float(s_max), _hip.ptr(self.skip_flag))

    # ---- the averaged weights in the model's place
    def _not_swapped_in(self):
        if self._ema_in:
            raise RuntimeError("an optimizer step inside ema_weights(): the model holds the averaged weights")

    def swap_ema(self):
        """Exchanges the parameter buffer and the shadow (cpc_ema_swap over the whole buffer) and bumps model._raw_updates: every
        engine's prepare_weights() rebuilds its operand copies and a pending prepare_ahead token is void.  An evaluation-time call: it
        waits for the device first, so that nothing on another stream still reads or writes the parameters."""
        if self.ema is None:
            raise ValueError("swap_ema() needs FusedAdam(ema_decay=...)")
        model = self.model
        if model._flat_param.is_cuda:
            torch.cuda.synchronize(model._flat_param.device)
        _hip.call("cpc_ema_swap", _hip.ptr(model._flat_param), _hip.ptr(self.ema), C.c_longlong(model._flat_param.numel()))
        model._raw_updates = getattr(model, "_raw_updates", 0) + 1
        self._ema_in = not self._ema_in

    @contextlib.contextmanager
    def ema_weights(self):
        """The model computes with the averaged weights inside the block and has its raw ones back after it, bit for bit, also on an
        exception.  RuntimeError when nested, and while pieces of a step are outstanding; step() / update_range() refuse inside."""
        if self.ema is None:
            raise ValueError("ema_weights() needs FusedAdam(ema_decay=...)")
        if self._ema_in:
            raise RuntimeError("ema_weights() does not nest")
        if self._done_lo is not None:
            raise RuntimeError("ema_weights() between the pieces of a step and its step(): the parameters are half updated")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self):
        """The model's state_dict() with every parameter taken from the shadow and every buffer from the live model (copies).
        BatchNorm's running statistics are buffers: they are not averaged."""
        if self.ema is None:
            raise ValueError("ema_state_dict() needs FusedAdam(ema_decay=...)")
        source = self.model._flat_param if self._ema_in else self.ema
        out = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for name, p in self.model.named_parameters():
            lo = self.model._offset[name]
            out[name] = source[lo:lo + p.numel()].view(p.shape).detach().clone()
        return out

    def _lamb_tables(self):
        """The per-parameter buffers of cpc_lamb, from model._offset (parameters in buffer order, each at a 64-float boundary, its
        padding behind it): _param_block (host int32 table, parameter q covers blocks [q], [q + 1]), its device copy, the per-block
        inverse map, the workspace and ``trust``."""
        flat, offset = self.model._flat_param, self.model._offset
        names = sorted(offset, key=offset.get)
        sizes = dict((n, p.numel()) for n, p in self.model.named_parameters())
        edges = [offset[n] for n in names] + [flat.numel()]
        assert edges[0] == 0 and all(e % 64 == 0 for e in edges), "parameters start at 64-float boundaries of the flat buffer"
        assert all(0 < sizes[n] <= b - a for n, a, b in zip(names, edges, edges[1:]))
        self._lamb_names = names
        self._param_at = {e: q for q, e in enumerate(edges)}          # float offset -> index of the parameter that starts there
        self._param_block = (C.c_int * len(edges))(*(e // 64 for e in edges))
        table = torch.tensor(list(self._param_block), dtype=torch.int32)
        self._param_block_dev = table.to(flat.device)
        self._block_param = torch.repeat_interleave(torch.arange(len(names), dtype=torch.int32),
                                                    (table[1:] - table[:-1]).long()).to(flat.device)
        floats = int(_hip.lib().cpc_lamb_workspace_floats(flat.numel() // 64))
        self._lamb_ws = torch.zeros(floats, device=flat.device, dtype=torch.float32)
        self.trust = torch.zeros(3, len(names), device=flat.device, dtype=torch.float32)

    def _update_lamb(self, lo, hi, t, grad_scale, coef):
        """_update under trust_ratio: one cpc_lamb call (three launches) over the whole parameters of flat_param[lo:hi)."""
        model = self.model
        assert lo in self._param_at and hi in self._param_at, f"a LAMB update covers whole parameters, got [{lo}, {hi})"
        first, count = self._param_at[lo], self._param_at[hi] - self._param_at[lo]
        model._raw_updates = getattr(model, "_raw_updates", 0) + 1
        _hip.call("cpc_lamb", *[_hip.ptr(x, lo) for x in (model._flat_param, model._flat_grad, self.m, self.v)],
                  C.c_longlong(hi - lo), C.c_float(self.lr), C.c_float(self.betas[0]), C.c_float(self.betas[1]), C.c_float(self.eps), t,
                  C.c_float(grad_scale), C.c_float(self.weight_decay), _hip.ptr(self.decay_bits), C.c_longlong(lo // 64), coef,
                  C.cast(self._param_block, C.c_void_p), _hip.ptr(self._param_block_dev), _hip.ptr(self._block_param), first, count,
                  len(self._lamb_names), C.c_float(-1.0 if self.trust_clip is None else self.trust_clip), _hip.ptr(self._lamb_ws),
                  _hip.ptr(self.trust), _hip.ptr(self.skip_flag))

    def trust_ratios(self):
        """{parameter name: (w_norm, u_norm, ratio applied)} of the latest step, with one synchronous read.  For inspection: not to
        be called in the training loop."""
        if not self.trust_ratio:
            raise ValueError("trust_ratios() needs FusedAdam(trust_ratio=True)")
        rows = self.trust.cpu().tolist()
        return {n: (rows[0][q], rows[1][q], rows[2][q]) for q, n in enumerate(self._lamb_names)}

    def _scheduled_lr(self, steps_done):
        """With a schedule: self.lr becomes the rate of the step that follows ``steps_done`` finished ones."""
        if self.schedule is not None:
            self.lr = self.base_lr * self.schedule.factor(self.step_offset + steps_done - self._t0)

    def _decay_bitmap(self, decay_filter):
        """int32 words on the buffer's device: bit j % 32 of word j // 32 is set when floats [64 j, 64 j + 64) belong to a parameter
        the filter selects (model._offset puts every parameter at a 64-float boundary; its padding follows it)."""
        offset, total = self.model._offset, self.model._flat_param.numel()
        assert total % 64 == 0
        blocks = total // 64
        words = [0] * ((blocks + 31) // 32)
        for name, p in self.model.named_parameters():
            assert offset[name] % 64 == 0
            if decay_filter(name, p):
                for j in range(offset[name] // 64, (offset[name] + p.numel() + 63) // 64):
                    words[j // 32] |= 1 << (j % 32)
        signed = [w - (1 << 32) if w >= (1 << 31) else w for w in words]
        return torch.tensor(signed, dtype=torch.int32).to(self.model._flat_param.device)

    # ---- state in torch.optim.Adam's format
    def state_dict(self):
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [one group]} with i in model.parameters() order, as
        torch.optim.Adam / AdamW write and load it (copies of the moments; 'lr' is the rate of the latest step)."""
        state, offset = {}, self.model._offset
        for i, (name, p) in enumerate(self.model.named_parameters()):
            lo, n = offset[name], p.numel()
            state[i] = {"step": torch.tensor(float(self.t)), "exp_avg": self.m[lo:lo + n].view(p.shape).clone(),
                        "exp_avg_sq": self.v[lo:lo + n].view(p.shape).clone()}
            if self.ema is not None:          # (the shadow rides along, as a fourth per-parameter tensor; without it: Adam's dict)
                self._not_swapped_in()
                state[i]["ema"] = self.ema[lo:lo + n].view(p.shape).clone()
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": True, "params": list(range(len(state)))}
        out = {"state": state, "param_groups": [group]}
        if self.temperature is not None:          # (the scalar rides along under a key of its own; without it: Adam's dict)
            out["temperature"] = self.temperature.state_dict()
        return out

    def load_state_dict(self, state_dict):
        """Takes the moments and the step count of a state dict in torch.optim.Adam's format (an empty 'state' — an optimizer that
        has not stepped — gives zero moments and step 0).  The hyper-parameters stay the constructor's: 'lr' of a scheduled run is
        one step's rate, not the base rate.  The schedule goes on from ``step_offset`` at the next step.  ValueError for entries
        that are missing, have the wrong shape, or carry different step counts."""
        saved, offset = state_dict["state"], self.model._offset
        named = list(self.model.named_parameters())
        if saved and sorted(saved) != list(range(len(named))):
            raise ValueError(f"the state dict has entries {sorted(saved)} for {len(named)} parameters")
        steps = set()
        # the shadow: taken where every entry carries it, otherwise started over from the parameters as they stand
        takes_ema = self.ema is not None and bool(saved) and all("ema" in saved[i] for i in range(len(named)))
        if self.ema is not None:
            self._not_swapped_in()
        for i, (name, p) in enumerate(named):
            if not saved:
                break
            entry = saved[i]
            for key in ("exp_avg", "exp_avg_sq") + (("ema",) if takes_ema else ()):
                if tuple(entry[key].shape) != tuple(p.shape):
                    raise ValueError(f"{key} of parameter {i} ({name}) has shape {tuple(entry[key].shape)}, expected {tuple(p.shape)}")
            steps.add(int(entry["step"]))
        if len(steps) > 1:
            raise ValueError(f"the parameters carry different step counts {sorted(steps)}; this optimizer keeps one")
        with torch.no_grad():
            self.m.zero_()
            self.v.zero_()
            for i, (name, p) in enumerate(named):
                if not saved:
                    break
                lo, n = offset[name], p.numel()
                self.m[lo:lo + n].view(p.shape).copy_(saved[i]["exp_avg"])
                self.v[lo:lo + n].view(p.shape).copy_(saved[i]["exp_avg_sq"])
                if takes_ema:
                    self.ema[lo:lo + n].view(p.shape).copy_(saved[i]["ema"])
            if self.ema is not None and not takes_ema:
                self.ema.copy_(self.model._flat_param.detach())
            self.t = self._t0 = steps.pop() if steps else 0
            self._done_lo = None
            if self.state is not None:          # cpc_adam_dev keeps the count as the bits of an int
                self.state[0:1].copy_(torch.tensor([self.t], dtype=torch.int32).view(torch.float32))
        if self.temperature is not None and state_dict.get("temperature") is not None:
            self.temperature.load_state_dict(state_dict["temperature"])
            self.temperature.step = self.step_offset

    def _grad_norm(self, grad_scale):
        """Queues the norm of grad_scale * (whole flat gradient) — under data parallelism the gradient summed over the ranks, the same
        on every rank — and returns the device pointer to the clipping coefficient.  Nothing is read back here."""
        grad = self.model._flat_grad
        _hip.call("cpc_grad_norm", _hip.ptr(grad), C.c_longlong(grad.numel()), C.c_float(grad_scale), C.c_float(self.max_grad_norm),
                  _hip.ptr(self._clip_ws), _hip.ptr(self.clip_state), _hip.ptr(self.nan_pair))
        return _hip.ptr(self.clip_state, 1)

    def step(self, grad_scale: float = 1.0):
        self._not_swapped_in()
        self._scheduled_lr(self.t)
        self.t += 1
        hi, clip = self.model._flat_param.numel(), self.max_grad_norm is not None
        if self._done_lo is not None:          # hook() / update_range() ran during the backward pass
            if not clip:                       # and updated [done_lo, end): the head of the buffer is left
                hi, self._done_lo = self._done_lo, None
            if float(grad_scale) != self._piece_scale:
                raise ValueError(f"the pieces of this step were {'recorded' if clip else 'updated'} with grad_scale "
                                 f"{self._piece_scale}, step() got {grad_scale}")
            self._done_lo = None
        coef = self._grad_norm(grad_scale) if clip else None
        self._update(0, hi, self.t, grad_scale, coef)
        self._update_temperature(self.t, grad_scale)
        if self.after_update is not None and self.state is None:
            self.after_update(0, hi, True)


class GraphedStep:
    """One whole train step — forward, loss, backward, fused Adam — captured once into a hipGraph and replayed with one call.
    Measured on MI355X at B = 256: 5.04 ms per step replayed (single stream) against 4.9-5.0 ms for the eager step with its side
    stream and 5.5 ms for the eager step on one stream — the graph closes the same gaps between short kernels that the side
    stream hides.  The small-batch step is bound by latency-bound kernels (the GRU's 100 sequential steps each way), not by
    launch overhead.  Kept as an option for hosts with slower launch paths.  Requirements: single process (no collective inside the graph), no host-side per-step state
    (dropout seeds)."""

    def __init__(self, eng, opt, softplus: bool, regularization: float, all_timesteps: bool = False, score: Optional[str] = None,
                 negatives=None, negative_groups=None, temperature=None, negative_bank=None):
        temperature = check_temperature(temperature, score_kind(softplus, score))
        # (the trainer refuses use_graph with a bank before it gets here: the keyword exists for direct callers, so that they get the
        # reason instead of a TypeError)
        check_negative_bank_supported(negative_bank, graphed=True)
        if negative_groups is not None:
            raise NotImplementedError("grouped negatives take the group ids of each step's batch from the host, which a captured graph "
                                      "cannot replay")
        if negatives is not None:
            raise NotImplementedError("sampled negatives draw a new set per step from a host-side counter (like dropout's seed), which a "
                                      "captured graph cannot replay")
        if opt.state is None:
            raise ValueError("GraphedStep needs FusedAdam(device_step=True)")
        ctx = eng.ctx
        if getattr(getattr(ctx, "ar", None), "dropout", 0.0) and ctx.ar.training:
            raise NotImplementedError("a step with dropout draws a new host-side seed per step and cannot be replayed from a graph")
        self.eng, self.opt = eng, opt
        shape = getattr(eng, "in_shape", None) or (eng.B, eng.L)
        self.x = torch.zeros(*shape, device=eng.device, dtype=torch.float32)
        args = dict(softplus=softplus, regularization=regularization, all_timesteps=all_timesteps)
        if score is not None:
            args["score"] = score
        if temperature is not None:          # (a launch argument of the captured normalise kernels: nothing on the host per step)
            args["temperature"] = temperature
            eng._norm_scratch()                # (allocated and zeroed here: torch.cuda.graph synchronises the device on entry)
        if isinstance(temperature, DeviceTemperature):
            # device state: the captured kernels read and write tstate, and a scheduled one takes its step from the optimizer's own count
            # on the device (the count starts at opt._t0 where the schedule stands at opt.step_offset)
            eng._norm_dots()
            if temperature.mode == "scheduled":
                if opt.step_offset - opt._t0 < 0:
                    raise ValueError(f"the loaded step count {opt._t0} lies beyond step_offset {opt.step_offset}")
                temperature.bind(opt.state, opt.step_offset - opt._t0)
            elif opt.temperature is not temperature:
                raise ValueError("a learnable DeviceTemperature needs FusedAdam(temperature=...) with the same object")
        # no warm-up run: nothing here initialises lazily on first use except buffers, which the capture allocates from the
        # graph's own pool — and a real step on a dummy batch would move BatchNorm's running statistics
        # captured on ONE stream: a capture with the side-stream forks replays slower (6.4 vs 5.0 ms at B = 256), and the graph
        # itself closes the launch gaps the side stream hides in the eager step
        eng.use_aux = False
        eng._ahead_token = None            # the captured step always rebuilds its operand copies
        opt.skip_flag = eng.nan_flag()     # NaN guard: part of the captured update
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = eng.loss_and_grads(self.x, **args)
            opt.step()
        opt.t -= 1                                        # the capture ran step() once on the host side only

    def __call__(self, batch):
        self.x.copy_(batch, non_blocking=True)
        self.graph.replay()
        self.opt.t += 1
        self.eng.model._raw_updates = getattr(self.eng.model, "_raw_updates", 0) + 1
        return self.out


def smoke_check(device):
    """One tiny train step on the GPU, checked against the CPU oracle (used by __graft_entry__.smoke)."""
    from oracle import cpc_oracle as O
    from .audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
    torch.manual_seed(0)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64] * 5, 'bias': True})
    ar = AudioGRUModel(input_size=64, hidden_size=64)
    model = AudioPredictiveCodingModel(enc, ar, enc_size=64, ar_size=64, visible_steps=10, prediction_steps=4,
                                       compute_dtype="fp32")
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("weight") and "encoder" in name:
                p.mul_(3.0)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(device)
    B, L = 8, 465 + 14 * 160
    x = torch.randn(B, L) * 0.5
    eng = model.engine(B, L)
    out = eng.loss_and_grads(x.to(device), softplus=True, regularization=1.0)
    torch.cuda.synchronize()
    tr = O.OracleTrainer(params, 10, 4, score="softplus", regularization=1.0)
    loss, smax, grads = tr.loss_and_grads(x)
    got = float(out[0])
    assert abs(got - float(loss)) < 1e-3 * abs(float(loss)), (got, float(loss))
    for name, gref in grads.items():
        gdev = model._grad[name].detach().cpu()
        err = (gdev - gref).abs().max().item() / (gref.abs().max().item() + 1e-12)
        assert err < 1e-3, (name, err)
    print(f"smoke ok: loss {got:.6f} (oracle {float(loss):.6f})")
