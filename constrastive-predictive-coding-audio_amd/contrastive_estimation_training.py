"""Drop-in trainer surface: score functions, ContrastiveEstimationTrainer, DeterministicSampler, grad_mean_var.

Mirrors the reference's ``contrastive_estimation_training.py`` (score functions :12-33, trainer :36-269,
DeterministicSampler :363-382, grad_mean_var :385-391).  ``train`` has two routes:

* fused (the hot path): AudioEncoder + AudioGRUModel model, softplus/linear score (either ``score_over_all_timesteps``
  setting), Adam; the difference score and NormalizedScoreFunction with Adam take it too (``_engine_difference``,
  ``_engine_normalized``), except under global negatives.  Forward, InfoNCE loss, analytic backward and the Adam update all run as
  HIP kernels (engine.CPCEngine); with torch.distributed initialised, one process per GPU, the flat gradient buffer is
  all-reduced over RCCL before the update (per-GPU in-batch negatives).
* generic: any other score function or optimizer: the model forward and backward run on the HIP path through the autograd
  bridge, the score function is the caller's, and the loss (:106-122, :141) and its gradient come from the same loss kernels
  (``_InfoNCE``, whatever the candidate selection: in-batch, sampled or grouped).  ``validate`` takes its per-step losses / accuracies from ``cpc_nce_eval`` on both routes.
"""
from __future__ import annotations

import collections
import ctypes
import itertools
import math
import random
import types

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim
import torch.utils.data

from .audio_model import *          # noqa: F401,F403  (the reference re-exports the model names from here)
from .audio_dataset import FileBatchSampler
from . import switches
from .sampled_negatives import (check_negatives, empty_negative_sets, file_group_ids, group_mode,        # noqa: F401
                                grouped_negative_mask, sampled_negative_mask)                                        # (public: the host restatements)
from .engine import LRSchedule          # noqa: F401  (public: trainer.lr_schedule takes one)
from .engine import DeviceTemperature, TemperatureSchedule          # noqa: F401  (public: NormalizedScoreFunction(schedule=...))


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only (libcpc_hip.so; there is no CPU fallback): move the tensors to the device")


class InputAhead:
    """The preprocessing module of batch i + 1 (CQT GEMMs + the pointwise scalogram kernel: 1.3 of the 12 ms of a BASELINE configs[2]
    step) issued on the side stream while step i runs, instead of on the main stream in front of step i + 1's encoder.  The reference
    preprocesses inside the step (:99-103); the scalogram does not depend on the parameters, so the result is the same tensor, one
    step early: ``submit(batch)`` queues it behind everything the main stream has been given so far (so that the batch itself is
    complete) and returns at once, ``take()`` makes the main stream wait for the oldest submitted batch and returns
    (batch, model input).  Buffers: the module allocates a fresh output per call; record_stream keeps the caching allocator from
    handing a block to the other stream while it is still being read."""

    def __init__(self, fn, device):
        from .contexts import side_stream
        self.fn, self.device = fn, torch.device(device)
        self.aux = side_stream(self.device)
        self.pending = []

    def submit(self, batch):
        main = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self.aux):
            self.aux.wait_event(ready)
            x = self.fn(batch)
            done = torch.cuda.Event()
            done.record(self.aux)
        batch.record_stream(self.aux)
        self.pending.append((batch, x, done))

    def take(self):
        batch, x, done = self.pending.pop(0)
        main = torch.cuda.current_stream(self.device)
        main.wait_event(done)
        if isinstance(x, torch.Tensor):
            x.record_stream(main)
        return batch, x


def _with_next(it):
    """(item, next item or None) pairs of an iterator."""
    it = iter(it)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)
        yield cur, nxt
        cur = nxt


class _ScoreContraction(torch.autograd.Function):
    """scores[b, k, b', k'] = sum_e predicted_z[b, k, e] * targets[b', e, k'] as ONE cpc_gemm_nt call (f32, exact-f32 MFMA) over
    the (B K) x E operands; the gradients are the two matching contractions (cpc_gemm_nt / cpc_gemm_tn)."""

    @staticmethod
    def forward(ctx, predicted_z, targets):
        from . import _hip
        _need_gpu(predicted_z, "the score contraction")
        B, K, E = predicted_z.shape
        if tuple(targets.shape) != (B, E, K) or E % 4 or (B * K) % 4:
            raise ValueError("score contraction: expected predicted_z (B, K, E) and targets (B, E, K) with E and B*K multiples of 4")
        R = B * K
        A = predicted_z.detach().reshape(R, E).float().contiguous()
        Tt = targets.detach().permute(0, 2, 1).reshape(R, E).float().contiguous()
        S = torch.empty(R, R, device=A.device, dtype=torch.float32)
        _hip.gemm_nt(_hip.ptr(A), _hip.ptr(Tt), _hip.ptr(S), R, R, E, E, E, R, _hip.F32)
        ctx.save_for_backward(A, Tt)
        ctx.shape = (B, K, E)
        return S.view(B, K, B, K)

    @staticmethod
    def backward(ctx, d_scores):
        from . import _hip
        A, Tt = ctx.saved_tensors
        B, K, E = ctx.shape
        R = B * K
        dS = d_scores.reshape(R, R).float().contiguous()
        dA = torch.empty(R, E, device=dS.device, dtype=torch.float32)
        dT = torch.empty(R, E, device=dS.device, dtype=torch.float32)
        TtT = Tt.t().contiguous()                                                        # [E][R]
        _hip.gemm_nt(_hip.ptr(dS), _hip.ptr(TtT), _hip.ptr(dA), R, E, R, R, R, E, _hip.F32)          # dA = dS Tt
        _hip.gemm_tn(_hip.ptr(dS), _hip.ptr(A), _hip.ptr(dT), R, R, E, R, E, E, _hip.F32, flags=_hip.GEMM_OUT_F32)   # dT = dS^T A
        return dA.view(B, K, E), dT.view(B, K, E).permute(0, 2, 1)


def linear_score_function(predicted_z, targets):
    """scores[b, k, b', k'] = sum_e predicted_z[b,k,e] * targets[b',e,k']  (reference :19-22)."""
    return _ScoreContraction.apply(predicted_z, targets)


def softplus_score_function(predicted_z, targets):
    """softplus of the linear scores (reference :12-16)."""
    return F.softplus(_ScoreContraction.apply(predicted_z, targets))


class _DifferenceScores(torch.autograd.Function):
    """scores[b, k, b', k'] = 1 / sum_e (predicted_z[b, k, e] - targets[b', e, k'])^2 as ONE cpc_diff_scores launch over the (B K) x E
    operands (f32, differences formed first, as the reference does); memory O((B K)^2): the scores and their transpose are kept for
    the backward, which is cpc_diff_scores_bwd (G = 2 g s^2 and its row / column sums), the two contractions of the linear score's
    gradient with G and the rank-1 terms (cpc_diff_scores_rank1)."""

    @staticmethod
    def forward(ctx, predicted_z, targets):
        from . import _hip
        _need_gpu(predicted_z, "the difference score function")
        B, K, E = predicted_z.shape
        if tuple(targets.shape) != (B, E, K) or E % 4 or (B * K) % 4:
            raise ValueError("difference scores: expected predicted_z (B, K, E) and targets (B, E, K) with E and B*K multiples of 4")
        R = B * K
        A = predicted_z.detach().reshape(R, E).float().contiguous()
        Tt = targets.detach().permute(0, 2, 1).reshape(R, E).float().contiguous()
        S = torch.empty(R, R, device=A.device, dtype=torch.float32)
        ST = torch.empty(R, R, device=A.device, dtype=torch.float32)
        L = ctypes.c_longlong
        _hip.call("cpc_diff_scores", _hip.ptr(A), _hip.ptr(Tt), _hip.ptr(S), _hip.ptr(ST), R, R, E, L(E), L(E), 0, L(0), L(0), L(0), L(0),
                  1, R, _hip.F32, work=2.0 * R * R * E)
        ctx.save_for_backward(A, Tt, S, ST)
        ctx.shape = (B, K, E)
        return S.view(B, K, B, K)

    @staticmethod
    def backward(ctx, d_scores):
        from . import _hip
        A, Tt, S, ST = ctx.saved_tensors
        B, K, E = ctx.shape
        R = B * K
        G = torch.empty(R, R, device=S.device, dtype=torch.float32)           # overwritten in place below: never autograd's own buffer
        G.copy_(d_scores.reshape(R, R))
        GT = G.t().contiguous()
        sums = torch.empty(2, R, device=S.device, dtype=torch.float32)
        L, P = ctypes.c_longlong, _hip.ptr
        _hip.call("cpc_diff_scores_bwd", P(G), P(S), P(sums[0]), P(GT), P(ST), P(sums[1]), R, R, R, L(0), 1, _hip.F32)
        dA = torch.empty(R, E, device=S.device, dtype=torch.float32)
        dT = torch.empty(R, E, device=S.device, dtype=torch.float32)
        TtT = Tt.t().contiguous()                                                        # [E][R]
        _hip.gemm_nt(P(G), P(TtT), P(dA), R, E, R, R, R, E, _hip.F32)                   # dA = G Tt
        _hip.gemm_tn(P(G), P(A), P(dT), R, R, E, R, E, E, _hip.F32, flags=_hip.GEMM_OUT_F32)   # dT = G^T A
        _hip.call("cpc_diff_scores_rank1", P(sums[0]), P(A), P(dA), R, E, 0, L(0), L(E), _hip.F32)    # - rowsum(G) * predicted_z
        _hip.call("cpc_diff_scores_rank1", P(sums[1]), P(Tt), P(dT), R, E, 0, L(0), L(E), _hip.F32)   # - colsum(G) * targets
        return dA.view(B, K, E), dT.view(B, K, E).permute(0, 2, 1)


def difference_score_function(predicted_z, targets):
    """1 / squared distance between every prediction and every target (reference :25-33), as HIP kernels (_DifferenceScores):
    O((B K)^2) memory instead of the reference broadcast's O(B^2 K^2 E)."""
    return _DifferenceScores.apply(predicted_z, targets)


class _NormalizeRows(torch.autograd.Function):
    """rows / max(|row|, eps) * scale over the last axis of an (R, E) f32 matrix: cpc_norm_rows, and cpc_norm_rows_bwd in the backward
    (the kernels of the engine route, so that both routes share one arithmetic)."""

    @staticmethod
    def forward(ctx, rows, scale):
        from . import _hip
        from .engine import NORM_EPS
        R, E = rows.shape
        X = rows.detach().float().contiguous()
        Y = torch.empty_like(X)
        inv = torch.empty(R, device=X.device, dtype=torch.float32)
        L, F_ = ctypes.c_longlong, ctypes.c_float
        _hip.call("cpc_norm_rows", _hip.ptr(X), _hip.ptr(Y), _hip.ptr(inv), R, E, 0, L(0), L(E), F_(scale), F_(NORM_EPS), _hip.F32)
        ctx.save_for_backward(Y, inv)
        ctx.scale = scale
        return Y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        from . import _hip
        from .engine import NORM_EPS
        Y, inv = ctx.saved_tensors
        R, E = Y.shape
        G = torch.empty_like(Y)              # overwritten in place below: never autograd's own buffer
        G.copy_(dY)
        L, F_ = ctypes.c_longlong, ctypes.c_float
        _hip.call("cpc_norm_rows_bwd", _hip.ptr(Y), _hip.ptr(inv), _hip.ptr(G), R, E, 0, L(0), L(E), F_(ctx.scale), F_(NORM_EPS), _hip.F32)
        return G, None


class NormalizedScoreFunction:
    """Cosine similarity over a temperature (not in the reference; wav2vec 2.0 / SimCLR / CLIP-style scores):
    scores[b, k, b', k'] = <predicted_z[b, k] / max(|.|, 1e-8), targets[b', :, k'] / max(|.|, 1e-8)> / temperature, i.e.
    linear_score_function(F.normalize(predicted_z, dim=2) / temperature, F.normalize(targets, dim=1)).  Bounded by 1 / temperature
    whatever the norms of the encodings.  As ``score_function=`` of ContrastiveEstimationTrainer with Adam the whole step runs on the
    engine (score kind "normalized"); called on tensors it is an autograd function over the same kernels (f32: cpc_norm_rows, the score
    contraction, cpc_norm_rows_bwd).  The temperature (finite and > 0) is a constant of the run, or
      learnable=True: a parameter of the run, s = log(1 / temperature), trained by Adam beside the weights at
        lr * schedule factor * ``temperature_lr_scale`` (the run's betas and eps, no decay) and kept inside
        [min_temperature, max_temperature]; ``temperature`` is where it starts.  Engine route, one process;
      schedule=TemperatureSchedule(...): step s of the run scores at schedule.value(s) (``temperature`` is then ignored).
    In both cases the trainer keeps the value in device memory (engine.DeviceTemperature; DESIGN.md, "Learnable and scheduled
    temperature"); called on tensors, the function uses the value as it stands as a constant."""

    def __init__(self, temperature=0.1, learnable=False, min_temperature=0.01, max_temperature=1.0, temperature_lr_scale=1.0,
                 schedule=None):
        from .engine import check_temperature, check_temperature_bounds, check_temperature_range
        if not isinstance(learnable, bool):
            raise ValueError(f"learnable must be True or False, got {learnable!r}")
        if schedule is not None and not isinstance(schedule, TemperatureSchedule):
            raise ValueError(f"schedule must be None or a TemperatureSchedule, got {schedule!r}")
        if learnable and schedule is not None:
            raise ValueError("a temperature is either learnable or scheduled, not both")
        self.learnable, self.schedule = learnable, schedule
        if schedule is not None:
            temperature = schedule.value(0)
        # (the pair is checked in every mode, so that a bad one does not wait for learnable=True to be noticed; only a learnable
        # temperature has to start inside it)
        self.min_temperature, self.max_temperature = check_temperature_range(min_temperature, max_temperature)
        self.temperature = check_temperature(temperature)
        if learnable:
            check_temperature_bounds(self.temperature, self.min_temperature, self.max_temperature)
        try:
            self.temperature_lr_scale = float(temperature_lr_scale)
        except (TypeError, ValueError):
            raise ValueError(f"temperature_lr_scale must be a finite number >= 0, got {temperature_lr_scale!r}") from None
        if isinstance(temperature_lr_scale, bool) or not math.isfinite(self.temperature_lr_scale) or self.temperature_lr_scale < 0.0:
            raise ValueError(f"temperature_lr_scale must be a finite number >= 0, got {temperature_lr_scale!r}")
        self.device_temperature = None          # the trainer's engine.DeviceTemperature, once a run has made one

    def make_device_temperature(self, device):
        """The engine.DeviceTemperature of this configuration on ``device`` (None for a constant)."""
        if self.learnable:
            return DeviceTemperature(self.temperature, "learnable", self.min_temperature, self.max_temperature,
                                     self.temperature_lr_scale, device=device)
        if self.schedule is not None:
            return DeviceTemperature(mode="scheduled", schedule=self.schedule, device=device)
        return None

    def current_temperature(self):
        """The value as it stands: the device's (one synchronous read) where a run keeps it there, else the constant."""
        if self.device_temperature is not None:
            return self.device_temperature.value()
        return self.temperature

    def __repr__(self):
        extra = ""
        if self.learnable:
            extra = (f", learnable=True, min_temperature={self.min_temperature!r}, max_temperature={self.max_temperature!r}, "
                     f"temperature_lr_scale={self.temperature_lr_scale!r}")
        elif self.schedule is not None:
            extra = f", schedule={self.schedule!r}"
        return f"NormalizedScoreFunction(temperature={self.temperature!r}{extra})"

    def __call__(self, predicted_z, targets):
        _need_gpu(predicted_z, "the normalized score function")
        B, K, E = predicted_z.shape
        if tuple(targets.shape) != (B, E, K):
            raise ValueError("normalized scores: expected predicted_z (B, K, E) and targets (B, E, K)")
        pn = _NormalizeRows.apply(predicted_z.reshape(B * K, E), 1.0 / self.current_temperature()).view(B, K, E)
        tn = _NormalizeRows.apply(targets.permute(0, 2, 1).reshape(B * K, E), 1.0).view(B, K, E).permute(0, 2, 1)
        return _ScoreContraction.apply(pn, tn)


def _score_layout(scores4, all_timesteps):
    """The 4-D score tensor of ANY score function in the layout the loss kernels read: the (B K) x (B K) matrix, or in the default
    branch its K equal-step blocks S[k][b][b'] = scores[b, k, b', k] with rows padded to a multiple of 8 floats."""
    B, K = scores4.shape[0], scores4.shape[1]
    if all_timesteps:
        return scores4.reshape(B * K, B * K).float().contiguous(), B * K
    ld = -(-B // 8) * 8
    S = torch.zeros(K, B, ld, device=scores4.device, dtype=torch.float32)
    S[:, :, :B] = torch.diagonal(scores4, dim1=1, dim2=3).permute(2, 0, 1)
    return S, ld


def _step_block_grads(dS, B, K, d_loss):
    """The default branch's d loss / d scores as autograd wants it: the K equal-step blocks dS[k][b][b'] (rows padded, as
    _score_layout lays them out) times d_loss on the [b, k, b', k] diagonal of a (B, K, B, K) tensor of zeros."""
    d = torch.zeros(B, K, B, K, device=dS.device, dtype=torch.float32)
    torch.diagonal(d, dim1=1, dim2=3).copy_(dS[:, :, :B].permute(1, 2, 0) * d_loss)
    return d


class _InfoNCE(torch.autograd.Function):
    """Loss of the train step (reference :108-122, :141) from a 4-D score tensor, through the same kernels as the fused route
    (the score function already applied): returns (loss incl. regulariser, max score, NaN indicator of the loss before the
    regulariser); the backward hands d loss / d scores back to autograd.  selection, shaped like engine.CPCEngine._nce_loss's:
      None: every other batch item is a candidate (cpc_nce_loss; cpc_nce_loss_all with all_timesteps);
      ("sampled", n_neg, seed, draw): n_neg seeded negatives per target (cpc_nce_loss_sampled; DESIGN.md, "Sampled negatives");
      ("grouped", groups, mode, n_neg, seed, draw): candidates by group id (cpc_nce_loss_grouped; DESIGN.md, "Grouped negatives");
        groups: int32 device tensor [B]; mode 0 = same, 1 = other; n_neg 0 = every eligible row.
    A selection is defined for the default branch only."""

    @staticmethod
    def forward(ctx, scores4, all_timesteps, regularization, selection=None):
        import ctypes as C
        from . import _hip
        kind = selection[0] if selection is not None else None
        assert kind is None or not all_timesteps, "a candidate selection exists for score_over_all_timesteps=False only"
        # every entry point cpc_nce_loss<suffix> has its cpc_nce<suffix>_workspace_floats
        suffix = "_all" if all_timesteps else f"_{kind}" if kind else ""
        _need_gpu(scores4, "the InfoNCE loss" + (f" over {kind} negatives" if kind else ""))
        B, K = scores4.shape[0], scores4.shape[1]
        P, u64 = _hip.ptr, lambda v: C.c_ulonglong(int(v) & (2 ** 64 - 1))
        pick = ()          # the entry point's arguments between the regulariser and the dtype
        if kind == "sampled":
            n_neg, seed, draw = selection[1:]
            pick = (check_negatives(B, n_neg), u64(seed), u64(draw))
        S, ld = _score_layout(scores4.detach(), all_timesteps)
        dev, f32 = S.device, torch.float32
        if kind == "grouped":
            groups, mode, n_neg, seed, draw = selection[1:]
            if groups.dtype != torch.int32 or tuple(groups.shape) != (B,) or groups.device != dev:
                raise ValueError(f"groups must be an int32 tensor of shape [{B}] on {dev}")
            groups = groups.contiguous()
            pick = (P(groups), int(mode), int(n_neg), u64(seed), u64(draw))
        out = torch.zeros(8, device=dev, dtype=f32)
        dS, dST = torch.zeros_like(S), torch.zeros_like(S)
        ws = torch.empty(int(getattr(_hip.lib(), f"cpc_nce{suffix}_workspace_floats")(B, K)), device=dev, dtype=f32)
        ST = S.t().contiguous() if all_timesteps else None          # cpc_nce_loss_all also reads the transposed scores
        scores = (P(S), P(ST)) if all_timesteps else (P(S),)
        _hip.call("cpc_nce_loss" + suffix, *scores, P(dS), P(dST), P(out), P(ws), B, K, ld, 0, C.c_float(regularization), *pick, _hip.F32)
        ctx.save_for_backward(dS)
        ctx.meta = (B, K, bool(all_timesteps), scores4.dtype)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, d_loss, _d_out):
        (dS,) = ctx.saved_tensors
        B, K, all_t, dtype = ctx.meta
        d = dS.view(B, K, B, K) * d_loss if all_t else _step_block_grads(dS, B, K, d_loss)
        return d.to(dtype), None, None, None


class _RecordingSampler:
    """Hands out a batch sampler's index lists and appends each to ``fifo`` first: whoever consumes the batches in order (a DataLoader
    reads its sampler ahead of the batch it yields) finds the indices of the batch in hand at the front."""

    def __init__(self, inner, fifo):
        self.inner, self.fifo = inner, fifo

    def __iter__(self):
        for idx in self.inner:
            idx = [int(i) for i in idx]
            self.fifo.append(idx)
            yield idx

    def __len__(self):
        return len(self.inner)


_NEGATIVE_GROUP_MODES = {"same_file": "same", "other_files": "other"}


def _ring_depth(trainer):
    """Slots of the readback ring and of the snapshot ring: the steps that can be in flight before the host has read the oldest."""
    return trainer.host_sync_interval + trainer.host_sync_lag + 2


class _StepReadback:
    """A run's per-step values on their way to the logger: ``push`` queues a step's row right behind its launches, ``flush`` reads rows
    back in order, feeds the logger's meters and sets the trainer's last_grad_norm / last_temperature.  Row layout, the one both
    sides use: the loss kernel's result cell (cpc_nce_loss: out[0], out[1], out[5]), with clipping the norm before clipping and the
    coefficient applied behind it (FusedAdam.clip_state[0:2] on the fused routes), with a device temperature the value as the step
    left it (tstate[5]) behind those."""
    LOSS, MAX_SCORE, NAN = 0, 1, 5
    GRAD_NORM, CLIP_COEF = 6, 7

    def __init__(self, trainer, optimizer, clip, fused, on_gpu, device_temp, temp_route):
        self.trainer, self.optimizer = trainer, optimizer
        self.clip, self.fused, self.on_gpu = clip, fused, on_gpu
        self.device_temp, self.temp_route = device_temp, temp_route
        self.base_width = (self.CLIP_COEF if clip else self.NAN) + 1
        self.TEMPERATURE = self.base_width if device_temp is not None else None
        self.width = self.base_width + (1 if device_temp is not None else 0)
        self.ring, self.ring_pos = [], 0          # pinned host buffers, handed out in turn
        self.pending = []                         # (step, row, event, lr, host temperature) not yet read back
        self.bad_grad_norm = False                # the NaN step flush() returned had a finite loss: the gradient was the cause

    def push(self, step, vals):
        """Queues a step's (loss, max score) for the logger.  On the GPU they travel to a pinned host buffer right behind the
        step's own kernels and an event marks their arrival: reading them later does not wait for LATER steps' work, which a
        synchronous read of a device tensor — queued behind everything launched since — would."""
        tr = self.trainer
        host_tau = tr.score_function.temperature if self.temp_route == "host" else None
        if not self.on_gpu:
            self.pending.append((step, vals.detach()[:self.width].clone(), None, tr.last_lr, host_tau))
            return
        while len(self.ring) < _ring_depth(tr):          # (host_sync_interval / host_sync_lag raised while training)
            self.ring.append(torch.empty(self.width, dtype=torch.float32, pin_memory=True))
        buf = self.ring[self.ring_pos % len(self.ring)]
        self.ring_pos += 1
        if self.clip and self.fused:          # the engine's result cell and FusedAdam.clip_state: two copies, one event
            buf[:self.GRAD_NORM].copy_(vals.detach()[:self.GRAD_NORM].float(), non_blocking=True)
            buf[self.GRAD_NORM:self.base_width].copy_(self.optimizer.clip_state[:2], non_blocking=True)
        else:
            buf[:self.base_width].copy_(vals.detach()[:self.base_width].float(), non_blocking=True)
        if self.device_temp is not None:          # the same buffer and event: no further wait
            buf[self.TEMPERATURE:].copy_(self.device_temp.tstate[5:6], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((step, buf, ev, tr.last_lr, host_tau))          # (the host knows the step's learning rate: it rides along)

    def flush(self, keep=0):
        """Reads back all pending steps but the ``keep`` most recent ones (in order); returns the step of a NaN loss."""
        tr, logger, pending = self.trainer, self.trainer.logger, self.pending
        n = max(len(pending) - keep, 0)
        for step, vals, ev, lr_v, host_tau in pending[:n]:
            if ev is not None:
                ev.synchronize()
            row = vals.tolist()
            loss_v, score_v, nan_v = float(row[self.LOSS]), float(row[self.MAX_SCORE]), float(row[self.NAN])
            if self.clip:
                tr.last_grad_norm = float(row[self.GRAD_NORM])
            tau_v = float(row[self.TEMPERATURE]) if self.device_temp is not None else host_tau
            # reference order (:124-133 before :164-169): a NaN loss ends the run before anything is logged for that step
            if nan_v != 0.0 or math.isnan(loss_v):
                # (the indicator is also what cpc_grad_norm raises: a finite loss under it means the gradient was the cause)
                self.bad_grad_norm = self.clip and not math.isnan(loss_v) and not math.isfinite(tr.last_grad_norm)
                pending.clear()
                return step
            if logger is not None:
                logger.loss_meter.update(loss_v)
                logger.score_meter.update(score_v)
                if self.clip and hasattr(logger, "grad_norm_meter"):
                    logger.grad_norm_meter.update(tr.last_grad_norm)
                if hasattr(logger, "lr_meter"):
                    logger.lr_meter.update(lr_v)
                if tau_v is not None and hasattr(logger, "temperature_meter"):
                    logger.temperature_meter.update(tau_v)
                logger.log(step)
            elif tr.verbose:
                print("loss at step step " + str(step) + ":", loss_v)
            if tau_v is not None:
                tr.last_temperature = tau_v
        del pending[:n]
        return None


class _NanRollback:
    """The host learns of a NaN loss host_sync_lag steps late; the steps launched meanwhile change nothing on the device that Adam
    owns (every stateful launch — the update, the average, the trust table, the learnable temperature's step — is skipped there
    under the sticky flag; DESIGN.md, "What the NaN guard holds still"), but their forward passes move the BatchNorm running
    statistics, a scheduled temperature's tick overwrites its device value, and the host-side counts advance.  All of that is put
    back to where the reference leaves it (it returns inside the NaN step, after that step's forward pass, :124-133): at the START
    of every step the buffers are snapshotted (one multi-tensor copy per dtype), a scheduled DeviceTemperature's tstate is copied
    (8 floats), and the host values are noted — the optimizer's t and lr, the trainer's last_lr, the temperature's step.  restore()
    takes the statistics of step `nan + 1` and everything else of step `nan`.  What cannot be taken back: the sampler has handed out
    the later batches; the negative bank is emptied instead (_nan_return).  The generic route reads every step's loss at once, before
    anything is updated: it snapshots no buffer and notes only last_lr, which train() has already set to the NaN step's rate."""

    def __init__(self, trainer, optimizer, fused, device_temp=None):
        self.trainer, self.optimizer, self.fused = trainer, optimizer, fused
        # (grouped by dtype, copied one dtype at a time: a mixed list — float32 statistics and int64 counters — takes _foreach_copy_'s
        # per-tensor route, 40 device-to-device copies and 0.13 ms per configs[2] step; a uniform list is one multi-tensor kernel)
        by_dtype = {}
        for n_, b in trainer.model.named_buffers():
            if "running_" in n_ or n_.endswith("num_batches_tracked"):
                by_dtype.setdefault(str(b.dtype), []).append(b)
        self.bufs = [by_dtype[k] for k in sorted(by_dtype)]          # BatchNorm's buffers, one list per dtype
        self.ring, self.ring_pos, self.snaps = [], 0, {}          # snaps: step -> (ring slot or None, the optimizer's t)
        if fused and self.bufs:          # the ring exists before the loop: no allocation inside the hot loop; models without BatchNorm keep none
            self.ring = [self._slot() for _ in range(_ring_depth(trainer))]
        # host: step -> what else the host held at the start of that step; temp_ring: tstate copies of a scheduled temperature (its
        # tick is no update: it is not skipped under the flag, so the steps behind a NaN loss leave their own values there)
        self.temp, self.host = device_temp, {}
        self.temp_ring, self.temp_pos = [], 0

    def _slot(self):
        return [[torch.empty_like(b) for b in group] for group in self.bufs]

    @staticmethod
    def _copy(dst, src):
        for d, s in zip(dst, src):
            torch._foreach_copy_(d, s)

    def snapshot(self, step):
        depth = _ring_depth(self.trainer)
        if not self.fused:          # nothing runs behind a NaN step there; last_lr is still the rate of a step that was not applied
            self.host = {step: {"lr": None, "last_lr": getattr(self.trainer, "last_lr", None), "temp_step": None, "tstate": None}}
            return
        dst = None
        if self.bufs:
            while len(self.ring) < depth:          # (host_sync_interval / host_sync_lag raised while training)
                self.ring.append(self._slot())
            dst = self.ring[self.ring_pos % depth]
            self.ring_pos += 1
            self._copy(dst, self.bufs)
        self.snaps[step] = (dst, getattr(self.optimizer, "t", None))
        temp, tslot = self.temp, None
        if temp is not None and temp.mode == "scheduled":
            while len(self.temp_ring) < depth:
                self.temp_ring.append(torch.empty_like(temp.tstate))
            tslot = self.temp_ring[self.temp_pos % depth]
            self.temp_pos += 1
            tslot.copy_(temp.tstate)
        self.host[step] = {"lr": getattr(self.optimizer, "lr", None), "last_lr": getattr(self.trainer, "last_lr", None),
                           "temp_step": None if temp is None else temp.step, "tstate": tslot}
        for old_step in [k for k in self.snaps if k < step - depth + 1]:
            del self.snaps[old_step]
            self.host.pop(old_step, None)

    def restore(self, step):
        """After a NaN loss at ``step``: the statistics of the start of step + 1; the optimizer's count and rate, the trainer's
        last_lr and the temperature's step (a scheduled one's device value too) of the start of ``step``."""
        later = self.snaps.get(step + 1)
        if later is not None and later[0] is not None:          # statistics as they were after the NaN step's own forward pass
            self._copy(self.bufs, later[0])
        here = self.snaps.get(step)
        if here is not None and here[1] is not None and hasattr(self.optimizer, "t"):
            self.optimizer.t = here[1]                          # no update has happened since the start of the NaN step
        host = self.host.get(step)
        if host is None:
            return
        if host["lr"] is not None and hasattr(self.optimizer, "lr"):
            self.optimizer.lr = host["lr"]                      # (state_dict() exports it as the rate of the latest step)
        if hasattr(self.trainer, "last_lr"):
            self.trainer.last_lr = host["last_lr"]
        if self.temp is not None:
            self.temp.step = host["temp_step"]
            if host["tstate"] is not None:
                self.temp.tstate.copy_(host["tstate"])


class ContrastiveEstimationTrainer:
    def __init__(self, model, dataset, logger=None, device=None,
                 regularization=1., validation_set=None, test_task_set=None, prediction_noise=0.01,
                 optimizer=torch.optim.Adam,
                 file_batch_size=1,
                 score_over_all_timesteps=False,
                 score_function=softplus_score_function,
                 wasserstein_gradient_penalty=False,
                 gradient_penalty_factor=10.,
                 preprocessing=None,
                 ar_size=256,
                 prediction_steps=16):
        self.model = model
        self.ar_size = ar_size
        self.prediction_steps = prediction_steps
        self.dataset = dataset
        self.logger = logger
        self.device = device
        self.regularization = regularization
        self.validation_set = validation_set
        self.test_task_set = test_task_set
        self.training_step = 0
        self.print_out_scores = False
        self.prediction_noise = prediction_noise
        self.optimizer = optimizer
        self.file_batch_size = file_batch_size
        self.score_over_all_timesteps = score_over_all_timesteps
        self.score_function = score_function
        self.wasserstein_gradient_penalty = wasserstein_gradient_penalty
        self.gradient_penalty_factor = gradient_penalty_factor
        self.preprocessing = preprocessing
        # Not in the reference: how often loss / max-score are read back to the host (the reference reads them every
        # step, :124 and :165-166).  Values are delivered to the logger in order, at most this many steps late.
        self.host_sync_interval = 1
        self.host_sync_lag = 1          # steps the loss readback trails the launches by (0: read every step's loss at once)
        # Not in the reference: replay the whole step from a captured hipGraph (single process, fused path, no preprocessing
        # module, no dropout).  Measured neutral on MI355X (launches are already hidden); off by default.
        self.use_graph = False
        # Not in the reference's signature: under torch.distributed take the InfoNCE loss over the batches of ALL ranks — what
        # the reference's nn.DataParallel wrap computes — instead of per-GPU negatives (engine.GlobalNegatives).
        self.global_negatives = False
        # Not in the reference's signature: contrast every target against num_negatives seeded negatives of the batch instead of all
        # batch_size - 1 (None: the reference's in-batch loss).  Step i draws the sets of (negative_seed, draw = i): a run continued
        # with continue_training_at_step resumes the same stream, and sampled_negative_mask(...) restates any step's sets on the host.
        # Default loss branch only; validate() stays in-batch, as the reference measures accuracy.
        self.num_negatives = None
        self.negative_seed = 0
        # Not in the reference's signature: restrict every target's negatives by a group id per example ("Grouped
        # negatives").  negative_groups: None (every other batch item is a candidate), "same_file" (only items with the target's id)
        # or "other_files" (only items with another id).  negative_group_ids: None — the id of an example is the index of its file in
        # dataset.get_example_count_per_file() — or a 1-D integer sequence of len(dataset), speaker ids for instance.  Composes with
        # num_negatives: a target then keeps min(num_negatives, eligible) seeded rows of its eligible set.  A target without eligible
        # rows contributes 0 to the loss; last_empty_negative_sets holds how many items of the latest step's batch had none.
        # Default loss branch only; validate() stays in-batch.
        self.negative_groups = None
        self.negative_group_ids = None
        self.last_empty_negative_sets = None
        # Not in the reference's signature: a cross-batch memory of negatives ("Negative bank").  negative_bank: None, or
        # M in 1 .. 63 — every target is also contrasted against the predictions of the M latest steps, kept as constants
        # (engine.NegativeBank; the candidate count grows from B to (M + 1) B at the cost of one skinny score GEMM and one longer
        # contraction per step, no encoder work).  The first step after an empty bank is the in-batch step bit for bit;
        # negative_bank_filled tells how many earlier steps the bank holds, reset_negative_bank() empties it.  The trainer owns the
        # bank across train() calls with the same batch shape.  It is not checkpointed: a resumed run starts with an empty bank.  Engine
        # route only (Adam with linear_score_function, softplus_score_function or a NormalizedScoreFunction of constant temperature),
        # default loss branch, no use_graph, not combined with num_negatives / negative_groups / global_negatives / the gradient
        # penalty; validate() stays in-batch.  Under data parallelism every rank keeps a bank of its own shard (permitted, unverified).
        self.negative_bank = None
        self._bank = None
        # Not in the reference's signature: clip the gradient to this global L2 norm before the update, as
        # torch.nn.utils.clip_grad_norm_ in front of optimizer.step() (None: no clipping, the reference's step).  On the fused routes
        # the norm and the clipped Adam are HIP kernels (engine.FusedAdam(max_grad_norm=...)); under data parallelism it is the norm of
        # the gradient the update applies, after the reduction over the ranks.  The norm BEFORE clipping of the latest step read back
        # is kept in last_grad_norm and goes to logger.grad_norm_meter where the logger has one; a norm that is not finite ends the run
        # like a NaN loss.
        self.max_grad_norm = None
        self.last_grad_norm = None
        # Not in the reference's signature (it runs Adam at one constant lr, without decay, from zero moments in every train() call):
        # weight_decay: torch.optim.AdamW's decoupled decay, p <- p (1 - lr_step * weight_decay) in front of Adam's update, on the
        #   parameters weight_decay_filter(name, parameter) selects (None: parameter.dim() >= 2 — conv, GRU, linear and attention
        #   matrices, not biases or BatchNorm's weight and bias);
        # lr_schedule: an LRSchedule; step s runs at lr * lr_schedule.factor(s) with s = training_step, so that
        #   continue_training_at_step resumes the schedule (None: the reference's constant lr);
        # optimizer_state: a state dict in torch.optim.Adam's format, loaded into the optimizer at the start of the next train() and
        #   then set back to None (trainer.last_optimizer.state_dict() takes one out of a fused run);
        # last_lr: the learning rate of the latest step launched; every step's rate goes to logger.lr_meter where the logger has one.
        # On the fused routes decay and schedule are engine.FusedAdam's (cpc_adamw; cpc_adamw_dev under use_graph).
        self.weight_decay = 0.0
        self.weight_decay_filter = None
        self.lr_schedule = None
        self.optimizer_state = None
        self.last_lr = None
        # Not in the reference's signature: LAMB's layer-wise trust ratio ("LAMB trust ratios").
        # trust_ratio: True scales the update of every parameter weight_decay_filter selects by ||p|| / ||u||, u = Adam's direction
        #   + weight_decay * p (the decay then is part of the direction, not AdamW's multiply in front); the parameters the filter
        #   leaves out keep Adam's update.  One filter chooses decay and ratio;
        # trust_clip: None, or the largest ratio applied (finite and > 0).
        # On the fused routes it is engine.FusedAdam's (cpc_lamb; trainer.last_optimizer.trust_ratios() reads the latest step's norms
        # and ratios), on the generic route engine.TorchLamb in the place of torch.optim.Adam.  Not with use_graph (no captured LAMB
        # step) and not with an optimizer other than torch.optim.Adam (a foreign optimizer's direction is not ours to rescale).
        self.trust_ratio = False
        self.trust_clip = None
        # Not in the reference's signature: an exponential moving average (EMA) of the weights ("EMA of the weights").
        # ema_decay: None, or d in [0, 1): behind every update, shadow <- shadow + (p - shadow) * (1 - d);
        # ema_warmup: True uses min(d, (1 + t) / (10 + t)) at the optimizer's update number t, so that a short run's average is not
        #   held at its start (t counts from the start of a train() call, or from the step count of a loaded optimizer_state).
        # train() builds a new optimizer on every call, so the trainer owns the shadow: the first train() with a decay starts it as a copy
        # of the parameters, later calls go on with it, reset_ema() drops it, and an optimizer_state that carries "ema" replaces it.
        # validate(use_ema=True) / calc_test_task_data(use_ema=True) evaluate the averaged weights, ema_state_dict() exports them.
        # BatchNorm's running statistics are buffers and are not averaged.  On the fused routes it is engine.FusedAdam's (cpc_ema behind
        # every update, also inside the captured step of use_graph, frozen by the device NaN guard), on the generic route
        # engine.TorchEma behind optimizer.step().  Single process or data parallel alike: every rank averages the same parameters.
        self.ema_decay = None
        self.ema_warmup = False
        # Not in the reference: NormalizedScoreFunction(learnable=True) / (schedule=...) keep the temperature in device memory
        # (engine.DeviceTemperature), which the trainer owns across train() calls: the learned value, its Adam moments and the schedule's
        # place carry on, and optimizer_state["temperature"] (FusedAdam.state_dict() writes it) replaces them.  last_temperature: the
        # value behind the latest step read back; every step's value goes to logger.temperature_meter where the logger has one.
        self._temperature = None
        self.last_temperature = None
        # Not in the reference's signature: waveform augmentation in the time domain ("Waveform augmentation").
        # augmentation: None, or an augmentation.WaveAugmentation — batch i of a train() call reaches the model, the engine or the
        #   preprocessing module as aug(batch, step = continue_training_at_step + i, clip_offset = rank * batch_size), so that a
        #   resumed run and every rank of a data-parallel run draw what one uninterrupted single-process run draws;
        # augment_targets: False leaves bit for bit every sample the prediction_steps target frames depend on (the augmentation
        #   then acts on the past only); it needs AudioEncoder's geometry, so not a preprocessing module in front of the encoder.
        # Not with use_graph (the step number is a host-side launch argument).  validate(), calc_test_task_data() and test_task
        # never augment.
        self.augmentation = None
        self.augment_targets = True
        # Not in the reference: masking on the preprocessed grid ("Grid masking").  grid_masking: None, or a
        # grid_masking.GridMasking — the scalogram or log-mel grid of batch i of a train() call is masked in place right behind the
        # preprocessing module, on its stream, with step = continue_training_at_step + i and clip_offset = rank * batch_size (behind
        # ``augmentation`` where both are set: waveform first, grid second).  Not with use_graph or the gradient penalty.
        # validate(), calc_test_task_data() and test_task never mask.
        self.grid_masking = None
        self._ema = None          # the shadow: a flat f32 tensor shaped like model._flat_param
        self._ema_owner = None    # who updates it at present: the latest train() call's FusedAdam or TorchEma
        # Not in the reference: the preprocessing module of the NEXT batch runs on the side stream beside the current step (InputAhead)
        self.preprocess_ahead = True
        self.verbose = True
        if wasserstein_gradient_penalty:
            # reference :144-158.  Its penalty differentiates the summed scores with respect to the PREPROCESSED batch, which only
            # requires grad behind a preprocessing module (:100-102): without one the reference itself fails in autograd.grad.
            if preprocessing is None:
                raise ValueError("wasserstein_gradient_penalty needs a preprocessing module (the reference takes the penalty's "
                                 "gradient with respect to the preprocessed batch, contrastive_estimation_training.py:100-102, :147)")
            if score_function not in (linear_score_function, softplus_score_function) or optimizer is not torch.optim.Adam:
                raise NotImplementedError("the gradient penalty on the HIP path covers linear_score_function / softplus_score_function "
                                          "+ Adam; see DESIGN.md section 8")
            from .audio_model import AudioGRUModel, AudioLSTMModel
            ar = getattr(model, "autoregressive_model", None)
            if isinstance(ar, AudioGRUModel) and getattr(ar, "num_layers", 1) > 1:
                from .contexts import GRUContext
                raise NotImplementedError(GRUContext.GP_STACK_REASON)
            if isinstance(ar, AudioLSTMModel):
                from .contexts import LSTMContext
                raise NotImplementedError(LSTMContext.GP_REASON)
            model.gradient_penalty_engine = True      # engines built from now on also give the gradient w.r.t. the scalogram
        if self.verbose:
            print("use score function", self.score_function)

    # ------------------------------------------------------------------------------------------ helpers
    def _device(self):
        if self.device is not None:
            return torch.device(self.device)
        return next(self.model.parameters()).device

    def _model_input(self, batch):
        """(B, L) device batch -> what the model is called with: (B, 1, L), or the scalogram when a preprocessing module
        (scalogram_model.PreprocessingModule) is set — reference :99-103, :221-223, :289-291."""
        x = batch.unsqueeze(1)
        if self.preprocessing is not None:
            x = self.preprocessing(x)
        return x

    def _fused(self):
        return self.score_function in (softplus_score_function, linear_score_function) and self.optimizer is torch.optim.Adam

    def _engine_difference(self):
        """difference_score_function + Adam also runs the whole step on the engine (cpc_diff_scores and its backward, FusedAdam, the
        device NaN guard); under global negatives it keeps the generic route."""
        return self.score_function is difference_score_function and self.optimizer is torch.optim.Adam and not self.global_negatives

    def _engine_normalized(self):
        """NormalizedScoreFunction + Adam also runs the whole step on the engine (cpc_norm_rows around the linear score's chain,
        FusedAdam, the device NaN guard); under global negatives it keeps the generic route."""
        return (isinstance(self.score_function, NormalizedScoreFunction) and self.optimizer is torch.optim.Adam
                and not self.global_negatives)

    def _check_negatives(self, batch_size):
        """Up-front checks of num_negatives (before any GPU work): ValueError unless 1 <= N <= batch_size - 1, NotImplementedError
        for what the sampled loss does not cover."""
        if self.num_negatives is None:
            return
        check_negatives(batch_size, self.num_negatives)
        if self.score_over_all_timesteps:
            raise NotImplementedError("num_negatives: the sampler is defined for score_over_all_timesteps=False only (it indexes the "
                                      "batch items of one prediction step, not the (item, step) pairs of the all-timesteps branch)")
        if self.wasserstein_gradient_penalty:
            raise NotImplementedError("num_negatives: wasserstein_gradient_penalty runs the dense loss kernels in its tangent passes; "
                                      "sampled negatives are not carried through them")
        if self.use_graph:
            raise NotImplementedError("num_negatives: use_graph replays one captured step, but the draw counter changes every step and "
                                      "lives on the host (like dropout's seed)")
        if self.global_negatives:
            raise NotImplementedError("num_negatives: global_negatives contrasts against the gathered batches of all ranks; the sampler "
                                      "draws from the rank's own batch only")

    def _check_negative_groups(self):
        """Up-front checks of negative_groups / negative_group_ids (before any GPU work): ValueError for an unknown value, for ids of
        the wrong kind or length, and for "same_file" over files that give one example per batch; NotImplementedError for what the
        grouped loss does not cover.  Returns None, or (mode, int32 numpy ids or None for the file index)."""
        if self.negative_groups is None:
            return None
        if self.negative_groups not in _NEGATIVE_GROUP_MODES:
            raise ValueError(f"negative_groups must be None or one of {tuple(_NEGATIVE_GROUP_MODES)}, got {self.negative_groups!r}")
        ids = None
        if self.negative_group_ids is not None:
            ids = np.asarray(self.negative_group_ids)
            if ids.ndim != 1 or ids.dtype.kind not in "iu":
                raise ValueError("negative_group_ids must be None or a 1-D sequence of integers")
            if ids.size != len(self.dataset):
                raise ValueError(f"negative_group_ids must have len(dataset) = {len(self.dataset)} entries, got {ids.size}")
            if ids.size and (int(ids.min()) < -2 ** 31 or int(ids.max()) > 2 ** 31 - 1):
                raise ValueError("negative_group_ids must fit 32-bit signed integers")
            ids = ids.astype(np.int32)
        elif self.negative_groups == "same_file" and int(self.file_batch_size) < 2:
            raise ValueError("negative_groups='same_file' with the file index as the group id needs file_batch_size >= 2: with one "
                             "example per file and batch no target would have a negative")
        if self.score_over_all_timesteps:
            raise NotImplementedError("negative_groups: defined for score_over_all_timesteps=False only (the groups index the batch "
                                      "items of one prediction step, not the (item, step) pairs of the all-timesteps branch)")
        if self.wasserstein_gradient_penalty:
            raise NotImplementedError("negative_groups: wasserstein_gradient_penalty runs the dense loss kernels in its tangent passes; "
                                      "grouped negatives are not carried through them")
        if self.use_graph:
            raise NotImplementedError("negative_groups: use_graph replays one captured step, but the group ids of a step's batch come "
                                      "from the host every step")
        if self.global_negatives:
            raise NotImplementedError("negative_groups: global_negatives contrasts against the gathered batches of all ranks; the "
                                      "groups are those of the rank's own batch only")
        return _NEGATIVE_GROUP_MODES[self.negative_groups], ids

    def _groups_kw(self, grouping, idx, device):
        """{} without negative_groups; else the step's negative_groups = (int32 device ids of the batch's examples, mode), and
        last_empty_negative_sets is set from the same ids."""
        if grouping is None:
            return {}
        mode, ids = grouping
        gid = np.ascontiguousarray(ids[np.asarray(idx, dtype=np.int64)], dtype=np.int32)
        self.last_empty_negative_sets = empty_negative_sets(gid, mode)
        return {"negative_groups": (torch.from_numpy(gid).to(device), mode)}

    def _check_negative_bank(self):
        """Up-front checks of negative_bank (before any GPU work): ValueError unless None or an integer in 1 .. 63,
        NotImplementedError for what the banked loss does not cover.  Returns None or M."""
        if self.negative_bank is None:
            return None
        from .engine import check_slots_back
        slots_back = check_slots_back(self.negative_bank)
        if self.score_over_all_timesteps:
            raise NotImplementedError("negative_bank: defined for score_over_all_timesteps=False only (its rows are the predictions of "
                                      "one step k each, not the (item, step) pairs of the all-timesteps branch)")
        if self.wasserstein_gradient_penalty:
            raise NotImplementedError("negative_bank: wasserstein_gradient_penalty runs the dense loss kernels in its tangent passes; "
                                      "a bank is not carried through them")
        if self.use_graph:
            raise NotImplementedError("negative_bank: use_graph replays one captured step, but the bank's cursor and its mask of filled "
                                      "slots live on the host and change every step")
        if self.global_negatives:
            raise NotImplementedError("negative_bank: global_negatives contrasts against the gathered batches of all ranks; the bank "
                                      "holds the rank's own earlier predictions only")
        if self.num_negatives is not None or self.negative_groups is not None:
            raise NotImplementedError("negative_bank together with num_negatives or negative_groups: no selection over the rows of "
                                      "earlier steps exists")
        sf = self.score_function
        if sf is difference_score_function:
            raise NotImplementedError("negative_bank: difference scores are formed by cpc_diff_scores, which takes no ring of earlier "
                                      "predictions")
        if isinstance(sf, NormalizedScoreFunction) and (sf.learnable or sf.schedule is not None):
            raise NotImplementedError("negative_bank: a learnable or scheduled temperature — the rows of earlier steps carry the "
                                      "1 / temperature of their own step")
        if not (self._fused() or self._engine_normalized()):
            raise NotImplementedError("negative_bank runs on the engine route only: optimizer=torch.optim.Adam with "
                                      "linear_score_function, softplus_score_function or a NormalizedScoreFunction of constant "
                                      f"temperature, not {self.optimizer!r} with {sf!r}")
        return slots_back

    def _check_anchors(self):
        """Up-front checks of the model's prediction_anchors (before any GPU work).  With A > 1 the engine route with
        softplus_score_function or linear_score_function and in-batch negatives is supported; it composes with what is orthogonal to
        the loss (clipping, AdamW and schedule, LAMB, EMA, waveform augmentation, a device-resident dataset).  NotImplementedError for
        everything that indexes K heads per item or has no stacked-head form."""
        A = int(getattr(self.model, "prediction_anchors", 1))
        if A <= 1:
            return
        what = f"prediction_anchors = {A}"
        if self.score_over_all_timesteps:
            raise NotImplementedError(f"{what}: score_over_all_timesteps contrasts the (item, step) pairs of ONE anchor's K steps; no "
                                      "all-timesteps loss over stacked anchors exists")
        if self.num_negatives is not None:
            raise NotImplementedError(f"{what}: num_negatives — the sampler's draws are keyed by the K prediction steps, not by A K heads")
        if self.negative_groups is not None:
            raise NotImplementedError(f"{what}: negative_groups — the grouped loss is not stacked over anchors")
        if self.negative_bank is not None:
            raise NotImplementedError(f"{what}: negative_bank — the bank's rows are [B][K][E] predictions of one anchor")
        if self.global_negatives:
            raise NotImplementedError(f"{what}: global_negatives — the gathered loss is built for K heads per item")
        if self.wasserstein_gradient_penalty:
            raise NotImplementedError(f"{what}: wasserstein_gradient_penalty — its tangent passes differentiate c = h_V alone")
        sf = self.score_function
        if sf is difference_score_function or isinstance(sf, NormalizedScoreFunction):
            raise NotImplementedError(f"{what}: difference and normalized scores are not stacked over anchors; use "
                                      "softplus_score_function or linear_score_function")
        if not self._fused():
            raise NotImplementedError(f"{what} runs on the engine route only: optimizer=torch.optim.Adam with linear_score_function or "
                                      f"softplus_score_function, not {self.optimizer!r} with {sf!r} (the generic route scores K heads)")
        if self.use_graph:
            raise NotImplementedError(f"{what}: use_graph — no captured step with anchors exists")

    def reset_negative_bank(self):
        """Empties the bank: the next step is the in-batch step again, the ones after it fill the bank anew."""
        if self._bank is not None:
            self._bank.reset()

    @property
    def negative_bank_filled(self):
        """How many earlier steps the bank holds at present (0 without a bank)."""
        return 0 if self._bank is None else self._bank.filled

    def _bank_kw(self, slots_back):
        """{} without negative_bank; else the step's negative_bank = the trainer's engine.NegativeBank, made anew when M changed."""
        if slots_back is None:
            self._bank = None
            return {}
        if self._bank is None or self._bank.slots != slots_back + 1:
            from .engine import NegativeBank
            self._bank = NegativeBank(slots_back)
        return {"negative_bank": self._bank}

    def _check_grad_clip(self):
        """Up-front checks of max_grad_norm (before any GPU work): ValueError unless None or finite and > 0, NotImplementedError
        together with use_graph."""
        from .engine import check_max_grad_norm
        value = check_max_grad_norm(self.max_grad_norm)
        if value is not None and self.use_graph:
            raise NotImplementedError("max_grad_norm: use_graph replays one captured step, and clipped steps are not captured into a "
                                      "hipGraph")
        return value

    def _check_adamw(self):
        """Up-front checks of weight_decay, weight_decay_filter, lr_schedule and optimizer_state (before any GPU work): ValueError
        for a decay that is not finite and >= 0, a filter that is not callable, a schedule that is no LRSchedule, a state that is no
        dict.  Returns (weight_decay, filter or None, schedule or None)."""
        from .engine import check_weight_decay
        value = check_weight_decay(self.weight_decay, self.weight_decay_filter)
        if self.lr_schedule is not None and not isinstance(self.lr_schedule, LRSchedule):
            raise ValueError(f"lr_schedule must be None or an LRSchedule, got {self.lr_schedule!r}")
        if self.optimizer_state is not None and not isinstance(self.optimizer_state, dict):
            raise ValueError("optimizer_state must be None or an optimizer's state dict")
        return value, self.weight_decay_filter, self.lr_schedule

    def _check_trust(self):
        """Up-front checks of trust_ratio and trust_clip (before any GPU work): ValueError for a trust_ratio that is no bool or a
        trust_clip that is not None or finite and > 0; with trust_ratio, NotImplementedError together with use_graph or an optimizer
        other than torch.optim.Adam.  Returns (trust_ratio, trust_clip)."""
        from .engine import check_trust
        trust_ratio, trust_clip = check_trust(self.trust_ratio, self.trust_clip)
        if trust_ratio and self.use_graph:
            raise NotImplementedError("trust_ratio: use_graph replays one captured step, and no captured LAMB step exists")
        if trust_ratio and self.optimizer is not torch.optim.Adam:
            raise NotImplementedError("trust_ratio rescales Adam's direction (optimizer=torch.optim.Adam); the direction of "
                                      f"{self.optimizer!r} is not ours to rescale")
        return trust_ratio, trust_clip

    def _check_ema(self):
        """Up-front checks of ema_decay and ema_warmup (before any GPU work): ValueError for a decay that is not None or a number in
        [0, 1), a warmup that is no bool, or a warmup without a decay.  Returns (ema_decay or None, ema_warmup)."""
        from .engine import check_ema
        return check_ema(self.ema_decay, self.ema_warmup)

    def reset_ema(self):
        """Drops the average: the next train() with an ema_decay starts it over from the parameters as they then stand."""
        self._ema = self._ema_owner = None

    def ema_state_dict(self):
        """The model's state_dict() with the parameters taken from the average and the buffers (BatchNorm's running statistics, which
        are not averaged) from the live model.  ValueError when no average exists."""
        owner = self._ema_holder()
        if hasattr(owner, "ema_state_dict"):
            return owner.ema_state_dict()
        out = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        out.update(owner.state_dict()["ema"])
        return out

    def _ema_holder(self):
        if self._ema is None or self._ema_owner is None:
            raise ValueError("no average of the weights exists: set ema_decay and train() first")
        return self._ema_owner

    def _ema_weights(self, use_ema):
        """Context of validate() / calc_test_task_data(): the averaged weights in the model's place when asked, else nothing."""
        import contextlib
        if not use_ema:
            return contextlib.nullcontext()
        owner = self._ema_holder()
        return owner.ema_weights() if hasattr(owner, "ema_weights") else owner.weights()

    def _shadow_views(self):
        """{parameter name: view of the flat shadow}, the form engine.TorchEma takes."""
        off = self.model._offset
        return {n: self._ema[off[n]:off[n] + p.numel()].view(p.shape) for n, p in self.model.named_parameters()}

    def _score_kind(self):
        if self.score_function is difference_score_function:
            return "difference"
        if isinstance(self.score_function, NormalizedScoreFunction):
            return "normalized"
        return "softplus" if self.score_function is softplus_score_function else "linear"

    def _score_kw(self):
        """The engine's score keywords: score=kind and, with NormalizedScoreFunction, its temperature — the device's where this
        trainer keeps one for that function, else the constant."""
        kw = {"score": self._score_kind()}
        if kw["score"] == "normalized":
            sf = self.score_function
            own = self._temperature is not None and sf.device_temperature is self._temperature
            kw["temperature"] = self._temperature if own else sf.temperature
        return kw

    def _check_temperature(self, world):
        """Up-front checks of a learnable or scheduled temperature (before any GPU work): NotImplementedError for learnable=True off
        the engine route (a foreign optimizer, global_negatives) or in a data-parallel run.  Returns None (a constant, or another score
        function), "device" (the engine route keeps it in device memory) or "host" (a schedule on the generic route or under data
        parallelism: the constant is set to schedule.value(step) before every step)."""
        sf = self.score_function
        if not isinstance(sf, NormalizedScoreFunction) or not (sf.learnable or sf.schedule is not None):
            return None
        if sf.learnable:
            if not self._engine_normalized():
                raise NotImplementedError("a learnable temperature is trained by the fused optimizer on the engine route "
                                          "(optimizer=torch.optim.Adam, no global_negatives): a foreign optimizer does not know the scalar, "
                                          "and under global_negatives its gradient is spread over the ranks")
            if world > 1:
                raise NotImplementedError("a learnable temperature in a data-parallel run: the scalar's gradient would need a reduction "
                                          "of its own over the ranks")
            return "device"
        return "device" if self._engine_normalized() and world == 1 else "host"

    def _start_temperature(self, temp_route, device, start_step):
        """_check_temperature's route at the start of a run.  "device": returns the DeviceTemperature this trainer keeps for its score
        function, made on first use.  "host": the callable's constant is set to the schedule's value at ``start_step``; returns None."""
        sf = self.score_function
        if temp_route == "device":
            kept = self._temperature
            if kept is None or sf.device_temperature is not kept or kept.device != torch.device(device):
                kept = self._temperature = sf.make_device_temperature(device)
                sf.device_temperature = kept
            kept.bind(None)          # (a captured step of an earlier call had it read the step from its optimizer's count)
            return kept
        if temp_route == "host":          # the callable's constant follows the schedule; no device value takes part
            sf.device_temperature = self._temperature = None
            sf.temperature = sf.schedule.value(int(start_step))
        return None

    def _check_augmentation(self):
        """None without augmentation; else (the WaveAugmentation, protect(L) -> the first protected sample of clips of L samples).
        TypeError for anything but a WaveAugmentation, NotImplementedError with use_graph, ValueError for augment_targets=False
        on a model whose encoder does not give the frame geometry of the waveform."""
        aug = self.augmentation
        if aug is None:
            return None
        from .augmentation import WaveAugmentation
        if not isinstance(aug, WaveAugmentation):
            raise TypeError(f"augmentation must be None or an augmentation.WaveAugmentation, got {type(aug).__name__}")
        if self.use_graph:
            raise NotImplementedError("augmentation: use_graph replays one captured step, but the augmentation's step number is a "
                                      "host-side launch argument that changes every step")
        if self.augment_targets:
            return aug, lambda L: None
        from .audio_model import AudioEncoder
        enc = getattr(self.model, "encoder", None)
        if self.preprocessing is not None or not isinstance(enc, AudioEncoder):
            raise ValueError("augment_targets=False needs the frame geometry of the waveform (AudioEncoder's receptive_field and "
                             "downsampling_factor): not available for a scalogram encoder behind a preprocessing module")
        field, hop, K = int(enc.receptive_field), int(enc.downsampling_factor), int(self.model.prediction_steps)

        def protect(L):
            T = (int(L) - field) // hop + 1
            if L < field or T <= K:
                raise ValueError(f"augment_targets=False: clips of {int(L)} samples give {max(T, 0)} frames, not more than the "
                                 f"{K} target frames")
            return hop * (T - K)          # the first sample of frame T - K: everything the K target frames read
        return aug, protect

    @staticmethod
    def _augmented(batches, aug, protect, steps, clip_offset, with_indices):
        """The batches of ``batches`` augmented: batch i of the run at step i (``steps``: the run's itertools.count, which goes on
        over the epochs).  Every output is a fresh tensor, so the one in hand stays valid while the following batch is prepared."""
        for item in batches:
            batch = item[0] if with_indices else item
            out = aug(batch, next(steps), clip_offset=clip_offset, protect_from=protect(batch.shape[1]))
            yield (out, item[1]) if with_indices else out

    def _check_grid_masking(self):
        """None without grid masking, else the GridMasking.  TypeError for anything else, ValueError where no grid exists (no
        preprocessing module, or one that hands the waveform on), NotImplementedError with use_graph or the gradient penalty."""
        masking = self.grid_masking
        if masking is None:
            return None
        from .grid_masking import GridMasking
        if not isinstance(masking, GridMasking):
            raise TypeError(f"grid_masking must be None or a grid_masking.GridMasking, got {type(masking).__name__}")
        pre = self.preprocessing
        if (pre is None or isinstance(pre, torch.nn.Identity) or (hasattr(pre, "cqt") and pre.cqt is None)
                or (hasattr(pre, "mel") and pre.mel is None)):
            raise ValueError("grid_masking needs a preprocessing module that returns a grid (scalogram_model.PreprocessingModule with a "
                             "cqt_dict, mel_spectrogram.MelPreprocessingModule with a mel_dict): the waveform has no frequency axis")
        if self.use_graph:
            raise NotImplementedError("grid_masking: use_graph replays one captured step, but the mask's step number is a host-side "
                                      "launch argument that changes every step")
        if self.wasserstein_gradient_penalty:
            raise NotImplementedError("grid_masking with wasserstein_gradient_penalty is not verified (the penalty differentiates with "
                                      "respect to the preprocessed grid)")
        return masking

    def _masked_input(self, masking, steps, clip_offset):
        """_model_input followed by the mask, in place and on the stream _model_input ran on: the i-th call of a run masks at step
        next(``steps``) (the batches are preprocessed in batch order, the one preprocessed ahead included)."""
        def model_input(batch):
            x = self._model_input(batch)
            if not isinstance(x, torch.Tensor) or x.dim() != 4:
                raise ValueError("grid_masking: the preprocessing module did not return a (B, channels, bins, frames) grid")
            masking(x.permute(0, 3, 2, 1), next(steps), clip_offset=clip_offset)          # the channels-last buffer behind the view
            return x
        return model_input

    @staticmethod
    def _world():
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _batches(self, dataset, sampler, device, num_workers, pin_memory, rank, world, with_indices=False):
        """Yields device batches (B, L).  A dataset exposing ``device_data`` (an (N, L) tensor already in HBM) is
        indexed on the device; one exposing ``device_batch`` with its samples in HBM (DeviceAudioDataset(device=...)) cuts each batch
        there with one launch; anything else goes through a torch DataLoader as in the reference (:87-91).
        with_indices: yields (batch, the example indices of that batch — this rank's slice under data parallelism) instead."""
        resident = getattr(dataset, "device_data", None)
        gather = getattr(dataset, "device_batch", None) if getattr(dataset, "device", None) is not None else None
        fifo = collections.deque() if with_indices else None

        def out(b):
            return (b, fifo.popleft()) if with_indices else b
        if world > 1:
            import torch.distributed as dist
            lists = [list(b) for b in iter(sampler)] if rank == 0 else None
            box = [lists]
            dist.broadcast_object_list(box, src=0)
            per = len(box[0][0]) // world if box[0] else 0
            index_lists = [b[rank * per:(rank + 1) * per] for b in box[0]]
        else:
            index_lists = None
        source = index_lists if index_lists is not None else sampler
        if with_indices:
            source = _RecordingSampler(source, fifo)
        if resident is not None:
            for idx in iter(source):
                yield out(resident[torch.as_tensor(list(idx), device=resident.device)])
            return
        if gather is not None:
            for idx in iter(source):
                batch = gather(list(idx))
                yield out(batch[0] if isinstance(batch, tuple) else batch)          # (a labels=True dataset hands out its labels too)
            return
        loader = torch.utils.data.DataLoader(dataset, batch_sampler=source, num_workers=num_workers, pin_memory=pin_memory)
        if torch.device(device).type != "cuda":
            for batch in iter(loader):
                yield out(batch.to(device=device, non_blocking=True))
            return
        # Host dataset: double-buffered upload.  Batch i + 1 travels pinned host -> HBM on a copy stream while step i computes
        # (21 MB per step at B = 256: 0.3-0.4 ms of PCIe time that would otherwise sit in front of every step).
        copy = torch.cuda.Stream(device=device)
        it = iter(loader)

        def fetch():
            batch = next(it, None)
            if batch is None:
                return None
            with torch.cuda.stream(copy):
                dev_batch = batch.to(device=device, non_blocking=True)
                done = torch.cuda.Event()
                done.record(copy)
            return dev_batch, done, batch          # the pinned source stays referenced until its copy has been waited for

        nxt = fetch()
        while nxt is not None:
            dev_batch, done, _src = nxt
            nxt = fetch()
            cur = torch.cuda.current_stream(device)
            cur.wait_event(done)
            dev_batch.record_stream(cur)
            yield out(dev_batch)

    # ------------------------------------------------------------------------------------------ train
    def train(self, batch_size=32, epochs=10, lr=0.0001, continue_training_at_step=0, num_workers=1, max_steps=None,
              profile=False):
        """Same contract as the reference's train (:74-176): returns ``prof`` (None unless profile=True) when max_steps is
        reached, None on a NaN loss or when the epochs are exhausted.  ``batch_size`` is the per-process batch; under
        torch.distributed the sampler draws batch_size * world_size indices and every rank takes its slice."""
        self._check_anchors()
        self._check_negatives(batch_size)
        grouping = self._check_negative_groups()
        bank_kw = self._bank_kw(self._check_negative_bank())
        augmenting = self._check_augmentation()
        aug_steps = itertools.count(int(continue_training_at_step))          # the step of the next batch the augmentation sees
        masking = self._check_grid_masking()
        max_grad_norm = self._check_grad_clip()
        weight_decay, decay_filter, schedule = self._check_adamw()
        trust = self._check_trust()
        ema = self._check_ema()
        device = self._device()
        rank, world = self._world()
        temp_route = self._check_temperature(world)
        self.model.train()
        device_temp = self._start_temperature(temp_route, device, continue_training_at_step)
        score_kw = self._score_kw()
        run = self._make_optimizer(lr, device, world, int(continue_training_at_step), max_grad_norm,
                                   (weight_decay, decay_filter, schedule), trust, ema, device_temp)
        optimizer, fused = run.optimizer, run.fused
        if masking is not None:
            run.model_input = self._masked_input(masking, itertools.count(int(continue_training_at_step)), rank * int(batch_size))
        sampler = FileBatchSampler(index_count_per_file=self.dataset.get_example_count_per_file(),
                                   batch_size=batch_size * world, file_batch_size=self.file_batch_size, drop_last=True,
                                   verbose=self.verbose)
        if grouping is not None and grouping[1] is None:
            grouping = (grouping[0], file_group_ids(self.dataset.get_example_count_per_file()))
        self.training_step = continue_training_at_step
        readback = _StepReadback(self, optimizer, run.clip, fused, device.type == "cuda", device_temp, temp_route)
        rollback = _NanRollback(self, optimizer, fused, device_temp)
        # A full collection of Python's cyclic garbage collector walks every tracked object of the process (38 - 43 ms with the module
        # trees of a model alive) and lands in whichever step crosses its allocation threshold — a GPU that is only a few steps of work
        # ahead of the host idles through it.  What is alive now stays alive for the whole run: collect once and freeze it, later
        # collections only look at what the steps allocate (bench.py, round 4: this is the 41 ms the round-3 driver run lost once).
        import gc
        gc.collect()
        gc.freeze()
        for current_epoch in range(epochs):
            if self.verbose:
                print("epoch", current_epoch)
            with torch.autograd.profiler.profile(use_device="cuda", enabled=profile) as prof_ctx:
                ahead = None
                if (fused and not run.graphed and self.preprocessing is not None and self.preprocess_ahead and device.type == "cuda"
                        and switches.preprocess_ahead()):
                    ahead = InputAhead(run.model_input, device)
                batches = self._batches(self.dataset, sampler, device, num_workers, True, rank, world,
                                        with_indices=grouping is not None)
                if augmenting is not None:          # in front of everything that sees a batch, the one preprocessed ahead included
                    batches = self._augmented(batches, augmenting[0], augmenting[1], aug_steps, rank * int(batch_size),
                                              grouping is not None)
                # (the sampler is read one batch ahead only where that batch is preprocessed ahead)
                for batch, next_batch in (_with_next(batches) if ahead is not None else ((b_, None) for b_ in batches)):
                    groups_kw = {}
                    if grouping is not None:          # the indices travel with their batch, the one ahead keeps its own
                        batch, batch_idx = batch
                        next_batch = next_batch[0] if next_batch is not None else None
                        groups_kw = self._groups_kw(grouping, batch_idx, device)
                    rollback.snapshot(self.training_step)
                    # the step's learning rate, before its first hook can fire (under use_graph the device evaluates the same factor)
                    self.last_lr = step_lr = lr if schedule is None else lr * schedule.factor(self.training_step)
                    if fused and schedule is not None:
                        optimizer.lr = step_lr
                    if device_temp is not None:          # scheduled: the tick's step (a captured step reads the device's count instead)
                        device_temp.step = int(self.training_step)
                    elif temp_route == "host":
                        self.score_function.temperature = score_kw["temperature"] = \
                            self.score_function.schedule.value(int(self.training_step))
                    if run.graphed:
                        vals = self._graphed_step(run, batch, score_kw)
                    elif fused:
                        vals = self._fused_step(run, batch, next_batch, ahead, score_kw, groups_kw, bank_kw)
                    else:
                        vals = self._generic_step(batch, batch.shape[0], optimizer, world, max_grad_norm,
                                                  (step_lr if schedule is not None else None, step_lr * weight_decay, run.decayed),
                                                  ema=run.generic_ema, model_input=run.model_input, **groups_kw)
                    readback.push(self.training_step, vals)
                    if not fused:            # this route has already read the loss (NaN check in front of backward(), as the reference)
                        nan_step = readback.flush()
                        if nan_step is not None:
                            return self._nan_return(nan_step, readback, rollback)
                    # the readback trails the launches by host_sync_lag steps: the host waits for step i - 1's loss while step i
                    # already runs (reading step i's loss right away left the GPU idle for 0.3 ms of every 5.1 ms step while the
                    # host prepared the next one); every step is still logged, in order, and a NaN loss still ends the run
                    if len(readback.pending) >= self.host_sync_interval + self.host_sync_lag:
                        nan_step = readback.flush(keep=self.host_sync_lag)
                        if nan_step is not None:
                            return self._nan_return(nan_step, readback, rollback)
                    self.training_step += 1
                    if max_steps is not None and self.training_step >= max_steps:
                        nan_step = readback.flush()
                        if nan_step is not None:
                            return self._nan_return(nan_step, readback, rollback)
                        return prof_ctx if profile else None
        nan_step = readback.flush()
        if nan_step is not None:
            return self._nan_return(nan_step, readback, rollback)
        return None

    def _nan_return(self, step, readback, rollback):
        """Leaves train() after a NaN loss at ``step`` with the run where a clean run of ``step`` steps leaves it ("What the
        NaN guard holds still"): the device state was never touched (skip flag), BatchNorm's statistics, the optimizer's count and rate,
        last_lr and the temperature's place are put back (_NanRollback), training_step is the NaN step, and the bank is emptied — the
        one thing that is reset, not restored.  last_grad_norm stays the NaN step's, which is what is reported below."""
        rollback.restore(step)
        self.training_step = step          # the reference leaves train() inside step `step`, before its update (:124-133)
        self.reset_negative_bank()         # (its latest rows come from the NaN step and the ones launched behind it)
        if readback.bad_grad_norm:
            print("gradient norm not finite at step", step, "(max_grad_norm): no update was applied")
        print("nan loss")
        print("returned with nan loss at step", step)
        return None

    def _make_optimizer(self, lr, device, world, start_step, max_grad_norm, adamw, trust, ema, device_temp):
        """The optimizer of one train() call and what its step routes share, as one namespace: optimizer, fused (the engine route),
        graphed (use_graph's captured step), sync (GradAllReduce under data parallelism), generic_ema (the generic route's TorchEma),
        decayed (the parameters the generic route decays itself), device / world / clip and the step routes' caches: graph_steps
        ((B, L) -> GraphedStep), glob_neg (id(engine) -> GlobalNegatives), guarded (engines whose sticky NaN flag was cleared for this
        run), model_input (batch -> what the model is called with: _model_input, which train() replaces by _masked_input under
        grid_masking).  adamw, trust, ema: what _check_adamw, _check_trust and _check_ema return.  Loads and clears optimizer_state."""
        (weight_decay, decay_filter, schedule), (trust_ratio, trust_clip), (ema_decay, ema_warmup) = adamw, trust, ema
        fused = self._fused() or self._engine_difference() or self._engine_normalized()
        run = types.SimpleNamespace(fused=fused, graphed=False, sync=None, generic_ema=None, decayed=[], device=device, world=world,
                                    clip=max_grad_norm is not None, graph_steps={}, glob_neg={}, guarded=set(),
                                    model_input=self._model_input)
        self.model._flatten_parameters(device)
        if fused:
            from .engine import FusedAdam, GradAllReduce
            run.graphed = bool(self.use_graph) and world == 1 and self.preprocessing is None
            lamb = dict(trust_ratio=True, trust_clip=trust_clip) if trust_ratio else {}
            if ema_decay is not None:          # (without a decay FusedAdam is called as before the keywords existed)
                flat = self.model._flat_param
                if self._ema is not None and (self._ema.shape != flat.shape or self._ema.device != flat.device):
                    self.reset_ema()          # another model or device: the old average means nothing here
                lamb.update(ema_decay=ema_decay, ema_warmup=ema_warmup, ema=self._ema)
            if device_temp is not None:          # (without one FusedAdam is called as before the keyword existed)
                lamb.update(temperature=device_temp)
            optimizer = FusedAdam(self.model, lr=lr, device_step=run.graphed, max_grad_norm=max_grad_norm, weight_decay=weight_decay,
                                  decay_filter=decay_filter, schedule=schedule, step_offset=start_step, **lamb)
            if ema_decay is not None:
                self._ema, self._ema_owner = optimizer.ema, optimizer
            self.last_optimizer = optimizer          # (inspection only: tests read its step count after a NaN return)
            self.model.link_grads()
            run.sync = GradAllReduce(self.model, optimizer=optimizer) if world > 1 else None
        elif trust_ratio:          # LAMB's decay is inside its direction: no multiply in front of the step
            from .engine import TorchLamb
            optimizer = TorchLamb(self.model.named_parameters(), lr=lr, weight_decay=weight_decay, decay_filter=decay_filter,
                                  trust_clip=trust_clip)
        else:
            optimizer = self.optimizer(self.model.parameters(), lr=lr)
        run.optimizer = optimizer
        if ema_decay is not None and not fused:
            from .engine import TorchEma
            flat = self.model._flat_param
            if self._ema is None or self._ema.shape != flat.shape or self._ema.device != flat.device:
                self._ema = flat.detach().float().clone()
            run.generic_ema = self._ema_owner = TorchEma(self.model.named_parameters(), ema_decay, ema_warmup,
                                                         shadow=self._shadow_views())
        if weight_decay > 0.0 and not fused and not trust_ratio:          # the generic route multiplies them itself, in front of optimizer.step()
            from .engine import default_decay_filter
            run.decayed = [p for n_, p in self.model.named_parameters() if (decay_filter or default_decay_filter)(n_, p)]
        if self.optimizer_state is not None:
            state, self.optimizer_state = self.optimizer_state, None
            optimizer.load_state_dict(state)
            if run.generic_ema is not None:          # (FusedAdam.load_state_dict has taken its "ema" itself)
                entries = state.get("state", {})
                names = [n for n, _ in self.model.named_parameters()]
                if entries and all(i in entries and "ema" in entries[i] for i in range(len(names))):
                    run.generic_ema.load_state_dict({"ema": {n: entries[i]["ema"] for i, n in enumerate(names)}})
                else:
                    with torch.no_grad():
                        self._ema.copy_(self.model._flat_param.detach())
        return run

    @staticmethod
    def _clear_nan_flag_once(run, eng):
        """The engine's sticky NaN flag is cleared the first time a run meets the engine."""
        if id(eng) not in run.guarded:
            eng.nan_flag().zero_()
            run.guarded.add(id(eng))

    def _graphed_step(self, run, batch, score_kw):
        """use_graph: the whole step replayed from the hipGraph captured for the batch's shape (engine.GraphedStep)."""
        eng = self.model.engine(batch.shape[0], batch.shape[1], run.device)
        key = (batch.shape[0], batch.shape[1])
        if key not in run.graph_steps:
            from .engine import GraphedStep
            run.graph_steps[key] = GraphedStep(eng, run.optimizer, self.score_function is softplus_score_function,
                                               float(self.regularization), bool(self.score_over_all_timesteps), **score_kw)
        self._clear_nan_flag_once(run, eng)
        return run.graph_steps[key](batch)

    def _fused_step(self, run, batch, next_batch, ahead, score_kw, groups_kw, bank_kw):
        """The engine route: forward, loss, analytic backward and the fused optimizer's update as HIP kernels.  ahead: None or the
        epoch's InputAhead, which hands over this batch's model input and is given ``next_batch`` beside this step."""
        optimizer, sync = run.optimizer, run.sync
        if self.preprocessing is not None:
            if ahead is not None:
                if not ahead.pending:              # first step of the epoch: nothing was submitted beside a previous one
                    ahead.submit(batch)
                _, x_eng = ahead.take()
            else:
                x_eng = run.model_input(batch)
            eng = self.model.engine_for(x_eng)
            if ahead is not None and next_batch is not None:
                # the engine runs it behind its encoder's forward pass, where its main queue turns latency-bound
                eng.side_job = lambda nb=next_batch: ahead.submit(nb)
        else:
            x_eng = batch.contiguous()
            eng = self.model.engine(batch.shape[0], batch.shape[1], run.device)
        gneg = None
        if self.global_negatives and run.world > 1:
            gneg = run.glob_neg.get(id(eng))
            if gneg is None:
                from .engine import GlobalNegatives
                gneg = run.glob_neg[id(eng)] = GlobalNegatives(eng)
        # the operand copies of the next step are rebuilt as soon as Adam has updated their parameters
        # (engine.CPCEngine.prepare_ahead; under data parallelism Adam follows each reduced gradient piece)
        optimizer.after_update = eng.prepare_ahead
        # NaN guard on the device (reference :124-133 returns before backward() / optimizer.step()): the loss
        # kernel — whichever the route takes: dense, sampled, grouped, banked, all-timesteps or the fused chain's finalize —
        # raises the engine's sticky flag; every stateful launch of this and of later steps (Adam / AdamW / LAMB with its trust
        # table, cpc_ema, cpc_temperature_step) is a no-op while it is up, and the host leaves train() when the step's indicator
        # arrives (host_sync_lag steps later); what is no update and so is not skipped — BatchNorm's statistics, a scheduled
        # temperature's tick, the host's counts — is _NanRollback's to put back
        self._clear_nan_flag_once(run, eng)
        optimizer.skip_flag = eng.nan_flag()
        if run.clip:
            optimizer.nan_pair = eng.nan_pair()
        # per-GPU negatives: mean of the shard gradients; global negatives: the shard gradients add up
        grad_scale = 1.0 if gneg is not None else 1.0 / run.world
        if sync is not None:
            sync.grad_scale = grad_scale
        if self.wasserstein_gradient_penalty:
            # three passes through the network (scalogram_engine.ScalogramCPCEngine._gp_step); the parameter
            # gradients are complete only at the end, so Adam runs once, after them
            route_kw = {"gradient_penalty": float(self.gradient_penalty_factor)}
        else:
            route_kw = dict(grad_ready_hook=sync.hook if sync is not None else getattr(optimizer, "hook", None),
                            **score_kw, **self._negatives_kw(), **groups_kw, **bank_kw)
        out = eng.loss_and_grads(x_eng, softplus=self.score_function is softplus_score_function,
                                 regularization=float(self.regularization), all_timesteps=bool(self.score_over_all_timesteps),
                                 global_negatives=gneg, after_loss=sync.reduce_flag if sync is not None else None, **route_kw)
        if sync is not None:
            sync.finish()
        optimizer.step(grad_scale=grad_scale)
        return out

    def _negatives_kw(self):
        """{} for the in-batch loss; else the step's negatives = (num_negatives, negative_seed, draw = training_step) — the same
        on every rank of a data-parallel run, each applying it to its own shard."""
        if self.num_negatives is None:
            return {}
        return {"negatives": (int(self.num_negatives), int(self.negative_seed), int(self.training_step))}

    def _generic_step(self, batch, batch_size, optimizer, world, max_grad_norm=None, adamw=(None, 0.0, ()), negative_groups=None,
                      ema=None, model_input=None):
        """Any score function / optimizer: model forward and backward through the autograd bridge (HIP), the score function as the
        caller wrote it, the loss and its gradient through the loss kernels (_InfoNCE).  This route reads the loss every step, so
        the NaN guard sits where the reference has it: in front of backward() and optimizer.step() (:124-133).  With max_grad_norm,
        torch.nn.utils.clip_grad_norm_ runs between the gradient all-reduce and optimizer.step() and the returned values grow by
        (norm before clipping, coefficient); a norm that is not finite raises the indicator and skips the update.
        adamw = (the step's learning rate under a schedule or None, lr * weight_decay of the step, the parameters that decay): every
        param group gets the rate, and the decay p <- p (1 - lr weight_decay) is applied right before optimizer.step().
        ema: None or the run's engine.TorchEma, updated right behind optimizer.step() with the number of the updates it has seen (the
        early returns above it — a NaN loss, a gradient norm that is not finite — leave the average where it is).
        model_input: None for _model_input, or the run's own (train() under grid_masking)."""
        predicted_z, targets, _, _ = self.model((model_input or self._model_input)(batch))
        scores = self.score_function(predicted_z, targets)
        selection = None
        if negative_groups is not None:
            selection = ("grouped", negative_groups[0], group_mode(negative_groups[1]),
                         *self._negatives_kw().get("negatives", (0, 0, 0)))
        elif self.num_negatives is not None:
            selection = ("sampled", *self._negatives_kw()["negatives"])
        loss, out = _InfoNCE.apply(scores, bool(self.score_over_all_timesteps), float(self.regularization), selection)
        nan = out[5:6].clone()
        if world > 1:          # every rank has its own loss: all ranks leave at the same step
            import torch.distributed as dist
            dist.all_reduce(nan, op=dist.ReduceOp.MAX)
        vals = torch.cat([out[:5], nan])
        if max_grad_norm is not None:
            vals = torch.cat([vals, vals.new_zeros(2)])
        if float(nan.item()) != 0.0:
            return vals
        self.model.zero_grad()
        loss.backward()
        if world > 1:
            for p in self.model.parameters():
                dist.all_reduce(p.grad)
                p.grad.div_(world)
        if max_grad_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_grad_norm).detach().float()
            vals[6], vals[7] = norm, torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0)
            if not math.isfinite(float(norm)):
                vals[5] = 1.0
                return vals
        step_lr, lr_wd, decayed = adamw
        if step_lr is not None:
            for group in optimizer.param_groups:
                group["lr"] = step_lr
        if lr_wd != 0.0 and decayed:
            with torch.no_grad():
                torch._foreach_mul_(list(decayed), 1.0 - lr_wd)
        optimizer.step()
        if ema is not None:
            ema.update(ema.updates + 1)
        return vals

    # ------------------------------------------------------------------------------------------ validate
    def validate(self, batch_size=64, num_workers=1, max_steps=None, use_ema=False):
        """_validate's measurement; with use_ema=True on the averaged weights (ema_decay): they take the model's place for the call and
        the raw weights are back afterwards, bit for bit, so it may be called from logger.log() in the middle of train().  ValueError
        when no average exists.  (The validation sampler seeds Python's random generator, as the reference's does; with use_ema=True
        the generator's state is put back, so that the epochs train() draws after the call are the ones it would have drawn.)"""
        if not use_ema:
            return self._validate(batch_size, num_workers, max_steps)
        state = random.getstate()
        try:
            with self._ema_weights(True):
                return self._validate(batch_size, num_workers, max_steps)
        finally:
            random.setstate(state)

    def _validate(self, batch_size=64, num_workers=1, max_steps=None):
        """Reference validate (:178-269): per-step loss, per-step arg-max accuracy, mean score and the mutual-information lower
        bound log(n) - loss over the validation set (eval mode, FileBatchSampler(seed=0, file_batch_size=8)).  The per-batch
        quantities come from cpc_nce_eval on the train step's own score matrices and are summed on the device; the host reads
        2 K + 1 numbers once, after the last batch.  Always in-batch, as the reference measures accuracy: num_negatives does not
        enter here."""
        import ctypes as C
        from . import _hip
        if self.validation_set is None:
            print("No validation set")
            return 0, 0
        device = self._device()
        K, all_t = self.prediction_steps, bool(self.score_over_all_timesteps)
        counts = self.validation_set.get_example_count_per_file()
        n_batches = sum(1 for _ in FileBatchSampler(counts, batch_size, 8, True, seed=0, verbose=False))
        steps = n_batches if max_steps is None else min(max_steps, n_batches)
        sampler = FileBatchSampler(index_count_per_file=counts, batch_size=batch_size, file_batch_size=8, drop_last=True, seed=0,
                                   verbose=self.verbose)
        sums = torch.zeros(2 * K + 1, device=device, dtype=torch.float32)
        ws = torch.empty(int(_hip.lib().cpc_nce_eval_workspace_floats(batch_size, K)), device=device, dtype=torch.float32)
        kernel_scores = (self.score_function in (softplus_score_function, linear_score_function, difference_score_function)
                         or isinstance(self.score_function, NormalizedScoreFunction))
        if int(getattr(self.model, "prediction_anchors", 1)) > 1 and (all_t or self.score_function not in (softplus_score_function,
                                                                                                             linear_score_function)):
            raise NotImplementedError("validate() with prediction_anchors > 1 scores the last anchor's K heads with "
                                      "softplus_score_function or linear_score_function, score_over_all_timesteps=False")
        self.model.eval()
        done = 0
        with torch.no_grad():
            for batch in self._batches(self.validation_set, sampler, device, num_workers, False, 0, 1):
                if done >= steps:
                    break
                if batch.shape[0] > batch_size:          # (the workspace and the sums above are sized for batch_size)
                    raise ValueError(f"validate(batch_size={batch_size}): the sampler draws runs of 8 clips per file and handed out a "
                                     f"batch of {batch.shape[0]}; use a batch size of at least 8")
                x = self._model_input(batch)
                if kernel_scores:
                    eng = self.model.engine_for(x)
                    eng.forward(x.float() if x.dim() == 4 else x[:, 0, :].contiguous().float())
                    eng.nce_eval(self.score_function is softplus_score_function, all_t, sums, ws, **self._score_kw())
                else:
                    predicted_z, targets, _, _ = self.model(x)
                    S, ld = _score_layout(self.score_function(predicted_z, targets), all_t)
                    _hip.call("cpc_nce_eval", _hip.ptr(S), _hip.ptr(sums), _hip.ptr(ws), batch_size, K, ld, 0, 1 if all_t else 0, 1)
                done += 1
        self.model.train()
        sums = sums / max(steps, 1)
        n = batch_size * K if all_t else batch_size
        step_losses, step_accuracy = sums[:K].clone(), sums[K:2 * K].clone()
        return step_losses, step_accuracy, float(sums[2 * K]), math.log(n) - step_losses

    def calc_test_task_data(self, batch_size=64, num_workers=1, use_ema=False):
        """Context vectors c of every item of the test-task set (reference :271-303); use_ema=True: from the averaged weights, as in
        validate()."""
        with self._ema_weights(use_ema):
            return self._calc_test_task_data(batch_size, num_workers)

    def extract_features(self, source, use_ema=False, **kw):
        """model.extract_features(source, **kw): z and c of every frame of every recording; use_ema=True: from the averaged weights,
        which take the model's place for the call as in validate() (the raw weights are back afterwards, bit for bit; ValueError
        when no average exists)."""
        with self._ema_weights(use_ema):
            return self.model.extract_features(source, **kw)

    def _calc_test_task_data(self, batch_size=64, num_workers=1):
        if self.test_task_set is None:
            print("No test task set")
        device = self._device()
        num_items = len(self.test_task_set)
        self.model.eval()
        task_data = torch.zeros(num_items, self.ar_size)
        task_labels = torch.zeros(num_items, dtype=torch.long)
        test_set = self.test_task_set
        if getattr(test_set, "device_batch", None) is not None and getattr(test_set, "device", None) is not None and test_set.labels:
            # samples in HBM: the batches a DataLoader would collate, in its order, each cut on the device
            loader = (test_set.device_batch(range(first, min(first + batch_size, num_items))) for first in range(0, num_items, batch_size))
        else:
            loader = torch.utils.data.DataLoader(test_set, batch_size=batch_size, num_workers=num_workers)
        with torch.no_grad():
            for step, (batch, labels) in enumerate(iter(loader)):
                _, _, _, c = self.model(self._model_input(batch.to(device)))
                task_data[step * batch_size:step * batch_size + c.shape[0], :] = c.cpu()
                task_labels[step * batch_size:step * batch_size + c.shape[0]] = labels.cpu()
        self.model.train()
        return task_data.numpy(), task_labels.numpy()

    def test_task(self, task_data, task_labels, evaluation_ratio=0.2):
        """Downstream probe of the context vectors (reference :305-350): a 128-64 ReLU MLP classifier trained with Adam
        (lr 1e-3, batch 64, 10 epochs) on a seeded 80/20 split; returns the evaluation accuracy after the last epoch.
        This is evaluation tooling outside the train-step hot path: a few thousand 256-vectors through
        a three-layer MLP, run with stock torch modules on ``self.device``."""
        num_items = task_data.shape[0]
        order = list(range(num_items))
        random.seed(0)
        random.shuffle(order)
        n_eval = int(num_items * evaluation_ratio)
        eval_idx, train_idx = order[:n_eval], order[n_eval:]
        files = getattr(self.test_task_set, "files", None)
        n_classes = len(files) if files is not None else int(task_labels.max()) + 1
        device = self._device()
        probe = torch.nn.Sequential(torch.nn.Linear(self.ar_size, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64), torch.nn.ReLU(),
                                    torch.nn.Linear(64, n_classes)).to(device)
        to_dev = lambda a, idx: torch.from_numpy(a[idx]).to(device)
        x_train, y_train = to_dev(task_data, train_idx), to_dev(task_labels, train_idx)
        x_eval, y_eval = to_dev(task_data, eval_idx), to_dev(task_labels, eval_idx)
        opt = torch.optim.Adam(probe.parameters(), lr=1e-3)
        accuracy = 0.0
        for epoch in range(10):
            for lo in range(0, y_train.shape[0], 64):
                loss = torch.nn.functional.cross_entropy(probe(x_train[lo:lo + 64]), y_train[lo:lo + 64])
                probe.zero_grad()
                loss.backward()
                opt.step()
            with torch.no_grad():
                hits = torch.eq(torch.argmax(probe(x_eval), dim=1), y_eval)
            accuracy = torch.sum(hits).item() / max(len(eval_idx), 1)
            if self.verbose:
                print("task accuracy after epoch", epoch, ":", accuracy)
        return accuracy


class DeterministicSampler(torch.utils.data.Sampler):
    """Shuffles range(len(data_source)) with a fixed seed: same order on every pass (reference :363-382)."""

    def __init__(self, data_source, seed=0):
        self.data_source = data_source
        self.seed = seed

    def __iter__(self):
        order = list(range(len(self.data_source)))
        random.seed(self.seed)
        random.shuffle(order)
        return iter(order)

    def __len__(self):
        return len(self.data_source)


def grad_mean_var(module):
    """{parameter name: [mean(grad), var(grad)]} (reference :385-391)."""
    out = {}
    for name, p in module.named_parameters():
        if p.grad is not None:
            out[name] = [torch.mean(p.grad).item(), torch.var(p.grad).item()]
    return out
