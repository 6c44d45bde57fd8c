"""Learnable and scheduled temperature of the cosine-similarity scores on the HIP path: the _dev normalise kernels against the existing
ones (bit for bit) and their per-row dots against float64, cpc_temperature_step / cpc_temperature_set against float64, and the engine /
trainer routes against the CPU oracle with
    scores = normalized_scores(p, t, exp(-s)),   s = log(1 / tau) a leaf tensor that requires grad
as its score function.  Shapes, fixtures and helpers are those of test_normalized_scores_gpu.py."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import test_normalized_scores_gpu as N
import test_temperature_host as H
from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction, TemperatureSchedule,
                                                           difference_score_function, grouped_negative_mask, linear_score_function,
                                                           sampled_negative_mask, softplus_score_function)
from cpc_audio_amd.engine import DeviceTemperature, FusedAdam
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = N.DEV
L_, F_, D_ = C.c_longlong, C.c_float, C.c_double
SENTINEL, U24 = N.SENTINEL, N.U24
NEW_ENTRY_POINTS = {"cpc_norm_rows_dev", "cpc_norm_rows_bwd_dev", "cpc_temperature_step", "cpc_temperature_set"}
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def _f32(x):
    return float(np.float32(x))


def _ulps(got, ref):
    """|got - ref| in units of the float32 spacing at ref."""
    return abs(float(got) - float(ref)) / float(np.spacing(np.float32(abs(ref))))


# ------------------------------------------------------------------------------------------ the _dev normalise kernels
def _both_kernels(Xd, Gd, rows, E, rpi, item, ld, off, scale, dt):
    """Runs cpc_norm_rows / cpc_norm_rows_bwd and their _dev counterparts on copies of the same sentinel-padded buffers, for the same
    scale value; returns (Y, inv, dX) of each pair and the dots."""
    code = _hip.dtype_code(dt)
    sc = torch.tensor([SENTINEL, scale, SENTINEL], device=DEV)          # the scale between two floats nobody may read as it
    out = []
    for dev in (False, True):
        Y = torch.full_like(Xd, SENTINEL)
        inv = torch.full((rows + 1,), SENTINEL, device=DEV)
        G = Gd.clone()
        dots = torch.full((rows + 1,), SENTINEL, device=DEV)
        tail = (rows, E, rpi, L_(item), L_(ld))
        if dev:
            _hip.call("cpc_norm_rows_dev", _hip.ptr(Xd, off), _hip.ptr(Y, off), _hip.ptr(inv), *tail, _hip.ptr(sc, 1), F_(1e-8), code)
            _hip.call("cpc_norm_rows_bwd_dev", _hip.ptr(Y, off), _hip.ptr(inv), _hip.ptr(G, off), _hip.ptr(dots), *tail, _hip.ptr(sc, 1),
                      F_(1e-8), code)
        else:
            _hip.call("cpc_norm_rows", _hip.ptr(Xd, off), _hip.ptr(Y, off), _hip.ptr(inv), *tail, F_(scale), F_(1e-8), code)
            _hip.call("cpc_norm_rows_bwd", _hip.ptr(Y, off), _hip.ptr(inv), _hip.ptr(G, off), *tail, F_(scale), F_(1e-8), code)
        out.append((Y, inv, G, dots))
    torch.cuda.synchronize()
    assert float(sc[0]) == SENTINEL and float(sc[1]) == _f32(scale) and float(sc[2]) == SENTINEL
    return out


def _bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                              b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def _check_dots(dots, Yrows, Grows, E, dt, what):
    """|dots - ref| <= (r + 1) 2^-24 sum_e |y_e g_e| per row, ref the float64 dot product of the stored values (r: the roundings of the
    kernel's sum, test_normalized_scores_gpu._sum_roundings; + 1: the product inside the first fma is exact, every later fma rounds
    once, and one is left for the reference's own conversion)."""
    y, g = Yrows.double().cpu(), Grows.double().cpu()
    ref, size = (y * g).sum(dim=1), (y * g).abs().sum(dim=1)
    err = (dots.double().cpu() - ref).abs()
    bound = (N._sum_roundings(E, dt) + 1) * U24 * size
    worst = (err / size.clamp_min(1e-300)).max().item()
    print(f"dots {what} {tuple(Yrows.shape)} {dt}: worst |dots - ref| / sum|y g| {worst:.3e} (bound {(N._sum_roundings(E, dt) + 1) * U24:.3e})")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,E,ld", [(r, e, e) for r, e in N.SHAPES] + N.PADDED)
def test_dev_kernels_equal_the_constant_kernels(rows, E, ld, dt):
    """Contiguous and padded rows: Y, inv and dX of the _dev kernels are the existing kernels' bits for the same scale, padding and the
    row behind the last keep their sentinel, and dots is <Y, G> per row (the zero row and the row under eps included: both are clamped
    rows, whose dots are written all the same)."""
    scale = 10.0
    Xc = N._rows(rows, E, dt, seed=rows * 10000 + E + ld)
    G0 = N._gradient_rows(Xc, dt, seed=E)

    def padded(values):
        buf = torch.full((rows + 1, ld), SENTINEL, dtype=dt)
        buf[:rows, :E] = values
        return buf.to(DEV)

    (Y0, inv0, dX0, _), (Y1, inv1, dX1, dots) = _both_kernels(padded(Xc), padded(G0), rows, E, 0, 0, ld, 0, scale, dt)
    assert _bits_equal(Y0, Y1) and _bits_equal(inv0, inv1) and _bits_equal(dX0, dX1)
    for buf in (Y1, dX1):
        assert (buf[:rows, E:] == SENTINEL).all() and (buf[rows] == SENTINEL).all()
    assert float(inv1[rows]) == SENTINEL and float(dots[rows]) == SENTINEL
    _check_dots(dots[:rows], Y1[:rows, :E], G0, E, dt, f"ld {ld}")
    if rows >= 3:
        assert float(inv1[1]) == N.INV_EPS and float(inv1[2]) == N.INV_EPS          # clamped rows ...
        assert float(dots[1]) == 0.0 and float(dots[2]) != 0.0                      # ... whose dots are written: zero row, sub-eps row


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_dev_kernels_through_the_top_layer_map(dt):
    """The K target rows of every item inside a top-layer-shaped buffer (rpi K, item Ltop E, from row T - K): the same bits as the
    existing kernels, untouched neighbours, dots in (b, k) order."""
    B, K, E, scale = 5, 3, 64, 2.5
    top, T, Ltop = N._top_layer(B, K, E, dt, seed=77)
    X = top[:, T - K:T, :].reshape(B * K, E)
    G0 = N._gradient_rows(X, dt, seed=5)
    G = torch.full_like(top, SENTINEL)
    G[:, T - K:T, :] = G0.view(B, K, E)
    (Y0, inv0, dX0, _), (Y1, inv1, dX1, dots) = _both_kernels(top.to(DEV), G.to(DEV), B * K, E, K, Ltop * E, E, (T - K) * E, scale, dt)
    assert _bits_equal(Y0, Y1) and _bits_equal(inv0, inv1) and _bits_equal(dX0, dX1)
    for buf in (Y1, dX1):
        assert (buf[:, :T - K] == SENTINEL).all() and (buf[:, T:] == SENTINEL).all()
    _check_dots(dots[:B * K], Y1[:, T - K:T, :].reshape(B * K, E), G0, E, dt, "top-layer map")
    assert float(dots[1]) == 0.0 and float(inv1[K]) == N.INV_EPS and float(dots[B * K]) == SENTINEL


# ------------------------------------------------------------------------------------------ cpc_temperature_step
def _tstate(tau=0.1, m=0.0, v=0.0):
    s, scale, t = DeviceTemperature.host_state(tau)
    return torch.tensor([s, scale, m, v, 0.0, t, 0.0, 0.0], device=DEV)


def _step(tstate, dots, lr, step, s_min, s_max, grad_scale=1.0, state=None, skip=None):
    _hip.call("cpc_temperature_step", _hip.ptr(tstate), _hip.ptr(dots), int(dots.numel()), F_(lr), F_(B1), F_(B2), F_(ADAM_EPS), step,
              _hip.ptr(state), F_(grad_scale), F_(s_min), F_(s_max), _hip.ptr(skip))


def _adam64(s, m, v, g, t, lr):
    """torch.optim.Adam's update of one scalar in Python floats (float64), with the betas and eps the kernel sees (C floats, as
    test_normalized_scores_gpu.EPS: float32(0.999) differs from 0.999 by 1.3e-8, which is 1.3e-5 of 1 - beta2)."""
    b1, b2, eps = _f32(B1), _f32(B2), _f32(ADAM_EPS)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    s = s - (lr / (1 - b1 ** t)) * m / (math.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return s, m, v


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 3072])
def test_temperature_step_against_float64(rows):
    """Five consecutive updates, new dots each: g within (ceil(rows / 256) + 8) 2^-24 sum|dots| of the float64 sum (a thread's chain,
    the eight levels of the tree; grad_scale 0.5 is exact), the change of s within 1e-5 relative of a float64 Adam on the same
    gradients, scale == exp(s) and tau == exp(-s) to one float32 unit in the last place, m and v carried in tstate[2:4]."""
    lr, gs = 1e-2, 0.5
    tstate = _tstate(0.1)
    s0 = float(tstate[0])
    s64, m64, v64 = s0, 0.0, 0.0
    gen = torch.Generator().manual_seed(rows)
    for t in range(1, 6):
        dots = (torch.randn(rows, generator=gen) + 0.3).to(DEV)
        _step(tstate, dots, lr, t, -3.0, 6.0, grad_scale=gs)
        row = tstate.cpu().double().tolist()
        ref = gs * dots.double().sum().item()
        bound = (math.ceil(rows / 256) + 8) * U24 * gs * dots.double().abs().sum().item()
        assert abs(row[4] - ref) <= bound, (t, row[4], ref, bound)
        s64, m64, v64 = _adam64(s64, m64, v64, row[4], t, _f32(lr))
        assert abs((row[0] - s0) - (s64 - s0)) <= 1e-5 * abs(s64 - s0), (t, row[0] - s0, s64 - s0)
        assert abs(row[2] - m64) <= 1e-5 * abs(m64) and abs(row[3] - v64) <= 1e-5 * abs(v64)
        assert _ulps(row[1], math.exp(row[0])) <= 1.0 and _ulps(row[5], math.exp(-row[0])) <= 1.0
        assert row[6] == 0.0 and row[7] == 0.0
    assert abs(s64 - s0) > 1e-2          # the five updates moved s by about lr each


def test_temperature_step_clamps_at_both_ends():
    s_min, s_max = 2.2, 2.4          # log(10) = 2.3026 lies inside
    for sign, edge in ((+1.0, s_min), (-1.0, s_max)):
        tstate = _tstate(0.1)
        dots = torch.full((300,), sign, device=DEV)
        _step(tstate, dots, 1.0, 1, s_min, s_max)          # Adam's first step moves s by lr = 1 against the gradient's sign
        row = tstate.cpu().tolist()
        assert row[0] == _f32(edge) and row[4] == sign * 300.0
        assert _ulps(row[1], math.exp(row[0])) <= 1.0 and _ulps(row[5], math.exp(-row[0])) <= 1.0


def test_temperature_step_skip_writes_nothing():
    before = torch.tensor([2.25, 9.5, 0.125, 0.25, -3.0, 0.105, 7.0, -7.0], device=DEV)
    tstate = before.clone()
    dots = torch.ones(17, device=DEV)
    _step(tstate, dots, 1e-2, 1, -3.0, 6.0, skip=torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(tstate, before)
    _step(tstate, dots, 1e-2, 1, -3.0, 6.0, skip=torch.zeros(1, device=DEV))          # a lowered flag lets the update through
    assert float(tstate[4]) == 17.0 and float(tstate[0]) != 2.25 and float(tstate[6]) == 7.0 and float(tstate[7]) == -7.0


def test_temperature_step_device_count_equals_host_count():
    """With the f32[4] of cpc_adam_dev — advanced by that call, as FusedAdam issues the two — the update is the host-count update of
    the same step number, bit for bit, over three steps (lr_scale 1: state[1] carries the whole step size)."""
    lr, n = 1e-2, 64
    p, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    m, v, state = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(4, device=DEV)
    host, dev = _tstate(0.2), _tstate(0.2)
    gen = torch.Generator().manual_seed(4)
    for t in range(1, 4):
        dots = torch.randn(500, generator=gen).to(DEV)
        _hip.call("cpc_adam_dev", _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), L_(n), F_(lr), F_(B1), F_(B2), F_(ADAM_EPS),
                  _hip.ptr(state), F_(1.0), None)
        _step(dev, dots, 1.0, 0, -3.0, 6.0, state=state)
        _step(host, dots, lr, t, -3.0, 6.0)
        assert int(state[0:1].view(torch.int32)) == t
        assert torch.equal(host, dev), (t, host.tolist(), dev.tolist())
    assert float(host[0]) != DeviceTemperature.host_state(0.2)[0]


# ------------------------------------------------------------------------------------------ cpc_temperature_set
def _set(tstate, sched, step, state=None, offset=0):
    _hip.call("cpc_temperature_set", _hip.ptr(tstate), *sched.abi_args(), L_(step), _hip.ptr(state), L_(offset))


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_temperature_set_against_the_host_schedule(kind):
    """Steps 0, mid, total_steps and beyond: tau, scale = 1 / tau and s = log(scale) within one float32 unit in the last place of
    TemperatureSchedule.value; m, v and the gradient cell are left alone; with an Adam state the step is offset + the device count."""
    sched = TemperatureSchedule(kind, 0.5, 0.07, 10)
    for step in (0, 3, 5, 10, 11, 10 ** 6):
        tstate = torch.tensor([0.0, 0.0, 0.25, 0.5, -2.0, 0.0, 0.0, 0.0], device=DEV)
        _set(tstate, sched, step)
        row = tstate.cpu().tolist()
        tau = sched.value(step)
        assert _ulps(row[5], tau) <= 1.0 and _ulps(row[1], 1.0 / tau) <= 1.0 and _ulps(row[0], math.log(row[1])) <= 1.0, (step, row, tau)
        assert row[2:5] == [0.25, 0.5, -2.0] and row[6:] == [0.0, 0.0]
    state = torch.zeros(4, device=DEV)
    state[0:1].copy_(torch.tensor([3], dtype=torch.int32).view(torch.float32))
    a, b = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    _set(a, sched, 999, state=state, offset=2)          # the step argument is ignored: 2 + 3
    _set(b, sched, 5)
    assert torch.equal(a, b) and float(a[5]) != 0.0


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_temperature_set_constant_schedule_is_the_constant(kind):
    """start == end == 0.1: exactly float32(1.0 / 0.1), the bit pattern the constant path passes, at every step."""
    sched = TemperatureSchedule(kind, 0.1, 0.1, 7)
    for step in (0, 3, 7, 50):
        tstate = torch.zeros(8, device=DEV)
        _set(tstate, sched, step)
        assert float(tstate[1]) == float(np.float32(1.0 / 0.1)) == C.c_float(1.0 / 0.1).value
        assert float(tstate[5]) == _f32(0.1)


def test_argument_refusals_with_device_pointers():
    """All -22 cases of the four entry points (test_temperature_host.py's tables, which need no GPU, run here too, next to a good call
    on real buffers so that the refusals are seen to come from the arguments)."""
    H.test_temperature_step_argument_checks_without_a_gpu()
    H.test_temperature_set_argument_checks_without_a_gpu()
    H.test_norm_rows_dev_argument_checks_without_a_gpu("cpc_norm_rows_dev", 3)
    H.test_norm_rows_dev_argument_checks_without_a_gpu("cpc_norm_rows_bwd_dev", 4)
    tstate, dots = _tstate(0.1), torch.ones(4, device=DEV)
    lib = _hip.lib()
    assert lib.cpc_temperature_step(_hip.ptr(tstate), _hip.ptr(dots), 4, 1e-3, B1, B2, ADAM_EPS, 1, None, 1.0, -1.0, 4.0, None,
                                    _hip.stream_ptr()) == 0
    assert lib.cpc_temperature_step(_hip.ptr(tstate), _hip.ptr(dots), 4, 1e-3, B1, B2, ADAM_EPS, 1, None, 1.0, 4.0, -1.0, None,
                                    _hip.stream_ptr()) == -22
    assert lib.cpc_temperature_set(_hip.ptr(tstate), 1, D_(0.5), D_(0.1), L_(10), L_(0), None, L_(0), _hip.stream_ptr()) == 0
    assert lib.cpc_temperature_set(_hip.ptr(tstate), 2, D_(0.5), D_(0.1), L_(10), L_(0), None, L_(0), _hip.stream_ptr()) == -22
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ engine
TAU, REG = 0.1, 0.5          # d loss / d s at the fixture: 0.60 (default branch) and 1.71 (all timesteps), from the CPU oracle


def _s_leaf(tau):
    return torch.tensor(DeviceTemperature.host_state(tau)[0], dtype=torch.float32, requires_grad=True)


def _learnable_oracle(params, V, K, s, **kw):
    ot = O.OracleTrainer(params, V, K, score="linear", **kw)
    ot.score = lambda p, t: N.normalized_scores(p, t, torch.exp(-s))
    return ot


def _engine_step(model, x, all_t, temp, **kw):
    """loss_and_grads + FusedAdam.step at lr 0 (the parameters stay, the temperature's gradient lands in tstate[4])."""
    model.train()
    model._flatten_parameters(DEV)
    opt = FusedAdam(model, lr=0.0, temperature=temp)
    model.link_grads()
    eng = model.engine(x.shape[0], x.shape[1])
    with N._Spy() as spy:
        out = eng.loss_and_grads(x.to(DEV).contiguous(), softplus=False, regularization=REG, all_timesteps=all_t, score="normalized",
                                 temperature=temp, **kw)
        opt.step()
    torch.cuda.synchronize()
    return eng, out, spy.names


@pytest.mark.parametrize("all_t", [False, True])
def test_engine_learnable_gradients_against_oracle(golden_dir, all_t):
    """One fp32 step with a DeviceTemperature: loss within 1e-4, every parameter gradient within 1e-3 relative L2, and tstate[4] within
    1e-3 relative of the oracle's s.grad (the project's f32 tolerances); |s.grad| > 1e-3, so that the check is not vacuous."""
    g, meta, data, params = N._small(golden_dir)
    model = N._small_model(g, meta, "fp32")
    x = data[:meta["B"]]
    temp = DeviceTemperature(TAU, "learnable", device=DEV)
    eng, out, names = _engine_step(model, x, all_t, temp)
    assert names.count("cpc_norm_rows_dev") == 1 and names.count("cpc_norm_rows_bwd_dev") == 1 and names.count("cpc_temperature_step") == 1
    assert names.count("cpc_norm_rows") == 1 and names.count("cpc_norm_rows_bwd") == 1          # the target rows: scale 1, as before
    s = _s_leaf(TAU)
    loss, smax, grads = _learnable_oracle(params, meta["V"], meta["K"], s, all_timesteps=all_t, regularization=REG).loss_and_grads(x)
    assert abs(float(s.grad)) > 1e-3
    assert abs(float(out[0]) - float(loss)) < 1e-4 * abs(float(loss)), (float(out[0]), float(loss))
    for name, ref in grads.items():
        assert ref.abs().max() > 0 and N._rel_l2(model._grad[name], ref) < 1e-3, name
    got = float(temp.tstate[4])
    print(f"d loss / d s all_timesteps={all_t}: engine {got:.6f}, oracle {float(s.grad):.6f}")
    assert abs(got - float(s.grad)) < 1e-3 * abs(float(s.grad))
    # lr 0: s stays, and tau is formed again from it (exp(-s), one rounding: float32(0.1) or its neighbour)
    assert float(temp.tstate[0]) == float(s.detach()) and _ulps(temp.value(), TAU) <= 1.0


@pytest.mark.parametrize("selection", ["sampled", "grouped"])
def test_engine_learnable_with_selected_negatives(golden_dir, selection):
    """Default branch with sampled / grouped negatives: loss, dpred and d loss / d s vs float64 autograd of the definition on the
    engine's own predictions and targets (1e-4 / 1e-3 / 1e-3), and the target-row gradient in the top layer (1e-3): the oracle has no
    candidate selection, so the parameter gradients are checked where the selection enters them, at the loss chain's two outputs."""
    g, meta, data, params = N._small(golden_dir)
    model = N._small_model(g, meta, "fp32")
    B, K = meta["B"], meta["K"]
    if selection == "sampled":
        kw, mask = {"negatives": (3, 41, 7)}, sampled_negative_mask(B, K, 3, 41, 7)
    else:
        kw = {"negative_groups": (torch.tensor(N.GROUPS, dtype=torch.int32, device=DEV), "other")}
        mask = grouped_negative_mask(N.GROUPS, K, "other")
    temp = DeviceTemperature(TAU, "learnable", device=DEV)
    eng, out, names = _engine_step(model, data[:B], False, temp, **kw)
    assert ("cpc_nce_loss_sampled" if selection == "sampled" else "cpc_nce_loss_grouped") in names and "cpc_nce_loss" not in names
    pred, targ, _, _ = eng.outputs()
    p64, t64 = pred.double().cpu().requires_grad_(True), targ.double().cpu().requires_grad_(True)
    s = _s_leaf(TAU).double().detach().requires_grad_(True)
    sp = torch.diagonal(N.normalized_scores(p64, t64, torch.exp(-s)), dim1=1, dim2=3).permute(2, 0, 1)
    loss = N.masked_loss(sp, mask, REG)
    dp, dt_, ds = torch.autograd.grad(loss, (p64, t64, s))
    assert abs(float(ds)) > 1e-3
    assert abs(float(out[0]) - float(loss.detach())) < 1e-4 * abs(float(loss.detach()))
    assert N._rel_l2(eng.dpred.view(B, K, -1), dp) < 1e-3
    T, Ltop = eng.T, eng.geo.alloc[-1]
    assert N._rel_l2(eng.dact[-1].view(B, Ltop, eng.E)[:, T - K:T, :], dt_.transpose(1, 2)) < 1e-3
    assert abs(float(temp.tstate[4]) - float(ds)) < 1e-3 * abs(float(ds)), (float(temp.tstate[4]), float(ds))


def _fused_route_model():
    """The smallest shape fused_scores_ok() accepts (bf16, B K = 256, E = 128), as test_normalized_scores_gpu builds it."""
    C_, H_, V, K, B = 128, 64, 4, 4, 64
    L = 465 + (V + K - 1) * 160
    torch.manual_seed(11)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(C_, H_), enc_size=C_, ar_size=H_, visible_steps=V, prediction_steps=K,
                                       compute_dtype="bf16")
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("weight") and n.startswith("encoder"):
                p.mul_(2.0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(3)) * 0.5
    return model.to(DEV), state, x, V, K


def test_engine_learnable_fused_all_timesteps_route():
    """The fused all-timesteps route (cpc_score_lse on the normalised operands) exists in bf16 storage only, so the bounds are the bf16
    ones of test_engine_normalized_fused_all_timesteps_route (loss 1e-3, parameter gradients 0.12) and 0.12 for the scalar.
    Measured on MI355X: see DESIGN.md, "Learnable and scheduled temperature"."""
    model, state, x, V, K = _fused_route_model()
    temp = DeviceTemperature(TAU, "learnable", device=DEV)
    timer = _hip.KernelTimer(only=["score_lse<bf16,256>"])
    _hip.set_timer(timer)
    try:
        eng, out, names = _engine_step(model, x, True, temp)
        ran = timer.summary()
    finally:
        _hip.set_timer(None)
    assert eng.fused_scores_ok() and ran["score_lse<bf16,256>"][0] == 1 and "cpc_norm_rows_bwd_dev" in names
    s = _s_leaf(TAU)
    loss, smax, grads = _learnable_oracle(state, V, K, s, all_timesteps=True, regularization=REG).loss_and_grads(x)
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((N._rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    srel = abs(float(temp.tstate[4]) - float(s.grad)) / abs(float(s.grad))
    print(f"fused all-timesteps route, learnable: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]}), "
          f"d loss / d s {float(temp.tstate[4]):.5f} vs {float(s.grad):.5f} (rel {srel:.2e})")
    assert abs(float(s.grad)) > 1e-3
    assert rel < 1e-3 and worst[0] < 0.12 and srel < 0.12


@pytest.mark.parametrize("all_t", [False, True])
def test_engine_learnable_bf16(golden_dir, all_t):
    """bf16 storage, one step vs the f32 oracle: loss within 1e-3, parameter gradients within 0.12 (test_engine_difference_bf16's
    bounds), the scalar's gradient within 0.12 relative.  Measured on MI355X: see DESIGN.md, "Learnable and scheduled temperature"."""
    g, meta, data, params = N._small(golden_dir)
    model = N._small_model(g, meta, "bf16")
    x = data[:meta["B"]]
    temp = DeviceTemperature(TAU, "learnable", device=DEV)
    eng, out, names = _engine_step(model, x, all_t, temp)
    s = _s_leaf(TAU)
    loss, smax, grads = _learnable_oracle(params, meta["V"], meta["K"], s, all_timesteps=all_t, regularization=REG).loss_and_grads(x)
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((N._rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    srel = abs(float(temp.tstate[4]) - float(s.grad)) / abs(float(s.grad))
    print(f"bf16 learnable all_timesteps={all_t}: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]}), "
          f"d loss / d s {float(temp.tstate[4]):.5f} vs {float(s.grad):.5f} (rel {srel:.2e})")
    assert rel < 1e-3
    assert worst[0] < 0.12, worst
    assert srel < 0.12


# ------------------------------------------------------------------------------------------ trainer
class _TLogger(N._Logger):
    def __init__(self):
        super().__init__()
        self.temperature_meter = N._Meter()


def _run(golden_dir, fn, steps, lr=1e-3, use_graph=False, first=0, seed=True, dtype="fp32", data=None, model=None, epochs=10, **attrs):
    g, meta, data0, params = N._small(golden_dir)
    data = data0 if data is None else data
    model = N._small_model(g, meta, dtype) if model is None else model
    logger = _TLogger()
    tr = N._trainer(model, data, meta, logger, fn)
    tr.use_graph = use_graph
    for k, v in attrs.items():
        setattr(tr, k, v)
    if seed:
        random.seed(5)
    with N._Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=epochs, lr=lr, continue_training_at_step=first, num_workers=0, max_steps=first + steps)
    torch.cuda.synchronize()
    return tr, logger, spy.names


def test_trainer_learnable_trajectory(golden_dir):
    """Five fp32 trainer steps at lr 1e-2: s_5 - s_0 within 1e-3 relative of the oracle's own Adam on s (clamped to the bounds), the
    parameters within the bounds of the normalized trainer test, and the logged temperatures are tstate[5] step by step."""
    g, meta, data, params = N._small(golden_dir)
    steps, lr = 5, 1e-2
    random.seed(5)          # the trainer draws a new shuffle per epoch from the same generator: four batches an epoch, five steps
    sampler = FileBatchSampler([data.shape[0]], meta["B"], 1, True, verbose=False)
    batches = [list(b) for _ in range(2) for b in sampler]
    fn = NormalizedScoreFunction(TAU, learnable=True)
    tr, logger, names = _run(golden_dir, fn, steps, lr=lr)
    assert names.count("cpc_temperature_step") == steps and names.count("cpc_norm_rows_dev") == steps
    temp = tr._temperature
    assert temp is fn.device_temperature and tr.last_optimizer.temperature is temp
    s = _s_leaf(TAU)
    s0 = float(s.detach())
    ot = _learnable_oracle(params, meta["V"], meta["K"], s, regularization=REG, lr=lr)
    m, v = torch.zeros(()), torch.zeros(())
    taus = []
    for i in range(steps):
        s.grad = None
        loss, smax = ot.step(data[batches[i]])
        if i == 0:          # (later losses see the parameters of two Adam runs at lr 1e-2; the issue bounds s and the parameters)
            assert abs(logger.loss_meter.values[i] - loss) < 2e-4 * abs(loss), (i, logger.loss_meter.values[i], loss)
        with torch.no_grad():
            O.adam_update(s, s.grad, m, v, i + 1, lr)
            s.clamp_(math.log(1.0 / 1.0), math.log(1.0 / 0.01))
        taus.append(math.exp(-float(s)))
    got = float(temp.tstate[0]) - s0
    print(f"s_5 - s_0: trainer {got:.6f}, oracle {float(s) - s0:.6f}; temperatures {logger.temperature_meter.values}")
    assert abs(float(s) - s0) > 1e-2
    assert abs(got - (float(s) - s0)) < 1e-3 * abs(float(s) - s0)
    assert len(logger.temperature_meter.values) == steps and tr.last_temperature == logger.temperature_meter.values[-1] == temp.value()
    assert max(abs(a - b) / b for a, b in zip(logger.temperature_meter.values, taus)) < 1e-3
    assert fn.current_temperature() == temp.value()          # called on tensors, the function uses the learned value
    for k, val in tr.model.state_dict().items():
        ref = ot.params[k].detach()
        err = (val.cpu() - ref).abs()
        assert err.max().item() <= 2 * lr * steps * 1.01 + 1e-6, k
        tight = err <= 0.05 * lr * steps + 1e-4 * ref.abs()
        assert tight.float().mean().item() > 0.97, (k, tight.float().mean().item())


def _state(tr):
    return ({n: p.detach().clone() for n, p in tr.model.named_parameters()},
            None if tr._temperature is None else tr._temperature.tstate.clone())


@pytest.mark.parametrize("mode", ["learnable", "scheduled"])
def test_graphed_step_equals_eager_bit_for_bit(golden_dir, mode):
    """trainer.use_graph: three steps replayed from the captured graph (the normalise, tick and temperature-step launches captured
    once) give the eager run's losses, parameters and tstate bit for bit."""
    make = {"learnable": lambda: NormalizedScoreFunction(TAU, learnable=True),
            "scheduled": lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("cosine", 0.3, 0.05, 4))}[mode]
    entry = "cpc_temperature_step" if mode == "learnable" else "cpc_temperature_set"
    results = []
    for use_graph in (False, True):
        tr, logger, names = _run(golden_dir, make(), 3, lr=1e-2, use_graph=use_graph)
        assert names.count(entry) == (1 if use_graph else 3) and names.count("cpc_norm_rows_dev") == (1 if use_graph else 3)
        results.append((logger.loss_meter.values, logger.temperature_meter.values, *_state(tr)))
    (l0, t0, p0, s0), (l1, t1, p1, s1) = results
    assert len(l0) == 3 and l0 == l1 and t0 == t1 and len(set(t0)) == 3          # the value moved every step
    assert torch.equal(s0[:6], s1[:6]), (s0.tolist(), s1.tolist())
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
    if mode == "scheduled":
        sched = TemperatureSchedule("cosine", 0.3, 0.05, 4)
        assert all(_ulps(t, sched.value(i)) <= 1.0 for i, t in enumerate(t0))


@pytest.mark.parametrize("use_graph", [False, True])
def test_constant_schedule_is_the_constant_temperature(golden_dir, use_graph):
    """A schedule with start == end == 0.1 gives losses and parameters bit-identical to NormalizedScoreFunction(0.1) over three steps."""
    ref, ref_log, ref_names = _run(golden_dir, NormalizedScoreFunction(0.1), 3, use_graph=use_graph)
    assert not NEW_ENTRY_POINTS & set(ref_names)
    tr, logger, names = _run(golden_dir, NormalizedScoreFunction(schedule=TemperatureSchedule("linear", 0.1, 0.1, 2)), 3,
                             use_graph=use_graph)
    assert "cpc_temperature_set" in names and "cpc_norm_rows_dev" in names and "cpc_temperature_step" not in names
    assert logger.loss_meter.values == ref_log.loss_meter.values and len(ref_log.loss_meter.values) == 3
    for (k, a), (k0, b) in zip(tr.model.state_dict().items(), ref.model.state_dict().items()):
        assert k == k0 and torch.equal(a, b), k
    assert logger.temperature_meter.values == [_f32(0.1)] * 3


@pytest.mark.parametrize("fn", ["softplus", "linear", "difference", "normalized"])
def test_default_steps_reach_no_new_entry_point(golden_dir, fn):
    """With a float temperature and with the three reference score functions, none of the four new entry points is reached and
    nothing new is allocated."""
    score = {"softplus": softplus_score_function, "linear": linear_score_function, "difference": difference_score_function,
             "normalized": NormalizedScoreFunction(0.1)}[fn]
    tr, logger, names = _run(golden_dir, score, 2)
    assert len(logger.loss_meter.values) == 2 and not NEW_ENTRY_POINTS & set(names)
    assert names.count("cpc_norm_rows") == (4 if fn == "normalized" else 0)
    assert tr._temperature is None and tr.last_temperature is None and logger.temperature_meter.values == []
    assert tr.last_optimizer.temperature is None and "temperature" not in tr.last_optimizer.state_dict()
    eng = tr.model.engine(6, N._small(golden_dir)[2].shape[1], DEV)
    norm = getattr(eng, "_norm", None)
    assert (norm is None) if fn != "normalized" else (norm.dots is None)


@pytest.mark.parametrize("mode", ["learnable", "scheduled"])
def test_resumed_run_is_the_uninterrupted_run(golden_dir, mode):
    """Two steps, last_optimizer.state_dict() (which carries "temperature") through optimizer_state into a new trainer on a copy of the
    model with continue_training_at_step=2, one more step: parameters and tstate are those of three steps in one run, bit for bit."""
    g, meta, data, params = N._small(golden_dir)
    data = data[:2 * meta["B"]]          # two batches per epoch: the second call's sampler starts where the second epoch does
    make = {"learnable": lambda: NormalizedScoreFunction(TAU, learnable=True),
            "scheduled": lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("linear", 0.3, 0.05, 4))}[mode]
    tr_a, log_a, _ = _run(golden_dir, make(), 3, lr=1e-2, data=data)
    tr_b, log_b, _ = _run(golden_dir, make(), 2, lr=1e-2, data=data)
    saved = tr_b.last_optimizer.state_dict()
    assert saved["temperature"]["mode"] == mode
    sampler_state = random.getstate()
    model_c = N._small_model(g, meta, "fp32")
    model_c.load_state_dict({k: v.detach().clone() for k, v in tr_b.model.state_dict().items()})
    random.setstate(sampler_state)
    tr_c, log_c, _ = _run(golden_dir, make(), 1, lr=1e-2, data=data, model=model_c, first=2, seed=False, optimizer_state=saved)
    assert log_b.loss_meter.values + log_c.loss_meter.values == log_a.loss_meter.values and tr_c.last_optimizer.t == 3
    assert torch.equal(tr_c.model._flat_param, tr_a.model._flat_param)
    assert torch.equal(tr_c._temperature.tstate, tr_a._temperature.tstate), (tr_c._temperature.tstate.tolist(), tr_a._temperature.tstate.tolist())
    assert log_c.temperature_meter.values == log_a.temperature_meter.values[2:]


def test_gradient_clipping_leaves_the_scalar_gradient_alone(golden_dir):
    """max_grad_norm beside a learnable temperature (one step at lr 0, a bound far below the norm): the norm before clipping and the
    coefficient are those of the parameters' gradient alone (the oracle's, 1e-3), and tstate[4] is the oracle's d loss / d s, not
    scaled by the coefficient.  The step's values travel in one pinned buffer: loss, norm, coefficient and temperature."""
    g, meta, data, params = N._small(golden_dir)
    batches = N._batches(data, meta)
    max_norm = 1e-3
    tr, logger, names = _run(golden_dir, NormalizedScoreFunction(TAU, learnable=True), 1, lr=0.0, max_grad_norm=max_norm)
    assert names.count("cpc_grad_norm") == 1 and names.count("cpc_adam_clip") == 1 and names.count("cpc_temperature_step") == 1
    s = _s_leaf(TAU)
    loss, smax, grads = _learnable_oracle(params, meta["V"], meta["K"], s, regularization=REG).loss_and_grads(data[batches[0]])
    norm = math.sqrt(sum(float(v.double().pow(2).sum()) for v in grads.values()))
    clip_state = tr.last_optimizer.clip_state.cpu().tolist()
    coef = max_norm / (norm + 1e-6)
    assert coef < 0.5, (norm, coef)          # the clipping is active
    assert abs(clip_state[0] - norm) < 1e-3 * norm and abs(clip_state[1] - coef) < 1e-3 * coef and clip_state[2] == 0.0
    assert tr.last_grad_norm == clip_state[0]
    got = float(tr._temperature.tstate[4])
    assert abs(float(s.grad)) > 1e-3 and abs(got - float(s.grad)) < 1e-3 * abs(float(s.grad)), (got, float(s.grad), coef)
    assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss))
    assert len(logger.temperature_meter.values) == 1 and _ulps(logger.temperature_meter.values[0], TAU) <= 1.0


def test_gradient_clipping_with_a_scheduled_temperature(golden_dir):
    """Two clipped steps with a scheduled temperature on the engine route: norm, coefficient and temperature of every step arrive."""
    sched = TemperatureSchedule("linear", 0.3, 0.1, 4)
    tr, logger, names = _run(golden_dir, NormalizedScoreFunction(schedule=sched), 2, lr=1e-3, max_grad_norm=1e-3)
    assert names.count("cpc_temperature_set") == 2 and names.count("cpc_adam_clip") == 2
    assert [_ulps(t, sched.value(i)) <= 1.0 for i, t in enumerate(logger.temperature_meter.values)] == [True, True]
    assert tr.last_grad_norm > 1e-3 and all(math.isfinite(v) for v in logger.loss_meter.values)


@pytest.mark.parametrize("beside", ["adamw_schedule", "lamb", "ema"])
def test_learnable_temperature_beside_the_other_optimizer_options(golden_dir, beside):
    """Two steps with weight decay and an lr schedule, with LAMB and with the EMA of the weights: the scalar's update follows every
    step's update, takes the step's scheduled rate, and gets no decay and no trust ratio (its Adam is checked against float64 from
    the gradients the device recorded, at the rate the trainer logged)."""
    from cpc_audio_amd.contrastive_estimation_training import LRSchedule
    lr = 1e-2
    attrs, entry = {
        "adamw_schedule": (dict(weight_decay=0.1, lr_schedule=LRSchedule("linear", warmup_steps=0, total_steps=4)), "cpc_adamw"),
        "lamb": (dict(trust_ratio=True, weight_decay=0.01), "cpc_lamb"),
        "ema": (dict(ema_decay=0.9), "cpc_ema"),
    }[beside]
    s0 = DeviceTemperature.host_state(TAU)[0]

    class Log(_TLogger):
        def __init__(self):
            super().__init__()
            self.lr_meter = N._Meter()

    s64, m64, v64 = s0, 0.0, 0.0
    for steps in (1, 2):          # the state after one step and after two: the gradient of each step is read from tstate[4]
        g, meta, data, params = N._small(golden_dir)
        model = N._small_model(g, meta, "fp32")
        logger = Log()
        tr = N._trainer(model, data, meta, logger, NormalizedScoreFunction(TAU, learnable=True))
        for k, v in attrs.items():
            setattr(tr, k, v)
        random.seed(5)
        with N._Spy() as spy:
            tr.train(batch_size=meta["B"], epochs=1, lr=lr, num_workers=0, max_steps=steps)
        torch.cuda.synchronize()
        assert spy.names.count("cpc_temperature_step") == steps and entry in spy.names
        row = tr._temperature.tstate.cpu().double().tolist()
        s64, m64, v64 = _adam64(s64, m64, v64, row[4], steps, _f32(logger.lr_meter.values[-1]))
        assert abs((row[0] - s0) - (s64 - s0)) <= 1e-5 * abs(s64 - s0), (beside, steps, row[0] - s0, s64 - s0)
        assert all(math.isfinite(x) for x in logger.loss_meter.values) and len(logger.temperature_meter.values) == steps
    assert abs(s64 - s0) > 1e-3


@pytest.mark.parametrize("case", ["lr_scale", "lr_schedule"])
def test_graphed_step_with_a_scaled_or_scheduled_rate(golden_dir, case):
    """Where the scalar's step size is not the parameters' own — temperature_lr_scale != 1, or an lr schedule — the captured step
    forms it on the device as state[1] * lr_scale in float32 (state[1] = lr factor / (1 - beta1^t), rounded once), the eager step on
    the host as one rounding of lr factor lr_scale / (1 - beta1^t): up to three float32 roundings apart, 1.8e-7 relative per step.
    Three steps: the change of s within 1e-5 relative, losses within 1e-6 and parameters within 1e-5 (the bounds of the graphed-step
    test of the constant temperature)."""
    from cpc_audio_amd.contrastive_estimation_training import LRSchedule
    make = lambda: NormalizedScoreFunction(TAU, learnable=True, temperature_lr_scale=0.3 if case == "lr_scale" else 1.0)
    attrs = {} if case == "lr_scale" else dict(lr_schedule=LRSchedule("cosine", warmup_steps=2, total_steps=6))
    s0 = DeviceTemperature.host_state(TAU)[0]
    results = []
    for use_graph in (False, True):
        tr, logger, names = _run(golden_dir, make(), 3, lr=1e-2, use_graph=use_graph, **attrs)
        assert names.count("cpc_temperature_step") == (1 if use_graph else 3)
        results.append((logger.loss_meter.values, *_state(tr)))
    (l0, p0, t0), (l1, p1, t1) = results
    d0, d1 = float(t0[0]) - s0, float(t1[0]) - s0
    print(f"{case}: s_3 - s_0 eager {d0:.8f}, captured {d1:.8f}")
    assert abs(d0) > 1e-3 and abs(d1 - d0) <= 1e-5 * abs(d0)
    assert max(abs(a - b) / abs(a) for a, b in zip(l0, l1)) < 1e-6
    for n in p0:
        assert N._rel(p1[n], p0[n]) < 1e-5, n


def test_trainer_keeps_the_temperature_across_train_calls(golden_dir):
    """A second train() goes on from the learned value (the reference's train() starts Adam over; the scalar's moments stay with it)."""
    fn = NormalizedScoreFunction(TAU, learnable=True)
    tr, logger, _ = _run(golden_dir, fn, 2, lr=1e-2)
    kept, after_two = tr._temperature, tr._temperature.value()
    random.seed(5)
    tr.train(batch_size=6, epochs=1, lr=1e-2, continue_training_at_step=2, num_workers=0, max_steps=3)
    torch.cuda.synchronize()
    assert tr._temperature is kept and kept.value() != after_two and after_two != _f32(TAU)


def test_validate_reads_the_learned_temperature(golden_dir):
    """validate() after training scores with the device's value: per-step losses, accuracies and the mean score vs the oracle's
    validation terms at tstate[5] on the trained parameters (the validate test's bounds, 1e-4)."""
    g = N._load(golden_dir, "validate.npz")
    meta = json.load(open(os.path.join(golden_dir, "validate.json")))
    data = torch.from_numpy(g["data"])
    model = N._small_model(g, meta, "fp32")
    B, K, V = meta["B"], meta["K"], meta["V"]
    fn = NormalizedScoreFunction(TAU, learnable=True)
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, counts=meta["counts"], device=DEV),
                                      validation_set=TensorAudioDataset(data, counts=meta["counts"], device=DEV), device=DEV,
                                      regularization=REG, score_function=fn, prediction_steps=K, ar_size=meta["H"])
    tr.verbose = False
    random.seed(5)
    tr.train(batch_size=B, epochs=10, lr=1e-2, num_workers=0, max_steps=3)
    tau = tr._temperature.value()
    assert abs(tau - TAU) > 1e-3 * TAU
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    with N._Spy() as spy:
        losses, acc, score, mi = tr.validate(batch_size=B, num_workers=0)
    lists = O.file_batch_sampler(meta["counts"], B, 8, True, seed=0)
    assert spy.names.count("cpc_norm_rows_dev") == len(lists) and "cpc_temperature_step" not in spy.names
    assert tr._temperature.value() == tau          # an evaluation changes nothing
    want_l, want_a, want_s = 0.0, 0.0, 0.0
    for idx in lists:
        pred, targ, _, _ = O.cpc_forward(data[idx].unsqueeze(1), params, V, K, training=False)
        pl, pa, ms = O.validation_terms(N.normalized_scores(pred.double(), targ.double(), tau), False)
        want_l, want_a, want_s = want_l + pl, want_a + pa, want_s + float(ms)
    n = len(lists)
    assert N._rel(losses, want_l / n) < 1e-4
    assert (acc.cpu().double() - want_a / n).abs().max().item() < 1e-4
    assert abs(score - want_s / n) < 1e-4 * max(1.0, abs(want_s / n))


def test_scalogram_trainer_step_with_a_learnable_temperature(golden_dir):
    """ScalogramCPCEngine, default branch, one trainer step at lr 0 with a learnable temperature: loss, all parameter gradients and
    the scalar's gradient vs the oracle, as the normalized scalogram test does."""
    g = N._load(golden_dir, "scalogram_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    B, K, H_, V = meta["B"], meta["K"], meta["H"], meta["V"]
    pre, model, blocks = N._scalogram_model(g, meta)
    model.train()
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    data = torch.from_numpy(g["data"])
    logger = _TLogger()
    fn = NormalizedScoreFunction(TAU, learnable=True)
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.1, score_function=fn, prediction_steps=K, ar_size=H_, preprocessing=pre)
    tr.verbose = False
    random.seed(91)
    idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
    random.seed(91)
    with N._Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    assert spy.names.count("cpc_norm_rows_dev") == 1 and spy.names.count("cpc_norm_rows_bwd_dev") == 1
    assert spy.names.count("cpc_temperature_step") == 1
    with torch.no_grad():
        scal = pre(data[idx].to(DEV).unsqueeze(1)).cpu()
    oblocks = [dict(b) for b in blocks]
    oblocks[0]["in_channels"] = 2
    s = _s_leaf(TAU)
    ot = _learnable_oracle(params, V, K, s, regularization=0.1, lr=0.0, scalogram=oblocks)
    loss, smax, grads = ot.loss_and_grads(scal)
    assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss)), (logger.loss_meter.values, float(loss))
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for name, ref in grads.items():
        got = dict(model.named_parameters())[name].grad.double().cpu()
        if ref.abs().max().item() < 1e-6 * largest:
            assert got.abs().max().item() < 1e-5 * largest, name
            continue
        assert N._rel_l2(got, ref) < 1e-3, name
    got = float(tr._temperature.tstate[4])
    print(f"scalogram engine d loss / d s: {got:.6f}, oracle {float(s.grad):.6f}")
    assert abs(float(s.grad)) > 1e-3 and abs(got - float(s.grad)) < 1e-3 * abs(float(s.grad))
    assert len(logger.temperature_meter.values) == 1 and _ulps(logger.temperature_meter.values[0], TAU) <= 1.0
