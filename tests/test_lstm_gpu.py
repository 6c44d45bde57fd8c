"""LSTM context (AudioLSTMModel) on the GPU: the recurrence kernels cpc_lstm_fwd / cpc_lstm_bwd (with cpc_lstm_tape_elems) step by step
against the float64 reference of tests/lstm_reference.py, and the routes that use them: stand-alone AudioLSTMModel calls, whole models in
both storage types against the composed float64 reference, train / validate / calc_test_task_data, a graphed step, trainer options
against the generic route, the scalogram engine, and the refusals.

Tolerances: f32 kernels 2e-5 (hidden states) and 5e-5 (gate blocks) per step, bf16 kernels 4 x the per-step error of the bf16 emulation
(lstm_reference.lstm_reference); models the bounds of test_gru_wide_gpu.py / test_gru_stacked_gpu.py, restated where used.  None was
obtained by running the code under test.
"""
import contextlib
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioLSTMModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,  # noqa: E402
                                                           softplus_score_function)
from oracle import cpc_oracle as O  # noqa: E402
import lstm_reference as L  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
SCORE = {"softplus": softplus_score_function, "linear": linear_score_function}
GUARD = 64           # sentinel elements behind every output
SENT = -7.5          # (exact in bf16)


def name(dt):
    return "f32" if dt == F32 else "bf16"


def host(t):
    return t.detach().double().cpu()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _rel(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


def padded(B, per_item, dt):
    """An output buffer for B items of per_item elements: NaN where the kernel must write, then the sentinel over the rows of the items
    B .. 16 ceil(B/16) - 1 (the workgroup's masked batch rows) and GUARD more elements.  Returns (whole buffer, view of the B items)."""
    n, pad = B * per_item, (-B % 16) * per_item
    buf = torch.full((n + pad + GUARD,), float("nan"), device=DEV, dtype=dt)
    buf[n:] = SENT
    return buf, buf[:n]


def intact(buf, n):
    return bool((buf[n:].float() == SENT).all())


# ======================================================================================================================= kernels
def _frags(w_hh, H, dt):
    code = _hip.dtype_code(dt)
    dW = w_hh.to(DEV).float().contiguous()
    wfrag = torch.empty(4 * H * H, device=DEV, dtype=dt)
    wTfrag = torch.empty(4 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wfrag), 4 * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wTfrag), H, 4 * H, H, 1, code)
    return wfrag, wTfrag


def _lstm_fwd(dt, B, V, H, gi, wfrag, b_hh, h0=None, c0=None):
    """cpc_lstm_fwd on device tensors; returns Hall, tape, h_out, cell_out (device views) after the guard checks."""
    code = _hip.dtype_code(dt)
    nt = int(_hip.lib().cpc_lstm_tape_elems(B, V, H, code))
    assert nt == B * V * 6 * H
    hb, Hall = padded(B, (V + 1) * H, dt)
    tb, tape = padded(B, V * 6 * H, dt)
    ob, h_out = padded(B, H, F32)
    cb, cell_out = padded(B, H, F32)
    _hip.call("cpc_lstm_fwd", _hip.ptr(gi), _hip.ptr(wfrag), _hip.ptr(b_hh), _hip.ptr(h0), _hip.ptr(c0), _hip.ptr(Hall), _hip.ptr(tape),
              _hip.ptr(h_out), _hip.ptr(cell_out), B, V, H, code)
    torch.cuda.synchronize()
    assert intact(hb, B * (V + 1) * H) and intact(tb, nt) and intact(ob, B * H) and intact(cb, B * H)
    for t in (Hall, tape, h_out, cell_out):
        assert bool(torch.isfinite(t.float()).all())
    return Hall, tape, h_out, cell_out


def _lstm_device(dt, B, V, H, ref):
    """cpc_prep_frag, cpc_lstm_fwd, cpc_lstm_bwd on the reference's inputs; returns Hall (B, V+1, H), h_out, cell_out, dG (B, V, 4H)."""
    code = _hip.dtype_code(dt)
    wfrag, wTfrag = _frags(ref["w_hh"], H, dt)
    gi = ref["gir"].to(dt).to(DEV).contiguous()
    db, ddh = ref["b_hh"].to(DEV), ref["dh"].to(DEV)
    h0 = None if ref["h0"] is None else ref["h0"].to(DEV)
    c0 = None if ref["c0"] is None else ref["c0"].to(DEV)
    Hall, tape, h_out, cell_out = _lstm_fwd(dt, B, V, H, gi, wfrag, db, h0, c0)
    gb, dG = padded(B, V * 4 * H, dt)
    _hip.call("cpc_lstm_bwd", _hip.ptr(ddh), _hip.ptr(tape), _hip.ptr(wTfrag), _hip.ptr(dG), B, V, H, code)
    torch.cuda.synchronize()
    assert intact(gb, B * V * 4 * H)
    assert bool(torch.isfinite(dG.float()).all())
    return host(Hall).view(B, V + 1, H), host(h_out).view(B, H), host(cell_out).view(B, H), host(dG).view(B, V, 4 * H)


def _lstm_check(dt, ref, Hall, h_out, cell_out, dG, label):
    errs = L.lstm_step_errors(Hall, dG, ref["hall"], ref["dG"])
    for k in L.LSTM_BLOCKS:
        ratio = (errs[k] / (ref["tol"][k] + 1e-300)).max().item()
        print(f"{label} {k}: largest per-step error {errs[k].max().item():.2e}, largest error / bound {ratio:.2f}")
    bad = L.lstm_violations(errs, ref["tol"])
    assert not bad, bad[:8]
    h0 = torch.zeros_like(ref["hall"][:, 0]) if ref["h0"] is None else L.rounded(ref["h0"], dt)
    assert torch.equal(Hall[:, 0], h0), "Hall[:, 0] is not the stored initial state"
    last = float(ref["tol"]["Hall"][-1])          # the last states to the hidden states' bound at the last step
    eh, ec = L.rel_err(h_out, ref["hV"]), L.rel_err(cell_out, ref["cV"])
    print(f"{label} h_out {eh:.2e}, cell_out {ec:.2e}, bound {last:.2e}")
    assert eh <= last and ec <= last
    assert torch.equal(L.rounded(h_out, dt), Hall[:, -1]), "Hall[:, V] is not h_out as stored"


@pytest.mark.parametrize("case", L.lstm_cases(), ids=L.lstm_case_id)
def test_lstm_fwd_bwd_per_step(case):
    """Both kernel families at their edges (a single batch row, a partial batch tile, one and two steps, hidden sizes that leave waves
    with unequal or no tiles, the 65 792-byte backward tiles), hidden states and the four gradient blocks judged step by step; the last
    pair; nothing written behind Hall, the tape, h_out, cell_out or dG, nor into the rows of items >= B."""
    _, dt, H, B, V = case
    ref = L.lstm_reference(dt, B, V, H, with_state=L.lstm_case_state(case))
    if ref["e_model"] is not None:
        assert max(float(v.max()) for v in ref["e_model"].values()) < L.LSTM_MODEL_CAP
    _lstm_check(dt, ref, *_lstm_device(dt, B, V, H, ref), L.lstm_case_id(case))


@pytest.mark.parametrize("dt,H", [(BF16, 32), (BF16, 256), (F32, 48), (F32, 288), (BF16, 288)])
def test_lstm_without_recurrent_weights_is_elementwise(dt, H):
    """W_hh = 0, b_hh = 0: cell_t = sigmoid(a_f) cell_{t-1} + sigmoid(a_i) tanh(a_g), h_t = sigmoid(a_o) tanh(cell_t) hold element by
    element, so any mix-up of batch row, step, gate or hidden unit shows as a gross error against the closed form: the input projections
    are a shuffled ramp over [-3, 3], different in every (b, t, j) in f32 (asserted).  Bounds as test_lstm_fwd_bwd_per_step."""
    B, V = 17, 5
    ref = L.lstm_reference(dt, B, V, H, with_state=True, zero_weights=True)
    if dt == F32:
        assert ref["gir"].unique().numel() == ref["gir"].numel()
    closed, cell = L.lstm_closed_form_zero_weights(ref["gir"], ref["h0r"], ref["c0r"])
    assert (closed[:, 1:] - ref["hall"][:, 1:]).abs().max() < 1e-14 and (cell - ref["cV"]).abs().max() < 1e-14
    Hall, h_out, cell_out, dG = _lstm_device(dt, B, V, H, ref)
    err = L.per_step_err(Hall[:, 1:], closed[:, 1:])
    print(f"zero weights {name(dt)} H={H}: per-step error of h against the closed form {err.max().item():.2e}")
    assert bool((err <= ref["tol"]["Hall"]).all()), err
    assert bool((dG[:, :V - 1, 3 * H:] == 0).all())          # dh reaches the earlier steps through W_hh only: do is exactly 0 there
    _lstm_check(dt, ref, Hall, h_out, cell_out, dG, f"zero weights {name(dt)} H={H}")


@pytest.mark.parametrize("H", [32, 288])
@pytest.mark.parametrize("dt", [F32, BF16], ids=name)
def test_lstm_run_in_two_pieces_is_bit_identical(dt, H):
    """13 steps equal, bit for bit in Hall, h_out and cell_out, the same data run as 6 + 7 steps with the f32 pair handed on through
    h0 / c0: the masters are f32 and the copy of h the matrix product reads is rounded from them the same way in both runs."""
    B, V, V1 = 17, 13, 6
    ref = L.lstm_reference(dt, B, V, H)
    wfrag, _ = _frags(ref["w_hh"], H, dt)
    gi = ref["gir"].to(dt).to(DEV).contiguous()
    db = ref["b_hh"].to(DEV)
    whole = _lstm_fwd(dt, B, V, H, gi, wfrag, db)
    first = _lstm_fwd(dt, B, V1, H, gi.view(B, V, 4 * H)[:, :V1].contiguous(), wfrag, db)
    second = _lstm_fwd(dt, B, V - V1, H, gi.view(B, V, 4 * H)[:, V1:].contiguous(), wfrag, db, first[2].clone(), first[3].clone())
    Hw, H1, H2 = whole[0].view(B, V + 1, H), first[0].view(B, V1 + 1, H), second[0].view(B, V - V1 + 1, H)
    assert torch.equal(bits(Hw[:, :V1 + 1]), bits(H1))
    assert torch.equal(bits(Hw[:, V1:]), bits(H2))
    assert torch.equal(bits(whole[2]), bits(second[2])) and torch.equal(bits(whole[3]), bits(second[3]))
    assert not torch.equal(bits(first[2]), bits(second[2]))


# ======================================================================================================================= routes
E_S, V_S, K_S, B_S = 64, 12, 4, 8
SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E_S] * 5, 'bias': True}
PREFIX = "autoregressive_model.lstmCell."


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_standalone_lstm(dtype):
    """AudioLSTMModel(16, 32)(z) on its own (the _ContextForward bridge): output, z.grad and the four parameter gradients against float64
    autograd on nn.LSTMCell with the weights and z as the device stores them.  fp32: 1e-4 output, 1e-3 gradients (the bounds of
    test_standalone_stacked_gru); bf16: 2e-2 output, 4e-2 gradients (the whole-tensor bf16 bounds of the GRU kernel tests).  A carried
    second call equals the float64 continuation from the first call's pair; backward after it raises."""
    B, E, V, H = 5, 16, 7, 32
    st = F32 if dtype == "fp32" else BF16
    t_out, t_grad = (1e-4, 1e-3) if dtype == "fp32" else (2e-2, 4e-2)
    torch.manual_seed(8)
    lstm = AudioLSTMModel(E, H)
    lstm.compute_dtype = st
    cell = torch.nn.LSTMCell(E, H).double()
    cell.load_state_dict({k: (v.to(st).double() if "weight" in k else v.double()) for k, v in lstm.lstmCell.state_dict().items()})
    z = torch.randn(B, E, V, generator=torch.Generator().manual_seed(9)).to(st).float()
    z2 = torch.randn(B, E, V, generator=torch.Generator().manual_seed(11)).to(st).float()
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(10))

    def loop(zz, h, c):
        for t in range(V):
            h, c = cell(zz[:, :, t], (h, c))
        return h, c
    zr = z.double().requires_grad_(True)
    zero = torch.zeros(B, H, dtype=torch.float64)
    h, c = loop(zr, zero, zero)
    (h * dh.double()).sum().backward()
    lstm = lstm.to(DEV)
    zd = z.to(DEV).requires_grad_(True)
    out = lstm(zd)
    assert out.shape == (B, H) and out.dtype == torch.float32 and lstm.hidden is None
    errs = {"out": L.rel_err(out, h)}
    assert errs["out"] < t_out, errs
    (out * dh.to(DEV)).sum().backward()
    errs["dz"] = L.rel_err(zd.grad, zr.grad)
    assert errs["dz"] < t_grad, errs
    ref = dict(cell.named_parameters())
    for n, p_ in lstm.lstmCell.named_parameters():
        errs[n] = L.rel_err(p_.grad, ref[n].grad)
        assert errs[n] < t_grad, errs
    print(f"stand-alone AudioLSTMModel {dtype}:", {k: f"{v:.2e}" for k, v in errs.items()})
    # carried pair: the second call continues the first
    lstm.reset_hidden = False
    with torch.no_grad():
        o1 = lstm(z.to(DEV))
        h1, c1 = (t.detach().clone() for t in lstm.hidden)
        assert h1.shape == (B, H) and c1.shape == (B, H) and h1.dtype == torch.float32 and torch.equal(h1, o1)
        o2 = lstm(z2.to(DEV))
        want, _ = loop(z2.double(), h1.double().cpu(), c1.double().cpu())
        fresh, _ = loop(z2.double(), zero, zero)
    assert L.rel_err(o2, want) < t_out
    assert L.rel_err(o2, fresh) > 1e-2          # the carried pair made a difference
    out3 = lstm(z.to(DEV).requires_grad_(True))
    with pytest.raises(RuntimeError, match="carried over"):
        out3.sum().backward()
    lstm.hidden = torch.zeros(B, H, device=DEV)          # not a pair
    with pytest.raises(ValueError, match="pair"), torch.no_grad():
        lstm(z.to(DEV))


def _model(dtype, H, seed=3, **kw):
    """The small encoder of test_gru_wide_gpu.py (64 channels, weights doubled so that the scores are not degenerate) with an
    AudioLSTMModel(64, H) context."""
    torch.manual_seed(seed)
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), AudioLSTMModel(E_S, H, **kw), enc_size=E_S, ar_size=H, visible_steps=V_S,
                                       prediction_steps=K_S, compute_dtype=dtype)
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if n.startswith("encoder.") and n.endswith("weight"):
                p_.mul_(2.0)
    return model


def _data(n, seed):
    length = _model("fp32", 32).item_length
    return torch.randn(n, length, generator=torch.Generator().manual_seed(seed)) * 0.5


class _Meter:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))


class _Logger:
    def __init__(self):
        self.loss_meter, self.score_meter = _Meter(), _Meter()

    def log(self, step):
        pass


def _trainer(model, data, logger, H, score_function=softplus_score_function, reg=1.0, all_t=False, **kw):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=reg, score_over_all_timesteps=all_t, score_function=score_function,
                                      prediction_steps=K_S, ar_size=H, **kw)
    tr.verbose = False
    return tr


_REFERENCE = {}          # (H, score, all_t) -> (loss, grads): computed once, shared by the storage types, never modified


def _reference_step(H, params, data, score, all_t, reg):
    key = (H, score, all_t)
    if key not in _REFERENCE:
        lo = L.LstmOracle(params, V_S, K_S, score=score, all_timesteps=all_t, regularization=reg, lr=0.0)
        loss, _, grads = lo.loss_and_grads(data)
        _REFERENCE[key] = (float(loss), {k: v.detach().clone() for k, v in grads.items()})
    return _REFERENCE[key]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [32, 288])
def test_lstm_model_loss_and_gradients_against_reference(H, dtype):
    """One trainer step (lr 0: the gradients stay on the parameters) at H = 32 (4 waves) and 288 (8 waves): loss and every parameter
    gradient against the composed float64 reference, softplus and linear scores, both score_over_all_timesteps settings.  Bounds of
    test_gru_wide_gpu.py: fp32 loss 1e-4, gradients 1e-3 (relative l2); bf16 loss 1e-2, context and predictor 0.12, encoder 0.2."""
    data = _data(B_S, 1)
    model = _model(dtype, H).to(DEV)
    assert type(model.engine(B_S, data.shape[1]).ctx).__name__ == "LSTMContext"
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    assert [k for k in params if k.startswith("autoregressive_model.")] == [PREFIX + n for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    worst = {"encoder": 0.0, "context / predictor": 0.0, "loss": 0.0}
    for score in ("softplus", "linear"):
        for all_t, reg in ((False, 1.0), (True, 0.01)):
            model.load_state_dict(params)
            logger = _Logger()
            tr = _trainer(model, data, logger, H, SCORE[score], reg, all_t)
            assert tr._fused()
            tr.train(batch_size=B_S, epochs=1, lr=0.0, num_workers=0, max_steps=1)
            loss, grads = _reference_step(H, params, data, score, all_t, reg)
            ltol = 1e-4 if dtype == "fp32" else 1e-2
            got = logger.loss_meter.values[0]
            worst["loss"] = max(worst["loss"], abs(got - loss) / abs(loss))
            assert abs(got - loss) <= ltol * abs(loss), (score, all_t, got, loss)
            named = dict(model.named_parameters())
            assert set(grads) == set(named)
            for pname, ref in grads.items():
                group = "encoder" if pname.startswith("encoder.") else "context / predictor"
                gtol = 1e-3 if dtype == "fp32" else (0.2 if group == "encoder" else 0.12)
                l2 = _rel(named[pname].grad, ref)
                worst[group] = max(worst[group], l2)
                assert l2 < gtol, (score, all_t, pname, l2)
    print(f"LSTM H={H} {dtype}: largest relative loss error and relative l2 gradient errors", {k: f"{v:.2e}" for k, v in worst.items()})


class _Labelled(torch.utils.data.Dataset):
    def __init__(self, clips):
        self.clips = clips

    def __len__(self):
        return self.clips.shape[0]

    def __getitem__(self, i):
        return self.clips[i], i


def test_lstm_train_validate_and_task_data_against_reference():
    """train() for three Adam steps on the fused route (softplus, fp32) against the float64 composition stepped with the oracle's
    adam_update from the same parameters, then validate() and calc_test_task_data() against the reference with its updated parameters
    (bounds of test_wide_gru_train_and_validate_against_oracle)."""
    B, steps, lr, H = 4, 3, 2e-4, 32
    data = _data(B, 5)
    model = _model("fp32", H).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    lo = L.LstmOracle(params, V_S, K_S, score="softplus", regularization=1.0, lr=lr)
    want = [lo.step(data)[0] for _ in range(steps)]
    val = _data(16, 6)
    logger = _Logger()
    tr = _trainer(model, data, logger, H, validation_set=TensorAudioDataset(val, device=DEV), test_task_set=_Labelled(val[:8]))
    assert tr._fused()
    tr.train(batch_size=B, epochs=steps, lr=lr, num_workers=0, max_steps=steps)
    got = logger.loss_meter.values
    assert len(got) == steps
    for i in range(steps):
        assert abs(got[i] - want[i]) <= 1e-4 * abs(want[i]) * (1 + 4 * i), (i, got, want)
    for k, v in model.state_dict().items():
        assert _rel(v, lo.params[k]) < 1e-4 * (1 + 4 * steps), k
    losses, acc, score, mi = tr.validate(batch_size=8, num_workers=0)
    want_l, want_a = 0.0, 0.0
    lists = O.file_batch_sampler([val.shape[0]], 8, 8, True, seed=0)
    for idx in lists:
        pl, pa, _ = lo.validation(val[idx])
        want_l, want_a = want_l + pl, want_a + pa
    assert len(lists) > 0
    assert _rel(losses, want_l / len(lists)) < 1e-4 * (1 + 4 * steps)
    assert (torch.as_tensor(acc).cpu().double() - want_a / len(lists)).abs().max().item() < 1e-4
    task, labels = tr.calc_test_task_data(batch_size=4, num_workers=0)
    with torch.no_grad():
        c = lo.forward(val[:8], training=False)[3]
    assert list(labels) == list(range(8)) and L.rel_err(task, c) < 1e-4


H_O, LR_O = 32, 2e-4


def _steps(route, steps, seed=11, **attrs):
    """Adam steps of the fp32 model with the trainer's attributes ``attrs``: route 'fused' (the engine's step), 'generic' (a score
    function the trainer does not recognise: autograd through model.forward, torch optimizers).  The batch is the whole set."""
    data = _data(B_S, seed)
    model = _model("fp32", H_O).to(DEV)
    logger = _Logger()
    sf = softplus_score_function if route == "fused" else (lambda p, t: softplus_score_function(p, t))
    tr = _trainer(model, data, logger, H_O, sf)
    assert tr._fused() == (route == "fused")
    for k, v in attrs.items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    random.seed(5)
    tr.train(batch_size=B_S, epochs=steps, lr=LR_O, num_workers=0, max_steps=steps)
    torch.cuda.synchronize()
    assert len(logger.loss_meter.values) == steps
    return logger.loss_meter.values, {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}, tr


def test_graphed_step_is_the_eager_step_bit_for_bit():
    """use_graph: three replayed steps give the eager steps' losses and parameters bit for bit (the same kernels in the same order on
    the same data; every reduction of the step has a fixed order)."""
    graphed, eager = _steps("fused", 3, use_graph=True), _steps("fused", 3)
    print("graphed / eager losses", graphed[0], eager[0])
    assert graphed[0] == eager[0]
    for k in eager[1]:
        assert torch.equal(graphed[1][k], eager[1][k]), k


OPTIONS = {"sampled negatives": dict(num_negatives=3, negative_seed=7), "clip": dict(max_grad_norm=0.05), "ema": dict(ema_decay=0.5)}


@pytest.mark.parametrize("option", list(OPTIONS))
def test_options_around_the_lstm_against_the_generic_route(option):
    """num_negatives, max_grad_norm and ema_decay with the LSTM context: two fused steps against the same option on the generic route.
    Bounds of test_options_around_a_stack_against_the_generic_route: 1e-5 on the losses, 1e-4 on every parameter (relative l2); for
    the sampled loss 2e-4 on the losses, test_sampled_negatives_gpu.py's bound between the two routes."""
    fused, generic = _steps("fused", 2, **OPTIONS[option]), _steps("generic", 2, **OPTIONS[option])
    ltol = 2e-4 if option == "sampled negatives" else 1e-5
    for la, lb in zip(fused[0], generic[0]):
        assert abs(la - lb) <= ltol * abs(lb), (fused[0], generic[0])
    for k in fused[1]:
        assert _rel(fused[1][k], generic[1][k]) < 1e-4, k
    if option == "ema":          # the average leaves the parameters alone: the shadow is what the option adds
        assert _rel(fused[2]._ema, generic[2]._ema) < 1e-4
        assert _rel(fused[2]._ema, fused[2].model._flat_param) > 1e-5
    else:
        plain = _steps("fused", 2)
        assert any(_rel(fused[1][k], plain[1][k]) > 1e-4 for k in plain[1]) or fused[0] != plain[0], "the option made no difference"


def test_scalogram_engine_with_an_lstm(golden_dir):
    """One fp32 step (lr 0) on the smallest scalogram fixture's encoder with an LSTM context, against the composed float64 reference
    (1e-4 loss, 1e-3 gradients: test_scalogram_engine_with_a_stacked_gru's)."""
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    z = np.load(os.path.join(golden_dir, "scalogram_model.npz"))
    meta = copy.deepcopy(json.load(open(os.path.join(golden_dir, "scalogram_model.json"))))
    B, K, E, V, H = meta["B"], meta["K"], meta["E"], meta["V"], 32
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    torch.manual_seed(21)
    model = AudioPredictiveCodingModel(enc, AudioLSTMModel(E, H), enc_size=E, ar_size=H, visible_steps=V, prediction_steps=K,
                                       compute_dtype="fp32")
    state = model.state_dict()
    for k in z.files:
        if k.startswith("param/encoder."):
            state[k[len("param/"):]] = torch.from_numpy(z[k])
    model.load_state_dict(state)
    pre, model = pre.to(DEV), model.to(DEV)
    oblocks = copy.deepcopy(blocks)
    oblocks[0]["in_channels"] = 2
    model.train()
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    data = torch.from_numpy(z["data"])
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.01, score_function=softplus_score_function, prediction_steps=K, ar_size=H,
                                      preprocessing=pre)
    tr.verbose = False
    random.seed(91)
    idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
    with torch.no_grad():
        scal = pre(data[idx].to(DEV).unsqueeze(1))
    assert type(model.engine_for(scal).ctx).__name__ == "LSTMContext"
    random.seed(91)
    tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    lo = L.LstmOracle(params, V, K, score="softplus", regularization=0.01, lr=0.0, scalogram=oblocks)
    loss, _, grads = lo.loss_and_grads(scal.float().cpu())
    got = logger.loss_meter.values[0]
    assert abs(got - float(loss)) < 1e-4 * abs(float(loss)), (got, float(loss))
    named = dict(model.named_parameters())
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for pname, ref in grads.items():
        if ref.abs().max().item() < 1e-6 * largest:          # a convolution bias in front of a train-mode BatchNorm: zero gradient
            assert named[pname].grad.abs().max().item() < 1e-5 * largest, pname
            continue
        assert _rel(named[pname].grad, ref) < 1e-3, pname


@contextlib.contextmanager
def _no_launch(monkeypatch):
    """Fails the test if anything is launched through the binding inside the block."""
    calls = []
    with monkeypatch.context() as m:
        for fn in ("call", "gemm_nt", "gemm_tn"):
            m.setattr(_hip, fn, lambda *a, _fn=fn, **k: calls.append((_fn, a[:1])))
        yield
    assert not calls, calls


def test_lstm_refusals_come_before_any_launch(monkeypatch):
    """H = 40 in bf16 (not a multiple of 32), H = 528 (> 512) and the gradient penalty raise NotImplementedError with the reason, and
    nothing has been launched by then."""
    for dtype, H, reason in (("bf16", 40, "multiple of 32"), ("fp32", 528, "<= 512"), ("bf16", 528, "<= 512"), ("fp32", 40, "of 16 in float32")):
        model = AudioPredictiveCodingModel(AudioEncoder(SMALL), AudioLSTMModel(E_S, H), enc_size=E_S, ar_size=H, visible_steps=8,
                                           prediction_steps=2, compute_dtype=dtype).to(DEV)
        with _no_launch(monkeypatch), pytest.raises(NotImplementedError, match=reason):
            model.engine(2, model.item_length)
    model = _model("fp32", 32).to(DEV)
    with _no_launch(monkeypatch), pytest.raises(NotImplementedError, match="gradient penalty through an AudioLSTMModel"):
        ContrastiveEstimationTrainer(model=model, dataset=None, score_function=linear_score_function, prediction_steps=K_S, ar_size=32,
                                     wasserstein_gradient_penalty=True, preprocessing=torch.nn.Identity())
    lstm = AudioLSTMModel(16, 40)
    lstm.compute_dtype = BF16
    with _no_launch(monkeypatch), pytest.raises(NotImplementedError, match="multiple of 32"):
        lstm.to(DEV)(torch.zeros(2, 16, 5, device=DEV))
