"""The GRU context for hidden sizes above 256 (up to 512): the 8-wave weight-streaming recurrences behind cpc_gru_fwd / cpc_gru_bwd,
the gradient-penalty kernels at 512 threads, and the routes that use them (GRUContext in both storage dtypes, a carried state across
calls of a reset_hidden=False model, the bf16 engine's Float32Context for the penalty, stand-alone AudioGRUModel calls).

Kernels against a float64 nn.GRUCell loop with the weights as the device stores them (tolerances of test_hip_kernels.py's GRU
tests); models against the CPU oracle (oracle/cpc_oracle.py, the reference's GRUCell loop).
"""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,  # noqa: E402
                                                           softplus_score_function)
from oracle import cpc_oracle as O  # noqa: E402

DEV = "cuda:0"
SCORE = {"softplus": softplus_score_function, "linear": linear_score_function}
GUARD = 64          # sentinel elements behind every output
SENT = -7.5         # (exact in bf16)


def rel_err(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def per_step_err(got, ref):
    """(B, V, X) -> max over the steps t of max_{b,j} |got - ref| / max_{b,j} |ref| within step t: the gradient of a recurrence decays
    backwards through time, so a maximum over the whole tensor hides the early steps."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().amax((0, 2)) / (ref.abs().amax((0, 2)) + 1e-30)).max().item()


def _rel(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


def guarded(n, dt, fill=float("nan")):
    """A device buffer of n elements followed by GUARD sentinel elements; returns (whole buffer, view of the first n)."""
    buf = torch.full((n + GUARD,), fill, device=DEV, dtype=dt)
    buf[n:] = SENT
    return buf, buf[:n]


def guard_intact(buf, n):
    return bool((buf[n:].float() == SENT).all())


def gru64(gi, w_hh, b_hh, h0):
    """float64 loop over the gates of nn.GRUCell given the input projections gi (B, V, 3H); returns all hidden states."""
    H = w_hh.shape[1]
    h, hs = h0, [h0]
    for t in range(gi.shape[1]):
        gh = h @ w_hh.T + b_hh
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        u = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - u) * n + u * h
        hs.append(h)
    return torch.stack(hs, 1)


# --------------------------------------------------------------------------------------- recurrence kernels
CASES = [(dt, H) for dt in (torch.float32, torch.bfloat16) for H in (288, 384, 512)] + [(torch.float32, 272)]


@pytest.mark.parametrize("V", [1, 5, 13])
@pytest.mark.parametrize("B", [7, 16, 37])
@pytest.mark.parametrize("dt,H", CASES)
def test_wide_gru_fwd_bwd(dt, H, B, V):
    """cpc_gru_fwd and cpc_gru_bwd at 256 < H <= 512 against float64; nothing is written behind any output (Hall, c, tape, dG).
    (The launch from a carried state is reached through whole-model runs: test_wide_gru_carried_state.)"""
    g = torch.Generator().manual_seed(B * 1000 + H + V)
    code = _hip.dtype_code(dt)
    w_hh = torch.randn(3 * H, H, generator=g) / math.sqrt(H)
    b_hh = torch.randn(3 * H, generator=g) * 0.1
    Gi = torch.randn(B, V, 3 * H, generator=g)
    dc = torch.randn(B, H, generator=g)
    dW = w_hh.to(DEV)
    wfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
    wTfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wfrag), 3 * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wTfrag), H, 3 * H, H, 1, code)
    dGi, db, ddc = Gi.to(DEV).to(dt), b_hh.to(DEV), dc.to(DEV)
    nt = int(_hip.lib().cpc_gru_tape_elems(B, V, H, code))
    assert nt == B * V * 5 * H
    wr, br = w_hh.to(dt).double(), b_hh.double()
    t_f = 2e-5 if dt == torch.float32 else 2e-2
    hb, Hall = guarded(B * (V + 1) * H, dt)
    cb, c = guarded(B * H, torch.float32)
    tb, tape = guarded(nt, dt, fill=0.0)
    _hip.call("cpc_gru_fwd", _hip.ptr(dGi), _hip.ptr(wfrag), _hip.ptr(db), _hip.ptr(Hall), _hip.ptr(tape), _hip.ptr(c), B, V, H, code)
    ref = gru64(Gi.to(dt).double(), wr, br, torch.zeros(B, H, dtype=torch.float64))
    assert rel_err(c.view(B, H), ref[:, -1]) < t_f
    assert rel_err(Hall.view(B, V + 1, H), ref) < t_f
    assert guard_intact(hb, B * (V + 1) * H) and guard_intact(cb, B * H) and guard_intact(tb, nt)
    wg = wr.clone().requires_grad_(True)
    bg = br.clone().requires_grad_(True)
    gig = Gi.to(dt).double().requires_grad_(True)
    hs = gru64(gig, wg, bg, torch.zeros(B, H, dtype=torch.float64))
    (hs[:, -1] * dc.double()).sum().backward()
    gb, dG = guarded(B * V * 4 * H, dt)
    _hip.call("cpc_gru_bwd", _hip.ptr(ddc), _hip.ptr(tape), _hip.ptr(wTfrag), _hip.ptr(dG), B, V, H, code)
    assert guard_intact(gb, B * V * 4 * H)
    dG = dG.view(B, V, 4 * H)
    t_b = 5e-5 if dt == torch.float32 else 4e-2
    assert per_step_err(dG[:, :, :3 * H], gig.grad) < t_b
    dGh = torch.cat([dG[:, :, :2 * H], dG[:, :, 3 * H:]], dim=2).double().cpu()
    assert rel_err(dGh.sum((0, 1)), bg.grad) < t_b
    dWhh = torch.einsum("bvg,bvh->gh", dGh, Hall.view(B, V + 1, H)[:, :V].double().cpu())
    assert rel_err(dWhh, wg.grad) < t_b


@pytest.mark.parametrize("B,V,E,H", [(3, 12, 64, 384), (2, 9, 32, 512)])
def test_wide_gru_gradient_penalty_kernels(B, V, E, H):
    """cpc_gru_gp_fwd / cpc_gru_gp_bwd at H = 384 and 512 (512 threads per workgroup): the gradient of the directional derivative
    D = <xt, d S / d x>, S = <wc, GRU(x)>, with respect to the GRU's parameters and its input, assembled from the kernels' outputs
    as contexts.GRUContext.gp_grads does, against autograd's double backward in float64 (test_hip_kernels.py's construction)."""
    g = torch.Generator().manual_seed(B * 1000 + H)
    f64 = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).float().double()
    Wih, Whh = f64(3 * H, E, s=E ** -0.5), f64(3 * H, H, s=H ** -0.5)
    bih, bhh = f64(3 * H, s=0.3), f64(3 * H, s=0.3)
    x, xt, wc = f64(B, V, E), f64(B, V, E), f64(B, H)
    params = [t.clone().requires_grad_(True) for t in (Wih, Whh, bih, bhh, x)]
    pWih, pWhh, pbih, pbhh, px = params
    hs = gru64((px.reshape(B * V, E) @ pWih.T + pbih).reshape(B, V, 3 * H), pWhh, pbhh, torch.zeros(B, H, dtype=torch.double))
    gx, = torch.autograd.grad((wc * hs[:, -1]).sum(), px, create_graph=True)
    ref = torch.autograd.grad((gx * xt).sum(), params)
    Gi = (x.reshape(B * V, E) @ Wih.T + bih).float().contiguous().to(DEV)
    GiT = (xt.reshape(B * V, E) @ Wih.T).float().contiguous().to(DEV)
    WT, W = Whh.T.float().contiguous().to(DEV), Whh.float().contiguous().to(DEV)
    d_bhh, d_wc = bhh.float().to(DEV), wc.float().contiguous().to(DEV)
    tb, tape = guarded(B * V * 10 * H, torch.float32)
    cb, ct = guarded(B * H, torch.float32)
    _hip.call("cpc_gru_gp_fwd", _hip.ptr(Gi), _hip.ptr(GiT), _hip.ptr(WT), _hip.ptr(d_bhh), _hip.ptr(tape), _hip.ptr(ct), B, V, H)
    ab, dA = guarded(B * V * 8 * H, torch.float32)
    _hip.call("cpc_gru_gp_bwd", _hip.ptr(d_wc), _hip.ptr(tape), _hip.ptr(W), _hip.ptr(dA), B, V, H)
    assert guard_intact(tb, B * V * 10 * H) and guard_intact(cb, B * H) and guard_intact(ab, B * V * 8 * H)
    assert torch.isfinite(tape).all() and torch.isfinite(dA).all() and torch.isfinite(ct).all()
    tp, da = tape.view(B, V, 10, H).double().cpu(), dA.double().cpu().reshape(B * V, 8 * H)
    hp, htp = tp[:, :, 4].reshape(B * V, H), tp[:, :, 9].reshape(B * V, H)
    X, XT = x.reshape(B * V, E), xt.reshape(B * V, E)
    d3, v3 = da[:, :3 * H], da[:, 4 * H:7 * H]
    dh, vh = torch.cat([da[:, :2 * H], da[:, 3 * H:4 * H]], 1), torch.cat([da[:, 4 * H:6 * H], da[:, 7 * H:]], 1)
    got = [d3.T @ XT + v3.T @ X, dh.T @ htp + vh.T @ hp, v3.sum(0), vh.sum(0), (v3 @ Wih).reshape(B, V, E)]
    for name, a, b in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh", "x"), got, ref):
        l2 = _rel(a, b)
        assert l2 < 2e-4, (name, l2)
    eps = 1e-6
    last = lambda xx: gru64((xx.reshape(B * V, E) @ Wih.T + bih).reshape(B, V, 3 * H), Whh, bhh, torch.zeros(B, H, dtype=torch.double))[:, -1]
    fd = (last(x + eps * xt) - last(x - eps * xt)) / (2 * eps)
    assert rel_err(ct.view(B, H), fd) < 1e-4


def test_wide_gru_refuses_unsupported_shapes():
    """The C ABI: H > 512, H % 32 != 0 in bf16, H % 16 != 0 -> -22, for every GRU entry point; the engine: NotImplementedError."""
    x = torch.zeros(64, device=DEV)
    p = _hip.ptr(x)
    lib, s = _hip.lib(), _hip.stream_ptr()
    for H, code in ((528, _hip.F32), (528, _hip.BF16), (496, _hip.BF16), (520, _hip.F32), (300, _hip.F32), (1024, _hip.F32)):
        assert lib.cpc_gru_fwd(p, p, p, p, p, p, 16, 4, H, code, s) == -22, H
        assert lib.cpc_gru_bwd(p, p, p, p, 16, 4, H, code, s) == -22, H
    for H in (528, 1024):
        assert lib.cpc_gru_gp_fwd(p, p, p, p, p, p, 2, 4, H, s) == -22, H
        assert lib.cpc_gru_gp_bwd(p, p, p, p, 2, 4, H, s) == -22, H
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64] * 5, 'bias': True})
    for dtype in ("fp32", "bf16"):
        model = AudioPredictiveCodingModel(enc, AudioGRUModel(64, 544), enc_size=64, ar_size=544, visible_steps=8, prediction_steps=2,
                                           compute_dtype=dtype).to(DEV)
        with pytest.raises(NotImplementedError, match="<= 512"):
            model.engine(2, model.item_length)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(64, 496), enc_size=64, ar_size=496, visible_steps=8, prediction_steps=2,
                                       compute_dtype="bf16").to(DEV)
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        model.engine(2, model.item_length)


# --------------------------------------------------------------------------------------- models
@pytest.mark.parametrize("H", [288, 384, 512])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wide_gru_carried_state(dtype, H):
    """AudioGRUModel(reset_hidden=False) as the context of a model (reference audio_model.py:69, :75): the second call starts from the
    first call's last hidden state.  Its c against a float64 nn.GRUCell loop over the second call's z from the first call's c, with
    the weights as the device stores them (tolerances of test_wide_gru_fwd_bwd)."""
    B, E, V, K = 7, 64, 5, 2
    torch.manual_seed(H)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(E, H, reset_hidden=False), enc_size=E, ar_size=H, visible_steps=V,
                                       prediction_steps=K, compute_dtype=dtype).to(DEV)
    gen = torch.Generator().manual_seed(7)
    x1, x2 = (torch.randn(B, 1, model.item_length, generator=gen).to(DEV) for _ in range(2))
    with torch.no_grad():
        _, _, _, c1 = model(x1)
        _, _, z2, c2 = model(x2)
    st = torch.float32 if dtype == "fp32" else torch.bfloat16
    p = {n: v.detach().cpu() for n, v in model.autoregressive_model.gruCell.named_parameters()}
    gi = z2.detach().cpu().to(st).double().transpose(1, 2) @ p["weight_ih"].to(st).double().T + p["bias_ih"].double()
    ref = gru64(gi, p["weight_hh"].to(st).double(), p["bias_hh"].double(), c1.detach().cpu().double())
    assert rel_err(c2, ref[:, -1]) < (2e-5 if dtype == "fp32" else 2e-2)
    fresh = gru64(gi, p["weight_hh"].to(st).double(), p["bias_hh"].double(), torch.zeros(B, H, dtype=torch.float64))
    assert rel_err(c2, fresh[:, -1]) > 1e-2          # the carried state made a difference


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


E_S, H_S, V_S, K_S, B_S = 64, 512, 12, 4, 8


def _wide_model(dtype, seed=3):
    """A small AudioEncoder (64 channels) with an AudioGRUModel(64, 512) context, seeded parameters (encoder weights doubled so
    that the scores are not degenerate)."""
    torch.manual_seed(seed)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E_S] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(E_S, H_S), enc_size=E_S, ar_size=H_S, visible_steps=V_S, prediction_steps=K_S,
                                       compute_dtype=dtype)
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if n.startswith("encoder.") and n.endswith("weight"):
                p_.mul_(2.0)
    return model


def _wide_data(n, seed):
    L = _wide_model("fp32").item_length
    return torch.randn(n, L, generator=torch.Generator().manual_seed(seed)) * 0.5


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wide_gru_model_loss_and_gradients_against_oracle(dtype):
    """One trainer step (lr 0: the gradients stay on the parameters) with H = 512: loss and every parameter gradient against the
    oracle, softplus and linear scores, both loss branches.  fp32: 1e-4 loss, 1e-3 gradients (l2, relative).  bf16: loss 1e-2 and
    the context's and the predictor's gradients 0.12 (the small-model bounds of test_model_gpu.py; measured up to 0.059); the
    encoder's 0.2, test_attention_long_gpu.py's bound for a small-channel encoder in bf16 storage (measured up to 0.123 here:
    rounding in the five bf16 layers, whatever the context's width)."""
    data = _wide_data(B_S, 1)
    model = _wide_model(dtype).to(DEV)
    assert type(model.engine(B_S, data.shape[1]).ctx).__name__ == "GRUContext"
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    worst = {"encoder": 0.0, "context / predictor": 0.0}
    for score in ("softplus", "linear"):
        for all_t, reg in ((False, 1.0), (True, 0.01)):
            model.load_state_dict(params)
            logger = _Logger()
            tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                              regularization=reg, score_over_all_timesteps=all_t, score_function=SCORE[score],
                                              prediction_steps=K_S, ar_size=H_S)
            tr.verbose = False
            tr.train(batch_size=B_S, epochs=1, lr=0.0, num_workers=0, max_steps=1)
            ot = O.OracleTrainer(params, V_S, K_S, score=score, all_timesteps=all_t, regularization=reg, lr=0.0)
            loss, _, grads = ot.loss_and_grads(data)          # the batch is the whole set: the sampler's order does not matter
            ltol = 1e-4 if dtype == "fp32" else 1e-2
            got = logger.loss_meter.values[0]
            assert abs(got - float(loss)) <= ltol * abs(float(loss)), (score, all_t, got, float(loss))
            named = dict(model.named_parameters())
            for name, ref in grads.items():
                group = "encoder" if name.startswith("encoder.") else "context / predictor"
                gtol = 1e-3 if dtype == "fp32" else (0.2 if group == "encoder" else 0.12)
                l2 = _rel(named[name].grad, ref)
                worst[group] = max(worst[group], l2)
                assert l2 < gtol, (score, all_t, name, l2)
    print(f"H=512 model, {dtype}: largest relative l2 gradient error", worst)


def test_wide_gru_train_and_validate_against_oracle():
    """train() for three Adam steps with H = 512 against the oracle's steps from the same parameters, then validate() against the
    oracle's validation terms with the oracle's updated parameters (fp32)."""
    B, steps, lr = 4, 3, 2e-4
    data = _wide_data(B, 5)
    model = _wide_model("fp32").to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    ot = O.OracleTrainer(params, V_S, K_S, score="softplus", all_timesteps=False, regularization=1.0, lr=lr)
    want = [ot.step(data)[0] for _ in range(steps)]
    val = _wide_data(16, 6)
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=1.0, score_over_all_timesteps=False, score_function=softplus_score_function,
                                      prediction_steps=K_S, ar_size=H_S, validation_set=TensorAudioDataset(val, device=DEV))
    tr.verbose = False
    tr.train(batch_size=B, epochs=steps, lr=lr, num_workers=0, max_steps=steps)
    got = logger.loss_meter.values
    assert len(got) == steps
    for i in range(steps):
        assert abs(got[i] - want[i]) <= 1e-4 * abs(want[i]) * (1 + 4 * i), (i, got, want)
    losses, acc, score, mi = tr.validate(batch_size=8, num_workers=0)
    oparams = {k: v.detach() for k, v in ot.params.items()}
    want_l, want_a = 0.0, 0.0
    lists = O.file_batch_sampler([val.shape[0]], 8, 8, True, seed=0)
    for idx in lists:
        pred, targ, _, _ = O.cpc_forward(val[idx].unsqueeze(1), oparams, V_S, K_S, training=False)
        pl, pa, _ = O.validation_terms(O.softplus_scores(pred.double(), targ.double()), False)
        want_l, want_a = want_l + pl, want_a + pa
    n = len(lists)
    assert n > 0
    assert _rel(losses, want_l / n) < 1e-4 * (1 + 4 * steps)
    assert (torch.as_tensor(acc).cpu().double() - want_a / n).abs().max().item() < 1e-4


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wide_gru_gradient_penalty_against_oracle(golden_dir, dtype):
    """The Wasserstein gradient penalty through an AudioGRUModel(64, 512) context on the scalogram fixture's encoder (its parameters,
    a seeded GRU): exact-f32 mode (GRUContext.tangent / gp_grads on cpc_gru_gp_*) and a bf16 engine whose GRU runs in float32
    (contexts.Float32Context), against the oracle's double backward.  Bounds of test_attention_long_gpu.py's penalty test: 1e-4 loss /
    1e-3 gradients in f32; in bf16 the loss within 1e-2 and gradient cosines > 0.95 (weights) / 0.85 (vectors)."""
    import copy
    import json
    import os
    import numpy as np
    from cpc_audio_amd.audio_dataset import FileBatchSampler
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    z = np.load(os.path.join(golden_dir, "scalogram_model.npz"))
    meta = copy.deepcopy(json.load(open(os.path.join(golden_dir, "scalogram_model.json"))))
    B, K, E, V, H = meta["B"], meta["K"], meta["E"], meta["V"], 512
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    torch.manual_seed(21)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(E, H), enc_size=E, ar_size=H, visible_steps=V, prediction_steps=K,
                                       compute_dtype=dtype)
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
    named = dict(model.named_parameters())
    for all_t, reg, factor in ((False, 0.01, 2.0), (True, 0.0, 10.0)):
        model.load_state_dict(params)
        logger = _Logger()
        tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                          regularization=reg, score_over_all_timesteps=all_t, score_function=SCORE["linear"],
                                          prediction_steps=K, ar_size=H, preprocessing=pre, wasserstein_gradient_penalty=True,
                                          gradient_penalty_factor=factor)
        tr.verbose = False
        random.seed(91)
        idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
        with torch.no_grad():
            scal = pre(data[idx].to(DEV).unsqueeze(1))
        ctx = model.engine_for(scal).ctx
        assert type(ctx).__name__ == ("GRUContext" if dtype == "fp32" else "Float32Context")
        assert type(getattr(ctx, "inner", ctx)).__name__ == "GRUContext"
        random.seed(91)
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
        ot = O.OracleTrainer(params, V, K, score="linear", all_timesteps=all_t, regularization=reg, lr=0.0, scalogram=oblocks,
                             gradient_penalty_factor=factor)
        loss, _, grads = ot.loss_and_grads(scal.float().cpu())
        got_loss = logger.loss_meter.values[0]
        largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
        if dtype == "fp32":
            assert abs(got_loss - float(loss)) < 1e-4 * abs(float(loss)), (all_t, got_loss, float(loss))
        else:
            assert abs(got_loss - float(loss)) < 1e-2 * abs(float(loss)), (all_t, got_loss, float(loss))
        for name, ref in grads.items():
            got = named[name].grad.double().cpu()
            if ref.abs().max().item() < 1e-6 * largest:
                # a convolution bias in front of a train-mode BatchNorm: its true gradient is zero
                if dtype == "fp32":
                    assert got.abs().max().item() < 1e-5 * largest, (all_t, name)
                continue
            if dtype == "fp32":
                l2 = _rel(got, ref)
                assert l2 < 1e-3, (all_t, name, l2)
            else:
                a, b = got.flatten(), ref.double().flatten()
                cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
                assert cos > (0.95 if got.dim() > 1 else 0.85), (all_t, name, cos)


def test_standalone_wide_gru():
    """AudioGRUModel(48, 512)(z) on its own: output, z.grad and the parameter gradients against a float64 nn.GRUCell loop with the
    same weights; reset_hidden=False carries the last hidden state into the next (forward-only) call."""
    B, E, V, H = 5, 48, 9, 512
    torch.manual_seed(8)
    gru = AudioGRUModel(input_size=E, hidden_size=H)
    cell = torch.nn.GRUCell(E, H).double()
    cell.load_state_dict({k: v.double() for k, v in gru.gruCell.state_dict().items()})
    z = torch.randn(B, E, V, generator=torch.Generator().manual_seed(9))
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(10))
    zr = z.double().requires_grad_(True)
    h = torch.zeros(B, H, dtype=torch.float64)
    for t in range(V):
        h = cell(zr[:, :, t], h)
    (h * dh.double()).sum().backward()
    gru = gru.to(DEV)
    zd = z.to(DEV).requires_grad_(True)
    out = gru(zd)
    assert rel_err(out, h) < 2e-5
    (out * dh.to(DEV)).sum().backward()
    assert rel_err(zd.grad, zr.grad) < 1e-4
    ref = dict(cell.named_parameters())
    for n, p_ in gru.gruCell.named_parameters():
        assert rel_err(p_.grad, ref[n].grad) < 1e-4, n
    # carried state: two forward calls == one float64 loop over both halves
    gru.reset_hidden = False
    gru.hidden = None
    z2 = torch.randn(B, E, V, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        gru(z.to(DEV))
        out2 = gru(z2.to(DEV))
        h = torch.zeros(B, H, dtype=torch.float64)
        for zz in (z, z2):
            for t in range(V):
                h = cell(zz[:, :, t].double(), h)
    assert rel_err(out2, h) < 2e-5


def test_full_size_wide_gru_bf16_vs_fp32():
    """AudioEncoder() + AudioGRUModel(512, 512), ar_size 512, at B = 256, V = 100, K = 12 (20480-sample clips): the bf16 loss within
    1e-3 of the exact-f32 one and every parameter gradient of the bf16 engine aligned with the f32 one (cosine > 0.99), and the
    whole-model gradient cosine > 0.995.  Both numbers are printed."""
    B, L = 256, 20480
    x = (torch.randn(B, L, generator=torch.Generator().manual_seed(1)) * 0.5).to(DEV)
    losses, grads = {}, {}
    for dtype in ("fp32", "bf16"):
        torch.manual_seed(0)
        model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 512), enc_size=512, ar_size=512,
                                           compute_dtype=dtype)
        with torch.no_grad():
            for n, p_ in model.named_parameters():
                if "encoder" in n and n.endswith("weight"):
                    p_.mul_(2.0)                               # non-degenerate scores
        model.to(DEV)
        eng = model.engine(B, L)
        assert type(eng.ctx).__name__ == "GRUContext"
        out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        losses[dtype] = float(out[0])
        assert torch.isfinite(model._flat_grad).all()
        grads[dtype] = {n: g.detach().double().cpu().flatten() for n, g in model._grad.items()}
        del eng, model
        torch.cuda.empty_cache()
    assert abs(losses["fp32"] - math.log(B)) > 0.05, losses
    loss_err = abs(losses["bf16"] - losses["fp32"]) / abs(losses["fp32"])
    a = torch.cat([grads["fp32"][n] for n in grads["fp32"]])
    b = torch.cat([grads["bf16"][n] for n in grads["fp32"]])
    whole = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
    print(f"H=512 full size: bf16 loss error vs exact f32 {loss_err:.2e}, whole-model gradient cosine {whole:.6f}")
    assert loss_err < 1e-3, losses
    assert whole > 0.995, whole
    for n, g32 in grads["fp32"].items():
        cos = float(torch.dot(g32, grads["bf16"][n]) / (g32.norm() * grads["bf16"][n].norm() + 1e-300))
        assert cos > 0.99, (n, cos)
