"""Difference scores on the HIP path (difference_score_function, reference contrastive_estimation_training.py:25-33):
the cpc_diff_scores / cpc_diff_scores_bwd / cpc_diff_scores_rank1 kernels against float64 references, the public autograd
function, and the engine route of ContrastiveEstimationTrainer.train / validate against the CPU oracle."""
import copy
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, difference_score_function,
                                                           softplus_score_function)
from oracle import cpc_oracle as O

DEV = torch.device("cuda:0")
L_ = C.c_longlong


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def _rel(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _rel_l2(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


def _elem_rel(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs() / ref.abs()).max().item()


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


# ------------------------------------------------------------------------------------------ host-side (no GPU)
def test_difference_scores_argument_checks_without_a_gpu():
    """The entry points refuse inconsistent arguments before any launch (-22), so this runs on a CPU-only host."""
    lib = _hip.lib()
    P, s = C.c_void_p(0x1000), C.c_void_p(0)
    # lds shorter than a score row
    assert lib.cpc_diff_scores(P, P, P, None, 8, 8, 64, L_(64), L_(64), 0, L_(0), L_(0), L_(0), L_(0), 1, 7, _hip.F32, s) == -22
    # ST needs lds >= M
    assert lib.cpc_diff_scores(P, P, P, P, 9, 8, 64, L_(64), L_(64), 0, L_(0), L_(0), L_(0), L_(0), 1, 8, _hip.F32, s) == -22
    # batched matrices that would overlap
    assert lib.cpc_diff_scores(P, P, P, None, 8, 8, 64, L_(64), L_(64), 0, L_(0), L_(64), L_(64), L_(63), 2, 8, _hip.F32, s) == -22
    assert lib.cpc_diff_scores(P, P, P, None, 8, 8, 64, L_(64), L_(64), 0, L_(0), L_(0), L_(0), L_(0), 1, 8, 7, s) == -22
    assert lib.cpc_diff_scores_bwd(P, P, P, P, None, P, 8, 8, 8, L_(0), 1, _hip.F32, s) == -22          # GT without ST
    assert lib.cpc_diff_scores_bwd(P, P, None, None, None, None, 8, 8, 8, L_(0), 1, _hip.F32, s) == -22  # no sums
    assert lib.cpc_diff_scores_rank1(P, P, P, 0, 64, 0, L_(0), L_(64), _hip.F32, s) == -22
    assert lib.cpc_diff_scores_rank1(P, P, P, 4, 64, -1, L_(0), L_(64), _hip.F32, s) == -22


def test_score_kind_and_refusals_without_a_gpu():
    from cpc_audio_amd.engine import score_kind
    assert score_kind(True) == "softplus" and score_kind(False) == "linear"
    assert score_kind(False, "difference") == "difference"
    with pytest.raises(ValueError):
        score_kind(False, "cosine")
    with pytest.raises(RuntimeError, match="GPU only"):
        difference_score_function(torch.randn(2, 2, 4), torch.randn(2, 4, 2))
    # the gradient penalty with difference scores stays refused
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                       prediction_steps=2)
    with pytest.raises(NotImplementedError):
        ContrastiveEstimationTrainer(model=model, dataset=None, score_function=difference_score_function, preprocessing=lambda x: x,
                                     wasserstein_gradient_penalty=True)
    tr = ContrastiveEstimationTrainer(model=model, dataset=None, score_function=difference_score_function)
    assert not tr._fused() and tr._engine_difference()
    tr.global_negatives = True
    assert not tr._engine_difference()
    tr.global_negatives = False
    tr.optimizer = torch.optim.SGD
    assert not tr._engine_difference()


# ------------------------------------------------------------------------------------------ kernels
def _operands(B, K, E, dt, seed, near=True):
    """predicted_z (B, K, E) and a top-layer-like buffer (B, Ltop, E) whose rows Ltop-1-K .. Ltop-1 are the targets (the engine's
    layout: a pad row behind them), in the storage dtype.  With ``near``, some targets differ from a prediction in two features only,
    by 2^-5 and 2^-6 (exact in bf16 too): squared distance 2^-10 + 2^-12 against |p|^2 ~ E, score ~800."""
    g = torch.Generator().manual_seed(seed)
    Ltop = K + 3
    T = Ltop - 1
    pred = torch.randn(B, K, E, generator=g).clamp(-3, 3).to(dt)
    top = torch.randn(B, Ltop, E, generator=g).clamp(-3, 3).to(dt)
    if near:
        for b in range(0, B, 3):
            for k in range(K):
                row = pred[b, k].float().clone()
                row[0] += 2.0 ** -5
                row[1] -= 2.0 ** -6
                top[(b + k) % B, T - K + k] = row.to(dt)
    targets = top[:, T - K:T, :].transpose(1, 2)
    return pred, top, targets, T, Ltop


def _launch_scores(pred_d, top_d, B, K, E, T, Ltop, all_t, code, with_t=True):
    R = B * K
    P = _hip.ptr
    if all_t:
        ld = -(-R // 8) * 8
        S = torch.full((R, ld), -7.0, device=DEV)
        ST = torch.full((R, ld), -7.0, device=DEV) if with_t else None
        _hip.call("cpc_diff_scores", P(pred_d), P(top_d, (T - K) * E), P(S), P(ST), R, R, E, L_(E), L_(E), K, L_(Ltop * E), L_(0), L_(0),
                  L_(0), 1, ld, code)
    else:
        ld = -(-B // 8) * 8
        S = torch.full((K, B, ld), -7.0, device=DEV)
        ST = torch.full((K, B, ld), -7.0, device=DEV) if with_t else None
        _hip.call("cpc_diff_scores", P(pred_d), P(top_d, (T - K) * E), P(S), P(ST), B, B, E, L_(K * E), L_(Ltop * E), 0, L_(0), L_(E),
                  L_(E), L_(B * ld), K, ld, code)
    return S, ST, ld


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,K,E", [(13, 1, 64), (13, 12, 512), (5, 12, 64), (37, 1, 512), (11, 3, 42)])
def test_diff_scores_kernel_against_float64(B, K, E, dt):
    """cpc_diff_scores in both layouts vs oracle.difference_scores in float64 on the same (storage-rounded) inputs: every score within
    1e-5 relative, including the near-coincident pairs where |p|^2 + |t|^2 - 2 p.t would cancel; pad columns untouched.
    (E = 42: the scalar-load path, E not a multiple of 4 nor of the 32-wide feature chunk.)"""
    pred, top, targets, T, Ltop = _operands(B, K, E, dt, seed=B * 100 + K * 10 + E)
    ref = O.difference_scores(pred.double(), targets.double())                                 # (B, K, B, K)
    R = B * K
    code = _hip.dtype_code(dt)
    pred_d, top_d = pred.to(DEV).contiguous(), top.to(DEV).contiguous()
    # score_over_all_timesteps: S [(b,k)][(b',k')] and its transpose
    S, ST, ld = _launch_scores(pred_d, top_d, B, K, E, T, Ltop, True, code)
    torch.cuda.synchronize()
    want = ref.reshape(R, R)
    assert _elem_rel(S[:, :R], want) < 1e-5
    assert torch.equal(ST[:, :R], S[:, :R].t())
    assert (S[:, R:] == -7.0).all() and (ST[:, R:] == -7.0).all()
    assert want.max() > 1e2            # the near-coincident pairs are in there
    # default branch: S[k][b][b'] = scores[b, k, b', k], ST[k][b'][b]
    S, ST, ld = _launch_scores(pred_d, top_d, B, K, E, T, Ltop, False, code)
    torch.cuda.synchronize()
    want = torch.diagonal(ref, dim1=1, dim2=3).permute(2, 0, 1)
    assert _elem_rel(S[:, :, :B], want) < 1e-5
    assert torch.equal(ST[:, :, :B], S[:, :, :B].transpose(1, 2))
    assert (S[:, :, B:] == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("all_t", [False, True])
@pytest.mark.parametrize("B,K,E", [(13, 12, 64), (7, 1, 512)])
def test_diff_scores_backward_against_float64(B, K, E, all_t):
    """cpc_diff_scores_bwd (G = 2 g s^2, row sums of G and of its transpose, in both layouts' row orders) and the gradient it leads to
    (the two contractions + cpc_diff_scores_rank1) vs float64 autograd of the oracle's score with a random upstream g: rel-L2 <= 1e-5."""
    pred, top, targets, T, Ltop = _operands(B, K, E, torch.float32, seed=7 + B + E, near=False)
    R = B * K
    p64, t64 = pred.double().requires_grad_(True), targets.double().detach().requires_grad_(True)
    s64 = O.difference_scores(p64, t64)
    g = torch.randn(B, K, B, K, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    if not all_t:
        mask = torch.zeros(B, K, B, K, dtype=torch.float64)
        torch.diagonal(mask, dim1=1, dim2=3).fill_(1.0)
        g = g * mask                          # the default branch's loss sees the K equal-step blocks only
    dp64, dt64 = torch.autograd.grad((s64 * g).sum(), (p64, t64))
    pred_d, top_d = pred.to(DEV).contiguous(), top.to(DEV).contiguous()
    S, ST, ld = _launch_scores(pred_d, top_d, B, K, E, T, Ltop, all_t, _hip.F32)
    P = _hip.ptr
    sums = torch.zeros(2, R, device=DEV)
    if all_t:
        G = torch.zeros(R, ld, device=DEV)
        G[:, :R] = g.reshape(R, R).float().to(DEV)
        GT = torch.zeros(R, ld, device=DEV)
        GT[:, :R] = G[:, :R].t()
        _hip.call("cpc_diff_scores_bwd", P(G), P(S), P(sums[0]), P(GT), P(ST), P(sums[1]), R, R, ld, L_(0), 1, _hip.F32)
        W = G[:, :R].double().cpu().view(B, K, B, K)
        assert torch.equal(GT[:, :R], G[:, :R].t())
    else:
        G = torch.zeros(K, B, ld, device=DEV)
        G[:, :, :B] = torch.diagonal(g, dim1=1, dim2=3).permute(2, 0, 1).float().to(DEV)
        GT = torch.zeros(K, B, ld, device=DEV)
        GT[:, :, :B] = G[:, :, :B].transpose(1, 2)
        _hip.call("cpc_diff_scores_bwd", P(G), P(S), P(sums[0]), P(GT), P(ST), P(sums[1]), B, B, ld, L_(B * ld), K, _hip.F32)
        W = torch.zeros(B, K, B, K, dtype=torch.float64)
        torch.diagonal(W, dim1=1, dim2=3).copy_(G[:, :, :B].double().cpu().permute(1, 2, 0))
        assert torch.equal(GT[:, :, :B], G[:, :, :B].transpose(1, 2))
    torch.cuda.synchronize()
    W_ref = 2.0 * g * s64.detach() ** 2
    assert _rel_l2(W, W_ref) < 1e-5
    mu, nu = sums[0].double().cpu(), sums[1].double().cpu()
    assert _rel_l2(mu, W_ref.sum(dim=(2, 3)).reshape(R)) < 1e-5          # rows of predicted_z, (b, k) order
    assert _rel_l2(nu, W_ref.sum(dim=(0, 1)).reshape(R)) < 1e-5          # rows of the targets, (b', k') order
    # the gradient: contractions in float64 here, the rank-1 terms by the kernel
    t_rows = targets.permute(0, 2, 1).reshape(R, E).double()
    dA = (W.reshape(R, R) @ t_rows).float().to(DEV)
    dT = (W.reshape(R, R).t() @ pred.reshape(R, E).double()).float().to(DEV)
    tgt_d = targets.permute(0, 2, 1).reshape(R, E).contiguous().to(DEV)
    _hip.call("cpc_diff_scores_rank1", P(sums[0]), P(pred_d), P(dA), R, E, 0, L_(0), L_(E), _hip.F32)
    # the targets' rows in the engine's top-layer layout: rows T-K+k of item b
    dtop = torch.zeros_like(top_d)
    dtop[:, T - K:T, :] = dT.view(B, K, E)
    _hip.call("cpc_diff_scores_rank1", P(sums[1]), P(top_d, (T - K) * E), P(dtop, (T - K) * E), R, E, K, L_(Ltop * E), L_(E), _hip.F32)
    _hip.call("cpc_diff_scores_rank1", P(sums[1]), P(tgt_d), P(dT), R, E, 0, L_(0), L_(E), _hip.F32)
    torch.cuda.synchronize()
    assert _rel_l2(dA.view(B, K, E), dp64) < 1e-5
    assert _rel_l2(dT.view(B, K, E).permute(0, 2, 1), dt64) < 1e-5
    assert torch.equal(dtop[:, T - K:T, :], dT.view(B, K, E))
    assert (dtop[:, :T - K] == 0).all() and (dtop[:, T:] == 0).all()


# ------------------------------------------------------------------------------------------ public function
@pytest.mark.gpu
def test_difference_score_function_directional_derivative():
    """gradcheck-style: <grad, v> of sum(g * scores) from the HIP backward vs a float64 central difference of the oracle along v."""
    B, K, E = 4, 2, 8
    gen = torch.Generator().manual_seed(11)
    p = torch.randn(B, K, E, generator=gen, dtype=torch.float64)
    t = torch.randn(B, E, K, generator=gen, dtype=torch.float64)
    g = torch.randn(B, K, B, K, generator=gen, dtype=torch.float64)
    vp, vt = torch.randn(B, K, E, generator=gen, dtype=torch.float64), torch.randn(B, E, K, generator=gen, dtype=torch.float64)
    pd = p.float().to(DEV).requires_grad_(True)
    td = t.float().to(DEV).requires_grad_(True)
    s = difference_score_function(pd, td)
    (s * g.float().to(DEV)).sum().backward()
    gp, gt = pd.grad.double().cpu(), td.grad.double().cpu()
    got = float((gp * vp).sum() + (gt * vt).sum())
    scale = float((gp * vp).abs().sum() + (gt * vt).abs().sum())
    f = lambda h: float((O.difference_scores(p + h * vp, t + h * vt) * g).sum())
    h = 1e-5
    want = (f(h) - f(-h)) / (2 * h)
    assert abs(got - want) <= 1e-5 * scale, (got, want, scale)


@pytest.mark.gpu
def test_difference_score_function_matches_the_broadcast_formula():
    """At B = 16 the scores and input gradients equal those of the reference's broadcast expression on the same inputs (rel 1e-5)."""
    B, K, E = 16, 12, 64
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(B, K, E, generator=gen).to(DEV)
    t0 = torch.randn(B, E, K, generator=gen).to(DEV)
    g = torch.randn(B, K, B, K, generator=gen).to(DEV)
    p1, t1 = p0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    s1 = difference_score_function(p1, t1)
    (s1 * g).sum().backward()
    p2, t2 = p0.double().requires_grad_(True), t0.double().requires_grad_(True)
    diff = p2.unsqueeze(3).unsqueeze(4) - t2.permute(1, 0, 2).unsqueeze(0).unsqueeze(1)        # reference :25-33
    s2 = 1 / torch.sum(diff ** 2, dim=2)
    (s2 * g.double()).sum().backward()
    assert s1.shape == (B, K, B, K)
    assert _rel(s1, s2) < 1e-5
    assert _rel(p1.grad, p2.grad) < 1e-5
    assert _rel(t1.grad, t2.grad) < 1e-5


@pytest.mark.gpu
def test_difference_score_function_memory_at_bench_size():
    """B = 256, K = 12, E = 512: forward + backward raise the peak allocation by < 1 GB (the broadcast formula needs ~19 GB)."""
    B, K, E = 256, 12, 512
    gen = torch.Generator(device=DEV).manual_seed(1)
    p = torch.randn(B, K, E, device=DEV, generator=gen).requires_grad_(True)
    t = torch.randn(B, E, K, device=DEV, generator=gen).requires_grad_(True)
    g = torch.randn(B, K, B, K, device=DEV, generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    s = difference_score_function(p, t)
    (s * g).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print(f"difference_score_function B={B} K={K} E={E}: peak +{peak / 2**20:.1f} MiB")
    assert peak < 2**30
    assert torch.isfinite(p.grad).all() and torch.isfinite(t.grad).all()


# ------------------------------------------------------------------------------------------ trainer / engine
def _small_model(g, meta, dtype):
    C_, H, K, V = meta["C"], meta["H"], meta["K"], meta["V"]
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    ar = AudioGRUModel(input_size=C_, hidden_size=H)
    model = AudioPredictiveCodingModel(enc, ar, enc_size=C_, ar_size=H, visible_steps=V, prediction_steps=K, compute_dtype=dtype)
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model.load_state_dict(state)
    return model.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("all_t", [False, True])
def test_trainer_engine_route_with_difference_scores(golden_dir, all_t):
    """difference_score_function + Adam takes the engine route (one cpc_diff_scores launch per step, FusedAdam, device NaN guard):
    two fp32 steps against OracleTrainer(score="difference") with the generic-route test's bounds."""
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    data = torch.from_numpy(g["data"])
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    random.seed(5)
    batches = [list(b) for b in FileBatchSampler([data.shape[0]], meta["B"], 1, True, verbose=False)]
    steps, lr = 2, 1e-3
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.5, score_over_all_timesteps=all_t, score_function=difference_score_function,
                                      prediction_steps=meta["K"], ar_size=meta["H"])
    tr.verbose = False
    assert tr._engine_difference() and not tr._fused()
    timer = _hip.KernelTimer(only=["cpc_diff_scores"])
    random.seed(5)
    _hip.set_timer(timer)
    try:
        tr.train(batch_size=meta["B"], epochs=1, lr=lr, num_workers=0, max_steps=steps)
        launches = timer.summary().get("cpc_diff_scores", (0, 0.0, 0.0))[0]
    finally:
        _hip.set_timer(None)
    assert launches == steps
    assert hasattr(tr, "last_optimizer")            # FusedAdam: the engine route
    ot = O.OracleTrainer(params, meta["V"], meta["K"], score="difference", all_timesteps=all_t, regularization=0.5, lr=lr)
    for i in range(steps):
        loss, smax = ot.step(data[batches[i]])
        assert abs(logger.loss_meter.values[i] - float(loss)) < 2e-4 * abs(float(loss)), i
        assert abs(logger.score_meter.values[i] - float(smax)) < 2e-4 * abs(float(smax)) + 1e-6, i
    for k, v in model.state_dict().items():
        ref = ot.params[k].detach()
        err = (v.cpu() - ref).abs()
        assert err.max().item() <= 2 * lr * steps * 1.01 + 1e-6, k
        tight = err <= 0.05 * lr * steps + 1e-4 * ref.abs()
        assert tight.float().mean().item() > 0.97, (k, tight.float().mean().item())


@pytest.mark.gpu
@pytest.mark.parametrize("all_t", [False, True])
def test_engine_difference_gradients_against_oracle(golden_dir, all_t):
    """One fp32 engine step (lr 0): loss and every parameter gradient vs the oracle's autograd of the difference score."""
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    data = torch.from_numpy(g["data"])
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model = _small_model(g, meta, "fp32")
    x = data[:meta["B"]]
    eng = model.engine(meta["B"], x.shape[1])
    out = eng.loss_and_grads(x.to(DEV), softplus=False, regularization=0.5, all_timesteps=all_t, score="difference")
    torch.cuda.synchronize()
    ot = O.OracleTrainer(params, meta["V"], meta["K"], score="difference", all_timesteps=all_t, regularization=0.5)
    loss, smax, grads = ot.loss_and_grads(x)
    assert abs(float(out[0]) - float(loss)) < 1e-4 * abs(float(loss))
    for name, ref in grads.items():
        assert _rel_l2(model._grad[name], ref) < 1e-3, name


@pytest.mark.gpu
@pytest.mark.parametrize("all_t", [False, True])
def test_engine_difference_bf16(golden_dir, all_t):
    """bf16 storage (G = 2 g s^2 stored as bf16, the operand type of the contractions; its sums of the rounded values): one engine
    step vs the fp32 oracle.  Measured on MI355X: loss within 3.3e-7 / 7.5e-7 (default / all timesteps), worst per-parameter gradient
    relative L2 8.6e-2 / 8.7e-2 (encoder.layers.1.bias, after five layers of bf16 gradients).  Bounds: loss 1e-3, gradients 0.12
    (the bf16 train test of test_model_gpu.py)."""
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    data = torch.from_numpy(g["data"])
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model = _small_model(g, meta, "bf16")
    x = data[:meta["B"]]
    eng = model.engine(meta["B"], x.shape[1])
    out = eng.loss_and_grads(x.to(DEV), softplus=False, regularization=0.5, all_timesteps=all_t, score="difference")
    torch.cuda.synchronize()
    ot = O.OracleTrainer(params, meta["V"], meta["K"], score="difference", all_timesteps=all_t, regularization=0.5)
    loss, smax, grads = ot.loss_and_grads(x)
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((_rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    print(f"bf16 difference scores all_timesteps={all_t}: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]})")
    assert rel < 1e-3
    assert worst[0] < 0.12, worst


def _scalogram_model(g, meta):
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["E"], hidden_size=meta["H"]), enc_size=meta["E"],
                                       ar_size=meta["H"], visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype="fp32")
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model.load_state_dict(state)
    return pre.to(DEV), model.to(DEV), blocks


@pytest.mark.gpu
@pytest.mark.parametrize("all_t", [False, True])
def test_scalogram_trainer_engine_route_with_difference_scores(golden_dir, all_t):
    """ScalogramCPCEngine (CQT scalogram + residual encoder + GRU, scalogram_model fixture): the difference preset's engine step,
    loss and all parameter gradients vs the oracle (lr 0, one step)."""
    g = _load(golden_dir, "scalogram_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    B, K, H, V = meta["B"], meta["K"], meta["H"], meta["V"]
    pre, model, blocks = _scalogram_model(g, meta)
    model.train()
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    data = torch.from_numpy(g["data"])
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.1, score_over_all_timesteps=all_t, score_function=difference_score_function,
                                      prediction_steps=K, ar_size=H, preprocessing=pre)
    tr.verbose = False
    assert tr._engine_difference()
    random.seed(91)
    idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
    random.seed(91)
    timer = _hip.KernelTimer(only=["cpc_diff_scores"])
    _hip.set_timer(timer)
    try:
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
        launches = timer.summary().get("cpc_diff_scores", (0, 0.0, 0.0))[0]
    finally:
        _hip.set_timer(None)
    assert launches == 1
    with torch.no_grad():
        scal = pre(data[idx].to(DEV).unsqueeze(1)).cpu()
    oblocks = [dict(b) for b in blocks]
    oblocks[0]["in_channels"] = 2
    ot = O.OracleTrainer(params, V, K, score="difference", all_timesteps=all_t, regularization=0.1, lr=0.0, scalogram=oblocks)
    loss, smax, grads = ot.loss_and_grads(scal)
    assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss)), (logger.loss_meter.values, float(loss))
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for name, ref in grads.items():
        got = dict(model.named_parameters())[name].grad.double().cpu()
        if ref.abs().max().item() < 1e-6 * largest:
            assert got.abs().max().item() < 1e-5 * largest, name
            continue
        assert _rel_l2(got, ref) < 1e-3, name


@pytest.mark.gpu
@pytest.mark.parametrize("all_t", [False, True])
def test_validate_with_difference_scores(golden_dir, all_t):
    """validate() routes difference scores through eng.nce_eval: per-step losses and accuracies and the mean score vs the oracle
    over the same FileBatchSampler(seed=0, file_batch_size=8) batches (1e-4)."""
    g = _load(golden_dir, "validate.npz")
    meta = json.load(open(os.path.join(golden_dir, "validate.json")))
    data = torch.from_numpy(g["data"])
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model = _small_model(g, meta, "fp32")
    B, K, V = meta["B"], meta["K"], meta["V"]
    tr = ContrastiveEstimationTrainer(model=model, dataset=None, validation_set=TensorAudioDataset(data, counts=meta["counts"], device=DEV),
                                      device=DEV, score_over_all_timesteps=all_t, score_function=difference_score_function,
                                      prediction_steps=K, ar_size=meta["H"])
    tr.verbose = False
    calls = []
    real = _hip.call

    def spy(name, *a, **kw):
        calls.append(name)
        return real(name, *a, **kw)

    _hip.call = spy
    try:
        losses, acc, score, mi = tr.validate(batch_size=B, num_workers=0)
    finally:
        _hip.call = real
    assert "cpc_diff_scores" in calls
    want_l, want_a, want_s = 0.0, 0.0, 0.0
    lists = O.file_batch_sampler(meta["counts"], B, 8, True, seed=0)
    for idx in lists:
        pred, targ, _, _ = O.cpc_forward(data[idx].unsqueeze(1), params, V, K, training=False)
        pl, pa, ms = O.validation_terms(O.difference_scores(pred.double(), targ.double()), all_t)
        want_l, want_a, want_s = want_l + pl, want_a + pa, want_s + float(ms)
    n = len(lists)
    assert _rel(losses, want_l / n) < 1e-4
    assert (acc.cpu().double() - want_a / n).abs().max().item() < 1e-4
    assert abs(score - want_s / n) < 1e-4 * max(1.0, abs(want_s / n))


@pytest.mark.gpu
def test_difference_refusals_on_the_engine(golden_dir):
    """Difference scores under global negatives keep the generic route (the engine refuses them); the trainer's generic route still
    trains them (one step against the oracle)."""
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    data = torch.from_numpy(g["data"])
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model = _small_model(g, meta, "fp32")
    eng = model.engine(meta["B"], data.shape[1])
    with pytest.raises(NotImplementedError):
        eng.loss_and_grads(data[:meta["B"]].to(DEV), softplus=False, regularization=0.5, score="difference", global_negatives=object())
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.5, score_function=difference_score_function, prediction_steps=meta["K"],
                                      ar_size=meta["H"])
    tr.verbose = False
    tr.global_negatives = True
    assert not tr._engine_difference()
    random.seed(5)
    batches = [list(b) for b in FileBatchSampler([data.shape[0]], meta["B"], 1, True, verbose=False)]
    random.seed(5)
    tr.train(batch_size=meta["B"], epochs=1, lr=0.0, num_workers=0, max_steps=1)
    assert not hasattr(tr, "last_optimizer")
    ot = O.OracleTrainer(params, meta["V"], meta["K"], score="difference", regularization=0.5, lr=0.0)
    loss, _, _ = ot.loss_and_grads(data[batches[0]])
    assert abs(logger.loss_meter.values[0] - float(loss)) < 2e-4 * abs(float(loss))
    # the softplus preset is unchanged by the score keyword
    tr2 = ContrastiveEstimationTrainer(model=model, dataset=None, score_function=softplus_score_function)
    assert tr2._fused() and tr2._score_kind() == "softplus"
