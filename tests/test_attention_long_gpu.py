"""The attention core for sequences of up to 128 steps (cpc_attn128_fwd / _bwd / _tangent / _gp) and the routes that use it: the
AttentionContext of the engines at visible_steps > 64 and the stand-alone TransformerEncoder(Layer) calls at S > 64.

Kernels against float64 autograd of the causal-softmax definition (tolerances of test_hip_kernels.py's attention tests), the penalty
kernels against the float64 formulas of tools/gp_attention_algebra.py, models against the oracle and the reference fixture
attention_long.npz (tests/golden/generate_attention_long.py).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.attention_model import AttentionModel  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioPredictiveCodingModel  # noqa: E402
from oracle import cpc_oracle as O  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
SEQS = [1, 37, 64, 65, 100, 127, 128]
# (C, heads): head size 64 (the matrix pipe in bf16), 32 and 8 (vector kernels)
SHAPES = [(128, 2), (64, 2), (64, 8)]
GUARD = 64          # sentinel elements behind every output
SENT = -7.5         # (exact in bf16)


def tol(dt):
    return 3e-5 if dt == torch.float32 else 1.2e-2


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def rounded(t, dt):
    return t.to(dt).double()


def guarded(n, dt, fill=float("nan")):
    """A device buffer of n elements followed by GUARD sentinel elements; returns (whole buffer, view of the first n)."""
    buf = torch.full((n + GUARD,), fill, device=DEV, dtype=dt)
    buf[n:] = SENT
    return buf, buf[:n]


def guard_intact(buf, n):
    return bool((buf[n:].float() == SENT).all())


def _reference(B, S, C, heads, dt, p_drop, seed, site, gen):
    d = C // heads
    qkv = rounded(torch.randn(B * S, 3 * C, generator=gen), dt).requires_grad_(True)
    dout = rounded(torch.randn(B * S, C, generator=gen), dt)
    if p_drop:
        mask = torch.empty(B * heads * S * S, device=DEV)
        _hip.call("cpc_dropout_mask", _hip.ptr(mask), mask.numel(), p_drop, seed, site)
        m = mask.cpu().double().reshape(B, heads, S, S)
    else:
        m = torch.ones(B, heads, S, S, dtype=torch.double)
    q, k, v = (t.reshape(B, S, heads, d).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1))
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(d) + torch.triu(torch.full((S, S), float("-inf"), dtype=torch.double), 1)
    P = torch.softmax(sc, -1)
    out = ((P * m) @ v).permute(0, 2, 1, 3).reshape(B * S, C)
    out.backward(dout)
    return qkv, dout, P, out


# --------------------------------------------------------------------------------------- forward / backward
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C,heads", SHAPES)
@pytest.mark.parametrize("S", SEQS)
def test_attn128_fwd_bwd(S, C, heads, dt, p_drop):
    """cpc_attn128_fwd / cpc_attn128_bwd vs autograd of the definition; P rows sum to 1 and are exactly zero above the diagonal;
    nothing is written past P, out or dqkv."""
    B, seed, site = 3, 987654321, 4
    g = torch.Generator().manual_seed(S * 7 + C + heads)
    qkv, dout, P, out = _reference(B, S, C, heads, dt, p_drop, seed, site, g)
    code = _hip.dtype_code(dt)
    d_qkv = qkv.detach().to(dt).to(DEV).contiguous()
    d_dout = dout.to(dt).to(DEV).contiguous()
    ob, o = guarded(B * S * C, dt)
    pb, Pd = guarded(B * heads * S * S, dt)
    _hip.call("cpc_attn128_fwd", _hip.ptr(d_qkv), _hip.ptr(o), _hip.ptr(Pd), B, S, C, heads, p_drop, seed, site, code)
    torch.cuda.synchronize()
    assert guard_intact(ob, B * S * C) and guard_intact(pb, B * heads * S * S)
    assert rel_err(o.view(B * S, C), out) < tol(dt)
    Pg = Pd.view(B * heads, S, S)
    assert rel_err(Pg, P.reshape(B * heads, S, S)) < tol(dt)          # the saved weights stay undropped
    upper = torch.triu(torch.ones(S, S, dtype=torch.bool, device=DEV), 1)
    assert bool((Pg[:, upper] == 0).all())
    assert (Pg.double().sum(-1) - 1).abs().max().item() < (1e-5 if dt == torch.float32 else 2e-2)
    db, dq = guarded(B * S * 3 * C, dt)
    _hip.call("cpc_attn128_bwd", _hip.ptr(d_qkv), _hip.ptr(Pd), _hip.ptr(d_dout), _hip.ptr(dq), B, S, C, heads, p_drop, seed, site, code)
    torch.cuda.synchronize()
    assert guard_intact(db, B * S * 3 * C)
    assert rel_err(dq.view(B * S, 3 * C), qkv.grad) < (1e-4 if dt == torch.float32 else 2.5e-2)


@pytest.mark.parametrize("dt", DTYPES)
def test_attn128_agrees_with_short_kernels_at_64_steps(dt):
    """At S <= 64 both cores compute the same function: results within rounding of each other (head sizes 64 and 32)."""
    for C, heads, S in ((512, 8, 60), (64, 2, 64)):
        B = 4
        g = torch.Generator().manual_seed(C + S)
        code = _hip.dtype_code(dt)
        qkv = torch.randn(B * S, 3 * C, generator=g).to(dt).to(DEV)
        dout = torch.randn(B * S, C, generator=g).to(dt).to(DEV)
        res = {}
        for abi in ("cpc_attn", "cpc_attn128"):
            o = torch.empty(B * S, C, device=DEV, dtype=dt)
            Pd = torch.empty(B * heads, S, S, device=DEV, dtype=dt)
            dq = torch.empty(B * S, 3 * C, device=DEV, dtype=dt)
            _hip.call(abi + "_fwd", _hip.ptr(qkv), _hip.ptr(o), _hip.ptr(Pd), B, S, C, heads, 0.2, 5, 1, code)
            _hip.call(abi + "_bwd", _hip.ptr(qkv), _hip.ptr(Pd), _hip.ptr(dout), _hip.ptr(dq), B, S, C, heads, 0.2, 5, 1, code)
            res[abi] = (o, Pd, dq)
        for a, b in zip(res["cpc_attn"], res["cpc_attn128"]):
            assert rel_err(b, a) < (1e-5 if dt == torch.float32 else 2.5e-2)


# --------------------------------------------------------------------------------------- gradient-penalty kernels
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("C,heads", [(128, 2), (64, 8)])
@pytest.mark.parametrize("S", [65, 100, 128])
def test_attn128_gradient_penalty_kernels(S, C, heads, p_drop):
    """cpc_attn128_tangent / cpc_attn128_gp (f32) against the float64 formulas (restated from test_hip_kernels.py's
    test_attention_gradient_penalty_kernels and tools/gp_attention_algebra.py): out_t = (pt m) v + (P m) vt with pt = P (u - <P,u>),
    u = scale (qt k^T + q kt^T); and dqkv += the second-order terms for the adjoint dO at the output."""
    B = 2
    g = torch.Generator().manual_seed(S + C + heads)
    d, M, seed, site = C // heads, B * S, 1234567, 5
    f64 = lambda *sh: torch.randn(*sh, generator=g).float().double()
    qkv, qkvt, dO, lam = f64(M, 3 * C), f64(M, 3 * C), f64(M, C), f64(M, 3 * C)
    hd = lambda t: t.reshape(B, S, heads, d).permute(0, 2, 1, 3)
    un = lambda t: t.permute(0, 2, 1, 3).reshape(M, C)
    q, k, v = (hd(t) for t in qkv.split(C, 1))
    qt, kt, vt = (hd(t) for t in qkvt.split(C, 1))
    causal = torch.tril(torch.ones(S, S)).bool()
    sc = 1.0 / math.sqrt(d)
    P = torch.softmax(((q @ k.transpose(-1, -2)) * sc).masked_fill(~causal, float("-inf")), -1)
    mask = torch.ones(B * heads * S * S, device=DEV)
    if p_drop:
        _hip.call("cpc_dropout_mask", _hip.ptr(mask), mask.numel(), p_drop, seed, site)
    m = mask.cpu().double().reshape(B, heads, S, S)
    u = ((qt @ k.transpose(-1, -2) + q @ kt.transpose(-1, -2)) * sc).masked_fill(~causal, 0.0)
    mrow = (P * u).sum(-1, keepdim=True)
    pt = P * (u - mrow)
    out_t = un((pt * m) @ v + (P * m) @ vt)
    a = m * (hd(dO) @ v.transpose(-1, -2))
    cc = (P * a).sum(-1, keepdim=True)
    dS = P * (a - cc)
    w = m * (hd(dO) @ vt.transpose(-1, -2)) + (a - cc) * (u - mrow)
    sig = P * (w - (P * w).sum(-1, keepdim=True))
    src = torch.cat([un(sc * (sig @ k + dS @ kt)), un(sc * (sig.transpose(-1, -2) @ q + dS.transpose(-1, -2) @ qt)),
                     un((pt * m).transpose(-1, -2) @ hd(dO))], 1)
    to = lambda t: t.float().to(DEV).contiguous()
    d_qkv, d_qkvt, d_dO, d_P = to(qkv), to(qkvt), to(dO), to(P.reshape(B * heads, S, S))
    ob, o = guarded(M * C, torch.float32)
    _hip.call("cpc_attn128_tangent", _hip.ptr(d_qkv), _hip.ptr(d_qkvt), _hip.ptr(d_P), _hip.ptr(o), B, S, C, heads, p_drop, seed, site)
    torch.cuda.synchronize()
    assert guard_intact(ob, M * C)
    assert rel_err(o.view(M, C), out_t) < 1e-5
    ab, acc = guarded(M * 3 * C, torch.float32)
    acc.copy_(to(lam).view(-1))
    _hip.call("cpc_attn128_gp", _hip.ptr(d_qkv), _hip.ptr(d_qkvt), _hip.ptr(d_P), _hip.ptr(d_dO), _hip.ptr(acc), B, S, C, heads, p_drop,
              seed, site)
    torch.cuda.synchronize()
    assert guard_intact(ab, M * 3 * C)
    assert rel_err(acc.view(M, 3 * C).double().cpu() - lam, src) < 1e-4


# --------------------------------------------------------------------------------------- refusals
def test_attn128_refuses_unsupported_shapes():
    x = torch.zeros(16, device=DEV)
    p = _hip.ptr(x)
    for B, S, C, heads in ((1, 0, 64, 1), (1, 129, 64, 1), (1, 8, 256, 2), (1, 8, 60, 8), (0, 8, 64, 1)):
        with pytest.raises(_hip.HipCallError):
            _hip.call("cpc_attn128_fwd", p, p, p, B, S, C, heads, 0.0, 0, 0, 0)
        with pytest.raises(_hip.HipCallError):
            _hip.call("cpc_attn128_bwd", p, p, p, p, B, S, C, heads, 0.0, 0, 0, 1)
        with pytest.raises(_hip.HipCallError):
            _hip.call("cpc_attn128_tangent", p, p, p, p, B, S, C, heads, 0.0, 0, 0)
        with pytest.raises(_hip.HipCallError):
            _hip.call("cpc_attn128_gp", p, p, p, p, p, B, S, C, heads, 0.0, 0, 0)


def test_model_refuses_129_visible_steps():
    ar = AttentionModel({'channels': 64, 'output_size': 32, 'num_layers': 1, 'num_heads': 1, 'feedforward_size': 64,
                         'sequence_length': 160, 'dropout': 0.0})
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, ar, enc_size=64, ar_size=32, visible_steps=129, prediction_steps=4,
                                       compute_dtype="fp32").to(DEV)
    with pytest.raises(NotImplementedError):
        model.engine(2, 465 + (129 + 4) * 160 + 3)


# --------------------------------------------------------------------------------------- models
from cpc_audio_amd.audio_dataset import TensorAudioDataset  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,  # noqa: E402
                                                           softplus_score_function)

SCORE = {"softplus": softplus_score_function, "linear": linear_score_function}


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


def _rel(got, ref):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "attention_long.npz"))
    g = {k: z[k] for k in z.files}
    meta = json.load(open(os.path.join(golden_dir, "attention_long.json")))
    return g, meta


def _long_model(g, meta, dtype, dropout=None, V=None):
    """AudioEncoder (small channel counts) + AttentionModel (head size 64, sequence_length 128) with the fixture's parameters."""
    ar = dict(meta["ar"]) if dropout is None else dict(meta["ar"], dropout=dropout)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': meta["enc_channels"], 'bias': True})
    model = AudioPredictiveCodingModel(enc, AttentionModel(ar), enc_size=meta["C"], ar_size=meta["H"], visible_steps=V or meta["V"],
                                       prediction_steps=meta["K"], compute_dtype=dtype)
    state = model.state_dict()
    fixed = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    assert set(fixed) == {k for k in state if not k.endswith("positional_encoder.pe")}
    state.update(fixed)
    model.load_state_dict(state)
    return model.to(DEV)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attention_long_model_matches_reference(golden_dir, dtype):
    """visible_steps = 100 with an AttentionModel context (head size 64, sequence_length 128): forward outputs, trainer losses of
    softplus and linear scores in both branches and the parameter gradients against the reference fixture attention_long.npz.
    bf16: loss within 2e-2 as test_model_gpu.py's attention test; gradients within 0.2 (l2, relative) instead of its 0.12, because this
    fixture's 8-channel encoder layers round more in bf16: measured against the exact-f32 engine, the worst gradients (encoder layer 1,
    first in_proj weight) are 0.15 off at V = 60 on the short-sequence kernels and the same at V = 100."""
    g, meta = _fixture(golden_dir)
    B, K, H = meta["B"], meta["K"], meta["H"]
    data = torch.from_numpy(g["data"])
    model = _long_model(g, meta, dtype)
    assert model.engine(B, data.shape[1]).ctx.attn_abi == "cpc_attn128"
    tol = 2e-4 if dtype == "fp32" else 4e-2
    with torch.no_grad():
        pz, tg, z, c = model(data.unsqueeze(1).to(DEV))
    assert _rel(c, g["fwd/c"]) < tol and _rel(pz, g["fwd/predicted_z"]) < tol
    for run in meta["runs"]:
        model = _long_model(g, meta, dtype)
        logger = _Logger()
        tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                          regularization=run["reg"], score_over_all_timesteps=run["all_timesteps"],
                                          score_function=SCORE[run["score"]], prediction_steps=K, ar_size=H)
        tr.verbose = False
        tr.train(batch_size=B, epochs=1, lr=1e-4, num_workers=0, max_steps=1)
        ltol = 1e-4 if dtype == "fp32" else 2e-2
        assert abs(logger.loss_meter.values[0] - run["loss"]) <= ltol * abs(run["loss"]), (run["tag"], logger.loss_meter.values, run["loss"])
        if run["grads"]:
            params = dict(model.named_parameters())
            for k in [k for k in g if k.startswith(run["tag"] + "/grad/")]:
                name = k.split("/grad/")[1]
                l2 = _rel(params[name].grad, g[k])
                assert l2 < (1e-3 if dtype == "fp32" else 0.2), (run["tag"], name, l2)


def test_full_size_attention_context_v100_bf16_vs_fp32():
    """attention_architecture_1 (sequence_length 100) behind the 512-channel AudioEncoder, 100 visible / 12 prediction steps, batch
    32, dropout off: bf16 vs exact-f32 (loss within 1e-3 relative, gradient cosines > 0.97), both on the cpc_attn128_* kernels."""
    from cpc_audio_amd import configs
    B, V, K, L = 32, 100, 12, 20480
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, L, generator=g).to(DEV)
    res = {}
    for dtype in ("fp32", "bf16"):
        torch.manual_seed(0)
        ar = AttentionModel(dict(configs.fresh(configs.attention_architecture_1), dropout=0.0, sequence_length=100))
        model = AudioPredictiveCodingModel(AudioEncoder(), ar, enc_size=512, ar_size=256, visible_steps=V, prediction_steps=K,
                                           compute_dtype=dtype).to(DEV)
        eng = model.engine(B, L)
        assert eng.ctx.attn_abi == "cpc_attn128"
        out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        res[dtype] = (float(out[0]), model)
    assert abs(res["bf16"][0] - res["fp32"][0]) <= 1e-3 * abs(res["fp32"][0])
    for n in res["fp32"][1]._grad:
        a, b = res["fp32"][1]._grad[n].double().flatten(), res["bf16"][1]._grad[n].double().flatten()
        if a.norm() > 0:
            cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
            assert cos > 0.97, (n, cos)


def test_attention_long_train_and_validate_against_oracle(golden_dir):
    """train() for three Adam steps at visible_steps = 100 against the oracle's steps from the same parameters (every batch is the
    whole four-item set, so the sampler's order does not matter), then validate() against the oracle's validation terms with the
    oracle's updated parameters.  (Adam turns gradient differences at rounding level into parameter differences of up to lr where a
    gradient is near zero: the parameters themselves are judged through the losses they give.)"""
    g, meta = _fixture(golden_dir)
    K, H, V, L = meta["K"], meta["H"], meta["V"], meta["L"]
    layers, heads = meta["ar"]["num_layers"], meta["ar"]["num_heads"]
    B, steps, lr = 4, 3, 2e-4
    gen = torch.Generator().manual_seed(5)
    data = torch.randn(B, L, generator=gen) * 0.5
    model = _long_model(g, meta, "fp32")
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    ot = O.OracleTrainer(params, V, K, score="softplus", all_timesteps=False, regularization=1.0, lr=lr, attention=(layers, heads))
    want = [ot.step(data)[0] for _ in range(steps)]
    val = torch.randn(16, L, generator=gen) * 0.5
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=1.0, score_over_all_timesteps=False, score_function=softplus_score_function,
                                      prediction_steps=K, ar_size=H, validation_set=TensorAudioDataset(val, device=DEV))
    tr.verbose = False
    tr.train(batch_size=B, epochs=steps, lr=lr, num_workers=0, max_steps=steps)
    got = logger.loss_meter.values
    assert len(got) == steps
    for i in range(steps):
        assert abs(got[i] - want[i]) <= 1e-4 * abs(want[i]) * (1 + 4 * i), (i, got, want)
    losses, acc, score, mi = tr.validate(batch_size=8, num_workers=0)
    oparams = {**{k: v.detach() for k, v in ot.params.items()}, **ot.buffers}
    want_l, want_a = 0.0, 0.0
    lists = O.file_batch_sampler([val.shape[0]], 8, 8, True, seed=0)
    for idx in lists:
        pred, targ, _, _ = O.cpc_forward(val[idx].unsqueeze(1), oparams, V, K, attention=(layers, heads), training=False)
        pl, pa, _ = O.validation_terms(O.softplus_scores(pred.double(), targ.double()), False)
        want_l, want_a = want_l + pl, want_a + pa
    n = len(lists)
    assert n > 0
    assert _rel(losses, want_l / n) < 1e-4 * (1 + 4 * steps)         # after the steps: the bound of the last step's loss
    assert (torch.as_tensor(acc).cpu().double() - want_a / n).abs().max().item() < 1e-4


def test_attention_long_dropout_against_oracle_with_same_masks(golden_dir):
    """Train-mode dropout (p = 0.2) at visible_steps = 100: the device masks (cpc_dropout_mask of the engine's seed and sites) handed
    to the oracle; loss and every gradient must agree (fp32)."""
    g, meta = _fixture(golden_dir)
    C, K, V = meta["C"], meta["K"], meta["V"]
    layers, heads, FF = meta["ar"]["num_layers"], meta["ar"]["num_heads"], meta["ar"]["feedforward_size"]
    p_drop, B = 0.2, meta["B"]
    model = _long_model(g, meta, "fp32", dropout=p_drop).train()
    x = torch.from_numpy(g["data"]).to(DEV)
    eng = model.engine(B, x.shape[1])
    eng.ctx.fixed_seed = 4321
    out = eng.loss_and_grads(x.contiguous(), softplus=True, regularization=1.0)
    seed, S = eng.ctx.drop_seed, V

    def factors(n, site):
        m = torch.empty(n, device=DEV)
        _hip.call("cpc_dropout_mask", _hip.ptr(m), n, p_drop, seed, site)
        return m.cpu()

    df = {}
    for l in range(layers):
        df[(l, 0)] = factors(B * heads * S * S, 4 * l + 0).view(B * heads, S, S)
        df[(l, 1)] = factors(B * S * C, 4 * l + 1).view(B, S, C).transpose(0, 1)
        df[(l, 2)] = factors(B * S * FF, 4 * l + 2).view(B, S, FF).transpose(0, 1)
        df[(l, 3)] = factors(B * S * C, 4 * l + 3).view(B, S, C).transpose(0, 1)
    params = {k: v.detach().clone().cpu().requires_grad_(True) for k, v in model.state_dict().items()
              if not k.endswith("positional_encoder.pe")}
    pz, tg, _, _ = O.cpc_forward(x.cpu().unsqueeze(1), params, V, K, attention=(layers, heads, df))
    loss, _ = O.info_nce_loss(O.softplus_scores(pz, tg), False, 1.0)
    loss.backward()
    assert abs(float(out[0]) - float(loss.detach())) < 2e-4 * abs(float(loss.detach()))
    for n in params:
        l2 = _rel(model._grad[n], params[n].grad)
        assert l2 < 2e-3, (n, l2)


def _gp_model(golden_dir, dtype, p_drop):
    """The penalty fixture's scalogram encoder (scalogram_model_gp_att) with its AttentionModel context (8 heads of 8 channels) at
    visible_steps = 100, sequence_length 128: the encoder parameters from the fixture, the context's too (the positional table is
    rebuilt for the longer sequence)."""
    import copy
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    z = np.load(os.path.join(golden_dir, "scalogram_model_gp_att.npz"))
    meta = copy.deepcopy(json.load(open(os.path.join(golden_dir, "scalogram_model_gp_att.json"))))
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    att = dict(meta["attention"], sequence_length=128, dropout=p_drop)
    model = AudioPredictiveCodingModel(enc, AttentionModel(att), enc_size=meta["E"], ar_size=meta["H"], visible_steps=100,
                                       prediction_steps=meta["K"], compute_dtype=dtype)
    state = model.state_dict()
    for k in z.files:
        name = k[len("param/"):]
        if k.startswith("param/") and not name.endswith("positional_encoder.pe"):
            state[name] = torch.from_numpy(z[k])
    model.load_state_dict(state)
    oblocks = copy.deepcopy(blocks)
    oblocks[0]["in_channels"] = 2
    return pre.to(DEV), model.to(DEV), meta, att, oblocks


@pytest.mark.parametrize("dtype,p_drop", [("fp32", 0.0), ("fp32", 0.25), ("bf16", 0.0)])
def test_attention_long_gradient_penalty_against_oracle(golden_dir, dtype, p_drop):
    """The Wasserstein gradient penalty through an AttentionModel context at visible_steps = 100 (cpc_attn128_tangent / _gp / _bwd):
    exact-f32 mode, with and without train-mode dropout (masks handed to the oracle), and a bf16 engine whose context runs in f32
    (contexts.Float32Context), against the oracle's double backward.  Bounds as test_scalogram_gpu.py's penalty tests: 1e-4 loss / 1e-3
    gradients in f32; in bf16 the loss within 1e-2 and gradient cosines > 0.95 (weights) / 0.85 (vectors)."""
    from cpc_audio_amd.audio_dataset import FileBatchSampler
    import random
    pre, model, meta, att, oblocks = _gp_model(golden_dir, dtype, p_drop)
    B, K, H, E, V = meta["B"], meta["K"], meta["H"], meta["E"], 100
    layers, heads, FF = att["num_layers"], att["num_heads"], att["feedforward_size"]
    model.train()
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(13)
    data = torch.randn(B, model.item_length, generator=gen) * 0.5
    all_t, reg, factor = (False, 0.01, 2.0) if p_drop == 0.0 else (True, 0.0, 10.0)
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
    eng = model.engine_for(scal)
    ctx = getattr(eng.ctx, "inner", eng.ctx)
    assert ctx.attn_abi == "cpc_attn128"
    ctx.fixed_seed = 777
    random.seed(91)
    tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    attention = (layers, heads)
    if p_drop:
        seed = ctx.drop_seed

        def factors(n, site):
            m = torch.empty(n, device=DEV)
            _hip.call("cpc_dropout_mask", _hip.ptr(m), n, p_drop, seed, site)
            return m.cpu()

        df = {}
        for l in range(layers):
            df[(l, 0)] = factors(B * heads * V * V, 4 * l + 0).view(B * heads, V, V)
            df[(l, 1)] = factors(B * V * E, 4 * l + 1).view(B, V, E).transpose(0, 1)
            df[(l, 2)] = factors(B * V * FF, 4 * l + 2).view(B, V, FF).transpose(0, 1)
            df[(l, 3)] = factors(B * V * E, 4 * l + 3).view(B, V, E).transpose(0, 1)
        attention = (layers, heads, df)
    ot = O.OracleTrainer(params, V, K, score="linear", all_timesteps=all_t, regularization=reg, lr=0.0, scalogram=oblocks,
                         attention=attention, gradient_penalty_factor=factor)
    loss, _, grads = ot.loss_and_grads(scal.float().cpu())
    got_loss = logger.loss_meter.values[0]
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    named = dict(model.named_parameters())
    if dtype == "fp32":
        assert abs(got_loss - float(loss)) < 1e-4 * abs(float(loss)), (got_loss, float(loss))
        for name, ref in grads.items():
            got = named[name].grad.double().cpu()
            if ref.abs().max().item() < 1e-6 * largest:
                assert got.abs().max().item() < 1e-5 * largest, name
                continue
            l2 = _rel(got, ref)
            assert l2 < 1e-3, (name, l2)
    else:
        assert abs(got_loss - float(loss)) < 1e-2 * abs(float(loss)), (got_loss, float(loss))
        for name, ref in grads.items():
            got = named[name].grad.double().cpu().flatten()
            ref = ref.double().flatten()
            if ref.abs().max().item() < 1e-6 * largest:
                continue
            cos = float(torch.dot(got, ref) / (got.norm() * ref.norm() + 1e-300))
            assert cos > (0.95 if named[name].dim() > 1 else 0.85), (name, cos)


def test_standalone_transformer_layers_at_100_steps():
    """TransformerEncoder / TransformerEncoderLayer at S = 100 (cpc_attn128_*): forward and backward against torch's own post-norm
    layers in float64 with the same state_dict (causal mask, eval mode)."""
    from cpc_audio_amd.attention_model import TransformerEncoder, TransformerEncoderLayer
    torch.manual_seed(11)
    S, B, C, heads, FF, N = 100, 3, 128, 2, 256, 2
    layer = TransformerEncoderLayer(C, heads, FF, dropout=0.1)
    enc = TransformerEncoder(layer, N, torch.nn.LayerNorm(C))
    for p_ in enc.parameters():
        p_.data.add_(torch.randn_like(p_) * 0.05)
    ref_enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(C, heads, FF, dropout=0.1), N, torch.nn.LayerNorm(C),
                                          enable_nested_tensor=False)
    ref_enc.load_state_dict(enc.state_dict())
    ref_enc = ref_enc.double().eval()
    src = torch.randn(S, B, C)
    mask = torch.triu(torch.full((S, S), float("-inf")), diagonal=1)
    up = torch.randn(S, B, C, generator=torch.Generator().manual_seed(12))
    enc = enc.to(DEV).eval()
    calls = []
    real = _hip.call

    def spy(name, *a, **kw):
        calls.append(name)
        return real(name, *a, **kw)

    ref_in = src.double().requires_grad_(True)
    want = ref_enc(ref_in, mask=mask.double())
    (want * up.double()).sum().backward()
    x_dev = src.to(DEV).requires_grad_(True)
    _hip.call = spy
    try:
        got = enc(x_dev, mask.to(DEV))
        (got * up.to(DEV)).sum().backward()
    finally:
        _hip.call = real
    assert "cpc_attn128_fwd" in calls and "cpc_attn128_bwd" in calls and "cpc_attn_fwd" not in calls
    assert (got.detach().cpu().double() - want.detach()).abs().max().item() < 2e-5
    assert (x_dev.grad.cpu().double() - ref_in.grad).abs().max().item() < 2e-4 * ref_in.grad.abs().max().item()
    ref_grads = dict(ref_enc.named_parameters())
    for name, p_ in enc.named_parameters():
        w = ref_grads[name].grad
        err = (p_.grad.cpu().double() - w).abs().max().item() / (w.abs().max().item() + 1e-12)
        assert err < 5e-4, (name, err)
    ref_in2 = src.double().requires_grad_(True)
    want2 = ref_enc.layers[1](ref_in2, src_mask=mask.double())
    (want2 * up.double()).sum().backward()
    x2 = src.to(DEV).requires_grad_(True)
    got2 = enc.layers[1](x2, mask.to(DEV))
    (got2 * up.to(DEV)).sum().backward()
    assert (got2.detach().cpu().double() - want2.detach()).abs().max().item() < 2e-5
    assert (x2.grad.cpu().double() - ref_in2.grad).abs().max().item() < 2e-4 * ref_in2.grad.abs().max().item()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_short_sequences_keep_the_short_kernels(golden_dir, dtype):
    """A step at visible_steps = 60 reaches only the existing cpc_attn_* entry points, never cpc_attn128_*."""
    g, meta = _fixture(golden_dir)
    model = _long_model(g, meta, dtype, V=60)
    x = torch.from_numpy(g["data"]).to(DEV)
    eng = model.engine(meta["B"], x.shape[1])
    calls = []
    real = _hip.call

    def spy(name, *a, **kw):
        calls.append(name)
        return real(name, *a, **kw)

    _hip.call = spy
    try:
        eng.loss_and_grads(x.contiguous(), softplus=True, regularization=1.0)
    finally:
        _hip.call = real
    assert "cpc_attn_fwd" in calls and "cpc_attn_bwd" in calls
    assert not [c for c in calls if c.startswith("cpc_attn128")]
