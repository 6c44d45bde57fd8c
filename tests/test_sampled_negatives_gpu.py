"""Sampled negatives on the HIP path: cpc_nce_sample_mask against the host restatement (bit-exact), cpc_nce_loss_sampled against a
float64 torch restatement (masked logsumexp + autograd), the engine and trainer routes against the CPU oracle model with the
masked loss on its outputs, and the unsampled step, which must not reach any of the new entry points."""
import copy
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, difference_score_function,
                                                           linear_score_function, sampled_negative_mask, softplus_score_function)
from cpc_audio_amd.engine import FusedAdam
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U64 = C.c_ulonglong
SENTINEL = -8192.0          # exact in f32 and bf16; byte buffers use 201
NEW_ENTRY_POINTS = {"cpc_nce_loss_sampled", "cpc_nce_sample_mask", "cpc_nce_sampled_workspace_floats"}


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _rel_l2(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


def masked_loss(sp, mask, reg):
    """The definition: sp [K][b][b'] the transformed scores, mask [K][b][b'] the candidate sets (diagonal included)."""
    valid = torch.diagonal(sp, dim1=1, dim2=2)
    lse = torch.logsumexp(sp.masked_fill(~mask, float("-inf")), dim=1)
    return -valid.mean() + lse.mean() + reg * (sp.mean(dim=0) ** 2).mean(), sp.max()


def _guarded(shape, fill, dtype, tail=64):
    """A device buffer of ``shape`` with ``tail`` sentinel elements behind it: (view, whole)."""
    n = int(np.prod(shape))
    whole = torch.full((n + tail,), _sentinel(dtype), device=DEV, dtype=dtype)
    whole[:n] = fill
    return whole[:n].view(*shape), whole


def _sentinel(dtype):
    return 201 if dtype == torch.uint8 else SENTINEL


def _tails_intact(*wholes, tail=64):
    return all(bool((w[-tail:] == _sentinel(w.dtype)).all()) for w in wholes)


# ------------------------------------------------------------------------------------------ the sampler on the device
# (257, 1, 23, 7, 18) and (1024, 1, 44, 7, 1): in one column the N-th and (N + 1)-th smallest keys are equal, so the row index decides
# (tests/test_sampled_negatives_host.py checks that they are); 1024 is the largest supported batch
TIES = [(257, 1, 23, 7, 18), (1024, 1, 44, 7, 1)]


@pytest.mark.parametrize("B,K,N,seed,draw", [(6, 4, 2, 1234, 5), (37, 3, 9, 99, 1000003), (256, 12, 128, 1234, 5),
                                             (257, 2, 128, 3, 2 ** 40 + 1), (1024, 2, 1023, 5, 6)] + TIES)
def test_sample_mask_is_bit_exact(B, K, N, seed, draw):
    """cpc_nce_sample_mask == sampled_negative_mask, element for element (B = 257: more than 256 rows per column, the wider
    per-lane row count of the selection)."""
    mask, whole = _guarded((K, B, B), 7, torch.uint8)
    _hip.call("cpc_nce_sample_mask", _hip.ptr(mask), B, K, N, U64(seed), U64(draw))
    torch.cuda.synchronize()
    want = sampled_negative_mask(B, K, N, seed, draw)
    assert torch.equal(mask.cpu(), want.to(torch.uint8))
    assert _tails_intact(whole)


# ------------------------------------------------------------------------------------------ the loss kernels
def _run_sampled(S, B, K, N, reg, softplus, dt, seed, draw):
    """Launches cpc_nce_loss_sampled on S [K][B][B] as test_nce_loss launches cpc_nce_loss: junk in the pad columns, NaN-prefilled
    outputs, sentinels behind every buffer.  Returns (out, dS, dST) on the host."""
    code = _hip.dtype_code(dt)
    ld = (B + 7) // 8 * 8
    Sp = torch.full((K, B, ld), 7.0)
    Sp[:, :, :B] = S
    S_d, S_w = _guarded((K, B, ld), Sp.to(DEV).reshape(-1), torch.float32)
    dSp, dS_w = _guarded((K, B, ld), float("nan"), dt)
    dSTp, dST_w = _guarded((K, B, ld), float("nan"), dt)
    out, out_w = _guarded((8,), float("nan"), torch.float32)
    nws = int(_hip.lib().cpc_nce_sampled_workspace_floats(B, K))
    ws, ws_w = _guarded((nws,), 0.0, torch.float32)
    _hip.call("cpc_nce_loss_sampled", _hip.ptr(S_d), _hip.ptr(dSp), _hip.ptr(dSTp), _hip.ptr(out), _hip.ptr(ws), B, K, ld, softplus,
              C.c_float(reg), N, U64(seed), U64(draw), code)
    torch.cuda.synchronize()
    assert _tails_intact(S_w, dS_w, dST_w, out_w, ws_w)
    assert torch.equal(S_d.cpu(), Sp)
    assert (dSp[:, :, B:] == 0).all() and (dSTp[:, :, B:] == 0).all()
    return out.cpu(), dSp[:, :, :B].cpu(), dSTp[:, :, :B].cpu()


def _scores(B, K):
    g = torch.Generator().manual_seed(B * 3 + K)
    S = torch.randn(K, B, B, generator=g) * 3.0
    S[0, 0, 0] = 25.0                                  # exercises the softplus threshold branch
    return S


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,N,reg", [(6, 4, 2, 1.0), (33, 3, 7, 0.5), (40, 12, 1, 0.01), (40, 12, 39, 0.01), (257, 2, 128, 0.0),
                                       (1024, 1, 700, 0.25)])
def test_nce_loss_sampled_against_float64(dt, softplus, B, K, N, reg):
    seed, draw = 1234 + B, 5 + K
    S = _scores(B, K)
    out, dS, dST = _run_sampled(S, B, K, N, reg, softplus, dt, seed, draw)
    lin = S.double().requires_grad_(True)
    sp = F.softplus(lin) if softplus else lin
    loss, smax = masked_loss(sp, sampled_negative_mask(B, K, N, seed, draw), reg)
    loss.backward()
    print(f"B={B} K={K} N={N} {dt} softplus={softplus}: loss {out[0].item():.7f} vs {loss.item():.7f}, dS rel {_rel(dS, lin.grad):.2e}")
    assert abs(out[0].item() - loss.item()) < 2e-5 * max(1.0, abs(loss.item()))
    assert abs(out[1].item() - smax.item()) < 1e-5 * max(1.0, abs(smax.item()))
    assert out[5].item() == 0.0
    t = 2e-5 if dt == torch.float32 else 1e-2
    assert _rel(dS, lin.grad) < t
    assert _rel(dST, lin.grad.transpose(1, 2)) < t


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("softplus", [0, 1])
def test_all_negatives_reproduce_the_dense_loss(dt, softplus):
    """N = B - 1 is cpc_nce_loss on the same input."""
    B, K, reg = 40, 12, 0.01
    S = _scores(B, K)
    out, dS, dST = _run_sampled(S, B, K, B - 1, reg, softplus, dt, 9, 9)
    ld = (B + 7) // 8 * 8
    Sp = torch.zeros(K, B, ld)
    Sp[:, :, :B] = S
    dS0 = torch.zeros(K, B, ld, device=DEV, dtype=dt)
    dST0 = torch.zeros(K, B, ld, device=DEV, dtype=dt)
    out0 = torch.zeros(8, device=DEV)
    ws = torch.empty(_hip.lib().cpc_nce_workspace_floats(B, K), device=DEV)
    _hip.call("cpc_nce_loss", _hip.ptr(Sp.to(DEV)), _hip.ptr(dS0), _hip.ptr(dST0), _hip.ptr(out0), _hip.ptr(ws), B, K, ld, softplus,
              C.c_float(reg), _hip.dtype_code(dt))
    torch.cuda.synchronize()
    assert abs(out[0].item() - out0[0].item()) < 2e-5 * max(1.0, abs(out0[0].item()))
    assert abs(out[1].item() - out0[1].item()) < 1e-5 * max(1.0, abs(out0[1].item()))
    t = 2e-5 if dt == torch.float32 else 1e-2
    assert _rel(dS, dS0[:, :, :B]) < t and _rel(dST, dST0[:, :, :B]) < t


@pytest.mark.parametrize("B,K,N,seed,draw", [(37, 3, 9, 99, 1000003), (257, 2, 128, 99, 1000003)] + TIES)
def test_gradient_support_is_the_candidate_set(B, K, N, seed, draw):
    """reg = 0, f32: dS is non-zero exactly on the candidate sets cpc_nce_sample_mask reports, and dST is its transpose — the loss
    kernels and the mask kernel select the same rows."""
    S = torch.randn(K, B, B, generator=torch.Generator().manual_seed(B)) * 2.0
    out, dS, dST = _run_sampled(S, B, K, N, 0.0, 1, torch.float32, seed, draw)
    mask = torch.zeros(K, B, B, device=DEV, dtype=torch.uint8)
    _hip.call("cpc_nce_sample_mask", _hip.ptr(mask), B, K, N, U64(seed), U64(draw))
    torch.cuda.synchronize()
    assert torch.equal(dS != 0, mask.cpu().bool())
    assert torch.equal(dST, dS.transpose(1, 2))


def test_bad_arguments_leave_the_buffers_alone():
    B, K, ld = 8, 2, 8
    S, S_w = _guarded((K, B, ld), 1.0, torch.float32)
    dS, dS_w = _guarded((K, B, ld), SENTINEL, torch.float32)
    dST, dST_w = _guarded((K, B, ld), SENTINEL, torch.float32)
    out, out_w = _guarded((8,), SENTINEL, torch.float32)
    ws, ws_w = _guarded((int(_hip.lib().cpc_nce_sampled_workspace_floats(B, K)),), SENTINEL, torch.float32)
    mask, mask_w = _guarded((K, B, B), 7, torch.uint8)
    lib, s, P = _hip.lib(), _hip.stream_ptr(), _hip.ptr

    def loss(S_=S, dS_=dS, dST_=dST, out_=out, ws_=ws, B_=B, ld_=ld, n=3):
        return lib.cpc_nce_loss_sampled(P(S_), P(dS_), P(dST_), P(out_), P(ws_), B_, K, ld_, 1, C.c_float(1.0), n, U64(1), U64(2), _hip.F32, s)

    for name in ("S_", "dS_", "dST_", "out_", "ws_"):
        assert loss(**{name: None}) == -22, name
    assert loss(n=0) == -22 and loss(n=B) == -22
    assert loss(B_=1025, ld_=1032, n=5) == -22
    assert lib.cpc_nce_sample_mask(None, B, K, 3, U64(1), U64(2), s) == -22
    assert lib.cpc_nce_sample_mask(P(mask), B, K, 0, U64(1), U64(2), s) == -22
    assert lib.cpc_nce_sample_mask(P(mask), B, K, B, U64(1), U64(2), s) == -22
    assert lib.cpc_nce_sample_mask(P(mask), 1025, K, 5, U64(1), U64(2), s) == -22
    torch.cuda.synchronize()
    for w in (dS_w, dST_w, out_w, ws_w):
        assert bool((w == SENTINEL).all())
    assert bool((mask_w[:K * B * B] == 7).all()) and _tails_intact(S_w, mask_w)


# ------------------------------------------------------------------------------------------ engine / trainer against the oracle
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def _small(golden_dir):
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    return g, meta, torch.from_numpy(g["data"]), params


def _small_model(g, meta, dtype):
    C_, H, K, V = meta["C"], meta["H"], meta["K"], meta["V"]
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    ar = AudioGRUModel(input_size=C_, hidden_size=H)
    model = AudioPredictiveCodingModel(enc, ar, enc_size=C_, ar_size=H, visible_steps=V, prediction_steps=K, compute_dtype=dtype)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return model.to(DEV)


def _oracle_sampled(ot, batch, mask):
    """OracleTrainer.loss_and_grads with the masked loss in place of info_nce_loss."""
    for p in ot.params.values():
        p.grad = None
    x = batch if ot.scalogram is not None else batch.unsqueeze(1)
    pred, targ, _, _ = O.cpc_forward(x, {**ot.params, **ot.buffers}, ot.V, ot.K, ot.strides, ot.conv_ar, ot.attention, ot.scalogram,
                                     ar_resnet=ot.ar_resnet)
    sp = torch.diagonal(ot.score(pred, targ), dim1=1, dim2=3).permute(2, 0, 1)          # [k][b][b']
    loss, smax = masked_loss(sp, mask, ot.regularization)
    loss.backward()
    return loss.detach(), smax.detach(), {k: p.grad for k, p in ot.params.items()}


def _oracle_sampled_step(ot, batch, mask):
    loss, smax, grads = _oracle_sampled(ot, batch, mask)
    ot.t += 1
    with torch.no_grad():
        for k, p in ot.params.items():
            O.adam_update(p, grads[k], ot.m[k], ot.v[k], ot.t, ot.lr)
    return float(loss), float(smax)


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


class _Spy:
    """Records the entry-point names that go through _hip.call while active."""

    def __enter__(self):
        self.names, self.real = [], _hip.call

        def spy(name, *a, **kw):
            self.names.append(name)
            return self.real(name, *a, **kw)

        _hip.call = spy
        return self

    def __exit__(self, *exc):
        _hip.call = self.real


@pytest.mark.parametrize("kind", ["softplus", "linear", "difference"])
def test_engine_gradients_against_oracle(golden_dir, kind):
    """One fp32 engine step with negatives = (N, seed, draw): loss and every parameter gradient vs autograd of the oracle model with
    the masked loss on its outputs (1e-4 / 1e-3 relative L2, the bounds of the difference-score engine test)."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "fp32")
    B, K, N, seed, draw = meta["B"], meta["K"], 2, 41, 3
    x = data[:B]
    eng = model.engine(B, x.shape[1])
    with _Spy() as spy:
        out = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=0.5, score=kind, negatives=(N, seed, draw))
    torch.cuda.synchronize()
    assert "cpc_nce_loss_sampled" in spy.names and "cpc_nce_loss" not in spy.names
    ot = O.OracleTrainer(params, meta["V"], K, score=kind, regularization=0.5)
    loss, smax, grads = _oracle_sampled(ot, x, sampled_negative_mask(B, K, N, seed, draw))
    dense, _, _ = ot.loss_and_grads(x)
    assert abs(float(loss) - float(dense)) > 1e-3 * abs(float(dense))           # the sampling is visible at this size
    assert abs(float(out[0]) - float(loss)) < 1e-4 * abs(float(loss))
    for name, ref in grads.items():
        assert _rel_l2(model._grad[name], ref) < 1e-3, name
    # another draw is another loss; the same draw again is the same bits
    first = float(out[0])
    out = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=0.5, score=kind, negatives=(N, seed, draw + 1))
    assert float(out[0]) != first
    out = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=0.5, score=kind, negatives=(N, seed, draw))
    assert float(out[0]) == first


def test_engine_bf16_against_oracle(golden_dir):
    """bf16 storage: loss within 1e-3, worst per-parameter gradient relative L2 within 0.12 (the project's bf16 bounds)."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "bf16")
    B, K, N, seed, draw = meta["B"], meta["K"], 3, 41, 3
    x = data[:B]
    eng = model.engine(B, x.shape[1])
    out = eng.loss_and_grads(x.to(DEV), softplus=True, regularization=0.5, negatives=(N, seed, draw))
    torch.cuda.synchronize()
    ot = O.OracleTrainer(params, meta["V"], K, score="softplus", regularization=0.5)
    loss, smax, grads = _oracle_sampled(ot, x, sampled_negative_mask(B, K, N, seed, draw))
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((_rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    print(f"bf16 sampled negatives: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]})")
    assert rel < 1e-3
    assert worst[0] < 0.12, worst


def test_scalogram_engine_against_oracle(golden_dir):
    """The scalogram engine takes the keyword too: one fp32 step through the trainer (lr 0) vs the oracle with the masked loss."""
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    g = _load(golden_dir, "scalogram_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    B, K, H, V = meta["B"], meta["K"], meta["H"], meta["V"]
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["E"], hidden_size=H), enc_size=meta["E"], ar_size=H,
                                       visible_steps=V, prediction_steps=K, compute_dtype="fp32")
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    pre, model = pre.to(DEV), model.to(DEV)
    model.train()
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    data = torch.from_numpy(g["data"])
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.1, score_function=softplus_score_function, prediction_steps=K, ar_size=H,
                                      preprocessing=pre)
    tr.verbose = False
    tr.num_negatives, tr.negative_seed = 2, 17
    random.seed(91)
    idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
    random.seed(91)
    with _Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    assert spy.names.count("cpc_nce_loss_sampled") == 1 and "cpc_nce_loss" not in spy.names
    with torch.no_grad():
        scal = pre(data[idx].to(DEV).unsqueeze(1)).cpu()
    oblocks = [dict(b) for b in blocks]
    oblocks[0]["in_channels"] = 2
    ot = O.OracleTrainer(params, V, K, score="softplus", regularization=0.1, lr=0.0, scalogram=oblocks)
    loss, smax, grads = _oracle_sampled(ot, scal, sampled_negative_mask(B, K, 2, 17, 0))
    assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss)), (logger.loss_meter.values, float(loss))
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for name, ref in grads.items():
        got = dict(model.named_parameters())[name].grad.double().cpu()
        if ref.abs().max().item() < 1e-6 * largest:
            assert got.abs().max().item() < 1e-5 * largest, name
            continue
        assert _rel_l2(got, ref) < 1e-3, name


def _trainer(model, data, meta, logger, score_function=softplus_score_function, optimizer=torch.optim.Adam):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.5, score_function=score_function, optimizer=optimizer,
                                      prediction_steps=meta["K"], ar_size=meta["H"])
    tr.verbose = False
    return tr


def _batches(data, meta, seed=5):
    random.seed(seed)
    return [list(b) for b in FileBatchSampler([data.shape[0]], meta["B"], 1, True, verbose=False)]


def test_trainer_three_steps_and_resume(golden_dir):
    """Three fused steps with num_negatives set: every logged loss equals a torch replay of the oracle model with draw = step, the
    parameters stay within the Adam bound; continue_training_at_step = s draws step s's sets."""
    g, meta, data, params = _small(golden_dir)
    B, K, N, seed, steps, lr = meta["B"], meta["K"], 2, 123, 3, 1e-3
    batches = _batches(data, meta)
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    tr.num_negatives, tr.negative_seed = N, seed
    random.seed(5)
    with _Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=lr, num_workers=0, max_steps=steps)
    assert spy.names.count("cpc_nce_loss_sampled") == steps and "cpc_nce_loss" not in spy.names
    assert tr.training_step == steps
    ot = O.OracleTrainer(params, meta["V"], K, score="softplus", regularization=0.5, lr=lr)
    for i in range(steps):
        loss, smax = _oracle_sampled_step(ot, data[batches[i]], sampled_negative_mask(B, K, N, seed, i))
        assert abs(logger.loss_meter.values[i] - loss) < 2e-4 * abs(loss), (i, logger.loss_meter.values[i], loss)
        assert abs(logger.score_meter.values[i] - smax) < 2e-4 * abs(smax) + 1e-6, i
    for k, v in model.state_dict().items():
        err = (v.cpu() - ot.params[k].detach()).abs()
        assert err.max().item() <= 2 * lr * steps * 1.01 + 1e-6, k
    # a run continued at step s: its first step uses draw = s (lr 0: the parameters are the golden ones)
    s = 7
    model2 = _small_model(g, meta, "fp32")
    logger2 = _Logger()
    tr2 = _trainer(model2, data, meta, logger2)
    tr2.num_negatives, tr2.negative_seed = N, seed
    random.seed(5)
    tr2.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=s + 1, continue_training_at_step=s)
    ot2 = O.OracleTrainer(params, meta["V"], K, score="softplus", regularization=0.5, lr=0.0)
    want, _, _ = _oracle_sampled(ot2, data[batches[0]], sampled_negative_mask(B, K, N, seed, s))
    other, _, _ = _oracle_sampled(ot2, data[batches[0]], sampled_negative_mask(B, K, N, seed, 0))
    assert abs(logger2.loss_meter.values[0] - float(want)) < 2e-4 * abs(float(want))
    assert abs(float(want) - float(other)) > 1e-3 * abs(float(want))


@pytest.mark.parametrize("score_function", [softplus_score_function, linear_score_function, difference_score_function])
def test_generic_route_logs_the_fused_route_loss(golden_dir, score_function):
    """Another optimizer sends the step through the autograd bridge and _InfoNCE's sampled selection: same first-step loss as the fused route."""
    g, meta, data, params = _small(golden_dir)
    B, N, seed = meta["B"], 2, 123
    losses = []
    for optimizer in (torch.optim.Adam, torch.optim.SGD):
        model = _small_model(g, meta, "fp32")
        logger = _Logger()
        tr = _trainer(model, data, meta, logger, score_function=score_function, optimizer=optimizer)
        tr.num_negatives, tr.negative_seed = N, seed
        random.seed(5)
        with _Spy() as spy:
            tr.train(batch_size=B, epochs=1, lr=1e-3, num_workers=0, max_steps=1)
        assert "cpc_nce_loss_sampled" in spy.names and "cpc_nce_loss" not in spy.names
        assert hasattr(tr, "last_optimizer") == (optimizer is torch.optim.Adam)
        losses.append(logger.loss_meter.values[0])
    assert abs(losses[0] - losses[1]) < 2e-4 * abs(losses[0]), losses


def test_unsampled_step_is_the_parent_step(golden_dir):
    """num_negatives = None: no new entry point is reached, and losses and parameters after two steps are bit-identical to the
    step as it was before the attribute existed — the engine called without the keyword, FusedAdam behind it."""
    g, meta, data, params = _small(golden_dir)
    B, steps, lr = meta["B"], 2, 1e-3
    batches = _batches(data, meta)
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    assert tr.num_negatives is None
    random.seed(5)
    with _Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=lr, num_workers=0, max_steps=steps)
    assert not NEW_ENTRY_POINTS & set(spy.names)
    assert spy.names.count("cpc_nce_loss") == steps
    # the same two steps by hand, with the calls train() made before num_negatives existed
    model0 = _small_model(g, meta, "fp32")
    model0.train()
    model0._flatten_parameters(DEV)
    opt = FusedAdam(model0, lr=lr)
    model0.link_grads()
    dev_data = data.to(DEV)
    losses = []
    for i in range(steps):
        x = dev_data[torch.as_tensor(batches[i], device=DEV)].contiguous()
        eng = model0.engine(x.shape[0], x.shape[1], DEV)
        if i == 0:
            eng.nan_flag().zero_()
        opt.after_update = eng.prepare_ahead
        opt.skip_flag = eng.nan_flag()
        out = eng.loss_and_grads(x, softplus=True, regularization=0.5, all_timesteps=False, grad_ready_hook=opt.hook,
                                 global_negatives=None, after_loss=None, score="softplus")
        opt.step(grad_scale=1.0)
        losses.append(float(out[0]))
    torch.cuda.synchronize()
    assert logger.loss_meter.values == losses
    for (k, v), (k0, v0) in zip(model.state_dict().items(), model0.state_dict().items()):
        assert k == k0 and torch.equal(v, v0), k
