"""Grouped negatives on the HIP path: cpc_nce_group_mask against the host restatement (bit-exact), cpc_nce_loss_grouped against a
float64 torch restatement (masked logsumexp + autograd), the engine and trainer routes against the CPU oracle model with the masked
loss on its outputs, and the step without the attribute, which must not reach any of the new entry points."""
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
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, difference_score_function, file_group_ids,
                                                           grouped_negative_mask, linear_score_function, sampled_negative_mask,
                                                           softplus_score_function)
from cpc_audio_amd.engine import FusedAdam
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U64 = C.c_ulonglong
SENTINEL = -8192.0          # exact in f32 and bf16; byte buffers use 201
NEW_ENTRY_POINTS = {"cpc_nce_loss_grouped", "cpc_nce_group_mask", "cpc_nce_grouped_workspace_floats"}
SAMPLED_ENTRY_POINTS = {"cpc_nce_loss_sampled", "cpc_nce_sample_mask", "cpc_nce_sampled_workspace_floats"}
MODES = {"same": 0, "other": 1}
EXAMPLE = [0, 0, 0, 1, 1, 2]
# singleton (an empty set under "same"); interleaved ids and pad columns; file runs at the K = 12 instantiation; more than 256 rows
# per column and extreme ids; the largest batch (n_neg = 300 exceeds the 255 eligible rows under "same", is below 768 under "other")
CASES = [(6, 4, EXAMPLE), (33, 3, [b % 5 for b in range(33)]), (40, 12, [b // 8 for b in range(40)]),
         (257, 2, [(-5, 2 ** 31 - 1, 0)[(7 * b) % 3] for b in range(257)]), (1024, 1, [b // 256 for b in range(1024)])]
CASE_IDS = [f"B{B}-K{K}" for B, K, _ in CASES]
# in one column the N-th and (N + 1)-th smallest keys are equal, so the row index decides (tests/test_sampled_negatives_host.py)
TIES = [(257, 1, 23, 7, 18), (1024, 1, 44, 7, 1)]


def _counts(B):
    return (0, 1, 5) + ((300,) if B == 1024 else ())


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


def _sentinel(dtype):
    return 201 if dtype == torch.uint8 else (-8192 if dtype == torch.int32 else SENTINEL)


def _guarded(shape, fill, dtype, tail=64):
    """A device buffer of ``shape`` with ``tail`` sentinel elements behind it: (view, whole)."""
    n = int(np.prod(shape))
    whole = torch.full((n + tail,), _sentinel(dtype), device=DEV, dtype=dtype)
    whole[:n] = fill
    return whole[:n].view(*shape), whole


def _tails_intact(*wholes, tail=64):
    return all(bool((w[-tail:] == _sentinel(w.dtype)).all()) for w in wholes)


def _groups_dev(groups):
    g, whole = _guarded((len(groups),), torch.tensor(groups, dtype=torch.int32, device=DEV), torch.int32)
    return g, whole


def _device_mask(groups, K, mode, n_neg, seed, draw):
    B = len(groups)
    g, g_w = _groups_dev(groups)
    mask, whole = _guarded((K, B, B), 7, torch.uint8)
    _hip.call("cpc_nce_group_mask", _hip.ptr(mask), _hip.ptr(g), B, K, MODES[mode], n_neg, U64(seed), U64(draw))
    torch.cuda.synchronize()
    assert _tails_intact(whole, g_w) and g.tolist() == list(groups)
    return mask.cpu()


# ------------------------------------------------------------------------------------------ the selection on the device
@pytest.mark.parametrize("B,K,groups", CASES, ids=CASE_IDS)
def test_group_mask_is_bit_exact(B, K, groups):
    """cpc_nce_group_mask == grouped_negative_mask, element for element."""
    seed, draw = 1234 + B, 5 + K
    for mode in MODES:
        for n_neg in _counts(B):
            got = _device_mask(groups, K, mode, n_neg, seed, draw)
            want = grouped_negative_mask(groups, K, mode, n_neg or None, seed, draw)
            assert torch.equal(got, want.to(torch.uint8)), (mode, n_neg)


@pytest.mark.parametrize("B,K,N,seed,draw", [(6, 4, 2, 1234, 5), (37, 3, 9, 99, 1000003)] + TIES)
def test_one_group_is_the_sampler_on_the_device(B, K, N, seed, draw):
    """Identity 1 on the device, the tie draws included: one group, "same", n_neg = N gives cpc_nce_sample_mask's sets bit for bit."""
    got = _device_mask([-3] * B, K, "same", N, seed, draw)
    ref = torch.zeros(K, B, B, device=DEV, dtype=torch.uint8)
    _hip.call("cpc_nce_sample_mask", _hip.ptr(ref), B, K, N, U64(seed), U64(draw))
    torch.cuda.synchronize()
    assert torch.equal(got, ref.cpu())
    assert torch.equal(got, sampled_negative_mask(B, K, N, seed, draw).to(torch.uint8))


# ------------------------------------------------------------------------------------------ the loss kernels
def _run_loss(entry, S, K, reg, softplus, dt, *selection):
    """Launches a loss entry point on S [K][B][B] as test_nce_loss launches cpc_nce_loss: junk in the pad columns, NaN-prefilled
    outputs, sentinels behind every buffer.  ``selection``: the arguments between the regularisation and the dtype.  Returns
    (out, dS, dST) on the host."""
    B = S.shape[1]
    code = _hip.dtype_code(dt)
    ld = (B + 7) // 8 * 8
    Sp = torch.full((K, B, ld), 7.0)
    Sp[:, :, :B] = S
    S_d, S_w = _guarded((K, B, ld), Sp.to(DEV).reshape(-1), torch.float32)
    dSp, dS_w = _guarded((K, B, ld), float("nan"), dt)
    dSTp, dST_w = _guarded((K, B, ld), float("nan"), dt)
    out, out_w = _guarded((8,), float("nan"), torch.float32)
    nws = int(getattr(_hip.lib(), entry.replace("loss_", "") + "_workspace_floats")(B, K))
    ws, ws_w = _guarded((nws,), 0.0, torch.float32)
    _hip.call(entry, _hip.ptr(S_d), _hip.ptr(dSp), _hip.ptr(dSTp), _hip.ptr(out), _hip.ptr(ws), B, K, ld, softplus, C.c_float(reg),
              *selection, code)
    torch.cuda.synchronize()
    assert _tails_intact(S_w, dS_w, dST_w, out_w, ws_w)
    assert torch.equal(S_d.cpu(), Sp)
    assert (dSp[:, :, B:] == 0).all() and (dSTp[:, :, B:] == 0).all()
    return out.cpu(), dSp[:, :, :B].cpu(), dSTp[:, :, :B].cpu()


def _run_grouped(S, groups, K, mode, n_neg, reg, softplus, dt, seed, draw):
    g, g_w = _groups_dev(groups)
    got = _run_loss("cpc_nce_loss_grouped", S, K, reg, softplus, dt, _hip.ptr(g), MODES[mode], n_neg, U64(seed), U64(draw))
    assert _tails_intact(g_w) and g.tolist() == list(groups)
    return got


def _scores(B, K):
    g = torch.Generator().manual_seed(B * 3 + K)
    S = torch.randn(K, B, B, generator=g) * 3.0
    S[0, 0, 0] = 25.0                                  # exercises the softplus threshold branch
    return S


REG = {6: 1.0, 33: 0.5, 40: 0.01, 257: 0.0, 1024: 0.25}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,groups", CASES, ids=CASE_IDS)
def test_nce_loss_grouped_against_float64(dt, softplus, B, K, groups):
    seed, draw, reg = 1234 + B, 5 + K, REG[B]
    S = _scores(B, K)
    for mode in MODES:
        for n_neg in _counts(B):
            out, dS, dST = _run_grouped(S, groups, K, mode, n_neg, reg, softplus, dt, seed, draw)
            lin = S.double().requires_grad_(True)
            sp = F.softplus(lin) if softplus else lin
            loss, smax = masked_loss(sp, grouped_negative_mask(groups, K, mode, n_neg or None, seed, draw), reg)
            loss.backward()
            assert bool(torch.isfinite(loss))
            print(f"B={B} K={K} {mode} n_neg={n_neg} {dt} softplus={softplus}: loss {out[0].item():.7f} vs {loss.item():.7f}, "
                  f"dS rel {_rel(dS, lin.grad):.2e}")
            assert abs(out[0].item() - loss.item()) < 2e-5 * max(1.0, abs(loss.item())), (mode, n_neg)
            assert abs(out[1].item() - smax.item()) < 1e-5 * max(1.0, abs(smax.item())), (mode, n_neg)
            assert out[5].item() == 0.0
            t = 2e-5 if dt == torch.float32 else 1e-2
            assert _rel(dS, lin.grad) < t, (mode, n_neg)
            assert _rel(dST, lin.grad.transpose(1, 2)) < t, (mode, n_neg)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,N,seed,draw", [(6, 4, 2, 1234, 5), (37, 3, 9, 99, 1000003), (40, 12, 5, 41, 3), TIES[0]])
def test_one_group_is_the_sampled_loss_bit_for_bit(dt, softplus, B, K, N, seed, draw):
    """Identity 1 for the loss: one group, "same", n_neg = N gives cpc_nce_loss_sampled's out[0:7], dS and dST with the same (N, seed,
    draw), bit for bit (the NaN that stays in out[6] included) — both entry points run one template."""
    S, reg = _scores(B, K), {6: 1.0, 37: 0.5, 40: 0.01, 257: 0.0}[B]
    got = _run_grouped(S, [-3] * B, K, "same", N, reg, softplus, dt, seed, draw)
    ref = _run_loss("cpc_nce_loss_sampled", S, K, reg, softplus, dt, N, U64(seed), U64(draw))
    assert torch.equal(_bits(got[0][:7]), _bits(ref[0][:7]))
    assert torch.equal(_bits(got[1]), _bits(ref[1])) and torch.equal(_bits(got[2]), _bits(ref[2]))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("softplus", [0, 1])
def test_one_group_without_a_count_reproduces_the_dense_loss(dt, softplus):
    """Identity 2: one group, "same", n_neg = 0 is cpc_nce_loss on the same input."""
    B, K, reg = 40, 12, 0.01
    S = _scores(B, K)
    out, dS, dST = _run_grouped(S, [11] * B, K, "same", 0, reg, softplus, dt, 9, 9)
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


@pytest.mark.parametrize("B,K,groups", [CASES[0], CASES[1], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[1], CASE_IDS[3]])
def test_gradient_support_is_the_candidate_set(B, K, groups):
    """reg = 0, f32: dS is non-zero exactly on the candidate sets cpc_nce_group_mask reports, and dST is its transpose — the loss
    kernels and the mask kernel select the same rows.  A column whose eligible set is empty has lse = its own score, so its
    diagonal gradient exp(0) - 1 is exactly zero: that target contributes nothing, and its diagonal leaves the support."""
    S = torch.randn(K, B, B, generator=torch.Generator().manual_seed(B)) * 2.0
    seed, draw = 99, 1000003
    for mode in MODES:
        for n_neg in (0, 1, 5):
            out, dS, dST = _run_grouped(S, groups, K, mode, n_neg, 0.0, 1, torch.float32, seed, draw)
            mask = _device_mask(groups, K, mode, n_neg, seed, draw).bool()
            alone = mask.sum(dim=1) == 1                                            # [k][b']: the column holds its own row only
            want = mask & ~torch.diag_embed(alone)
            assert torch.equal(dS != 0, want), (mode, n_neg)
            assert torch.equal(dST, dS.transpose(1, 2))
            if B == 6 and mode == "same":
                assert alone[:, 5].all() and int(alone.sum()) == K                  # the singleton group


def test_bad_arguments_leave_the_buffers_alone():
    B, K, ld = 8, 2, 8
    S, S_w = _guarded((K, B, ld), 1.0, torch.float32)
    dS, dS_w = _guarded((K, B, ld), SENTINEL, torch.float32)
    dST, dST_w = _guarded((K, B, ld), SENTINEL, torch.float32)
    out, out_w = _guarded((8,), SENTINEL, torch.float32)
    ws, ws_w = _guarded((int(_hip.lib().cpc_nce_grouped_workspace_floats(B, K)),), SENTINEL, torch.float32)
    mask, mask_w = _guarded((K, B, B), 7, torch.uint8)
    g, g_w = _groups_dev([0, 0, 1, 1, 2, 2, 3, 3])
    lib, s, P = _hip.lib(), _hip.stream_ptr(), _hip.ptr

    def loss(S_=S, dS_=dS, dST_=dST, out_=out, ws_=ws, g_=g, B_=B, ld_=ld, mode=0, n=3, dtype=_hip.F32):
        return lib.cpc_nce_loss_grouped(P(S_), P(dS_), P(dST_), P(out_), P(ws_), B_, K, ld_, 1, C.c_float(1.0), P(g_), mode, n, U64(1),
                                        U64(2), dtype, s)

    def gmask(m=mask, g_=g, B_=B, mode=0, n=3):
        return lib.cpc_nce_group_mask(P(m), P(g_), B_, K, mode, n, U64(1), U64(2), s)

    for name in ("S_", "dS_", "dST_", "out_", "ws_", "g_"):
        assert loss(**{name: None}) == -22, name
    assert loss(n=-1) == -22 and loss(n=B) == -22
    assert loss(mode=2) == -22 and loss(mode=-1) == -22
    assert loss(B_=1025, ld_=1032, n=5) == -22 and loss(B_=1, ld_=1, n=0) == -22
    assert loss(ld_=7) == -22 and loss(ld_=16) == -22
    assert loss(dtype=7) == -22
    assert loss(ws_=ws.view(-1)[1:]) == -22                                         # 4 bytes past an 8-byte boundary
    assert gmask(m=None) == -22 and gmask(g_=None) == -22
    assert gmask(n=-1) == -22 and gmask(n=B) == -22
    assert gmask(mode=2) == -22 and gmask(B_=1025, n=5) == -22 and gmask(B_=1) == -22
    torch.cuda.synchronize()
    for w in (dS_w, dST_w, out_w, ws_w):
        assert bool((w == SENTINEL).all())
    assert bool((mask_w[:K * B * B] == 7).all()) and _tails_intact(S_w, mask_w, g_w)


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


def _oracle_masked(ot, batch, mask):
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


def _oracle_masked_step(ot, batch, mask):
    loss, smax, grads = _oracle_masked(ot, batch, mask)
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


@pytest.mark.parametrize("negatives", [None, (1, 41, 3)], ids=["all", "one"])
@pytest.mark.parametrize("mode", ["same", "other"])
@pytest.mark.parametrize("kind", ["softplus", "linear", "difference"])
def test_engine_gradients_against_oracle(golden_dir, kind, mode, negatives):
    """One fp32 engine step with negative_groups = (groups, mode), alone and together with negatives = (1, seed, draw): loss and
    every parameter gradient vs autograd of the oracle model with the masked loss on its outputs (1e-4 / 1e-3 relative L2)."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "fp32")
    B, K = meta["B"], meta["K"]
    assert B == len(EXAMPLE)
    x = data[:B]
    eng = model.engine(B, x.shape[1])
    groups = torch.tensor(EXAMPLE, dtype=torch.int32, device=DEV)
    kw = {} if negatives is None else {"negatives": negatives}
    with _Spy() as spy:
        out = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=0.5, score=kind, negative_groups=(groups, mode),
                                 **kw)
    torch.cuda.synchronize()
    assert "cpc_nce_loss_grouped" in spy.names and "cpc_nce_loss" not in spy.names and "cpc_nce_loss_sampled" not in spy.names
    n_neg, seed, draw = negatives or (None, 0, 0)
    ot = O.OracleTrainer(params, meta["V"], K, score=kind, regularization=0.5)
    loss, smax, grads = _oracle_masked(ot, x, grouped_negative_mask(EXAMPLE, K, mode, n_neg, seed, draw))
    dense, _, _ = ot.loss_and_grads(x)
    assert abs(float(loss) - float(dense)) > 1e-3 * abs(float(dense))           # the grouping is visible at this size
    assert abs(float(out[0]) - float(loss)) < 1e-4 * abs(float(loss))
    for name, ref in grads.items():
        assert _rel_l2(model._grad[name], ref) < 1e-3, name
    # the same call again is the same bits; the workspace was allocated once
    first, ws = float(out[0]), eng.nce_grouped_ws
    out = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=0.5, score=kind, negative_groups=(groups, mode), **kw)
    assert float(out[0]) == first and eng.nce_grouped_ws is ws


def test_engine_bf16_against_oracle(golden_dir):
    """bf16 storage: loss within 1e-3, worst per-parameter gradient relative L2 within 0.12 (the project's bf16 bounds)."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "bf16")
    B, K = meta["B"], meta["K"]
    x = data[:B]
    eng = model.engine(B, x.shape[1])
    groups = torch.tensor(EXAMPLE, dtype=torch.int32, device=DEV)
    out = eng.loss_and_grads(x.to(DEV), softplus=True, regularization=0.5, negative_groups=(groups, "other"), negatives=(2, 41, 3))
    torch.cuda.synchronize()
    ot = O.OracleTrainer(params, meta["V"], K, score="softplus", regularization=0.5)
    loss, smax, grads = _oracle_masked(ot, x, grouped_negative_mask(EXAMPLE, K, "other", 2, 41, 3))
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((_rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    print(f"bf16 grouped negatives: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]})")
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
    n = data.shape[0]
    counts = [n // 2, n - n // 2]
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, counts=counts, device=DEV), logger=logger, device=DEV,
                                      regularization=0.1, score_function=softplus_score_function, prediction_steps=K, ar_size=H,
                                      preprocessing=pre, file_batch_size=2)
    tr.verbose = False
    tr.negative_groups = "other_files"
    random.seed(91)
    idx = [list(b) for b in FileBatchSampler(counts, B, 2, True, verbose=False)][0]
    gid = file_group_ids(counts)[idx]
    assert len(set(gid.tolist())) > 1
    random.seed(91)
    with _Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    assert spy.names.count("cpc_nce_loss_grouped") == 1 and "cpc_nce_loss" not in spy.names
    with torch.no_grad():
        scal = pre(data[idx].to(DEV).unsqueeze(1)).cpu()
    oblocks = [dict(b) for b in blocks]
    oblocks[0]["in_channels"] = 2
    ot = O.OracleTrainer(params, V, K, score="softplus", regularization=0.1, lr=0.0, scalogram=oblocks)
    loss, smax, grads = _oracle_masked(ot, scal, grouped_negative_mask(gid, K, "other"))
    assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss)), (logger.loss_meter.values, float(loss))
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for name, ref in grads.items():
        got = dict(model.named_parameters())[name].grad.double().cpu()
        if ref.abs().max().item() < 1e-6 * largest:
            assert got.abs().max().item() < 1e-5 * largest, name
            continue
        assert _rel_l2(got, ref) < 1e-3, name


COUNTS = [8, 8, 8]


def _trainer(model, data, meta, logger, score_function=softplus_score_function, optimizer=torch.optim.Adam, resident=True):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, counts=COUNTS, device=DEV if resident else None),
                                      logger=logger, device=DEV, regularization=0.5, score_function=score_function, optimizer=optimizer,
                                      prediction_steps=meta["K"], ar_size=meta["H"], file_batch_size=2)
    tr.verbose = False
    return tr


def _batches(meta, seed=5):
    random.seed(seed)
    return [list(b) for b in FileBatchSampler(COUNTS, meta["B"], 2, True, verbose=False)]


def test_the_sampler_replay_is_the_one_the_issue_pins(golden_dir):
    g, meta, data, params = _small(golden_dir)
    files = file_group_ids(COUNTS)
    assert [files[b].tolist() for b in _batches(meta)[:3]] == [[1, 1, 1, 1, 0, 0], [2, 2, 0, 0, 2, 2], [1, 1, 2, 2, 0, 0]]


@pytest.mark.parametrize("setting,N", [("same_file", 2), ("other_files", None)])
def test_trainer_three_steps_and_routes(golden_dir, setting, N):
    """Three fused steps with negative_groups set: every logged loss equals a torch replay of the oracle model with the groups of a
    sampler replay and draw = step, the parameters stay within the Adam bound, and the host DataLoader route (one batch uploaded
    ahead) logs the resident route's losses."""
    g, meta, data, params = _small(golden_dir)
    B, K, seed, steps, lr = meta["B"], meta["K"], 123, 3, 1e-3
    mode = {"same_file": "same", "other_files": "other"}[setting]
    batches, files = _batches(meta), file_group_ids(COUNTS)
    logged = []
    for resident in (True, False):
        model = _small_model(g, meta, "fp32")
        logger = _Logger()
        tr = _trainer(model, data, meta, logger, resident=resident)
        tr.negative_groups, tr.num_negatives, tr.negative_seed = setting, N, seed
        random.seed(5)
        with _Spy() as spy:
            tr.train(batch_size=B, epochs=1, lr=lr, num_workers=0, max_steps=steps)
        assert spy.names.count("cpc_nce_loss_grouped") == steps
        assert "cpc_nce_loss" not in spy.names and "cpc_nce_loss_sampled" not in spy.names
        assert tr.training_step == steps and tr.last_empty_negative_sets == 0
        logged.append(logger.loss_meter.values)
        if not resident:
            continue
        ot = O.OracleTrainer(params, meta["V"], K, score="softplus", regularization=0.5, lr=lr)
        for i in range(steps):
            mask = grouped_negative_mask(files[batches[i]], K, mode, N, seed, i)
            loss, smax = _oracle_masked_step(ot, data[batches[i]], mask)
            assert abs(logger.loss_meter.values[i] - loss) < 2e-4 * abs(loss), (i, logger.loss_meter.values[i], loss)
            assert abs(logger.score_meter.values[i] - smax) < 2e-4 * abs(smax) + 1e-6, i
        for k, v in model.state_dict().items():
            err = (v.cpu() - ot.params[k].detach()).abs()
            assert err.max().item() <= 2 * lr * steps * 1.01 + 1e-6, k
    assert len(logged[0]) == steps and logged[0] == logged[1]


def test_trainer_ids_resume_and_empty_sets(golden_dir):
    """negative_group_ids overrides the files; continue_training_at_step = s draws step s's sets; last_empty_negative_sets counts the
    batch items without an eligible row (lr 0 throughout: the parameters are the golden ones)."""
    g, meta, data, params = _small(golden_dir)
    B, K, seed = meta["B"], meta["K"], 123
    batches = _batches(meta)
    ot = O.OracleTrainer(params, meta["V"], K, score="softplus", regularization=0.5, lr=0.0)

    def first_loss(ids, setting, N, at=0):
        model = _small_model(g, meta, "fp32")
        logger = _Logger()
        tr = _trainer(model, data, meta, logger)
        tr.negative_groups, tr.negative_group_ids, tr.num_negatives, tr.negative_seed = setting, ids, N, seed
        random.seed(5)
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=at + 1, continue_training_at_step=at)
        return logger.loss_meter.values[0], tr.last_empty_negative_sets

    # the user's own ids: index parity instead of the file
    ids = np.arange(24) % 2
    got, empty = first_loss(ids.tolist(), "same_file", None)
    want, _, _ = _oracle_masked(ot, data[batches[0]], grouped_negative_mask(ids[batches[0]], K, "same"))
    by_file, _, _ = _oracle_masked(ot, data[batches[0]], grouped_negative_mask(file_group_ids(COUNTS)[batches[0]], K, "same"))
    assert abs(got - float(want)) < 2e-4 * abs(float(want))
    assert abs(float(want) - float(by_file)) > 1e-3 * abs(float(want))
    part = ids[batches[0]]
    assert empty == sum(1 for v in part if (part == v).sum() == 1)
    # a run continued at step s: its first step uses draw = s
    s = 7
    files = file_group_ids(COUNTS)[batches[0]]
    got, empty = first_loss(None, "other_files", 1, at=s)
    want, _, _ = _oracle_masked(ot, data[batches[0]], grouped_negative_mask(files, K, "other", 1, seed, s))
    other, _, _ = _oracle_masked(ot, data[batches[0]], grouped_negative_mask(files, K, "other", 1, seed, 0))
    assert abs(got - float(want)) < 2e-4 * abs(float(want)) and empty == 0
    assert abs(float(want) - float(other)) > 1e-3 * abs(float(want))
    # one id for everybody, "other_files": no target has a negative, every one contributes 0
    got, empty = first_loss([5] * 24, "other_files", None)
    want, _, _ = _oracle_masked(ot, data[batches[0]], torch.eye(B, dtype=torch.bool).expand(K, B, B))
    assert empty == B and abs(got - float(want)) < 2e-4 * abs(float(want)) + 1e-6


def test_generic_route_logs_the_fused_route_loss(golden_dir):
    """Another optimizer sends the step through the autograd bridge and _InfoNCE's grouped selection: same first-step loss as the fused route."""
    g, meta, data, params = _small(golden_dir)
    B, seed = meta["B"], 123
    for score_function, N in ((softplus_score_function, 2), (linear_score_function, None), (difference_score_function, 1)):
        losses = []
        for optimizer in (torch.optim.Adam, torch.optim.SGD):
            model = _small_model(g, meta, "fp32")
            logger = _Logger()
            tr = _trainer(model, data, meta, logger, score_function=score_function, optimizer=optimizer)
            tr.negative_groups, tr.num_negatives, tr.negative_seed = "same_file", N, seed
            random.seed(5)
            with _Spy() as spy:
                tr.train(batch_size=B, epochs=1, lr=1e-3, num_workers=0, max_steps=1)
            assert "cpc_nce_loss_grouped" in spy.names and "cpc_nce_loss" not in spy.names and "cpc_nce_loss_sampled" not in spy.names
            assert hasattr(tr, "last_optimizer") == (optimizer is torch.optim.Adam)
            losses.append(logger.loss_meter.values[0])
        assert abs(losses[0] - losses[1]) < 2e-4 * abs(losses[0]), (score_function, losses)


def test_step_without_groups_is_the_parent_step(golden_dir):
    """negative_groups = None: no new entry point is reached, and losses and parameters after two steps are bit-identical to the
    step as it was before the attribute existed — the engine called without the keyword, FusedAdam behind it."""
    g, meta, data, params = _small(golden_dir)
    B, steps, lr = meta["B"], 2, 1e-3
    batches = _batches(meta)
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    assert tr.negative_groups is None and tr.negative_group_ids is None
    random.seed(5)
    with _Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=lr, num_workers=0, max_steps=steps)
    assert not (NEW_ENTRY_POINTS | SAMPLED_ENTRY_POINTS) & set(spy.names)
    assert spy.names.count("cpc_nce_loss") == steps and tr.last_empty_negative_sets is None
    # the same two steps by hand, with the calls train() made before negative_groups existed
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
