"""Stacked GRU context (AudioGRUModel(num_layers > 1)) on the GPU: cpc_gru_bwd_steps, the backward sweep of a layer that receives a
gradient at every hidden state, in its three kernel families (csrc/gru.hip: weight-resident bf16, 4-wave and 8-wave streaming) against
the float64 reference of tests/gru_stacked_reference.py, and the routes that use it: GRUContext with 2 and 3 layers in both storage
types against the float64 model composed from the oracle's pieces, a carried per-layer state, stand-alone AudioGRUModel calls, the
trainer's options around a two-layer context, the scalogram engine, and the single-layer step, which must be launch for launch what it
was.  test_gru_stacked_host.py holds the host side: the references against autograd, the cap on the bf16 emulation's error in every
case used here, and the sensitivity of the per-step verdict to an off-by-one in t.

Kernel bounds: per time step, for the four blocks of dG = [dr | du | dn | dn r] (and the hidden states of the forward pass that fed the
sweep): f32 GRU_TOL_F32; bf16 GRU_MODEL_FACTOR = 4 x the error of the bf16 emulation at that step (below 2e-2 everywhere, largest
1.15e-2, so no bound exceeds 8e-2).  Model bounds: those of test_gru_wide_gpu.py (fp32 loss 1e-4, gradients 1e-3 relative l2; bf16
loss 1e-2, context and predictor 0.12, encoder 0.2).  No bound here was obtained by running a kernel.
"""
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
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,  # noqa: E402
                                                           softplus_score_function)
from cpc_audio_amd.engine import NegativeBank  # noqa: E402
from oracle import cpc_oracle as O  # noqa: E402
import context_reference as R  # noqa: E402
import gru_stacked_reference as S  # noqa: E402
import negative_bank_reference as NB  # noqa: E402
from test_attention_long_gpu import guard_intact, guarded  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
SCORE = {"softplus": softplus_score_function, "linear": linear_score_function}
SENT = -7.5          # (exact in bf16)


def name(dt):
    return "f32" if dt == F32 else "bf16"


def host(t):
    return t.detach().double().cpu()


def _rel(got, ref):
    got, ref = host(torch.as_tensor(got)), host(torch.as_tensor(ref))
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


# ======================================================================================================================= kernels
class _Layer:
    """One recurrence on the device: fragments of W_hh, the forward pass (cpc_gru_fwd / cpc_gru_fwd_h0) and its tape."""

    def __init__(self, dt, B, V, H, w_hh, b_hh, Gi, h0=None):
        self.dt, self.B, self.V, self.H, self.code = dt, B, V, H, _hip.dtype_code(dt)
        code = self.code
        dW = w_hh.float().to(DEV).contiguous()
        self.wfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
        self.wTfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
        _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(self.wfrag), 3 * H, H, H, 0, code)
        _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(self.wTfrag), H, 3 * H, H, 1, code)
        dGi, db = Gi.to(dt).to(DEV).contiguous(), b_hh.float().to(DEV)
        nt = int(_hip.lib().cpc_gru_tape_elems(B, V, H, code))
        hb, Hall = guarded(B * (V + 1) * H, dt)
        cb, c = guarded(B * H, F32)
        tb, self.tape = guarded(nt, dt)
        if h0 is not None:
            dh0 = h0.float().to(DEV)
            _hip.call("cpc_gru_fwd_h0", _hip.ptr(dGi), _hip.ptr(self.wfrag), _hip.ptr(db), _hip.ptr(dh0), _hip.ptr(Hall), _hip.ptr(self.tape),
                      _hip.ptr(c), B, V, H, code)
        else:
            _hip.call("cpc_gru_fwd", _hip.ptr(dGi), _hip.ptr(self.wfrag), _hip.ptr(db), _hip.ptr(Hall), _hip.ptr(self.tape), _hip.ptr(c),
                      B, V, H, code)
        torch.cuda.synchronize()
        assert guard_intact(hb, B * (V + 1) * H) and guard_intact(cb, B * H) and guard_intact(tb, nt)
        self.Hall, self.c = host(Hall).view(B, V + 1, H), host(c).view(B, H)

    def dhs_buffer(self, dhs, ld_h=None, pad=float("nan")):
        """dhs (B, V, H) -> device rows of ld_h elements (default H); the pad columns hold NaN: they must never be read."""
        B, V, H = self.B, self.V, self.H
        ld_h = H if ld_h is None else ld_h
        buf = torch.full((B * V, ld_h), pad, dtype=self.dt)
        buf[:, :H] = dhs.reshape(B * V, H).to(self.dt)
        return buf.to(DEV).contiguous(), ld_h

    def bwd_steps(self, dc, dhs, ld_h=None, items=None):
        """cpc_gru_bwd_steps; dG comes back as (items, V, 4H) with items >= B rows of storage (the rows >= B start as sentinels)."""
        B, V, H = self.B, self.V, self.H
        items = B if items is None else items
        gb, dG = guarded(items * V * 4 * H, self.dt)
        dG[B * V * 4 * H:] = SENT
        ddc = None if dc is None else dc.float().to(DEV).contiguous()
        if dhs is None:
            dbuf, ld = None, 0
        else:
            dbuf, ld = self.dhs_buffer(dhs, ld_h)
        _hip.call("cpc_gru_bwd_steps", _hip.ptr(ddc), _hip.ptr(dbuf), _hip.C.c_longlong(ld), _hip.ptr(self.tape), _hip.ptr(self.wTfrag),
                  _hip.ptr(dG), B, V, H, self.code)
        torch.cuda.synchronize()
        assert guard_intact(gb, items * V * 4 * H)
        return dG.detach().clone().view(items, V, 4 * H)

    def bwd(self, dc):
        B, V, H = self.B, self.V, self.H
        gb, dG = guarded(B * V * 4 * H, self.dt)
        _hip.call("cpc_gru_bwd", _hip.ptr(dc.float().to(DEV).contiguous()), _hip.ptr(self.tape), _hip.ptr(self.wTfrag), _hip.ptr(dG),
                  B, V, H, self.code)
        torch.cuda.synchronize()
        assert guard_intact(gb, B * V * 4 * H)
        return dG.detach().clone().view(B, V, 4 * H)


def _layer_of(dt, case, ref):
    H, B, V = case
    return _Layer(dt, B, V, H, ref["w_hh"], ref["b_hh"], ref["Gi"], ref["h0"])


def _check_steps(dt, case, label):
    """Both calls of a case (the recipe's dc, and dc = NULL as a lower layer calls it) against the float64 reference, per step."""
    H, B, V = case
    for with_dc in (True, False):
        ref = S.stacked_reference(dt, case, with_dc=with_dc)
        if ref["e_model"] is not None:
            assert max(float(v.max()) for v in ref["e_model"].values()) < R.GRU_MODEL_CAP
        lay = _layer_of(dt, case, ref)
        dG = host(lay.bwd_steps(ref["dc"], ref["dhs"]))
        assert bool(torch.isfinite(dG).all())
        errs = R.gru_step_errors(lay.Hall, dG, ref["hall"], ref["dG"])
        for k in R.GRU_BLOCKS:
            ratio = (errs[k] / ref["tol"][k]).max().item()
            print(f"{label} {'dc' if with_dc else 'dc=NULL'} {k}: largest per-step error {errs[k].max().item():.2e}, error / bound {ratio:.2f}")
        bad = R.gru_violations(errs, ref["tol"])
        assert not bad, bad[:8]


@pytest.mark.parametrize("dt", [F32, BF16], ids=name)
@pytest.mark.parametrize("case", S.stacked_cases(), ids=S.stacked_case_id)
def test_bwd_steps_per_step(case, dt):
    """cpc_prep_frag, cpc_gru_fwd(_h0) and cpc_gru_bwd_steps in every family at its edges: B = 1 and 17 leave rows of a 16-row workgroup
    to mask, V = 1 has no step to prefetch, V = 2 is the first prefetched one, H = 96 and 224 have waves with unequal or no tiles,
    H = 288 and 512 run the 8-wave form; bf16 at H in {32, 64, 128, 256} is the weight-resident kernel."""
    _check_steps(dt, case, f"{S.stacked_case_id(case)} {name(dt)}")


def test_bwd_steps_streaming_forced_at_64():
    """The 4-wave streaming kernels at a hidden size the resident ones would take (bf16, H = 64), via cpc_gru_set_streaming."""
    old = _hip.lib().cpc_gru_set_streaming(1)
    try:
        assert int(_hip.lib().cpc_gru_tape_elems(17, 13, 64, _hip.BF16)) == 17 * 13 * 5 * 64
        _check_steps(BF16, (64, 17, 13), "forced streaming H64-B17-V13 bf16")
    finally:
        _hip.lib().cpc_gru_set_streaming(old)


FAMILIES = [(BF16, (64, 17, 13)), (BF16, (256, 17, 2)), (BF16, (96, 17, 13)), (F32, (64, 17, 13)), (BF16, (288, 17, 13)), (F32, (288, 17, 13))]
FAMILY_IDS = [f"{name(dt)}-{S.stacked_case_id(c)}" for dt, c in FAMILIES]


@pytest.mark.parametrize("dt,case", FAMILIES, ids=FAMILY_IDS)
def test_null_dhs_is_gru_bwd_and_zero_dhs_equals_it(dt, case):
    """dHs = NULL: cpc_gru_bwd's kernels, bit for bit.  dHs of zeros with dc given: the same numbers (a zero's sign may differ)."""
    ref = S.stacked_reference(dt, case)
    lay = _layer_of(dt, case, ref)
    plain = lay.bwd(ref["dc"])
    assert torch.equal(lay.bwd_steps(ref["dc"], None), plain)
    zeros = lay.bwd_steps(ref["dc"], torch.zeros_like(ref["dhs"]))
    assert bool((zeros.float() == plain.float()).all())
    assert float(plain.float().abs().max()) > 0


@pytest.mark.parametrize("dt", [F32, BF16], ids=name)
@pytest.mark.parametrize("H", [64, 96, 288])
def test_one_step_of_dhs_with_zero_weights(H, dt):
    """W_hh = 0, b_hh = 0, dc = NULL, dHs non-zero at one step s only (first, interior, last), for all (b, j): dG is exactly zero after
    s; at s it is the gate derivatives of dhs[:, s] alone, from the closed form of the gates (gru_closed_form_zero_weights' setting: the
    gates depend on the input projections only), judged like every step here, max |got - want| / max |want| within the step, against
    GRU_TOL_F32 (f32) or 2^-8 (bf16); before s it is dhs[:, s] prod u handed down: not zero, and within the same bound.

    The data is exact data (gru_stacked_reference.exact_gate_data): pre-activations of r and n from -12, 0, +12, different in every
    (b, t, j), and u = 0.5, so that the gates and hidden states the bf16 tape holds ARE the closed form's (to 6e-6), the gradient handed
    down is d 2^-k, every product is exact in f32, and the one rounding left is the store of the result: at most 2^-8 / (1 + 2^-8) of
    its value in bf16's 8 significant bits.  test_gru_stacked_host.py::test_exact_gate_data_is_exact_in_bf16 shows that on the host.
    (A first version of this test drew the input projections from N(0, 1): r, u, n and h_prev then each take a rounding of up to 2^-8
    when cpc_gru_fwd writes them to the bf16 tape, before the sweep under test runs at all, and a product of three or four of them
    was off by up to 1.6 x 2^-8 -- a property of that data, not of the sweep.)"""
    B, V = 17, 13
    Gi = S.exact_gate_data(B, V, H)
    gir = R.rounded(Gi, dt)
    assert torch.equal(gir, Gi.double())
    r, u, n, hp = S.zero_weight_gates(gir)
    assert (hp[:, 1:] - R.gru_closed_form_zero_weights(gir)[:, 1:V]).abs().max() < 1e-14
    lay = _Layer(dt, B, V, H, torch.zeros(3 * H, H), torch.zeros(3 * H), Gi)
    bad = []
    for s in (0, 6, V - 1):
        dhs = torch.zeros(B, V, H, dtype=torch.float64)
        dhs[:, s] = R.rounded(torch.randn(B, H, generator=torch.Generator().manual_seed(s + H)), dt)
        dG = host(lay.bwd_steps(None, dhs))
        assert bool((dG[:, s + 1:] == 0).all())
        assert bool((dG[:, :, :H] == 0).all())          # dr = dn_pre q r (1 - r) with q = 0
        d = dhs[:, s].clone()
        for t in range(s, -1, -1):
            want = {"du": d * (hp[:, t] - n[:, t]) * u[:, t] * (1 - u[:, t]), "dn": d * (1 - u[:, t]) * (1 - n[:, t] ** 2)}
            want["dnr"] = want["dn"] * r[:, t]
            for i, k in ((1, "du"), (2, "dn"), (3, "dnr")):
                got = dG[:, t, i * H:(i + 1) * H]
                err = float((got - want[k]).abs().max() / want[k].abs().max())
                bound = R.GRU_TOL_F32[k] if dt == F32 else 2.0 ** -8
                if t == s or t == 0:
                    print(f"zero weights {name(dt)} H={H} s={s} t={t} {k}: error {err:.2e} (bound {bound:.2e})")
                if not err <= bound:
                    bad.append((s, t, k, err, bound))
                assert float(got.abs().max()) > 0
            d = d * u[:, t]
    if bad:
        worst = max(bad, key=lambda v: v[3] / v[4])
        print(f"zero weights {name(dt)} H={H}: {len(bad)} of {3 * sum(s + 1 for s in (0, 6, V - 1))} figures above their bound, worst {worst}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("dt,case", FAMILIES, ids=FAMILY_IDS)
def test_neighbours_untouched_and_padded_rows(dt, case):
    """dG has storage for the whole last 16-row workgroup: the rows of items >= B are sentinels and stay.  A dHs buffer with rows of
    ld_h = H + 8 elements whose pad columns hold NaN gives the bits of the unpadded one."""
    H, B, V = case
    ref = S.stacked_reference(dt, case, with_dc=False)
    lay = _layer_of(dt, case, ref)
    items = (B + 15) // 16 * 16
    assert items > B
    whole = lay.bwd_steps(None, ref["dhs"], items=items)
    assert bool((whole[B:].float() == SENT).all())
    padded = lay.bwd_steps(None, ref["dhs"], ld_h=H + 8)
    assert torch.equal(padded, whole[:B]) and bool(torch.isfinite(padded.float()).all())


# ======================================================================================================================= models
E_S, V_S, K_S, B_S = 64, 12, 4, 8
SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E_S] * 5, 'bias': True}


def _model(dtype, L, H, seed=3, **gru):
    """The small encoder of test_gru_wide_gpu.py (64 channels, weights doubled so that the scores are not degenerate) with an
    AudioGRUModel(64, H, num_layers=L) context."""
    torch.manual_seed(seed)
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), AudioGRUModel(E_S, H, num_layers=L, **gru), enc_size=E_S, ar_size=H,
                                       visible_steps=V_S, prediction_steps=K_S, compute_dtype=dtype)
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if n.startswith("encoder.") and n.endswith("weight"):
                p_.mul_(2.0)
    return model


def _data(n, seed):
    L = _model("fp32", 1, 32).item_length
    return torch.randn(n, L, generator=torch.Generator().manual_seed(seed)) * 0.5


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


_REFERENCE = {}          # (L, H, score, all_t) -> (loss, grads): computed once, shared by the storage types, never modified


def _reference_step(L, H, params, data, score, all_t, reg):
    key = (L, H, score, all_t)
    if key not in _REFERENCE:
        so = S.StackedOracle(params, V_S, K_S, L, score=score, all_timesteps=all_t, regularization=reg, lr=0.0)
        loss, _, grads = so.loss_and_grads(data)
        _REFERENCE[key] = (float(loss), {k: v.detach().clone() for k, v in grads.items()})
    return _REFERENCE[key]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [64, 96, 288])
@pytest.mark.parametrize("L", [2, 3])
def test_stacked_model_loss_and_gradients_against_reference(L, H, dtype):
    """One trainer step (lr 0) of a 2- and 3-layer model at H = 64 (weight-resident in bf16), 96 and 288: loss and every parameter
    gradient, the upper cells' included, against the float64 stacked reference; softplus and linear scores, both loss branches."""
    data = _data(B_S, 1)
    model = _model(dtype, L, H).to(DEV)
    ctx = model.engine(B_S, data.shape[1]).ctx
    assert type(ctx).__name__ == "GRUContext" and ctx.L == L and len(ctx.upper) == L - 1
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    assert sum(k.startswith("autoregressive_model.upper_cells.") for k in params) == 4 * (L - 1)
    worst = {"encoder": 0.0, "context / predictor": 0.0, "loss": 0.0}
    for score in ("softplus", "linear"):
        for all_t, reg in ((False, 1.0), (True, 0.01)):
            model.load_state_dict(params)
            logger = _Logger()
            tr = _trainer(model, data, logger, H, SCORE[score], reg, all_t)
            tr.train(batch_size=B_S, epochs=1, lr=0.0, num_workers=0, max_steps=1)
            loss, grads = _reference_step(L, H, params, data, score, all_t, reg)
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
    print(f"L={L} H={H} {dtype}: largest relative loss error and relative l2 gradient errors", {k: f"{v:.2e}" for k, v in worst.items()})


class _Labelled(torch.utils.data.Dataset):
    def __init__(self, clips):
        self.clips = clips

    def __len__(self):
        return self.clips.shape[0]

    def __getitem__(self, i):
        return self.clips[i], i


def test_stacked_train_validate_and_task_data_against_reference():
    """train() for three Adam steps on a two-layer model (fp32) against the reference's steps from the same parameters, then validate()
    and calc_test_task_data() against the reference with its updated parameters (bounds of
    test_wide_gru_train_and_validate_against_oracle)."""
    B, steps, lr, H = 4, 3, 2e-4, 96
    data = _data(B, 5)
    model = _model("fp32", 2, H).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    so = S.StackedOracle(params, V_S, K_S, 2, score="softplus", regularization=1.0, lr=lr)
    want = [so.step(data)[0] for _ in range(steps)]
    val = _data(16, 6)
    logger = _Logger()
    tr = _trainer(model, data, logger, H, validation_set=TensorAudioDataset(val, device=DEV), test_task_set=_Labelled(val[:8]))
    tr.train(batch_size=B, epochs=steps, lr=lr, num_workers=0, max_steps=steps)
    got = logger.loss_meter.values
    assert len(got) == steps
    for i in range(steps):
        assert abs(got[i] - want[i]) <= 1e-4 * abs(want[i]) * (1 + 4 * i), (i, got, want)
    for k, v in model.state_dict().items():
        assert _rel(v, so.params[k]) < 1e-4 * (1 + 4 * steps), k
    losses, acc, score, mi = tr.validate(batch_size=8, num_workers=0)
    want_l, want_a = 0.0, 0.0
    lists = O.file_batch_sampler([val.shape[0]], 8, 8, True, seed=0)
    for idx in lists:
        pl, pa, _ = so.validation(val[idx])
        want_l, want_a = want_l + pl, want_a + pa
    assert _rel(losses, want_l / len(lists)) < 1e-4 * (1 + 4 * steps)
    assert (torch.as_tensor(acc).cpu().double() - want_a / len(lists)).abs().max().item() < 1e-4
    task, labels = tr.calc_test_task_data(batch_size=4, num_workers=0)
    with torch.no_grad():
        c = so.forward(val[:8], training=False)[3]
    assert list(labels) == list(range(8)) and R.rel_err(task, c) < 1e-4


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stacked_carried_state(dtype):
    """AudioGRUModel(reset_hidden=False, num_layers=2): the second call starts every layer from its own last state of the first call
    ((num_layers, B, H) in ``hidden``).  Its c against a float64 loop over the second call's z from those states, with the weights as
    the device stores them; the carried states make a difference; a backward pass after a carried start raises."""
    B, V, K, H = 7, 5, 2, 64
    torch.manual_seed(H)
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), AudioGRUModel(E_S, H, reset_hidden=False, num_layers=2), enc_size=E_S, ar_size=H,
                                       visible_steps=V, prediction_steps=K, compute_dtype=dtype).to(DEV)
    gen = torch.Generator().manual_seed(7)
    x1, x2 = (torch.randn(B, 1, model.item_length, generator=gen).to(DEV) for _ in range(2))
    with torch.no_grad():
        _, _, _, c1 = model(x1)
        h1 = model.autoregressive_model.hidden.detach().clone()
        _, _, z2, c2 = model(x2)
    assert tuple(h1.shape) == (2, B, H) and torch.equal(h1[1], c1)
    st = F32 if dtype == "fp32" else BF16
    p = {"autoregressive_model." + k: v.detach().cpu() for k, v in model.autoregressive_model.state_dict().items()}
    p = {k: (v.to(st).double() if "weight" in k else v.double()) for k, v in p.items()}
    zz = z2.detach().cpu().to(st).double()
    ref = S.stacked_gru_forward(zz, p, 2, h0=[h1[0].cpu().double(), h1[1].cpu().double()])
    fresh = S.stacked_gru_forward(zz, p, 2)
    err = R.rel_err(c2, ref)
    print(f"carried two-layer state, {dtype}: error of c {err:.2e}")
    assert err < (2e-5 if dtype == "fp32" else 2e-2)
    assert R.rel_err(c2, fresh) > 1e-2
    pred = model(x2)[0]
    with pytest.raises(RuntimeError, match="carried over"):
        pred.sum().backward()
    model.autoregressive_model.hidden = torch.zeros(B, H, device=DEV)          # a single layer's shape
    with pytest.raises(ValueError, match="carried GRU state"), torch.no_grad():
        model(x2)


def test_standalone_stacked_gru():
    """AudioGRUModel(32, 64, num_layers=2)(z) on its own (the _ContextForward bridge): output, z.grad and every parameter gradient
    against torch autograd on two stacked nn.GRUCell in float64 (fp32: 1e-4 output, 1e-3 gradients)."""
    B, E, V, H = 5, 32, 9, 64
    torch.manual_seed(8)
    gru = AudioGRUModel(E, H, num_layers=2)
    cells = [torch.nn.GRUCell(E, H).double(), torch.nn.GRUCell(H, H).double()]
    cells[0].load_state_dict({k: v.double() for k, v in gru.gruCell.state_dict().items()})
    cells[1].load_state_dict({k: v.double() for k, v in gru.upper_cells[0].state_dict().items()})
    z = torch.randn(B, E, V, generator=torch.Generator().manual_seed(9))
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(10))
    zr = z.double().requires_grad_(True)
    hs = [torch.zeros(B, H, dtype=torch.float64) for _ in range(2)]
    for t in range(V):
        hs[0] = cells[0](zr[:, :, t], hs[0])
        hs[1] = cells[1](hs[0], hs[1])
    (hs[1] * dh.double()).sum().backward()
    gru = gru.to(DEV)
    zd = z.to(DEV).requires_grad_(True)
    out = gru(zd)
    assert R.rel_err(out, hs[1]) < 1e-4
    (out * dh.to(DEV)).sum().backward()
    assert R.rel_err(zd.grad, zr.grad) < 1e-3
    for cell, mod in zip(cells, (gru.gruCell, gru.upper_cells[0])):
        ref = dict(cell.named_parameters())
        for n, p_ in mod.named_parameters():
            assert R.rel_err(p_.grad, ref[n].grad) < 1e-3, n


# ------------------------------------------------------------------------------------------ the rest of the step around a stack
H_O, LR_O = 64, 2e-4


def _two_steps(route, seed=11, **attrs):
    """Two Adam steps of a two-layer fp32 model with the trainer's attributes ``attrs``: route 'fused' (the engine's step), 'generic'
    (a score function the trainer does not recognise: autograd through model.forward, torch optimizers).  The batch is the whole set."""
    data = _data(B_S, seed)
    model = _model("fp32", 2, H_O).to(DEV)
    logger = _Logger()
    sf = softplus_score_function if route == "fused" else (lambda p, t: softplus_score_function(p, t))
    tr = _trainer(model, data, logger, H_O, sf)
    assert tr._fused() == (route == "fused")
    for k, v in attrs.items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    random.seed(5)
    tr.train(batch_size=B_S, epochs=2, lr=LR_O, num_workers=0, max_steps=2)
    torch.cuda.synchronize()
    assert len(logger.loss_meter.values) == 2
    return logger.loss_meter.values, {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}, tr


def _same_run(a, b):
    for la, lb in zip(a[0], b[0]):
        assert abs(la - lb) <= 1e-5 * abs(lb), (a[0], b[0])
    for k in a[1]:
        assert _rel(a[1][k], b[1][k]) < 1e-4, k


OPTIONS = {"clip and decay": dict(max_grad_norm=0.05, weight_decay=0.05), "trust ratio": dict(trust_ratio=True, weight_decay=0.01),
           "ema": dict(ema_decay=0.5)}


@pytest.mark.parametrize("option", list(OPTIONS))
def test_options_around_a_stack_against_the_generic_route(option):
    """max_grad_norm with weight_decay (AdamW), trust_ratio (LAMB) and ema_decay on a two-layer model: two fused steps against the same
    option on the generic route (1e-5 on the losses, 1e-4 on every parameter, relative l2)."""
    fused, generic = _two_steps("fused", **OPTIONS[option]), _two_steps("generic", **OPTIONS[option])
    _same_run(fused, generic)
    if option == "ema":          # the average leaves the parameters alone: the shadow is what the option adds
        assert _rel(fused[2]._ema, generic[2]._ema) < 1e-4
        assert _rel(fused[2]._ema, fused[2].model._flat_param) > 1e-5
    else:
        plain = _two_steps("fused")
        assert any(_rel(fused[1][k], plain[1][k]) > 1e-4 for k in plain[1]), "the option made no difference"


def test_graphed_step_around_a_stack():
    """use_graph: two replayed steps of a two-layer model against the ungraphed ones."""
    _same_run(_two_steps("fused", use_graph=True), _two_steps("fused"))


def test_negative_bank_around_a_stack():
    """negative_bank = 2 on a two-layer model (fp32): three engine steps on three batches, loss and every gradient against autograd of the
    float64 stacked reference with the banked reference loss on its outputs (negative_bank_reference.banked_loss; 1e-4 / 1e-3, the
    bounds of test_negative_bank_gpu.py's engine test)."""
    data = _data(3 * B_S, 13)
    model = _model("fp32", 2, H_O).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    so = S.StackedOracle(params, V_S, K_S, 2)
    eng = model.engine(B_S, data.shape[1])
    bank, reg = NegativeBank(2), 0.5
    rows, cur, valid = None, 0, 1
    for i in range(3):
        x = data[i * B_S:(i + 1) * B_S]
        out = eng.loss_and_grads(x.to(DEV), softplus=True, regularization=reg, score="softplus", negative_bank=bank)
        torch.cuda.synchronize()
        for p in so.params.values():
            p.grad = None
        pred, targ, _, _ = so.forward(x)
        rows = [torch.zeros_like(pred) for _ in range(3)] if rows is None else rows
        rows[cur] = pred
        loss, _ = NB.banked_loss(torch.cat(rows), targ, cur, valid, True, reg)
        loss.backward()
        rows[cur] = pred.detach()
        cur = (cur + 1) % 3
        valid |= 1 << cur
        want = float(loss.detach())
        assert abs(float(out[0]) - want) < 1e-4 * abs(want), (i, float(out[0]), want)
        for pname, p in so.params.items():
            assert _rel(model._grad[pname], p.grad) < 1e-3, (i, pname)
    assert bank.filled == 2


def test_scalogram_engine_with_a_stacked_gru(golden_dir):
    """One fp32 step (lr 0) on the smallest scalogram fixture's encoder with a two-layer GRU context, against the composed float64
    reference (1e-4 loss, 1e-3 gradients)."""
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    z = np.load(os.path.join(golden_dir, "scalogram_model.npz"))
    meta = copy.deepcopy(json.load(open(os.path.join(golden_dir, "scalogram_model.json"))))
    B, K, E, V, H = meta["B"], meta["K"], meta["E"], meta["V"], 64
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    torch.manual_seed(21)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(E, H, num_layers=2), enc_size=E, ar_size=H, visible_steps=V, prediction_steps=K,
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
    ctx = model.engine_for(scal).ctx
    assert type(ctx).__name__ == "GRUContext" and ctx.L == 2
    random.seed(91)
    tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    so = S.StackedOracle(params, V, K, 2, score="softplus", regularization=0.01, lr=0.0, scalogram=oblocks)
    loss, _, grads = so.loss_and_grads(scal.float().cpu())
    got = logger.loss_meter.values[0]
    assert abs(got - float(loss)) < 1e-4 * abs(float(loss)), (got, float(loss))
    named = dict(model.named_parameters())
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for pname, ref in grads.items():
        if ref.abs().max().item() < 1e-6 * largest:          # a convolution bias in front of a train-mode BatchNorm: zero gradient
            assert named[pname].grad.abs().max().item() < 1e-5 * largest, pname
            continue
        assert _rel(named[pname].grad, ref) < 1e-3, pname


# ------------------------------------------------------------------------------------------ the single-layer step
# What GRUContext(num_layers = 1) launched before stacks existed, in order: prepare_weights, forward, backward (the parameter gradients
# on the side stream between the sweep and the dz GEMM), read off GRUContext (then in engine.py) at that commit.
PARENT_LAUNCHES = {
    "prepare_weights": ["cpc_cast2d", "cpc_cast2d", "cpc_prep_frag", "cpc_prep_frag"],
    "forward": ["gemm_nt", "cpc_gru_fwd"],
    "backward": ["cpc_gru_bwd",
                 "gemm_tn", "cpc_reduce_slabs", "gemm_tn", "cpc_reduce_slabs", "gemm_tn", "cpc_reduce_slabs",
                 "cpc_colsum", "cpc_reduce_slabs", "cpc_reduce_slabs", "cpc_reduce_slabs",
                 "gemm_nt"],
}
_LAYER_PARAMS = ["gemm_tn", "cpc_reduce_slabs", "gemm_tn", "cpc_reduce_slabs", "gemm_tn", "cpc_reduce_slabs",
                 "cpc_colsum", "cpc_reduce_slabs", "cpc_reduce_slabs", "cpc_reduce_slabs"]
# The same three phases of the two-layer context (_model(dtype, 2, 64), both storage types alike), recorded with _Spy at the commit
# before GRUContext's layers became one loop: per layer the projection GEMM and the recurrence; backward the top sweep, that layer's
# parameter gradients, the GEMM that hands dH down, the sweep below with its parameter gradients, the dz GEMM.
PARENT_LAUNCHES_TWO_LAYERS = {
    "prepare_weights": ["cpc_cast2d", "cpc_cast2d", "cpc_prep_frag", "cpc_prep_frag"] * 2,
    "forward": ["gemm_nt", "cpc_gru_fwd", "gemm_nt", "cpc_gru_fwd"],
    "backward": ["cpc_gru_bwd"] + _LAYER_PARAMS + ["gemm_nt", "cpc_gru_bwd_steps"] + _LAYER_PARAMS + ["gemm_nt"],
}


def _context_launches(eng):
    got, ctx = {}, eng.ctx
    for phase, fn in (("prepare_weights", ctx.prepare_weights), ("forward", ctx.forward), ("backward", lambda: ctx.backward(eng.dc))):
        with _Spy() as spy:
            fn()
            torch.cuda.current_stream().wait_stream(eng.aux)
            torch.cuda.synchronize()
        got[phase] = spy.names
    return got


class _Spy:
    """Records the names that go through _hip.call, _hip.gemm_nt and _hip.gemm_tn while active."""

    def __enter__(self):
        self.names, self.real = [], (_hip.call, _hip.gemm_nt, _hip.gemm_tn)

        def call(fn, *a, **kw):
            self.names.append(fn)
            return self.real[0](fn, *a, **kw)

        def nt(*a, **kw):
            self.names.append("gemm_nt")
            return self.real[1](*a, **kw)

        def tn(*a, **kw):
            self.names.append("gemm_tn")
            return self.real[2](*a, **kw)

        _hip.call, _hip.gemm_nt, _hip.gemm_tn = call, nt, tn
        return self

    def __exit__(self, *exc):
        _hip.call, _hip.gemm_nt, _hip.gemm_tn = self.real


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_single_layer_step_is_the_parent_step(dtype):
    """A step of a num_layers = 1 model never names cpc_gru_bwd_steps, and its context launches exactly what it launched before; a
    two-layer context adds, per upper layer, one projection GEMM and one recurrence forward, and one sweep, one GEMM and a set of
    parameter-gradient launches backward."""
    data = _data(B_S, 1)
    model = _model(dtype, 1, 64).to(DEV)
    eng = model.engine(B_S, data.shape[1])
    with _Spy() as spy:
        eng.loss_and_grads(data.to(DEV), softplus=True, regularization=1.0)
        torch.cuda.synchronize()
    assert "cpc_gru_bwd_steps" not in spy.names and spy.names.count("cpc_gru_bwd") == 1 and spy.names.count("cpc_gru_fwd") == 1
    ctx = eng.ctx
    assert ctx.L == 1 and ctx.upper == []
    assert _context_launches(eng) == PARENT_LAUNCHES
    model2 = _model(dtype, 2, 64).to(DEV)
    eng2 = model2.engine(B_S, data.shape[1])
    eng2.loss_and_grads(data.to(DEV), softplus=True, regularization=1.0)
    got2 = _context_launches(eng2)
    assert got2 == PARENT_LAUNCHES_TWO_LAYERS
    n = got2["prepare_weights"] + got2["forward"] + got2["backward"]
    assert n.count("cpc_gru_fwd") == 2 and n.count("cpc_gru_bwd") == 1 and n.count("cpc_gru_bwd_steps") == 1
    assert n.count("gemm_nt") == 2 + 2 and n.count("gemm_tn") == 6 and n.count("cpc_prep_frag") == 4
    assert n.index("cpc_gru_bwd") < n.index("cpc_gru_bwd_steps")
