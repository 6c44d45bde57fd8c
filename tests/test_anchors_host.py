"""Prediction anchors without a GPU: the float64 reference of tests/anchor_reference.py against the oracle, the constructor's refusals,
the state dict, every CPC_EINVAL precondition of cpc_lstm_bwd_steps and cpc_anchor_target_grad (the library loads without a GPU and the
calls are refused before any launch), and the trainer's refusals.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioLSTMModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction,
                                                           difference_score_function, linear_score_function, softplus_score_function)
from oracle import cpc_oracle as O
import anchor_reference as R

E_S, V_S, K_S = 64, 12, 4
SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E_S] * 5, 'bias': True}


def _model(ar=None, **kw):
    torch.manual_seed(3)
    ar = AudioGRUModel(E_S, 32) if ar is None else ar
    return AudioPredictiveCodingModel(AudioEncoder(SMALL), ar, enc_size=E_S, ar_size=32, visible_steps=V_S, prediction_steps=K_S,
                                      compute_dtype="fp32", **kw)


def test_stacked_heads_are_single_anchor_models_on_shortened_clips():
    """(A, s) = (3, 2), regularization 0: the stacked-head loss of the reference equals the mean of O.info_nce_loss over three
    O.cpc_forward calls on the clip shortened by d_a * downsampling samples at its end, with visible_steps = V - d_a; so does every
    parameter gradient.  1e-12 relative in float64 (sums of a few thousand float64 terms in another order)."""
    A, s, B = 3, 2, 6
    params = O.init_params(channels=(E_S,) * 5, ar_size=32, prediction_steps=K_S, seed=5, dtype=torch.float64)
    for k in params:
        if k.startswith("encoder.") and k.endswith("weight"):
            params[k] = params[k] * 2.0
    ds, rf = O.encoder_geometry(O.DEFAULT_STRIDES, O.DEFAULT_KERNELS)
    length = O.item_length(rf, ds, V_S, K_S)
    x = torch.randn(B, length, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.5
    for score in ("softplus", "linear"):
        orc = R.AnchorOracle(params, V_S, K_S, A, s, ("gru", 1), score=score, regularization=0.0)
        loss, _, grads = orc.loss_and_grads(x)
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        total = 0.0
        for d in R.shifts(A, s):
            clip = x[:, :length - d * ds].unsqueeze(1)
            pred, targ, z, _ = O.cpc_forward(clip, leaves, V_S - d, K_S)
            assert z.shape[2] == V_S - d
            total = total + O.info_nce_loss(O.SCORE_FUNCTIONS[score](pred, targ), False, 0.0)[0]
        mean = total / A
        mean.backward()
        mean = mean.detach()
        assert abs(float(loss) - float(mean)) <= 1e-12 * abs(float(mean)), (score, float(loss), float(mean))
        for k, g in grads.items():
            ref = leaves[k].grad
            assert float((g - ref).norm()) <= 1e-12 * float(ref.norm()), (score, k)
    # the last anchor alone is the oracle's model
    one = R.AnchorOracle(params, V_S, K_S, 1, 1, ("gru", 1))
    pred, targ, z, c = one.forward(x)
    want = O.cpc_forward(x.unsqueeze(1), params, V_S, K_S)
    for got, ref in zip((pred, targ, z, c), want):
        assert torch.allclose(got, ref, rtol=1e-13, atol=1e-13)


def test_reference_lstm_sweep_with_injected_gradients_is_autograd():
    """lstm_run_steps in float64 against autograd of sum_t <dHs[:, t], h_{t+1}> + <dh_last, h_V>; without dHs it is lstm_run."""
    import lstm_reference as L
    B, V, H = 3, 5, 16
    w, b, Gi, dh, _, _ = (None if t is None else t.double() for t in L.lstm_data(B, V, H))
    dHs = torch.randn(B, V, H, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    for dh_last, inj in ((dh, dHs), (None, dHs), (dh, None)):
        dG = R.lstm_run_steps(Gi, w, b, dh_last, inj)[3]
        ref = R.lstm_steps_autograd(Gi, w, b, dh_last, inj)
        assert float((dG - ref).abs().max()) < 1e-12
    assert torch.equal(R.lstm_run_steps(Gi, w, b, dh, None)[3], L.lstm_run(Gi, w, b, dh)[3])


def test_reference_target_gather_against_a_scatter():
    """The numpy restatement of cpc_anchor_target_grad against the obvious scatter-add of every window."""
    rng = np.random.default_rng(0)
    A, B, K, E, rows, first, stride = 3, 2, 4, 8, 20, 5, 3
    dT = rng.integers(-3, 4, size=(A, B, K, E)).astype(np.float64)
    full = np.zeros((B, rows, E))
    for a in range(A):
        full[:, first + a * stride:first + a * stride + K] += dT[a]
    base = rng.integers(-3, 4, size=(B, rows, E)).astype(np.float64)
    lo, hi = 3, 17
    got = R.anchor_target_grad(dT, base, first, stride, lo, hi, 0)
    assert np.array_equal(got[:, lo:hi], full[:, lo:hi]) and np.array_equal(got[:, :lo], base[:, :lo]) and np.array_equal(got[:, hi:], base[:, hi:])
    got = R.anchor_target_grad(dT, base, first, stride, lo, hi, 1)
    want = base.copy()
    want[:, lo:hi] += full[:, lo:hi]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kw", [dict(prediction_anchors=0), dict(anchor_stride=0), dict(prediction_anchors=-1), dict(prediction_anchors=True),
                                dict(anchor_stride=True), dict(prediction_anchors=2.0), dict(prediction_anchors=2, anchor_stride=V_S),
                                dict(prediction_anchors=V_S + 1, anchor_stride=1), dict(prediction_anchors=4, anchor_stride=4)])
def test_constructor_refuses_bad_anchor_settings(kw):
    """A = 0, s = 0, bools, non-ints, and (A - 1) s = V (or more) raise ValueError in the constructor."""
    with pytest.raises(ValueError, match="prediction_anchors|anchor_stride"):
        _model(**kw)


def test_constructor_accepts_the_edges_and_adds_no_parameter():
    """(A - 1) s = V - 1 is allowed; state_dict keys and shapes do not depend on the setting; the defaults are (1, 1)."""
    base = _model()
    assert (base.prediction_anchors, base.anchor_stride) == (1, 1)
    assert _model(prediction_anchors=1, anchor_stride=1000).anchor_stride == 1000          # a single anchor has no shift to bound
    for kw in (dict(prediction_anchors=3, anchor_stride=2), dict(prediction_anchors=V_S, anchor_stride=1),
               dict(prediction_anchors=2, anchor_stride=V_S - 1)):
        for ar in (AudioGRUModel(E_S, 32), AudioGRUModel(E_S, 32, num_layers=2), AudioLSTMModel(E_S, 32)):
            m = _model(ar=ar, **kw)
            ref = _model(ar=type(ar)(E_S, 32, **({"num_layers": 2} if getattr(ar, "num_layers", 1) == 2 else {})))
            assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
            ref.load_state_dict(m.state_dict())
    m3, m1 = _model(prediction_anchors=3), _model()
    assert list(m3.state_dict()) == list(m1.state_dict())
    assert all(m3.state_dict()[k].shape == m1.state_dict()[k].shape for k in m1.state_dict())


def test_lstm_bwd_steps_argument_checks_come_before_any_launch():
    """Every CPC_EINVAL precondition of cpc_lstm_bwd_steps, with pointers that are never dereferenced."""
    lib = _hip.lib()
    P, s = C.c_void_p(0x1000), C.c_void_p(0)
    f32, bf16 = _hip.F32, _hip.BF16

    def steps(dh=P, dHs=P, ld_h=32, tape=P, WT=P, dG=P, B=2, V=3, H=32, dt=bf16):
        return lib.cpc_lstm_bwd_steps(dh, dHs, C.c_longlong(ld_h), tape, WT, dG, B, V, H, dt, s)

    for name in ("tape", "WT", "dG"):
        assert steps(**{name: None}) == -22, name
    assert steps(dh=None, dHs=None) == -22
    for ld in (31, 24, 0, -32, 36, 33):          # below H, or no multiple of 8 in bf16
        assert steps(ld_h=ld) == -22, ld
    for ld in (15, 18, 17, 0):                   # f32, H = 16: below H, or no multiple of 4
        assert steps(ld_h=ld, H=16, dt=f32) == -22, ld
    bad_shapes = [dict(B=0), dict(B=-1), dict(V=0), dict(H=0), dict(H=-32), dict(H=40), dict(H=48), dict(H=16), dict(H=528), dict(H=1024),
                  dict(dt=2), dict(dt=-1), dict(H=8, dt=f32), dict(H=24, dt=f32), dict(H=528, dt=f32)]
    for kw in bad_shapes:
        kw = dict(kw)
        kw.setdefault("ld_h", max(kw.get("H", 32), 8) + 8 * 64)          # a good ld_h for every H: the refusal is the shape's
        assert steps(**kw) == -22, kw
        assert steps(dh=None, **kw) == -22, kw


def test_anchor_target_grad_argument_checks_come_before_any_launch():
    """Every CPC_EINVAL precondition of cpc_anchor_target_grad, with pointers that are never dereferenced."""
    lib = _hip.lib()
    P, s = C.c_void_p(0x1000), C.c_void_p(0)
    f32, bf16 = _hip.F32, _hip.BF16

    def atg(dT=P, dtop=P, item=20 * 64, A=2, B=2, K=4, E=64, first=3, stride=2, lo=3, hi=9, acc=0, dt=bf16):
        return lib.cpc_anchor_target_grad(dT, dtop, C.c_longlong(item), A, B, K, E, first, stride, lo, hi, acc, dt, s)

    assert atg(dT=None) == -22 and atg(dtop=None) == -22
    for kw in (dict(A=0), dict(A=-1), dict(B=0), dict(B=-2), dict(K=0), dict(K=-1), dict(stride=0), dict(stride=-1),
               dict(E=0), dict(E=-8), dict(E=4), dict(E=12), dict(E=68), dict(E=2, dt=f32), dict(E=6, dt=f32),
               dict(lo=5, hi=5), dict(lo=6, hi=5), dict(lo=-1, hi=4), dict(lo=0, hi=0), dict(lo=0, hi=-3),
               dict(dt=2), dict(dt=-1), dict(item=20 * 64 + 4), dict(item=8 * 64)):
        for acc in (0, 1):
            assert atg(acc=acc, **kw) == -22, kw


class _Logger:
    def log(self, step):
        pass


REFUSED = {
    "score_over_all_timesteps": dict(score_over_all_timesteps=True),
    "num_negatives": dict(num_negatives=2),
    "negative_groups": dict(negative_groups="same_file"),
    "negative_bank": dict(negative_bank=2),
    "global_negatives": dict(global_negatives=True),
    "gradient penalty": dict(wasserstein_gradient_penalty=True),
    "difference scores": dict(score_function=difference_score_function),
    "normalized scores": dict(score_function=NormalizedScoreFunction(0.1)),
    "foreign score function": dict(score_function=lambda p, t: softplus_score_function(p, t)),
    "foreign optimizer": dict(optimizer=torch.optim.SGD),
    "use_graph": dict(use_graph=True),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_trainer_refuses_what_anchors_do_not_cover_before_any_launch(what, monkeypatch):
    """Each unsupported combination raises NotImplementedError naming prediction_anchors from train(), before anything is launched
    through the binding (call / gemm_nt / gemm_tn are patched to fail); the same settings with a single anchor pass the check."""
    def boom(*a, **k):
        raise AssertionError("a launch was attempted")
    for fn in ("call", "gemm_nt", "gemm_tn"):
        monkeypatch.setattr(_hip, fn, boom)
    for A, refused in ((3, True), (1, False)):
        model = _model(prediction_anchors=A, anchor_stride=2)
        tr = ContrastiveEstimationTrainer(model=model, dataset=None, logger=_Logger(), score_function=linear_score_function,
                                          prediction_steps=K_S, ar_size=32)
        for k, v in REFUSED[what].items():
            assert hasattr(tr, k), k
            setattr(tr, k, v)
        if refused:
            with pytest.raises(NotImplementedError, match="prediction_anchors = 3"):
                tr.train(batch_size=4, epochs=1, lr=1e-4, num_workers=0, max_steps=1)
            with pytest.raises(NotImplementedError, match="prediction_anchors = 3"):
                tr._check_anchors()
        else:
            tr._check_anchors()
    # the supported route passes the check with anchors
    tr = ContrastiveEstimationTrainer(model=_model(prediction_anchors=3, anchor_stride=2), dataset=None, logger=_Logger(),
                                      score_function=softplus_score_function, prediction_steps=K_S, ar_size=32)
    tr._check_anchors()
    for k, v in dict(max_grad_norm=0.1, weight_decay=0.01, ema_decay=0.9, trust_ratio=True).items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    tr._check_anchors()
