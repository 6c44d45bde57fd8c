"""EMA of the weights, what needs no GPU: engine.TorchEma in float64 against a numpy restatement of the definition, the warmup
formula, decay 0, the argument checks of cpc_ema and cpc_ema_swap (refused before any launch), the up-front refusals of check_ema,
FusedAdam and ContrastiveEstimationTrainer, and FusedAdam's state dict with and without the shadow on a CPU-flattened model."""
import ctypes as C

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd import engine
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer
from cpc_audio_amd.engine import FusedAdam, TorchEma, check_ema, ema_weight

L, F = C.c_longlong, C.c_float
SHAPES = [("conv.weight", (6, 4, 3)), ("conv.bias", (6,)), ("gru.weight_hh", (12, 4)), ("head.weight", (5, 7))]


def _named(seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    return [(name, torch.nn.Parameter(torch.randn(*shape, generator=gen, dtype=dtype))) for name, shape in SHAPES]


# ------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("warmup", [False, True])
def test_torch_ema_is_the_definition(warmup):
    """Five updates in float64 against ema + (p - ema) * (1 - d) in numpy, d = decay or min(decay, (1 + t) / (10 + t)): to 1e-12."""
    decay = 0.75          # above (1 + t) / (10 + t) up to t = 26: the warmup binds at every step here
    named = _named(1)
    ema = TorchEma(named, decay, warmup)
    ref = {n: p.detach().numpy().copy() for n, p in named}
    for n, p in named:
        assert torch.equal(ema.shadow[n], p.detach()) and ema.shadow[n].data_ptr() != p.data_ptr()          # starts as a copy
    gen = torch.Generator().manual_seed(2)
    for t in range(1, 6):
        with torch.no_grad():
            for n, p in named:
                p.add_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.1)
        ema.update(t)
        d = min(decay, (1 + t) / (10 + t)) if warmup else decay
        assert warmup == (d != decay)
        for n, p in named:
            ref[n] = ref[n] + (p.detach().numpy() - ref[n]) * (1 - d)
            assert np.abs(ema.shadow[n].numpy() - ref[n]).max() <= 1e-12, (n, t)
    assert ema.updates == 5
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            ema.update(bad)


def test_warmup_formula():
    for t, want in ((1, 2 / 11), (2, 3 / 12), (100, 101 / 110)):
        assert ema_weight(0.9999, True, t) == 1.0 - want, t
        assert ema_weight(0.9999, False, t) == 1.0 - 0.9999
    assert ema_weight(0.9, True, 100) == 1.0 - 0.9          # the decay binds once (1 + t) / (10 + t) passes it (t = 80 for 0.9)
    assert ema_weight(0.9, True, 79) > 1.0 - 0.9 and ema_weight(0.9, True, 81) == 1.0 - 0.9


def test_decay_zero_makes_the_shadow_the_parameters():
    """w = 1 copies: (p - ema) + ema rounds twice and would not give p back bit for bit."""
    named = _named(3, torch.float32)
    ema = TorchEma(named, 0.0)
    with torch.no_grad():
        for n, p in named:
            p.mul_(1e-9).add_(1e-12)          # far below the shadow's magnitudes
    ema.update(1)
    for n, p in named:
        assert torch.equal(ema.shadow[n], p.detach()), n


def test_torch_ema_swap_weights_and_state():
    named = _named(4, torch.float32)
    ema = TorchEma(named, 0.5)
    with torch.no_grad():
        for n, p in named:
            p.add_(1.0)
    ema.update(1)
    raw = {n: p.detach().clone() for n, p in named}
    avg = {n: e.clone() for n, e in ema.shadow.items()}
    with pytest.raises(KeyError):
        with ema.weights():
            for n, p in named:
                assert torch.equal(p.detach(), avg[n]) and not torch.equal(p.detach(), raw[n])
            with pytest.raises(RuntimeError):
                with ema.weights():
                    pass
            with pytest.raises(RuntimeError):
                ema.update(2)
            raise KeyError("inside")
    for n, p in named:          # back after the exception, bit for bit
        assert torch.equal(p.detach(), raw[n]) and torch.equal(ema.shadow[n], avg[n])
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "ema"} and set(sd["ema"]) == set(raw)
    other = TorchEma(_named(5, torch.float32), 0.9)
    other.load_state_dict(sd)
    assert all(torch.equal(other.shadow[n], avg[n]) for n in avg) and other.decay == 0.9
    with pytest.raises(ValueError):
        other.load_state_dict({"ema": {n: v for n, v in list(avg.items())[:-1]}})
    with pytest.raises(ValueError):
        other.load_state_dict({"ema": {n: v.reshape(-1) for n, v in avg.items()}})
    with pytest.raises(ValueError):
        TorchEma(named, None)
    given = {n: torch.zeros_like(p) for n, p in named}
    mine = TorchEma(named, 0.5, shadow=given)
    mine.update(1)
    assert all(mine.shadow[n] is given[n] and torch.equal(given[n], 0.5 * raw[n]) for n in given)          # updated in place


# ------------------------------------------------------------------------------------------ the entry points' argument checks
def test_entry_points_check_their_arguments_before_any_launch():
    """Every refusal include/cpc_hip.h states for cpc_ema and cpc_ema_swap returns CPC_EINVAL (-22) from the argument check: no kernel
    is launched, so this runs without a GPU."""
    lib = _hip.lib()
    for name in ("cpc_ema", "cpc_ema_swap"):
        assert name in _hip.EXPORTED_SYMBOLS
    P, Q = C.c_void_p(0x1000), C.c_void_p(0x2000)          # 16-byte aligned, never dereferenced
    s = C.c_void_p(0)

    def ema(p=P, e=Q, n=64, decay=0.9, warmup=0, step=1, state=None, skip=None):
        return lib.cpc_ema(p, e, L(n), F(decay), warmup, step, state, skip, s)

    def swap(p=P, e=Q, n=64):
        return lib.cpc_ema_swap(p, e, L(n), s)

    for call in (ema, swap):
        assert call(p=None) == -22 and call(e=None) == -22
        assert call(n=0) == -22 and call(n=-4) == -22
        for off in (4, 8, 12, 1):
            assert call(p=C.c_void_p(0x1000 + off)) == -22 and call(e=C.c_void_p(0x2000 + off)) == -22, off
    for bad in (1.0, 1.5, -0.1, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert ema(decay=bad) == -22, bad
        assert ema(decay=bad, state=P) == -22, bad
    # the host route counts from 1; the device route reads its count from the state and ignores the argument
    for bad in (0, -1):
        assert ema(step=bad) == -22 and ema(step=bad, warmup=1) == -22
    for bad in (dict(p=None), dict(e=None), dict(n=0), dict(decay=1.0)):
        assert ema(state=P, step=0, **bad) == -22, bad


# ------------------------------------------------------------------------------------------ refusals up front
BAD_DECAYS = (True, False, "0.9", [0.9], 1.0, 1.5, -0.1, float("nan"), float("inf"), float("-inf"))


def test_check_ema():
    assert check_ema(None) == (None, False) and check_ema(None, False) == (None, False)
    assert check_ema(0.999, True) == (0.999, True) and check_ema(0, False) == (0.0, False) and check_ema(np.float32(0.5)) == (0.5, False)
    for bad in BAD_DECAYS:
        with pytest.raises(ValueError, match="ema_decay"):
            check_ema(bad)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="ema_warmup"):
            check_ema(0.9, bad)
    with pytest.raises(ValueError, match="ema_warmup"):
        check_ema(None, True)


def test_trainer_refuses_up_front():
    """Before any GPU work (there is no model, dataset or device here to get as far as one)."""
    tr = ContrastiveEstimationTrainer(model=None, dataset=None)
    assert tr.ema_decay is None and tr.ema_warmup is False
    for bad in BAD_DECAYS:
        tr.ema_decay = bad
        with pytest.raises(ValueError):
            tr.train(batch_size=4, max_steps=1)
    tr.ema_decay = 0.9
    for bad in (1, "yes", None):
        tr.ema_warmup = bad
        with pytest.raises(ValueError):
            tr.train(batch_size=4, max_steps=1)
    tr.ema_decay, tr.ema_warmup = None, True
    with pytest.raises(ValueError):
        tr.train(batch_size=4, max_steps=1)
    # no average exists: nothing to evaluate or export
    tr.ema_warmup = False
    with pytest.raises(ValueError, match="average"):
        tr.validate(use_ema=True)
    with pytest.raises(ValueError, match="average"):
        tr.calc_test_task_data(use_ema=True)
    with pytest.raises(ValueError, match="average"):
        tr.ema_state_dict()
    tr.reset_ema()


def _cpu_model(seed=0):
    torch.manual_seed(seed)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=16), enc_size=8, ar_size=16, visible_steps=6,
                                       prediction_steps=3, compute_dtype="fp32")
    model._flatten_parameters("cpu")
    return model


def test_fused_adam_refusals_and_the_shadow(monkeypatch):
    model = _cpu_model()

    def no_launch(name, *a, **kw):
        raise AssertionError(f"FusedAdam launched {name}")

    monkeypatch.setattr(_hip, "call", no_launch)
    for bad in BAD_DECAYS:
        with pytest.raises(ValueError):
            FusedAdam(model, lr=1e-3, ema_decay=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            FusedAdam(model, lr=1e-3, ema_decay=0.9, ema_warmup=bad)
    with pytest.raises(ValueError):
        FusedAdam(model, lr=1e-3, ema_warmup=True)
    flat = model._flat_param
    for bad in (torch.zeros(flat.numel() - 64), torch.zeros(flat.numel(), dtype=torch.float64), torch.zeros(1, flat.numel()), "shadow"):
        with pytest.raises(ValueError):
            FusedAdam(model, lr=1e-3, ema_decay=0.9, ema=bad)
    with pytest.raises(ValueError):
        FusedAdam(model, lr=1e-3, ema=torch.zeros_like(flat))          # a shadow without a decay
    plain = FusedAdam(model, lr=1e-3)
    assert plain.ema is None and plain.ema_decay is None and plain.ema_warmup is False          # nothing new without the keyword
    for call in (plain.swap_ema, plain.ema_state_dict, lambda: plain.ema_weights().__enter__()):
        with pytest.raises(ValueError):
            call()
    opt = FusedAdam(model, lr=1e-3, ema_decay=0.99, ema_warmup=True)
    assert (opt.ema_decay, opt.ema_warmup) == (0.99, True)
    assert opt.ema.dtype == torch.float32 and opt.ema.shape == flat.shape and opt.ema.data_ptr() != flat.data_ptr()
    assert torch.equal(opt.ema, flat.detach())          # a copy of the parameters at construction
    given = torch.full_like(flat.detach(), 0.25)
    assert FusedAdam(model, lr=1e-3, ema_decay=0.5, ema=given).ema is given
    # while pieces of a step are outstanding the weights cannot be exchanged
    opt._done_lo = 64
    with pytest.raises(RuntimeError, match="pieces"):
        opt.ema_weights().__enter__()
    opt._done_lo = None
    # inside ema_weights(): no nesting, no step (the flag is all these checks read)
    opt._ema_in = True
    with pytest.raises(RuntimeError, match="nest"):
        opt.ema_weights().__enter__()
    for call in (opt.step, lambda: opt.update_range(0, 64), opt.state_dict):
        with pytest.raises(RuntimeError):
            call()


def test_state_dict_round_trip_with_and_without_the_shadow():
    model = _cpu_model()
    named = list(model.named_parameters())
    plain = FusedAdam(model, lr=1e-3)
    sd0 = plain.state_dict()
    assert set(sd0) == {"state", "param_groups"}          # with the average off: the dict as it was
    assert all(set(sd0["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} for i in range(len(named)))
    opt = FusedAdam(model, lr=1e-3, ema_decay=0.9)
    gen = torch.Generator().manual_seed(1)
    pad = torch.ones(model._flat_param.numel(), dtype=torch.bool)
    for name, p in named:
        lo, n = model._offset[name], p.numel()
        opt.m[lo:lo + n] = torch.randn(n, generator=gen)
        opt.v[lo:lo + n] = torch.rand(n, generator=gen)
        opt.ema[lo:lo + n] = torch.randn(n, generator=gen)
        pad[lo:lo + n] = False
    opt.t = 7
    sd = opt.state_dict()
    assert set(sd) == set(sd0) and sd["param_groups"][0].keys() == sd0["param_groups"][0].keys()
    for i, (name, p) in enumerate(named):
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq", "ema"} and sd["state"][i]["ema"].shape == p.shape
    # into an optimizer with the average on: the shadow travels (the padding between the parameters is not part of the dict)
    other = FusedAdam(model, lr=1e-3, ema_decay=0.5)
    other.load_state_dict(sd)
    assert other.t == 7 and torch.equal(other.m, opt.m) and torch.equal(other.v, opt.v)
    assert torch.equal(other.ema[~pad], opt.ema[~pad]) and not torch.equal(other.ema, model._flat_param.detach())
    # into one with the average off: the entry is ignored
    plain.load_state_dict(sd)
    assert plain.t == 7 and plain.ema is None and torch.equal(plain.m, opt.m)
    # a dict without the shadow (today's), or with it in some entries only: the shadow starts over from the parameters
    partial = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": sd["param_groups"]}
    del partial["state"][1]["ema"]
    for source in (sd0, partial):
        other.ema.fill_(3.0)
        other.load_state_dict(source)
        assert torch.equal(other.ema, model._flat_param.detach())
    # a shadow of the wrong shape is refused like a moment of the wrong shape
    wrong = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": sd["param_groups"]}
    wrong["state"][0]["ema"] = wrong["state"][0]["ema"].reshape(-1)[:-1]
    with pytest.raises(ValueError, match="ema"):
        other.load_state_dict(wrong)
    # torch.optim.Adam loads the dict too (the extra tensor rides along in its state)
    theirs = torch.optim.Adam(model.parameters())
    theirs.load_state_dict(sd)
    back = FusedAdam(model, lr=1e-3, ema_decay=0.9)
    back.load_state_dict(theirs.state_dict())
    assert back.t == 7 and torch.equal(back.m, opt.m) and torch.equal(back.ema[~pad], opt.ema[~pad])
    # ema_state_dict: the model's keys, parameters from the shadow, buffers from the live model
    esd = opt.ema_state_dict()
    live = model.state_dict()
    assert list(esd) == list(live)
    for name, p in named:
        lo = model._offset[name]
        assert torch.equal(esd[name], opt.ema[lo:lo + p.numel()].view(p.shape)) and not torch.equal(esd[name], live[name])
    for k in set(live) - {n for n, _ in named}:
        assert torch.equal(esd[k], live[k])
    assert engine.check_ema(0.5) == (0.5, False)
