"""LAMB trust ratios, what needs no GPU: engine.TorchLamb in float64 against a numpy restatement of the definition and against
torch.optim.Adam, the ratios the definition sets to 1, trust_clip, the argument checks of cpc_lamb (refused before any launch),
the up-front refusals of ContrastiveEstimationTrainer and FusedAdam, FusedAdam's per-parameter tables on a CPU-flattened model and
the state dict round trip under trust_ratio."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, softplus_score_function
from cpc_audio_amd import engine
from cpc_audio_amd.engine import FusedAdam, TorchLamb

L, F = C.c_longlong, C.c_float
B1, B2, EPS = 0.9, 0.999, 1e-8


# ------------------------------------------------------------------------------------------ the definition, restated in numpy
def _lamb_numpy(p, g, m, v, t, lr, wd, selected, clip):
    """One step of the definition ("LAMB trust ratios") on one parameter, in the dtype of its arguments."""
    m = m + (g - m) * (1 - B1)
    v = B2 * v + (1 - B2) * g * g
    r = (m / (1 - B1 ** t)) / (np.sqrt(v) / math.sqrt(1 - B2 ** t) + EPS)
    u = r + wd * p if selected else r
    w_norm, u_norm = math.sqrt(float((p * p).sum())), math.sqrt(float((u * u).sum()))
    trust = 1.0
    if selected and w_norm > 0 and u_norm > 0 and math.isfinite(w_norm) and math.isfinite(u_norm):
        trust = w_norm / u_norm
    if clip is not None:
        trust = min(trust, clip)
    return p - lr * trust * u, m, v, (w_norm, u_norm, trust)


def _named(shapes, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [(name, torch.nn.Parameter(torch.randn(*shape, generator=gen, dtype=torch.float64) * scale)) for name, shape in shapes]


SHAPES = [("conv.weight", (6, 4, 3)), ("conv.bias", (6,)), ("gru.weight_hh", (12, 4)), ("gru.bias_hh", (12,)), ("head.weight", (5, 7))]


@pytest.mark.parametrize("clip", [None, 1.1])
def test_torch_lamb_is_the_definition(clip):
    """Three steps in float64, matrices selected and biases not: parameters, moments and (w_norm, u_norm, ratio) to 1e-12."""
    lr, wd = 2e-2, 0.3
    named = _named(SHAPES, 1)
    opt = TorchLamb(named, lr=lr, weight_decay=wd, trust_clip=clip)
    ref = {n: (p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for n, p in named}
    gen = torch.Generator().manual_seed(2)
    seen = set()
    for t in range(1, 4):
        for n, p in named:
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64) * (10.0 if "gru" in n else 0.1)
        opt.step()
        for n, p in named:
            q, m, v, trust = _lamb_numpy(ref[n][0], p.grad.numpy(), ref[n][1], ref[n][2], t, lr, wd, p.dim() >= 2, clip)
            ref[n] = (q, m, v)
            st = opt.state[p]
            assert int(st["step"]) == t
            assert np.abs(p.detach().numpy() - q).max() <= 1e-12, (n, t)
            assert np.abs(st["exp_avg"].numpy() - m).max() <= 1e-12 and np.abs(st["exp_avg_sq"].numpy() - v).max() <= 1e-12, (n, t)
            got = [float(x) for x in opt.last_trust[n]]
            assert all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(got, trust)), (n, t, got, trust)
            assert p.dim() >= 2 or got[2] == 1.0
            seen.add(round(got[2], 6))
    assert len(seen) > 4          # the ratios differ from tensor to tensor and from step to step
    if clip is not None:
        assert max(seen) == clip and min(seen) < clip


def test_ratios_the_definition_sets_to_one_and_the_clip():
    lr = 1e-2
    named = _named([("zero.weight", (4, 4)), ("still.weight", (4, 4)), ("plain.bias", (16,)), ("big.weight", (4, 4)),
                    ("small.weight", (4, 4))], 3)
    by = dict(named)
    with torch.no_grad():
        by["zero.weight"].zero_()
        by["big.weight"].mul_(100.0)
    start = {n: p.detach().clone() for n, p in named}
    opt = TorchLamb(named, lr=lr, weight_decay=0.0, trust_clip=5.0)
    for n, p in named:
        p.grad = torch.zeros_like(p) if n == "still.weight" else torch.ones_like(p)
    opt.step()
    trust = {n: tuple(float(x) for x in opt.last_trust[n]) for n, _ in named}
    assert trust["zero.weight"][0] == 0.0 and trust["zero.weight"][2] == 1.0          # an all-zero parameter
    assert trust["still.weight"][1] == 0.0 and trust["still.weight"][2] == 1.0        # a zero direction
    assert torch.equal(by["still.weight"], start["still.weight"])
    assert trust["plain.bias"][2] == 1.0 and trust["plain.bias"][0] > 0 and trust["plain.bias"][1] > 0          # not selected
    assert trust["big.weight"][0] / trust["big.weight"][1] > 5.0 and trust["big.weight"][2] == 5.0          # the clip binds
    natural = trust["small.weight"][0] / trust["small.weight"][1]
    assert 0.0 < natural < 5.0 and abs(trust["small.weight"][2] - natural) <= 1e-15 and natural != 1.0
    # the first step's direction is sign(g) (to eps): the zero parameter moved by lr, the unselected one too
    assert (by["zero.weight"] + lr).abs().max().item() < 1e-8 and (by["plain.bias"] - start["plain.bias"] + lr).abs().max().item() < 1e-8
    for bad in (0.0, -1.0, float("nan"), float("inf"), "wide", True):
        with pytest.raises(ValueError):
            TorchLamb(_named(SHAPES, 1), lr=lr, trust_clip=bad)
    with pytest.raises(ValueError):
        TorchLamb(_named(SHAPES, 1), lr=lr, weight_decay=-0.1)


def test_without_selection_and_decay_torch_lamb_is_adam():
    lr = 3e-3
    ours, theirs = _named(SHAPES, 5), _named(SHAPES, 5)
    opt = TorchLamb(ours, lr=lr, weight_decay=0.0, decay_filter=lambda n, p: False)
    adam = torch.optim.Adam([p for _, p in theirs], lr=lr, betas=(B1, B2), eps=EPS)
    gen = torch.Generator().manual_seed(6)
    for _ in range(3):
        for (n, p), (_, q) in zip(ours, theirs):
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64)
            q.grad = p.grad.clone()
        opt.step()
        adam.step()
        for (n, p), (_, q) in zip(ours, theirs):
            assert (p - q).abs().max().item() <= 1e-12, n
            assert float(opt.last_trust[n][2]) == 1.0
    # ... and its state is Adam's: the dict loads into torch.optim.Adam and back
    adam.load_state_dict(opt.state_dict())
    assert all(torch.equal(adam.state[q]["exp_avg"], opt.state[p]["exp_avg"]) for (_, p), (_, q) in zip(ours, theirs))
    opt.load_state_dict(adam.state_dict())
    assert int(opt.state[ours[0][1]]["step"]) == 3


def test_a_loaded_adam_state_keeps_the_constructor_hyper_parameters_and_steps():
    """A run resumed with trust_ratio switched on: torch.optim.AdamW (its own lr and weight_decay) steps twice, its state dict goes
    into a TorchLamb built with other hyper-parameters, and the third step is the definition's step 3 on AdamW's moments, with
    TorchLamb's lr, weight_decay and trust_clip — the saved param group replaces none of them.  FusedAdam's state dict loads alike."""
    lr, wd, clip = 2e-2, 0.3, 1.05
    theirs = _named(SHAPES, 8)
    adamw = torch.optim.AdamW([p for _, p in theirs], lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=0.7)
    gen = torch.Generator().manual_seed(9)
    for _ in range(2):
        for _, q in theirs:
            q.grad = torch.randn(q.shape, generator=gen, dtype=torch.float64)
        adamw.step()
    ours = [(n, torch.nn.Parameter(q.detach().clone())) for n, q in theirs]
    opt = TorchLamb(ours, lr=lr, weight_decay=wd, trust_clip=clip)
    opt.load_state_dict(adamw.state_dict())
    group = opt.param_groups[0]
    assert (group["lr"], group["weight_decay"], group["trust_clip"], group["betas"], group["eps"]) == (lr, wd, clip, (B1, B2), EPS)
    clipped = 0
    for (n, p), (_, q) in zip(ours, theirs):
        p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    # (torch's load_state_dict shares tensors that need no cast: the moments are copied out before the step updates them in place)
    before = {n: (p.detach().numpy().copy(), adamw.state[q]["exp_avg"].numpy().copy(), adamw.state[q]["exp_avg_sq"].numpy().copy())
              for (n, p), (_, q) in zip(ours, theirs)}
    opt.step()
    for n, p in ours:
        want, m, v, trust = _lamb_numpy(before[n][0], p.grad.numpy(), before[n][1], before[n][2], 3, lr, wd, p.dim() >= 2, clip)
        assert int(opt.state[p]["step"]) == 3
        assert np.abs(p.detach().numpy() - want).max() <= 1e-12 and np.abs(opt.state[p]["exp_avg"].numpy() - m).max() <= 1e-12, n
        assert abs(float(opt.last_trust[n][2]) - trust[2]) <= 1e-12, n
        clipped += trust[2] == clip
    assert clipped >= 1
    # FusedAdam.state_dict() (torch.optim.Adam's format, one group with its own weight_decay) loads the same way
    model = _cpu_model()
    fused = FusedAdam(model, lr=1e-3, weight_decay=0.05)
    fused.t = 4
    lamb = TorchLamb(model.named_parameters(), lr=lr, weight_decay=wd, trust_clip=clip)
    lamb.load_state_dict(fused.state_dict())
    assert (lamb.param_groups[0]["weight_decay"], lamb.param_groups[0]["trust_clip"], lamb.param_groups[0]["lr"]) == (wd, clip, lr)
    for _, p in model.named_parameters():
        p.grad = torch.ones_like(p)
    lamb.step()
    assert all(int(lamb.state[p]["step"]) == 5 for _, p in model.named_parameters())


# ------------------------------------------------------------------------------------------ the entry point's argument checks
def test_lamb_arguments_are_checked_before_any_launch():
    """Every refusal include/cpc_hip.h states for cpc_lamb returns CPC_EINVAL (-22) from the argument check: no kernel is launched,
    so this runs without a GPU.  The parameter table is the one argument the check reads: a real host array."""
    lib = _hip.lib()
    for name in ("cpc_lamb", "cpc_lamb_workspace_floats"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert lib.cpc_lamb_workspace_floats(L(10)) == 20 and lib.cpc_lamb_workspace_floats(L(0)) == 0
    P = C.c_void_p(0x1000)        # 16-byte aligned, never dereferenced
    s = C.c_void_p(0)
    hyper = (F(1e-3), F(0.9), F(0.999), F(1e-8))
    table = (C.c_int * 5)(0, 1, 3, 4, 9)          # four parameters of 1, 2, 1 and 5 blocks
    T = C.cast(table, C.c_void_p)

    def lamb(p=P, g=P, m=P, v=P, n=192, step=1, wd=0.1, bits=P, first_block=1, coef=None, host=T, dev=P, inverse=P, first=1, count=2,
             total=4, clip=-1.0, ws=P, trust=P):
        return lib.cpc_lamb(p, g, m, v, L(n), *hyper, step, F(1.0), F(wd), bits, L(first_block), coef, host, dev, inverse, first, count,
                            total, F(clip), ws, trust, None, s)

    # cpc_adamw's cases
    assert lamb(n=0) == -22 and lamb(n=-64) == -22
    assert lamb(step=0) == -22 and lamb(step=-3) == -22
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert lamb(wd=bad) == -22, bad
    assert lamb(first_block=-1) == -22
    for hole in ("p", "g", "m", "v"):
        assert lamb(**{hole: None}) == -22, hole
    # the bitmap selects the ratios: required also without decay
    assert lamb(bits=None) == -22 and lamb(bits=None, wd=0.0) == -22
    # a NULL table, workspace or trust array
    for hole in ("host", "dev", "inverse", "ws", "trust"):
        assert lamb(**{hole: None}) == -22, hole
    # the parameters of the range
    assert lamb(count=0) == -22 and lamb(count=-1) == -22 and lamb(first=-1) == -22
    assert lamb(first=3, count=2) == -22 and lamb(total=2) == -22 and lamb(total=0) == -22
    # a range whose n differs from the blocks the table gives it, or that does not start where the table says
    assert lamb(n=128) == -22 and lamb(n=256) == -22 and lamb(n=191) == -22
    assert lamb(first_block=0) == -22 and lamb(first=0, first_block=0, count=2, n=256) == -22
    descending = (C.c_int * 5)(0, 3, 1, 4, 9)
    assert lamb(host=C.cast(descending, C.c_void_p), first=0, first_block=0, count=3, n=256) == -22
    # the block sums travel in 8-byte pairs
    assert lamb(ws=C.c_void_p(0x1004)) == -22
    # trust_clip: negative means none; given, it has to be finite and > 0
    for bad in (0.0, float("nan"), float("inf")):
        assert lamb(clip=bad) == -22, bad


# ------------------------------------------------------------------------------------------ the refusals of trainer and optimizer
def test_trainer_refuses_up_front():
    """Before any GPU work (there is no model, dataset or device here to get as far as one)."""
    tr = ContrastiveEstimationTrainer(model=None, dataset=None)
    assert tr.trust_ratio is False and tr.trust_clip is None
    for bad in (1, 0, "yes", None, 1.0):
        tr.trust_ratio = bad
        with pytest.raises(ValueError):
            tr.train(batch_size=4, max_steps=1)
    tr.trust_ratio = True
    for bad in (0, 0.0, -2.0, float("nan"), float("inf"), "wide", True):
        tr.trust_clip = bad
        with pytest.raises(ValueError):
            tr.train(batch_size=4, max_steps=1)
    tr.trust_ratio = False          # the clip is checked also while the ratio is off
    with pytest.raises(ValueError):
        tr.train(batch_size=4, max_steps=1)
    tr.trust_ratio, tr.trust_clip, tr.use_graph = True, 10.0, True
    with pytest.raises(NotImplementedError):
        tr.train(batch_size=4, max_steps=1)
    for score in (softplus_score_function, lambda p, t: softplus_score_function(p, t)):
        foreign = ContrastiveEstimationTrainer(model=None, dataset=None, optimizer=torch.optim.SGD, score_function=score)
        foreign.trust_ratio = True
        with pytest.raises(NotImplementedError):
            foreign.train(batch_size=4, max_steps=1)


def _cpu_model(seed=0):
    torch.manual_seed(seed)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=16), enc_size=8, ar_size=16, visible_steps=6,
                                       prediction_steps=3, compute_dtype="fp32")
    model._flatten_parameters("cpu")
    return model


def test_fused_adam_refusals_and_tables(monkeypatch):
    model = _cpu_model()

    def no_launch(name, *a, **kw):
        raise AssertionError(f"FusedAdam's constructor launched {name}")

    monkeypatch.setattr(_hip, "call", no_launch)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            FusedAdam(model, lr=1e-3, trust_ratio=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError):
            FusedAdam(model, lr=1e-3, trust_ratio=True, trust_clip=bad)
    with pytest.raises(NotImplementedError):
        FusedAdam(model, lr=1e-3, trust_ratio=True, device_step=True)
    plain = FusedAdam(model, lr=1e-3)
    assert plain.trust_ratio is False and plain.decay_bits is None          # nothing new without the keyword
    assert not any(hasattr(plain, a) for a in ("trust", "_param_block", "_param_block_dev", "_block_param", "_lamb_ws"))
    with pytest.raises(ValueError):
        plain.trust_ratios()
    opt = FusedAdam(model, lr=1e-3, trust_ratio=True, trust_clip=10)          # weight_decay 0: the bitmap is built all the same
    assert opt.trust_clip == 10.0 and opt.decay_bits is not None
    assert opt.decay_bits.tolist() == FusedAdam(model, lr=1e-3, weight_decay=0.1).decay_bits.tolist()
    named = list(model.named_parameters())
    table = list(opt._param_block)
    total = model._flat_param.numel()
    assert len(table) == len(named) + 1 and table[0] == 0 and table[-1] * 64 == total and table == sorted(table)
    assert opt._param_block_dev.tolist() == table and opt._param_block_dev.dtype == torch.int32
    inverse = opt._block_param.tolist()
    assert len(inverse) == total // 64 and opt._block_param.dtype == torch.int32
    for q, (name, p) in enumerate(named):
        assert opt._lamb_names[q] == name and table[q] * 64 == model._offset[name]
        assert table[q + 1] - table[q] == (p.numel() + 63) // 64
        assert inverse[table[q]:table[q + 1]] == [q] * (table[q + 1] - table[q])
    assert opt._lamb_ws.numel() == 2 * (total // 64) and tuple(opt.trust.shape) == (3, len(named))
    assert set(opt.trust_ratios()) == {n for n, _ in named}
    with pytest.raises(AssertionError, match="whole parameters"):          # a range that ends inside a parameter: refused before the call
        opt._update(0, 32, 1, 1.0)


def test_state_dict_round_trip_under_trust_ratio():
    """LAMB's state is Adam's: state_dict() of a trust-ratio optimizer loads into a plain FusedAdam, into torch.optim.Adam and back,
    bit for bit, with the step count."""
    model = _cpu_model()
    opt = FusedAdam(model, lr=1e-3, weight_decay=0.05, trust_ratio=True, trust_clip=4.0)
    gen = torch.Generator().manual_seed(1)
    pad = torch.ones(model._flat_param.numel(), dtype=torch.bool)
    for name, p in model.named_parameters():
        lo, n = model._offset[name], p.numel()
        opt.m[lo:lo + n] = torch.randn(n, generator=gen)
        opt.v[lo:lo + n] = torch.rand(n, generator=gen)
        pad[lo:lo + n] = False
    opt.t = 7
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["param_groups"][0]["weight_decay"] == 0.05
    for other in (FusedAdam(model, lr=1e-3, trust_ratio=True), FusedAdam(model, lr=1e-3)):
        other.load_state_dict(sd)
        assert other.t == 7 and torch.equal(other.m, opt.m) and torch.equal(other.v, opt.v) and not other.m[pad].any()
    theirs = torch.optim.Adam(model.parameters())
    theirs.load_state_dict(sd)
    back = FusedAdam(model, lr=1e-3, trust_ratio=True)
    back.load_state_dict(theirs.state_dict())
    assert back.t == 7 and torch.equal(back.m, opt.m) and torch.equal(back.v, opt.v)
    assert engine.check_trust(True, 2) == (True, 2.0) and engine.check_trust(False) == (False, None)
