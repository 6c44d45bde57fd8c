"""AdamW weight decay and the learning-rate schedule, what needs no GPU: LRSchedule.factor against torch's LambdaLR, the up-front
refusals of ContrastiveEstimationTrainer, FusedAdam's decay bitmap on a CPU-flattened model, the state dict round trips with
torch.optim.AdamW, and the argument checks of cpc_adamw / cpc_adamw_dev / cpc_lr_factors (refused before any launch)."""
import ctypes as C

import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, LRSchedule
from cpc_audio_amd import engine
from cpc_audio_amd.engine import FusedAdam

L, F = C.c_longlong, C.c_float
KINDS = ("constant", "linear", "cosine")


# ------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("warmup", [0, 1, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_factor_is_lambda_lr(kind, warmup):
    """Step s of torch.optim.AdamW under LambdaLR(opt, factor), scheduler.step() behind every optimizer.step(), runs at
    lr * factor(s): equal to 1e-15 for steps 0 ... T + 3."""
    T, lr, r = 9, 1e-3, 0.1
    sched = LRSchedule(kind, warmup_steps=warmup, total_steps=T, min_lr_ratio=r)
    p = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.AdamW([p], lr=lr)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sched.factor)
    for s in range(T + 4):
        assert abs(opt.param_groups[0]["lr"] - lr * sched.factor(s)) <= 1e-15, (kind, warmup, s)
        p.grad = torch.ones(3)
        opt.step()
        lam.step()
    if warmup:
        assert sched.factor(0) == 1.0 / warmup and sched.factor(0) > 0.0          # the first warm-up step is 1 / W, never 0
        assert sched.factor(warmup - 1) == 1.0
    for s in (T, T + 1, T + 1000, 10 ** 9):
        assert sched.factor(s) == (1.0 if kind == "constant" else r), (kind, s)
    if kind != "constant":
        assert sched.factor(warmup) == 1.0
        decay = [sched.factor(s) for s in range(warmup, T + 1)]
        assert all(a > b for a, b in zip(decay, decay[1:]))


def test_constant_schedule_needs_no_total():
    sched = LRSchedule("constant", warmup_steps=4)
    assert [sched.factor(s) for s in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    assert LRSchedule("constant").factor(0) == 1.0


@pytest.mark.parametrize("args,kw", [
    (("exponential",), {}), ((None,), {}),
    (("linear",), {}), (("cosine",), {"warmup_steps": 2}),                                  # total_steps is required
    (("linear",), {"warmup_steps": 5, "total_steps": 5}), (("cosine",), {"warmup_steps": 5, "total_steps": 3}),
    (("constant",), {"warmup_steps": 3, "total_steps": 3}),
    (("linear",), {"warmup_steps": -1, "total_steps": 5}), (("linear",), {"warmup_steps": 1.5, "total_steps": 5}),
    (("linear",), {"total_steps": 5.0}), (("linear",), {"total_steps": 0}),
    (("linear",), {"total_steps": 5, "min_lr_ratio": -0.1}), (("linear",), {"total_steps": 5, "min_lr_ratio": 1.5}),
    (("linear",), {"total_steps": 5, "min_lr_ratio": float("nan")}), (("linear",), {"total_steps": 5, "min_lr_ratio": "low"}),
])
def test_invalid_schedules_are_refused(args, kw):
    with pytest.raises(ValueError):
        LRSchedule(*args, **kw)


# ------------------------------------------------------------------------------------------ the trainer's refusals
def test_trainer_refuses_up_front():
    """Before any GPU work (there is no model, dataset or device here to get as far as one)."""
    tr = ContrastiveEstimationTrainer(model=None, dataset=None)
    assert tr.weight_decay == 0.0 and tr.weight_decay_filter is None and tr.lr_schedule is None
    assert tr.optimizer_state is None and tr.last_lr is None
    for bad in (-1, -1e-9, float("nan"), float("inf"), float("-inf"), "some"):
        tr.weight_decay = bad
        with pytest.raises(ValueError):
            tr.train(batch_size=4, max_steps=1)
    tr.weight_decay, tr.weight_decay_filter = 0.1, "biases"
    with pytest.raises(ValueError):
        tr.train(batch_size=4, max_steps=1)
    tr.weight_decay_filter, tr.lr_schedule = None, "cosine"
    with pytest.raises(ValueError):
        tr.train(batch_size=4, max_steps=1)
    tr.lr_schedule, tr.optimizer_state = None, [1, 2]
    with pytest.raises(ValueError):
        tr.train(batch_size=4, max_steps=1)


# ------------------------------------------------------------------------------------------ FusedAdam on a CPU-flattened model
def _cpu_model(seed=0):
    torch.manual_seed(seed)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=16), enc_size=8, ar_size=16, visible_steps=6,
                                       prediction_steps=3, compute_dtype="fp32")
    model._flatten_parameters("cpu")
    return model


def _bits(opt):
    """The bitmap as a list of booleans, one per 64-float block."""
    words = [w & 0xFFFFFFFF for w in opt.decay_bits.tolist()]
    blocks = opt.model._flat_param.numel() // 64
    return [bool(words[j // 32] >> (j % 32) & 1) for j in range(blocks)], words


def _expected_blocks(model, chosen):
    blocks = [False] * (model._flat_param.numel() // 64)
    for name, p in model.named_parameters():
        lo = model._offset[name]
        assert lo % 64 == 0
        for j in range(lo // 64, (lo + p.numel() + 63) // 64):          # the parameter's padding follows its bit
            blocks[j] = chosen(name, p)
    return blocks


def test_decay_bitmap(monkeypatch):
    model = _cpu_model()

    def no_launch(name, *a, **kw):
        raise AssertionError(f"FusedAdam's constructor launched {name}")

    monkeypatch.setattr(_hip, "call", no_launch)
    plain = FusedAdam(model, lr=1e-3)
    assert plain.decay_bits is None and plain.weight_decay == 0.0 and plain.schedule is None          # nothing new without the keywords
    assert FusedAdam(model, lr=1e-3, schedule=LRSchedule("constant", 3)).decay_bits is None
    opt = FusedAdam(model, lr=1e-3, weight_decay=0.1)
    bits, words = _bits(opt)
    nblocks = model._flat_param.numel() // 64
    assert opt.decay_bits.dtype == torch.int32 and len(words) == -(-nblocks // 32) and nblocks > 32
    want = _expected_blocks(model, lambda n, p: p.dim() >= 2)
    assert bits == want and any(want) and not all(want)
    assert words[-1] >> (nblocks % 32 or 32) == 0                                                        # no bit past the buffer
    dims = {n: p.dim() for n, p in model.named_parameters()}
    assert any(n.endswith("bias") and d == 1 for n, d in dims.items())
    # a custom filter's choice: the biases alone
    custom = FusedAdam(model, lr=1e-3, weight_decay=0.1, decay_filter=lambda n, p: n.endswith("bias"))
    assert _bits(custom)[0] == _expected_blocks(model, lambda n, p: n.endswith("bias"))
    assert _bits(custom)[0] != bits
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            FusedAdam(model, lr=1e-3, weight_decay=bad)
    with pytest.raises(ValueError):
        FusedAdam(model, lr=1e-3, weight_decay=0.1, decay_filter=3)
    with pytest.raises(ValueError):
        FusedAdam(model, lr=1e-3, schedule="cosine")
    with pytest.raises(ValueError):
        FusedAdam(model, lr=1e-3, step_offset=-1)


def test_scheduled_lr_follows_step_offset_and_loaded_count():
    model = _cpu_model()
    sched = LRSchedule("linear", warmup_steps=2, total_steps=8, min_lr_ratio=0.25)
    opt = FusedAdam(model, lr=2e-3, schedule=sched, step_offset=3)
    opt._scheduled_lr(opt.t)
    assert opt.lr == 2e-3 * sched.factor(3)
    sd = opt.state_dict()
    for entry in sd["state"].values():
        entry["step"] = torch.tensor(3.0)
    opt.load_state_dict(sd)          # a resumed run: three steps are counted, the schedule still goes on from step_offset
    assert opt.t == 3
    opt._scheduled_lr(opt.t)
    assert opt.lr == 2e-3 * sched.factor(3)
    opt._scheduled_lr(opt.t + 1)
    assert opt.lr == 2e-3 * sched.factor(4)


# ------------------------------------------------------------------------------------------ state dicts
def _fill(opt, t, seed=1):
    gen = torch.Generator().manual_seed(seed)
    for name, p in opt.model.named_parameters():
        lo, n = opt.model._offset[name], p.numel()
        opt.m[lo:lo + n] = torch.randn(n, generator=gen)
        opt.v[lo:lo + n] = torch.rand(n, generator=gen)
    opt.t = t


def _padding_mask(model):
    pad = torch.ones(model._flat_param.numel(), dtype=torch.bool)
    for name, p in model.named_parameters():
        pad[model._offset[name]:model._offset[name] + p.numel()] = False
    return pad


def test_state_dict_round_trips_with_torch_adamw():
    model = _cpu_model()
    opt = FusedAdam(model, lr=1e-3, weight_decay=0.05)
    _fill(opt, 7)
    sd = opt.state_dict()
    params = list(model.parameters())
    assert sorted(sd["state"]) == list(range(len(params))) and len(sd["param_groups"]) == 1
    group = sd["param_groups"][0]
    assert group["params"] == list(range(len(params))) and group["amsgrad"] is False
    assert (group["lr"], group["betas"], group["eps"], group["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 0.05)
    # FusedAdam -> torch.optim.AdamW
    theirs = torch.optim.AdamW(model.parameters())
    theirs.load_state_dict(sd)
    for i, (name, p) in enumerate(model.named_parameters()):
        lo, n = model._offset[name], p.numel()
        st = theirs.state[p]
        assert float(st["step"]) == 7.0
        assert torch.equal(st["exp_avg"], opt.m[lo:lo + n].view(p.shape)) and torch.equal(st["exp_avg_sq"], opt.v[lo:lo + n].view(p.shape))
    assert theirs.param_groups[0]["weight_decay"] == 0.05 and theirs.param_groups[0]["lr"] == 1e-3
    for p in params:
        p.grad = torch.zeros_like(p)
    theirs.step()                                                    # the loaded optimizer is usable
    assert float(theirs.state[params[0]]["step"]) == 8.0
    # torch.optim.AdamW -> FusedAdam: into a fresh optimizer whose buffers hold something else
    back = FusedAdam(model, lr=1e-3)
    _fill(back, 2, seed=9)
    back.m[_padding_mask(model)] = 0.0
    back.v[_padding_mask(model)] = 0.0
    their_sd = theirs.state_dict()
    back.load_state_dict(their_sd)
    assert back.t == 8
    for i, (name, p) in enumerate(model.named_parameters()):
        lo, n = model._offset[name], p.numel()
        assert torch.equal(back.m[lo:lo + n].view(p.shape), their_sd["state"][i]["exp_avg"]), name
        assert torch.equal(back.v[lo:lo + n].view(p.shape), their_sd["state"][i]["exp_avg_sq"]), name
    pad = _padding_mask(model)
    assert pad.any() and not back.m[pad].any() and not back.v[pad].any()          # the alignment padding stays zero
    # its own round trip is exact
    again = FusedAdam(model, lr=1e-3)
    again.load_state_dict(opt.state_dict())
    assert again.t == 7 and torch.equal(again.m, opt.m * ~pad) and torch.equal(again.v, opt.v * ~pad)
    # an optimizer that has not stepped: torch writes an empty state
    fresh = FusedAdam(model, lr=1e-3)
    _fill(fresh, 4)
    fresh.load_state_dict(torch.optim.AdamW(model.parameters()).state_dict())
    assert fresh.t == 0 and not fresh.m.any() and not fresh.v.any()


def test_state_dicts_that_do_not_fit_are_refused():
    model = _cpu_model()
    opt = FusedAdam(model, lr=1e-3)
    _fill(opt, 3)
    before = (opt.m.clone(), opt.v.clone(), opt.t)
    sd = opt.state_dict()
    sd["state"][1]["step"] = torch.tensor(4.0)                       # per-parameter counts that differ
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
    sd = opt.state_dict()
    sd["state"][0]["exp_avg"] = sd["state"][0]["exp_avg"].reshape(-1)[:-1]
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
    sd = opt.state_dict()
    sd["state"][2]["exp_avg_sq"] = sd["state"][2]["exp_avg_sq"].unsqueeze(0)
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
    sd = opt.state_dict()
    del sd["state"][len(sd["state"]) - 1]                            # a parameter without an entry
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
    assert torch.equal(opt.m, before[0]) and torch.equal(opt.v, before[1]) and opt.t == before[2]          # refused: nothing was loaded


# ------------------------------------------------------------------------------------------ the entry points' argument checks
def test_adamw_arguments_are_checked_before_any_launch():
    """Every refusal include/cpc_hip.h states for cpc_adamw, cpc_adamw_dev and cpc_lr_factors returns CPC_EINVAL (-22) from the
    argument check: no kernel is launched, so this runs without a GPU."""
    lib = _hip.lib()
    for name in ("cpc_adamw", "cpc_adamw_dev", "cpc_lr_factors"):
        assert name in _hip.EXPORTED_SYMBOLS
    P = C.c_void_p(0x1000)        # 16-byte aligned, never dereferenced
    s = C.c_void_p(0)
    hyper = (F(1e-3), F(0.9), F(0.999), F(1e-8))

    def adamw(p=P, g=P, m=P, v=P, n=64, step=1, wd=0.1, bits=P, first=0, coef=None):
        return lib.cpc_adamw(p, g, m, v, L(n), *hyper, step, F(1.0), F(wd), bits, L(first), coef, None, s)

    assert adamw(n=0) == -22 and adamw(n=-64) == -22
    assert adamw(step=0) == -22 and adamw(step=-3) == -22
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert adamw(wd=bad) == -22, bad
        assert adamw(wd=bad, bits=None) == -22, bad
    assert adamw(wd=0.1, bits=None) == -22                            # a decay without a bitmap
    assert adamw(first=-1) == -22
    for hole in ("p", "g", "m", "v"):
        assert adamw(**{hole: None}) == -22, hole

    def dev(p=P, g=P, m=P, v=P, n=64, state=P, wd=0.1, bits=P, kind=2, warm=2, total=10, ratio=0.1, offset=0, coef=None):
        return lib.cpc_adamw_dev(p, g, m, v, L(n), *hyper, state, F(1.0), F(wd), bits, kind, L(warm), L(total), F(ratio), L(offset),
                                 coef, None, s)

    assert dev(n=0) == -22 and dev(state=None) == -22
    assert dev(coef=P) == -22                                         # clipped steps are not captured
    for bad in (-1.0, float("nan"), float("inf")):
        assert dev(wd=bad) == -22, bad
    assert dev(bits=None) == -22 and dev(offset=-1) == -22
    for hole in ("p", "g", "m", "v"):
        assert dev(**{hole: None}) == -22, hole
    assert dev(kind=3) == -22 and dev(kind=-1) == -22 and dev(warm=-1) == -22
    assert dev(warm=10, total=10) == -22 and dev(kind=1, warm=4, total=2) == -22
    assert dev(ratio=-0.5) == -22 and dev(ratio=1.5) == -22 and dev(ratio=float("nan")) == -22

    def factors(kind=2, warm=2, total=10, ratio=0.1, step0=0, count=4, out=P):
        return lib.cpc_lr_factors(kind, L(warm), L(total), F(ratio), L(step0), count, out, s)

    assert factors(kind=3) == -22 and factors(kind=-1) == -22
    assert factors(warm=-1) == -22 and factors(warm=10) == -22 and factors(kind=1, total=0) == -22
    assert factors(ratio=-0.1) == -22 and factors(ratio=1.01) == -22 and factors(ratio=float("nan")) == -22
    assert factors(step0=-1) == -22 and factors(count=0) == -22 and factors(count=-2) == -22 and factors(out=None) == -22


def test_abi_arguments_of_a_schedule():
    kind, warm, total, ratio = LRSchedule("cosine", 2, 10, 0.5).abi_args()
    assert (kind, warm.value, total.value, ratio.value) == (2, 2, 10, 0.5)
    kind, warm, total, ratio = LRSchedule("constant", 4).abi_args()          # no total: any value above the warm-up
    assert kind == 0 and warm.value == 4 and total.value > 4
    assert engine.default_decay_filter("w", torch.zeros(2, 2)) and not engine.default_decay_filter("b", torch.zeros(4))
    assert engine.check_weight_decay(1) == 1.0 and isinstance(engine.check_weight_decay(1), float)
