"""EMA of the weights on the HIP path: cpc_ema against a float64 restatement of the definition at a bound counted from the kernel's
arithmetic (host and device route, decay 0, a raised skip flag, pieces, the grid-stride wrap), cpc_ema_swap; FusedAdam(ema_decay=...)
on every update route with the average on against off, bit for bit; and ContrastiveEstimationTrainer (NaN guard, validate(use_ema),
the shadow across train() calls, a resumed run, use_graph, the generic route).  Fixtures and the fused step by hand are those of
tests/test_adamw_gpu.py."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import test_adamw_gpu as A
from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import TensorAudioDataset
from cpc_audio_amd.engine import FusedAdam, ema_weight

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
L, F = C.c_longlong, C.c_float
E24 = 2.0 ** -24          # half a unit in the last place of a float32 result: one rounding, relative

# The capped grid of cpc_ema / cpc_ema_swap (csrc/pointwise.hip, ema_blocks: adam_stream's shape): at most 2048 workgroups of 256 threads,
# one float4 per thread and round.  One float4 more than that and the grid-stride loop wraps; + 5 floats: one more body and a tail of one.
GRID_REACH = 2048 * 256 * 4
SIZES = [1, 3, 4, 5, 64, 65, 2048 + 7, GRID_REACH + 5]


def _f32(x):
    return float(np.float32(x))


def _host_w(decay, warmup, t):
    """The weight cpc_ema's host route hands its kernel: 1 - d in double on the float32 decay it received, rounded once."""
    return _f32(ema_weight(_f32(decay), warmup, t))


def _bound(p, e):
    """ema + (p - ema) * w from float32 inputs: one rounding each for the subtraction, the product and the sum, each at most 2^-24 of
    a quantity below |p| + |ema| (0 <= w <= 1); the kernel's fma only removes one of them."""
    return 3 * E24 * (p.double().abs() + e.double().abs())


def _ema64(p, e, w):
    return e.double() + (p.double() - e.double()) * w


def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    e = p + torch.randn(n, generator=gen) * 0.05          # a shadow near the parameters, as in a run
    e[::7] = torch.randn(e[::7].numel(), generator=gen) * 30.0          # ... and far from them
    return p, e


def _ema(p, e, n, decay, warmup=0, step=1, state=None, skip=None, lo=0):
    _hip.call("cpc_ema", _hip.ptr(p, lo), _hip.ptr(e, lo), L(n), F(decay), warmup, step, _hip.ptr(state), _hip.ptr(skip))


# ------------------------------------------------------------------------------------------ 1. the kernel against float64
@pytest.mark.parametrize("n", SIZES)
def test_ema_against_float64(n):
    """Three host-route calls (the decay alone, then under warmup at t = 2 with the warmup and with the decay binding) from the step's own float32 inputs and the float-rounded 1 - d:
    every element within 3 * 2^-24 (|p| + |ema|); p and both guard tails untouched."""
    p0, e0 = _inputs(n, n)
    (p, pw), (e, ew) = A._guarded_copy(p0), A._guarded_copy(e0)
    worst = 0.0
    for decay, warmup, t in ((0.999, 0, 1), (0.999, 1, 2), (0.2, 1, 2)):
        before = e.clone()
        _ema(p, e, n, decay, warmup, t)
        torch.cuda.synchronize()
        w = _host_w(decay, warmup, t)
        assert w == _f32(1 - min(_f32(decay), 3 / 12) if warmup else 1 - _f32(decay))
        err = (e.double() - _ema64(p, before, w)).abs()
        bound = _bound(p, before)
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert bool((err <= bound).all()), (decay, warmup, (err / bound.clamp_min(1e-300)).max().item())
        assert not torch.equal(e, before)
    print(f"cpc_ema n {n}: worst error / bound {worst:.3f}")
    assert torch.equal(p.cpu(), p0) and A._intact(pw, ew)


@pytest.mark.parametrize("n", SIZES)
def test_decay_zero_skip_and_swap(n):
    """Decay 0: ema == p bit for bit (also where |ema| >> |p|).  A raised skip flag: nothing changes.  cpc_ema_swap: one call
    exchanges the bits, a second restores both buffers; guard tails untouched throughout."""
    p0, e0 = _inputs(n, 100 + n)
    p0[::5] *= 1e-6
    (p, pw), (e, ew) = A._guarded_copy(p0), A._guarded_copy(e0)
    flag = torch.ones(1, device=DEV)
    _ema(p, e, n, 0.5, skip=flag)
    _ema(p, e, n, 0.0, 1, 3, skip=flag)
    torch.cuda.synchronize()
    assert torch.equal(e.cpu(), e0) and torch.equal(p.cpu(), p0)
    _hip.call("cpc_ema_swap", _hip.ptr(p), _hip.ptr(e), L(n))
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), e0) and torch.equal(e.cpu(), p0) and A._intact(pw, ew)
    _hip.call("cpc_ema_swap", _hip.ptr(p), _hip.ptr(e), L(n))
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and torch.equal(e.cpu(), e0) and A._intact(pw, ew)
    flag.zero_()          # a lowered flag lets the update through
    _ema(p, e, n, 0.0, skip=flag)
    torch.cuda.synchronize()
    assert torch.equal(e.cpu(), p0) and torch.equal(p.cpu(), p0) and A._intact(pw, ew)


@pytest.mark.parametrize("n", [65, 2048 + 7])
def test_pieces_at_float4_cuts_give_the_whole_call_bits(n):
    p0, e0 = _inputs(n, 200 + n)
    (p, pw), (whole, ww), (parts, sw) = A._guarded_copy(p0), A._guarded_copy(e0), A._guarded_copy(e0)
    _ema(p, whole, n, 0.9, 1, 4)
    cuts = [0, 4 * (n // 12), 4 * (n // 6) + 8, n]
    assert all(c % 4 == 0 for c in cuts[:-1]) and sorted(set(cuts)) == cuts
    for lo, hi in reversed(list(zip(cuts, cuts[1:]))):          # from the tail, as the backward pass issues its pieces
        _ema(p, parts, hi - lo, 0.9, 1, 4, lo=lo)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts) and not torch.equal(whole.cpu(), e0) and A._intact(pw, ww, sw)


@pytest.mark.parametrize("warmup", [0, 1])
def test_device_route_reads_the_step_count_cpc_adam_dev_keeps(warmup):
    """Three cpc_adam_dev steps from a zeroed state, each followed by cpc_ema with that state: the count in state[0] is t, and the
    shadow follows the float64 recurrence on the parameters read back, within the host route's bound widened by one unit in the last
    place of w = 1 - d times |p - ema| (the device divides in float where the host divides in double and rounds).  A step under a
    raised skip flag moves neither the count nor the shadow."""
    n, decay = 2048 + 7, 0.9
    gen = torch.Generator().manual_seed(7)
    p0, e0 = _inputs(n, 300 + warmup)
    (p, pw), (e, ew), (m, mw), (v, vw), (state, sw) = A._guarded_copy(p0), A._guarded_copy(e0), A._guarded(n), A._guarded(n), A._guarded(4)
    skip = torch.zeros(1, device=DEV)

    def step(g):
        _hip.call("cpc_adam_dev", _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), L(n), F(1e-2), F(A.B1), F(A.B2), F(A.EPS),
                  _hip.ptr(state), F(1.0), _hip.ptr(skip))
        _ema(p, e, n, decay, warmup, 0, state=state, skip=skip)          # the step argument is ignored on this route

    for t in range(1, 4):
        before = e.clone()
        g = torch.randn(n, generator=gen).to(DEV)
        step(g)
        torch.cuda.synchronize()
        assert int(state.cpu()[:1].view(torch.int32)) == t
        w = ema_weight(_f32(decay), bool(warmup), t)          # exact: the device's float is within one unit in the last place of it
        ulp = float(np.spacing(np.float32(w)))
        err = (e.double() - _ema64(p, before, w)).abs()
        bound = _bound(p, before) + ulp * (p.double() - before.double()).abs()
        print(f"device route warmup {warmup} t {t}: w {w:.6f}, worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), t
        assert warmup == 0 or w > 1 - _f32(decay)          # the warmup binds at these steps
    after = (p.clone(), e.clone(), state.clone())
    skip.fill_(1.0)
    step(g)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(after, (p, e, state))) and A._intact(pw, ew, mw, vw, sw)


# ------------------------------------------------------------------------------------------ 2. FusedAdam
DECAY = 0.5          # far from 1: three steps move the shadow visibly


def _one_step_at_a_time(model, data, batches, steps, **adam):
    """A._engine_steps one step per call: yields (optimizer, loss, shadow before the step or None) after every step."""
    opt = None
    for i in range(steps):
        before = None if opt is None or opt.ema is None else opt.ema.clone()
        kw = dict(optimizer=opt) if opt is not None else adam
        opt, losses, _ = A._engine_steps(model, data, batches[i:] + batches[:i], 1, **kw)
        yield opt, losses[0], before


@pytest.mark.parametrize("context", ["gru", "conv", "attention"])
def test_engine_shadow_follows_the_float64_recurrence(golden_dir, context):
    """FusedAdam(ema_decay, ema_warmup) under the gradient-ready hooks: after every step the shadow is ema + (p - ema) * w of the
    previous shadow and the parameters read back, within the per-step bound, on every element exactly once (the hook pieces and the head)."""
    meta, data, state, build, _ = A._fixture(golden_dir, context)
    model = build("fp32")
    model._flatten_parameters(DEV)
    start = model._flat_param.detach().clone()
    steps = min(3, data.shape[0] // meta["B"])
    with A._Spy() as spy:
        for t, (opt, loss, before) in enumerate(_one_step_at_a_time(model, data, A._batches(data, meta["B"]), steps, ema_decay=DECAY,
                                                                    ema_warmup=True), 1):
            before = start if before is None else before          # the shadow starts as a copy of the parameters
            p = model._flat_param.detach()
            w = _host_w(DECAY, True, t)
            err = (opt.ema.double() - _ema64(p, before, w)).abs()
            bound = _bound(p, before)
            print(f"{context} step {t}: w {w:.6f}, worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert bool((err <= bound).all()), (context, t)
            assert opt.t == t and not torch.equal(opt.ema, before)
    assert spy.names.count("cpc_ema") == spy.names.count("cpc_adam") > steps          # one behind every update: pieces and the head


ROUTES = {
    "adam with hooks": ("fp32", {}),
    "adamw with a schedule": ("fp32", dict(weight_decay=A.WD, schedule=A.SCHED)),
    "max_grad_norm": ("fp32", dict(max_grad_norm=0.05)),
    "trust_ratio": ("fp32", dict(weight_decay=0.1, trust_ratio=True)),
    "bf16": ("bf16", {}),
}
UPDATES = {"adam with hooks": "cpc_adam", "adamw with a schedule": "cpc_adamw", "max_grad_norm": "cpc_adam_clip", "trust_ratio": "cpc_lamb",
           "bf16": "cpc_adam"}


@pytest.mark.parametrize("route", list(ROUTES))
def test_average_on_is_the_run_with_it_off(golden_dir, route):
    """Three steps with the average on and off: losses, parameters and moments are bit-identical — the average writes nothing but the
    shadow, and the default step is the step it was.  The run with it on issues one cpc_ema behind every update, the other none."""
    dtype, kw = ROUTES[route]
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    batches = A._batches(data, meta["B"])
    runs = []
    for ema in ({}, dict(ema_decay=DECAY)):
        model = build(dtype)
        with A._Spy() as spy:
            opt, losses, _ = A._engine_steps(model, data, batches, 3, **kw, **ema)
        runs.append((losses, model._flat_param.detach().clone(), opt.m.clone(), opt.v.clone()))
        assert spy.names.count("cpc_ema") == (spy.names.count(UPDATES[route]) if ema else 0)
        assert spy.names.count(UPDATES[route]) >= 3
        if ema:
            assert not torch.equal(opt.ema, runs[-1][1]) and bool(torch.isfinite(opt.ema).all())
        else:
            assert opt.ema is None
    assert runs[0][0] == runs[1][0]
    for a, b, name in zip(runs[0][1:], runs[1][1:], "pmv"):
        assert torch.equal(a, b), (route, name)


def test_update_range_pieces_average_every_element_once(golden_dir):
    """update_range pieces at parameter boundaries plus step() — the data-parallel route — against one whole-buffer step: the same bits
    in parameters, moments and shadow; and parameters and moments are those of the run with the average off."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    results = {}
    for mode in ("pieces", "whole", "pieces, average off"):
        model = build("fp32")
        model._flatten_parameters(DEV)
        n = model._flat_param.numel()
        gen = torch.Generator().manual_seed(6)
        model._flat_grad.copy_(torch.randn(n, generator=gen) * 0.3)
        shadow = (model._flat_param.detach() + torch.randn(n, generator=gen).to(DEV) * 0.01) if "off" not in mode else None
        opt = FusedAdam(model, lr=A.LR, **(dict(ema_decay=0.9, ema_warmup=True, ema=shadow) if shadow is not None else {}))
        with A._Spy() as spy:
            if mode != "whole":
                edges = sorted(model._offset.values()) + [n]
                cuts = [edges[0], edges[len(edges) // 3], edges[2 * len(edges) // 3], edges[-3], n]
                for lo, hi in reversed(list(zip(cuts[1:-1], cuts[2:]))):
                    opt.update_range(lo, hi, 1.0)
            opt.step(grad_scale=1.0)
        torch.cuda.synchronize()
        assert spy.names.count("cpc_ema") == {"pieces": 4, "whole": 1, "pieces, average off": 0}[mode]
        results[mode] = (model._flat_param.detach().clone(), opt.m.clone(), opt.v.clone(), None if shadow is None else opt.ema.clone())
        if shadow is not None:
            assert opt.ema is shadow          # the caller's tensor, updated in place
    for a, b, name in zip(results["pieces"], results["whole"], ("p", "m", "v", "ema")):
        assert torch.equal(a, b), name
    for a, b, name in zip(results["pieces"][:3], results["pieces, average off"][:3], "pmv"):
        assert torch.equal(a, b), name


def test_swap_and_ema_weights(golden_dir):
    """swap_ema() exchanges buffer and shadow and voids every engine's operand copies; ema_weights() restores the raw weights bit for
    bit, also on an exception, and a step inside it is refused."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    model = build("fp32")
    opt, _, _ = A._engine_steps(model, data, A._batches(data, meta["B"]), 2, ema_decay=DECAY)
    raw, avg = model._flat_param.detach().clone(), opt.ema.clone()
    x = data[A._batches(data, meta["B"])[0]].to(DEV).contiguous()
    eng = model.engine(x.shape[0], x.shape[1], DEV)
    token = eng._param_state()
    loss_raw = float(eng.loss_and_grads(x, softplus=True, regularization=A.REG)[0])
    with pytest.raises(KeyError):
        with opt.ema_weights():
            assert torch.equal(model._flat_param.detach(), avg) and torch.equal(opt.ema, raw) and eng._param_state() != token
            loss_avg = float(eng.loss_and_grads(x, softplus=True, regularization=A.REG)[0])          # the engine computes with them
            esd = opt.ema_state_dict()          # still the averaged weights
            with pytest.raises(RuntimeError):
                opt.step()
            with pytest.raises(RuntimeError):
                with opt.ema_weights():
                    pass
            raise KeyError("inside")
    assert torch.equal(model._flat_param.detach(), raw) and torch.equal(opt.ema, avg) and eng._param_state() != token
    assert loss_avg != loss_raw and float(eng.loss_and_grads(x, softplus=True, regularization=A.REG)[0]) == loss_raw
    for name, q in model.named_parameters():
        lo = model._offset[name]
        assert torch.equal(esd[name], avg[lo:lo + q.numel()].view(q.shape)), name
    assert opt.t == 2


# ------------------------------------------------------------------------------------------ 3. the trainer
class _Recorder(A._Logger):
    """Keeps (step, parameters, shadow) of every logged step; with host_sync_lag = 0 a step is logged before the next is launched."""

    def __init__(self):
        super().__init__()
        self.snaps, self.hook = [], None

    def log(self, step):
        super().log(step)
        torch.cuda.synchronize()
        tr = self.trainer
        self.snaps.append((step, tr.model._flat_param.detach().clone(), None if tr._ema is None else tr._ema.clone()))
        if self.hook is not None:
            self.hook(step)


def _train(model, data, meta, steps, first=0, trainer=None, lag=0, seed=True, **attrs):
    logger = _Recorder() if trainer is None else trainer.logger
    tr = trainer or A._trainer(model, data, meta, logger)
    tr.host_sync_lag = lag
    for k, v in attrs.items():
        setattr(tr, k, v)
    if seed:
        random.seed(A.SEED)
    ret = tr.train(batch_size=meta["B"], epochs=10, lr=A.LR, continue_training_at_step=first, num_workers=0, max_steps=first + steps)
    torch.cuda.synchronize()
    return tr, logger, ret


def _follows(snaps, start, decay, warmup, first_t=1, device_route=False):
    """Every recorded shadow against the float64 recurrence from the previous one (``start`` in front of the first) and the recorded
    parameters, at the host route's bound or, under device_route, widened by one unit in the last place of w times |p - ema|."""
    before = start
    for i, (step, p, e) in enumerate(snaps):
        t = first_t + i
        if device_route:
            w = ema_weight(_f32(decay), warmup, t)
            bound = _bound(p, before) + float(np.spacing(np.float32(w))) * (p.double() - before.double()).abs()
        else:
            w, bound = _host_w(decay, warmup, t), _bound(p, before)
        err = (e.double() - _ema64(p, before, w)).abs()
        print(f"  step {step}: t {t}, w {w:.6f}, worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), (step, t)
        assert not torch.equal(e, before)
        before = e


def _start(build):
    model = build("fp32")
    model._flatten_parameters(DEV)
    return model, model._flat_param.detach().clone()


@pytest.mark.parametrize("warmup", [False, True])
def test_graphed_shadow_against_eager(golden_dir, warmup):
    """trainer.use_graph: cpc_ema sits in the captured step behind cpc_adam_dev and reads the device's count.  Its shadow follows the
    float64 recurrence on the run's own parameters at the device route's bound, and lies from the eager run's shadow no further than
    both runs' bounds and the runs' own parameter differences allow: D_t = (1 - w) D_(t-1) + w |p_graph - p_eager| + the two bounds
    (each with its route's rounding of w) — the device route's bound where the parameters agree.  Losses, parameters and moments are those of the captured run with
    the average off, bit for bit."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    steps = 4
    runs = {}
    for name, attrs in (("eager", dict(ema_decay=DECAY, ema_warmup=warmup)), ("graph", dict(ema_decay=DECAY, ema_warmup=warmup, use_graph=True)),
                        ("graph, average off", dict(use_graph=True))):
        model, start = _start(build)
        with A._Spy() as spy:
            tr, logger, _ = _train(model, data, meta, steps, **attrs)
        assert ("cpc_adam_dev" in spy.names) == ("graph" in name)
        assert ("cpc_ema" in spy.names) == ("off" not in name)
        runs[name] = (tr, logger, start)
    for name in ("eager", "graph"):
        print(name)
        _follows(runs[name][1].snaps, runs[name][2], DECAY, warmup, device_route=name == "graph")
    assert int(runs["graph"][0].last_optimizer.state.cpu()[:1].view(torch.int32)) == steps
    spread = torch.zeros_like(runs["eager"][2], dtype=torch.float64)
    prev = {name: runs[name][2] for name in ("eager", "graph")}
    for t, ((_, pe, ee), (_, pg, eg)) in enumerate(zip(runs["eager"][1].snaps, runs["graph"][1].snaps), 1):
        w = ema_weight(_f32(DECAY), warmup, t)
        ulp = float(np.spacing(np.float32(w)))
        spread = ((1 - w) * spread + w * (pg.double() - pe.double()).abs() + _bound(pe, prev["eager"]) + _bound(pg, prev["graph"])
                  + ulp * ((pg.double() - prev["graph"].double()).abs() + (pe.double() - prev["eager"].double()).abs()))
        worst = ((eg.double() - ee.double()).abs() / spread.clamp_min(1e-300)).max().item()
        print(f"graph against eager, step {t}: parameters differ by at most {(pg - pe).abs().max().item():.3e}, shadow / bound {worst:.3f}")
        assert bool(((eg.double() - ee.double()).abs() <= spread).all()), t
        prev = {"eager": ee, "graph": eg}
    on, off = runs["graph"], runs["graph, average off"]
    assert on[1].loss_meter.values == off[1].loss_meter.values
    assert torch.equal(on[0].model._flat_param, off[0].model._flat_param)
    assert torch.equal(on[0].last_optimizer.m, off[0].last_optimizer.m) and torch.equal(on[0].last_optimizer.v, off[0].last_optimizer.v)
    assert off[0].last_optimizer.ema is None and off[0]._ema is None


@pytest.mark.parametrize("use_graph", [False, True])
def test_nan_guard_freezes_the_shadow(golden_dir, use_graph):
    """An inf in one clip of batch 1: train() returns None at step 1, although the host has launched later steps by then (host_sync_lag
    1); the shadow is bit for bit the shadow of a clean run of one step — the launches behind the NaN loss moved neither Adam nor the
    average."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    bad_step = 1
    batches = A._batches(data, meta["B"])
    assert len(batches) > bad_step + 1
    victim = batches[bad_step][1]
    assert all(victim not in b for b in batches[:bad_step])
    model, start = _start(build)
    tr0, _, _ = _train(model, data, meta, bad_step, lag=1, ema_decay=DECAY, use_graph=use_graph)
    good_p, good_e = model._flat_param.detach().clone(), tr0._ema.clone()
    assert not torch.equal(good_e, start) and not torch.equal(good_e, good_p)
    poisoned = data.clone()
    poisoned[victim, poisoned.shape[1] // 2] = float("inf")
    model, _ = _start(build)
    with A._Spy() as spy:
        tr, logger, ret = _train(model, poisoned, meta, bad_step + 3, lag=1, ema_decay=DECAY, use_graph=use_graph)
    assert ret is None and tr.training_step == bad_step and len(logger.loss_meter.values) == bad_step
    if not use_graph:          # (a captured step's launches do not pass through the spy)
        assert spy.names.count("cpc_nce_loss") > bad_step + 1          # later steps were launched
    assert torch.equal(model._flat_param.detach(), good_p) and torch.equal(tr._ema, good_e)


VAL_B = 8          # validate() draws runs of eight clips per file (FileBatchSampler(file_batch_size=8)): its batch size is a multiple of 8


def _validation(v):
    losses, acc, score, mi = v
    return losses.cpu().double(), acc.cpu().double(), float(score), mi.cpu().double()


@pytest.mark.parametrize("use_graph", [False, True])
def test_validate_with_the_averaged_weights(golden_dir, use_graph):
    """validate(use_ema=True) after training equals validate() of a fresh model loaded from ema_state_dict() at the existing validate
    tolerance (tests/test_model_gpu.py: 2e-4 on losses, bound and mean score, 1e-6 on accuracies), differs from validate() on the raw
    weights, and leaves the raw parameters bit for bit.  Called from logger.log() in the middle of train() — and calc_test_task_data
    with it — the run goes on as the run without the call, into the next epoch (whose batches are drawn after the call: validate's
    sampler seeds Python's generator, and use_ema=True puts its state back): losses, parameters, moments and shadow bit for bit."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    vset = TensorAudioDataset(data, device=DEV)
    steps = 6
    assert data.shape[0] // meta["B"] < steps          # the run crosses an epoch boundary behind the call
    model, _ = _start(build)
    plain, plain_log, _ = _train(model, data, meta, steps, lag=1, ema_decay=DECAY, use_graph=use_graph)
    model, _ = _start(build)
    logger = _Recorder()
    tr = A._trainer(model, data, meta, logger)
    tr.validation_set, tr.test_task_set = vset, _Labelled(data[:6])
    seen = {}

    def hook(step):
        if step == 1:
            raw = tr.model._flat_param.detach().clone()
            seen["ema"] = _validation(tr.validate(batch_size=VAL_B, num_workers=0, use_ema=True))
            seen["task"] = tr.calc_test_task_data(batch_size=4, num_workers=0, use_ema=True)[0]
            seen["task raw"] = tr.calc_test_task_data(batch_size=4, num_workers=0)[0]
            assert torch.equal(tr.model._flat_param.detach(), raw)

    logger.hook = hook
    _train(model, data, meta, steps, trainer=tr, lag=1, ema_decay=DECAY, use_graph=use_graph)
    assert "ema" in seen and np.abs(seen["task"] - seen["task raw"]).max() > 0
    assert logger.loss_meter.values == plain_log.loss_meter.values and logger.steps == plain_log.steps
    assert torch.equal(tr.model._flat_param, plain.model._flat_param) and torch.equal(tr._ema, plain._ema)
    assert torch.equal(tr.last_optimizer.m, plain.last_optimizer.m) and torch.equal(tr.last_optimizer.v, plain.last_optimizer.v)
    # after the run: against a fresh model that holds the averaged weights
    raw = tr.model._flat_param.detach().clone()
    got = _validation(tr.validate(batch_size=VAL_B, num_workers=0, use_ema=True))
    assert torch.equal(tr.model._flat_param.detach(), raw) and tr.model.training
    on_raw = _validation(tr.validate(batch_size=VAL_B, num_workers=0))
    fresh = build("fp32")
    fresh.load_state_dict(tr.ema_state_dict())
    other = A._trainer(fresh, data, meta, A._Logger())
    other.validation_set = vset
    want = _validation(other.validate(batch_size=VAL_B, num_workers=0))
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-30)).item()
    print(f"validate(use_ema) against the loaded model: losses {rel(got[0], want[0]):.3e}, bound {rel(got[3], want[3]):.3e}; "
          f"against the raw weights: losses {rel(got[0], on_raw[0]):.3e}")
    assert rel(got[0], want[0]) < 2e-4 and rel(got[3], want[3]) < 2e-4 and (got[1] - want[1]).abs().max().item() < 1e-6
    assert abs(got[2] - want[2]) < 2e-4 * max(1.0, abs(want[2]))
    assert not torch.equal(got[0], on_raw[0])
    with pytest.raises(ValueError):
        A._trainer(build("fp32"), data, meta, A._Logger()).validate(batch_size=VAL_B, num_workers=0, use_ema=True)


class _Labelled(torch.utils.data.Dataset):
    def __init__(self, clips):
        self.clips = clips

    def __len__(self):
        return self.clips.shape[0]

    def __getitem__(self, i):
        return self.clips[i], i


def test_the_trainer_owns_the_shadow(golden_dir):
    """Two train() calls carry the shadow across (the second call's first average starts from the first call's last shadow, with the
    new optimizer's update number 1); reset_ema() between them starts over from the parameters as they then stand."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    finals = []
    for reset in (False, True):
        model, start = _start(build)
        tr, logger, _ = _train(model, data, meta, 2, ema_decay=DECAY, ema_warmup=True)
        shadow, first = tr._ema, list(logger.snaps)
        assert tr.last_optimizer.ema is shadow
        _follows(first, start, DECAY, True)
        if reset:
            tr.reset_ema()
            assert tr._ema is None
            with pytest.raises(ValueError):
                tr.ema_state_dict()
        _train(model, data, meta, 2, first=2, trainer=tr, seed=False, ema_decay=DECAY, ema_warmup=True)
        second = logger.snaps[len(first):]
        assert [s for s, _, _ in second] == [2, 3] and (tr._ema is shadow) == (not reset) and tr.last_optimizer.ema is tr._ema
        _follows(second, first[-1][1] if reset else first[-1][2], DECAY, True)
        finals.append(tr._ema.clone())
        esd = tr.ema_state_dict()
        assert list(esd) == list(model.state_dict())
        for name, q in model.named_parameters():
            lo = model._offset[name]
            assert torch.equal(esd[name], tr._ema[lo:lo + q.numel()].view(q.shape)), name
    assert not torch.equal(finals[0], finals[1])
    # without a decay the next train() leaves the shadow alone and issues nothing for it
    with A._Spy() as spy:
        _train(model, data, meta, 1, first=4, trainer=tr, seed=False, ema_decay=None, ema_warmup=False)
    assert "cpc_ema" not in spy.names and torch.equal(tr._ema, finals[1]) and tr.last_optimizer.ema is None


def test_resumed_run_is_the_uninterrupted_run(golden_dir):
    """Six steps against three, last_optimizer.state_dict() (which carries "ema") through optimizer_state into a new trainer on a
    fresh model, and three more: parameters, moments and shadow bit for bit.  Without "ema" in the state the shadow starts over."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    data = data[:3 * meta["B"]]          # three batches per epoch: the second call's sampler starts where the second epoch does
    kw = dict(ema_decay=0.9, ema_warmup=True)
    tr_a, log_a, _ = _train(build("fp32"), data, meta, 6, **kw)
    model_b = build("fp32")
    tr_b, log_b, _ = _train(model_b, data, meta, 3, **kw)
    saved = tr_b.last_optimizer.state_dict()
    assert all("ema" in entry for entry in saved["state"].values())
    sampler_state = random.getstate()          # both continuations draw the batches the uninterrupted run draws from here on
    model_c = build("fp32")
    model_c.load_state_dict({k: v.detach().clone() for k, v in model_b.state_dict().items()})
    random.setstate(sampler_state)
    tr_c, log_c, _ = _train(model_c, data, meta, 3, first=3, seed=False, optimizer_state=saved, **kw)
    assert log_b.loss_meter.values + log_c.loss_meter.values == log_a.loss_meter.values and tr_c.last_optimizer.t == 6
    assert torch.equal(tr_c.model._flat_param, tr_a.model._flat_param) and torch.equal(tr_c._ema, tr_a._ema)
    assert torch.equal(tr_c.last_optimizer.m, tr_a.last_optimizer.m) and torch.equal(tr_c.last_optimizer.v, tr_a.last_optimizer.v)
    for entry in saved["state"].values():
        del entry["ema"]
    model_d = build("fp32")
    model_d.load_state_dict({k: v.detach().clone() for k, v in model_b.state_dict().items()})
    random.setstate(sampler_state)
    tr_d, _, _ = _train(model_d, data, meta, 3, first=3, seed=False, optimizer_state=saved, **kw)
    assert torch.equal(tr_d.model._flat_param, tr_a.model._flat_param) and not torch.equal(tr_d._ema, tr_a._ema)


def test_generic_route_averages_behind_a_foreign_optimizer(golden_dir):
    """torch.optim.SGD takes the generic route: engine.TorchEma behind optimizer.step(), no cpc_ema; the shadow follows the float64
    recurrence at the bound of the three float32 roundings its torch ops make, validate(use_ema=True) swaps through TorchEma."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    model, start = _start(build)
    logger = _Recorder()
    tr = A._trainer(model, data, meta, logger)
    tr.optimizer, tr.validation_set = torch.optim.SGD, TensorAudioDataset(data, device=DEV)
    assert not tr._fused()
    with A._Spy() as spy:
        _train(model, data, meta, 3, trainer=tr, ema_decay=DECAY, ema_warmup=True)
    assert "cpc_ema" not in spy.names and "cpc_adam" not in spy.names and len(logger.snaps) == 3
    _follows(logger.snaps, start, DECAY, True)
    raw = model._flat_param.detach().clone()
    got = _validation(tr.validate(batch_size=VAL_B, num_workers=0, use_ema=True))
    assert torch.equal(model._flat_param.detach(), raw)
    assert not torch.equal(got[0], _validation(tr.validate(batch_size=VAL_B, num_workers=0))[0])
    esd = tr.ema_state_dict()
    lo = model._offset["prediction_model.weight"]
    assert list(esd) == list(model.state_dict())
    assert torch.equal(esd["prediction_model.weight"].reshape(-1), tr._ema[lo:lo + esd["prediction_model.weight"].numel()])
