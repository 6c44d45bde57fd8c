"""The NaN guard at the level where its promise is made ("What the NaN guard holds still"): on every step route of
ContrastiveEstimationTrainer a NaN loss at step n leaves train() with the whole run state — parameters, buffers, Adam's moments and
counts, the shadow, the temperature, the trust table, the host counters, the logger's meters and the exported optimizer state —
bit for bit where a clean run of n steps leaves it, although the host has launched further steps by the time it learns of the
loss.  One case function over a table of configurations; a control per update-kernel family shows that the comparison fails when
that family's launches lose the skip flag.  No tolerance anywhere: every comparison is of bits."""
import json
import os
import random
from types import SimpleNamespace

import pytest
import torch

import test_adamw_gpu as A
import test_gru_stacked_gpu as TG
import test_lstm_gpu as TL
import test_scalogram_gpu as TS
import test_temperature_gpu as TM
from cpc_audio_amd import contrastive_estimation_training as CET
from cpc_audio_amd.audio_dataset import TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioPredictiveCodingModel, ConvolutionalArModel
from cpc_audio_amd.augmentation import WaveAugmentation
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, LRSchedule, NormalizedScoreFunction,
                                                           TemperatureSchedule, difference_score_function, linear_score_function,
                                                           softplus_score_function)
from cpc_audio_amd.engine import FusedAdam
from cpc_audio_amd.grid_masking import GridMasking

pytestmark = pytest.mark.gpu

DEV = A.DEV
SEED, LR = A.SEED, A.LR
SCHED = LRSchedule("cosine", warmup_steps=2, total_steps=12, min_lr_ratio=0.1)          # every step of a case has a rate of its own


# ------------------------------------------------------------------------------------------ fixtures
def _conv_bn(golden_dir):
    """conv_ar_bn.npz, variant 'bn': the small waveform encoder under a ConvolutionalArModel with BatchNorm1d."""
    g = A._load(golden_dir, "conv_ar_bn.npz")
    meta = json.load(open(os.path.join(golden_dir, "conv_ar_bn.json")))
    state = {k[len("bn/param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("bn/param/")}
    ar_dict = dict(meta["variants"]["bn"]["ar"], activation_register=None)

    def build(dtype):
        enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [meta["C"]] * 5, 'bias': True})
        model = AudioPredictiveCodingModel(enc, ConvolutionalArModel(ar_dict), enc_size=meta["C"], ar_size=meta["H"],
                                           visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype=dtype)
        model.load_state_dict(state)
        return model.to(DEV), None
    return SimpleNamespace(data=torch.from_numpy(g["data"]), B=meta["B"], K=meta["K"], H=meta["H"], build=build, adamw=None)


def _scalogram(golden_dir, name):
    g = A._load(golden_dir, name + ".npz")
    meta = json.load(open(os.path.join(golden_dir, name + ".json")))

    def build(dtype):
        pre, model = TS._build_scalogram_model(g, meta, dtype)
        return model, pre
    return SimpleNamespace(data=torch.from_numpy(g["data"]), B=meta["B"], K=meta["K"], H=meta["H"], build=build, adamw=None)


def _fx(golden_dir, name):
    """data, B, K, H and build(dtype) -> (model on the device, preprocessing module or None) of a fixture; ``adamw``: the meta of
    tests/test_adamw_gpu.py's fixtures, whose _trainer then builds the trainer."""
    if name in ("gru", "conv", "attention"):
        meta, data, _, build, _ = A._fixture(golden_dir, name)
        return SimpleNamespace(data=data, B=meta["B"], K=meta["K"], H=meta["H"], build=lambda dtype: (build(dtype), None), adamw=meta)
    if name == "lstm":
        return SimpleNamespace(data=TL._data(3 * TL.B_S, 5), B=TL.B_S, K=TL.K_S, H=32, adamw=None,
                               build=lambda dtype: (TL._model(dtype, 32).to(DEV), None))
    if name == "gru_stack2":
        return SimpleNamespace(data=TG._data(3 * TG.B_S, 5), B=TG.B_S, K=TG.K_S, H=64, adamw=None,
                               build=lambda dtype: (TG._model(dtype, 2, 64).to(DEV), None))
    if name == "fused_all_t":          # the smallest shape whose all-timesteps loss takes the fused score route (bf16, B K = 256, E = 128)
        B, length = 64, TM._fused_route_model()[2].shape[1]
        data = torch.randn(3 * B, length, generator=torch.Generator().manual_seed(3)) * 0.5
        return SimpleNamespace(data=data, B=B, K=4, H=64, adamw=None, build=lambda dtype: (TM._fused_route_model()[0], None))
    if name == "conv_bn":
        return _conv_bn(golden_dir)
    return _scalogram(golden_dir, name)


# ------------------------------------------------------------------------------------------ the table
def _cfg(fixture="gru", dtype="fp32", attrs=None, score=None, ctor=None, reg=A.REG, loss=("cpc_nce_loss",), lag=1, interval=1, extra=2,
         cont=False, bad_steps=(0, 2), graph=False, generic=False, batchnorm=False, checks_ring=False):
    """attrs: trainer attributes; score: factory of the score function (a NormalizedScoreFunction keeps its device temperature, so
    every run gets its own); ctor: further constructor keywords; loss: the loss entry point(s) of the route; the poisoned run has
    bad_step + lag + extra steps; cont: the going-on check; batchnorm: the model has running statistics."""
    return SimpleNamespace(fixture=fixture, dtype=dtype, attrs=attrs or {}, score=score or (lambda: softplus_score_function), ctor=ctor or {},
                           reg=reg, loss=loss, lag=lag, interval=interval, extra=extra, cont=cont, bad_steps=bad_steps, graph=graph,
                           generic=generic, batchnorm=batchnorm, checks_ring=checks_ring)


def _generic_score():
    return lambda p, t: softplus_score_function(p, t)          # a callable the trainer does not recognise: the generic route


GROUP_IDS = [i % 3 for i in range(24)]          # small_model has 24 clips: three "speakers", interleaved
ADAMW = dict(weight_decay=A.WD, lr_schedule=SCHED)
CONFIGS = {
    "adamw_sched": _cfg(attrs=ADAMW, cont=True),
    "adamw_sched_graph": _cfg(attrs=ADAMW, graph=True, cont=True),
    "lamb": _cfg(attrs=dict(trust_ratio=True, trust_clip=0.5, weight_decay=0.1, max_grad_norm=0.05)),
    "ema_adamw_clip": _cfg(attrs=dict(ema_decay=0.5, ema_warmup=True, weight_decay=A.WD, max_grad_norm=0.05), cont=True),
    "temp_learnable": _cfg(score=lambda: NormalizedScoreFunction(learnable=True), cont=True),
    "temp_learnable_graph": _cfg(score=lambda: NormalizedScoreFunction(learnable=True), graph=True),
    "temp_scheduled": _cfg(score=lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("cosine", 0.2, 0.05, 12))),
    "sampled": _cfg(attrs=dict(num_negatives=3, negative_seed=7), loss=("cpc_nce_loss_sampled",), cont=True),
    "grouped": _cfg(attrs=dict(negative_groups="other_files", negative_group_ids=GROUP_IDS, num_negatives=2, negative_seed=7),
                    loss=("cpc_nce_loss_grouped",)),
    "bank": _cfg(attrs=dict(negative_bank=2), loss=("cpc_nce_loss", "cpc_nce_loss_banked"), cont=True, bad_steps=(0, 2, 3)),
    "difference": _cfg(score=lambda: difference_score_function),
    "all_t_bf16": _cfg(dtype="bf16", attrs=dict(score_over_all_timesteps=True), loss=("cpc_nce_loss_all",)),
    "all_t_fused_bf16": _cfg(fixture="fused_all_t", dtype="bf16", reg=1.0, attrs=dict(score_over_all_timesteps=True),
                             loss=("cpc_nce_fused_finalize",)),
    "lstm": _cfg(fixture="lstm", reg=1.0),
    "gru_stack2": _cfg(fixture="gru_stack2", reg=1.0),
    "attention": _cfg(fixture="attention"),
    "conv_bn": _cfg(fixture="conv_bn", reg=1.0, batchnorm=True),
    "scalogram_ahead": _cfg(fixture="scalogram_model", reg=1.0, batchnorm=True,
                            attrs=dict(preprocess_ahead=True,
                                       grid_masking=GridMasking(freq_masks=(2, 6), time_masks=(2, 12), fill="mean", protect_last=2, seed=31),
                                       augmentation=WaveAugmentation(speed=0.1, noise_snr_db=(10.0, 20.0), gain_db=(-3.0, 3.0), polarity=0.5,
                                                                     seed=21))),
    "scalogram_gp": _cfg(fixture="scalogram_model_gp", reg=0.01, batchnorm=True, score=lambda: linear_score_function,
                         ctor=dict(wasserstein_gradient_penalty=True, gradient_penalty_factor=1.0)),
    "lag0": _cfg(lag=0, interval=1, extra=6, checks_ring=True),
    "lag2_interval3": _cfg(lag=2, interval=3, extra=4, checks_ring=True),
    "generic_ema_adamw": _cfg(score=_generic_score, generic=True, attrs=dict(ema_decay=0.5, weight_decay=A.WD, lr_schedule=SCHED)),
    "generic_lamb": _cfg(score=_generic_score, generic=True, attrs=dict(trust_ratio=True, weight_decay=0.1)),
}
CASES = [pytest.param(name, bad_step, id=f"{name}-{bad_step}") for name, cfg in CONFIGS.items() for bad_step in cfg.bad_steps]


# ------------------------------------------------------------------------------------------ one run and its state
class _Log(A._Logger):
    def __init__(self):
        super().__init__()
        self.grad_norm_meter, self.temperature_meter = A._Meter(), A._Meter()

    def meters(self):
        return {k: list(v.values) for k, v in vars(self).items() if isinstance(v, A._Meter)}


def _run(fx, cfg, data, steps, first=0, resume=None, lag=None, seed=True):
    """One train() call of the configuration over ``data`` under the Python seed (seed=False: the sampler draws on from where Python's
    generator stands): ``steps`` steps from step ``first`` (0 steps: the run is set up and left as it starts).  resume: (model state
    dict, optimizer state dict) of an earlier run."""
    model, pre = fx.build(cfg.dtype)
    logger = _Log()
    if fx.adamw is not None and not cfg.ctor:
        tr = A._trainer(model, data, fx.adamw, logger, score_function=cfg.score())
        assert tr.regularization == cfg.reg
    else:
        kw = dict(cfg.ctor, **({} if pre is None else {"preprocessing": pre}))
        tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                          regularization=cfg.reg, score_function=cfg.score(), prediction_steps=fx.K, ar_size=fx.H, **kw)
        tr.verbose = False
        logger.trainer = tr
    for k, v in cfg.attrs.items():
        setattr(tr, k, v)
    tr.use_graph, tr.host_sync_interval = cfg.graph, cfg.interval
    tr.host_sync_lag = cfg.lag if lag is None else lag
    if resume is not None:
        model.load_state_dict({k: v.detach().clone() for k, v in resume[0].items()})
        tr.optimizer_state = resume[1]
    assert tr._fused() or tr._engine_difference() or tr._engine_normalized() or cfg.generic
    if seed:
        random.seed(SEED)
    with A._Spy() as spy:
        ret = tr.train(batch_size=fx.B, epochs=10 if steps else 0, lr=LR, continue_training_at_step=first, num_workers=0,
                       max_steps=first + steps if steps else None)
    torch.cuda.synchronize()
    return SimpleNamespace(ret=ret, tr=tr, model=model, logger=logger, names=spy.names)


def _flat(prefix, value, out):
    if isinstance(value, dict):
        for k, v in value.items():
            _flat(f"{prefix}/{k}", v, out)
    else:
        out[prefix] = value.detach().clone() if isinstance(value, torch.Tensor) else value
    return out


def _state(run):
    """Everything a run leaves behind, by name: tensors (clones) and plain values."""
    tr = run.tr
    out = _flat("model", run.model.state_dict(), {})
    out.update(training_step=tr.training_step, last_lr=tr.last_lr, last_temperature=tr.last_temperature)
    opt = getattr(tr, "last_optimizer", None)
    if opt is not None:
        out.update(m=opt.m.clone(), v=opt.v.clone(), t=opt.t)
        if opt.state is not None:
            out["device step count"] = int(opt.state[0:1].view(torch.int32).item())
            out["state[1:4]"] = opt.state[1:4].clone()
        if opt.trust_ratio:
            out["trust table"] = opt.trust.clone()
            _flat("trust_ratios", opt.trust_ratios(), out)
        _flat("state_dict", opt.state_dict(), out)
    if tr._ema is not None:
        out["shadow"] = tr._ema.clone()
    if tr._temperature is not None:
        out["tstate"] = tr._temperature.tstate.clone()
    if tr._bank is not None:
        out["negative_bank_filled"] = tr.negative_bank_filled
    return out


def _same_bits(a, b):
    if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
        return False
    if not isinstance(a, torch.Tensor):
        return type(a) is type(b) and a == b
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.detach().reshape(-1).cpu(), b.detach().reshape(-1).cpu()
    if a.is_floating_point():          # (NaN statistics compare equal to themselves, -0 differs from 0)
        as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(as_int), b.view(as_int)
    return torch.equal(a, b)


def _differences(got, want):
    """Names present on one side only, or whose bits differ."""
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or not _same_bits(got[k], want[k]))


def _is_statistic(name):
    return "running_" in name or name.endswith("num_batches_tracked")


def _poison(fx, bad_step):
    batches = A._batches(fx.data, fx.B)
    assert len(batches) > bad_step
    victim = batches[bad_step][1]
    assert all(victim not in b for b in batches[:bad_step])
    poisoned = fx.data.clone()
    poisoned[victim, poisoned.shape[1] // 2] = float("inf")
    return poisoned


def _in_flight(cfg, names, bad_step):
    """The route's loss kernel behind the NaN step: launches went on while the host had not yet read the step's loss; with nothing in
    flight (host_sync_lag 0, the generic route, which reads every loss at once) the NaN step's is the last."""
    count = sum(names.count(n) for n in cfg.loss)
    if cfg.lag == 0 or cfg.generic:
        assert count == bad_step + 1, (count, bad_step)
    else:
        assert count > bad_step + 1, (count, bad_step)


def _nan_case(golden_dir, name, bad_step):
    """The clean run and the poisoned run of a configuration, after every assertion that does not compare their states: ->
    (configuration, fixture, clean run, poisoned run, the state to expect, the poisoned run's state)."""
    cfg, fx = CONFIGS[name], _fx(golden_dir, CONFIGS[name].fixture)
    clean = _run(fx, cfg, fx.data, bad_step)
    assert clean.ret is None and clean.tr.training_step == bad_step and clean.logger.steps == list(range(bad_step))
    poisoned_data = _poison(fx, bad_step)
    bad = _run(fx, cfg, poisoned_data, bad_step + cfg.lag + cfg.extra)
    assert bad.ret is None
    assert bad.tr.training_step == bad_step
    meters = bad.logger.meters()
    assert len(meters["loss_meter"]) == len(meters["score_meter"]) == len(meters["lr_meter"]) == bad_step
    assert meters == clean.logger.meters() and bad.logger.steps == list(range(bad_step))
    if "max_grad_norm" in cfg.attrs:
        assert len(meters["grad_norm_meter"]) == bad_step
    if isinstance(bad.tr.score_function, NormalizedScoreFunction) and bad.tr._temperature is not None:
        assert len(meters["temperature_meter"]) == bad_step
    if not cfg.graph:          # (a captured step's launches do not pass through the spy)
        _in_flight(cfg, bad.names, bad_step)
    want, got = _state(clean), _state(bad)
    if cfg.batchnorm:
        # the reference returns inside the NaN step, behind its forward pass: the statistics are those of a run that stops there,
        # which is this configuration at host_sync_lag 0 (nothing is launched behind the NaN step, nothing is put back)
        at_once = _state(_run(fx, cfg, poisoned_data, bad_step + 1, lag=0))
        statistics = [k for k in want if _is_statistic(k)]
        assert statistics
        for k in statistics:
            want[k] = at_once[k]
        counts = [int(got[k]) for k in statistics if k.endswith("num_batches_tracked")]
        assert counts and all(c == bad_step + 1 for c in counts), counts
    if "negative_bank_filled" in got:          # by design the one place the two runs differ: the bank is emptied
        assert got.pop("negative_bank_filled") == 0 and want.pop("negative_bank_filled") == min(bad_step, 2)
    return cfg, fx, clean, bad, want, got


def _ring_watch(monkeypatch):
    """Records (entries, BatchNorm slots, allowed depth) behind every snapshot of the rollback."""
    seen, real = [], CET._NanRollback.snapshot

    def snapshot(self, step):
        real(self, step)
        seen.append((len(self.snaps), len(self.host), len(self.ring), CET._ring_depth(self.trainer)))
    monkeypatch.setattr(CET._NanRollback, "snapshot", snapshot)
    return seen


# ------------------------------------------------------------------------------------------ 1. the cases
@pytest.mark.parametrize("name,bad_step", CASES)
def test_nan_loss_leaves_the_state_of_the_clean_run(golden_dir, monkeypatch, name, bad_step):
    """An inf in the middle of one clip of batch ``bad_step``: train() returns None with training_step == bad_step, the logger holds
    the bad_step good steps, and everything _state() names is bit for bit what the clean run of bad_step steps left (BatchNorm's
    statistics: what a run that stops inside the NaN step leaves; the bank: emptied)."""
    ring = _ring_watch(monkeypatch) if CONFIGS[name].checks_ring else None
    cfg, fx, clean, bad, want, got = _nan_case(golden_dir, name, bad_step)
    assert _differences(got, want) == []
    if name == "temp_scheduled" and bad_step:
        # the last good step's value: what the logger got for it, one float32 rounding from the host's schedule
        assert bad.tr.last_temperature == bad.logger.temperature_meter.values[-1]
        host = bad.tr.score_function.schedule.value(bad_step - 1)
        assert abs(bad.tr.last_temperature - host) <= 2.0 ** -23 * host
    if ring is not None:
        assert ring and all(max(snaps, host, slots) <= depth for snaps, host, slots, depth in ring), ring
        assert all(depth == cfg.interval + cfg.lag + 2 for _, _, _, depth in ring)
    if not cfg.cont:
        return
    # going on from either final state is the same run
    ends = []
    for run in (clean, bad):
        resume = (run.model.state_dict(), run.tr.last_optimizer.state_dict())
        nxt = _run(fx, cfg, fx.data, 2, first=bad_step, resume=resume)
        assert nxt.ret is None and nxt.tr.training_step == bad_step + 2 and nxt.logger.steps == [bad_step, bad_step + 1]
        assert nxt.tr.last_optimizer.t == bad_step + 2
        ends.append((nxt, dict(_state(nxt), **{"meter/" + k: v for k, v in nxt.logger.meters().items()})))
    assert _differences(ends[1][1], ends[0][1]) == []
    assert not _same_bits(ends[0][1]["m"], want["m"])          # ... and it did go on
    if name == "bank":          # a resumed bank starts empty: the first step is the in-batch step
        for nxt, _ in ends:
            assert [n for n in nxt.names if n in cfg.loss] == ["cpc_nce_loss", "cpc_nce_loss_banked"]
            assert nxt.tr.negative_bank_filled == 2


# ------------------------------------------------------------------------------------------ 2. the controls
def _without_skip_flag(method):
    """The FusedAdam method with skip_flag = None for its duration: its launches get NULL in the flag's place.  Numbers only: no
    pointer, size or index of the launch changes."""
    def wrapped(self, *args, **kw):
        real, self.skip_flag = self.skip_flag, None
        try:
            return method(self, *args, **kw)
        finally:
            self.skip_flag = real
    return wrapped


CONTROLS = {          # family -> (configuration, FusedAdam method that issues it, entry point, what must then differ, what must not)
    "adam": ("adamw_sched", "_update", "cpc_adamw", ["m", "v"], []),
    "lamb": ("lamb", "_update_lamb", "cpc_lamb", ["m", "v", "trust table"], []),
    "ema": ("ema_adamw_clip", "_update_ema", "cpc_ema", ["shadow"], ["m", "v"]),
    "temperature": ("temp_learnable", "_update_temperature", "cpc_temperature_step", ["tstate"], ["m", "v"]),
}


@pytest.mark.parametrize("family", list(CONTROLS))
def test_control_a_launch_without_the_skip_flag_is_noticed(golden_dir, monkeypatch, family):
    """The case above with one family's launches given NULL for the skip flag: that family's state no longer equals the clean run's
    (and the other families', still guarded, does) — the comparison of the cases sees a forgotten skip_flag argument."""
    name, method, entry, differs, holds = CONTROLS[family]
    bad_step = 2
    monkeypatch.setattr(FusedAdam, method, _without_skip_flag(getattr(FusedAdam, method)))
    cfg, fx, clean, bad, want, got = _nan_case(golden_dir, name, bad_step)
    assert bad.names.count(entry) > bad_step
    changed = _differences(got, want)
    print(f"{family}: {len(changed)} entries differ, among them {changed[:6]}")
    for k in differs:
        assert k in changed, (k, changed)
    for k in holds:
        assert k not in changed, (k, changed)
    if family in ("adam", "lamb"):
        assert any(k.startswith("model/") for k in changed)


# ------------------------------------------------------------------------------------------ 3. repeatability
@pytest.mark.parametrize("name", ["scalogram_gp", "scalogram_ahead", "lamb"])
def test_two_clean_runs_are_the_same_run(golden_dir, name):
    """The cases compare two runs, so the step has to be bit-repeatable: shown here for the routes nobody had checked — the
    gradient penalty's three passes, the scalogram computed ahead on the side stream, LAMB's block sums."""
    cfg, fx = CONFIGS[name], _fx(golden_dir, CONFIGS[name].fixture)
    a, b = _run(fx, cfg, fx.data, 3), _run(fx, cfg, fx.data, 3)
    assert a.logger.meters() == b.logger.meters() and len(a.logger.loss_meter.values) == 3
    assert _differences(_state(a), _state(b)) == []
