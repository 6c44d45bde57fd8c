"""Learnable and scheduled temperature of the cosine-similarity scores: everything that is decided on the host — the constructor's
argument checks, TemperatureSchedule.value, the trainer's refusals (raised before any GPU work), the -22 refusals of the four entry
points (before any launch, so the library alone is enough) and the state dict of the device object's host side.  No GPU needed."""
import ctypes as C
import inspect
import math

import pytest
import torch

from cpc_audio_amd import _hip, engine
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction, TemperatureSchedule)

L_, F_, D_ = C.c_longlong, C.c_float, C.c_double
P, NULL, S = C.c_void_p(0x1000), None, C.c_void_p(0)
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------ constructor
@pytest.mark.parametrize("kw", [
    dict(min_temperature=0.0), dict(min_temperature=-0.1), dict(min_temperature=NAN), dict(min_temperature=INF),
    dict(max_temperature=0.0), dict(max_temperature=NAN), dict(max_temperature=INF), dict(min_temperature="low"),
    dict(min_temperature=0.5, max_temperature=0.2),                                   # out of order
    dict(temperature=2.0, learnable=True), dict(temperature=0.001, learnable=True),     # the start outside the bounds
    dict(temperature=0.0, learnable=True), dict(learnable=1),
    dict(temperature_lr_scale=NAN), dict(temperature_lr_scale=-1.0), dict(temperature_lr_scale=INF),
    dict(schedule="cosine"), dict(schedule=0.1),
])
def test_constructor_refusals(kw):
    with pytest.raises(ValueError):
        NormalizedScoreFunction(**kw)


def test_learnable_and_schedule_exclude_each_other():
    sched = TemperatureSchedule("linear", 0.5, 0.1, 10)
    with pytest.raises(ValueError, match="not both"):
        NormalizedScoreFunction(0.2, learnable=True, schedule=sched)


def test_constructor_defaults_and_modes():
    sig = inspect.signature(NormalizedScoreFunction.__init__).parameters
    assert [sig[k].default for k in ("temperature", "learnable", "min_temperature", "max_temperature", "temperature_lr_scale",
                                     "schedule")] == [0.1, False, 0.01, 1.0, 1.0, None]
    plain = NormalizedScoreFunction(0.25)
    assert plain.temperature == 0.25 and not plain.learnable and plain.schedule is None and plain.current_temperature() == 0.25
    assert NormalizedScoreFunction(2.0).temperature == 2.0          # a constant is not held to the learnable mode's bounds
    learn = NormalizedScoreFunction(0.5, learnable=True, min_temperature=0.05, max_temperature=0.5, temperature_lr_scale=3)
    assert (learn.learnable, learn.min_temperature, learn.max_temperature, learn.temperature_lr_scale) == (True, 0.05, 0.5, 3.0)
    sched = NormalizedScoreFunction(schedule=TemperatureSchedule("cosine", 0.4, 0.1, 8))
    assert sched.temperature == 0.4 and sched.current_temperature() == 0.4          # the schedule's first value


@pytest.mark.parametrize("args", [("step", 0.5, 0.1, 10), ("linear", 0.0, 0.1, 10), ("linear", 0.5, -0.1, 10), ("linear", NAN, 0.1, 10),
                                  ("cosine", 0.5, INF, 10), ("cosine", 0.5, 0.1, 0), ("cosine", 0.5, 0.1, 2.5), ("linear", 0.5, 0.1, True)])
def test_bad_schedules(args):
    with pytest.raises(ValueError):
        TemperatureSchedule(*args)


def test_schedule_values():
    """End points, the mid point and beyond total_steps, for both kinds; a constant schedule is exact."""
    lin = TemperatureSchedule("linear", 0.5, 0.1, 10)
    assert lin.value(0) == 0.5 and lin.value(10) == pytest.approx(0.1, abs=1e-15) and lin.value(25) == lin.value(10)
    assert lin.value(5) == pytest.approx(0.3, abs=1e-15)
    cos = TemperatureSchedule("cosine", 0.5, 0.1, 10)
    assert cos.value(0) == 0.5 and cos.value(10) == 0.1 and cos.value(11) == 0.1 and cos.value(10 ** 9) == 0.1
    assert cos.value(5) == pytest.approx(0.3, abs=1e-15)
    assert cos.value(2) == pytest.approx(0.1 + 0.4 * 0.5 * (1.0 + math.cos(math.pi * 0.2)), abs=1e-15)
    assert lin.value(2) > cos.value(8) > cos.value(9)
    for kind in TemperatureSchedule.KINDS:
        flat = TemperatureSchedule(kind, 0.1, 0.1, 7)
        assert all(flat.value(s) == 0.1 for s in (0, 3, 7, 99))
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            lin.value(bad)
    assert lin.abi_args()[0] == 0 and cos.abi_args()[0] == 1 and cos.abi_args()[3].value == 10


# ------------------------------------------------------------------------------------------ trainer
def _tiny_model():
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    return AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                      prediction_steps=2)


def _trainer(fn, **kw):
    tr = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=None, score_function=fn, **kw)
    tr.verbose = False
    return tr


def test_learnable_is_refused_off_the_engine_route():
    """A foreign optimizer and global_negatives take the generic route: NotImplementedError from train(), before any GPU work (the
    model is on the CPU and there is no dataset: nothing behind the check could run)."""
    tr = _trainer(NormalizedScoreFunction(0.2, learnable=True), optimizer=torch.optim.SGD)
    with pytest.raises(NotImplementedError, match="learnable temperature"):
        tr.train(batch_size=4, epochs=1, max_steps=1)
    tr = _trainer(NormalizedScoreFunction(0.2, learnable=True))
    tr.global_negatives = True
    with pytest.raises(NotImplementedError, match="learnable temperature"):
        tr.train(batch_size=4, epochs=1, max_steps=1)


def test_learnable_is_refused_under_data_parallelism():
    tr = _trainer(NormalizedScoreFunction(0.2, learnable=True))
    tr._world = lambda: (0, 2)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.train(batch_size=4, epochs=1, max_steps=1)


@pytest.mark.parametrize("fn", [lambda: NormalizedScoreFunction(0.2, learnable=True),
                                lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("linear", 0.5, 0.1, 10))])
def test_gradient_penalty_is_refused_in_both_modes(fn):
    with pytest.raises(NotImplementedError):
        ContrastiveEstimationTrainer(model=_tiny_model(), dataset=None, score_function=fn(), preprocessing=lambda x: x,
                                     wasserstein_gradient_penalty=True)


def test_temperature_routes():
    """_check_temperature: a constant and the presets have no route; learnable is the device's; a schedule is the device's on the
    engine route of one process and the host's on the generic route and under data parallelism (allowed there)."""
    sched = lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("cosine", 0.5, 0.1, 10))
    assert _trainer(NormalizedScoreFunction(0.2))._check_temperature(1) is None
    assert ContrastiveEstimationTrainer(model=_tiny_model(), dataset=None)._check_temperature(1) is None
    assert _trainer(NormalizedScoreFunction(0.2, learnable=True))._check_temperature(1) == "device"
    assert _trainer(sched())._check_temperature(1) == "device"
    assert _trainer(sched())._check_temperature(2) == "host"
    assert _trainer(sched(), optimizer=torch.optim.SGD)._check_temperature(1) == "host"
    tr = _trainer(sched())
    tr.global_negatives = True
    assert tr._check_temperature(1) == "host"
    # without a device object the score keywords carry the constant
    assert _trainer(NormalizedScoreFunction(0.2, learnable=True))._score_kw() == {"score": "normalized", "temperature": 0.2}
    assert tr.last_temperature is None


def test_engine_surfaces_take_a_device_temperature():
    """FusedAdam and DeviceTemperature exist with the documented keywords; a float keeps check_temperature's float checks."""
    assert inspect.signature(engine.FusedAdam.__init__).parameters["temperature"].default is None
    sig = inspect.signature(engine.DeviceTemperature.__init__).parameters
    assert {"temperature", "mode", "min_temperature", "max_temperature", "lr_scale", "schedule", "device"} <= set(sig)
    for name in ("value", "state_dict", "load_state_dict", "tick", "bind"):
        assert callable(getattr(engine.DeviceTemperature, name))
    for bad in (0, -1, NAN, INF, "warm"):
        with pytest.raises(ValueError):
            engine.check_temperature(bad, "normalized")
    with pytest.raises(ValueError):
        engine.FusedAdam(None, 1e-3, temperature=0.1)          # a float is no DeviceTemperature (refused before the model is read)


def test_state_dict_round_trip_on_the_host():
    """DeviceTemperature's host side on a CPU tensor (the class only needs torch for its eight floats): host_state gives the constant
    path's bit pattern, and state_dict -> load_state_dict restores s, m, v, the derived values and the step."""
    import numpy as np
    s, scale, tau = engine.DeviceTemperature.host_state(0.1)
    assert scale == float(np.float32(1.0 / 0.1)) == C.c_float(1.0 / 0.1).value
    assert s == float(np.float32(math.log(scale))) and tau == float(np.float32(0.1))
    a = engine.DeviceTemperature(0.2, "learnable", 0.05, 0.5, lr_scale=2.0, device="cpu")
    assert a.bounds == (math.log(1.0 / 0.5), math.log(1.0 / 0.05)) and a.value() == float(np.float32(0.2))
    a.tstate[2], a.tstate[3], a.tstate[4] = 0.25, 0.5, -0.125
    a.step = 7
    saved = a.state_dict()
    assert saved["mode"] == "learnable" and saved["step"] == 7 and set(saved) >= {"s", "m", "v", "mode"}
    b = engine.DeviceTemperature(0.4, "learnable", 0.05, 0.5, device="cpu")
    b.load_state_dict(saved)
    assert torch.equal(a.tstate, b.tstate) and b.step == 7
    c = engine.DeviceTemperature(0.4, "learnable", 0.05, 0.5, device="cpu")
    c.load_state_dict({k: saved[k] for k in ("mode", "s", "m", "v")})          # the derived values are formed again from s
    assert torch.equal(c.tstate[:4], a.tstate[:4]) and float(c.tstate[5]) == pytest.approx(0.2, rel=1e-6)
    sched = engine.DeviceTemperature(mode="scheduled", schedule=TemperatureSchedule("linear", 0.5, 0.1, 10), device="cpu")
    assert sched.value() == 0.5
    with pytest.raises(ValueError, match="mode"):
        sched.load_state_dict(saved)
    for bad in ({"mode": "learnable"}, {"mode": "learnable", "s": NAN, "m": 0.0, "v": 0.0}, None):
        with pytest.raises(ValueError):
            b.load_state_dict(bad)
    with pytest.raises(ValueError):
        engine.DeviceTemperature(0.2, "annealed", device="cpu")
    with pytest.raises(ValueError):
        engine.DeviceTemperature(0.2, "scheduled", device="cpu")          # no schedule
    with pytest.raises(ValueError):
        engine.DeviceTemperature(2.0, "learnable", device="cpu")          # outside the bounds


# ------------------------------------------------------------------------------------------ the C ABI's refusals
def _norm_dev(name, ptrs, **over):
    k = dict(rows=4, E=64, rpi=0, item=0, ld=64, eps=1e-8, dtype=_hip.F32, scale=P)
    k.update(over)
    return getattr(_hip.lib(), name)(*ptrs, k["rows"], k["E"], k["rpi"], L_(k["item"]), L_(k["ld"]), k["scale"], k["eps"], k["dtype"], S)


@pytest.mark.parametrize("name,n", [("cpc_norm_rows_dev", 3), ("cpc_norm_rows_bwd_dev", 4)])
def test_norm_rows_dev_argument_checks_without_a_gpu(name, n):
    for over in (dict(rows=0), dict(rows=-3), dict(E=0), dict(E=4097), dict(rpi=-1), dict(eps=0.0), dict(eps=NAN), dict(eps=INF),
                 dict(dtype=2), dict(dtype=-1), dict(scale=NULL)):
        assert _norm_dev(name, [P] * n, **over) == -22, over
    for i in range(n):
        assert _norm_dev(name, [NULL if j == i else P for j in range(n)]) == -22, i


def _tstep(**over):
    k = dict(tstate=P, dots=P, rows=12, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, state=NULL, gs=1.0, s_min=-1.0, s_max=4.0, skip=NULL)
    k.update(over)
    return _hip.lib().cpc_temperature_step(k["tstate"], k["dots"], k["rows"], k["lr"], k["b1"], k["b2"], k["eps"], k["step"], k["state"],
                                           k["gs"], k["s_min"], k["s_max"], k["skip"], S)


def test_temperature_step_argument_checks_without_a_gpu():
    bad = [dict(tstate=NULL), dict(dots=NULL), dict(rows=0), dict(rows=-1), dict(s_min=2.0, s_max=1.0), dict(step=0)]
    bad += [{key: value} for key in ("lr", "b1", "b2", "eps", "gs", "s_min", "s_max") for value in (NAN, INF, -INF)]
    for over in bad:
        assert _tstep(**over) == -22, over


def _tset(**over):
    k = dict(tstate=P, kind=0, start=0.5, end=0.1, total=10, step=0, state=NULL, offset=0)
    k.update(over)
    return _hip.lib().cpc_temperature_set(k["tstate"], k["kind"], D_(k["start"]), D_(k["end"]), L_(k["total"]), L_(k["step"]), k["state"],
                                          L_(k["offset"]), S)


def test_temperature_set_argument_checks_without_a_gpu():
    bad = [dict(tstate=NULL), dict(kind=-1), dict(kind=2), dict(total=0), dict(total=-5), dict(step=-1), dict(state=P, offset=-1)]
    bad += [{key: value} for key in ("start", "end") for value in (0.0, -0.1, NAN, INF)]
    for over in bad:
        assert _tset(**over) == -22, over
