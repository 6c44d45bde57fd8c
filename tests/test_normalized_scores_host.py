"""Cosine-similarity scores with a temperature (score kind "normalized", NormalizedScoreFunction): everything that is decided on the
host — the argument checks of cpc_norm_rows / cpc_norm_rows_bwd (refused with -22 before any launch, so the library alone is enough),
the score kind and its temperature keyword, the public callable's refusals and the trainer's route predicates.  No GPU needed."""
import ctypes as C
import inspect

import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction,
                                                           softplus_score_function)
from cpc_audio_amd import engine
from cpc_audio_amd.engine import SCORE_KINDS, check_temperature, score_kind

L_ = C.c_longlong
P, NULL, S = C.c_void_p(0x1000), None, C.c_void_p(0)
GOOD = dict(rows=4, E=64, rpi=0, item=0, ld=64, scale=10.0, eps=1e-8, dtype=_hip.F32)


def _call(name, a=P, b=P, c=P, **over):
    k = dict(GOOD, **over)
    return getattr(_hip.lib(), name)(a, b, c, k["rows"], k["E"], k["rpi"], L_(k["item"]), L_(k["ld"]), k["scale"], k["eps"], k["dtype"], S)


BAD = [dict(rows=0), dict(rows=-3), dict(E=0), dict(E=4097), dict(rpi=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
       dict(scale=float("inf")), dict(eps=0.0), dict(eps=-1e-8), dict(eps=float("nan")), dict(eps=float("inf")), dict(dtype=2),
       dict(dtype=-1)]


@pytest.mark.parametrize("name", ["cpc_norm_rows", "cpc_norm_rows_bwd"])
def test_norm_rows_argument_checks_without_a_gpu(name):
    """-22 before any launch for each argument check of both entry points: a NULL pointer in every position, rows < 1, E outside
    [1, 4096], rpi < 0, scale or eps not finite and > 0, an unknown dtype."""
    for over in BAD:
        assert _call(name, **over) == -22, over
    assert _call(name, a=NULL) == -22 and _call(name, b=NULL) == -22 and _call(name, c=NULL) == -22


def test_score_kind_and_temperature_pairing():
    assert "normalized" in SCORE_KINDS and score_kind(False, "normalized") == "normalized" and score_kind(True, "normalized") == "normalized"
    with pytest.raises(ValueError):
        score_kind(False, "cosine")
    assert check_temperature(0.1, "normalized") == pytest.approx(0.1) and check_temperature(None, "linear") is None
    with pytest.raises(ValueError, match="needs a temperature"):
        check_temperature(None, "normalized")
    for kind in ("softplus", "linear", "difference"):
        with pytest.raises(ValueError, match="temperature belongs"):
            check_temperature(0.1, kind)
    for bad in (0, -1, float("nan"), float("inf"), "warm"):
        with pytest.raises(ValueError):
            check_temperature(bad, "normalized")


def test_every_loss_entry_of_the_engine_takes_the_temperature():
    """temperature=None sits next to score= on the five surfaces, and each checks the pairing before it touches the device."""
    from cpc_audio_amd.scalogram_engine import ScalogramCPCEngine
    for fn in (engine.CPCEngine.nce_forward_backward, engine.CPCEngine.nce_all_forward_backward, engine.CPCEngine.nce_eval,
               engine.CPCEngine.loss_and_grads, ScalogramCPCEngine.loss_and_grads, engine.GraphedStep.__init__):
        sig = inspect.signature(fn).parameters
        assert "score" in sig and sig["temperature"].default is None, fn
    blank = object.__new__(engine.CPCEngine)          # the checks run before any attribute of the engine is read
    with pytest.raises(ValueError, match="needs a temperature"):
        blank.loss_and_grads(None, False, 0.5, score="normalized")
    with pytest.raises(ValueError, match="temperature belongs"):
        blank.loss_and_grads(None, True, 0.5, temperature=0.1)
    with pytest.raises(ValueError, match="needs a temperature"):
        blank.nce_forward_backward(False, 0.5, score="normalized")
    with pytest.raises(ValueError, match="temperature belongs"):
        blank.nce_all_forward_backward(False, 0.5, score="difference", temperature=1.0)
    with pytest.raises(ValueError, match="needs a temperature"):
        blank.nce_eval(False, False, None, None, score="normalized")
    with pytest.raises(ValueError, match="temperature belongs"):
        engine.GraphedStep(None, None, True, 0.5, temperature=0.1)
    with pytest.raises(ValueError):
        blank.loss_and_grads(None, False, 0.5, score="normalized", temperature=0.0)


def test_normalized_score_function_refusals():
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            NormalizedScoreFunction(bad)
    assert NormalizedScoreFunction().temperature == pytest.approx(0.1)
    assert NormalizedScoreFunction(2).temperature == 2.0
    with pytest.raises(RuntimeError, match="GPU only"):
        NormalizedScoreFunction(0.1)(torch.randn(2, 2, 4), torch.randn(2, 4, 2))


def _tiny_model():
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    return AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                      prediction_steps=2)


def test_trainer_predicates():
    model = _tiny_model()
    fn = NormalizedScoreFunction(0.25)
    tr = ContrastiveEstimationTrainer(model=model, dataset=None, score_function=fn)
    assert tr._engine_normalized() and not tr._fused() and not tr._engine_difference()
    assert tr._score_kind() == "normalized" and tr._score_kw() == {"score": "normalized", "temperature": 0.25}
    tr.global_negatives = True
    assert not tr._engine_normalized()
    tr.global_negatives = False
    tr.optimizer = torch.optim.SGD
    assert not tr._engine_normalized()
    with pytest.raises(NotImplementedError):
        ContrastiveEstimationTrainer(model=model, dataset=None, score_function=fn, preprocessing=lambda x: x,
                                     wasserstein_gradient_penalty=True)
    # the presets keep their kinds and carry no temperature
    tr2 = ContrastiveEstimationTrainer(model=model, dataset=None, score_function=softplus_score_function)
    assert tr2._fused() and not tr2._engine_normalized() and tr2._score_kw() == {"score": "softplus"}
