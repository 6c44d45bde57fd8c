"""Resume with the options together: a run handed on through model.state_dict(), last_optimizer.state_dict() -> optimizer_state and
continue_training_at_step is the uninterrupted run bit for bit, with the largest option sets the trainer's up-front checks allow
switched on at once — AdamW, the schedule, clipping, LAMB, the shadow, a learnable or scheduled temperature, sampled and grouped
negatives, waveform augmentation, grid masking, the grid computed ahead, use_graph.  Each option alone has a resume test of its
own; several of them share one step counter and one optimizer state dict, which is what this module is about."""
import copy
import json
import os
import random
from types import SimpleNamespace

import pytest
import torch

import test_adamw_gpu as A
import test_grid_masking_gpu as GM
import test_nan_guard_routes_gpu as R
from cpc_audio_amd.audio_model import AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.augmentation import WaveAugmentation
from cpc_audio_amd.contrastive_estimation_training import LRSchedule, NormalizedScoreFunction, TemperatureSchedule
from cpc_audio_amd.grid_masking import GridMasking
from cpc_audio_amd.scalogram_model import ScalogramResidualEncoder

pytestmark = pytest.mark.gpu

DEV = A.DEV
SCHED = LRSchedule("cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.1)
AUGMENT = WaveAugmentation(speed=0.1, time_drop=(2, 300), noise_snr_db=(10.0, 20.0), gain_db=(-3.0, 3.0), polarity=0.5, seed=21)
GROUP_IDS = [i % 3 for i in range(18)]          # three batches of small_model's six clips


def _learnable():
    return NormalizedScoreFunction(learnable=True)


SET_A = dict(weight_decay=A.WD, lr_schedule=SCHED, max_grad_norm=0.05, ema_decay=0.9, ema_warmup=True, num_negatives=2, negative_seed=7,
             negative_groups="other_files", negative_group_ids=GROUP_IDS, augmentation=AUGMENT)
GRAPH_REFUSES = ("max_grad_norm", "num_negatives", "negative_seed", "negative_groups", "negative_group_ids", "augmentation")
SET_A_GRAPHED = {k: v for k, v in SET_A.items() if k not in GRAPH_REFUSES}
SETS = {
    "A": R._cfg(attrs=SET_A, score=_learnable, loss=("cpc_nce_loss_grouped",)),
    "B": R._cfg(attrs=dict(trust_ratio=True, trust_clip=0.5, weight_decay=0.1, lr_schedule=SCHED, ema_decay=0.9, ema_warmup=True,
                           augmentation=AUGMENT, augment_targets=False),
                score=lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("cosine", 0.2, 0.05, 6))),
    "C": R._cfg(fixture="mel", reg=1.0, batchnorm=True,
                attrs=dict(weight_decay=A.WD, lr_schedule=SCHED, ema_decay=0.9, ema_warmup=True, preprocess_ahead=True, augmentation=AUGMENT,
                           grid_masking=GridMasking(freq_masks=(2, 6), time_masks=(2, 12), fill="mean", protect_last=2, seed=31))),
    "A_graph": R._cfg(attrs=SET_A_GRAPHED, score=_learnable, graph=True),
    "A_graph_options_eager": R._cfg(attrs=SET_A_GRAPHED, score=_learnable),
}


def _mel(golden_dir):
    """scalogram_model's encoder and GRU behind the small log-mel front end of tests/test_grid_masking_gpu.py."""
    g = A._load(golden_dir, "scalogram_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])

    def build(dtype):
        pre = GM._front_end("mel", meta)
        enc = ScalogramResidualEncoder(args_dict={'phase': True, 'blocks': copy.deepcopy(blocks), 'activation_register': None},
                                       preprocessing_module=pre)
        model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["E"], hidden_size=meta["H"]), enc_size=meta["E"],
                                           ar_size=meta["H"], visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype=dtype)
        model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
        return model.to(DEV), pre.to(DEV)
    return SimpleNamespace(data=torch.from_numpy(g["data"]), B=meta["B"], K=meta["K"], H=meta["H"], build=build, adamw=None)


def _fixture_of(golden_dir, cfg):
    return _mel(golden_dir) if cfg.fixture == "mel" else R._fx(golden_dir, cfg.fixture)


def _everything(run):
    """R._state plus the exported average."""
    out = R._state(run)
    if run.tr._ema is not None:
        R._flat("ema_state_dict", run.tr.ema_state_dict(), out)
    return out


_STRAIGHT = {}          # set -> the uninterrupted run, computed once and left as it is (the graphed set is compared with its eager twin)


def _straight(golden_dir, name):
    if name not in _STRAIGHT:
        cfg = SETS[name]
        fx = _fixture_of(golden_dir, cfg)
        run = R._run(fx, cfg, fx.data[:3 * fx.B], 6)
        assert run.ret is None and run.tr.training_step == 6 and run.logger.steps == list(range(6))
        _STRAIGHT[name] = (run, _everything(run))
    return _STRAIGHT[name]


@pytest.mark.parametrize("name", ["A", "B", "C", "A_graph"])
def test_resumed_run_with_the_options_together_is_the_uninterrupted_run(golden_dir, name):
    """Six steps against three, a hand-over, and three more (three batches per epoch: the second call's sampler starts where the
    second epoch does): every meter's values of the two halves concatenated, the parameters and buffers, m, v, t, the device's
    count, the shadow, its export, tstate, the trust table and the exported optimizer state, bit for bit."""
    cfg = SETS[name]
    fx = _fixture_of(golden_dir, cfg)
    data = fx.data[:3 * fx.B]
    straight, want = _straight(golden_dir, name)
    first = R._run(fx, cfg, data, 3)
    handed_on = (first.model.state_dict(), first.tr.last_optimizer.state_dict())
    second = R._run(fx, cfg, data, 3, first=3, resume=handed_on, seed=False)          # the sampler draws on: the second epoch
    assert second.tr.optimizer_state is None and second.tr.training_step == 6 and second.logger.steps == [3, 4, 5]
    whole, halves = straight.logger.meters(), (first.logger.meters(), second.logger.meters())
    assert set(whole) == set(halves[0]) == set(halves[1])
    for meter, values in whole.items():
        assert halves[0][meter] + halves[1][meter] == values, meter
    assert len(whole["loss_meter"]) == len(whole["lr_meter"]) == 6 and len(set(whole["lr_meter"])) > 3
    if "max_grad_norm" in cfg.attrs:
        assert len(whole["grad_norm_meter"]) == 6
    if second.tr._temperature is not None:
        assert len(whole["temperature_meter"]) == 6 and len(set(whole["temperature_meter"])) > 3          # ... and it moved
    got = _everything(second)
    assert R._differences(got, want) == []
    for key in ("m", "v", "t", "shadow") + (("tstate",) if second.tr._temperature is not None else ()):
        assert key in got, key
    assert got["t"] == 6
    # ... and the hand-over mattered: without the optimizer's state the second half is another run
    bare = R._run(fx, cfg, data, 3, first=3, resume=(handed_on[0], None), seed=False)
    assert "m" in R._differences(_everything(bare), want)


def test_graphed_set_follows_its_eager_twin(golden_dir):
    """Set A's options that use_graph admits, captured against eager: the bound of test_graphed_step_with_schedule_and_decay_follows_the_eager_step
    (tests/test_adamw_gpu.py), losses 1e-4 (1 + 2 i) and every parameter 1e-3 relative L2.  Between the routes only; straight against
    resumed on one route is bitwise (above)."""
    (graph, _), (eager, _) = _straight(golden_dir, "A_graph"), _straight(golden_dir, "A_graph_options_eager")
    assert "cpc_adamw_dev" in graph.names and "cpc_adamw_dev" not in eager.names and "cpc_adamw" in eager.names
    l1, l0 = graph.logger.loss_meter.values, eager.logger.loss_meter.values
    print(f"eager {l0}\ngraph {l1}")
    for i in range(6):
        assert abs(l1[i] - l0[i]) <= 1e-4 * abs(l0[i]) * (1 + 2 * i), i
    p0 = dict(eager.model.named_parameters())
    for n, p in graph.model.named_parameters():
        assert A._rel_l2(p, p0[n]) < 1e-3, (n, A._rel_l2(p, p0[n]))


def test_the_bank_stays_out_of_a_combined_run(golden_dir):
    """A resumed bank starts empty by design (it is not checkpointed; tests/test_nan_guard_routes_gpu.py, 'bank', shows the first step
    after a hand-over to be the in-batch step), and the trainer refuses it beside the selections of set A before any GPU work."""
    cfg = R._cfg(attrs=dict(SET_A, negative_bank=2), score=lambda: A.softplus_score_function)
    fx = R._fx(golden_dir, "gru")
    with pytest.raises(NotImplementedError, match="negative_bank together with num_negatives or negative_groups"):
        R._run(fx, cfg, fx.data[:3 * fx.B], 1)
