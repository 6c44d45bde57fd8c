"""Grid masking, the part that needs no GPU: the constructor's ValueErrors, the argument checks of cpc_grid_sum / cpc_grid_mask
(raised before any launch, so the pointers are never dereferenced), the host restatement GridMasking.spans (ranges, the protected
frames, determinism, independence of the waveform augmentation's fields, sharding, the time_fraction cap) and the trainer's refusals
(raised before any GPU work)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cpc_audio_amd
from cpc_audio_amd import _hip
from cpc_audio_amd.augmentation import _clip_keys, _field
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, linear_score_function
from cpc_audio_amd.grid_masking import GridMasking
from cpc_audio_amd.mel_spectrogram import MelPreprocessingModule, mel_default_dict
from cpc_audio_amd.scalogram_model import PreprocessingModule

LL = C.c_longlong
INF, NAN = float("inf"), float("nan")


def _full(seed=0, **kw):
    a = dict(freq_masks=(2, 27), time_masks=(2, 40), time_fraction=1.0, fill="zero", protect_last=0, seed=seed)
    a.update(kw)
    return GridMasking(**a)


# ------------------------------------------------------------------------------------------ public surface
def test_module_and_entry_points_are_public():
    assert "grid_masking" in cpc_audio_amd.__all__
    for name in ("cpc_grid_sum_chunks", "cpc_grid_sum", "cpc_grid_mask"):
        assert name in _hip.EXPORTED_SYMBOLS
    chunks = _hip.lib().cpc_grid_sum_chunks
    assert [chunks(n) for n in (-1, 0, 1, 4096, 4097, 322048, 2 ** 31 - 1)] == [0, 0, 1, 1, 2, 79, 524288]


# ------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw", [dict(freq_masks=(0, 5)), dict(freq_masks=(9, 5)), dict(freq_masks=(2, 0)), dict(freq_masks=(1.5, 5)),
                                dict(freq_masks=(2, 2.5)), dict(freq_masks=3), dict(freq_masks=(1, 2, 3)), dict(freq_masks=(1, 2 ** 31)),
                                dict(time_masks=(0, 5)), dict(time_masks=(9, 5)), dict(time_masks=(2, -1)), dict(time_masks="wide"),
                                dict(time_fraction=-0.1), dict(time_fraction=1.1), dict(time_fraction=NAN), dict(time_fraction="half"),
                                dict(fill="median"), dict(fill=INF), dict(fill=NAN), dict(fill=1e39), dict(fill=None), dict(fill=True),
                                dict(protect_last=-1), dict(protect_last=0.5), dict(protect_last=2 ** 31),
                                dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_constructor_refuses_out_of_range_values(kw):
    with pytest.raises(ValueError):
        GridMasking(**kw)


def test_constructor_gives_the_abi_values():
    gm = GridMasking(freq_masks=(8, 1), time_masks=(1, 1000), time_fraction=0.25, fill=-2.5, protect_last=3, seed=(1 << 64) - 1)
    cfg = gm.config(step=5, clip_offset=7, W=43)          # Wa = 40: the cap is min(1000, floor(0.25 * 40), 40)
    assert (cfg.seed, cfg.step, cfg.clip_offset, cfg.protect_last) == ((1 << 64) - 1, 5, 7, 3)
    assert (cfg.freq_count, cfg.freq_max, cfg.time_count, cfg.time_cap, cfg.fill_mode, cfg.fill_value) == (8, 1, 1, 10, 1, -2.5)
    off = GridMasking()
    cfg = off.config(0, 0, 10)
    assert (cfg.freq_count, cfg.freq_max, cfg.time_count, cfg.time_cap, cfg.fill_mode, cfg.fill_value) == (0, 0, 0, 0, 0, 0.0)
    assert GridMasking(fill="mean").config(0, 0, 10).fill_mode == 2
    with pytest.raises(ValueError, match="protect_last"):
        gm.config(0, 0, W=2)
    with pytest.raises(ValueError, match="protect_last"):
        gm.spans(0, 2, 2, 5)


def test_a_cpu_tensor_and_other_dtypes_are_refused():
    gm = _full()
    with pytest.raises(RuntimeError, match="GPU only"):
        gm(torch.zeros(2, 5, 3, 2), step=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        gm(torch.zeros(2, 5, 3, 2).permute(0, 3, 2, 1), step=0)
    for bad in (torch.zeros(2, 5, 3, 2, dtype=torch.float64), torch.zeros(2, 5, 3, 2, dtype=torch.bfloat16), torch.zeros(5, 3, 2), "grid"):
        with pytest.raises(ValueError):
            gm(bad, step=0)


# ------------------------------------------------------------------------------------------ the entry points
P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
Q = C.c_void_p(0x1000 + (1 << 30))


def _sum(**kw):
    a = dict(x=P, partial=P, B=3, n=1000, ldb=1000, Cc=2)
    a.update(kw)
    return _hip.lib().cpc_grid_sum(a["x"], a["partial"], a["B"], a["n"], LL(a["ldb"]), a["Cc"], None)


@pytest.mark.parametrize("case", [dict(x=None), dict(partial=None), dict(B=0), dict(B=65536), dict(n=0, ldb=0), dict(n=-4), dict(ldb=999),
                                  dict(Cc=0), dict(Cc=3), dict(Cc=8), dict(n=1001, ldb=1001), dict(n=1002, ldb=1002, Cc=4)],
                         ids=lambda c: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in c.items()))
def test_sum_entry_point_refuses_before_any_launch(case):
    assert _sum(**case) == -22


def _mask(cfg_null=False, **kw):
    a = dict(x=P, y=Q, partial=P, spans=None, fill=None, B=3, W=50, H=10, Cc=2, ldbx=1000, ldby=1000, seed=1, step=2, clip_offset=0,
             protect_last=5, freq_count=2, freq_max=4, time_count=2, time_cap=20, fill_mode=2, fill_value=0.0)
    a.update(kw)
    cfg = _hip.CpcGridMask(a["seed"], a["step"], a["clip_offset"], a["protect_last"], a["freq_count"], a["freq_max"], a["time_count"],
                           a["time_cap"], a["fill_mode"], a["fill_value"])
    return _hip.lib().cpc_grid_mask(a["x"], a["y"], a["partial"], a["spans"], a["fill"], a["B"], a["W"], a["H"], a["Cc"], LL(a["ldbx"]),
                                    LL(a["ldby"]), None if cfg_null else C.byref(cfg), None)


@pytest.mark.parametrize("case", [dict(x=None), dict(y=None), dict(cfg_null=True), dict(partial=None), dict(B=0), dict(B=65536),
                                  dict(W=0, protect_last=0, time_cap=0), dict(H=0), dict(W=-1), dict(H=-3),
                                  dict(W=1 << 16, H=1 << 14, ldbx=1 << 40, ldby=1 << 40),          # W H Cc = 2^31
                                  dict(Cc=0), dict(Cc=3), dict(Cc=8), dict(ldbx=999), dict(ldby=999),
                                  dict(protect_last=-1), dict(protect_last=51),
                                  dict(freq_count=-1), dict(freq_count=9), dict(time_count=-1), dict(time_count=9), dict(freq_max=-1),
                                  dict(time_cap=-1), dict(time_cap=46), dict(protect_last=50, time_cap=1),
                                  dict(fill_mode=-1), dict(fill_mode=3), dict(fill_mode=1, fill_value=INF), dict(fill_mode=1, fill_value=NAN),
                                  dict(y=C.c_void_p(0x1000 + 4 * 2999)),          # the last element of x's last clip
                                  dict(x=C.c_void_p(0x1000 + 4 * 500), y=P),
                                  dict(y=P, ldby=1004)],          # in place needs one leading dimension
                         ids=lambda c: ",".join(f"{k}={'NULL' if v is None else getattr(v, 'value', v)}" for k, v in c.items()))
def test_mask_entry_point_refuses_before_any_launch(case):
    """-22 for a NULL required pointer (partial with the mean fill), B outside [1, 65535], W or H < 1, W H Cc > 2^31 - 1, Cc not in
    {1, 2, 4}, a leading dimension below W H Cc, protect_last outside [0, W], a count outside [0, 8], freq_max < 0, time_cap outside
    [0, Wa], a fill mode outside {0, 1, 2}, a constant fill that is not finite, two different buffers whose clip ranges meet, and the
    in-place form with two leading dimensions."""
    assert _mask(**case) == -22


# ------------------------------------------------------------------------------------------ the draws
def test_spans_stay_inside_their_ranges_over_200_step_clip_pairs():
    W, H = 41, 25
    for protect_last in (0, 1, 7, 40):
        gm = _full(seed=4, freq_masks=(3, 6), time_masks=(3, 9), protect_last=protect_last)
        Wa, cap = W - protect_last, min(9, W - protect_last)
        for step in range(20):
            spans, mask = gm.spans(step, 10, W, H, clip_offset=3 * step)          # 200 (step, clip) pairs per protect_last
            assert spans.shape == (10, 32) and spans.dtype == np.int32 and mask.shape == (10, W, H) and mask.dtype == bool
            f0, fw, t0, tw = spans[:, 0:16:2], spans[:, 1:16:2], spans[:, 16::2], spans[:, 17::2]
            assert (f0 >= 0).all() and (fw >= 0).all() and (fw <= 6).all() and (f0 + fw <= H).all()
            assert (t0 >= 0).all() and (tw >= 0).all() and (tw <= cap).all() and (t0 + tw <= Wa).all()
            assert not spans[:, 6:16].any() and not spans[:, 22:].any()          # masks that are not drawn
            assert not mask[:, Wa:, :].any()
            for b in range(10):          # the mask is the union of the rectangles
                want = np.zeros((W, H), dtype=bool)
                for d in range(3):
                    want[:Wa, f0[b, d]:f0[b, d] + fw[b, d]] = True
                    want[t0[b, d]:t0[b, d] + tw[b, d], :] = True
                assert np.array_equal(mask[b], want)
    # the ends of the ranges are reached, width 0 included
    spans, _ = _full(seed=4, freq_masks=(8, 6), time_masks=(8, 9)).spans(0, 512, W, H)
    assert spans[:, 1:16:2].min() == 0 and spans[:, 1:16:2].max() == 6 and spans[:, 17::2].min() == 0 and spans[:, 17::2].max() == 9
    assert spans[:, 0:16:2].min() == 0 and spans[:, 0:16:2].max() >= H - 2 and spans[:, 16::2].max() >= W - 3
    # a maximum beyond the grid is capped by the grid
    spans, _ = _full(freq_masks=(2, 1000), time_masks=(2, 1000)).spans(1, 256, 5, 3)
    assert spans[:, 1:4:2].max() == 3 and spans[:, 17:20:2].max() == 5
    # everything protected: nothing is drawn
    spans, mask = _full(protect_last=W).spans(0, 8, W, H)
    assert not spans.any() and not mask.any()


def test_spans_are_deterministic_and_differ_between_steps_clips_and_seeds():
    gm = _full(seed=7)
    s, m = gm.spans(3, 16, 629, 256)
    s2, m2 = _full(seed=7).spans(3, 16, 629, 256)
    assert np.array_equal(s, s2) and np.array_equal(m, m2)
    assert not np.array_equal(s, gm.spans(4, 16, 629, 256)[0]) and not np.array_equal(s, _full(seed=8).spans(3, 16, 629, 256)[0])
    assert len({tuple(r) for r in s.tolist()}) == 16          # sixteen clips, sixteen draws


def test_spans_against_a_recomputation_from_the_fields():
    """The same (seed, step, clip) gives the spans recomputed here from augmentation._field at f = 0x4D41534B + j, in Python integers;
    the fields lie beyond everything the waveform augmentation draws from (f < 32 and 32 + n, n < 2^24)."""
    assert 0x4D41534B > 32 + (1 << 24)
    W, H, protect_last = 37, 24, 4
    gm = GridMasking(freq_masks=(2, 5), time_masks=(3, 30), time_fraction=0.5, protect_last=protect_last, seed=99)
    Wa = W - protect_last
    cap = min(30, (Wa * 1) // 2, Wa)
    spans, _ = gm.spans(12, 6, W, H, clip_offset=100)
    kb = _clip_keys(99, 12, np.arange(100, 106, dtype=np.uint64))

    def draw(j, lo, hi):
        u = [int(v) for v in _field(kb, 0x4D41534B + j)]
        return [lo_ + ((u_ * (hi_ - lo_ + 1)) >> 32) for u_, lo_, hi_ in zip(u, lo, hi)]

    for d in range(2):
        w = draw(2 * d, [0] * 6, [min(5, H)] * 6)
        f0 = draw(2 * d + 1, [0] * 6, [H - w_ for w_ in w])
        assert spans[:, 2 * d].tolist() == f0 and spans[:, 2 * d + 1].tolist() == w
    for d in range(3):
        w = draw(16 + 2 * d, [0] * 6, [cap] * 6)
        t0 = draw(17 + 2 * d, [0] * 6, [Wa - w_ for w_ in w])
        assert spans[:, 16 + 2 * d].tolist() == t0 and spans[:, 17 + 2 * d].tolist() == w


def test_a_shard_draws_what_the_whole_batch_draws():
    gm, B, k = _full(seed=3, fill="mean"), 6, 5
    whole_s, whole_m = gm.spans(9, k + B, 130, 80)
    shard_s, shard_m = gm.spans(9, B, 130, 80, clip_offset=k)
    assert np.array_equal(shard_s, whole_s[k:k + B]) and np.array_equal(shard_m, whole_m[k:k + B])


def test_time_fraction_caps_the_time_masks():
    W = 100
    for fraction, protect_last, want in ((1.0, 0, 40), (0.25, 0, 25), (0.25, 20, 20), (0.0, 0, 0), (0.999, 99, 0), (1.0, 70, 30)):
        gm = _full(time_masks=(8, 40), time_fraction=fraction, protect_last=protect_last)
        assert gm.time_cap(W) == want == min(40, int(np.floor(fraction * (W - protect_last))), W - protect_last)
        widths = gm.spans(0, 256, W, 8)[0][:, 17::2]
        assert widths.max() == want and widths.min() == 0
    assert GridMasking(freq_masks=(1, 3)).time_cap(W) == 0


# ------------------------------------------------------------------------------------------ refusals of the trainer
def _tiny_model():
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    return AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                      prediction_steps=2)


class _NoDataset:
    def __len__(self):
        return 24

    def get_example_count_per_file(self):
        raise AssertionError("train() went past its up-front checks")


def _trainer(**kw):
    tr = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=_NoDataset(), device="cpu", file_batch_size=2, **kw)
    tr.verbose = False
    return tr


def test_trainer_refusals_come_before_any_device_use():
    grid_pre = MelPreprocessingModule(dict(mel_default_dict, n_fft=256, win_length=256, hop_length=32, n_mels=24), delta=True)
    tr = _trainer(preprocessing=grid_pre)
    assert tr.grid_masking is None and tr._check_grid_masking() is None
    # 1. anything but a GridMasking
    for bad in (True, 0.1, "mask", dict(freq_masks=(2, 27)), GridMasking):
        tr.grid_masking = bad
        with pytest.raises(TypeError, match="GridMasking"):
            tr.train(batch_size=8, epochs=1, max_steps=1)
    # 2. no grid: no preprocessing module, or one that hands the waveform on
    for pre in (None, torch.nn.Identity(), PreprocessingModule(), MelPreprocessingModule()):
        t2 = _trainer(preprocessing=pre)
        t2.grid_masking = _full()
        with pytest.raises(ValueError, match="grid"):
            t2.train(batch_size=8, epochs=1, max_steps=1)
    # 3. a captured step
    tr.grid_masking = _full()
    tr.use_graph = True
    with pytest.raises(NotImplementedError, match="use_graph"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.use_graph = False
    # 4. the gradient penalty
    t4 = _trainer(preprocessing=grid_pre, wasserstein_gradient_penalty=True, score_function=linear_score_function)
    t4.grid_masking = _full()
    with pytest.raises(NotImplementedError, match="wasserstein_gradient_penalty"):
        t4.train(batch_size=8, epochs=1, max_steps=1)
    # what is covered passes the checks (and only then reaches the dataset)
    with pytest.raises(AssertionError, match="up-front"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    assert tr._check_grid_masking() is tr.grid_masking
