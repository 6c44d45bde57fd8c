"""Waveform augmentation, the part that needs no GPU: the host restatements WaveAugmentation.parameters / .noise (determinism, ranges,
sharding, the protected tail), the generator's moments, the Catmull-Rom weights, the argument checks of cpc_wave_power /
cpc_wave_augment (raised before any launch, so the pointers are never dereferenced), the constructor's ValueErrors, the trainer's
refusals (raised before any GPU work) and the float64 reference of tests/augmentation_reference.py against its own definition."""
import ctypes as C

import numpy as np
import pytest
import torch

import cpc_audio_amd
from cpc_audio_amd import _hip
from cpc_audio_amd.augmentation import WaveAugmentation
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer

import augmentation_reference as R

LL = C.c_longlong


def _full(seed=0):
    return WaveAugmentation(speed=0.25, time_drop=(3, 400), noise_snr_db=(5.0, 20.0), gain_db=(-6.0, 3.0), polarity=0.5, seed=seed)


def _same(p, q):
    return all(np.array_equal(p[k], q[k], equal_nan=True) for k in p)


# ------------------------------------------------------------------------------------------ the draws
def test_module_is_public():
    assert "augmentation" in cpc_audio_amd.__all__


def test_parameters_are_deterministic_and_differ_between_steps_clips_and_seeds():
    aug = _full(seed=7)
    p = aug.parameters(3, 16, 8000)
    assert _same(p, _full(seed=7).parameters(3, 16, 8000))
    assert set(p) == {"q", "snr_db", "gain_db", "flip", "drop_start", "drop_len"}
    assert p["q"].shape == (16,) and p["drop_start"].shape == (16, 3) and p["drop_len"].shape == (16, 3)
    for other in (aug.parameters(4, 16, 8000), _full(seed=8).parameters(3, 16, 8000)):
        for k in ("q", "snr_db", "gain_db", "drop_start", "drop_len"):
            assert not np.array_equal(p[k], other[k]), k
    for k in ("q", "snr_db", "gain_db"):
        assert len(set(p[k].tolist())) == 16, k          # sixteen clips, sixteen values
    assert 0 < p["flip"].sum() < 16


def test_every_draw_is_inside_its_range():
    aug = _full(seed=1)
    assert (aug.q_lo, aug.q_hi) == (49152, 81920)
    for a in (None, 1, 7, 399, 400, 5000):
        p = aug.parameters(11, 512, 8000, protect_from=a)
        a = 8000 if a is None else a
        assert p["q"].min() >= aug.q_lo and p["q"].max() <= aug.q_hi
        assert p["snr_db"].min() >= 5.0 and p["snr_db"].max() <= 20.0
        assert p["gain_db"].min() >= -6.0 and p["gain_db"].max() <= 3.0
        assert p["drop_len"].min() >= 1 and p["drop_len"].max() <= min(400, a)
        assert p["drop_start"].min() >= 0 and (p["drop_start"] + p["drop_len"]).max() <= a          # the spans lie inside [0, a)
    p = aug.parameters(11, 4096, 8000)          # the ends of the integer ranges are reached
    assert p["drop_len"].min() == 1 and p["drop_len"].max() == 400
    assert p["q"].min() < aug.q_lo + 64 and p["q"].max() > aug.q_hi - 64
    assert abs(p["flip"].mean() - 0.5) < 0.05
    assert not WaveAugmentation(polarity=0.0).parameters(0, 64, 100)["flip"].any()
    assert WaveAugmentation(polarity=1.0).parameters(0, 64, 100)["flip"].all()


def test_a_shard_draws_what_the_whole_batch_draws():
    aug, B = _full(seed=3), 6
    whole = aug.parameters(9, 2 * B, 5000)
    shard = aug.parameters(9, B, 5000, clip_offset=B)
    assert all(np.array_equal(shard[k], whole[k][B:]) for k in whole)


def test_protect_from_zero_yields_no_stage():
    p = _full().parameters(2, 8, 5000, protect_from=0)
    assert (p["q"] == 65536).all() and not p["flip"].any() and not p["drop_len"].any() and not p["drop_start"].any()
    assert np.isnan(p["snr_db"]).all() and np.isnan(p["gain_db"]).all()
    off = WaveAugmentation().parameters(2, 8, 5000)
    assert (off["q"] == 65536).all() and not off["flip"].any() and off["drop_len"].shape == (8, 0)
    for bad in (-1, 5001):
        with pytest.raises(ValueError, match="protect_from"):
            _full().parameters(2, 8, 5000, protect_from=bad)


def test_noise_generator_moments():
    """|mean| < 0.01 and variance within 1 % of 1 over 10^6 samples; the range is the four-fold sum's; other clips and steps differ."""
    aug = WaveAugmentation(noise_snr_db=(10.0, 10.0), seed=5)
    g = aug.noise(step=4, clip=2, n0=0, n1=10 ** 6)
    assert g.shape == (10 ** 6,) and g.dtype == np.float64
    assert abs(g.mean()) < 0.01 and abs(g.var() - 1.0) < 0.01
    assert np.abs(g).max() <= 131070 * np.sqrt(3.0) / 65536 and np.abs(g).max() > 3.0
    assert abs(np.corrcoef(g[:-1], g[1:])[0, 1]) < 0.01
    assert np.array_equal(g[100:200], aug.noise(4, 2, 100, 200))
    assert not np.array_equal(g[:100], aug.noise(4, 3, 0, 100)) and not np.array_equal(g[:100], aug.noise(5, 2, 0, 100))


def test_catmull_rom_weights_sum_to_one_at_all_fractions():
    t = np.arange(65536, dtype=np.float64) / 65536.0
    w, f = R.catmull_rom(t), R.catmull_rom_factored(t)
    assert np.abs(sum(w) - 1.0).max() < 1e-15 and np.abs(sum(f) - 1.0).max() < 1e-15
    assert max(np.abs(a - b).max() for a, b in zip(w, f)) < 1e-15          # the kernel's factored forms are the same polynomials
    assert sum(np.abs(x) for x in w).max() <= 1.25
    assert [float(x[0]) for x in w] == [0.0, 1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------ the reference against its definition
def test_reference_against_its_definition():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(50)
    y, mag = R.augment(x, 50)
    assert np.array_equal(y, x) and np.array_equal(mag, np.abs(x))
    # rate 1 through the interpolator is the identity; a ramp is reproduced exactly by the cubic (away from the zero-extended ends)
    v, _ = R.resample(x, 50, 65536)
    assert np.array_equal(v, x)
    ramp = np.arange(200, dtype=np.float64)
    a, q = 150, 70000
    v, _ = R.resample(ramp, a, q)
    want = a - (a - np.arange(a)) * q / 65536.0
    inside = (want >= 1) & (want <= 197)
    assert np.abs(v[inside] - want[inside]).max() < 1e-10
    # q > 1 reads in front of the clip: the head is the zero extension
    assert want[0] < -2 and v[0] == 0.0
    # drop, noise and gain in the stated order
    g = rng.standard_normal(40)
    y, mag = R.augment(x, 40, drops=[(5, 3), (6, 10)], sigma=0.5, g=g, gain=-2.0)
    assert np.array_equal(y[40:], x[40:]) and not mag[40:].any()
    assert np.allclose(y[5:16], -2.0 * 0.5 * g[5:16], rtol=0, atol=1e-15) and np.allclose(mag[5:16], 0.5 * np.abs(g[5:16]))
    assert np.allclose(y[:5], -2.0 * (x[:5] + 0.5 * g[:5]), rtol=0, atol=1e-15)
    assert np.allclose(R.power_partials(x, 37), [np.sum(x[:37] ** 2)])
    assert R.power_partials(np.ones(10000), 8193).tolist() == [4096.0, 4096.0, 1.0]


# ------------------------------------------------------------------------------------------ the entry points
def test_entry_points_are_exported():
    for name in ("cpc_wave_power_chunks", "cpc_wave_power", "cpc_wave_augment"):
        assert name in _hip.EXPORTED_SYMBOLS
    chunks = _hip.lib().cpc_wave_power_chunks
    assert [chunks(n) for n in (-1, 0, 1, 4096, 4097, 20480, 1 << 24)] == [0, 0, 1, 1, 2, 5, 4096]


P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
INF, NAN = float("inf"), float("nan")


def _power(**kw):
    a = dict(x=P, partial=P, B=3, L=1000, ldx=1000, n=1000)
    a.update(kw)
    return _hip.lib().cpc_wave_power(a["x"], a["partial"], a["B"], a["L"], LL(a["ldx"]), a["n"], None)


@pytest.mark.parametrize("case", [dict(x=None), dict(partial=None), dict(B=0), dict(B=65536), dict(L=0, ldx=0, n=0), dict(L=(1 << 24) + 1, ldx=1 << 25),
                                  dict(ldx=999), dict(n=0), dict(n=-1), dict(n=1001)],
                         ids=lambda c: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in c.items()))
def test_power_entry_point_refuses_before_any_launch(case):
    assert _power(**case) == -22


def _augment(cfg_null=False, **kw):
    a = dict(x=P, y=P, partial=P, params=P, B=3, L=1000, ldx=1000, ldy=1000, seed=1, step=2, clip_offset=0, protect_from=1000,
             q_lo=60000, q_hi=70000, drop_count=2, drop_max_len=50, noise_on=1, snr_lo=5.0, snr_hi=20.0, gain_on=1, gain_lo_db=-6.0,
             gain_hi_db=3.0, polarity_threshold=1 << 31)
    a.update(kw)
    cfg = _hip.CpcWaveAugment(a["seed"], a["step"], a["clip_offset"], a["protect_from"], a["q_lo"], a["q_hi"], a["drop_count"],
                              a["drop_max_len"], a["noise_on"], a["snr_lo"], a["snr_hi"], a["gain_on"], a["gain_lo_db"], a["gain_hi_db"],
                              a["polarity_threshold"])
    return _hip.lib().cpc_wave_augment(a["x"], a["y"], a["partial"], a["params"], a["B"], a["L"], LL(a["ldx"]), LL(a["ldy"]),
                                       None if cfg_null else C.byref(cfg), None)


@pytest.mark.parametrize("case", [dict(x=None), dict(y=None), dict(partial=None), dict(cfg_null=True), dict(B=0), dict(B=65536),
                                  dict(L=0, ldx=0, ldy=0, protect_from=0), dict(L=(1 << 24) + 1, ldx=1 << 25, ldy=1 << 25),
                                  dict(ldx=999), dict(ldy=999), dict(protect_from=-1), dict(protect_from=1001),
                                  dict(q_lo=32767), dict(q_hi=131073), dict(q_lo=70001), dict(q_lo=65536, q_hi=65535),
                                  dict(drop_count=-1), dict(drop_count=9), dict(drop_max_len=0), dict(drop_max_len=-5),
                                  dict(snr_lo=21.0), dict(snr_lo=NAN), dict(snr_hi=INF), dict(snr_lo=-INF),
                                  dict(gain_lo_db=4.0), dict(gain_lo_db=NAN), dict(gain_hi_db=INF), dict(gain_hi_db=NAN),
                                  dict(polarity_threshold=(1 << 32) + 1)],
                         ids=lambda c: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in c.items()))
def test_augment_entry_point_refuses_before_any_launch(case):
    """-22 for a NULL required pointer (partial with the noise on), B outside [1, 65535], L outside [1, 2^24], a leading dimension
    below L, protect_from outside [0, L], a rate outside 32768 <= q_lo <= q_hi <= 131072, drop_count outside [0, 8], drop_max_len < 1
    with spans to draw, lo > hi or a dB value that is not finite, a polarity threshold above 2^32."""
    assert _augment(**case) == -22


# ------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw", [dict(speed=0.0), dict(speed=-0.1), dict(speed=0.51), dict(speed=float("nan")),
                                dict(time_drop=(0, 10)), dict(time_drop=(9, 10)), dict(time_drop=(2, 0)), dict(time_drop=(1.5, 10)),
                                dict(time_drop=3), dict(time_drop=(1, 2, 3)),
                                dict(noise_snr_db=(20.0, 5.0)), dict(noise_snr_db=(5.0, float("inf"))), dict(noise_snr_db=10.0),
                                dict(gain_db=(3.0, -3.0)), dict(gain_db=(float("nan"), 0.0)), dict(gain_db="loud"),
                                dict(polarity=-0.1), dict(polarity=1.1), dict(polarity=float("nan")),
                                dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_constructor_refuses_out_of_range_values(kw):
    with pytest.raises(ValueError):
        WaveAugmentation(**kw)


def test_constructor_rounds_to_the_abi_values():
    aug = WaveAugmentation(speed=0.1, time_drop=(8, 1), noise_snr_db=(0, 0), gain_db=(-3, -3), polarity=1.0, seed=(1 << 64) - 1)
    assert (aug.q_lo, aug.q_hi) == (58982, 72090) and aug.polarity_threshold == 1 << 32 and aug.speed_on and aug.noise_on
    cfg = aug.config(step=5, clip_offset=7, protect_from=9)
    assert (cfg.seed, cfg.step, cfg.clip_offset, cfg.protect_from, cfg.drop_count, cfg.drop_max_len) == ((1 << 64) - 1, 5, 7, 9, 8, 1)
    assert (cfg.noise_on, cfg.gain_on, cfg.gain_lo_db, cfg.polarity_threshold) == (1, 1, -3.0, 1 << 32)
    off = WaveAugmentation()
    assert not off.speed_on and not off.noise_on and off.polarity_threshold == 0 and off.config(0, 0, 0).gain_on == 0
    with pytest.raises(RuntimeError, match="GPU only"):
        off(torch.zeros(2, 10), step=0)
    with pytest.raises(ValueError):
        off(torch.zeros(2, 10, dtype=torch.float64), step=0)


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
    tr = _trainer()
    assert tr.augmentation is None and tr.augment_targets is True and tr._check_augmentation() is None
    for bad in (True, 0.1, "speed", dict(speed=0.1), WaveAugmentation):
        tr.augmentation = bad
        with pytest.raises(TypeError, match="WaveAugmentation"):
            tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.augmentation = WaveAugmentation(polarity=0.5)
    tr.use_graph = True
    with pytest.raises(NotImplementedError, match="use_graph"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.use_graph = False
    # the past only: needs the encoder's own frame geometry, which a preprocessing module in front of it hides
    tr2 = _trainer(preprocessing=torch.nn.Identity())
    tr2.augmentation, tr2.augment_targets = WaveAugmentation(polarity=0.5), False
    with pytest.raises(ValueError, match="augment_targets"):
        tr2.train(batch_size=8, epochs=1, max_steps=1)
    # what is covered passes the checks (and only then reaches the dataset)
    with pytest.raises(AssertionError, match="up-front"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    aug, protect = tr._check_augmentation()
    assert aug is tr.augmentation and protect(5000) is None
    tr.augment_targets = False
    aug, protect = tr._check_augmentation()
    enc = tr.model.encoder
    field, hop = int(enc.receptive_field), int(enc.downsampling_factor)
    assert (field, hop) == (465, 160)
    L = tr.model.item_length          # 4 + 2 hops behind one receptive field: 7 frames, the last 2 of them targets
    assert L == field + 6 * hop
    assert protect(L) == hop * 5 and protect(L + hop - 1) == hop * 5 and protect(L + hop) == hop * 6
    with pytest.raises(ValueError, match="target frames"):
        protect(field + hop)          # 2 frames: nothing in front of the targets
