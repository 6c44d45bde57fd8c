"""Waveform augmentation on the HIP path: cpc_wave_power against float64 at the bound of its own summation order, the identity, the
drawn parameters against WaveAugmentation.parameters(), every stage alone and all together against the float64 reference of
tests/augmentation_reference.py fed with the device's own scalars, the protected tail, addressing, determinism and sharding, and the
trainer on the small model: nothing changes without an augmentation, and with one the engine receives aug(batch, step) bit for bit."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.augmentation import WaveAugmentation
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,
                                                           softplus_score_function)

import augmentation_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LL = C.c_longlong
SENTINEL = -8192.0
NEW_ENTRY_POINTS = {"cpc_wave_power", "cpc_wave_augment"}
EPS = 2.0 ** -24

# ------------------------------------------------------------------------------------------ the bounds
# cpc_wave_power (csrc/augment.hip, wave_power_kernel): roundings on the longest path from one element to its partial sum
#   16     a thread's chain s = fma(x, x, s) over its 4 pieces of 4 floats (the square itself is not rounded)
#   6      the xor-shuffle butterfly over the 64 lanes
#   2      (w0 + w1) + (w2 + w3) over the four waves
# Every term is a square, so a partial's relative error is at most 24 * 2^-24 (to first order).
POWER_ROUNDINGS = 16 + 6 + 2
# cpc_wave_augment (wave_augment_kernel): roundings between the stored samples and one output, each relative to a quantity of at most
# mag = sum_j |w_j x[i + j]| + sigma |g| (times |gain| behind the gain)
#   2      a Catmull-Rom weight in its factored form (t and u = 1 - t are exact; two rounded products, or one fma and one product)
#   4      v = w_-1 x_-1 (a product) and three fmas, each rounding a partial sum whose magnitude is at most sum_j |w_j x[i + j]|
#   2      g = float(s - 131070) * float(sqrt(3) / 65536): the constant's own rounding and the product's, relative to sigma |g|
#   1      v = fma(sigma, g, v)
#   1      v * gain
# 10 to first order; one more covers the second-order terms.  (Without the speed stage the first six do not occur; the bound stays.)
SAMPLE_ROUNDINGS = 2 + 4 + 2 + 1 + 1 + 1
# sigma, the gain and the mean square against the float64 restatement: the device's exp2f and sqrtf are not ours to derive, so this is
# 4 x the worst relative difference seen on the MI355X over this file's cases (test_drawn_parameters prints them: sigma 2.44e-7,
# gain 1.01e-7, mean square 9.1e-8), and never above 1e-5.
PARAM_RTOL = 4 * 2.44e-7


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _clips(B, L, ldx=None, seed=0, rows_before=0, rows_after=0):
    """(x view (B, L), the whole buffer): random clips of amplitude 0.3 with NaN in the padding behind every row and in whole rows
    before and after, so that a read outside the clips poisons what it feeds."""
    ldx = L if ldx is None else ldx
    whole = torch.full((B + rows_before + rows_after, ldx), float("nan"), dtype=torch.float32)
    data = torch.randn(B, L, generator=torch.Generator().manual_seed(seed * 1000 + L)) * 0.3
    whole[rows_before:rows_before + B, :L] = data
    whole = whole.to(DEV)
    return whole[rows_before:rows_before + B, :L], whole


def _out(B, L, ldy=None, rows=1):
    ldy = L if ldy is None else ldy
    whole = torch.full((B + 2 * rows, ldy), SENTINEL, device=DEV, dtype=torch.float32)
    return whole[rows:rows + B, :L], whole


def _out_intact(whole, B, L, rows=1):
    return bool((whole[:rows] == SENTINEL).all() and (whole[rows + B:] == SENTINEL).all() and (whole[rows:rows + B, L:] == SENTINEL).all())


def _run(aug, x, step, a=None, clip_offset=0, out=None):
    """(y, params as float32 numpy (B, 8))."""
    params = torch.full((x.shape[0], 8), SENTINEL, device=DEV, dtype=torch.float32)
    y = aug(x, step, clip_offset=clip_offset, protect_from=a, out=out, params_out=params)
    torch.cuda.synchronize()
    return y, params.cpu().numpy()


def _check_against_reference(aug, x, y, params, step, a, what, clip_offset=0):
    """Every output against the float64 reference fed with the device's own q, sigma and gain (params_out), the spans of parameters()
    (which test_drawn_parameters holds params_out to) and the host's noise variates: |y - ref| <= SAMPLE_ROUNDINGS 2^-24 |gain| mag."""
    B, L = x.shape
    a = L if a is None else a
    host = aug.parameters(step, B, L, clip_offset=clip_offset, protect_from=a)
    xs, ys = x.cpu().double().numpy(), y.cpu().double().numpy()
    worst = 0.0
    for b in range(B):
        q, sigma, gain = int(params[b, 0]), float(params[b, 1]), float(params[b, 2])
        assert q == host["q"][b]
        drops = list(zip(host["drop_start"][b].tolist(), host["drop_len"][b].tolist())) if a > 0 else []
        g = aug.noise(step, clip_offset + b, 0, a) if aug.noise_on and a > 0 else None
        ref, mag = R.augment(xs[b], a, q, drops, sigma, g, gain)
        bound = SAMPLE_ROUNDINGS * EPS * abs(gain) * mag
        err = np.abs(ys[b] - ref)
        assert np.array_equal(ys[b, a:], xs[b, a:])
        ratio = (err[:a] / np.maximum(bound[:a], 1e-300)).max() if a > 0 else 0.0
        worst = max(worst, ratio * SAMPLE_ROUNDINGS)
        assert (err <= bound).all(), (what, b, int(np.argmax(err - bound)), float((err - bound).max()))
    print(f"{what} B={B} L={L} a={a}: worst error {worst:.2f} x 2^-24 |gain| mag (bound {SAMPLE_ROUNDINGS})")


# ------------------------------------------------------------------------------------------ 1. the power pass
@pytest.mark.parametrize("L", [1, 5, 4096, 4097, 10000])
def test_power_against_float64(L):
    assert POWER_ROUNDINGS * EPS < 2e-6
    B = 3
    for ldx in (L, L + 3):                                   # rows 16-byte aligned (where L allows) and not
        for n in sorted({L, max(1, L - 1), max(1, L // 2 + 1)}):
            x, whole = _clips(B, L, ldx, seed=n, rows_before=1, rows_after=1)
            x[:, n:] = 1e3                                    # valid samples behind n take no part
            before = _bits(whole).clone()
            chunks = _hip.lib().cpc_wave_power_chunks(n)
            assert chunks == -(-n // 4096)
            partial = torch.full((B * chunks + 8,), SENTINEL, device=DEV, dtype=torch.float32)
            _hip.call("cpc_wave_power", _hip.ptr(x), _hip.ptr(partial), B, L, LL(ldx), n)
            torch.cuda.synchronize()
            assert torch.equal(_bits(whole), before) and bool((partial[B * chunks:] == SENTINEL).all())
            got = partial[:B * chunks].cpu().double().numpy().reshape(B, chunks)
            xs = x.cpu().numpy()
            for b in range(B):
                ref = R.power_partials(xs[b], n)
                rel = np.abs(got[b] - ref) / ref
                print(f"cpc_wave_power L={L} ldx={ldx} n={n} clip {b}: rel {rel.max():.3e} (bound {POWER_ROUNDINGS * EPS:.3e})")
                assert (rel <= POWER_ROUNDINGS * EPS).all(), (L, ldx, n, b, rel)


# ------------------------------------------------------------------------------------------ 2. the identity
@pytest.mark.parametrize("L,ldx", [(1001, 1003), (1000, 1000), (3, 3), (4100, 4101)])
def test_all_stages_off_is_the_identity(L, ldx):
    x, whole = _clips(3, L, ldx)
    x[0, 0], x[1, L - 1], x[2, L // 2] = -0.0, -0.0, float("inf")
    whole.view(torch.int32)[2, 0] = 0x7FC12345               # a NaN with a payload
    with _Spy() as spy:
        y, params = _run(WaveAugmentation(), x, step=3)
    assert spy.names == ["cpc_wave_augment"]                  # no power pass without the noise
    assert _same_bits(y, x)
    assert params[:, 0].tolist() == [65536.0] * 3 and not params[:, 1].any() and params[:, 2].tolist() == [1.0] * 3
    assert not params[:, 3:].any()


# ------------------------------------------------------------------------------------------ 3. what the device drew
def _stage(name, seed=11):
    kw = {"speed": dict(speed=0.25), "drop": dict(time_drop=(3, 200)), "noise": dict(noise_snr_db=(5.0, 25.0)),
          "gain": dict(gain_db=(-12.0, 6.0)), "polarity": dict(polarity=0.5),
          "all": dict(speed=0.25, time_drop=(8, 200), noise_snr_db=(5.0, 25.0), gain_db=(-12.0, 6.0), polarity=0.5)}[name]
    return WaveAugmentation(seed=seed, **kw)


def test_drawn_parameters():
    """params_out against parameters(): q and the first two spans exactly; sigma, the signed gain and the mean square within
    PARAM_RTOL of the float64 restatement sqrt(mean(x^2)) 10^(-snr_db / 20), +-10^(gain_db / 20), mean(x^2)."""
    worst = {"sigma": 0.0, "gain": 0.0, "power": 0.0}
    for L, a in [(3, None), (7, 5), (1000, None), (1001, 700), (4100, None), (10000, 9999)]:
        for step in (0, 6):
            aug = _stage("all", seed=L)
            x, _ = _clips(3, L, L + 1, seed=step)
            y, params = _run(aug, x, step, a=a, clip_offset=40)
            aa = L if a is None else a
            host = aug.parameters(step, 3, L, clip_offset=40, protect_from=a)
            xs = x.cpu().double().numpy()
            assert params[:, 0].tolist() == host["q"].tolist()
            assert params[:, 4].tolist() == host["drop_start"][:, 0].tolist() and params[:, 5].tolist() == host["drop_len"][:, 0].tolist()
            assert params[:, 6].tolist() == host["drop_start"][:, 1].tolist() and params[:, 7].tolist() == host["drop_len"][:, 1].tolist()
            for b in range(3):
                power = float(np.mean(xs[b, :aa] ** 2))
                sigma = math.sqrt(power) * 10.0 ** (-host["snr_db"][b] / 20.0)
                gain = (-1.0 if host["flip"][b] else 1.0) * 10.0 ** (host["gain_db"][b] / 20.0)
                rel = {"sigma": abs(params[b, 1] - sigma) / sigma, "gain": abs(params[b, 2] - gain) / abs(gain),
                       "power": abs(params[b, 3] - power) / power}
                for k, v in rel.items():
                    worst[k] = max(worst[k], v)
                assert (params[b, 2] < 0) == bool(host["flip"][b])
    print("params_out against the float64 restatement, worst relative difference: "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f" (PARAM_RTOL {PARAM_RTOL:.3e})")
    assert PARAM_RTOL <= 1e-5
    assert max(worst.values()) <= PARAM_RTOL, worst
    # a single span and no noise: the second pair, sigma and the mean square stay 0; the gain is +-1 without the gain stage
    aug = WaveAugmentation(time_drop=(1, 50), polarity=0.5, seed=2)
    x, _ = _clips(4, 300)
    _, params = _run(aug, x, 1)
    host = aug.parameters(1, 4, 300)
    assert not params[:, 1].any() and not params[:, 3].any() and not params[:, 6:].any()
    assert params[:, 2].tolist() == [-1.0 if f else 1.0 for f in host["flip"]]
    assert params[:, 4].tolist() == host["drop_start"][:, 0].tolist() and params[:, 5].tolist() == host["drop_len"][:, 0].tolist()


# ------------------------------------------------------------------------------------------ 4. the stages
@pytest.mark.parametrize("L", [3, 7, 1000, 1001, 4100])
@pytest.mark.parametrize("stage", ["speed", "drop", "noise", "gain", "polarity", "all"])
def test_stage_against_reference(stage, L):
    B, step = 3, 4
    aug = _stage(stage, seed=L + 1)
    x, whole = _clips(B, L, L + (L % 2), seed=3)
    before = _bits(whole).clone()
    y, params = _run(aug, x, step)
    assert torch.equal(_bits(whole), before)                  # x is never written
    _check_against_reference(aug, x, y, params, step, None, stage)
    host = aug.parameters(step, B, L)
    xs, ys = x.cpu(), y.cpu()
    if stage == "drop":                                       # dropped samples are exactly 0, every other one is x bit for bit
        dropped = torch.zeros(B, L, dtype=torch.bool)
        for b in range(B):
            for s, n in zip(host["drop_start"][b], host["drop_len"][b]):
                dropped[b, s:s + n] = True
        assert dropped.any() and not ys[dropped].any() and not torch.signbit(ys[dropped]).any()
        assert torch.equal(_bits(ys)[~dropped], _bits(xs)[~dropped])
    if stage == "polarity":                                   # bitwise +-x
        for b in range(B):
            assert _same_bits(ys[b], -xs[b] if host["flip"][b] else xs[b])
    if stage == "gain":
        gain = torch.from_numpy(params[:, 2:3].copy())
        assert torch.equal(ys, xs * gain)
    if stage == "speed" and L == 3:                           # three samples: every clip reads in front of and behind itself
        for b in range(B):
            q = int(host["q"][b])
            i = [(L * 65536 - (L - n) * q) >> 16 for n in range(L)]
            assert min(i) - 1 < 0 and max(i) + 2 >= L


def test_speed_up_produces_the_zero_extended_head():
    L = 1000
    aug = WaveAugmentation(speed=0.25, seed=1)
    aug.q_lo = 75000                                          # every clip is sped up: its head lies in front of the clip
    x, _ = _clips(3, L)
    y, params = _run(aug, x, step=2)
    _check_against_reference(aug, x, y, params, 2, None, "speed-up")
    for b in range(3):
        q = int(params[b, 0])
        assert 75000 <= q <= aug.q_hi
        head = sum(1 for n in range(L) if ((L * 65536 - (L - n) * q) >> 16) + 2 < 0)
        assert head > 50 and not y[b, :head].cpu().any() and bool(y[b, head + 2] != 0)
    aug.q_lo, aug.q_hi = 50000, 60000                         # slowed down: the clip's start moves out of the window, no zeros
    y, params = _run(aug, x, step=2)
    _check_against_reference(aug, x, y, params, 2, None, "slow-down")
    assert bool((y != 0).all())


# ------------------------------------------------------------------------------------------ 5. the protected tail
@pytest.mark.parametrize("L", [1001, 4100])
def test_protected_tail(L):
    aug = _stage("all", seed=5)
    x, _ = _clips(3, L, L + 2)
    for a in (0, 1, L - 1, L, L // 2 + 1):
        y, params = _run(aug, x, step=7, a=a)
        assert _same_bits(y[:, a:], x[:, a:]), a
        if a == 0:
            assert _same_bits(y, x)
            assert params[:, 0].tolist() == [65536.0] * 3 and not params[:, 1].any() and not params[:, 3:].any()
        else:
            assert not _same_bits(y[:, :a], x[:, :a])
        # (with the speed on, the sample just below a is the cubic through the samples around the boundary, tail included)
        _check_against_reference(aug, x, y, params, 7, a, f"protect_from={a}")
    # continuity at the boundary: speed alone on a smooth signal leaves no step between y[a - 1] and x[a]
    t = torch.arange(L, dtype=torch.float32)
    smooth = torch.sin(t * 0.01).repeat(3, 1).to(DEV)
    a = L // 2
    y, params = _run(_stage("speed"), smooth, step=1, a=a)
    _check_against_reference(_stage("speed"), smooth, y, params, 1, a, "smooth")
    assert float((y[:, a - 1] - smooth[:, a]).abs().max()) < 0.02


# ------------------------------------------------------------------------------------------ 6. addressing
@pytest.mark.parametrize("L,ldx,ldy", [(1001, 1001, 1005), (1000, 1004, 1000), (1000, 1003, 1006), (7, 7, 9), (4100, 4100, 4104)])
def test_addressing(L, ldx, ldy):
    B, step = 3, 9
    aug = _stage("all", seed=4)
    x, x_whole = _clips(B, L, ldx, rows_before=1, rows_after=1)
    before = _bits(x_whole).clone()
    out, out_whole = _out(B, L, ldy)
    y, params = _run(aug, x, step, out=out)
    assert y.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(x_whole), before) and _out_intact(out_whole, B, L)
    _check_against_reference(aug, x, y, params, step, None, "addressing")
    # the same clips, contiguous and 16-byte aligned, give the same bits
    y2, params2 = _run(aug, x.contiguous(), step)
    assert _same_bits(y, y2) and params.tobytes() == params2.tobytes()


# ------------------------------------------------------------------------------------------ 7. determinism and sharding
def test_determinism_and_sharding():
    aug = _stage("all", seed=8)
    x, _ = _clips(4, 1001, 1003)
    y1, p1 = _run(aug, x, step=5)
    y2, p2 = _run(aug, x, step=5)
    assert _same_bits(y1, y2) and p1.tobytes() == p2.tobytes()
    y3, _ = _run(aug, x, step=6)
    assert not _same_bits(y1, y3)
    y4, _ = _run(_stage("all", seed=9), x, step=5)
    assert not _same_bits(y1, y4)
    shard, p_shard = _run(aug, x[2:4], step=5, clip_offset=2)          # (rows 2 and 3 start 8 bytes off a 16-byte boundary)
    assert _same_bits(shard, y1[2:4]) and p_shard.tobytes() == p1[2:4].tobytes()


# ------------------------------------------------------------------------------------------ 8. the trainer
class _Spy:
    """Records the entry-point names that go through _hip.call while active."""

    def __enter__(self):
        self.names, self.real = [], _hip.call

        def spy(name, *a, **kw):
            self.names.append(name)
            return self.real(name, *a, **kw)

        _hip.call = spy
        return self

    def __exit__(self, *exc):
        _hip.call = self.real


class _Meter:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))


class _Logger:
    def __init__(self):
        self.loss_meter, self.score_meter, self.steps = _Meter(), _Meter(), []

    def log(self, step):
        self.steps.append(step)


class _Labelled(torch.utils.data.Dataset):
    def __init__(self, clips):
        self.clips = clips

    def __len__(self):
        return self.clips.shape[0]

    def __getitem__(self, i):
        return self.clips[i], i


REG, LR, STEPS, SEED, START = 0.5, 1e-3, 3, 5, 5
_FIXTURE = {}


def _fixture(golden_dir):
    """(meta, data, build()) of the small model with the GRU context, loaded once."""
    if not _FIXTURE:
        z = np.load(os.path.join(golden_dir, "small_model.npz"))
        meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
        state = {k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
        _FIXTURE.update(meta=meta, data=torch.from_numpy(z["data"]), state=state)
    meta, state = _FIXTURE["meta"], _FIXTURE["state"]

    def build():
        enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [meta["C"]] * 5, 'bias': True})
        model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["C"], hidden_size=meta["H"]), enc_size=meta["C"],
                                           ar_size=meta["H"], visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype="fp32")
        model.load_state_dict(state)
        return model.to(DEV)
    return meta, _FIXTURE["data"], build


def _index_lists(data, B):
    random.seed(SEED)
    return [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)]


def _trainer(model, data, meta, score=softplus_score_function):
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=REG, score_function=score, prediction_steps=meta["K"], ar_size=meta["H"])
    tr.verbose = False
    return tr, logger


def _train(tr, meta, start=START, steps=STEPS):
    """train() for ``steps`` steps from ``start`` with the engine's inputs recorded: (entry-point names, the tensors the engine got)."""
    model = tr.model
    model._flatten_parameters(DEV)
    eng = model.engine(meta["B"], meta["L"], DEV)
    seen, real = [], eng.loss_and_grads

    def record(x, *a, **kw):
        seen.append(x.detach().clone())
        return real(x, *a, **kw)

    eng.loss_and_grads = record
    random.seed(SEED)
    try:
        with _Spy() as spy:
            tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, continue_training_at_step=start, max_steps=start + steps)
    finally:
        del eng.loss_and_grads
    torch.cuda.synchronize()
    assert model.engine(meta["B"], meta["L"], DEV) is eng and len(seen) == steps
    return spy.names, seen


def test_trainer_without_augmentation_is_unchanged(golden_dir):
    """Three steps reach neither new entry point; a second trainer built the same way reproduces losses and parameters bit for bit, and
    the engine receives the sampler's batches themselves."""
    meta, data, build = _fixture(golden_dir)
    runs = []
    for _ in range(2):
        tr, logger = _trainer(build(), data, meta)
        assert tr.augmentation is None
        names, seen = _train(tr, meta)
        assert not NEW_ENTRY_POINTS & set(names)
        runs.append((logger.loss_meter.values, tr.model._flat_param.detach().clone(), seen))
    assert len(runs[0][0]) == STEPS and runs[0][0] == runs[1][0] and all(math.isfinite(v) for v in runs[0][0])
    assert _same_bits(runs[0][1], runs[1][1])
    dev = data.to(DEV)
    for got, idx in zip(runs[0][2], _index_lists(data, meta["B"])):
        assert _same_bits(got, dev[idx])


def test_trainer_feeds_the_engine_the_augmented_batches(golden_dir):
    """Run-step i receives aug(sampler batch i, step = 5 + i) bit for bit; the losses are those of a trainer without augmentation fed
    the same clips augmented beforehand, in the same order; validate() and calc_test_task_data() reach neither entry point."""
    meta, data, build = _fixture(golden_dir)
    B = meta["B"]
    make = lambda: WaveAugmentation(speed=0.1, time_drop=(2, 300), noise_snr_db=(10.0, 20.0), gain_db=(-3.0, 3.0), polarity=0.5, seed=21)
    tr, logger = _trainer(build(), data, meta)
    tr.augmentation = make()
    names, seen = _train(tr, meta)
    assert names.count("cpc_wave_augment") == STEPS and names.count("cpc_wave_power") == STEPS
    lists = _index_lists(data, B)
    dev, by_hand, pre = data.to(DEV), make(), data.clone()
    assert len({i for idx in lists[:STEPS] for i in idx}) == STEPS * B          # distinct rows: they can be replaced in the dataset
    for i in range(STEPS):
        want = by_hand(dev[lists[i]], START + i)
        assert _same_bits(seen[i], want), i
        assert not _same_bits(want, dev[lists[i]])
        pre[lists[i]] = want.cpu()
    plain, plain_logger = _trainer(build(), pre, meta)
    plain_names, plain_seen = _train(plain, meta)
    assert not NEW_ENTRY_POINTS & set(plain_names)
    assert all(_same_bits(a, b) for a, b in zip(seen, plain_seen))
    assert logger.loss_meter.values == plain_logger.loss_meter.values and len(logger.loss_meter.values) == STEPS
    assert logger.steps == plain_logger.steps == [START + i for i in range(STEPS)]
    assert _same_bits(tr.model._flat_param.detach(), plain.model._flat_param.detach())
    # evaluation never augments
    tr.validation_set, tr.test_task_set = TensorAudioDataset(data, device=DEV), _Labelled(data[:6])
    with _Spy() as spy:
        tr.validate(batch_size=8, num_workers=0, max_steps=1)
        tr.calc_test_task_data(batch_size=3, num_workers=0)
    assert not NEW_ENTRY_POINTS & set(spy.names)


def test_trainer_protects_the_targets(golden_dir):
    """augment_targets=False: the last L - protect_from samples reach the engine bit for bit, the part in front of them does not."""
    meta, data, build = _fixture(golden_dir)
    tr, logger = _trainer(build(), data, meta)
    tr.augmentation = WaveAugmentation(speed=0.1, noise_snr_db=(10.0, 20.0), gain_db=(-3.0, 3.0), seed=3)
    tr.augment_targets = False
    enc = tr.model.encoder
    field, hop = int(enc.receptive_field), int(enc.downsampling_factor)
    T = (meta["L"] - field) // hop + 1
    a = hop * (T - meta["K"])
    assert 0 < a < meta["L"] and a == tr._check_augmentation()[1](meta["L"])
    names, seen = _train(tr, meta, steps=2)
    dev = data.to(DEV)
    by_hand = WaveAugmentation(speed=0.1, noise_snr_db=(10.0, 20.0), gain_db=(-3.0, 3.0), seed=3)
    for i, idx in enumerate(_index_lists(data, meta["B"])[:2]):
        assert _same_bits(seen[i][:, a:], dev[idx][:, a:])
        assert _same_bits(seen[i], by_hand(dev[idx], START + i, protect_from=a))
        assert float((seen[i][:, :a] - dev[idx][:, :a]).abs().max()) > 0
    assert all(math.isfinite(v) for v in logger.loss_meter.values) and len(logger.loss_meter.values) == 2


def test_polarity_only_on_a_linear_score_model(golden_dir):
    """A sanity check, not a parity claim: with every clip's sign flipped the step runs and the loss is finite."""
    meta, data, build = _fixture(golden_dir)
    tr, logger = _trainer(build(), data, meta, score=linear_score_function)
    tr.augmentation = WaveAugmentation(polarity=1.0)
    names, seen = _train(tr, meta, steps=1)
    assert names.count("cpc_wave_augment") == 1 and "cpc_wave_power" not in names
    assert _same_bits(seen[0], -data.to(DEV)[_index_lists(data, meta["B"])[0]])
    assert len(logger.loss_meter.values) == 1 and math.isfinite(logger.loss_meter.values[0])
