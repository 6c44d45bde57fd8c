"""Log-mel front end on the GPU: cpc_mel_pointwise alone on spectra the test writes, MelSpectrogram end to end against the float64
restatement (tests/mel_reference.py), and MelPreprocessingModule in front of the scalogram encoder through the trainer.

Error bounds of the kernel-alone checks (u = 2^-24, gamma_n = n u / (1 - n u), all weights and powers non-negative):
  power     p^ = fl(fl(re^2) + fl(im^2)): three roundings, |p^ - p| <= gamma_3 p.
  band      the fma chain over the n bins of band m adds one rounding per term: |M^ - M| <= gamma_(n+3) M, M = sum_k w_k p_k the exact sum
            of the f32 weights and the f32 inputs (the float64 reference: its own error, 4097 terms of 2^-53, is below 1e-12 of M).
  log       the argument fl(M^ + log_offset) is within gamma_(n+4) of M + log_offset, relatively (log_offset > 0), which moves the
            logarithm by at most gamma_(n+4) / (1 - gamma_(n+4)); the device's logf is documented to 1 ulp (HIP math API, logf), taken as
            LOGF_ULPS = 2 ulps of |l| (an ulp is at most 2^-23 |l|; the second one covers the binade edge between l^ and l); the product
            with ``scaling`` is one more rounding.  E_l = gamma_(n+4) / (1 - gamma_(n+4)) + LOGF_ULPS 2^-23 |l| bounds the logarithm,
            |scaling| E_l + u |A| channel 0.
  delta     fl(delta_scaling fl(l^[w+1] - l^[w])): |delta_scaling| (E_l[w+1] + E_l[w]) + 2 u |d|.
With integer-valued re / im, weights that are multiples of 1/16 and sums below 2^20 every operation is exact in f32: the mel power
(take_log = 0) then equals the float64 sum bit for bit."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mel_reference as R  # noqa: E402
from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,  # noqa: E402
                                                           softplus_score_function)
from cpc_audio_amd.mel_spectrogram import MelPreprocessingModule, MelSpectrogram, mel_default_dict  # noqa: E402
from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder  # noqa: E402
from oracle import cpc_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24
LOGF_ULPS = 2
SENTINEL = -12345.5
GUARD = 64


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _tables(rng, n_freq, n_mels, kind):
    """Random band tables with the edge cases in fixed places: band 0 is exactly one bin, band 1 covers every bin, the last band ends
    at the Nyquist bin.  ``kind``: "dyadic" weights are multiples of 1/16 in [1/16, 1], "real" weights are uniform in (0, 1);
    "overrun": bands 2 and 3 run past n_freq / start below 0 (the kernel clamps them; their weights exist); "narrow": bands of at most
    three bins, dyadic weights -- the whole table is at most 2 n_freq weights, which the kernel then keeps in LDS (the random tables
    of the other kinds are longer at n_freq = 33 and are read from global memory; a mel bank is of the narrow kind)."""
    lo = rng.integers(0, n_freq, size=n_mels)
    cnt = np.array([rng.integers(1, min(3, n_freq - a) + 1 if kind == "narrow" else n_freq - a + 1) for a in lo])
    if kind == "narrow":
        lo[0], cnt[0] = n_freq // 3, 1
        lo[-1] = n_freq - cnt[-1]
        assert cnt.sum() <= 2 * n_freq - 8
        off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        w = rng.integers(1, 17, size=int(cnt.sum())) / 16.0
        return lo.astype(np.int32), cnt.astype(np.int32), off.astype(np.int32), w.astype(np.float32)
    lo[0], cnt[0] = n_freq // 3, 1
    if n_mels > 1:
        lo[1], cnt[1] = 0, n_freq
    lo[-1] = n_freq - cnt[-1]
    if kind == "overrun":
        lo[2], cnt[2] = n_freq - 3, 9
        lo[3], cnt[3] = -4, 7
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    total = int(cnt.sum())
    w = rng.integers(1, 17, size=total) / 16.0 if kind != "real" else rng.uniform(0.01, 1.0, size=total)
    return lo.astype(np.int32), cnt.astype(np.int32), off.astype(np.int32), w.astype(np.float32)


def _run_kernel(spec, lds, tables, n_freq, delta, take_log, log_offset=1e-3, scaling=1.0, delta_scaling=1.0):
    """spec (B, Tn, lds) device tensor -> (out (B, W, n_mels, Cc) numpy, guards intact?)."""
    B, Tn = spec.shape[:2]
    n_mels = len(tables[0])
    dev = [torch.from_numpy(a).to(DEV) for a in tables]
    W, Cc = (Tn - 1, 2) if delta else (Tn, 1)
    n = B * W * n_mels * Cc
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    out = buf[GUARD:GUARD + n]
    _hip.call("cpc_mel_pointwise", _hip.ptr(spec), lds, *[_hip.ptr(t) for t in dev], _hip.ptr(out), B, Tn, n_freq, n_mels,
              int(delta), int(take_log), float(log_offset), float(scaling), float(delta_scaling))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all())
    return host[GUARD:GUARD + n].reshape(B, W, n_mels, Cc).copy(), intact


def _spectrum(rng, B, Tn, n_freq, lds, integers, amp=4):
    """f32 (B, Tn, lds) with NaN in the row padding behind 2 n_freq."""
    z = np.full((B, Tn, lds), np.nan, dtype=np.float32)
    if integers:
        z[:, :, :2 * n_freq] = rng.integers(-amp, amp + 1, size=(B, Tn, 2 * n_freq)).astype(np.float32)
    else:
        z[:, :, :2 * n_freq] = (rng.standard_normal((B, Tn, 2 * n_freq)) * rng.uniform(0.1, 3.0, size=(B, Tn, 1))).astype(np.float32)
    return z


def _power64(z, n_freq):
    re, im = z[..., 0:2 * n_freq:2].astype(np.float64), z[..., 1:2 * n_freq:2].astype(np.float64)
    return re * re + im * im


KERNEL_CASES = [  # B, Tn, n_freq, n_mels, table kind
    (2, 5, 33, 12, "dyadic"), (2, 2, 33, 12, "dyadic"), (1, 5, 33, 12, "dyadic"), (2, 5, 33, 80, "dyadic"), (2, 5, 33, 256, "dyadic"),
    (2, 5, 33, 300, "dyadic"), (1, 3, 33, 1024, "dyadic"), (2, 5, 33, 12, "overrun"), (2, 35, 33, 12, "dyadic"), (1, 19, 1300, 12, "dyadic"),
    (1, 3, 4097, 256, "dyadic"), (2, 5, 33, 12, "narrow"), (2, 35, 33, 18, "narrow"), (1, 19, 1300, 300, "narrow"), (1, 3, 4097, 1024, "narrow")]


@pytest.mark.parametrize("B,Tn,n_freq,n_mels,kind", KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_exact_data(B, Tn, n_freq, n_mels, kind):
    """Integer re / im, dyadic weights, take_log = 0: the mel power equals the float64 sums bit for bit (delta off: take_log = 0 has no
    delta).  The cases: several clips and one; Tn = 2; n_mels = 80 and 256 (every lane of some or all waves owns a band), 300 and 1024
    (a lane owns several bands, up to the limit); a band of one bin, one of all bins, the last ending at the Nyquist bin (_tables); a
    table that runs past both ends of the row (the clamp: no NaN from the padding, which is NaN, and nothing from the next row);
    35 frames and 19 frames at n_freq = 1300 (more than one run of frames per clip, with a short last pass, at 8 and 4 frames per
    pass); the limit n_freq = 4097 (2 frames per pass); tables short enough for the kernel to keep them in LDS ("narrow"), at each
    number of frames per pass.  Two runs are bit-identical; the guards around the output and the spectrum's
    padding are untouched."""
    rng = np.random.default_rng(n_freq * 7 + n_mels + Tn)
    lds = 2 * n_freq + 8
    tables = _tables(rng, n_freq, n_mels, kind)
    z = _spectrum(rng, B, Tn, n_freq, lds, integers=True)
    spec = torch.from_numpy(z).to(DEV)
    got, intact = _run_kernel(spec, lds, tables, n_freq, delta=False, take_log=False)
    want = R.band_sums(_power64(z, n_freq), *tables, n_freq)
    assert want.max() < 2 ** 20 and intact
    assert np.array_equal(got[..., 0].astype(np.float64), want)
    again, intact = _run_kernel(spec, lds, tables, n_freq, delta=False, take_log=False)
    assert intact and np.array_equal(got, again)
    back = spec.cpu().numpy()
    assert np.array_equal(back, z, equal_nan=True) and np.isnan(back[:, :, 2 * n_freq:]).all()


@pytest.mark.parametrize("delta", [False, True], ids=["plain", "delta"])
@pytest.mark.parametrize("B,Tn,n_freq,n_mels,kind", [c for c in KERNEL_CASES if c[1] >= 2], ids=lambda v: str(v))
def test_kernel_general_data_against_float64(B, Tn, n_freq, n_mels, kind, delta):
    """Gaussian spectra, weights uniform in (0, 1) (dyadic for the overrun table, whose layout is fixed), mel power and the log / delta
    output against float64 within the bounds of the module docstring; scaling 0.7, delta_scaling 1.9, log_offset 1e-3.  Bit-identical
    between two runs.  Measured on MI355X, largest error / bound over the cases: power 0.56, channel 0 0.58, delta 0.44."""
    rng = np.random.default_rng(n_freq * 11 + n_mels + Tn + int(delta))
    lds = 2 * n_freq + 8
    tables = _tables(rng, n_freq, n_mels, "real" if kind == "dyadic" else kind)
    if kind == "narrow":
        tables = tables[:3] + (rng.uniform(0.01, 1.0, size=len(tables[3])).astype(np.float32),)
    z = _spectrum(rng, B, Tn, n_freq, lds, integers=False)
    spec = torch.from_numpy(z).to(DEV)
    M = R.band_sums(_power64(z, n_freq), *tables, n_freq)                              # (B, Tn, n_mels)
    terms = np.minimum(tables[1].astype(np.int64), n_freq)                             # (at most) the chain length of each band
    got, intact = _run_kernel(spec, lds, tables, n_freq, delta=False, take_log=False)
    assert intact and np.isfinite(got).all()
    ratio_p = (np.abs(got[..., 0] - M) / (np.array([gamma(n + 3) for n in terms]) * M + 1e-300)).max()
    off, sc, dsc = 1e-3, 0.7, 1.9
    got, intact = _run_kernel(spec, lds, tables, n_freq, delta=delta, take_log=True, log_offset=off, scaling=sc, delta_scaling=dsc)
    again, _ = _run_kernel(spec, lds, tables, n_freq, delta=delta, take_log=True, log_offset=off, scaling=sc, delta_scaling=dsc)
    assert intact and np.array_equal(got, again) and np.isfinite(got).all()
    l = np.log(M + np.float64(np.float32(off)))
    g4 = np.array([gamma(n + 4) for n in terms])
    E_l = g4 / (1.0 - g4) + LOGF_ULPS * 2.0 ** -23 * np.abs(l)
    sc_f = np.float64(np.float32(sc))
    A = sc_f * l
    E_A = abs(sc_f) * E_l + U * np.abs(A)
    if not delta:
        ratio_a, ratio_d = (np.abs(got[..., 0] - A) / E_A).max(), 0.0
    else:
        d = np.float64(np.float32(dsc)) * (l[:, 1:] - l[:, :-1])
        E_d = abs(np.float64(np.float32(dsc))) * (E_l[:, 1:] + E_l[:, :-1]) + 2 * U * np.abs(d)
        ratio_a = (np.abs(got[..., 0] - A[:, 1:]) / E_A[:, 1:]).max()
        ratio_d = (np.abs(got[..., 1] - d) / E_d).max()
    print(f"error / bound: power {ratio_p:.3f}, channel 0 {ratio_a:.3f}, delta {ratio_d:.3f}")
    assert ratio_p <= 1.0 and ratio_a <= 1.0 and ratio_d <= 1.0


# ------------------------------------------------------------------------------------------------ 2. MelSpectrogram end to end
E2E = [(64, 64, 16, 12, 0.0), (512, 400, 160, 80, 0.0), (2048, 2048, 128, 256, 30.0)]
_signals = {}


def _signal(L):
    """(3, L) f32: 0.2 randn + 0.5 sin(2 pi 440 t), seeded by L; shared by the cases."""
    if L not in _signals:
        g = torch.Generator().manual_seed(1000 + L)
        t = torch.arange(L, dtype=torch.float64) / 16000.0
        _signals[L] = (0.2 * torch.randn(3, L, generator=g, dtype=torch.float64) + 0.5 * torch.sin(2 * np.pi * 440.0 * t)).float()
    return _signals[L]


_refs = {}


def _reference(cfg, L):
    if (cfg, L) not in _refs:
        n_fft, win, hop, n_mels, f_min = cfg
        _refs[(cfg, L)] = R.mel_power(_signal(L).double().numpy(), 16000, n_fft, win, hop, n_mels, f_min)
    return _refs[(cfg, L)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("L", [400, 4000, 8192])
@pytest.mark.parametrize("cfg", E2E, ids=lambda c: f"nfft{c[0]}")
def test_mel_spectrogram_against_reference(cfg, L, precision):
    """Waveform -> DFT GEMM -> cpc_mel_pointwise against the float64 restatement, B = 3, both GEMM precisions.
    Spectrum: within 2e-5 (fp32) / 5e-5 (bf16x3) of the largest magnitude -- the bounds test_cqt_full_size_against_oracle holds the same
    GEMM to at K up to 16 384.  Mel power (take_log = 0): within 4e-5 (1e-4) max p_ref sum_k W[m, k] per band -- the amplitude bound
    carried through the square and the non-negative weights.  Log output (log_offset 1e-6, both scalings 1): inside
    [scaling log(max(M_ref - D, 0) + offset), scaling log(M_ref + D + offset)] with D the power-domain bound, widened by the logf ulps
    and the two roundings around it (module docstring); the delta channel within twice the channel-0 bound (and within the sum of its
    two frames' bounds).  A clip shorter than one frame raises ValueError.
    Measured on MI355X (fp32 / bf16x3), ranges over the cases: spectrum 3.0e-7 ... 1.7e-6 / 9.4e-7 ... 3.2e-6 of max |X|; mel power at
    most 5.2e-2 / 3.2e-2 of its bound (2.1e-6 / 3.2e-6 of max p_ref sum W); log output at most 6.0e-2 / 3.2e-2 of its bound, delta
    channel 3.9e-2 / 1.7e-2."""
    n_fft, win, hop, n_mels, f_min = cfg
    mel = MelSpectrogram(n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, f_min=f_min)
    mel.precision = precision
    assert mel.band_n.min() >= 1                                           # no empty band
    x = _signal(L).to(DEV).unsqueeze(1)
    if L < n_fft:
        with pytest.raises(ValueError, match="shorter than one frame"):
            mel.transform(x)
        return
    M_ref, p_ref, X_ref = _reference(cfg, L)
    Tn = mel.frames(L)
    spec, Tn_got, lds = mel.transform(x)
    assert (Tn_got, lds) == (Tn, n_fft + 8) and tuple(spec.shape) == (3, Tn, lds) and X_ref.shape == (3, Tn, mel.n_freq)
    z = spec.cpu().numpy().astype(np.float64)
    X = z[..., 0:2 * mel.n_freq:2] + 1j * z[..., 1:2 * mel.n_freq:2]
    s_err = np.abs(X - X_ref).max() / np.abs(X_ref).max()
    assert s_err < (2e-5 if precision == "fp32" else 5e-5), s_err
    fwd = mel(x)
    assert tuple(fwd.shape) == (3, mel.n_freq, Tn, 2) and torch.equal(fwd[..., 0].permute(0, 2, 1), spec[..., 0:2 * mel.n_freq:2])
    # mel power
    Wsum = R.mel_filterbank(16000, n_fft, n_mels, f_min).sum(axis=1)
    D = (4e-5 if precision == "fp32" else 1e-4) * p_ref.max() * Wsum                     # (n_mels,)
    Mp = mel.pointwise(spec, Tn, take_log=False).cpu().numpy().astype(np.float64)[..., 0]
    assert Mp.shape == M_ref.shape
    p_frac = (np.abs(Mp - M_ref) / D).max()
    assert p_frac <= 1.0, p_frac
    # log output through the module
    off, sc, dsc = 1e-6, 1.0, 1.0
    lo = sc * np.log(np.maximum(M_ref - D, 0.0) + off)
    hi = sc * np.log(M_ref + D + off)
    A_ref = sc * np.log(M_ref + off)
    slack = sc * (LOGF_ULPS * 2.0 ** -23 + 2 * U) * np.abs(A_ref / sc) + U * np.abs(A_ref)
    E0 = np.maximum(hi - A_ref, A_ref - lo) + slack                                       # (B, Tn, n_mels)
    a_frac = d_frac = 0.0
    for delta in (False, True):
        pre = MelPreprocessingModule(dict(mel_default_dict, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, f_min=f_min),
                                     delta=delta, log_offset=off, scaling=sc, delta_scaling=dsc)
        pre.mel.precision = precision
        out = pre(x)
        ref = R.log_mel(M_ref, delta=delta, log_offset=off, scaling=sc, delta_scaling=dsc)
        assert tuple(out.shape) == ref.shape == (3, 2 if delta else 1, n_mels, Tn - 1 if delta else Tn) and pre.output is out
        assert out.permute(0, 3, 2, 1).is_contiguous()
        got = out.cpu().numpy().astype(np.float64)
        e = E0.transpose(0, 2, 1)
        if not delta:
            assert (got[:, 0] >= lo.transpose(0, 2, 1) - slack.transpose(0, 2, 1)).all() and (got[:, 0] <= hi.transpose(0, 2, 1) + slack.transpose(0, 2, 1)).all()
            a_frac = (np.abs(got[:, 0] - ref[:, 0]) / e).max()
        else:
            assert (np.abs(got[:, 0] - ref[:, 0]) <= e[:, :, 1:]).all()
            Ed = (dsc / sc) * np.minimum(2 * e[:, :, 1:], e[:, :, 1:] + e[:, :, :-1])
            d_frac = (np.abs(got[:, 1] - ref[:, 1]) / Ed).max()
            assert d_frac <= 1.0, d_frac
    print(f"n_fft {n_fft} L {L} {precision}: spectrum {s_err:.2e} of max |X|, mel power {p_frac:.2e} of its bound, "
          f"log {a_frac:.2e} and delta {d_frac:.2e} of theirs")


# ------------------------------------------------------------------------------------------------ 3. - 5. through the trainer
SCORE = {"softplus": softplus_score_function, "linear": linear_score_function}
MEL_SMALL = dict(mel_default_dict, n_fft=256, win_length=256, hop_length=32, n_mels=24)


class _Meter:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))


class _Logger:
    def __init__(self):
        self.loss_meter, self.score_meter = _Meter(), _Meter()

    def log(self, step):
        pass


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "scalogram_model.npz"))
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    return {k: z[k] for k in z.files}, meta, blocks


def _model(g, meta, blocks, pre, dtype):
    enc = ScalogramResidualEncoder(args_dict={'phase': True, 'blocks': copy.deepcopy(blocks), 'activation_register': None},
                                   preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["E"], hidden_size=meta["H"]), enc_size=meta["E"],
                                       ar_size=meta["H"], visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype=dtype)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return model


def _trainer(model, pre, data, logger, meta, score="softplus", all_t=False, reg=1.0, **kw):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=reg, score_over_all_timesteps=all_t, score_function=SCORE[score],
                                      prediction_steps=meta["K"], ar_size=meta["H"], preprocessing=pre, **kw)
    tr.verbose = False
    return tr


def test_train_step_against_oracle(golden_dir):
    """One train() step at lr = 0 of the fixture's encoder and GRU context behind MelPreprocessingModule(n_fft 256, hop 32, 24 bands,
    delta): 61 frames of the fixture's (12, 2177) clips, a (4, 2, 24, 60) input, the fixture's own shape.  The oracle is fed the
    device's mel output (as test_gradient_penalty_plain_conv_context_against_oracle feeds the device's scalogram): loss within 1e-4
    relative, every parameter gradient within 1e-3 relative L2 (the project's f32 tolerances), both loss branches."""
    g, meta, blocks = _fixture(golden_dir)
    B, K, H, V = meta["B"], meta["K"], meta["H"], meta["V"]
    data = torch.from_numpy(g["data"])
    assert tuple(data.shape) == (12, 2177)
    pre = MelPreprocessingModule(MEL_SMALL, delta=True)
    model = _model(g, meta, blocks, pre, "fp32")
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pre, model = pre.to(DEV), model.to(DEV)
    for score, all_t, reg in (("softplus", False, 1.0), ("linear", True, 0.01)):
        logger = _Logger()
        tr = _trainer(model, pre, data, logger, meta, score, all_t, reg)
        model.load_state_dict(params)
        random.seed(91)
        idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
        random.seed(91)
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
        with torch.no_grad():
            mel_out = pre(data[idx].to(DEV).unsqueeze(1)).cpu()
        assert tuple(mel_out.shape) == (4, 2, 24, 60)
        oblocks = [dict(b) for b in blocks]
        oblocks[0]["in_channels"] = 2
        ot = O.OracleTrainer(params, V, K, score=score, all_timesteps=all_t, regularization=reg, lr=0.0, scalogram=oblocks)
        loss, smax, grads = ot.loss_and_grads(mel_out)
        assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss)), (all_t, logger.loss_meter.values, float(loss))
        largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
        worst = 0.0
        for name, ref in grads.items():
            got = dict(model.named_parameters())[name].grad.double().cpu()
            if ref.abs().max().item() < 1e-6 * largest:
                assert got.abs().max().item() < 1e-5 * largest, (all_t, name)
                continue
            l2 = ((got - ref.double()).norm() / (ref.double().norm() + 1e-30)).item()
            worst = max(worst, l2)
            assert l2 < 1e-3, (all_t, name, l2)
        print(f"{score} all_timesteps={all_t}: loss {logger.loss_meter.values[0]:.6f} vs {float(loss):.6f}, worst gradient l2 {worst:.2e}")


class _Labelled(torch.utils.data.Dataset):
    def __init__(self, clips):
        self.clips = clips

    def __len__(self):
        return self.clips.shape[0]

    def __getitem__(self, i):
        return self.clips[i], i


def test_preprocessing_ahead_validate_and_bf16(golden_dir):
    """Three steps with trainer.preprocess_ahead on and off give identical losses (as test_preprocessing_one_step_ahead_changes_nothing
    for the CQT); validate() and calc_test_task_data() return finite values; with compute_dtype bf16 and the bf16x3 DFT the step runs,
    loss and gradients are finite and the engine reads the module's output in place."""
    g, meta, blocks = _fixture(golden_dir)
    B = meta["B"]
    data = torch.from_numpy(g["data"])
    runs = []
    for ahead in (False, True):
        pre = MelPreprocessingModule(MEL_SMALL, delta=True)
        model = _model(g, meta, blocks, pre, "fp32")
        pre, model = pre.to(DEV), model.to(DEV)
        logger = _Logger()
        tr = _trainer(model, pre, data, logger, meta, validation_set=TensorAudioDataset(data, device=DEV), test_task_set=_Labelled(data[:8]))
        tr.preprocess_ahead = ahead
        random.seed(17)
        tr.train(batch_size=B, epochs=10, lr=1e-3, num_workers=0, max_steps=3)
        torch.cuda.synchronize()
        runs.append(list(logger.loss_meter.values))
    assert len(runs[0]) == 3 and runs[0] == runs[1] and all(np.isfinite(runs[0])), runs
    losses, acc, score, mi = tr.validate(batch_size=8, num_workers=0)          # (the validation sampler hands out runs of 8 clips per file)
    for v in (losses, acc, score, mi):
        assert torch.isfinite(torch.as_tensor(v, dtype=torch.float64)).all()
    task, labels = tr.calc_test_task_data(batch_size=4, num_workers=0)
    assert task.shape == (8, meta["H"]) and np.isfinite(task).all() and list(labels) == list(range(8))
    # bf16 engine behind the bf16x3 DFT
    pre = MelPreprocessingModule(MEL_SMALL, delta=True)
    model = _model(g, meta, blocks, pre, "bf16")
    pre, model = pre.to(DEV), model.to(DEV)
    pre.mel.precision = "bf16x3"
    logger = _Logger()
    tr = _trainer(model, pre, data, logger, meta)
    random.seed(17)
    tr.train(batch_size=B, epochs=1, lr=1e-3, num_workers=0, max_steps=1)
    torch.cuda.synchronize()
    assert len(logger.loss_meter.values) == 1 and np.isfinite(logger.loss_meter.values[0])
    assert torch.isfinite(model._flat_grad).all() and model._flat_grad.abs().max().item() > 0
    eng = model.engine_for(pre.output)
    assert eng._x_alias is not None and tuple(eng._x_alias[0].shape) == (4, 2, 24, 60)


def test_cqt_step_never_reaches_the_mel_kernel(golden_dir, monkeypatch):
    """A CQT-fed step of the fixture model runs the launches it ran before: cpc_mel_pointwise is never called (counted through
    _hip.call), and its loss is the parent's value in scalogram_model.npz, to test_scalogram_model_matches_reference's tolerance."""
    g, meta, blocks = _fixture(golden_dir)
    run = meta["runs"][0]
    calls = {}
    real = _hip.call

    def counting(name, *a, **kw):
        calls[name] = calls.get(name, 0) + 1
        return real(name, *a, **kw)

    monkeypatch.setattr(_hip, "call", counting)
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta["pre"])
    model = _model(g, meta, blocks, pre, "fp32")
    pre, model = pre.to(DEV), model.to(DEV)
    logger = _Logger()
    tr = _trainer(model, pre, torch.from_numpy(g["data"]), logger, meta, run["score"], run["all_timesteps"], run["reg"])
    random.seed(run["python_seed"])
    tr.train(batch_size=meta["B"], epochs=10, lr=run["lr"], num_workers=0, max_steps=run["steps"])
    torch.cuda.synchronize()
    assert calls.get("cpc_scalogram_pointwise", 0) >= 1 and "cpc_mel_pointwise" not in calls, calls
    assert abs(logger.loss_meter.values[0] - run["loss"][0]) <= 2e-4 * abs(run["loss"][0])
