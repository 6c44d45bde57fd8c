"""Log-mel front end, what needs no GPU: the float64 restatement (tests/mel_reference.py) against torch.stft on the CPU, the filter
bank's properties, MelSpectrogram's band tables against the reference matrix, the constructors' ValueError tables and the argument
checks of cpc_mel_pointwise, which refuse before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import mel_reference as R
from cpc_audio_amd import _hip
from cpc_audio_amd.mel_spectrogram import MelPreprocessingModule, MelSpectrogram, mel_default_dict

SHAPES = [(64, 64, 16), (512, 400, 160), (2048, 2048, 128)]


@pytest.mark.parametrize("n_fft,win,hop", SHAPES)
def test_reference_spectrum_matches_torch_stft(n_fft, win, hop):
    """torch.stft(center=False) with a periodic Hann window (padded by torch.stft itself to n_fft, centred) is the same framed DFT:
    agreement to 1e-10 of the largest magnitude (float64 on both sides; measured 5e-16 ... 8e-16)."""
    g = torch.Generator().manual_seed(n_fft)
    L = n_fft + 37 * hop + 5
    x = torch.randn(2, L, generator=g, dtype=torch.float64)
    ref = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                     center=False, return_complex=True).permute(0, 2, 1).numpy()
    got = R.spectrum(x.numpy(), n_fft, win, hop)
    assert got.shape == ref.shape == (2, R.frames(L, n_fft, hop), n_fft // 2 + 1)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"n_fft {n_fft}: {err:.2e}")
    assert err < 1e-10


def test_default_dict_and_frames():
    assert mel_default_dict == dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=80, f_min=0.0, f_max=None)
    mel = MelSpectrogram(**mel_default_dict)
    assert mel.f_max == 8000.0 and mel.n_freq == 257 and mel.lds == 520 and mel.precision == "fp32"
    assert [mel.frames(n) for n in (511, 512, 671, 672, 16000)] == [0, 1, 1, 2, 97]
    assert np.array_equal(mel.window(), R.window(512, 400))
    pre = MelPreprocessingModule(mel_default_dict)
    assert pre.downsampling_factor == 160 and pre.receptive_field == 512 and pre.mel.n_mels == 80 and pre.output is None
    ident = MelPreprocessingModule()
    x = torch.zeros(2, 1, 8)
    assert ident.mel is None and ident(x) is x and ident.downsampling_factor == 1 and ident.receptive_field == 1


@pytest.mark.parametrize("n_fft,n_mels,f_min", [(64, 12, 0.0), (512, 80, 0.0), (2048, 256, 30.0)])
def test_filterbank_properties(n_fft, n_mels, f_min):
    sr = 16000
    W = R.mel_filterbank(sr, n_fft, n_mels, f_min)
    pts = R.mel_points(n_mels, f_min, sr / 2.0)
    f = np.arange(n_fft // 2 + 1) * sr / n_fft
    assert W.shape == (n_mels, n_fft // 2 + 1) and W.min() >= 0.0 and W.max() <= 1.0
    # between the first and the last band centre the triangles of neighbouring bands sum to one at every bin
    inside = (f >= pts[1]) & (f <= pts[-2])
    assert inside.sum() > n_mels // 2
    assert np.abs(W.sum(axis=0)[inside] - 1.0).max() < 1e-12
    # every band's support is one contiguous bin range, none is empty
    for m in range(n_mels):
        nz = np.flatnonzero(W[m])
        assert nz.size > 0 and nz[-1] - nz[0] + 1 == nz.size, m
        assert np.all(f[nz] > pts[m]) and np.all(f[nz] < pts[m + 2])


@pytest.mark.parametrize("n_fft,win,hop,n_mels", [(512, 400, 160, 80), (2048, 2048, 128, 256)])
def test_pure_tone_peaks_in_its_band(n_fft, win, hop, n_mels):
    sr = 16000
    pts = R.mel_points(n_mels, 0.0, sr / 2.0)
    t = np.arange(n_fft + 4 * hop, dtype=np.float64) / sr
    for freq in (440.0, 1000.0, 3300.0):
        M, _, _ = R.mel_power(np.sin(2 * np.pi * freq * t)[None], sr, n_fft, win, hop, n_mels)
        peak = int(M[0].mean(axis=0).argmax())
        # the band whose triangle weighs the tone most: its centre is the corner point nearest to the tone
        assert peak == int(np.abs(pts[1:-1] - freq).argmin()), (freq, peak)
        assert pts[peak] < freq < pts[peak + 2]


@pytest.mark.parametrize("n_fft,n_mels,f_min", [(64, 12, 0.0), (512, 80, 0.0), (2048, 256, 30.0)])
def test_band_tables_reproduce_the_reference_matrix(n_fft, n_mels, f_min):
    mel = MelSpectrogram(n_fft=n_fft, win_length=n_fft, hop_length=16, n_mels=n_mels, f_min=f_min)
    ref = R.mel_filterbank(16000, n_fft, n_mels, f_min)
    assert np.array_equal(mel.mel_filterbank(), ref) and mel.mel_filterbank().dtype == np.float64
    assert mel.band_lo.dtype == mel.band_n.dtype == mel.band_off.dtype == np.int32 and mel.band_w.dtype == np.float32
    assert np.array_equal(mel.band_off, np.concatenate([[0], np.cumsum(mel.band_n)[:-1]])) and len(mel.band_w) == mel.band_n.sum()
    assert mel.band_lo.min() >= 0 and (mel.band_lo + mel.band_n).max() <= mel.n_freq and mel.band_n.min() >= 1
    # float64 before the one rounding: equal; the uploaded f32 weights: within one ulp (half an ulp, in fact: one rounding)
    assert np.array_equal(R.expand_bands(mel.band_lo, mel.band_n, mel.band_off, mel.band_w64, mel.n_freq), ref)
    dense32 = R.expand_bands(mel.band_lo, mel.band_n, mel.band_off, mel.band_w, mel.n_freq)
    assert dense32.dtype == np.float32
    assert np.all(np.abs(dense32.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)))
    assert np.array_equal(dense32, ref.astype(np.float32))


def test_dft_operand_rows():
    mel = MelSpectrogram(n_fft=64, win_length=48, hop_length=8, n_mels=8)
    op = mel.dft_operand(72).numpy()
    basis = R.dft_basis(64) * R.window(64, 48)
    assert op.shape == (72, 64) and not op[66:].any()
    assert np.array_equal(op[0:66:2], basis.real.astype(np.float32)) and np.array_equal(op[1:66:2], basis.imag.astype(np.float32))


@pytest.mark.parametrize("kw", [dict(n_fft=96), dict(n_fft=32, win_length=32), dict(n_fft=16384), dict(win_length=0), dict(win_length=513),
                                dict(hop_length=0), dict(hop_length=4), dict(hop_length=100), dict(f_min=-1.0), dict(f_min=8000.0),
                                dict(f_min=300.0, f_max=200.0), dict(f_max=8000.5), dict(n_mels=0), dict(n_mels=1025)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_mel_spectrogram_constructor_refuses(kw):
    with pytest.raises(ValueError):
        MelSpectrogram(**dict(mel_default_dict, **kw))


def test_empty_band_is_named():
    with pytest.raises(ValueError, match=r"mel band \d+ has no bin"):
        MelSpectrogram(n_fft=64, win_length=64, hop_length=16, n_mels=16)
    W = R.mel_filterbank(16000, 64, 16)
    empty = [m for m in range(16) if not W[m].any()]
    assert empty
    with pytest.raises(ValueError, match=f"mel band {empty[0]} "):
        MelPreprocessingModule(dict(mel_default_dict, n_fft=64, win_length=64, hop_length=16, n_mels=16))
    for n_fft, n_mels, f_min in ((64, 12, 0.0), (512, 80, 0.0), (2048, 256, 30.0), (256, 24, 0.0)):      # the shapes the GPU tests use
        MelSpectrogram(n_fft=n_fft, win_length=n_fft, hop_length=16, n_mels=n_mels, f_min=f_min)


@pytest.mark.parametrize("kw", [dict(log_offset=0.0), dict(log_offset=-1e-6), dict(log_offset=float("nan")), dict(log_offset=float("inf")),
                                dict(scaling=float("inf")), dict(delta_scaling=float("nan"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_preprocessing_constructor_refuses(kw):
    with pytest.raises(ValueError):
        MelPreprocessingModule(mel_default_dict, **kw)


def test_cpu_tensor_and_short_clip_raise():
    mel = MelSpectrogram(**mel_default_dict)
    with pytest.raises(RuntimeError, match="GPU only"):
        mel.transform(torch.zeros(2, 1, 4000))
    with pytest.raises(RuntimeError, match="GPU only"):
        MelPreprocessingModule(mel_default_dict)(torch.zeros(2, 1, 4000))


P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
INF, NAN = float("inf"), float("nan")


def _mel(**kw):
    a = dict(spec=P, lds=74, band_lo=P, band_n=P, band_off=P, band_w=P, out=P, B=2, Tn=5, n_freq=33, n_mels=12, delta=1, take_log=1,
             log_offset=1e-6, scaling=1.0, delta_scaling=1.0)
    a.update(kw)
    return _hip.lib().cpc_mel_pointwise(a["spec"], a["lds"], a["band_lo"], a["band_n"], a["band_off"], a["band_w"], a["out"], a["B"], a["Tn"],
                                        a["n_freq"], a["n_mels"], a["delta"], a["take_log"], a["log_offset"], a["scaling"],
                                        a["delta_scaling"], None)


@pytest.mark.parametrize("case", [dict(spec=None), dict(band_lo=None), dict(band_n=None), dict(band_off=None), dict(band_w=None), dict(out=None),
                                  dict(B=0), dict(B=-1), dict(Tn=0), dict(Tn=1), dict(Tn=0, delta=0), dict(n_mels=0), dict(n_mels=1025),
                                  dict(n_freq=1, lds=8), dict(n_freq=4098, lds=8200), dict(lds=64), dict(lds=75), dict(lds=-2),
                                  dict(delta=2), dict(delta=-1), dict(take_log=2), dict(take_log=-1), dict(take_log=0, delta=1),
                                  dict(log_offset=0.0), dict(log_offset=-1.0), dict(log_offset=NAN), dict(log_offset=INF),
                                  dict(scaling=INF), dict(scaling=NAN), dict(delta_scaling=INF), dict(delta_scaling=NAN),
                                  dict(spec=C.c_void_p(0x1004)), dict(out=C.c_void_p(0x1004))],
                         ids=lambda c: ",".join(f"{k}={'NULL' if v is None else getattr(v, 'value', v)}" for k, v in c.items()))
def test_mel_entry_point_refuses_before_any_launch(case):
    """-22 for a NULL pointer in any position; B, Tn or n_mels < 1; Tn < 2 with delta; n_freq < 2 or above 4097; n_mels above 1024;
    lds < 2 n_freq or odd; delta or take_log outside {0, 1}; take_log = 0 with delta; log_offset not finite or <= 0 with take_log;
    scaling or delta_scaling not finite; a spectrum (or, with delta, an output) that is not 8-byte aligned."""
    assert _mel(**case) == -22
