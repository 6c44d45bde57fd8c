"""Resampling without a GPU: the package's filter design against the independent float64 restatement (resample_reference.py) and that
against scipy's upfirdn; the properties of the restatement the GPU tests lean on (unit gain, sines, stop band, the overshoot of a square
wave); cpc_resample's argument checks, which return before any launch; and DeviceAudioDataset(convert=True) without a device, where
width and channel conversion run in numpy and another rate is refused."""
import ctypes as C
import os
import struct
import wave

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip, resampling
from cpc_audio_amd.audio_dataset import DeviceAudioDataset

import resample_reference as R


def _ulps(a, b):
    """The distance of two float32 arrays in units in the last place (both finite, same sign or zero)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("orig,new", R.RATE_PAIRS, ids=lambda v: str(v))
def test_taps_equal_the_restatement_to_one_ulp(orig, new):
    taps, L, M, W = resampling.resample_taps(orig, new)
    want, Lr, Mr, Wr = R.resample_taps(orig, new)
    assert (L, M, W) == (Lr, Mr, Wr) == R.SHAPES[(orig, new)]
    assert taps.dtype == np.float32 and taps.shape == (L, 2 * W + 1) == want.shape
    assert int(_ulps(taps, want).max()) <= 1
    assert abs(float(taps.astype(np.float64).sum()) - L) < 1e-4          # the prototype sums to L, every phase to about 1
    assert (resampling.output_length(6000, L, M), resampling.rate_ratio(orig, new)) == (R.output_count(6000, L, M), (L, M))


def test_equal_rates_give_the_identity_table_and_large_tables_are_refused():
    for rate in (16000, 44100, 1):
        taps, L, M, W = resampling.resample_taps(rate, rate)
        assert (L, M, W) == (1, 1, 0) and taps.dtype == np.float32 and taps.tolist() == [[1.0]]
    assert R.resample_taps(8000, 8000)[1:] == (1, 1, 0)
    with pytest.raises(ValueError, match=r"44101.*16000|16000.*44101"):          # L = 16000, W = 47: 1.5 M floats
        resampling.resample_taps(44101, 16000)
    with pytest.raises(ValueError, match="320000"):          # M / L = 20: a tile's input span exceeds the LDS budget
        resampling.plan_for(320000, 16000)
    with pytest.raises(ValueError):
        resampling.rate_ratio(0, 16000)


@pytest.mark.parametrize("orig,new", R.RATE_PAIRS, ids=lambda v: str(v))
def test_the_restatement_equals_upfirdn(orig, new):
    """scipy.signal.upfirdn(h, x, L, M) with the prototype shifted by r = (-W L) mod M leading zeros, read from (W L + r) / M."""
    signal = pytest.importorskip("scipy.signal")
    taps, L, M, W = R.resample_taps(orig, new)
    x = np.random.default_rng(orig + new).uniform(-1.0, 1.0, 257)
    y, _ = R.resample(x, taps, L, M, W)
    h = np.zeros(2 * W * L + 1)
    for p in range(L):          # the prototype as the table holds it (float32)
        for t in range(2 * W + 1):
            j = p - (t - W) * L + W * L
            if 0 <= j <= 2 * W * L:
                h[j] = taps[p][t]
    r = (-W * L) % M
    full = signal.upfirdn(np.concatenate([np.zeros(r), h]), x, L, M)
    first = (W * L + r) // M
    assert len(y) == R.output_count(257, L, M) and first + len(y) <= len(full)
    assert float(np.abs(full[first:first + len(y)] - y).max()) <= 1e-7


N_IN = 6000


def _run(orig, new, x):
    taps, L, M, W = R.resample_taps(orig, new)
    y, bound = R.resample(x, taps, L, M, W)
    return y, bound, R.interior(len(y), L, M, W)


@pytest.mark.parametrize("orig,new", R.RATE_PAIRS, ids=lambda v: str(v))
def test_reference_passes_a_constant(orig, new):
    y, bound, mid = _run(orig, new, np.ones(N_IN))
    worst = float(np.abs(y[mid] - 1.0).max())
    print("constant 1, interior error", orig, new, worst)
    assert len(y[mid]) > 100 and worst <= 1e-6
    assert np.all(bound >= np.abs(y) - 1e-12)


@pytest.mark.parametrize("freq", [440.0, 1000.0])
@pytest.mark.parametrize("orig,new", R.AUDIO_PAIRS, ids=lambda v: str(v))
def test_reference_resamples_a_sine_to_the_analytic_sine(orig, new, freq):
    y, _, mid = _run(orig, new, np.sin(2.0 * np.pi * freq * np.arange(N_IN) / orig))
    want = np.sin(2.0 * np.pi * freq * np.arange(len(y)) / new)
    worst = float(np.abs(y - want)[mid].max())
    print("sine", freq, orig, new, worst)
    assert worst <= 2e-7


@pytest.mark.parametrize("orig,new", [(44100, 16000), (48000, 16000), (22050, 16000), (3, 2)], ids=lambda v: str(v))
def test_reference_rejects_a_tone_above_the_lower_nyquist(orig, new):
    y, _, mid = _run(orig, new, np.sin(2.0 * np.pi * (1.25 * new / 2.0) * np.arange(N_IN) / orig))
    worst = float(np.abs(y[mid]).max())
    print("stop band", orig, new, worst)
    assert worst <= 1e-6


def test_reference_overshoots_on_a_square_wave():
    """A +-32767 square wave with period 80 at 44.1 kHz leaves the int16 range at 16 kHz: what the GPU saturation test rests on."""
    y, _, _ = _run(44100, 16000, R.square_wave(N_IN))
    print("square wave extremes", y.min(), y.max())
    assert y.max() > 38000.0 and y.min() < -38000.0


def test_resample_arguments_are_checked_before_any_launch():
    """Every CPC_EINVAL case of include/cpc_hip.h returns -22 from the argument check: no kernel is launched, so fake pointers do."""
    assert "cpc_resample" in _hip.EXPORTED_SYMBOLS
    lib = _hip.lib()
    P, s = 0x1000, C.c_void_p(0)         # never dereferenced

    def call(src=P, src_code=1, src_total=1000, Cn=2, mix=1, in_scale=1.0, taps=P, L=160, M=441, W=47, segs=P, tile_first=P, nseg=1,
             ntiles=1, dst=P, dst_code=0, dst_total=400, out_scale=1.0):
        ptr = lambda v: None if v is None else C.c_void_p(v)
        return lib.cpc_resample(ptr(src), src_code, src_total, Cn, mix, in_scale, ptr(taps), L, M, W, ptr(segs), ptr(tile_first), nseg,
                                ntiles, ptr(dst), dst_code, dst_total, out_scale, s)

    for name in ("src", "taps", "segs", "tile_first", "dst"):
        assert call(**{name: None}) == -22, name
    assert call(Cn=0) == -22 and call(Cn=9) == -22 and call(Cn=-1) == -22
    for name in ("mix", "src_code", "dst_code"):
        assert call(**{name: 2}) == -22 and call(**{name: -1}) == -22, name
    assert call(L=0) == -22 and call(M=0) == -22 and call(L=-3) == -22 and call(M=-1) == -22 and call(W=-1) == -22
    assert call(L=(1 << 20) + 1) == -22 and call(M=(1 << 20) + 1, L=1 << 20) == -22
    assert call(L=1 << 20, M=1 << 20, W=8) == -22                                   # L (2 W + 1) > 2^24
    assert call(nseg=0) == -22 and call(nseg=-1) == -22 and call(ntiles=0) == -22 and call(ntiles=(1 << 23) + 1) == -22
    assert call(src_total=0) == -22 and call(dst_total=0) == -22 and call(src_total=(1 << 40) + 1) == -22 and call(dst_total=-5) == -22
    for name in ("in_scale", "out_scale"):
        assert call(**{name: float("inf")}) == -22 and call(**{name: float("nan")}) == -22, name
    assert call(src=P + 1) == -22 and call(src_code=0, src=P + 2) == -22            # not aligned to the element size
    assert call(dst=P + 2) == -22 and call(dst_code=1, dst=P + 1) == -22
    assert call(taps=P + 2) == -22 and call(segs=P + 4) == -22 and call(tile_first=P + 4) == -22
    # the input span of a tile must fit 16384 floats of LDS: 1023 M div L + 2 W + 2
    assert call(L=1, M=16, W=8) == -22 and call(L=1, M=1, W=7681) == -22
    assert resampling.TILE == 1024 and resampling.MAX_SPAN_FLOATS == 16384


# ---------------------------------------------------------------------------------------------------------------- the dataset
def _write_pcm(path, frames, rate, width):
    """frames: integer array [n] or [n, channels] in the width's own range (8-bit: unsigned)."""
    frames = np.asarray(frames)
    channels = 1 if frames.ndim == 1 else frames.shape[1]
    if width == 1:
        raw = frames.astype(np.uint8).tobytes()
    elif width == 2:
        raw = frames.astype("<i2").tobytes()
    elif width == 4:
        raw = frames.astype("<i4").tobytes()
    else:
        v = frames.astype(np.int64).reshape(-1) & 0xFFFFFF
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


def _write_float_wav(path, samples, rate):
    data = np.asarray(samples, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)          # format tag 3: IEEE float
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def _integers(width, shape, seed):
    rng = np.random.default_rng(seed)
    if width == 1:
        a = rng.integers(0, 256, size=shape)
        a.reshape(-1)[:2] = [0, 255]
    else:
        top = 1 << (8 * width - 1)
        a = rng.integers(-top, top, size=shape)
        a.reshape(-1)[:2] = [-top, top - 1]
    return a


def _as_float(width, a):
    """The loader's rule for a file of that width: int16 as it is, the others as float32 in [-1, 1)."""
    if width == 2:
        return a.astype(np.int16)
    if width == 1:
        return ((a.astype(np.float64) - 128.0) / 128.0).astype(np.float32)
    x = (a.astype(np.float64) / float(1 << (8 * width - 1))).astype(np.float32)
    return np.minimum(x, np.float32(1.0 - 2.0 ** -24))


def _downmix(x, channels):
    """float32 [n] from [n] or [n, C] in the source's own units: channel 0, or the channels summed in order in float32 over C."""
    x = x.reshape(len(x), -1).astype(np.float32)
    if channels == "first":
        return x[:, 0].copy()
    total = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        total = total + x[:, c]
    return total / np.float32(x.shape[1])


@pytest.mark.parametrize("channels", ["first", "mean"])
@pytest.mark.parametrize("storage", ["int16", "float32"])
def test_convert_without_a_device(tmp_path, storage, channels):
    """8-, 16-, 24- and 32-bit files, mono and stereo, at the dataset's rate: lengths and samples against numpy."""
    sources, want, lengths = [], [], []
    for k, (width, nch) in enumerate([(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2)]):
        n = 130 + 17 * k
        a = _integers(width, (n,) if nch == 1 else (n, nch), seed=k)
        _write_pcm(tmp_path / f"f{k}_{8 * width}bit_{nch}ch.wav", a, 16000, width)
        x = _downmix(_as_float(width, a), channels)
        unit = np.float32(1.0 if width != 2 else 1.0 / 32768.0)          # x in units of full scale
        if storage == "int16":
            stored = np.rint(np.clip(x if width == 2 else x * np.float32(32768.0), -32768.0, 32767.0)).astype(np.int16)
            want.append(stored.astype(np.float32) * np.float32(1.0 / 32768.0))
        else:
            want.append(x * unit)
        lengths.append(n)
    ds = DeviceAudioDataset(tmp_path, item_length=50, unique_length=25, storage=storage, convert=True, channels=channels)
    assert ds.file_lengths == lengths and ds.convert and ds.channels == channels and ds.hbm_bytes() == 0
    want = np.concatenate(want)
    assert len(ds) == (len(want) - 25) // 25
    for i in range(len(ds)):
        assert np.array_equal(ds[i].numpy(), want[25 * i:25 * i + 50]), i


@pytest.mark.parametrize("storage", ["int16", "float32"])
def test_convert_of_mono_16_bit_files_is_bit_identical_to_the_plain_loader(tmp_path, storage):
    rng = np.random.default_rng(3)
    for k, n in enumerate([400, 1, 333]):
        a = rng.integers(-32768, 32768, size=n)
        a[:1] = -32768
        _write_pcm(tmp_path / f"{k}.wav", a, 16000, 2)
    kw = dict(item_length=64, unique_length=16, storage=storage, labels=True)
    plain, conv = DeviceAudioDataset(tmp_path, **kw), DeviceAudioDataset(tmp_path, convert=True, **kw)
    assert plain.file_lengths == conv.file_lengths and len(plain) == len(conv) > 10
    assert conv._host.dtype == plain._host.dtype and torch.equal(conv._host, plain._host)
    for i in range(len(plain)):
        assert torch.equal(plain[i][0], conv[i][0]) and int(plain[i][1]) == int(conv[i][1])
    # arrays take the same route: (frames,) and (frames, 1) are the same file
    a = rng.integers(-32768, 32768, size=300).astype(np.int16)
    one = DeviceAudioDataset(arrays=[a], item_length=64, storage=storage)
    two = DeviceAudioDataset(arrays=[a.reshape(-1, 1)], item_length=64, storage=storage, convert=True, array_rates=16000)
    assert torch.equal(one._host, two._host)


def test_convert_without_a_device_refuses_what_needs_the_device_or_another_decoder(tmp_path):
    _write_pcm(tmp_path / "a" / "ok.wav", np.zeros(50, np.int64), 16000, 2)
    _write_pcm(tmp_path / "a" / "slow.wav", np.zeros(50, np.int64), 8000, 2)
    with pytest.raises(ValueError, match="slow.wav"):          # resampling runs on the device
        DeviceAudioDataset(tmp_path / "a", item_length=10, convert=True)
    assert len(DeviceAudioDataset(arrays=[np.zeros(50, np.int16)], item_length=10, convert=True, sampling_rate=8000,
                                  array_rates=[8000])) == 5
    with pytest.raises(ValueError, match=r"arrays\[1\]"):
        DeviceAudioDataset(arrays=[np.zeros(50, np.int16), np.zeros((50, 2), np.float32)], item_length=10, convert=True,
                           array_rates=[16000, 44100], storage="float32")
    os.makedirs(tmp_path / "b")
    _write_pcm(tmp_path / "b" / "ok.wav", np.zeros(50, np.int64), 16000, 2)
    _write_float_wav(tmp_path / "b" / "float.wav", np.zeros(50), 16000)
    with pytest.raises(ValueError, match="float.wav"):
        DeviceAudioDataset(tmp_path / "b", item_length=10, convert=True)
    # the new options are opt-in and checked
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros(50, np.int16)], item_length=10, channels="mean")          # needs convert=True
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros(50, np.int16)], item_length=10, array_rates=8000)         # needs convert=True
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros(50, np.int16)], item_length=10, convert=True, channels="left")
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros(50, np.int16)], item_length=10, convert=True, array_rates=[16000, 16000])
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros((50, 9), np.int16)], item_length=10, convert=True)
    with pytest.raises(RuntimeError):
        resampling.resample(torch.zeros(100), 44100, 16000)                                           # no CPU fallback
