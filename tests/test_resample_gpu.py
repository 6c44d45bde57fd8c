"""cpc_resample, resampling.resample and DeviceAudioDataset(convert=True) on the GPU: the kernel against the float64 restatement
(resample_reference.py) under the derived rounding bound, the segment borders (no sample of a neighbour enters), the int16 store bit
for bit against the rounded f32 store, the identity table, the guard, the argument checks, and the dataset over files of three rates."""
import os
import random
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip, resampling  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, softplus_score_function  # noqa: E402

import device_dataset_reference as D  # noqa: E402
import resample_reference as R  # noqa: E402

DEV = "cuda:0"
TILE = 1024
GAP, GUARD = 5, 64          # untouched elements between the segments' outputs, and behind the last
SENT_F, SENT_I = -7.5, 12345
PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (16000, 44100), (16000, 16000)]
MIX = {"first": 0, "mean": 1}

_TAPS = {}


def _taps(orig, new):
    """(taps [L, 2 W + 1] float32, L, M, W, the transposed table on the device), once per rate pair."""
    if (orig, new) not in _TAPS:
        taps, L, M, W = resampling.resample_taps(orig, new)
        _TAPS[(orig, new)] = (taps, L, M, W, torch.from_numpy(np.ascontiguousarray(taps.T)).to(DEV))
    return _TAPS[(orig, new)]


def _gamma(k):
    u = k * 2.0 ** -24
    return u / (1.0 - u)


def _source(code, frames, C, seed):
    """[frames, C] samples: every int16 value range, or floats in [-1, 1)."""
    rng = np.random.default_rng(seed)
    if code == 1:
        a = rng.integers(-32768, 32768, size=(frames, C)).astype(np.int16)
        a.reshape(-1)[:2] = [-32768, 32767]
        return a
    return rng.uniform(-1.0, 1.0, size=(frames, C)).astype(np.float32)


def _fifth(L, M, target):
    """The fewest frames whose output count reaches target (for L <= M it is target exactly)."""
    n = (target * M) // L
    while R.output_count(n, L, M) < target:
        n += 1
    while n > 1 and R.output_count(n - 1, L, M) >= target:
        n -= 1
    return n


def _layout(frames, counts):
    """Segments back to back in the source, GAP elements apart in the output: (segs int64 [n, 4], dst elements without the guard)."""
    segs, s, d = [], 0, 0
    for n, c in zip(frames, counts):
        segs.append([s, n, d, c])
        s, d = s + n, d + c + GAP
    return np.asarray(segs, dtype=np.int64), d


def _launch(src, C, mix, in_scale, pair, segs, dst, out_scale, tile_first=None, src_total=None, dst_total=None, ntiles=None):
    """The raw entry point with tables made here.  src: device tensor of interleaved frames; dst: device tensor (with its guard)."""
    _, L, M, W, taps_dev = _taps(*pair)
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    if tile_first is None:
        tiles = -(-np.maximum(segs[:, 3], 0) // TILE)
        tile_first = np.concatenate([np.zeros(1, np.int64), np.cumsum(tiles)[:-1]])
        ntiles = int(tiles.sum()) if ntiles is None else ntiles
    table = torch.from_numpy(np.concatenate([segs.reshape(-1), np.asarray(tile_first, dtype=np.int64)])).to(DEV)
    _hip.call("cpc_resample", _hip.ptr(src), 1 if src.dtype == torch.int16 else 0, src.numel() // C if src_total is None else src_total,
              C, mix, in_scale, _hip.ptr(taps_dev), L, M, W, _hip.ptr(table), _hip.ptr(table, 4 * len(segs)), len(segs), ntiles,
              _hip.ptr(dst), 1 if dst.dtype == torch.int16 else 0, dst.numel() - GUARD if dst_total is None else dst_total, out_scale)
    torch.cuda.synchronize()


def _buffer(n, dtype=torch.float32):
    """n output elements of NaN (int16: SENT_I) with the guard's sentinels behind them."""
    if dtype == torch.int16:
        return torch.full((n + GUARD,), SENT_I, device=DEV, dtype=torch.int16)
    buf = torch.full((n + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    buf[n:] = SENT_F
    return buf


def _untouched(buf, segs, n):
    """Everything outside the segments' output ranges is as _buffer left it."""
    host = buf.cpu()
    keep = torch.ones(n + GUARD, dtype=torch.bool)
    for _, _, d, c in segs.tolist():
        keep[d:d + c] = False
    if host.dtype == torch.int16:
        return bool((host[keep] == SENT_I).all())
    return bool(torch.isnan(host[:n][keep[:n]]).all()) and bool((host[n:] == SENT_F).all())


_WORST = [0.0]


def _check_segments(buf, host_src, segs, pair, mix_name, in_scale, out_scale, C, only=None):
    taps, L, M, W, _ = _taps(*pair)
    got = buf.cpu().numpy().astype(np.float64)
    g = _gamma((2 * W + 1) + C + 3)
    for k, (s, n, d, c) in enumerate(segs.tolist()):
        if only is not None and k != only:
            continue
        y, bound = R.resample(host_src[s:s + n], taps, L, M, W, mix_name, in_scale, out_scale)
        assert c <= len(y)
        err = np.abs(got[d:d + c] - y[:c])
        live = bound[:c] > 0.0
        if live.any():          # the largest share of the bound any output has used, printed by the kernel test
            _WORST[0] = max(_WORST[0], float((err[live] / (g * bound[:c][live])).max()))
        assert np.all(np.isfinite(got[d:d + c])) and np.all(err <= g * bound[:c]), (pair, k, float((err - g * bound[:c]).max()))


@pytest.mark.parametrize("code", [1, 0], ids=["int16", "f32"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_kernel_against_the_float64_reference(pair, code):
    """Four segments of 1, 37, 2 W + 1 and 2 500 frames and a fifth whose outputs fill one tile exactly, one more, one fewer, in one
    launch each; C in {1, 2, 3}, both mixes; every output within gamma_k bound[n], k = (2 W + 1) + C + 3; nothing else written."""
    _, L, M, W, _ = _taps(*pair)
    in_scale, out_scale = (1.0 / 32768.0, 1.0) if code == 1 else (0.75, 3.0)
    _WORST[0] = 0.0
    for extra in (0, 1, -1):
        target = TILE + extra
        frames = [1, 37, 2 * W + 1, 2500, _fifth(L, M, target)]
        counts = [R.output_count(n, L, M) for n in frames[:4]] + [target]          # (up-sampling: the fifth is cut at the target)
        assert counts[4] <= R.output_count(frames[4], L, M)
        segs, n_dst = _layout(frames, counts)
        for C in (1, 2, 3):
            host = _source(code, sum(frames), C, seed=C + 10 * (extra + 1))
            src = torch.from_numpy(host).to(DEV)
            for mix_name in ("first", "mean"):
                buf = _buffer(n_dst)
                _launch(src, C, MIX[mix_name], in_scale, pair, segs, buf, out_scale)
                _check_segments(buf, host, segs, pair, mix_name, in_scale, out_scale, C)
                assert _untouched(buf, segs, n_dst)
    print(f"resample {pair[0]} -> {pair[1]}, {'int16' if code else 'f32'} source: worst error / (gamma_k bound) = {_WORST[0]:.4f}")


@pytest.mark.parametrize("pair", [(44100, 16000), (8000, 16000)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_no_sample_of_a_neighbouring_segment_enters(pair):
    """f32 sources: one segment at a time holds finite data, every other frame is NaN; its outputs are finite and within the bound.
    And mix = first with NaN in the channels 1 .. C - 1 of every frame."""
    _, L, M, W, _ = _taps(*pair)
    frames = [1, 37, 2 * W + 1, 1200, 3]
    segs, n_dst = _layout(frames, [R.output_count(n, L, M) for n in frames])
    for C, mix_name in ((1, "first"), (2, "mean"), (3, "first")):
        clean = _source(0, sum(frames), C, seed=7 + C)
        for k, (s, n, _, _) in enumerate(segs.tolist()):
            host = np.full_like(clean, np.nan)
            host[s:s + n] = clean[s:s + n]
            buf = _buffer(n_dst)
            _launch(torch.from_numpy(host).to(DEV), C, MIX[mix_name], 1.0, pair, segs, buf, 1.0)
            _check_segments(buf, host, segs, pair, mix_name, 1.0, 1.0, C, only=k)
            assert _untouched(buf, segs, n_dst)
    host = _source(0, sum(frames), 3, seed=3)
    host[:, 1:] = np.nan
    buf = _buffer(n_dst)
    _launch(torch.from_numpy(host).to(DEV), 3, MIX["first"], 1.0, pair, segs, buf, 1.0)
    _check_segments(buf, host, segs, pair, "first", 1.0, 1.0, 3)


@pytest.mark.parametrize("code", [1, 0], ids=["int16", "f32"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_int16_store_is_the_rounded_f32_store(pair, code):
    """The int16 destination equals torch.round(torch.clamp(f32 destination, -32768, 32767)) bit for bit for the same launch and
    scales; the scales put part of the outputs beyond the range, so that the saturation is met."""
    _, L, M, W, _ = _taps(*pair)
    frames = [1, 37, 2 * W + 1, 2500, _fifth(L, M, TILE + 1)]
    counts = [R.output_count(n, L, M) for n in frames[:4]] + [TILE + 1]
    segs, n_dst = _layout(frames, counts)
    for C, mix_name in ((1, "first"), (2, "mean"), (3, "mean")):
        src = torch.from_numpy(_source(code, sum(frames), C, seed=C)).to(DEV)
        for in_scale, out_scale in ((1.0, 1.0), (1.0, 8.0)) if code == 1 else ((1.0, 32768.0), (0.9, 3.0e5)):
            f, q = _buffer(n_dst), _buffer(n_dst, torch.int16)
            _launch(src, C, MIX[mix_name], in_scale, pair, segs, f, out_scale)
            _launch(src, C, MIX[mix_name], in_scale, pair, segs, q, out_scale)
            assert _untouched(q, segs, n_dst)
            f, q = f.cpu(), q.cpu()
            hit = 0
            for _, _, d, c in segs.tolist():
                want = torch.round(torch.clamp(f[d:d + c], -32768.0, 32767.0)).to(torch.int16)
                assert torch.equal(q[d:d + c], want)
                hit += int((f[d:d + c].abs() > 32768.0).sum())
            assert hit > 0 or out_scale in (1.0, 32768.0)


def test_a_square_wave_saturates():
    """The +-32767 square wave of the host test, 44.1 kHz to 16 kHz: 32767 / -32768 wherever the reference leaves the range."""
    pair = (44100, 16000)
    taps, L, M, W, _ = _taps(*pair)
    x = R.square_wave(6000)
    y, _ = R.resample(x, taps, L, M, W)
    segs, n_dst = _layout([len(x)], [len(y)])
    q = _buffer(n_dst, torch.int16)
    _launch(torch.from_numpy(x).to(DEV), 1, 0, 1.0, pair, segs, q, 1.0)
    got = q.cpu().numpy()[:len(y)]
    over, under = y > 32768.0, y < -32769.0
    assert over.sum() > 20 and under.sum() > 20
    assert np.all(got[over] == 32767) and np.all(got[under] == -32768)
    inside = np.abs(y) < 32000.0
    assert np.all(np.abs(got[inside] - y[inside]) <= 0.5 + 1e-2) and _untouched(q, segs, n_dst)


def test_identity_table():
    """W = 0, L = M = 1, taps = {1}: int16 mono to f32 with in_scale = 2^-15 is x / 32768 bit for bit, int16 to int16 is a copy, and
    a stereo file's mean goes through the same launch."""
    pair = (16000, 16000)
    assert _taps(*pair)[1:4] == (1, 1, 0)
    x = _source(1, 3000, 1, seed=1)
    x[:65536 // 32].reshape(-1)[:] = np.arange(-32768, 32768, 32, dtype=np.int64).astype(np.int16)
    frames = [1, 1023, 1025, 951]
    segs, n_dst = _layout(frames, frames)
    src = torch.from_numpy(x).to(DEV)
    f, q = _buffer(n_dst), _buffer(n_dst, torch.int16)
    _launch(src, 1, 0, 2.0 ** -15, pair, segs, f, 1.0)
    _launch(src, 1, 1, 1.0, pair, segs, q, 1.0)
    assert _untouched(f, segs, n_dst) and _untouched(q, segs, n_dst)
    f, q, xt = f.cpu(), q.cpu(), torch.from_numpy(x.reshape(-1))
    for s, n, d, c in segs.tolist():
        assert torch.equal(f[d:d + c].view(torch.int32), (xt[s:s + n].to(torch.float32) / 32768.0).view(torch.int32))
        assert torch.equal(q[d:d + c], xt[s:s + n])
    st = _source(1, 3000, 2, seed=2)
    f = _buffer(n_dst)
    _launch(torch.from_numpy(st).to(DEV), 2, 1, 1.0, pair, segs, f, 1.0)
    want = (st[:, 0].astype(np.float32) + st[:, 1].astype(np.float32)) / np.float32(2.0)
    for s, n, d, c in segs.tolist():
        assert np.array_equal(f.cpu().numpy()[d:d + c], want[s:s + n])


def test_segments_outside_the_buffers_are_skipped():
    """Valid calls with a defined result: table entries that reach in front of 0 or behind either total, or are negative, leave their
    outputs untouched beside correctly converted neighbours; so does a tile that a wrong tile table places behind its segment's end."""
    pair = (44100, 16000)
    _, L, M, W, _ = _taps(*pair)
    host = _source(1, 6000, 2, seed=5)
    src = torch.from_numpy(host).to(DEV)
    oc = lambda n: R.output_count(n, L, M)
    good = [[0, 2900, 0, oc(2900)], [2900, 1000, 1200, oc(1000)], [3900, 2100, 3200, oc(2100)]]
    n_dst = 4200
    bad = [[-1, 500, 1700, 180], [5900, 101, 1700, 36], [1 << 50, 10, 1700, 4], [100, -5, 1700, 4], [-(1 << 50), 100, 1700, 30],
           [100, 500, -3, 100], [100, 500, n_dst - 50, 51], [100, 500, 1 << 50, 100], [100, 500, 1700, -7], [100, 500, 1700, 1 << 50],
           [100, 1 << 62, 1700, 100]]
    for entry in bad:
        segs = np.asarray([good[0], entry, good[1], good[2]], dtype=np.int64)
        buf = _buffer(n_dst)
        # tiles 2, 1, 1, 1: every segment has its tiles, whatever its entry says
        _launch(src, 2, 1, 1.0 / 32768.0, pair, segs, buf, 1.0, tile_first=np.asarray([0, 2, 3, 4]), ntiles=5)
        kept = np.asarray(good, dtype=np.int64)
        _check_segments(buf, host, kept, pair, "mean", 1.0 / 32768.0, 1.0, 2)
        assert _untouched(buf, kept, n_dst), entry
    # totals stated shorter than the allocations: a segment inside the allocation but outside the stated range is skipped as well
    segs = np.asarray(good, dtype=np.int64)
    buf = _buffer(n_dst)
    _launch(src, 2, 1, 1.0 / 32768.0, pair, segs, buf, 1.0, src_total=5999, dst_total=n_dst)
    _check_segments(buf, host, segs[:2], pair, "mean", 1.0 / 32768.0, 1.0, 2)
    assert _untouched(buf, segs[:2], n_dst)
    buf = _buffer(n_dst)
    _launch(src, 2, 1, 1.0 / 32768.0, pair, segs, buf, 1.0, dst_total=int(segs[2, 2] + segs[2, 3]) - 1)
    assert _untouched(buf, segs[:2], n_dst)
    # a tile table that gives the first segment a tile too many: the tile behind the segment's end writes nothing
    buf = _buffer(n_dst)
    _launch(src, 2, 1, 1.0 / 32768.0, pair, segs, buf, 1.0, tile_first=np.asarray([0, 3, 4]), ntiles=5)
    _check_segments(buf, host, segs, pair, "mean", 1.0 / 32768.0, 1.0, 2)
    assert _untouched(buf, segs, n_dst)


def test_resample_refuses_bad_arguments():
    """Every CPC_EINVAL case of include/cpc_hip.h raises _hip.HipCallError, and the output is not touched."""
    import ctypes as C
    pair = (44100, 16000)
    _, L, M, W, taps_dev = _taps(*pair)
    src = torch.from_numpy(_source(1, 500, 2, seed=1)).to(DEV)
    fsrc = torch.zeros(1000, device=DEV)
    n_out = R.output_count(500, L, M)
    table = torch.tensor([0, 500, 0, n_out, 0], dtype=torch.int64, device=DEV)
    out = torch.full((n_out + GUARD,), SENT_F, device=DEV)
    p = _hip.ptr
    odd = lambda t, by: C.c_void_p(t.data_ptr() + by)

    def call(src_=p(src), src_code=1, src_total=500, Cn=2, mix=1, in_scale=1.0, taps=p(taps_dev), L=L, M=M, W=W, segs=p(table),
             tile_first=p(table, 4), nseg=1, ntiles=1, dst=p(out), dst_code=0, dst_total=n_out, out_scale=1.0):
        _hip.call("cpc_resample", src_, src_code, src_total, Cn, mix, in_scale, taps, L, M, W, segs, tile_first, nseg, ntiles, dst,
                  dst_code, dst_total, out_scale)

    bad = [dict(src_=None), dict(taps=None), dict(segs=None), dict(tile_first=None), dict(dst=None), dict(Cn=0), dict(Cn=9),
           dict(mix=2), dict(mix=-1), dict(src_code=2), dict(dst_code=-1), dict(L=0), dict(M=0), dict(W=-1), dict(L=(1 << 20) + 1),
           dict(M=(1 << 20) + 1), dict(L=1 << 20, M=1 << 20, W=8), dict(nseg=0), dict(ntiles=0), dict(ntiles=(1 << 23) + 1),
           dict(src_total=0), dict(dst_total=0), dict(src_total=(1 << 40) + 1), dict(in_scale=float("inf")), dict(out_scale=float("nan")),
           dict(src_=odd(src, 1)), dict(src_=odd(fsrc, 2), src_code=0), dict(dst=odd(out, 2)), dict(dst=odd(out, 1), dst_code=1),
           dict(taps=odd(taps_dev, 2)), dict(segs=odd(table, 4)), dict(tile_first=odd(table, 36)), dict(L=1, M=16, W=8),
           dict(L=1, M=1, W=7681)]
    for kw in bad:
        with pytest.raises(_hip.HipCallError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == SENT_F).all())
    call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:n_out]).all()) and bool((out[:n_out] != SENT_F).any()) and bool((out[n_out:] == SENT_F).all())


def test_the_public_function():
    """resample() takes (N,) and (B, N), keeps the dtype, refuses a CPU tensor and equals the raw entry point bit for bit."""
    pair = (44100, 16000)
    _, L, M, W, _ = _taps(*pair)
    N, B = 2501, 3
    n_out = R.output_count(N, L, M)
    for code in (1, 0):
        host = _source(code, B * N, 1, seed=code).reshape(B, N)
        x = torch.from_numpy(host).to(DEV)
        y = resampling.resample(x, *pair)
        assert y.shape == (B, n_out) and y.dtype == x.dtype and y.device == x.device
        one = resampling.resample(x[1], *pair)
        assert one.shape == (n_out,) and torch.equal(one, y[1])
        r = np.arange(B, dtype=np.int64)
        segs = np.stack([r * N, np.full(B, N), r * n_out, np.full(B, n_out)], axis=1)
        raw = _buffer(B * n_out, x.dtype)
        _launch(x.reshape(-1), 1, 0, 1.0, pair, segs, raw, 1.0)
        assert torch.equal(raw[:B * n_out].view(B, n_out), y)
        with pytest.raises(RuntimeError):
            resampling.resample(x.cpu(), *pair)
    same = resampling.resample(x, 16000, 16000)
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()
    up = resampling.resample(x[0], 8000, 16000, zeros=8)          # the filter's keywords reach the design
    assert up.shape == (2 * N,) and bool(torch.isfinite(up).all())
    with pytest.raises(ValueError):
        resampling.resample(x.to(torch.float64), *pair)
    with pytest.raises(ValueError):
        resampling.resample(x.view(1, B, N), *pair)


# ---------------------------------------------------------------------------------------------------------------- the dataset
def _write(path, frames, rate, width):
    frames = np.asarray(frames)
    channels = 1 if frames.ndim == 1 else frames.shape[1]
    if width == 2:
        raw = frames.astype("<i2").tobytes()
    else:
        v = frames.astype(np.int64).reshape(-1) & 0xFFFFFF
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


def _three_files(folder, n8, n44, n16, seed=0, amplitude=1.0):
    """8 kHz mono 16-bit, 44.1 kHz stereo 24-bit, 16 kHz mono 16-bit; (arrays as written, rates)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(int(-32768 * amplitude), int(32768 * amplitude), size=n8)
    b = rng.integers(int(-(1 << 23) * amplitude), int((1 << 23) * amplitude), size=(n44, 2))
    c = rng.integers(int(-32768 * amplitude), int(32768 * amplitude), size=n16)
    os.makedirs(folder, exist_ok=True)
    _write(os.path.join(folder, "a_8k.wav"), a, 8000, 2)
    _write(os.path.join(folder, "b_44k.wav"), b, 44100, 3)
    _write(os.path.join(folder, "c_16k.wav"), c, 16000, 2)
    return [a, b, c], [8000, 44100, 16000]


def _expected_store(arrays, rates, storage, channels):
    """The store as float32 in units of full scale, from per-file resample() calls on host-side downmixes."""
    out = []
    for a, rate in zip(arrays, rates):
        if a.ndim == 1:          # 16-bit mono
            x = torch.from_numpy(a.astype(np.int16)).to(DEV)
            if storage == "int16":
                y = resampling.resample(x, rate, 16000).to(torch.float32) / 32768.0
            else:
                y = resampling.resample(x.to(torch.float32) / 32768.0, rate, 16000)
        else:                    # 24-bit stereo: float32 in [-1, 1), exact
            f = a.astype(np.float32) * np.float32(1.0 / 8388608.0)
            mono = f[:, 0] if channels == "first" else (f[:, 0] + f[:, 1]) / np.float32(2.0)
            y = resampling.resample(torch.from_numpy(np.ascontiguousarray(mono)).to(DEV), rate, 16000)
            if storage == "int16":
                y = torch.round(torch.clamp(y * 32768.0, -32768.0, 32767.0)) / 32768.0
        out.append(y.cpu())
    return out


class _Spy:
    def __enter__(self):
        self.names, self.real = [], _hip.call

        def spy(name, *a, **kw):
            self.names.append(name)
            return self.real(name, *a, **kw)

        _hip.call = spy
        return self

    def __exit__(self, *exc):
        _hip.call = self.real


@pytest.mark.parametrize("channels", ["first", "mean"])
@pytest.mark.parametrize("storage", ["int16", "float32"])
def test_dataset_converts_files_of_three_rates(tmp_path, storage, channels):
    arrays, rates = _three_files(tmp_path, 2000, 5000, 1500, seed=1)
    kw = dict(item_length=300, unique_length=100, storage=storage, channels=channels, convert=True, device=DEV, labels=True)
    with _Spy() as spy:
        ds = DeviceAudioDataset(tmp_path, **kw)
    assert spy.names.count("cpc_resample") == 3 == ds.convert_launches          # three (rate, channels, sample type) groups
    lengths = [4000, R.output_count(5000, 160, 441), 1500]
    assert ds.file_lengths == lengths and ds._host is None
    assert ds.hbm_bytes() == sum(lengths) * (2 if storage == "int16" else 4) + 2 * 8 * len(ds)
    want = torch.cat(_expected_store(arrays, rates, storage, channels))
    n = len(ds)
    assert n == (sum(lengths) - 200) // 100 > 60
    batch, labels = ds.device_batch(range(n))
    windows = torch.stack([want[100 * i:100 * i + 300] for i in range(n)])
    assert torch.equal(batch.cpu().view(torch.int32), windows.view(torch.int32))
    assert labels.cpu().tolist() == [D.position(lengths, 300, 100, True, i)[0] for i in range(n)] and set(labels.cpu().tolist()) == {0, 1, 2}
    # a host copy is read back from the converted store
    kept = DeviceAudioDataset(tmp_path, keep_host=True, **kw)
    assert torch.equal(kept._host, kept._store.cpu()) and torch.equal(kept._store, ds._store)
    assert torch.equal(kept[7][0], batch[7].cpu())


@pytest.mark.parametrize("storage", ["int16", "float32"])
def test_chunked_conversion_gives_the_identical_store(tmp_path, storage):
    """Three files of one group go through one launch by default and through three with a small convert_chunk_bytes; the three files
    of three rates with a small chunk as well: the same store."""
    rng = np.random.default_rng(2)
    group = [rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16) for n in (1500, 2600, 700)]
    kw = dict(arrays=group, array_rates=44100, item_length=300, unique_length=100, storage=storage, channels="mean", convert=True,
              device=DEV)
    with _Spy() as one:
        whole = DeviceAudioDataset(**kw)
    with _Spy() as three:
        split = DeviceAudioDataset(convert_chunk_bytes=7000, **kw)          # 6000 + 10400 + 2800 bytes: no two files fit a chunk
    assert one.names.count("cpc_resample") == 1 and three.names.count("cpc_resample") == 3
    assert whole.file_lengths == split.file_lengths == [R.output_count(n, 160, 441) for n in (1500, 2600, 700)]
    assert torch.equal(whole._store, split._store) and bool((whole._store != 0).any())
    _three_files(tmp_path, 2000, 5000, 1500, seed=4)
    kw = dict(item_length=300, unique_length=100, storage=storage, channels="mean", convert=True, device=DEV)
    a, b = DeviceAudioDataset(tmp_path, **kw), DeviceAudioDataset(tmp_path, convert_chunk_bytes=1, **kw)
    assert torch.equal(a._store, b._store) and b.convert_launches == 3


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


def test_two_train_steps_fed_by_a_converted_dataset(tmp_path):
    torch.manual_seed(11)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=64, hidden_size=64), enc_size=64, ar_size=64, visible_steps=12,
                                       prediction_steps=4, compute_dtype="fp32").to(DEV)
    item = int(model.item_length)
    _three_files(tmp_path, item, 3 * item, item, seed=6, amplitude=0.125)
    ds = DeviceAudioDataset(tmp_path, item_length=item, unique_length=item // 8, convert=True, channels="mean", device=DEV)
    assert len(ds) >= 16
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=DEV, regularization=0.5,
                                      score_function=softplus_score_function, prediction_steps=4, ar_size=64)
    tr.verbose = False
    random.seed(5)
    torch.manual_seed(7)
    with _Spy() as spy:
        tr.train(batch_size=8, epochs=2, lr=1e-3, num_workers=0, max_steps=2)
    torch.cuda.synchronize()
    assert len(logger.loss_meter.values) == 2 and all(np.isfinite(logger.loss_meter.values)), logger.loss_meter.values
    assert spy.names.count("cpc_window_gather") == 2 and "cpc_resample" not in spy.names          # converted once, at load
