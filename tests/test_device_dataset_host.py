"""DeviceAudioDataset without a GPU: the index semantics against the naive restatement (device_dataset_reference.py), the WAV loader,
the two storages, the setters, labels, the sampler and the DataLoader route; and cpc_window_gather's argument checks, which return
before any launch."""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import DeviceAudioDataset, FileBatchSampler

import device_dataset_reference as R

LENGTHS = [[1000], [700, 1, 1300], [512, 512, 512], [300, 2000]]
WINDOWS = [(256, 256), (256, 64), (257, 1), (300, 128)]


@pytest.mark.parametrize("cross_files", [True, False])
@pytest.mark.parametrize("item_length,unique_length", WINDOWS)
@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda v: "-".join(map(str, v)))
def test_index_semantics_against_the_naive_restatement(lengths, item_length, unique_length, cross_files):
    """len, the examples per file (which sum to len), the file of every example and every window, sample for sample."""
    ints, floats = R.make_files(lengths, seed=len(lengths))
    make = lambda: DeviceAudioDataset(arrays=ints, item_length=item_length, unique_length=unique_length, cross_files=cross_files,
                                      labels=True)
    if not cross_files and min(lengths) < item_length:
        with pytest.raises(ValueError, match=r"arrays\[\d\]"):
            make()
        return
    ds = make()
    n = R.length(lengths, item_length, unique_length, cross_files)
    assert n > 0 and len(ds) == n
    assert ds.start_samples == R.start_samples(lengths, item_length, cross_files)
    counts = ds.get_example_count_per_file()
    assert counts == R.example_count_per_file(lengths, item_length, unique_length, cross_files) and sum(counts) == n
    for i in range(n):
        clip, label = ds[i]
        f, pos = R.position(lengths, item_length, unique_length, cross_files, i)
        assert label.dtype == torch.int64 and label.dim() == 0 and int(label) == f, i
        assert ds.get_position(i) == (f, pos)
        want = R.window(floats, item_length, unique_length, cross_files, i)
        assert clip.dtype == torch.float32 and clip.shape == (item_length,)
        assert np.array_equal(clip.numpy(), want), i
    with pytest.raises(IndexError):
        ds[n]


def test_the_bisect_left_quirk_is_kept():
    """An example that starts exactly on a later file's first sample belongs to the file in front of it."""
    ints, _ = R.make_files([512, 512, 512])
    ds = DeviceAudioDataset.from_arrays(ints, 256, unique_length=256, labels=True)
    assert [int(ds[i][1]) for i in range(len(ds))] == [0, 0, 0, 1, 1, 2]
    assert ds.get_example_count_per_file() == [2, 2, 2]


def _write_wav(path, samples, rate=16000, width=2, channels=1):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(samples.tobytes())


def test_wav_loading(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.integers(-32768, 32768, size=900).astype("<i2")
    a[:2] = [-32768, 32767]
    stereo = rng.integers(-32768, 32768, size=(700, 2)).astype("<i2")
    c = rng.integers(-32768, 32768, size=400).astype("<i2")
    _write_wav(tmp_path / "b" / "x.wav", a)
    _write_wav(tmp_path / "a" / "deep" / "y.wav", stereo, channels=2)
    _write_wav(tmp_path / "c.wav", c)
    (tmp_path / "notes.txt").write_text("not audio")
    ds = DeviceAudioDataset(tmp_path, item_length=100, unique_length=50)
    # sorted recursive discovery: a/deep/y.wav, b/x.wav, c.wav
    assert [os.path.relpath(f, tmp_path) for f in ds.files] == [os.path.join("a", "deep", "y.wav"), os.path.join("b", "x.wav"), "c.wav"]
    assert ds.file_lengths == [700, 900, 400]
    want = np.concatenate([stereo[:, 0], a, c]).astype(np.float32) / np.float32(32768.0)       # channel 0 of the stereo file
    for i in range(len(ds)):
        assert np.array_equal(ds[i].numpy(), want[50 * i:50 * i + 100])
    # the int16 extremes: exactly -1.0 and 32767 / 32768
    first = DeviceAudioDataset(tmp_path / "b", item_length=2)[0]
    assert first[0].item() == -1.0 and first[1].item() == 32767.0 / 32768.0
    two = DeviceAudioDataset(tmp_path, item_length=100, max_file_count=2)
    assert len(two.files) == 2 and two.file_lengths == [700, 900]
    with pytest.raises(ValueError):
        DeviceAudioDataset(tmp_path / "nothing_here", item_length=10)


@pytest.mark.parametrize("width", [1, 3])
def test_other_sample_widths_are_refused_by_name(tmp_path, width):
    _write_wav(tmp_path / "ok.wav", np.zeros(50, "<i2"))
    _write_wav(tmp_path / "wide.wav", np.zeros(50 * width, np.uint8), width=width)
    with pytest.raises(ValueError, match="wide.wav"):
        DeviceAudioDataset(tmp_path, item_length=10)


def test_another_sampling_rate_is_refused_by_name(tmp_path):
    _write_wav(tmp_path / "slow.wav", np.zeros(50, "<i2"), rate=8000)
    with pytest.raises(ValueError, match="slow.wav"):
        DeviceAudioDataset(tmp_path, item_length=10)
    assert len(DeviceAudioDataset(tmp_path, item_length=10, sampling_rate=8000)) == 5


def test_sources_and_storage():
    ints, floats = R.make_files([300, 2000], seed=3)
    a = DeviceAudioDataset(arrays=ints, item_length=300, unique_length=128, storage="int16")
    b = DeviceAudioDataset(arrays=ints, item_length=300, unique_length=128, storage="float32")
    c = DeviceAudioDataset(arrays=[torch.from_numpy(floats[0]), ints[1]], item_length=300, unique_length=128, storage="float32")
    assert len(a) == len(b) == len(c) > 0
    for i in range(len(a)):
        assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i])
    assert a.files is None and a.hbm_bytes() == 0 and a.device is None
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=floats, item_length=300, storage="int16")          # int16 storage needs int16 sources
    with pytest.raises(ValueError):
        DeviceAudioDataset(item_length=300)                                          # neither source
    with pytest.raises(ValueError):
        DeviceAudioDataset("somewhere", item_length=300, arrays=ints)                # both
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros((4, 4), np.int16)], item_length=2)
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=[np.zeros(40, np.float64)], item_length=2, storage="float32")
    with pytest.raises(ValueError):
        DeviceAudioDataset(arrays=ints, item_length=300, keep_host=False)            # no device and no host copy
    with pytest.raises(RuntimeError):
        a.device_batch([0, 1])                                                       # no silent host route for a device batch


def test_the_setters_rebuild_the_table():
    lengths = [700, 1, 1300]
    ints, floats = R.make_files(lengths, seed=8)
    ds = DeviceAudioDataset(arrays=ints, item_length=256, unique_length=64)
    for item, unique in ((300, 64), (300, 128)):
        ds.item_length = item
        ds.unique_length = unique
        assert (ds.item_length, ds.unique_length) == (item, unique)
        assert len(ds) == R.length(lengths, item, unique, True)
        assert ds.get_example_count_per_file() == R.example_count_per_file(lengths, item, unique, True)
        for i in range(len(ds)):
            assert np.array_equal(ds[i].numpy(), R.window(floats, item, unique, True, i))
    short = DeviceAudioDataset(arrays=ints[::2], item_length=256, cross_files=False)
    with pytest.raises(ValueError):
        short.item_length = 701


def test_sampler_and_dataloader_over_a_host_only_dataset():
    ints, floats = R.make_files([700, 1, 1300], seed=2)
    ds = DeviceAudioDataset(arrays=ints, item_length=256, unique_length=64)
    sampler = FileBatchSampler(ds.get_example_count_per_file(), batch_size=4, file_batch_size=2, drop_last=True, seed=1, verbose=False)
    lists = [list(b) for b in sampler]
    assert lists and sorted(i for b in lists for i in b) == sorted(set(i for b in lists for i in b))
    assert max(i for b in lists for i in b) < len(ds)
    sampler = FileBatchSampler(ds.get_example_count_per_file(), batch_size=4, file_batch_size=2, drop_last=True, seed=1, verbose=False)
    loader = torch.utils.data.DataLoader(ds, batch_sampler=sampler, num_workers=0)
    got = list(loader)
    assert len(got) == len(lists)
    for batch, idx in zip(got, lists):
        assert batch.shape == (4, 256) and batch.dtype == torch.float32
        for row, i in zip(batch, idx):
            assert np.array_equal(row.numpy(), R.window(floats, 256, 64, True, i))
    labelled = DeviceAudioDataset(arrays=ints, item_length=256, unique_length=64, labels=True)
    clips, labels = next(iter(torch.utils.data.DataLoader(labelled, batch_size=5)))
    assert clips.shape == (5, 256) and labels.dtype == torch.int64 and labels.tolist() == [0] * 5


def test_window_gather_arguments_are_checked_before_any_launch():
    """Every CPC_EINVAL case of include/cpc_hip.h returns -22 from the argument check: no kernel is launched, so fake pointers do."""
    assert "cpc_window_gather" in _hip.EXPORTED_SYMBOLS
    lib = _hip.lib()
    P, s = 0x1000, C.c_void_p(0)         # never dereferenced

    def gather(store=P, code=1, store_len=100, starts=P, n_items=5, idx=P, out=P, B=2, L=10, ldo=10, scale=1.0):
        ptr = lambda v: None if v is None else C.c_void_p(v)
        return lib.cpc_window_gather(ptr(store), code, store_len, ptr(starts), n_items, ptr(idx), ptr(out), B, L, ldo, scale, s)

    for name in ("store", "starts", "idx", "out"):
        assert gather(**{name: None}) == -22, name
    assert gather(B=0) == -22 and gather(B=65536) == -22 and gather(B=-1) == -22
    assert gather(L=0) == -22 and gather(L=(1 << 24) + 1, ldo=(1 << 24) + 1, store_len=1 << 30) == -22
    assert gather(ldo=9) == -22 and gather(store_len=9) == -22 and gather(n_items=0) == -22
    assert gather(code=2) == -22 and gather(code=-1) == -22
    assert gather(scale=float("inf")) == -22 and gather(scale=float("nan")) == -22
    assert gather(code=1, store=P + 1) == -22 and gather(code=0, store=P + 2) == -22          # not aligned to the element size
    assert gather(out=P + 2) == -22
