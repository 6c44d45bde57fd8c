"""cpc_window_gather and DeviceAudioDataset on the GPU: the kernel bit for bit against host slicing (both store types, every alignment
of the source and of the output rows, the guard), its argument checks, device_batch against a host twin, and the trainer fed by the
device dataset against the same windows materialised in a TensorAudioDataset: losses and parameters bit for bit."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset, FileBatchSampler, TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.augmentation import WaveAugmentation  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, softplus_score_function  # noqa: E402

import device_dataset_reference as R  # noqa: E402

DEV = "cuda:0"
GUARD = 64          # sentinel elements behind every output
SENT = -7.5


def _store(code, n, seed):
    """(host tensor, device tensor) of n samples: every int16 value, or floats with a denormal, a negative zero and the extremes."""
    g = torch.Generator().manual_seed(seed)
    if code == 1:
        host = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)
        host[0], host[-1] = -32768, 32767
    else:
        host = torch.randn(n, generator=g)
        host[0], host[-1] = -0.0, 3.0e38
        if n > 2:
            host[1] = 1.0e-41
    return host, host.to(DEV)


def _gather(store_dev, code, starts, idx, B, L, ldo, scale, out_offset=0, store_len=None):
    """One launch into a NaN buffer of (B - 1) ldo + L elements with sentinels behind it; (whole buffer, the element count)."""
    n = (B - 1) * ldo + L
    buf = torch.full((out_offset + n + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    buf[out_offset + n:] = SENT
    starts_dev = torch.as_tensor(starts, dtype=torch.int64).to(DEV)
    idx_dev = torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    _hip.call("cpc_window_gather", _hip.ptr(store_dev), code, store_dev.numel() if store_len is None else store_len, _hip.ptr(starts_dev),
              len(starts), _hip.ptr(idx_dev), _hip.ptr(buf, out_offset), B, L, ldo, scale)
    torch.cuda.synchronize()
    return buf.cpu(), n


def _check(buf, n, rows, B, L, ldo, out_offset=0):
    """rows: the expected (B, L) tensor; the gaps between rows still NaN, the buffer's head and the guard untouched."""
    got = buf[out_offset:out_offset + n]
    for b in range(B):
        row = got[b * ldo:b * ldo + L]
        assert torch.equal(row.view(torch.int32), rows[b].view(torch.int32)), b          # bit for bit, signed zeros and denormals too
        if b + 1 < B:
            assert torch.isnan(got[b * ldo + L:(b + 1) * ldo]).all(), b
    assert torch.isnan(buf[:out_offset]).all()
    assert bool((buf[out_offset + n:] == SENT).all())


def _expected(host, starts, idx, L, scale):
    return torch.stack([host[starts[i]:starts[i] + L].to(torch.float32) * scale for i in idx])


@pytest.mark.parametrize("L", [1, 3, 4, 5, 257, 4099])
@pytest.mark.parametrize("code", [0, 1], ids=["f32", "int16"])
def test_window_gather_bit_for_bit(code, L):
    """Starts 0, 1, odd, even and store_len - L (the last sample is read, nothing behind it), B in {1, 3, 64} with repeated indices,
    ldo = L and L + 3, an output that is 16-byte aligned or only 4-byte aligned, scale 1 and 1 / 32768: torch.equal on the bits against
    slices of the host copy.  (A float times 2^-15 is exact unless it leaves the normal range, where both sides round the same way.)"""
    store_len = L + 1000
    host, dev = _store(code, store_len, seed=L)
    starts = [0, 1, 7, 10, store_len - L, 501, 334]
    g = random.Random(L)
    for B in (1, 3, 64):
        idx = [4] if B == 1 else [g.randrange(len(starts)) for _ in range(B)]
        if B == 64:
            idx[:7] = range(7)
            assert len(set(idx)) < B
        for ldo in (L, L + 3):
            for scale in (1.0, 1.0 / 32768.0):
                for off in (0, 1):
                    buf, n = _gather(dev, code, starts, idx, B, L, ldo, scale, out_offset=off)
                    _check(buf, n, _expected(host, starts, idx, L, scale), B, L, ldo, out_offset=off)


@pytest.mark.parametrize("B,L", [(512, 2049), (1024, 4099)])
@pytest.mark.parametrize("code", [0, 1], ids=["f32", "int16"])
def test_window_gather_larger_grids(code, B, L):
    """The launcher sizes its workgroups from B L (256, 1024 or 4096 outputs): the two larger forms, which the shapes above do not
    reach (B ceil(L / 1024) >= 1024, and B ceil(L / 4096) >= 1024)."""
    store_len = 6 * L + 11
    host, dev = _store(code, store_len, seed=B)
    g = random.Random(B)
    starts = [0, 1, store_len - L] + [g.randrange(store_len - L + 1) for _ in range(61)]
    idx = [g.randrange(len(starts)) for _ in range(B)]
    idx[:3] = [0, 1, 2]
    scale = 1.0 if code == 0 else 1.0 / 32768.0
    for ldo in (L, L + 3):
        buf, n = _gather(dev, code, starts, idx, B, L, ldo, scale)
        _check(buf, n, _expected(host, starts, idx, L, scale), B, L, ldo)


@pytest.mark.parametrize("code", [0, 1], ids=["f32", "int16"])
def test_rows_outside_the_store_are_zeros(code):
    """Valid calls with a defined result: an index outside [0, n_items) and a table entry whose window would leave the store (in front
    of it, behind it by one sample, far behind it) give rows of zeros; their neighbours are cut as usual and nothing else is written."""
    L, store_len = 257, 1000
    host, dev = _store(code, store_len, seed=9)
    starts = [5, store_len - L + 1, -3, store_len - L, 1 << 40, -(1 << 40)]
    idx = [0, -1, len(starts), 1, 2, 3, 4, 5, 0]
    scale = 1.0 if code == 0 else 1.0 / 32768.0
    for ldo in (L, L + 3):
        buf, n = _gather(dev, code, starts, idx, len(idx), L, ldo, scale)
        rows = torch.zeros(len(idx), L)
        for b in (0, 5, 8):
            s = starts[idx[b]]
            rows[b] = host[s:s + L].to(torch.float32) * scale
        _check(buf, n, rows, len(idx), L, ldo)
    # a store_len shorter than the allocation: the window that fits the allocation but not the stated store is zeros as well
    buf, n = _gather(dev, code, [store_len - L, 100], [0, 1], 2, L, L, scale, store_len=store_len - 1)
    rows = torch.zeros(2, L)
    rows[1] = host[100:100 + L].to(torch.float32) * scale
    _check(buf, n, rows, 2, L, L)


def test_window_gather_refuses_bad_arguments():
    """Every CPC_EINVAL case of include/cpc_hip.h raises _hip.HipCallError, and the output is not touched."""
    L, B = 10, 2
    host, dev = _store(1, 100, seed=1)
    fdev = torch.zeros(100, device=DEV)
    starts = torch.tensor([0, 5, 90], dtype=torch.int64, device=DEV)
    idx = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    out = torch.full((B * L + GUARD,), SENT, device=DEV)
    p = _hip.ptr

    def call(store=p(dev), code=1, store_len=100, starts_=p(starts), n_items=3, idx_=p(idx), out_=p(out), B=B, L=L, ldo=L, scale=1.0):
        _hip.call("cpc_window_gather", store, code, store_len, starts_, n_items, idx_, out_, B, L, ldo, scale)

    import ctypes as C
    odd = lambda t, by: C.c_void_p(t.data_ptr() + by)
    big = (1 << 24) + 1
    bad = [dict(store=None), dict(starts_=None), dict(idx_=None), dict(out_=None), dict(B=0), dict(B=65536), dict(L=0),
           dict(L=big, ldo=big, store_len=1 << 30), dict(ldo=L - 1), dict(store_len=L - 1), dict(n_items=0), dict(code=2), dict(code=-1),
           dict(scale=float("inf")), dict(scale=float("nan")), dict(store=odd(dev, 1)), dict(store=odd(fdev, 2), code=0),
           dict(out_=odd(out, 2))]
    for kw in bad:
        with pytest.raises(_hip.HipCallError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    call()
    torch.cuda.synchronize()
    assert torch.equal(out[:B * L].cpu().view(B, L), _expected(host, [0, 5, 90], [0, 2], L, 1.0)) and bool((out[B * L:] == SENT).all())


LENGTHS = [700, 301, 1300]


@pytest.mark.parametrize("storage", ["int16", "float32"])
@pytest.mark.parametrize("cross_files", [True, False])
def test_device_batch_against_a_host_twin(cross_files, storage):
    ints, floats = R.make_files(LENGTHS, seed=4)
    kw = dict(arrays=ints, item_length=300, unique_length=128, cross_files=cross_files, storage=storage, labels=True)
    ds, twin = DeviceAudioDataset(device=DEV, **kw), DeviceAudioDataset(**kw)
    assert ds._host is None and twin._store is None and len(ds) == len(twin) > 8
    n = len(ds)
    store_bytes = sum(LENGTHS) * (2 if storage == "int16" else 4)
    assert ds.hbm_bytes() == store_bytes + 2 * 8 * n
    order = list(range(n)) + [n - 1, 0, 0, 3]
    batch, labels = ds.device_batch(order)
    assert batch.shape == (len(order), 300) and batch.dtype == torch.float32 and batch.device == torch.device(DEV)
    assert labels.device == torch.device(DEV) and labels.dtype == torch.int64
    for row, lab, i in zip(batch.cpu(), labels.cpu(), order):
        clip, file_index = twin[i]
        assert torch.equal(row, clip) and int(lab) == int(file_index), i
        assert np.array_equal(clip.numpy(), R.window(floats, 300, 128, cross_files, i))
        assert int(file_index) == R.position(LENGTHS, 300, 128, cross_files, i)[0]
    again, _ = ds.device_batch(torch.tensor(order, dtype=torch.int64))                    # an int64 tensor instead of a list
    assert torch.equal(again, batch) and again.data_ptr() != batch.data_ptr()
    clip, file_index = ds[5]                                                              # no host copy: read from the device store
    assert clip.device.type == "cpu" and torch.equal(clip, twin[5][0]) and int(file_index) == int(twin[5][1])
    for wrong in ([0, n], [-1], []):
        with pytest.raises((IndexError, ValueError)):
            ds.device_batch(wrong)
    ds.unique_length = 64                                                                 # the setters rebuild the device tables too
    twin.unique_length = 64
    assert len(ds) == len(twin) > n
    batch, labels = ds.device_batch(range(len(ds)))
    for i in range(len(ds)):
        assert torch.equal(batch[i].cpu(), twin[i][0]) and int(labels[i]) == int(twin[i][1])


# ---------------------------------------------------------------------------------------------------------------- the trainer
C_, H_, V_, K_, B_ = 64, 64, 12, 4, 8
FILES = [9000, 8500, 12001]
UNIQUE = 1000


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


def _model():
    torch.manual_seed(11)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=C_, hidden_size=H_), enc_size=C_, ar_size=H_, visible_steps=V_,
                                       prediction_steps=K_, compute_dtype="fp32")
    return model.to(DEV)


_DATA = {}


def _datasets():
    """(item_length, the int16 files, the device dataset's windows materialised on the host with its counts), made once."""
    if not _DATA:
        item = int(_model().item_length)
        ints, _ = R.make_files(FILES, seed=6)
        ints = [(a // 8).astype(np.int16) for a in ints]          # |x| <= 1/8: a calmer input for the model
        twin = DeviceAudioDataset(arrays=ints, item_length=item, unique_length=UNIQUE)
        assert UNIQUE < item and len(twin) >= 3 * B_ and min(twin.get_example_count_per_file()) >= 8
        windows = torch.stack([twin[i] for i in range(len(twin))])
        _DATA.update(item=item, ints=ints, windows=windows, counts=twin.get_example_count_per_file())
    return _DATA


def _device_dataset(**kw):
    d = _datasets()
    return DeviceAudioDataset(arrays=d["ints"], item_length=d["item"], unique_length=UNIQUE, device=DEV, **kw)


def _tensor_dataset():
    d = _datasets()
    return TensorAudioDataset(d["windows"], counts=d["counts"], device=DEV)


def _train(dataset, steps=3, groups=None, augmentation=None):
    """train(max_steps=steps) in fp32 from the same seeds: (losses, the parameters, the entry points called, the trainer)."""
    model, logger = _model(), _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=dataset, logger=logger, device=DEV, regularization=0.5,
                                      score_function=softplus_score_function, prediction_steps=K_, ar_size=H_,
                                      file_batch_size=2 if groups else 1)
    tr.verbose = False
    tr.negative_groups = groups
    tr.augmentation = augmentation
    random.seed(5)
    torch.manual_seed(7)
    with _Spy() as spy:
        tr.train(batch_size=B_, epochs=2, lr=1e-3, num_workers=0, max_steps=steps)
    torch.cuda.synchronize()
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return logger.loss_meter.values, params, spy.names, tr


@pytest.mark.parametrize("variant", ["plain", "same_file", "augmented"])
def test_training_is_bit_identical_to_materialised_windows(variant):
    """Three fp32 steps fed by the device dataset (3 files, unique_length < item_length) and by a TensorAudioDataset(device=...) that
    holds the same windows with the same counts: the logged losses and every parameter are the same bits; also with grouped negatives
    on same-file candidates (the indices and file counts travel the same way) and with a waveform augmentation.  The device dataset's
    run cuts one batch per step with cpc_window_gather, the tensor dataset's never calls it."""
    kw = {"plain": {}, "same_file": dict(groups="same_file"),
          "augmented": dict(augmentation=WaveAugmentation(speed=0.1, time_drop=(2, 300), noise_snr_db=(10.0, 20.0), gain_db=(-3.0, 3.0),
                                                          polarity=0.5, seed=21))}[variant]
    steps = 3
    loss_a, params_a, names_a, _ = _train(_device_dataset(), steps, **kw)
    loss_b, params_b, names_b, _ = _train(_tensor_dataset(), steps, **kw)
    assert len(loss_a) == steps and all(np.isfinite(loss_a)) and loss_a == loss_b, (loss_a, loss_b)
    assert params_a.keys() == params_b.keys()
    for k in params_a:
        assert torch.equal(params_a[k], params_b[k]), k
    assert names_a.count("cpc_window_gather") == steps and "cpc_window_gather" not in names_b
    assert [n for n in names_a if n != "cpc_window_gather"] == names_b          # launch for launch otherwise
    if variant == "same_file":
        assert "cpc_nce_loss_grouped" in names_a
    if variant == "augmented":
        assert names_a.count("cpc_wave_augment") == steps


def test_validation_and_test_task_data():
    """validate(batch_size=8) is the same for the two datasets, and calc_test_task_data on a labels=True device dataset returns what
    its host twin returns through the DataLoader, the labels being the file indices."""
    d = _datasets()
    results = []
    for val in (_device_dataset(), _tensor_dataset()):
        tr = ContrastiveEstimationTrainer(model=_model(), dataset=val, validation_set=val, logger=_Logger(), device=DEV,
                                          regularization=0.5, score_function=softplus_score_function, prediction_steps=K_, ar_size=H_)
        tr.verbose = False
        with _Spy() as spy:
            results.append(tr.validate(batch_size=8, num_workers=0))
        assert ("cpc_window_gather" in spy.names) == isinstance(val, DeviceAudioDataset)
    (la, aa, sa, ma), (lb, ab, sb, mb) = results
    assert torch.equal(la, lb) and torch.equal(aa, ab) and sa == sb and torch.equal(ma, mb) and bool(torch.isfinite(la).all())

    kw = dict(arrays=d["ints"], item_length=d["item"], unique_length=UNIQUE, cross_files=False, labels=True)
    out = []
    for test_set in (DeviceAudioDataset(device=DEV, **kw), DeviceAudioDataset(**kw)):
        tr = ContrastiveEstimationTrainer(model=_model(), dataset=test_set, test_task_set=test_set, logger=_Logger(), device=DEV,
                                          prediction_steps=K_, ar_size=H_)
        tr.verbose = False
        with _Spy() as spy:
            out.append(tr.calc_test_task_data(batch_size=8, num_workers=0))
        n = len(test_set)
        assert spy.names.count("cpc_window_gather") == (-(-n // 8) if test_set.device is not None else 0)
    (data_a, labels_a), (data_b, labels_b) = out
    assert data_a.shape == (n, H_) and np.array_equal(data_a, data_b) and np.array_equal(labels_a, labels_b)
    assert labels_a.tolist() == [R.position(FILES, d["item"], UNIQUE, False, i)[0] for i in range(n)]
    assert len(set(labels_a.tolist())) == 3 and np.isfinite(data_a).all() and np.abs(data_a).max() > 0
