"""Batch composition for the trainer: FileBatchSampler (index semantics of the reference's audio_dataset.py:202-263)
and a synthetic stand-in for AudioDataset that implements the protocol the trainer uses
(``dataset[i] -> (item_length,) float tensor``, ``get_example_count_per_file()``; reference :155-168).

File I/O (torchaudio / mutagen decoding, reference :16-153) is outside the hot path and not rebuilt.
The sampler draws from Python's ``random`` in the same call order as the reference, so a given seed (or a given
global RNG state when seed is None) yields bit-identical index lists.

DeviceAudioDataset is the route for recordings: the 16-bit PCM of every file is read once (the standard library's ``wave``; any other
decoder hands in arrays) and kept concatenated in HBM, and a batch of overlapping windows is cut out of it by one launch of
cpc_window_gather.  Its index semantics are the reference's AudioDataset / AudioTestingDataset (:77-127, :155-165, :191-199).
With convert=True it takes PCM files of any rate, width and channel count and converts them on the device at load (resampling.py).
"""
from __future__ import annotations

import math
import random
import wave
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.utils.data


def _split(seq, n, drop_last):
    out = []
    for start in range(0, len(seq), n):
        if drop_last and start + n > len(seq):
            break
        out.append(seq[start:start + n])
    return out


class FileBatchSampler(torch.utils.data.Sampler):
    """Batches of example indices; with file_batch_size > 1 every batch is made of runs of that many examples taken
    from one file each (examples are numbered file after file)."""

    def __init__(self, index_count_per_file, batch_size, file_batch_size=1, drop_last=True, seed=None, verbose=True):
        self.index_count_per_file = list(index_count_per_file)
        self.indices_in_file: List[List[int]] = []
        first = 0
        for count in self.index_count_per_file:
            self.indices_in_file.append(list(range(first, first + count)))
            first += count
        self.batch_size = batch_size
        self.file_batch_size = file_batch_size
        self.drop_last = drop_last
        self.seed = seed
        rounding = math.floor if drop_last else math.ceil
        self.batches_per_file = [rounding(n / file_batch_size) for n in self.index_count_per_file]
        if verbose:
            print("minimum batches per file:", min(self.batches_per_file),
                  "maximum batches per file:", max(self.batches_per_file))

    def __len__(self):
        # As in the reference: the number of FILE batches (also the index range shuffled when file_batch_size == 1).
        return int(sum(self.batches_per_file))

    def __iter__(self):
        if self.file_batch_size == 1:
            order = list(range(len(self)))
            if self.seed is not None:
                random.seed(self.seed)
            random.shuffle(order)
            return iter(_split(order, self.batch_size, self.drop_last))
        # NB: like the reference, the per-file lists are shuffled in place and keep their order between passes
        for i, indices in enumerate(self.indices_in_file):
            if self.seed is not None:
                random.seed(self.seed + i)
            random.shuffle(indices)
        runs = []
        for indices in self.indices_in_file:
            runs.extend(_split(indices, self.file_batch_size, self.drop_last))
        if self.seed is not None:
            random.seed(self.seed)
        random.shuffle(runs)
        runs_per_batch = self.batch_size // self.file_batch_size
        if runs_per_batch > 1:
            merged = []
            for start in range(0, len(runs), runs_per_batch):
                if self.drop_last and start + runs_per_batch > len(runs):
                    break
                merged.append([i for run in runs[start:start + runs_per_batch] for i in run])
            return iter(merged)
        return iter(runs)


class SyntheticAudioDataset(torch.utils.data.Dataset):
    """``n_items`` clips of ``item_length`` samples of seeded white noise.

    ``device`` != None keeps the whole set resident in HBM (``device_data``) so that the trainer indexes it on the
    device instead of going through a DataLoader (the benchmark contract: inputs already in HBM)."""

    def __init__(self, n_items: int, item_length: int, seed: int = 0, scale: float = 1.0,
                 counts: Optional[Sequence[int]] = None, device=None):
        g = torch.Generator().manual_seed(seed)
        self.data = torch.randn(n_items, item_length, generator=g) * scale
        self.counts = list(counts) if counts is not None else [n_items]
        assert sum(self.counts) == n_items
        self._item_length = item_length
        self.device_data = self.data.to(device) if device is not None else None

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, idx):
        return self.data[idx]

    def get_example_count_per_file(self):
        return list(self.counts)


class TensorAudioDataset(SyntheticAudioDataset):
    """Wraps an existing (n_items, item_length) tensor (e.g. golden fixture data) in the same protocol."""

    def __init__(self, data: torch.Tensor, counts: Optional[Sequence[int]] = None, device=None):
        self.data = data
        self.counts = list(counts) if counts is not None else [data.shape[0]]
        self._item_length = data.shape[1]
        self.device_data = data.to(device) if device is not None else None


def _read_wav(path, sampling_rate):
    """Channel 0 of a 16-bit PCM file as int16 (the reference takes ``data[0, :]`` of what torchaudio decodes)."""
    try:
        with wave.open(str(path), "rb") as f:
            width, rate, channels = f.getsampwidth(), f.getframerate(), f.getnchannels()
            raw = f.readframes(f.getnframes()) if width == 2 and rate == sampling_rate else b""
    except (wave.Error, EOFError) as err:
        raise ValueError(f"{path}: not a PCM WAV file ({err})") from err
    if width != 2:
        raise ValueError(f"{path}: {8 * width}-bit samples; only 16-bit PCM is read (decode other formats yourself and pass arrays=)")
    if rate != sampling_rate:
        raise ValueError(f"{path}: sampling rate {rate}, the dataset's is {sampling_rate}; there is no resampling")
    frames = np.frombuffer(raw, dtype="<i2")
    frames = frames[:len(frames) - len(frames) % channels].reshape(-1, channels)
    return np.ascontiguousarray(frames[:, 0]).astype(np.int16, copy=False)


def _read_wav_frames(path):
    """(frames [n, channels], rate) of a PCM WAV file of any rate, 8, 16, 24 or 32 bits and up to 8 channels, for convert=True: 16-bit
    samples as int16, the other widths as float32 in [-1, 1) (8-bit WAV is unsigned, the wider ones are signed little-endian)."""
    try:
        with wave.open(str(path), "rb") as f:
            width, rate, channels = f.getsampwidth(), f.getframerate(), f.getnchannels()
            raw = f.readframes(f.getnframes()) if width in (1, 2, 3, 4) and 1 <= channels <= 8 else b""
    except (wave.Error, EOFError) as err:
        raise ValueError(f"{path}: not a PCM WAV file ({err})") from err
    if width not in (1, 2, 3, 4):
        raise ValueError(f"{path}: {8 * width}-bit samples; 8-, 16-, 24- and 32-bit PCM are read")
    if not 1 <= channels <= 8:
        raise ValueError(f"{path}: {channels} channels; up to 8 are read")
    count = len(raw) // (width * channels) * channels
    raw = raw[:count * width]
    if width == 2:
        samples = np.frombuffer(raw, dtype="<i2").astype(np.int16, copy=False)
    elif width == 1:
        samples = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        value = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        value -= (value & 0x800000) << 1
        samples = value.astype(np.float32) * np.float32(1.0 / 8388608.0)          # 24 bits are exact in float32
    else:
        samples = (np.frombuffer(raw, dtype="<i4").astype(np.float64) * (1.0 / 2147483648.0)).astype(np.float32)
        samples = np.minimum(samples, np.float32(1.0 - 2.0 ** -24))                # the rounding of 2^31 - 1 must not reach 1.0
    return np.ascontiguousarray(samples.reshape(-1, channels)), int(rate)


class DeviceAudioDataset(torch.utils.data.Dataset):
    """Overlapping windows of ``item_length`` samples, ``unique_length`` apart, over the samples of all files, which are held once:
    concatenated, as int16 or float32, in HBM (``device``) and / or on the host (``keep_host``, the default without a device).

    Sources: ``location``, a directory searched recursively for ``.wav`` files (sorted; 16-bit PCM at ``sampling_rate``, channel 0;
    anything else is a ValueError that names the file), or ``arrays``, one 1-D int16 or float32 numpy array or tensor per file.
    ``storage="int16"`` needs int16 sources and converts in the gather (sample / 32768, exact in float32, what the reference's loader
    returns); ``storage="float32"`` scales int16 sources once at load.

    Indices as in the reference: example i lies at sample i * unique_length of the files laid end to end (``cross_files=False``: of
    the files each shortened by item_length, so that the window stays in its file), its file is bisect_left(start_samples, sample) - 1,
    at least 0: a sample that falls exactly on a later file's start belongs to the file in front of it.  One deviation:
    with cross_files=False the window is always the item_length samples of that file from the position in it; the reference's
    load_sample takes the file's length from the shortened start_samples there and can run on into the next file.

    ``convert=True`` (opt-in; every default above stays) takes files as they come: WAV of 8-, 16-, 24- or 32-bit PCM, up to 8 channels,
    any sampling rate; arrays ``(frames,)`` or ``(frames, channels)`` at ``array_rates`` (one number or one per array).  16-bit sources
    are uploaded as they are, interleaved, the other widths as float32 in [-1, 1); the files of one (rate, channels, sample type) are
    downmixed (``channels="first"`` or ``"mean"``), resampled to ``sampling_rate`` and stored as ``storage`` by cpc_resample
    (resampling.py) in chunks of at most ``convert_chunk_bytes`` of source, so that peak HBM is the store plus one chunk.
    ``file_lengths`` are then the converted lengths, ceil(frames new / orig), and everything behind the store is as without it; a host
    copy is read back from the store.  Without a device only width and channel conversion run (numpy); a file at another rate is a
    ValueError, because resampling runs on the device.  IEEE-float WAV and other containers: a ValueError that names the file.

    ``dataset[i]`` is the (item_length,) float32 clip, with ``labels=True`` the pair (clip, file index as a 0-d long tensor).
    ``device_batch(indices)`` is the (B, item_length) float32 batch in HBM, cut by one cpc_window_gather launch; the trainer takes its
    batches there, with no DataLoader.  A dataset without a device goes through the trainer's DataLoader route."""

    def __init__(self, location=None, item_length=None, unique_length=None, sampling_rate=16000, max_file_count=None,
                 cross_files=True, device=None, storage="int16", arrays=None, labels=False, keep_host=None, convert=False,
                 channels="first", array_rates=None, convert_chunk_bytes=256 << 20):
        super().__init__()
        if (location is None) == (arrays is None):
            raise ValueError("exactly one of location and arrays must be given")
        if item_length is None or int(item_length) < 1:
            raise ValueError("item_length must be a positive number of samples")
        if storage not in ("int16", "float32"):
            raise ValueError(f"storage must be 'int16' or 'float32', not {storage!r}")
        if channels not in ("first", "mean"):
            raise ValueError(f"channels must be 'first' or 'mean', not {channels!r}")
        if not convert and (channels != "first" or array_rates is not None):
            raise ValueError("channels='mean' and array_rates need convert=True")
        if int(convert_chunk_bytes) < 1:
            raise ValueError("convert_chunk_bytes must be positive")
        self.convert = bool(convert)
        self.channels = channels
        self.sampling_rate = sampling_rate
        self.cross_files = bool(cross_files)
        self.labels = bool(labels)
        self.storage = storage
        self.device = torch.device(device) if device is not None else None
        keep_host = self.device is None if keep_host is None else bool(keep_host)
        if self.device is None and not keep_host:
            raise ValueError("a dataset without a device needs its host copy (keep_host)")
        if location is not None:
            self.location = Path(location)
            files = sorted(self.location.glob("**/*.wav"))
            if max_file_count is not None:
                files = files[:max_file_count]
            self.files = [str(f) for f in files]
            if convert:
                read = [_read_wav_frames(f) for f in self.files]
                sources, rates = [a for a, _ in read], [r for _, r in read]
            else:
                sources = [_read_wav(f, sampling_rate) for f in self.files]
        else:
            self.location, self.files = None, None
            arrays = list(arrays)
            if array_rates is None or np.isscalar(array_rates):
                rates = [int(sampling_rate if array_rates is None else array_rates)] * len(arrays)
            else:
                rates = [int(r) for r in array_rates]
                if len(rates) != len(arrays):
                    raise ValueError(f"array_rates has {len(rates)} entries for {len(arrays)} arrays")
            if max_file_count is not None:
                arrays, rates = arrays[:max_file_count], rates[:max_file_count]
            sources = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in arrays]
        if not sources:
            raise ValueError("no audio files" + (f" under {self.location}" if self.location is not None else ""))
        self._item_length = int(item_length)
        self._unique_length = int(item_length if unique_length is None else unique_length)
        self._scale = 1.0 / 32768.0 if storage == "int16" else 1.0
        if convert:
            host = self._load_converted(sources, rates, int(convert_chunk_bytes), keep_host)
            del sources
            self._host = host if keep_host else None
            self.calculate_length()
            return
        for k, a in enumerate(sources):
            name = self.files[k] if self.files is not None else f"arrays[{k}]"
            if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
                raise ValueError(f"{name}: a file is a 1-D int16 or float32 array, not {a.dtype} with {a.ndim} dimensions")
            if storage == "int16" and a.dtype != np.int16:
                raise ValueError(f"{name}: storage='int16' needs int16 samples, not {a.dtype}")
        self.max_file_count = len(sources)
        self.file_lengths = [int(a.shape[0]) for a in sources]
        if storage == "float32":
            sources = [a.astype(np.float32) * np.float32(1.0 / 32768.0) if a.dtype == np.int16 else a for a in sources]
        host = torch.from_numpy(np.concatenate(sources))
        del sources
        self._store = host.to(self.device) if self.device is not None else None
        self._host = host if keep_host else None
        self.calculate_length()

    def _load_converted(self, sources, rates, chunk_bytes, keep_host):
        """convert=True: sets file_lengths and the store from sources of any rate, channel count and sample type, and returns the host
        copy (None where none is asked for).  With a device, the files of one (rate, channels, sample type) go through cpc_resample in
        chunks of at most chunk_bytes of source (a longer file goes alone), each straight into its place in the store; without one,
        width and channel conversion run in numpy and a file at another rate is refused."""
        from . import resampling
        name = lambda k: self.files[k] if self.files is not None else f"arrays[{k}]"
        for k, a in enumerate(sources):
            if a.ndim == 1:
                sources[k] = a = a.reshape(-1, 1)
            if a.ndim != 2 or not 1 <= a.shape[1] <= 8 or a.dtype not in (np.int16, np.float32):
                raise ValueError(f"{name(k)}: a file is an int16 or float32 array (frames,) or (frames, channels <= 8), not {a.dtype} "
                                 f"with shape {a.shape}")
            if rates[k] < 1:
                raise ValueError(f"{name(k)}: sampling rate {rates[k]}")
        self.max_file_count = len(sources)
        to_int16 = self.storage == "int16"
        mix = resampling.MIX_MEAN if self.channels == "mean" else resampling.MIX_FIRST

        def scales(dtype):          # (in_scale, out_scale): int16 sources count in units of 1 / 32768, float sources in units of 1
            if dtype == np.int16:
                return (1.0, 1.0) if to_int16 else (1.0 / 32768.0, 1.0)
            return (1.0, 32768.0) if to_int16 else (1.0, 1.0)

        self.convert_launches = 0          # cpc_resample launches this load made
        if self.device is None:
            converted = []
            for k, a in enumerate(sources):
                if rates[k] != self.sampling_rate:
                    raise ValueError(f"{name(k)}: sampling rate {rates[k]}, the dataset's is {self.sampling_rate}; resampling runs on "
                                     f"the device (pass device=)")
                x = a[:, 0].astype(np.float32)
                if mix == resampling.MIX_MEAN:
                    for c in range(1, a.shape[1]):
                        x = x + a[:, c].astype(np.float32)
                    x = x / np.float32(a.shape[1])
                in_scale, out_scale = scales(a.dtype)
                x = (x * np.float32(in_scale)) * np.float32(out_scale)
                converted.append(np.rint(np.clip(x, -32768.0, 32767.0)).astype(np.int16) if to_int16 else x)
            self.file_lengths = [int(x.shape[0]) for x in converted]
            self._store = None
            return torch.from_numpy(np.concatenate(converted))

        plans, groups = {}, {}
        self.file_lengths = []
        for k, a in enumerate(sources):
            if rates[k] not in plans:
                try:
                    plans[rates[k]] = resampling.plan_for(rates[k], self.sampling_rate)
                except ValueError as err:
                    raise ValueError(f"{name(k)}: {err}") from err
            self.file_lengths.append(plans[rates[k]].output_length(a.shape[0]))
            groups.setdefault((rates[k], a.shape[1], a.dtype.str), []).append(k)
        first = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(self.file_lengths, dtype=np.int64))])
        store = torch.empty(int(first[-1]), dtype=torch.int16 if to_int16 else torch.float32, device=self.device)

        def flush(members):
            frames = np.asarray([sources[k].shape[0] for k in members], dtype=np.int64)
            begin = np.concatenate([np.zeros(1, np.int64), np.cumsum(frames)[:-1]])
            out = np.asarray([self.file_lengths[k] for k in members], dtype=np.int64)
            keep = out > 0
            if not keep.any():
                return
            a0 = sources[members[0]]
            in_scale, out_scale = scales(a0.dtype)
            chunk = torch.from_numpy(np.concatenate([sources[k] for k in members])).to(self.device)
            segments = np.stack([begin, frames, first[np.asarray(members)], out], axis=1)[keep]
            resampling.convert_segments(chunk, a0.shape[1], mix, plans[rates[members[0]]], segments, store, in_scale, out_scale)
            self.convert_launches += 1

        for members in groups.values():
            chunk, size = [], 0
            for k in members:
                if chunk and size + sources[k].nbytes > chunk_bytes:
                    flush(chunk)
                    chunk, size = [], 0
                chunk.append(k)
                size += sources[k].nbytes
            flush(chunk)
        self._store = store
        return store.cpu() if keep_host else None

    @classmethod
    def from_arrays(cls, arrays, item_length, **kwargs):
        return cls(arrays=arrays, item_length=item_length, **kwargs)

    @property
    def item_length(self):
        return self._item_length

    @item_length.setter
    def item_length(self, value):
        self._item_length = int(value)
        self.calculate_length()

    @property
    def unique_length(self):
        return self._unique_length

    @unique_length.setter
    def unique_length(self, value):
        self._unique_length = int(value)
        self.calculate_length()

    def calculate_length(self):
        """start_samples, the length and the per-example tables (first sample in the store, file), for the current item_length and
        unique_length; the tables are built vectorised, checked once and uploaded once."""
        item, unique = self._item_length, self._unique_length
        if item < 1 or unique < 1:
            raise ValueError("item_length and unique_length must be positive")
        lengths = np.asarray(self.file_lengths, dtype=np.int64)
        store_len = int(lengths.sum())
        if self.cross_files:
            counted = lengths
        else:
            short = [k for k, n in enumerate(self.file_lengths) if n < item]
            if short:
                name = self.files[short[0]] if self.files is not None else f"arrays[{short[0]}]"
                raise ValueError(f"{name}: {self.file_lengths[short[0]]} samples, shorter than item_length = {item} (cross_files=False)")
            counted = lengths - item
        cum = np.concatenate([np.zeros(1, np.int64), np.cumsum(counted)])
        self.start_samples = [int(v) for v in cum]
        self._length = max(0, math.floor((self.start_samples[-1] - (item - unique)) / unique))
        sample_index = np.arange(self._length, dtype=np.int64) * unique
        file_of = np.maximum(np.searchsorted(cum, sample_index, side="left") - 1, 0)
        first = np.concatenate([np.zeros(1, np.int64), np.cumsum(lengths)])          # the files as they lie in the store
        starts = first[file_of] + (sample_index - cum[file_of])
        if self._length and (int(file_of.max()) >= len(self.file_lengths) or int(starts.min()) < 0 or int(starts.max()) + item > store_len):
            raise ValueError("window table out of range: a window would leave the stored samples")
        self._store_len = store_len
        self._starts = torch.from_numpy(starts)
        self._file_of = torch.from_numpy(file_of.astype(np.int64))
        if self.device is not None:
            self._starts_dev = self._starts.to(self.device)
            self._file_dev = self._file_of.to(self.device)

    def __len__(self):
        return self._length

    def get_position(self, idx):
        """(file index, position in the reference's start_samples numbering) of example idx."""
        file_index = int(self._file_of[idx])
        return file_index, idx * self._unique_length - self.start_samples[file_index]

    def get_example_count_per_file(self):
        unique = self._unique_length
        counts = [math.ceil(self.start_samples[i] / unique) - math.ceil(self.start_samples[i - 1] / unique)
                  for i in range(1, len(self.start_samples))]
        total = sum(counts)
        if total > self._length:
            counts[-1] -= total - self._length
        return counts

    def __getitem__(self, idx):
        idx = int(idx)
        if not 0 <= idx < self._length:
            raise IndexError(f"example {idx} of {self._length}")
        if self._host is not None:
            s = int(self._starts[idx])
            clip = self._host[s:s + self._item_length]
            clip = clip.to(torch.float32) * self._scale if clip.dtype == torch.int16 else clip.clone()
        else:
            clip = self._gather(torch.tensor([idx], dtype=torch.int64))[0][0].cpu()
        return (clip, self._file_of[idx].clone()) if self.labels else clip

    def _gather(self, idx):
        """(batch, the indices on the device) for a checked int64 host tensor of example indices."""
        from . import _hip
        B, L = int(idx.numel()), self._item_length
        with torch.cuda.device(self.device):
            idx_dev = idx.to(self.device)
            out = torch.empty((B, L), device=self.device, dtype=torch.float32)
            _hip.call("cpc_window_gather", _hip.ptr(self._store), 1 if self.storage == "int16" else 0, self._store_len,
                      _hip.ptr(self._starts_dev), self._length, _hip.ptr(idx_dev), _hip.ptr(out), B, L, L, self._scale)
        return out, idx_dev

    def device_batch(self, indices):
        """The (B, item_length) float32 batch of the examples ``indices`` (a sequence or an int64 tensor; repeats allowed) in HBM: the
        range check on the host, one small upload of the indices, one launch.  With labels=True: (batch, file indices on the device)."""
        if self.device is None:
            raise RuntimeError("device_batch needs a dataset built with device=")
        idx = indices.detach().cpu() if isinstance(indices, torch.Tensor) else torch.as_tensor(list(indices))
        if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1:
            raise ValueError("indices: a non-empty 1-D sequence of integers (an int64 tensor)")
        if int(idx.min()) < 0 or int(idx.max()) >= self._length:
            raise IndexError(f"example indices outside [0, {self._length})")
        out, idx_dev = self._gather(idx.contiguous())
        return (out, self._file_dev[idx_dev]) if self.labels else out

    def file_ranges(self):
        """[(first sample in the store, length)] of every file, in file order: where each recording lies, whatever item_length,
        unique_length and cross_files are (feature_extraction.FeatureExtractor reads whole files)."""
        first = 0
        out = []
        for n in self.file_lengths:
            out.append((first, int(n)))
            first += int(n)
        return out

    def hbm_bytes(self):
        """Bytes this dataset holds in HBM: the samples and the two per-example tables."""
        if self.device is None:
            return 0
        return sum(t.numel() * t.element_size() for t in (self._store, self._starts_dev, self._file_dev))
