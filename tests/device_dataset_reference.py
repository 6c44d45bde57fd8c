"""A deliberately naive restatement of the window indexing of DeviceAudioDataset, for the tests: scalar bisect per example, Python
slicing per file and recursion across files.  Nothing here is shared with the vectorised tables of the code under test.

``files`` is a list of 1-D float32 numpy arrays (the samples as the dataset hands them out: int16 / 32768)."""
import bisect
import math

import numpy as np


def start_samples(lengths, item_length, cross_files):
    starts = [0]
    for n in lengths:
        nxt = starts[-1] + n
        if not cross_files:
            nxt -= item_length
        starts.append(nxt)
    return starts


def length(lengths, item_length, unique_length, cross_files):
    starts = start_samples(lengths, item_length, cross_files)
    return math.floor((starts[-1] - (item_length - unique_length)) / unique_length)


def position(lengths, item_length, unique_length, cross_files, i):
    """(file, position in that file's counted samples) of example i."""
    starts = start_samples(lengths, item_length, cross_files)
    sample = i * unique_length
    f = bisect.bisect_left(starts, sample) - 1
    if f < 0:
        f = 0
    assert f + 1 < len(starts)
    return f, sample - starts[f]


def _take(files, f, pos, n):
    """n samples from position pos of file f, running on into the files behind it."""
    here = files[f][pos:pos + n]
    if len(here) == n:
        return here
    return np.concatenate([here, _take(files, f + 1, 0, n - len(here))])


def window(files, item_length, unique_length, cross_files, i):
    lengths = [len(a) for a in files]
    f, pos = position(lengths, item_length, unique_length, cross_files, i)
    if cross_files:
        return _take(files, f, pos, item_length)
    assert 0 <= pos and pos + item_length <= lengths[f], (i, f, pos)
    return files[f][pos:pos + item_length]


def example_count_per_file(lengths, item_length, unique_length, cross_files):
    starts = start_samples(lengths, item_length, cross_files)
    n = length(lengths, item_length, unique_length, cross_files)
    counts = [math.ceil(starts[k] / unique_length) - math.ceil(starts[k - 1] / unique_length) for k in range(1, len(starts))]
    if sum(counts) > n:
        counts[-1] -= sum(counts) - n
    return counts


def make_files(lengths, seed=0):
    """int16 files with every value possible, the extremes included."""
    rng = np.random.default_rng(seed)
    files = [rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16) for n in lengths]
    return files, [a.astype(np.float32) / np.float32(32768.0) for a in files]
