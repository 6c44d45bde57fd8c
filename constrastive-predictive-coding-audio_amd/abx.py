"""ABX phone discriminability over extracted features on the HIP path ("ABX discriminability").

For triples (A, B, X) with A and X tokens of one phone and B a token of another, all in one context and from one speaker, the ABX error
is the share of triples in which X lies closer to B than to A; "closer" is the dynamic-time-warping distance between two segments of
frames, the accumulated frame distance along the best path divided by the path's length (ZeroSpeech / Libri-light).  It needs no
training.  ``abx_error`` plans every segment pair and every (cell, phone, phone) task on the host, uploads the two tables once, runs
cpc_dtw (frame distances by MFMA fused with the recurrence: the P x La x Lb distances never reach HBM) and cpc_abx_count, and reads the
T counts back once; between the first and the last launch there is no synchronisation, no host <-> device copy and no allocation.
Forward only: engines, the random state of torch and ``model.training`` are not touched.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _hip
from .clustering import _rows_of

METRICS = {"angular": 0, "cosine": 1, "sqeuclidean": 2}          # include/cpc_hip.h, the frame distance
MAX_LEN = 128                                                    # frames of a segment (the kernel's limit)
# pairs of a cpc_dtw call, tasks of a cpc_abx_count call: the ABI's limit on P and T (an int32's range).  The library itself cuts a call
# into grids the runtime accepts (below 2^32 threads: 2^25 pairs, 2^23 tasks per launch, csrc/dtw.hip), so nothing smaller is needed here.
MAX_PAIRS = 2 ** 31 - 1
MIN_GROUP, MAX_GROUP = 2, 1024                                   # items of a group a task may hold (n_p from 2, n_q from 1)
COLUMNS = ("file", "first", "last", "phone", "context", "speaker")
LL = C.c_longlong

ABXResult = namedtuple("ABXResult", "error pair_scores phones n_pairs n_tasks n_triples n_invalid")


def _metric_code(metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    return METRICS[metric]


def _ldx(x):
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


# ======================================================================================================================== items
class Items:
    """Segments to compare: host int64 arrays of one length.  ``file`` is the index of the recording within the ``Features`` result,
    [``first``, ``last``) the frame range within that recording, ``phone``, ``context`` and ``speaker`` integer codes."""

    def __init__(self, file, first, last, phone, context, speaker):
        cols = [np.ascontiguousarray(np.asarray(v, dtype=np.int64)) for v in (file, first, last, phone, context, speaker)]
        n = cols[0].shape
        if any(c.ndim != 1 or c.shape != n for c in cols):
            raise ValueError("the columns of Items must be one-dimensional and of one length")
        self.file, self.first, self.last, self.phone, self.context, self.speaker = cols

    def __len__(self):
        return int(self.file.shape[0])


def frames_of(onset_s, offset_s, frame_rate):
    """[first, last) of the frames t with (t + 0.5) / frame_rate in [onset, offset), in float64."""
    rate = float(frame_rate)

    def first_at_or_after(t_s):
        """The smallest t >= 0 with (t + 0.5) / rate >= t_s, the comparison made exactly as the rule states it."""
        t_s = np.asarray(t_s, np.float64)
        t = np.maximum(np.ceil(t_s * rate - 0.5), 0.0)
        t = np.where((t > 0) & ((t - 0.5) / rate >= t_s), t - 1, t)          # (the estimate is off by one at most)
        return np.where((t + 0.5) / rate < t_s, t + 1, t).astype(np.int64)

    lo, hi = first_at_or_after(onset_s), first_at_or_after(offset_s)
    return lo, np.maximum(hi, lo)


def items_from_times(onset_s, offset_s, frame_rate, file=None, phone=None, context=None, speaker=None):
    """Items from onsets and offsets in seconds (columns left out are zeros).  An item that comes out empty or longer than 128 frames
    is dropped, which is no error; returns (items, report) with report = {"kept": indices, "empty": indices, "too_long": indices,
    "dropped": count} over the input order."""
    first, last = frames_of(onset_s, offset_s, frame_rate)
    n = first.shape[0]
    length = last - first
    empty, too_long = np.flatnonzero(length < 1), np.flatnonzero(length > MAX_LEN)
    kept = np.flatnonzero((length >= 1) & (length <= MAX_LEN))
    cols = [np.zeros(n, np.int64) if v is None else np.asarray(v, np.int64) for v in (file, phone, context, speaker)]
    items = Items(cols[0][kept], first[kept], last[kept], cols[1][kept], cols[2][kept], cols[3][kept])
    return items, {"kept": kept, "empty": empty, "too_long": too_long, "dropped": int(empty.size + too_long.size)}


def read_item_file(path, frame_rate=100.0, files=None):
    """A ZeroSpeech .item file: a header line starting with '#', then ``file onset offset phone prev-phone next-phone speaker``, times
    in seconds (``frame_rate``: frames per second of the features; 100 for the encoder's 160 samples per frame at 16 kHz).  The
    context is the pair (prev, next).  Names become integers in sorted order (files: in the order of ``files`` when that list is given,
    the order of the recordings in the Features result); returns (items, names, report), names = {"files", "phones", "contexts",
    "speakers"} and report as items_from_times gives it."""
    rows = []
    with open(path) as f:
        header = f.readline()
        if not header.startswith("#"):
            raise ValueError(f"{path}: the first line must be a header starting with '#'")
        for no, line in enumerate(f, 2):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 7:
                raise ValueError(f"{path}:{no}: expected 7 columns, got {len(parts)}")
            rows.append(parts)
    names = {"files": sorted({r[0] for r in rows}) if files is None else list(files), "phones": sorted({r[3] for r in rows}),
             "contexts": sorted({(r[4], r[5]) for r in rows}), "speakers": sorted({r[6] for r in rows})}
    index = {k: {name: i for i, name in enumerate(v)} for k, v in names.items()}
    missing = sorted({r[0] for r in rows} - set(index["files"]))
    if missing:
        raise ValueError(f"{path}: files not in the given list: {missing[:5]}")
    items, report = items_from_times(
        [float(r[1]) for r in rows], [float(r[2]) for r in rows], frame_rate, file=[index["files"][r[0]] for r in rows],
        phone=[index["phones"][r[3]] for r in rows], context=[index["contexts"][(r[4], r[5])] for r in rows],
        speaker=[index["speakers"][r[6]] for r in rows])
    return items, names, report


# ===================================================================================================================== planning
def plan_abx(items, row_offsets, max_group=10, seed=0, by=("context", "speaker")):
    """The pair and task tables of ``abx_error``, on the host in int64.  Cells are the distinct values of the ``by`` columns, the groups
    of a cell its phones; groups are visited in lexicographic order of (cell key, phone) and one numpy.random.default_rng(seed) is
    consumed in that order: a group above ``max_group`` items keeps numpy.sort(rng.choice(n, max_group, replace=False)).  A cell's items
    lie group after group; pairs [P, 4] holds every (row item, column item) of every cell as (a_first, La, b_first, Lb) in rows of the
    store, tasks [T, 6] every ordered (p, q), p != q, with n_p >= 2 as cpc_abx_count reads it, keys [T, len(by) + 2] the cell key and
    the two phones of each task, picked the indices of the items kept, in table order."""
    by = tuple(by)
    if not by or any(b not in ("context", "speaker") for b in by) or len(set(by)) != len(by):
        raise ValueError(f"by must name 'context' and / or 'speaker', got {by!r}")
    if not (MIN_GROUP <= int(max_group) <= MAX_GROUP):
        raise ValueError(f"max_group = {max_group} is outside [{MIN_GROUP}, {MAX_GROUP}]")
    n = len(items)
    if n == 0:
        raise ValueError("no items")
    row_offsets = np.asarray(row_offsets, np.int64)
    length = items.last - items.first
    if (items.file < 0).any() or (items.file >= row_offsets.shape[0] - 1).any():
        raise ValueError(f"an item names a recording outside [0, {row_offsets.shape[0] - 1})")
    if (length < 1).any() or (length > MAX_LEN).any():
        raise ValueError(f"an item has a length outside [1, {MAX_LEN}] frames")
    if (items.first < 0).any() or (items.last > row_offsets[items.file + 1] - row_offsets[items.file]).any():
        raise ValueError("an item reaches beyond the frames of its recording")
    row_first = row_offsets[items.file] + items.first
    cols = [getattr(items, b) for b in by] + [items.phone]
    order = np.lexsort(tuple(cols[::-1]))                        # stable: the items of a group keep their order
    key = np.stack([c[order] for c in cols], 1)
    new_group = np.ones(n, bool)
    new_group[1:] = (key[1:] != key[:-1]).any(1)
    new_cell = np.ones(n, bool)
    new_cell[1:] = (key[1:, :-1] != key[:-1, :-1]).any(1)
    starts = np.flatnonzero(new_group)
    ends = np.append(starts[1:], n)
    rng = np.random.default_rng(seed)
    cells, cur = [], None
    for s, e in zip(starts, ends):
        idx = order[s:e]
        if e - s > max_group:
            idx = idx[np.sort(rng.choice(e - s, max_group, replace=False))]
        if new_cell[s]:
            cur = SimpleNamespace(key=key[s, :-1], phones=[], groups=[])
            cells.append(cur)
        cur.phones.append(int(key[s, -1]))
        cur.groups.append(idx)
    pairs, tasks, keys, picked, off = [], [], [], [], 0
    for cell in cells:
        idx = np.concatenate(cell.groups)
        nc = idx.shape[0]
        seg = np.stack([row_first[idx], length[idx]], 1)
        pairs.append(np.concatenate([np.repeat(seg, nc, 0), np.tile(seg, (nc, 1))], 1))
        picked.append(idx)
        sizes = np.array([g.shape[0] for g in cell.groups], np.int64)
        first = np.cumsum(sizes) - sizes
        for p in range(len(sizes)):
            if sizes[p] < 2:
                continue
            for q in range(len(sizes)):
                if q != p:
                    tasks.append((off, nc, first[p], sizes[p], first[q], sizes[q]))
                    keys.append(tuple(cell.key) + (cell.phones[p], cell.phones[q]))
        off += nc * nc
    return SimpleNamespace(pairs=np.concatenate(pairs).astype(np.int64), tasks=np.array(tasks, np.int64).reshape(-1, 6),
                           keys=np.array(keys, np.int64).reshape(-1, len(by) + 2), picked=np.concatenate(picked), by=by)


def average_scores(keys, scores):
    """The Libri-light "within" order in float64: the scores of the tasks (keys [T, levels + 2] = the ``by`` values, then p, q) are
    averaged over the last ``by`` column within what remains, then over the one before, and last over the ordered pairs (p, q).
    Returns (mean score, {(p, q): score})."""
    keys, scores = np.asarray(keys, np.int64), np.asarray(scores, np.float64)
    table = {tuple(int(v) for v in k): float(s) for k, s in zip(keys, scores)}
    if len(table) != len(scores):
        raise ValueError("two tasks share a key")
    for level in range(keys.shape[1] - 3, -1, -1):                # drop column ``level``: the mean over it within the rest
        groups = {}
        for k, s in table.items():
            groups.setdefault(k[:level] + k[level + 1:], []).append(s)
        table = {k: float(np.mean(np.array(v, np.float64))) for k, v in groups.items()}
    if not table:
        return float("nan"), {}
    pair_scores = {k: table[k] for k in sorted(table)}
    return float(np.mean(np.array(list(pair_scores.values()), np.float64))), pair_scores


# ================================================================================================================= device calls
def _device_pairs(pairs, n_rows, device):
    """pairs as an int64 (P, 4) device tensor.  Host arrays are validated here; a device tensor is trusted (the kernel gives a pair
    whose table row is out of range the NaN result)."""
    if isinstance(pairs, torch.Tensor) and pairs.is_cuda:
        if pairs.dtype != torch.int64 or pairs.dim() != 2 or pairs.shape[1] != 4 or pairs.shape[0] < 1 or not pairs.is_contiguous():
            raise ValueError(f"pairs must be a contiguous int64 (P, 4) tensor with P >= 1, got {pairs.dtype} {tuple(pairs.shape)}")
        if pairs.device != device:
            raise ValueError(f"pairs is on {pairs.device}, x is on {device}")
        return pairs
    host = pairs.numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if host.dtype.kind not in "iu":
        raise TypeError(f"pairs must hold integers, got {host.dtype}")
    if host.ndim != 2 or host.shape[1] != 4 or host.shape[0] < 1:
        raise ValueError(f"pairs must be (P, 4) with P >= 1, got {host.shape}")
    host = np.ascontiguousarray(host.astype(np.int64))
    for first, length in ((host[:, 0], host[:, 1]), (host[:, 2], host[:, 3])):
        if (length < 1).any() or (length > MAX_LEN).any():
            raise ValueError(f"a segment has a length outside [1, {MAX_LEN}]")
        if (first < 0).any() or (first > n_rows - length).any():
            raise ValueError(f"a segment lies outside the rows [0, {n_rows})")
    return torch.from_numpy(host).to(device)


def _launch_dtw(x, code, pairs, metric, dist, cost, path_len):
    """cpc_dtw over the pair table, in as many launches as the limit on P needs: launches only."""
    N, D = x.shape
    P = pairs.shape[0]
    for p0 in range(0, P, MAX_PAIRS):
        n = min(MAX_PAIRS, P - p0)
        _hip.call("cpc_dtw", _hip.ptr(x), code, LL(N), D, LL(_ldx(x)), _hip.ptr(pairs, 4 * p0), LL(n), metric, _hip.ptr(dist, p0),
                  _hip.ptr(cost, p0), _hip.ptr(path_len, p0))


def dtw_distance(x, pairs, metric="angular", kind="c", return_path=False):
    """The DTW distance of every segment pair: ``x`` an (N, D) f32 or bf16 device tensor with contiguous rows or a ``Features`` object
    (``kind`` picks z or c), ``pairs`` int64 (P, 4) = (a_first, La, b_first, Lb) in rows of x, a host array or a device tensor.
    Returns f32 (P,) on the device: the accumulated frame distance along the best path over the path's length; with ``return_path``
    also the accumulated distance f32 (P,) and the path length int32 (P,).  A pair with a NaN, an infinity or (angular, cosine) a
    zero row gives (NaN, NaN, -1)."""
    x, _ = _rows_of(x, kind)
    code = _metric_code(metric)
    pairs = _device_pairs(pairs, x.shape[0], x.device)
    P = pairs.shape[0]
    with torch.cuda.device(x.device):
        dist = torch.empty(P, device=x.device, dtype=torch.float32)
        cost = torch.empty(P, device=x.device, dtype=torch.float32) if return_path else None
        path_len = torch.empty(P, device=x.device, dtype=torch.int32) if return_path else None
        _launch_dtw(x, _hip.dtype_code(x.dtype), pairs, code, dist, cost, path_len)
    return (dist, cost, path_len) if return_path else dist


def frame_distance(x, a, b, metric="angular", kind="c"):
    """The (La, Lb) f32 matrix of frame distances of the segments a = (first, length) and b = (first, length) of x, bit for bit what
    ``dtw_distance`` accumulates for this pair."""
    x, _ = _rows_of(x, kind)
    code = _metric_code(metric)
    (a_first, La), (b_first, Lb) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    N, D = x.shape
    for first, length in ((a_first, La), (b_first, Lb)):
        if not (1 <= length <= MAX_LEN):
            raise ValueError(f"a segment length of {length} is outside [1, {MAX_LEN}]")
        if first < 0 or first + length > N:
            raise ValueError(f"the segment [{first}, {first + length}) lies outside the rows [0, {N})")
    with torch.cuda.device(x.device):
        out = torch.empty((La, Lb), device=x.device, dtype=torch.float32)
        _hip.call("cpc_frame_distance", _hip.ptr(x), _hip.dtype_code(x.dtype), LL(N), D, LL(_ldx(x)), LL(a_first), La, LL(b_first), Lb,
                  code, _hip.ptr(out), LL(Lb))
    return out


# ==================================================================================================================== abx_error
def _launch_abx(run):
    """Everything between the upload of the tables and the read-back of the counts: launches only."""
    _launch_dtw(run.x, run.code, run.pairs, run.metric, run.dist, None, None)
    T = run.tasks.shape[0]
    for t0 in range(0, T, MAX_PAIRS):
        n = min(MAX_PAIRS, T - t0)
        _hip.call("cpc_abx_count", _hip.ptr(run.dist), LL(run.dist.shape[0]), _hip.ptr(run.tasks, 6 * t0), LL(n), _hip.ptr(run.out, t0))


def abx_error(features, items, metric="angular", kind="c", max_group=10, seed=0, by=("context", "speaker")):
    """The within-speaker ABX error of ``features`` (a ``Features`` object, or an (N, D) device tensor holding one recording) on
    ``items``.  Tasks are scored as out / (2 n_p (n_p - 1) n_q) (a tie counts half), averaged over speakers within (context, p, q), over
    contexts within (p, q) and over the ordered phone pairs; ``by=("context",)`` pools the speakers.  A task one of whose distances is
    NaN is left out and counted in ``n_invalid``.  Returns ABXResult(error = 1 - mean score, pair_scores {(p, q): score}, phones,
    n_pairs, n_tasks, n_triples, n_invalid)."""
    x, offsets = _rows_of(features, kind)
    code = _metric_code(metric)
    if not isinstance(items, Items):
        raise TypeError(f"items must be an Items object, got {type(items).__name__}")
    plan = plan_abx(items, [0, x.shape[0]] if offsets is None else offsets, max_group, seed, by)
    if plan.tasks.shape[0] == 0:
        raise ValueError("no (cell, phone, phone) task: no cell holds two phones one of which has two items")
    dev = x.device
    with torch.cuda.device(dev):
        run = SimpleNamespace(x=x, code=_hip.dtype_code(x.dtype), metric=code, pairs=torch.from_numpy(plan.pairs).to(dev),
                              tasks=torch.from_numpy(plan.tasks).to(dev),
                              dist=torch.empty(plan.pairs.shape[0], device=dev, dtype=torch.float32),
                              out=torch.empty(plan.tasks.shape[0], device=dev, dtype=torch.int64))
        _launch_abx(run)
        out = run.out.cpu().numpy()
    n_p, n_q = plan.tasks[:, 3], plan.tasks[:, 5]
    triples = n_p * (n_p - 1) * n_q
    valid = out >= 0
    scores = out[valid].astype(np.float64) / (2.0 * triples[valid].astype(np.float64))
    mean, pair_scores = average_scores(plan.keys[valid], scores)
    return ABXResult(error=1.0 - mean, pair_scores=pair_scores, phones=sorted({int(v) for v in items.phone[plan.picked]}),
                     n_pairs=int(plan.pairs.shape[0]), n_tasks=int(plan.tasks.shape[0]), n_triples=int(triples[valid].sum()),
                     n_invalid=int((~valid).sum()))
