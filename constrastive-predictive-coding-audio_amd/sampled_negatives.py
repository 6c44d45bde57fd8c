"""Host restatement of the negative sampler of the sampled InfoNCE loss (include/cpc_hip.h, cpc_nce_loss_sampled; DESIGN.md,
"Sampled negatives").  CPU only, numpy uint64 arithmetic (which wraps modulo 2^64): what "bit-exact given a fixed seed" is tested
against, and what a run can call to log which negatives a step drew.  grouped_negative_mask restates the grouped selection
(cpc_nce_loss_grouped; DESIGN.md, "Grouped negatives") the same way."""
import numpy as np
import torch

_M64 = (1 << 64) - 1
_DRAW, _STEP, _IDX = 0x632BE59BD9B4E019, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
_MIX1, _MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def check_negatives(B, n_neg):
    """1 <= n_neg <= B - 1, as every layer of the sampled loss requires; returns n_neg as an int."""
    if int(n_neg) != n_neg or not 1 <= int(n_neg) <= int(B) - 1:
        raise ValueError(f"num_negatives must be an integer in [1, batch_size - 1] = [1, {int(B) - 1}], got {n_neg}")
    return int(n_neg)


def sampled_negative_keys(B, K, seed, draw):
    """key[k][b'][b] (uint32 values in a uint64 array [K, B, B]) of prediction step k, target b' and candidate row b."""
    B, K = int(B), int(K)
    u = np.uint64
    s = (int(seed) + _DRAW * int(draw)) & _M64
    k = np.arange(K, dtype=np.uint64).reshape(K, 1, 1)
    bp = np.arange(B, dtype=np.uint64).reshape(1, B, 1)
    b = np.arange(B, dtype=np.uint64).reshape(1, 1, B)
    with np.errstate(over="ignore"):
        z = u(s) + u(_STEP) * (k + u(1)) + (bp * u(B) + b) * u(_IDX)
        z = (z ^ (z >> u(30))) * u(_MIX1)
        z = (z ^ (z >> u(27))) * u(_MIX2)
        z = z ^ (z >> u(31))
    return z >> u(32)


def sampled_negative_mask(B, K, n_neg, seed, draw):
    """BoolTensor [K, B, B], mask[k][b][b'] = row b is a candidate of target column (k, b'): its own row b' and the n_neg rows
    b != b' with the smallest (key, b).  Every column has exactly n_neg + 1 ones; n_neg = B - 1 gives all ones."""
    B, K = int(B), int(K)
    n_neg = check_negatives(B, n_neg)
    comp = (sampled_negative_keys(B, K, seed, draw) << np.uint64(32)) | np.arange(B, dtype=np.uint64).reshape(1, 1, B)   # [k][b'][b]
    diag = np.arange(B)
    comp[:, diag, diag] = np.uint64(_M64)                     # a column's own row takes no part in the selection
    thr = np.partition(comp, n_neg - 1, axis=2)[:, :, n_neg - 1:n_neg]
    m = comp <= thr
    m[:, diag, diag] = True
    return torch.from_numpy(np.ascontiguousarray(m.transpose(0, 2, 1)))


GROUP_MODES = {"same": 0, "other": 1}


def group_mode(mode):
    """0 for "same", 1 for "other" (the C ABI's mode); ValueError for anything else."""
    if mode not in GROUP_MODES:
        raise ValueError(f"mode must be one of {tuple(GROUP_MODES)}, got {mode!r}")
    return GROUP_MODES[mode]


def check_group_negatives(B, n_neg):
    """None or 0 (every eligible row) or 1 <= n_neg <= B - 1; returns the C ABI's n_neg (0 for None)."""
    if n_neg is None or (int(n_neg) == n_neg and int(n_neg) == 0):
        return 0
    return check_negatives(B, n_neg)


def group_eligibility(groups, mode):
    """bool array [b'][b]: row b is eligible for target b' — b != b' and (groups[b] == groups[b']) == (mode == "same")."""
    g = np.asarray(groups).astype(np.int64).reshape(-1)
    e = (g[:, None] == g[None, :]) == (group_mode(mode) == 0)
    e[np.arange(g.size), np.arange(g.size)] = False
    return e


def empty_negative_sets(groups, mode):
    """Number of batch items whose eligible set is empty (the same for every prediction step): under "same" the items whose id no
    other item shares, under "other" all of them when the batch holds one id and none otherwise.  O(B log B): the trainer calls it
    every step."""
    g = np.asarray(groups).reshape(-1)
    _, inverse, counts = np.unique(g, return_inverse=True, return_counts=True)
    if group_mode(mode) == 0:
        return int((counts[inverse] == 1).sum())
    return int(g.size) if counts.size == 1 else 0


def grouped_negative_mask(groups, K, mode, n_neg=None, seed=0, draw=0):
    """BoolTensor [K, B, B], mask[k][b][b'] = row b is a candidate of target column (k, b'): its own row b' and, of the rows eligible
    for b' (group_eligibility), the min(n_neg, their number) with the smallest (key, b) — all of them with n_neg None.  The keys are
    sampled_negative_keys(B, K, seed, draw), B = len(groups)."""
    g = np.asarray(groups).reshape(-1)
    B, K = int(g.size), int(K)
    n_neg = check_group_negatives(B, n_neg)
    elig = group_eligibility(g, mode)                          # [b'][b]
    comp = (sampled_negative_keys(B, K, seed, draw) << np.uint64(32)) | np.arange(B, dtype=np.uint64).reshape(1, 1, B)   # [k][b'][b]
    comp = np.where(elig[None], comp, np.uint64(_M64))         # a row that is not eligible takes no part in the selection
    count = elig.sum(axis=1)
    n = count if n_neg == 0 else np.minimum(n_neg, count)      # [b']
    srt = np.sort(comp, axis=2)
    thr = np.take_along_axis(srt, np.broadcast_to(np.maximum(n, 1).reshape(1, B, 1) - 1, (K, B, 1)), axis=2)
    m = (comp <= thr) & elig[None] & (n > 0).reshape(1, B, 1)
    diag = np.arange(B)
    m[:, diag, diag] = True
    return torch.from_numpy(np.ascontiguousarray(m.transpose(0, 2, 1)))


def file_group_ids(index_count_per_file):
    """int32 array: the file of every example index, for a dataset whose file f holds index_count_per_file[f] consecutive indices
    (audio_dataset's get_example_count_per_file())."""
    counts = np.asarray(list(index_count_per_file), dtype=np.int64)
    return np.repeat(np.arange(counts.size, dtype=np.int32), counts)
