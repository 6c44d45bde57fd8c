"""Host restatement of the negative sampler of the sampled InfoNCE loss (include/cpc_hip.h, cpc_nce_loss_sampled; DESIGN.md,
"Sampled negatives").  CPU only, numpy uint64 arithmetic (which wraps modulo 2^64): what "bit-exact given a fixed seed" is tested
against, and what a run can call to log which negatives a step drew."""
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
