"""K-means units over feature rows on the HIP path ("K-means units").

``FeatureExtractor`` leaves z and c of every frame in HBM; a k-means codebook over those frames gives the per-frame labels that serve
as discrete units (unit discovery, ABX-style evaluation, targets of later models).  ``KMeans.fit`` runs Lloyd iterations on the device:
cpc_kmeans_assign (the N x K x D distance product fused with the argmin, the N x K values never stored) and cpc_kmeans_update (a
stable counting sort by label and f64 sums in a fixed order: no floating-point atomics, the same bits on every run).  Everything is
allocated before the first launch; between the first and the last launch of ``fit`` there is no synchronisation, no host <-> device
copy and no allocation.  Forward only: engines, the random state of torch and ``model.training`` are not touched.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _hip

MIN_DIM, MAX_DIM, DIM_STEP = 16, 512, 16          # the kernels' limits (include/cpc_hip.h, k-means)
MIN_CLUSTERS, MAX_CLUSTERS = 2, 1024
MAX_ROWS = 2 ** 31 - 1


def sample_rows(n_rows, n_clusters, seed):
    """The rows init="sample" starts from: numpy.random.default_rng(seed).choice(n_rows, n_clusters, replace=False), sorted."""
    if n_rows < n_clusters:
        raise ValueError(f"{n_rows} rows cannot seed {n_clusters} clusters")
    return np.sort(np.random.default_rng(seed).choice(n_rows, n_clusters, replace=False)).astype(np.int64)


def _rows_of(x, kind):
    """(tensor, frame_offsets or None) of a tensor or a Features object; the refusals that need no device."""
    offsets = None
    if not isinstance(x, torch.Tensor):
        if kind not in ("z", "c"):
            raise ValueError(f"kind must be 'z' or 'c', got {kind!r}")
        if not hasattr(x, "frame_offsets"):
            raise TypeError(f"expected a tensor or a Features object, got {type(x).__name__}")
        if not hasattr(x, kind):
            raise ValueError(f"the Features object holds no {kind!r}")
        offsets, x = x.frame_offsets, getattr(x, kind)
    if not x.is_cuda:
        raise ValueError("KMeans runs on the device: x is a CPU tensor (there is no CPU path)")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"x must be float32 or bfloat16, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"x must be (N, D), got {tuple(x.shape)}")
    n, d = x.shape
    if not (1 <= n <= MAX_ROWS):
        raise ValueError(f"N = {n} is outside [1, 2^31 - 1]")
    if not (MIN_DIM <= d <= MAX_DIM) or d % DIM_STEP:
        raise ValueError(f"D = {d} must be a multiple of {DIM_STEP} in [{MIN_DIM}, {MAX_DIM}]")
    ch = 4 if x.dtype == torch.float32 else 8
    if x.stride(1) != 1 or (n > 1 and (x.stride(0) < d or x.stride(0) % ch)):
        raise ValueError(f"the rows of x must be contiguous, at a row stride that is a multiple of {ch} elements (strides {x.stride()})")
    if x.data_ptr() % 16:
        raise ValueError("x must start at a 16-byte boundary")
    return x, offsets


class KMeans:
    """Lloyd's k-means on the device.  After ``fit``: ``centers`` f32 (K, D), ``counts`` int32 (K,), ``labels`` int32 (N,) of the last
    assignment (taken against the centres before the last update) and ``inertia`` f64 (iterations,), the summed squared distance of
    each assignment; all device tensors.  A cluster that loses all its rows keeps its centre; a row holding a NaN or an infinity gets
    the label -1 and enters no centre."""

    def __init__(self, n_clusters, iterations=20, seed=0, init="sample"):
        if not (MIN_CLUSTERS <= int(n_clusters) <= MAX_CLUSTERS):
            raise ValueError(f"n_clusters = {n_clusters} is outside [{MIN_CLUSTERS}, {MAX_CLUSTERS}]")
        if int(iterations) < 1:
            raise ValueError("iterations must be at least 1")
        if isinstance(init, torch.Tensor):
            if init.dim() != 2 or init.shape[0] != int(n_clusters):
                raise ValueError(f"init must be ({n_clusters}, D), got {tuple(init.shape)}")
        elif init != "sample":
            raise ValueError(f"init must be 'sample' or a (K, D) tensor, got {init!r}")
        self.n_clusters, self.iterations, self.seed, self.init = int(n_clusters), int(iterations), int(seed), init
        self.centers = self.cnorm = self.counts = self.labels = self.inertia = None

    # ------------------------------------------------------------------------------------------------------------ fit
    def _prepare(self, x):
        """Everything ``fit`` allocates, and the initial centres with their norms."""
        K, (N, D), dev = self.n_clusters, x.shape, x.device
        if isinstance(self.init, torch.Tensor):
            if self.init.shape[1] != D:
                raise ValueError(f"init has {self.init.shape[1]} columns, x has {D}")
            rows = None
        else:
            rows = sample_rows(N, K, self.seed)
        nbytes = _hip.lib().cpc_kmeans_scratch_bytes(N, K, D)
        if nbytes < 0:
            raise _hip.HipCallError(f"cpc_kmeans_scratch_bytes refused (N, K, D) = {(N, K, D)}")
        with torch.cuda.device(dev):
            if rows is None:
                centers = self.init.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
            else:
                centers = x.index_select(0, torch.from_numpy(rows).to(dev)).to(torch.float32).contiguous()
            run = SimpleNamespace(
                x=x, N=N, D=D, K=K, ldx=x.stride(0) if N > 1 else D, code=_hip.dtype_code(x.dtype), centers=centers,
                cnorm=torch.empty(K, device=dev, dtype=torch.float32), counts=torch.zeros(K, device=dev, dtype=torch.int32),
                labels=torch.empty(N, device=dev, dtype=torch.int32), dist=torch.empty(N, device=dev, dtype=torch.float32),
                scratch=torch.empty(nbytes, device=dev, dtype=torch.uint8), scratch_bytes=nbytes,
                inertia=torch.zeros(self.iterations, device=dev, dtype=torch.float64))
            _hip.call("cpc_kmeans_cnorm", _hip.ptr(run.centers), _hip.ptr(run.cnorm), K, D)
        return run

    def _iterate(self, run, i):
        """One Lloyd iteration: launches only."""
        LL = C.c_longlong
        _hip.call("cpc_kmeans_assign", _hip.ptr(run.x), run.code, LL(run.N), run.D, LL(run.ldx), _hip.ptr(run.centers), _hip.ptr(run.cnorm),
                  run.K, _hip.ptr(run.labels), _hip.ptr(run.dist))
        _hip.call("cpc_kmeans_update", _hip.ptr(run.x), run.code, LL(run.N), run.D, LL(run.ldx), _hip.ptr(run.labels), _hip.ptr(run.dist),
                  _hip.ptr(run.centers), run.K, _hip.ptr(run.scratch), LL(run.scratch_bytes), _hip.ptr(run.centers), _hip.ptr(run.cnorm),
                  _hip.ptr(run.counts), _hip.ptr(run.inertia, i))

    def fit(self, x, kind="c"):
        """``x``: an (N, D) f32 or bf16 device tensor with contiguous rows (a row stride above D is allowed), or a ``Features`` object,
        of which ``kind`` picks z or c.  Returns self."""
        x, _ = _rows_of(x, kind)
        if isinstance(self.init, str) and x.shape[0] < self.n_clusters:
            raise ValueError(f"{x.shape[0]} rows cannot seed {self.n_clusters} clusters")
        run = self._prepare(x)
        with torch.cuda.device(x.device):
            for i in range(self.iterations):
                self._iterate(run, i)
        self.centers, self.cnorm, self.counts, self.labels, self.inertia = run.centers, run.cnorm, run.counts, run.labels, run.inertia
        return self

    # --------------------------------------------------------------------------------------------------------- assign
    def assign(self, x, return_distance=False, kind="c"):
        """Labels int32 (N,) of the rows of ``x`` against the current centres; with ``return_distance`` also the squared distances f32
        (N,).  For a ``Features`` input the labels share its ``frame_offsets``: recording i owns
        labels[frame_offsets[i]:frame_offsets[i + 1]]."""
        x, _ = _rows_of(x, kind)
        if self.centers is None:
            raise RuntimeError("assign before fit or load_state_dict")
        N, D = x.shape
        if D != self.centers.shape[1]:
            raise ValueError(f"x has {D} columns, the centres have {self.centers.shape[1]}")
        if x.device != self.centers.device:
            raise ValueError(f"x is on {x.device}, the centres are on {self.centers.device}")
        with torch.cuda.device(x.device):
            labels = torch.empty(N, device=x.device, dtype=torch.int32)
            dist = torch.empty(N, device=x.device, dtype=torch.float32) if return_distance else None
            _hip.call("cpc_kmeans_assign", _hip.ptr(x), _hip.dtype_code(x.dtype), C.c_longlong(N), D,
                      C.c_longlong(x.stride(0) if N > 1 else D), _hip.ptr(self.centers), _hip.ptr(self.cnorm), self.n_clusters,
                      _hip.ptr(labels), _hip.ptr(dist))
        return (labels, dist) if return_distance else labels

    # ----------------------------------------------------------------------------------------------------------- state
    def state_dict(self):
        if self.centers is None:
            raise RuntimeError("state_dict before fit or load_state_dict")
        return {"centers": self.centers.detach().clone(), "counts": self.counts.detach().clone()}

    def load_state_dict(self, state, device=None):
        """Centres and counts of a saved codebook; they go to ``device`` (default: where the saved centres are, which must be a GPU)."""
        centers, counts = state["centers"], state["counts"]
        K, D = centers.shape
        if K != self.n_clusters or counts.shape != (K,):
            raise ValueError(f"the state holds {K} centres and {tuple(counts.shape)} counts, this codebook has {self.n_clusters} clusters")
        if not (MIN_DIM <= D <= MAX_DIM) or D % DIM_STEP:
            raise ValueError(f"D = {D} must be a multiple of {DIM_STEP} in [{MIN_DIM}, {MAX_DIM}]")
        dev = torch.device(device) if device is not None else centers.device
        if dev.type != "cuda":
            raise ValueError("KMeans runs on the device: give load_state_dict a GPU device for a CPU state")
        with torch.cuda.device(dev):
            self.centers = centers.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
            self.counts = counts.detach().to(device=dev, dtype=torch.int32).contiguous().clone()
            self.cnorm = torch.empty(K, device=dev, dtype=torch.float32)
            _hip.call("cpc_kmeans_cnorm", _hip.ptr(self.centers), _hip.ptr(self.cnorm), K, D)
        self.labels = self.inertia = None
        return self
