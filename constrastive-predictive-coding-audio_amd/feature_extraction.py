"""Whole-recording feature extraction: z_t and c_t of every frame of every recording, on the HIP path ("Whole-recording
feature extraction").

A train step sees clips of one length and keeps the context at the last visible step.  The step after pre-training runs the trained
encoder and context network over whole recordings and feeds the per-frame vectors to a probe.  ``FeatureExtractor`` does that in
chunks: ``streams`` recordings advance side by side, ``chunk_frames`` frames per step, and the recurrent state of a recording is handed
from one chunk to the next on the device.  The conv stack is valid and unpadded, so frame t depends on samples [t ds, t ds + rf) only
and a chunk of frames is computed from its own window of samples; the recurrence kernels take an initial state and return f32 masters.

All steps are laid out on the host up front (``plan_schedule``) and uploaded once; between the first and the last launch of
``extract`` there is no synchronisation, no host <-> device copy and no allocation.  Per step: cpc_stream_gather (the samples),
cpc_conv1_fwd / cpc_conv_fwd (the encoder), cpc_gemm_nt + cpc_gru_fwd_h0 per layer or cpc_lstm_fwd (the context), cpc_feature_emit
(the frames into the feature stores, and the pooled sums), cpc_stream_carry (the state hand-off).  Forward only; the buffers are the
extractor's own, so the training engines, ``autoregressive_model.hidden``, ``model.training`` and the random state stay as they are.
"""
from __future__ import annotations

import ctypes as C
import heapq
from types import SimpleNamespace
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _hip

ROW = 6          # int64 entries per table row: first_sample, n_samples, n_frames, out_row, rec, keep
MAX_CHUNK_FRAMES = 1 << 20          # cpc_feature_emit's grid; the recurrence kernels themselves put no limit on the steps of a call
MAX_STREAMS = 65535


def frame_count(n_samples, receptive_field, downsampling):
    """Frames of a recording of n_samples samples: (N - rf) // ds + 1, or 0 below one receptive field.  Scalars or arrays."""
    n = np.asarray(n_samples, dtype=np.int64)
    return np.where(n >= receptive_field, (n - receptive_field) // downsampling + 1, 0).astype(np.int64)


class Schedule(NamedTuple):
    table: np.ndarray               # int64 [n_steps][R][6]
    frame_counts: np.ndarray        # int64 [n]
    frame_offsets: np.ndarray       # int64 [n + 1]


def plan_schedule(first_samples, lengths, receptive_field, downsampling, streams, chunk_frames) -> Schedule:
    """Every step of an extraction: recordings are dealt to ``streams`` streams from a queue in their order, a stream takes the next
    recording at the step after its current one ends (of several free streams the lowest goes first), and a recording of F frames runs
    as ceil(F / Tc) chunks of at most Tc = ``chunk_frames`` frames on consecutive steps of its stream.  Row (j, r) of the table is what
    stream r does at step j (the entries: include/cpc_hip.h, feature extraction); idle rows are (0, 0, 0, 0, -1, 0)."""
    rf, ds, R, Tc = int(receptive_field), int(downsampling), int(streams), int(chunk_frames)
    first = np.asarray(first_samples, dtype=np.int64).reshape(-1)
    length = np.asarray(lengths, dtype=np.int64).reshape(-1)
    n = first.shape[0]
    frames = frame_count(length, rf, ds)
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(frames)])
    chunks = -(-frames // Tc)
    # the deal: a heap of (first free step, stream); only the recordings' chunk counts enter, the rows follow vectorised below
    stream_of = np.full(n, -1, np.int64)
    first_step = np.full(n, -1, np.int64)
    free = [(0, r) for r in range(R)]
    n_steps = 0
    for i in np.nonzero(chunks)[0]:
        at, r = heapq.heappop(free)
        stream_of[i], first_step[i] = r, at
        n_steps = max(n_steps, at + int(chunks[i]))
        heapq.heappush(free, (at + int(chunks[i]), r))
    table = np.zeros((n_steps, R, ROW), np.int64)
    table[:, :, 4] = -1
    total = int(chunks.sum())
    if total:
        rec = np.repeat(np.arange(n, dtype=np.int64), chunks)                      # the recording of every chunk
        k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(chunks) - chunks, chunks)          # its number in the recording
        nf = np.minimum(Tc, frames[rec] - k * Tc)
        rows = np.stack([first[rec] + k * Tc * ds, (nf - 1) * ds + rf, nf, offsets[rec] + k * Tc, rec,
                         (k < chunks[rec] - 1).astype(np.int64)], axis=1)
        table[first_step[rec] + k, stream_of[rec]] = rows
    return Schedule(table, frames, offsets)


class PooledFeatures(NamedTuple):
    mean: torch.Tensor          # (n, channels) float32
    std: torch.Tensor           # (n, channels) float32: the population deviation, sqrt(max(E[x^2] - mean^2, 0))


class Features:
    """What ``FeatureExtractor.extract`` returns.  ``z`` (total_frames, E) and ``c`` (total_frames, H): device tensors of the
    extractor's out_dtype, present for the kinds that were asked for; c_t is the (top layer's) state after frame t from a zero state at
    the start of the recording.  Recording i of the result owns rows [frame_offsets[i], frame_offsets[i + 1]); ``frame_counts`` and
    ``file_indices`` (the index of each recording in its source) are host lists like ``frame_offsets``.  ``pooled``: with pool=True
    {"z": PooledFeatures, "c": PooledFeatures} for the kinds asked for, else None."""

    def __init__(self, z, c, frame_offsets, frame_counts, file_indices, pooled):
        if z is not None:
            self.z = z
        if c is not None:
            self.c = c
        self.frame_offsets, self.frame_counts, self.file_indices, self.pooled = frame_offsets, frame_counts, file_indices, pooled

    @property
    def total_frames(self):
        return self.frame_offsets[-1]

    def recording(self, i, kind="c"):
        """The (frames, channels) rows of recording i of the result."""
        return getattr(self, kind)[self.frame_offsets[i]:self.frame_offsets[i + 1]]


def check_extraction_supported(model, features):
    """The refusals, before anything touches a device: returns the kinds as a tuple in the order ("z", "c")."""
    from .audio_model import AudioEncoder, AudioGRUModel, AudioLSTMModel
    kinds = (features,) if isinstance(features, str) else tuple(features)
    if not kinds or any(k not in ("z", "c") for k in kinds) or len(set(kinds)) != len(kinds):
        raise ValueError(f"features must name 'z', 'c' or both, got {features!r}")
    kinds = tuple(k for k in ("z", "c") if k in kinds)
    enc, ar = model.encoder, model.autoregressive_model
    if not isinstance(enc, AudioEncoder):
        raise NotImplementedError(f"whole-recording feature extraction needs an AudioEncoder, not {type(enc).__name__}: the CQT front end "
                                  "of a ScalogramResidualEncoder is padded, so a frame depends on samples outside its own window and a "
                                  "recording cannot be computed chunk by chunk from windows of samples")
    if "c" in kinds and not isinstance(ar, (AudioGRUModel, AudioLSTMModel)):
        raise NotImplementedError(f"'c' of every frame needs a recurrent context (AudioGRUModel or AudioLSTMModel), not "
                                  f"{type(ar).__name__}: a convolutional or attention context defines c for a window of visible_steps "
                                  "frames only (a sliding-window recompute per frame is not built); features=('z',) works")
    return kinds


class _StreamEngine:
    """The device side for one (streams, chunk_frames) on one device in one storage type: activation buffers of the encoder for R
    windows of L = (Tc - 1) ds + rf samples (no gradient buffers), the recurrence's buffers for R items of Tc steps, the two state sets
    of the hand-off, and operand copies of its own."""

    def __init__(self, model, kinds, R, Tc, device, dtype):
        from .contexts import ContextHost
        from .engine import CPCEngine, EncoderGeometry
        from .audio_model import AudioGRUModel
        enc, ar = model.encoder, model.autoregressive_model
        self.model, self.kinds, self.R, self.Tc = model, kinds, R, Tc
        self.device, self.dt, self.code = torch.device(device), dtype, _hip.dtype_code(dtype)
        model._flatten_parameters(self.device)
        self.strides, self.kernels, self.channels = list(enc.strides), list(enc.kernel_sizes), list(enc.channel_count)
        self.n, self.E = len(self.strides), self.channels[-1]
        CPCEngine._check_supported(self)          # (the encoder kernels' shape rules, as for a train step)
        self.ds, self.rf = int(enc.downsampling_factor), int(enc.receptive_field)
        self.L = (Tc - 1) * self.ds + self.rf
        self.geo = EncoderGeometry(self.L, self.strides, self.kernels)
        assert self.geo.frames == Tc
        La = self.geo.alloc
        if self.L > (1 << 24) or R * La[0] >= (1 << 31) or R * La[0] * self.channels[0] >= (1 << 40):
            raise ValueError(f"streams = {R} with chunk_frames = {Tc} is too large: windows of {self.L} samples (at most 2^24) and "
                             f"{R * La[0]} layer-1 rows (below 2^31)")
        buf = lambda rows, cols, guard_rows: ContextHost._buf(self, rows, cols, guard_rows)
        f32 = dict(device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self.x = torch.zeros(R * self.L + 64, **f32)          # the step's windows [R][L] (zeros behind: layer 1 never reads them)
            # act[l] is read (kernel - stride) rows past its end by layer l + 1: ContextHost._buf's guard rows
            guard_rows = max([16] + [self.kernels[l] - self.strides[l] for l in range(1, self.n)])
            self.act, self.guard, self._keep = [], [], []
            for l in range(self.n):
                full, view, g_el = buf(R * La[l], self.channels[l], guard_rows)
                self._keep.append(full)
                self.act.append(view)
                self.guard.append(g_el)
            self.w_fwd = [None] + [torch.empty(self.channels[l] * self.kernels[l] * self.channels[l - 1], device=self.device, dtype=dtype)
                                   for l in range(1, self.n)]
            self.layers, self.lstm = [], None
            if "c" in kinds:
                self.H = H = int(ar.hidden_size)
                ch = 8 if dtype == torch.bfloat16 else 4
                if ar.input_size != self.E or H % (4 * ch) or H > 512 or H < 1:
                    raise NotImplementedError(f"HIP recurrence kernels: input size = the encoder's {self.E} channels, hidden size <= 512 and "
                                              f"a multiple of {4 * ch} in this storage type (got {ar.input_size}, {H})")
                if isinstance(ar, AudioGRUModel):
                    self._alloc_gru(ar)
                else:
                    self._alloc_lstm()
            else:
                self.H = 0
            nblk = -(-Tc // 32)          # (cpc_feature_emit's blocks of 32 frames, include/cpc_hip.h)
            self.partial = torch.empty(R * nblk * 2 * (self.E + self.H), device=self.device, dtype=torch.float64)

    def _alloc_gru(self, ar):
        R, Tc, H, dev, dt = self.R, self.Tc, self.H, self.device, self.dt
        tape = max(1, int(_hip.lib().cpc_gru_tape_elems(R, Tc, H, self.code)))
        for l in range(int(getattr(ar, "num_layers", 1))):
            In = self.E if l == 0 else H
            lay = SimpleNamespace(prefix="autoregressive_model.gruCell." if l == 0 else f"autoregressive_model.upper_cells.{l - 1}.", In=In)
            lay.w_ih = torch.empty(3 * H * In, device=dev, dtype=dt)
            lay.w_hh_frag = torch.empty(3 * H * H, device=dev, dtype=dt)
            lay.Gi = torch.empty(R * Tc * 3 * H, device=dev, dtype=dt)
            lay.Hall = torch.empty(R * (Tc + 1) * H, device=dev, dtype=dt)
            lay.tape = torch.zeros(tape, device=dev, dtype=dt)
            lay.h0 = torch.zeros(R, H, device=dev, dtype=torch.float32)          # the state the step starts from (cpc_stream_carry's dst)
            lay.h_out = torch.zeros(R, H, device=dev, dtype=torch.float32)       # the f32 master the recurrence leaves
            self.layers.append(lay)
        self.state_src = [lay.h_out for lay in self.layers]
        self.state_dst = [lay.h0 for lay in self.layers]

    def _alloc_lstm(self):
        R, Tc, H, dev, dt = self.R, self.Tc, self.H, self.device, self.dt
        tape = max(1, int(_hip.lib().cpc_lstm_tape_elems(R, Tc, H, self.code)))
        f32 = dict(device=dev, dtype=torch.float32)
        self.lstm = SimpleNamespace(prefix="autoregressive_model.lstmCell.",
                                    w_ih=torch.empty(4 * H * self.E, device=dev, dtype=dt), w_hh_frag=torch.empty(4 * H * H, device=dev, dtype=dt),
                                    Gi=torch.empty(R * Tc * 4 * H, device=dev, dtype=dt), Hall=torch.empty(R * (Tc + 1) * H, device=dev, dtype=dt),
                                    tape=torch.zeros(tape, device=dev, dtype=dt), h0=torch.zeros(R, H, **f32), c0=torch.zeros(R, H, **f32),
                                    h_out=torch.zeros(R, H, **f32), cell_out=torch.zeros(R, H, **f32))
        self.state_src = [self.lstm.h_out, self.lstm.cell_out]
        self.state_dst = [self.lstm.h0, self.lstm.c0]

    def hbm_bytes(self):
        seen = list(self._keep) + [self.x, self.partial] + [w for w in self.w_fwd if w is not None]
        for rec in self.layers + ([self.lstm] if self.lstm is not None else []):
            seen += [v for v in vars(rec).values() if isinstance(v, torch.Tensor)]
        return sum(t.numel() * t.element_size() for t in seen)

    # ------------------------------------------------------------------------------------------------------------- per call
    def prepare(self):
        """The operand copies from the parameters as they are now, and zero states (every call starts its recordings from zero)."""
        p, code = self.model._param, self.code
        for l in range(1, self.n):
            _hip.call("cpc_conv_w_prep", _hip.ptr(p[f"encoder.layers.{l}.weight"]), _hip.ptr(self.w_fwd[l]), None, self.channels[l],
                      self.channels[l - 1], self.kernels[l], self.strides[l], code)
        H = self.H
        for lay in self.layers:
            _hip.call("cpc_cast2d", _hip.ptr(p[lay.prefix + "weight_ih"]), _hip.ptr(lay.w_ih), 3 * H, lay.In, lay.In, 1, code)
            _hip.call("cpc_prep_frag", _hip.ptr(p[lay.prefix + "weight_hh"]), _hip.ptr(lay.w_hh_frag), 3 * H, H, H, 0, code)
        if self.lstm is not None:
            ls = self.lstm
            _hip.call("cpc_cast2d", _hip.ptr(p[ls.prefix + "weight_ih"]), _hip.ptr(ls.w_ih), 4 * H, self.E, self.E, 1, code)
            _hip.call("cpc_prep_frag", _hip.ptr(p[ls.prefix + "weight_hh"]), _hip.ptr(ls.w_hh_frag), 4 * H, H, H, 0, code)
        if "c" in self.kinds:
            for t in self.state_dst:
                t.zero_()
            n = len(self.state_src)
            self._carry_src = (C.c_void_p * n)(*[t.data_ptr() for t in self.state_src])
            self._carry_dst = (C.c_void_p * n)(*[t.data_ptr() for t in self.state_dst])

    def step(self, run, block):
        """One step: ``block`` is the device address of its table block.  Launches only."""
        p, code, R, Tc, La, Lv = self.model._param, self.code, self.R, self.Tc, self.geo.alloc, self.geo.valid
        ext = (C.c_longlong(run.store_len), self.L, Tc, C.c_longlong(run.total_frames), run.n_rec)
        _hip.call("cpc_stream_gather", _hip.ptr(run.store), run.store_code, C.c_longlong(run.store_len), block, _hip.ptr(self.x), R, self.L,
                  C.c_longlong(self.L), run.scale, Tc, C.c_longlong(run.total_frames), run.n_rec)
        _hip.call("cpc_conv1_fwd", _hip.ptr(self.x), _hip.ptr(p["encoder.layers.0.weight"]), _hip.ptr(p.get("encoder.layers.0.bias")),
                  _hip.ptr(self.act[0]), R, self.channels[0], self.strides[0], self.kernels[0], C.c_longlong(self.L), Lv[0], La[0],
                  1 if self.n > 1 else 0, code, None)
        for l in range(1, self.n):
            _hip.call("cpc_conv_fwd", _hip.ptr(self.act[l - 1]), _hip.ptr(self.w_fwd[l]), _hip.ptr(p.get(f"encoder.layers.{l}.bias")),
                      _hip.ptr(self.act[l]), R, self.channels[l - 1], self.channels[l], self.kernels[l], self.strides[l], La[l], Lv[l],
                      1 if l < self.n - 1 else 0, C.c_longlong(self.guard[l - 1]), code)
        H, E = self.H, self.E
        hall = None
        for l, lay in enumerate(self.layers):
            if l == 0:
                x, x_item, x_extent = _hip.ptr(self.act[-1]), La[-1] * E, 0
            else:          # rows h_1 .. h_Tc of the layer below, straight out of its hidden-state buffer
                x, x_item, x_extent = _hip.ptr(self.layers[l - 1].Hall, H), (Tc + 1) * H, R * (Tc + 1) * H - H
            _hip.gemm_nt(x, _hip.ptr(lay.w_ih), _hip.ptr(lay.Gi), R * Tc, 3 * H, lay.In, lay.In, lay.In, 3 * H, code,
                         bias=_hip.ptr(p.get(lay.prefix + "bias_ih")), a_rpi=Tc, a_item=x_item, a_extent=x_extent)
            _hip.call("cpc_gru_fwd_h0", _hip.ptr(lay.Gi), _hip.ptr(lay.w_hh_frag), _hip.ptr(p.get(lay.prefix + "bias_hh")), _hip.ptr(lay.h0),
                      _hip.ptr(lay.Hall), _hip.ptr(lay.tape), _hip.ptr(lay.h_out), R, Tc, H, code)
            hall = lay.Hall
        if self.lstm is not None:
            ls = self.lstm
            _hip.gemm_nt(_hip.ptr(self.act[-1]), _hip.ptr(ls.w_ih), _hip.ptr(ls.Gi), R * Tc, 4 * H, E, E, E, 4 * H, code,
                         bias=_hip.ptr(p.get(ls.prefix + "bias_ih")), a_rpi=Tc, a_item=La[-1] * E)
            _hip.call("cpc_lstm_fwd", _hip.ptr(ls.Gi), _hip.ptr(ls.w_hh_frag), _hip.ptr(p.get(ls.prefix + "bias_hh")), _hip.ptr(ls.h0),
                      _hip.ptr(ls.c0), _hip.ptr(ls.Hall), _hip.ptr(ls.tape), _hip.ptr(ls.h_out), _hip.ptr(ls.cell_out), R, Tc, H, code)
            hall = ls.Hall
        _hip.call("cpc_feature_emit", block, _hip.ptr(self.act[-1]), C.c_longlong(La[-1] * E), _hip.ptr(hall), C.c_longlong((Tc + 1) * H),
                  code, _hip.ptr(run.z), _hip.ptr(run.c), run.out_code, R, Tc, E, H, *ext[:2], *ext[3:],
                  _hip.ptr(self.partial) if run.pool else None, _hip.ptr(run.acc_z), _hip.ptr(run.acc_c))
        if "c" in self.kinds:
            _hip.call("cpc_stream_carry", block, self._carry_src, self._carry_dst, len(self.state_src), R, H, ext[0], self.L, Tc,
                      ext[3], run.n_rec)


class FeatureExtractor:
    """z and c of every frame of every recording of a source, on the HIP path.

    ``model``: an AudioPredictiveCodingModel with an AudioEncoder and, for "c", an AudioGRUModel (1 .. 4 layers) or AudioLSTMModel;
    ``features=("z",)`` works with any context network behind an AudioEncoder.  Other combinations raise NotImplementedError here,
    before anything touches a device.  ``streams`` recordings advance side by side, ``chunk_frames`` frames per step; the device
    buffers are sized once per extractor, at the first ``extract``.  ``out_dtype``: torch.float32 or torch.bfloat16, the type of the
    feature stores.  ``pool``: also the mean and population deviation of every channel over each recording's frames.

    ``extract(source, files=None)``: ``source`` is a DeviceAudioDataset that has a device (its store and file boundaries are used;
    item_length, unique_length and cross_files play no part), or a sequence of 1-D int16 / float32 arrays or tensors, uploaded once
    (int16 is scaled by 1 / 32768 as the dataset does); ``files``: the recordings to run, as indices into the source (default: all, in
    order).  A recording shorter than one receptive field has no frames and contributes nothing.  Forward only, under no_grad, with
    the model's weights as they are at the call."""

    def __init__(self, model, features=("z", "c"), streams=32, chunk_frames=1024, out_dtype=torch.float32, pool=True):
        self.kinds = check_extraction_supported(model, features)
        for name, v, hi in (("streams", streams, MAX_STREAMS), ("chunk_frames", chunk_frames, MAX_CHUNK_FRAMES)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
                raise ValueError(f"{name} must be an int in 1 .. {hi}, got {v!r}")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype!r}")
        self.model, self.streams, self.chunk_frames = model, int(streams), int(chunk_frames)
        self.out_dtype, self.pool = out_dtype, bool(pool)
        self._engine = None

    def _engine_for(self, device):
        eng, dt = self._engine, self.model.compute_dtype
        stale = eng is None or eng.device != device or eng.dt != dt or self.model._flat_param is None or any(
            p.data_ptr() != self.model._param[n].data_ptr() for n, p in self.model.named_parameters())
        if stale:
            eng = self._engine = _StreamEngine(self.model, self.kinds, self.streams, self.chunk_frames, device, dt)
        return eng

    def _source(self, source, device):
        """(store, store_code, scale, [(first sample, length)] per file) of a dataset or of arrays uploaded into a temporary store."""
        from .audio_dataset import DeviceAudioDataset
        if isinstance(source, DeviceAudioDataset):
            if source.device is None:
                raise ValueError("feature extraction reads the samples in HBM: build the DeviceAudioDataset with device=")
            store, scale = source._store, source._scale          # (read only: the dataset goes on cutting its windows from the store)
            if store.device != device:
                raise ValueError(f"the dataset's samples are on {store.device}, the model is on {device}")
            return store, 1 if store.dtype == torch.int16 else 0, scale, source.file_ranges()
        arrays = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in source]
        if not arrays:
            raise ValueError("no recordings")
        for k, a in enumerate(arrays):
            if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
                raise ValueError(f"recording {k}: a 1-D int16 or float32 array, not {a.dtype} with {a.ndim} dimensions")
        if any(a.dtype != np.int16 for a in arrays):          # mixed: everything as float32 (int16 / 32768 is exact)
            arrays = [a.astype(np.float32) * np.float32(1.0 / 32768.0) if a.dtype == np.int16 else a for a in arrays]
            code, scale = 0, 1.0
        else:
            code, scale = 1, 1.0 / 32768.0
        lengths = np.asarray([a.shape[0] for a in arrays], dtype=np.int64)
        first = np.concatenate([np.zeros(1, np.int64), np.cumsum(lengths)[:-1]])
        host = np.concatenate(arrays) if int(lengths.sum()) else np.zeros(1, arrays[0].dtype)
        return torch.from_numpy(host).to(device), code, scale, list(zip(first.tolist(), lengths.tolist()))

    def extract(self, source, files: Optional[Sequence[int]] = None) -> Features:
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("feature extraction runs on the GPU only (no CPU fallback): call model.to('cuda') first")
        with torch.no_grad(), torch.cuda.device(device):
            store, store_code, scale, ranges = self._source(source, device)
            index = list(range(len(ranges))) if files is None else [int(i) for i in files]
            if any(not 0 <= i < len(ranges) for i in index):
                raise IndexError(f"file indices outside [0, {len(ranges)})")
            eng = self._engine_for(device)
            sched = plan_schedule([ranges[i][0] for i in index], [ranges[i][1] for i in index], eng.rf, eng.ds, self.streams,
                                  self.chunk_frames)
            return self._run(eng, sched, store, store_code, scale, index)

    def _run(self, eng, sched, store, store_code, scale, index):
        n, total, n_steps = len(index), int(sched.frame_offsets[-1]), sched.table.shape[0]
        dev, f64 = eng.device, torch.float64
        run = SimpleNamespace(store=store, store_code=store_code, store_len=int(store.numel()), scale=float(scale), total_frames=total,
                              n_rec=max(n, 1), pool=self.pool, out_code=_hip.dtype_code(self.out_dtype), z=None, c=None, acc_z=None,
                              acc_c=None)
        # everything the loop needs, before its first launch: the feature stores, the accumulators, the table (one upload)
        if "z" in self.kinds:
            run.z = torch.empty(total, eng.E, device=dev, dtype=self.out_dtype)
            run.acc_z = torch.zeros(run.n_rec, 2, eng.E, device=dev, dtype=f64) if self.pool else None
        if "c" in self.kinds:
            run.c = torch.empty(total, eng.H, device=dev, dtype=self.out_dtype)
            run.acc_c = torch.zeros(run.n_rec, 2, eng.H, device=dev, dtype=f64) if self.pool else None
        table = torch.from_numpy(sched.table.reshape(-1)).to(dev) if n_steps else None
        counts = torch.from_numpy(sched.frame_counts.astype(np.float64)).to(dev) if self.pool else None
        eng.prepare()
        base, block_bytes = (table.data_ptr(), eng.R * ROW * 8) if n_steps else (0, 0)
        for j in range(n_steps):
            self._step(eng, run, C.c_void_p(base + j * block_bytes))
        pooled = None
        if self.pool:
            pooled = {k: self._finish_pool(acc, counts) for k, acc in (("z", run.acc_z), ("c", run.acc_c)) if k in self.kinds}
        return Features(run.z, run.c, [int(v) for v in sched.frame_offsets], [int(v) for v in sched.frame_counts], list(index), pooled)

    def _step(self, eng, run, block):
        """The loop body (launches only; tests wrap it to see that no host copy happens inside)."""
        eng.step(run, block)

    @staticmethod
    def _finish_pool(acc, counts):
        """mean and sqrt(max(E[x^2] - mean^2, 0)) from the f64 sums; a recording without frames has both 0."""
        acc = acc[:counts.shape[0]]
        n = counts.clamp(min=1.0).unsqueeze(1)
        mean = acc[:, 0] / n
        std = (acc[:, 1] / n - mean * mean).clamp(min=0.0).sqrt()
        return PooledFeatures(mean.float(), std.float())


def extract_features(model, source, files=None, **kw) -> Features:
    """``FeatureExtractor(model, **kw).extract(source, files)`` with the extractor (and its device buffers) kept on the model per
    keyword set, so that repeated calls allocate once."""
    cache = model.__dict__.setdefault("_feature_extractors", {})
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))
    if key not in cache:
        cache[key] = FeatureExtractor(model, **kw)
    return cache[key].extract(source, files)
