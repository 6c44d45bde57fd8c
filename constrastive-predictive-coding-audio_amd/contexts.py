"""The context networks of the CPC train step, and what they may see of the engine that hosts them.

A context network (``Context``: GRUContext for AudioGRUModel, LSTMContext for AudioLSTMModel, ConvArContext / scalogram_engine.ConvArGridContext for
ConvolutionalArModel, AttentionContext for AttentionModel, scalogram_engine.ResNetArContext for a ScalogramResidualEncoder — the two
of scalogram_engine share its GridContext base —, Float32Context around the first or the third) turns the frames z = rows [T-K-V, T-K) of the encoder's top buffer into c and, backward, dc into dz in the same rows of the top
buffer's gradient plus its own parameter gradients.  It is built by make_context() for a ``ContextHost``: engine.CPCEngine and
scalogram_engine.ScalogramCPCEngine for a train step, ContextOnlyEngine for a stand-alone ``AudioGRUModel(...)(z)`` call, Float32Host
for a context that computes in float32 inside a bf16 engine.  A context reads its host and never writes it.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from types import SimpleNamespace

import torch

from . import _hip


_SIDE_STREAMS = {}


def side_stream(device):
    """ONE high-priority side stream per device for the whole process, shared by every engine: HIP multiplexes its streams
    onto a few hardware queues, and an engine created late in a process that had made one stream per engine ended up with a
    side stream sharing a hardware queue with the main stream (measured: the same step 6.9 -> 12.9 ms)."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device, priority=-1)
    return _SIDE_STREAMS[key]


def _ceil_div(a, b):
    return -(-a // b)


class ContextHost:
    """What a context network (and a grid layer of scalogram_engine) may read of the object it was built for.  This list is the
    contract; a host provides all of it, a context uses nothing else and writes none of it.

    Set by ``__init__`` here:
      model                 the AudioPredictiveCodingModel: ``_param`` / ``_grad`` (name -> view of the flat f32 buffers), ``_flat_param``
      device, dt, code      torch device, storage dtype and its C ABI code (_hip.dtype_code)
      B, E, H, K, V         batch size, enc_size, ar_size, prediction_steps, visible_steps
      colsum_blocks         most workgroups of a column-sum launch (sizes the bias-gradient scratch)
      aux                   the device's side stream (side_stream)
    Set by the subclass before it calls make_context():
      T, geo                encoder frames per item; ``geo.alloc[-1]`` = allocated rows per item of the top buffer
      act, dact             ``act[-1]`` / ``dact[-1]``: the encoder's top buffer [B][geo.alloc[-1]][E] and its gradient (storage dtype);
                            the context reads rows [T-K-V, T-K) of the first and writes dz into the same rows of the second
    Set by the subclass before the first forward():
      c                     (B, H) f32: the recurrent contexts leave c here
      slabs                 f32 workspace of at least ``ctx.slab_floats()`` elements (main-stream split reductions)
    Class-level defaults, overridden on an instance where needed:
      use_aux               False: everything on the launching stream (GraphedStep captures that way)
      _gp_phase             gradient-penalty step: which of its passes is running (0: an ordinary step)
      gp_capable            built for gradient-penalty steps
    Methods: side(), _buf(), _pick_split(), _chunk(), _tn_to_grad(), _colsum_to_grad(), count_batch().
    The grid layers also use ``_twins`` (the tangent grids of a gradient-penalty step), which ScalogramCPCEngine alone provides."""

    use_aux = True
    _gp_phase = 0
    gp_capable = False
    _nbt_batch = None           # count_batch: the counters collected by the forward pass in flight

    def __init__(self, model, device, dtype: torch.dtype, batch_size, enc_size, ar_size, prediction_steps, visible_steps):
        self.model = model
        self.device = torch.device(device)
        self.dt = dtype
        self.code = _hip.dtype_code(dtype)
        self.B, self.E, self.H = int(batch_size), int(enc_size), int(ar_size)
        self.K, self.V = int(prediction_steps), int(visible_steps)
        self.colsum_blocks = 1024
        model._flatten_parameters(self.device)
        # high-priority side stream for short kernels that need not sit between the large GEMMs (see CPCEngine._alloc_encoder)
        self.aux = side_stream(self.device)

    @contextlib.contextmanager
    def side(self, ev):
        """Work issued inside runs on the high-priority side stream once everything issued so far on the current stream
        has finished (event ``ev``); backward() joins the side stream before it returns."""
        if not self.use_aux:
            yield
            return
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.aux):
            self.aux.wait_event(ev)
            yield

    def _buf(self, rows: int, cols: int, guard_rows: int = 16):
        """Zeroed [rows][cols] storage-dtype buffer with ``guard_rows`` (>= 16) zero rows on both sides; returns (full, view,
        guard_elems).  The guards are what the overlapped-row GEMMs read beyond the array (include/cpc_hip.h, guard contract):
        kernel - stride rows after a convolution input, ceil(kernel / stride) - 1 rows before an output gradient."""
        guard = max(16, int(guard_rows)) * cols
        full = torch.zeros(guard + rows * cols + guard, device=self.device, dtype=self.dt)
        return full, full[guard:guard + rows * cols], guard

    def _pick_split(self, I, J, M, dt=None):
        dt = self.dt if dt is None else dt
        big = dt == torch.bfloat16 and I >= 256 and J >= 256       # 256x256 tiles, one workgroup per CU
        tile = 256 if big else 128
        tiles = _ceil_div(I, tile) * _ceil_div(J, tile)
        blk = 64 if dt == torch.bfloat16 else 32
        # as many splits as fit in ONE round of workgroups (256 CUs x one 256-tile or two 128-tile workgroups): rounding the
        # count up instead (30 tiles x 18 splits = 540 workgroups on 512 slots) leaves a second, almost empty round
        want = max(1, (256 if big else 512) // tiles)
        return max(1, min(want, _ceil_div(M, 8 * blk), 256))

    def _chunk(self, M, nsplit, dt=None):
        blk = 64 if (self.dt if dt is None else dt) == torch.bfloat16 else 32
        return _ceil_div(_ceil_div(M, nsplit), blk) * blk

    def _tn_to_grad(self, A, B_, grad, M, I, J, lda, ldb, nsplit, grad_offset=0, scratch=None, **kw):
        """grad[grad_offset + i*J + j] = sum_m A[m][i] B[m][j] via f32 slabs + deterministic reduction."""
        code = self.code
        chunk = self._chunk(M, nsplit)
        scratch = self.slabs if scratch is None else scratch
        _hip.gemm_tn(A, B_, _hip.ptr(scratch), M, I, J, lda, ldb, J, code, nsplit=nsplit, m_chunk=chunk, slab_stride=I * J,
                     flags=_hip.GEMM_OUT_F32, **kw)
        _hip.call("cpc_reduce_slabs", _hip.ptr(scratch), _hip.ptr(grad, grad_offset), I, J, nsplit, I * J, 1, 1, J, 0)

    def _colsum_to_grad(self, X, grad, M, N, code=None, scratch=None):
        nb = min(self.colsum_blocks, max(1, M // 64))
        scratch = self.slabs if scratch is None else scratch
        _hip.call("cpc_colsum", X, _hip.ptr(scratch), M, N, N, nb, self.code if code is None else code)
        _hip.call("cpc_reduce_slabs", _hip.ptr(scratch), _hip.ptr(grad), 1, N, nb, N, 1, 1, 0, 0)

    def count_batch(self, counter):
        """`num_batches_tracked += 1` of a train-mode BatchNorm (twelve of them in a configs[2] step, each a 5 us launch on the main queue):
        collected while forward() runs and added with one launch at its end; outside forward() (stand-alone calls) added at once."""
        if self._nbt_batch is None:
            counter += 1
        else:
            self._nbt_batch.append(counter)


class Context:
    """The protocol of a context network, with its defaults.  ``__init__(host, ar)`` checks the configuration; ``allocate()`` and
    ``slab_floats()`` size the buffers; ``prepare_weights()``, ``forward()``, ``backward(dc)`` are the step; ``c_operand()`` gives
    (tensor, element offset, item stride) of c in the storage dtype, ``c_float()`` c as (B, H) float32."""

    ahead_ok = False      # True: prepare_weights is a pure function of the parameters (CPCEngine.prepare_ahead)
    z_scale = 1.0         # what the network multiplies z by in place (AttentionModel: sqrt(C))
    anchors_ok = False    # True: backward() accepts gradients at earlier hidden states (``anchor_dHs``; GRUContext, LSTMContext)
    anchor_dHs = None     # prediction anchors: storage-dtype [B][V][H], row (b, t) the gradient that reaches h_{t+1} from the predictor;
                          # owned and filled by the engine (CPCEngine._alloc_head), read by backward() of the top recurrent layer

    def tangent(self, top_t):
        raise NotImplementedError(f"{type(self).__name__} has no tangent pass: no gradient penalty through this context network")

    def gp_grads(self, gp_grad):
        raise NotImplementedError(f"{type(self).__name__} has no tangent pass: no gradient penalty through this context network")


class GRUContext(Context):
    """AudioGRUModel as the context network (audio_model.py:47-77): per layer one batched input-projection GEMM for all V steps, the
    persistent GRU kernels for the recurrence, GEMMs for the weight gradients and for the gradient of the layer's input.

    ``self.layers``: one record per layer, bottom first, with its own operands, input projections ``Gi``, hidden states ``Hall``, tape
    and ``dG``.  Layer 0 reads the frames in the encoder's top buffer; layer l >= 1 (AudioGRUModel(num_layers = L > 1), DESIGN.md
    "Stacked GRU") reads the hidden states of the layer below as its input rows and runs behind it.  Backward: the top layer takes dc
    (cpc_gru_bwd); each layer below takes the gradient its hidden states receive from the input projection above, one row per
    (item, step) (cpc_gru_bwd_steps)."""

    ahead_ok = True       # prepare_weights is a pure function of the parameters (CPCEngine.prepare_ahead)
    anchors_ok = True

    def __init__(self, eng, ar):
        self.eng = eng
        self.ar = ar
        self.H = int(ar.hidden_size)
        ch = 8 if eng.dt == torch.bfloat16 else 4
        if ar.input_size != eng.E or self.H != eng.H:
            raise ValueError("AudioGRUModel sizes do not match enc_size / ar_size")
        if self.H % (4 * ch) or self.H > 512:
            raise NotImplementedError(f"HIP GRU kernel: hidden size must be <= 512 and a multiple of 32 in bf16, of 16 in float32 "
                                      f"(this engine: {'bf16' if ch == 8 else 'float32'}, hidden size {self.H})")
        self.L = int(getattr(ar, "num_layers", 1))
        self.layers = []          # (allocate)

    @property
    def upper(self):
        """Layers 1 .. L-1."""
        return self.layers[1:]

    def allocate(self):
        e = self.eng
        B, V, H, dev, dt = e.B, e.V, self.H, e.device, e.dt
        tape = max(1, int(_hip.lib().cpc_gru_tape_elems(B, max(V, 1), H, e.code)))
        for l in range(self.L):
            In = e.E if l == 0 else H             # input size: the frames' for layer 0, the hidden size of the layer below above it
            lay = SimpleNamespace(prefix="autoregressive_model.gruCell." if l == 0 else f"autoregressive_model.upper_cells.{l - 1}.", In=In)
            lay.w_ih = torch.empty(3 * H * In, device=dev, dtype=dt)          # [3H][In]
            lay.w_ih_t = torch.empty(In * 3 * H, device=dev, dtype=dt)        # [In][3H]
            lay.w_hh_frag = torch.empty(3 * H * H, device=dev, dtype=dt)
            lay.w_hh_t_frag = torch.empty(3 * H * H, device=dev, dtype=dt)
            lay.Gi = torch.empty(B * V * 3 * H, device=dev, dtype=dt)
            lay.Hall = torch.empty(B * (V + 1) * H, device=dev, dtype=dt)
            lay.tape = torch.zeros(tape, device=dev, dtype=dt)
            lay.dG = torch.empty(B * V * 4 * H, device=dev, dtype=dt)       # [dr | du | dn | dn*r] per (item, step)
            lay.split_ih = e._pick_split(3 * H, In, B * V)
            lay.split_hh = e._pick_split(2 * H, H, B * V)
            lay.ev = torch.cuda.Event()
            self.layers.append(lay)
        if self.L > 1:
            self.c_low = torch.empty(self.L - 1, B, H, device=dev, dtype=torch.float32)    # last hidden state of every layer below the top
            self.dH = torch.empty(B * V * H, device=dev, dtype=dt)       # gradient at h_1 .. h_V of the layer being differentiated
        self.scratch = torch.empty(self.slab_floats(), device=dev, dtype=torch.float32)     # side-stream workspace

    def slab_floats(self):
        """The side-stream workspace is shared by all layers (their parameter gradients run there one after the other): the largest."""
        e, H = self.eng, self.H
        return max(e.colsum_blocks * 4 * H, *[max(lay.split_ih * 3 * H * lay.In, lay.split_hh * 2 * H * H) for lay in self.layers])

    def prepare_weights(self):
        H, code = self.H, self.eng.code
        p = self.eng.model._param
        for lay in self.layers:
            w_ih, w_hh, In = p[lay.prefix + "weight_ih"], p[lay.prefix + "weight_hh"], lay.In
            _hip.call("cpc_cast2d", _hip.ptr(w_ih), _hip.ptr(lay.w_ih), 3 * H, In, In, 1, code)
            _hip.call("cpc_cast2d", _hip.ptr(w_ih), _hip.ptr(lay.w_ih_t), In, 3 * H, 1, In, code)
            _hip.call("cpc_prep_frag", _hip.ptr(w_hh), _hip.ptr(lay.w_hh_frag), 3 * H, H, H, 0, code)
            _hip.call("cpc_prep_frag", _hip.ptr(w_hh), _hip.ptr(lay.w_hh_t_frag), H, 3 * H, H, 1, code)

    def _input(self, l):
        """Layer l's input rows, V per item: (pointer, item stride in elements, elements readable from the pointer or 0 = unchecked).
        Layer 0 reads frames [T-K-V, T-K) of the encoder's top buffer, layer l >= 1 the rows h_1 .. h_V of the layer below straight
        out of its hidden-state buffer (from element H on)."""
        e, H, V = self.eng, self.H, self.eng.V
        if l == 0:
            return _hip.ptr(e.act[-1], (e.T - e.K - V) * e.E), e.geo.alloc[-1] * e.E, 0
        return _hip.ptr(self.layers[l - 1].Hall, H), (V + 1) * H, e.B * (V + 1) * H - H

    def forward(self):
        e, H = self.eng, self.H
        p, code, B, V = e.model._param, e.code, e.B, e.V
        # reset_hidden=False (audio_model.py:69, :75): the last hidden state of the previous call is this call's initial one
        carry = not getattr(self.ar, "reset_hidden", True)
        h0 = self.ar.hidden if carry else None
        want = (B, H) if self.L == 1 else (self.L, B, H)          # one state per layer of a stack
        if h0 is not None and (tuple(h0.shape) != want or h0.device != e.c.device):
            raise ValueError(f"carried GRU state has shape {tuple(h0.shape)} on {h0.device}, this call needs {want} on {e.c.device}")
        self.carried = h0 is not None
        h0 = None if h0 is None else h0.detach().float().contiguous().view(self.L, B, H)
        # the recurrences, bottom to top, each behind its batched input projection
        for l, lay in enumerate(self.layers):
            x, x_item, x_extent = self._input(l)
            _hip.gemm_nt(x, _hip.ptr(lay.w_ih), _hip.ptr(lay.Gi), B * V, 3 * H, lay.In, lay.In, lay.In, 3 * H, code,
                         bias=_hip.ptr(p.get(lay.prefix + "bias_ih")), a_rpi=V, a_item=x_item, a_extent=x_extent)
            c_out = e.c if l == self.L - 1 else self.c_low[l]
            args = (_hip.ptr(lay.Hall), _hip.ptr(lay.tape), _hip.ptr(c_out), B, V, H, code)
            if h0 is not None:
                _hip.call("cpc_gru_fwd_h0", _hip.ptr(lay.Gi), _hip.ptr(lay.w_hh_frag), _hip.ptr(p.get(lay.prefix + "bias_hh")),
                          _hip.ptr(h0[l]), *args)
            else:
                _hip.call("cpc_gru_fwd", _hip.ptr(lay.Gi), _hip.ptr(lay.w_hh_frag), _hip.ptr(p.get(lay.prefix + "bias_hh")), *args)
        if not carry:
            self.ar.hidden = None
        elif self.L == 1:
            self.ar.hidden = e.c.detach().clone()
        else:
            self.ar.hidden = torch.cat([self.c_low, e.c.detach().unsqueeze(0)], 0)

    def c_operand(self):
        """(tensor, element offset, item stride): storage-dtype rows of c, one per item (h_V inside the top layer's hidden-state buffer)."""
        return self.layers[-1].Hall, self.eng.V * self.H, (self.eng.V + 1) * self.H

    def c_float(self):
        return self.eng.c

    def backward(self, dc):
        e, H = self.eng, self.H
        code, B, V, E, K = e.code, e.B, e.V, e.E, e.K
        Ltop, t0, dtop = e.geo.alloc[-1], e.T - K - V, e.dact[-1]
        phase = e._gp_phase
        if getattr(self, "carried", False):
            raise RuntimeError("this GRU call started from a state carried over from the previous call (reset_hidden=False): it cannot be "
                               "differentiated -- the reference's autograd cannot either (the previous call's graph is gone after its "
                               "backward()); use reset_hidden=False for inference / streaming, or set model.hidden = None before a train step")
        if phase == 1:               # gradient penalty, pass 1: dc is the adjoint of the summed scores (gp_grads starts from it)
            self._gp_buffers()
            self.gp_dc1.copy_(dc)
        # Top layer from dc; then, layer by layer, dH = dG_l[:, :3H] W_ih_l (one row per (item, step): the layout cpc_gru_bwd_steps
        # reads) and the sweep of the layer below; layer 0's dG gives dz.  Each layer's parameter gradients (ten short launches, off the
        # critical path dG -> dz -> encoder backward) follow its dG on the side stream, in this order: they share one workspace, and the
        # encoder's gradient-ready hook runs on that stream behind all of them.
        for l in range(self.L - 1, -1, -1):
            lay = self.layers[l]
            if l == self.L - 1 and self.anchor_dHs is not None:          # prediction anchors: gradients at earlier states of the top layer
                _hip.call("cpc_gru_bwd_steps", _hip.ptr(dc), _hip.ptr(self.anchor_dHs), C.c_longlong(H), _hip.ptr(lay.tape),
                          _hip.ptr(lay.w_hh_t_frag), _hip.ptr(lay.dG), B, V, H, code)
            elif l == self.L - 1:
                _hip.call("cpc_gru_bwd", _hip.ptr(dc), _hip.ptr(lay.tape), _hip.ptr(lay.w_hh_t_frag), _hip.ptr(lay.dG), B, V, H, code)
            else:
                _hip.call("cpc_gru_bwd_steps", None, _hip.ptr(self.dH), C.c_longlong(H), _hip.ptr(lay.tape), _hip.ptr(lay.w_hh_t_frag),
                          _hip.ptr(lay.dG), B, V, H, code)
            with e.side(lay.ev):
                self._layer_params(l)
            if l > 0:
                _hip.gemm_nt(_hip.ptr(lay.dG), _hip.ptr(lay.w_ih_t), _hip.ptr(self.dH), B * V, H, 3 * H, 4 * H, 3 * H, H, code)
            else:            # dz -> rows [t0, t0+V) of the top-layer gradient
                _hip.gemm_nt(_hip.ptr(lay.dG), _hip.ptr(lay.w_ih_t), _hip.ptr(dtop, t0 * E), B * V, E, 3 * H, 4 * H, 3 * H, E, code,
                             c_rpi=V, c_item=Ltop * E, c_valid=V)
        if phase == 3:               # gradient penalty, pass 3: what z gains through the tangent recurrence's coefficients
            dtop.view(B, Ltop, E)[:, t0:t0 + V, :].add_(self.gp_dz.view(B, V, E))

    def _layer_params(self, l):
        """Parameter gradients of layer l from its dG (all steps) and its input rows, on the current stream."""
        e, H, lay = self.eng, self.H, self.layers[l]
        g, code, B, V, In = e.model._grad, e.code, e.B, e.V, lay.In
        x, x_item, _ = self._input(l)
        # dG[b][t] = [dr | du | dn | dn*r]: columns [0,3H) are the gradient of the input-projection term, columns [0,2H) and
        # [3H,4H) that of the recurrent term
        g_ih, g_hh = g[lay.prefix + "weight_ih"], g[lay.prefix + "weight_hh"]
        sl = self.scratch
        e._tn_to_grad(_hip.ptr(lay.dG), x, g_ih, B * V, 3 * H, In, 4 * H, In, lay.split_ih,
                      b_rpi=V, b_item=x_item, scratch=sl)
        e._tn_to_grad(_hip.ptr(lay.dG), _hip.ptr(lay.Hall), g_hh, B * V, 2 * H, H, 4 * H, H, lay.split_hh,
                      b_rpi=V, b_item=(V + 1) * H, scratch=sl)
        e._tn_to_grad(_hip.ptr(lay.dG, 3 * H), _hip.ptr(lay.Hall), g_hh, B * V, H, H, 4 * H, H, lay.split_hh,
                      b_rpi=V, b_item=(V + 1) * H, grad_offset=2 * H * H, scratch=sl)
        if (lay.prefix + "bias_ih") in g:
            g_bi, g_bh = g[lay.prefix + "bias_ih"], g[lay.prefix + "bias_hh"]
            M = B * V
            nb = min(e.colsum_blocks, max(1, M // 64))
            _hip.call("cpc_colsum", _hip.ptr(lay.dG), _hip.ptr(sl), M, 4 * H, 4 * H, nb, code)
            _hip.call("cpc_reduce_slabs", _hip.ptr(sl), _hip.ptr(g_bi), 1, 3 * H, nb, 4 * H, 1, 1, 0, 0)
            _hip.call("cpc_reduce_slabs", _hip.ptr(sl), _hip.ptr(g_bh), 1, 2 * H, nb, 4 * H, 1, 1, 0, 0)
            _hip.call("cpc_reduce_slabs", _hip.ptr(sl, 3 * H), _hip.ptr(g_bh, 2 * H), 1, H, nb, 4 * H, 1, 1, 0, 0)

    # ---- Wasserstein gradient penalty (scalogram_engine._gp_step; exact-f32 mode): tangent of c, penalty parts of the gradients.
    # Single layer only: everything below reads ``self.layers[0]``.
    GP_STACK_REASON = ("the gradient penalty through a stacked GRU (num_layers > 1) is not implemented: its reverse sweep "
                       "(cpc_gru_gp_bwd) differentiates ONE recurrence from the adjoint at its last state, and a lower layer of a "
                       "stack would need the second-order adjoints of every step handed down from the layer above")

    def _gp_buffers(self):
        if self.L > 1:
            raise NotImplementedError(self.GP_STACK_REASON)
        if getattr(self, "gp_tape", None) is not None:
            return
        e, H = self.eng, self.H
        B, V, E, dev = e.B, e.V, e.E, e.device
        if e.dt != torch.float32:
            raise NotImplementedError("the gradient penalty runs in the exact-f32 mode (compute_dtype='fp32')")
        f32 = dict(device=dev, dtype=torch.float32)
        self.gp_dc1 = torch.empty(B, H, **f32)
        self.gp_GiT = torch.empty(B * V * 3 * H, **f32)
        self.gp_whh_t = torch.empty(H * 3 * H, **f32)                 # [H][3H]
        self.gp_tape = torch.empty(B * V * 10 * H, **f32)
        self.gp_ct = torch.empty(B, H, **f32)
        self.gp_dA = torch.empty(B * V * 8 * H, **f32)
        self.gp_dz = torch.empty(B * V * E, **f32)
        self.gp_scratch = torch.empty(2 * self.slab_floats(), **f32)

    def tangent(self, top_t):
        """``top_t``: tangent of the encoder's top buffer; returns (tensor, offset, item stride) of the tangent of c.  Runs the
        primal and the tangent recurrence together (cpc_gru_gp_fwd) and keeps what gp_grads' reverse sweep reads."""
        e, H, lay = self.eng, self.H, self.layers[0]
        p, code, B, V, E, K = e.model._param, e.code, e.B, e.V, e.E, e.K
        Ltop, t0 = e.geo.alloc[-1], e.T - K - V
        self._gp_buffers()          # (raises for a stack, before any GPU work)
        _hip.gemm_nt(_hip.ptr(top_t, t0 * E), _hip.ptr(lay.w_ih), _hip.ptr(self.gp_GiT), B * V, 3 * H, E, E, E, 3 * H, code,
                     a_rpi=V, a_item=Ltop * E)
        _hip.call("cpc_cast2d", _hip.ptr(p[lay.prefix + "weight_hh"]), _hip.ptr(self.gp_whh_t), H, 3 * H, 1, H, code)
        _hip.call("cpc_gru_gp_fwd", _hip.ptr(lay.Gi), _hip.ptr(self.gp_GiT), _hip.ptr(self.gp_whh_t),
                  _hip.ptr(p[lay.prefix + "bias_hh"]), _hip.ptr(self.gp_tape), _hip.ptr(self.gp_ct), B, V, H)
        self._gp_top_t = top_t
        return self.gp_ct, 0, H

    def gp_grads(self, gp_grad):
        """Penalty parts of the GRU's parameter gradients and of dz.  With dA = [delta | nu] from cpc_gru_gp_bwd (delta: adjoints of
        the summed scores, nu: second-order adjoints): dW_ih = delta^T (tangent x) + nu^T x, dW_hh = delta'^T (tangent h) + nu'^T h,
        the biases take the column sums of nu, z takes nu W_ih (added to the top-layer gradient in pass 3)."""
        e, H, lay = self.eng, self.H, self.layers[0]
        p, code, B, V, E, K = e.model._param, e.code, e.B, e.V, e.E, e.K
        Ltop, t0, top, top_t = e.geo.alloc[-1], e.T - K - V, e.act[-1], self._gp_top_t
        if (lay.prefix + "bias_hh") not in p:
            raise NotImplementedError("gradient penalty through a GRU without biases")
        _hip.call("cpc_gru_gp_bwd", _hip.ptr(self.gp_dc1), _hip.ptr(self.gp_tape), _hip.ptr(p[lay.prefix + "weight_hh"]),
                  _hip.ptr(self.gp_dA), B, V, H)
        dA, tape, sl = self.gp_dA, self.gp_tape, self.gp_scratch
        M = B * V

        def pair(grad, I, J, nsplit, first, second, grad_offset=0):
            # grad = first product + second product: both into f32 slabs, one fixed-order reduction over all of them
            chunk = e._chunk(M, nsplit)
            for idx, (a_off, b_ptr, ldb, kw) in enumerate((first, second)):
                _hip.gemm_tn(_hip.ptr(dA, a_off), b_ptr, _hip.ptr(sl, idx * nsplit * I * J), M, I, J, 8 * H, ldb, J, code, nsplit=nsplit,
                             m_chunk=chunk, slab_stride=I * J, flags=_hip.GEMM_OUT_F32, **kw)
            _hip.call("cpc_reduce_slabs", _hip.ptr(sl), _hip.ptr(grad, grad_offset), I, J, 2 * nsplit, I * J, 1, 1, J, 0)

        rows = dict(b_rpi=V, b_item=Ltop * E)
        g_ih, g_hh = gp_grad[lay.prefix + "weight_ih"], gp_grad[lay.prefix + "weight_hh"]
        pair(g_ih, 3 * H, E, lay.split_ih, (0, _hip.ptr(top_t, t0 * E), E, rows), (4 * H, _hip.ptr(top, t0 * E), E, rows))
        ht_prev, h_prev = _hip.ptr(tape, 9 * H), _hip.ptr(tape, 4 * H)
        pair(g_hh, 2 * H, H, lay.split_hh, (0, ht_prev, 10 * H, {}), (4 * H, h_prev, 10 * H, {}))
        pair(g_hh, H, H, lay.split_hh, (3 * H, ht_prev, 10 * H, {}), (7 * H, h_prev, 10 * H, {}), grad_offset=2 * H * H)
        nb = min(e.colsum_blocks, max(1, M // 64))
        _hip.call("cpc_colsum", _hip.ptr(dA), _hip.ptr(sl), M, 8 * H, 8 * H, nb, code)
        g_bi, g_bh = gp_grad[lay.prefix + "bias_ih"], gp_grad[lay.prefix + "bias_hh"]
        _hip.call("cpc_reduce_slabs", _hip.ptr(sl, 4 * H), _hip.ptr(g_bi), 1, 3 * H, nb, 8 * H, 1, 1, 0, 0)
        _hip.call("cpc_reduce_slabs", _hip.ptr(sl, 4 * H), _hip.ptr(g_bh), 1, 2 * H, nb, 8 * H, 1, 1, 0, 0)
        _hip.call("cpc_reduce_slabs", _hip.ptr(sl, 7 * H), _hip.ptr(g_bh, 2 * H), 1, H, nb, 8 * H, 1, 1, 0, 0)
        _hip.gemm_nt(_hip.ptr(dA, 4 * H), _hip.ptr(lay.w_ih_t), _hip.ptr(self.gp_dz), M, E, 3 * H, 8 * H, 3 * H, E, code)


class LSTMContext(Context):
    """AudioLSTMModel as the context network (nn.LSTMCell stepped over the V frames; DESIGN.md "LSTM context"): one batched
    input-projection GEMM for all V steps, the persistent LSTM kernels (csrc/lstm.hip) for the recurrence, GEMMs for the weight
    gradients and for dz.  dG[b][t] = [di | df | dg | do] is the gradient of the input-projection term and of the recurrent term alike,
    so every parameter gradient is one product over all 4H columns.  Single layer; no gradient penalty (``tangent`` / ``gp_grads`` keep
    the base class's refusal)."""

    ahead_ok = True       # prepare_weights is a pure function of the parameters (CPCEngine.prepare_ahead)
    anchors_ok = True
    prefix = "autoregressive_model.lstmCell."

    def __init__(self, eng, ar):
        self.eng = eng
        self.ar = ar
        self.H = int(ar.hidden_size)
        ch = 8 if eng.dt == torch.bfloat16 else 4
        if ar.input_size != eng.E or self.H != eng.H:
            raise ValueError("AudioLSTMModel sizes do not match enc_size / ar_size")
        if self.H < 1 or self.H % (4 * ch) or self.H > 512:
            raise NotImplementedError(f"HIP LSTM kernel: hidden size must be <= 512 and a multiple of 32 in bf16, of 16 in float32 "
                                      f"(this engine: {'bf16' if ch == 8 else 'float32'}, hidden size {self.H})")
        if eng.gp_capable:
            raise NotImplementedError(self.GP_REASON)

    GP_REASON = ("the gradient penalty through an AudioLSTMModel is not implemented: there is no tangent recurrence and no "
                 "second-order reverse sweep for the LSTM kernels (AudioGRUModel, AttentionModel and ConvolutionalArModel have them)")

    def allocate(self):
        e = self.eng
        B, V, H, In, dev, dt = e.B, e.V, self.H, e.E, e.device, e.dt
        tape = max(1, int(_hip.lib().cpc_lstm_tape_elems(B, max(V, 1), H, e.code)))
        self.w_ih = torch.empty(4 * H * In, device=dev, dtype=dt)          # [4H][In]
        self.w_ih_t = torch.empty(In * 4 * H, device=dev, dtype=dt)        # [In][4H]
        self.w_hh_frag = torch.empty(4 * H * H, device=dev, dtype=dt)
        self.w_hh_t_frag = torch.empty(4 * H * H, device=dev, dtype=dt)
        self.Gi = torch.empty(B * V * 4 * H, device=dev, dtype=dt)
        self.Hall = torch.empty(B * (V + 1) * H, device=dev, dtype=dt)
        self.tape = torch.zeros(tape, device=dev, dtype=dt)
        self.dG = torch.empty(B * V * 4 * H, device=dev, dtype=dt)         # [di | df | dg | do] per (item, step)
        self.cell = torch.empty(B, H, device=dev, dtype=torch.float32)     # last cell state
        self.split_ih = e._pick_split(4 * H, In, B * V)
        self.split_hh = e._pick_split(4 * H, H, B * V)
        self.ev = torch.cuda.Event()
        self.scratch = torch.empty(self.slab_floats(), device=dev, dtype=torch.float32)     # side-stream workspace

    def slab_floats(self):
        e, H = self.eng, self.H
        return max(e.colsum_blocks * 4 * H, self.split_ih * 4 * H * e.E, self.split_hh * 4 * H * H)

    def prepare_weights(self):
        H, In, code = self.H, self.eng.E, self.eng.code
        p = self.eng.model._param
        w_ih, w_hh = p[self.prefix + "weight_ih"], p[self.prefix + "weight_hh"]
        _hip.call("cpc_cast2d", _hip.ptr(w_ih), _hip.ptr(self.w_ih), 4 * H, In, In, 1, code)
        _hip.call("cpc_cast2d", _hip.ptr(w_ih), _hip.ptr(self.w_ih_t), In, 4 * H, 1, In, code)
        _hip.call("cpc_prep_frag", _hip.ptr(w_hh), _hip.ptr(self.w_hh_frag), 4 * H, H, H, 0, code)
        _hip.call("cpc_prep_frag", _hip.ptr(w_hh), _hip.ptr(self.w_hh_t_frag), H, 4 * H, H, 1, code)

    def _input(self):
        """The frames [T-K-V, T-K) of the encoder's top buffer: (pointer, item stride in elements)."""
        e = self.eng
        return _hip.ptr(e.act[-1], (e.T - e.K - e.V) * e.E), e.geo.alloc[-1] * e.E

    def forward(self):
        e, H = self.eng, self.H
        p, code, B, V, In = e.model._param, e.code, e.B, e.V, e.E
        # reset_hidden=False: the last (h, cell) of the previous call is this call's initial pair
        carry = not getattr(self.ar, "reset_hidden", True)
        pair = self.ar.hidden if carry else None
        if pair is not None:
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError("carried LSTM state must be a pair (h, cell) of (batch, hidden) tensors")
            for s in pair:
                if tuple(s.shape) != (B, H) or s.device != e.c.device:
                    raise ValueError(f"carried LSTM state has shape {tuple(s.shape)} on {s.device}, this call needs {(B, H)} on {e.c.device}")
            pair = tuple(s.detach().float().contiguous() for s in pair)
        self.carried = pair is not None
        x, x_item = self._input()
        _hip.gemm_nt(x, _hip.ptr(self.w_ih), _hip.ptr(self.Gi), B * V, 4 * H, In, In, In, 4 * H, code,
                     bias=_hip.ptr(p.get(self.prefix + "bias_ih")), a_rpi=V, a_item=x_item)
        _hip.call("cpc_lstm_fwd", _hip.ptr(self.Gi), _hip.ptr(self.w_hh_frag), _hip.ptr(p.get(self.prefix + "bias_hh")),
                  _hip.ptr(pair[0]) if pair else None, _hip.ptr(pair[1]) if pair else None, _hip.ptr(self.Hall), _hip.ptr(self.tape),
                  _hip.ptr(e.c), _hip.ptr(self.cell), B, V, H, code)
        self.ar.hidden = (e.c.detach().clone(), self.cell.clone()) if carry else None

    def c_operand(self):
        """(tensor, element offset, item stride): storage-dtype rows of c, one per item (h_V inside the hidden-state buffer)."""
        return self.Hall, self.eng.V * self.H, (self.eng.V + 1) * self.H

    def c_float(self):
        return self.eng.c

    def backward(self, dc):
        e, H = self.eng, self.H
        code, B, V, E, K = e.code, e.B, e.V, e.E, e.K
        Ltop, t0, dtop = e.geo.alloc[-1], e.T - K - V, e.dact[-1]
        if getattr(self, "carried", False):
            raise RuntimeError("this LSTM call started from a pair (h, cell) carried over from the previous call (reset_hidden=False): it "
                               "cannot be differentiated -- autograd could not either (the previous call's graph is gone after its "
                               "backward()); use reset_hidden=False for inference / streaming, or set model.hidden = None before a train step")
        if e._gp_phase:
            raise NotImplementedError(self.GP_REASON)
        if self.anchor_dHs is not None:          # prediction anchors: gradients at earlier hidden states
            _hip.call("cpc_lstm_bwd_steps", _hip.ptr(dc), _hip.ptr(self.anchor_dHs), C.c_longlong(H), _hip.ptr(self.tape),
                      _hip.ptr(self.w_hh_t_frag), _hip.ptr(self.dG), B, V, H, code)
        else:
            _hip.call("cpc_lstm_bwd", _hip.ptr(dc), _hip.ptr(self.tape), _hip.ptr(self.w_hh_t_frag), _hip.ptr(self.dG), B, V, H, code)
        # the parameter gradients (short launches, off the critical path dG -> dz -> encoder backward) follow dG on the side stream
        with e.side(self.ev):
            self._params()
        # dz -> rows [t0, t0+V) of the top-layer gradient
        _hip.gemm_nt(_hip.ptr(self.dG), _hip.ptr(self.w_ih_t), _hip.ptr(dtop, t0 * E), B * V, E, 4 * H, 4 * H, 4 * H, E, code,
                     c_rpi=V, c_item=Ltop * E, c_valid=V)

    def _params(self):
        """Parameter gradients from dG (all steps), the frames and the hidden states h_0 .. h_{V-1}, on the current stream."""
        e, H = self.eng, self.H
        g, code, B, V, In = e.model._grad, e.code, e.B, e.V, e.E
        x, x_item = self._input()
        sl = self.scratch
        e._tn_to_grad(_hip.ptr(self.dG), x, g[self.prefix + "weight_ih"], B * V, 4 * H, In, 4 * H, In, self.split_ih,
                      b_rpi=V, b_item=x_item, scratch=sl)
        e._tn_to_grad(_hip.ptr(self.dG), _hip.ptr(self.Hall), g[self.prefix + "weight_hh"], B * V, 4 * H, H, 4 * H, H, self.split_hh,
                      b_rpi=V, b_item=(V + 1) * H, scratch=sl)
        if (self.prefix + "bias_ih") in g:
            M = B * V
            nb = min(e.colsum_blocks, max(1, M // 64))
            _hip.call("cpc_colsum", _hip.ptr(self.dG), _hip.ptr(sl), M, 4 * H, 4 * H, nb, code)
            _hip.call("cpc_reduce_slabs", _hip.ptr(sl), _hip.ptr(g[self.prefix + "bias_ih"]), 1, 4 * H, nb, 4 * H, 1, 1, 0, 0)
            _hip.call("cpc_reduce_slabs", _hip.ptr(sl), _hip.ptr(g[self.prefix + "bias_hh"]), 1, 4 * H, nb, 4 * H, 1, 1, 0, 0)


class ConvArContext(Context):
    """ConvolutionalArModel as the context network (audio_model.py:80-161) for the plain configuration (no batch norm, no
    residual branch; e.g. ``ar_conv_default_dict``): per block [MaxPool1d(pool, ceil)] -> Conv1d(k, stride 1) -> ReLU on
    channels-last buffers; the convolutions are the same overlapped-row GEMMs as the encoder's; c = the last position."""

    ahead_ok = True       # prepare_weights is a pure function of the parameters (CPCEngine.prepare_ahead)

    def __init__(self, eng, ar):
        self.eng = eng
        self.kernels = list(ar.kernel_sizes)
        self.strides = list(ar.strides)
        self.pools = list(ar.poolings)
        self.channels = list(ar.channel_count)
        self.nb = len(self.kernels)
        if ar.batch_norm or ar.residual:
            raise NotImplementedError("ConvArContext is the lean path for plain configurations; make_context() routes batch_norm / residual to ConvArGridContext")
        if any(s != 1 for s in self.strides):
            raise NotImplementedError("ConvArContext handles stride-1 convolutions; make_context() routes strided ones to ConvArGridContext")
        if self.channels[0] != eng.E or self.channels[-1] != eng.H:
            raise ValueError("ConvolutionalArModel channel_count does not match enc_size / ar_size")
        ch = 8 if eng.dt == torch.bfloat16 else 4
        if any(c % 8 for c in self.channels) or any((k * c) % ch for k, c in zip(self.kernels, self.channels)):
            raise NotImplementedError("ConvolutionalArModel channel counts must be multiples of 8")
        # lengths: pooled input and conv output of every block
        self.lp, self.lo = [], []
        cur = eng.V
        for l in range(self.nb):
            cur = _ceil_div(cur, self.pools[l])
            self.lp.append(cur)
            cur = cur - self.kernels[l] + 1
            if cur <= 0:
                raise ValueError("visible_steps too short for this ConvolutionalArModel")
            self.lo.append(cur)
        # padded row counts per item: the conv input buffer of block l and its output share one value (stride 1) and keep
        # >= kernel-1 zero pad rows, which is what the overlapped-row data-gradient GEMM needs between items
        self.la = [max(self.lp[l], self.lo[l]) + self.kernels[l] for l in range(self.nb)]
        self.conv_idx = [1 if self.pools[l] > 1 else 0 for l in range(self.nb)]

    def _name(self, l, what):
        return f"autoregressive_model.module_list.{l}.main_modules.{self.conv_idx[l]}.{what}"

    def allocate(self):
        e = self.eng
        B, dev, dt = e.B, e.device, e.dt
        self.x, self.dx, self.y, self.dy, self.w_fwd, self.w_dgrad, self.nsplit = [], [], [], [], [], [], []
        self._keep = []
        for l in range(self.nb):
            cin, cout, kw = self.channels[l], self.channels[l + 1], self.kernels[l]
            for store, cols in ((self.x, cin), (self.dx, cin), (self.y, cout), (self.dy, cout)):
                if l == 0 and self.pools[0] == 1 and store in (self.x, self.dx):
                    store.append(None)        # block 0 without pooling reads z straight out of the encoder's top buffer
                    continue
                full, view, _ = e._buf(B * self.la[l], cols, max(self.kernels))
                self._keep.append(full)
                store.append(view)
            self.w_fwd.append(torch.empty(cout * kw * cin, device=dev, dtype=dt))
            self.w_dgrad.append(torch.empty(cin * kw * cout, device=dev, dtype=dt))
            self.nsplit.append(e._pick_split(kw * cin, cout, B * self.la[l]))
        self.c32 = torch.empty(B, self.channels[-1], device=dev, dtype=torch.float32)
        # side-stream reductions: per-layer weight-gradient slabs, one bias scratch, events
        self.wslab = [torch.empty(self.nsplit[l] * self.kernels[l] * self.channels[l] * self.channels[l + 1], device=dev, dtype=torch.float32)
                      for l in range(self.nb)]
        self.bscratch = torch.empty(e.colsum_blocks * max(self.channels), device=dev, dtype=torch.float32)
        self._ev = [(torch.cuda.Event(), torch.cuda.Event()) for _ in range(self.nb)]

    def slab_floats(self):
        return max(self.nsplit[l] * self.kernels[l] * self.channels[l] * self.channels[l + 1] for l in range(self.nb)) + \
            self.eng.colsum_blocks * max(self.channels)

    def prepare_weights(self):
        e = self.eng
        p, code = e.model._param, e.code
        for l in range(self.nb):
            _hip.call("cpc_conv_w_prep", _hip.ptr(p[self._name(l, "weight")]), _hip.ptr(self.w_fwd[l]), _hip.ptr(self.w_dgrad[l]),
                      self.channels[l + 1], self.channels[l], self.kernels[l], 1, code)

    def _block_input(self, l):
        """(pointer to the conv input rows of block l, a_rpi, a_item) — block 0 without pooling reads the encoder output."""
        e = self.eng
        if self.x[l] is None:
            t0 = e.T - e.K - e.V
            return _hip.ptr(e.act[-1], t0 * e.E), self.la[0], e.geo.alloc[-1] * e.E
        return _hip.ptr(self.x[l]), 0, 0

    def forward(self):
        e = self.eng
        p, code, B = e.model._param, e.code, e.B
        for l in range(self.nb):
            cin, cout, kw, la = self.channels[l], self.channels[l + 1], self.kernels[l], self.la[l]
            if self.pools[l] > 1:
                if l == 0:
                    t0 = e.T - e.K - e.V
                    raise NotImplementedError("ConvArContext: no pooling in the first block (make_context() routes that to ConvArGridContext)")
                _hip.call("cpc_maxpool_fwd", _hip.ptr(self.y[l - 1]), _hip.ptr(self.x[l]), B, cin, self.pools[l], self.lo[l - 1],
                          self.la[l - 1], self.lp[l], la, code)
            elif l > 0:
                raise NotImplementedError("ConvArContext: pooling in every later block (make_context() routes other layouts to ConvArGridContext)")
            a, a_rpi, a_item = self._block_input(l)
            _hip.gemm_nt(a, _hip.ptr(self.w_fwd[l]), _hip.ptr(self.y[l]), B * la, cout, kw * cin, cin, kw * cin, cout, code,
                         bias=_hip.ptr(p.get(self._name(l, "bias"))), a_rpi=a_rpi, a_item=a_item, c_rpi=la, c_item=la * cout,
                         c_valid=self.lo[l], flags=_hip.GEMM_RELU)

    def c_operand(self):
        l = self.nb - 1
        return self.y[l], (self.lo[l] - 1) * self.channels[-1], self.la[l] * self.channels[-1]

    def c_float(self):
        l = self.nb - 1
        H = self.channels[-1]
        self.c32.copy_(self.y[l].view(self.eng.B, self.la[l], H)[:, self.lo[l] - 1, :])
        return self.c32

    def backward(self, dc):
        e = self.eng
        g, code, B = e.model._grad, e.code, e.B
        last = self.nb - 1
        H = self.channels[-1]
        # gradient enters at the single position forward() returns; everything else of dy[last] stays zero
        _hip.call("cpc_relu_row_bwd", _hip.ptr(dc), _hip.ptr(self.y[last]), _hip.ptr(self.dy[last]), B, H, self.la[last] * H,
                  (self.lo[last] - 1) * H, code)
        for l in range(last, -1, -1):
            cin, cout, kw, la = self.channels[l], self.channels[l + 1], self.kernels[l], self.la[l]
            bname = self._name(l, "bias")
            if bname in g:
                with e.side(self._ev[l][0]):
                    e._colsum_to_grad(_hip.ptr(self.dy[l]), g[bname], B * la, cout, scratch=self.bscratch)
            a, a_rpi, a_item = self._block_input(l)
            chunk = e._chunk(B * la, self.nsplit[l])
            # The weight-gradient GEMM stays on the main stream (on the high-priority side stream it takes the CUs from the short
            # data-gradient chain it runs beside: measured 3.9 -> 5.3 ms per step); only the short reductions go to the side stream.
            _hip.gemm_tn(a, _hip.ptr(self.dy[l]), _hip.ptr(self.wslab[l]), B * la, kw * cin, cout, cin, cout, cout, code, a_rpi=a_rpi,
                         a_item=a_item, nsplit=self.nsplit[l], m_chunk=chunk, slab_stride=kw * cin * cout, flags=_hip.GEMM_OUT_F32)
            with e.side(self._ev[l][1]):
                _hip.call("cpc_reduce_conv_w", _hip.ptr(self.wslab[l]), _hip.ptr(g[self._name(l, "weight")]), cin, cout, kw,
                          self.nsplit[l], kw * cin * cout)
            D = kw                                   # stride 1: every input position is touched by kw output rows
            dy_shift = _hip.ptr(self.dy[l], -(D - 1) * cout)
            if self.x[l] is None:
                # data gradient straight into rows [t0, t0+V) of the encoder's top-layer gradient (no ReLU on that layer)
                t0 = e.T - e.K - e.V
                _hip.gemm_nt(dy_shift, _hip.ptr(self.w_dgrad[l]), _hip.ptr(e.dact[-1], t0 * e.E), B * la, cin, D * cout, cout,
                             D * cout, cin, code, c_rpi=la, c_item=e.geo.alloc[-1] * e.E, c_valid=e.V, flags=_hip.GEMM_SKIP_PAD_ROWS)
            else:
                _hip.gemm_nt(dy_shift, _hip.ptr(self.w_dgrad[l]), _hip.ptr(self.dx[l]), B * la, cin, D * cout, cout, D * cout, cin,
                             code, mask=_hip.ptr(self.x[l]), c_rpi=la, c_item=la * cin, c_valid=self.lp[l])
                _hip.call("cpc_maxpool_bwd", _hip.ptr(self.y[l - 1]), _hip.ptr(self.dx[l]), _hip.ptr(self.dy[l - 1]), B, cin,
                          self.pools[l], self.lo[l - 1], self.la[l - 1], la, code)


class AttentionContext(Context):
    """AttentionModel as the context network (attention_model.py:38-82): positional encoding, ``num_layers`` post-norm
    transformer encoder layers with a causal mask (transformer.py:262-271), a final LayerNorm, the mean over time and
    ``end_layer``.  Rows are (item, step) with C channels; every Linear is a cpc_gemm_nt / cpc_gemm_tn call, the
    per-(item, head) attention, the residual + LayerNorm and the mean are the kernels of csrc/attn.hip.
    Dropout (train mode, p > 0) uses counter-based masks that the backward regenerates (include/cpc_hip.h, cpc_dropout):
    same distribution as the reference's nn.Dropout, not its random stream."""

    LN_EPS = 1e-5
    SITE_ATTN, SITE_DROP1, SITE_FF, SITE_DROP2 = 0, 1, 2, 3       # dropout sites of layer l: 4*l + ...

    def __init__(self, eng, ar):
        self.eng = eng
        self.C, self.N, self.heads, self.FF = ar.channels, ar.num_layers, ar.num_heads, ar.feedforward_size
        self.out = ar.output_size
        self.S = eng.V
        self.ar = ar
        if self.C != eng.E or self.out != eng.H:
            raise ValueError("AttentionModel channels / output_size do not match enc_size / ar_size")
        if self.S > ar.sequence_length:
            raise ValueError("visible_steps exceeds the AttentionModel's sequence_length (positional table)")
        if self.S > 128 or self.C % self.heads or self.C // self.heads > 64:
            raise NotImplementedError("HIP attention kernels: visible_steps <= 128 and head size <= 64")
        # the attention core: the short-sequence kernels up to 64 steps, the cpc_attn128_* ones beyond
        self.attn_abi = "cpc_attn" if self.S <= 64 else "cpc_attn128"
        ch = 8 if eng.dt == torch.bfloat16 else 4
        if self.C % 8 or self.FF % 8 or self.out % ch or self.C > 2048:
            raise NotImplementedError("AttentionModel sizes must be multiples of 8 (channels <= 2048)")
        self.z_scale = math.sqrt(self.C)
        self.prefix = "autoregressive_model."
        self.drop_p, self.drop_seed, self._drop_counter, self._l2_scale = 0.0, 0, 0, 1.0
        self.fixed_seed = None          # tests pin the mask seed here

    def _lname(self, l, what):
        return f"{self.prefix}encoder.layers.{l}.{what}"

    def allocate(self):
        e = self.eng
        B, dev, dt, f32 = e.B, e.device, e.dt, torch.float32
        C, FF, S, N, H = self.C, self.FF, self.S, self.N, self.out
        M = B * S
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=dt)
        self.pe = self.ar.positional_encoder.pe[:S, 0, :].detach().to(device=dev, dtype=f32).contiguous()
        self.X = [new(M * C) for _ in range(N + 1)]
        self.qkv = [new(M * 3 * C) for _ in range(N)]
        self.P = [new(B * self.heads * S * S) for _ in range(N)]
        self.att = [new(M * C) for _ in range(N)]
        self.r1 = [new(M * C) for _ in range(N)]
        self.x1 = [new(M * C) for _ in range(N)]
        self.f1 = [new(M * FF) for _ in range(N)]
        self.r2 = [new(M * C) for _ in range(N)]
        self.st1 = [torch.empty(M * 2, device=dev, dtype=f32) for _ in range(N)]
        self.st2 = [torch.empty(M * 2, device=dev, dtype=f32) for _ in range(N)]
        self.stn = torch.empty(M * 2, device=dev, dtype=f32)
        self.ytmp, self.xn = new(M * C), new(M * C)
        self.mean, self.dmean = new(B * C), new(B * C)
        self.c32 = torch.empty(B, H, device=dev, dtype=f32)
        self.ct = self.c32 if dt == f32 else new(B * H)
        self.dct = new(B * H)
        # gradient scratch
        # Gradient buffers that the parameter-gradient kernels read exist twice (layer parity): those kernels run on the side
        # stream while the main stream already differentiates the next layer down, which writes the other set.
        self.gA, self.gB = [new(M * C), new(M * C)], [new(M * C), new(M * C)]
        self.gC, self.gD = new(M * C), new(M * C)
        self.gAd, self.gBd = [new(M * C), new(M * C)], [new(M * C), new(M * C)]   # dropped-out summands (dropout only)
        self.dqkv, self.df1, self.datt = [new(M * 3 * C), new(M * 3 * C)], [new(M * FF), new(M * FF)], new(M * C)
        self.scratch = None
        self._cast_jobs = None
        self._ev = [[torch.cuda.Event() for _ in range(5)] for _ in range(self.N + 1)]
        # weight operands in the storage dtype: [out][in] for the forward GEMMs, [in][out] for the data gradients
        shapes = {"in": (3 * C, C), "o": (C, C), "l1": (FF, C), "l2": (C, FF)}
        self.w = [{k: new(r * c) for k, (r, c) in shapes.items()} for _ in range(N)]
        self.wt = [{k: new(r * c) for k, (r, c) in shapes.items()} for _ in range(N)]
        self.w_end, self.w_end_t = new(H * C), new(C * H)
        # LayerNorm backward: a wave walks its rows one at a time (load -> two wave reductions -> store), so the row loop is latency-
        # bound; 512 workgroups = 2 waves per SIMD overlap the rows (attention_architecture_1 at B = 256: 5.60 ms per step with 256 workgroups, 5.45 with 512 or 1024, 5.57 with 2048)
        self.ln_blocks = max(1, min(512, M // 4))
        self.split = {k: e._pick_split(r, c, M) for k, (r, c) in shapes.items()}

    def slab_floats(self):
        C, FF = self.C, self.FF
        shapes = {"in": 3 * C * C, "o": C * C, "l1": FF * C, "l2": C * FF}
        return max([self.split[k] * n for k, n in shapes.items()] + [self.ln_blocks * 2 * C,
                                                                     self.eng.colsum_blocks * max(3 * C, FF)])

    _WNAMES = {"in": "self_attn.in_proj_weight", "o": "self_attn.out_proj.weight", "l1": "linear1.weight", "l2": "linear2.weight"}
    _BNAMES = {"in": "self_attn.in_proj_bias", "o": "self_attn.out_proj.bias", "l1": "linear1.bias", "l2": "linear2.bias"}

    def prepare_weights(self):
        e = self.eng
        p, code, C, FF, H = e.model._param, e.code, self.C, self.FF, self.out
        shapes = {"in": (3 * C, C), "o": (C, C), "l1": (FF, C), "l2": (C, FF)}
        if self._cast_jobs is None or self._cast_jobs[1] is not e.model._flat_param:
            # all operand-layout copies (weight and transposed weight of every Linear) as one batched launch; the job table holds
            # raw addresses, which are stable: parameters are views of the model's flat buffer
            jobs = []
            for l in range(self.N):
                for k, (r, c) in shapes.items():
                    src = p[self._lname(l, self._WNAMES[k])].data_ptr()
                    jobs.append((src, self.w[l][k].data_ptr(), r, c, c, 1))
                    jobs.append((src, self.wt[l][k].data_ptr(), c, r, 1, c))
            src = p[self.prefix + "end_layer.weight"].data_ptr()
            jobs.append((src, self.w_end.data_ptr(), H, C, C, 1))
            jobs.append((src, self.w_end_t.data_ptr(), C, H, 1, C))
            self._cast_jobs = (torch.tensor(jobs, dtype=torch.int64, device=e.device), e.model._flat_param, len(jobs))
        _hip.call("cpc_cast2d_batch", _hip.ptr(self._cast_jobs[0]), self._cast_jobs[2], code)
        self._l2_scale = 1.0

    ahead_ok = True       # prepare_weights is a pure function of the parameters (CPCEngine.prepare_ahead); the dropout state is drawn in forward()

    def _begin_forward(self):
        """Dropout state of this forward pass (train mode, p > 0): a fresh mask seed, and the 1 / (1 - p) of the feed-forward dropout folded
        into the operand of the feed-forward data-gradient GEMM (d relu(.) dropout = keep / (1 - p): the keep part comes with the ReLU
        mask of the stored, dropped activation)."""
        dp = float(self.ar.dropout) if (self.ar.training and self.ar.dropout > 0.0) else 0.0
        if dp > 0.0:
            if not dp < 1.0:
                raise ValueError("dropout probability must be < 1")
            self._drop_counter += 1
            base = torch.initial_seed() if self.fixed_seed is None else int(self.fixed_seed)
            self.drop_seed = (base * 0x9E3779B1 + (0 if self.fixed_seed is not None else self._drop_counter)) & 0x7FFFFFFFFFFFFFFF
        want = 1.0 / (1.0 - dp) if dp > 0.0 else 1.0
        if want != self._l2_scale:
            if self._l2_scale != 1.0:          # (train <-> eval without a parameter update in between: rebuild rather than rescale twice)
                self.prepare_weights()
            if want != 1.0:
                for l in range(self.N):
                    self.wt[l]["l2"].mul_(want)
            self._l2_scale = want
        self.drop_p = dp

    def _ln(self, a, b, wname, r_out, y, stats, site=None):
        p = self.eng.model._param
        dp = self.drop_p if site is not None else 0.0
        _hip.call("cpc_add_ln_fwd", _hip.ptr(a), _hip.ptr(b), _hip.ptr(p[wname + ".weight"]), _hip.ptr(p[wname + ".bias"]),
                  _hip.ptr(r_out), _hip.ptr(y), _hip.ptr(stats), self.eng.B * self.S, self.C, self.LN_EPS, dp, self.drop_seed,
                  site or 0, self.eng.code)

    def forward(self):
        e = self.eng
        p, code, B = e.model._param, e.code, e.B
        C, FF, S, H = self.C, self.FF, self.S, self.out
        M = B * S
        Ltop, t0 = e.geo.alloc[-1], e.T - e.K - e.V
        P = _hip.ptr
        self._begin_forward()
        dp, seed = self.drop_p, self.drop_seed
        _hip.call("cpc_pe_scale_fwd", P(e.act[-1], t0 * C), P(self.pe), P(self.X[0]), B, S, C, Ltop * C, self.z_scale, code)
        for l in range(self.N):
            X, w = self.X[l], self.w[l]
            bias = {k: P(p[self._lname(l, n)]) for k, n in self._BNAMES.items()}
            _hip.gemm_nt(P(X), P(w["in"]), P(self.qkv[l]), M, 3 * C, C, C, C, 3 * C, code, bias=bias["in"])
            _hip.call(self.attn_abi + "_fwd", P(self.qkv[l]), P(self.att[l]), P(self.P[l]), B, S, C, self.heads, dp, seed, 4 * l + self.SITE_ATTN,
                      code)
            _hip.gemm_nt(P(self.att[l]), P(w["o"]), P(self.ytmp), M, C, C, C, C, C, code, bias=bias["o"])
            self._ln(X, self.ytmp, self._lname(l, "norm1"), self.r1[l], self.x1[l], self.st1[l], site=4 * l + self.SITE_DROP1)
            _hip.gemm_nt(P(self.x1[l]), P(w["l1"]), P(self.f1[l]), M, FF, C, C, C, FF, code, bias=bias["l1"], flags=_hip.GEMM_RELU)
            if dp > 0.0:
                _hip.call("cpc_dropout", P(self.f1[l]), M * FF, dp, seed, 4 * l + self.SITE_FF, code)
            _hip.gemm_nt(P(self.f1[l]), P(w["l2"]), P(self.ytmp), M, C, FF, FF, FF, C, code, bias=bias["l2"])
            self._ln(self.x1[l], self.ytmp, self._lname(l, "norm2"), self.r2[l], self.X[l + 1], self.st2[l], site=4 * l + self.SITE_DROP2)
        self._ln(self.X[self.N], None, self.prefix + "encoder.norm", None, self.xn, self.stn)
        _hip.call("cpc_mean_time", P(self.xn), P(self.mean), B, S, C, code)
        b_end = P(p[self.prefix + "end_layer.bias"])
        _hip.gemm_nt(P(self.mean), P(self.w_end), P(self.c32), B, H, C, C, C, H, code, bias=b_end, flags=_hip.GEMM_OUT_F32)
        if self.ct is not self.c32:
            _hip.gemm_nt(P(self.mean), P(self.w_end), P(self.ct), B, H, C, C, C, H, code, bias=b_end)

    def c_operand(self):
        return self.ct, 0, self.out

    def c_float(self):
        return self.c32

    def _ln_bwd(self, g1, g2, r, stats, wname, dr, bcast=0, gscale=1.0, dr_b=None, site=0):
        e, C = self.eng, self.C
        g, p = e.model._grad, e.model._param
        nb = self.ln_blocks
        _hip.call("cpc_ln_bwd", _hip.ptr(g1), _hip.ptr(g2), _hip.ptr(r), _hip.ptr(stats), _hip.ptr(p[wname + ".weight"]),
                  _hip.ptr(dr), _hip.ptr(e.slabs), e.B * self.S, C, bcast, gscale, nb, _hip.ptr(dr_b),
                  self.drop_p if dr_b is not None else 0.0, self.drop_seed, site, e.code)
        _hip.call("cpc_reduce_slabs", _hip.ptr(e.slabs), _hip.ptr(g[wname + ".weight"]), 1, C, nb, 2 * C, 1, 1, 0, 0)
        _hip.call("cpc_reduce_slabs", _hip.ptr(e.slabs, C), _hip.ptr(g[wname + ".bias"]), 1, C, nb, 2 * C, 1, 1, 0, 0)

    # ---- Wasserstein gradient penalty (scalogram_engine._gp_step; exact-f32 mode).  The context is not piecewise linear, so the
    # penalty's gradient is the reverse sweep of the JOINT (primal, tangent) program: tangent() runs the tangent pass and keeps the
    # tangent of every Linear's input; the last pass (_backward_gp) carries two adjoints down the layers — lambda, the real loss's
    # (the ordinary backward, which also takes the second-order terms of LayerNorm and of the attention core on the way:
    # cpc_ln_gp, cpc_attn_gp), and delta, the summed scores' (pass 1 again, seeded with the dc kept from it), whose products with the
    # tangent inputs are the penalty parts of the weight gradients.  tools/gp_attention_algebra.py checks the algebra on the CPU.
    def _gp_buffers(self):
        if getattr(self, "gp", None) is not None:
            return
        e = self.eng
        if e.dt != torch.float32:
            raise NotImplementedError("the gradient penalty runs in the exact-f32 mode (compute_dtype='fp32')")
        B, C, FF, S, N, H = e.B, self.C, self.FF, self.S, self.N, self.out
        M = B * S
        new = lambda *shape: torch.empty(*shape, device=e.device, dtype=torch.float32)
        self.gp = SimpleNamespace(
            dc1=new(B, H), zero_pe=torch.zeros(S * C, device=e.device, dtype=torch.float32),
            Xt=[new(M * C) for _ in range(N + 1)], qkvt=[new(M * 3 * C) for _ in range(N)], attt=[new(M * C) for _ in range(N)],
            r1t=[new(M * C) for _ in range(N)], x1t=[new(M * C) for _ in range(N)], f1t=[new(M * FF) for _ in range(N)],
            r2t=[new(M * C) for _ in range(N)], ytmp=new(M * C), xnt=new(M * C), meant=new(B * C), ct=new(B, H),
            # the delta sweep's own gradient buffers
            dmean=new(B * C), gA=new(M * C), gB=new(M * C), gC=new(M * C), gD=new(M * C), gAd=new(M * C), gBd=new(M * C),
            df1=new(M * FF), dqkv=new(M * 3 * C), datt=new(M * C), slabs=new(max(self.slab_floats(), self.ln_blocks * 2 * C)))

    def tangent(self, top_t):
        """``top_t``: tangent of the encoder's top buffer; returns (tensor, offset, item stride) of the tangent of c."""
        e = self.eng
        p, code, B = e.model._param, e.code, e.B
        C, FF, S, H = self.C, self.FF, self.S, self.out
        M = B * S
        Ltop, t0 = e.geo.alloc[-1], e.T - e.K - e.V
        P = _hip.ptr
        self._gp_buffers()
        gp, dp, seed = self.gp, self.drop_p, self.drop_seed

        def ln_t(at, bt, r, stats, wname, rt_out, yt, site=0):
            _hip.call("cpc_ln_tangent", P(at), P(bt), P(r), P(stats), P(p[wname + ".weight"]), P(rt_out), P(yt), M, C,
                      dp if bt is not None else 0.0, seed, site)
        _hip.call("cpc_pe_scale_fwd", P(top_t, t0 * C), P(gp.zero_pe), P(gp.Xt[0]), B, S, C, Ltop * C, self.z_scale, code)
        for l in range(self.N):
            Xt, w = gp.Xt[l], self.w[l]
            _hip.gemm_nt(P(Xt), P(w["in"]), P(gp.qkvt[l]), M, 3 * C, C, C, C, 3 * C, code)
            _hip.call(self.attn_abi + "_tangent", P(self.qkv[l]), P(gp.qkvt[l]), P(self.P[l]), P(gp.attt[l]), B, S, C, self.heads, dp, seed,
                      4 * l + self.SITE_ATTN)
            _hip.gemm_nt(P(gp.attt[l]), P(w["o"]), P(gp.ytmp), M, C, C, C, C, C, code)
            ln_t(Xt, gp.ytmp, self.r1[l], self.st1[l], self._lname(l, "norm1"), gp.r1t[l], gp.x1t[l], 4 * l + self.SITE_DROP1)
            _hip.gemm_nt(P(gp.x1t[l]), P(w["l1"]), P(gp.f1t[l]), M, FF, C, C, C, FF, code, mask=P(self.f1[l]))
            if dp > 0.0:
                gp.f1t[l].mul_(1.0 / (1.0 - dp))          # the stored f1 is the dropped activation: its zeros carry the keep mask
            _hip.gemm_nt(P(gp.f1t[l]), P(w["l2"]), P(gp.ytmp), M, C, FF, FF, FF, C, code)
            ln_t(gp.x1t[l], gp.ytmp, self.r2[l], self.st2[l], self._lname(l, "norm2"), gp.r2t[l], gp.Xt[l + 1], 4 * l + self.SITE_DROP2)
        ln_t(gp.Xt[self.N], None, self.X[self.N], self.stn, self.prefix + "encoder.norm", None, gp.xnt)
        _hip.call("cpc_mean_time", P(gp.xnt), P(gp.meant), B, S, C, code)
        _hip.gemm_nt(P(gp.meant), P(self.w_end), P(gp.ct), B, H, C, C, C, H, code, flags=_hip.GEMM_OUT_F32)
        return gp.ct, 0, H

    def gp_grads(self, gp_grad):
        self._gp_grad = gp_grad           # filled by the last pass (_backward_gp)

    def _backward_gp(self, dc):
        """The last pass of a gradient-penalty step: the ordinary backward of ``dc`` (lambda) with the second-order terms joining
        on the way down, beside the sweep of the summed scores' adjoint (delta, from the dc of pass 1) that gives the penalty parts
        of the weight gradients.  Everything on the main stream."""
        e = self.eng
        g, p, code, B = e.model._grad, e.model._param, e.code, e.B
        C, FF, S, H = self.C, self.FF, self.S, self.out
        M = B * S
        Ltop, t0 = e.geo.alloc[-1], e.T - e.K - e.V
        P = _hip.ptr
        gp, gpg, dp, seed = self.gp, self._gp_grad, self.drop_p, self.drop_seed
        drop = dp > 0.0
        sc, nb = gp.slabs, self.ln_blocks

        def ln_pair(lam, dl, rt, r, stats, wname, lam_out, lam_out_b, dl_out, dl_out_b, bcast=0, gscale=1.0, site=0):
            # lambda through the LayerNorm (+ its weight / bias gradients), the second-order terms from delta, then delta itself
            self._ln_bwd(lam[0], lam[1], r, stats, wname, lam_out, bcast=bcast, gscale=gscale, dr_b=lam_out_b, site=site)
            _hip.call("cpc_ln_gp", P(dl[0]), P(dl[1]), P(rt), P(r), P(stats), P(p[wname + ".weight"]), P(lam_out), P(lam_out_b), P(sc),
                      M, C, bcast, gscale, nb, dp if lam_out_b is not None else 0.0, seed, site)
            _hip.call("cpc_reduce_slabs", P(sc), P(gpg[wname + ".weight"]), 1, C, nb, C, 1, 1, 0, 0)
            _hip.call("cpc_ln_bwd", P(dl[0]), P(dl[1]), P(r), P(stats), P(p[wname + ".weight"]), P(dl_out), P(sc), M, C, bcast, gscale,
                      nb, P(dl_out_b), dp if dl_out_b is not None else 0.0, seed, site, code)

        def linear_grads(lam_y, dl_y, x, xt, k, l, rows, cols):
            e._colsum_to_grad(P(lam_y), g[self._lname(l, self._BNAMES[k])], M, rows, scratch=sc)
            e._tn_to_grad(P(lam_y), P(x), g[self._lname(l, self._WNAMES[k])], M, rows, cols, rows, cols, self.split[k], scratch=sc)
            e._tn_to_grad(P(dl_y), P(xt), gpg[self._lname(l, self._WNAMES[k])], M, rows, cols, rows, cols, self.split[k], scratch=sc)

        # end_layer and the mean over time
        _hip.call("cpc_cast2d", P(dc), P(self.dct), B, H, H, 1, code)
        _hip.gemm_tn(P(self.dct), P(self.mean), P(g[self.prefix + "end_layer.weight"]), B, H, C, H, C, C, code, flags=_hip.GEMM_OUT_F32)
        e._colsum_to_grad(P(self.dct), g[self.prefix + "end_layer.bias"], B, H)
        _hip.gemm_nt(P(self.dct), P(self.w_end_t), P(self.dmean), B, C, H, H, H, C, code)
        _hip.gemm_tn(P(gp.dc1), P(gp.meant), P(gpg[self.prefix + "end_layer.weight"]), B, H, C, H, C, C, code, flags=_hip.GEMM_OUT_F32)
        _hip.gemm_nt(P(gp.dc1), P(self.w_end_t), P(gp.dmean), B, C, H, H, H, C, code)
        lamA, lamB, lamAd, lamBd = self.gA[0], self.gB[0], self.gAd[0], self.gBd[0]
        ln_pair((self.dmean, None), (gp.dmean, None), gp.Xt[self.N], self.X[self.N], self.stn, self.prefix + "encoder.norm",
                self.gA[1], None, gp.gA, None, bcast=S, gscale=1.0 / S)
        lam, dl = (self.gA[1], None), (gp.gA, None)
        for l in range(self.N - 1, -1, -1):
            wt = self.wt[l]
            # norm2 over r2 = x1 + dropout(f2); delta's input gA is free again once this is done
            ln_pair(lam, dl, gp.r2t[l], self.r2[l], self.st2[l], self._lname(l, "norm2"), lamB, lamBd if drop else None,
                    gp.gB, gp.gBd if drop else None, site=4 * l + self.SITE_DROP2)
            lam_y2, dl_y2 = (lamBd, gp.gBd) if drop else (lamB, gp.gB)
            linear_grads(lam_y2, dl_y2, self.f1[l], gp.f1t[l], "l2", l, C, FF)
            _hip.gemm_nt(P(lam_y2), P(wt["l2"]), P(self.df1[0]), M, FF, C, C, C, FF, code, mask=P(self.f1[l]))
            _hip.gemm_nt(P(dl_y2), P(wt["l2"]), P(gp.df1), M, FF, C, C, C, FF, code, mask=P(self.f1[l]))
            linear_grads(self.df1[0], gp.df1, self.x1[l], gp.x1t[l], "l1", l, FF, C)
            _hip.gemm_nt(P(self.df1[0]), P(wt["l1"]), P(self.gC), M, C, FF, FF, FF, C, code)
            _hip.gemm_nt(P(gp.df1), P(wt["l1"]), P(gp.gC), M, C, FF, FF, FF, C, code)
            # norm1 over r1 = x + dropout(attention output projection)
            ln_pair((lamB, self.gC), (gp.gB, gp.gC), gp.r1t[l], self.r1[l], self.st1[l], self._lname(l, "norm1"), lamA,
                    lamAd if drop else None, gp.gA, gp.gAd if drop else None, site=4 * l + self.SITE_DROP1)
            lam_y, dl_y = (lamAd, gp.gAd) if drop else (lamA, gp.gA)
            linear_grads(lam_y, dl_y, self.att[l], gp.attt[l], "o", l, C, C)
            _hip.gemm_nt(P(lam_y), P(wt["o"]), P(self.datt), M, C, C, C, C, C, code)
            _hip.gemm_nt(P(dl_y), P(wt["o"]), P(gp.datt), M, C, C, C, C, C, code)
            site = 4 * l + self.SITE_ATTN
            _hip.call(self.attn_abi + "_bwd", P(self.qkv[l]), P(self.P[l]), P(self.datt), P(self.dqkv[0]), B, S, C, self.heads, dp, seed, site, code)
            _hip.call(self.attn_abi + "_gp", P(self.qkv[l]), P(gp.qkvt[l]), P(self.P[l]), P(gp.datt), P(self.dqkv[0]), B, S, C, self.heads, dp,
                      seed, site)
            _hip.call(self.attn_abi + "_bwd", P(self.qkv[l]), P(self.P[l]), P(gp.datt), P(gp.dqkv), B, S, C, self.heads, dp, seed, site, code)
            linear_grads(self.dqkv[0], gp.dqkv, self.X[l], gp.Xt[l], "in", l, 3 * C, C)
            _hip.gemm_nt(P(self.dqkv[0]), P(wt["in"]), P(self.gD), M, C, 3 * C, 3 * C, 3 * C, C, code)
            _hip.gemm_nt(P(gp.dqkv), P(wt["in"]), P(gp.gD), M, C, 3 * C, 3 * C, 3 * C, C, code)
            # (lamA is read by the next layer's norm2 and rewritten only by its norm1, after that read)
            lam, dl = (lamA, self.gD), (gp.gA, gp.gD)
        _hip.call("cpc_pe_scale_bwd", P(lam[0]), P(lam[1]), P(e.dact[-1], t0 * C), B, S, C, Ltop * C, self.z_scale, code)

    def backward(self, dc):
        e = self.eng
        phase = e._gp_phase
        if phase == 1:               # gradient penalty, pass 1: dc is the adjoint of the summed scores (the last pass starts from it)
            self._gp_buffers()
            self.gp.dc1.copy_(dc)
        elif phase == 3:
            if e.use_aux:
                torch.cuda.current_stream().wait_stream(e.aux)
            return self._backward_gp(dc)
        g, code, B = e.model._grad, e.code, e.B
        C, FF, S, H = self.C, self.FF, self.S, self.out
        M = B * S
        Ltop, t0 = e.geo.alloc[-1], e.T - e.K - e.V
        P = _hip.ptr
        # end_layer and the mean over time
        _hip.call("cpc_cast2d", P(dc), P(self.dct), B, H, H, 1, code)
        _hip.gemm_tn(P(self.dct), P(self.mean), P(g[self.prefix + "end_layer.weight"]), B, H, C, H, C, C, code, flags=_hip.GEMM_OUT_F32)
        e._colsum_to_grad(P(self.dct), g[self.prefix + "end_layer.bias"], B, H)
        _hip.gemm_nt(P(self.dct), P(self.w_end_t), P(self.dmean), B, C, H, H, H, C, code)
        if self.scratch is None:
            self.scratch = torch.empty(self.slab_floats(), device=e.device, dtype=torch.float32)     # side-stream workspace
        sc = self.scratch
        top = self.N & 1
        self._ln_bwd(self.dmean, None, self.X[self.N], self.stn, self.prefix + "encoder.norm", self.gA[top], bcast=S, gscale=1.0 / S)
        g1, g2 = self.gA[top], None
        for l in range(self.N - 1, -1, -1):
            wt = self.wt[l]
            gname = lambda k, names: g[self._lname(l, names[k])]
            drop = self.drop_p > 0.0
            s_ = l & 1
            ev = self._ev[l]
            if e.use_aux and l + 2 <= self.N - 1:
                # this layer writes buffer set l & 1, which the side stream last read for layer l + 2
                torch.cuda.current_stream().wait_event(self._ev[l + 2][4])
            gA, gB, gAd_, gBd_, df1, dqkv = self.gA[s_], self.gB[s_], self.gAd[s_], self.gBd[s_], self.df1[s_], self.dqkv[s_]
            # norm2 over r2 = x1 + dropout(f2)
            gBd = gBd_ if drop else gB
            self._ln_bwd(g1, g2, self.r2[l], self.st2[l], self._lname(l, "norm2"), gB, dr_b=gBd_ if drop else None,
                         site=4 * l + self.SITE_DROP2)
            with e.side(ev[0]):
                e._colsum_to_grad(P(gBd), gname("l2", self._BNAMES), M, C, scratch=sc)
                e._tn_to_grad(P(gBd), P(self.f1[l]), gname("l2", self._WNAMES), M, C, FF, C, FF, self.split["l2"], scratch=sc)
            _hip.gemm_nt(P(gBd), P(wt["l2"]), P(df1), M, FF, C, C, C, FF, code, mask=P(self.f1[l]))
            with e.side(ev[1]):
                e._colsum_to_grad(P(df1), gname("l1", self._BNAMES), M, FF, scratch=sc)
                e._tn_to_grad(P(df1), P(self.x1[l]), gname("l1", self._WNAMES), M, FF, C, FF, C, self.split["l1"], scratch=sc)
            _hip.gemm_nt(P(df1), P(wt["l1"]), P(self.gC), M, C, FF, FF, FF, C, code)
            # norm1 over r1 = x + dropout(attention output projection)
            gAd = gAd_ if drop else gA
            self._ln_bwd(gB, self.gC, self.r1[l], self.st1[l], self._lname(l, "norm1"), gA, dr_b=gAd_ if drop else None,
                         site=4 * l + self.SITE_DROP1)
            with e.side(ev[2]):
                e._colsum_to_grad(P(gAd), gname("o", self._BNAMES), M, C, scratch=sc)
                e._tn_to_grad(P(gAd), P(self.att[l]), gname("o", self._WNAMES), M, C, C, C, C, self.split["o"], scratch=sc)
            _hip.gemm_nt(P(gAd), P(wt["o"]), P(self.datt), M, C, C, C, C, C, code)
            _hip.call(self.attn_abi + "_bwd", P(self.qkv[l]), P(self.P[l]), P(self.datt), P(dqkv), B, S, C, self.heads, self.drop_p,
                      self.drop_seed, 4 * l + self.SITE_ATTN, code)
            with e.side(ev[3]):
                e._colsum_to_grad(P(dqkv), gname("in", self._BNAMES), M, 3 * C, scratch=sc)
                e._tn_to_grad(P(dqkv), P(self.X[l]), gname("in", self._WNAMES), M, 3 * C, C, 3 * C, C, self.split["in"], scratch=sc)
                if e.use_aux:
                    ev[4].record(e.aux)
            _hip.gemm_nt(P(dqkv), P(wt["in"]), P(self.gD), M, C, 3 * C, 3 * C, 3 * C, C, code)
            g1, g2 = gA, self.gD
        # positional encoder: dz = sqrt(C) * dx0 into rows [t0, t0+V) of the encoder's top-layer gradient
        _hip.call("cpc_pe_scale_bwd", P(g1), P(g2), P(e.dact[-1], t0 * C), B, S, C, Ltop * C, self.z_scale, code)


class Float32Host(ContextHost):
    """The host of a context network that computes in float32 inside an engine with bf16 storage (Float32Context).  Its own: ``dt`` /
    ``code`` are float32's (so ContextHost's helpers size and launch for float32), ``act[-1]`` / ``dact[-1]`` float32 shadows of the
    engine's top buffer and its gradient in the same [B][L_top][E] indexing.  The rest of the contract, ``ENGINE_NAMES``, is read from
    the engine at every access (``slabs`` and ``c`` appear after the context is built; ``use_aux`` and ``_gp_phase`` change between
    steps); any other name raises AttributeError."""

    ENGINE_NAMES = ("model", "device", "B", "E", "H", "K", "V", "T", "geo", "colsum_blocks", "aux", "c", "slabs",
                    "use_aux", "_gp_phase", "gp_capable", "_nbt_batch")

    def __init__(self, eng, top32, dtop32):
        self._e = eng
        self.dt, self.code = torch.float32, _hip.dtype_code(torch.float32)
        self.act, self.dact = [top32], [dtop32]


for _name in Float32Host.ENGINE_NAMES:
    setattr(Float32Host, _name, property(lambda self, _name=_name: getattr(self._e, _name)))
del _name


class Float32Context(Context):
    """An AudioGRUModel / AttentionModel context that computes in float32 inside an engine with bf16 storage.  Built for the
    gradient-penalty engines only (make_context): the penalty's tangent recurrence and reverse sweep of these two networks
    (GRUContext.tangent / gp_grads, AttentionContext.tangent / _backward_gp) carry second-order terms of saturating gates,
    LayerNorm and softmax and exist as float32 kernels; the encoder — where the FLOPs are — keeps bf16 storage.  The frames the
    context reads are converted into a float32 shadow of the top-layer buffer on the way in, dz and c on the way out."""

    def __init__(self, eng, cls, ar):
        self.eng = eng
        B, Ltop, E, H = eng.B, eng.geo.alloc[-1], eng.E, eng.H
        f32 = dict(device=eng.device, dtype=torch.float32)
        self.top32, self.dtop32 = torch.zeros(B * Ltop * E, **f32), torch.zeros(B * Ltop * E, **f32)
        self.top_t32 = None
        self.inner = cls(Float32Host(eng, self.top32, self.dtop32), ar)
        self.c_st = torch.zeros(B * H, device=eng.device, dtype=eng.dt)
        self.ct_st = torch.zeros(B * H, device=eng.device, dtype=eng.dt)
        self.z_scale, self.ahead_ok = self.inner.z_scale, self.inner.ahead_ok

    def _z(self, flat):
        e = self.eng
        t0 = e.T - e.K - e.V
        return flat.view(e.B, e.geo.alloc[-1], e.E)[:, t0:t0 + e.V, :]

    def allocate(self):
        self.inner.allocate()

    def slab_floats(self):
        return self.inner.slab_floats()

    def prepare_weights(self):
        self.inner.prepare_weights()

    def forward(self):
        self._z(self.top32).copy_(self._z(self.eng.act[-1]))
        self.inner.forward()
        self.c_st.view(self.eng.B, self.eng.H).copy_(self.inner.c_float())

    def c_operand(self):
        return self.c_st, 0, self.eng.H

    def c_float(self):
        return self.inner.c_float()

    def backward(self, dc):
        self.inner.backward(dc)
        self._z(self.eng.dact[-1]).copy_(self._z(self.dtop32))

    def tangent(self, top_t):
        if self.top_t32 is None:
            self.top_t32 = torch.zeros_like(self.top32)
        self._z(self.top_t32).copy_(self._z(top_t))
        ct, off, stride = self.inner.tangent(self.top_t32)
        B, H = self.eng.B, self.eng.H
        self.ct_st.view(B, H).copy_(ct.reshape(-1)[off:].as_strided((B, H), (stride, 1)))
        return self.ct_st, 0, H

    def gp_grads(self, gp_grad):
        self.inner.gp_grads(gp_grad)


def make_context(eng, ar):
    from .audio_model import AudioGRUModel, AudioLSTMModel, ConvolutionalArModel
    from .attention_model import AttentionModel
    if eng.gp_capable and eng.dt != torch.float32 and isinstance(ar, (AudioGRUModel, AttentionModel)):
        return Float32Context(eng, GRUContext if isinstance(ar, AudioGRUModel) else AttentionContext, ar)
    if isinstance(ar, AudioGRUModel):
        return GRUContext(eng, ar)
    if isinstance(ar, AudioLSTMModel):          # (never behind Float32Context: the LSTM has no gradient-penalty passes to run in float32)
        return LSTMContext(eng, ar)
    if isinstance(ar, ConvolutionalArModel):
        # ConvArContext is the lean path for the reference's plain default (no pooling in the first block, pooling in every
        # later one, stride 1); every other configuration runs on the grid kernels
        lean = not (ar.batch_norm or ar.residual) and all(s == 1 for s in ar.strides) and ar.poolings[0] == 1 and \
            all(p > 1 for p in ar.poolings[1:])
        if eng.gp_capable:
            lean = False          # the gradient penalty's tangent pass lives in the grid implementation
        if not lean:
            from .scalogram_engine import ConvArGridContext
            return ConvArGridContext(eng, ar)
        return ConvArContext(eng, ar)
    if isinstance(ar, AttentionModel):
        return AttentionContext(eng, ar)
    from .scalogram_model import ScalogramResidualEncoder
    if isinstance(ar, ScalogramResidualEncoder):
        from .scalogram_engine import ResNetArContext
        return ResNetArContext(eng, ar)
    raise NotImplementedError(f"no HIP context network for {type(ar).__name__}")


class ContextOnlyEngine(ContextHost):
    """A context network called on its own (``AudioGRUModel(...)(z)`` etc.): z (B, E, V) -> c (B, H), and its backward for the autograd
    bridge.  Reuses the context classes unchanged by presenting z as the encoder's top buffer: the host owns that buffer and its
    gradient, c, dc and the slab workspace, and nothing of a train step's predictor or loss."""

    def __init__(self, owner, batch_size, enc_size, steps, device, dtype: torch.dtype):
        super().__init__(owner, device, dtype, batch_size, enc_size, owner.ar_size, 0, steps)
        self.T = self.V
        self.geo = SimpleNamespace(alloc=[self.V], valid=[self.V])
        self._keep = []
        self.act, self.dact = [], []
        for store in (self.act, self.dact):
            full, view, _ = self._buf(self.B * self.V, self.E)
            self._keep.append(full)
            store.append(view)
        self.ctx = make_context(self, owner.autoregressive_model)
        self.c = torch.empty(self.B, self.H, device=self.device, dtype=torch.float32)
        self.dc = torch.zeros(self.B, self.H, device=self.device, dtype=torch.float32)
        self.ctx.allocate()
        self.slabs = torch.empty(max(1, self.ctx.slab_floats()), device=self.device, dtype=torch.float32)

    def run(self, z):
        if not z.is_cuda:
            raise RuntimeError("the context networks run on the GPU only (no CPU fallback)")
        if tuple(z.shape) != (self.B, self.E, self.V):
            raise ValueError(f"expected input of shape ({self.B}, {self.E}, {self.V}) = (batch, channels, steps), got {tuple(z.shape)}")
        self.act[-1].view(self.B, self.V, self.E).copy_(z.detach().transpose(1, 2))
        self.ctx.prepare_weights()
        self.ctx.forward()
        return self.ctx.c_float().clone()

    def backward_context(self, dc):
        """dc (B, H) -> d z (B, E, V) float32; the context network's parameter gradients go to the owner's flat gradient buffer
        (the autograd bridge of a stand-alone call, audio_model._ContextForward)."""
        self.dact[-1].zero_()
        self.dc.copy_(dc)
        self.ctx.backward(self.dc)
        if self.use_aux:
            torch.cuda.current_stream().wait_stream(self.aux)
        return self.dact[-1].view(self.B, self.V, self.E).float().transpose(1, 2)


def standalone_context_forward(ar, z, ar_size):
    """Host side of ``<context network>.forward(z)`` outside an AudioPredictiveCodingModel."""
    from .audio_model import AudioPredictiveCodingModel, _LinearParams
    import torch.nn as nn
    owner = getattr(ar, "_owner", None)
    if owner is None:
        object.__setattr__(ar, "_owner", None)
        owner = AudioPredictiveCodingModel.__new__(AudioPredictiveCodingModel)
        nn.Module.__init__(owner)
        owner.enc_size, owner.ar_size = int(z.shape[1]), int(ar_size)
        owner.visible_steps, owner.prediction_steps = int(z.shape[2]), 0
        owner.encoder = None
        owner.autoregressive_model = ar
        owner.prediction_model = _LinearParams(int(ar_size), 8)
        owner.compute_dtype = getattr(ar, "compute_dtype", torch.float32)
        owner._engines, owner._flat_param, owner._flat_grad, owner._param, owner._grad = {}, None, None, {}, {}
        owner._scalogram = False
        object.__setattr__(ar, "_owner", owner)
    dev = z.device
    if next(owner.prediction_model.parameters()).device != dev:
        owner.prediction_model.to(dev)
    key = ("ctx", tuple(z.shape), owner.compute_dtype, str(dev))
    eng = owner._engines.get(key)
    if eng is None or owner._flat_param is None or any(p.data_ptr() != owner._param[n].data_ptr() for n, p in owner.named_parameters()):
        owner._flatten_parameters(dev)
        eng = ContextOnlyEngine(owner, z.shape[0], z.shape[1], z.shape[2], dev, owner.compute_dtype)
        owner._engines = {key: eng}
    if torch.is_grad_enabled() and (z.requires_grad or any(p_.requires_grad for p_ in ar.parameters())):
        from .audio_model import _ContextForward
        names = [n for n, _ in owner.named_parameters() if n.startswith("autoregressive_model.")]
        return _ContextForward.apply(eng, names, z, *[dict(owner.named_parameters())[n] for n in names])
    return eng.run(z.float())
