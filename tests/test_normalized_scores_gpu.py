"""Cosine-similarity scores with a temperature on the HIP path (score kind "normalized", NormalizedScoreFunction): the cpc_norm_rows /
cpc_norm_rows_bwd kernels against float64, the public autograd function, and the engine / trainer routes against the CPU oracle with
    scores = linear_scores(F.normalize(predicted_z, dim=2, eps=1e-8) / tau, F.normalize(targets, dim=1, eps=1e-8))
as its score function."""
import copy
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd import contrastive_estimation_training as cet
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, grouped_negative_mask, sampled_negative_mask,
                                                           softplus_score_function)
from cpc_audio_amd.engine import FusedAdam
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
L_, F_ = C.c_longlong, C.c_float
SENTINEL = -8192.0                                  # exact in f32 and bf16
EPS = float(np.float32(1e-8))                       # the eps the kernels see (a C float)
INV_EPS = float(np.float32(1.0) / np.float32(1e-8))
U24, U8 = 2.0 ** -24, 2.0 ** -8
NEW_ENTRY_POINTS = {"cpc_norm_rows", "cpc_norm_rows_bwd"}


def NormalizedScoreFunction(temperature):
    """(looked up at call time: test_default_step_is_the_parent_step also runs on a tree from before the class existed)"""
    return cet.NormalizedScoreFunction(temperature)


# (rows, E) on contiguous rows (ld = E): E no multiple of the vector width (these take the scalar loads, since their rows do not start
# 16-byte aligned), exactly one 16-byte load per lane in bf16, one lane past that, fewer rows than a workgroup's waves, the largest E
SHAPES = [(1, 1), (5, 42), (13, 64), (7, 512), (3, 520), (2, 4096)]
# (rows, E, ld): rows padded to 16 bytes with E no multiple of the vector width — the 16-byte loads with the one-element-per-lane tail
# behind them (a tail alone, one piece + tail, several pieces + tail) — and the largest scalar-load instantiations (odd ld at E = 4095:
# sixteen f32 / eight bf16 pieces per lane)
PADDED = [(1, 1, 8), (5, 42, 48), (3, 517, 520), (2, 4095, 4095)]


def normalized_scores(p, t, tau, eps=1e-8):
    """The definition (the issue's torch expression), in the dtype of its inputs."""
    return O.linear_scores(F.normalize(p, dim=2, eps=eps) / tau, F.normalize(t, dim=1, eps=eps))


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _rel_l2(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


# ------------------------------------------------------------------------------------------ kernels
def _sum_roundings(E, dt):
    """Roundings on the longest path of the kernels' row sum (csrc/nrows.hip): a lane adds its own elements with one fma each — with
    16-byte loads (rows that start 16-byte aligned) CH elements of every 64th piece and at most one tail element, with scalar loads
    (all other rows) every 64th element — and six butterfly additions follow.  The larger of the two is taken for every case."""
    ch = 4 if dt == torch.float32 else 8
    vec = ch * -(-(E // ch) // 64) + (1 if E % ch else 0)
    scalar = -(-E // 64)
    return max(vec, scalar) + 6


def _fwd_bounds(E, dt):
    """(bound on |Y - ref| / |ref|, bound on |inv - ref| / ref).  f32: every term of the sum is a square, so its relative error is at
    most (roundings) 2^-24 to first order; the square root, the reciprocal, scale * inv and the product with X add one rounding each
    (the halving by the square root is not claimed).  bf16: one bf16 rounding of the exact result, 2^-8 with the f32 errors inside."""
    r = _sum_roundings(E, dt)
    return ((r + 4) * U24 if dt == torch.float32 else U8), (r + 2) * U24


def _bwd_bound(E, dt):
    """Bound on max_e |dX - ref| / (scale inv |G|) per row.  f32: the dot product's roundings (same shape as the sum), (inv / scale) *
    dot (two), scale * inv * G and the final fma (one each); the reference is evaluated at x = Y / (scale inv), whose norm differs
    from 1 / inv by delta <= ((sum roundings) / 2 + 3) 2^-24 of the forward, which enters the projection term twice and the leading
    factor once.  bf16: 2^-8, one bf16 rounding of an element the size of scale inv |G| (the elements of dX are smaller than
    that unless one element carries the whole row)."""
    r = _sum_roundings(E, dt)
    return (r + 4 + 3 * (r / 2 + 3)) * U24 if dt == torch.float32 else U8


def _rows(rows, E, dt, seed):
    """X (rows, E) in the storage dtype; with rows >= 3, row 1 is zero and row 2 has norm 1e-10."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, E, generator=g)
    if rows >= 3:
        X[1] = 0.0
        X[2] *= 1e-10 / X[2].norm()
    return X.to(dt)


def _forward_ref(X, scale):
    x = X.double()
    inv = 1.0 / x.norm(dim=1).clamp_min(EPS)
    return x * (scale * inv)[:, None], inv


def _check_forward(X, Y, inv, scale, dt):
    ref, inv_ref = _forward_ref(X, scale)
    yb, ib = _fwd_bounds(X.shape[1], dt)
    err = (Y.double().cpu() - ref).abs()
    worst = (err / ref.abs().clamp_min(1e-300)).max().item()
    inv_worst = ((inv.double().cpu() - inv_ref).abs() / inv_ref).max().item()
    print(f"cpc_norm_rows {tuple(X.shape)} {dt}: worst |Y - ref| / |ref| {worst:.3e} (bound {yb:.3e}), inv {inv_worst:.3e} (bound {ib:.3e})")
    assert (err <= yb * ref.abs()).all(), worst
    assert inv_worst <= ib
    if X.shape[0] >= 3:
        assert (Y[1] == 0).all() and float(inv[1]) == INV_EPS and float(inv[2]) == INV_EPS
        assert _rel(Y[2], X[2].double() * scale / EPS) <= yb


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,E", SHAPES)
def test_norm_rows_against_float64(rows, E, dt):
    """cpc_norm_rows on contiguous rows (rpi 0, ld E) vs float64 from the stored inputs; a zero row gives zeros, a row of norm 1e-10
    gives X scale / eps, both with inv = 1 / eps; the floats behind the last row stay untouched."""
    scale = 10.0
    X = _rows(rows, E, dt, seed=rows * 10000 + E).to(DEV)
    Y = torch.full((rows + 1, E), SENTINEL, device=DEV, dtype=dt)
    inv = torch.full((rows + 1,), SENTINEL, device=DEV)
    _hip.call("cpc_norm_rows", _hip.ptr(X), _hip.ptr(Y), _hip.ptr(inv), rows, E, 0, L_(0), L_(E), F_(scale), F_(1e-8), _hip.dtype_code(dt))
    torch.cuda.synchronize()
    _check_forward(X.cpu(), Y[:rows], inv[:rows], scale, dt)
    assert (Y[rows] == SENTINEL).all() and float(inv[rows]) == SENTINEL


def _top_layer(B, K, E, dt, seed):
    """(B, Ltop, E) like the top layer; target row (0, 1) is zero and (1, 0) has norm 1e-10, every other row is ordinary."""
    Ltop = K + 3
    T = Ltop - 1                  # a pad row behind the targets, as in the engine's top-layer buffer
    top = torch.randn(B, Ltop, E, generator=torch.Generator().manual_seed(seed)).to(dt)
    top[0, T - K + 1] = 0.0
    top[1, T - K] *= 1e-10 / top[1, T - K].float().norm()
    return top, T, Ltop


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_norm_rows_through_the_top_layer_map(dt):
    """The K target rows of every item inside a buffer shaped like the top layer (rpi K, item Ltop E, ld E, from row T - K): the
    named rows against float64, inv in (b, k) order, and every other row of a sentinel-filled Y untouched."""
    B, K, E, scale = 5, 3, 64, 1.0
    top, T, Ltop = _top_layer(B, K, E, dt, seed=77)
    top_d = top.to(DEV)
    Y = torch.full_like(top_d, SENTINEL)
    inv = torch.full((B * K,), SENTINEL, device=DEV)
    tg = (T - K) * E
    _hip.call("cpc_norm_rows", _hip.ptr(top_d, tg), _hip.ptr(Y, tg), _hip.ptr(inv), B * K, E, K, L_(Ltop * E), L_(E), F_(scale), F_(1e-8),
              _hip.dtype_code(dt))
    torch.cuda.synchronize()
    X = top[:, T - K:T, :].reshape(B * K, E)
    ref, inv_ref = _forward_ref(X, scale)
    yb, ib = _fwd_bounds(E, dt)
    got = Y[:, T - K:T, :].reshape(B * K, E).double().cpu()
    assert ((got - ref).abs() <= yb * ref.abs()).all()
    assert ((inv.double().cpu() - inv_ref).abs() <= ib * inv_ref).all()
    assert (got[1] == 0).all() and float(inv[1]) == INV_EPS and float(inv[K]) == INV_EPS          # rows (0, 1) and (1, 0)
    assert (Y[:, :T - K] == SENTINEL).all() and (Y[:, T:] == SENTINEL).all()


def _gradient_rows(X, dt, seed):
    """G like X: random, with row 0 parallel to X (the result cancels to ~0) and the last row orthogonal to X (where it is not row 0)."""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(X.shape, generator=g).double()
    x = X.double()
    G[0] = 0.5 * x[0]
    last = X.shape[0] - 1
    if last > 2:
        xh = x[last] / x[last].norm()
        G[last] = G[last] - xh * (xh * G[last]).sum()
    return G.to(dt)


def _backward_ref(Y, inv, G, scale):
    """float64 autograd of scale x / clamp(|x|, eps) at x = Y / (scale inv) — the stored Y-side inputs — with upstream G."""
    x = (Y.double() / (scale * inv.double())[:, None]).requires_grad_(True)
    y = scale * x / x.norm(dim=1, keepdim=True).clamp_min(EPS)
    return torch.autograd.grad((y * G.double()).sum(), x)[0]


def _check_backward(Y, inv, G, dX, scale, dt, what):
    ref = _backward_ref(Y.cpu(), inv.cpu(), G.cpu(), scale)
    size = scale * inv.double().cpu() * G.double().cpu().norm(dim=1)             # the terms before they cancel
    err = (dX.double().cpu() - ref).abs().max(dim=1).values
    bound = _bwd_bound(Y.shape[1], dt)
    worst = (err / size.clamp_min(1e-300)).max().item()
    print(f"cpc_norm_rows_bwd {what} {tuple(Y.shape)} {dt}: worst row error / (scale inv |G|) {worst:.3e} (bound {bound:.3e})")
    assert (err <= bound * size).all(), worst
    return ref


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,E", SHAPES)
def test_norm_rows_bwd_against_float64(rows, E, dt):
    """cpc_norm_rows_bwd in place over G vs float64 autograd, per row against scale inv |G|: a row with G parallel to X (result ~ 0), one
    with G orthogonal to X, the zero row and the row under eps (both: scale G / eps, no projection term)."""
    scale = 10.0
    code = _hip.dtype_code(dt)
    Xc = _rows(rows, E, dt, seed=rows * 10000 + E)
    X = Xc.to(DEV)
    Y = torch.empty_like(X)
    inv = torch.empty(rows, device=DEV)
    _hip.call("cpc_norm_rows", _hip.ptr(X), _hip.ptr(Y), _hip.ptr(inv), rows, E, 0, L_(0), L_(E), F_(scale), F_(1e-8), code)
    G0 = _gradient_rows(Xc, dt, seed=E)
    G = torch.full((rows + 1, E), SENTINEL, device=DEV, dtype=dt)
    G[:rows] = G0.to(DEV)
    _hip.call("cpc_norm_rows_bwd", _hip.ptr(Y), _hip.ptr(inv), _hip.ptr(G), rows, E, 0, L_(0), L_(E), F_(scale), F_(1e-8), code)
    torch.cuda.synchronize()
    ref = _check_backward(Y, inv, G0, G[:rows], scale, dt, "contiguous")
    assert (G[rows] == SENTINEL).all()
    if rows >= 3:                       # clamped rows: exactly the first term
        for r in (1, 2):
            assert _rel(G[r], G0[r].double() * scale / EPS) <= (3 * U24 if dt == torch.float32 else U8)
    if E > 1:                           # the parallel row cancels: far below the terms it is made of
        assert ref[0].abs().max().item() <= 2.0 ** -6 * scale * float(inv[0]) * G0[0].double().norm().item()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_norm_rows_bwd_through_the_top_layer_map(dt):
    B, K, E, scale = 5, 3, 64, 1.0
    code = _hip.dtype_code(dt)
    top, T, Ltop = _top_layer(B, K, E, dt, seed=78)
    top_d = top.to(DEV)
    Y = torch.zeros_like(top_d)
    inv = torch.empty(B * K, device=DEV)
    tg = (T - K) * E
    args = (B * K, E, K, L_(Ltop * E), L_(E), F_(scale), F_(1e-8), code)
    _hip.call("cpc_norm_rows", _hip.ptr(top_d, tg), _hip.ptr(Y, tg), _hip.ptr(inv), *args)
    X = top[:, T - K:T, :].reshape(B * K, E)
    G0 = _gradient_rows(X, dt, seed=5)
    G = torch.full_like(top_d, SENTINEL)
    G[:, T - K:T, :] = G0.view(B, K, E).to(DEV)
    _hip.call("cpc_norm_rows_bwd", _hip.ptr(Y, tg), _hip.ptr(inv), _hip.ptr(G, tg), *args)
    torch.cuda.synchronize()
    ref = _check_backward(Y[:, T - K:T, :].reshape(B * K, E), inv, G0, G[:, T - K:T, :].reshape(B * K, E), scale, dt, "top-layer map")
    assert (G[:, :T - K] == SENTINEL).all() and (G[:, T:] == SENTINEL).all()
    # target row (0, 0) is an ordinary row with G parallel to X: the projection branch ran and cancelled; (0, 1) and (1, 0) were clamped
    assert float(inv[0]) < INV_EPS and float(inv[1]) == INV_EPS and float(inv[K]) == INV_EPS
    size0 = scale * float(inv[0]) * G0[0].double().norm().item()
    assert ref[0].abs().max().item() <= 2.0 ** -6 * size0
    assert G[0, T - K].double().abs().max().item() <= (2.0 ** -6 + _bwd_bound(E, dt)) * size0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,E,ld", PADDED)
def test_norm_rows_padded_and_unaligned_rows(rows, E, ld, dt):
    """Both kernels on rows of ld >= E elements: with ld a multiple of the vector width and E not, the 16-byte loads and the scalar tail
    behind them; with an odd ld at E = 4095 the scalar loads at the most pieces per lane.  Forward and backward against float64 with
    the bounds of the contiguous tests; the padding [E, ld) of X, Y and G holds a sentinel, which no result may have seen and which must
    still be there afterwards, as must the row behind the last."""
    scale = 10.0
    code = _hip.dtype_code(dt)
    Xc = _rows(rows, E, dt, seed=rows * 10000 + E + ld)

    def padded(values):
        buf = torch.full((rows + 1, ld), SENTINEL, dtype=dt)
        buf[:rows, :E] = values
        return buf.to(DEV)

    def padding_intact(buf):
        return bool((buf[:rows, E:] == SENTINEL).all() and (buf[rows] == SENTINEL).all())

    X = padded(Xc)
    Y = torch.full((rows + 1, ld), SENTINEL, device=DEV, dtype=dt)
    inv = torch.full((rows + 1,), SENTINEL, device=DEV)
    _hip.call("cpc_norm_rows", _hip.ptr(X), _hip.ptr(Y), _hip.ptr(inv), rows, E, 0, L_(0), L_(ld), F_(scale), F_(1e-8), code)
    torch.cuda.synchronize()
    _check_forward(Xc, Y[:rows, :E], inv[:rows], scale, dt)
    assert padding_intact(Y) and float(inv[rows]) == SENTINEL
    G0 = _gradient_rows(Xc, dt, seed=E)
    G = padded(G0)
    _hip.call("cpc_norm_rows_bwd", _hip.ptr(Y), _hip.ptr(inv), _hip.ptr(G), rows, E, 0, L_(0), L_(ld), F_(scale), F_(1e-8), code)
    torch.cuda.synchronize()
    _check_backward(Y[:rows, :E], inv[:rows], G0, G[:rows, :E], scale, dt, f"ld {ld}")
    assert padding_intact(G) and padding_intact(Y)


# ------------------------------------------------------------------------------------------ public function
def test_normalized_score_function_against_float64():
    """NormalizedScoreFunction(0.1) at B, K, E = 2, 2, 8: scores and both input gradients vs the float64 expression, 1e-5 relative."""
    B, K, E = 2, 2, 8
    gen = torch.Generator().manual_seed(21)
    p0, t0 = torch.randn(B, K, E, generator=gen), torch.randn(B, E, K, generator=gen)
    g = torch.randn(B, K, B, K, generator=gen)
    p1, t1 = p0.to(DEV).requires_grad_(True), t0.to(DEV).requires_grad_(True)
    s1 = NormalizedScoreFunction(0.1)(p1, t1)
    (s1 * g.to(DEV)).sum().backward()
    p2, t2 = p0.double().requires_grad_(True), t0.double().requires_grad_(True)
    s2 = normalized_scores(p2, t2, 0.1)
    (s2 * g.double()).sum().backward()
    assert s1.shape == (B, K, B, K) and s2.abs().max().item() <= 10.0 + 1e-9
    assert _rel(s1, s2) < 1e-5
    assert _rel(p1.grad, p2.grad) < 1e-5
    assert _rel(t1.grad, t2.grad) < 1e-5


# ------------------------------------------------------------------------------------------ engine
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def _small(golden_dir):
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    return g, meta, torch.from_numpy(g["data"]), params


def _small_model(g, meta, dtype):
    C_, H, K, V = meta["C"], meta["H"], meta["K"], meta["V"]
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    ar = AudioGRUModel(input_size=C_, hidden_size=H)
    model = AudioPredictiveCodingModel(enc, ar, enc_size=C_, ar_size=H, visible_steps=V, prediction_steps=K, compute_dtype=dtype)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return model.to(DEV)


def _oracle(params, V, K, tau, **kw):
    """OracleTrainer with the definition as its score function (assigned from outside: oracle/ stays as it is)."""
    ot = O.OracleTrainer(params, V, K, score="linear", **kw)
    ot.score = lambda p, t: normalized_scores(p, t, tau)
    return ot


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


@pytest.mark.parametrize("tau", [0.1, 1.0])
@pytest.mark.parametrize("all_t", [False, True])
def test_engine_normalized_gradients_against_oracle(golden_dir, all_t, tau):
    """One fp32 engine step: loss within 1e-4 and every parameter gradient within 1e-3 relative L2 of the oracle's autograd."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "fp32")
    x = data[:meta["B"]]
    eng = model.engine(meta["B"], x.shape[1])
    out = eng.loss_and_grads(x.to(DEV), softplus=False, regularization=0.5, all_timesteps=all_t, score="normalized", temperature=tau)
    torch.cuda.synchronize()
    ot = _oracle(params, meta["V"], meta["K"], tau, all_timesteps=all_t, regularization=0.5)
    loss, smax, grads = ot.loss_and_grads(x)
    assert abs(float(out[0]) - float(loss)) < 1e-4 * abs(float(loss)), (float(out[0]), float(loss))
    assert abs(float(out[1]) - float(smax)) < 1e-4 * abs(float(smax)) and float(smax) <= 1.0 / tau + 1e-6
    for name, ref in grads.items():
        assert ref.abs().max() > 0 and _rel_l2(model._grad[name], ref) < 1e-3, name
    # the same call again is the same bits, on the scratch operands allocated once
    first, scratch = float(out[0]), eng._norm
    out = eng.loss_and_grads(x.to(DEV), softplus=False, regularization=0.5, all_timesteps=all_t, score="normalized", temperature=tau)
    assert float(out[0]) == first and eng._norm is scratch


@pytest.mark.parametrize("all_t", [False, True])
def test_engine_normalized_bf16(golden_dir, all_t):
    """bf16 storage (normalised operands and both gradients rounded to bf16 once per kernel): one engine step vs the fp32 oracle.
    Measured on MI355X: loss within 2.2e-4 / 3.2e-4 (default / all timesteps), worst per-parameter gradient relative L2 5.8e-2 /
    8.7e-2 (encoder.layers.0.weight).  Bounds: loss 1e-3, gradients 0.12 (test_engine_difference_bf16's)."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "bf16")
    x = data[:meta["B"]]
    eng = model.engine(meta["B"], x.shape[1])
    out = eng.loss_and_grads(x.to(DEV), softplus=False, regularization=0.5, all_timesteps=all_t, score="normalized", temperature=0.1)
    torch.cuda.synchronize()
    ot = _oracle(params, meta["V"], meta["K"], 0.1, all_timesteps=all_t, regularization=0.5)
    loss, smax, grads = ot.loss_and_grads(x)
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((_rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    print(f"bf16 normalized scores all_timesteps={all_t}: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]})")
    assert rel < 1e-3
    assert worst[0] < 0.12, worst


def masked_loss(sp, mask, reg):
    """The definition: sp [K][b][b'] the scores, mask [K][b][b'] the candidate sets (diagonal included)."""
    valid = torch.diagonal(sp, dim1=1, dim2=2)
    lse = torch.logsumexp(sp.masked_fill(~mask, float("-inf")), dim=1)
    return -valid.mean() + lse.mean() + reg * (sp.mean(dim=0) ** 2).mean()


GROUPS = [0, 0, 0, 1, 1, 2]


@pytest.mark.parametrize("selection", ["sampled", "grouped"])
def test_engine_normalized_with_selected_negatives(golden_dir, selection):
    """Default branch with negatives=(3, seed, draw) / negative_groups=(ids, "other"): loss and dpred vs float64 of the definition on
    the engine's own predictions and targets, the candidate sets restated on the host (1e-4 / 1e-3 relative L2)."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "fp32")
    B, K, tau, reg = meta["B"], meta["K"], 0.1, 0.5
    x = data[:B].to(DEV)
    eng = model.engine(B, x.shape[1])
    if selection == "sampled":
        kw, mask, entry = {"negatives": (3, 41, 7)}, sampled_negative_mask(B, K, 3, 41, 7), "cpc_nce_loss_sampled"
    else:
        assert B == len(GROUPS)
        kw = {"negative_groups": (torch.tensor(GROUPS, dtype=torch.int32, device=DEV), "other")}
        mask, entry = grouped_negative_mask(GROUPS, K, "other"), "cpc_nce_loss_grouped"
    eng.forward(x)
    with _Spy() as spy:
        eng.nce_forward_backward(False, reg, score="normalized", temperature=tau, **kw)
    torch.cuda.synchronize()
    assert entry in spy.names and "cpc_nce_loss" not in spy.names
    assert spy.names.count("cpc_norm_rows") == 2 and spy.names.count("cpc_norm_rows_bwd") == 2
    pred, targ, _, _ = eng.outputs()
    p64, t64 = pred.double().cpu().requires_grad_(True), targ.double().cpu().requires_grad_(True)
    sp = torch.diagonal(normalized_scores(p64, t64, tau), dim1=1, dim2=3).permute(2, 0, 1)
    loss = masked_loss(sp, mask, reg)
    dense = masked_loss(sp, torch.ones_like(mask), reg).detach()
    assert abs(float(loss.detach()) - float(dense)) > 1e-3 * abs(float(dense))           # the selection is visible at this size
    dp, dt_ = torch.autograd.grad(loss, (p64, t64))
    assert abs(float(eng.nce_out[0]) - float(loss.detach())) < 1e-4 * abs(float(loss.detach()))
    assert _rel_l2(eng.dpred.view(B, K, -1), dp) < 1e-3
    T, Ltop = eng.T, eng.geo.alloc[-1]
    assert _rel_l2(eng.dact[-1].view(B, Ltop, eng.E)[:, T - K:T, :], dt_.transpose(1, 2)) < 1e-3


def test_engine_normalized_fused_all_timesteps_route():
    """The fused all-timesteps route at the smallest shape fused_scores_ok() accepts (bf16, B K = 256, E = 128, even K): cpc_score_lse
    runs on the normalised operands; loss and gradients vs the oracle with the bf16 bounds (1e-3, 0.12).  Measured on MI355X: loss
    within 3.1e-4, worst per-parameter gradient relative L2 6.3e-2 (encoder.layers.0.weight)."""
    C_, H, V, K, B, tau = 128, 64, 4, 4, 64, 0.1
    L = 465 + (V + K - 1) * 160
    torch.manual_seed(11)
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(C_, H), enc_size=C_, ar_size=H, visible_steps=V, prediction_steps=K,
                                       compute_dtype="bf16")
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("weight") and n.startswith("encoder"):
                p.mul_(2.0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(3)) * 0.5
    eng = model.engine(B, L)
    assert eng.fused_scores_ok()
    timer = _hip.KernelTimer(only=["score_lse<bf16,256>", "cpc_norm_rows", "cpc_norm_rows_bwd"])
    _hip.set_timer(timer)
    try:
        out = eng.loss_and_grads(x.to(DEV).contiguous(), softplus=False, regularization=0.5, all_timesteps=True, score="normalized",
                                 temperature=tau)
        ran = timer.summary()
    finally:
        _hip.set_timer(None)
    assert ran["score_lse<bf16,256>"][0] == 1 and ran["cpc_norm_rows"][0] == 2 and ran["cpc_norm_rows_bwd"][0] == 2
    ot = _oracle(state, V, K, tau, all_timesteps=True, regularization=0.5)
    loss, smax, grads = ot.loss_and_grads(x)
    rel = abs(float(out[0]) - float(loss)) / abs(float(loss))
    worst = max((_rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
    print(f"bf16 normalized scores, fused all-timesteps route: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]})")
    assert rel < 1e-3
    assert worst[0] < 0.12, worst


# ------------------------------------------------------------------------------------------ trainer
def _trainer(model, data, meta, logger, score_function, all_t=False, **kw):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.5, score_over_all_timesteps=all_t, score_function=score_function,
                                      prediction_steps=meta["K"], ar_size=meta["H"], **kw)
    tr.verbose = False
    return tr


def _batches(data, meta, seed=5):
    random.seed(seed)
    return [list(b) for b in FileBatchSampler([data.shape[0]], meta["B"], 1, True, verbose=False)]


@pytest.mark.parametrize("all_t", [False, True])
def test_trainer_engine_route_with_normalized_scores(golden_dir, all_t):
    """NormalizedScoreFunction + Adam takes the engine route (two cpc_norm_rows launches per step, FusedAdam, device NaN guard): two
    fp32 steps against OracleTrainer.step with the bounds of the difference-score trainer test."""
    g, meta, data, params = _small(golden_dir)
    batches = _batches(data, meta)
    steps, lr, tau = 2, 1e-3, 0.1
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger, NormalizedScoreFunction(tau), all_t)
    assert tr._engine_normalized() and not tr._fused()
    timer = _hip.KernelTimer(only=["cpc_norm_rows"])
    random.seed(5)
    _hip.set_timer(timer)
    try:
        tr.train(batch_size=meta["B"], epochs=1, lr=lr, num_workers=0, max_steps=steps)
        launches = timer.summary().get("cpc_norm_rows", (0, 0.0, 0.0))[0]
    finally:
        _hip.set_timer(None)
    assert launches == 2 * steps
    assert hasattr(tr, "last_optimizer")            # FusedAdam: the engine route
    ot = _oracle(params, meta["V"], meta["K"], tau, all_timesteps=all_t, regularization=0.5, lr=lr)
    for i in range(steps):
        loss, smax = ot.step(data[batches[i]])
        assert abs(logger.loss_meter.values[i] - float(loss)) < 2e-4 * abs(float(loss)), i
        assert abs(logger.score_meter.values[i] - float(smax)) < 2e-4 * abs(float(smax)) + 1e-6, i
    for k, v in model.state_dict().items():
        ref = ot.params[k].detach()
        err = (v.cpu() - ref).abs()
        assert err.max().item() <= 2 * lr * steps * 1.01 + 1e-6, k
        tight = err <= 0.05 * lr * steps + 1e-4 * ref.abs()
        assert tight.float().mean().item() > 0.97, (k, tight.float().mean().item())


@pytest.mark.parametrize("all_t", [False, True])
def test_validate_with_normalized_scores(golden_dir, all_t):
    """validate() routes the kind through eng.nce_eval (normalise, score GEMM, cpc_nce_eval): per-step losses and accuracies and the
    mean score vs O.validation_terms on the same scores over the same batches (1e-4)."""
    g = _load(golden_dir, "validate.npz")
    meta = json.load(open(os.path.join(golden_dir, "validate.json")))
    data = torch.from_numpy(g["data"])
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model = _small_model(g, meta, "fp32")
    B, K, V, tau = meta["B"], meta["K"], meta["V"], 0.1
    tr = ContrastiveEstimationTrainer(model=model, dataset=None, validation_set=TensorAudioDataset(data, counts=meta["counts"], device=DEV),
                                      device=DEV, score_over_all_timesteps=all_t, score_function=NormalizedScoreFunction(tau),
                                      prediction_steps=K, ar_size=meta["H"])
    tr.verbose = False
    with _Spy() as spy:
        losses, acc, score, mi = tr.validate(batch_size=B, num_workers=0)
    lists = O.file_batch_sampler(meta["counts"], B, 8, True, seed=0)
    assert spy.names.count("cpc_norm_rows") == 2 * len(lists) and "cpc_norm_rows_bwd" not in spy.names
    want_l, want_a, want_s = 0.0, 0.0, 0.0
    for idx in lists:
        pred, targ, _, _ = O.cpc_forward(data[idx].unsqueeze(1), params, V, K, training=False)
        pl, pa, ms = O.validation_terms(normalized_scores(pred.double(), targ.double(), tau), all_t)
        want_l, want_a, want_s = want_l + pl, want_a + pa, want_s + float(ms)
    n = len(lists)
    assert _rel(losses, want_l / n) < 1e-4
    assert (acc.cpu().double() - want_a / n).abs().max().item() < 1e-4
    assert abs(score - want_s / n) < 1e-4 * max(1.0, abs(want_s / n))


def test_graphed_step_matches_eager_with_normalized_scores(golden_dir):
    """trainer.use_graph: three steps replayed from the captured graph against three eager steps, with the comparison of
    test_model_gpu.py's graphed-step test (losses 1e-6 relative, parameters 1e-5)."""
    g, meta, data, params = _small(golden_dir)
    results = []
    for use_graph in (False, True):
        model = _small_model(g, meta, "fp32")
        logger = _Logger()
        tr = _trainer(model, data, meta, logger, NormalizedScoreFunction(0.1))
        tr.use_graph = use_graph
        random.seed(5)
        with _Spy() as spy:
            tr.train(batch_size=meta["B"], epochs=1, lr=1e-3, num_workers=0, max_steps=3)
        assert spy.names.count("cpc_norm_rows") == (2 if use_graph else 6)          # captured once, replayed
        results.append((logger.loss_meter.values, {n: p.detach().clone() for n, p in model.named_parameters()}))
    (l0, p0), (l1, p1) = results
    assert len(l0) == 3 and len(l1) == 3
    assert max(abs(a - b) / abs(a) for a, b in zip(l0, l1)) < 1e-6
    for n in p0:
        assert _rel(p1[n], p0[n]) < 1e-5, n


def _scalogram_model(g, meta):
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    pre = PreprocessingModule(cqt_dict=meta["cqt"], **meta.get("pre", {"phase": True}))
    enc = ScalogramResidualEncoder(args_dict={'phase': meta.get("phase", True), 'blocks': blocks, 'activation_register': None},
                                   preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["E"], hidden_size=meta["H"]), enc_size=meta["E"],
                                       ar_size=meta["H"], visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype="fp32")
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return pre.to(DEV), model.to(DEV), blocks


@pytest.mark.parametrize("all_t", [False, True])
def test_scalogram_trainer_engine_route_with_normalized_scores(golden_dir, all_t):
    """ScalogramCPCEngine (CQT scalogram + residual encoder + GRU, scalogram_model fixture): one trainer step (lr 0), loss and all
    parameter gradients vs the oracle, as the difference-score test of that engine does."""
    g = _load(golden_dir, "scalogram_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    B, K, H, V, tau = meta["B"], meta["K"], meta["H"], meta["V"], 0.1
    pre, model, blocks = _scalogram_model(g, meta)
    model.train()
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    data = torch.from_numpy(g["data"])
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=0.1, score_over_all_timesteps=all_t, score_function=NormalizedScoreFunction(tau),
                                      prediction_steps=K, ar_size=H, preprocessing=pre)
    tr.verbose = False
    assert tr._engine_normalized()
    random.seed(91)
    idx = [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)][0]
    random.seed(91)
    with _Spy() as spy:
        tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=1)
    assert spy.names.count("cpc_norm_rows") == 2 and spy.names.count("cpc_norm_rows_bwd") == 2
    with torch.no_grad():
        scal = pre(data[idx].to(DEV).unsqueeze(1)).cpu()
    oblocks = [dict(b) for b in blocks]
    oblocks[0]["in_channels"] = 2
    ot = _oracle(params, V, K, tau, all_timesteps=all_t, regularization=0.1, lr=0.0, scalogram=oblocks)
    loss, smax, grads = ot.loss_and_grads(scal)
    assert abs(logger.loss_meter.values[0] - float(loss)) < 1e-4 * abs(float(loss)), (logger.loss_meter.values, float(loss))
    largest = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for name, ref in grads.items():
        got = dict(model.named_parameters())[name].grad.double().cpu()
        if ref.abs().max().item() < 1e-6 * largest:
            assert got.abs().max().item() < 1e-5 * largest, name
            continue
        assert _rel_l2(got, ref) < 1e-3, name


def test_default_step_is_the_parent_step(golden_dir):
    """softplus_score_function: no new entry point is reached, and losses and parameters after two steps are bit-identical to the step
    as it was before the temperature keyword existed — loss_and_grads called without it, FusedAdam behind it."""
    g, meta, data, params = _small(golden_dir)
    steps, lr = 2, 1e-3
    batches = _batches(data, meta)
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger, softplus_score_function)
    timer = _hip.KernelTimer(only=sorted(NEW_ENTRY_POINTS))
    random.seed(5)
    _hip.set_timer(timer)
    try:
        with _Spy() as spy:
            tr.train(batch_size=meta["B"], epochs=1, lr=lr, num_workers=0, max_steps=steps)
        ran = timer.summary()
    finally:
        _hip.set_timer(None)
    assert not ran and not NEW_ENTRY_POINTS & set(spy.names)
    assert spy.names.count("cpc_nce_loss") == steps
    eng = model.engine(meta["B"], data.shape[1], DEV)
    assert getattr(eng, "_norm", None) is None          # nothing new was allocated
    # the same two steps by hand, with the calls train() made before the keyword existed
    model0 = _small_model(g, meta, "fp32")
    model0.train()
    model0._flatten_parameters(DEV)
    opt = FusedAdam(model0, lr=lr)
    model0.link_grads()
    dev_data = data.to(DEV)
    losses = []
    for i in range(steps):
        x = dev_data[torch.as_tensor(batches[i], device=DEV)].contiguous()
        eng0 = model0.engine(x.shape[0], x.shape[1], DEV)
        if i == 0:
            eng0.nan_flag().zero_()
        opt.after_update = eng0.prepare_ahead
        opt.skip_flag = eng0.nan_flag()
        out = eng0.loss_and_grads(x, softplus=True, regularization=0.5, all_timesteps=False, grad_ready_hook=opt.hook,
                                  global_negatives=None, after_loss=None, score="softplus")
        opt.step(grad_scale=1.0)
        losses.append(float(out[0]))
    torch.cuda.synchronize()
    assert logger.loss_meter.values == losses
    for (k, v), (k0, v0) in zip(model.state_dict().items(), model0.state_dict().items()):
        assert k == k0 and torch.equal(v, v0), k
