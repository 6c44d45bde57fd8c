"""LAMB trust ratios on the HIP path: cpc_lamb against a float64 restatement of the definition at bounds counted from the kernels'
own summation shape and arithmetic (norms, ratios, parameters, moments), in pieces, with a clipping coefficient, under a raised skip
flag and with trust_clip; FusedAdam(trust_ratio=True) and ContrastiveEstimationTrainer (fused, clipped, generic route, resumed,
data-parallel pieces, bf16) against the CPU oracle model with engine.TorchLamb; and the default step, which must not reach cpc_lamb.
The fixtures, the fused step by hand and the bounds of the oracle comparison are those of tests/test_adamw_gpu.py."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

import test_adamw_gpu as A
from cpc_audio_amd import _hip
from cpc_audio_amd.contrastive_estimation_training import softplus_score_function
from cpc_audio_amd.engine import FusedAdam, GradAllReduce, TorchLamb
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
L, F = C.c_longlong, C.c_float
E24 = 2.0 ** -24          # half a unit in the last place of a float32 result: one rounding, relative
B1, B2, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))          # the values the kernels receive

# ---- the kernels' rounding counts (csrc/pointwise.hip, "LAMB layer-wise trust ratios") ----
# Sum of squares of a parameter of nb 64-float blocks, longest path from an element to the total:
#   4  a lane's four squares: one product and three fmas
#   4  xor-shuffle levels 8, 4, 2, 1 inside the block's 16 lanes
#   ceil(nb / 1024)  a thread of the ratio kernel adds the block sums t + 256 c, c = chain, chain + 4, ... : 256 threads x 4 chains
#   2  (a0 + a1) + (a2 + a3)     6  the wave's xor-shuffle tree     2  (w0 + w1) + (w2 + w3)
# Every term is a square, so the sum's relative error is at most count * 2^-24 (first order); the square root halves it and adds its own
# rounding, which stays below the count: the norm is held to count * 2^-24, as tests/test_grad_clip_gpu.py holds cpc_grad_norm's.
# Both norms are held to it; measured worst case on MI355X: w_norm 0.10, u_norm 0.14 of the count (the direction's own float32
# roundings, which u_norm also carries, average out over a tensor and stay far inside it).
def sum_roundings(nb):
    return 4 + 4 + -(-nb // 1024) + 2 + 6 + 2


# Direction of one element, from the float32 inputs p, g, m, v (first order, every count an upper limit; a contraction into an fma
# only removes roundings):
#   ge = (g * grad_scale) * cf                                   C_GE = 2 relative
#   m' = m + (ge - m) * (1 - b1): the difference, the constant 1 - b1, the product and the sum round once each, ge's own error enters
#        scaled by 1 - b1: |dm| <= (C_GE + 4) 2^-24 (|ge| + |m|)                                    C_M = 6, absolute, no cancellation assumed
#   v' = v b2 + (1 - b2) ge ge: all terms >= 0, so relative: v b2, 1 - b2, two products, the sum, twice ge's error     C_V = 5 + 2 C_GE = 9
#   r  = (m' * inv_bc1) / (sqrt(v') * inv_bc2_sqrt + eps): the two constants, two products, the square root, the sum with eps and the
#        (correctly rounded) division round once each, v' enters through the root with half its error: C_R = 7 + C_V / 2 = 11.5
#        relative to |r|, and dm enters as dm * inv_bc1 / denominator
#   u  = fma(wd, p, r): one rounding of |u|
C_GE, C_M, C_V = 2, 6, 9
C_R = 7 + C_V / 2
SIZES = [1, 3, 63, 64, 65, 200, 4096 + 5, 70000]          # floats per parameter, each padded to 64


class Buffers:
    """A synthetic flat buffer of the SIZES parameters with guard tails behind p, g, m, v, the workspace and the trust array; the
    parameters q with q % 2 == flip are selected, parameter 2 + flip has p = 0 everywhere, parameter 4 + flip g = m = v = 0."""

    def __init__(self, flip, seed):
        self.blocks = [-(-s // 64) for s in SIZES]
        self.table = [0] + [int(b) for b in np.cumsum(self.blocks)]
        self.nparams, self.nblocks, self.n = len(SIZES), self.table[-1], 64 * self.table[-1]
        self.selected = [q % 2 == flip for q in range(self.nparams)]
        self.zero_p, self.zero_g = 2 + flip, 4 + flip
        gen = torch.Generator().manual_seed(seed)
        host = {k: torch.zeros(self.n) for k in "pgmv"}
        self.real = torch.zeros(self.n, dtype=torch.bool)          # False on the alignment padding
        for q, size in enumerate(SIZES):
            lo = 64 * self.table[q]
            self.real[lo:lo + size] = True
            wscale, gscale = 0.02 * 3.0 ** (q % 4), 10.0 ** -(q % 3)
            if q != self.zero_p:
                host["p"][lo:lo + size] = torch.randn(size, generator=gen) * wscale
            if q != self.zero_g:
                host["g"][lo:lo + size] = torch.randn(size, generator=gen) * gscale
                host["m"][lo:lo + size] = torch.randn(size, generator=gen) * gscale * 0.5
                host["v"][lo:lo + size] = torch.rand(size, generator=gen) * gscale ** 2
        self.host = host
        (self.p, self.pw), (self.g, self.gw), (self.m, self.mw), (self.v, self.vw) = (A._guarded_copy(host[k]) for k in "pgmv")
        bits = np.repeat(np.array(self.selected), self.blocks)
        words = np.zeros(-(-self.nblocks // 32), dtype=np.uint32)
        for j in np.nonzero(bits)[0]:
            words[j // 32] |= np.uint32(1) << np.uint32(j % 32)
        self.words = torch.from_numpy(words.view(np.int32).copy()).to(DEV)
        self.table_host = (C.c_int * (self.nparams + 1))(*[int(b) for b in self.table])
        self.table_dev = torch.tensor([int(b) for b in self.table], dtype=torch.int32, device=DEV)
        self.inverse = torch.from_numpy(np.repeat(np.arange(self.nparams, dtype=np.int32), self.blocks)).to(DEV)
        floats = int(_hip.lib().cpc_lamb_workspace_floats(L(self.nblocks)))
        assert floats == 2 * self.nblocks
        self.ws, self.wsw = A._guarded(floats, fill=A.SENTINEL)
        self.trust, self.tw = A._guarded(3 * self.nparams, fill=A.SENTINEL)

    def call(self, first, count, t, lr, wd, scale=1.0, coef=None, clip=None, skip=None):
        lo, hi = 64 * self.table[first], 64 * self.table[first + count]
        _hip.call("cpc_lamb", *[_hip.ptr(x, lo) for x in (self.p, self.g, self.m, self.v)], L(hi - lo), F(lr), F(B1), F(B2), F(EPS), t,
                  F(scale), F(wd), _hip.ptr(self.words), L(lo // 64), _hip.ptr(coef), C.cast(self.table_host, C.c_void_p),
                  _hip.ptr(self.table_dev), _hip.ptr(self.inverse), first, count, self.nparams, F(-1.0 if clip is None else clip),
                  _hip.ptr(self.ws), _hip.ptr(self.trust), _hip.ptr(skip))

    def state(self):
        torch.cuda.synchronize()
        return [x.clone() for x in (self.p, self.m, self.v, self.trust, self.ws)]

    def intact(self):
        return A._intact(self.pw, self.gw, self.mw, self.vw, self.wsw, self.tw) and torch.equal(self.g.cpu(), self.host["g"])

    def rows(self):
        return self.trust.cpu().double().view(3, self.nparams)


def _lamb64(buf, p, g, m, v, t, lr, wd, scale=1.0, cf=1.0, clip=None):
    """One step of the definition in float64 on the float32 inputs, with the first-order error bounds of the kernels' arithmetic:
    (p', m', v', rows [w_norm, u_norm, ratio], per-parameter norm bounds (w, u), per-element bound on p', natural ratios)."""
    p, g, m, v = (x.double().cpu() for x in (p, g, m, v))
    lr, wd, scale, cf = (float(np.float32(x)) for x in (lr, wd, scale, cf))
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    ge = g * scale * cf
    m1 = m + (ge - m) * (1 - B1)
    v1 = B2 * v + (1 - B2) * ge * ge
    den = v1.sqrt() / math.sqrt(bc2) + EPS
    r = (m1 / bc1) / den
    sel = torch.from_numpy(np.repeat(np.array(buf.selected), buf.blocks).repeat(64))
    u = torch.where(sel, r + wd * p, r)
    du = E24 * (C_R * r.abs() + C_M * (ge.abs() + m.abs()) / bc1 / den + u.abs())
    rows, bounds, natural = torch.zeros(3, buf.nparams, dtype=torch.float64), [], []
    trust_el, dtrust_el = torch.ones_like(p), torch.zeros_like(p)
    for q in range(buf.nparams):
        lo, hi = 64 * buf.table[q], 64 * buf.table[q + 1]
        w_norm, u_norm = p[lo:hi].norm().item(), u[lo:hi].norm().item()
        count = sum_roundings(buf.blocks[q]) * E24
        # Both norms are HELD to the plain count (_check_step).  For the ratio's and the parameters' bounds the derivation also allows
        # for the computed direction's own error, which moves u_norm by at most sum |u| du / ||u||^2, relative:
        bound_u = count + ((u[lo:hi].abs() * du[lo:hi]).sum().item() / u_norm ** 2 if u_norm > 0 else 0.0)
        ratio, dratio = 1.0, 0.0
        if buf.selected[q] and w_norm > 0 and u_norm > 0:
            ratio, dratio = w_norm / u_norm, count + bound_u + E24          # both norms and the division
        natural.append(ratio)
        if clip is not None and ratio > clip:
            ratio, dratio = float(np.float32(clip)), 0.0
        rows[:, q] = torch.tensor([w_norm, u_norm, ratio])
        bounds.append((count, bound_u))
        trust_el[lo:hi], dtrust_el[lo:hi] = ratio, dratio
    p1 = p - lr * trust_el * u
    # p' = p - (lr * trust) * u: the ratio's error, the products lr * trust and (.) * u, the direction's error, and the rounding of the
    # difference, at most 2^-24 (|p| + |update|):  lr trust |u| (ratio bound + 3 * 2^-24)  +  lr trust du  +  2^-24 |p|
    dp = lr * trust_el * (u.abs() * (dtrust_el + 3 * E24) + du) + E24 * p.abs()
    return p1, m1, v1, rows, bounds, dp, natural


def _check_step(buf, before, t, lr, wd, scale=1.0, cf=1.0, clip=None, tag=""):
    """Everything the definition fixes about one cpc_lamb call over the whole buffer, against _lamb64 fed the call's float32 inputs."""
    p64, m64, v64, rows64, bounds, dp, natural = _lamb64(buf, before[0], buf.g, before[1], before[2], t, lr, wd, scale, cf, clip)
    torch.cuda.synchronize()
    assert buf.intact(), tag
    rows = buf.rows()
    worst_w = worst_u = worst_p = 0.0
    for q in range(buf.nparams):
        for k, name in ((0, "w_norm"), (1, "u_norm")):
            want, got, bound = rows64[k, q].item(), rows[k, q].item(), bounds[q][0]          # the summation count, for both norms
            if want == 0.0:
                assert got == 0.0, (tag, q, name)
                continue
            rel = abs(got - want) / want
            worst_w, worst_u = (max(worst_w, rel / bound), worst_u) if k == 0 else (worst_w, max(worst_u, rel / bound))
            assert rel <= bound, (tag, q, name, rel, bound)
        says_one = not buf.selected[q] or rows64[0, q] == 0.0 or rows64[1, q] == 0.0
        if says_one and (clip is None or clip >= 1.0):
            assert rows[2, q].item() == 1.0, (tag, q)          # exactly 1.0f
        elif clip is not None and natural[q] > clip:
            assert rows[2, q].item() == float(np.float32(clip)), (tag, q)
        else:
            assert abs(rows[2, q].item() - rows64[2, q].item()) <= (2 * bounds[q][0] + bounds[q][1]) * rows64[2, q].item(), (tag, q)
    err_p = (buf.p.double().cpu() - p64).abs()
    worst_p = (err_p / dp.clamp_min(1e-300))[buf.real].max().item()
    print(f"cpc_lamb {tag} step {t}: worst error / bound: w_norm {worst_w:.3f}, u_norm {worst_u:.3f}, p {worst_p:.3f}; "
          f"ratios {[round(x, 4) for x in rows[2].tolist()]}")
    assert bool((err_p <= dp).all()), (tag, worst_p)
    # the moments: the bound tests/test_adamw_gpu.py holds cpc_adamw's to
    assert (buf.m.double().cpu() - m64).abs().max().item() < 2e-6 and (buf.v.double().cpu() - v64).abs().max().item() < 2e-6, tag
    # the alignment padding is zero and stays zero
    pad = ~buf.real
    assert not buf.p.cpu()[pad].any() and not buf.m.cpu()[pad].any() and not buf.v.cpu()[pad].any(), tag
    return rows, natural


# ------------------------------------------------------------------------------------------ 1. the entry point against float64
@pytest.mark.parametrize("wd", [0.1, 0.0])
@pytest.mark.parametrize("flip", [0, 1])
def test_lamb_against_float64(flip, wd):
    """Three whole-buffer steps from non-zero moments.  Both norms at count * 2^-24, ratios exactly 1.0f where the definition says 1, parameters at lr trust |u| (ratio bound + direction count) + 2^-24 |p|,
    moments at 2e-6; padding and guard tails intact."""
    lr = 1e-2
    buf = Buffers(flip, seed=10 + flip)
    assert sum_roundings(buf.blocks[-1]) == 20 and sum_roundings(16384) * E24 < 2.1e-6          # the bound stays useful at layer 2's size
    start = buf.p.clone()
    for t in range(1, 4):
        before = buf.state()
        buf.call(0, buf.nparams, t, lr, wd)
        rows, natural = _check_step(buf, before, t, lr, wd, tag=f"flip {flip} wd {wd}")
        assert rows[0, buf.zero_p] == 0.0 or t > 1          # the all-zero parameter: ratio 1 (asserted above), Adam's plain step
        if t == 1:
            if wd == 0.0:
                assert rows[1, buf.zero_g] == 0.0 and rows[2, buf.zero_g] == 1.0          # a zero direction
            else:          # u = wd p: the ratio is 1 / wd
                assert abs(rows[2, buf.zero_g].item() * float(np.float32(wd)) - 1.0) < 1e-5
            moved = [q for q in range(buf.nparams) if buf.selected[q] and rows[2, q] != 1.0]
            assert len(moved) >= 2 and len({round(rows[2, q].item(), 3) for q in moved}) == len(moved)
    assert (buf.p - start).abs().max().item() > 1e-3          # ... and the steps were applied


# ------------------------------------------------------------------------------------------ 2. pieces
def test_pieces_at_parameter_boundaries_give_the_whole_buffer_bits():
    """The buffer updated as four ranges (three splits at parameter boundaries, issued from the tail as the backward pass does) and
    as single parameters: p, m, v, trust and the block sums carry the bits of the one whole-buffer call."""
    lr, wd = 1e-2, 0.1
    results = []
    for cuts in ([0, 8], [0, 2, 5, 7, 8], list(range(9))):
        buf = Buffers(1, seed=20)
        for a, b in reversed(list(zip(cuts, cuts[1:]))):
            buf.call(a, b - a, 2, lr, wd, scale=0.5)
        results.append(buf.state())
        assert buf.intact()
    for other in results[1:]:
        for x, y, name in zip(results[0], other, ("p", "m", "v", "trust", "workspace")):
            assert torch.equal(x, y), name
    assert not (results[0][4] == A.SENTINEL).any() and not (results[0][3] == A.SENTINEL).any()          # every cell was written


# ------------------------------------------------------------------------------------------ 3. the clipping coefficient
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_coefficient(scale):
    """coef -> 1.0f: (g * grad_scale) * 1 is exact, the bits are those without coef (grad_scale 1 and 1/2: exact products).  coef -> 0.5f:
    the float64 restatement's step on the halved gradient."""
    lr, wd = 1e-2, 0.1
    plain, one, half = Buffers(0, seed=30), Buffers(0, seed=30), Buffers(0, seed=30)
    plain.call(0, plain.nparams, 3, lr, wd, scale=scale)
    one.call(0, one.nparams, 3, lr, wd, scale=scale, coef=torch.full((1,), 1.0, device=DEV))
    for x, y, name in zip(plain.state(), one.state(), ("p", "m", "v", "trust", "workspace")):
        assert torch.equal(x, y), name
    before = half.state()
    half.call(0, half.nparams, 3, lr, wd, scale=scale, coef=torch.full((1,), 0.5, device=DEV))
    _check_step(half, before, 3, lr, wd, scale=scale, cf=0.5, tag=f"coef 0.5 scale {scale}")
    assert not torch.equal(half.m, plain.m)


# ------------------------------------------------------------------------------------------ 4. the skip flag
def test_raised_skip_flag_changes_nothing():
    buf = Buffers(1, seed=40)
    buf.call(0, buf.nparams, 1, 1e-2, 0.1)
    before = buf.state()
    flag = torch.ones(1, device=DEV)
    buf.call(0, buf.nparams, 2, 1e-2, 0.1, skip=flag)
    buf.call(2, 3, 2, 1e-2, 0.1, coef=torch.full((1,), 0.5, device=DEV), skip=flag)
    for x, y, name in zip(before, buf.state(), ("p", "m", "v", "trust", "workspace")):
        assert torch.equal(x, y), name
    assert buf.intact()
    flag.zero_()
    buf.call(0, buf.nparams, 2, 1e-2, 0.1, skip=flag)          # a lowered flag lets the update through
    assert not torch.equal(before[0], buf.state()[0])


# ------------------------------------------------------------------------------------------ 5. trust_clip
def test_trust_clip_clamps_exactly_the_ratios_above_it():
    lr, wd = 1e-2, 0.1
    free, clipped = Buffers(1, seed=50), Buffers(1, seed=50)
    before = free.state()
    free.call(0, free.nparams, 1, lr, wd)
    natural = free.rows()[2].tolist()
    above = sorted(x for x in natural if x != 1.0)
    assert len(above) >= 3
    clip = 0.5 * (above[-1] + above[-2])          # below the largest natural ratio only; far from both
    assert clip > 1.0
    clipped.call(0, clipped.nparams, 1, lr, wd, clip=clip)
    rows, nat64 = _check_step(clipped, before, 1, lr, wd, clip=clip, tag="trust_clip")
    hit = [q for q in range(free.nparams) if natural[q] > clip]
    assert len(hit) == 1 and [q for q in range(free.nparams) if nat64[q] > clip] == hit
    for q in range(free.nparams):
        lo, hi = 64 * free.table[q], 64 * free.table[q + 1]
        if q in hit:
            assert rows[2, q].item() == float(np.float32(clip)) and not torch.equal(free.p[lo:hi], clipped.p[lo:hi])
        else:          # the other parameters do not see the clip: the free run's bits
            assert clipped.trust[2 * free.nparams + q] == free.trust[2 * free.nparams + q] and torch.equal(free.p[lo:hi], clipped.p[lo:hi])


# ------------------------------------------------------------------------------------------ engine / trainer against the oracle
WD = 0.1
_LAMB_ORACLE = {}


def _nsteps(data, meta):
    return min(3, data.shape[0] // meta["B"])


def _oracle_lamb(golden_dir, context, clip_fraction=None, trust_clip=None):
    """The oracle model under engine.TorchLamb (default filter: dim() >= 2) with the schedule set per step as LambdaLR would, and,
    with clip_fraction, torch.nn.utils.clip_grad_norm_ at that fraction of the first step's gradient norm in front of the step:
    (losses, learning rates, parameters, {name: (w_norm, u_norm, ratio)} of the last step, max_grad_norm); computed once per setting."""
    key = (context, clip_fraction, trust_clip)
    if key not in _LAMB_ORACLE:
        meta, data, state, _, okw = A._fixture(golden_dir, context)
        batches = A._batches(data, meta["B"])
        ot = O.OracleTrainer(state, meta["V"], meta["K"], score="softplus", regularization=A.REG, lr=A.LR, **okw)
        opt = TorchLamb(ot.params.items(), lr=A.LR, weight_decay=WD, trust_clip=trust_clip)
        losses, lrs, max_norm = [], [], None
        for i in range(_nsteps(data, meta)):
            loss, _, grads = ot.loss_and_grads(data[batches[i]])
            if clip_fraction is not None:
                if max_norm is None:
                    max_norm = clip_fraction * float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values())))
                torch.nn.utils.clip_grad_norm_(list(ot.params.values()), max_norm)
            lrs.append(A.LR * A.SCHED.factor(i))
            opt.param_groups[0]["lr"] = lrs[-1]
            opt.step()
            losses.append(float(loss))
        trust = {k: tuple(float(x) for x in t3) for k, t3 in opt.last_trust.items()}
        _LAMB_ORACLE[key] = (losses, lrs, {k: p.detach().clone() for k, p in ot.params.items()}, trust, max_norm)
    return _LAMB_ORACLE[key]


def _oracle_adamw(golden_dir, context, max_norm=None):
    """The run with trust_ratio=False: the same oracle steps under torch.optim.AdamW with the same decay, filter and schedule
    (tests/test_adamw_gpu.py _oracle_run, for this file's step count) and, with max_norm, the same clip_grad_norm_ in front of every
    step; computed once: the parameters."""
    key = (context, "adamw", max_norm)
    if key not in _LAMB_ORACLE:
        meta, data, state, _, okw = A._fixture(golden_dir, context)
        batches = A._batches(data, meta["B"])
        ot = O.OracleTrainer(state, meta["V"], meta["K"], score="softplus", regularization=A.REG, lr=A.LR, **okw)
        plist = list(ot.params.values())
        opt = torch.optim.AdamW([{"params": [p for p in plist if p.dim() >= 2], "weight_decay": WD},
                                 {"params": [p for p in plist if p.dim() < 2], "weight_decay": 0.0}], lr=A.LR)
        for i in range(_nsteps(data, meta)):
            ot.loss_and_grads(data[batches[i]])
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(plist, max_norm)
            for group in opt.param_groups:
                group["lr"] = A.LR * A.SCHED.factor(i)
            opt.step()
        _LAMB_ORACLE[key] = {k: p.detach().clone() for k, p in ot.params.items()}
    return _LAMB_ORACLE[key]


def _scaled_down(oracle_trust):
    """The tensors whose update the ratio shrinks at least five times (on the fixtures: all matrices but the first convolution and
    the predictor, whose ratios lie near 1)."""
    names = [k for k, v in oracle_trust.items() if v[2] <= 0.2]
    assert len(names) >= 4
    return names


def _differs_from_the_run_without_trust_ratio(golden_dir, context, model, oracle_trust, bound=1e-3, max_norm=None):
    """A silently ignored trust_ratio fails.  That the route was taken is shown by the callers' launch counts (every update a cpc_lamb
    call, none a cpc_adam*); this shows that the RESULT is another one: the trust_ratio=False run of the same settings is, within the
    f32 bounds of tests/test_adamw_gpu.py, the oracle run under torch.optim.AdamW (same decay, schedule, steps and gradient clip), and
    every tensor with a ratio <= 0.2 lies beyond 10 x the relative-L2 bound it is held to against the TorchLamb run."""
    adamw = _oracle_adamw(golden_dir, context, max_norm)
    sd = model.state_dict()
    for k in _scaled_down(oracle_trust):
        assert A._rel_l2(sd[k].cpu(), adamw[k]) >= 10 * bound, (k, A._rel_l2(sd[k].cpu(), adamw[k]))


def _ratios_follow_the_oracle(opt, oracle_trust):
    """FusedAdam.trust_ratios() of the last step next to TorchLamb's on the oracle model: the same parameters, exactly 1 where the
    oracle's is 1 (the parameters the filter leaves out).  The worst relative difference is printed, not bounded: the parameters the
    ratios produce are what the oracle comparison holds."""
    got = opt.trust_ratios()
    assert set(got) == set(oracle_trust)
    worst = max(abs(got[k][2] - oracle_trust[k][2]) / oracle_trust[k][2] for k in got)
    print(f"  trust ratios: worst relative difference to the oracle's {worst:.3e}; "
          f"range {min(v[2] for v in got.values()):.4g} ... {max(v[2] for v in got.values()):.4g}")
    assert any(v[2] != 1.0 for v in got.values()) and all(v[2] == 1.0 for k, v in got.items() if oracle_trust[k][2] == 1.0)


@pytest.mark.parametrize("context", ["gru", "conv", "attention"])
def test_engine_lamb_steps_against_oracle(golden_dir, context):
    """eng.loss_and_grads + FusedAdam(trust_ratio=True, weight_decay, schedule) with piecewise hooks: every update is a cpc_lamb call
    (pieces and the head), none a cpc_adam / cpc_adamw; losses and parameters at the bounds tests/test_adamw_gpu.py holds its AdamW
    runs to (_check_against_oracle: loss 1e-4 (1 + 2 i), 97 % of the elements within 0.05 sum(lr_i) + 1e-4 |ref|, relative L2 1e-3)."""
    meta, data, state, build, _ = A._fixture(golden_dir, context)
    oracle = _oracle_lamb(golden_dir, context)
    steps = _nsteps(data, meta)
    model = build("fp32")
    with A._Spy() as spy:
        opt, losses, lrs = A._engine_steps(model, data, A._batches(data, meta["B"]), steps, weight_decay=WD, schedule=A.SCHED,
                                           trust_ratio=True)
    assert spy.names.count("cpc_lamb") > steps and not {"cpc_adam", "cpc_adamw", "cpc_adam_clip"} & set(spy.names)
    assert lrs == oracle[1] and opt.t == steps
    A._check_against_oracle(context, model, losses, oracle[:3])
    _ratios_follow_the_oracle(opt, oracle[3])
    _differs_from_the_run_without_trust_ratio(golden_dir, context, model, oracle[3], max_norm=oracle[4])


def test_trainer_clipped_lamb_steps_against_oracle(golden_dir):
    """ContrastiveEstimationTrainer.train with trust_ratio, trust_clip, weight_decay, lr_schedule and max_grad_norm: the deferred
    whole-buffer route, one cpc_grad_norm and one cpc_lamb per step; the same bounds."""
    context = "gru"
    meta, data, state, build, _ = A._fixture(golden_dir, context)
    free = _oracle_lamb(golden_dir, context)
    trust_clip = 0.5 * max(v[2] for v in free[3].values())          # binds on the largest ratio of the unclipped run
    oracle = _oracle_lamb(golden_dir, context, clip_fraction=0.5, trust_clip=trust_clip)
    steps = _nsteps(data, meta)
    model = build("fp32")
    logger = A._Logger()
    tr = A._trainer(model, data, meta, logger)
    tr.trust_ratio, tr.trust_clip, tr.weight_decay, tr.lr_schedule, tr.max_grad_norm = True, trust_clip, WD, A.SCHED, oracle[4]
    tr.host_sync_lag = 0
    random.seed(A.SEED)
    with A._Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=A.LR, num_workers=0, max_steps=steps)
    torch.cuda.synchronize()
    assert tr.training_step == steps and spy.names.count("cpc_lamb") == steps and spy.names.count("cpc_grad_norm") == steps
    assert not {"cpc_adam", "cpc_adamw", "cpc_adam_clip"} & set(spy.names)
    assert logger.lr_meter.values == oracle[1] and tr.last_optimizer.t == steps
    assert float(tr.last_optimizer.clip_state[1]) < 1.0          # the gradient was clipped
    A._check_against_oracle(context, model, logger.loss_meter.values, oracle[:3])
    _ratios_follow_the_oracle(tr.last_optimizer, oracle[3])
    assert max(v[2] for v in tr.last_optimizer.trust_ratios().values()) == float(np.float32(trust_clip))
    _differs_from_the_run_without_trust_ratio(golden_dir, context, model, oracle[3], max_norm=oracle[4])


def test_generic_route_builds_torch_lamb(golden_dir):
    """A score function the trainer does not recognise takes the generic route: TorchLamb in the place of torch.optim.Adam, no
    _foreach_mul_ decay in front of it, the schedule in group['lr'].  Against the oracle run at the generic route's bounds
    (tests/test_adamw_gpu.py test_generic_route_decays_and_schedules)."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    losses, lrs, o_params, o_trust, _ = _oracle_lamb(golden_dir, "gru")
    steps = len(losses)
    model = build("fp32")
    logger = A._Logger()
    tr = A._trainer(model, data, meta, logger, score_function=lambda p, t: softplus_score_function(p, t))
    assert not tr._fused()
    tr.trust_ratio, tr.weight_decay, tr.lr_schedule = True, WD, A.SCHED
    random.seed(A.SEED)
    with A._Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=A.LR, num_workers=0, max_steps=steps)
    assert not {"cpc_lamb", "cpc_adam", "cpc_adamw"} & set(spy.names)
    assert logger.lr_meter.values == lrs
    for i in range(steps):
        assert abs(logger.loss_meter.values[i] - losses[i]) < 2e-4 * abs(losses[i]), i
    for k, v in model.state_dict().items():
        ref = o_params[k]
        err = (v.cpu() - ref).abs()
        assert err.max().item() <= 2 * sum(lrs) * 1.01 + 1e-6, k
        tight = err <= 0.05 * sum(lrs) + 1e-4 * ref.abs()
        assert tight.float().mean().item() > 0.97, (k, tight.float().mean().item())
    # against the AdamW run of the same route's oracle the selected tensors lie far outside the tight band
    adamw = _oracle_adamw(golden_dir, "gru")
    sd = model.state_dict()
    for k in _scaled_down(o_trust):
        tight = (sd[k].cpu() - adamw[k]).abs() <= 0.05 * sum(lrs) + 1e-4 * adamw[k].abs()
        assert tight.float().mean().item() < 0.5, (k, tight.float().mean().item())


# ------------------------------------------------------------------------------------------ resume
def test_resumed_lamb_run_is_the_uninterrupted_run(golden_dir):
    """Three steps, state_dict(), a fresh model and optimizer with step_offset = 3, three steps more: parameters, m, v and the last
    step's trust array carry the bits of six uninterrupted steps."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    batches = A._batches(data, meta["B"])
    kw = dict(weight_decay=WD, schedule=A.RESUME_SCHED, trust_ratio=True, trust_clip=2.0)
    opt_a, losses_a, lrs_a = A._engine_steps(build("fp32"), data, batches, 6, **kw)
    model_b = build("fp32")
    opt_b, losses_b, _ = A._engine_steps(model_b, data, batches, 3, **kw)
    saved_opt = opt_b.state_dict()
    saved_model = {k: v.detach().clone() for k, v in model_b.state_dict().items()}
    model_c = build("fp32")
    model_c.load_state_dict(saved_model)
    model_c._flatten_parameters(DEV)
    opt_c = FusedAdam(model_c, lr=A.LR, step_offset=3, **kw)
    opt_c.load_state_dict(saved_opt)
    assert opt_c.t == 3
    _, losses_c, lrs_c = A._engine_steps(model_c, data, batches[3:] + batches[:3], 3, optimizer=opt_c)
    assert lrs_c == lrs_a[3:] and losses_b + losses_c == losses_a
    a, c = A._optimizer_bits(opt_a), A._optimizer_bits(opt_c)
    assert a[3] == c[3] == 6
    for x, y, name in zip(a[:3], c[:3], "pmv"):
        assert torch.equal(x, y), name
    assert torch.equal(opt_a.trust, opt_c.trust)


# ------------------------------------------------------------------------------------------ data parallel
def test_update_range_pieces_behind_the_all_reduce_give_the_hook_route_bits(golden_dir):
    """A process group of one rank (RCCL): the pieces GradAllReduce hands to update_range behind their reductions and the head in
    step() give the bits of the single-process hook route, in parameters, moments and ratios."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29655")
    started = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
        started = True
    try:
        meta, data, state, build, _ = A._fixture(golden_dir, "gru")
        x = data[A._batches(data, meta["B"])[0]].to(DEV).contiguous()
        results = []
        for route in ("hook", "all-reduce"):
            model = build("fp32")
            model.train()
            model._flatten_parameters(DEV)
            eng = model.engine(x.shape[0], x.shape[1], DEV)
            opt = FusedAdam(model, lr=A.LR, weight_decay=WD, schedule=A.SCHED, trust_ratio=True)
            opt.after_update = eng.prepare_ahead
            sync = GradAllReduce(model, optimizer=opt) if route == "all-reduce" else None
            with A._Spy() as spy:
                for _ in range(2):
                    eng.loss_and_grads(x, softplus=True, regularization=A.REG, grad_ready_hook=sync.hook if sync else opt.hook)
                    if sync:
                        sync.finish()
                    opt.step(grad_scale=1.0)
            torch.cuda.synchronize()
            assert spy.names.count("cpc_lamb") > 2 and "cpc_adam" not in spy.names
            results.append((spy.names.count("cpc_lamb"), model._flat_param.clone(), opt.m.clone(), opt.v.clone(), opt.trust.clone()))
        assert results[0][0] == results[1][0]
        for a, b, name in zip(results[0][1:], results[1][1:], ("p", "m", "v", "trust")):
            assert torch.equal(a, b), name
    finally:
        if started:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------------------ bf16
def test_bf16_lamb_steps(golden_dir):
    """bf16 storage, three steps: losses and parameters stay finite, and every selected parameter's (w_norm, u_norm, ratio) of the
    last step is the exact-f32 run's within 1e-2 relative — loose by design: the norms of whole tensors barely see the bf16 rounding
    of the activations.  Measured worst case on MI355X: 3.5e-3 (the figure is printed)."""
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    batches = A._batches(data, meta["B"])
    runs = {}
    for dtype in ("fp32", "bf16"):
        model = build(dtype)
        opt, losses, _ = A._engine_steps(model, data, batches, 3, weight_decay=WD, schedule=A.SCHED, trust_ratio=True)
        assert all(math.isfinite(x) for x in losses) and bool(torch.isfinite(model._flat_param).all()), dtype
        runs[dtype] = opt.trust_ratios()
    worst = 0.0
    for name, p in build("fp32").named_parameters():
        if p.dim() >= 2:
            for a, b in zip(runs["bf16"][name], runs["fp32"][name]):
                worst = max(worst, abs(a - b) / abs(b))
    print(f"bf16 against f32, selected parameters: worst relative difference of (w_norm, u_norm, ratio) {worst:.3e}")
    assert worst <= 1e-2, worst


# ------------------------------------------------------------------------------------------ the default step
def test_default_step_is_the_parent_step(golden_dir):
    """With trust_ratio at its default no cpc_lamb* symbol is reached and nothing is allocated for it; losses, parameters and moments
    after two steps are bit-identical to the engine and FusedAdam called without the keyword, as train() called them before it existed."""
    steps = 2
    meta, data, state, build, _ = A._fixture(golden_dir, "gru")
    model = build("fp32")
    logger = A._Logger(lr=False)
    tr = A._trainer(model, data, meta, logger)
    random.seed(A.SEED)
    with A._Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=A.LR, num_workers=0, max_steps=steps)
    torch.cuda.synchronize()
    assert (tr.trust_ratio, tr.trust_clip) == (False, None)
    assert not [n for n in spy.names if n.startswith("cpc_lamb")]
    assert spy.names.count("cpc_nce_loss") == steps and spy.names.count("cpc_adam") > steps          # pieces and the head
    last = tr.last_optimizer
    assert last.trust_ratio is False and last.decay_bits is None and not hasattr(last, "trust") and not hasattr(last, "_lamb_ws")
    model0 = build("fp32")
    model0.train()
    model0._flatten_parameters(DEV)
    opt, losses, _ = A._engine_steps(model0, data, A._batches(data, meta["B"]), steps, optimizer=FusedAdam(model0, lr=A.LR))
    assert logger.loss_meter.values == losses
    for (k, v), (k0, v0) in zip(model.state_dict().items(), model0.state_dict().items()):
        assert k == k0 and torch.equal(v, v0), k
    assert torch.equal(last.m, opt.m) and torch.equal(last.v, opt.v)
