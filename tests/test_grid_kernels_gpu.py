"""GPU unit tests of the "grid" kernels of csrc/scalogram.hip (BatchNorm statistics / finalize / apply and their backward passes,
the fused BatchNorm + residual route, 2-D max pooling, the cropped residual add) against float64 references, at the shapes, types
and edges where their launchers take another branch: bf16 with C % 8 != 0 (generic kernels), float32 inputs on a bf16 engine
(x_f32 / in_f32 / r_f32), the per-position coefficient reload of bn_bwd_apply8_kernel (C/8 not dividing the launch), grid-stride
second trips, more than 192 slabs in bn_finalize_kernel, row phases that leave idle threads (C/8 not dividing 256) or a single phase
(C = 1024), blocks with a short or an empty row range, relu = 0 with y = NULL, pooling with p = 3 / floor extents / one-column
grids / accumulate, and what the kernels must NOT write (pad rows, guard rows, positions outside a crop or outside every window).

Conventions of test_scalogram_kernels_gpu.py: references are computed on the values the device sees (inputs rounded to the storage
type first), every grid a kernel writes is checked for untouched pad rows (zero) and guard rows (a sentinel written before the call).

Two kinds of data.
EXACT data finds indexing faults (a dropped, doubled or misplaced row, a wrong channel): dyadic inputs chosen so that every product
and every partial sum is exactly representable in float32, whatever the summation order or the use of fused multiply-adds.  The tests
assert that premise on the float64 reference itself (representable in float32; sum |term| / resolution < 2^24; a plain float32
torch.sum on the CPU equals the float64 sum) and then assert torch.equal against the float64 reference, rounded once to the output type.
RANDOM data finds arithmetic faults: Gaussian inputs against float64 autograd with derived bounds, none tuned to the kernels:
  element-wise outputs of type T   |got - ref| <= u_T |ref| + 8 * 2^-24 * A      u_bf16 = 2^-8, u_f32 = 2^-22, A = the sum of the absolute
                                   values of the terms of the element's expression (dx: |g k1| + |k2| + |k3| (|x| + |mu|));
                                   where the device computed the batch mean itself (train mode), |mu| is the sum of ITS terms'
                                   absolute values, mean |x|: a channel's mean can cancel to nearly nothing while its rounding
                                   error is set by the summands, which an element with x, mu and beta all near 0 then shows
  slab sums (added in float64)     |got - ref| <= n * 2^-24 * sum |term|         n = rows of the channel (<= 2048 here): the worst case of
                                   recursive summation in any order
  bn_finalize outputs              2 ulp of float32 (the kernel computes in double and rounds once)
The backward apply pass takes the reference's dgamma / dbeta rounded to float32 (what the device would be given), so that its bound
does not inherit the reductions' worst case; the reductions are checked on their own.  ReLU masks are the device's own activation
(a sign flip of a value within rounding of zero is not an error).

Largest observed error as a fraction of its bound on an MI355X (every test prints "[ratio] <group> <value>" before it asserts):
  test_bn_chain_random_against_float64   bn_stats sums 0.12, mean 0.023, rstd 0.045, running statistics 0.063, bn_bwd_reduce 0.044;
                                         bn_apply 0.34 and bn_bwd_apply 0.41 into float32; into bf16 both reach 0.996, which is the
                                         rounding of the output itself (half an ulp of bf16 just above a power of two is 2^-8 relative)
  test_bn_finalize_against_float64       0.25 of the 2 ulp, on all four outputs: half an ulp, correctly rounded
  test_bn_stats_with_a_large_mean        0.013 of n_slab * 2^-24 * mean(x^2).  mean(x^2) / var = 68: the E[x^2] - mean^2 form gives up 1.8 of
                                         float32's 7.2 decimal digits by construction; the observed relative variance error was 3.7e-5 with one
                                         slab of 4096 rows (float32 input) and 6.9e-6 with 32 slabs of 128: 4.4 to 5.2 digits are left
  test_residual_add_and_backward         forward 0.083 into float32, 0.996 into bf16 (the output's own rounding again); the backward asserts equality
  test_bn_chain_exact, test_bn_apply_residual_route_exact, test_maxpool2d_forward_backward, test_grid_stride_second_trips_*,
  test_refusals_write_nothing            assert equality
The whole file (250 cases) takes 5 s on an MI355X: about 1 s for the first case (library load), 0.4 s for the first grid-stride case, a few
hundredths of a second for the other grid-stride cases (their references are torch expressions on the device, see there) and less for the rest.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.scalogram_engine import Grid  # noqa: E402

DEV = torch.device("cuda:0")
F32, BF = torch.float32, torch.bfloat16
SENTINEL = 7.25          # guard rows: exact in bf16 and f32
FILL = -96.0             # pre-fill of valid rows a kernel must leave alone: exact in bf16, beyond every value of the test data
EPS32 = torch.tensor(1e-5, dtype=F32).double().item()          # the eps / momentum the device sees (float arguments)
MOM32 = torch.tensor(0.1, dtype=F32).double().item()
E24 = 2.0 ** -24
U = {BF: 2.0 ** -8, F32: 2.0 ** -22}
L = C.c_longlong


def _d(desc):
    return C.cast(desc, C.c_void_p)


def _code(dt):
    return _hip.dtype_code(dt)


def _tn(dt):
    return "f32" if dt == F32 else "bf16"


def _grid(B, W, H, Cc, dt, top=0, tail=0):
    """A zeroed grid whose guard rows hold SENTINEL."""
    g = Grid(B, W, H, Cc, DEV, dt, top=top, tail=tail, guard_rows=4)
    n = g.guard_rows * Cc
    g.full[:n] = SENTINEL
    g.full[n + g.rows * Cc:] = SENTINEL
    return g


def _view(g):
    return g.t.view(g.B, g.W, g.Ha, g.C)


def _valid(g):
    return _view(g)[:, :, g.top:g.top + g.H, :]


def _fill(g, nchw):
    """NCHW tensor -> valid rows of the grid (rounded to its storage type)."""
    _view(g)[:, :, g.top:g.top + g.H, :] = nchw.permute(0, 3, 2, 1).to(g.dtype).to(DEV)


def _read(g):
    return _view(g)[:, :, g.top:g.top + g.H, :].permute(0, 3, 2, 1).double().cpu()


def _check_frame(g):
    """Pad rows [0, top) and [top + H, Ha) still zero, guard rows still SENTINEL."""
    v = _view(g)
    assert v[:, :, :g.top].abs().max().item() == 0 if g.top else True, "top pad rows written"
    assert v[:, :, g.top + g.H:].abs().max().item() == 0 if g.Ha > g.top + g.H else True, "tail pad rows written"
    n = g.guard_rows * g.C
    assert bool((g.full[:n] == SENTINEL).all()) and bool((g.full[n + g.rows * g.C:] == SENTINEL).all()), "guard rows written"


def _pack_bits(t):
    """Sign bits as the kernels write them: one byte per 8 consecutive elements, bit e = element 8 i + e is > 0."""
    want = (t.float().view(-1, 8) > 0).to(torch.uint8)
    return (want << torch.arange(8, device=t.device, dtype=torch.uint8)).sum(1).to(torch.uint8)


def _within(group, got, ref, bound):
    """max |got - ref| / bound <= 1, the figure printed first (run with -s to collect the module docstring's figures)."""
    got, ref, bound = (torch.as_tensor(t).double().cpu() for t in (got, ref, bound))
    assert bool(torch.isfinite(got).all()), f"{group}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double()).max().item()
    print(f"[ratio] {group} {ratio:.4g}")
    assert ratio <= 1.0, f"{group}: error is {ratio:.3g} of its derived bound"


def _ebound(ref, A, dt):
    return U[dt] * ref.abs() + 8 * E24 * A


def _ulp2(ref):
    """Two units in the last place of float32 at ref (float64 tensor)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return 2 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


def _dyadic(gen, shape, step, lim):
    """Multiples of `step` in [-lim, lim] (float64)."""
    k = int(round(lim / step))
    return torch.randint(-k, k + 1, shape, generator=gen).double() * step


def _choice(gen, n, vals):
    return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (n,), generator=gen)]


def _per_c(t):
    return t.view(1, -1, 1, 1)


def _premise(terms, resolution):
    """The exact-data premise for a per-channel sum of `terms` [B, C, H, W] (float64): every term a multiple of `resolution`, the sum
    representable in float32, sum |term| / resolution < 2^24 (so every partial sum of every order is exact in float32), and a plain
    float32 sum on the CPU equals the float64 sum.  Returns the float64 sums."""
    q = terms / resolution
    assert torch.equal(q, q.round())
    ref = terms.sum((0, 2, 3))
    assert torch.equal(ref.float().double(), ref)
    assert (terms.abs().sum((0, 2, 3)) / resolution).max().item() < 2 ** 24
    assert torch.equal(terms.float().sum((0, 2, 3)).double(), ref)
    return ref


def _f32_exact(t):
    assert torch.equal(t.float().double(), t)
    return t


def _mode(mode):
    """-> (type of x / dx, type of the activation and its gradient, dtype code of the calls, x_f32)"""
    if mode == "f32":
        return F32, F32, _code(F32), 0
    if mode == "bf16":
        return BF, BF, _code(BF), 0
    return F32, BF, _code(BF), 1


# ------------------------------------------------------------------------------------------------ 1. BatchNorm chain
BN_C = [4, 12, 16, 24, 40, 72, 256, 1024]          # generic and 8-wide kernels, C/8 not dividing 256 (24, 40, 72), one row phase (1024 f32)
BN_MODES = ["f32", "bf16", "bf16x"]                 # bf16x: x_f32 = 1 (float32 x / dx grids, bf16 activation)


def _bn_shape(Cc):
    """(B, W, H): rows per channel n = B W H <= 2048; several unrolled trips at small C, a range shorter than one trip at large C."""
    return (2, 5, 150) if Cc <= 16 else (2, 5, 60) if Cc <= 72 else (2, 5, 13) if Cc == 256 else (2, 5, 7)


def _empty_from(total, nb):
    """First block with an empty range when `total` rows / columns are dealt to nb blocks in chunks of ceil(total / nb)."""
    per = -(-total // nb)
    return -(-total // per)


def _stats_slabs(gx, nb):
    slabs = torch.full((nb * 2 * gx.C,), float("nan"), device=DEV)
    _hip.call("cpc_bn_stats", gx.ptr(), _hip.ptr(slabs), gx.rows, gx.C, nb, gx.code)
    s = slabs.view(nb, 2 * gx.C)
    e = _empty_from(gx.rows, nb)
    assert e == nb or bool((s[e:] == 0).all()), "blocks with an empty row range must write zero slabs"
    return s.view(nb, 2, gx.C)


def _bwd_reduce_slabs(gda, ga, gx, stats, relu, nb, xf, code):
    slabs = torch.full((nb * 2 * gx.C,), float("nan"), device=DEV)
    _hip.call("cpc_bn_bwd_reduce", gda.ptr(), ga.ptr() if relu else None, _d(ga.desc), gx.ptr(), _d(gx.desc), _hip.ptr(stats), _hip.ptr(slabs),
              relu, nb, xf, code)
    s = slabs.view(nb, 2 * gx.C)
    e = _empty_from(gx.B * gx.W, nb)
    assert e == nb or bool((s[e:] == 0).all()), "blocks with an empty column range must write zero slabs"
    return s.view(nb, 2, gx.C)


def _bn_random(Cc, mode, relu, train):
    B, W, H = _bn_shape(Cc)
    n = B * W * H
    tx, ta, code, xf = _mode(mode)
    gen = torch.Generator().manual_seed(Cc * 16 + BN_MODES.index(mode) * 4 + relu * 2 + int(train))
    x = (torch.randn(B, Cc, H, W, generator=gen) * 1.5 + 0.3).to(tx).double()
    gamma = (1 + 0.3 * torch.randn(Cc, generator=gen)).float().double().requires_grad_(True)
    beta = (0.2 * torch.randn(Cc, generator=gen)).float().double().requires_grad_(True)
    dy = torch.randn(B, Cc, H, W, generator=gen).to(ta).double()
    gx, ga = _grid(B, W, H, Cc, tx, tail=3), _grid(B, W, H, Cc, ta, top=2)
    _fill(gx, x)
    nbs = [1, 3, B * W, B * W + 5]
    xr = x.clone().requires_grad_(True)
    if train:
        s1, s2, a1 = x.sum((0, 2, 3)), (x * x).sum((0, 2, 3)), x.abs().sum((0, 2, 3))
        for nb in nbs + [gx.rows + 3]:              # the last: one row per block at most, three empty blocks
            slabs = _stats_slabs(gx, nb)
            got = slabs.double().sum(0).cpu()
            _within("bn_stats sum x", got[0], s1, n * E24 * a1)
            _within("bn_stats sum x^2", got[1], s2, n * E24 * s2)
            if nb == 3:
                keep = slabs.clone()
        stats = torch.full((2, Cc), float("nan"), device=DEV)
        rm, rv = (0.1 * torch.randn(Cc, generator=gen)).float(), (1 + 0.5 * torch.rand(Cc, generator=gen)).float()
        d_rm, d_rv = rm.to(DEV), rv.to(DEV)
        _hip.call("cpc_bn_finalize", _hip.ptr(keep), 3, Cc, float(n), 1e-5, 0.1, _hip.ptr(stats), _hip.ptr(d_rm), _hip.ptr(d_rv))
        mean, var = s1 / n, x.var((0, 2, 3), unbiased=False)
        rstd = (var + EPS32).rsqrt()
        # the slab sums' worst case carried through mean = s1 / n, var = s2 / n - mean^2 and rstd = (var + eps)^-1/2 (first order, 1 % for
        # the rest), plus the rounding of each output to float32
        dmean = E24 * a1
        dvar = E24 * (s2 + 2 * mean.abs() * a1)
        assert (dvar / var).max().item() < 1e-2
        _within("bn mean", stats[0], mean, dmean + 2 * E24 * mean.abs())
        _within("bn rstd", stats[1], rstd, 1.01 * 0.5 * rstd ** 3 * dvar + 2 * E24 * rstd)
        _within("bn running mean", d_rm, (1 - MOM32) * rm.double() + MOM32 * mean, MOM32 * dmean + 2 * E24 * (rm.double().abs() + mean.abs()))
        _within("bn running var", d_rv, (1 - MOM32) * rv.double() + MOM32 * var * n / (n - 1),
                MOM32 * dvar * n / (n - 1) + 2 * E24 * (rv.double() + var * n / (n - 1)))
        z = F.batch_norm(xr, None, None, gamma, beta, training=True, eps=EPS32)
    else:
        mean = (0.3 * torch.randn(Cc, generator=gen)).float().double()
        rstd = (0.5 + torch.rand(Cc, generator=gen)).float().double()
        stats = torch.stack([mean, rstd]).float().to(DEV)
        z = F.batch_norm(xr, mean, rstd.pow(-2) - EPS32, gamma, beta, training=False, eps=EPS32)
    d_gamma, d_beta = gamma.detach().float().to(DEV), beta.detach().float().to(DEV)
    gm, bt, mu, rs = (_per_c(t) for t in (gamma.detach(), beta.detach(), mean, rstd))
    # |mean| as a term of an element's expression: a given number in eval mode; in train mode the mean is itself the sum of x_i / n
    # computed on the device, whose terms sum to mean |x| in absolute value (the mean of a channel can cancel to nearly nothing while
    # its rounding error is set by the summands)
    mabs = _per_c(a1 / n) if train else mu.abs()

    _hip.call("cpc_bn_apply", gx.ptr(), _d(gx.desc), ga.ptr(), _d(ga.desc), _hip.ptr(stats), _hip.ptr(d_gamma), _hip.ptr(d_beta), relu, xf, code)
    _check_frame(ga)
    _check_frame(gx)
    y_dev = _read(ga)
    y_ref = torch.relu(z.detach()) if relu else z.detach()
    _within(f"bn_apply -> {_tn(ta)}", y_dev, y_ref, _ebound(y_ref, (x.abs() + mabs) * (rs * gm).abs() + bt.abs(), ta))

    gda = _grid(B, W, H, Cc, ta, top=2)
    _fill(gda, dy)
    g = dy * (y_dev > 0) if relu else dy
    z.backward(g)
    t1, t2 = (g * (x - mu) * rs).abs().sum((0, 2, 3)), g.abs().sum((0, 2, 3))
    for nb in nbs:
        slabs = _bwd_reduce_slabs(gda, ga, gx, stats, relu, nb, xf, code)
        got = slabs.double().sum(0).cpu()
        _within("bn_bwd_reduce dgamma", got[0], gamma.grad, n * E24 * t1)
        _within("bn_bwd_reduce dbeta", got[1], beta.grad, n * E24 * t2)
        if nb == 3:
            keep = slabs.clone()
    dgam, dbet = gamma.grad.float().to(DEV), beta.grad.float().to(DEV)
    gdx = _grid(B, W, H, Cc, tx, tail=3)
    _hip.call("cpc_bn_bwd_apply", gda.ptr(), ga.ptr() if relu else None, _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc), _hip.ptr(stats),
              _hip.ptr(d_gamma), _hip.ptr(dgam), _hip.ptr(dbet), float(n), relu, int(train), xf, code)
    _check_frame(gdx)
    k1 = gm * rs
    k2 = k1 * _per_c(beta.grad) / n if train else torch.zeros_like(k1)
    k3 = k1 * rs * _per_c(gamma.grad) / n if train else torch.zeros_like(k1)
    A = (g * k1).abs() + k2.abs() + k3.abs() * (x.abs() + mabs)
    _within(f"bn_bwd_apply -> {_tn(tx)}", _read(gdx), xr.grad, _ebound(xr.grad, A, tx))
    for gr in (gx, ga, gda):
        _check_frame(gr)

    if mode == "bf16" and Cc % 8 == 0:
        # the sign-bit variants: bit for bit the plain calls
        bits = torch.zeros(ga.rows * Cc // 8, device=DEV, dtype=torch.uint8)
        ga2 = _grid(B, W, H, Cc, ta, top=2)
        _hip.call("cpc_bn_apply_bits", gx.ptr(), _d(gx.desc), ga2.ptr(), _d(ga2.desc), _hip.ptr(stats), _hip.ptr(d_gamma), _hip.ptr(d_beta), relu,
                  _hip.ptr(bits), code)
        assert torch.equal(ga2.full, ga.full)
        assert torch.equal(bits, _pack_bits(ga.t))
        if relu:
            slabs2 = torch.full((3 * 2 * Cc,), float("nan"), device=DEV)
            _hip.call("cpc_bn_bwd_reduce_bits", gda.ptr(), _hip.ptr(bits), _d(ga.desc), gx.ptr(), _d(gx.desc), _hip.ptr(stats), _hip.ptr(slabs2), 3,
                      code)
            assert torch.equal(slabs2.view(3, 2, Cc), keep)
            gdx2 = _grid(B, W, H, Cc, tx, tail=3)
            _hip.call("cpc_bn_bwd_apply_bits", gda.ptr(), _hip.ptr(bits), _d(ga.desc), gx.ptr(), gdx2.ptr(), _d(gx.desc), _hip.ptr(stats),
                      _hip.ptr(d_gamma), _hip.ptr(dgam), _hip.ptr(dbet), float(n), int(train), code)
            assert torch.equal(gdx2.full, gdx.full)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mode", BN_MODES)
@pytest.mark.parametrize("Cc", BN_C)
def test_bn_chain_random_against_float64(Cc, mode, relu):
    """cpc_bn_stats -> cpc_bn_finalize -> cpc_bn_apply and cpc_bn_bwd_reduce -> cpc_bn_bwd_apply, train and eval, on Gaussian data
    against F.batch_norm in float64 and its autograd, with the derived bounds of the module docstring; nblocks 1, 3, B W and B W + 5
    (empty blocks write zero slabs); input and activation grids of different row geometry; relu = 0 passes y = NULL."""
    for train in (True, False):
        _bn_random(Cc, mode, relu, train)


def _bn_exact_data(Cc, seed):
    B, W, H = _bn_shape(Cc)
    gen = torch.Generator().manual_seed(seed)
    d = dict(x=_dyadic(gen, (B, Cc, H, W), 0.5, 2), mean=_dyadic(gen, (Cc,), 0.5, 2), rstd=_choice(gen, Cc, [1.0, 2.0]),
             gamma=_choice(gen, Cc, [0.5, 1.0, 2.0]), beta=_dyadic(gen, (Cc,), 0.25, 1), dy=_dyadic(gen, (B, Cc, H, W), 0.25, 2),
             dgamma=_dyadic(gen, (Cc,), 0.25, 4), dbeta=_dyadic(gen, (Cc,), 0.25, 4), xs=_dyadic(gen, (B, Cc, H, W), 0.25, 4))
    return B, W, H, d


COUNT = 64.0          # the `count` of the exact backward apply: a power of two, so that dbeta / count and dgamma / count stay dyadic


def _dx_exact(d, g, train):
    """dx = k1 g - k2 - k3 (x - mean) with every coefficient, product and sum exact in float32 (multiples of 2^-10 below 16)."""
    gm, rs, mu = _per_c(d["gamma"]), _per_c(d["rstd"]), _per_c(d["mean"])
    k1 = gm * rs
    if not train:
        return _f32_exact(k1 * g)
    k2, k3 = k1 * _per_c(d["dbeta"]) / COUNT, k1 * rs * _per_c(d["dgamma"]) / COUNT
    for t in (k1 * g, k2, k3, k3 * (d["x"] - mu), k1 * g - k2):
        _f32_exact(t)
    return _f32_exact(k1 * g - k2 - k3 * (d["x"] - mu))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mode", BN_MODES)
@pytest.mark.parametrize("Cc", BN_C)
def test_bn_chain_exact(Cc, mode, relu):
    """The same five kernels on exact data (module docstring): torch.equal with the float64 reference for the statistics' and the
    backward reductions' slab sums at every nblocks, for the normalised activation and for dx (train with dyadic dgamma, dbeta and
    count = 64, and eval).  One dropped, doubled or misplaced row, or a channel's coefficient taken from another channel, fails."""
    B, W, H, d = _bn_exact_data(Cc, Cc * 8 + BN_MODES.index(mode) * 2 + relu)
    tx, ta, code, xf = _mode(mode)
    x, mu, rs, gm, bt = d["x"], _per_c(d["mean"]), _per_c(d["rstd"]), _per_c(d["gamma"]), _per_c(d["beta"])
    nbs = [1, 3, B * W, B * W + 5]
    # statistics: x a multiple of 1/4 in [-4, 4], x^2 a multiple of 1/16 up to 16
    s1, s2 = _premise(d["xs"], 0.25), _premise(d["xs"] ** 2, 1.0 / 16)
    gs = _grid(B, W, H, Cc, tx, top=1, tail=2)
    _fill(gs, d["xs"])
    for nb in nbs + [gs.rows + 3]:
        got = _stats_slabs(gs, nb).double().sum(0).cpu()
        assert torch.equal(got[0], s1) and torch.equal(got[1], s2), f"bn_stats, nblocks {nb}"
    # normalisation with given statistics
    gx, ga = _grid(B, W, H, Cc, tx, tail=3), _grid(B, W, H, Cc, ta, top=2)
    _fill(gx, x)
    stats = torch.stack([d["mean"], d["rstd"]]).float().to(DEV)
    d_gamma, d_beta = d["gamma"].float().to(DEV), d["beta"].float().to(DEV)
    pre = _f32_exact((x - mu) * rs * gm + bt)
    out = (torch.relu(pre) if relu else pre).to(ta).double()
    _hip.call("cpc_bn_apply", gx.ptr(), _d(gx.desc), ga.ptr(), _d(ga.desc), _hip.ptr(stats), _hip.ptr(d_gamma), _hip.ptr(d_beta), relu, xf, code)
    _check_frame(ga)
    assert torch.equal(_read(ga), out)
    # backward reductions: g (x - mean) rstd a multiple of 1/8 up to 16, g a multiple of 1/4
    g = d["dy"] * (out > 0) if relu else d["dy"]
    r1, r2 = _premise(g * (x - mu) * rs, 0.125), _premise(g, 0.25)
    gda = _grid(B, W, H, Cc, ta, top=2)
    _fill(gda, d["dy"])
    for nb in nbs:
        got = _bwd_reduce_slabs(gda, ga, gx, stats, relu, nb, xf, code).double().sum(0).cpu()
        assert torch.equal(got[0], r1) and torch.equal(got[1], r2), f"bn_bwd_reduce, nblocks {nb}"
    dgam, dbet = d["dgamma"].float().to(DEV), d["dbeta"].float().to(DEV)
    for train in (1, 0):
        gdx = _grid(B, W, H, Cc, tx, tail=3)
        _hip.call("cpc_bn_bwd_apply", gda.ptr(), ga.ptr() if relu else None, _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc), _hip.ptr(stats),
                  _hip.ptr(d_gamma), _hip.ptr(dgam), _hip.ptr(dbet), COUNT, relu, train, xf, code)
        _check_frame(gdx)
        assert torch.equal(_read(gdx), _dx_exact(d, g, train).to(tx).double()), f"bn_bwd_apply, train {train}"
    for gr in (gs, gx, ga, gda):
        _check_frame(gr)


# ------------------------------------------------------------------------------------------------ 2. bn_finalize alone
def _finalize_ref(s1, s2, count, rm, rv):
    S1, S2 = s1.double().sum(0), s2.double().sum(0)
    mean = S1 / count
    raw = S2 / count - mean * mean
    var = raw.clamp_min(0.0)
    unbiased = var * count / (count - 1) if count > 1 else var
    return mean, raw, (var + EPS32).rsqrt(), (1 - MOM32) * rm.double() + MOM32 * mean, (1 - MOM32) * rv.double() + MOM32 * unbiased


def _finalize_call(slabs, nslab, Cc, count, rm, rv):
    """-> (stats [2][C], run_mean, run_var) with 8 sentinel floats behind each buffer checked."""
    stats = torch.full((2 * Cc + 8,), SENTINEL, device=DEV)
    bufs = [stats]
    if rm is not None:
        bufs += [torch.cat([rm, torch.full((8,), SENTINEL)]).to(DEV), torch.cat([rv, torch.full((8,), SENTINEL)]).to(DEV)]
    running = [None, None] if rm is None else [_hip.ptr(b) for b in bufs[1:]]
    _hip.call("cpc_bn_finalize", _hip.ptr(slabs), nslab, Cc, float(count), 1e-5, 0.1, _hip.ptr(stats), *running)
    for b in bufs:
        assert bool((b[-8:] == SENTINEL).all()), "written past the C channels"
    return [stats[:2 * Cc].view(2, Cc)] + [b[:Cc] for b in bufs[1:]]


@pytest.mark.parametrize("Cc", [4, 16, 20, 1024])
@pytest.mark.parametrize("nslab", [1, 63, 64, 65, 192, 193, 256, 257, 449, 2048])
def test_bn_finalize_against_float64(nslab, Cc):
    """cpc_bn_finalize on synthetic slabs [nslab][2][C] against float64 sums of the same float32 slabs: mean, rstd and torch's running
    update (momentum on the batch mean and the UNBIASED batch variance), with and without the running statistics; nslab on both
    sides of the 64 slab lanes and of the four-loads-per-trip loop (entered above 192); C = 20 masks the last block of 16 channels.
    The kernel computes in double and rounds once: 2 ulp of float32 on every output.  For rstd that needs var + eps not to be a
    cancellation result: asserted as (E[x^2] + mean^2) / (var + eps) <= 2^10 on every channel but the last, whose slabs are built so
    that E[x^2] - mean^2 comes out slightly NEGATIVE and must clamp to 0 (rstd = eps^-1/2, running variance decays)."""
    gen = torch.Generator().manual_seed(nslab * 2048 + Cc)
    cnt = 37                                                   # rows per slab
    count = nslab * cnt
    m = (0.5 + 1.5 * torch.rand(Cc, generator=gen)) * (torch.randint(0, 2, (Cc,), generator=gen) * 2 - 1)
    sd = 0.5 + torch.rand(Cc, generator=gen)
    s1 = (cnt * (m + 0.3 * sd * torch.randn(nslab, Cc, generator=gen))).float()
    s2 = (cnt * (sd * sd + (s1.double() / cnt) ** 2) * (1 + 0.1 * torch.rand(nslab, Cc, generator=gen))).float()     # var >= sd^2 > 0
    s1[:, -1] = cnt * 1.25                                     # exact;  cnt * 1.25^2 = 57.8125 is exact too: one ulp less per slab
    s2[:, -1] = torch.nextafter(torch.tensor(cnt * 1.5625, dtype=F32), torch.tensor(0.0))
    rm, rv = (0.2 * torch.randn(Cc, generator=gen)).float(), (0.5 + torch.rand(Cc, generator=gen)).float()
    mean, raw, rstd, rm_new, rv_new = _finalize_ref(s1, s2, count, rm, rv)
    assert raw[-1].item() < 0 and abs(rstd[-1].item() - EPS32 ** -0.5) < 1e-9
    cond = (s2.double().sum(0) / count + mean * mean) / (raw + EPS32)
    assert cond[:-1].max().item() <= 2 ** 10 and raw[:-1].min().item() > 0
    assert (s1.double().abs().sum(0) / s1.double().sum(0).abs()).max().item() <= 2 ** 10        # nor is the mean a cancellation result
    slabs = torch.stack([s1, s2], 1).contiguous().to(DEV)     # [nslab][2][C]
    stats, d_rm, d_rv = _finalize_call(slabs, nslab, Cc, count, rm, rv)
    _within("finalize mean", stats[0], mean, _ulp2(mean))
    _within("finalize rstd", stats[1], rstd, _ulp2(rstd))
    _within("finalize running mean", d_rm, rm_new, _ulp2(rm_new))
    _within("finalize running var", d_rv, rv_new, _ulp2(rv_new))
    stats2, = _finalize_call(slabs, nslab, Cc, count, None, None)
    assert torch.equal(stats2, stats)


def test_bn_finalize_with_a_count_of_one():
    """count = 1: the variance is exactly 0 on dyadic data (x^2 exact), rstd = eps^-1/2, and the running variance takes the biased
    value (torch divides by count - 1 only above 1)."""
    Cc = 20
    gen = torch.Generator().manual_seed(1)
    xv = _dyadic(gen, (1, Cc), 0.25, 4).float()
    rm, rv = (0.2 * torch.randn(Cc, generator=gen)).float(), (0.5 + torch.rand(Cc, generator=gen)).float()
    mean, raw, rstd, rm_new, rv_new = _finalize_ref(xv, xv * xv, 1, rm, rv)
    assert bool((raw == 0).all())
    stats, d_rm, d_rv = _finalize_call(torch.stack([xv, xv * xv], 1).contiguous().to(DEV), 1, Cc, 1, rm, rv)
    assert torch.equal(stats[0].double().cpu(), mean)
    _within("finalize rstd, count 1", stats[1], rstd, _ulp2(rstd))
    _within("finalize running mean, count 1", d_rm, rm_new, _ulp2(rm_new))
    _within("finalize running var, count 1", d_rv, rv_new, _ulp2(rv_new))


# ------------------------------------------------------------------------------------------------ 3. statistics with a large mean
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", [16, 12])
def test_bn_stats_with_a_large_mean(Cc, dt):
    """mean = 8 sigma, 4096 rows per channel: where var = E[x^2] - mean^2 loses digits (mean(x^2) / var = 65, 1.8 decimal digits of
    float32's 7.2).  The variance from the finalized statistics against float64 within n_slab * 2^-24 * mean(x^2), n_slab the rows one
    slab covers (one slab of 4096 rows, and 32 slabs of 128)."""
    B, W, H = 2, 8, 256
    n = B * W * H
    gen = torch.Generator().manual_seed(Cc)
    x = (8 + torch.randn(B, Cc, H, W, generator=gen)).to(dt).double()
    gx = _grid(B, W, H, Cc, dt)
    _fill(gx, x)
    var, ex2 = x.var((0, 2, 3), unbiased=False), (x * x).mean((0, 2, 3))
    for nb in (1, 32):
        assert gx.rows % nb == 0
        slabs = _stats_slabs(gx, nb)
        stats, = _finalize_call(slabs.contiguous(), nb, Cc, n, None, None)
        got = stats[1].double().cpu().pow(-2) - EPS32
        print(f"[digits] C {Cc} {dt} nblocks {nb}: mean(x^2) / var = {(ex2 / var).max().item():.1f}, "
              f"relative variance error {((got - var).abs() / var).max().item():.3g}")
        _within("large-mean variance", got, var, (n // nb) * E24 * ex2)


# ------------------------------------------------------------------------------------------------ 4. fused BatchNorm + residual route
@pytest.mark.parametrize("off", [(0, 0), (2, 1)], ids=["origin", "corner"])
@pytest.mark.parametrize("r_f32", [0, 1])
@pytest.mark.parametrize("relu_out", [0, 1])
@pytest.mark.parametrize("Cc", [16, 24, 72])
def test_bn_apply_residual_route_exact(Cc, relu_out, r_f32, off):
    """cpc_bn_apply_residual / cpc_bn_bwd_reduce_res / cpc_bn_bwd_apply_res on exact data against float64
    act_out(bf16(relu(BN(x))) + crop(res)) and its autograd gradients (dgamma, dbeta as slab sums, dx of the eval form, dres inside the
    crop), plus dx of the train form with dyadic dgamma / dbeta / count; obits and dres NULL and not; the crop at the origin of a larger
    residual grid and in its far corner (oh + H = Hr, ow + W = Wr); dres outside the crop keeps its pre-fill."""
    B, W, H, d = _bn_exact_data(Cc, Cc * 8 + relu_out * 4 + r_f32 * 2 + (off[0] > 0))
    oh, ow = off
    Hr, Wr = (H + oh, W + ow) if oh else (H + 1, W + 2)
    code, tr = _code(BF), F32 if r_f32 else BF
    gen = torch.Generator().manual_seed(Cc + 1000)
    res = _dyadic(gen, (B, Cc, Hr, Wr), 0.25, 2)
    mu, rs = _per_c(d["mean"]), _per_c(d["rstd"])
    xr, gam, bet, rr = (t.clone().requires_grad_(True) for t in (d["x"], d["gamma"], d["beta"], res))
    a = torch.relu((xr - mu) * rs * _per_c(gam) + _per_c(bet))
    assert torch.equal(a.detach().to(BF).double(), a.detach())          # the branch's rounding to bf16 is the identity on this data
    s = a + rr[:, :, oh:oh + H, ow:ow + W]
    out = torch.relu(s) if relu_out else s
    assert torch.equal(out.detach().to(BF).double(), out.detach())
    out.backward(d["dy"])

    gx, ga = _grid(B, W, H, Cc, BF, tail=3), _grid(B, W, H, Cc, BF, top=1)
    gr, go = _grid(B, Wr, Hr, Cc, tr, tail=1), _grid(B, W, H, Cc, BF, top=2, tail=1)
    _fill(gx, d["x"])
    _fill(gr, res)
    _fill(ga, a.detach())                                                # only to form the expected sign bits: the fused route never stores it
    abits_ref = _pack_bits(ga.t)
    stats = torch.stack([d["mean"], d["rstd"]]).float().to(DEV)
    d_gamma, d_beta = d["gamma"].float().to(DEV), d["beta"].float().to(DEV)
    for with_obits in (False, True):
        go = _grid(B, W, H, Cc, BF, top=2, tail=1)
        bits = torch.zeros(ga.rows * Cc // 8, device=DEV, dtype=torch.uint8)
        obits = torch.zeros(go.rows * Cc // 8, device=DEV, dtype=torch.uint8)
        _hip.call("cpc_bn_apply_residual", gx.ptr(), _d(gx.desc), gr.ptr(), _d(gr.desc), go.ptr(), _d(go.desc), _hip.ptr(stats), _hip.ptr(d_gamma),
                  _hip.ptr(d_beta), oh, ow, 1, relu_out, r_f32, _hip.ptr(bits), _d(ga.desc), _hip.ptr(obits) if with_obits else None, code)
        _check_frame(go)
        _check_frame(gr)
        assert torch.equal(_read(go), out.detach())
        assert torch.equal(bits, abits_ref)
        assert torch.equal(obits, _pack_bits(go.t) if with_obits else torch.zeros_like(obits))

    # backward: g = dout [out > 0] [bn_out > 0]
    ob = _hip.ptr(obits) if relu_out else None
    g = d["dy"] * (a.detach() > 0) * ((out.detach() > 0) if relu_out else 1)
    r1, r2 = _premise(g * (d["x"] - mu) * rs, 0.125), _premise(g, 0.25)
    assert torch.equal(gam.grad, r1) and torch.equal(bet.grad, r2)       # autograd's sums are exact in float64 as well
    gdo = _grid(B, W, H, Cc, BF, top=2, tail=1)
    _fill(gdo, d["dy"])
    for nb in (1, 3, B * W, B * W + 5):
        slabs = torch.full((nb * 2 * Cc,), float("nan"), device=DEV)
        _hip.call("cpc_bn_bwd_reduce_res", gdo.ptr(), _d(gdo.desc), ob, _hip.ptr(bits), _d(ga.desc), gx.ptr(), _d(gx.desc), _hip.ptr(stats),
                  _hip.ptr(slabs), nb, code)
        got = slabs.view(nb, 2, Cc).double().sum(0).cpu()
        assert torch.equal(got[0], r1) and torch.equal(got[1], r2), f"bn_bwd_reduce_res, nblocks {nb}"
        assert nb <= B * W or bool((slabs.view(nb, -1)[B * W:] == 0).all())
    dgam, dbet = d["dgamma"].float().to(DEV), d["dbeta"].float().to(DEV)
    assert torch.equal(xr.grad, _dx_exact(d, g, 0))
    for with_dres in ((False,) if r_f32 else (False, True)):             # (dres is a bf16 grid: the float32 residual's gradient is not written here)
        for train in (1, 0):
            gdx = _grid(B, W, H, Cc, BF, tail=3)
            gdr = _grid(B, Wr, Hr, Cc, BF, tail=1)
            _valid(gdr).fill_(FILL)
            _hip.call("cpc_bn_bwd_apply_res", gdo.ptr(), _d(gdo.desc), ob, _hip.ptr(bits), _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc),
                      _hip.ptr(stats), _hip.ptr(d_gamma), _hip.ptr(dgam), _hip.ptr(dbet), COUNT, train, gdr.ptr() if with_dres else None,
                      _d(gdr.desc) if with_dres else None, oh, ow, code)
            _check_frame(gdx)
            _check_frame(gdr)
            assert torch.equal(_read(gdx), _dx_exact(d, g, train).to(BF).double()), f"bn_bwd_apply_res, train {train}"
            want = torch.full((B, Cc, Hr, Wr), FILL, dtype=torch.float64)
            if with_dres:
                want[:, :, oh:oh + H, ow:ow + W] = rr.grad[:, :, oh:oh + H, ow:ow + W]
            assert torch.equal(_read(gdr), want), "dres: the crop holds dout [out > 0], everything else is left alone"
    for gr_ in (gx, ga, gdo):
        _check_frame(gr_)


# ------------------------------------------------------------------------------------------------ 5. max pooling
def _pool_extents(H, W, p, ceil):
    """Output extents per axis: ceil mode, or floor mode where that leaves at least one window (a one-column grid is pooled with the
    window clipped to the column, as the ConvolutionalArModel path does)."""
    ext = lambda s: -(-s // p) if (ceil or s // p == 0) else s // p          # noqa: E731
    return ext(H), ext(W)


def _windows(t, p, Ho, Wo, fill):
    """[B, C, H, W] -> [B, C, Ho, Wo, p p] windows, dh outer and dw inner; clipped windows padded with `fill`, a floor-mode remainder dropped."""
    B, Cc, H, W = t.shape
    tp = torch.full((B, Cc, Ho * p, Wo * p), fill, dtype=t.dtype)
    hh, ww = min(H, Ho * p), min(W, Wo * p)
    tp[:, :, :hh, :ww] = t[:, :, :hh, :ww]
    return tp.view(B, Cc, Ho, p, Wo, p).permute(0, 1, 2, 4, 3, 5).reshape(B, Cc, Ho, Wo, p * p)


def _first_max_scatter(x, dout, p, Ho, Wo):
    """The contract of cpc_maxpool2d_bwd: dout goes to the FIRST maximum of its window in (dh outer, dw inner) order, every other
    covered position gets 0.  -> (gradient [B, C, H, W], covered [H, W])"""
    B, Cc, H, W = x.shape
    win = _windows(x, p, Ho, Wo, float("-inf"))
    eq = win == win.max(-1, keepdim=True).values
    first = eq & (eq.cumsum(-1) == 1)
    sc = first.double() * dout.unsqueeze(-1)
    full = sc.view(B, Cc, Ho, Wo, p, p).permute(0, 1, 2, 4, 3, 5).reshape(B, Cc, Ho * p, Wo * p)
    hh, ww = min(H, Ho * p), min(W, Wo * p)
    grad = torch.zeros(B, Cc, H, W, dtype=torch.float64)
    grad[:, :, :hh, :ww] = full[:, :, :hh, :ww]
    covered = torch.zeros(H, W, dtype=torch.bool)
    covered[:hh, :ww] = True
    return grad, covered


# (name, type of the input, type of the output, C, in_f32): f32; bf16 8-wide; bf16 generic; float32 input on a bf16 engine (forward only)
POOL_KINDS = [("f32", F32, F32, 6, 0), ("bf16-c8", BF, BF, 8, 0), ("bf16-c12", BF, BF, 12, 0), ("in_f32", F32, BF, 8, 1)]


@pytest.mark.parametrize("size", [(7, 9), (6, 6), (5, 1), (1, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ceil", [True, False], ids=["ceil", "floor"])
@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("kind", POOL_KINDS, ids=lambda k: k[0])
def test_maxpool2d_forward_backward(kind, p, ceil, size):
    """cpc_maxpool2d_fwd equals F.max_pool2d on Gaussian and on tie-laden data; cpc_maxpool2d_bwd on tie-laden data (three bf16-exact
    values) equals the first-maximum scatter: with accumulate = 0 on a pre-filled din every covered position holds its gradient or 0 and
    a floor-mode remainder keeps the pre-fill; with accumulate = 1 din ends as old + scatter, one rounding of the float32 sum."""
    _, ti, to, Cc, in_f32 = kind
    H, W = size
    B = 2
    Ho, Wo = _pool_extents(H, W, p, ceil)
    hh, ww = min(H, Ho * p), min(W, Wo * p)
    code = _code(to)
    gen = torch.Generator().manual_seed(p * 100 + H * 10 + W + int(ceil))
    ties = (torch.randint(0, 3, (B, Cc, H, W), generator=gen) * 0.5 - 0.5).double()
    for x in (torch.randn(B, Cc, H, W, generator=gen).to(ti).double(), ties):
        gi, go = _grid(B, W, H, Cc, ti, top=1), _grid(B, Wo, Ho, Cc, to, top=1, tail=1)
        _fill(gi, x)
        _hip.call("cpc_maxpool2d_fwd", gi.ptr(), _d(gi.desc), go.ptr(), _d(go.desc), p, in_f32, code)
        _check_frame(go)
        _check_frame(gi)
        assert torch.equal(_read(go), F.max_pool2d(x[:, :, :hh, :ww], p, ceil_mode=True).to(to).double())
    if in_f32:
        return
    dout = torch.randn(B, Cc, Ho, Wo, generator=gen).to(to).double()
    old = torch.randn(B, Cc, H, W, generator=gen).to(to)
    grad, covered = _first_max_scatter(ties, dout, p, Ho, Wo)
    assert bool(covered.all()) == (hh == H and ww == W)
    gdo = _grid(B, Wo, Ho, Cc, to, top=1, tail=1)
    _fill(gdo, dout)
    # accumulate = 0: exactly the covered positions are written
    gdi = _grid(B, W, H, Cc, to, top=1)
    _valid(gdi).fill_(FILL)
    _hip.call("cpc_maxpool2d_bwd", gi.ptr(), gdi.ptr(), _d(gi.desc), gdo.ptr(), _d(go.desc), p, 0, code)
    _check_frame(gdi)
    assert torch.equal(_read(gdi), torch.where(covered, grad, torch.full_like(grad, FILL)))
    # accumulate = 1
    _fill(gdi, old)
    _hip.call("cpc_maxpool2d_bwd", gi.ptr(), gdi.ptr(), _d(gi.desc), gdo.ptr(), _d(go.desc), p, 1, code)
    _check_frame(gdi)
    assert torch.equal(_read(gdi), (old.float() + grad.float()).to(to).double())
    for gr in (gi, gdo):
        _check_frame(gr)


# ------------------------------------------------------------------------------------------------ 6. cropped residual add
# (name, storage type, C, r_f32)
RES_KINDS = [("f32", F32, 12, 0), ("bf16-c8", BF, 8, 0), ("bf16-c12", BF, 12, 0), ("bf16-r_f32", BF, 8, 1)]


@pytest.mark.parametrize("corner", [False, True], ids=["inside", "corner"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", RES_KINDS, ids=lambda k: k[0])
def test_residual_add_and_backward(kind, relu, corner):
    """cpc_residual_add against float64 within the element-wise bound; cpc_residual_add_bwd copies or zeroes: torch.equal, on an
    activation that also holds exact +0 and -0 (both mask under ReLU), da and the crop of dr; dr outside the crop keeps its pre-fill.
    The crop strictly inside the residual grid, and in its far corner (oh + H = Hr, ow + W = Wr)."""
    _, dt, Cc, r_f32 = kind
    tr = F32 if r_f32 else dt
    code = _code(dt)
    B, W, H, Wr, Hr = 2, 5, 7, 8, 10
    oh, ow = (Hr - H, Wr - W) if corner else (1, 2)
    gen = torch.Generator().manual_seed(Cc * 4 + relu * 2 + int(corner))
    a = torch.randn(B, Cc, H, W, generator=gen).to(dt).double()
    r = torch.randn(B, Cc, Hr, Wr, generator=gen).to(tr).double()
    ga, gr, go = _grid(B, W, H, Cc, dt, top=1), _grid(B, Wr, Hr, Cc, tr, tail=2), _grid(B, W, H, Cc, dt, top=2, tail=1)
    _fill(ga, a)
    _fill(gr, r)
    _hip.call("cpc_residual_add", ga.ptr(), _d(ga.desc), gr.ptr(), _d(gr.desc), go.ptr(), _d(go.desc), oh, ow, relu, r_f32, code)
    for g_ in (ga, gr, go):
        _check_frame(g_)
    rc = r[:, :, oh:oh + H, ow:ow + W]
    ref = torch.relu(a + rc) if relu else a + rc
    _within(f"residual_add -> {_tn(dt)}", _read(go), ref, _ebound(ref, a.abs() + rc.abs(), dt))

    # backward on the device's activation with exact zeros of both signs planted
    v = _valid(go)
    v[:, 0::2, 1::3, 0] = 0.0
    v[:, 1::2, 2::3, 1] = -0.0
    out = _read(go)
    dout = torch.randn(B, Cc, H, W, generator=gen).to(dt).double()
    gdo, gda, gdr = _grid(B, W, H, Cc, dt, top=2, tail=1), _grid(B, W, H, Cc, dt, top=1), _grid(B, Wr, Hr, Cc, tr, tail=2)
    _fill(gdo, dout)
    _valid(gdr).fill_(FILL)
    _hip.call("cpc_residual_add_bwd", gdo.ptr(), go.ptr() if relu else None, _d(go.desc), gda.ptr(), _d(gda.desc), gdr.ptr(), _d(gdr.desc), oh, ow,
              relu, r_f32, code)
    for g_ in (gda, gdr, gdo, go):
        _check_frame(g_)
    g = torch.where(out > 0, dout, torch.zeros_like(dout)) if relu else dout
    assert torch.equal(_read(gda), g)
    want = torch.full((B, Cc, Hr, Wr), FILL, dtype=torch.float64)
    want[:, :, oh:oh + H, ow:ow + W] = g
    assert torch.equal(_read(gdr), want)


# ------------------------------------------------------------------------------------------------ 7. grid-stride second trips
def _gdyadic(gen, shape, step, lim, dtype=torch.float64):
    k = int(round(lim / step))
    return torch.randint(-k, k + 1, shape, generator=gen, device=DEV).to(dtype) * step


def _vfill(g, bwhc):
    _valid(g).copy_(bwhc)


def _gstride_data(Cc):
    """Exact data in grid layout [B][W][H][C] on the device, with more than 8192 * 256 eight-channel positions: every thread of the
    capped launch makes a second trip, a last partial one included.  C = 16: the launch is a multiple of C/8 (coefficients preloaded);
    C = 24: it is not (coefficients reloaded per position)."""
    B, W, H = (2, 700, 750) if Cc == 16 else (2, 700, 500)
    assert B * W * H * (Cc // 8) > 8192 * 256 and ((8192 * 256) % (Cc // 8) == 0) == (Cc == 16)
    gen = torch.Generator(device=DEV).manual_seed(Cc)
    d = dict(x=_gdyadic(gen, (B, W, H, Cc), 0.5, 2), dy=_gdyadic(gen, (B, W, H, Cc), 0.25, 2), mean=_gdyadic(gen, (Cc,), 0.5, 2),
             rstd=torch.randint(1, 3, (Cc,), generator=gen, device=DEV).double(), gamma=torch.pow(2.0, _gdyadic(gen, (Cc,), 1, 1)), beta=_gdyadic(gen, (Cc,), 0.25, 1),
             dgamma=_gdyadic(gen, (Cc,), 0.25, 4), dbeta=_gdyadic(gen, (Cc,), 0.25, 4))
    return B, W, H, d


def _gdx(d, g):
    k1 = d["gamma"] * d["rstd"]
    k2, k3 = k1 * d["dbeta"] / COUNT, k1 * d["rstd"] * d["dgamma"] / COUNT
    want = k1 * g - k2 - k3 * (d["x"] - d["mean"])
    assert torch.equal(want.float().double(), want)
    return want.to(BF)


@pytest.mark.parametrize("Cc", [16, 24])
def test_grid_stride_second_trips_batchnorm_and_residual(Cc):
    """cpc_bn_apply, cpc_bn_bwd_apply, cpc_bn_apply_residual + cpc_bn_bwd_apply_res and cpc_residual_add (+ backward) once each on
    bf16 grids with more positions than the 8192 x 256 threads of the capped launch, exact data, torch.equal.  The reference is the
    same float64 expression as in the small tests, evaluated by torch on the device (IEEE float64, exact on this data wherever it
    runs): the grids hold 16.8 M elements and the CPU would take several seconds per kernel."""
    B, W, H, d = _gstride_data(Cc)
    code = _code(BF)
    x, mu, rs, gm, bt = d["x"], d["mean"], d["rstd"], d["gamma"], d["beta"]
    stats = torch.stack([mu, rs]).float()
    d_gamma, d_beta, dgam, dbet = gm.float(), bt.float(), d["dgamma"].float(), d["dbeta"].float()
    gx, ga, gda = _grid(B, W, H, Cc, BF, tail=1), _grid(B, W, H, Cc, BF, top=1), _grid(B, W, H, Cc, BF, top=1)
    _vfill(gx, x)
    _vfill(gda, d["dy"])
    a = torch.relu((x - mu) * rs * gm + bt)
    assert torch.equal(a.to(BF).double(), a)
    _hip.call("cpc_bn_apply", gx.ptr(), _d(gx.desc), ga.ptr(), _d(ga.desc), _hip.ptr(stats), _hip.ptr(d_gamma), _hip.ptr(d_beta), 1, 0, code)
    _check_frame(ga)
    assert torch.equal(_valid(ga), a.to(BF))
    gdx = _grid(B, W, H, Cc, BF, tail=1)
    _hip.call("cpc_bn_bwd_apply", gda.ptr(), ga.ptr(), _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc), _hip.ptr(stats), _hip.ptr(d_gamma),
              _hip.ptr(dgam), _hip.ptr(dbet), COUNT, 1, 1, 0, code)
    _check_frame(gdx)
    assert torch.equal(_valid(gdx), _gdx(d, d["dy"] * (a > 0)))
    del gdx

    # the fused residual route and the two-pass residual add on the same operands: crop at (oh, ow) = (1, 2) of a larger grid
    oh, ow = 1, 2
    gen = torch.Generator(device=DEV).manual_seed(Cc + 1)
    res = _gdyadic(gen, (B, W + ow, H + oh + 1, Cc), 0.25, 2)
    gr, go = _grid(B, W + ow, H + oh + 1, Cc, BF), _grid(B, W, H, Cc, BF, top=2)
    _vfill(gr, res)
    out = torch.relu(a + res[:, ow:ow + W, oh:oh + H, :])
    assert torch.equal(out.to(BF).double(), out)
    bits = torch.zeros(ga.rows * Cc // 8, device=DEV, dtype=torch.uint8)
    obits = torch.zeros(go.rows * Cc // 8, device=DEV, dtype=torch.uint8)
    _hip.call("cpc_bn_apply_residual", gx.ptr(), _d(gx.desc), gr.ptr(), _d(gr.desc), go.ptr(), _d(go.desc), _hip.ptr(stats), _hip.ptr(d_gamma),
              _hip.ptr(d_beta), oh, ow, 1, 1, 0, _hip.ptr(bits), _d(ga.desc), _hip.ptr(obits), code)
    _check_frame(go)
    assert torch.equal(_valid(go), out.to(BF))
    assert torch.equal(bits, _pack_bits(ga.t)) and torch.equal(obits, _pack_bits(go.t))
    go2 = _grid(B, W, H, Cc, BF, top=2)
    _hip.call("cpc_residual_add", ga.ptr(), _d(ga.desc), gr.ptr(), _d(gr.desc), go2.ptr(), _d(go2.desc), oh, ow, 1, 0, code)
    _check_frame(go2)
    assert torch.equal(go2.full, go.full)
    del go2
    gout = d["dy"] * (out > 0)                                            # dout [out > 0]: da of the two-pass route, dres of both
    gdr_want = torch.zeros_like(res)
    gdr_want[:, ow:ow + W, oh:oh + H, :] = gout
    del gda
    gdo = _grid(B, W, H, Cc, BF, top=2)                                   # dout on the output grid's geometry: obits are addressed like it
    _vfill(gdo, d["dy"])
    gdx, gdr = _grid(B, W, H, Cc, BF, tail=1), _grid(B, W + ow, H + oh + 1, Cc, BF)
    _hip.call("cpc_bn_bwd_apply_res", gdo.ptr(), _d(gdo.desc), _hip.ptr(obits), _hip.ptr(bits), _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc),
              _hip.ptr(stats), _hip.ptr(d_gamma), _hip.ptr(dgam), _hip.ptr(dbet), COUNT, 1, gdr.ptr(), _d(gdr.desc), oh, ow, code)
    _check_frame(gdx)
    _check_frame(gdr)
    assert torch.equal(_valid(gdx), _gdx(d, gout * (a > 0)))
    assert torch.equal(_valid(gdr), gdr_want.to(BF))
    del gdx
    gdm, gdr2 = _grid(B, W, H, Cc, BF, top=1), _grid(B, W + ow, H + oh + 1, Cc, BF)
    _hip.call("cpc_residual_add_bwd", gdo.ptr(), go.ptr(), _d(go.desc), gdm.ptr(), _d(gdm.desc), gdr2.ptr(), _d(gdr2.desc), oh, ow, 1, 0, code)
    _check_frame(gdm)
    _check_frame(gdr2)
    assert torch.equal(_valid(gdm), gout.to(BF))
    assert torch.equal(gdr2.full, gdr.full)


@pytest.mark.parametrize("Cc", [16, 24])
def test_grid_stride_second_trips_maxpool(Cc):
    """cpc_maxpool2d_fwd / _bwd (p = 2, 8-wide bf16 kernels) with more than 8192 x 256 eight-channel OUTPUT positions, tie-laden data,
    torch.equal with the first-maximum scatter.  The reference runs in float32 on the device: the data are three bf16-exact values and
    the gradient is copied, so float32 is exact; accumulate = 1 adds in float32 and rounds once, as the kernel does."""
    B, Wo, Ho = (2, 700, 750) if Cc == 16 else (2, 700, 500)
    assert B * Wo * Ho * (Cc // 8) > 8192 * 256
    p, code = 2, _code(BF)
    gen = torch.Generator(device=DEV).manual_seed(Cc + 2)
    x = torch.randint(0, 3, (B, Wo * p, Ho * p, Cc), generator=gen, device=DEV).float() * 0.5 - 0.5
    dout = _gdyadic(gen, (B, Wo, Ho, Cc), 0.25, 2, F32)
    old = _gdyadic(gen, (B, Wo * p, Ho * p, Cc), 0.25, 2, F32)
    gi, go = _grid(B, Wo * p, Ho * p, Cc, BF, top=1), _grid(B, Wo, Ho, Cc, BF, tail=1)
    _vfill(gi, x)
    win = x.view(B, Wo, p, Ho, p, Cc).permute(0, 1, 3, 5, 4, 2).reshape(B, Wo, Ho, Cc, p * p)          # [.., dh p + dw]
    del x
    m = win.max(-1).values
    _hip.call("cpc_maxpool2d_fwd", gi.ptr(), _d(gi.desc), go.ptr(), _d(go.desc), p, 0, code)
    _check_frame(go)
    assert torch.equal(_valid(go), m.to(BF))
    eq = win == m.unsqueeze(-1)
    del win, m
    first = eq & (eq.cumsum(-1, dtype=torch.int32) == 1)
    del eq
    grad = (first.float() * dout.unsqueeze(-1)).view(B, Wo, Ho, Cc, p, p).permute(0, 1, 5, 2, 4, 3).reshape(B, Wo * p, Ho * p, Cc)
    del first
    gdo, gdi = _grid(B, Wo, Ho, Cc, BF, tail=1), _grid(B, Wo * p, Ho * p, Cc, BF, top=1)
    _vfill(gdo, dout)
    _valid(gdi).fill_(FILL)
    _hip.call("cpc_maxpool2d_bwd", gi.ptr(), gdi.ptr(), _d(gi.desc), gdo.ptr(), _d(go.desc), p, 0, code)
    _check_frame(gdi)
    assert torch.equal(_valid(gdi), grad.to(BF))
    _vfill(gdi, old)
    _hip.call("cpc_maxpool2d_bwd", gi.ptr(), gdi.ptr(), _d(gi.desc), gdo.ptr(), _d(go.desc), p, 1, code)
    _check_frame(gdi)
    assert torch.equal(_valid(gdi), (old + grad).to(BF))


# ------------------------------------------------------------------------------------------------ 8. refusals
def _refused(name, *args, outputs):
    """The call raises HipCallError and leaves every output buffer (pre-filled with FILL) as it was."""
    for o in outputs:
        o.fill_(FILL)
    with pytest.raises(_hip.HipCallError):
        _hip.call(name, *args)
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == FILL).all()), f"{name} wrote before refusing"


def test_refusals_write_nothing():
    """Arguments the launchers must refuse (CPC_EINVAL -> HipCallError) without writing: C not a multiple of 4, C above 1024 for the
    reductions (their shared-memory layout ends there; the apply passes take any multiple of 4), the sign-bit calls on float32 grids
    (an x_f32 engine's first stage) or with C = 12, nblocks = 0, pooling extents that are neither ceil nor floor, a crop that leaves
    the residual grid, cpc_bn_finalize with one of the two running-statistic pointers."""
    B, W, H = 2, 3, 5
    p = _hip.ptr

    def bn_args(Cc, tx=BF, ta=BF):
        gx, ga, gda, gdx = (_grid(B, W, H, Cc, t) for t in (tx, ta, ta, tx))
        v = {k: torch.ones(Cc, device=DEV) for k in ("gamma", "beta", "dgamma", "dbeta")}
        return gx, ga, gda, gdx, torch.ones(2, Cc, device=DEV), v

    for Cc in (6, 1028):
        gx, ga, gda, gdx, stats, v = bn_args(Cc)
        slabs = torch.empty(3 * 2 * Cc, device=DEV)
        _refused("cpc_bn_stats", gx.ptr(), p(slabs), gx.rows, Cc, 3, _code(BF), outputs=[slabs])
        _refused("cpc_bn_bwd_reduce", gda.ptr(), ga.ptr(), _d(ga.desc), gx.ptr(), _d(gx.desc), p(stats), p(slabs), 1, 3, 0, _code(BF), outputs=[slabs])
        if Cc % 4:
            _refused("cpc_bn_apply", gx.ptr(), _d(gx.desc), ga.ptr(), _d(ga.desc), p(stats), p(v["gamma"]), p(v["beta"]), 1, 0, _code(BF),
                     outputs=[ga.full])
            _refused("cpc_bn_bwd_apply", gda.ptr(), ga.ptr(), _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc), p(stats), p(v["gamma"]), p(v["dgamma"]),
                     p(v["dbeta"]), 15.0, 1, 1, 0, _code(BF), outputs=[gdx.full])
    # the sign-bit calls: bf16 grids with C a multiple of 8 only
    for Cc, dt in ((16, F32), (12, BF)):
        gx, ga, gda, gdx, stats, v = bn_args(Cc, dt, dt)
        bits = torch.zeros(ga.rows * Cc // 8 + 8, device=DEV, dtype=torch.uint8)
        slabs = torch.empty(3 * 2 * Cc, device=DEV)
        _refused("cpc_bn_apply_bits", gx.ptr(), _d(gx.desc), ga.ptr(), _d(ga.desc), p(stats), p(v["gamma"]), p(v["beta"]), 1, p(bits), _code(dt),
                 outputs=[ga.full])
        assert int(bits.sum().item()) == 0
        _refused("cpc_bn_bwd_reduce_bits", gda.ptr(), p(bits), _d(ga.desc), gx.ptr(), _d(gx.desc), p(stats), p(slabs), 3, _code(dt), outputs=[slabs])
        _refused("cpc_bn_bwd_apply_bits", gda.ptr(), p(bits), _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc), p(stats), p(v["gamma"]), p(v["dgamma"]),
                 p(v["dbeta"]), 15.0, 1, _code(dt), outputs=[gdx.full])
    # nblocks = 0
    gx, ga, gda, gdx, stats, v = bn_args(16)
    slabs = torch.empty(2 * 16, device=DEV)
    bits = torch.zeros(ga.rows * 2, device=DEV, dtype=torch.uint8)
    _refused("cpc_bn_stats", gx.ptr(), p(slabs), gx.rows, 16, 0, _code(BF), outputs=[slabs])
    _refused("cpc_bn_bwd_reduce", gda.ptr(), ga.ptr(), _d(ga.desc), gx.ptr(), _d(gx.desc), p(stats), p(slabs), 1, 0, 0, _code(BF), outputs=[slabs])
    _refused("cpc_bn_bwd_reduce_res", gda.ptr(), _d(gda.desc), None, p(bits), _d(ga.desc), gx.ptr(), _d(gx.desc), p(stats), p(slabs), 0, _code(BF),
             outputs=[slabs])
    # cpc_bn_finalize with one running-statistic pointer
    run, st = torch.empty(16, device=DEV), torch.empty(2, 16, device=DEV)
    slabs.fill_(1.0)
    _refused("cpc_bn_finalize", p(slabs), 1, 16, 30.0, 1e-5, 0.1, p(st), p(run), None, outputs=[st, run])
    slabs.fill_(1.0)
    _refused("cpc_bn_finalize", p(slabs), 1, 16, 30.0, 1e-5, 0.1, p(st), None, p(run), outputs=[st, run])
    # pooling: H = 7, p = 2 pools to 4 (ceil) or 3 (floor) rows, not to 2; W = 9 to 5 or 4, not to 3
    for Ho, Wo in ((2, 5), (4, 3)):
        gi, go, gdi = _grid(B, 9, 7, 8, BF), _grid(B, Wo, Ho, 8, BF), _grid(B, 9, 7, 8, BF)
        _refused("cpc_maxpool2d_fwd", gi.ptr(), _d(gi.desc), go.ptr(), _d(go.desc), 2, 0, _code(BF), outputs=[go.full])
        _refused("cpc_maxpool2d_bwd", gi.ptr(), gdi.ptr(), _d(gi.desc), go.ptr(), _d(go.desc), 2, 0, _code(BF), outputs=[gdi.full])
    # a crop that leaves the residual grid, by one row or by one column
    Cc = 16
    gx, ga, gda, gdx, stats, v = bn_args(Cc)
    bits = torch.zeros(ga.rows * Cc // 8, device=DEV, dtype=torch.uint8)
    for oh, ow in ((3, 0), (0, 2)):
        gr, go, gdr = _grid(B, W + 1, H + 2, Cc, BF), _grid(B, W, H, Cc, BF), _grid(B, W + 1, H + 2, Cc, BF)
        _refused("cpc_residual_add", ga.ptr(), _d(ga.desc), gr.ptr(), _d(gr.desc), go.ptr(), _d(go.desc), oh, ow, 1, 0, _code(BF), outputs=[go.full])
        _refused("cpc_residual_add_bwd", gda.ptr(), ga.ptr(), _d(ga.desc), gdx.ptr(), _d(gdx.desc), gdr.ptr(), _d(gdr.desc), oh, ow, 1, 0, _code(BF),
                 outputs=[gdx.full, gdr.full])
        _refused("cpc_bn_apply_residual", gx.ptr(), _d(gx.desc), gr.ptr(), _d(gr.desc), go.ptr(), _d(go.desc), p(stats), p(v["gamma"]), p(v["beta"]),
                 oh, ow, 1, 1, 0, p(bits), _d(ga.desc), None, _code(BF), outputs=[go.full])
        _refused("cpc_bn_bwd_apply_res", gda.ptr(), _d(gda.desc), None, p(bits), _d(ga.desc), gx.ptr(), gdx.ptr(), _d(gx.desc), p(stats),
                 p(v["gamma"]), p(v["dgamma"]), p(v["dbeta"]), 30.0, 1, gdr.ptr(), _d(gdr.desc), oh, ow, _code(BF), outputs=[gdx.full, gdr.full])
