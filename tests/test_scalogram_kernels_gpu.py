"""GPU unit tests of the scalogram path's own kernels against float64 PyTorch references: the stem (first convolution + train-mode
BatchNorm + ReLU recomputed in every pass, csrc/stem.hip) and its residual branch, the depthwise convolution of separable blocks, and
the gradient-penalty helpers (csrc/scalogram.hip, cpc_reduce_conv_w2d in csrc/gemm.hip).

References are computed on the values the device sees (inputs rounded to the storage type first).  Tolerances as in
test_hip_kernels.py: f32 3e-5 relative to the operand scale, bf16 1.2e-2.  Every grid a kernel writes is checked for untouched pad rows
(zero) and guard rows (a sentinel written before the call).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.scalogram_engine import Grid  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 7.25          # exact in bf16 and f32, and not a value any kernel here produces from the test data
EPS = 1e-5
L = C.c_longlong

# (Cin, kh, kw, sh) of csrc/stem.hip STEM_SHAPES
STEM_SHAPES = [(2, 3, 3, 2), (1, 3, 3, 2), (2, 3, 3, 1), (1, 3, 3, 1), (1, 5, 1, 1), (2, 5, 1, 1), (1, 2, 2, 1), (2, 2, 2, 1)]


def _tol(dt):
    return 3e-5 if dt == torch.float32 else 1.2e-2


def _d(desc):
    return C.cast(desc, C.c_void_p)


def _grid(B, W, H, Cc, dt, top=0, tail=0):
    """A zeroed grid whose guard rows hold SENTINEL."""
    g = Grid(B, W, H, Cc, DEV, dt, top=top, tail=tail, guard_rows=4)
    n = g.guard_rows * Cc
    g.full[:n] = SENTINEL
    g.full[n + g.rows * Cc:] = SENTINEL
    return g


def _view(g):
    return g.t.view(g.B, g.W, g.Ha, g.C)


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


def _rel(got, ref, scale=None):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    s = ref.abs().max().item() if scale is None else scale
    return ((got - ref).abs().max() / (s + 1e-30)).item()


def _pack_bits(t):
    """Sign bits as the kernels write them: one byte per 8 consecutive elements, bit e = element 8 i + e is > 0."""
    want = (t.float().view(-1, 8) > 0).to(torch.uint8)
    return (want << torch.arange(8, device=t.device, dtype=torch.uint8)).sum(1).to(torch.uint8)


def _reduce(slabs, nb, n):
    """cpc_reduce_slabs over nb slabs of n floats (what the engine does with the stem's slabs)."""
    out = torch.zeros(n, device=DEV)
    _hip.call("cpc_reduce_slabs", _hip.ptr(slabs), _hip.ptr(out), 1, n, nb, n, 1, 1, 0, 0)
    return out


# ------------------------------------------------------------------------------------------------ stem
def _stem_case(shape, Cout, ph, Ho, Wo, sw, dt, top_out, with_bias, nblocks_list, B=2, seed=0, H=None):
    """Forward (stats -> finalize -> apply) and backward (bwd_reduce -> reduce_slabs -> bwd_wgrad -> reduce_slabs) of the stem kernels
    for every nblocks in nblocks_list against float64 autograd; returns the activations of each nblocks."""
    Cin, kh, kw, sh = shape
    pw = ph
    if H is None:
        H = (Ho - 1) * sh + kh - 2 * ph
    else:
        Ho = (H + 2 * ph - kh) // sh + 1
    W = (Wo - 1) * sw + kw - 2 * pw
    assert H >= 1 and W >= 1 and (H + 2 * ph - kh) // sh + 1 == Ho and (W + 2 * pw - kw) // sw + 1 == Wo
    assert _hip.lib().cpc_stem_supported(Cin, Cout, kh, kw, sh, H, ph) == 1
    g = torch.Generator().manual_seed(seed * 1000 + Cout * 7 + Ho)
    code = _hip.dtype_code(dt)
    x = (torch.randn(B, Cin, H, W, generator=g) + 0.5).float().double()
    w = (torch.randn(Cout, Cin, kh, kw, generator=g) / (Cin * kh * kw) ** 0.5).float().double().requires_grad_(True)
    b = (0.3 * torch.randn(Cout, generator=g)).float().double().requires_grad_(True) if with_bias else None
    gamma = (1 + 0.3 * torch.randn(Cout, generator=g)).float().double().requires_grad_(True)
    beta = (0.2 * torch.randn(Cout, generator=g)).float().double().requires_grad_(True)
    y = F.conv2d(x, w, b, stride=(sh, sw), padding=(ph, pw))
    z = F.batch_norm(y, None, None, gamma, beta, training=True, eps=EPS)          # BatchNorm output before its ReLU
    mean, var = y.detach().mean((0, 2, 3)), y.detach().var((0, 2, 3), unbiased=False)

    gx = _grid(B, W, H, Cin, torch.float32)
    _fill(gx, x)
    dw_, db_ = w.detach().float().to(DEV).contiguous(), (b.detach().float().to(DEV) if with_bias else None)
    dgam, dbet = gamma.detach().float().to(DEV), beta.detach().float().to(DEV)
    conv = (C.c_int * 9)(Cout, kh, kw, sh, sw, ph, pw, Ho, Wo)
    count = float(B * Ho * Wo)
    taps = Cin * kh * kw
    da = torch.randn(B, Cout, Ho, Wo, generator=g).to(dt).double()
    outs = []
    for nb in nblocks_list:
        args = (gx.ptr(), _d(gx.desc), _hip.ptr(dw_), _hip.ptr(db_), _d(conv))
        slabs = torch.full((nb * max(2 * Cout, Cout * taps),), float("nan"), device=DEV)
        _hip.call("cpc_stem_stats", *args, _hip.ptr(slabs), nb)
        st = torch.zeros(2, Cout, device=DEV)
        _hip.call("cpc_bn_finalize", _hip.ptr(slabs), nb, Cout, count, EPS, 0.1, _hip.ptr(st), None, None)
        # statistics against their operand scales: the mean against max |y|, the variance (from rstd) against mean(y^2)
        assert _rel(st[0], mean, scale=y.detach().abs().max().item()) < 3e-5
        assert _rel(st[1].double().pow(-2) - EPS, var, scale=y.detach().pow(2).mean((0, 2, 3)).max().item()) < 3e-5
        # the passes below take the statistics of the first nblocks: the slab sums group differently with another block count, and
        # the per-position passes are then compared bit for bit on identical inputs
        if nb == nblocks_list[0]:
            stats = st
        ga = _grid(B, Wo, Ho, Cout, dt, top=top_out, tail=1)
        _hip.call("cpc_stem_apply", *args, _hip.ptr(stats), _hip.ptr(dgam), _hip.ptr(dbet), ga.ptr(), _d(ga.desc), nb, code)
        _check_frame(ga)
        a_dev = _read(ga)
        assert _rel(a_dev, torch.relu(z.detach())) < _tol(dt)
        outs.append(ga.t.clone())
        _check_frame(gx)

        # backward.  The ReLU mask is the device's own activation (a sign flip of a value within rounding of zero is not an error);
        # everything behind it is float32 arithmetic in both storage modes, so the f32 bound applies to the reductions.
        gda = _grid(B, Wo, Ho, Cout, dt, top=top_out, tail=1)
        _fill(gda, da)
        gmask = da * (a_dev > 0)
        for t in (w, b, gamma, beta):
            if t is not None:
                t.grad = None
        z.backward(gmask, retain_graph=True)
        _hip.call("cpc_stem_bwd_reduce", *args, _hip.ptr(stats), gda.ptr(), ga.ptr(), _d(ga.desc), _hip.ptr(slabs), nb, code)
        dgamma = torch.zeros(Cout, device=DEV)
        dbeta = torch.zeros(Cout, device=DEV)
        _hip.call("cpc_reduce_slabs", _hip.ptr(slabs), _hip.ptr(dgamma), 1, Cout, nb, 2 * Cout, 1, 1, 0, 0)
        _hip.call("cpc_reduce_slabs", _hip.ptr(slabs, Cout), _hip.ptr(dbeta), 1, Cout, nb, 2 * Cout, 1, 1, 0, 0)
        gscale = gmask.abs().sum((0, 2, 3)).max().item()          # sum of |terms| of the reductions
        assert _rel(dgamma, gamma.grad, scale=gscale) < 3e-5
        assert _rel(dbeta, beta.grad, scale=gscale) < 3e-5
        slabs.fill_(float("nan"))
        _hip.call("cpc_stem_bwd_wgrad", *args, _hip.ptr(stats), _hip.ptr(dgam), _hip.ptr(dgamma), _hip.ptr(dbeta), count, gda.ptr(), ga.ptr(),
                  _d(ga.desc), _hip.ptr(slabs), nb, code)
        gw = _reduce(slabs, nb, Cout * taps).view(Cout, Cin, kh, kw)
        # scale: the weight gradient of |x| against |dy| (the sum of |terms| of every entry)
        dy = torch.autograd.grad(z, y, gmask, retain_graph=True)[0]
        wscale = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(), stride=(sh, sw), padding=(ph, pw)).max().item()
        assert torch.isfinite(gw).all()
        assert _rel(gw, w.grad, scale=wscale) < 3e-5
        if with_bias:
            # the bias sits in front of a train-mode BatchNorm: its gradient is exactly zero (the engine writes zero, no kernel computes it)
            assert b.grad.abs().max().item() < 1e-9 * max(gscale, 1.0)
    return outs


def _nblocks(ncol):
    nd = next(k for k in range(3, ncol + 2) if ncol % k)          # a block count that does not divide the column count
    return [1, nd, ncol + 5]


# (shape, Cout, ph, Ho, Wo, sw, dtype, top_out, bias): every STEM_SHAPES entry, Cout 4 / 16 / 64 with 8 and 32 once each, ph 0 / 1,
# Ho % 4 = 0..3, f32 and bf16 outputs, output grids with and without top rows, with and without a bias
STEM_CASES = [
    ((2, 3, 3, 2), 64, 1, 8, 7, 2, torch.float32, 0, True),
    ((2, 3, 3, 2), 16, 0, 9, 5, 1, torch.bfloat16, 2, False),
    ((1, 3, 3, 2), 4, 1, 10, 6, 2, torch.bfloat16, 1, True),
    ((1, 3, 3, 2), 32, 0, 7, 5, 1, torch.float32, 0, False),
    ((2, 3, 3, 1), 16, 1, 11, 7, 1, torch.float32, 3, False),
    ((2, 3, 3, 1), 64, 0, 12, 4, 2, torch.bfloat16, 0, True),
    ((1, 3, 3, 1), 4, 0, 5, 9, 1, torch.float32, 1, True),
    ((1, 3, 3, 1), 64, 1, 6, 5, 1, torch.bfloat16, 0, False),
    ((1, 5, 1, 1), 16, 0, 13, 6, 1, torch.bfloat16, 2, True),
    ((1, 5, 1, 1), 8, 1, 4, 7, 2, torch.float32, 0, False),
    ((2, 5, 1, 1), 64, 1, 15, 5, 1, torch.float32, 1, True),
    ((2, 5, 1, 1), 4, 0, 2, 8, 1, torch.bfloat16, 0, False),
    ((1, 2, 2, 1), 16, 1, 9, 6, 1, torch.float32, 2, False),
    ((1, 2, 2, 1), 64, 0, 3, 7, 1, torch.bfloat16, 1, True),
    ((2, 2, 2, 1), 4, 1, 14, 5, 2, torch.float32, 0, True),
    ((2, 2, 2, 1), 16, 0, 1, 6, 1, torch.bfloat16, 0, False),
]


@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: f"{c[0]}-co{c[1]}-ph{c[2]}-ho{c[3]}-{str(c[6])[6:]}-top{c[7]}-b{int(c[8])}")
def test_stem_forward_backward_against_float64(case):
    """cpc_stem_* against conv2d -> batch_norm(training) -> relu and its autograd, for nblocks 1, a value that does not divide the
    B * Wo output columns and one larger than it; the activation is bit-identical across the three (each position is computed on
    its own, so a difference means a column computed twice from different data, or skipped)."""
    shape, Cout, ph, Ho, Wo, sw, dt, top, bias = case
    B = 2
    outs = _stem_case(shape, Cout, ph, Ho, Wo, sw, dt, top, bias, _nblocks(B * Wo), B=B)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def _max_stem_height(cin, cout, kh, kw, sh, ph=1):
    hs = [h for h in range(1, 4096) if _hip.lib().cpc_stem_supported(cin, cout, kh, kw, sh, h, ph)]
    assert hs and hs == list(range(1, hs[-1] + 1)), "supported heights are not one contiguous range from 1"
    return hs[-1]


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=str)
def test_stem_at_the_largest_supported_height(shape):
    """The largest input height cpc_stem_supported accepts (ph = 1): where an LDS bound (MAX_XS, MAXPF) that is off would show."""
    Cin, kh, kw, sh = shape
    Cout = 64 if Cin == 2 else 16
    hin = _max_stem_height(Cin, Cout, kh, kw, sh)
    _stem_case(shape, Cout, 1, None, 3, 1, torch.bfloat16 if Cin == 1 else torch.float32, 1, True, [1, 2], B=1, seed=3, H=hin)


# ------------------------------------------------------------------------------------------------ stem residual branch
# (dtype, Cin, Cout, relu): Cout at the smallest and the largest allowed multiple of the channels a thread owns (8 bf16 / 4 f32)
RES_CASES = [(torch.float32, 1, 4, 1), (torch.float32, 2, 1024, 0), (torch.float32, 2, 32, 1),
             (torch.bfloat16, 1, 8, 0), (torch.bfloat16, 2, 2048, 1), (torch.bfloat16, 1, 64, 1)]


@pytest.mark.parametrize("case", RES_CASES, ids=lambda c: f"{str(c[0])[6:]}-cin{c[1]}-co{c[2]}-relu{c[3]}")
def test_stem_residual_add_and_backward(case):
    """cpc_stem_residual_add: act(main + wr xp(w + ow, h + oh)) with a cropped, shifted window of the float32 pooled input;
    cpc_stem_residual_bwd: dmain = dout [out > 0] bit for bit, and the projection's gradient (slabs summed on the host)."""
    dt, Cin, Cout, relu = case
    B, mW, mH, oh, ow = 2, 3, 5, 2, 1
    g = torch.Generator().manual_seed(Cout + Cin)
    code = _hip.dtype_code(dt)
    xp = torch.randn(B, Cin, mH + oh + 2, mW + ow + 1, generator=g).float().double()
    main = torch.randn(B, Cout, mH, mW, generator=g).to(dt).double()
    wr = torch.randn(Cout, Cin, generator=g).float().double()
    gp = _grid(B, mW + ow + 1, mH + oh + 2, Cin, torch.float32, tail=1)
    gm = _grid(B, mW, mH, Cout, dt, top=1)
    go = _grid(B, mW, mH, Cout, dt, top=2, tail=1)
    _fill(gp, xp)
    _fill(gm, main)
    dwr = wr.float().to(DEV).contiguous()
    xw = xp[:, :, oh:oh + mH, ow:ow + mW]
    pre = main + torch.einsum("oc,bchw->bohw", wr, xw)
    ref = torch.relu(pre) if relu else pre
    _hip.call("cpc_stem_residual_add", gm.ptr(), _d(gm.desc), gp.ptr(), _d(gp.desc), _hip.ptr(dwr), go.ptr(), _d(go.desc), oh, ow, relu, code)
    for gr in (gp, gm, go):
        _check_frame(gr)
    out = _read(go)
    assert _rel(out, ref, scale=pre.abs().max().item()) < _tol(dt)

    gdo = _grid(B, mW, mH, Cout, dt, top=2, tail=1)
    dout = torch.randn(B, Cout, mH, mW, generator=g).to(dt).double()
    _fill(gdo, dout)
    gdm = _grid(B, mW, mH, Cout, dt, top=1)
    nb = 4                                  # B * mW = 6 columns: 4 blocks split them unevenly
    slabs = torch.full((nb * Cout * Cin,), float("nan"), device=DEV)
    _hip.call("cpc_stem_residual_bwd", gdo.ptr(), go.ptr(), _d(go.desc), gdm.ptr(), _d(gdm.desc), gp.ptr(), _d(gp.desc), _hip.ptr(slabs),
              oh, ow, relu, nb, code)
    _check_frame(gdm)
    gmask = dout * (out > 0) if relu else dout
    assert torch.equal(_read(gdm), gmask)
    got = slabs.view(nb, Cout, Cin).double().sum(0).cpu()
    want = torch.einsum("bohw,bchw->oc", gmask, xw)
    scale = torch.einsum("bohw,bchw->oc", gmask.abs(), xw.abs()).max().item()
    assert _rel(got, want, scale=scale) < 3e-5


@pytest.mark.parametrize("Cin", [1, 2])
def test_stem_residual_bn_add_and_wgrad_bits_equal_the_separate_passes(Cin):
    """bf16: cpc_stem_residual_bn_add = cpc_bn_apply (+ReLU) followed by cpc_stem_residual_add bit for bit, with the sign bits of the
    normalised branch (bits, addressed like its grid) and of the output (obits); cpc_stem_residual_wgrad_bits (mask from obits, nothing
    stored) gives the slabs of cpc_stem_residual_bwd with relu = 1."""
    bf = torch.bfloat16
    code = _hip.dtype_code(bf)
    B, mW, mH, Cc, oh, ow = 2, 5, 6, 16, 1, 2
    g = torch.Generator().manual_seed(40 + Cin)
    gy = _grid(B, mW, mH, Cc, bf, tail=3)
    ga = _grid(B, mW, mH, Cc, bf, top=1)
    gp = _grid(B, mW + ow, mH + oh + 1, Cin, torch.float32)
    _fill(gy, torch.randn(B, Cc, mH, mW, generator=g) * 1.5 + 0.3)
    _fill(gp, torch.randn(B, Cin, mH + oh + 1, mW + ow, generator=g))
    wr = torch.randn(Cc, Cin, generator=g).to(DEV)
    stats = torch.stack([torch.randn(Cc, generator=g) * 0.2, 1 + 0.3 * torch.rand(Cc, generator=g)]).to(DEV)
    gamma, beta = (1 + 0.3 * torch.randn(Cc, generator=g)).to(DEV), (0.2 * torch.randn(Cc, generator=g)).to(DEV)
    for relu in (1, 0):
        go1, go2 = _grid(B, mW, mH, Cc, bf, top=2, tail=1), _grid(B, mW, mH, Cc, bf, top=2, tail=1)
        bits = torch.zeros(ga.rows * Cc // 8, device=DEV, dtype=torch.uint8)
        obits = torch.zeros(go2.rows * Cc // 8, device=DEV, dtype=torch.uint8)
        _hip.call("cpc_bn_apply", gy.ptr(), _d(gy.desc), ga.ptr(), _d(ga.desc), _hip.ptr(stats), _hip.ptr(gamma), _hip.ptr(beta), 1, 0, code)
        _hip.call("cpc_stem_residual_add", ga.ptr(), _d(ga.desc), gp.ptr(), _d(gp.desc), _hip.ptr(wr), go1.ptr(), _d(go1.desc), oh, ow, relu, code)
        _hip.call("cpc_stem_residual_bn_add", gy.ptr(), _d(gy.desc), gp.ptr(), _d(gp.desc), _hip.ptr(wr), go2.ptr(), _d(go2.desc), oh, ow, relu,
                  _hip.ptr(stats), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(bits), _d(ga.desc), _hip.ptr(obits), code)
        _check_frame(go2)
        assert torch.equal(go1.full, go2.full)
        assert go1.t.abs().max().item() > 0 and bool((go1.t < 0).any()) == (relu == 0)
        assert torch.equal(bits, _pack_bits(ga.t))
        assert torch.equal(obits, _pack_bits(go1.t))

        gdo = _grid(B, mW, mH, Cc, bf, top=2, tail=1)
        _fill(gdo, torch.randn(B, Cc, mH, mW, generator=g))
        gdm = _grid(B, mW, mH, Cc, bf, top=1)
        for nb in (1, 3, 2 * B * mW + 1):
            s1 = torch.full((nb * Cc * Cin,), float("nan"), device=DEV)
            s2 = torch.full_like(s1, float("nan"))
            _hip.call("cpc_stem_residual_bwd", gdo.ptr(), go1.ptr(), _d(go1.desc), gdm.ptr(), _d(gdm.desc), gp.ptr(), _d(gp.desc), _hip.ptr(s1),
                      oh, ow, 1, nb, code)
            _hip.call("cpc_stem_residual_wgrad_bits", gdo.ptr(), _hip.ptr(obits), _d(go1.desc), _d(gy.desc), gp.ptr(), _d(gp.desc), _hip.ptr(s2),
                      oh, ow, nb, code)
            assert torch.equal(s1, s2)
            assert s1.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------ depthwise convolution
# (dtype, C, (kh, kw), stride, pad, extra K columns, output rows inside a grid): C as the separable blocks use them and 12 (not a power of 2)
DW_CASES = [(torch.float32, 16, (3, 3), 1, 1, 0, True), (torch.bfloat16, 64, (3, 3), 1, 1, 8, True),
            (torch.float32, 12, (2, 2), 2, 0, 4, False), (torch.bfloat16, 12, (3, 1), 1, 1, 0, False),
            (torch.bfloat16, 32, (1, 3), (1, 2), 0, 16, True)]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: f"{str(c[0])[6:]}-C{c[1]}-k{c[2][0]}x{c[2][1]}-kx{c[5]}-{'grid' if c[6] else 'flat'}")
def test_depthwise_convolution_against_grouped_conv2d(case):
    """cpc_dw_fwd / cpc_dw_bwd_col (+ cpc_col2im2d) / cpc_dw_bwd_w on the im2col matrix of a grid against conv2d(groups=C) and its
    autograd; output rows either inside a grid (rpi = Ho, an item stride larger than Ho * C: pad rows between items stay untouched)
    or plain [M][C]."""
    dt, Cc, (kh, kw), stride, pad, kx, in_grid = case
    sh, sw = stride if isinstance(stride, tuple) else (stride, stride)
    B, H, W = 2, 7, 6
    code = _hip.dtype_code(dt)
    g = torch.Generator().manual_seed(Cc + kh * 10 + kw)
    x = torch.randn(B, Cc, H, W, generator=g).to(dt).double().requires_grad_(True)
    w = torch.randn(Cc, 1, kh, kw, generator=g).float().double().requires_grad_(True)
    ref = F.conv2d(x, w, stride=(sh, sw), padding=pad, groups=Cc)
    Ho, Wo = ref.shape[2], ref.shape[3]
    M, taps = B * Wo * Ho, kh * kw
    K, Kp = taps * Cc, taps * Cc + kx
    gin = _grid(B, W, H, Cc, dt)
    _fill(gin, x.detach())
    col = torch.full((M, Kp), float("nan"), device=DEV, dtype=dt)
    _hip.call("cpc_im2col2d", gin.ptr(), _hip.ptr(col), _d(gin.padded_desc), kh, kw, sh, sw, pad, pad, Ho, Wo, Kp, 0, code)
    dw_ = w.detach().float().view(Cc, taps).to(DEV).contiguous()

    if in_grid:
        gy = _grid(B, Wo, Ho, Cc, dt, top=1, tail=2)
        rpi, item, yptr = Ho, gy.Ha * Cc, gy.ptr(gy.top * Cc)
        read = lambda: _read(gy)                                                      # noqa: E731
        gdy = _grid(B, Wo, Ho, Cc, dt, top=1, tail=2)
        dyptr = gdy.ptr(gdy.top * Cc)
    else:
        gy = _grid(1, 1, M, Cc, dt)                                                  # a flat [M][C] buffer with guards
        rpi, item, yptr = 0, 0, gy.ptr()
        read = lambda: _view(gy)[0, 0].double().cpu().view(B, Wo, Ho, Cc).permute(0, 3, 2, 1)   # noqa: E731  (m = (b Wo + wo) Ho + ho)
        gdy = _grid(1, 1, M, Cc, dt)
        dyptr = gdy.ptr()
    _hip.call("cpc_dw_fwd", _hip.ptr(col), _hip.ptr(dw_), yptr, L(M), Cc, taps, Kp, rpi, L(item), code)
    _check_frame(gy)
    assert _rel(read(), ref.detach()) < _tol(dt)

    dy = torch.randn(B, Cc, Ho, Wo, generator=g).to(dt).double()
    ref.backward(dy)
    if in_grid:
        _fill(gdy, dy)
    else:
        _view(gdy)[0, 0, :, :] = dy.permute(0, 3, 2, 1).reshape(M, Cc).to(dt).to(DEV)
    dcol = torch.full((M, Kp), float("nan"), device=DEV, dtype=dt)
    _hip.call("cpc_dw_bwd_col", dyptr, _hip.ptr(dw_), _hip.ptr(dcol), L(M), Cc, taps, Kp, rpi, L(item), code)
    if Kp > K:
        assert dcol[:, K:].abs().max().item() == 0
    dy_rows = dy.permute(0, 3, 2, 1).reshape(M, 1, Cc)
    want = (dy_rows * w.detach().view(Cc, taps).t().unsqueeze(0)).reshape(M, K)          # dcol[m][t C + c] = dy[m][c] w[c][t]
    assert _rel(dcol[:, :K].double().cpu(), want) < _tol(dt)
    gdin = _grid(B, W, H, Cc, dt)
    _hip.call("cpc_col2im2d", _hip.ptr(dcol), gdin.ptr(), _d(gdin.padded_desc), kh, kw, sh, sw, pad, pad, Ho, Wo, Kp, 0, code)
    _check_frame(gdin)
    assert _rel(_read(gdin), x.grad) < _tol(dt)

    # weight gradient: f32 sums of products of values the reference sees exactly (bf16 inputs are exact in f32), so the f32 bound
    scale = torch.nn.grad.conv2d_weight(x.detach().abs(), w.shape, dy.abs(), stride=(sh, sw), padding=pad, groups=Cc).max().item()
    for nb in (1, 5, M + 3):
        slabs = torch.full((nb * Cc * taps,), float("nan"), device=DEV)
        _hip.call("cpc_dw_bwd_w", _hip.ptr(col), dyptr, _hip.ptr(slabs), L(M), Cc, taps, Kp, rpi, L(item), nb, code)
        got = slabs.view(nb, Cc, taps).double().sum(0).cpu()
        assert _rel(got, w.grad.view(Cc, taps), scale=scale) < 3e-5


# ------------------------------------------------------------------------------------------------ gradient-penalty kernels
@pytest.mark.parametrize("Cc", [1, 2])
@pytest.mark.parametrize("npix", [1000, 5003])
def test_gp_direction_against_autograd(Cc, npix):
    """cpc_gp_direction: v = d/dg of factor * mean((|g| - 1)^2) over pixels (torch's norm backward: 0 where g = 0, no NaN) and the
    per-block partial sums of (|g| - 1)^2, for one block and many."""
    gen = torch.Generator().manual_seed(npix + Cc)
    g = torch.randn(npix, Cc, generator=gen).float()
    g[::17] = 0.0                                              # pixels whose gradient is exactly zero
    factor = 10.0
    g64 = g.double().requires_grad_(True)
    n = g64.norm(dim=1)
    pen_sum = ((n - 1) ** 2).sum()
    (factor * pen_sum / npix).backward()
    dg = g.to(DEV)
    for nb in (1, 7, 64):
        v = torch.full((npix, Cc), float("nan"), device=DEV)
        part = torch.full((nb,), float("nan"), device=DEV)
        _hip.call("cpc_gp_direction", _hip.ptr(dg), _hip.ptr(v), L(npix), Cc, factor, _hip.ptr(part), nb)
        vc = v.cpu()
        assert torch.isfinite(vc).all()
        assert torch.equal(vc[::17], torch.zeros_like(vc[::17]))
        assert _rel(vc, g64.grad) < 3e-5
        assert _rel(part.double().sum().cpu(), pen_sum.detach()) < 3e-5


def _first_max_select(x, sel, p, Ho, Wo):
    """The element of sel at the first maximum of x in every p x p window, windows scanned row by row (dh outer, dw inner) as
    cpc_maxpool2d_fwd scans them; windows clipped at the border (ceil mode) or the remainder dropped (floor mode)."""
    B, Cc, H, W = x.shape
    xp = torch.full((B, Cc, Ho * p, Wo * p), float("-inf"), dtype=x.dtype)
    sp = torch.zeros((B, Cc, Ho * p, Wo * p), dtype=sel.dtype)
    hh, ww = min(H, Ho * p), min(W, Wo * p)
    xp[:, :, :hh, :ww] = x[:, :, :hh, :ww]
    sp[:, :, :hh, :ww] = sel[:, :, :hh, :ww]
    win = lambda t: t.view(B, Cc, Ho, p, Wo, p).permute(0, 1, 2, 4, 3, 5).reshape(B, Cc, Ho, Wo, p * p)   # noqa: E731
    idx = win(xp).argmax(-1, keepdim=True)                    # first maximum (torch.argmax returns the first of equal maxima)
    return win(sp).gather(-1, idx).squeeze(-1)


@pytest.mark.parametrize("dt,in_f32", [(torch.float32, 0), (torch.bfloat16, 0), (torch.float32, 1), (torch.bfloat16, 1)])
@pytest.mark.parametrize("p,ceil", [(2, True), (3, True), (2, False)])
def test_maxpool2d_select_takes_the_first_maximum_of_ties(dt, in_f32, p, ceil):
    """cpc_maxpool2d_select on inputs full of ties (three bf16-exact values): `sel` at the FIRST maximum of each window."""
    B, Cc, H, W = 2, 3, 7, 9
    gen = torch.Generator().manual_seed(p * 10 + in_f32)
    tin = torch.float32 if in_f32 else dt
    x = (torch.randint(0, 3, (B, Cc, H, W), generator=gen) * 0.5 - 0.5).to(tin).double()
    sel = torch.randn(B, Cc, H, W, generator=gen).to(tin).double()
    Ho, Wo = ((H + p - 1) // p, (W + p - 1) // p) if ceil else (H // p, W // p)
    gi, gs = _grid(B, W, H, Cc, tin, top=1), _grid(B, W, H, Cc, tin, top=1)
    _fill(gi, x)
    _fill(gs, sel)
    go = _grid(B, Wo, Ho, Cc, dt, top=1, tail=1)
    _hip.call("cpc_maxpool2d_select", gi.ptr(), gs.ptr(), _d(gi.desc), go.ptr(), _d(go.desc), p, in_f32, _hip.dtype_code(dt))
    _check_frame(go)
    want = _first_max_select(x, sel, p, Ho, Wo).to(dt).double()
    assert torch.equal(_read(go), want)


@pytest.mark.parametrize("dt,x_f32", [(torch.float32, 0), (torch.float32, 1), (torch.bfloat16, 0), (torch.bfloat16, 1)])
def test_bn_gp_cross_against_float64(dt, x_f32):
    """cpc_bn_gp_cross: coef[c] xhat + coef[C + c] yt + coef[2C + c] delta on the valid rows; pad and guard rows untouched."""
    B, Cc, H, W = 2, 8, 6, 5
    gen = torch.Generator().manual_seed(3 + x_f32)
    tx = torch.float32 if (x_f32 or dt == torch.float32) else dt
    x = (torch.randn(B, Cc, H, W, generator=gen) * 2 + 0.4).to(tx).double()
    yt = torch.randn(B, Cc, H, W, generator=gen).to(dt).double()
    delta = torch.randn(B, Cc, H, W, generator=gen).to(tx).double()
    stats = torch.stack([torch.randn(Cc, generator=gen) * 0.3, 0.5 + torch.rand(Cc, generator=gen)]).float()
    coef = torch.randn(3, Cc, generator=gen).float()
    grids = [_grid(B, W, H, Cc, t, top=2, tail=1) for t in (tx, dt, tx, tx)]
    for gr, v in zip(grids, (x, yt, delta)):
        _fill(gr, v)
    gx, gyt, gdl, gout = grids
    dstats, dcoef = stats.to(DEV), coef.to(DEV)
    _hip.call("cpc_bn_gp_cross", gx.ptr(), gyt.ptr(), gdl.ptr(), gout.ptr(), _d(gx.desc), _hip.ptr(dstats), _hip.ptr(dcoef), x_f32, _hip.dtype_code(dt))
    _check_frame(gout)
    s, k = stats.double().view(2, 1, Cc, 1, 1), coef.double().view(3, 1, Cc, 1, 1)
    terms = (k[0] * (x - s[0]) * s[1], k[1] * yt, k[2] * delta)
    want = terms[0] + terms[1] + terms[2]
    scale = sum(t.abs() for t in terms).max().item()
    assert _rel(_read(gout), want, scale=scale) < _tol(tx)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [4, 4 * 100003])
def test_relu_mask_bit_exact(dt, n):
    """cpc_relu_mask: g = g [y > 0] bit for bit (y = 0 and y = -0 mask), nothing beyond n written; n % 4 != 0 is refused."""
    gen = torch.Generator().manual_seed(n)
    y = torch.randn(n + 8, generator=gen).to(dt)
    y[1::7] = 0.0
    y[2::11] = -0.0
    g = torch.randn(n + 8, generator=gen).to(dt)
    want = torch.where(y[:n] > 0, g[:n], torch.zeros_like(g[:n]))
    dg, dy = g.to(DEV), y.to(DEV)
    _hip.call("cpc_relu_mask", _hip.ptr(dg), _hip.ptr(dy), L(n), _hip.dtype_code(dt))
    got = dg.cpu()
    assert torch.equal(got[:n].view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dt == torch.bfloat16 else torch.int32))
    assert torch.equal(got[n:], g[n:])
    with pytest.raises(_hip.HipCallError):
        _hip.call("cpc_relu_mask", _hip.ptr(dg), _hip.ptr(dy), L(n + 2), _hip.dtype_code(dt))


# (cout, cin, kh, kw, G, nslab, extra floats between slabs): G > 1 is the row-grouped tall-kernel call (scalogram_engine.py, mode 'col'),
# G = 1 the gathered-window call (slabs [dw][dh][c][co], a nonzero kernel-column stride s_dw)
W2D_CASES = [(32, 16, 4, 1, 4, 3, 0), (8, 3, 5, 1, 16, 1, 0), (16, 2, 3, 1, 6, 5, 24), (32, 2, 3, 3, 1, 4, 0), (12, 1, 2, 5, 1, 2, 40)]


@pytest.mark.parametrize("case", W2D_CASES, ids=str)
def test_reduce_conv_w2d_against_the_host_sum(case):
    """cpc_reduce_conv_w2d in the two ways the engine calls it, on slab values whose sums are exact in f32: bit-identical to the
    host sum permuted to [Cout][Cin][kh][kw]; nothing written past the output."""
    cout, cin, kh, kw, G, nslab, gap = case
    gen = torch.Generator().manual_seed(cout * 100 + G)
    if G > 1:
        Rw = kh + G - 1
        rows, cols = Rw * cin, G * cout
        size = rows * cols
        args = (cout, cin, kh, 1, L(0), L(cin * G * cout), L(G * cout), G, L(cout))
    else:
        kc = kh * cin * cout
        size = kw * kc
        args = (cout, cin, kh, kw, L(kc), L(cin * cout), L(cout), 1, L(0))
    stride = size + gap
    body = torch.randint(-64, 65, (nslab, size), generator=gen).float() / 16          # multiples of 1/16: every partial sum exact
    slabs = torch.full((nslab, stride), float("nan"))
    slabs[:, :size] = body
    if G > 1:
        S = body.double().view(nslab, Rw, cin, G, cout)
        want = torch.zeros(cout, cin, kh, 1, dtype=torch.float64)
        for j in range(kh):
            for gg in range(G):
                want[:, :, j, 0] += S[:, j + gg, :, gg, :].sum(0).t()
    else:
        want = body.double().view(nslab, kw, kh, cin, cout).sum(0).permute(3, 2, 1, 0)
    total = cout * cin * kh * kw
    out = torch.full((total + 8,), SENTINEL, device=DEV)
    dslabs = slabs.to(DEV)
    _hip.call("cpc_reduce_conv_w2d", _hip.ptr(dslabs), _hip.ptr(out), nslab, L(stride), *args)
    assert torch.equal(out[:total].double().cpu().view(cout, cin, kh, kw), want)
    assert bool((out[total:] == SENTINEL).all())
