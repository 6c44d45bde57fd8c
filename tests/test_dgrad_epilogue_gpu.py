"""The compile-time epilogue forms of the 256 x 256 bf16 NT kernel (csrc/gemm.hip, EPI_DGRAD, EPI_DGRAD_MASK and EPI_DGRAD_C1) against the
generic body.

The forms serve the masked data-gradient launches that cpc_conv_dgrad(_rows) and cpc_conv_dgrad_conv1(_rows) build.  They take every
sum in the generic body's order, so everything they write must be bit-identical (torch.equal) to what the same launch writes with
CPC_GEMM_GENERIC_EPI: the stored gradient, the per-tile column-sum slabs and the layer-1 slabs.  CPC_GEMM_QUERY_EPI tells which body a
launch would run, so every comparison first checks that its two sides really are the two bodies.  One float64 check per form closes the
set, with the tolerances of the existing data-gradient tests (test_audio_kernels_gpu.py, test_hip_kernels.py).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from cpc_audio_amd import _hip

DEV = torch.device("cuda:0")
BF = torch.bfloat16
SENTINEL = 7.25          # exact in bf16 and f32, and not a value any kernel here produces from the test data
EINVAL = -22
GENERIC, QUERY, BIG, SKIP = _hip.GEMM_GENERIC_EPI, _hip.GEMM_QUERY_EPI, _hip.GEMM_BIG_TILE, _hip.GEMM_SKIP_PAD_ROWS
FORM_GENERIC, FORM_DGRAD, FORM_C1, FORM_MASK = 100, 101, 102, 103


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def raw(name, *args):
    return getattr(_hip.lib(), name)(*args, _hip.stream_ptr())


def full(n, dt, value=SENTINEL):
    return torch.full((n,), value, device=DEV, dtype=dt)


class debug_flags:
    """cpc_gemm_nt_debug_flags for the launches of a with-block (the entry points of the conv launches take no flags)."""

    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.prev = _hip.lib().cpc_gemm_nt_debug_flags(self.flags)
        assert self.prev == 0

    def __exit__(self, *exc):
        _hip.lib().cpc_gemm_nt_debug_flags(0)


# ------------------------------------------------------------------------------------------ which body a launch takes (no GPU work)
def _nt_args(M=300, N=256, K=128, rpi=100, alloc=128, valid=90, flags=BIG, a_rpi=None, bias=None, mask=None, b_rpi=0, dtype=_hip.BF16):
    P = C.c_void_p(0x10000)       # never dereferenced: CPC_GEMM_QUERY_EPI launches nothing
    a_rpi = rpi if a_rpi is None else a_rpi
    return _hip.GemmNTArgs(P, P, P, bias, mask, M, N, K, K, K, N, a_rpi, alloc * K if a_rpi else 0, b_rpi, 64 * K if b_rpi else 0,
                           rpi, alloc * N if rpi else 0, valid, 0, 0, 0, 1, flags | QUERY, dtype, 0, 0)


def test_launches_that_match_no_form_keep_the_generic_body():
    """Host only (the query flag returns before any launch): the launch of the tests below is EPI_DGRAD; each single departure from what
    cpc_conv_dgrad(_rows) builds is still accepted and keeps the generic body; the fused launches likewise; and the process-wide flag
    takes only the two A/B flags."""
    lib = _hip.lib()
    P, s = C.c_void_p(0x10000), C.c_void_p(0)

    def form(**kw):
        return lib.cpc_gemm_nt_bits(C.byref(_nt_args(**kw)), P, P, s)

    assert form() == FORM_DGRAD
    assert form(rpi=0) == FORM_DGRAD and form(flags=BIG | SKIP) == FORM_DGRAD and form(N=1024, K=1024) == FORM_DGRAD
    assert form(mask=P) == FORM_DGRAD                                   # the bits replace a full-size mask given beside them
    assert form(flags=BIG | GENERIC) == FORM_GENERIC                    # forced
    assert form(bias=P) == FORM_GENERIC
    assert form(flags=BIG | _hip.GEMM_RELU) == FORM_GENERIC
    assert form(rpi=20, alloc=32, valid=20) == FORM_GENERIC             # items shorter than a row step: addresses by division
    assert form(a_rpi=0) == FORM_GENERIC                                # A and C rows in different items
    assert form(b_rpi=64) == FORM_GENERIC
    assert form(valid=-1) == FORM_GENERIC
    # no sign bits: the full-size mask has a form of its own (layers 5 - 3 of the train step); no mask at all, none
    assert lib.cpc_gemm_nt(C.byref(_nt_args(mask=P)), s) == FORM_MASK
    assert lib.cpc_gemm_nt_bits(C.byref(_nt_args(mask=P)), None, P, s) == FORM_MASK
    assert lib.cpc_gemm_nt(C.byref(_nt_args(mask=P, flags=BIG | GENERIC)), s) == FORM_GENERIC
    assert lib.cpc_gemm_nt(C.byref(_nt_args(mask=P, bias=P)), s) == FORM_GENERIC
    assert lib.cpc_gemm_nt(C.byref(_nt_args(mask=P, flags=BIG | _hip.GEMM_DIRECT_MASK)), s) == FORM_GENERIC      # register epilogue
    assert lib.cpc_gemm_nt(C.byref(_nt_args(flags=BIG | _hip.GEMM_NO_PERS)), s) == FORM_GENERIC
    assert lib.cpc_gemm_nt_bits(C.byref(_nt_args()), None, None, s) == EINVAL
    assert form(N=264) == EINVAL and form(M=255) == EINVAL             # no 256 x 256 tile with the bits: refused as before
    # the conv entry points, through the process-wide flag
    B, Cin, Cout, kw, st, La, kw1, s1 = 3, 256, 64, 8, 4, 128, 10, 5
    ldx = (La * st - 1) * s1 + kw1
    head = C.c_longlong(Cout)

    def conv_forms():
        return (lib.cpc_conv_dgrad(P, P, None, P, B, Cin, Cout, kw, st, La, La * st, head, _hip.BF16, P, P, s),
                lib.cpc_conv_dgrad_rows(P, P, P, P, B, Cin, Cout, kw, st, La, head, _hip.BF16, P, P, 10, 110, s),
                lib.cpc_conv_dgrad_conv1(P, P, None, P, P, 32, Cin, Cout, kw, st, 1600, C.c_longlong(1600 * st * s1 + kw1), kw1, s1, 1600 * st,
                                         head, _hip.BF16, P, s),
                lib.cpc_conv_dgrad_conv1_rows(P, P, P, P, P, B, Cin, Cout, kw, st, La, C.c_longlong(ldx), kw1, s1, La * st, head, _hip.BF16, P,
                                              10, 110, s))

    assert lib.cpc_gemm_nt_debug_flags(QUERY) == 0
    try:
        # (cpc_conv_dgrad on 384 rows takes the 128 x 128 tile, where the bits do not exist: refused as before)
        assert conv_forms() == (EINVAL, FORM_DGRAD, FORM_C1, FORM_C1)
        assert lib.cpc_conv_dgrad_rows(P, P, P, P, B, Cin, Cout, kw, st, La, head, _hip.BF16, None, P, 10, 110, s) == FORM_MASK
        assert lib.cpc_conv_dgrad(P, P, None, P, 32, Cin, Cout, kw, st, 1600, 6400, head, _hip.BF16, P, None, s) == FORM_DGRAD
        assert lib.cpc_conv_dgrad_conv1_rows(P, P, P, P, P, B, Cin, Cout, kw, st, La, C.c_longlong(ldx), kw1, s1, La * st, head, _hip.BF16,
                                             None, 10, 110, s) == FORM_GENERIC            # full-size mask instead of the bits
        assert lib.cpc_gemm_nt_debug_flags(QUERY | GENERIC) == QUERY
        assert conv_forms() == (EINVAL, FORM_GENERIC, FORM_GENERIC, FORM_GENERIC)
        assert lib.cpc_gemm_nt_debug_flags(_hip.GEMM_RELU) == -1 and lib.cpc_gemm_nt_debug_flags(BIG) == -1
    finally:
        lib.cpc_gemm_nt_debug_flags(0)
    assert lib.cpc_gemm_nt_debug_flags(0) == 0


# ------------------------------------------------------------------------------------------ EPI_DGRAD through cpc_gemm_nt_bits
def _run_nt_bits(ops, N, K, rpi, alloc, valid, M, flags, want_cs, use_bits=True):
    A, Bt, bits, act = ops
    Cbuf = full(3 * alloc * N + 64, BF)
    tiles = -(-M // 256)
    cs = full(tiles * N + 64, torch.float32)
    args = _hip.GemmNTArgs(_hip.ptr(A), _hip.ptr(Bt), _hip.ptr(Cbuf), None, None if use_bits else _hip.ptr(act), M, N, K, K, K, N, rpi, alloc * K if rpi else 0, 0, 0,
                           rpi, alloc * N if rpi else 0, valid, 0, 0, 0, 1, flags, _hip.BF16, 0, 0)
    want = FORM_GENERIC if flags & GENERIC else FORM_DGRAD if use_bits else FORM_MASK
    mb = _hip.ptr(bits) if use_bits else None
    args.flags = flags | QUERY
    assert raw("cpc_gemm_nt_bits", C.byref(args), mb, _hip.ptr(cs) if want_cs else None) == want
    args.flags = flags
    assert raw("cpc_gemm_nt_bits", C.byref(args), mb, _hip.ptr(cs) if want_cs else None) == 0
    return Cbuf, cs


@pytest.mark.gpu
@pytest.mark.parametrize("use_bits", [True, False])
@pytest.mark.parametrize("N,K", [(256, 128), (256, 1024), (1024, 128), (1024, 1024)])
def test_masked_dgrad_form_is_bit_identical_to_the_generic_body(N, K, use_bits):
    """3 items of 100 rows in slots of 128 (M = 300: the second tile is partial and item boundaries fall inside both tiles), c_valid = 90 < 100
    under both pad-row policies, and the same rows without items; N of one and of four column tiles; K of 2 and of 16 stages; with and
    without column sums; the mask as sign bits (EPI_DGRAD) and full size (EPI_DGRAD_MASK).  Stored rows, untouched rows (sentinel) and the column-sum slabs are equal bit for bit; for the first combination
    also against float64."""
    g = torch.Generator().manual_seed(N + K)
    rpi, alloc, M = 100, 128, 300
    A = (torch.randn(3 * alloc, K, generator=g) * 0.5).to(DEV).to(BF)
    Bt = (torch.randn(N, K, generator=g) * 0.1).to(DEV).to(BF)
    act = torch.randn(3 * alloc * N, generator=g).to(DEV).to(BF)
    bits = torch.zeros(act.numel() // 8, device=DEV, dtype=torch.uint8)
    _hip.call("cpc_sign_bits", _hip.ptr(act), _hip.ptr(bits), C.c_longlong(act.numel()), _hip.BF16)
    ops = (A, Bt, bits, act)
    first = True
    for r, valid, pol in ((rpi, 90, 0), (rpi, 90, SKIP), (0, 0, 0)):
        for want_cs in (True, False):
            got, cs = _run_nt_bits(ops, N, K, r, alloc, valid, M, BIG | pol, want_cs, use_bits)
            ref, cs_ref = _run_nt_bits(ops, N, K, r, alloc, valid, M, BIG | pol | GENERIC, want_cs, use_bits)
            assert torch.equal(got, ref), (r, pol, want_cs)
            assert torch.equal(cs, cs_ref), (r, pol, want_cs)
            assert bool((cs == SENTINEL).all()) != want_cs
            if first:
                first = False
                Cv = got[:3 * alloc * N].view(3, alloc, N)
                want = (A.double().view(3, alloc, K)[:, :rpi] @ Bt.double().t()) * (act.view(3, alloc, N)[:, :rpi] > 0)
                assert rel_err(Cv[:, :valid], want[:, :valid]) < 1.2e-2               # tol(bf16) of the data-gradient tests
                assert bool((Cv[:, valid:rpi] == 0).all()) and bool((Cv[:, rpi:] == SENTINEL).all())
                sums = Cv[:, :rpi].double().reshape(-1, N)
                want_cs2 = torch.stack([sums[:256].sum(0), sums[256:].sum(0)])
                assert rel_err(cs[:2 * N].view(2, N), want_cs2) < 1e-5
            elif pol == SKIP and r:
                assert bool((got[:3 * alloc * N].view(3, alloc, N)[:, valid:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------ the conv launches
def _conv_case(B, Cin, Cout, kw, stride, La1, seed):
    g = torch.Generator().manual_seed(seed)
    La0 = La1 * stride
    guard = 16 * max(Cin, Cout)
    act = torch.randn(B, La0, Cin, generator=g)
    dy = torch.randn(B, La1, Cout, generator=g)
    w = torch.randn(Cout, Cin, kw, generator=g) * 0.05

    def padded(t):
        buf = torch.zeros(guard + t.numel() + guard, device=DEV, dtype=BF)
        buf[guard:guard + t.numel()] = t.reshape(-1).to(DEV).to(BF)
        return buf

    abuf, dybuf = padded(act), padded(dy)
    D = -(-kw // stride)
    wd = torch.empty(stride * Cin * D * Cout, device=DEV, dtype=BF)
    _hip.call("cpc_conv_w_prep", _hip.ptr(w.to(DEV)), None, _hip.ptr(wd), Cout, Cin, kw, stride, _hip.BF16)
    bits = torch.zeros(abuf.numel() // 8, device=DEV, dtype=torch.uint8)
    _hip.call("cpc_sign_bits", _hip.ptr(abuf), _hip.ptr(bits), C.c_longlong(abuf.numel()), _hip.BF16)
    return act, dy, w, abuf, dybuf, wd, bits, guard, La0


@pytest.mark.gpu
@pytest.mark.parametrize("use_bits", [True, False])
@pytest.mark.parametrize("Cout", [64, 512])
def test_row_range_launches_are_bit_identical_to_the_generic_body(Cout, use_bits):
    """The target lane's launch form: cpc_conv_dgrad_rows on rows [10, 110) and [110, 250) of 3 items of 256 (ranges that start and end
    inside items; M = 300 and 420), each with its own set of column-sum slabs, the mask as sign bits and full size (the engine's layers 5 - 3), K of 2 (Cout 64) and 16 (Cout 512) stages, N = 1024.
    Gradient, rows outside the ranges (sentinel) and both slab sets are bit-identical to the generic body; Cout 64 also against float64."""
    B, Cin, kw, stride, La1 = 3, 256, 8, 4, 256
    act, dy, w, abuf, dybuf, wd, bits, guard, La0 = _conv_case(B, Cin, Cout, kw, stride, La1, 7 + Cout)
    n = B * La0 * Cin
    ranges = ((10, 110), (110, 250))
    tiles = [-(-B * (hi - lo) // 256) for lo, hi in ranges]
    cs_tile = stride * Cin

    def run(flags):
        dx = full(guard + n + guard, BF)
        cs = full(sum(tiles) * cs_tile + 64, torch.float32)
        off = 0
        for (lo, hi), t in zip(ranges, tiles):
            a = (_hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(abuf, guard), _hip.ptr(dx, guard), B, Cin, Cout, kw, stride, La1,
                 C.c_longlong(guard), _hip.BF16, _hip.ptr(bits, guard // 8) if use_bits else None, _hip.ptr(cs, off * cs_tile), lo, hi)
            with debug_flags(flags | QUERY):
                assert raw("cpc_conv_dgrad_rows", *a) == (FORM_GENERIC if flags else FORM_DGRAD if use_bits else FORM_MASK)
            with debug_flags(flags):
                assert raw("cpc_conv_dgrad_rows", *a) == 0
            off += t
        return dx, cs

    dx, cs = run(0)
    dx_ref, cs_ref = run(GENERIC)
    assert torch.equal(dx, dx_ref) and torch.equal(cs, cs_ref)
    got = dx[guard:guard + n].view(B, La0, Cin)
    assert bool((got[:, :10 * stride] == SENTINEL).all()) and bool((got[:, 250 * stride:] == SENTINEL).all())
    assert bool((cs[sum(tiles) * cs_tile:] == SENTINEL).all()) and not bool((cs[:sum(tiles) * cs_tile] == SENTINEL).any())
    if Cout == 64:
        xin = act.to(BF).double().transpose(1, 2).clone().requires_grad_(True)
        out = F.conv1d(xin, w.to(BF).double(), None, stride=stride)
        (out * dy.to(BF).double()[:, :out.shape[2]].transpose(1, 2)).sum().backward()
        # (rows of dy beyond the convolution's last output position take part in the GEMM: zero them in the reference's view instead)
        ref = xin.grad.transpose(1, 2) * (act.to(BF).double() > 0)
        Lo = out.shape[2]
        hi_ok = min(250, Lo - 2) * stride                          # positions that only see dy rows the reference has too
        assert rel_err(got[:, 10 * stride:hi_ok], ref[:, 10 * stride:hi_ok]) < 1.2e-2        # tol(bf16) of the data-gradient tests


@pytest.mark.gpu
@pytest.mark.parametrize("Cout,stride,kw", [(64, 4, 8), (512, 4, 8), (64, 1, 2)])
def test_fused_layer1_form_is_bit_identical_to_the_generic_body(Cout, stride, kw):
    """cpc_conv_dgrad_conv1_rows on rows [10, 110) of 3 items of 128 (M = 300) with c1_kw = 10 and L1_valid cutting into the range, so the
    last windows of every clip run past c1_valid and count nothing; N = 1024 (stride 4) and 256 (stride 1), K of 2 and 16 stages.  The
    layer-1 slabs are bit-identical to the generic body's; for the first case the reduced weight and bias gradient are also checked against
    float64 sums over the gradient cpc_conv_dgrad_rows stores."""
    B, Cin, La1, kw1, s1 = 3, 256, 128, 10, 5
    lo, hi = 10, 110
    act, dy, w, abuf, dybuf, wd, bits, guard, La0 = _conv_case(B, Cin, Cout, kw, stride, La1, 11 + Cout + stride)
    Lv0 = (hi - 6) * stride - 1
    ldx = (La0 - 1) * s1 + kw1 + 3
    g = torch.Generator().manual_seed(5)
    xwave = torch.randn(B, ldx, generator=g)
    xd = xwave.to(DEV)
    tiles = -(-B * (hi - lo) // 256)
    c1_tile = (stride * Cin // 256) * (kw1 + 1) * 256

    def run(flags):
        slabs = full(tiles * c1_tile + 64, torch.float32)
        a = (_hip.ptr(dybuf, guard), _hip.ptr(wd), None, _hip.ptr(xd), _hip.ptr(slabs), B, Cin, Cout, kw, stride, La1, C.c_longlong(ldx), kw1,
             s1, Lv0, C.c_longlong(guard), _hip.BF16, _hip.ptr(bits, guard // 8), lo, hi)
        with debug_flags(flags | QUERY):
            assert raw("cpc_conv_dgrad_conv1_rows", *a) == (FORM_GENERIC if flags else FORM_C1)
        with debug_flags(flags):
            assert raw("cpc_conv_dgrad_conv1_rows", *a) == 0
        return slabs

    slabs, ref = run(0), run(GENERIC)
    assert torch.equal(slabs, ref)
    assert bool((slabs[tiles * c1_tile:] == SENTINEL).all())
    if (Cout, stride) == (64, 4):
        n = B * La0 * Cin
        dx = torch.zeros(guard + n + guard, device=DEV, dtype=BF)
        # (without column sums 300 rows take the 128 x 128 tile, which reads the full-size mask)
        _hip.call("cpc_conv_dgrad_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(abuf, guard), _hip.ptr(dx, guard), B, Cin, Cout, kw,
                  stride, La1, C.c_longlong(guard), _hip.BF16, None, None, lo, hi)
        G = dx[guard:guard + n].view(B, La0, Cin).double().cpu()[:, lo * stride:Lv0]
        win = xwave.double().unfold(1, kw1, s1)[:, lo * stride:Lv0]
        ref_w, ref_b = torch.einsum("btc,btj->cj", G, win), G.sum((0, 1))
        n_tmp = int(_hip.lib().cpc_conv_dgrad_conv1_floats(B, Cin, stride, La1, kw1, 1))
        tmp = full(n_tmp, torch.float32, float("nan"))
        dw = torch.full((Cin, 1, kw1), float("nan"), device=DEV)
        db = torch.full((Cin,), float("nan"), device=DEV)
        _hip.call("cpc_conv1_fused_reduce_tiles", _hip.ptr(slabs), _hip.ptr(tmp), _hip.ptr(dw), _hip.ptr(db), tiles, Cin, stride, kw1)
        assert rel_err(dw[:, 0, :], ref_w) < 2e-4          # the bound of the existing fused-gradient tests
        assert rel_err(db, ref_b) < 2e-4


@pytest.mark.gpu
def test_whole_launches_are_bit_identical_to_the_generic_body():
    """cpc_conv_dgrad (rows not in items, 50 x 4 tiles, the last row tile partial) and cpc_conv_dgrad_conv1 at the smallest size that takes
    the 256 x 256 tile without a row range: gradient, column sums and layer-1 slabs against the generic body."""
    B, Cin, Cout, kw, stride, La1, kw1, s1 = 8, 256, 64, 8, 4, 1590, 10, 5
    act, dy, w, abuf, dybuf, wd, bits, guard, La0 = _conv_case(B, Cin, Cout, kw, stride, La1, 3)
    n = B * La0 * Cin
    Lv0 = La0 - 7
    ldx = (La0 - 1) * s1 + kw1 + 3
    xd = torch.randn(B, ldx, generator=torch.Generator().manual_seed(9)).to(DEV)
    nf = int(_hip.lib().cpc_conv_dgrad_colsum_floats(B, Cin, stride, La1))
    ns = int(_hip.lib().cpc_conv_dgrad_conv1_floats(B, Cin, stride, La1, kw1, 0))

    def run(flags):
        dx, cs, slabs = full(guard + n + guard, BF), full(nf + 64, torch.float32), full(ns + 64, torch.float32)
        a = (_hip.ptr(dybuf, guard), _hip.ptr(wd), None, _hip.ptr(dx, guard), B, Cin, Cout, kw, stride, La1, Lv0, C.c_longlong(guard),
             _hip.BF16, _hip.ptr(bits, guard // 8), _hip.ptr(cs))
        b = (_hip.ptr(dybuf, guard), _hip.ptr(wd), None, _hip.ptr(xd), _hip.ptr(slabs), B, Cin, Cout, kw, stride, La1, C.c_longlong(ldx), kw1,
             s1, Lv0, C.c_longlong(guard), _hip.BF16, _hip.ptr(bits, guard // 8))
        with debug_flags(flags | QUERY):
            assert raw("cpc_conv_dgrad", *a) == (FORM_GENERIC if flags else FORM_DGRAD)
            assert raw("cpc_conv_dgrad_conv1", *b) == (FORM_GENERIC if flags else FORM_C1)
        with debug_flags(flags):
            assert raw("cpc_conv_dgrad", *a) == 0 and raw("cpc_conv_dgrad_conv1", *b) == 0
        return dx, cs, slabs

    for got, ref in zip(run(0), run(GENERIC)):
        assert torch.equal(got, ref)
