"""GPU unit tests of the audio path's entry points that only whole-model runs reached before: the encoder's row-range launches behind
the backward target lane (and the lane's stream ordering in the engine), the fused score gradient and the validation scores, the ConvAr
pooling and last-row ReLU backward, the GRU from a given initial state and its streaming switch, the weight casts, dropout, and the
scalogram front end's operand split and pointwise chain.

References are float64 PyTorch computations on the values the device sees (inputs rounded to the storage type first).  Every element a
call must not touch holds a sentinel before the call and is checked afterwards; where the code claims bit-identity (a row range against
one launch, a NULL output against a non-NULL one) the test asserts it.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from oracle import cpc_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 7.25          # exact in bf16 and f32, and not a value any kernel here produces from the test data
EINVAL = -22


def tol(dt):
    return 3e-5 if dt == torch.float32 else 1.2e-2


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def rounded(t, dt):
    return t.to(dt).double()


def raw(name, *args):
    """Return code of an entry point (no raise), on the current stream."""
    return getattr(_hip.lib(), name)(*args, _hip.stream_ptr())


def full(n, dt, value=SENTINEL):
    return torch.full((n,) if isinstance(n, int) else n, value, device=DEV, dtype=dt)


# ================================================================================ A. the backward target lane's stream ordering
def _sleep_cycles_for(ms):
    """torch.cuda._sleep cycles that spin about `ms` milliseconds (calibrated once with events)."""
    torch.cuda.synchronize()
    cycles = 1_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    per_ms = cycles / max(a.elapsed_time(b), 1e-3)
    return int(min(per_ms * ms, 4e9))


@pytest.mark.parametrize("wgrad_stream", ["1", "0"])
def test_target_lane_is_ordered_before_its_readers(monkeypatch, wgrad_stream):
    """bf16, default encoder, 64 clips, as test_target_lanes_equal_the_single_lane_step — but every side-stream launch of the backward
    lane (_lane_dgrad part 1) is preceded by a bounded ~20 ms spin on that stream, and the lane step runs on a DIFFERENT input than the
    step before it.  A main-stream reader of lane-written rows (the layer-1 slab reduction, a weight gradient) that does not wait on the
    lane's event then reads the previous input's numbers.  With CPC_WGRAD_STREAM=0 the engine does not take the lane at all; the test pins
    that the step stays right there as well."""
    monkeypatch.setenv("CPC_WGRAD_STREAM", wgrad_stream)
    B, L = 64, 20480
    g = torch.Generator().manual_seed(3)
    x1 = (torch.randn(B, L, generator=g) * 0.5).to(DEV)
    x2 = (torch.randn(B, L, generator=g) * 0.5).to(DEV)
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, compute_dtype="bf16")
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "encoder" in n and n.endswith("weight"):
                p.mul_(2.0)
    model.to(DEV)
    eng = model.engine(B, L)
    assert eng._target_lane_rows() is not None and eng._bwd_lane() is not None, "the headline configuration is expected to split"
    rows, bl = eng._tl_rows, eng._bl
    # reference: the same engine, one launch per layer, on x2
    eng._tl_rows, eng._bl = None, None
    out = eng.loss_and_grads(x2, softplus=True, regularization=1.0)
    ref_loss, ref = float(out[0]), model._flat_grad.detach().double().cpu().clone()
    # the lanes on x1, then on x2 with the side stream's lane launches delayed
    eng._tl_rows, eng._bl = rows, bl
    eng.loss_and_grads(x1, softplus=True, regularization=1.0)
    torch.cuda.synchronize()
    cycles = _sleep_cycles_for(20.0)
    orig = eng._lane_dgrad

    def delayed(bl_, l, part, x):
        if part == 1:
            torch.cuda._sleep(cycles)                  # on the current (side) stream: a finite spin in front of the launch
        return orig(bl_, l, part, x)

    monkeypatch.setattr(eng, "_lane_dgrad", delayed)
    out = eng.loss_and_grads(x2, softplus=True, regularization=1.0)
    loss, grad = float(out[0]), model._flat_grad.detach().double().cpu().clone()
    torch.cuda.synchronize()
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss), (loss, ref_loss)
    assert torch.isfinite(grad).all()
    for pname, gr in model._grad.items():
        lo = model._offset[pname]
        a, b = grad[lo:lo + gr.numel()], ref[lo:lo + gr.numel()]
        assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item() + 1e-12, pname


# ================================================================================ B. encoder row-range launches
def _ranges(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc,kw,stride", [(64, 10, 5), (512, 10, 5), (64, 7, 3), (512, 7, 3)])
@pytest.mark.parametrize("B,cut_rows", [(3, (85, 86)), (3, (171,)), (4, (64, 65))])
def test_conv1_fwd_rows_equal_one_launch(dt, Cc, kw, stride, B, cut_rows):
    """cpc_conv1_fwd_rows over ranges [0, L_alloc) is split into (rows with B * rows = 255 or 256 k + 1 or 256, a single row, up to
    L_alloc): each range is bit-identical to one cpc_conv1_fwd launch, rows outside it keep their sentinel, and for C = 512 the
    sign-bit bytes of the range equal the one-launch mask while the other bytes keep theirs."""
    g = torch.Generator().manual_seed(Cc + kw + B)
    L = 1234
    x = torch.randn(B, L, generator=g).to(DEV)
    w = (torch.randn(Cc, 1, kw, generator=g) * 0.3).to(DEV)
    bias = (torch.randn(Cc, generator=g) * 0.1).to(DEV)
    Lv = (L - kw) // stride + 1
    La = Lv + 3
    code = _hip.dtype_code(dt)
    cuts = (0,) + cut_rows + (La,)
    for relu in (0, 1):
        ref = full((B, La, Cc), dt)
        rbits = torch.zeros(B * La * Cc // 8, device=DEV, dtype=torch.uint8) if Cc == 512 else None
        _hip.call("cpc_conv1_fwd", _hip.ptr(x), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(ref), B, Cc, stride, kw, L, Lv, La, relu, code,
                  _hip.ptr(rbits))
        for lo, hi in _ranges(cuts):
            y = full((B, La, Cc), dt)
            bits = torch.full((B * La * Cc // 8,), 0xA5, device=DEV, dtype=torch.uint8) if Cc == 512 else None
            _hip.call("cpc_conv1_fwd_rows", _hip.ptr(x), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(y), B, Cc, stride, kw, L, Lv, La, relu,
                      code, _hip.ptr(bits), lo, hi)
            assert torch.equal(y[:, lo:hi], ref[:, lo:hi]), (lo, hi)
            assert bool((y[:, :lo] == SENTINEL).all()) and bool((y[:, hi:] == SENTINEL).all()), (lo, hi)
            if bits is not None:
                bv, rv = bits.view(B, La, Cc // 8), rbits.view(B, La, Cc // 8)
                assert torch.equal(bv[:, lo:hi], rv[:, lo:hi]), (lo, hi)
                assert bool((bv[:, :lo] == 0xA5).all()) and bool((bv[:, hi:] == 0xA5).all()), (lo, hi)
    # invalid ranges are refused
    y = full((B, La, Cc), dt)
    for lo, hi in ((-1, 5), (5, 5), (6, 5), (0, La + 1)):
        assert raw("cpc_conv1_fwd_rows", _hip.ptr(x), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(y), B, Cc, stride, kw, L, Lv, La, 1, code,
                   None, lo, hi) == EINVAL, (lo, hi)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


def _conv_operands(B, Cin, Cout, kw, stride, La_out, Lin_valid, dt, seed):
    g = torch.Generator().manual_seed(seed)
    La_in = La_out * stride
    guard = 16 * max(Cin, Cout)
    x = torch.relu(torch.randn(B, La_in, Cin, generator=g))
    x[:, Lin_valid:] = 0
    dy = torch.randn(B, La_out, Cout, generator=g)
    w = torch.randn(Cout, Cin, kw, generator=g) * 0.2

    def padded(t):
        buf = torch.zeros(guard + t.numel() + guard, device=DEV, dtype=dt)
        buf[guard:guard + t.numel()] = t.reshape(-1).to(DEV).to(dt)
        return buf

    D = -(-kw // stride)
    wd = torch.empty(stride * Cin * D * Cout, device=DEV, dtype=dt)
    wdev = w.to(DEV)
    _hip.call("cpc_conv_w_prep", _hip.ptr(wdev), None, _hip.ptr(wd), Cout, Cin, kw, stride, _hip.dtype_code(dt))
    return x, dy, w, padded(x), padded(dy), wd, guard, La_in


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cin,Cout,kw,stride", [(64, 64, 8, 4), (32, 64, 4, 2)])
def test_conv_dgrad_rows_against_float64(dt, Cin, Cout, kw, stride):
    """cpc_conv_dgrad_rows on [0, 5), [5, 6), [6, L_alloc): the pieces together are the float64 data gradient with the ReLU mask,
    bit-identical to one cpc_conv_dgrad launch, and every launch leaves input positions outside [lo stride, hi stride) alone."""
    B, Lin_valid = 3, 67
    Lout_valid = (Lin_valid - kw) // stride + 1
    La = Lout_valid + 2
    code = _hip.dtype_code(dt)
    x, dy, w, xbuf, dybuf, wd, guard, La_in = _conv_operands(B, Cin, Cout, kw, stride, La, Lin_valid, dt, Cin + kw)
    dy[:, Lout_valid:] = 0
    dybuf[guard:guard + dy.numel()] = dy.reshape(-1).to(DEV).to(dt)
    n = B * La_in * Cin
    one = full(guard + n + guard, dt)
    _hip.call("cpc_conv_dgrad", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(xbuf, guard), _hip.ptr(one, guard), B, Cin, Cout, kw,
              stride, La, La_in, C.c_longlong(guard), code, None, None)
    whole = full(guard + n + guard, dt)
    for lo, hi in _ranges((0, 5, 6, La)):
        piece = full(guard + n + guard, dt)
        _hip.call("cpc_conv_dgrad_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(xbuf, guard), _hip.ptr(piece, guard), B, Cin, Cout,
                  kw, stride, La, C.c_longlong(guard), code, None, None, lo, hi)
        pv = piece[guard:guard + n].view(B, La_in, Cin)
        assert bool((pv[:, :lo * stride] == SENTINEL).all()) and bool((pv[:, hi * stride:] == SENTINEL).all()), (lo, hi)
        assert bool((piece[:guard] == SENTINEL).all()) and bool((piece[guard + n:] == SENTINEL).all()), (lo, hi)
        whole[guard:guard + n].view(B, La_in, Cin)[:, lo * stride:hi * stride] = pv[:, lo * stride:hi * stride]
    assert torch.equal(whole[guard:guard + n], one[guard:guard + n])
    xin = rounded(x, dt)[:, :Lin_valid].transpose(1, 2).clone().requires_grad_(True)
    out = F.conv1d(xin, rounded(w, dt), None, stride=stride)
    (out * rounded(dy, dt)[:, :Lout_valid].transpose(1, 2)).sum().backward()
    ref = xin.grad.transpose(1, 2) * (rounded(x, dt)[:, :Lin_valid] > 0)
    got = whole[guard:guard + n].view(B, La_in, Cin)
    assert rel_err(got[:, :Lin_valid], ref) < tol(dt)
    assert (got[:, Lin_valid:] == 0).all()
    for lo, hi in ((-1, 3), (4, 4), (0, La + 1)):
        assert raw("cpc_conv_dgrad_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(xbuf, guard), _hip.ptr(whole, guard), B, Cin, Cout,
                   kw, stride, La, C.c_longlong(guard), code, None, None, lo, hi) == EINVAL, (lo, hi)


@pytest.mark.parametrize("Cin,B,La1,cuts", [(256, 8, 1600, (32, 1000)), (512, 5, 1312, (205, 700))])
def test_conv_dgrad_rows_bits_colsum_and_fused_layer1(Cin, B, La1, cuts):
    """bf16 at the engine's widths, ranges split at rows with B * rows = 256 and 256 k + 1 (these kernels take whole 256-row tiles
    worth of rows at least, as the engine's lane does):
    - cpc_conv_dgrad_rows with the sign-bit mask and per-tile column sums: each launch writes its tiles' slabs at its own offset; the
      pieces are bit-identical to one cpc_conv_dgrad launch, and the summed slabs are the column sums of the stored gradient;
    - cpc_conv_dgrad_conv1_rows into consecutive tile offsets (x_act and sign bits give identical slabs) + cpc_conv1_fused_reduce_tiles:
      layer 1's weight and bias gradient against float64, with L1_valid cutting into the last range;
    - launches below one 256-row tile and invalid ranges are refused."""
    dt, code = torch.bfloat16, _hip.BF16
    Cout, kw, stride, kw1, s1 = 64, 8, 4, 10, 5
    La0 = stride * La1
    Lv0 = La0 - 7
    ldx = (La0 - 1) * s1 + kw1 + 3
    x, dy, w, abuf, dybuf, wd, guard, _ = _conv_operands(B, Cin, Cout, kw, stride, La1, Lv0, dt, Cin + B)
    g = torch.Generator().manual_seed(Cin * 3 + B)
    xwave = torch.randn(B, ldx, generator=g)
    xd = xwave.to(DEV)
    bits = torch.zeros(abuf.numel() // 8, device=DEV, dtype=torch.uint8)
    _hip.call("cpc_sign_bits", _hip.ptr(abuf), _hip.ptr(bits), C.c_longlong(abuf.numel()), code)
    n = B * La0 * Cin
    one = torch.zeros(guard + n + guard, device=DEV, dtype=dt)
    _hip.call("cpc_conv_dgrad", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(abuf, guard), _hip.ptr(one, guard), B, Cin, Cout, kw,
              stride, La1, La0, C.c_longlong(guard), code, None, None)
    rng = _ranges((0,) + cuts + (La1,))
    tiles = [-(-B * (hi - lo) // 256) for lo, hi in rng]
    # data gradient with bits and per-tile column sums
    cs_tile = stride * Cin
    cs = full(sum(tiles) * cs_tile + 64, torch.float32)
    dx = full(guard + n + guard, dt)
    off = 0
    for (lo, hi), t in zip(rng, tiles):
        _hip.call("cpc_conv_dgrad_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), None, _hip.ptr(dx, guard), B, Cin, Cout, kw, stride, La1,
                  C.c_longlong(guard), code, _hip.ptr(bits, guard // 8), _hip.ptr(cs, off * cs_tile), lo, hi)
        off += t
    assert torch.equal(dx[guard:guard + n], one[guard:guard + n])
    assert bool((cs[sum(tiles) * cs_tile:] == SENTINEL).all())
    got = torch.zeros(Cin, device=DEV)
    _hip.call("cpc_reduce_slabs", _hip.ptr(cs), _hip.ptr(got), 1, Cin, sum(tiles) * stride, Cin, 1, 1, 0, 0)
    want = dx[guard:guard + n].view(-1, Cin).double().sum(0)
    assert rel_err(got, want) < 1e-5
    # the fused layer-1 weight gradient
    G = one[guard:guard + n].view(B, La0, Cin).double().cpu()[:, :Lv0]
    win = xwave.double().unfold(1, kw1, s1)[:, :Lv0]
    ref_w = torch.einsum("btc,btj->cj", G, win)
    ref_b = G.sum((0, 1))
    c1_tile = (stride * Cin // 256) * (kw1 + 1) * 256
    n_tmp = int(_hip.lib().cpc_conv_dgrad_conv1_floats(B, Cin, stride, La1, kw1, 1))
    results = []
    for mask, mbits in ((abuf, None), (None, bits)):
        slabs = full(sum(tiles) * c1_tile + 64, torch.float32)
        off = 0
        for (lo, hi), t in zip(rng, tiles):
            _hip.call("cpc_conv_dgrad_conv1_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(mask, guard), _hip.ptr(xd),
                      _hip.ptr(slabs, off * c1_tile), B, Cin, Cout, kw, stride, La1, ldx, kw1, s1, Lv0, C.c_longlong(guard), code,
                      _hip.ptr(mbits, guard // 8), lo, hi)
            off += t
        assert bool((slabs[sum(tiles) * c1_tile:] == SENTINEL).all())
        results.append(slabs)
    assert torch.equal(results[0], results[1])
    tmp = full(n_tmp, torch.float32, float("nan"))
    dw = full((Cin, 1, kw1), torch.float32, float("nan"))
    db = full((Cin,), torch.float32, float("nan"))
    _hip.call("cpc_conv1_fused_reduce_tiles", _hip.ptr(results[0]), _hip.ptr(tmp), _hip.ptr(dw), _hip.ptr(db), sum(tiles), Cin, stride, kw1)
    assert rel_err(dw[:, 0, :], ref_w) < 2e-4
    assert rel_err(db, ref_b) < 2e-4
    # refused: M = B * rows < 256 for the bits / column-sum and fused kernels, invalid ranges, no row tiles
    small = 255 // B
    assert raw("cpc_conv_dgrad_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), None, _hip.ptr(dx, guard), B, Cin, Cout, kw, stride, La1,
               C.c_longlong(guard), code, _hip.ptr(bits, guard // 8), _hip.ptr(cs), 0, small) == EINVAL
    for lo, hi in ((0, small), (-1, 300), (300, 300), (0, La1 + 1)):
        assert raw("cpc_conv_dgrad_conv1_rows", _hip.ptr(dybuf, guard), _hip.ptr(wd), _hip.ptr(abuf, guard), _hip.ptr(xd), _hip.ptr(results[1]),
                   B, Cin, Cout, kw, stride, La1, ldx, kw1, s1, Lv0, C.c_longlong(guard), code, None, lo, hi) == EINVAL, (lo, hi)
    assert raw("cpc_conv1_fused_reduce_tiles", _hip.ptr(results[0]), _hip.ptr(tmp), _hip.ptr(dw), _hip.ptr(db), 0, Cin, stride, kw1) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(results[0], results[1])


# ================================================================================ C. score kernels
def _fused_grad_case(items, K, softplus, reg, seed):
    """A row-and-column strip of a square all-timesteps problem of items + 3 items: rows of items [1, 1 + items), columns
    [4, 4 + ncols) with ncols % 8 == 4 (diag_off = K - 4).  Returns the device operands and the float64 autograd gradient of the
    oracle loss restricted to the strip."""
    it_tot = items + 3
    R = it_tot * K
    lo_c = 4
    ncols = (R - lo_c - 4) // 8 * 8 + 4
    g = torch.Generator().manual_seed(seed)
    lin = (torch.randn(R, R, generator=g) * 2.0).float().double()
    lin[K, K] = 25.0                                   # the softplus threshold branch
    lin.requires_grad_(True)
    sc = F.softplus(lin) if softplus else lin
    loss, _ = O.info_nce_loss(sc.view(it_tot, K, it_tot, K), all_timesteps=True, regularization=reg)
    loss.backward()
    lse = torch.logsumexp(sc.detach(), dim=0)
    rows = slice(K, K + items * K)
    cols = slice(lo_c, lo_c + ncols)
    ld = ncols + 12
    Sp = torch.full((items * K, ld), 1e4)             # pad columns hold junk the kernel must ignore
    Sp[:, :ncols] = lin.detach()[rows, cols]
    m = (sc.detach()[rows, cols].view(items, K, ncols)).mean(1)
    return SimpleCase(S=Sp.float().to(DEV), lse=lse[cols].float().to(DEV), ref=lin.grad[rows, cols], msq=(m ** 2).sum().item(),
                      ncols=ncols, ld=ld, R=R, it_tot=it_tot, diag_off=K - lo_c)


class SimpleCase:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("items", [1, 3, 17, 33])
@pytest.mark.parametrize("K", [2, 6, 10, 12, 14, 24])
def test_nce_fused_grad_partial_item_blocks_and_runtime_k(softplus, items, K):
    """cpc_nce_fused_grad on a strip (diag_off != 0, ncols % 8 == 4, ld > ncols) with partial last item blocks, for the compile-time K
    kernels and the run-time K one: dS and dS^T against float64 autograd of the oracle loss, the regulariser partials, the pad columns
    of dS and dS^T untouched, and dST = NULL / gradp = NULL give the same dS bit for bit.
    (Per-element bounds and the exact-data twins of this kernel: test_fused_score_kernels_gpu.py.)"""
    reg = 0.5
    c = _fused_grad_case(items, K, softplus, reg, items * 31 + K)
    ldT = (items * K // 8 + 1) * 8
    nb = int(_hip.lib().cpc_nce_fused_grad_blocks(items, c.ncols))
    dS = full((items * K, c.ld), torch.bfloat16)
    dST = full((c.ncols, ldT), torch.bfloat16)
    gradp = full(nb + 8, torch.float32)
    args = (items, K, c.ncols, C.c_longlong(c.ld), C.c_longlong(ldT), c.diag_off, softplus, C.c_float(reg), C.c_float(c.R),
            C.c_float(c.it_tot))
    _hip.call("cpc_nce_fused_grad", _hip.ptr(c.S), _hip.ptr(c.lse), _hip.ptr(dS), _hip.ptr(dST), _hip.ptr(gradp), *args)
    assert rel_err(dS[:, :c.ncols].float(), c.ref) < 1.5e-2
    assert bool((dS[:, c.ncols:] == SENTINEL).all()), "dS pad columns written"
    assert torch.equal(dST[:, :items * K], dS[:, :c.ncols].T), "dS^T is not the transpose of dS"
    assert bool((dST[:, items * K:] == SENTINEL).all()), "dS^T pad columns written"
    assert abs(gradp[:nb].double().sum().item() - c.msq) <= 1e-5 * c.msq
    assert bool((gradp[nb:] == SENTINEL).all())
    dS2 = full((items * K, c.ld), torch.bfloat16)
    _hip.call("cpc_nce_fused_grad", _hip.ptr(c.S), _hip.ptr(c.lse), _hip.ptr(dS2), None, None, *args)
    assert torch.equal(dS2, dS)


def _eval_ref(S, B, K, softplus, all_t):
    """oracle.validation_terms in float64 on the device's f32 scores (S as the kernel reads it)."""
    S = S.double().cpu()
    sc = F.softplus(S) if softplus else S
    if all_t:
        s4 = sc[:, :B * K].reshape(B, K, B, K)
    else:
        s3 = sc[:, :B].reshape(K, B, B)                  # [k][b][b']
        s4 = torch.zeros(B, K, B, K, dtype=torch.float64)
        for k in range(K):
            s4[:, k, :, k] = s3[k]
    losses, acc, mean = O.validation_terms(s4, all_timesteps=all_t)
    return torch.cat([losses, acc, mean.view(1)])


def _eval_scores(B, K, all_t, ld, g, ties=False, nans=False):
    rows, cols = (B * K, B * K) if all_t else (K * B, B)
    S = torch.randn(rows, ld, generator=g) * 2.0
    S[:, cols:] = 1e4                                  # columns beyond the row's targets: ignored
    diag = (lambda r: r) if all_t else (lambda r: r % B)
    if ties and cols >= 3:
        for r in range(0, rows, 2):                    # the own target ties with an EARLIER column (first maximum wins: a miss) ...
            d = diag(r)
            S[r, :cols] = torch.linspace(-3, 1, cols)
            S[r, d] = 5.0
            S[r, (d + 1) % cols if d == 0 else 0] = 5.0
        for r in range(1, rows, 2):                    # ... or with a LATER one (a hit)
            d = diag(r)
            if d + 1 < cols:
                S[r, :cols] = torch.linspace(-3, 1, cols)
                S[r, d] = 5.0
                S[r, cols - 1] = 5.0
    if nans and cols >= 8:
        for r in range(rows):
            d = diag(r)
            if d + 1 < cols and r % 3 == 0:            # first NaN at the own target, a second one in the next lane: a hit
                S[r, d] = float("nan")
                S[r, d + 1] = float("nan")
            elif d >= 1 and r % 3 == 1:                 # first NaN in front of the own target: a miss
                S[r, d - 1] = float("nan")
                S[r, d] = float("nan")
    return S.float()


@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("all_t", [0, 1])
@pytest.mark.parametrize("B,K", [(1, 1), (5, 3), (33, 12), (1, 12), (33, 1), (5, 12), (70, 2), (257, 1)])
@pytest.mark.parametrize("special", ["", "ties", "nans"])
def test_nce_eval_against_oracle(softplus, all_t, B, K, special):
    """cpc_nce_eval (the validate() quantities) against oracle.validation_terms in float64: both branches (all-timesteps R below and
    at least 128: the one-way and the 16-way column split), default-branch ld = B and B + 7, exact ties (the first maximum wins), rows
    with NaN in two lanes (the first NaN wins, as torch.argmax), accumulate over two batches, and nothing written behind the workspace
    cpc_nce_eval_workspace_floats sizes."""
    g = torch.Generator().manual_seed(B * 100 + K * 7 + softplus + 2 * all_t + len(special))
    R = B * K
    lds = [R + 5] if all_t else [B, B + 7]
    nw = int(_hip.lib().cpc_nce_eval_workspace_floats(B, K))
    for ld in lds:
        S1 = _eval_scores(B, K, all_t, ld, g, ties=special == "ties", nans=special == "nans")
        S2 = _eval_scores(B, K, all_t, ld, g)
        ws = full(nw + 64, torch.float32)
        out = full(2 * K + 1 + 8, torch.float32)
        for i, S in enumerate((S1, S2)):
            Sd = S.to(DEV)
            _hip.call("cpc_nce_eval", _hip.ptr(Sd), _hip.ptr(out), _hip.ptr(ws), B, K, ld, softplus, all_t, 1 if i else 0)
            if i == 0:
                first = out[:2 * K + 1].double().cpu().clone()
        assert bool((ws[nw:] == SENTINEL).all()), "written behind the workspace"
        assert bool((out[2 * K + 1:] == SENTINEL).all())
        r1, r2 = _eval_ref(S1, B, K, softplus, all_t), _eval_ref(S2, B, K, softplus, all_t)
        assert torch.equal(first[K:2 * K], r1[K:2 * K].float().double()), (ld, first[K:2 * K], r1[K:2 * K])      # hits / n, one rounding
        for got, ref in ((first, r1), (out[:2 * K + 1].double().cpu(), r1 + r2)):
            loss_g, loss_r = got[:K], ref[:K]
            assert torch.equal(torch.isnan(loss_g), torch.isnan(loss_r)), (ld, loss_g, loss_r)
            ok = ~torch.isnan(loss_r)
            assert ((loss_g - loss_r)[ok].abs() <= 2e-5 * loss_r[ok].abs().clamp(min=1.0)).all(), (ld, loss_g, loss_r)
            assert ((got[K:2 * K] - ref[K:2 * K]).abs() <= 1e-6).all(), (ld, got[K:2 * K], ref[K:2 * K])
            if not torch.isnan(ref[2 * K]):
                assert abs(got[2 * K] - ref[2 * K]) <= 2e-5 * max(1.0, abs(ref[2 * K].item()))
    assert raw("cpc_nce_eval", _hip.ptr(out), _hip.ptr(out), _hip.ptr(ws), B, K, B + 8, softplus, 0, 0) == EINVAL


# ================================================================================ D. ConvAr context kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pool", [2, 3, 5])
@pytest.mark.parametrize("special", ["", "ties", "nans"])
def test_maxpool_fwd_bwd_against_torch(dt, pool, special):
    """cpc_maxpool_fwd / _bwd against float64 F.max_pool1d(ceil_mode=True) and its autograd with Lin_valid % pool != 0 and pad rows
    on both sides: pad rows of out and din are zero; windows of ties send the gradient to the first maximum; a NaN in a window is the
    window's maximum and takes the gradient (torch's rule: the running maximum is replaced by a greater element or a NaN, so a window
    holding two NaNs sends it to the later one)."""
    B, Cc = 3, 12
    Lin_valid = 7 * pool + 2
    Lout_valid = -(-Lin_valid // pool)
    Lin_alloc, Lout_alloc = Lin_valid + 3, Lout_valid + 2
    g = torch.Generator().manual_seed(pool * 10 + len(special))
    x = torch.randn(B, Lin_alloc, Cc, generator=g)
    if special == "ties":
        x = torch.round(x)                               # many equal values in a window
        x[:, :, 0] = 1.0                                 # a channel that is all ties
    if special == "nans":
        x[0, 1, 0] = float("nan")                        # one NaN in a window
        x[1, 0, 1] = float("nan")
        x[1, pool - 1, 1] = float("nan")                 # two NaN in one window
        x[2, Lin_valid - 1, 2] = float("nan")            # in the partial last window
    x[:, Lin_valid:] = SENTINEL * 3                      # beyond Lin_valid: never read into a window
    code = _hip.dtype_code(dt)
    xd = x.to(DEV).to(dt)
    out = full((B, Lout_alloc, Cc), dt)
    _hip.call("cpc_maxpool_fwd", _hip.ptr(xd), _hip.ptr(out), B, Cc, pool, Lin_valid, Lin_alloc, Lout_valid, Lout_alloc, code)
    xr = rounded(x, dt)[:, :Lin_valid].transpose(1, 2).clone().requires_grad_(True)
    ref = F.max_pool1d(xr, pool, pool, ceil_mode=True)
    assert ref.shape[2] == Lout_valid
    got = out[:, :Lout_valid].double().cpu().transpose(1, 2)
    assert torch.equal(torch.isnan(got), torch.isnan(ref.detach()))
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref.detach(), nan=0.0))
    assert (out[:, Lout_valid:] == 0).all()
    dout = torch.randn(B, Lout_alloc, Cc, generator=g)
    dout[:, Lout_valid:] = 0
    ref.backward(rounded(dout, dt)[:, :Lout_valid].transpose(1, 2))
    din = full((B, Lin_alloc, Cc), dt)
    doutd = dout.to(DEV).to(dt)
    _hip.call("cpc_maxpool_bwd", _hip.ptr(xd), _hip.ptr(doutd), _hip.ptr(din), B, Cc, pool, Lin_valid, Lin_alloc,
              Lout_alloc, code)
    assert torch.equal(din[:, :Lin_valid].double().cpu().transpose(1, 2), xr.grad)
    assert (din[:, Lin_valid:] == 0).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_relu_row_bwd_writes_one_row(dt):
    """cpc_relu_row_bwd writes dy[b item_stride + row_off + c] = y > 0 ? dc : 0 only (y = +0 and -0 give 0); every other element keeps
    its sentinel."""
    B, Cc, rows = 5, 40, 6
    item_stride, row_off = rows * Cc + 8, 3 * Cc
    g = torch.Generator().manual_seed(7)
    y = torch.randn(B * item_stride, generator=g)
    yv = y.view(-1)
    idx = torch.arange(B).unsqueeze(1) * item_stride + row_off + torch.arange(Cc).unsqueeze(0)
    yv[idx[:, 0]] = 0.0
    yv[idx[:, 1]] = -0.0
    dc = torch.randn(B, Cc, generator=g)
    code = _hip.dtype_code(dt)
    yd = y.to(DEV).to(dt)
    dy = full(B * item_stride, dt)
    dcd = dc.to(DEV)
    _hip.call("cpc_relu_row_bwd", _hip.ptr(dcd), _hip.ptr(yd), _hip.ptr(dy), B, Cc, C.c_longlong(item_stride), C.c_longlong(row_off), code)
    want = torch.full((B * item_stride,), SENTINEL, dtype=torch.float64)
    yr = rounded(y, dt)
    want[idx.reshape(-1)] = torch.where(yr[idx] > 0, rounded(dc, dt), torch.zeros(())).reshape(-1)
    assert torch.equal(dy.double().cpu(), want)


# ================================================================================ E. GRU
def _gru_ref(Gi, w, b, h0, V, H):
    h = h0
    hs = [h]
    for t in range(V):
        gh = h @ w.T + b
        r = torch.sigmoid(Gi[:, t, :H] + gh[:, :H])
        u = torch.sigmoid(Gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(Gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - u) * n + u * h
        hs.append(h)
    return h, torch.stack(hs, 1)


def per_step_err(got, ref):
    """(B, V, X) -> max over the steps t of max_{b,j} |got - ref| / max_{b,j} |ref| within step t: the gradient of a recurrence decays
    backwards through time, so a maximum over the whole tensor hides the early steps."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().amax((0, 2)) / (ref.abs().amax((0, 2)) + 1e-30)).max().item()


def _gru_case(dt, B, V, H, streaming, with_bwd):
    g = torch.Generator().manual_seed(B * 7 + H + streaming)
    code = _hip.dtype_code(dt)
    w_hh = torch.randn(3 * H, H, generator=g) / math.sqrt(H)
    b_hh = torch.randn(3 * H, generator=g) * 0.1
    Gi = torch.randn(B, V, 3 * H, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.5
    dW, db = w_hh.to(DEV), b_hh.to(DEV)
    wfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wfrag), 3 * H, H, H, 0, code)
    Gid = Gi.to(DEV).to(dt)
    nt = _hip.lib().cpc_gru_tape_elems(B, V, H, code)
    Hall = full((B, V + 1, H), dt)
    tape = torch.zeros(nt, device=DEV, dtype=dt)
    c = full((B, H), torch.float32)
    h0d = h0.to(DEV)
    _hip.call("cpc_gru_fwd_h0", _hip.ptr(Gid), _hip.ptr(wfrag), _hip.ptr(db), _hip.ptr(h0d), _hip.ptr(Hall), _hip.ptr(tape), _hip.ptr(c),
              B, V, H, code)
    wr, br, gir = rounded(w_hh, dt), b_hh.double(), rounded(Gi, dt)
    h, hs = _gru_ref(gir, wr, br, h0.double(), V, H)
    t_f = 2e-5 if dt == torch.float32 else 2e-2
    assert rel_err(c, h) < t_f
    assert rel_err(Hall, hs) < t_f
    assert torch.equal(Hall[:, 0], h0d.to(dt)), "Hall[:, 0] is not the stored h0"
    # h0 = NULL is the zero initial state, bit for bit what cpc_gru_fwd computes
    Hn, cn = full((B, V + 1, H), dt), full((B, H), torch.float32)
    Hf, cf = full((B, V + 1, H), dt), full((B, H), torch.float32)
    tn, tf = torch.zeros(nt, device=DEV, dtype=dt), torch.zeros(nt, device=DEV, dtype=dt)
    _hip.call("cpc_gru_fwd_h0", _hip.ptr(Gid), _hip.ptr(wfrag), _hip.ptr(db), None, _hip.ptr(Hn), _hip.ptr(tn), _hip.ptr(cn), B, V, H, code)
    _hip.call("cpc_gru_fwd", _hip.ptr(Gid), _hip.ptr(wfrag), _hip.ptr(db), _hip.ptr(Hf), _hip.ptr(tf), _hip.ptr(cf), B, V, H, code)
    assert torch.equal(Hn, Hf) and torch.equal(cn, cf) and torch.equal(tn, tf)
    if not with_bwd:
        return
    wTfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wTfrag), H, 3 * H, H, 1, code)
    dc = torch.randn(B, H, generator=g)
    gir0 = gir.clone().requires_grad_(True)
    wr0 = wr.clone().requires_grad_(True)
    hz, _ = _gru_ref(gir0, wr0, br, torch.zeros(B, H, dtype=torch.float64), V, H)
    (hz * dc.double()).sum().backward()
    dG = full((B, V, 4 * H), dt)
    dcd = dc.to(DEV)
    _hip.call("cpc_gru_bwd", _hip.ptr(dcd), _hip.ptr(tf), _hip.ptr(wTfrag), _hip.ptr(dG), B, V, H, code)
    t_b = 5e-5 if dt == torch.float32 else 4e-2
    assert per_step_err(dG[:, :, :3 * H], gir0.grad) < t_b
    dGh = torch.cat([dG[:, :, :2 * H], dG[:, :, 3 * H:]], dim=2)
    dWhh = torch.einsum("bvg,bvh->gh", dGh.double().cpu(), Hf[:, :V].double().cpu())
    assert rel_err(dWhh, wr0.grad) < t_b


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [32, 64, 128, 256, 96])
@pytest.mark.parametrize("B", [1, 7, 33])
def test_gru_fwd_h0_against_float64(dt, H, B):
    """cpc_gru_fwd_h0 from a random initial state (the weight-resident bf16 kernels at H = 32 .. 256 with partial batch tiles, the
    generic kernels otherwise) against the float64 GRUCell loop; Hall[:, 0] = h0; h0 = NULL is cpc_gru_fwd bit for bit."""
    _gru_case(dt, B, 9, H, 0, with_bwd=False)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [32, 64, 128, 256])
@pytest.mark.parametrize("B", [1, 7, 33])
def test_gru_streaming_switch_at_resident_sizes(dt, H, B):
    """cpc_gru_set_streaming(1) forces the weight-streaming kernels at the sizes the resident ones take: the forward from h0, the
    forward from zero and the backward still match float64; the switch returns its previous setting and is restored."""
    lib = _hip.lib()
    torch.cuda.synchronize()
    assert lib.cpc_gru_set_streaming(1) == 0
    try:
        assert lib.cpc_gru_set_streaming(1) == 1
        _gru_case(dt, B, 6, H, 1, with_bwd=True)
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        lib.cpc_gru_set_streaming(0)
    assert lib.cpc_gru_set_streaming(0) == 0


# ================================================================================ F. casts, split, dropout, pointwise
def _special_values():
    f = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, -1.0,
                      1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,                    # bf16 round-to-even ties (down, up)
                      -(1.0 + 2.0 ** -8), 3.0e38, 1e-40, -1e-40, 1.2e-38], dtype=torch.float32)
    return f


def _check_cast(got, src, dt):
    want = src.to(dt)
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn)
    if dt == torch.float32:
        gb, wb = got[~gn].view(torch.int32), want[~wn].view(torch.int32)
        # subnormal f32 inputs: exact (the device keeps them) or a zero of the same sign (flushed)
        sub = (src[~wn].abs() < 1.1754944e-38) & (src[~wn] != 0)
        ok = (gb == wb) | (sub.to(DEV) & (got[~gn] == 0) & (torch.signbit(got[~gn]) == torch.signbit(want[~wn])))
        assert bool(ok.all())
        return bool((gb[sub.to(DEV)] == wb[sub.to(DEV)]).all()) if bool(sub.any()) else None
    gb, wb = got[~gn].view(torch.int16), want[~wn].view(torch.int16)
    sub = ((src[~wn].abs() < 1.1754944e-38) & (src[~wn] != 0)).to(DEV)
    ok = (gb == wb) | (sub & (got[~gn] == 0) & (torch.signbit(got[~gn].float()) == torch.signbit(want[~wn].float())))
    assert bool(ok.all())
    return bool((gb[sub] == wb[sub]).all()) if bool(sub.any()) else None


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("R,Cc,transposed", [(7, 13, False), (37, 45, False), (129, 67, False), (70, 59, True), (33, 200, True)])
def test_cast2d_bit_exact(dt, R, Cc, transposed):
    """cpc_cast2d (element path below 4096 elements, 32 x 32 tile path above it with sc == 1 and with the transposed read) is torch's
    .to(dt) bit for bit, ragged R and C, with +-0, +-inf, NaN, round-to-even ties and f32 subnormals among the values."""
    g = torch.Generator().manual_seed(R * Cc)
    src = torch.randn(R, Cc, generator=g)
    sv = _special_values()
    src.view(-1)[:sv.numel()] = sv
    base = src.T.contiguous() if transposed else src                    # the array in memory
    sr, sc = (1, R) if transposed else (Cc, 1)
    dst = full((R, Cc + 1), dt)                                          # one column of room: checked below
    flat = dst.view(-1)[:R * Cc]
    based = base.to(DEV)
    _hip.call("cpc_cast2d", _hip.ptr(based), _hip.ptr(flat), R, Cc, C.c_longlong(sr), C.c_longlong(sc), _hip.dtype_code(dt))
    _check_cast(flat.view(R, Cc), src.to(DEV), dt)
    assert bool((dst.view(-1)[R * Cc:] == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_cast2d_batch_bit_exact(dt):
    """cpc_cast2d_batch: three jobs of different shapes (one of them a transposed read) in one device table, each torch's .to(dt)."""
    g = torch.Generator().manual_seed(11)
    shapes = [(5, 7, False), (64, 33, True), (300, 17, False)]
    srcs, bases, dsts, rec = [], [], [], []
    for R, Cc, tr in shapes:
        s = torch.randn(R, Cc, generator=g)
        s.view(-1)[:14] = _special_values()
        b = (s.T.contiguous() if tr else s).to(DEV)
        d = full(R * Cc + 16, dt)
        srcs.append(s), bases.append(b), dsts.append(d)
        sr, sc = (1, R) if tr else (Cc, 1)
        rec += [b.data_ptr(), d.data_ptr(), R, Cc, sr, sc]
    table = torch.tensor(rec, dtype=torch.int64).to(DEV)
    _hip.call("cpc_cast2d_batch", _hip.ptr(table), len(shapes), _hip.dtype_code(dt))
    for (R, Cc, _), s, d in zip(shapes, srcs, dsts):
        _check_cast(d[:R * Cc].view(R, Cc), s.to(DEV), dt)
        assert bool((d[R * Cc:] == SENTINEL).all())


def test_split3_bf16_layout_and_accuracy():
    """cpc_split3_bf16: (hi, lo, hi) per sample, hi = bf16(x), lo = bf16(x - hi), bit for bit; |hi + lo - x| <= 2^-16 |x|."""
    n = 4099
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 3)
    x[:4] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, -3.0])
    dst = full(3 * n + 8, torch.bfloat16)
    xd = x.to(DEV)
    _hip.call("cpc_split3_bf16", _hip.ptr(xd), _hip.ptr(dst), C.c_longlong(n))
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    got = dst[:3 * n].view(n, 3).cpu()
    assert torch.equal(got[:, 0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(got[:, 1].view(torch.int16), lo.view(torch.int16))
    assert torch.equal(got[:, 2].view(torch.int16), hi.view(torch.int16))
    assert bool(((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -16 * x.double().abs()).all())
    assert bool((dst[3 * n:] == SENTINEL).all())


M64 = (1 << 64) - 1


def _drop_hash(seed, site, idx):
    """csrc/attn.hip drop_hash restated with uint64 arithmetic (numpy wraps modulo 2^64)."""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(site) + np.uint64(1))
             + idx.astype(np.uint64) * np.uint64(0xD1B54A32D192ED03))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint64)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_is_the_documented_hash(dt, p):
    """cpc_dropout_mask is the hash restated here bit for bit; cpc_dropout is x * mask rounded once to dt; p = 0 is the identity;
    another site gives another mask."""
    n, seed, site = 10007, 0x1234_5678_9ABC_DEF1, 3
    idx = np.arange(n, dtype=np.uint64)
    thresh = min(4294967295.0, float(np.float64(np.float32(p)) * 4294967296.0))
    keep = _drop_hash(seed, site, idx) >= np.uint64(int(thresh))
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    want = torch.from_numpy(np.where(keep, inv, np.float32(0.0)).astype(np.float32))
    mask = full(n + 8, torch.float32)
    _hip.call("cpc_dropout_mask", _hip.ptr(mask), C.c_longlong(n), C.c_float(p), C.c_ulonglong(seed), C.c_uint(site))
    assert torch.equal(mask[:n].cpu(), want)
    assert bool((mask[n:] == SENTINEL).all())
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(dt)
    xd = torch.cat([x, torch.full((8,), SENTINEL, dtype=dt)]).to(DEV)
    _hip.call("cpc_dropout", _hip.ptr(xd), C.c_longlong(n), C.c_float(p), C.c_ulonglong(seed), C.c_uint(site), _hip.dtype_code(dt))
    assert torch.equal(xd[:n].cpu(), (x.float() * want).to(dt))
    assert bool((xd[n:] == SENTINEL).all())
    x0 = x.to(DEV)
    _hip.call("cpc_dropout", _hip.ptr(x0), C.c_longlong(n), C.c_float(0.0), C.c_ulonglong(seed), C.c_uint(site), _hip.dtype_code(dt))
    assert torch.equal(x0.cpu(), x)
    other = full(n, torch.float32)
    _hip.call("cpc_dropout_mask", _hip.ptr(other), C.c_longlong(n), C.c_float(p), C.c_ulonglong(seed), C.c_uint(site + 1))
    assert not torch.equal(other, mask[:n])


def _pointwise_ref(cq, fixed, scale, B, Tn, bins, phase, offset, log_offset, norm, power, ph, pw):
    z = cq[:, :, :2 * bins].reshape(B, Tn, bins, 2)
    amp = torch.log(z[..., 0] ** 2 + z[..., 1] ** 2 + offset) + log_offset           # (B, Tn, bins)
    if phase:
        ang = torch.atan2(z[..., 1], z[..., 0])
        pd = ang[:, 1:] - ang[:, :-1] + fixed
        pd = torch.where(pd > math.pi, pd - 2 * math.pi, pd)
        pd = torch.where(pd < -math.pi, pd + 2 * math.pi, pd)
        x = torch.stack([amp[:, 1:], pd * scale], 1)                                 # (B, 2, W, bins)
    else:
        x = amp.unsqueeze(1)
    x = F.max_pool2d(x.transpose(2, 3), [ph, pw]) if (ph, pw) != (1, 1) else x.transpose(2, 3)    # (B, Cc, bins', W')
    x = x * norm
    if power != 1:
        x = x ** power
    return x.permute(0, 3, 2, 1)                                                     # (B, W', bins', Cc)


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("ph,pw,power", [(1, 1, 1.0), (3, 2, 2.0), (2, 3, 1.0)])
def test_scalogram_pointwise_against_float64(phase, ph, pw, power):
    """cpc_scalogram_pointwise against a float64 restatement of PreprocessingModule.forward: log power, the wrapped phase advance
    (advances built to need the wrap, kept 1e-2 away from +-pi so that float32 rounding cannot flip it), floor-mode pooling with
    bins % ph != 0 and W % pw != 0, power != 1, ldq > 2 bins."""
    B, Tn, bins = 2, 12, 19
    ldq = 2 * bins + 6
    g = torch.Generator().manual_seed(phase * 10 + ph + pw)
    fixed = ((torch.rand(bins, generator=g) * 2 - 1) * math.pi).float()
    scale = (0.5 + torch.rand(bins, generator=g)).float()
    mag = torch.exp(torch.randn(B, Tn, bins, generator=g)).float()
    ang = ((torch.rand(B, Tn, bins, generator=g) * 2 - 1) * math.pi).float()
    for _ in range(50):
        cq = torch.full((B, Tn, ldq), 1e6)
        cq[:, :, :2 * bins].view(B, Tn, bins, 2)[..., 0] = mag * torch.cos(ang)
        cq[:, :, :2 * bins].view(B, Tn, bins, 2)[..., 1] = mag * torch.sin(ang)
        cq = cq.float()
        z = cq.double()[:, :, :2 * bins].reshape(B, Tn, bins, 2)
        a = torch.atan2(z[..., 1], z[..., 0])
        d = a[:, 1:] - a[:, :-1] + fixed.double()
        near = ((d.abs() - math.pi).abs() < 1e-2) | (a.abs()[:, 1:] > math.pi - 1e-3) | (a.abs()[:, :-1] > math.pi - 1e-3)
        if not bool(near.any()):
            break
        bad = torch.zeros(B, Tn, bins, dtype=torch.bool)
        bad[:, 1:] |= near
        ang = torch.where(bad, ang * 0.9 + 0.1, ang)
    assert not bool(near.any())
    assert bool((d > math.pi).any()) and bool((d < -math.pi).any()), "the data is meant to need both wraps"
    offset, log_offset, norm = 1e-3, 0.5, 0.7
    W = Tn - 1 if phase else Tn
    Cc = 2 if phase else 1
    Wp, Hp = W // pw, bins // ph
    out = full(B * Wp * Hp * Cc + 8, torch.float32)
    cqd, fixd, scd = cq.to(DEV), fixed.to(DEV), scale.to(DEV)            # (kept alive until the launch has read them)
    _hip.call("cpc_scalogram_pointwise", _hip.ptr(cqd), _hip.ptr(fixd if phase else None), _hip.ptr(scd if phase else None), _hip.ptr(out), B, Tn, bins, C.c_longlong(ldq), phase, C.c_float(offset),
              C.c_float(log_offset), C.c_float(norm), C.c_float(power), ph, pw)
    ref = _pointwise_ref(cq.double(), fixed.double(), scale.double(), B, Tn, bins, phase, offset, log_offset, norm, power, ph, pw)
    assert ref.shape == (B, Wp, Hp, Cc)
    got = out[:B * Wp * Hp * Cc].view(B, Wp, Hp, Cc)
    assert rel_err(got, ref) < 2e-5
    assert bool((out[B * Wp * Hp * Cc:] == SENTINEL).all())
