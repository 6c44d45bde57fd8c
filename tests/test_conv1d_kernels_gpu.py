"""The 1-D convolution kernels at their edges: encoder layer 1 (csrc/conv1.hip), layers >= 2 and the convolutional context network
through cpc_conv_fwd / cpc_conv_dgrad / cpc_conv_wgrad, the operand re-layout cpc_conv_w_prep, and cpc_reduce_conv_w, cpc_reduce_slabs
and cpc_colsum, each against a plain float64 reference of the same operation (tests/conv1d_reference.py; test_conv1d_reference_host.py
checks those references against F.conv1d / autograd and shows that the metric used here rejects deliberate mistakes).

Conventions.  Device inputs are the reference's inputs rounded to the storage type.  Every output buffer starts as NaN (sign bits:
0xA5 bytes) and is followed by sentinel elements that must be intact afterwards.  Every random-data case (seeded torch.Generator
normal data) has an exact-data twin, integer inputs in {-2 .. 2} and weights in {-1, 0, 1}, thinned so that sum |a||b| <= 256 (asserted on
the host): every partial sum in any order is an integer both formats hold, and the twin must equal the reference exactly.

The bound, per element, no element left out:   |got - ref| <= u_out |ref| + 2 (n + 2) 2^-24 S
S = the same operation on absolute values, n = the number of summed terms (stated at each check), u_out = 2^-8 for bf16 outputs, 0 for
f32 outputs (slabs and reduced gradients are f32 in both storage types).  It is derived (conv1d_reference.py), not measured; no
tolerance in this file comes from a kernel run.  The float32 host emulation alone ("reference alone", from
test_conv1d_reference_host.py, the float32 value against the bound without its u_out term) reaches at most

    layer-1 forward   0.20 (f32 and bf16 inputs)         layer-1 backward  0.18 (f32) / 0.20 (bf16)
    layers >= 2       forward 0.016 / 0.008, data gradient 0.031 / 0.012, weight gradient 0.042 / 0.016   (f32 / bf16)
    cpc_reduce_slabs  0.14                               cpc_colsum        0.059 (f32) / 0.0014 (bf16)
    tile-kernel cases 0.008

of the bound.  (A stored bf16 output can use the whole u_out |ref| term through its one rounding alone; see that module's docstring.)

A  Layer 1.  conv1_fwd_kernel<T, KW, WROW, BITS>: KW = 10 compile-time for kw = 10, the run-time form (KW = 0) for every other kw; WROW (one
wave per row) for C = 512, BITS with y_bits.  Lanes per row C / 8, rows per pass 256 / (C / 8): C = 8 gives 256 row lanes, C = 2048 one
(no cross-lane reduction in the backward).  The case lists (conv1d_reference.c1_fwd_cases / c1_bwd_cases, coverage asserted on the host)
give every C every value of L_valid, pad, relu, bias, ldx slack (forward) and of L_valid, B, nblk_t kind, nblk_b kind (backward).

B  Layers >= 2, B = 3, Lout_valid = 17, Lout_alloc = 17 + D - 1, x_tail and dy_head at their minimum.  What launch_gemm_nt / launch_gemm_tn
take (conv1d_reference.nt_variant / tn_variant restate the launcher's conditions: fast = K % 64 == 0 for bf16, K % 32 == 0 for f32;
tap-innermost = fast, lda < K, K % lda == 0, lda % 64 (32) == 0; every launch here is 128 x 128 tiles, asserted with _hip.nt_tile /
_hip.tn_tile; TN: bf16 fast (I % 8 == 0), f32 generic):

    (Cin,Cout,kw,s)  D   forward f32            forward bf16           data gradient f32      data gradient bf16
    (64,64,7,3)      3   fast storage           fast storage           fast 3 taps            fast 3 taps
    (64,32,5,1)      5   fast 5 taps            fast 5 taps            fast 5 taps            generic
    (32,64,3,2)      2   fast storage           generic                fast 2 taps            fast 2 taps
    (64,64,4,4)      1   fast storage           fast storage           fast storage           fast storage
    (64,64,2,4)      1   fast storage           fast storage           fast storage           fast storage
    (24,40,3,1)      3   generic                generic                generic                generic
    (16,16,40,2)    20   fast 20 taps           fast storage           fast storage           fast storage
    (64,64,33,1)    33   fast 33 taps           fast 33 taps           fast 33 taps           fast 33 taps
    (64,64,8,4)      2   fast 2 taps            fast 2 taps            fast 2 taps            fast 2 taps

nsplit = 5 leaves 1 .. 4 empty chunks (chunks are rounded up to 64 rows bf16 / 32 rows f32) at every shape except (64,64,33,1) in f32
(147 rows in 5 chunks of 32); whichever chunks are empty must be zero slabs.
Tile kernels through the wrappers (bf16): cpc_conv_wgrad (64,256,8,4), B = 4, Lout_alloc = 520, nsplit = 2: I = 512, J = 256, chunk 1088
>= 1024 -> the 256 x 256 TN tile (_hip.tn_tile).  cpc_conv_fwd (32,256,4,2), Lout_alloc = 1280: N = 256, K = 128.  launch_gemm_nt takes
256 x 256 tiles when "fast && bf16 && N >= 256 && M >= 1024 && big_tiles >= 200" (B = 40: exactly 200), the register epilogue ("direct")
when "fast && dma && bf16 && GEMM_WIDE_EPI && bias 16-byte aligned && no mask", and the persistent kernel when in addition
"batch == 1 && m_off == 0 && 2 <= K / 64 <= 16 && blocks > 2 * 256 && M % 32 == 0 && a_rpi == 0 && b_rpi == 0 && N % 256 == 0": B = 104 gives
520 tiles.  Their references are computed on the valid rows among a seeded subset of 4096 rows plus the first and last valid row of
the first and last item and the rows around the 256-row edges of the first and last tile (conv1d_reference.tile_rows); all pad rows
are compared with zero on the device.

C  cpc_conv_w_prep: the single launch shrinks its tile to tco = 4 below 2048 workgroups, the batched one keeps 32 (8 for kw = 40, 33).

D  cpc_reduce_slabs, launch_reduce_slabs' choice per (I, J, nslab):  (1,64,7) (1,64,15) grid-stride; (1,64,16) small<16>; (1,2048,600)
small<256>; (1,2052,600) small<64>; (11,512,127) small<16>; (11,512,130) small<64>; (256,256,24) small<16>; (257,256,24) grid-stride
(total4 > 16384); (10,512,6) grid-stride.  The conv-weight permutation runs where I factors: (256,256,24) as kw = 2, cin = 128 and
(10,512,6) as kw = 2, cin = 5.

E  cpc_colsum: f32 always takes 16-byte loads here (both bases are 16-byte aligned), one pass for N <= 1024, 2 / 3 / 4 passes for N =
2048 / 2056 / 4096.  bf16 takes them with N % 8 == 0, ldx % 8 == 0 and the aligned base (8 columns per thread: one pass up to N = 2048,
two for 2056 and 4096), and the 4-column variant otherwise: always for N = 12, for ldx = N + 4 and for the base offset by 4 elements
(1 / 2 / 3 / 4 passes for N <= 1024 / 2048 / 2056 / 4096).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
import conv1d_reference as R  # noqa: E402
from test_attention_long_gpu import guard_intact, guarded  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
EINVAL = -22
NGUARD = 64


def dev(t, dt):
    """A float64 host tensor that is exact in dt -> contiguous device tensor of dt."""
    return t.to(dt).to(DEV).contiguous()


def host(t):
    return t.detach().double().cpu()


def rc(fn, *args):
    """The raw status of an exported function (the argument checks: _hip.call would raise)."""
    return getattr(_hip.lib(), fn)(*args, _hip.stream_ptr())


def same_bits(a, b):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    return torch.equal(a.contiguous().view(it[a.element_size()]), b.contiguous().view(it[b.element_size()]))


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def guarded_bytes(n):
    """n bytes of 0xA5 followed by NGUARD sentinel bytes 0x5A."""
    buf = torch.full((n + NGUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    buf[n:] = 0x5A
    return buf, buf[:n]


def bytes_intact(buf, n):
    return bool((buf[n:] == 0x5A).all())


def check(got, ref, S, n, dt, what, exact=False):
    """Every element within the bound (exact data: equal to the reference as stored in dt); prints the ratio."""
    if exact:
        g = got if torch.is_tensor(got) and got.dtype == torch.float64 else host(got)
        assert torch.equal(g.reshape(-1), ref.to(dt).double().reshape(-1)), f"{what}: exact data differ at " \
            f"{int((g.reshape(-1) != ref.to(dt).double().reshape(-1)).sum())} of {ref.numel()} elements"
        return 0.0
    r = R.bound_ratio(got, ref, S, n, R.u_out(dt))
    print(f"ratio {what}: {r:.4f}")
    assert r <= 1.0, f"{what}: |got - ref| reaches {r:.3f} of the bound"
    return r


def pack_bits(y):
    """bits[i] bit e = y[8 i + e] > 0 (include/cpc_hip.h at cpc_sign_bits)."""
    b = (y.reshape(-1, 8) > 0).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32, device=y.device)).sum(1).to(torch.uint8)


# ======================================================================================================================= A  layer 1
def _c1_fwd(case, dt, exact, bits=False, rows=None, B=3):
    C, kw, s, Lv, pad, relu, hb, slack = case
    La = Lv + pad
    x, x_dev, w, bias, ldx = R.c1_fwd_data(case, dt, exact, B)
    dX, dW = x_dev.float().to(DEV).contiguous(), w.float().to(DEV).contiguous()
    dB = bias.float().to(DEV) if bias is not None else None
    yb, y = guarded(B * La * C, dt)
    bb, bt = guarded_bytes(B * La * C // 8) if bits else (None, None)
    code = _hip.dtype_code(dt)
    if rows is None:
        _hip.call("cpc_conv1_fwd", _hip.ptr(dX), _hip.ptr(dW), _hip.ptr(dB), _hip.ptr(y), B, C, s, kw, ldx, Lv, La, relu, code, _hip.ptr(bt))
    else:
        _hip.call("cpc_conv1_fwd_rows", _hip.ptr(dX), _hip.ptr(dW), _hip.ptr(dB), _hip.ptr(y), B, C, s, kw, ldx, Lv, La, relu, code,
                  _hip.ptr(bt), rows[0], rows[1])
    torch.cuda.synchronize()
    assert guard_intact(yb, B * La * C) and (bb is None or bytes_intact(bb, B * La * C // 8))
    ref = R.conv1_fwd(x, w, bias, s, Lv, La, relu)
    S = R.abs_bound_terms(R.conv1_fwd, x, w, bias, stride=s, L_valid=Lv, L_alloc=La, relu=0)
    return y.view(B, La, C), (bt.view(B, La, C // 8) if bits else None), ref, S


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.c1_fwd_cases(), ids=R.c1_fwd_id)
def test_conv1_fwd(case, dt):
    """cpc_conv1_fwd against float64 at every lane layout (C = 8 .. 2048), with the compile-time kw = 10 and the run-time kw kernels,
    L_valid around the 256-position workgroup, workgroups of pad rows only, relu 0 / 1, bias / NULL, ldx exact or with NaN slack;
    pad rows exactly zero (their bound is zero); the exact-data twin bitwise."""
    C, kw, s, Lv, pad, relu, hb, slack = case
    for exact in (False, True):
        y, _, ref, S = _c1_fwd(case, dt, exact)
        assert bool((y[:, Lv:] == 0).all()), "pad rows"
        check(y, ref, S, kw + 1, dt, f"A fwd {R.c1_fwd_id(case)} {R.name(dt)}", exact)


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kw,s,Lv,pad", [(10, 5, 257, 3), (16, 8, 600, 300), (1, 1, 255, 0), (7, 8, 256, 3)])
def test_conv1_fwd_sign_bits(kw, s, Lv, pad, relu, dt):
    """C = 512 with y_bits: the bits are (y_device > 0) packed, pad-row bytes 0, y bitwise equal to the launch without bits and within
    the bound; relu 0 and 1."""
    case = (512, kw, s, Lv, pad, relu, 1, 0)
    for exact in (False, True):
        y, bits, ref, S = _c1_fwd(case, dt, exact, bits=True)
        y0, _, _, _ = _c1_fwd(case, dt, exact)
        assert same_bits(y, y0), "y with and without y_bits"
        assert torch.equal(bits.reshape(-1), pack_bits(y.float()))
        assert bool((bits[:, Lv:] == 0).all())
        check(y, ref, S, kw + 1, dt, f"A bits k{kw}-s{s}-L{Lv}+{pad}-relu{relu} {R.name(dt)}", exact)


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
def test_conv1_fwd_rows(dt):
    """cpc_conv1_fwd_rows on rows [100, 700) of 600 + 300: starts mid-workgroup, ends inside the pad rows; rows and bit bytes outside
    keep their sentinel values; random data and the exact-data twin."""
    case, lo, hi = (512, 10, 5, 600, 300, 1, 1, 0), 100, 700
    for bits in (False, True):
        for exact in (False, True):
            y, b, ref, S = _c1_fwd(case, dt, exact, bits=bits, rows=(lo, hi))
            assert all_nan(y[:, :lo]) and all_nan(y[:, hi:])
            check(y[:, lo:hi], ref[:, lo:hi], S[:, lo:hi], 11, dt, f"A rows bits{int(bits)} {R.name(dt)}", exact)
            assert bool((y[:, 600:hi] == 0).all())
            if bits:
                assert bool((b[:, :lo] == 0xA5).all()) and bool((b[:, hi:] == 0xA5).all()) and bool((b[:, 600:hi] == 0).all())
                assert torch.equal(b[:, lo:hi].reshape(-1), pack_bits(y[:, lo:hi].float()))


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.c1_bwd_cases(), ids=R.c1_bwd_id)
def test_conv1_bwd(case, dt):
    """cpc_conv1_bwd: every slab finite, slabs of blocks that own no position exactly zero, the float64 sum of the slabs within the
    bound (n = B L_valid + slabs), and the same slabs through cpc_reduce_slabs in the engine's two forms giving [C][1][kw] / [C]."""
    C, kw, s, B, Lv, nt, nb = case
    code = _hip.dtype_code(dt)
    tpb = -(-(-(-Lv // nt)) // 64) * 64
    nslab, per = nt * nb, (kw + 1) * C
    for exact in (False, True):
        x, dy, ldx, La = R.c1_bwd_data(case, dt, exact)
        dX, dY = x.float().to(DEV).contiguous(), dev(dy, dt)
        sb, slabs = guarded(nslab * per, torch.float32)
        _hip.call("cpc_conv1_bwd", _hip.ptr(dX), _hip.ptr(dY), _hip.ptr(slabs), B, C, s, kw, ldx, Lv, La, nt, nb, code)
        wb, dw = guarded(C * kw, torch.float32)
        bb, db = guarded(C, torch.float32)
        _hip.call("cpc_reduce_slabs", _hip.ptr(slabs), _hip.ptr(dw), kw, C, nslab, per, 1, kw, 1, 0)
        _hip.call("cpc_reduce_slabs", _hip.ptr(slabs, kw * C), _hip.ptr(db), 1, C, nslab, per, 1, 1, 0, 0)
        torch.cuda.synchronize()
        assert guard_intact(sb, nslab * per) and guard_intact(wb, C * kw) and guard_intact(bb, C)
        sl = host(slabs).view(nb, nt, kw + 1, C)
        assert bool(torch.isfinite(sl).all())
        for bx in range(nt):
            if bx * tpb >= Lv:
                assert bool((sl[:, bx] == 0).all()), f"time block {bx} owns no position"
        ref = R.conv1_bwd(x, dy, s, kw, Lv)
        S = R.abs_bound_terms(R.conv1_bwd, x, dy, stride=s, kw=kw, L_valid=Lv)
        n, cid = B * Lv + nslab, f"{R.c1_bwd_id(case)} {R.name(dt)}"
        check(sl.sum((0, 1)), ref, S, n, torch.float32, "A bwd slabs " + cid, exact)
        check(host(dw).view(C, kw), ref[:kw].T, S[:kw].T, n, torch.float32, "A bwd dw " + cid, exact)
        check(host(db), ref[kw], S[kw], n, torch.float32, "A bwd db " + cid, exact)


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
def test_conv1_argument_checks(dt):
    B, C, kw, s, Lv, La = 3, 512, 10, 5, 20, 24
    ldx, code = (Lv - 1) * s + kw, _hip.dtype_code(dt)
    x, w, bias = torch.zeros(B * ldx + 64, device=DEV), torch.zeros(4096 * 17, device=DEV), torch.zeros(4096, device=DEV)
    dy = torch.zeros(B * La * 4096, device=DEV, dtype=dt)
    yb, y = guarded(B * La * 4096, dt)
    sb, slabs = guarded(8 * 18 * 4096, torch.float32)
    bb, bits = guarded_bytes(B * La * 4096 // 8)
    P = _hip.ptr

    def fwd(C=C, kw=kw, s=s, ldx=ldx, Lv=Lv, La=La, bits_=None):
        return rc("cpc_conv1_fwd", P(x), P(w), P(bias), P(y), B, C, s, kw, ldx, Lv, La, 1, code, P(bits_))

    def rows(lo, hi):
        return rc("cpc_conv1_fwd_rows", P(x), P(w), P(bias), P(y), B, C, s, kw, ldx, Lv, La, 1, code, None, lo, hi)

    def bwd(C=C, kw=kw, s=s, ldx=ldx, Lv=Lv, La=La, nt=2, nb=2):
        return rc("cpc_conv1_bwd", P(x), P(dy), P(slabs), B, C, s, kw, ldx, Lv, La, nt, nb, code)

    bad = [fwd(ldx=ldx - 1), bwd(ldx=ldx - 1), fwd(La=Lv - 1), bwd(La=Lv - 1), bwd(nb=B + 1), fwd(C=256, bits_=bits), rows(5, 5), rows(9, 4),
           rows(0, La + 1), rows(-1, 4)]
    for c_ in (4, 24, 4096):
        bad += [fwd(C=c_), bwd(C=c_)]
    for k_ in (0, 17):
        bad += [fwd(kw=k_, ldx=ldx + 64), bwd(kw=k_, ldx=ldx + 64)]
    for s_ in (0, 9):
        bad += [fwd(s=s_, ldx=ldx + 64 if s_ else ldx), bwd(s=s_, ldx=ldx + 64 if s_ else ldx)]
    torch.cuda.synchronize()
    assert all(r == EINVAL for r in bad), bad
    assert all_nan(y) and all_nan(slabs) and bool((bits == 0xA5).all())
    assert guard_intact(yb, y.numel()) and guard_intact(sb, slabs.numel()) and bytes_intact(bb, bits.numel())
    assert fwd() == 0 and bwd() == 0 and fwd(bits_=bits) == 0                  # (the same calls with valid arguments are accepted)
    torch.cuda.synchronize()


# ======================================================================================================================= B  layers >= 2
def _prep(w, shape, dt):
    """The two operand layouts through cpc_conv_w_prep (section C checks them bitwise against their definition)."""
    Cin, Cout, kw, s = shape
    D = -(-kw // s)
    fb, wf = guarded(Cout * kw * Cin, dt)
    db, wd = guarded(s * Cin * D * Cout, dt)
    dW = w.float().to(DEV).contiguous()
    _hip.call("cpc_conv_w_prep", _hip.ptr(dW), _hip.ptr(wf), _hip.ptr(wd), Cout, Cin, kw, s, _hip.dtype_code(dt))
    torch.cuda.synchronize()
    assert guard_intact(fb, wf.numel()) and guard_intact(db, wd.numel())
    return wf, wd


def _with_tail(x, n_tail, value, dt):
    """[x | n_tail elements of value], exactly that many elements."""
    buf = torch.full((x.numel() + n_tail,), value, dtype=dt, device=DEV)
    buf[:x.numel()] = dev(x, dt).reshape(-1)
    return buf


def _with_head(dy, n_head, dt):
    buf = torch.zeros(n_head + dy.numel(), dtype=dt, device=DEV)
    buf[n_head:] = dev(dy, dt).reshape(-1)
    return buf


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=R.conv_id)
def test_conv_fwd_dgrad_wgrad(shape, dt):
    """cpc_conv_fwd / cpc_conv_dgrad / cpc_conv_wgrad (+ cpc_reduce_conv_w) in the tightest layout the guard contract allows: exactly
    D - 1 pad rows, x_tail and dy_head at their minimum, the tail holding zeros and then 1e4 (forward outputs and weight-gradient
    slabs bitwise equal), Lin_valid with and without uncovered valid positions, random data against the bound and exact data bitwise."""
    Cin, Cout, kw, s = shape
    code, B = _hip.dtype_code(dt), R.CONV_B
    for exact in (False, True):
        for slack in (False, True):
            geo, x, w, bias, dy = R.conv_data(shape, dt, exact, slack)
            D, Lo, La, Li, Lv = geo["D"], geo["Lout_valid"], geo["Lout_alloc"], geo["Lin_alloc"], geo["Lin_valid"]
            M, K, Kd = B * La, kw * Cin, D * Cout
            cid = f"{R.conv_id(shape)} {R.name(dt)} slack{int(slack)}"
            assert _hip.nt_tile(code, M, Cout, K) == 128 and _hip.nt_tile(code, M, s * Cin, Kd) == 128
            wf, wd = _prep(w, shape, dt)
            dB = bias.float().to(DEV)
            xs = [_with_tail(x, geo["x_tail"], v, dt) for v in (0.0, 1e4)]
            dyb = _with_head(dy, geo["dy_head"], dt)
            p_dy = _hip.ptr(dyb, geo["dy_head"])
            # ---- forward
            for relu in (0, 1):
                for b_host, b_dev in ((bias, dB), (None, None)):
                    ys = []
                    for xb in xs:
                        yb, y = guarded(M * Cout, dt)
                        _hip.call("cpc_conv_fwd", _hip.ptr(xb), _hip.ptr(wf), _hip.ptr(b_dev), _hip.ptr(y), B, Cin, Cout, kw, s, La, Lo, relu,
                                  geo["x_tail"], code)
                        torch.cuda.synchronize()
                        assert guard_intact(yb, M * Cout)
                        ys.append(y)
                    assert same_bits(ys[0], ys[1]), "forward depends on the values in x_tail"
                    y = ys[0].view(B, La, Cout)
                    assert bool((y[:, Lo:] == 0).all()), "pad rows"
                    ref = R.conv_fwd(x, w, b_host, s, Lo, La, relu)
                    S = R.abs_bound_terms(R.conv_fwd, x, w, b_host, stride=s, Lout_valid=Lo, Lout_alloc=La, relu=0)
                    check(y, ref, S, K + 1, dt, f"B fwd {cid} relu{relu} bias{int(b_host is not None)}", exact)
            # ---- data gradient
            cov = R.covered_positions(shape, geo)
            for mask in (True, False):
                db_, dx = guarded(B * Li * Cin, dt)
                _hip.call("cpc_conv_dgrad", p_dy, _hip.ptr(wd), _hip.ptr(xs[0]) if mask else None, _hip.ptr(dx), B, Cin, Cout, kw, s, La, Lv,
                          geo["dy_head"], code, None, None)
                torch.cuda.synchronize()
                assert guard_intact(db_, B * Li * Cin)
                dx = dx.view(B, Li, Cin)
                assert bool((dx[:, Lv:] == 0).all()) and bool((dx[:, ~cov.to(DEV)] == 0).all()), "positions no window covers"
                xa = x if mask else None
                check(dx, R.conv_dgrad(dy, w, s, Li, xa), R.conv_dgrad(dy.abs(), w.abs(), s, Li, xa), Kd, dt, f"B dgrad {cid} mask{int(mask)}", exact)
            # ---- weight gradient
            ref_dw, S_dw = R.conv_wgrad(x, dy, s, kw), R.conv_wgrad(x.abs(), dy.abs(), s, kw)
            blk = 64 if dt == torch.bfloat16 else 32
            for nsplit in (1, 2, 5):
                chunk = -(-(-(-M // nsplit)) // blk) * blk
                assert _hip.tn_tile(code, M, K, Cout, nsplit, chunk) == 128
                per, sl = K * Cout, []
                for xb in xs:
                    sb, slabs = guarded(nsplit * per, torch.float32)
                    _hip.call("cpc_conv_wgrad", _hip.ptr(xb), _hip.ptr(dyb, geo["dy_head"]), _hip.ptr(slabs), B, Cin, Cout, kw, s, La, nsplit,
                              geo["x_tail"], code)
                    torch.cuda.synchronize()
                    assert guard_intact(sb, nsplit * per)
                    sl.append(slabs)
                assert same_bits(sl[0], sl[1]), "weight-gradient slabs depend on the values in x_tail"
                hs = host(sl[0]).view(nsplit, K, Cout)
                assert bool(torch.isfinite(hs).all())
                for z in range(nsplit):
                    if z * chunk >= M:
                        assert bool((hs[z] == 0).all()), f"empty chunk {z} of {nsplit}"
                n = M + nsplit
                check(hs.sum(0), R.slab_layout(ref_dw), R.slab_layout(S_dw), n, torch.float32, f"B wgrad slabs {cid} nsplit{nsplit}", exact)
                ob, out = guarded(Cout * Cin * kw, torch.float32)
                _hip.call("cpc_reduce_conv_w", _hip.ptr(sl[0]), _hip.ptr(out), Cin, Cout, kw, nsplit, per)
                torch.cuda.synchronize()
                assert guard_intact(ob, out.numel())
                check(out.view(Cout, Cin, kw), ref_dw, S_dw, n, torch.float32, f"B wgrad reduced {cid} nsplit{nsplit}", exact)


@pytest.mark.parametrize("cin,cout,kw", [(32, 64, 3), (64, 64, 8), (24, 40, 3), (16, 16, 40)])
def test_reduce_conv_w_integer_slabs(cin, cout, kw):
    """cpc_reduce_conv_w on integer slabs, bitwise against the exact sum: every remainder of the four-way unrolled slab loop, slabs
    packed and 8 floats apart; the LDS-tiled kernel (cin, cout multiples of 32, kw <= 8) and both reasons for the fall-back through
    cpc_reduce_slabs (cin = 24; kw = 40)."""
    per = kw * cin * cout
    for nslab in (1, 2, 3, 4, 5, 9):
        for stride in (per, per + 8):
            g = R.gen(nslab * 100 + kw)
            sl = R.ints(g, -3, 3, nslab, kw * cin, cout)
            buf = torch.full((nslab * stride,), float("nan"), device=DEV)
            buf.view(nslab, stride)[:, :per] = sl.float().to(DEV).view(nslab, per)
            ob, out = guarded(per, torch.float32)
            _hip.call("cpc_reduce_conv_w", _hip.ptr(buf), _hip.ptr(out), cin, cout, kw, nslab, stride)
            torch.cuda.synchronize()
            assert guard_intact(ob, per)
            ref = sl.sum(0).view(kw, cin, cout).permute(2, 1, 0)
            assert torch.equal(host(out).view(cout, cin, kw), ref), (nslab, stride)


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
def test_conv_argument_checks(dt):
    """x_tail / dy_head one element below the minimum, nsplit = 0 and Lout_valid > Lout_alloc return -22 and write nothing."""
    code, B = _hip.dtype_code(dt), R.CONV_B
    for shape in [(64, 64, 7, 3), (64, 32, 5, 1), (16, 16, 40, 2)]:
        Cin, Cout, kw, s = shape
        geo, x, w, bias, dy = R.conv_data(shape, dt, False, False)
        La, Lo, Li = geo["Lout_alloc"], geo["Lout_valid"], geo["Lin_alloc"]
        wf, wd = _prep(w, shape, dt)
        xb, dyb = _with_tail(x, geo["x_tail"], 0.0, dt), _with_head(dy, geo["dy_head"], dt)
        p_dy = _hip.ptr(dyb, geo["dy_head"])
        yb, y = guarded(B * La * Cout, dt)
        gb, dx = guarded(B * Li * Cin, dt)
        sb, slabs = guarded(2 * kw * Cin * Cout, torch.float32)
        P = _hip.ptr
        bad = [rc("cpc_conv_fwd", P(xb), P(wf), None, P(y), B, Cin, Cout, kw, s, La, Lo, 1, geo["x_tail"] - 1, code),
               rc("cpc_conv_wgrad", P(xb), p_dy, P(slabs), B, Cin, Cout, kw, s, La, 2, geo["x_tail"] - 1, code),
               rc("cpc_conv_dgrad", p_dy, P(wd), P(xb), P(dx), B, Cin, Cout, kw, s, La, geo["Lin_valid"], geo["dy_head"] - 1, code, None, None),
               rc("cpc_conv_wgrad", P(xb), p_dy, P(slabs), B, Cin, Cout, kw, s, La, 0, geo["x_tail"], code),
               rc("cpc_conv_fwd", P(xb), P(wf), None, P(y), B, Cin, Cout, kw, s, La, La + 1, 1, geo["x_tail"], code)]
        torch.cuda.synchronize()
        assert all(r == EINVAL for r in bad), (shape, bad)
        assert all_nan(y) and all_nan(dx) and all_nan(slabs)
        assert guard_intact(yb, y.numel()) and guard_intact(gb, dx.numel()) and guard_intact(sb, slabs.numel())


@pytest.mark.parametrize("B,kernel", [(40, "256-tile, register epilogue"), (104, "persistent")])
def test_conv_fwd_tile_kernels(B, kernel):
    """cpc_conv_fwd, bf16, (Cin, Cout, kw, stride) = (32, 256, 4, 2), Lout_alloc = 1280: M = 1280 B, N = 256, K = 128 (two taps, tap-innermost).
    B = 40: 200 tiles of 256 x 256 -> the 256-tile kernel with the register epilogue; B = 104: 520 tiles > 2 x 256 -> the persistent
    kernel (conditions quoted in the module docstring).  Random data against the bound and the exact-data twin bitwise, both on the
    valid rows of conv1d_reference.tile_rows (4096 seeded rows plus the edge rows); all pad rows are compared with zero on the device."""
    dt, (Cin, Cout, kw, s), La = torch.bfloat16, R.TILE_FWD_SHAPE, R.TILE_FWD_LA
    Lo, M, K = La - 1, B * La, kw * Cin
    code = _hip.dtype_code(dt)
    tiles = -(-M // 256) * (Cout // 256)
    assert _hip.nt_tile(code, M, Cout, K) == 256 and (tiles > 512) == (kernel == "persistent") and tiles >= 200
    assert K % 64 == 0 and 2 <= K // 64 <= 16 and M % 32 == 0 and Cout % 256 == 0 and (s * Cin) % 64 == 0 and K % (s * Cin) == 0
    rows = R.tile_rows(M, La, Lo, 4096, B)
    assert rows.numel() >= 4000 and all(r in rows for r in (0, Lo - 1, M - La, M - La + Lo - 1, 255, 256))
    for exact in (False, True):
        x, w, bias = R.tile_fwd_data(B, exact)
        wf, _ = _prep(w, (Cin, Cout, kw, s), dt)
        xb, dB = _with_tail(x, (kw - s) * Cin, 1e4, dt), bias.float().to(DEV)
        yb, y = guarded(M * Cout, dt)
        _hip.call("cpc_conv_fwd", _hip.ptr(xb), _hip.ptr(wf), _hip.ptr(dB), _hip.ptr(y), B, Cin, Cout, kw, s, La, Lo, 1, (kw - s) * Cin, code)
        torch.cuda.synchronize()
        assert guard_intact(yb, M * Cout)
        y = y.view(B, La, Cout)
        assert bool((y[:, Lo:] == 0).all()) and not bool(torch.isnan(y.float()).any())
        win = R.gathered_windows(x, rows, La, s, kw)
        ref = R.conv_fwd(win, w, bias, s, 1, 1, 1)[:, 0]
        S = R.abs_bound_terms(R.conv_fwd, win, w, bias, stride=s, Lout_valid=1, Lout_alloc=1, relu=0)[:, 0]
        check(y.view(M, Cout)[rows.to(DEV)], ref, S, K + 1, dt, f"B tile fwd B{B} ({kernel})", exact)


def test_conv_wgrad_tile_kernel():
    """cpc_conv_wgrad, bf16, (64, 256, 8, 4), B = 4, Lout_alloc = 520, nsplit = 2: I = 512, J = 256, chunks of 1088 rows -> the 256 x 256
    TN tile; the whole gradient against float64 (random data) and bitwise (exact data), then through cpc_reduce_conv_w."""
    dt, (Cin, Cout, kw, s) = torch.bfloat16, R.TILE_WGRAD_SHAPE
    B, La, nsplit = R.TILE_WGRAD_B, R.TILE_WGRAD_LA, R.TILE_WGRAD_NSPLIT
    M, K = B * La, kw * Cin
    code = _hip.dtype_code(dt)
    chunk = -(-(-(-M // nsplit)) // 64) * 64
    assert _hip.tn_tile(code, M, K, Cout, nsplit, chunk) == 256
    for exact in (False, True):
        x, dy = R.tile_wgrad_data(exact)
        xs = [_with_tail(x, (kw - s) * Cin, v, dt) for v in (0.0, 1e4)]
        dY, per, sl = dev(dy, dt), K * Cout, []
        for xb in xs:
            sb, slabs = guarded(nsplit * per, torch.float32)
            _hip.call("cpc_conv_wgrad", _hip.ptr(xb), _hip.ptr(dY), _hip.ptr(slabs), B, Cin, Cout, kw, s, La, nsplit, (kw - s) * Cin, code)
            torch.cuda.synchronize()
            assert guard_intact(sb, nsplit * per)
            sl.append(slabs)
        assert same_bits(sl[0], sl[1])
        ref, S = R.conv_wgrad(x, dy, s, kw), R.conv_wgrad(x.abs(), dy.abs(), s, kw)
        check(host(sl[0]).view(nsplit, K, Cout).sum(0), R.slab_layout(ref), R.slab_layout(S), M + nsplit, torch.float32, "B tile wgrad slabs", exact)
        ob, out = guarded(per, torch.float32)
        _hip.call("cpc_reduce_conv_w", _hip.ptr(sl[0]), _hip.ptr(out), Cin, Cout, kw, nsplit, per)
        torch.cuda.synchronize()
        assert guard_intact(ob, per)
        check(out.view(Cout, Cin, kw), ref, S, M + nsplit, torch.float32, "B tile wgrad reduced", exact)


# ======================================================================================================================= C  cpc_conv_w_prep
@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
@pytest.mark.parametrize("shape", R.PREP_SHAPES, ids=R.conv_id)
def test_conv_w_prep(shape, dt):
    """w_fwd and w_dgrad bitwise equal to the storage-type rounding of their definition, zero taps included; with either output NULL the
    other is still written and nothing else is touched."""
    Cin, Cout, kw, s = shape
    D, code = -(-kw // s), _hip.dtype_code(dt)
    w = R.normal(R.gen(Cin + Cout + kw + s), Cout, Cin, kw).float()
    dW = w.to(DEV)
    ref_f, ref_d = R.w_fwd_layout(w).to(dt).reshape(-1), R.w_dgrad_layout(w, s).to(dt).reshape(-1)
    assert D * s == kw or int((ref_d == 0).sum()) >= (D * s - kw) * Cin * Cout
    for want_f, want_d in ((True, True), (True, False), (False, True)):
        fb, wf = guarded(ref_f.numel(), dt)
        db, wd = guarded(ref_d.numel(), dt)
        _hip.call("cpc_conv_w_prep", _hip.ptr(dW), _hip.ptr(wf) if want_f else None, _hip.ptr(wd) if want_d else None, Cout, Cin, kw, s, code)
        torch.cuda.synchronize()
        assert guard_intact(fb, wf.numel()) and guard_intact(db, wd.numel())
        assert same_bits(wf.cpu(), ref_f) if want_f else all_nan(wf)
        assert same_bits(wd.cpu(), ref_d) if want_d else all_nan(wd)
    assert rc("cpc_conv_w_prep", _hip.ptr(dW), None, None, Cout, Cin, kw, s, code) == EINVAL


@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
def test_conv_w_prep_batch_mixed(dt):
    """_hip.ConvPrepBatch bitwise equal to single launches for a list that mixes kw = 40 (tile narrowed for LDS) with kw = 3 and a job
    without w_dgrad."""
    code = _hip.dtype_code(dt)
    shapes = [(16, 16, 40, 2), (24, 40, 3, 1), (64, 64, 33, 1), (32, 64, 3, 2), (96, 40, 8, 4)]
    no_dgrad = 3
    jobs, singles, keep = [], [], []
    for k, (Cin, Cout, kw, s) in enumerate(shapes):
        D = -(-kw // s)
        dW = R.normal(R.gen(k), Cout, Cin, kw).float().to(DEV)
        f1, f2 = guarded(Cout * kw * Cin, dt), guarded(Cout * kw * Cin, dt)
        d1, d2 = guarded(s * Cin * D * Cout, dt), guarded(s * Cin * D * Cout, dt)
        nd = k == no_dgrad
        _hip.call("cpc_conv_w_prep", _hip.ptr(dW), _hip.ptr(f1[1]), None if nd else _hip.ptr(d1[1]), Cout, Cin, kw, s, code)
        jobs.append((dW, f2[1], torch.empty(0, device=DEV, dtype=dt) if nd else d2[1], Cout, Cin, kw, s))
        singles.append((f1, d1, f2, d2, nd))
    assert jobs[no_dgrad][2].data_ptr() == 0
    _hip.ConvPrepBatch(jobs, DEV).run(code)
    torch.cuda.synchronize()
    for f1, d1, f2, d2, nd in singles:
        for buf, v in (f1, d1, f2, d2):
            assert guard_intact(buf, v.numel())
        assert same_bits(f1[1], f2[1]) and not all_nan(f2[1])
        assert (all_nan(d1[1]) and all_nan(d2[1])) if nd else same_bits(d1[1], d2[1])


# ======================================================================================================================= D  cpc_reduce_slabs
@pytest.mark.parametrize("I,J,nslab", R.REDUCE_CASES, ids=lambda v: str(v))
def test_reduce_slabs_forms(I, J, nslab):
    """Every kernel of launch_reduce_slabs (both sides of each threshold) in the four output forms the engines use, slabs packed and 8
    floats apart: integer slabs bitwise, normal slabs within the bound (n = nslab); elements the form does not address stay NaN."""
    g = R.gen(I * 7 + J + nslab)
    data = {"int": R.ints(g, -2, 2, nslab, I, J), "normal": R.normal(g, nslab, I, J).float().double()}
    for kind, sl in data.items():
        total, S = sl.sum(0), sl.abs().sum(0)
        for stride in (I * J, I * J + 8):
            buf = torch.full((nslab * stride,), float("nan"), device=DEV)
            buf.view(nslab, stride)[:, :I * J] = sl.float().to(DEV).view(nslab, I * J)
            for fname, cdiv, s_j, s_hi, s_lo, n_out, off in R.reduce_forms(I, J):
                ob, out = guarded(off + n_out, torch.float32)
                _hip.call("cpc_reduce_slabs", _hip.ptr(buf), _hip.ptr(out, off), I, J, nslab, stride, cdiv, s_j, s_hi, s_lo)
                torch.cuda.synchronize()
                assert guard_intact(ob, off + n_out)
                got = host(out)
                idx = R.reduce_index(I, J, cdiv, s_j, s_hi, s_lo) + off
                untouched = torch.ones(off + n_out, dtype=torch.bool)
                untouched[idx] = False
                assert all_nan(got[untouched]), f"{fname}: an element the form does not address was written"
                check(got[idx], total.reshape(-1), S.reshape(-1), nslab, torch.float32,
                      f"D reduce I{I}-J{J}-z{nslab}-{fname}-stride+{stride - I * J} {kind} [{R.reduce_kernel(I, J, nslab)}]", kind == "int")


def test_reduce_slabs_argument_checks():
    slabs = torch.zeros(4 * 64, device=DEV)
    ob, out = guarded(64, torch.float32)
    P = _hip.ptr
    bad = [rc("cpc_reduce_slabs", P(slabs), P(out), 1, 62, 4, 64, 1, 1, 62, 0), rc("cpc_reduce_slabs", P(slabs), P(out), 1, 64, 0, 64, 1, 1, 64, 0),
           rc("cpc_reduce_slabs", P(slabs), P(out), 1, 64, 4, 64, 0, 1, 64, 0), rc("cpc_reduce_slabs", None, P(out), 1, 64, 4, 64, 1, 1, 64, 0),
           rc("cpc_reduce_slabs", P(slabs), None, 1, 64, 4, 64, 1, 1, 64, 0), rc("cpc_reduce_conv_w", None, P(out), 4, 4, 4, 1, 64),
           rc("cpc_reduce_conv_w", P(slabs), P(out), 4, 4, 4, 0, 64)]
    torch.cuda.synchronize()
    assert all(r == EINVAL for r in bad), bad
    assert all_nan(out) and guard_intact(ob, 64)


# ======================================================================================================================= E  cpc_colsum
@pytest.mark.parametrize("dt", DTYPES, ids=R.name)
@pytest.mark.parametrize("M,N", R.COLSUM_SHAPES, ids=lambda v: str(v))
def test_colsum(M, N, dt):
    """cpc_colsum in its vector and non-vector variants, one and several column passes, row pitches N, N + 4, N + 8, an aligned base
    and one offset by 4 elements, 1, 7 and M + 3 blocks: the float64 sum of the slabs within the bound (n = M), slabs of blocks
    beyond M exactly zero, integer data bitwise; the pitch's slack columns hold NaN."""
    code = _hip.dtype_code(dt)
    g = R.gen(M * 3 + N)
    data = {"int": R.ints(g, -2, 2, M, N), "normal": R.rounded(R.normal(g, M, N), dt)}
    seen = set()
    for kind, X in data.items():
        ref, S = X.sum(0), X.abs().sum(0)
        for ldx in (N, N + 4, N + 8):
            for off in (0, 4):
                buf = torch.full((off + M * ldx,), float("nan"), device=DEV, dtype=dt)
                buf[off:].view(M, ldx)[:, :N] = dev(X, dt)
                seen.add(R.colsum_variant(dt, N, ldx, off))
                for nblocks in (1, 7, M + 3):
                    sb, slabs = guarded(nblocks * N, torch.float32)
                    _hip.call("cpc_colsum", _hip.ptr(buf, off), _hip.ptr(slabs), M, N, ldx, nblocks, code)
                    torch.cuda.synchronize()
                    assert guard_intact(sb, nblocks * N)
                    hs = host(slabs).view(nblocks, N)
                    assert bool(torch.isfinite(hs).all())
                    rpb = -(-M // nblocks)
                    for b in range(nblocks):
                        if b * rpb >= M:
                            assert bool((hs[b] == 0).all()), f"block {b} owns no row"
                    check(hs.sum(0), ref, S, M, torch.float32, f"E colsum {M}x{N} {R.name(dt)} ldx+{ldx - N} off{off} blocks{nblocks} {kind}", kind == "int")
    assert (False in {v for v, _ in seen}) or dt == torch.float32          # bf16 reaches the non-vector variant at every shape (offset base)
    assert {p for _, p in seen} >= {-(-(N // 4) // 256)}


def test_colsum_argument_checks():
    X = torch.zeros(16 * 16, device=DEV)
    sb, slabs = guarded(64, torch.float32)
    P = _hip.ptr
    bad = [rc("cpc_colsum", P(X), P(slabs), 8, 6, 8, 2, _hip.F32), rc("cpc_colsum", P(X), P(slabs), 8, 8, 10, 2, _hip.F32),
           rc("cpc_colsum", P(X), P(slabs), 8, 8, 8, 0, _hip.F32), rc("cpc_colsum", None, P(slabs), 8, 8, 8, 2, _hip.F32),
           rc("cpc_colsum", P(X), None, 8, 8, 8, 2, _hip.F32)]
    torch.cuda.synchronize()
    assert all(r == EINVAL for r in bad), bad
    assert all_nan(slabs) and guard_intact(sb, 64)
