"""Plain references of the 1-D convolution kernels (csrc/conv1.hip, the cpc_conv_* wrappers over the GEMMs, cpc_conv_w_prep,
cpc_reduce_conv_w, cpc_reduce_slabs, cpc_colsum), the per-element error bound they are judged by, the case lists and the data recipes.
Shared by test_conv1d_kernels_gpu.py (the kernels against these references) and test_conv1d_reference_host.py (these references
against F.conv1d / autograd, a float32 emulation against the bound, and the metric against deliberate mistakes).  Nothing here
touches a device.

Every function works in the dtype of its inputs: float64 inputs give the reference, float32 inputs the host emulation of f32
accumulation.  Layouts are the device's: channels-last activations [B][L_alloc][C] with zero pad rows, weights in the reference
model's [Cout][Cin][kw].

The bound, per element:   |got - ref| <= u_out |ref| + 2 (n + 2) 2^-24 S
  S      the same operation run on absolute values (sum_k |a_k| |b_k| + |bias|), n the number of summed terms;
  u_out  2^-8 for an output stored as bf16, 0 for an f32 output.
n 2^-24 S bounds f32 accumulation of n exact or once-rounded products in any order; the factor 2 is the margin for the matrix
pipe's internal accumulation.  ReLU and a 0/1 mask are 1-Lipschitz, so the bound holds behind them.  Where S = 0 the bound is 0 and
the output has to be exact.
"""
import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U24 = 2.0 ** -24
U8 = 2.0 ** -8
C1_KA = 16          # accumulator rows of the run-time-kw instantiation of conv1_bwd_kernel (C1_MAXK)


def name(dt):
    return "f32" if dt == F32 else "bf16"


def rounded(t, dt):
    """The value the device sees after storage in dt (so that references use identical inputs)."""
    return t.to(dt).double()


def u_out(dt):
    return U8 if dt == BF16 else 0.0


def bound(ref, S, n, u):
    return u * ref.abs() + 2.0 * (n + 2) * U24 * S


def bound_ratio(got, ref, S, n, u):
    """max over ALL elements of |got - ref| / bound; an element whose bound is 0 counts 0 when exact and inf otherwise; a
    non-finite output counts inf."""
    got, ref, S = (torch.as_tensor(t).detach().double().cpu().reshape(-1) for t in (got, ref, S))
    assert got.numel() == ref.numel() == S.numel(), (got.numel(), ref.numel(), S.numel())
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err, b = (got - ref).abs(), bound(ref, S, n, u)
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------ layer 1
def conv1_fwd(x, w, bias, stride, L_valid, L_alloc, relu):
    """x [B][ldx], w [C][kw], bias [C] or None -> y [B][L_alloc][C], pad rows zero.  y[b][t][c] = act(bias[c] + sum_j x[b][t s + j] w[c][j])."""
    B, (C, kw) = x.shape[0], w.shape
    idx = torch.arange(L_valid)[:, None] * stride + torch.arange(kw)[None, :]
    y = torch.einsum("btj,cj->btc", x[:, idx], w)
    if bias is not None:
        y = y + bias
    if relu:
        y = y.clamp_min(0)
    out = torch.zeros(B, L_alloc, C, dtype=x.dtype)
    out[:, :L_valid] = y
    return out


def conv1_bwd(x, dy, stride, kw, L_valid):
    """x [B][ldx], dy [B][L_alloc][C] -> [(kw+1)][C]: rows j < kw  sum_{b,t} dy[b][t][c] x[b][t s + j];  row kw  sum_{b,t} dy[b][t][c]."""
    idx = torch.arange(L_valid)[:, None] * stride + torch.arange(kw)[None, :]
    g = dy[:, :L_valid]
    return torch.cat([torch.einsum("btj,btc->jc", x[:, idx], g), g.sum((0, 1))[None]], 0)


# ------------------------------------------------------------------------------------------------------------------ layers >= 2
def conv_fwd(x, w, bias, stride, Lout_valid, Lout_alloc, relu):
    """x [B][Lin_alloc][Cin], w [Cout][Cin][kw] -> y [B][Lout_alloc][Cout], pad rows zero.  Explicit index arithmetic."""
    B, (Cout, Cin, kw) = x.shape[0], w.shape
    idx = torch.arange(Lout_valid)[:, None] * stride + torch.arange(kw)[None, :]
    y = torch.einsum("btjc,ocj->bto", x[:, idx], w)
    if bias is not None:
        y = y + bias
    if relu:
        y = y.clamp_min(0)
    out = torch.zeros(B, Lout_alloc, Cout, dtype=x.dtype)
    out[:, :Lout_valid] = y
    return out


def conv_dgrad(dy, w, stride, Lin_alloc, x_act=None):
    """dy [B][Lout_alloc][Cout] -> dx [B][Lin_alloc][Cin]: dx[b][p][c] = sum_{t, j: t s + j = p} sum_co dy[b][t][co] w[co][c][j],
    times (x_act > 0) when a mask is given.  Contributions that would land beyond Lin_alloc (they come from the last D - 1 rows of an
    item, which the layout keeps zero) must be zero."""
    B, Lout_alloc, Cout = dy.shape
    Cin, kw = w.shape[1], w.shape[2]
    ext = torch.zeros(B, (Lout_alloc - 1) * stride + kw + stride, Cin, dtype=dy.dtype)
    for j in range(kw):
        ext[:, j:j + (Lout_alloc - 1) * stride + 1:stride] += dy @ w[:, :, j]
    assert not bool(ext[:, Lin_alloc:].any()), "dy does not end in D - 1 zero pad rows"
    dx = ext[:, :Lin_alloc].clone()
    if x_act is not None:
        dx = dx * (x_act > 0).to(dx.dtype)
    return dx


def conv_wgrad(x, dy, stride, kw):
    """-> dw [Cout][Cin][kw] = sum_{b,t} x[b][t s + j][c] dy[b][t][co] over the rows whose window lies inside the item (the others are
    pad rows: dy is zero there)."""
    Lin_alloc, Lout_alloc = x.shape[1], dy.shape[1]
    nt = min(Lout_alloc, (Lin_alloc - kw) // stride + 1)
    assert not bool(dy[:, nt:].any())
    idx = torch.arange(nt)[:, None] * stride + torch.arange(kw)[None, :]
    return torch.einsum("btjc,bto->ocj", x[:, idx], dy[:, :nt])


def slab_layout(dw):
    """[Cout][Cin][kw] -> the slab layout of cpc_conv_wgrad [(j, c)][co]."""
    Cout, Cin, kw = dw.shape
    return dw.permute(2, 1, 0).reshape(kw * Cin, Cout)


def w_fwd_layout(w):
    """fwd[co][(j, c)] = w[co][c][j]."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def w_dgrad_layout(w, stride, fill_from_last=False, reverse_dd=False):
    """dgrd[(r, c)][(dd, co)] = w[co][c][r + (D - 1 - dd) stride], zero where that tap >= kw; D = ceil(kw / stride).
    fill_from_last / reverse_dd: the two deliberate mistakes of test_conv1d_reference_host.py."""
    Cout, Cin, kw = w.shape
    D = -(-kw // stride)
    out = torch.zeros(stride, Cin, D, Cout, dtype=w.dtype)
    for r in range(stride):
        for dd in range(D):
            tap = r + (D - 1 - (D - 1 - dd if reverse_dd else dd)) * stride
            if tap < kw:
                out[r, :, dd, :] = w[:, :, tap].T
            elif fill_from_last:
                out[r, :, dd, :] = w[:, :, kw - 1].T
    return out.reshape(stride * Cin, D * Cout)


def dgrad_by_gemm(dy, wd, stride, Cin, x_act=None):
    """The data gradient the way the device forms it: GEMM row (b, q) = the D rows of dy ending at q in the FLAT buffer (row 0 of item
    b reads the last D - 1 rows of item b - 1; D - 1 zero rows precede item 0), times the w_dgrad operand."""
    B, Lout_alloc, Cout = dy.shape
    D = wd.shape[1] // Cout
    flat = torch.cat([torch.zeros((D - 1), Cout, dtype=dy.dtype), dy.reshape(-1, Cout)], 0)
    rows = flat.unfold(0, D, 1).permute(0, 2, 1).reshape(B * Lout_alloc, D * Cout)       # [(b,q)][(dd, co)]
    dx = (rows @ wd.T).reshape(B, Lout_alloc * stride, Cin)
    if x_act is not None:
        dx = dx * (x_act > 0).to(dx.dtype)
    return dx


# ------------------------------------------------------------------------------------------------------------------ reductions
def reduce_slabs(slabs, I, J, cdiv, s_j, s_hi, s_lo, out):
    """slabs [nslab][I][J]: out[j s_j + (i / cdiv) s_hi + (i % cdiv) s_lo] = sum_z slabs[z][i][j]; other elements of out stay."""
    out = out.clone()
    out[reduce_index(I, J, cdiv, s_j, s_hi, s_lo)] = slabs.reshape(slabs.shape[0], I * J).sum(0).to(out.dtype)
    return out


def reduce_index(I, J, cdiv, s_j, s_hi, s_lo):
    """The element of out that slab element (i, j) goes to, for all (i, j) in storage order."""
    i, j = torch.arange(I)[:, None], torch.arange(J)[None, :]
    return (j * s_j + (i // cdiv) * s_hi + (i % cdiv) * s_lo).reshape(-1)


def abs_bound_terms(fn, *tensors, **kw):
    """S of a reference: the same function on the absolute values of its tensor arguments (None stays None); masks, ReLU and other
    non-tensor arguments are passed through kw."""
    return fn(*[None if t is None else t.abs() for t in tensors], **kw)


# ------------------------------------------------------------------------------------------------------------------ data
def gen(seed):
    return torch.Generator().manual_seed(seed)


def normal(g, *shape):
    return torch.randn(*shape, generator=g)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def sparse(g, t, keep):
    """Keeps each element with probability keep (exact-data twins: so that sum |a||b| stays <= 256)."""
    return t * (torch.rand(t.shape, generator=g) < keep).to(t.dtype)


EXACT_MAX = 256.0


# ------------------------------------------------------------------------------------------------------------------ cases: layer 1
C1_SHAPES = [(8, 1, 1), (8, 16, 8), (16, 10, 5), (128, 9, 8), (128, 11, 3), (256, 10, 5), (512, 10, 5), (512, 16, 8), (512, 1, 1),
             (512, 7, 8), (1024, 10, 5), (2048, 16, 1), (2048, 10, 8)]
C1_FWD_LV = [1, 255, 256, 257, 600]
C1_FWD_PAD = [0, 3, 300]
C1_BWD_LV = [1, 63, 64, 65, 600]


def c1_fwd_cases():
    """(C, kw, stride, L_valid, pad, relu, has_bias, slack): for every lane layout (every C) each value of L_valid, pad, relu, bias and
    slack appears at least once: the values are dealt round-robin with different periods over the shapes of one C and every C gets at
    least five cases."""
    cases = []
    byC = {}
    for shp in C1_SHAPES:
        byC.setdefault(shp[0], []).append(shp)
    for C, shapes in byC.items():
        for k in range(max(6, len(shapes))):
            _, kw, s = shapes[k % len(shapes)]
            cases.append((C, kw, s, C1_FWD_LV[k % 5], C1_FWD_PAD[(k + k // 3) % 3], (k + 1) % 2, (k // 2 + 1) % 2, (0, 7)[(k // 2 + k) % 2]))
    # every (C, kw, stride) at least once
    seen = {c[:3] for c in cases}
    for k, shp in enumerate(C1_SHAPES):
        if shp not in seen:
            cases.append(shp + (C1_FWD_LV[(k + 2) % 5], C1_FWD_PAD[k % 3], k % 2, (k + 1) % 2, (0, 7)[k % 2]))
    return cases


def c1_bwd_cases():
    """(C, kw, stride, B, L_valid, nblk_t, nblk_b): L_valid x nblk_t in {1, 3, ceil(L_valid / 64) + 2} x nblk_b in {1, 2, B}, B in {3, 5},
    dealt over the shapes so that every C sees every value of every axis."""
    cases = []
    byC = {}
    for shp in C1_SHAPES:
        byC.setdefault(shp[0], []).append(shp)
    for C, shapes in byC.items():
        for k in range(max(6, len(shapes))):
            _, kw, s = shapes[k % len(shapes)]
            B = (3, 5)[k % 2]
            Lv = C1_BWD_LV[k % 5]
            nt = (1, 3, -(-Lv // 64) + 2)[(k + k // 3) % 3]
            nb = (1, 2, B)[(k + k // 5 + 1) % 3]
            cases.append((C, kw, s, B, Lv, nt, nb))
    seen = {c[:3] for c in cases}
    for k, shp in enumerate(C1_SHAPES):
        if shp not in seen:
            B, Lv = (3, 5)[k % 2], C1_BWD_LV[(k + 1) % 5]
            cases.append(shp + (B, Lv, (1, 3, -(-Lv // 64) + 2)[k % 3], (1, 2, B)[(k + 2) % 3]))
    return cases


def c1_fwd_id(c):
    C, kw, s, Lv, pad, relu, hb, slack = c
    return f"C{C}-k{kw}-s{s}-L{Lv}+{pad}-relu{relu}-bias{hb}-slack{slack}"


def c1_bwd_id(c):
    C, kw, s, B, Lv, nt, nb = c
    return f"C{C}-k{kw}-s{s}-B{B}-L{Lv}-t{nt}-b{nb}"


def c1_fwd_data(case, dt, exact, B=3):
    """x [B][ldx] f32 values (unused samples NaN when ldx has slack), w, bias as float64 tensors exact in f32."""
    C, kw, s, Lv, pad, relu, hb, slack = case
    g = gen(1000 * C + 100 * kw + 10 * s + Lv + pad + (7 if exact else 0))
    need = (Lv - 1) * s + kw
    ldx = need + slack
    if exact:
        x = ints(g, -2, 2, B, ldx)
        w = ints(g, -1, 1, C, kw)
        bias = ints(g, -2, 2, C) if hb else None
    else:
        x = normal(g, B, ldx).float().double()
        w = (normal(g, C, kw) / kw ** 0.5).float().double()
        bias = (normal(g, C) * 0.5).float().double() if hb else None
    x_dev = x.clone()
    x_dev[:, need:] = float("nan")
    return x[:, :need].contiguous(), x_dev, w, bias, ldx


def c1_bwd_data(case, dt, exact):
    """x f32-exact, dy [B][L_alloc][C] exact in dt with zero pad rows (L_alloc = L_valid + 2)."""
    C, kw, s, B, Lv, nt, nb = case
    g = gen(2000 * C + 100 * kw + 10 * s + Lv + B + (7 if exact else 0))
    ldx = (Lv - 1) * s + kw
    La = Lv + 2
    if exact:
        x = ints(g, -2, 2, B, ldx)
        dy = sparse(g, ints(g, -1, 1, B, La, C), min(1.0, 48.0 / (B * Lv)))
    else:
        x = normal(g, B, ldx).float().double()
        dy = rounded(normal(g, B, La, C), dt)
        dy = dy * (torch.rand(dy.shape, generator=g) < 0.6)            # (already ReLU-masked gradients: some exact zeros)
    dy[:, Lv:] = 0
    return x, dy, ldx, La


# ------------------------------------------------------------------------------------------------------------------ cases: layers >= 2
CONV_SHAPES = [(64, 64, 7, 3), (64, 32, 5, 1), (32, 64, 3, 2), (64, 64, 4, 4), (64, 64, 2, 4), (24, 40, 3, 1), (16, 16, 40, 2),
               (64, 64, 33, 1), (64, 64, 8, 4)]
PREP_SHAPES = CONV_SHAPES + [(512, 512, 8, 4), (96, 40, 8, 4)]
CONV_B, CONV_LOUT = 3, 17


def conv_id(s):
    return "ci%d-co%d-k%d-s%d" % s


def conv_geometry(shape, slack):
    """The tightest layout the guard contract allows.  slack False: Lin_valid = (Lout_valid - 1) s + kw; True: the largest Lin_valid that
    adds no output position and fits the allocation (valid input positions no window covers)."""
    Cin, Cout, kw, s = shape
    D = -(-kw // s)
    Lout_alloc = CONV_LOUT + (D - 1)
    Lin_alloc = s * Lout_alloc
    base = (CONV_LOUT - 1) * s + kw
    r = min(s - 1, Lin_alloc - base) if slack else 0
    return dict(D=D, Lout_valid=CONV_LOUT, Lout_alloc=Lout_alloc, Lin_alloc=Lin_alloc, Lin_valid=base + r,
                x_tail=max(0, kw - s) * Cin, dy_head=(D - 1) * Cout)


def conv_data(shape, dt, exact, slack):
    """x [B][Lin_alloc][Cin] post-ReLU data (about half zeros, rows >= Lin_valid zero), w, bias, dy [B][Lout_alloc][Cout] with zero pad
    rows; all float64, exact in dt (w, bias: w is rounded where it is used as an operand, bias stays f32)."""
    Cin, Cout, kw, s = shape
    geo = conv_geometry(shape, slack)
    g = gen(Cin * 1000 + Cout * 100 + kw * 10 + s + (7 if exact else 0) + (3 if slack else 0))
    B, K = CONV_B, kw * Cin
    if exact:
        x = ints(g, 0, 2, B, geo["Lin_alloc"], Cin)
        w = sparse(g, ints(g, -1, 1, Cout, Cin, kw), min(1.0, 40.0 / K, 40.0 / (geo["D"] * Cout)))
        bias = ints(g, -2, 2, Cout)
        dy = sparse(g, ints(g, -2, 2, B, geo["Lout_alloc"], Cout), 0.5)
    else:
        x = rounded(normal(g, B, geo["Lin_alloc"], Cin).clamp_min(0), dt)
        w = rounded(normal(g, Cout, Cin, kw) / K ** 0.5, dt)
        bias = (normal(g, Cout) * 0.5).float().double()
        dy = rounded(normal(g, B, geo["Lout_alloc"], Cout), dt)
    x[:, geo["Lin_valid"]:] = 0
    dy[:, geo["Lout_valid"]:] = 0
    return geo, x, w, bias, dy


def covered_positions(shape, geo):
    """bool [Lin_alloc]: input positions some window of a valid output row covers."""
    Cin, Cout, kw, s = shape
    cov = torch.zeros(geo["Lin_alloc"], dtype=torch.bool)
    for t in range(geo["Lout_valid"]):
        cov[t * s:t * s + kw] = True
    return cov


def nt_variant(dt, M, N, K, lda):
    """What launch_gemm_nt (csrc/gemm.hip) picks for a conv view: ('fast' | 'generic', 'tap-innermost' | 'storage', taps).
    fast: K % (8 ch) == 0 (ch = 8 bf16 / 4 f32 elements per 16 bytes); tap-innermost: fast and lda < K, K % lda == 0, lda % (8 ch) == 0."""
    ch = 8 if dt == BF16 else 4
    bk = 8 * ch
    fast = K % bk == 0
    taps = K // lda if (fast and 0 < lda < K and K % lda == 0 and lda % bk == 0) else 1
    return ("fast" if fast else "generic", "tap-innermost" if taps > 1 else "storage", taps)


def tn_variant(dt, I, J):
    """launch_gemm_tn for cpc_conv_wgrad: 'skinny' (f32, I <= 32, J <= 64, I J / 4 <= 256), 'fast' (bf16, I % 8 == 0) or 'generic'."""
    if dt == F32 and I <= 32 and J <= 64 and I * (J // 4) <= 256:
        return "skinny"
    return "fast" if (dt == BF16 and I % 8 == 0 and I >= 8 and J >= 8) else "generic"


# ------------------------------------------------------------------------------------------------------------------ cases: reductions
REDUCE_CASES = [(1, 64, 7), (1, 64, 15), (1, 64, 16), (1, 2048, 600), (1, 2052, 600), (11, 512, 127), (11, 512, 130), (256, 256, 24),
                (257, 256, 24), (10, 512, 6)]


def reduce_kernel(I, J, nslab):
    """The kernel launch_reduce_slabs picks."""
    total4 = I * J // 4
    if total4 <= 512 and nslab >= 512:
        return "small<256>"
    if total4 <= 16384 and nslab >= 16:
        return "small<64>" if nslab >= 128 else "small<16>"
    return "grid-stride"


def reduce_forms(I, J):
    """(name, cdiv, s_j, s_hi, s_lo, out_elems, out_offset) of the four output forms; the conv-weight permutation where I factors as
    kw cin (the smallest kw > 1 dividing I)."""
    forms = [("plain", 1, 1, J, 0, I * J, 0), ("wide", 1, 1, J + 6, 0, I * (J + 6), 2), ("transposed", 1, I, 1, 0, I * J, 0)]
    kw = next((k for k in range(2, I) if I % k == 0), None)
    if kw:
        cin = I // kw
        forms.append(("convw", cin, cin * kw, 1, kw, I * J, 0))
    return forms


COLSUM_SHAPES = [(1, 8), (5, 12), (77, 8), (1000, 64), (1003, 2048), (130, 2056), (67, 4096)]


def colsum_variant(dt, N, ldx, offset):
    """(vector?, column passes) of launch_colsum: 16-byte loads for f32 with a 16-byte-aligned base, for bf16 with N % 8 == 0,
    ldx % 8 == 0 and such a base; a thread owns 16 bytes of a row then, else 4 columns; 256 column groups per pass."""
    es = 4 if dt == F32 else 2
    aligned = (offset * es) % 16 == 0
    vec = aligned if dt == F32 else (aligned and N % 8 == 0 and ldx % 8 == 0)
    cw = 16 // es if vec else 4
    return vec, -(-(N // cw) // 256)


# ------------------------------------------------------------------------------------------------------------------ cases: tile kernels
TILE_FWD_SHAPE, TILE_FWD_LA, TILE_FWD_B = (32, 256, 4, 2), 1280, (40, 104)
TILE_WGRAD_SHAPE, TILE_WGRAD_LA, TILE_WGRAD_B, TILE_WGRAD_NSPLIT = (64, 256, 8, 4), 520, 4, 2


def tile_fwd_data(B, exact, dt=BF16):
    """x [B][2 La][Cin] post-ReLU, w, bias of the wrapper-level tile-kernel forward cases (D = 2: one pad row per item)."""
    Cin, Cout, kw, s = TILE_FWD_SHAPE
    g = gen(B + (7 if exact else 0))
    if exact:
        x = ints(g, 0, 2, B, s * TILE_FWD_LA, Cin)
        w = sparse(g, ints(g, -1, 1, Cout, Cin, kw), 40.0 / (kw * Cin))
        bias = ints(g, -2, 2, Cout)
    else:
        x = rounded(normal(g, B, s * TILE_FWD_LA, Cin).clamp_min(0), dt)
        w = rounded(normal(g, Cout, Cin, kw) / (kw * Cin) ** 0.5, dt)
        bias = (normal(g, Cout) * 0.5).float().double()
    return x, w, bias


def tile_rows(M, La, Lo, n_random, seed):
    """A seeded subset of the valid GEMM rows (b La + t, t < Lo): first and last valid row of the first and last item, the valid rows
    around the 256-row edges of the first and last tile, and the valid ones of n_random others."""
    last_tile = (M - 1) // 256 * 256
    fixed = [0, Lo - 1, M - La, M - La + Lo - 1, 255, 256, last_tile - 1, last_tile, min(M - 1, last_tile + 255)]
    rows = torch.unique(torch.cat([torch.tensor(fixed), torch.randperm(M, generator=gen(seed))[:n_random]]))
    return rows[(rows % La) < Lo]


def gathered_windows(x, rows, La, stride, kw):
    """[rows][kw][Cin]: the window of GEMM row b La + t as an item of its own (conv_fwd of it with one output row is that row)."""
    return x[(rows // La)[:, None], (rows % La)[:, None] * stride + torch.arange(kw)[None, :]]


def tile_wgrad_data(exact, dt=BF16):
    Cin, Cout, kw, s = TILE_WGRAD_SHAPE
    B, La = TILE_WGRAD_B, TILE_WGRAD_LA
    g = gen(77 + (7 if exact else 0))
    if exact:
        x = ints(g, 0, 2, B, s * La, Cin)
        dy = sparse(g, ints(g, -1, 1, B, La, Cout), 40.0 / (B * La))
    else:
        x = rounded(normal(g, B, s * La, Cin).clamp_min(0), dt)
        dy = rounded(normal(g, B, La, Cout), dt)
    dy[:, La - 1:] = 0
    return x, dy
