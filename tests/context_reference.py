"""Plain float64 references of the context-network kernels (GRU recurrence, causal attention, residual + LayerNorm, dropout masks) and a
float64 emulation of where the GRU kernels round to their storage type.  Shared by test_context_kernels_gpu.py (the kernels against
these references) and test_context_reference_host.py (these references against torch's own modules, the caps on the emulation's error
and the sensitivity of the metrics to deliberate mistakes).  Nothing here touches a device.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16


def rounded(t, dt):
    """The value the device sees after storage in dt (so that references use identical inputs)."""
    return t.to(dt).double()


def ident(t):
    return t


def to_bf16(t):
    return t.to(BF16).double()


def rel_err(got, ref):
    """The whole-tensor measure of the older tests: max |got - ref| / max |ref|."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def per_step_err(got, ref):
    """(B, V, X) -> (V,): max_{b,j} |got - ref| / max_{b,j} |ref| within each time step."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return (got - ref).abs().amax((0, 2)) / (ref.abs().amax((0, 2)) + 1e-30)


# ------------------------------------------------------------------------------------------------------------------ GRU
# (family, storage type, H, B, V) of every kernel case of test_context_kernels_gpu.py
def gru_cases():
    cases = []
    for H in (32, 64, 128, 256):          # weight-resident bf16 (gru_fwd_res_kernel / gru_bwd_res_kernel)
        for B in (1, 16, 17, 33):
            for V in (1, 2, 13):
                cases.append(("resident", BF16, H, B, V))
    for H in (96, 160, 192, 224):         # 4-wave streaming kernels, bf16: waves with unequal or no tiles
        for B in (1, 17):
            for V in (1, 13):
                cases.append(("streaming", BF16, H, B, V))
    for H in (16, 48, 96, 160, 256):      # 4-wave streaming kernels, f32
        for B in (1, 17):
            for V in (1, 13):
                cases.append(("streaming", F32, H, B, V))
    for H in (288, 512):                  # 8-wave kernels
        for dt in (F32, BF16):
            cases.append(("wide", dt, H, 17, 13))
    for dt in (F32, BF16):
        cases.append(("long", dt, 64, 7, 40))
    return cases


def gru_case_seed(case):
    """The data seed of a case: B 1000 + H + V, except the long case, whose emulation error passes the cap of 2e-2 with that seed (dn
    3.3e-2 at one step) and stays below it with seed 2 (1.7e-2; seeds 1 .. 8 give 1.7e-2 .. 3.7e-2)."""
    return 2 if case[0] == "long" else None


def gru_case_h0(case):
    """Short cases start from a random carried state (cpc_gru_fwd_h0: with V = 1 and h_0 = 0 the recurrent weights would not matter);
    the others from zero (cpc_gru_fwd)."""
    return case[4] <= 2


def gru_case_id(case):
    fam, dt, H, B, V = case
    return f"{fam}-{'f32' if dt == F32 else 'bf16'}-H{H}-B{B}-V{V}"


def gru_data(B, V, H, seed=None, with_h0=False):
    """The data recipe of the GRU kernel tests (test_hip_kernels.py::test_gru_fwd_bwd): W_hh ~ N(0, 1/H), b_hh ~ 0.1 N, Gi, dc ~ N(0, 1)."""
    g = torch.Generator().manual_seed(B * 1000 + H + V if seed is None else seed)
    w_hh = torch.randn(3 * H, H, generator=g) / math.sqrt(H)
    b_hh = torch.randn(3 * H, generator=g) * 0.1
    Gi = torch.randn(B, V, 3 * H, generator=g)
    dc = torch.randn(B, H, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.5 if with_h0 else None
    return w_hh, b_hh, Gi, dc, h0


def gru_run(Gi, w, b, dc, h0=None, rnd=ident, mutation=None, below=None):
    """The GRUCell recurrence of audio_model.py:66-77 and its backward through time, written out in float64.
    Gi (B, V, 3H) input projections, w (3H, H), b (3H), dc (B, H) the gradient at the last hidden state, h0 (B, H) or None.
    Returns Hall (B, V+1, H), c (B, H), dG (B, V, 4H) = [d r_pre | d u_pre | d n_pre | d n_pre * r].

    rnd is applied where the kernels of csrc/gru.hip store in their storage type (ident: the pure float64 reference):
      forward   the LDS copy of h that feeds the MFMAs (hbuf / hnext: store4((T*)hnext ...)), the stored Hall, and the five tape
                values r, u, n, q = W_hn h + b_hn, h_prev; the master copy of h (hprev[][]) and c_out stay f32 (here: unrounded);
      backward  the gate values are the tape's; the dgh tile (dr, du, dn*r) that feeds the MFMAs (gcur) and the stored dG; dh stays f32.
    mutation (test_context_reference_host.py's sensitivity checks): "drop_keep": dh_{t-1} loses its dh*u term for t < below
    (default V - 3); "scale_rec": the dgh W_hh term is scaled by 0.9."""
    B, V, H3 = Gi.shape
    H = H3 // 3
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    hall, tape = [rnd(h)], []
    for t in range(V):
        gh = rnd(h) @ w.T + b
        r = torch.sigmoid(Gi[:, t, :H] + gh[:, :H])
        u = torch.sigmoid(Gi[:, t, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        n = torch.tanh(Gi[:, t, 2 * H:] + r * q)
        tape.append((rnd(r), rnd(u), rnd(n), rnd(q), rnd(h)))
        h = (1 - u) * n + u * h
        hall.append(rnd(h))
    c = h
    dh = dc
    dG = torch.zeros(B, V, 4 * H, dtype=torch.float64)
    for t in range(V - 1, -1, -1):
        r, u, n, q, hp = tape[t]
        dn_pre = dh * (1 - u) * (1 - n * n)
        du_pre = dh * (hp - n) * u * (1 - u)
        dr_pre = dn_pre * q * r * (1 - r)
        dnr = dn_pre * r
        dG[:, t] = torch.cat([rnd(dr_pre), rnd(du_pre), rnd(dn_pre), rnd(dnr)], 1)
        keep = dh * u
        rec = torch.cat([rnd(dr_pre), rnd(du_pre), rnd(dnr)], 1) @ w
        if mutation == "drop_keep" and t < (V - 3 if below is None else below):
            keep = torch.zeros_like(keep)
        if mutation == "scale_rec":
            rec = rec * 0.9
        dh = keep + rec
    return torch.stack(hall, 1), c, dG


GRU_BLOCKS = ("Hall", "dr", "du", "dn", "dnr")


def gru_step_errors(hall, dG, ref_hall, ref_dG):
    """Per-step errors {block: (V,)} of the hidden states h_1 .. h_V and of the four blocks of dG."""
    H = ref_hall.shape[2]
    hall, dG = torch.as_tensor(hall).detach().double().cpu(), torch.as_tensor(dG).detach().double().cpu()
    out = {"Hall": per_step_err(hall[:, 1:], ref_hall[:, 1:])}
    for i, name in enumerate(GRU_BLOCKS[1:]):
        out[name] = per_step_err(dG[:, :, i * H:(i + 1) * H], ref_dG[:, :, i * H:(i + 1) * H])
    return out


GRU_TOL_F32 = {"Hall": 2e-5, "dr": 5e-5, "du": 5e-5, "dn": 5e-5, "dnr": 5e-5}       # the f32 figures of test_gru_fwd_bwd, now per step
GRU_MODEL_CAP = 2e-2          # the bf16 emulation alone stays below this at every step of every case
GRU_MODEL_FACTOR = 4.0        # device <= 4 e_model(t): the f32 summation order of the MFMAs and the device's exp / rcp


def gru_reference(dt, B, V, H, seed=None, with_h0=False, zero_weights=False):
    """Inputs as the device stores them, the float64 reference, and the per-step tolerances {block: (V,)}.
    f32: the constants above.  bf16: 4 x e_model(t), e_model = the error of the emulation (gru_run with bf16 rounding) against float64."""
    w_hh, b_hh, Gi, dc, h0 = gru_data(B, V, H, seed, with_h0)
    if zero_weights:          # ... and input projections that differ in every (b, t, j): a shuffled ramp over [-3, 3]
        w_hh, b_hh = torch.zeros_like(w_hh), torch.zeros_like(b_hh)
        n = Gi.numel()
        Gi = torch.linspace(-3, 3, n)[torch.randperm(n, generator=torch.Generator().manual_seed(n))].reshape(Gi.shape)
    wr, br, gir, dcr = rounded(w_hh, dt), b_hh.double(), rounded(Gi, dt), dc.double()
    h0r = None if h0 is None else h0.double()
    hall, c, dG = gru_run(gir, wr, br, dcr, h0r)
    if dt == F32:
        tol = {k: torch.full((V,), v, dtype=torch.float64) for k, v in GRU_TOL_F32.items()}
        e_model = None
    else:
        e_model = gru_step_errors(*gru_run(gir, wr, br, dcr, h0r, rnd=to_bf16)[::2], hall, dG)
        tol = {k: GRU_MODEL_FACTOR * v for k, v in e_model.items()}
    return dict(w_hh=w_hh, b_hh=b_hh, Gi=Gi, dc=dc, h0=h0, wr=wr, br=br, gir=gir, hall=hall, c=c, dG=dG, tol=tol, e_model=e_model)


def gru_weight_grads(dG, hall):
    """(d b_hh, d W_hh) from dG and the hidden states: the column sums and sum_t dGh_t^T h_{t-1} of the gradient w.r.t. h W_hh^T + b_hh."""
    H = hall.shape[2]
    dG, hall = torch.as_tensor(dG).detach().double().cpu(), torch.as_tensor(hall).detach().double().cpu()
    dGh = torch.cat([dG[:, :, :2 * H], dG[:, :, 3 * H:]], 2)
    return dGh.sum((0, 1)), torch.einsum("bvg,bvh->gh", dGh, hall[:, :-1])


def gru_closed_form_zero_weights(gir, h0=None):
    """W_hh = 0, b_hh = 0: h_t = (1 - sigmoid(a_u)) tanh(a_n) + sigmoid(a_u) h_{t-1} elementwise (no matrix product at all)."""
    B, V, H3 = gir.shape
    H = H3 // 3
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    hs = [h]
    for t in range(V):
        u = torch.sigmoid(gir[:, t, H:2 * H])
        h = (1 - u) * torch.tanh(gir[:, t, 2 * H:]) + u * h
        hs.append(h)
    return torch.stack(hs, 1)


# ------------------------------------------------------------------------------------------------------------------ dropout masks
_M64 = (1 << 64) - 1


def dropout_mask_host(n, p, seed, site):
    """cpc_dropout_mask on the host (csrc/attn.hip: drop_hash / drop_factor / make_drop): factor 1/(1-p) in f32 where the upper half of a
    64-bit mix of (seed, site, index) is >= p 2^32, else 0."""
    if p <= 0:
        return torch.ones(n, dtype=torch.float64)
    pf = float(np.float32(p))
    thresh = int(min(4294967295.0, pf * 4294967296.0))
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64)
        base = np.uint64((seed + 0x9E3779B97F4A7C15 * (site + 1)) & _M64)
        z = base + idx * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    keep = (z >> np.uint64(32)) >= np.uint64(thresh)
    return torch.from_numpy(np.where(keep, inv_keep, 0.0))


# ------------------------------------------------------------------------------------------------------------------ attention
ATTN_SEQS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
# (C, heads): head size 64 (the matrix pipe in bf16), 32, 8, 60 (not a power of two) and 4 (the smallest)
ATTN_SHAPES = [(128, 2), (64, 2), (64, 8), (120, 2), (8, 2)]


def attn_tol(dt):
    return 3e-5 if dt == F32 else 1.2e-2


def attn_bwd_tol(dt):
    return 1e-4 if dt == F32 else 2.5e-2


def attn_inputs(B, S, C, heads, dt, seed, qk_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * C, generator=g)
    qkv[:, :2 * C] *= qk_scale
    return rounded(qkv, dt), rounded(torch.randn(B * S, C, generator=g), dt)


def attn_reference(qkv, dout, B, S, C, heads, m=None, mutation=None, dtype=torch.float64):
    """Causal softmax(q k^T / sqrt(d)) v per head with dropout factors m (B, heads, S, S) on the weights; autograd gives d qkv.
    Returns (P, out, dqkv).  mutation: "strict_causal" masks j >= i instead of j > i (row 0 then attends to itself only through
    the guard below); "transposed_mask" reads the dropout factor of (i, j) at index j S + i; "no_max" computes the softmax without
    subtracting the row maximum, in `dtype`."""
    d = C // heads
    qkv = qkv.to(dtype).clone().requires_grad_(True)
    if m is None:
        m = torch.ones(B, heads, S, S, dtype=dtype)
    m = m.to(dtype)
    if mutation == "transposed_mask":
        m = m.transpose(-1, -2)
    q, k, v = (t.reshape(B, S, heads, d).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1))
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(d)
    allowed = torch.tril(torch.ones(S, S, dtype=torch.bool), -1 if mutation == "strict_causal" else 0)
    if mutation == "strict_causal":
        allowed[0, 0] = True          # (a row must keep one entry)
    if mutation == "no_max":
        e = torch.exp(sc) * allowed
        P = e / e.sum(-1, keepdim=True)
    else:
        P = torch.softmax(sc.masked_fill(~allowed, float("-inf")), -1)
    out = ((P * m) @ v).permute(0, 2, 1, 3).reshape(B * S, C)
    out.backward(dout.to(dtype))
    return P.detach(), out.detach(), qkv.grad


def attn_score_delta(qkv, B, S, C, heads):
    """delta = 2 scale 2^-24 max_{i,j} sum_c |q_ic k_jc|: a bound of first order on what f32 products and sums move a scaled score by
    (each of the d products and each partial sum is rounded to 24 bits; the factor 2 is the bound the derivation uses for the two).
    A softmax weight then moves by a factor of at most exp(delta) - 1 relative to itself, hence relative to the largest weight."""
    d = C // heads
    q, k = (t.double().abs().reshape(B, S, heads, d).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1)[:2])
    return 2.0 / math.sqrt(d) * 2.0 ** -24 * float((q @ k.transpose(-1, -2)).max())


def attn_exact_data(B, S, C, heads):
    """q = 0, v[j][c] = 1 if c == j mod d: P[i][j] = 1/(i+1) for j <= i, out[i][c] = #{j <= i: j mod d == c} / (i+1)."""
    d = C // heads
    qkv = torch.zeros(B, S, 3, heads, d, dtype=torch.float64)
    qkv[:, :, 1] = torch.randn(B, S, heads, d, generator=torch.Generator().manual_seed(S))      # k does not matter
    j = torch.arange(S)
    qkv[:, j, 2, :, j % d] = 1.0
    i = torch.arange(S).double()
    P = torch.tril(torch.ones(S, S, dtype=torch.float64)) / (i + 1)[:, None]
    cnt = torch.zeros(S, d, dtype=torch.float64)
    for ii in range(S):
        for jj in range(ii + 1):
            cnt[ii, jj % d] += 1
    out = (cnt / (i + 1)[:, None])[None, :, None, :].expand(B, S, heads, d).reshape(B * S, C)
    return qkv.reshape(B * S, 3 * C), P, out


def bf16_ulp(ref):
    """Spacing of bf16 numbers at |ref| (8 significant bits)."""
    _, e = torch.frexp(ref.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 8)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5
# mean and rstd are f32 sums over a row: at most 16 additions in a lane, 6 exchange levels, the product with the dropout factor, the
# sum a + b, the division by C and the reciprocal square root: fewer than 32 roundings of 2^-24 each on top of one another
LN_STAT_ROUNDINGS = 32


def ln_reference(a, b, w, bias, dy, mask=None, eps=LN_EPS):
    """float64: r = a + mask b, y = F.layer_norm(r) w + bias, and the gradients for dy: returns y, r, mean, rstd, dr, dw, dbias."""
    r = a.clone()
    if b is not None:
        r = r + (b if mask is None else b * mask)
    r = r.requires_grad_(True)
    w = w.clone().requires_grad_(True)
    bias = bias.clone().requires_grad_(True)
    y = F.layer_norm(r, (r.shape[1],), w, bias, eps)
    y.backward(dy)
    rd = r.detach()
    mean = rd.mean(1)
    rstd = 1.0 / torch.sqrt(rd.var(1, unbiased=False) + eps)
    return y.detach(), rd, mean, rstd, r.grad, w.grad, bias.grad


def _sum_sequential(x):
    return np.cumsum(x, axis=1, dtype=np.float32)[:, -1]


def _sum_pairwise(x):
    x = x.astype(np.float32)
    while x.shape[1] > 1:
        if x.shape[1] % 2:
            x = np.concatenate([x, np.zeros((x.shape[0], 1), np.float32)], 1)
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _sum_lane_strided(x):
    """The order of add_ln_fwd_kernel: lane l adds the column groups l, l + 64, ... (four columns each, left to right), then the 64
    lanes combine by exchanges over the distances 32, 16, .., 1."""
    M, C = x.shape
    c4n = C // 4
    lanes = np.zeros((M, 64), np.float32)
    for u in range((c4n + 63) // 64):
        for lane in range(min(64, c4n - 64 * u)):
            v = x[:, 4 * (lane + 64 * u):4 * (lane + 64 * u) + 4].astype(np.float32)
            lanes[:, lane] = lanes[:, lane] + (((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3])
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o //= 2
    return lanes[:, 0]


LN_F32_ORDERS = {"sequential": _sum_sequential, "pairwise": _sum_pairwise, "lane-strided": _sum_lane_strided}


def ln_forward_f32(x, w, bias, order, one_pass=False, eps=LN_EPS):
    """LayerNorm forward in float32 on the host with a given order of summation; two passes as the kernel (mean, then the squared
    deviations), or (one_pass) var = E[x^2] - E[x]^2.  Returns y, mean, rstd as float32 arrays."""
    x = np.asarray(x, np.float32)
    C = np.float32(x.shape[1])
    s = LN_F32_ORDERS[order]
    mean = s(x) / C
    if one_pass:
        var = s(x * x) / C - mean * mean
    else:
        dev = x - mean[:, None]
        var = s(dev * dev) / C
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = (x - mean[:, None]) * rstd[:, None] * np.asarray(w, np.float32) + np.asarray(bias, np.float32)
    return y, mean, rstd


def ln_large_mean_data(M, C):
    g = torch.Generator().manual_seed(C)
    x = (1000.0 + torch.randn(M, C, generator=g)).float()
    w = (1 + 0.3 * torch.randn(C, generator=g)).float()
    bias = (0.2 * torch.randn(C, generator=g)).float()
    return x, w, bias


def ln_large_mean_errors(y, rstd, x, w, bias):
    """(error of y relative to its largest entry, largest relative error of rstd) against float64."""
    y64, _, _, rstd64, _, _, _ = ln_reference(x.double(), None, w.double(), bias.double(), torch.zeros(x.shape, dtype=torch.float64))
    y, rstd = torch.as_tensor(y).double().cpu(), torch.as_tensor(rstd).double().cpu()
    return rel_err(y, y64), float(((rstd - rstd64).abs() / rstd64).max())


def ln_large_mean_bound(M, C):
    """4 x the largest error of the float32 two-pass algorithm over the three summation orders: (bound on y, bound on rstd, the
    errors per order)."""
    x, w, bias = ln_large_mean_data(M, C)
    errs = {}
    for order in LN_F32_ORDERS:
        y, _, rstd = ln_forward_f32(x.numpy(), w.numpy(), bias.numpy(), order)
        errs[order] = ln_large_mean_errors(torch.from_numpy(y), torch.from_numpy(rstd), x, w, bias)
    return 4 * max(e[0] for e in errs.values()), 4 * max(e[1] for e in errs.values()), errs


# ------------------------------------------------------------------------------------------------------------------ shared verdicts
def gru_violations(errs, tol):
    """[(block, step, error, bound)] where a per-step error is not within its bound (a NaN is a violation)."""
    bad = []
    for k in GRU_BLOCKS:
        for t, (e, b) in enumerate(zip(errs[k].tolist(), tol[k].tolist())):
            if not e <= b:
                bad.append((k, t, e, b))
    return bad


# Large scores: q and k scaled by 3 (scores reach about +-30) and by 5.5 (about +-100: beyond 88.7, where exp overflows in f32, so that
# a softmax without max-subtraction cannot survive; at +-30 it would, exp(30) being an ordinary f32 number)
ATTN_LARGE_CASES = [(S, C, heads) for S in (17, 64) for C, heads in ((64, 2), (128, 2))]
ATTN_LARGE_SCALES = (3.0, 5.5)


def attn_large_tol(dt, delta):
    """The tolerance of P and out at large scores: the usual one; in f32 plus exp(delta) - 1 (attn_score_delta: derived, not measured)."""
    return attn_tol(dt) + (math.expm1(delta) if dt == F32 else 0.0)
