"""Float64 references, float32 host emulations, measures, bounds and the case tables of the gradient-penalty kernels: cpc_gru_gp_fwd /
cpc_gru_gp_bwd (csrc/gru.hip) and cpc_ln_tangent / cpc_ln_gp / cpc_attn_tangent / cpc_attn_gp / cpc_attn128_tangent / cpc_attn128_gp
(csrc/attn.hip).  Shared by test_penalty_kernels_gpu.py (the kernels against these references) and test_penalty_reference_host.py
(the references against each other and against autograd's double backward, the caps on the emulations' errors, and the table of
deliberate mistakes that the measures must reject).  Nothing here touches a device.

The references are the operations' definitions, not the kernels' formulas:
  GRU        a float64 joint (primal, tangent) recurrence with zero-valued probe leaves on the four pre-activations and on their four
             tangents; D = <wc, tangent of h_V> differentiated once: the gradients at the tangent probes are the four delta blocks of dA,
             those at the primal probes the four second-order blocks.  Independently: autograd's double backward of the plain GRU.
  attention  torch.autograd.functional.jvp of the causal softmax attention (with dropout factors on the weights) gives the tangent,
             grad(<dO, tangent>, qkv) what cpc_attn*_gp must add.
  LayerNorm  the same on LayerNorm(a + dropout(b)) w; the gradient with respect to w is the sum of the slabs.
The closed formulas that the older tests restate (tools/gp_attention_algebra.py's) are kept here as a second implementation
(attn_gp_closed, ln_gp_closed); run in float32 they are the emulations whose error against float64 gives every bound:
  bound of a block = max(4 x the emulation's largest error in that block, FLOOR), and 0 where the reference is exactly 0
  (bounds_from).
"""
import math

import numpy as np
import torch

import context_reference as R

U24 = 2.0 ** -24
# Floor of a bound, for blocks where the float32 emulation happens to be exact (q = b_hn at t = 0, a sigmoid that lands on an f32
# number): an elementwise output of one step is at most 16 float32 roundings of 2^-24 away from its inputs (the bias + projection sum,
# exp, 1 + e, the reciprocal, r q, the sum under tanh, tanh, and the products of the tangent and adjoint formulas, none of which
# chains more than 8 operations, each counted twice for fma contraction and the device's exp / tanh being within 2 ulp).  The
# elementwise outputs of the attention and LayerNorm kernels at their smallest shapes (S = 1: out_t = m vt; C = 4) stay within the same count.
FLOOR = 16 * U24
FACTOR = 4.0                  # device <= 4 x emulation: fma contraction, device expf / tanhf, reduction order
# No bound may exceed 10 x the older tests' tolerance for the same quantity, so the emulation alone must stay below a quarter of that.
CAP = {"gru": 10 * 2e-4 / FACTOR, "gru_ct": 10 * 1e-4 / FACTOR,                                    # L2 2e-4 of the gradients; ct 1e-4
       "attn_out_t": 10 * 1e-5 / FACTOR, "attn_inc": 10 * 1e-4 / FACTOR,                          # out_t 1e-5; acc - lam 1e-4
       "ln_rt": 10 * 1e-6 / FACTOR, "ln_yt": 10 * 1e-5 / FACTOR, "ln_inc": 10 * 1e-4 / FACTOR}    # rt 1e-6, yt 1e-5, dr / slabs 1e-4


def f32_exact(t):
    return t.float().double()


def block_err(got, ref, dims):
    """max over dims of |got - ref| relative to max over dims of |ref|; where the reference block is exactly 0 the error is 0 if the
    block is exactly 0 (either sign) and inf otherwise: such a block is never skipped.  NaN stays NaN (and fails every bound)."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    num, den = (got - ref).abs().amax(dims), ref.abs().amax(dims)
    zero = torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf")))
    zero = torch.where(torch.isnan(num), num, zero)
    return torch.where(den == 0, zero, num / den.clamp_min(1e-300))


def bounds_from(e_emul, ref_zero=None):
    """{block: tensor of the emulation's errors per step / position / row} -> bounds of the same shape.  The bound of a block (a tape
    slot, a dA block, ct, one assembled gradient, out_t, a third of the increment, rt, yt, ...) is 4 x the LARGEST error of the
    emulation in that block, the same at every step / position / row of the block; the measure stays relative to the reference's
    maximum within each step / position / row, so a step whose values are 1e-7 of the last step's is judged against its own size.
    (One error per (block, step) is a single sample of rounding noise: 4 x that sample is no bound on another sample, least of all
    over the 1536 rows of a weight gradient.)  Where the reference is exactly 0 (ref_zero: {block: bool tensor}) the bound is 0."""
    out = {}
    for k, e in e_emul.items():
        b = torch.full_like(e, max(FACTOR * float(e.max()), FLOOR))
        if ref_zero is not None:
            b = torch.where(ref_zero[k], torch.zeros_like(b), b)
        out[k] = b
    return out


def violations(errs, bounds):
    """[(name, index, error, bound)] where an error is not within its bound (NaN and inf are violations)."""
    bad = []
    for k in bounds:
        e, b = errs[k].reshape(-1).tolist(), bounds[k].reshape(-1).tolist()
        bad += [(k, i, x, y) for i, (x, y) in enumerate(zip(e, b)) if not x <= y]
    return bad


def worst_ratio(errs, bounds):
    """Largest error / bound over the blocks with a non-zero bound."""
    w = 0.0
    for k in bounds:
        nz = bounds[k] > 0
        if bool(nz.any()):
            w = max(w, float((errs[k][nz] / bounds[k][nz]).max()))
    return w


# ====================================================================================================================== GRU
GRU_E = 16
GRU_SHAPES = [("smallest", 1, 1, 16), ("smallest", 1, 2, 16), ("below one wave", 3, 13, 48), ("one full wave", 2, 13, 64),
              ("partial last wave", 2, 5, 80), ("full width", 2, 3, 512), ("full width", 2, 3, 384), ("decay", 2, 40, 64)]
GRU_RECIPES = ("plain", "saturated", "whh0")


def gru_gp_cases():
    """(route, B, V, H, recipe) of every GRU case of test_penalty_kernels_gpu.py: every shape with the plain recipe; W_hh = 0 on the
    smallest, a partial wave, full width and the decay case; the saturated gates (W_ih x 6) where a row of a weight gradient sums at
    least 26 (item, step) terms.  With fewer terms whole rows of the weight gradients belong to units that are saturated at every
    step: their float64 value is 1e-11 of the matrix's largest entry and float32 gives 0 (r = 1.0f, so r (1 - r) = 0), an error of
    100 % of that row in the emulation itself ((1, 2, 16): 1.0; (2, 5, 80): 7.8e-3), far above the cap; the per-step measures of the
    tape and dA do not suffer from this."""
    cases = [(route, B, V, H, "plain") for route, B, V, H in GRU_SHAPES]
    cases += [(route, B, V, H, "whh0") for route, B, V, H in GRU_SHAPES if (B, V, H) in ((1, 2, 16), (3, 13, 48), (2, 3, 512), (2, 40, 64))]
    cases += [(route, B, V, H, "saturated") for route, B, V, H in GRU_SHAPES if (B, V, H) in ((3, 13, 48), (2, 13, 64), (2, 40, 64))]
    return cases


def gru_gp_case_seed(case):
    """The data seed of a case: B 1000 + H + V, except the saturated decay case, whose emulation error passes the cap of 5e-4 with that
    seed (6.9e-4 in one row of the weight_ih gradient) and stays below it with seed 1 (5.6e-5; seed 2 gives 1.6e-4)."""
    return 1 if case[1:] == (2, 40, 64, "saturated") else None


def gru_gp_case_id(case):
    return f"B{case[1]}-V{case[2]}-H{case[3]}-{case[4]}"


def gru_gp_data(B, V, H, recipe="plain", E=GRU_E, seed=None):
    """The recipe of test_hip_kernels.py::test_gru_gradient_penalty_kernels with seed B 1000 + H + V.  Gi = x W_ih^T + b_ih and
    GiT = xt W_ih^T are rounded to float32 once: these are the device's inputs and the per-step references'."""
    g = torch.Generator().manual_seed(B * 1000 + H + V if seed is None else seed)
    f = lambda *sh, s=1.0: f32_exact(torch.randn(*sh, generator=g) * s)
    Wih, Whh = f(3 * H, E, s=E ** -0.5), f(3 * H, H, s=H ** -0.5)
    bih, bhh = f(3 * H, s=0.3), f(3 * H, s=0.3)
    x, xt, wc = f(B, V, E), f(B, V, E), f(B, H)
    if recipe == "saturated":
        Wih = Wih * 6.0
    elif recipe == "whh0":
        Whh = torch.zeros_like(Whh)
    else:
        assert recipe == "plain"
    Gi64, GiT64 = x @ Wih.T + bih, xt @ Wih.T
    return dict(B=B, V=V, H=H, E=E, Wih=Wih, Whh=Whh, bih=bih, bhh=bhh, x=x, xt=xt, wc=wc, Gi64=Gi64, GiT64=GiT64,
                Gi=f32_exact(Gi64.reshape(B, V, 3 * H)), GiT=f32_exact(GiT64.reshape(B, V, 3 * H)))


def gru_gp_probe_reference(Gi, GiT, Whh, bhh, wc):
    """The probe construction (module docstring).  Returns tape (B, V, 10, H), ct (B, H), dA (B, V, 8, H) in float64."""
    B, V, H3 = Gi.shape
    H = H3 // 3
    probes = [torch.zeros(V, B, H, dtype=torch.float64, requires_grad=True) for _ in range(8)]
    pr, pz, pn, pq, tr, tz, tn, tq = probes
    h = torch.zeros(B, H, dtype=torch.float64)
    ht = torch.zeros(B, H, dtype=torch.float64)
    tape = []
    for t in range(V):
        gh, ght = h @ Whh.T + bhh, ht @ Whh.T
        ar = Gi[:, t, :H] + gh[:, :H] + pr[t]
        az = Gi[:, t, H:2 * H] + gh[:, H:2 * H] + pz[t]
        q = gh[:, 2 * H:] + pq[t]
        art = GiT[:, t, :H] + ght[:, :H] + tr[t]
        azt = GiT[:, t, H:2 * H] + ght[:, H:2 * H] + tz[t]
        qt = ght[:, 2 * H:] + tq[t]
        r, z = torch.sigmoid(ar), torch.sigmoid(az)
        n = torch.tanh(Gi[:, t, 2 * H:] + r * q + pn[t])
        rt, zt = r * (1 - r) * art, z * (1 - z) * azt          # tangents of the sigmoids
        ant = GiT[:, t, 2 * H:] + rt * q + r * qt + tn[t]
        nt = (1 - n * n) * ant
        tape.append(torch.stack([r, z, n, q, h, art, azt, qt, ant, ht], 1).detach())
        h, ht = (1 - z) * n + z * h, zt * (h - n) + (1 - z) * nt + z * ht
    D = (wc * ht).sum()
    gr = torch.autograd.grad(D, probes)
    dA = torch.stack([gr[4], gr[5], gr[6], gr[7], gr[0], gr[1], gr[2], gr[3]], 2).permute(1, 0, 2, 3).contiguous()
    return torch.stack(tape, 1), ht.detach(), dA


def gru_gp_assemble(tape, dA, x, xt, Wih):
    """The five penalty gradients from the kernels' outputs as contexts.GRUContext.gp_grads assembles them (float64 on the host):
    weight_ih, weight_hh, bias_ih, bias_hh, x."""
    tape, dA = torch.as_tensor(tape).double().cpu(), torch.as_tensor(dA).double().cpu()
    B, V, _, H = tape.shape
    E = x.shape[-1]
    da = dA.reshape(B * V, 8 * H)
    hp, htp = tape[:, :, 4].reshape(B * V, H), tape[:, :, 9].reshape(B * V, H)
    X, XT = x.reshape(B * V, E), xt.reshape(B * V, E)
    d3, v3 = da[:, :3 * H], da[:, 4 * H:7 * H]
    dh, vh = torch.cat([da[:, :2 * H], da[:, 3 * H:4 * H]], 1), torch.cat([da[:, 4 * H:6 * H], da[:, 7 * H:]], 1)
    return dict(weight_ih=d3.T @ XT + v3.T @ X, weight_hh=dh.T @ htp + vh.T @ hp, bias_ih=v3.sum(0), bias_hh=vh.sum(0),
                x=(v3 @ Wih).reshape(B, V, E))


GRU_GRADS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "x")


def gru_gp_double_backward(d):
    """Autograd's double backward of the plain GRU (unrounded projections): the gradient of D = <xt, d<wc, h_V>/dx> with respect to
    the four parameters and x."""
    B, V, H = d["B"], d["V"], d["H"]
    params = [d[k].clone().requires_grad_(True) for k in ("Wih", "Whh", "bih", "bhh", "x")]
    pWih, pWhh, pbih, pbhh, px = params
    h = torch.zeros(B, H, dtype=torch.float64)
    for t in range(V):
        gi, gh = px[:, t] @ pWih.T + pbih, h @ pWhh.T + pbhh
        r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
    gx, = torch.autograd.grad((d["wc"] * h).sum(), px, create_graph=True)
    return dict(zip(GRU_GRADS, torch.autograd.grad((gx * d["xt"]).sum(), params, allow_unused=True)))


def gru_gp_whh0_closed(d):
    """W_hh = 0: the units decouple and h_V = sum_t (prod_{s>t} z_s) (1 - z_t) n_t is a closed form per unit (cumulative products, no
    recurrence).  f = <wc, h_V> as a function of the pre-activations a_r, a_z, a_n and of q (value b_hn); delta = grad f; D =
    <delta, tangent direction> (GiT on the pre-activations, 0 on q); nu = grad D.  Returns dA (B, V, 8, H) and ct."""
    B, V, H = d["B"], d["V"], d["H"]
    Gi, GiT, bhh = d["Gi"], d["GiT"], d["bhh"]
    a_r = (Gi[:, :, :H] + bhh[:H]).clone().requires_grad_(True)
    a_z = (Gi[:, :, H:2 * H] + bhh[H:2 * H]).clone().requires_grad_(True)
    a_n = Gi[:, :, 2 * H:].clone().requires_grad_(True)
    q = bhh[2 * H:].expand(B, V, H).clone().requires_grad_(True)
    r, z = torch.sigmoid(a_r), torch.sigmoid(a_z)
    n = torch.tanh(a_n + r * q)
    # prod_{s > t} z_s = (prod of all z) / (prod_{s <= t} z_s) would divide; use a reversed cumulative product instead
    zr = torch.flip(torch.cumprod(torch.flip(z, (1,)), 1), (1,))          # prod_{s >= t} z_s
    tail = torch.cat([zr[:, 1:], torch.ones(B, 1, H, dtype=torch.float64)], 1)
    f = (d["wc"] * (tail * (1 - z) * n).sum(1)).sum()
    delta = torch.autograd.grad(f, (a_r, a_z, a_n, q), create_graph=True)
    D = (delta[0] * GiT[:, :, :H]).sum() + (delta[1] * GiT[:, :, H:2 * H]).sum() + (delta[2] * GiT[:, :, 2 * H:]).sum()
    nu = torch.autograd.grad(D, (a_r, a_z, a_n, q))
    ct = sum((dl.detach() * g).sum(1) for dl, g in zip(delta[:3], (GiT[:, :, :H], GiT[:, :, H:2 * H], GiT[:, :, 2 * H:]))) / d["wc"]
    return torch.stack([t.detach() for t in delta] + list(nu), 2), ct


GRU_MUTATIONS = ("sz_no_1m2z", "sr_no_1m2r", "sz_hp_for_htp", "sn_no_2n", "no_sq", "vh_no_sh", "swap_78", "drop_zt_term", "ht_init")


def gru_mutation_expressible(mut, case):
    """hp for htp and the loss of s_h need a second step: at t = 0 both h_{-1} and its tangent are 0, and v_h only feeds step t - 1."""
    return case[2] >= 2 or mut not in ("sz_hp_for_htp", "vh_no_sh")


def _chain(acc, x, Wm, seq):
    """acc + x @ Wm, x (B, K), Wm (K, N).  seq: the kernels' chain acc = fmaf(w, x_i, acc) for i = 0 .. K-1, one float32 rounding per
    step (the product of two float32 numbers is exact in float64)."""
    if not seq:
        return acc + x @ Wm
    a, xd, Wd = acc.double(), x.double(), Wm.double()
    for i in range(x.shape[1]):
        a = (a + xd[:, i:i + 1] * Wd[i][None]).float().double()
    return a.float()


def gru_gp_emulate(Gi, GiT, Whh, bhh, wc, dtype=torch.float32, seq=True, mut=None):
    """The algorithm of gru_gp_fwd_kernel / gru_gp_bwd_kernel on the host in `dtype`: the same formulas in the same order, the
    recurrent products as the kernels' sequential fma chains over i (seq), exp / tanh torch's.  mut: one of GRU_MUTATIONS."""
    B, V, H3 = Gi.shape
    H = H3 // 3
    Gi, GiT, Whh, bhh, wc = (t.to(dtype) for t in (Gi, GiT, Whh, bhh, wc))
    WT = Whh.T.contiguous()
    h = torch.zeros(B, H, dtype=dtype)
    ht = torch.full((B, H), 1e-3 if mut == "ht_init" else 0.0, dtype=dtype)
    tape = torch.zeros(B, V, 10, H, dtype=dtype)
    for t in range(V):
        gh = _chain(bhh[None].expand(B, 3 * H), h, WT, seq)
        ght = _chain(torch.zeros(B, 3 * H, dtype=dtype), ht, WT, seq)
        ar, az, q = gh[:, :H] + Gi[:, t, :H], gh[:, H:2 * H] + Gi[:, t, H:2 * H], gh[:, 2 * H:]
        art, azt, qt = ght[:, :H] + GiT[:, t, :H], ght[:, H:2 * H] + GiT[:, t, H:2 * H], ght[:, 2 * H:]
        r, z = 1 / (1 + torch.exp(-ar)), 1 / (1 + torch.exp(-az))
        n = torch.tanh(Gi[:, t, 2 * H:] + r * q)
        rt, zt = r * (1 - r) * art, z * (1 - z) * azt
        ant = GiT[:, t, 2 * H:] + rt * q + r * qt
        nt = (1 - n * n) * ant
        slots = [r, z, n, q, h, art, azt, qt, ant, ht]
        if mut == "swap_78":
            slots[7], slots[8] = slots[8], slots[7]
        tape[:, t] = torch.stack(slots, 1)
        hn = (1 - z) * n + z * h
        ht = ((1 - z) * nt + z * ht) if mut == "drop_zt_term" else (zt * (h - n) + (1 - z) * nt + z * ht)
        h = hn
    ct = ht
    G, N = wc.clone(), torch.zeros(B, H, dtype=dtype)
    dA = torch.zeros(B, V, 8, H, dtype=dtype)
    for t in range(V - 1, -1, -1):
        r, z, n, q, hp, art, azt, qt, ant, htp = tape[:, t].unbind(1)
        sr, sz, sn = r * (1 - r), z * (1 - z), 1 - n * n
        rt, zt, nt = sr * art, sz * azt, sn * ant
        d_n, d_z = G * (1 - z), G * (hp - n)
        d_an = d_n * sn
        d_r, d_q = d_an * q, d_an * r
        d_ar, d_az = d_r * sr, d_z * sz
        s_h = G * zt
        s_n = -G * zt - (0 if mut == "sn_no_2n" else 2 * n * d_n * ant)
        s_z = G * ((hp if mut == "sz_hp_for_htp" else htp) - nt) + (0 if mut == "sz_no_1m2z" else d_z * (1 - 2 * z) * azt)
        s_q = 0 if mut == "no_sq" else d_an * rt
        s_r = d_an * qt + (0 if mut == "sr_no_1m2r" else d_r * (1 - 2 * r) * art)
        v_n, v_z = N * (1 - z) + s_n, N * (hp - n) + s_z
        v_h = N * z + (0 if mut == "vh_no_sh" else s_h)
        v_an = v_n * sn
        v_r, v_q = v_an * q + s_r, v_an * r + s_q
        v_ar, v_az = v_r * sr, v_z * sz
        dA[:, t] = torch.stack([d_ar, d_az, d_an, d_q, v_ar, v_az, v_an, v_q], 1)
        G = _chain(G * z, torch.cat([d_ar, d_az, d_q], 1), Whh, seq)
        N = _chain(v_h, torch.cat([v_ar, v_az, v_q], 1), Whh, seq)
    return tape.double(), ct.double(), dA.double()


def gru_gp_errors(tape, ct, dA, grads, ref):
    """Every measure of a GRU case: the 10 tape slots and 8 dA blocks per step ((V,) each), ct per item, the two weight gradients per
    row, the bias gradients per gate block, the input gradient per (item, step)."""
    H = ref["tape"].shape[-1]
    errs = {}
    for k in range(10):
        errs[f"tape{k}"] = block_err(torch.as_tensor(tape)[:, :, k], ref["tape"][:, :, k], (0, 2))
    for k in range(8):
        errs[f"dA{k}"] = block_err(torch.as_tensor(dA)[:, :, k], ref["dA"][:, :, k], (0, 2))
    errs["ct"] = block_err(ct, ref["ct"], (1,))
    for k in ("weight_ih", "weight_hh"):
        errs[k] = block_err(grads[k], ref["grads"][k], (1,))
    for k in ("bias_ih", "bias_hh"):
        errs[k] = block_err(grads[k].reshape(3, H), ref["grads"][k].reshape(3, H), (1,))
    errs["x"] = block_err(grads["x"], ref["grads"]["x"], (2,))
    return errs


def gru_ref_zero(ref):
    H = ref["tape"].shape[-1]
    z = {f"tape{k}": ref["tape"][:, :, k].abs().amax((0, 2)) == 0 for k in range(10)}
    z.update({f"dA{k}": ref["dA"][:, :, k].abs().amax((0, 2)) == 0 for k in range(8)})
    z["ct"] = ref["ct"].abs().amax(1) == 0
    for k in ("weight_ih", "weight_hh"):
        z[k] = ref["grads"][k].abs().amax(1) == 0
    for k in ("bias_ih", "bias_hh"):
        z[k] = ref["grads"][k].reshape(3, H).abs().amax(1) == 0
    z["x"] = ref["grads"]["x"].abs().amax(2) == 0
    return z


_gru_cache = {}


def gru_gp_reference(B, V, H, recipe="plain", seed=None):
    """Data, the float64 reference on the rounded projections (tape, ct, dA, the five assembled gradients), the float32 emulation's
    errors and the bounds.  Computed once per case and shared."""
    key = (B, V, H, recipe, seed)
    if key not in _gru_cache:
        d = gru_gp_data(B, V, H, recipe, seed=seed)
        tape, ct, dA = gru_gp_probe_reference(d["Gi"], d["GiT"], d["Whh"], d["bhh"], d["wc"])
        ref = dict(d=d, tape=tape, ct=ct, dA=dA, grads=gru_gp_assemble(tape, dA, d["x"], d["xt"], d["Wih"]))
        et, ec, ea = gru_gp_emulate(d["Gi"], d["GiT"], d["Whh"], d["bhh"], d["wc"])
        ref["e_emul"] = gru_gp_errors(et, ec, ea, gru_gp_assemble(et, ea, d["x"], d["xt"], d["Wih"]), ref)
        ref["bounds"] = bounds_from(ref["e_emul"], gru_ref_zero(ref))
        _gru_cache[key] = ref
    return _gru_cache[key]


def emul_max(e_emul, keys=None):
    """Largest finite emulation error over the named measures."""
    return max(float(v.max()) for k, v in e_emul.items() if keys is None or k in keys)


def gru_old_measures_reject(tape, ct, dA, ref):
    """The older tests' verdict: L2 of each assembled gradient over the whole tensor at 2e-4, ct's whole-tensor maximum at 1e-4."""
    d = ref["d"]
    grads = gru_gp_assemble(tape, dA, d["x"], d["xt"], d["Wih"])
    for k in GRU_GRADS:
        if not float((grads[k] - ref["grads"][k]).norm() / (ref["grads"][k].norm() + 1e-30)) < 2e-4:
            return True
    return not R.rel_err(ct, ref["ct"]) < 1e-4


def gru_old_measures_blind_share(ref):
    """Share of the (dA block, step) pairs that the older measure cannot see: replacing the whole block at that step by zeros (a 100 %
    error there) moves no assembled gradient by 2e-4 in L2."""
    V = ref["dA"].shape[1]
    blind = 0
    for t in range(V):
        for k in range(8):
            dA = ref["dA"].clone()
            dA[:, t, k] = 0
            blind += not gru_old_measures_reject(ref["tape"], ref["ct"], dA, ref)
    return blind / (8 * V)


# ====================================================================================================================== attention
ATTN_SHORT = [(1, 1, 4, 1), (2, 2, 8, 2), (2, 63, 64, 1), (2, 64, 128, 2), (3, 10, 64, 8)]
ATTN_LONG_S = (1, 37, 64, 65, 127, 128)
ATTN_LONG_SHAPES = ((64, 1), (64, 2), (32, 8))
ATTN_SEED, ATTN_SITE = 1234567, 5
ATTN_PEAKED = 3.0


def attn_gp_cases():
    """(family, B, S, C, heads, p_drop, qk_scale).  Short kernels: every shape without and with dropout.  128-step kernels: every S
    with every (C, heads); dropout with (64, 2), so that every S appears with it once (18 cases keep the file inside its time).
    At S <= 64 the GPU test also runs the short kernels on the 128-step cases.  One peaked-softmax recipe: q and k scaled by 3 (the
    median of the rows' largest weight is 0.94).  With a scale of 8 the weights are one-hot to rounding, the penalty terms vanish to
    rounding with them and the float32 emulation is 100 % off in dq (even float64 formulas differ by 12 %); a scale of 4 still gives
    4.2e-3 in dv, above the cap of 2.5e-4; 3 gives 3.0e-5."""
    cases = [("short", B, S, C, h, p, 1.0) for B, S, C, h in ATTN_SHORT for p in (0.0, 0.3)]
    cases += [("long", 2, S, C, h, 0.3 if (C, h) == (64, 2) else 0.0, 1.0) for S in ATTN_LONG_S for C, h in ATTN_LONG_SHAPES]
    cases += [("short", 2, 64, 64, 2, 0.0, ATTN_PEAKED), ("long", 2, 64, 64, 2, 0.0, ATTN_PEAKED)]
    return cases


def attn_gp_case_id(case):
    fam, B, S, C, h, p, sc = case
    return f"{fam}-B{B}-S{S}-C{C}-h{h}-p{p}" + ("" if sc == 1.0 else f"-qk{sc:g}")


def attn_softmax(qkv, B, S, C, heads):
    d = C // heads
    q, k = (t.reshape(B, S, heads, d).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1)[:2])
    causal = torch.tril(torch.ones(S, S, dtype=torch.bool))
    return torch.softmax(((q @ k.transpose(-1, -2)) / math.sqrt(d)).masked_fill(~causal, float("-inf")), -1)


def attn_gp_data(B, S, C, heads, p_drop, qk_scale=1.0, mask_fn=R.dropout_mask_host):
    """qkv, qkvt, dO ~ N(0, 1) exact in float32 (seed S + C + heads, the older tests'); P = the float64 softmax rounded to float32 (the
    kernels read the saved weights); m = the dropout factors of element index bh S S + i S + j."""
    g = torch.Generator().manual_seed(S + C + heads)
    f = lambda *sh: f32_exact(torch.randn(*sh, generator=g))
    M = B * S
    qkv, qkvt, dO, lam = f(M, 3 * C), f(M, 3 * C), f(M, C), f(M, 3 * C)
    qkv[:, :2 * C] *= qk_scale
    mflat = mask_fn(B * heads * S * S, p_drop, ATTN_SEED, ATTN_SITE)
    return dict(B=B, S=S, C=C, heads=heads, p_drop=p_drop, qkv=qkv, qkvt=qkvt, dO=dO, lam=lam, mflat=mflat,
                m=mflat.reshape(B, heads, S, S), P=f32_exact(attn_softmax(qkv, B, S, C, heads)))


def attn_gp_reference(d):
    """jvp + grad on the definition: out_t (M, C) and what cpc_attn*_gp must add to dqkv (M, 3C)."""
    B, S, C, heads, m = d["B"], d["S"], d["C"], d["heads"], d["m"]
    dh = C // heads

    def f(qkv):
        v = qkv[:, 2 * C:].reshape(B, S, heads, dh).permute(0, 2, 1, 3)
        return ((attn_softmax(qkv, B, S, C, heads) * m) @ v).permute(0, 2, 1, 3).reshape(B * S, C)

    x = d["qkv"].clone().requires_grad_(True)
    _, out_t = torch.autograd.functional.jvp(f, x, d["qkvt"], create_graph=True)
    inc, = torch.autograd.grad((d["dO"] * out_t).sum(), x)
    return out_t.detach(), inc


ATTN_MUTATIONS = ("diag_out", "no_mask_e", "mask_dS", "pw_part", "k_from_t1", "no_scale_dSkt", "tri_mask")


def attn_mutation_expressible(mut, case):
    fam, B, S, C, h, p, sc = case
    """With one step the softmax is the constant 1: its tangent, dS and sig vanish, so the whole increment is exactly 0 and only a
    mistake in <P, u> (which would make pt non-zero) can show there."""
    if mut in ("no_mask_e", "mask_dS"):
        return p > 0 and S >= 2
    if mut == "tri_mask":
        return p > 0 and S > 64 and fam == "long"
    return S >= 2 or mut == "diag_out"


def attn_gp_closed(d, dtype=torch.float64, mut=None):
    """The closed formulas of csrc/attn.hip (the second implementation; in float32 the emulation), on the saved weights P.
    Returns out_t (M, C), inc (M, 3C).  mut: one of ATTN_MUTATIONS."""
    B, S, C, heads = d["B"], d["S"], d["C"], d["heads"]
    dh, M = C // heads, B * S
    hd = lambda t: t.to(dtype).reshape(B, S, heads, dh).permute(0, 2, 1, 3)
    un = lambda t: t.permute(0, 2, 1, 3).reshape(M, C)
    q, k, v = (hd(t) for t in d["qkv"].split(C, 1))
    qt, kt, vt = (hd(t) for t in d["qkvt"].split(C, 1))
    dO, P, m = hd(d["dO"]), d["P"].to(dtype), d["m"].to(dtype)
    causal = torch.tril(torch.ones(S, S, dtype=torch.bool))
    if mut == "tri_mask":
        i, j = torch.tril_indices(S, S)
        bh = torch.arange(B * heads)[:, None] * S * S
        mt = torch.ones(B * heads, S, S, dtype=dtype)
        mt[:, i, j] = d["mflat"].to(dtype)[bh + (i * (i + 1) // 2 + j)[None]]
        m = mt.reshape(B, heads, S, S)
    sc = 1.0 / math.sqrt(dh)
    u = ((qt @ k.transpose(-1, -2) + q @ kt.transpose(-1, -2)) * sc).masked_fill(~causal, 0.0)
    Pu = P * u
    if mut == "diag_out":
        Pu = Pu * ~torch.eye(S, dtype=torch.bool)
    mrow = Pu.sum(-1, keepdim=True)
    pt = P * (u - mrow)
    out_t = un((pt * m) @ v + (P * m) @ vt)
    a = (m * (dO @ v.transpose(-1, -2))).masked_fill(~causal, 0.0)
    cc = (P * a).sum(-1, keepdim=True)
    dS = P * (a - cc)
    if mut == "mask_dS":
        dS = dS * m
    e = dO @ vt.transpose(-1, -2)
    if mut != "no_mask_e":
        e = m * e
    w = (e + (a - cc) * (u - mrow)).masked_fill(~causal, 0.0)
    Pw = P * w
    if mut == "pw_part":
        Pw = Pw * (torch.arange(S) % 4 == 0)
    sig = P * (w - Pw.sum(-1, keepdim=True))
    sigk, dSk, ptk = sig, dS, pt * m
    if mut == "k_from_t1":
        low = torch.tril(torch.ones(S, S, dtype=torch.bool), -1)
        sigk, dSk, ptk = sig * low, dS * low, ptk * low
    dq = sc * (sig @ k) + (1.0 if mut == "no_scale_dSkt" else sc) * (dS @ kt)
    dk = sc * (sigk.transpose(-1, -2) @ q + dSk.transpose(-1, -2) @ qt)
    dv = ptk.transpose(-1, -2) @ dO
    return out_t.double(), torch.cat([un(dq), un(dk), un(dv)], 1).double()


ATTN_BLOCKS = ("out_t", "dq", "dk", "dv")


def attn_gp_errors(out_t, inc, ref):
    """Per time position and block (out_t; the q, k and v thirds of the increment): the maximum over items, heads and channels."""
    B, S, C = ref["d"]["B"], ref["d"]["S"], ref["d"]["C"]
    errs = {"out_t": block_err(torch.as_tensor(out_t).reshape(B, S, C), ref["out_t"].reshape(B, S, C), (0, 2))}
    inc = torch.as_tensor(inc).reshape(B, S, 3, C)
    for i, k in enumerate(ATTN_BLOCKS[1:]):
        errs[k] = block_err(inc[:, :, i], ref["inc"].reshape(B, S, 3, C)[:, :, i], (0, 2))
    return errs


_attn_cache = {}


def attn_gp_case_reference(case):
    """Data, reference, emulation errors and bounds of one case; the two families share them (same data at the same shape)."""
    key = case[1:]
    if key not in _attn_cache:
        _, B, S, C, h, p, scl = case
        d = attn_gp_data(B, S, C, h, p, scl)
        out_t, inc = attn_gp_reference(d)
        ref = dict(d=d, out_t=out_t, inc=inc)
        ref["e_emul"] = attn_gp_errors(*attn_gp_closed(d, torch.float32), ref)
        zero = {"out_t": out_t.reshape(B, S, C).abs().amax((0, 2)) == 0}
        zero.update({k: inc.reshape(B, S, 3, C)[:, :, i].abs().amax((0, 2)) == 0 for i, k in enumerate(ATTN_BLOCKS[1:])})
        ref["zero"] = zero
        ref["bounds"] = bounds_from(ref["e_emul"], zero)
        _attn_cache[key] = ref
    return _attn_cache[key]


def attn_old_measures_reject(out_t, inc, ref):
    return not (R.rel_err(out_t, ref["out_t"]) < 1e-5 and R.rel_err(inc, ref["inc"]) < 1e-4)


# ====================================================================================================================== LayerNorm
LN_SHAPES = [(1, 4), (5, 8), (37, 96), (24, 1024), (8197, 8)]
LN_SEED, LN_SITE = 424242, 3
LN_WIDE_CASE = (9, 1028, 0.3, "layer", 0, "plain")          # cpc_ln_tangent accepts C > 1024, cpc_ln_gp refuses it


def ln_gp_cases():
    """(M, C, p_drop, form, bcast, recipe).  Forms, as the engine calls the kernels (contexts.py: ln_t / ln_pair):
      layer        bt, rt_out, dr_b and g2 given (norm1 / norm2 inside a layer)
      layer_no_g2  the same with g2 = NULL and no broadcast
      final        bt = NULL, rt_out = NULL, dr_b = NULL, g2 = NULL (the encoder's final norm; no dropout there)
    bcast = 60 at M = 120: the final form (the mean over time folded in, gscale = 1/60) and the layer form with g2 (the only one where
    a gscale on g2 would show).  Every case runs cpc_ln_gp with 1, 5 and ceil(M / 4) + 3 blocks.  Large-mean rows at C = 64, 1024."""
    cases = []
    for M, C in LN_SHAPES:
        for p in (0.0, 0.3):
            cases += [(M, C, p, "layer", 0, "plain"), (M, C, p, "layer_no_g2", 0, "plain")]
        cases.append((M, C, 0.0, "final", 0, "plain"))
    for C in (8, 96):
        cases += [(120, C, 0.0, "final", 60, "plain"), (120, C, 0.3, "layer", 60, "plain")]
    cases += [(37, 64, 0.3, "layer", 0, "large_mean"), (37, 1024, 0.3, "layer", 0, "large_mean")]
    return cases


def ln_gp_case_id(case):
    M, C, p, form, bcast, rec = case
    return f"M{M}-C{C}-p{p}-{form}-bcast{bcast}" + ("" if rec == "plain" else "-" + rec)


def ln_nblocks(M):
    return (1, 5, (M + 3) // 4 + 3)


def ln_gp_data(M, C, p_drop, form="layer", bcast=0, recipe="plain", mask_fn=R.dropout_mask_host):
    """r (the primal LayerNorm input, as cpc_add_ln_fwd stored it), the tangents at, bt, the weight, delta's parts g1 (M / bcast rows
    when bcast) and g2, the accumulator's start lam: all exact in float32; stats = float64 (mean, rstd) of r rounded to float32."""
    g = torch.Generator().manual_seed(M + C + bcast)
    f = lambda *sh: f32_exact(torch.randn(*sh, generator=g))
    r = f(M, C) + (1000.0 if recipe == "large_mean" else 0.0)
    r = f32_exact(r)
    at, bt, lam, lam_b = f(M, C), f(M, C), f(M, C), f(M, C)
    w = f32_exact(1 + 0.3 * f(C))
    g1, g2 = f(M // bcast if bcast else M, C), f(M, C)
    final = form == "final"
    m = mask_fn(M * C, 0.0 if final else p_drop, LN_SEED, LN_SITE).reshape(M, C)
    mean = r.mean(1)
    rstd = 1.0 / torch.sqrt(r.var(1, unbiased=False) + R.LN_EPS)
    gscale = float(torch.tensor(1.0 / bcast if bcast else 1.0, dtype=torch.float32))
    return dict(M=M, C=C, p_drop=0.0 if final else p_drop, form=form, bcast=bcast, r=r, at=at, bt=None if final else bt, w=w, g1=g1,
                g2=g2 if form == "layer" else None, lam=lam, lam_b=lam_b, m=m, gscale=gscale, with_rt_out=not final, with_dr_b=not final,
                stats=f32_exact(torch.stack([mean, rstd], 1)))


def ln_dy(d, g2_scaled=False, mod=False):
    g1 = d["g1"]
    if d["bcast"]:
        idx = torch.arange(d["M"])
        g1 = g1[(idx % d["bcast"]) % g1.shape[0] if mod else idx // d["bcast"]]
    dy = g1 * d["gscale"]
    if d["g2"] is not None:
        dy = dy + d["g2"] * (d["gscale"] if g2_scaled else 1.0)
    return dy


def ln_gp_reference(d):
    """jvp + grad on y(a, b, w) = LayerNorm(a + m b) w at (a, b) = (r, 0): the function depends on (a, b) through a + m b alone, so r is
    the only primal input it needs.  Returns rt, yt, the input increment, the increment times the dropout factor (dr_b) and the sum
    over the rows of the weight gradient."""
    m, eps = d["m"], R.LN_EPS
    bt = torch.zeros_like(d["at"]) if d["bt"] is None else d["bt"]

    def f(a, b, w):
        x = a + m * b
        mu = x.mean(1, keepdim=True)
        return (x - mu) / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps) * w

    prim = tuple(t.clone().requires_grad_(True) for t in (d["r"], torch.zeros_like(d["r"]), d["w"]))
    _, yt = torch.autograd.functional.jvp(f, prim, (d["at"], bt, torch.zeros_like(d["w"])), create_graph=True)
    inc, inc_b, gw = torch.autograd.grad((ln_dy(d) * yt).sum(), prim)
    return dict(rt=d["at"] + m * bt, yt=yt.detach(), inc=inc, inc_b=inc_b, gw=gw)


LN_MUTATIONS = ("drop_ppr", "sum_for_mean", "drb_no_factor", "bcast_mod", "gscale_on_g2", "drop_last_partial")


def ln_mutation_expressible(mut, case):
    M, C, p, form, bcast, rec = case
    return {"drb_no_factor": p > 0 and form != "final", "bcast_mod": bcast > 0, "gscale_on_g2": bcast > 0 and form == "layer",
            "drop_last_partial": M % 4 != 0}.get(mut, True)


def _exact_sum(x):
    return x.sum(1)


def ln_gp_closed(d, dtype=np.float64, rowsum=_exact_sum, colsum=None, mut=None):
    """The closed formulas of ln_tangent_kernel / ln_gp_kernel on the float32 stats (the second implementation; with float32 arrays
    and one of context_reference.LN_F32_ORDERS as rowsum the emulation).  Returns rt, yt, inc, inc_b, gw and the per-row
    contributions to gw (M, C)."""
    A = lambda t: np.asarray(t.numpy(), dtype)
    M, C = d["M"], d["C"]
    r, at, w, m = A(d["r"]), A(d["at"]), A(d["w"]), A(d["m"])
    mean, rstd = A(d["stats"][:, 0])[:, None], A(d["stats"][:, 1])[:, None]
    rt = at if d["bt"] is None else at + A(d["bt"]) * m
    inv = dtype(1.0) / dtype(C)
    rs = lambda x: rowsum(np.ascontiguousarray(x, dtype))[:, None].astype(dtype)
    xh = (r - mean) * rstd
    m1, m2 = rs(rt) * (dtype(1.0) if mut == "sum_for_mean" else inv), rs(rt * xh) * inv
    yt = w * rstd * (rt - m1 - xh * m2)
    dy = A(ln_dy(d, g2_scaled=mut == "gscale_on_g2", mod=mut == "bcast_mod"))
    p = dy * w
    m_rt, b, m_p, a = m1, m2, rs(p) * inv, rs(p * xh) * inv
    ppr = rs(p * rt) * inv - m_p * m_rt - a * b
    pr, pp = rt - m_rt - xh * b, p - m_p - xh * a
    src = -rstd * rstd * ((0 if mut == "drop_ppr" else xh * ppr) + b * pp + a * pr)
    contrib = dy * rstd * pr
    used = contrib[:M - M % 4] if mut == "drop_last_partial" else contrib
    gw = (colsum or rowsum)(np.ascontiguousarray(used.T, dtype)).astype(dtype) if used.shape[0] else np.zeros(C, dtype)
    T = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    return dict(rt=T(rt), yt=T(yt), inc=T(src), inc_b=T(src if mut == "drb_no_factor" else src * m), gw=T(gw), contrib=T(contrib))


def _colsum_ok(name):
    """The lane-strided order adds groups of four columns and drops a remainder: usable for the row sums (C % 4 == 0 in every case),
    not for the sum over M rows; there the pairwise order stands in for it."""
    return "pairwise" if name == "lane-strided" else name


def ln_gp_emulate(d, order, mut=None):
    return ln_gp_closed(d, np.float32, R.LN_F32_ORDERS[order], R.LN_F32_ORDERS[_colsum_ok(order)], mut)


LN_BLOCKS = ("rt", "yt", "inc", "inc_b", "gw")


def ln_gp_errors(got, ref):
    """rt, yt and the two increments per row; the weight-gradient sum per channel relative to the column's largest contribution."""
    errs = {k: block_err(got[k], ref[k], (1,)) for k in ("rt", "yt", "inc", "inc_b")}
    gw = torch.as_tensor(got["gw"]).double().cpu()
    errs["gw"] = (gw - ref["gw"]).abs() / ref["contrib_max"]
    return errs


_ln_cache = {}


def ln_gp_case_reference(case):
    if case not in _ln_cache:
        d = ln_gp_data(*case)
        ref = ln_gp_reference(d)
        ref["d"] = d
        ref["contrib_max"] = ln_gp_closed(d)["contrib"].abs().amax(0).clamp_min(1e-300)
        per_order = {o: ln_gp_errors(ln_gp_emulate(d, o), ref) for o in R.LN_F32_ORDERS}
        ref["e_emul"] = {k: torch.stack([per_order[o][k] for o in per_order]).amax(0) for k in LN_BLOCKS}
        zero = {k: ref[k].abs().amax(1) == 0 for k in ("rt", "yt", "inc", "inc_b")}
        zero["gw"] = torch.zeros(d["C"], dtype=torch.bool)
        ref["zero"] = zero
        ref["bounds"] = bounds_from(ref["e_emul"], zero)
        _ln_cache[case] = ref
    return _ln_cache[case]


def ln_old_measures_reject(got, ref):
    return not (R.rel_err(got["rt"], ref["rt"]) < 1e-6 and R.rel_err(got["yt"], ref["yt"]) < 1e-5 and R.rel_err(got["inc"], ref["inc"]) < 1e-4
                and R.rel_err(got["inc_b"], ref["inc_b"]) < 1e-4 and R.rel_err(got["gw"], ref["gw"]) < 1e-4)


# ====================================================================================================================== accumulate
def _ulp(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def within_one_ulp(acc, lam, inc):
    """The accumulate contract acc = lam + inc (lam: the float32 start, inc: the float32 increment of the acc = 0 run): every element of
    acc within 1 float32 ulp of lam + inc evaluated in float64 and rounded to float32, plus half an ulp of inc.  The last term: the
    compiler may contract o += s * scale into one fma, which adds the UNROUNDED product s * scale to lam, while inc is that product
    rounded (half an ulp of inc away from it); where lam and inc cancel, an ulp of inc is many ulps of the sum, so without the term a
    kernel that is more exact than its own two-step evaluation would fail.  NaN fails."""
    exact = torch.as_tensor(lam).double().cpu() + torch.as_tensor(inc).double().cpu()
    got = torch.as_tensor(acc).double().cpu()
    return bool(((got - exact).abs() <= _ulp(exact) + 0.5 * _ulp(torch.as_tensor(inc).cpu())).all())
