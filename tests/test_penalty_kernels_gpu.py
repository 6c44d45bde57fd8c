"""The eight gradient-penalty entry points at their edges: cpc_gru_gp_fwd / cpc_gru_gp_bwd (csrc/gru.hip) and cpc_ln_tangent /
cpc_ln_gp / cpc_attn_tangent / cpc_attn_gp / cpc_attn128_tangent / cpc_attn128_gp (csrc/attn.hip), all f32, each against the float64
definition of the same operation (tests/penalty_reference.py: probe leaves on a joint primal / tangent GRU recurrence; jvp + grad on
the attention and LayerNorm definitions; test_penalty_reference_host.py checks those references against autograd's double backward
and shows that the measures used here reject a table of deliberate mistakes).  Device inputs are the reference's inputs, exact in
f32; every output buffer starts as NaN (an accumulator as 0 or lam) and is followed by sentinels.

Measures.  GRU: every one of the 10 tape slots and 8 dA blocks per time step, max_{b,j} |got - ref| / max_{b,j} |ref| within the step
(the penalty adjoint decays backwards through time: step 0 of dA is 1e-7 of the last step's at V = 40); ct per item; the assembled
weight gradients per row, the bias gradients per gate, the input gradient per (item, step).  Attention: out_t and the q, k, v thirds
of the increment per time position.  LayerNorm: rt, yt and the dr / dr_b increments per row, the slab sum per channel relative to
the column's largest contribution.  Increments come from a run with acc = 0, never from a subtraction.  A block whose reference is
exactly 0 (the tangent slots of h~_{-1} and W_hn h~_{-1} at t = 0, the q third at t = 0, the whole increment at S = 1) must be exactly 0.

Bounds.  bound of a block (a tape slot, a dA block, ct, an assembled gradient, out_t, a third of the increment, rt, yt, ...) =
max(4 x the largest error of the float32 host emulation of the kernel's algorithm against float64 in that block, 16 x 2^-24), the same
at every step / position / row of the block, while each step / position / row is measured relative to its own largest reference value
(penalty_reference.FLOOR counts the roundings; the floor only matters where the emulation happens to be exact).  The
emulation alone stays below a quarter of 10 x the older tests' tolerances (asserted on the host), so no bound exceeds 10 x those.
Largest emulation error per case (host, float32 against float64):

  GRU (B,V,H)      tape     dA       ct       gradients          (sequential fma chains over i, as the kernels)
    plain     (1,1,16) 6.2e-8 1.5e-7 5.6e-8 4.4e-7   (1,2,16) 1.2e-7 9.1e-7 1.0e-7 8.5e-7   (3,13,48) 4.7e-7 1.9e-6 1.7e-7 1.8e-6
              (2,13,64) 4.3e-7 5.1e-6 2.7e-7 2.2e-6  (2,5,80) 4.4e-7 1.5e-6 2.2e-7 1.8e-6   (2,3,512) 1.1e-6 2.5e-6 5.0e-7 1.3e-5
              (2,3,384) 7.6e-7 2.2e-6 2.1e-7 4.7e-6  (2,40,64) 4.4e-7 5.1e-6 2.0e-7 5.6e-6
    W_hh = 0  (1,2,16) 8.3e-8 2.1e-7 1.0e-7 8.2e-7   (3,13,48) 1.9e-7 7.2e-7 1.7e-7 9.5e-7  (2,3,512) 1.1e-7 2.3e-7 1.1e-7 1.1e-6
              (2,40,64) 2.0e-7 1.1e-6 1.5e-7 4.8e-7
    saturated (3,13,48) 3.4e-7 3.0e-6 3.5e-7 1.5e-4  (2,13,64) 4.9e-7 3.4e-6 2.6e-7 3.0e-4
              (2,40,64) 4.6e-7 2.8e-5 2.3e-7 5.6e-5  (data seed 1: with seed B 1000 + H + V one row of the weight_ih gradient reaches
              6.9e-4, above the cap of 5e-4; the saturated recipe is not run where a gradient row sums fewer than 26 terms, see
              penalty_reference.gru_gp_cases)
  attention (B,S,C,heads) p: out_t / increment        (plain float32, torch's summation order)
    short  (1,1,4,1) 0: 0 / 0  .3: 1.3e-8 / 0    (2,2,8,2) 0: 1.6e-7 / 5.1e-7  .3: 1.0e-7 / 4.6e-7
           (2,63,64,1) 0: 3.8e-7 / 4.7e-7  .3: 4.2e-7 / 1.8e-6    (2,64,128,2) 0: 4.3e-7 / 5.5e-7  .3: 4.0e-7 / 6.3e-7
           (3,10,64,8) 0: 2.5e-7 / 2.9e-7  .3: 2.2e-7 / 3.5e-7
    long, B = 2, (C,heads) = (64,1) p 0 | (64,2) p .3 | (32,8) p 0:
           S=1   0 / 0 | 4.7e-8 / 0 | 0 / 0                      S=37  2.7e-7 / 4.9e-7 | 2.7e-7 / 5.7e-7 | 3.5e-7 / 4.1e-7
           S=64  3.3e-7 / 6.6e-7 | 2.9e-7 / 4.5e-7 | 3.9e-7 / 6.8e-7    S=65  4.0e-7 / 5.3e-7 | 2.9e-7 / 5.0e-7 | 3.3e-7 / 5.2e-7
           S=127 4.3e-7 / 7.8e-7 | 4.2e-7 / 8.3e-7 | 4.8e-7 / 7.8e-7    S=128 5.4e-7 / 8.5e-7 | 5.1e-7 / 6.6e-7 | 5.9e-7 / 1.0e-6
    peaked (2,64,64,2), q and k scaled by 3: 5.9e-7 / 3.0e-5   (a scale of 8 makes the weights one-hot to rounding and the emulation
           100 % off; 4 gives 4.2e-3, above the cap of 2.5e-4: penalty_reference.attn_gp_cases)
  LayerNorm (M,C): largest of yt / dr, dr_b / slab sum over the forms and p   (three summation orders; rt stays below 1.4e-7)
    (1,4) 4.4e-8 / 2.2e-7 / 4.1e-6      (5,8) 2.7e-7 / 3.6e-7 / 3.3e-7      (37,96) 1.8e-7 / 1.5e-6 / 9.4e-7
    (24,1024) 1.7e-7 / 3.7e-6 / 1.2e-6  (8197,8) 8.7e-7 / 3.6e-6 / 3.6e-5   (120,8) bcast 60: 3.3e-7 / 7.0e-7 / 1.1e-6
    (120,96) bcast 60: 1.9e-7 / 8.2e-7 / 3.3e-6    large mean (37,64) 5.5e-6 / 1.0e-4 / 2.1e-5    (37,1024) 1.6e-6 / 5.1e-5 / 6.9e-6
(test_penalty_reference_host.py prints every figure.)  No tolerance here was obtained by running a kernel.

The older tests of these kernels (test_hip_kernels.py::test_gru_gradient_penalty_kernels, ::test_attention_gradient_penalty_kernels,
::test_layernorm_gradient_penalty_kernels, test_gru_wide_gpu.py, test_attention_long_gpu.py) stay as they are; their H = 384 / 512
and S = 65 / 128 shapes are also cases here, under the finer measures.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
import penalty_reference as G  # noqa: E402
from test_attention_long_gpu import guard_intact, guarded  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
P = _hip.ptr


def dev(t):
    """A float64 host tensor that is exact in f32 -> device f32."""
    return t.float().contiguous().to(DEV)


def host(t):
    return t.detach().cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def filled(values):
    """A guarded device buffer that starts with `values` (an accumulator)."""
    buf, view = guarded(values.numel(), F32, fill=0.0)
    view.copy_(values.reshape(-1).float().to(DEV))
    return buf, view


def report(label, errs, bounds):
    print(f"{label}: largest error / bound {G.worst_ratio(errs, bounds):.2f}")
    bad = G.violations(errs, bounds)
    assert not bad, (label, bad[:8])


# ======================================================================================================================= GRU
def _gru_device(d, GiT=None, perm=None):
    """cpc_gru_gp_fwd, cpc_gru_gp_bwd on the reference's inputs -> tape (B, V, 10, H), ct (B, H), dA (B, V, 8, H) as f32 host tensors."""
    B, V, H = d["B"], d["V"], d["H"]
    Gi, GiT, wc = d["Gi"], d["GiT"] if GiT is None else GiT, d["wc"]
    if perm is not None:
        Gi, GiT, wc = Gi[perm], GiT[perm], wc[perm]
    dGi, dGiT, dwc = dev(Gi), dev(GiT), dev(wc)
    WT, W, bhh = dev(d["Whh"].T), dev(d["Whh"]), dev(d["bhh"])
    tb, tape = guarded(B * V * 10 * H, F32)
    cb, ct = guarded(B * H, F32)
    _hip.call("cpc_gru_gp_fwd", P(dGi), P(dGiT), P(WT), P(bhh), P(tape), P(ct), B, V, H)
    torch.cuda.synchronize()
    assert guard_intact(tb, B * V * 10 * H) and guard_intact(cb, B * H)
    ab, dA = guarded(B * V * 8 * H, F32)
    _hip.call("cpc_gru_gp_bwd", P(dwc), P(tape), P(W), P(dA), B, V, H)
    torch.cuda.synchronize()
    assert guard_intact(ab, B * V * 8 * H) and guard_intact(tb, B * V * 10 * H)
    return host(tape).view(B, V, 10, H), host(ct).view(B, H), host(dA).view(B, V, 8, H)


@pytest.mark.parametrize("case", G.gru_gp_cases(), ids=G.gru_gp_case_id)
def test_gru_penalty_per_step(case):
    """Every tape slot and dA block at every step, ct per item and the five gradients assembled as GRUContext.gp_grads assembles them,
    at one and two steps, below one wave, one full wave, a partial last wave, full width and over 40 steps (where the early steps are
    1e-7 of the last); plain data, W_hh = 0 and saturated gates."""
    _, B, V, H, rec = case
    ref = G.gru_gp_reference(B, V, H, rec, G.gru_gp_case_seed(case))
    d = ref["d"]
    tape, ct, dA = _gru_device(d)
    grads = G.gru_gp_assemble(tape, dA, d["x"], d["xt"], d["Wih"])
    report("GRU " + G.gru_gp_case_id(case), G.gru_gp_errors(tape, ct, dA, grads, ref), ref["bounds"])
    assert bool((tape[:, 0, 4] == 0).all()) and bool((tape[:, 0, 7] == 0).all()) and bool((tape[:, 0, 9] == 0).all())


@pytest.mark.parametrize("B,V,H", [(1, 2, 16), (2, 5, 80), (2, 3, 512)])
def test_gru_penalty_is_linear_in_the_tangent_input(B, V, H):
    """GiT = 0: tape slots 5 .. 9, ct and the second-order half of dA are exactly 0 and the delta half is bit-identical to the run with
    a random GiT.  2 GiT: slots 5 .. 9, ct and the second-order half are exactly doubled (scaling by 2 is exact in f32; plain data
    stays far from overflow and underflow), slots 0 .. 4 and the delta half are bit-identical."""
    d = G.gru_gp_reference(B, V, H)["d"]
    tape, ct, dA = _gru_device(d)
    tape0, ct0, dA0 = _gru_device(d, GiT=torch.zeros_like(d["GiT"]))
    assert bool((tape0[:, :, 5:] == 0).all()) and bool((ct0 == 0).all()) and bool((dA0[:, :, 4:] == 0).all())
    assert same_bits(tape0[:, :, :5], tape[:, :, :5]) and same_bits(dA0[:, :, :4], dA[:, :, :4])
    tape2, ct2, dA2 = _gru_device(d, GiT=2 * d["GiT"])
    assert same_bits(tape2[:, :, :5], tape[:, :, :5]) and same_bits(dA2[:, :, :4], dA[:, :, :4])
    assert same_bits(tape2[:, :, 5:], 2 * tape[:, :, 5:]) and same_bits(ct2, 2 * ct) and same_bits(dA2[:, :, 4:], 2 * dA[:, :, 4:])
    assert bool(torch.isfinite(dA).all()) and bool((dA[:, :, 4:] != 0).any())


def test_gru_penalty_items_are_independent():
    """Permuting the batch items permutes every output bit for bit."""
    d = G.gru_gp_reference(3, 13, 48)["d"]
    perm = torch.tensor([2, 0, 1])
    tape, ct, dA = _gru_device(d)
    tape_p, ct_p, dA_p = _gru_device(d, perm=perm)
    assert same_bits(tape_p, tape[perm]) and same_bits(ct_p, ct[perm]) and same_bits(dA_p, dA[perm])


def test_gru_penalty_refusals_write_nothing():
    """H = 0 and 513, B = 0, V = 0: -22 and the outputs stay as they were (valid device pointers throughout)."""
    lib, s = _hip.lib(), _hip.stream_ptr()
    src = torch.zeros(2 * 4 * 3 * 512, device=DEV)
    w = torch.zeros(3 * 512 * 512, device=DEV)
    out = [torch.randn(2 * 4 * 10 * 512, device=DEV) for _ in range(3)]
    keep = [o.clone() for o in out]
    for B, V, H in ((2, 4, 0), (2, 4, 513), (0, 4, 64), (2, 0, 64)):
        assert lib.cpc_gru_gp_fwd(P(src), P(src), P(w), P(src), P(out[0]), P(out[1]), B, V, H, s) == -22, (B, V, H)
        assert lib.cpc_gru_gp_bwd(P(src), P(src), P(w), P(out[2]), B, V, H, s) == -22, (B, V, H)
    torch.cuda.synchronize()
    assert all(same_bits(host(o), host(k)) for o, k in zip(out, keep))


# ======================================================================================================================= attention
def _abi(fam):
    return "cpc_attn" if fam == "short" else "cpc_attn128"


def _attn_device(fam, d, qkvt=None, lam=None, perm=None):
    """<abi>_tangent and <abi>_gp (acc starting at 0, or at lam) -> out_t (M, C), acc (M, 3C) as f32 host tensors."""
    B, S, C, heads, p = d["B"], d["S"], d["C"], d["heads"], d["p_drop"]
    M = B * S
    qkv, qkvt, dO, Pw = d["qkv"], d["qkvt"] if qkvt is None else qkvt, d["dO"], d["P"]
    if perm is not None:
        rows = lambda t: t.reshape(B, S, -1)[perm].reshape(M, -1)
        qkv, qkvt, dO, Pw = rows(qkv), rows(qkvt), rows(dO), Pw[perm]
    dq, dqt, ddO, dP = dev(qkv), dev(qkvt), dev(dO), dev(Pw)
    ob, o = guarded(M * C, F32)
    _hip.call(_abi(fam) + "_tangent", P(dq), P(dqt), P(dP), P(o), B, S, C, heads, p, G.ATTN_SEED, G.ATTN_SITE)
    torch.cuda.synchronize()
    assert guard_intact(ob, M * C)
    ab, acc = filled(torch.zeros(M * 3 * C) if lam is None else lam)
    _hip.call(_abi(fam) + "_gp", P(dq), P(dqt), P(dP), P(ddO), P(acc), B, S, C, heads, p, G.ATTN_SEED, G.ATTN_SITE)
    torch.cuda.synchronize()
    assert guard_intact(ab, M * 3 * C)
    return host(o).view(M, C), host(acc).view(M, 3 * C)


def _device_mask_is_host_mask(d):
    n = d["mflat"].numel()
    if d["p_drop"]:
        mb, m = guarded(n, F32)
        _hip.call("cpc_dropout_mask", P(m), n, d["p_drop"], G.ATTN_SEED, G.ATTN_SITE)
        torch.cuda.synchronize()
        assert guard_intact(mb, n) and torch.equal(host(m).double(), d["mflat"])


@pytest.mark.parametrize("case", G.attn_gp_cases(), ids=G.attn_gp_case_id)
def test_attention_penalty_per_position(case):
    """out_t and the q, k, v thirds of the increment per time position against jvp + grad on the definition; the row-0 identities;
    the accumulate contract; and, for the 128-step cases with S <= 64, the short kernels on the same data: each within the bound of
    the reference, and the two families within the bound of each other (different summation order, so not bitwise)."""
    fam, B, S, C, heads, p, _ = case
    ref = G.attn_gp_case_reference(case)
    d = ref["d"]
    _device_mask_is_host_mask(d)
    results = {}
    for f in [fam] + (["short"] if fam == "long" and S <= 64 else []):
        out_t, inc = _attn_device(f, d)
        results[f] = (out_t, inc)
        report(f"attention {G.attn_gp_case_id(case)} [{f}]", G.attn_gp_errors(out_t, inc, ref), ref["bounds"])
        # row 0: one key, weight 1: out_t[b, 0] = m_00 vt[b, 0] (one f32 product), and q gains exactly nothing
        m00 = d["m"][:, :, 0, 0].float()[:, :, None].expand(B, heads, C // heads).reshape(B, C)
        assert torch.equal(out_t.view(B, S, C)[:, 0], m00 * d["qkvt"].view(B, S, 3 * C)[:, 0, 2 * C:].float()), f
        assert bool((inc.view(B, S, 3 * C)[:, 0, :C] == 0).all()), f
        _, acc = _attn_device(f, d, lam=d["lam"])
        assert G.within_one_ulp(acc, d["lam"], inc), f
    if len(results) == 2:
        (o_l, i_l), (o_s, i_s) = results["long"], results["short"]
        errs = {"out_t": (o_s.double() - o_l.double()).view(B, S, C).abs().amax((0, 2)) / ref["out_t"].view(B, S, C).abs().amax((0, 2)).clamp_min(1e-300)}
        di, ri = (i_s.double() - i_l.double()).view(B, S, 3, C), ref["inc"].view(B, S, 3, C)
        for i, k in enumerate(G.ATTN_BLOCKS[1:]):
            errs[k] = di[:, :, i].abs().amax((0, 2)) / ri[:, :, i].abs().amax((0, 2)).clamp_min(1e-300)
        report(f"attention {G.attn_gp_case_id(case)} [short against long]", errs, ref["bounds"])


@pytest.mark.parametrize("fam,B,S,C,heads,p", [("short", 3, 10, 64, 8, 0.3), ("short", 2, 64, 128, 2, 0.0), ("long", 2, 65, 64, 2, 0.3),
                                               ("long", 2, 37, 32, 8, 0.0)])
def test_attention_penalty_is_linear_in_the_tangent_input(fam, B, S, C, heads, p):
    """qkvt = 0: out_t is exactly 0 and the accumulator stays bit-identical to lam.  2 qkvt: out_t and the increment (acc from 0) are
    exactly doubled."""
    d = G.attn_gp_case_reference((fam, B, S, C, heads, p, 1.0))["d"]
    out_t, inc = _attn_device(fam, d)
    out0, acc0 = _attn_device(fam, d, qkvt=torch.zeros_like(d["qkvt"]), lam=d["lam"])
    assert bool((out0 == 0).all()) and same_bits(acc0, d["lam"].float())
    out2, inc2 = _attn_device(fam, d, qkvt=2 * d["qkvt"])
    assert same_bits(out2, 2 * out_t) and same_bits(inc2, 2 * inc)


@pytest.mark.parametrize("fam,S", [("short", 10), ("long", 65)])
def test_attention_penalty_items_are_independent(fam, S):
    """Without dropout (its factors depend on the item's index) permuting the items permutes out_t and the increment bit for bit."""
    B, C, heads = 3, 64, 8
    d = G.attn_gp_data(B, S, C, heads, 0.0)
    perm = torch.tensor([1, 2, 0])
    out_t, inc = _attn_device(fam, d)
    out_p, inc_p = _attn_device(fam, d, perm=perm)
    assert same_bits(out_p.view(B, S, C), out_t.view(B, S, C)[perm]) and same_bits(inc_p.view(B, S, 3 * C), inc.view(B, S, 3 * C)[perm])


def test_attention_penalty_refusals_write_nothing():
    """S = 0, S above the family's limit, a head size that is no multiple of 4 or above 64, drop_p < 0 or >= 1: -22 and nothing
    written (valid device pointers, large enough for any of the refused shapes)."""
    src = torch.zeros(2 * 129 * 3 * 136, device=DEV)
    out = [torch.randn(2 * 129 * 3 * 136, device=DEV) for _ in range(2)]
    keep = [o.clone() for o in out]
    for fam, limit in (("short", 64), ("long", 128)):
        bad = [(2, 0, 64, 2, 0.0), (2, limit + 1, 64, 2, 0.0), (2, 129, 64, 2, 0.0), (2, 8, 12, 2, 0.0), (2, 8, 68, 1, 0.0), (2, 8, 136, 2, 0.0),
               (0, 8, 64, 2, 0.0), (2, 8, 64, 2, -0.1), (2, 8, 64, 2, 1.0), (2, 8, 64, 2, 1.5)]
        for B, S, C, heads, p in bad:
            with pytest.raises(_hip.HipCallError, match="-22"):
                _hip.call(_abi(fam) + "_tangent", P(src), P(src), P(src), P(out[0]), B, S, C, heads, p, 0, 0)
            with pytest.raises(_hip.HipCallError, match="-22"):
                _hip.call(_abi(fam) + "_gp", P(src), P(src), P(src), P(src), P(out[1]), B, S, C, heads, p, 0, 0)
    torch.cuda.synchronize()
    assert all(same_bits(host(o), host(k)) for o, k in zip(out, keep))


# ======================================================================================================================= LayerNorm
def _ln_tangent_device(d, at=None, bt=None):
    M, C = d["M"], d["C"]
    at = d["at"] if at is None else at
    bt = d["bt"] if bt is None else bt
    dat, dbt = dev(at), (None if d["bt"] is None else dev(bt))
    rb, rt_out = guarded(M * C, F32) if d["with_rt_out"] else (None, None)
    yb, yt = guarded(M * C, F32)
    dr_, dst, dw = dev(d["r"]), dev(d["stats"]), dev(d["w"])          # (named: a temporary's memory would be reused by the next one)
    _hip.call("cpc_ln_tangent", P(dat), P(dbt), P(dr_), P(dst), P(dw), P(rt_out), P(yt), M, C, d["p_drop"], G.LN_SEED, G.LN_SITE)
    torch.cuda.synchronize()
    assert guard_intact(yb, M * C) and (rb is None or guard_intact(rb, M * C))
    return (rt_out if d["with_rt_out"] else dat), yt


def _ln_gp_device(d, rt, nb, lam=None, lam_b=None):
    """cpc_ln_gp with nb blocks; dr (and dr_b) start at 0 or at lam (lam_b).  rt: the device tensor the tangent pass left."""
    M, C = d["M"], d["C"]
    zero = torch.zeros(M * C)
    ab, acc = filled(zero if lam is None else lam)
    bb, acc_b = filled(zero if lam_b is None else lam_b) if d["with_dr_b"] else (None, None)
    sb, slabs = guarded(nb * C, F32)
    g1, g2 = dev(d["g1"]), (None if d["g2"] is None else dev(d["g2"]))
    dr_, dst, dw = dev(d["r"]), dev(d["stats"]), dev(d["w"])
    _hip.call("cpc_ln_gp", P(g1), P(g2), P(rt), P(dr_), P(dst), P(dw), P(acc), P(acc_b), P(slabs), M, C, d["bcast"], d["gscale"], nb,
              d["p_drop"], G.LN_SEED, G.LN_SITE)
    torch.cuda.synchronize()
    assert guard_intact(ab, M * C) and guard_intact(sb, nb * C) and (bb is None or guard_intact(bb, M * C))
    return host(acc).view(M, C), (None if acc_b is None else host(acc_b).view(M, C)), host(slabs).view(nb, C)


@pytest.mark.parametrize("case", G.ln_gp_cases(), ids=G.ln_gp_case_id)
def test_layernorm_penalty_per_row(case):
    """rt, yt, the dr and dr_b increments per row and the slab sum per channel against jvp + grad on LayerNorm(a + dropout(b)), with
    the operands given or NULL as the engine passes them, with 1, 5 and ceil(M / 4) + 3 blocks: the increments do not depend on the
    block count bit for bit, surplus blocks write zero slabs into NaN-filled memory; then the accumulate contract."""
    M, C = case[:2]
    ref = G.ln_gp_case_reference(case)
    d = ref["d"]
    if d["p_drop"]:
        mb, m = guarded(M * C, F32)
        _hip.call("cpc_dropout_mask", P(m), M * C, d["p_drop"], G.LN_SEED, G.LN_SITE)
        torch.cuda.synchronize()
        assert torch.equal(host(m).double().view(M, C), d["m"])
    rt, yt = _ln_tangent_device(d)
    first = None
    for nb in G.ln_nblocks(M):
        inc, inc_b, slabs = _ln_gp_device(d, rt, nb)
        got = dict(rt=host(rt).view(M, C), yt=host(yt).view(M, C), inc=inc, inc_b=ref["inc_b"] if inc_b is None else inc_b,
                   gw=slabs.double().sum(0))
        bounds = {k: v for k, v in ref["bounds"].items() if (k != "rt" or d["with_rt_out"]) and (k != "inc_b" or d["with_dr_b"])}
        report(f"LayerNorm {G.ln_gp_case_id(case)} nblocks={nb}", G.ln_gp_errors(got, ref), bounds)
        assert bool((slabs[(M + 3) // 4:] == 0).all()), nb
        if inc_b is not None:
            assert bool(((inc_b == 0) | (d["m"] != 0)).all()), nb
        if first is None:
            first = (inc, inc_b)
        else:
            assert same_bits(inc, first[0]) and (inc_b is None or same_bits(inc_b, first[1])), nb
    acc, acc_b, _ = _ln_gp_device(d, rt, 5, lam=d["lam"], lam_b=d["lam_b"])
    assert G.within_one_ulp(acc, d["lam"], first[0]) and (acc_b is None or G.within_one_ulp(acc_b, d["lam_b"], first[1]))


@pytest.mark.parametrize("case", [(37, 96, 0.3, "layer", 0, "plain"), (5, 8, 0.0, "final", 0, "plain"), (24, 1024, 0.3, "layer_no_g2", 0, "plain")],
                         ids=G.ln_gp_case_id)
def test_layernorm_penalty_is_linear_in_the_tangent_input(case):
    """at = bt = 0: rt_out and yt are exactly 0 and cpc_ln_gp leaves dr and dr_b bit-identical to lam with zero slabs.  2 at, 2 bt: rt_out,
    yt and the increments are exactly doubled."""
    M, C = case[:2]
    d = G.ln_gp_case_reference(case)["d"]
    rt, yt = _ln_tangent_device(d)
    inc, inc_b, slabs = _ln_gp_device(d, rt, 5)
    rt0, yt0 = _ln_tangent_device(d, at=torch.zeros(M, C), bt=torch.zeros(M, C))
    assert bool((host(yt0) == 0).all()) and bool((host(rt0) == 0).all())
    acc, acc_b, slabs0 = _ln_gp_device(d, rt0, 5, lam=d["lam"], lam_b=d["lam_b"])
    assert same_bits(acc, d["lam"].float()) and (acc_b is None or same_bits(acc_b, d["lam_b"].float())) and bool((slabs0 == 0).all())
    rt2, yt2 = _ln_tangent_device(d, at=2 * d["at"], bt=None if d["bt"] is None else 2 * d["bt"])
    assert same_bits(host(yt2), 2 * host(yt)) and same_bits(host(rt2), 2 * host(rt))
    inc2, inc_b2, slabs2 = _ln_gp_device(d, rt2, 5)
    assert same_bits(inc2, 2 * inc) and (inc_b is None or same_bits(inc_b2, 2 * inc_b)) and same_bits(slabs2, 2 * slabs)


def test_layernorm_wide_rows_tangent_only():
    """C = 1028: cpc_ln_tangent accepts it (rt and yt per row within the emulation's bounds); cpc_ln_gp returns -22 and leaves dr, dr_b
    and the slabs bit for bit untouched."""
    case = G.LN_WIDE_CASE
    M, C = case[:2]
    ref = G.ln_gp_case_reference(case)
    d = ref["d"]
    rt, yt = _ln_tangent_device(d)
    got = dict(rt=host(rt).view(M, C), yt=host(yt).view(M, C), inc=ref["inc"], inc_b=ref["inc_b"], gw=ref["gw"])
    report("LayerNorm C=1028 tangent", G.ln_gp_errors(got, ref), {k: ref["bounds"][k] for k in ("rt", "yt")})
    nb = 3
    out = [torch.randn(M * C, device=DEV), torch.randn(M * C, device=DEV), torch.randn(nb * C, device=DEV)]
    keep = [o.clone() for o in out]
    g1, g2, dr_, dst, dw = dev(d["g1"]), dev(d["g2"]), dev(d["r"]), dev(d["stats"]), dev(d["w"])
    rc = _hip.lib().cpc_ln_gp(P(g1), P(g2), P(rt), P(dr_), P(dst), P(dw), P(out[0]), P(out[1]), P(out[2]), M, C, 0, 1.0, nb, d["p_drop"],
                              G.LN_SEED, G.LN_SITE, _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -22 and all(same_bits(host(o), host(k)) for o, k in zip(out, keep))


def test_layernorm_penalty_refusals_write_nothing():
    """M = 0, C = 0, nblocks = 0, drop_p < 0 or >= 1: -22 and nothing written."""
    src = torch.zeros(8 * 64, device=DEV)
    out = [torch.randn(8 * 64, device=DEV) for _ in range(5)]
    keep = [o.clone() for o in out]
    for M, C, nb, p in ((0, 64, 2, 0.0), (8, 0, 2, 0.0), (8, 64, 0, 0.0), (8, 64, 2, -0.1), (8, 64, 2, 1.0)):
        if nb:
            with pytest.raises(_hip.HipCallError, match="-22"):
                _hip.call("cpc_ln_tangent", P(src), P(src), P(src), P(src), P(src), P(out[0]), P(out[1]), M, C, p, 0, 0)
        with pytest.raises(_hip.HipCallError, match="-22"):
            _hip.call("cpc_ln_gp", P(src), P(src), P(src), P(src), P(src), P(src), P(out[2]), P(out[3]), P(out[4]), M, C, 0, 1.0, nb, p, 0, 0)
    torch.cuda.synchronize()
    assert all(same_bits(host(o), host(k)) for o, k in zip(out, keep))
