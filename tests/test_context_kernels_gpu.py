"""The context-network kernels at their edges: the GRU recurrences (csrc/gru.hip: weight-resident bf16, 4-wave and 8-wave streaming),
the short-sequence attention core, residual + LayerNorm, positional scale, mean over time and dropout (csrc/attn.hip), each against a
plain float64 reference of the same operation (tests/context_reference.py; test_context_reference_host.py checks those references
against torch's own modules and shows that the metrics used here reject deliberate mistakes).  Device inputs are the reference's
inputs rounded to the storage type; every output buffer starts as NaN and is followed by sentinel elements.

GRU: errors are measured per time step, max_{b,j} |got - ref| / max_{b,j} |ref| within step t, for the hidden states and for each of
the four blocks of dG = [dr | du | dn | dn r]: the gradient decays backwards through time, so a whole-tensor maximum hides the early
steps.  f32: 2e-5 (hidden states) and 5e-5 (gradients) at every step.  bf16: the device must be within 4 e_model(t), e_model being the
per-step error against float64 of a float64 emulation that rounds to bf16 exactly where the kernels store bf16 (the h tile that feeds
the MFMAs, the five tape values, the dgh tile, the stored Hall and dG); the factor 4 covers the f32 summation order of the MFMAs and
the device's exp / rcp.  The emulation alone stays below 2e-2 at every step of every case (checked on the host), so no bound
exceeds 8e-2.  max_t e_model(t), the largest of the five quantities, for every bf16 case as (B,V) value (cases with V <= 2 start from
a carried state h0; data seed B 1000 + H + V):

    resident  H=32   (1,1) 7.0e-3  (1,2) 7.6e-3  (1,13) 1.6e-2  (16,1) 3.8e-3  (16,2) 5.2e-3  (16,13) 1.1e-2
                     (17,1) 5.1e-3  (17,2) 7.9e-3  (17,13) 1.1e-2  (33,1) 4.4e-3  (33,2) 8.6e-3  (33,13) 1.5e-2
    resident  H=64   (1,1) 8.1e-3  (1,2) 6.8e-3  (1,13) 1.6e-2  (16,1) 3.4e-3  (16,2) 6.5e-3  (16,13) 1.0e-2
                     (17,1) 3.6e-3  (17,2) 7.7e-3  (17,13) 1.1e-2  (33,1) 3.6e-3  (33,2) 5.9e-3  (33,13) 1.4e-2
    resident  H=128  (1,1) 5.6e-3  (1,2) 1.7e-2  (1,13) 1.5e-2  (16,1) 4.4e-3  (16,2) 8.7e-3  (16,13) 9.4e-3
                     (17,1) 4.5e-3  (17,2) 4.3e-3  (17,13) 1.3e-2  (33,1) 4.8e-3  (33,2) 6.2e-3  (33,13) 1.2e-2
    resident  H=256  (1,1) 5.0e-3  (1,2) 5.7e-3  (1,13) 9.8e-3  (16,1) 7.3e-3  (16,2) 6.6e-3  (16,13) 1.6e-2
                     (17,1) 5.4e-3  (17,2) 8.0e-3  (17,13) 1.5e-2  (33,1) 4.0e-3  (33,2) 8.8e-3  (33,13) 9.8e-3
    streaming H=96   (1,1) 4.3e-3  (1,13) 1.2e-2  (17,1) 6.0e-3  (17,13) 1.2e-2
    streaming H=160  (1,1) 5.4e-3  (1,13) 1.6e-2  (17,1) 5.3e-3  (17,13) 1.3e-2
    streaming H=192  (1,1) 5.7e-3  (1,13) 9.6e-3  (17,1) 4.6e-3  (17,13) 1.3e-2
    streaming H=224  (1,1) 7.2e-3  (1,13) 1.9e-2  (17,1) 5.1e-3  (17,13) 1.4e-2
    wide      H=288  (17,13) 1.3e-2
    wide      H=512  (17,13) 1.4e-2
    long      H=64   (7,40) 1.7e-2   (data seed 2; with seed B 1000 + H + V the emulation reaches 3.3e-2 in dn, above the cap)

The hidden states alone stay at 2.0e-3 .. 3.7e-3 in every case; the largest figures belong to the gradient blocks.
(test_context_reference_host.py::test_gru_bf16_emulation_stays_below_its_cap prints all five figures of every case.)

LayerNorm with a large mean (rows 1000 + N(0,1), f32, M = 37): the bound is 4 x the largest error against float64 of the same two-pass
algorithm run in float32 on the host in three summation orders (y relative to its largest entry / rstd relative):

    C = 64     sequential 9.2e-5 / 1.5e-7   pairwise 2.4e-5 / 7.1e-8   lane-strided 2.8e-5 / 1.3e-7   -> bounds 3.7e-4 / 6.1e-7
    C = 1024   sequential 3.0e-4 / 7.5e-7   pairwise 2.3e-5 / 1.2e-7   lane-strided 2.0e-5 / 8.8e-8   -> bounds 1.2e-3 / 3.0e-6

No tolerance here was obtained by running a kernel: they are the older tests' figures, the emulation's and the host algorithms' own
errors, or counted roundings (stated where used).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
import context_reference as R  # noqa: E402
from test_attention_long_gpu import guard_intact, guarded  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
U24 = 2.0 ** -24          # half the spacing of f32 numbers, relative
U8 = 2.0 ** -8            # the same of bf16 (8 significant bits)


def name(dt):
    return "f32" if dt == torch.float32 else "bf16"


def dev(t, dt):
    """A float64 host tensor that is exact in dt -> device tensor of dt."""
    return t.to(dt).to(DEV).contiguous()


def host(t):
    return t.detach().double().cpu()


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def device_mask(n, p, seed, site):
    """cpc_dropout_mask, checked against its host twin (context_reference.dropout_mask_host)."""
    mb, m = guarded(n, torch.float32)
    _hip.call("cpc_dropout_mask", _hip.ptr(m), n, p, seed, site)
    torch.cuda.synchronize()
    assert guard_intact(mb, n)
    m = host(m)
    assert torch.equal(m, R.dropout_mask_host(n, p, seed, site))
    return m


# ======================================================================================================================= A1  GRU
def _gru_device(dt, B, V, H, ref):
    """cpc_prep_frag, cpc_gru_fwd / cpc_gru_fwd_h0, cpc_gru_bwd on the reference's inputs; returns Hall (B, V+1, H), c, dG (B, V, 4H)."""
    code = _hip.dtype_code(dt)
    dW = ref["w_hh"].to(DEV).contiguous()
    wfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
    wTfrag = torch.empty(3 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wfrag), 3 * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wTfrag), H, 3 * H, H, 1, code)
    dGi, db, ddc = dev(ref["gir"], dt), ref["b_hh"].to(DEV), ref["dc"].to(DEV)
    nt = int(_hip.lib().cpc_gru_tape_elems(B, V, H, code))
    hb, Hall = guarded(B * (V + 1) * H, dt)
    cb, c = guarded(B * H, torch.float32)
    tb, tape = guarded(nt, dt)
    if ref["h0"] is not None:
        dh0 = ref["h0"].to(DEV)
        _hip.call("cpc_gru_fwd_h0", _hip.ptr(dGi), _hip.ptr(wfrag), _hip.ptr(db), _hip.ptr(dh0), _hip.ptr(Hall), _hip.ptr(tape),
                  _hip.ptr(c), B, V, H, code)
    else:
        _hip.call("cpc_gru_fwd", _hip.ptr(dGi), _hip.ptr(wfrag), _hip.ptr(db), _hip.ptr(Hall), _hip.ptr(tape), _hip.ptr(c), B, V, H, code)
    torch.cuda.synchronize()
    assert guard_intact(hb, B * (V + 1) * H) and guard_intact(cb, B * H) and guard_intact(tb, nt)
    gb, dG = guarded(B * V * 4 * H, dt)
    _hip.call("cpc_gru_bwd", _hip.ptr(ddc), _hip.ptr(tape), _hip.ptr(wTfrag), _hip.ptr(dG), B, V, H, code)
    torch.cuda.synchronize()
    assert guard_intact(gb, B * V * 4 * H)
    Hall, c, dG = host(Hall).view(B, V + 1, H), host(c).view(B, H), host(dG).view(B, V, 4 * H)
    assert bool(torch.isfinite(Hall).all()) and bool(torch.isfinite(c).all()) and bool(torch.isfinite(dG).all())
    return Hall, c, dG


def _gru_check(dt, ref, Hall, c, dG, label):
    errs = R.gru_step_errors(Hall, dG, ref["hall"], ref["dG"])
    for k in R.GRU_BLOCKS:
        ratio = (errs[k] / ref["tol"][k]).max().item()
        print(f"{label} {k}: largest per-step error {errs[k].max().item():.2e}, largest error / bound {ratio:.2f}")
    bad = R.gru_violations(errs, ref["tol"])
    assert not bad, bad[:8]
    h0 = torch.zeros_like(ref["hall"][:, 0]) if ref["h0"] is None else R.rounded(ref["h0"], dt)
    assert torch.equal(Hall[:, 0], h0), "Hall[:, 0] is not the stored initial state"
    t_f, t_b = (2e-5, 5e-5) if dt == torch.float32 else (2e-2, 4e-2)
    assert R.rel_err(c, ref["c"]) < t_f
    (db, dW), (db_ref, dW_ref) = R.gru_weight_grads(dG, Hall), R.gru_weight_grads(ref["dG"], ref["hall"])
    assert R.rel_err(db, db_ref) < t_b          # the b_hh gradient: column sums of the gradient w.r.t. h W_hh^T + b_hh
    assert R.rel_err(dW, dW_ref) < t_b          # dW_hh = sum_t dGh_t^T h_{t-1}


@pytest.mark.parametrize("case", R.gru_cases(), ids=R.gru_case_id)
def test_gru_fwd_bwd_per_step(case):
    """Every kernel family at its edges (a single batch row, partial batch tiles, one and two steps, hidden sizes that leave waves with
    unequal or no tiles), hidden states and the four gradient blocks judged step by step; the b_hh and W_hh gradients derived from
    them as the engine derives them; nothing written behind Hall, c, the tape or dG."""
    _, dt, H, B, V = case
    ref = R.gru_reference(dt, B, V, H, seed=R.gru_case_seed(case), with_h0=R.gru_case_h0(case))
    if ref["e_model"] is not None:
        assert max(float(v.max()) for v in ref["e_model"].values()) < R.GRU_MODEL_CAP
    Hall, c, dG = _gru_device(dt, B, V, H, ref)
    _gru_check(dt, ref, Hall, c, dG, R.gru_case_id(case))


@pytest.mark.parametrize("dt,H", [(torch.bfloat16, 64), (torch.bfloat16, 256), (torch.bfloat16, 96), (torch.float32, 48),
                                  (torch.float32, 288), (torch.bfloat16, 288)])
def test_gru_without_recurrent_weights_is_elementwise(dt, H):
    """W_hh = 0, b_hh = 0: h_t = (1 - sigmoid(a_u)) tanh(a_n) + sigmoid(a_u) h_{t-1} holds element by element, so any mix-up of batch
    row, step or hidden unit shows as a gross error against the closed form: the input projections are a shuffled ramp over [-3, 3],
    different in every (b, t, j) in f32 (asserted; bf16 has too few numbers for that, there the ramp is rounded).  Every dr entry is
    exactly 0 because q = W_hn h + b_hn = 0.  Bounds as test_gru_fwd_bwd_per_step."""
    B, V = 17, 5
    ref = R.gru_reference(dt, B, V, H, with_h0=True, zero_weights=True)
    if dt == torch.float32:
        assert ref["gir"].unique().numel() == ref["gir"].numel()
    closed = R.gru_closed_form_zero_weights(ref["gir"], ref["h0"].double())
    assert (closed - ref["hall"]).abs().max() < 1e-14
    Hall, c, dG = _gru_device(dt, B, V, H, ref)
    err = R.per_step_err(Hall[:, 1:], closed[:, 1:])
    print(f"zero weights {name(dt)} H={H}: per-step error of h against the closed form {err.max().item():.2e}")
    assert bool((err <= ref["tol"]["Hall"]).all()), err
    assert bool((dG[:, :, :H] == 0).all())
    _gru_check(dt, ref, Hall, c, dG, f"zero weights {name(dt)} H={H}")


# ======================================================================================================================= A2  attention
def _attn_device(qkv, dout, B, S, C, heads, dt, p_drop, seed, site):
    code = _hip.dtype_code(dt)
    d_qkv, d_dout = dev(qkv, dt), dev(dout, dt)
    ob, o = guarded(B * S * C, dt)
    pb, Pd = guarded(B * heads * S * S, dt)
    _hip.call("cpc_attn_fwd", _hip.ptr(d_qkv), _hip.ptr(o), _hip.ptr(Pd), B, S, C, heads, p_drop, seed, site, code)
    torch.cuda.synchronize()
    assert guard_intact(ob, B * S * C) and guard_intact(pb, B * heads * S * S)
    db, dq = guarded(B * S * 3 * C, dt)
    _hip.call("cpc_attn_bwd", _hip.ptr(d_qkv), _hip.ptr(Pd), _hip.ptr(d_dout), _hip.ptr(dq), B, S, C, heads, p_drop, seed, site, code)
    torch.cuda.synchronize()
    assert guard_intact(db, B * S * 3 * C)
    return host(o).view(B * S, C), Pd.view(B * heads, S, S), host(dq).view(B * S, 3 * C)


@pytest.mark.parametrize("C,heads", R.ATTN_SHAPES)
@pytest.mark.parametrize("S", R.ATTN_SEQS)
def test_attn_fwd_bwd_edges(S, C, heads):
    """cpc_attn_fwd / cpc_attn_bwd against float64 autograd of the definition in both storage types, without and with dropout on the
    weights (masks from cpc_dropout_mask), at every sequence length where the kernels change path (2 x 2 blocks, 4-row groups,
    S % 4 stores, 16-row MFMA bands) and at head sizes 64, 32, 8, 60 and 4: P rows sum to 1 and are exactly zero above the
    diagonal, nothing is written past out, P or dqkv, and dq, dk and dv are each judged against their own maximum.
    Tolerances of test_attn128_fwd_bwd."""
    B, seed, site = 3, 987654321, 4
    upper = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
    for dt in DTYPES:
        qkv, dout = R.attn_inputs(B, S, C, heads, dt, seed=S * 7 + C + heads)
        for p_drop in (0.0, 0.3):
            m = device_mask(B * heads * S * S, p_drop, seed, site).reshape(B, heads, S, S) if p_drop else None
            P, out, grad = R.attn_reference(qkv, dout, B, S, C, heads, m)
            o, Pd, dq = _attn_device(qkv, dout, B, S, C, heads, dt, p_drop, seed, site)
            Pg = host(Pd)
            tag = f"S={S} C={C} heads={heads} {name(dt)} p={p_drop}"
            e_o, e_p = R.rel_err(o, out), R.rel_err(Pg, P.reshape(B * heads, S, S))
            e_g = [R.rel_err(dq[:, i * C:(i + 1) * C], grad[:, i * C:(i + 1) * C]) for i in range(3)]
            print(f"{tag}: out {e_o:.2e} P {e_p:.2e} dq {e_g[0]:.2e} dk {e_g[1]:.2e} dv {e_g[2]:.2e} dqkv {R.rel_err(dq, grad):.2e}")
            assert e_o < R.attn_tol(dt), tag
            assert e_p < R.attn_tol(dt), tag                      # the saved weights stay undropped
            assert bool((Pg[:, upper] == 0).all()), tag
            assert (Pg.sum(-1) - 1).abs().max().item() < (1e-5 if dt == torch.float32 else 2e-2), tag
            assert R.rel_err(dq, grad) < R.attn_bwd_tol(dt), tag
            for blk, e in zip(("dq", "dk", "dv"), e_g):
                assert e < R.attn_bwd_tol(dt), (tag, blk, e)


@pytest.mark.parametrize("qk_scale", R.ATTN_LARGE_SCALES)
@pytest.mark.parametrize("S,C,heads", R.ATTN_LARGE_CASES)
def test_attn_large_scores(S, C, heads, qk_scale):
    """q and k scaled so that the scores reach about +-30 (scale 3) and about +-100 (scale 5.5: beyond the overflow of exp in f32, where
    only the max-subtraction keeps the softmax finite): P and out are finite and match float64.  The f32 tolerance gains the
    first-order term exp(delta) - 1, delta = 2 scale 2^-24 max_ij sum_c |q_ic k_jc| computed from the data in float64: what rounding
    the products and partial sums of a score to 24 bits can move it by, and so a softmax weight relative to itself.  Derived, not
    measured."""
    B = 3
    for dt in DTYPES:
        qkv, dout = R.attn_inputs(B, S, C, heads, dt, seed=S + C, qk_scale=qk_scale)
        P, out, _ = R.attn_reference(qkv, dout, B, S, C, heads)
        delta = R.attn_score_delta(qkv, B, S, C, heads)
        tol = R.attn_large_tol(dt, delta)
        o, Pd, dq = _attn_device(qkv, dout, B, S, C, heads, dt, 0.0, 0, 0)
        Pg = host(Pd)
        assert bool(torch.isfinite(Pg).all()) and bool(torch.isfinite(o).all()) and bool(torch.isfinite(dq).all())
        e_p, e_o = R.rel_err(Pg, P.reshape(B * heads, S, S)), R.rel_err(o, out)
        print(f"S={S} C={C} heads={heads} {name(dt)} scale {qk_scale}: delta {delta:.2e} tol {tol:.2e} P {e_p:.2e} out {e_o:.2e}")
        assert e_p < tol and e_o < tol


@pytest.mark.parametrize("C,heads", [(128, 2), (64, 8), (8, 2)])
@pytest.mark.parametrize("S", [1, 16, 17, 64])
def test_attn_exact_data(S, C, heads):
    """q = 0 and v[j][c] = 1 if c == j mod d else 0: P[i][j] = 1 / (i + 1) for j <= i and out[i][c] = #{j <= i: j mod d = c} / (i + 1).
    f32 within 1e-6 relative; bf16 within one bf16 ulp (P is one rounding of 1 / (i + 1); on the matrix pipe out sums rounded weights
    and is rounded once more: two half ulps)."""
    B = 2
    qkv, P, out = R.attn_exact_data(B, S, C, heads)
    for dt in DTYPES:
        o, Pd, _ = _attn_device(qkv, torch.zeros(B * S, C, dtype=torch.float64), B, S, C, heads, dt, 0.0, 0, 0)
        Pg = host(Pd)
        for got, want in ((Pg, P.expand(B * heads, S, S)), (o, out)):
            bound = 1e-6 * want.abs() if dt == torch.float32 else R.bf16_ulp(want) * (want != 0)
            assert bool(((got - want).abs() <= bound).all()), (name(dt), float((got - want).abs().max()))


# ======================================================================================================================= A3  LayerNorm
def _ln_case(dt, M, C, *, with_b=True, with_r_out=True, with_g2=True, bcast=0, p_drop=0.0, nblocks=(5,), eps=R.LN_EPS):
    """cpc_add_ln_fwd, then cpc_ln_bwd + cpc_reduce_slabs for every block count, against float64 F.layer_norm autograd: y, r_out, the
    saved mean and rstd, dr, dr_b and the reduced dw, db.  Tolerances: y and r_out 3e-5 / 1.2e-2, gradients 1e-4 / 2.5e-2 (those of
    test_add_layernorm_fwd_bwd); mean within 32 2^-24 of the row's mean magnitude and rstd within 32 2^-24 of itself
    (context_reference.LN_STAT_ROUNDINGS counts the roundings)."""
    assert with_r_out or not with_b
    g = torch.Generator().manual_seed(M * 3 + C + bcast)
    seed, site = 24681357, 3
    code = _hip.dtype_code(dt)
    a = R.rounded(torch.randn(M, C, generator=g), dt)
    b = R.rounded(torch.randn(M, C, generator=g) * 0.5, dt) if with_b else None
    w = (1 + 0.3 * torch.randn(C, generator=g)).double()
    bias = (0.2 * torch.randn(C, generator=g)).double()
    g1 = R.rounded(torch.randn(M // bcast if bcast else M, C, generator=g), dt)
    g2 = R.rounded(torch.randn(M, C, generator=g), dt) if with_g2 else None
    gscale = 1.0 / bcast if bcast else 1.0
    dy = (g1.repeat_interleave(bcast, 0) if bcast else g1) * float(torch.tensor(gscale, dtype=torch.float32))
    if with_g2:
        dy = dy + g2
    mask = device_mask(M * C, p_drop, seed, site).reshape(M, C) if p_drop else None
    y_ref, r_ref, mean_ref, rstd_ref, dr_ref, dw_ref, db_ref = R.ln_reference(a, b, w, bias, dy, mask)
    da, dw_, dbias = dev(a, dt), w.float().to(DEV), bias.float().to(DEV)
    dbb = dev(b, dt) if with_b else None
    rb, r = guarded(M * C, dt) if with_r_out else (None, None)
    yb, y = guarded(M * C, dt)
    sb, stats = guarded(2 * M, torch.float32)
    _hip.call("cpc_add_ln_fwd", _hip.ptr(da), _hip.ptr(dbb), _hip.ptr(dw_), _hip.ptr(dbias), _hip.ptr(r), _hip.ptr(y), _hip.ptr(stats),
              M, C, eps, p_drop, seed, site, code)
    torch.cuda.synchronize()
    assert guard_intact(yb, M * C) and guard_intact(sb, 2 * M) and (rb is None or guard_intact(rb, M * C))
    tag = f"M={M} C={C} {name(dt)}"
    t_f, t_b = (3e-5, 1e-4) if dt == torch.float32 else (1.2e-2, 2.5e-2)
    assert R.rel_err(y.view(M, C), y_ref) < t_f, tag
    if with_r_out:
        assert R.rel_err(r.view(M, C), r_ref) < t_f, tag
    st = host(stats).view(M, 2)
    slack = R.LN_STAT_ROUNDINGS * U24
    assert bool(((st[:, 0] - mean_ref).abs() <= slack * r_ref.abs().mean(1) + 1e-30).all()), tag
    assert bool(((st[:, 1] - rstd_ref).abs() <= slack * rstd_ref).all()), tag
    r_in = r if with_r_out else da
    dg1, dg2 = dev(g1, dt), (dev(g2, dt) if with_g2 else None)
    for nb in nblocks:
        slb, slabs = guarded(nb * 2 * C, torch.float32)
        drb, dr = guarded(M * C, dt)
        dbb2, dr_b = guarded(M * C, dt) if p_drop else (None, None)
        _hip.call("cpc_ln_bwd", _hip.ptr(dg1), _hip.ptr(dg2), _hip.ptr(r_in), _hip.ptr(stats), _hip.ptr(dw_), _hip.ptr(dr), _hip.ptr(slabs),
                  M, C, bcast, gscale, nb, _hip.ptr(dr_b), p_drop, seed, site, code)
        gwb, gw = guarded(C, torch.float32)
        gbb, gb = guarded(C, torch.float32)
        _hip.call("cpc_reduce_slabs", _hip.ptr(slabs), _hip.ptr(gw), 1, C, nb, 2 * C, 1, 1, 0, 0)
        _hip.call("cpc_reduce_slabs", _hip.ptr(slabs, C), _hip.ptr(gb), 1, C, nb, 2 * C, 1, 1, 0, 0)
        torch.cuda.synchronize()
        assert guard_intact(slb, nb * 2 * C) and guard_intact(drb, M * C) and guard_intact(gwb, C) and guard_intact(gbb, C), (tag, nb)
        sl = host(slabs).view(nb, 2 * C)
        assert bool(torch.isfinite(sl).all()), (tag, nb)
        first_surplus = (M + 3) // 4          # block blk owns the rows 4 blk + wave (+ 4 nb k): none from here on
        assert bool((sl[first_surplus:] == 0).all()), (tag, nb)
        assert R.rel_err(dr.view(M, C), dr_ref) < t_b, (tag, nb)
        if p_drop:
            assert guard_intact(dbb2, M * C)
            assert R.rel_err(dr_b.view(M, C), dr_ref * mask) < t_b, (tag, nb)
            assert bool(((host(dr_b).view(M, C) == 0) | (mask != 0)).all())
        assert R.rel_err(gw, dw_ref) < t_b, (tag, nb)
        assert R.rel_err(gb, db_ref) < t_b, (tag, nb)
        assert R.rel_err(sl.sum(0), torch.cat([dw_ref, db_ref])) < t_b, (tag, nb)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("M", [1, 3, 4, 5, 37])
@pytest.mark.parametrize("C", [4, 8, 252, 256, 260, 1020, 1024])
def test_layernorm_sizes(C, M, dt):
    """One column group, the last lane slot partly and entirely full (C = 1020, 1024), rows that do not fill a block's four waves, and
    1, 5 and ceil(M / 4) + 3 backward blocks: surplus blocks write zero slabs into NaN-filled memory."""
    _ln_case(dt, M, C, nblocks=(1, 5, (M + 3) // 4 + 3))


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_layernorm_second_grid_trip(dt):
    """M = 8197 rows: more than the forward's 2048 blocks x 4 rows, so some waves take a second row."""
    _ln_case(dt, 8197, 8, nblocks=(5, 300))


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("C", [8, 260])
@pytest.mark.parametrize("form", ["no_b", "final_norm", "no_g2", "bcast1", "bcast60", "bcastM", "bcast60_no_g2"])
def test_layernorm_argument_forms(form, C, dt):
    """b = NULL; b = NULL and r_out = NULL (the final norm of attention_model.py: the backward reads a itself); g2 = NULL; gradient rows
    broadcast over 1, 60 and M rows with gscale = 1 / bcast (the mean over time folded into the final norm's backward)."""
    M = 120
    kw = {"no_b": dict(with_b=False), "final_norm": dict(with_b=False, with_r_out=False), "no_g2": dict(with_g2=False),
          "bcast1": dict(bcast=1), "bcast60": dict(bcast=60), "bcastM": dict(bcast=M),
          "bcast60_no_g2": dict(bcast=60, with_g2=False, with_b=False, with_r_out=False)}[form]
    _ln_case(dt, M, C, nblocks=(7,), **kw)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("C", [8, 260, 1024])
def test_layernorm_dropout(C, dt):
    """p = 0.3 on the summand b in the forward (r = a + dropout(b)) and on dr_b in the backward, masks of index m C + c."""
    _ln_case(dt, 37, C, p_drop=0.3, nblocks=(1, 5))


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("C", [1028, 2048])
def test_layernorm_wide_rows_forward_only(C, dt):
    """C > 1024: the forward's second path (three passes over memory), with and without dropout; cpc_ln_bwd refuses C = 1028 and
    leaves dr and the slabs bit for bit untouched."""
    M, seed, site = 9, 97531, 2
    code = _hip.dtype_code(dt)
    g = torch.Generator().manual_seed(C)
    a = R.rounded(torch.randn(M, C, generator=g), dt)
    b = R.rounded(torch.randn(M, C, generator=g) * 0.5, dt)
    w, bias = (1 + 0.3 * torch.randn(C, generator=g)).double(), (0.2 * torch.randn(C, generator=g)).double()
    da, dbb, dw_, dbias = dev(a, dt), dev(b, dt), w.float().to(DEV), bias.float().to(DEV)
    for p_drop in (0.0, 0.3):
        mask = device_mask(M * C, p_drop, seed, site).reshape(M, C) if p_drop else None
        y_ref, r_ref, mean_ref, rstd_ref, _, _, _ = R.ln_reference(a, b, w, bias, torch.zeros(M, C, dtype=torch.float64), mask)
        rb, r = guarded(M * C, dt)
        yb, y = guarded(M * C, dt)
        sb, stats = guarded(2 * M, torch.float32)
        _hip.call("cpc_add_ln_fwd", _hip.ptr(da), _hip.ptr(dbb), _hip.ptr(dw_), _hip.ptr(dbias), _hip.ptr(r), _hip.ptr(y), _hip.ptr(stats),
                  M, C, R.LN_EPS, p_drop, seed, site, code)
        torch.cuda.synchronize()
        assert guard_intact(yb, M * C) and guard_intact(sb, 2 * M) and guard_intact(rb, M * C)
        t_f = 3e-5 if dt == torch.float32 else 1.2e-2
        assert R.rel_err(y.view(M, C), y_ref) < t_f and R.rel_err(r.view(M, C), r_ref) < t_f
        st = host(stats).view(M, 2)
        slack = 2 * R.LN_STAT_ROUNDINGS * U24          # (a lane adds up to 32 values here: twice the roundings of C <= 1024)
        assert bool(((st[:, 0] - mean_ref).abs() <= slack * r_ref.abs().mean(1)).all())
        assert bool(((st[:, 1] - rstd_ref).abs() <= slack * rstd_ref).all())
    if C == 1028:
        nb = 3
        dr = torch.randn(M * C, device=DEV).to(dt)
        slabs = torch.randn(nb * 2 * C, device=DEV)
        dr0, slabs0 = dr.clone(), slabs.clone()
        rc = _hip.lib().cpc_ln_bwd(_hip.ptr(da), None, _hip.ptr(r), _hip.ptr(stats), _hip.ptr(dw_), _hip.ptr(dr), _hip.ptr(slabs), M, C, 0,
                                   1.0, nb, None, 0.0, 0, 0, code, _hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -22
        assert torch.equal(bits(dr), bits(dr0)) and torch.equal(bits(slabs), bits(slabs0))


@pytest.mark.parametrize("C", [64, 1024])
def test_layernorm_large_mean(C):
    """Rows 1000 + N(0, 1) in f32: y and rstd within 4 x the largest error of the float32 two-pass algorithm on the host over three
    summation orders (the figures are in the module docstring); a one-pass variance E[x^2] - E[x]^2 misses this bound
    (test_context_reference_host.py::test_large_mean_bound_rejects_a_one_pass_variance)."""
    M = 37
    bound_y, bound_rstd, errs = R.ln_large_mean_bound(M, C)
    x, w, bias = R.ln_large_mean_data(M, C)
    dx, dw_, dbias = x.to(DEV), w.to(DEV), bias.to(DEV)
    yb, y = guarded(M * C, torch.float32)
    sb, stats = guarded(2 * M, torch.float32)
    _hip.call("cpc_add_ln_fwd", _hip.ptr(dx), None, _hip.ptr(dw_), _hip.ptr(dbias), None, _hip.ptr(y), _hip.ptr(stats), M, C, R.LN_EPS,
              0.0, 0, 0, _hip.F32)
    torch.cuda.synchronize()
    assert guard_intact(yb, M * C) and guard_intact(sb, 2 * M)
    e_y, e_rstd = R.ln_large_mean_errors(host(y).view(M, C), host(stats).view(M, 2)[:, 1], x, w, bias)
    print(f"large mean C={C}: y {e_y:.2e} (bound {bound_y:.2e}) rstd {e_rstd:.2e} (bound {bound_rstd:.2e}); host orders {errs}")
    assert e_y < bound_y and e_rstd < bound_rstd


# ======================================================================================================================= A4  pointwise
def _close(got, ref, mag, dt, roundings=2):
    """|got - ref| within `roundings` f32 roundings of the magnitude mag of the intermediate values; bf16 one more rounding of the
    result to 8 bits."""
    bound = roundings * U24 * mag + 1e-37
    if dt == torch.bfloat16:
        bound = bound + U8 * ref.abs()
    return bool(((host(got) - ref).abs() <= bound).all())


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("B,S,C,gap,with_g2", [(3, 1, 32, 0, True), (3, 11, 32, 9, True), (2, 5, 8, 3, False), (9, 64, 4096, 0, True),
                                               (9, 64, 4096, 0, False)])
def test_pe_scale(B, S, C, gap, with_g2, dt):
    """cpc_pe_scale_fwd / _bwd: one step; items further apart than S C with sentinels in the gaps of dtop untouched; g2 = NULL; and
    B S C / 4 > 2048 x 256 threads, so that the grid-stride loops take a second trip.  One product and one sum in f32 (two roundings,
    or one when fused), then one rounding to the storage type."""
    g = torch.Generator().manual_seed(B + S + C)
    code = _hip.dtype_code(dt)
    stride, t0 = (S + gap) * C, gap // 2
    scale = math.sqrt(C)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    top = R.rounded(torch.randn(B, S + gap, C, generator=g), dt)
    pe = torch.randn(S, C, generator=g).float()
    d_top, d_pe = dev(top, dt), pe.to(DEV)
    xb, x0 = guarded(B * S * C, dt)
    _hip.call("cpc_pe_scale_fwd", _hip.ptr(d_top, t0 * C), _hip.ptr(d_pe), _hip.ptr(x0), B, S, C, stride, scale, code)
    torch.cuda.synchronize()
    assert guard_intact(xb, B * S * C)
    v = top[:, t0:t0 + S] * sc
    assert _close(x0.view(B, S, C), v + pe.double(), v.abs() + pe.double().abs(), dt)
    g1 = R.rounded(torch.randn(B, S, C, generator=g), dt)
    g2 = R.rounded(torch.randn(B, S, C, generator=g), dt) if with_g2 else None
    tb, dtop = guarded(B * stride, dt, fill=-7.5)          # (the gaps are sentinels too)
    d1, d2 = dev(g1, dt), (dev(g2, dt) if with_g2 else None)
    _hip.call("cpc_pe_scale_bwd", _hip.ptr(d1), _hip.ptr(d2), _hip.ptr(dtop, t0 * C), B, S, C, stride, scale, code)
    torch.cuda.synchronize()
    assert guard_intact(tb, B * stride)
    dtv = dtop.view(B, S + gap, C)
    gs = g1 + g2 if with_g2 else g1
    assert _close(dtv[:, t0:t0 + S], gs * sc, (g1.abs() + (g2.abs() if with_g2 else 0)) * sc, dt)
    assert bool((dtv[:, :t0] == -7.5).all()) and bool((dtv[:, t0 + S:] == -7.5).all())


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("B,S,C", [(3, 1, 32), (3, 128, 30), (5, 7, 33), (65, 3, 4100)])
def test_mean_time(B, S, C, dt):
    """cpc_mean_time: one and 128 steps, channel counts that are no multiple of 4, and B C > 1024 x 256 threads (a second trip of the
    grid-stride loop).  S sequential f32 additions and a division, then one rounding to the storage type."""
    g = torch.Generator().manual_seed(B + S + C)
    x = R.rounded(torch.randn(B, S, C, generator=g), dt)
    mb, m = guarded(B * C, dt)
    dx = dev(x, dt)
    _hip.call("cpc_mean_time", _hip.ptr(dx), _hip.ptr(m), B, S, C, _hip.dtype_code(dt))
    torch.cuda.synchronize()
    assert guard_intact(mb, B * C)
    assert _close(m.view(B, C), x.mean(1), x.abs().mean(1), dt, roundings=S + 1)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
@pytest.mark.parametrize("n", [5, 4096 * 256 + 3])
def test_dropout_in_place(n, dt):
    """cpc_dropout: x *= mask in place, bit-equal to x mask rounded once; n = 4096 x 256 + 3 takes the grid-stride loop into a second
    trip with an odd tail."""
    p, seed, site = 0.3, 1357911, 6
    mask = device_mask(n, p, seed, site)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dt)
    xb, xd = guarded(n, dt)
    xd.copy_(x.to(DEV))
    _hip.call("cpc_dropout", _hip.ptr(xd), n, p, seed, site, _hip.dtype_code(dt))
    torch.cuda.synchronize()
    assert guard_intact(xb, n)
    want = (x.float() * mask.float()).to(dt)
    assert torch.equal(xd.cpu(), want)
    assert bool(((want == 0) | (mask != 0)).all())
    assert n < 100 or 0.29 < float((mask == 0).double().mean()) < 0.31
