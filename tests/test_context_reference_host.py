"""The references of test_context_kernels_gpu.py (tests/context_reference.py) judged on the host: they are the definitions (torch's own
GRU, scaled-dot-product attention and layer_norm in float64), the bf16 emulation of the GRU kernels stays below its cap on every kernel
case, and the metrics and tolerances the kernel tests use reject deliberate mistakes put into the reference, while the whole-tensor
measure of the older GRU tests accepts a backward pass whose early steps are 100 % wrong (the gap the per-step measure closes).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import context_reference as R

BF16_CASES = [c for c in R.gru_cases() if c[1] == R.BF16]


# ------------------------------------------------------------------------------------------------------------------ the definitions
@pytest.mark.parametrize("B,V,H,with_h0", [(3, 5, 16, False), (2, 7, 32, True), (1, 1, 16, True)])
def test_gru_reference_is_nn_gru(B, V, H, with_h0):
    """gru_run (forward and hand-written backward) against autograd of torch.nn.GRU in float64 fed with the input projections (an
    identity weight_ih, no bias_ih)."""
    w_hh, b_hh, Gi, dc, h0 = (None if t is None else t.double() for t in R.gru_data(B, V, H, with_h0=with_h0))
    gru = torch.nn.GRU(3 * H, H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H, dtype=torch.float64))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(w_hh)
        gru.bias_hh_l0.copy_(b_hh)
    x = Gi.clone().requires_grad_(True)
    start = torch.zeros(1, B, H, dtype=torch.float64) if h0 is None else h0[None]
    hs, last = gru(x, start)
    (last[0] * dc).sum().backward()
    hall, c, dG = R.gru_run(Gi, w_hh, b_hh, dc, h0)
    assert (hall[:, 1:] - hs).abs().max() < 1e-13 and (c - last[0]).abs().max() < 1e-13
    assert torch.equal(hall[:, 0], start[0])
    assert R.rel_err(dG[:, :, :3 * H], x.grad) < 1e-12
    db, dW = R.gru_weight_grads(dG, hall)
    assert R.rel_err(db, gru.bias_hh_l0.grad) < 1e-12 and R.rel_err(dW, gru.weight_hh_l0.grad) < 1e-12


def test_gru_closed_form_without_recurrent_weights():
    w_hh, b_hh, Gi, dc, h0 = (t.double() for t in R.gru_data(3, 6, 16, with_h0=True))
    hall, _, dG = R.gru_run(Gi, torch.zeros_like(w_hh), torch.zeros_like(b_hh), dc, h0)
    assert (hall - R.gru_closed_form_zero_weights(Gi, h0)).abs().max() < 1e-15
    assert bool((dG[:, :, :16] == 0).all())


@pytest.mark.parametrize("S,C,heads", [(1, 8, 2), (5, 64, 8), (17, 120, 2), (64, 128, 2)])
def test_attention_reference_is_scaled_dot_product_attention(S, C, heads):
    B, d = 3, C // heads
    qkv, dout = R.attn_inputs(B, S, C, heads, torch.float64, seed=S + C)
    P, out, grad = R.attn_reference(qkv, dout, B, S, C, heads)
    x = qkv.clone().requires_grad_(True)
    q, k, v = (t.reshape(B, S, heads, d).permute(0, 2, 1, 3) for t in x.split(C, dim=1))
    want = F.scaled_dot_product_attention(q, k, v, is_causal=True).permute(0, 2, 1, 3).reshape(B * S, C)
    want.backward(dout)
    assert R.rel_err(out, want) < 1e-13 and R.rel_err(grad, x.grad) < 1e-12
    assert (P.sum(-1) - 1).abs().max() < 1e-14 and bool((P[..., torch.triu(torch.ones(S, S, dtype=torch.bool), 1)] == 0).all())


@pytest.mark.parametrize("S,C,heads", [(1, 8, 2), (16, 64, 8), (17, 128, 2), (64, 8, 2)])
def test_attention_exact_data_is_what_the_definition_gives(S, C, heads):
    qkv, P, out = R.attn_exact_data(2, S, C, heads)
    Pr, outr, _ = R.attn_reference(qkv, torch.zeros(2 * S, C, dtype=torch.float64), 2, S, C, heads)
    assert (Pr - P).abs().max() < 1e-15 and (outr - out).abs().max() < 1e-15


def test_layernorm_reference_is_layer_norm():
    g = torch.Generator().manual_seed(1)
    a, b, dy = (torch.randn(7, 12, generator=g).double() for _ in range(3))
    w, bias = torch.randn(12, generator=g).double(), torch.randn(12, generator=g).double()
    mask = R.dropout_mask_host(7 * 12, 0.3, 5, 2).reshape(7, 12)
    y, r, mean, rstd, dr, dw, db = R.ln_reference(a, b, w, bias, dy, mask)
    assert torch.equal(r, a + b * mask)
    assert (y - F.layer_norm(r, (12,), w, bias, R.LN_EPS)).abs().max() == 0
    assert (y - ((r - mean[:, None]) * rstd[:, None] * w + bias)).abs().max() < 1e-14
    assert (db - dy.sum(0)).abs().max() < 1e-14 and (dw - (dy * (r - mean[:, None]) * rstd[:, None]).sum(0)).abs().max() < 1e-13
    # float32 host versions of the two-pass algorithm agree with it to float32 accuracy on ordinary data, in every order
    for order in R.LN_F32_ORDERS:
        y32, m32, s32 = R.ln_forward_f32(r.numpy(), w.numpy(), bias.numpy(), order)
        assert R.rel_err(torch.from_numpy(y32), y) < 1e-6 and R.rel_err(torch.from_numpy(s32), rstd) < 1e-6


def test_host_dropout_mask():
    m = R.dropout_mask_host(100000, 0.3, 987654321, 4)
    keep = float(torch.tensor(1.0, dtype=torch.float32) / (1 - torch.tensor(0.3, dtype=torch.float32)))
    assert set(m.unique().tolist()) == {0.0, keep}
    assert abs(float((m > 0).double().mean()) - 0.7) < 0.01
    assert not torch.equal(m, R.dropout_mask_host(100000, 0.3, 987654321, 5))
    assert torch.equal(R.dropout_mask_host(10, 0.0, 1, 1), torch.ones(10, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------ the caps
@pytest.mark.parametrize("case", BF16_CASES, ids=R.gru_case_id)
def test_gru_bf16_emulation_stays_below_its_cap(case):
    """max_t e_model(t) < 2e-2 for Hall and the four blocks of dG: the kernel test's bound 4 e_model(t) never exceeds 8e-2."""
    _, dt, H, B, V = case
    ref = R.gru_reference(dt, B, V, H, seed=R.gru_case_seed(case), with_h0=R.gru_case_h0(case))
    worst = {k: float(v.max()) for k, v in ref["e_model"].items()}
    print(R.gru_case_id(case), {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < R.GRU_MODEL_CAP, worst
    assert min(float(v.min()) for v in ref["e_model"].values()) > 0


# ------------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("mutation", ["drop_keep", "scale_rec"])
@pytest.mark.parametrize("case", [c for c in R.gru_cases() if c[4] >= 13], ids=R.gru_case_id)
def test_gru_metric_rejects_a_wrong_recurrence(case, mutation):
    """dh_{t-1} without its dh * u term for t < V - 3, or with its dgh W_hh term scaled by 0.9: the mutated float64 reference against
    the true one fails the per-step bounds of the kernel test (every case with more than two steps; with one or two steps the
    mutations change nothing or next to nothing)."""
    _, dt, H, B, V = case
    ref = R.gru_reference(dt, B, V, H, seed=R.gru_case_seed(case), with_h0=R.gru_case_h0(case))
    h0 = None if ref["h0"] is None else ref["h0"].double()
    hall, _, dG = R.gru_run(ref["gir"], ref["wr"], ref["br"], ref["dc"].double(), h0, mutation=mutation)
    bad = R.gru_violations(R.gru_step_errors(hall, dG, ref["hall"], ref["dG"]), ref["tol"])
    assert bad, "the mutation passes the kernel test's bounds"
    assert all(k != "Hall" for k, *_ in bad)          # (the forward is untouched)
    assert not R.gru_violations(R.gru_step_errors(ref["hall"], ref["dG"], ref["hall"], ref["dG"]), ref["tol"])


def test_whole_tensor_measure_accepts_wrong_early_steps():
    """The gap, pinned.  (B, V, H) = (7, 13, 64) with the data of test_hip_kernels.py::test_gru_fwd_bwd (seed B + H), bf16 inputs: the
    largest gradient entry of step t is 5.9e-3 (t = 0) .. 2.1e-2 (t = 4) .. 0.16 (t = 7, 8) of the global maximum.  A backward pass
    whose dh_{t-1} loses the dh * u term for t < 6 gets steps 0 .. 4 about 100 % wrong, yet max |got - ref| / max |ref| stays below
    the old bf16 tolerance 4e-2 for the whole dG (2.4e-2), the derived b_hh gradient (2.9e-2) and the derived dW_hh (1.6e-2), while
    the per-step measure sees errors near 1.  (Further up the old checks do notice: for t < 7 the b_hh check reads 4.06e-2, and
    for t < V - 3 = 10, which reaches steps 7 and 8, the whole-tensor error is 0.17.)"""
    B, V, H = 7, 13, 64
    w, b, Gi, dc, _ = R.gru_data(B, V, H, seed=B + H)
    wr, gir, br, dcr = R.rounded(w, R.BF16), R.rounded(Gi, R.BF16), b.double(), dc.double()
    hall, _, dG = R.gru_run(gir, wr, br, dcr)
    share = dG.abs().amax((0, 2)) / dG.abs().max()
    assert share[0] < 1e-2 and share[:5].max() < 2.5e-2 and share[12] == 1
    _, _, bad = R.gru_run(gir, wr, br, dcr, mutation="drop_keep", below=6)
    t_old = 4e-2
    assert R.rel_err(bad[:, :, :3 * H], dG[:, :, :3 * H]) < t_old
    (db_bad, dW_bad), (db, dW) = R.gru_weight_grads(bad, hall), R.gru_weight_grads(dG, hall)
    assert R.rel_err(db_bad, db) < t_old and R.rel_err(dW_bad, dW) < t_old
    errs = R.gru_step_errors(hall, bad, hall, dG)
    assert min(float(errs[k][:5].min()) for k in R.GRU_BLOCKS[1:]) > 0.5
    e_model = R.gru_step_errors(*R.gru_run(gir, wr, br, dcr, rnd=R.to_bf16)[::2], hall, dG)
    assert R.gru_violations(errs, {k: R.GRU_MODEL_FACTOR * v for k, v in e_model.items()})
    _, _, literal = R.gru_run(gir, wr, br, dcr, mutation="drop_keep")
    assert R.rel_err(literal[:, :, :3 * H], dG[:, :, :3 * H]) > t_old


@pytest.mark.parametrize("C,heads", R.ATTN_SHAPES)
@pytest.mark.parametrize("S", [s for s in R.ATTN_SEQS if s > 1])
def test_attention_metrics_reject_a_wrong_mask(S, C, heads):
    """A causal mask j < i instead of j <= i fails the P check, a dropout factor read at j S + i instead of i S + j fails the out and
    dqkv checks (the widest tolerances of the kernel test: bf16's), at every kernel case with more than one step."""
    B, p_drop, seed, site = 3, 0.3, 987654321, 4
    qkv, dout = R.attn_inputs(B, S, C, heads, R.BF16, seed=S * 7 + C + heads)
    m = R.dropout_mask_host(B * heads * S * S, p_drop, seed, site).reshape(B, heads, S, S)
    P, out, grad = R.attn_reference(qkv, dout, B, S, C, heads, m)
    Pm, _, _ = R.attn_reference(qkv, dout, B, S, C, heads, m, mutation="strict_causal")
    assert R.rel_err(Pm, P) > R.attn_tol(R.BF16)
    _, outm, gradm = R.attn_reference(qkv, dout, B, S, C, heads, m, mutation="transposed_mask")
    assert R.rel_err(outm, out) > R.attn_tol(R.BF16)
    assert R.rel_err(gradm[:, 2 * C:], grad[:, 2 * C:]) > R.attn_bwd_tol(R.BF16)


@pytest.mark.parametrize("S,C,heads", R.ATTN_LARGE_CASES)
def test_large_scores_need_the_max_subtraction(S, C, heads):
    """A float32 softmax without max-subtraction: with scores of about +-100 its weights are not finite (exp overflows above 88.7),
    so the kernel test's check rejects it; with scores of about +-30 exp(30) is an ordinary float32 number and the mutation is
    as accurate as the real thing: only the larger of the kernel test's two scales can tell the two apart."""
    B = 3
    reach = {}
    for qk in R.ATTN_LARGE_SCALES:
        qkv, dout = R.attn_inputs(B, S, C, heads, R.F32, seed=S + C, qk_scale=qk)
        P, out, _ = R.attn_reference(qkv, dout, B, S, C, heads)
        d = C // heads
        q, k = (t.reshape(B, S, heads, d).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1)[:2])
        reach[qk] = float(((q @ k.transpose(-1, -2)) / math.sqrt(d)).tril().abs().max())
        tol = R.attn_large_tol(R.F32, R.attn_score_delta(qkv, B, S, C, heads))
        assert tol < 2e-4
        Pm, _, _ = R.attn_reference(qkv, dout, B, S, C, heads, mutation="no_max", dtype=torch.float32)
        P32, _, _ = R.attn_reference(qkv, dout, B, S, C, heads, dtype=torch.float32)
        assert R.rel_err(P32, P) < tol          # (a float32 softmax with max-subtraction passes)
        rejected = not (bool(torch.isfinite(Pm).all()) and R.rel_err(Pm, P) < tol)
        assert rejected == (qk == R.ATTN_LARGE_SCALES[1]), (qk, reach)
    assert 20 < reach[R.ATTN_LARGE_SCALES[0]] < 60 and reach[R.ATTN_LARGE_SCALES[1]] > 89, reach


@pytest.mark.parametrize("C", [64, 1024])
def test_large_mean_bound_rejects_a_one_pass_variance(C):
    """Rows 1000 + N(0, 1) in float32: the two-pass algorithm in three summation orders gives the bound (4 x its largest error); a
    variance computed as E[x^2] - E[x]^2 misses that bound in every order."""
    M = 37
    by, bs, errs = R.ln_large_mean_bound(M, C)
    print(f"C={C}: two-pass float32 errors (y, rstd) per order", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in errs.items()},
          f"bounds y {by:.2e} rstd {bs:.2e}")
    assert by < 1e-2 and bs < 1e-2
    x, w, bias = R.ln_large_mean_data(M, C)
    for order in R.LN_F32_ORDERS:
        y, _, rstd = R.ln_forward_f32(x.numpy(), w.numpy(), bias.numpy(), order, one_pass=True)
        ey, es = R.ln_large_mean_errors(torch.from_numpy(y), torch.from_numpy(rstd), x, w, bias)
        assert not ey < by and not es < bs, (order, ey, es)
