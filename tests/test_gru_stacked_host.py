"""Stacked GRU context (AudioGRUModel(num_layers > 1)), host side: the float64 references of tests/gru_stacked_reference.py against
torch autograd and stacked nn.GRUCell, the cap on the bf16 emulation's error for every kernel case of test_gru_stacked_gpu.py, the
sensitivity of the per-step verdict to an off-by-one in t and to a misplaced addition, the argument checks of cpc_gru_bwd_steps (the
library loads on a CPU host; the pointers are never dereferenced) and the model surface.  No device is touched.
"""
import ctypes as C
import os

import pytest
import torch

import context_reference as R
import gru_stacked_reference as S
from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel, encoder_default_dict
from oracle import cpc_oracle as O

SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64] * 5, 'bias': True}


def _cell_loop(gi, w, b, h0):
    """nn.GRUCell's gates from the input projections, differentiable; returns all hidden states (B, V+1, H)."""
    H = w.shape[1]
    h, hs = h0, [h0]
    for t in range(gi.shape[1]):
        gh = h @ w.T + b
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        u = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - u) * n + u * h
        hs.append(h)
    return torch.stack(hs, 1)


@pytest.mark.parametrize("with_h0,with_dc", [(False, True), (True, True), (False, False)])
def test_steps_reference_against_autograd(with_h0, with_dc):
    """gru_run_steps against torch autograd in float64 on L = sum c dc + sum Hall[:, 1:] dhs: the gradient of the input projections is
    dG[:, :, :3H], that of h W_hh^T + b_hh is [dr | du | dn r]; to 1e-12 (the formulation agrees to 2e-16 at these sizes)."""
    B, V, H = 3, 5, 16
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(3 * H, H, generator=g) / 4).double().requires_grad_(True)
    b = (torch.randn(3 * H, generator=g) * 0.1).double().requires_grad_(True)
    gi = torch.randn(B, V, 3 * H, generator=g).double().requires_grad_(True)
    dc = torch.randn(B, H, generator=g).double() if with_dc else None
    dhs = torch.randn(B, V, H, generator=g).double()
    h0 = torch.randn(B, H, generator=g).double() * 0.5 if with_h0 else None
    hs = _cell_loop(gi, w, b, torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0)
    loss = (hs[:, 1:] * dhs).sum() + ((hs[:, -1] * dc).sum() if with_dc else 0.0)
    loss.backward()
    hall, c, dG = S.gru_run_steps(gi.detach(), w.detach(), b.detach(), dc, dhs, h0)
    assert (hall - hs.detach()).abs().max() < 1e-12 and (c - hs[:, -1].detach()).abs().max() < 1e-12
    assert R.rel_err(dG[:, :, :3 * H], gi.grad) < 1e-12
    db, dW = R.gru_weight_grads(dG, hall)
    assert R.rel_err(db, b.grad) < 1e-12 and R.rel_err(dW, w.grad) < 1e-12
    # with dhs = 0 it is context_reference.gru_run
    if with_dc:
        plain = R.gru_run(gi.detach(), w.detach(), b.detach(), dc, h0)
        zero = S.gru_run_steps(gi.detach(), w.detach(), b.detach(), dc, torch.zeros_like(dhs), h0)
        assert all(torch.equal(a, b_) for a, b_ in zip(plain, zero))


@pytest.mark.parametrize("L", [2, 3])
def test_stacked_reference_against_stacked_grucell(L):
    """The model reference's stack (oracle gru_cell per layer) against a stack of torch.nn.GRUCell in float64: output, gradient of the
    input and of every parameter, to 1e-12."""
    B, E, V, H = 4, 24, 7, 32
    torch.manual_seed(L)
    gru = AudioGRUModel(E, H, num_layers=L)
    params = {"autoregressive_model." + k: v.detach().double().requires_grad_(True) for k, v in gru.state_dict().items()}
    cells = [torch.nn.GRUCell(E if l == 0 else H, H).double() for l in range(L)]
    for cell, pre in zip(cells, S.gru_prefixes(L)):
        cell.load_state_dict({k: params[pre + k].detach() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")})
    z = torch.randn(B, E, V, generator=torch.Generator().manual_seed(1)).double()
    dcv = torch.randn(B, H, generator=torch.Generator().manual_seed(2)).double()
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    hs = [torch.zeros(B, H, dtype=torch.float64) for _ in range(L)]
    for t in range(V):
        x = za[:, :, t]
        for l in range(L):
            hs[l] = cells[l](x, hs[l])
            x = hs[l]
    (hs[-1] * dcv).sum().backward()
    c = S.stacked_gru_forward(zb, params, L)
    (c * dcv).sum().backward()
    assert R.rel_err(c, hs[-1]) < 1e-12 and R.rel_err(zb.grad, za.grad) < 1e-12
    for cell, pre in zip(cells, S.gru_prefixes(L)):
        for k, p in cell.named_parameters():
            assert R.rel_err(params[pre + k].grad, p.grad) < 1e-12, (pre, k)


@pytest.mark.parametrize("case", S.stacked_cases(), ids=S.stacked_case_id)
def test_steps_bf16_emulation_stays_below_its_cap(case):
    """The bf16 bound of the kernel test is GRU_MODEL_FACTOR x the emulation's own per-step error; that error must stay below
    GRU_MODEL_CAP = 2e-2 at every step of every block, with the recipe's dc and with dc = 0 (a lower layer has none)."""
    for with_dc in (True, False):
        ref = S.stacked_reference(R.BF16, case, with_dc=with_dc)
        worst = {k: float(v.max()) for k, v in ref["e_model"].items()}
        print(S.stacked_case_id(case), "dc" if with_dc else "dc=0", {k: f"{v:.2e}" for k, v in worst.items()})
        assert max(worst.values()) < R.GRU_MODEL_CAP, (with_dc, worst)


@pytest.mark.parametrize("mutation", ["shift", "after_keep"])
@pytest.mark.parametrize("dt", [R.F32, R.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(64, 17, 13), (96, 17, 13), (288, 17, 13), (64, 1, 2)], ids=S.stacked_case_id)
def test_steps_verdict_rejects_mistakes(case, dt, mutation):
    """A sweep that reads dhs one step off, or that adds it after the keep term d u was formed, violates the per-step bounds the GPU
    test applies (f32: GRU_TOL_F32; bf16: 4 x the emulation's error, the mistaken sweep itself run through the bf16 emulation)."""
    for with_dc in (True, False):
        ref = S.stacked_reference(dt, case, with_dc=with_dc, mutation=mutation)
        hall, _, dG = ref["mutant"]
        bad = R.gru_violations(R.gru_step_errors(hall, dG, ref["hall"], ref["dG"]), ref["tol"])
        assert bad, (case, mutation, with_dc)
        assert not any(k == "Hall" for k, *_ in bad)          # the forward pass is untouched by both


@pytest.mark.parametrize("H", [64, 96, 288])
def test_exact_gate_data_is_exact_in_bf16(H):
    """The data of the GPU test's exact-data case: its pre-activations are exact in bf16, the closed-form gates and hidden states differ
    from their bf16 roundings by at most 6.2e-6 (r near 1) and 1e-9 (u, n, h_prev), all nine pairs of r and n levels occur, and the bf16
    emulation of the sweep stays within 2^-8 of the unrounded closed form at every step for a gradient at the first, an interior and
    the last step: the store of the result is the one rounding left, and 2^-8 is the largest relative error of one rounding to bf16's
    8 significant bits (strictly: 2^-8 / (1 + 2^-8), which leaves 1.5e-5 for the 6.1e-6 of r)."""
    B, V = 17, 13
    Gi = S.exact_gate_data(B, V, H)
    gir = Gi.double()
    assert torch.equal(R.rounded(Gi, R.BF16), gir)
    r, u, n, hp = S.zero_weight_gates(gir)
    assert float((r - R.to_bf16(r)).abs().max()) <= 6.2e-6
    for x in (u, n, hp):
        assert float((x - R.to_bf16(x)).abs().max()) <= 1e-9
    assert float(hp.abs().max()) > 0.9 and len(hp.unique()) > 100
    assert len({(float(a), float(c)) for a, c in zip(gir[:, :S.EXACT_N_STEPS, :H].flatten()[:2000],
                                                     gir[:, :S.EXACT_N_STEPS, 2 * H:].flatten()[:2000])}) == 9
    w, b = torch.zeros(3 * H, H, dtype=torch.float64), torch.zeros(3 * H, dtype=torch.float64)
    for s in (0, 6, V - 1):
        dhs = torch.zeros(B, V, H, dtype=torch.float64)
        dhs[:, s] = R.to_bf16(torch.randn(B, H, generator=torch.Generator().manual_seed(s + H)))
        ref = S.gru_run_steps(gir, w, b, None, dhs)
        emu = S.gru_run_steps(gir, w, b, None, dhs, rnd=R.to_bf16)
        errs = R.gru_step_errors(emu[0], emu[2], ref[0], ref[2])
        for k in ("du", "dn", "dnr"):
            assert float(errs[k][:s + 1].max()) <= 2.0 ** -8, (s, k, errs[k])
            assert float(ref[2][:, :s + 1].abs().amax((0, 2)).min()) > 0


def test_bwd_steps_arguments_are_checked_before_any_launch():
    """Every CPC_EINVAL (-22) of cpc_gru_bwd_steps: NULL tape / WTfrag / dG, dc and dHs both NULL, B or V < 1, an H or dtype that
    cpc_gru_bwd refuses, ld_h < H or not a multiple of the 16-byte vector width with dHs given.  No kernel is launched."""
    lib = _hip.lib()
    P, N, s = C.c_void_p(0x1000), None, C.c_void_p(0)
    ll = C.c_longlong
    bf, f32 = _hip.BF16, _hip.F32
    call = lib.cpc_gru_bwd_steps
    assert call(P, P, ll(64), N, P, P, 16, 4, 64, bf, s) == -22
    assert call(P, P, ll(64), P, N, P, 16, 4, 64, bf, s) == -22
    assert call(P, P, ll(64), P, P, N, 16, 4, 64, bf, s) == -22
    assert call(N, N, ll(64), P, P, P, 16, 4, 64, bf, s) == -22
    assert call(N, N, ll(0), P, P, P, 16, 4, 64, f32, s) == -22
    for B, V in ((0, 4), (-1, 4), (16, 0), (16, -3)):
        assert call(P, P, ll(64), P, P, P, B, V, 64, bf, s) == -22
        assert call(P, N, ll(0), P, P, P, B, V, 64, bf, s) == -22
    for H, code in ((528, f32), (528, bf), (496, bf), (520, f32), (300, f32), (1024, f32), (0, f32), (48, bf)):
        assert call(P, P, ll(1024), P, P, P, 16, 4, H, code, s) == -22, H
        assert call(N, P, ll(1024), P, P, P, 16, 4, H, code, s) == -22, H
    for code in (2, -1, 7):
        assert call(P, P, ll(64), P, P, P, 16, 4, 64, code, s) == -22
    for H, code, ld in ((64, bf, 63), (64, bf, 56), (64, bf, 0), (64, bf, -64), (64, bf, 68), (64, bf, 65), (64, f32, 66), (64, f32, 60),
                        (288, bf, 292), (288, f32, 290), (512, bf, 256)):
        assert call(P, P, ll(ld), P, P, P, 16, 4, H, code, s) == -22, (H, code, ld)
        assert call(N, P, ll(ld), P, P, P, 16, 4, H, code, s) == -22, (H, code, ld)


GRU_KEYS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _expected_keys(L):
    keys = [f"encoder.layers.{l}.{n}" for l in range(5) for n in ("weight", "bias")]
    keys += ["autoregressive_model.gruCell." + n for n in GRU_KEYS]
    keys += [f"autoregressive_model.upper_cells.{i}.{n}" for i in range(L - 1) for n in GRU_KEYS]
    return keys + ["prediction_model.weight"]


def _full_model(L, seed=0, **kw):
    torch.manual_seed(seed)
    enc = AudioEncoder(encoder_default_dict)
    ar = AudioGRUModel(input_size=512, hidden_size=256, **({} if L is None else {"num_layers": L}), **kw)
    return AudioPredictiveCodingModel(enc, ar, enc_size=512, ar_size=256, visible_steps=100, prediction_steps=12)


def test_num_layers_surface():
    """Keys and parameter count for num_layers 1, 2, 4; num_layers = 1 (given or defaulted) is today's model: today's key list, today's
    count and the oracle's seed-0 values; under one seed the encoder and gruCell do not depend on num_layers (the upper cells are
    created after gruCell); values outside 1 .. 4 and non-integers are refused."""
    per_upper = 2 * 3 * 256 * 256 + 2 * 3 * 256
    models = {L: _full_model(L) for L in (None, 1, 2, 4)}
    ref = O.init_params(seed=0)
    for L, m in models.items():
        n = 1 if L is None else L
        assert list(m.state_dict().keys()) == _expected_keys(n), L
        assert m.parameter_count() == 7414784 + (n - 1) * per_upper, L
        assert m.autoregressive_model.num_layers == n
        for k, v in m.state_dict().items():
            if k.startswith("encoder.") or k.startswith("autoregressive_model.gruCell."):
                assert torch.equal(v, ref[k]), (L, k)
    for L in (None, 1):
        assert not hasattr(models[L].autoregressive_model, "upper_cells")
        for k, v in models[L].state_dict().items():
            assert torch.equal(v, ref[k]), (L, k)          # the predictor too: no random number was drawn in between
    for i in range(3):
        cell = models[4].autoregressive_model.upper_cells[i]
        assert cell.input_size == 256 and cell.hidden_size == 256
        assert tuple(cell.weight_ih.shape) == (768, 256) and tuple(cell.bias_hh.shape) == (768,)
        assert float(cell.weight_ih.detach().abs().max()) <= 1.0 / 16 and float(cell.weight_ih.detach().std()) > 0.02          # U(-1/sqrt(H), 1/sqrt(H))
    nb = AudioGRUModel(64, 32, bias=False, num_layers=3)
    assert [k for k, _ in nb.named_parameters()] == ["gruCell.weight_ih", "gruCell.weight_hh", "upper_cells.0.weight_ih",
                                                    "upper_cells.0.weight_hh", "upper_cells.1.weight_ih", "upper_cells.1.weight_hh"]
    for bad in (0, 5, 2.5, True, -1, "2", None):
        with pytest.raises(ValueError, match="num_layers"):
            AudioGRUModel(64, 32, num_layers=bad)
    assert AudioGRUModel(64, 32, True, False, 2).reset_hidden is False          # positional order: bias, reset_hidden, num_layers


def test_gradient_penalty_through_a_stack_is_refused_by_the_trainer():
    """The penalty's reverse sweep covers one recurrence: a trainer asked for it on a stacked GRU raises in its constructor, with the
    reason, before any GPU work; the same request on a single layer is accepted."""
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, linear_score_function
    from cpc_audio_amd.contexts import GRUContext

    def trainer(L):
        enc = AudioEncoder(SMALL)
        model = AudioPredictiveCodingModel(enc, AudioGRUModel(64, 32, num_layers=L), enc_size=64, ar_size=32, visible_steps=8,
                                           prediction_steps=2, compute_dtype="fp32")
        tr = ContrastiveEstimationTrainer(model=model, dataset=None, score_function=linear_score_function, prediction_steps=2, ar_size=32,
                                          wasserstein_gradient_penalty=True, preprocessing=torch.nn.Identity())
        return tr, model
    for L in (2, 4):
        with pytest.raises(NotImplementedError, match="stacked GRU"):
            trainer(L)
    tr, model = trainer(1)
    assert tr.wasserstein_gradient_penalty and model.gradient_penalty_engine
    assert "num_layers > 1" in GRUContext.GP_STACK_REASON


def test_grad_all_reduce_plan_covers_a_three_layer_model_once(tmp_path):
    """GradAllReduce's bucket plan on a three-layer model: the ranges the backward pass reports (everything from encoder layer 3 up,
    which holds the context's twelve tensors, then layer 2) plus finish() tile the flat gradient buffer exactly once."""
    import torch.distributed as dist
    from cpc_audio_amd.engine import GradAllReduce
    enc = AudioEncoder(SMALL)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(64, 32, num_layers=3), enc_size=64, ar_size=32, visible_steps=8, prediction_steps=2)
    model._flatten_parameters("cpu")
    off, total = model._offset, model._flat_grad.numel()
    names = [n for n, _ in model.named_parameters()]
    assert [n for n in names if "upper_cells" in n] == [f"autoregressive_model.upper_cells.{i}.{k}" for i in range(2) for k in GRU_KEYS]
    assert total == sum((p.numel() + 63) // 64 * 64 for p in model.parameters())
    lo_ctx, hi_ctx = off["autoregressive_model.gruCell.weight_ih"], off["prediction_model.weight"]
    assert all(lo_ctx <= off[n] < hi_ctx for n in names if n.startswith("autoregressive_model."))          # one contiguous range
    dist.init_process_group("gloo", init_method="file://" + os.path.join(str(tmp_path), "store"), rank=0, world_size=1)
    try:
        sync = GradAllReduce(model)
        model._flat_grad.fill_(1.0)
        sync.hook(off["encoder.layers.2.weight"], total)          # CPCEngine._backward_encoder at l = 2, then l = 1
        sync.hook(off["encoder.layers.1.weight"], off["encoder.layers.2.weight"])
        sync.finish()
        d = sync.describe()
    finally:
        dist.destroy_process_group()
    assert d["covers_once"], d
    assert d["grad_bytes"] == 4 * total and len(d["buckets"]) == 3
    assert d["buckets"][0]["lo"] <= lo_ctx and d["buckets"][0]["hi"] == total
