"""LSTM context (AudioLSTMModel), host side: the float64 reference of tests/lstm_reference.py against torch's nn.LSTMCell under
autograd, the cap on the bf16 emulation's error for every kernel case of test_lstm_gpu.py, the sensitivity of the per-step verdict to a
dropped cell carry and to swapped gate blocks, the argument checks of cpc_lstm_tape_elems / cpc_lstm_fwd / cpc_lstm_bwd (the library
loads on a CPU host; the pointers are never dereferenced), the model surface and the trainer's refusal of the gradient penalty.  No
device is touched.
"""
import ctypes as C

import pytest
import torch

import lstm_reference as L
from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioLSTMModel, AudioPredictiveCodingModel

SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64] * 5, 'bias': True}


@pytest.mark.parametrize("with_state", [False, True])
def test_reference_against_lstm_cell_autograd(with_state):
    """lstm_run against float64 torch.nn.LSTMCell under autograd to 1e-12: hidden states, last pair, and dG = the gradient with respect
    to Gi, which enters the pre-activations additively."""
    B, V, H = 3, 6, 16
    w, b, Gi, dh, h0, c0 = (None if t is None else t.double() for t in L.lstm_data(B, V, H, seed=5, with_state=with_state))
    hall, hV, cV, dG = L.lstm_run(Gi, w, b, dh, h0, c0)
    hall_t, hV_t, cV_t, dG_t = L.lstm_cell_autograd(Gi, w, b, dh, h0, c0)
    assert (hall - hall_t).abs().max() < 1e-12 and (hV - hV_t).abs().max() < 1e-12 and (cV - cV_t).abs().max() < 1e-12
    assert L.rel_err(dG, dG_t) < 1e-12
    assert torch.equal(hall[:, -1], hV)


def test_model_reference_is_the_cell_loop():
    """lstm_model_reference (what the route tests differentiate) against nn.LSTMCell with the same parameters, float64."""
    B, E, V, H = 3, 8, 5, 16
    torch.manual_seed(3)
    cell = torch.nn.LSTMCell(E, H).double()
    z = torch.randn(B, E, V, dtype=torch.float64)
    h = c = torch.zeros(B, H, dtype=torch.float64)
    for t in range(V):
        h, c = cell(z[:, :, t], (h, c))
    hV, cV = L.lstm_model_reference(z, dict(cell.named_parameters()))
    assert (hV - h).abs().max() < 1e-12 and (cV - c).abs().max() < 1e-12


@pytest.mark.parametrize("case", [c for c in L.lstm_cases() if c[1] == L.BF16], ids=L.lstm_case_id)
def test_emulation_stays_below_the_cap(case):
    """A condition on the inputs, not a measurement: the bf16 emulation alone is below 2e-2 at every step of every case."""
    _, dt, H, B, V = case
    ref = L.lstm_reference(dt, B, V, H, with_state=L.lstm_case_state(case))
    worst = max(float(v.max()) for v in ref["e_model"].values())
    print(f"{L.lstm_case_id(case)}: emulation's largest per-step error {worst:.2e}")
    assert worst < L.LSTM_MODEL_CAP


@pytest.mark.parametrize("mutation", ["drop_cell_carry", "swap_fg"])
def test_per_step_verdict_sees_deliberate_mistakes(mutation):
    """Each mutation violates the per-step verdict in the long case, in both storage types' bounds.  The dropped carry leaves the last
    three steps exact, where the gradients are largest: a per-tensor maximum hides it."""
    for dt in (L.F32, L.BF16):
        ref = L.lstm_reference(dt, 7, 40, 64)
        rnd = L.ident if dt == L.F32 else L.to_bf16
        hall, _, _, dG = L.lstm_run(ref["gir"], ref["wr"], ref["br"], ref["dhr"], rnd=rnd, mutation=mutation)
        errs = L.lstm_step_errors(hall, dG, ref["hall"], ref["dG"])
        bad = L.lstm_violations(errs, ref["tol"])
        assert bad, f"{mutation} passes the per-step verdict"
        if mutation == "drop_cell_carry":
            assert all(t < 40 - 3 for _, t, _, _ in bad) and all(k != "Hall" for k, _, _, _ in bad)
            H = 64
            assert all(L.rel_err(dG[:, -3:, i * H:(i + 1) * H], ref["dG"][:, -3:, i * H:(i + 1) * H]) <= float(ref["tol"][k][-3:].max())
                       for i, k in enumerate(L.LSTM_BLOCKS[1:]))


def test_model_surface():
    """state_dict keys and shapes are nn.LSTMCell's under ``lstmCell``; initial values are nn.LSTMCell's under the same seed and
    construction order; a GRU model is what it was."""
    torch.manual_seed(11)
    ar = AudioLSTMModel(64, 32)
    torch.manual_seed(11)
    cell = torch.nn.LSTMCell(64, 32)
    assert [n for n, _ in ar.named_parameters()] == ["lstmCell." + n for n, _ in cell.named_parameters()]
    for (n, p), (_, q) in zip(ar.named_parameters(), cell.named_parameters()):
        assert p.shape == q.shape and torch.equal(p, q), n
    assert ar.lstmCell.weight_ih.shape == (128, 64) and ar.lstmCell.weight_hh.shape == (128, 32)
    assert ar.hidden is None and ar.reset_hidden is True
    nb = AudioLSTMModel(64, 32, bias=False)
    assert [n for n, _ in nb.named_parameters()] == ["lstmCell.weight_ih", "lstmCell.weight_hh"]
    with pytest.raises(TypeError):
        AudioLSTMModel(64, 32, num_layers=2)
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), ar, enc_size=64, ar_size=32, visible_steps=8, prediction_steps=2)
    keys = [k for k in model.state_dict() if k.startswith("autoregressive_model.")]
    assert keys == ["autoregressive_model.lstmCell." + n for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    # AudioGRUModel-based models: same keys and values as nn.GRUCell gives them
    torch.manual_seed(12)
    gru = AudioGRUModel(64, 32)
    torch.manual_seed(12)
    gcell = torch.nn.GRUCell(64, 32)
    assert [n for n, _ in gru.named_parameters()] == ["gruCell." + n for n, _ in gcell.named_parameters()]
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(gru.named_parameters(), gcell.named_parameters()))


def test_argument_checks_come_before_any_launch():
    """Every CPC_EINVAL precondition of cpc_lstm_tape_elems, cpc_lstm_fwd and cpc_lstm_bwd, with pointers that are never dereferenced."""
    lib = _hip.lib()
    P, s = C.c_void_p(0x1000), C.c_void_p(0)
    f32, bf16 = _hip.F32, _hip.BF16
    assert lib.cpc_lstm_tape_elems(3, 5, 32, bf16) == 3 * 5 * 6 * 32
    assert lib.cpc_lstm_tape_elems(3, 5, 16, f32) == 3 * 5 * 6 * 16

    def fwd(Gi=P, W=P, Hall=P, tape=P, h_out=P, cell_out=P, B=2, V=3, H=32, dt=bf16, bhh=None, h0=None, c0=None):
        return lib.cpc_lstm_fwd(Gi, W, bhh, h0, c0, Hall, tape, h_out, cell_out, B, V, H, dt, s)

    def bwd(dh=P, tape=P, WT=P, dG=P, B=2, V=3, H=32, dt=bf16):
        return lib.cpc_lstm_bwd(dh, tape, WT, dG, B, V, H, dt, s)

    for name in ("Gi", "W", "Hall", "tape", "h_out", "cell_out"):
        assert fwd(**{name: None}) == -22, name
    for name in ("dh", "tape", "WT", "dG"):
        assert bwd(**{name: None}) == -22, name
    bad_shapes = [dict(B=0), dict(B=-1), dict(V=0), dict(H=0), dict(H=-32), dict(H=40), dict(H=48), dict(H=16), dict(H=528), dict(H=544),
                  dict(H=1024), dict(dt=2), dict(dt=-1), dict(H=8, dt=f32), dict(H=24, dt=f32), dict(H=528, dt=f32)]
    for kw in bad_shapes:
        assert fwd(**kw) == -22, kw
        assert bwd(**kw) == -22, kw
        assert lib.cpc_lstm_tape_elems(kw.get("B", 2), kw.get("V", 3), kw.get("H", 32), kw.get("dt", bf16)) == -22, kw


def test_gradient_penalty_through_an_lstm_is_refused_by_the_trainer():
    """The LSTM has no tangent recurrence: a trainer asked for the penalty raises in its constructor, with the reason, before any GPU
    work, and leaves the model unmarked."""
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, linear_score_function
    from cpc_audio_amd.contexts import Context, LSTMContext
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), AudioLSTMModel(64, 32), enc_size=64, ar_size=32, visible_steps=8,
                                       prediction_steps=2, compute_dtype="fp32")
    with pytest.raises(NotImplementedError, match="gradient penalty through an AudioLSTMModel"):
        ContrastiveEstimationTrainer(model=model, dataset=None, score_function=linear_score_function, prediction_steps=2, ar_size=32,
                                     wasserstein_gradient_penalty=True, preprocessing=torch.nn.Identity())
    assert not getattr(model, "gradient_penalty_engine", False)
    assert LSTMContext.tangent is Context.tangent and LSTMContext.gp_grads is Context.gp_grads
    tr = ContrastiveEstimationTrainer(model=model, dataset=None, score_function=linear_score_function, prediction_steps=2, ar_size=32)
    assert not tr.wasserstein_gradient_penalty
