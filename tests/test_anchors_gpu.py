"""Prediction anchors on the GPU: cpc_lstm_bwd_steps step by step and cpc_anchor_target_grad on exact data against
tests/anchor_reference.py, whole models (GRU with one and two layers, LSTM; both storage types) against the composed float64
reference, the equivalence with single-anchor steps on shortened clips, the autograd bridge, train / validate / calc_test_task_data,
the target lanes, and the refusals.

Tolerances are the project's own, restated from test_lstm_gpu.py / test_gru_wide_gpu.py / test_model_gpu.py where used; none was
obtained by running the code under test.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import (AudioEncoder, AudioGRUModel, AudioLSTMModel, AudioPredictiveCodingModel,  # noqa: E402
                                       ConvolutionalArModel)
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, linear_score_function,  # noqa: E402
                                                           softplus_score_function)
import anchor_reference as R  # noqa: E402
import lstm_reference as L  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
SCORE = {"softplus": softplus_score_function, "linear": linear_score_function}
GUARD = 64           # sentinel elements behind every output
SENT = -7.5          # (exact in bf16)


def name(dt):
    return "f32" if dt == F32 else "bf16"


def host(t):
    return t.detach().double().cpu()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _rel(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


# ================================================================================================================ cpc_lstm_bwd_steps
def _padded(B, per_item, dt):
    """NaN where the kernel must write, then the sentinel over the rows of the workgroup's masked items and GUARD more elements."""
    n, pad = B * per_item, (-B % 16) * per_item
    buf = torch.full((n + pad + GUARD,), float("nan"), device=DEV, dtype=dt)
    buf[n:] = SENT
    return buf, buf[:n]


def _lstm_tape(dt, B, V, H, ref):
    code = _hip.dtype_code(dt)
    dW = ref["w_hh"].to(DEV).float().contiguous()
    wfrag = torch.empty(4 * H * H, device=DEV, dtype=dt)
    wTfrag = torch.empty(4 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wfrag), 4 * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(dW), _hip.ptr(wTfrag), H, 4 * H, H, 1, code)
    gi = ref["gir"].to(dt).to(DEV).contiguous()
    Hall = torch.empty(B * (V + 1) * H, device=DEV, dtype=dt)
    tape = torch.empty(B * V * 6 * H, device=DEV, dtype=dt)
    h_out, cell_out = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
    _hip.call("cpc_lstm_fwd", _hip.ptr(gi), _hip.ptr(wfrag), _hip.ptr(ref["b_hh"].to(DEV)), None, None, _hip.ptr(Hall), _hip.ptr(tape),
              _hip.ptr(h_out), _hip.ptr(cell_out), B, V, H, code)
    return tape, wTfrag


def _steps_call(dt, B, V, H, tape, wTfrag, dh, dHs, ld_h):
    """cpc_lstm_bwd_steps (or cpc_lstm_bwd when ld_h is None) into a guarded dG; returns dG (B, V, 4H) on the device."""
    code = _hip.dtype_code(dt)
    gb, dG = _padded(B, V * 4 * H, dt)
    if ld_h is None:
        _hip.call("cpc_lstm_bwd", _hip.ptr(dh), _hip.ptr(tape), _hip.ptr(wTfrag), _hip.ptr(dG), B, V, H, code)
    else:
        _hip.call("cpc_lstm_bwd_steps", _hip.ptr(dh), _hip.ptr(dHs), C.c_longlong(ld_h), _hip.ptr(tape), _hip.ptr(wTfrag), _hip.ptr(dG),
                  B, V, H, code)
    torch.cuda.synchronize()
    assert bool((gb[B * V * 4 * H:].float() == SENT).all()), "something was written behind dG or into the rows of items >= B"
    assert bool(torch.isfinite(dG.float()).all())
    return dG.view(B, V, 4 * H)


def _dhs_buffer(dt, B, V, H, ld_h, values):
    """dHs rows at stride ld_h with NaN in the pad columns [H, ld_h) and in the rows of the items B .. 16 ceil(B / 16) - 1."""
    Bp = B + (-B % 16)
    buf = torch.full((Bp, V, ld_h), float("nan"), device=DEV, dtype=dt)
    buf[:B, :, :H] = values.to(dt).to(DEV)
    return buf


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("H", [32, 288])
@pytest.mark.parametrize("dt", [F32, BF16], ids=name)
def test_lstm_bwd_steps_per_step(dt, H, B, V):
    """cpc_lstm_bwd_steps against the float64 sweep with injected gradients, gate block by gate block and step by step: a single item
    and a partial 16-item workgroup, one and three steps, 4 waves (H = 32) and 8 (H = 288); ld_h = H and H + 8 with NaN in the pad
    columns and in the rows of items >= B; dHs dense and non-zero at one step only; dh_last given and NULL.  Bounds of
    test_lstm_fwd_bwd_per_step: f32 5e-5, bf16 4 x the per-step error of the bf16 emulation.  dHs = NULL is cpc_lstm_bwd bit for
    bit.  Nothing is written behind dG."""
    base = R.lstm_steps_reference(dt, B, V, H, "dense", True)
    tape, wTfrag = _lstm_tape(dt, B, V, H, base)
    dh_dev = base["dh"].to(DEV).contiguous()
    plain = _steps_call(dt, B, V, H, tape, wTfrag, dh_dev, None, None)
    same = _steps_call(dt, B, V, H, tape, wTfrag, dh_dev, None, H)          # dHs = NULL through the new entry point
    assert torch.equal(bits(plain), bits(same))
    for mode in ("dense", "one"):
        for with_dh in (True, False):
            ref = R.lstm_steps_reference(dt, B, V, H, mode, with_dh)
            for ld_h in (H, H + 8):
                dHs = _dhs_buffer(dt, B, V, H, ld_h, ref["dHs"])
                dG = _steps_call(dt, B, V, H, tape, wTfrag, dh_dev if with_dh else None, dHs, ld_h)
                bad, worst = R.gate_violations(host(dG), ref)
                print(f"lstm_bwd_steps {name(dt)} H={H} B={B} V={V} {mode} dh={with_dh} ld_h={ld_h}: largest per-step errors",
                      {k: f"{v:.2e}" for k, v in worst.items()})
                assert not bad, (mode, with_dh, ld_h, bad[:6])
            if mode == "dense" and with_dh:
                assert not torch.equal(bits(dG), bits(plain)), "the injected gradients made no difference"


# ============================================================================================================ cpc_anchor_target_grad
def _atg_case(dt, E, A, K, stride, B, rng):
    """One geometry: every (accumulate, row range) against the numpy restatement, bit for bit, sentinels included."""
    code = _hip.dtype_code(dt)
    first = 3
    span = (A - 1) * stride + K
    rows = first + span + 2                                # uncovered rows in front of the first window and behind the last
    item = rows * E + E                                    # ... and E sentinel elements between the items
    guard = 2 * E
    dT = rng.integers(-3, 4, size=(A, B, K, E)).astype(np.float32)          # sums of at most 5 + 1 such integers: exact in bf16
    dT_dev = torch.from_numpy(dT).to(DEV)
    ranges = {(0, rows), (first + K // 2, first + K // 2 + 1), (first + span - 1, rows)}
    if span > 2:
        ranges.add((first + 1, first + span - 1))          # cuts through the first and the last window where K > 1
    if A > 1 and K > 1:
        ranges.add((first + stride + 1, first + stride + 2))          # one row in the middle of the second window
    for accumulate in (0, 1):
        for lo, hi in sorted(ranges):
            init = np.full((B, item // E, E), np.nan, dtype=np.float32)
            if accumulate:
                init[:, lo:hi, :] = rng.integers(-3, 4, size=(B, hi - lo, E))
            whole = torch.full((guard + B * item + guard,), float("nan"), device=DEV, dtype=dt)
            whole[guard:guard + B * item] = torch.from_numpy(init).reshape(-1).to(dt).to(DEV)
            before = whole.clone()
            _hip.call("cpc_anchor_target_grad", _hip.ptr(dT_dev), _hip.ptr(whole, guard), C.c_longlong(item), A, B, K, E, first, stride,
                      lo, hi, accumulate, code)
            torch.cuda.synchronize()
            want = R.anchor_target_grad(dT, init[:, :rows, :], first, stride, lo, hi, accumulate)
            expect = before.clone()
            view = expect[guard:guard + B * item].view(B, item // E, E)
            view[:, lo:hi, :] = torch.from_numpy(want[:, lo:hi, :]).to(dt).to(DEV)
            assert torch.equal(bits(whole), bits(expect)), (A, K, stride, B, E, accumulate, lo, hi)
            got_rows = whole[guard:guard + B * item].view(B, item // E, E)[:, lo:hi, :]
            assert bool(torch.isfinite(got_rows.float()).all())
            if not accumulate:          # uncovered rows of the range are zeros
                for r in range(lo, hi):
                    if not any(0 <= r - first - a * stride < K for a in range(A)):
                        assert bool((got_rows[:, r - lo, :] == 0).all())


@pytest.mark.parametrize("A", [1, 2, 3, 5])
@pytest.mark.parametrize("dt,E", [(BF16, 8), (BF16, 64), (BF16, 72), (F32, 4)], ids=lambda v: name(v) if isinstance(v, torch.dtype) else f"E{v}")
def test_anchor_target_grad_exact(dt, E, A):
    """Small integers (exact in bf16, every sum exact): the result equals the numpy restatement bit for bit — K in {1, 4}, stride in
    {1, K - 1, K, K + 2} (overlapping, tiling and gapped windows), B in {1, 3}, row ranges over the whole item, through the middle of
    windows and of one row, accumulate 0 and 1; uncovered rows are zeros or untouched; the NaN sentinels in every row outside the range,
    in the guard rows and between the items keep their bits."""
    rng = np.random.default_rng(1000 * A + E)
    for K in (1, 4):
        for stride in sorted({1, K, K + 2} | ({K - 1} if K > 1 else set())):
            for B in (1, 3):
                _atg_case(dt, E, A, K, stride, B, rng)


# ======================================================================================================================= whole model
E_S, V_S, K_S, B_S = 64, 12, 4, 8
SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E_S] * 5, 'bias': True}
CONTEXTS = {"gru": ("gru", 1), "gru2": ("gru", 2), "lstm": ("lstm",)}
ANCHORS = [(2, 4), (3, 2), (3, 5), (12, 1)]          # tiling, overlapping, gapped windows; the earliest possible anchor (after one frame)


def _model(context, dtype, H=32, A=1, s=1, V=V_S, seed=3):
    """The small model of test_lstm_gpu.py: 64 channels, encoder weights doubled so that the scores are not degenerate."""
    torch.manual_seed(seed)
    if context == "lstm":
        ar = AudioLSTMModel(E_S, H)
    else:
        ar = AudioGRUModel(E_S, H, num_layers=CONTEXTS[context][1])
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), ar, enc_size=E_S, ar_size=H, visible_steps=V, prediction_steps=K_S,
                                       compute_dtype=dtype, prediction_anchors=A, anchor_stride=s)
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if n.startswith("encoder.") and n.endswith("weight"):
                p_.mul_(2.0)
    return model


def _data(n, seed):
    length = _model("gru", "fp32").item_length
    return torch.randn(n, length, generator=torch.Generator().manual_seed(seed)) * 0.5


class _Meter:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))


class _Logger:
    def __init__(self):
        self.loss_meter, self.score_meter = _Meter(), _Meter()

    def log(self, step):
        pass


def _trainer(model, data, logger, H=32, score_function=softplus_score_function, reg=1.0, **kw):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=reg, score_function=score_function, prediction_steps=K_S, ar_size=H, **kw)
    tr.verbose = False
    return tr


def _one_step(model, data, score="softplus", reg=1.0, H=32):
    """One trainer step with lr 0 (the gradients stay on the parameters): returns the logged loss."""
    logger = _Logger()
    tr = _trainer(model, data, logger, H, SCORE[score], reg)
    assert tr._fused()
    tr.train(batch_size=data.shape[0], epochs=1, lr=0.0, num_workers=0, max_steps=1)
    torch.cuda.synchronize()
    return logger.loss_meter.values[0]


_REFERENCE = {}          # (context, H, A, s, score) -> (loss, grads): computed once, shared by the storage types, never modified


def _reference_step(context, H, A, s, score, params, data):
    key = (context, H, A, s, score)
    if key not in _REFERENCE:
        orc = R.AnchorOracle(params, V_S, K_S, A, s, CONTEXTS[context], score=score, regularization=1.0, lr=0.0)
        loss, _, grads = orc.loss_and_grads(data)
        _REFERENCE[key] = (float(loss), {k: v.detach().clone() for k, v in grads.items()})
    return _REFERENCE[key]


def _check_model(context, dtype, H, A, s):
    data = _data(B_S, 1)
    model = _model(context, dtype, H, A, s).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    eng = model.engine(B_S, data.shape[1])
    assert (eng.A, eng.s, eng.AK) == (A, s, A * K_S)
    worst = {"encoder": 0.0, "context / predictor": 0.0, "loss": 0.0}
    for score in ("softplus", "linear"):
        model.load_state_dict(params)
        got = _one_step(model, data, score, 1.0, H)
        loss, grads = _reference_step(context, H, A, s, score, params, data)
        ltol = 1e-4 if dtype == "fp32" else 1e-2
        worst["loss"] = max(worst["loss"], abs(got - loss) / abs(loss))
        named = dict(model.named_parameters())
        assert set(grads) == set(named)
        errs = {}
        for pname, ref in grads.items():
            group = "encoder" if pname.startswith("encoder.") else "context / predictor"
            errs[pname] = _rel(named[pname].grad, ref)
            worst[group] = max(worst[group], errs[pname])
        print(f"anchors {context} H={H} {dtype} A={A} s={s} {score}: loss {got:.6f} / {loss:.6f}, largest gradient error "
              f"{max(errs.values()):.2e} ({max(errs, key=errs.get)})")
        assert abs(got - loss) <= ltol * abs(loss), (score, got, loss)
        for pname, e in errs.items():
            group = "encoder" if pname.startswith("encoder.") else "context / predictor"
            gtol = 1e-3 if dtype == "fp32" else (0.2 if group == "encoder" else 0.12)
            assert e < gtol, (score, pname, e)
    print(f"anchors {context} H={H} {dtype} A={A} s={s}: worst", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("A,s", ANCHORS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("context", list(CONTEXTS))
def test_anchor_model_loss_and_gradients_against_reference(context, dtype, A, s):
    """One trainer step (lr 0) of the small model with a GRU (one and two layers) or LSTM context, softplus and linear scores,
    regularization 1: the loss and every parameter gradient against the composed float64 reference on the A K stacked heads.  Bounds
    of test_lstm_gpu.py / test_gru_wide_gpu.py: fp32 loss 1e-4, gradients 1e-3 (relative l2); bf16 loss 1e-2, context and predictor
    0.12, encoder 0.2."""
    _check_model(context, dtype, 32, A, s)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_anchor_model_wide_lstm(dtype):
    """The same at H = 288 (the 8-wave LSTM kernels), (A, s) = (3, 2)."""
    _check_model("lstm", dtype, 288, 3, 2)


@pytest.mark.parametrize("context", ["gru", "lstm"])
def test_anchor_loss_is_the_mean_of_single_anchor_steps_on_shortened_clips(context):
    """fp32, regularization 0, (A, s) = (3, 2): the loss equals the mean of three single-anchor trainer steps on the clips shortened
    by d_a * downsampling samples at their end with visible_steps = V - d_a, same weights.  1e-4 relative (the fp32 loss bound)."""
    A, s = 3, 2
    data = _data(B_S, 2)
    model = _model(context, "fp32", 32, A, s).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    ds = model.encoder.downsampling_factor
    for score in ("softplus", "linear"):
        got = _one_step(model, data, score, 0.0)
        singles = []
        for d in R.shifts(A, s):
            one = _model(context, "fp32", 32, 1, 1, V=V_S - d)
            one.load_state_dict(params)
            one = one.to(DEV)
            clip = data[:, :data.shape[1] - d * ds].contiguous()
            assert clip.shape[1] == one.item_length
            singles.append(_one_step(one, clip, score, 0.0))
        mean = sum(singles) / A
        print(f"anchors {context} {score}: stacked loss {got:.6f}, single-anchor losses {singles}, mean {mean:.6f}")
        assert abs(got - mean) <= 1e-4 * abs(mean), (score, got, singles)
        assert max(singles) - min(singles) > 1e-4 * abs(mean), "the anchors do not differ: the check would pass with one of them thrice"


@pytest.mark.parametrize("context", ["gru2", "lstm"])
def test_anchor_bridge_outputs_and_backward(context):
    """model(x): predicted_z (B, A K, E), targets (B, E, A K), z (B, E, V), c = h_V (B, H) against the reference (fp32, 1e-4), and
    backward() of a random linear functional of (predicted_z, targets) against its autograd (gradients 1e-3 relative l2)."""
    A, s, H = 3, 2, 32
    data = _data(B_S, 3)
    model = _model(context, "fp32", H, A, s).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    w_pred, w_targ = torch.randn(B_S, A * K_S, E_S, generator=g), torch.randn(B_S, E_S, A * K_S, generator=g)
    orc = R.AnchorOracle(params, V_S, K_S, A, s, CONTEXTS[context])
    ref_pred, ref_targ, grads = orc.functional_grads(data, w_pred, w_targ)
    pred, targ, z, c = model(data.to(DEV).unsqueeze(1))
    assert pred.shape == (B_S, A * K_S, E_S) and targ.shape == (B_S, E_S, A * K_S) and z.shape == (B_S, E_S, V_S) and c.shape == (B_S, H)
    with torch.no_grad():
        _, _, ref_z, ref_c = orc.forward(data)
    for got, ref, what in ((pred, ref_pred, "predicted_z"), (targ, ref_targ, "targets"), (z, ref_z, "z"), (c, ref_c, "c")):
        assert _rel(got, ref) < 1e-4, what
    ((pred * w_pred.to(DEV)).sum() + (targ * w_targ.to(DEV)).sum()).backward()
    for n, p_ in model.named_parameters():
        e = _rel(p_.grad, grads[n])
        assert e < 1e-3, (n, e)
    # predictions alone, targets alone: the missing gradient is zeros
    for use_pred in (True, False):
        model.zero_grad()
        pred, targ, _, _ = model(data.to(DEV).unsqueeze(1))
        ((pred * w_pred.to(DEV)).sum() if use_pred else (targ * w_targ.to(DEV)).sum()).backward()
        _, _, part = orc.functional_grads(data, w_pred if use_pred else torch.zeros_like(w_pred),
                                          torch.zeros_like(w_targ) if use_pred else w_targ)
        for n, p_ in model.named_parameters():
            if float(part[n].norm()) > 0:
                assert _rel(p_.grad, part[n]) < 1e-3, (use_pred, n)
            else:
                assert float(p_.grad.abs().max()) == 0.0, (use_pred, n)


class _Labelled(torch.utils.data.Dataset):
    def __init__(self, clips):
        self.clips = clips

    def __len__(self):
        return self.clips.shape[0]

    def __getitem__(self, i):
        return self.clips[i], i


def test_anchor_train_validate_and_task_data():
    """Three steps of train() with A = 3 (fp32, softplus, GRU) against three reference Adam steps (oracle.adam_update) from the same
    parameters: losses and parameters within 1e-4 (1 + 4 steps), as the LSTM test.  validate() and calc_test_task_data() of the A = 3
    model equal those of an A = 1 model holding the same weights within 1e-4: they measure the last anchor's K heads and h_V."""
    B, steps, lr, A, s = 4, 3, 2e-4, 3, 2
    data = _data(B, 5)
    model = _model("gru", "fp32", 32, A, s).to(DEV)
    params = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    orc = R.AnchorOracle(params, V_S, K_S, A, s, ("gru", 1), score="softplus", regularization=1.0, lr=lr)
    want = [orc.step(data)[0] for _ in range(steps)]
    val = _data(16, 6)
    logger = _Logger()
    tr = _trainer(model, data, logger, validation_set=TensorAudioDataset(val, device=DEV), test_task_set=_Labelled(val[:8]))
    tr.train(batch_size=B, epochs=steps, lr=lr, num_workers=0, max_steps=steps)
    got = logger.loss_meter.values
    assert len(got) == steps
    for i in range(steps):
        assert abs(got[i] - want[i]) <= 1e-4 * abs(want[i]) * (1 + 4 * i), (i, got, want)
    for k, v in model.state_dict().items():
        assert _rel(v, orc.params[k]) < 1e-4 * (1 + 4 * steps), k
    one = _model("gru", "fp32", 32, 1, 1)
    one.load_state_dict({k: v.detach().clone().cpu() for k, v in model.state_dict().items()})
    one = one.to(DEV)
    tr1 = _trainer(one, data, _Logger(), validation_set=TensorAudioDataset(val, device=DEV), test_task_set=_Labelled(val[:8]))
    v3, v1 = tr.validate(batch_size=8, num_workers=0), tr1.validate(batch_size=8, num_workers=0)
    assert len(v3[0]) == K_S
    for a, b in ((v3[0], v1[0]), (v3[1], v1[1]), (v3[3], v1[3])):
        assert (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max().item() < 1e-4
    assert abs(v3[2] - v1[2]) < 1e-4 * max(1.0, abs(v1[2]))
    # ... and the reference's numbers for the last anchor
    from oracle import cpc_oracle as O
    lists = O.file_batch_sampler([val.shape[0]], 8, 8, True, seed=0)
    want_l = sum(orc.validation(val[idx])[0] for idx in lists) / len(lists)
    assert _rel(v3[0], want_l) < 1e-4 * (1 + 4 * steps)
    t3, l3 = tr.calc_test_task_data(batch_size=4, num_workers=0)
    t1, l1 = tr1.calc_test_task_data(batch_size=4, num_workers=0)
    assert list(l3) == list(l1) == list(range(8))
    assert float(np.abs(t3 - t1).max()) < 1e-4 * max(1.0, float(np.abs(t1).max()))


def test_anchor_target_lanes_equal_the_single_lane_step():
    """The shape of test_target_lanes_equal_the_single_lane_step (bf16, default encoder, 64 clips of 20480 samples) with A = 4, s = 5:
    the target windows reach below row T - K and into the rows >= T - K that both lanes start from.  Both lanes are active with
    anchors; the step with them equals the step with one launch per layer within that test's bounds (loss 1e-6, gradients 1e-3 of
    each parameter's largest element)."""
    B, Lc = 64, 20480
    x = (torch.randn(B, Lc, generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, compute_dtype="bf16",
                                       prediction_anchors=4, anchor_stride=5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "encoder" in n and n.endswith("weight"):
                p.mul_(2.0)
    model.to(DEV)
    eng = model.engine(B, Lc)
    assert eng.A == 4 and eng._target_lane_rows() is not None and eng._bwd_lane() is not None, "both lanes are expected with anchors"
    lanes = {"both": (eng._tl_rows, eng._bl), "none": (None, None)}
    got = {}
    for lane, (rows, bl) in lanes.items():
        eng._tl_rows, eng._bl = rows, bl
        for _ in range(2):
            out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        got[lane] = (float(out[0]), model._flat_grad.detach().double().cpu().clone())
    ref_loss, ref = got["none"]
    loss, grad = got["both"]
    assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss), (loss, ref_loss)
    assert torch.isfinite(grad).all()
    for pname, g in model._grad.items():
        lo = model._offset[pname]
        a, b = grad[lo:lo + g.numel()], ref[lo:lo + g.numel()]
        assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item() + 1e-12, pname


# ========================================================================================================================= refusals
@contextlib.contextmanager
def _no_launch(monkeypatch):
    """Fails the test if anything is launched through the binding inside the block."""
    calls = []
    with monkeypatch.context() as m:
        for fn in ("call", "gemm_nt", "gemm_tn"):
            m.setattr(_hip, fn, lambda *a, _fn=fn, **k: calls.append((_fn, a[:1])))
        yield
    assert not calls, calls


def test_contexts_without_hidden_states_refuse_anchors_before_any_launch(monkeypatch):
    """ConvolutionalArModel, AttentionModel and the scalogram engine expose c at the last position only: with A > 1 engine
    construction raises NotImplementedError naming the reason, and nothing has been launched by then.  The engine itself refuses
    the loss options that are not stacked over anchors, before its forward pass."""
    from cpc_audio_amd import configs
    from cpc_audio_amd.attention_model import AttentionModel
    from cpc_audio_amd.scalogram_model import ScalogramResidualEncoder

    def conv_ar():
        return ConvolutionalArModel(configs.fresh(configs.ar_conv_default_dict))

    def attention():
        cfg = configs.fresh(configs.attention_architecture_1)
        cfg["dropout"] = 0.0
        return AttentionModel(cfg)
    for make, E in ((conv_ar, 256), (attention, 512)):
        enc_cfg = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [64, 64, 64, 64, E], 'bias': True}
        model = AudioPredictiveCodingModel(AudioEncoder(dict(enc_cfg)), make(), enc_size=E, ar_size=256, visible_steps=60,
                                           prediction_steps=4, compute_dtype="bf16", prediction_anchors=2, anchor_stride=3).to(DEV)
        with _no_launch(monkeypatch), pytest.raises(NotImplementedError, match="last position only"):
            model.engine(2, model.item_length)
    enc = ScalogramResidualEncoder(configs.fresh(configs.scalogram_resnet_architecture_1))
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=60, prediction_steps=4,
                                       prediction_anchors=2, anchor_stride=3).to(DEV)
    with _no_launch(monkeypatch), pytest.raises(NotImplementedError, match="last position only"):
        model.engine(2, (2, 216, 200))
    # the loss options the engine itself refuses with anchors
    model = _model("gru", "fp32", 32, 2, 2).to(DEV)
    eng = model.engine(B_S, model.item_length)
    x = _data(B_S, 1).to(DEV)
    with _no_launch(monkeypatch):
        for kw in (dict(all_timesteps=True), dict(score="difference"), dict(negatives=(2, 1, 0))):
            with pytest.raises(NotImplementedError, match="prediction_anchors"):
                eng.loss_and_grads(x, softplus=True, regularization=1.0, **kw)
