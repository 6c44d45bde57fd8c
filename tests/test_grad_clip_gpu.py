"""Gradient clipping by global norm on the HIP path: cpc_grad_norm against float64 at the bound of its own summation order,
non-finite gradients and the NaN-guard pair, cpc_adam_clip against a float64 Adam and against cpc_adam, FusedAdam(max_grad_norm=...)
and ContrastiveEstimationTrainer.max_grad_norm against the CPU oracle model with torch.nn.utils.clip_grad_norm_ + torch.optim.Adam,
and the unclipped step, which must not reach any of the new entry points."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.attention_model import AttentionModel
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel, ConvolutionalArModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, softplus_score_function
from cpc_audio_amd.engine import FusedAdam
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
L, F = C.c_longlong, C.c_float
SENTINEL = -8192.0
NEW_ENTRY_POINTS = {"cpc_grad_norm", "cpc_adam_clip", "cpc_grad_norm_workspace_floats"}

# ------------------------------------------------------------------------------------------ launch geometry of cpc_grad_norm
# (csrc/pointwise.hip) a workgroup of 256 threads takes GN_CHAIN 16-byte loads per thread = 8 192 consecutive floats and writes one
# partial; one workgroup then adds the partials.  Roundings on the longest path from one element to the sum of squares:
#   2            x = g * grad_scale is rounded once and enters as x * x
#   GN_CHAIN     the thread's chain acc = fma(x, x, acc)
#   2            (acc0 + acc1) + (acc2 + acc3)
#   1            a scalar-tail element added to one thread's sum
#   6 + 2        xor-shuffle tree over the 64 lanes, (w0 + w1) + (w2 + w3) over the four waves
#   ceil(workgroups / 256) + 6 + 2     second launch: a thread's chain over the partials, then the same trees
# Every term is a square, so the sum's relative error is at most (roundings) * 2^-24 (to first order); the square root halves it and
# adds half an ulp of its own, which stays below the same number.
GN_CHAIN, GN_THREADS = 8, 256
GN_TILE = GN_THREADS * GN_CHAIN * 4


def gn_workgroups(n):
    return max(1, -(-(n // 4) // (GN_THREADS * GN_CHAIN)))


def gn_bound(n):
    roundings = 2 + GN_CHAIN + 2 + 1 + 6 + 2 + -(-gn_workgroups(n) // 256) + 6 + 2
    return roundings * 2.0 ** -24


def _guarded(n, fill=0.0, tail=64):
    whole = torch.full((n + tail,), SENTINEL, device=DEV, dtype=torch.float32)
    whole[:n] = fill
    return whole[:n], whole


def _intact(*wholes, tail=64):
    return all(bool((w[-tail:] == SENTINEL).all()) for w in wholes)


def _grad_norm(g, scale, max_norm, pair=None):
    """One cpc_grad_norm call: (state as float32 numpy[4], guards intact)."""
    n = g.numel()
    nws = int(_hip.lib().cpc_grad_norm_workspace_floats(L(n)))
    assert nws == gn_workgroups(n)
    ws, ws_whole = _guarded(nws)
    state, st_whole = _guarded(4)
    _hip.call("cpc_grad_norm", _hip.ptr(g), L(n), F(scale), F(max_norm), _hip.ptr(ws), _hip.ptr(state), _hip.ptr(pair))
    torch.cuda.synchronize()
    return state.cpu().numpy().copy(), _intact(ws_whole, st_whole)


def _coef32(max_norm, norm32):
    """float32 evaluation of min(1, max_norm / (norm + 1e-6))."""
    return min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6)))


# ------------------------------------------------------------------------------------------ 1. the norm against float64
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [4, 7, 1023, 1024, 256 * 1024 + 5, 3 * 2 ** 20 + 1])
def test_grad_norm_against_float64(n, scale):
    assert gn_bound(n) < 1e-5
    gen = torch.Generator().manual_seed(n)
    host = torch.randn(n, generator=gen) * 0.37
    g, g_whole = _guarded(n)
    g.copy_(host)
    ref = float((host.double() * scale).norm())
    for max_norm in (0.5 * ref, 2.0 * ref):
        st, ok = _grad_norm(g, scale, max_norm)
        assert ok and _intact(g_whole)
        rel = abs(float(st[0]) - ref) / ref
        print(f"cpc_grad_norm n={n} scale={scale}: rel {rel:.3e} (bound {gn_bound(n):.3e}, {gn_workgroups(n)} workgroups)")
        assert rel <= gn_bound(n), (n, rel, gn_bound(n))
        assert st[1] == _coef32(max_norm, st[0]), (st, max_norm)
        assert (st[1] < 1.0) == (max_norm < ref)
        assert st[2] == 0.0 and st[3] == np.float32(max_norm)
        again, _ = _grad_norm(g, scale, max_norm)
        assert st.tobytes() == again.tobytes()


# ------------------------------------------------------------------------------------------ 2. non-finite gradients
def test_non_finite_gradient_raises_the_pair_and_stops_adam():
    n = 2 * GN_TILE + 7                                    # three workgroups, a partial last one, three scalar-tail elements
    host = torch.randn(n, generator=torch.Generator().manual_seed(2)) * 0.1
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(3))
    for pos in (0, 4 * (n // 4) - 1, n - 2, n - 1):       # first, last of the vector body, inside the scalar tail, last
        for bad in (float("nan"), float("inf"), float("-inf")):
            g = host.clone()
            g[pos] = bad
            g = g.to(DEV)
            pair, pair_whole = _guarded(2)
            st, ok = _grad_norm(g, 1.0, 1.0, pair)
            assert ok and _intact(pair_whole)
            assert st[2] == 1.0 and st[1] == 0.0 and not math.isfinite(float(st[0])), (pos, bad, st)
            assert pair.tolist() == [1.0, 1.0], (pos, bad)
            # a following update with the pair's second float (the sticky flag) as `skip` changes nothing
            state = torch.from_numpy(st).to(DEV)
            p, m, v = p0.to(DEV), torch.full((n,), 0.25, device=DEV), torch.full((n,), 0.5, device=DEV)
            before = [t.clone() for t in (p, m, v)]
            _hip.call("cpc_adam_clip", _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), L(n), F(1e-3), F(0.9), F(0.999), F(1e-8), 1,
                      F(1.0), _hip.ptr(state, 1), _hip.ptr(pair, 1))
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v))), (pos, bad)
    # an element whose square overflows float32 counts as non-finite (torch's float32 norm of it is inf as well)
    g = host.clone()
    g[5] = 3e19
    assert not math.isfinite(float(g.norm()))
    st, _ = _grad_norm(g.to(DEV), 1.0, 1.0)
    assert st[2] == 1.0 and st[1] == 0.0
    # finite data leave the pair alone, whatever it holds
    g = host.to(DEV)
    for preset in (0.0, SENTINEL):
        pair, pair_whole = _guarded(2, preset)
        st, ok = _grad_norm(g, 1.0, 1.0, pair)
        assert ok and st[2] == 0.0 and pair.tolist() == [preset, preset] and _intact(pair_whole)


# ------------------------------------------------------------------------------------------ 3. the clipped Adam
def _adam_args(p, g, m, v, step, scale):
    return (_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), L(p.numel()), F(1e-3), F(0.9), F(0.999), F(1e-8), step, F(scale))


@pytest.mark.parametrize("n", [8192, 10007])          # without and with a scalar tail
def test_adam_clip_against_float64_adam(n):
    """Three steps of cpc_grad_norm + cpc_adam_clip against Adam in float64 on the clipped gradients, at cpc_adam's own tolerance
    (tests/test_hip_kernels.py test_adam_matches_torch: 2e-6 absolute on the parameters)."""
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    ws = torch.empty(gn_workgroups(n), device=DEV)
    state = torch.zeros(4, device=DEV)
    scale, lr, b1, b2, eps = 0.5, 1e-3, 0.9, 0.999, 1e-8
    for step in range(1, 4):
        grad = torch.randn(n, generator=gen) * 2.0
        g64 = grad.double() * scale
        norm = float(g64.norm())
        max_norm = norm * (0.3 if step != 2 else 1.5)          # clipped, not clipped, clipped
        g64 = g64 * min(1.0, max_norm / (norm + 1e-6))
        m64 = b1 * m64 + (1 - b1) * g64
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        p64 = p64 - (lr / (1 - b1 ** step)) * m64 / (v64.sqrt() / math.sqrt(1 - b2 ** step) + eps)
        dg = grad.to(DEV)
        _hip.call("cpc_grad_norm", _hip.ptr(dg), L(n), F(scale), F(max_norm), _hip.ptr(ws), _hip.ptr(state), None)
        _hip.call("cpc_adam_clip", *_adam_args(p, dg, m, v, step, scale), _hip.ptr(state, 1), None)
        assert (float(state[1]) < 1.0) == (step != 2)
        assert (p.double().cpu() - p64).abs().max().item() < 2e-6, step
    assert (m.double().cpu() - m64).abs().max().item() < 2e-6 and (v.double().cpu() - v64).abs().max().item() < 2e-6


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [8192, 10007])
def test_adam_clip_with_coefficient_one_is_cpc_adam(n, scale):
    """coef[0] == 1.0f: (g * grad_scale) * 1 is exact, so parameters and moments carry cpc_adam's bits (grad_scale 1 and 1/2, the
    scales of a single process and of two ranks: products g * grad_scale that are themselves exact, see include/cpc_hip.h)."""
    gen = torch.Generator().manual_seed(7 * n)
    p0, m0, v0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01
    one = torch.ones(1, device=DEV)
    a = [t.to(DEV) for t in (p0, m0, v0)]
    b = [t.to(DEV) for t in (p0, m0, v0)]
    for step in range(1, 4):
        dg = (torch.randn(n, generator=gen) * 3.0).to(DEV)
        _hip.call("cpc_adam", *_adam_args(a[0], dg, a[1], a[2], step, scale), None)
        _hip.call("cpc_adam_clip", *_adam_args(b[0], dg, b[1], b[2], step, scale), _hip.ptr(one), None)
        for x, y, name in zip(a, b, "pmv"):
            assert torch.equal(x, y), (name, step)
    # ... and cpc_grad_norm writes exactly 1.0 when max_norm is far above the norm
    st, _ = _grad_norm(dg, scale, 1e30)
    assert st[1] == 1.0 and st[2] == 0.0
    # a raised skip flag: nothing changes
    flag = torch.ones(1, device=DEV)
    before = [t.clone() for t in b]
    _hip.call("cpc_adam_clip", *_adam_args(b[0], dg, b[1], b[2], 4, scale), _hip.ptr(one), _hip.ptr(flag))
    assert all(torch.equal(x, y) for x, y in zip(before, b))


# ------------------------------------------------------------------------------------------ engine / trainer against the oracle
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def _fixture(golden_dir, context):
    """(meta, data, state, build(dtype), oracle keywords) for the small model with a GRU, convolutional or attention context."""
    name = {"gru": "small_model", "conv": "conv_ar_model", "attention": "attention_model"}[context]
    g = _load(golden_dir, name + ".npz")
    meta = json.load(open(os.path.join(golden_dir, name + ".json")))
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    C_, H, K, V = meta["C"], meta["H"], meta["K"], meta["V"]

    def build(dtype):
        enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
        if context == "gru":
            ar = AudioGRUModel(input_size=C_, hidden_size=H)
        elif context == "conv":
            ar = ConvolutionalArModel(dict(meta["ar"], activation_register=None))
        else:
            ar = AttentionModel(meta["ar"])
        model = AudioPredictiveCodingModel(enc, ar, enc_size=C_, ar_size=H, visible_steps=V, prediction_steps=K, compute_dtype=dtype)
        model.load_state_dict(state)
        return model.to(DEV)

    okw = {}
    if context == "conv":
        okw = {"conv_ar": meta["ar"]}
    elif context == "attention":
        okw = {"attention": (meta["ar"]["num_layers"], meta["ar"]["num_heads"])}
    return meta, torch.from_numpy(g["data"]), state, build, okw


class _Meter:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))


class _Logger:
    def __init__(self, grad_norm=True):
        self.loss_meter, self.score_meter, self.steps = _Meter(), _Meter(), []
        if grad_norm:
            self.grad_norm_meter = _Meter()

    def log(self, step):
        self.steps.append(step)


class _Spy:
    """Records the entry-point names that go through _hip.call while active."""

    def __enter__(self):
        self.names, self.real = [], _hip.call

        def spy(name, *a, **kw):
            self.names.append(name)
            return self.real(name, *a, **kw)

        _hip.call = spy
        return self

    def __exit__(self, *exc):
        _hip.call = self.real


REG, LR, STEPS, SEED = 0.5, 1e-3, 3, 5
_ORACLE = {}


def _batches(data, B, seed=SEED):
    random.seed(seed)
    return [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)]


def _oracle_run(golden_dir, context):
    """The oracle model for STEPS steps with torch.nn.utils.clip_grad_norm_ + torch.optim.Adam, max_grad_norm = half its own
    first-step gradient norm; computed once per context and shared: (max_grad_norm, losses, norms before clipping, parameters)."""
    if context not in _ORACLE:
        meta, data, state, _, okw = _fixture(golden_dir, context)
        batches = _batches(data, meta["B"])
        ot = O.OracleTrainer(state, meta["V"], meta["K"], score="softplus", regularization=REG, lr=LR, **okw)
        plist = list(ot.params.values())
        _, _, grads = ot.loss_and_grads(data[batches[0]])
        max_norm = 0.5 * float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values())))
        opt = torch.optim.Adam(plist, lr=LR)
        losses, norms = [], []
        for i in range(STEPS):
            loss, _, _ = ot.loss_and_grads(data[batches[i]])
            norms.append(float(torch.nn.utils.clip_grad_norm_(plist, max_norm)))
            opt.step()
            losses.append(float(loss))
        _ORACLE[context] = (max_norm, losses, norms, {k: p.detach().clone() for k, p in ot.params.items()})
    return _ORACLE[context]


def _gradient_is_not_identically_zero(name, ref):
    """Mask of the elements the 97 % criterion below counts.  The key bias of an attention layer (the middle third of in_proj_bias)
    shifts every score of a query by the same q . b_k, which softmax does not see: its exact gradient is zero, both sides hold
    rounding noise there, and Adam divides that noise by its own size — the element moves by up to lr per step in a direction no
    reference fixes.  Those elements are held to Adam's bound and to the tensor's relative L2 only."""
    mask = torch.ones_like(ref, dtype=torch.bool)
    if name.endswith("self_attn.in_proj_bias"):
        third = ref.numel() // 3
        mask[third:2 * third] = False
    return mask


def _check_against_oracle(context, model, losses, norms, oracle):
    """The f32 bounds of the unclipped comparison of these fixtures (tests/test_model_gpu.py test_small_model_train_matches_reference):
    loss 1e-4 (times 1 + 2 i at step i), gradients — here their norm — 1e-3, parameters: Adam's bound on every element, 97 % of them
    within 0.05 lr steps + 1e-4 |ref|, and 1e-3 in relative L2.  Every figure is printed before anything is asserted."""
    max_norm, o_losses, o_norms, o_params = oracle
    sd = model.state_dict()
    rows = []
    for k, ref in o_params.items():
        got = sd[k].cpu()
        err = (got - ref).abs()
        tight = (err <= 0.05 * LR * STEPS + 1e-4 * ref.abs())[_gradient_is_not_identically_zero(k, ref)].float().mean().item()
        l2 = ((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-30)).item()
        rows.append((k, err.max().item(), tight, l2))
    print(f"{context}: max_grad_norm {max_norm:.6g}\n  losses {losses}\n  oracle {o_losses}\n  norms  {norms}\n  oracle {o_norms}")
    for k, worst, tight, l2 in rows:
        print(f"  {k}: max |err| {worst:.3e}, tight fraction {tight:.4f}, rel L2 {l2:.3e}")
    for i in range(STEPS):
        assert abs(losses[i] - o_losses[i]) <= 1e-4 * abs(o_losses[i]) * (1 + 2 * i), (context, i, losses, o_losses)
        assert abs(norms[i] - o_norms[i]) <= 1e-3 * o_norms[i], (context, i, norms, o_norms)
    for k, worst, tight, l2 in rows:
        assert worst <= 2 * LR * STEPS * 1.01 + 1e-6, k
        assert tight > 0.97, (k, tight)
        assert l2 < 1e-3, (k, l2)


def _engine_steps(model, data, batches, max_grad_norm, steps=STEPS):
    """The fused step by hand, as train() issues it: (optimizer, losses, clip_state rows)."""
    model.train()
    model._flatten_parameters(DEV)
    opt = FusedAdam(model, lr=LR, max_grad_norm=max_grad_norm)
    model.link_grads()
    dev_data = data.to(DEV)
    losses, states = [], []
    for i in range(steps):
        x = dev_data[torch.as_tensor(batches[i], device=DEV)].contiguous()
        eng = model.engine(x.shape[0], x.shape[1], DEV)
        if i == 0:
            eng.nan_flag().zero_()
        opt.after_update = eng.prepare_ahead
        opt.skip_flag = eng.nan_flag()
        if max_grad_norm is not None:
            opt.nan_pair = eng.nan_pair()
        out = eng.loss_and_grads(x, softplus=True, regularization=REG, all_timesteps=False, grad_ready_hook=opt.hook,
                                 global_negatives=None, after_loss=None, score="softplus")
        opt.step(grad_scale=1.0)
        losses.append(float(out[0]))
        if max_grad_norm is not None:
            states.append(opt.clip_state.cpu().numpy().copy())
    torch.cuda.synchronize()
    return opt, losses, states


def _trainer(model, data, meta, logger):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=REG, score_function=softplus_score_function, prediction_steps=meta["K"],
                                      ar_size=meta["H"])
    tr.verbose = False
    return tr


@pytest.mark.parametrize("context", ["gru", "conv", "attention"])
def test_engine_clipped_steps_against_oracle(golden_dir, context):
    """eng.loss_and_grads + FusedAdam(max_grad_norm=...) for three steps: one cpc_grad_norm and one cpc_adam_clip per step and no
    cpc_adam; the clip is active on step 1; losses, norms before clipping and parameters against the clipped oracle."""
    meta, data, state, build, _ = _fixture(golden_dir, context)
    oracle = _oracle_run(golden_dir, context)
    model = build("fp32")
    with _Spy() as spy:
        opt, losses, states = _engine_steps(model, data, _batches(data, meta["B"]), oracle[0])
    assert spy.names.count("cpc_grad_norm") == STEPS and spy.names.count("cpc_adam_clip") == STEPS and "cpc_adam" not in spy.names
    assert states[0][1] < 1.0 and abs(states[0][1] - 0.5) < 1e-3
    for st in states:
        assert st[1] == _coef32(oracle[0], st[0]) and st[2] == 0.0 and st[3] == np.float32(oracle[0])
    assert opt.t == STEPS
    _check_against_oracle(context, model, losses, [float(st[0]) for st in states], oracle)


@pytest.mark.parametrize("context", ["gru", "conv", "attention"])
def test_trainer_clipped_steps_against_oracle(golden_dir, context):
    """The same through ContrastiveEstimationTrainer.train: logger.grad_norm_meter receives the three norms in step order and
    last_grad_norm holds the latest."""
    meta, data, state, build, _ = _fixture(golden_dir, context)
    oracle = _oracle_run(golden_dir, context)
    model = build("fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    tr.max_grad_norm = oracle[0]
    assert tr.last_grad_norm is None
    random.seed(SEED)
    with _Spy() as spy:
        ret = tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, max_steps=STEPS)
    assert ret is None and tr.training_step == STEPS and logger.steps == list(range(STEPS))
    assert spy.names.count("cpc_grad_norm") == STEPS and spy.names.count("cpc_adam_clip") == STEPS and "cpc_adam" not in spy.names
    norms = logger.grad_norm_meter.values
    assert len(norms) == STEPS and tr.last_grad_norm == norms[-1]
    assert float(tr.last_optimizer.clip_state[0]) == norms[-1]
    assert norms[0] > oracle[0]                                   # the clip was active on step 1
    _check_against_oracle(context, model, logger.loss_meter.values, norms, oracle)


def test_bf16_clipped_step(golden_dir):
    """bf16 storage: the norm before clipping within the fixture's bf16 gradient bound (0.12 relative, tests/test_model_gpu.py) of
    the oracle's, and the clip applied."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    oracle = _oracle_run(golden_dir, "gru")
    opt, losses, states = _engine_steps(build("bf16"), data, _batches(data, meta["B"]), oracle[0], steps=1)
    rel = abs(float(states[0][0]) - oracle[2][0]) / oracle[2][0]
    print(f"bf16 gradient norm {states[0][0]:.6g} vs oracle {oracle[2][0]:.6g}: rel {rel:.3e}")
    assert rel < 0.12
    assert states[0][1] < 1.0 and states[0][1] == _coef32(oracle[0], states[0][0])


def test_generic_route_clips_with_torch(golden_dir):
    """A foreign optimizer: torch.nn.utils.clip_grad_norm_ in front of optimizer.step(); the norm it reports is the fused route's."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    oracle = _oracle_run(golden_dir, "gru")
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=build("fp32"), dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=REG, score_function=softplus_score_function, optimizer=torch.optim.SGD,
                                      prediction_steps=meta["K"], ar_size=meta["H"])
    tr.verbose = False
    tr.max_grad_norm = oracle[0]
    random.seed(SEED)
    with _Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, max_steps=1)
    assert not NEW_ENTRY_POINTS & set(spy.names)
    assert abs(logger.grad_norm_meter.values[0] - oracle[2][0]) <= 1e-3 * oracle[2][0]
    assert tr.last_grad_norm == logger.grad_norm_meter.values[0]


# ------------------------------------------------------------------------------------------ 6. / 7. what must not change
def _train(golden_dir, max_grad_norm, steps=STEPS):
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    model = build("fp32")
    logger = _Logger(grad_norm=False)
    tr = _trainer(model, data, meta, logger)
    tr.max_grad_norm = max_grad_norm
    random.seed(SEED)
    with _Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, max_steps=steps)
    torch.cuda.synchronize()
    return tr, model, logger, spy


def test_large_max_grad_norm_is_the_unclipped_step(golden_dir):
    """max_grad_norm = 1e30: the coefficient is exactly 1 and (g * grad_scale) * 1 is exact, so the one deferred whole-buffer Adam
    launch leaves the bits of the piecewise launches of the unclipped step — losses, parameters and both moments."""
    tr0, model0, logger0, _ = _train(golden_dir, None)
    tr1, model1, logger1, spy = _train(golden_dir, 1e30)
    assert spy.names.count("cpc_adam_clip") == STEPS
    assert float(tr1.last_optimizer.clip_state[1]) == 1.0
    assert logger0.loss_meter.values == logger1.loss_meter.values
    for (k, v), (k1, v1) in zip(model0.state_dict().items(), model1.state_dict().items()):
        assert k == k1 and torch.equal(v, v1), k
    assert torch.equal(tr0.last_optimizer.m, tr1.last_optimizer.m) and torch.equal(tr0.last_optimizer.v, tr1.last_optimizer.v)


def test_unclipped_step_is_the_parent_step(golden_dir):
    """max_grad_norm = None: no new entry point is reached, no clip buffer exists, and losses and parameters after two steps are
    bit-identical to the step as it was before the attribute existed — the engine and FusedAdam called as train() called them."""
    steps = 2
    tr, model, logger, spy = _train(golden_dir, None, steps)
    assert tr.max_grad_norm is None and tr.last_grad_norm is None
    assert not NEW_ENTRY_POINTS & set(spy.names)
    assert spy.names.count("cpc_nce_loss") == steps and spy.names.count("cpc_adam") > steps          # pieces and the head
    assert not hasattr(tr.last_optimizer, "clip_state") and tr.last_optimizer.nan_pair is None
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    model0 = build("fp32")
    opt, losses, _ = _engine_steps(model0, data, _batches(data, meta["B"]), None, steps)
    assert logger.loss_meter.values == losses
    for (k, v), (k0, v0) in zip(model.state_dict().items(), model0.state_dict().items()):
        assert k == k0 and torch.equal(v, v0), k


# ------------------------------------------------------------------------------------------ 10. a non-finite gradient ends the run
@pytest.mark.parametrize("bad_step", [0, 2])
def test_non_finite_gradient_ends_the_run(golden_dir, monkeypatch, capsys, bad_step):
    """An inf written into the flat gradient of step `bad_step` (through the grad_ready_hook, FusedAdam.hook; the loss of that step is
    finite): train() returns None with training_step == bad_step and exactly bad_step steps logged, parameters and both Adam moments
    are bit for bit those of a clean clipped run of bad_step steps, and optimizer.t is put back — the assertions of the NaN-loss
    test (tests/test_model_gpu.py test_nan_guard_keeps_the_last_good_parameters)."""
    oracle = _oracle_run(golden_dir, "gru")
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    if bad_step:
        tr0, model0, _, _ = _train(golden_dir, oracle[0], bad_step)
        good = {k: v.detach().clone() for k, v in model0.state_dict().items()}
        good_m, good_v = tr0.last_optimizer.m.clone(), tr0.last_optimizer.v.clone()
    else:
        good = {k: v.to(DEV) for k, v in state.items()}
        good_m = good_v = None
    real_hook = FusedAdam.hook

    def poisoned_hook(self, lo, hi):
        if self.t == bad_step:
            self.model._flat_grad[hi - 1] = float("inf")
        return real_hook(self, lo, hi)

    monkeypatch.setattr(FusedAdam, "hook", poisoned_hook)
    capsys.readouterr()
    model = build("fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    tr.max_grad_norm = oracle[0]
    random.seed(SEED)
    ret = tr.train(batch_size=meta["B"], epochs=10, lr=LR, num_workers=0, max_steps=bad_step + 3)
    torch.cuda.synchronize()
    printed = capsys.readouterr().out
    assert ret is None and tr.training_step == bad_step
    assert len(logger.loss_meter.values) == bad_step and logger.steps == list(range(bad_step))
    assert len(logger.grad_norm_meter.values) == bad_step
    assert "gradient norm not finite" in printed and "nan loss" in printed
    assert not math.isfinite(tr.last_grad_norm)
    for k, v in good.items():
        assert torch.equal(model.state_dict()[k], v), k
    opt = tr.last_optimizer
    assert opt.t == bad_step
    if bad_step:
        assert torch.equal(opt.m, good_m) and torch.equal(opt.v, good_v)
    else:
        assert not opt.m.any() and not opt.v.any()
