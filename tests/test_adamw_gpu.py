"""AdamW weight decay and the learning-rate schedule on the HIP path: cpc_adamw against a float64 AdamW and against cpc_adam /
cpc_adam_clip bit for bit, cpc_lr_factors against LRSchedule.factor, cpc_adamw_dev's device-side step, FusedAdam and
ContrastiveEstimationTrainer (eager, use_graph, generic route, resumed) against the CPU oracle model with torch.optim.AdamW +
LambdaLR, and the default step, which must not reach any of the new entry points."""
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
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, LRSchedule, softplus_score_function
from cpc_audio_amd.engine import FusedAdam
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
L, F = C.c_longlong, C.c_float
SENTINEL = -8192.0
NEW_ENTRY_POINTS = {"cpc_adamw", "cpc_adamw_dev", "cpc_lr_factors"}
ULP = 2.0 ** -23          # one float32 rounding of a double result (relative)
B1, B2, EPS = 0.9, 0.999, 1e-8


def _guarded(n, fill=0.0, tail=64):
    whole = torch.full((n + tail,), SENTINEL, device=DEV, dtype=torch.float32)
    whole[:n] = fill
    return whole[:n], whole


def _intact(*wholes, tail=64):
    return all(bool((w[-tail:] == SENTINEL).all()) for w in wholes)


def _guarded_copy(host):
    view, whole = _guarded(host.numel())
    view.copy_(host)
    return view, whole


def _bitmap(pattern, blocks, seed=0):
    """(per-block booleans, int32 device words): bit j % 32 of word j // 32 covers block j."""
    if pattern == "clear":
        bits = np.zeros(blocks, dtype=bool)
    elif pattern == "set":
        bits = np.ones(blocks, dtype=bool)
    elif pattern == "alternating":
        bits = np.arange(blocks) % 2 == 1
    else:
        bits = np.random.default_rng(seed).random(blocks) < 0.5
    words = np.zeros(-(-blocks // 32), dtype=np.uint32)
    for j in np.nonzero(bits)[0]:
        words[j // 32] |= np.uint32(1) << np.uint32(j % 32)
    return bits, torch.from_numpy(words.view(np.int32).copy()).to(DEV)


def _args(p, g, m, v, lr, step, scale):
    return (_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), L(p.numel()), F(lr), F(B1), F(B2), F(EPS), step, F(scale))


def _adamw64(p, g, m, v, lr, step, decayed, wd):
    """One float64 AdamW step in torch.optim.AdamW's order: the decay first, then Adam with the new moments."""
    p = torch.where(decayed, p * (1.0 - lr * wd), p)
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    p = p - (lr / (1 - B1 ** step)) * m / (v.sqrt() / math.sqrt(1 - B2 ** step) + EPS)
    return p, m, v


# ------------------------------------------------------------------------------------------ 1. cpc_adamw against float64 AdamW
@pytest.mark.parametrize("n", [4, 64, 65, 2048 + 7, 3 * 2048 + 5, 256 * 1024 + 5])
def test_adamw_against_float64(n):
    """Three steps at lr 1e-3 with weight_decay 0.1 and 10, ranges that begin at blocks 0, 1, 31, 32 and 45 of the bitmap, four bit
    patterns.  Every element: 2e-6 absolute on parameters and moments against float64 (cpc_adam's own tolerance,
    tests/test_hip_kernels.py test_adam_matches_torch); undecayed blocks, and both moments everywhere: cpc_adam's bits."""
    lr = 1e-3
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 2.0 for _ in range(3)]
    worst = 0.0
    for first_block in (0, 1, 31, 32, 45):
        blocks = first_block + -(-n // 64)
        for pattern in ("clear", "set", "alternating", "random"):
            bits, words = _bitmap(pattern, blocks, seed=n + first_block)
            decayed = torch.from_numpy(bits[first_block + np.arange(n) // 64])
            for wd in (0.1, 10.0):
                (p, pw), (m, mw), (v, vw) = _guarded_copy(p0), _guarded(n), _guarded(n)
                q, qm, qv = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)          # cpc_adam on the same data
                p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
                for step in range(1, 4):
                    g, gw = _guarded_copy(grads[step - 1])
                    _hip.call("cpc_adamw", *_args(p, g, m, v, lr, step, 1.0), F(wd), _hip.ptr(words), L(first_block), None, None)
                    _hip.call("cpc_adam", *_args(q, g, qm, qv, lr, step, 1.0), None)
                    p64, m64, v64 = _adamw64(p64, grads[step - 1].double(), m64, v64, lr, step, decayed, wd)
                    torch.cuda.synchronize()
                    case = (n, first_block, pattern, wd, step)
                    assert _intact(pw, mw, vw, gw) and torch.equal(g.cpu(), grads[step - 1]), case
                    err = max((p.double().cpu() - p64).abs().max().item(), (m.double().cpu() - m64).abs().max().item(),
                              (v.double().cpu() - v64).abs().max().item())
                    worst = max(worst, err)
                    assert err < 2e-6, (case, err)
                    assert torch.equal(m, qm) and torch.equal(v, qv), case          # the moments do not see the decay
                    keep = ~decayed.to(DEV)
                    assert torch.equal(p[keep], q[keep]), case
                    q.copy_(p)                                                       # (the next step starts from the same parameters)
                if pattern == "set" and wd == 10.0:                                  # the decay was applied: 3 % of |p| after three steps
                    moved = (p.cpu() - p0).abs() > 0.02 * p0.abs()
                    assert moved[p0.abs() > 0.5].all(), (n, first_block)
    print(f"cpc_adamw n={n}: worst |err| against float64 {worst:.3e}")


# ------------------------------------------------------------------------------------------ 2. bit-identity without decay
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [8192, 10007])
def test_adamw_without_decay_is_cpc_adam_and_cpc_adam_clip(n, scale):
    """weight_decay = 0 (no bitmap, or one with every bit set): without coef the bits of cpc_adam, with coef those of cpc_adam_clip
    (coefficient 1 and 0.37), for grad_scale 1 and 1/2, over three steps from non-zero moments; a raised skip changes nothing."""
    gen = torch.Generator().manual_seed(11 * n)
    start = (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01)
    _, words = _bitmap("set", -(-n // 64) + 3)
    for coef_value in (None, 1.0, 0.37):
        coef = None if coef_value is None else torch.full((1,), coef_value, device=DEV)
        for bits, first in ((None, 0), (words, 3)):
            a = [t.to(DEV) for t in start]
            b = [_guarded_copy(t) for t in start]
            for step in range(1, 4):
                dg = (torch.randn(n, generator=torch.Generator().manual_seed(step)) * 3.0).to(DEV)
                if coef is None:
                    _hip.call("cpc_adam", *_args(a[0], dg, a[1], a[2], 1e-3, step, scale), None)
                else:
                    _hip.call("cpc_adam_clip", *_args(a[0], dg, a[1], a[2], 1e-3, step, scale), _hip.ptr(coef), None)
                _hip.call("cpc_adamw", *_args(b[0][0], dg, b[1][0], b[2][0], 1e-3, step, scale), F(0.0), _hip.ptr(bits), L(first),
                          _hip.ptr(coef), None)
                torch.cuda.synchronize()
                for x, (y, whole), name in zip(a, b, "pmv"):
                    assert torch.equal(x, y) and _intact(whole), (name, step, coef_value, first)
            flag = torch.ones(1, device=DEV)
            before = [y.clone() for y, _ in b]
            _hip.call("cpc_adamw", *_args(b[0][0], dg, b[1][0], b[2][0], 1e-3, 4, scale), F(0.5), _hip.ptr(words), L(0), _hip.ptr(coef),
                      _hip.ptr(flag))
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, (y, _) in zip(before, b)), coef_value


# ------------------------------------------------------------------------------------------ 3. the schedule on the device
@pytest.mark.parametrize("ratio", [0.0, 0.1])
@pytest.mark.parametrize("warmup", [0, 1, 5])
@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_lr_factors_against_the_host_schedule(kind, warmup, ratio):
    T, count = 12, 8
    sched = LRSchedule(kind, warmup_steps=warmup, total_steps=T, min_lr_ratio=ratio)
    for step0 in (0, T - 2, 10 ** 6):
        out, whole = _guarded(count)
        _hip.call("cpc_lr_factors", *sched.abi_args(), L(step0), count, _hip.ptr(out))
        torch.cuda.synchronize()
        assert _intact(whole)
        got = out.double().cpu().tolist()
        want = [sched.factor(step0 + i) for i in range(count)]
        for i, (a, b) in enumerate(zip(got, want)):
            assert abs(a - b) <= ULP * abs(b), (kind, warmup, ratio, step0 + i, a, b)


# ------------------------------------------------------------------------------------------ 4. the step count on the device
def test_adamw_dev_counts_and_schedules_on_the_device():
    """Five cpc_adamw_dev calls from a zeroed state, then one under a raised skip: the count stays at 5, state[1:4] are the host
    formulas at schedule index step_offset + 4 to one float32 rounding, parameters and moments within 2e-6 of five cpc_adamw calls
    with host-side steps and learning rates."""
    n, lr, wd, offset = 2048 + 7, 1e-3, 0.1, 2
    sched = LRSchedule("cosine", warmup_steps=4, total_steps=9, min_lr_ratio=0.1)
    gen = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=gen)
    _, words = _bitmap("random", -(-n // 64), seed=4)
    (p, pw), (m, mw), (v, vw), (state, sw) = _guarded_copy(p0), _guarded(n), _guarded(n), _guarded(4)
    q, qm, qv = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    skip = torch.zeros(1, device=DEV)

    def dev_call(g):
        _hip.call("cpc_adamw_dev", _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), L(n), F(lr), F(B1), F(B2), F(EPS), _hip.ptr(state),
                  F(1.0), F(wd), _hip.ptr(words), *sched.abi_args(), L(offset), None, _hip.ptr(skip))

    for step in range(1, 6):
        g = (torch.randn(n, generator=gen) * 2.0).to(DEV)
        dev_call(g)
        _hip.call("cpc_adamw", *_args(q, g, qm, qv, lr * sched.factor(offset + step - 1), step, 1.0), F(wd), _hip.ptr(words), L(0), None,
                  None)
    torch.cuda.synchronize()
    after = [t.clone() for t in (p, m, v, state)]
    skip.fill_(1.0)
    dev_call(g)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(after, (p, m, v, state))) and _intact(pw, mw, vw, sw)
    st = state.cpu()
    assert int(st[:1].view(torch.int32)) == 5
    lr5 = float(np.float32(lr)) * sched.factor(offset + 4)
    want = (lr5 / (1 - float(np.float32(B1)) ** 5), 1 / math.sqrt(1 - float(np.float32(B2)) ** 5), 1 - lr5 * float(np.float32(wd)))
    for i, w in enumerate(want):
        assert abs(float(st[1 + i]) - w) <= ULP * abs(w), (i, float(st[1 + i]), w)
    for a, b, name in ((p, q, "p"), (m, qm, "m"), (v, qv, "v")):
        assert (a - b).abs().max().item() < 2e-6, name
    assert (p.cpu() - p0).abs().max().item() > 1e-3          # ... and five updates were applied


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("entry", ["cpc_adam_dev", "cpc_adamw_dev"])
def test_device_step_entry_points_carry_the_host_step_bits(entry, scale):
    """cpc_adam_dev next to cpc_adam, cpc_adamw_dev (constant schedule, weight_decay 0.1, a random bitmap) next to cpc_adamw: three
    steps from a zeroed state and non-zero moments, every step of both from the same parameters and moments.  Step 1: state[1],
    state[2] and, for cpc_adamw_dev, state[3] are bitwise the floats of the host formulas on the f32 values of lr / betas / decay
    (pow(x, 1) is exact, so one correctly rounded double division / square root and one rounding to float is all there is), and
    p, m, v are the host-step entry point's bits.  Steps 2 and 3: the same comparison wherever the scalars agree with the host's."""
    n = 2048 + 7
    lr, b1, b2, wd = (float(np.float32(x)) for x in (1e-3, B1, B2, 0.1))
    decays = entry == "cpc_adamw_dev"
    gen = torch.Generator().manual_seed(17)
    _, words = _bitmap("random", -(-n // 64), seed=17)
    start = (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01)
    dev, host = [_guarded_copy(t) for t in start], [_guarded(n) for _ in start]
    (state, sw), compared = _guarded(4), 0
    for t in range(1, 4):
        g, gw = _guarded_copy(torch.randn(n, generator=gen) * 2.0)
        for (h, _), (d, _) in zip(host, dev):
            h.copy_(d)
        (p, _), (m, _), (v, _) = dev
        (q, _), (qm, _), (qv, _) = host
        if decays:
            _hip.call(entry, *_args(p, g, m, v, lr, _hip.ptr(state), scale), F(wd), _hip.ptr(words), *LRSchedule("constant").abi_args(),
                      L(0), None, None)
            _hip.call("cpc_adamw", *_args(q, g, qm, qv, lr, t, scale), F(wd), _hip.ptr(words), L(0), None, None)
        else:
            _hip.call(entry, *_args(p, g, m, v, lr, _hip.ptr(state), scale), None)
            _hip.call("cpc_adam", *_args(q, g, qm, qv, lr, t, scale), None)
        torch.cuda.synchronize()
        assert _intact(sw, gw, *(w for _, w in dev + host)), t
        st = state.cpu().numpy()
        assert int(st[:1].view(np.int32)[0]) == t and (decays or st[3] == 0.0)
        want = [lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)] + ([1.0 - lr * wd] if decays else [])
        agree = [np.float32(w).tobytes() == st[1 + i].tobytes() for i, w in enumerate(want)]
        print(f"{entry} scale {scale} step {t}: state[1:4] = {st[1:4].tolist()}, host {want}, bitwise equal {agree}")
        assert t > 1 or all(agree), (st[1:4].tolist(), want)
        if all(agree):
            compared += 1
            for (d, _), (h, _), name in zip(dev, host, "pmv"):
                assert torch.equal(d, h), (name, t)
    print(f"{entry} scale {scale}: {compared} of 3 steps compared bit for bit")
    assert (dev[0][0].cpu() - start[0]).abs().max().item() > 1e-3          # ... and the updates were applied


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
    def __init__(self, lr=True):
        self.loss_meter, self.score_meter, self.steps, self.trainer, self.last_lrs = _Meter(), _Meter(), [], None, []
        if lr:
            self.lr_meter = _Meter()

    def log(self, step):
        self.steps.append(step)
        if self.trainer is not None:
            self.last_lrs.append(self.trainer.last_lr)


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


REG, LR, WD, SEED = 0.5, 1e-3, 10.0, 5
SCHED = LRSchedule("cosine", warmup_steps=2, total_steps=4, min_lr_ratio=0.1)
_ORACLE = {}


def _batches(data, B, seed=SEED):
    random.seed(seed)
    return [list(b) for b in FileBatchSampler([data.shape[0]], B, 1, True, verbose=False)]


def _steps(data, meta):
    return min(4, data.shape[0] // meta["B"])          # as many steps as the fixture's batches allow, at most 4


def _oracle_run(golden_dir, context, weight_decay=WD, schedule=SCHED):
    """The oracle model under torch.optim.AdamW — two groups: dim() >= 2 with the decay, the rest without — and LambdaLR;
    computed once per setting and shared: (losses, learning rates, parameters)."""
    key = (context, weight_decay, schedule)
    if key not in _ORACLE:
        meta, data, state, _, okw = _fixture(golden_dir, context)
        batches = _batches(data, meta["B"])
        ot = O.OracleTrainer(state, meta["V"], meta["K"], score="softplus", regularization=REG, lr=LR, **okw)
        plist = list(ot.params.values())
        opt = torch.optim.AdamW([{"params": [p for p in plist if p.dim() >= 2], "weight_decay": weight_decay},
                                 {"params": [p for p in plist if p.dim() < 2], "weight_decay": 0.0}], lr=LR)
        lam = torch.optim.lr_scheduler.LambdaLR(opt, schedule.factor if schedule is not None else (lambda s: 1.0))
        losses, lrs = [], []
        for i in range(_steps(data, meta)):
            loss, _, _ = ot.loss_and_grads(data[batches[i]])
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            lam.step()
            losses.append(float(loss))
        _ORACLE[key] = (losses, lrs, {k: p.detach().clone() for k, p in ot.params.items()})
    return _ORACLE[key]


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _feature_is_visible(golden_dir):
    """So that the comparisons below cannot pass with the feature missing — on the oracle alone (small_model): every decayed tensor
    of the decayed run lies >= 10 x the relative-L2 bound (1e-3) from the undecayed run, every tensor of the scheduled run >= 5 x
    that bound from the constant-lr run, and a bias moves by < 5e-3 under the decay alone (the filter matters)."""
    full = _oracle_run(golden_dir, "gru")[2]
    undecayed = _oracle_run(golden_dir, "gru", weight_decay=0.0)[2]
    constant = _oracle_run(golden_dir, "gru", schedule=None)[2]
    plain = _oracle_run(golden_dir, "gru", weight_decay=0.0, schedule=None)[2]
    for k, ref in full.items():
        if ref.dim() >= 2:
            assert _rel_l2(undecayed[k], ref) >= 10 * 1e-3, (k, _rel_l2(undecayed[k], ref))
            assert _rel_l2(plain[k], constant[k]) >= 10 * 1e-3, k
        else:
            assert _rel_l2(plain[k], constant[k]) < 5e-3, (k, _rel_l2(plain[k], constant[k]))
        assert _rel_l2(constant[k], ref) >= 5 * 1e-3, (k, _rel_l2(constant[k], ref))


def _gradient_is_not_identically_zero(name, ref):
    """Mask of the elements the 97 % criterion counts (tests/test_grad_clip_gpu.py): the key bias of an attention layer has an exact
    gradient of zero, both sides hold rounding noise there, and Adam divides that noise by its own size."""
    mask = torch.ones_like(ref, dtype=torch.bool)
    if name.endswith("self_attn.in_proj_bias"):
        third = ref.numel() // 3
        mask[third:2 * third] = False
    return mask


def _check_against_oracle(context, model, losses, oracle):
    """The project's f32 bounds (tests/test_grad_clip_gpu.py _check_against_oracle) with the sum of the steps' learning rates in
    the place of lr * steps: loss 1e-4 (1 + 2 i), 97 % of a tensor's elements within 0.05 sum(lr_i) + 1e-4 |ref|, relative L2 below
    1e-3.  Every figure is printed before anything is asserted."""
    o_losses, lrs, o_params = oracle
    sd = model.state_dict()
    rows = []
    for k, ref in o_params.items():
        got = sd[k].cpu()
        err = (got - ref).abs()
        tight = (err <= 0.05 * sum(lrs) + 1e-4 * ref.abs())[_gradient_is_not_identically_zero(k, ref)].float().mean().item()
        rows.append((k, err.max().item(), tight, _rel_l2(got, ref)))
    print(f"{context}: lrs {lrs}\n  losses {losses}\n  oracle {o_losses}")
    for k, worst, tight, l2 in rows:
        print(f"  {k}: max |err| {worst:.3e}, tight fraction {tight:.4f}, rel L2 {l2:.3e}")
    assert len(losses) == len(o_losses)
    for i in range(len(o_losses)):
        assert abs(losses[i] - o_losses[i]) <= 1e-4 * abs(o_losses[i]) * (1 + 2 * i), (context, i, losses, o_losses)
    for k, worst, tight, l2 in rows:
        assert tight > 0.97, (k, tight)
        assert l2 < 1e-3, (k, l2)


def _engine_steps(model, data, batches, steps, **adam):
    """The fused step by hand, as train() issues it: (optimizer, losses, learning rates)."""
    model.train()
    model._flatten_parameters(DEV)
    opt = adam.pop("optimizer", None) or FusedAdam(model, lr=LR, **adam)
    model.link_grads()
    dev_data = data.to(DEV)
    losses, lrs = [], []
    for i in range(steps):
        x = dev_data[torch.as_tensor(batches[i % len(batches)], device=DEV)].contiguous()
        eng = model.engine(x.shape[0], x.shape[1], DEV)
        if i == 0:
            eng.nan_flag().zero_()
        opt.after_update = eng.prepare_ahead
        opt.skip_flag = eng.nan_flag()
        if opt.max_grad_norm is not None:
            opt.nan_pair = eng.nan_pair()
        out = eng.loss_and_grads(x, softplus=True, regularization=REG, all_timesteps=False, grad_ready_hook=opt.hook,
                                 global_negatives=None, after_loss=None, score="softplus")
        opt.step(grad_scale=1.0)
        losses.append(float(out[0]))
        lrs.append(opt.lr)
    torch.cuda.synchronize()
    return opt, losses, lrs


def _trainer(model, data, meta, logger, score_function=softplus_score_function):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=REG, score_function=score_function, prediction_steps=meta["K"],
                                      ar_size=meta["H"])
    tr.verbose = False
    logger.trainer = tr
    return tr


@pytest.mark.parametrize("context", ["gru", "conv", "attention"])
def test_engine_decayed_scheduled_steps_against_oracle(golden_dir, context):
    """eng.loss_and_grads + FusedAdam(weight_decay=10, schedule=...) by hand: every update is a cpc_adamw launch (pieces at
    parameter boundaries and the head), none a cpc_adam, and the step runs at lr * factor(s)."""
    _feature_is_visible(golden_dir)
    meta, data, state, build, _ = _fixture(golden_dir, context)
    oracle = _oracle_run(golden_dir, context)
    steps = _steps(data, meta)
    model = build("fp32")
    with _Spy() as spy:
        opt, losses, lrs = _engine_steps(model, data, _batches(data, meta["B"]), steps, weight_decay=WD, schedule=SCHED)
    assert spy.names.count("cpc_adamw") > steps and "cpc_adam" not in spy.names and "cpc_adamw_dev" not in spy.names
    assert lrs == [LR * SCHED.factor(s) for s in range(steps)] and max(abs(a - b) for a, b in zip(lrs, oracle[1])) <= 1e-15
    assert opt.t == steps
    _check_against_oracle(context, model, losses, oracle)


@pytest.mark.parametrize("context", ["gru", "conv", "attention"])
def test_trainer_decayed_scheduled_steps_against_oracle(golden_dir, context):
    """The same through ContrastiveEstimationTrainer.train: last_lr and logger.lr_meter are lr * factor(s) at every step."""
    _feature_is_visible(golden_dir)
    meta, data, state, build, _ = _fixture(golden_dir, context)
    oracle = _oracle_run(golden_dir, context)
    steps = _steps(data, meta)
    model = build("fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    tr.weight_decay, tr.lr_schedule = WD, SCHED
    tr.host_sync_lag = 0          # every step is logged before the next is launched: log() sees the step's own last_lr
    assert tr.last_lr is None
    random.seed(SEED)
    with _Spy() as spy:
        ret = tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, max_steps=steps)
    assert ret is None and tr.training_step == steps and logger.steps == list(range(steps))
    assert spy.names.count("cpc_adamw") > steps and "cpc_adam" not in spy.names
    want = [LR * SCHED.factor(s) for s in range(steps)]
    assert logger.lr_meter.values == want and logger.last_lrs == want and tr.last_lr == want[-1]
    assert tr.last_optimizer.t == steps and tr.last_optimizer.lr == want[-1]
    _check_against_oracle(context, model, logger.loss_meter.values, oracle)


# ------------------------------------------------------------------------------------------ 6. piecewise against whole
def test_piecewise_decayed_update_is_the_whole_buffer_update(golden_dir):
    """One decayed step as update_range pieces at parameter boundaries plus step(), as one whole-buffer launch, and as the clipped
    launch with max_grad_norm = 1e30 (coefficient exactly 1): the same bits in parameters and moments."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    results = []
    for mode in ("pieces", "whole", "clipped"):
        model = build("fp32")
        model._flatten_parameters(DEV)
        n = model._flat_param.numel()
        gen = torch.Generator().manual_seed(6)
        model._flat_grad.copy_(torch.randn(n, generator=gen) * 0.3)
        opt = FusedAdam(model, lr=LR, weight_decay=WD, schedule=SCHED, max_grad_norm=1e30 if mode == "clipped" else None)
        opt.m.copy_(torch.randn(n, generator=gen) * 0.1)
        opt.v.copy_(torch.rand(n, generator=gen) * 0.01)
        with _Spy() as spy:
            if mode == "pieces":
                edges = sorted(model._offset.values()) + [n]
                cuts = [edges[0], edges[len(edges) // 3], edges[2 * len(edges) // 3], edges[-3], n]
                assert cuts[0] == 0 and all(c % 64 == 0 for c in cuts) and sorted(set(cuts)) == cuts
                for lo, hi in reversed(list(zip(cuts[1:-1], cuts[2:]))):          # from the tail of the buffer, as the backward pass
                    opt.update_range(lo, hi, 1.0)
            opt.step(grad_scale=1.0)
        torch.cuda.synchronize()
        assert spy.names.count("cpc_adamw") == {"pieces": 4, "whole": 1, "clipped": 1}[mode] and "cpc_adam" not in spy.names
        if mode == "clipped":
            assert float(opt.clip_state[1]) == 1.0
        assert opt.lr == LR * SCHED.factor(0) and opt.t == 1
        results.append((model._flat_param.clone(), opt.m.clone(), opt.v.clone()))
    for other in results[1:]:
        for a, b, name in zip(results[0], other, "pmv"):
            assert torch.equal(a, b), name
    start = build("fp32")
    start._flatten_parameters(DEV)
    assert (results[0][0] - start._flat_param).abs().max().item() > 1e-3          # ... and the step was applied


# ------------------------------------------------------------------------------------------ 7. resume
RESUME_SCHED = LRSchedule("cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.1)


def _optimizer_bits(opt):
    return opt.model._flat_param.clone(), opt.m.clone(), opt.v.clone(), opt.t


def test_resumed_engine_run_is_the_uninterrupted_run(golden_dir):
    """Run A: 6 fused steps on fixed batches.  Run B: 3 steps, FusedAdam.state_dict() and the model's state_dict() into a fresh
    model and a fresh FusedAdam with step_offset = 3, 3 steps more.  Parameters, m, v and t: bit-identical."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    batches = _batches(data, meta["B"])
    kw = dict(weight_decay=WD, schedule=RESUME_SCHED)
    opt_a, losses_a, lrs_a = _engine_steps(build("fp32"), data, batches, 6, **kw)
    model_b = build("fp32")
    opt_b, losses_b, _ = _engine_steps(model_b, data, batches, 3, **kw)
    saved_opt = opt_b.state_dict()
    saved_model = {k: v.detach().clone() for k, v in model_b.state_dict().items()}
    model_c = build("fp32")
    model_c.load_state_dict(saved_model)
    model_c._flatten_parameters(DEV)
    opt_c = FusedAdam(model_c, lr=LR, step_offset=3, **kw)
    opt_c.load_state_dict(saved_opt)
    assert opt_c.t == 3
    _, losses_c, lrs_c = _engine_steps(model_c, data, batches[3:] + batches[:3], 3, optimizer=opt_c)
    assert lrs_c == lrs_a[3:] == [LR * RESUME_SCHED.factor(s) for s in (3, 4, 5)]
    assert losses_b + losses_c == losses_a
    a, c = _optimizer_bits(opt_a), _optimizer_bits(opt_c)
    assert a[3] == c[3] == 6
    for x, y, name in zip(a[:3], c[:3], "pmv"):
        assert torch.equal(x, y), name
    # ... and a resumed run WITHOUT the optimizer state is a different run (what train() did before optimizer_state existed)
    model_d = build("fp32")
    model_d.load_state_dict(saved_model)
    opt_d, _, _ = _engine_steps(model_d, data, batches[3:] + batches[:3], 3, step_offset=3, **kw)
    assert not torch.equal(opt_d.model._flat_param, a[0])


def test_resumed_trainer_run_is_the_uninterrupted_run(golden_dir):
    """The same through trainer.optimizer_state, trainer.last_optimizer and continue_training_at_step (three batches per epoch, so
    that the second call's sampler starts where the first run's second epoch does)."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    data = data[:3 * meta["B"]]

    def run(model, first, steps, optimizer_state=None):
        logger = _Logger()
        tr = _trainer(model, data, meta, logger)
        tr.weight_decay, tr.lr_schedule, tr.optimizer_state = WD, RESUME_SCHED, optimizer_state
        tr.train(batch_size=meta["B"], epochs=10, lr=LR, continue_training_at_step=first, num_workers=0, max_steps=first + steps)
        torch.cuda.synchronize()
        assert tr.optimizer_state is None and tr.training_step == first + steps
        return tr, logger

    random.seed(SEED)
    tr_a, log_a = run(build("fp32"), 0, 6)
    random.seed(SEED)
    model_b = build("fp32")
    tr_b, log_b = run(model_b, 0, 3)
    saved_opt = tr_b.last_optimizer.state_dict()
    model_c = build("fp32")
    model_c.load_state_dict({k: v.detach().clone() for k, v in model_b.state_dict().items()})
    tr_c, log_c = run(model_c, 3, 3, optimizer_state=saved_opt)
    assert log_c.steps == [3, 4, 5] and log_c.lr_meter.values == log_a.lr_meter.values[3:]
    assert log_b.loss_meter.values + log_c.loss_meter.values == log_a.loss_meter.values
    a, c = _optimizer_bits(tr_a.last_optimizer), _optimizer_bits(tr_c.last_optimizer)
    assert a[3] == c[3] == 6
    for x, y, name in zip(a[:3], c[:3], "pmv"):
        assert torch.equal(x, y), name


# ------------------------------------------------------------------------------------------ 8. use_graph
def test_graphed_step_with_schedule_and_decay_follows_the_eager_step(golden_dir):
    """trainer.use_graph with decay and schedule: the captured step is cpc_adamw_dev (no refusal), the losses follow the eager run
    at the existing graph test's bound (tests/test_model_gpu.py test_graphed_step_matches_eager: 1e-4 (1 + 2 i)), and the device's
    step count and state[1] after the run are the host formulas."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    steps, first = 4, 1
    runs = []
    for use_graph in (False, True):
        model = build("fp32")
        logger = _Logger()
        tr = _trainer(model, data, meta, logger)
        tr.weight_decay, tr.lr_schedule, tr.use_graph = WD, SCHED, use_graph
        random.seed(SEED)
        with _Spy() as spy:
            tr.train(batch_size=meta["B"], epochs=10, lr=LR, continue_training_at_step=first, num_workers=0, max_steps=first + steps)
        torch.cuda.synchronize()
        assert ("cpc_adamw_dev" in spy.names) == use_graph and "cpc_adam_dev" not in spy.names and "cpc_adam" not in spy.names
        assert logger.lr_meter.values == [LR * SCHED.factor(first + i) for i in range(steps)]
        runs.append((logger.loss_meter.values, {n: p.detach().clone() for n, p in model.named_parameters()}, tr.last_optimizer))
    (l0, p0, _), (l1, p1, opt) = runs
    print(f"eager {l0}\ngraph {l1}")
    for i in range(steps):
        assert abs(l1[i] - l0[i]) <= 1e-4 * abs(l0[i]) * (1 + 2 * i), i
    for n in p0:
        assert _rel_l2(p1[n], p0[n]) < 1e-3, (n, _rel_l2(p1[n], p0[n]))
    st = opt.state.cpu()
    assert int(st[:1].view(torch.int32)) == steps and opt.t == steps
    want = float(np.float32(LR)) * SCHED.factor(first + steps - 1) / (1 - float(np.float32(B1)) ** steps)
    assert abs(float(st[1]) - want) <= ULP * want, (float(st[1]), want)


# ------------------------------------------------------------------------------------------ 9. the generic route
def test_generic_route_decays_and_schedules(golden_dir):
    """A score function the trainer does not recognise (a lambda around softplus_score_function) takes the generic route with
    torch.optim.Adam: the decay is a _foreach_mul_ in front of optimizer.step(), every group gets the step's rate.  Against the same
    oracle run at the generic route's bounds (tests/test_model_gpu.py test_generic_route_through_the_loss_kernels)."""
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    losses, lrs, o_params = _oracle_run(golden_dir, "gru")
    steps = len(losses)
    model = build("fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger, score_function=lambda p, t: softplus_score_function(p, t))
    assert not tr._fused()
    tr.weight_decay, tr.lr_schedule = WD, SCHED
    random.seed(SEED)
    with _Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, max_steps=steps)
    assert not NEW_ENTRY_POINTS & set(spy.names) and "cpc_adam" not in spy.names
    assert logger.lr_meter.values == [LR * SCHED.factor(s) for s in range(steps)]
    for i in range(steps):
        assert abs(logger.loss_meter.values[i] - losses[i]) < 2e-4 * abs(losses[i]), i
    for k, v in model.state_dict().items():
        ref = o_params[k]
        err = (v.cpu() - ref).abs()
        assert err.max().item() <= 2 * sum(lrs) * 1.01 + 1e-6, k
        tight = err <= 0.05 * sum(lrs) + 1e-4 * ref.abs()
        assert tight.float().mean().item() > 0.97, (k, tight.float().mean().item())


# ------------------------------------------------------------------------------------------ 10. the default step
def test_default_step_is_the_parent_step(golden_dir):
    """With the attributes at their defaults no new entry point is reached and nothing new is allocated; losses and parameters after
    two steps are bit-identical to a run that never touches the new attributes — the engine and FusedAdam called as train() called
    them before the attributes existed."""
    steps = 2
    meta, data, state, build, _ = _fixture(golden_dir, "gru")
    model = build("fp32")
    logger = _Logger(lr=False)
    tr = _trainer(model, data, meta, logger)
    random.seed(SEED)
    with _Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=LR, num_workers=0, max_steps=steps)
    torch.cuda.synchronize()
    assert (tr.weight_decay, tr.weight_decay_filter, tr.lr_schedule, tr.optimizer_state) == (0.0, None, None, None)
    assert not NEW_ENTRY_POINTS & set(spy.names)
    assert spy.names.count("cpc_nce_loss") == steps and spy.names.count("cpc_adam") > steps          # pieces and the head
    assert tr.last_optimizer.decay_bits is None and tr.last_optimizer.schedule is None and tr.last_lr == LR
    model0 = build("fp32")
    model0.train()
    model0._flatten_parameters(DEV)
    opt = FusedAdam(model0, lr=LR)
    opt, losses, _ = _engine_steps(model0, data, _batches(data, meta["B"]), steps, optimizer=opt)
    assert logger.loss_meter.values == losses
    for (k, v), (k0, v0) in zip(model.state_dict().items(), model0.state_dict().items()):
        assert k == k0 and torch.equal(v, v0), k
    assert torch.equal(tr.last_optimizer.m, opt.m) and torch.equal(tr.last_optimizer.v, opt.v)


# ------------------------------------------------------------------------------------------ 11. bf16
def test_bf16_decayed_scheduled_step(golden_dir):
    """One bf16 step with decay, schedule and clipping: the gradient norm within the bf16 clipped step's bound of the oracle's (0.12
    relative, tests/test_grad_clip_gpu.py test_bf16_clipped_step), and every parameter within one Adam step (<= lr_0 per element) of
    its decayed — or, for a parameter the filter leaves out, undecayed — start."""
    meta, data, state, build, okw = _fixture(golden_dir, "gru")
    batches = _batches(data, meta["B"])
    ot = O.OracleTrainer(state, meta["V"], meta["K"], score="softplus", regularization=REG, lr=LR, **okw)
    _, _, grads = ot.loss_and_grads(data[batches[0]])
    ref_norm = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values())))
    model = build("bf16")
    opt, losses, lrs = _engine_steps(model, data, batches, 1, weight_decay=WD, schedule=SCHED, max_grad_norm=0.5 * ref_norm)
    lr0 = LR * SCHED.factor(0)
    assert lrs == [lr0]
    norm, coef = float(opt.clip_state[0]), float(opt.clip_state[1])
    rel = abs(norm - ref_norm) / ref_norm
    print(f"bf16 gradient norm {norm:.6g} vs oracle {ref_norm:.6g}: rel {rel:.3e}; coefficient {coef:.4f}")
    assert rel < 0.12 and coef < 1.0
    for k, v in model.state_dict().items():
        start = state[k] * (1.0 - lr0 * WD) if state[k].dim() >= 2 else state[k]
        assert (v.cpu() - start).abs().max().item() <= lr0 * 1.01 + 1e-6 * (1 + start.abs().max().item()), k
