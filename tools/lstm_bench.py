"""The LSTM recurrence at hidden sizes 128, 256 and 512 beside the streaming GRU recurrence, and a whole train step with an
AudioLSTMModel(512, 256) context beside the AudioGRUModel(512, 256) one.

    python tools/lstm_bench.py [--steps 20]

(1) cpc_lstm_fwd / cpc_lstm_bwd alone at B = 256, V = 100 for H in {128, 256, 512}, bf16 and f32: ms per launch (HIP events around
    10 launches after 3 warm-up launches).  H <= 256 runs the 4-wave kernels, H = 512 the 8-wave ones.  Beside each figure the
    project's own weight-streaming GRU kernels at the same shape in the same run (cpc_gru_set_streaming(1), restored afterwards)
    and the ratio: an LSTM launch moves and multiplies 4/3 of the GRU's recurrent weights per step.
(2) train step (engine forward + loss + backward + FusedAdam) of AudioEncoder(encoder_default_dict) with AudioLSTMModel(512, 256)
    and, in the same run, with AudioGRUModel(512, 256) (the headline context: weight-resident bf16 GRU kernels), B = 256,
    20480-sample clips (100 visible / 12 predicted steps), bf16: ms per step over --steps steps after 10 warm-up steps, host clock
    around work that ends in a device synchronise."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_model import (AudioEncoder, AudioGRUModel, AudioLSTMModel, AudioPredictiveCodingModel,  # noqa: E402
                                       encoder_default_dict)
from cpc_audio_amd.engine import FusedAdam  # noqa: E402

DEV = "cuda:0"


def _time(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 10


def recurrence(kind, B, V, H, dt):
    """ms per launch of the forward and the backward recurrence; kind 'lstm' (4 gates) or 'gru' (3 gates, streaming kernels)."""
    code = _hip.dtype_code(dt)
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(G * H, H, generator=g) / math.sqrt(H)).to(DEV)
    b = (torch.randn(G * H, generator=g) * 0.1).to(DEV)
    Gi = torch.randn(B, V, G * H, generator=g).to(DEV).to(dt)
    dc = torch.randn(B, H, generator=g).to(DEV)
    wf = torch.empty(G * H * H, device=DEV, dtype=dt)
    wt = torch.empty(G * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(w), _hip.ptr(wf), G * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(w), _hip.ptr(wt), H, G * H, H, 1, code)
    Hall = torch.empty(B, V + 1, H, device=DEV, dtype=dt)
    c = torch.empty(B, H, device=DEV)
    cell = torch.empty(B, H, device=DEV)
    dG = torch.empty(B, V, 4 * H, device=DEV, dtype=dt)
    if kind == "lstm":
        tape = torch.zeros(_hip.lib().cpc_lstm_tape_elems(B, V, H, code), device=DEV, dtype=dt)
        fwd = lambda: _hip.call("cpc_lstm_fwd", _hip.ptr(Gi), _hip.ptr(wf), _hip.ptr(b), None, None, _hip.ptr(Hall), _hip.ptr(tape),  # noqa: E731
                                _hip.ptr(c), _hip.ptr(cell), B, V, H, code)
        bwd = lambda: _hip.call("cpc_lstm_bwd", _hip.ptr(dc), _hip.ptr(tape), _hip.ptr(wt), _hip.ptr(dG), B, V, H, code)  # noqa: E731
        return {"fwd": _time(fwd), "bwd": _time(bwd)}
    old = _hip.lib().cpc_gru_set_streaming(1)
    try:
        tape = torch.zeros(_hip.lib().cpc_gru_tape_elems(B, V, H, code), device=DEV, dtype=dt)
        fwd = lambda: _hip.call("cpc_gru_fwd", _hip.ptr(Gi), _hip.ptr(wf), _hip.ptr(b), _hip.ptr(Hall), _hip.ptr(tape), _hip.ptr(c),  # noqa: E731
                                B, V, H, code)
        bwd = lambda: _hip.call("cpc_gru_bwd", _hip.ptr(dc), _hip.ptr(tape), _hip.ptr(wt), _hip.ptr(dG), B, V, H, code)  # noqa: E731
        return {"fwd": _time(fwd), "bwd": _time(bwd)}
    finally:
        torch.cuda.synchronize()
        _hip.lib().cpc_gru_set_streaming(old)


def train_step(B, ar, steps):
    L, V, K = 20480, 100, 12
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(encoder_default_dict), ar(), enc_size=512, ar_size=256, visible_steps=V,
                                       prediction_steps=K, compute_dtype="bf16").to(DEV)
    eng = model.engine(B, L)
    opt = FusedAdam(model, lr=1e-4)
    for _ in range(10):          # the first steps after an engine is built run slower (queues, allocator): keep them out
        out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        opt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        opt.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    loss = float(out[0])
    ctx = type(eng.ctx).__name__
    del model, eng, opt
    torch.cuda.empty_cache()
    return ms, loss, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    B, V = 256, 100
    for dt in (torch.bfloat16, torch.float32):
        for H in (128, 256, 512):
            r, g = recurrence("lstm", B, V, H, dt), recurrence("gru", B, V, H, dt)
            print(f"recurrence B={B} V={V} H={H:3d} {str(dt).split('.')[1]:8s} LSTM fwd {r['fwd']:.3f} ms  bwd {r['bwd']:.3f} ms | "
                  f"streaming GRU fwd {g['fwd']:.3f} ms  bwd {g['bwd']:.3f} ms | LSTM / GRU fwd {r['fwd'] / g['fwd']:.2f}  "
                  f"bwd {r['bwd'] / g['bwd']:.2f}", flush=True)
    res = {}
    for label, ar in (("AudioGRUModel(512, 256)", lambda: AudioGRUModel(512, 256)), ("AudioLSTMModel(512, 256)", lambda: AudioLSTMModel(512, 256))):
        ms, loss, ctx = train_step(B, ar, args.steps)
        res[label] = ms
        print(f"train step bf16 B={B} {label} [{ctx}] {ms:.3f} ms/step  loss {loss:.5f}", flush=True)
    print(f"LSTM step / GRU step {res['AudioLSTMModel(512, 256)'] / res['AudioGRUModel(512, 256)']:.2f}", flush=True)


if __name__ == "__main__":
    main()
