"""The GRU recurrence at hidden sizes 256, 384 and 512, and a whole train step with an AudioGRUModel(512, 512) context.

    python tools/gru_wide_bench.py [--steps 20]

(1) cpc_gru_fwd / cpc_gru_bwd alone at B = 256, V = 100 for H in {256, 384, 512}, bf16 and f32: ms per launch (HIP events
    around 10 launches after 3 warm-up launches).  H = 256 runs the weight-resident kernels in bf16 and the 4-wave streaming ones
    in f32; H = 384 and 512 the 8-wave streaming ones.
(2) train step (engine forward + loss + backward + FusedAdam) of AudioEncoder(encoder_default_dict) with AudioGRUModel(512, H),
    ar_size H, for H = 256 (the headline context) and 512, B = 256, 20480-sample clips (100 visible / 12 predicted steps), bf16:
    ms per step over --steps steps after 10 warm-up steps, host clock around work that ends in a device synchronise."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel, encoder_default_dict  # noqa: E402
from cpc_audio_amd.engine import FusedAdam  # noqa: E402

DEV = "cuda:0"


def recurrence(B, V, H, dt):
    code = _hip.dtype_code(dt)
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(3 * H, H, generator=g) / math.sqrt(H)).to(DEV)
    b = (torch.randn(3 * H, generator=g) * 0.1).to(DEV)
    Gi = torch.randn(B, V, 3 * H, generator=g).to(DEV).to(dt)
    dc = torch.randn(B, H, generator=g).to(DEV)
    wf = torch.empty(3 * H * H, device=DEV, dtype=dt)
    wt = torch.empty(3 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(w), _hip.ptr(wf), 3 * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(w), _hip.ptr(wt), H, 3 * H, H, 1, code)
    Hall = torch.empty(B, V + 1, H, device=DEV, dtype=dt)
    c = torch.empty(B, H, device=DEV)
    dG = torch.empty(B, V, 4 * H, device=DEV, dtype=dt)
    tape = torch.zeros(_hip.lib().cpc_gru_tape_elems(B, V, H, code), device=DEV, dtype=dt)
    res = {}
    for name, fn in (("fwd", lambda: _hip.call("cpc_gru_fwd", _hip.ptr(Gi), _hip.ptr(wf), _hip.ptr(b), _hip.ptr(Hall), _hip.ptr(tape),
                                               _hip.ptr(c), B, V, H, code)),
                     ("bwd", lambda: _hip.call("cpc_gru_bwd", _hip.ptr(dc), _hip.ptr(tape), _hip.ptr(wt), _hip.ptr(dG), B, V, H, code))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / 10
    return res


def train_step(B, H, steps):
    L, V, K = 20480, 100, 12
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(encoder_default_dict), AudioGRUModel(512, H), enc_size=512, ar_size=H,
                                       visible_steps=V, prediction_steps=K, compute_dtype="bf16").to(DEV)
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
    del model, eng, opt
    torch.cuda.empty_cache()
    return ms, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    B, V = 256, 100
    for dt in (torch.bfloat16, torch.float32):
        for H in (256, 384, 512):
            r = recurrence(B, V, H, dt)
            print(f"recurrence B={B} V={V} H={H:3d} {str(dt).split('.')[1]:8s} fwd {r['fwd']:.3f} ms  bwd {r['bwd']:.3f} ms", flush=True)
    for H in (256, 512):
        ms, loss = train_step(B, H, args.steps)
        print(f"train step bf16 B={B} AudioGRUModel(512, {H}) {ms:.3f} ms/step  loss {loss:.5f}", flush=True)


if __name__ == "__main__":
    main()
