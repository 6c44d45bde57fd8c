"""The stacked GRU context: what the per-step gradient costs the backward sweep, and what a layer costs the train step.

    python tools/gru_stacked_bench.py [--steps 20] [--launches 50]

(a) cpc_gru_bwd_steps (dc = NULL, a gradient row per (item, step)) against cpc_gru_bwd on the same tape, same process, B = 256,
    V = 100, bf16, H = 256 (weight-resident kernels) and H = 512 (8-wave streaming kernels): the two alternate, warm, in three
    windows of --launches launches each (HIP events around every launch); mean per window and the spread of the window means.
(b) train step (engine forward + loss + backward + FusedAdam) of AudioEncoder(encoder_default_dict) with
    AudioGRUModel(512, 256, num_layers=L), L = 1, 2, 3, B = 256, 20480-sample clips (100 visible / 12 predicted steps), bf16: the
    three configurations live in one process and take turns, --steps steps a turn, three turns each after 10 warm-up steps; ms per
    step per turn (host clock around work that ends in a device synchronise)."""
import argparse
import ctypes as C
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


def sweep_cost(B, V, H, launches):
    dt, code = torch.bfloat16, _hip.BF16
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(3 * H, H, generator=g) / math.sqrt(H)).to(DEV)
    b = (torch.randn(3 * H, generator=g) * 0.1).to(DEV)
    Gi = torch.randn(B, V, 3 * H, generator=g).to(DEV).to(dt)
    dc = torch.randn(B, H, generator=g).to(DEV)
    dhs = torch.randn(B * V, H, generator=g).to(DEV).to(dt)
    wf = torch.empty(3 * H * H, device=DEV, dtype=dt)
    wt = torch.empty(3 * H * H, device=DEV, dtype=dt)
    _hip.call("cpc_prep_frag", _hip.ptr(w), _hip.ptr(wf), 3 * H, H, H, 0, code)
    _hip.call("cpc_prep_frag", _hip.ptr(w), _hip.ptr(wt), H, 3 * H, H, 1, code)
    Hall = torch.empty(B, V + 1, H, device=DEV, dtype=dt)
    c = torch.empty(B, H, device=DEV)
    dG = torch.empty(B, V, 4 * H, device=DEV, dtype=dt)
    tape = torch.zeros(_hip.lib().cpc_gru_tape_elems(B, V, H, code), device=DEV, dtype=dt)
    _hip.call("cpc_gru_fwd", _hip.ptr(Gi), _hip.ptr(wf), _hip.ptr(b), _hip.ptr(Hall), _hip.ptr(tape), _hip.ptr(c), B, V, H, code)
    fns = {"cpc_gru_bwd": lambda: _hip.call("cpc_gru_bwd", _hip.ptr(dc), _hip.ptr(tape), _hip.ptr(wt), _hip.ptr(dG), B, V, H, code),
           "cpc_gru_bwd_steps": lambda: _hip.call("cpc_gru_bwd_steps", None, _hip.ptr(dhs), C.c_longlong(H), _hip.ptr(tape), _hip.ptr(wt),
                                                  _hip.ptr(dG), B, V, H, code)}
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in fns}
    for _ in range(3):
        ev = {k: [] for k in fns}
        for _ in range(launches):
            for k, fn in fns.items():          # alternating: both see the same clocks and the same cache state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        for k in fns:
            windows[k].append(sum(a.elapsed_time(b_) for a, b_ in ev[k]) / launches)
    return windows


def build(B, L):
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(encoder_default_dict), AudioGRUModel(512, 256, num_layers=L), enc_size=512,
                                       ar_size=256, visible_steps=100, prediction_steps=12, compute_dtype="bf16").to(DEV)
    return model, model.engine(B, 20480), FusedAdam(model, lr=1e-4)


def turn(x, eng, opt, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(out[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    B, V = 256, 100
    for H in (256, 512):
        w = sweep_cost(B, V, H, args.launches)
        for k, v in w.items():
            print(f"sweep B={B} V={V} H={H} bf16 {k:18s} mean {sum(v) / len(v):.4f} ms  windows " + " ".join(f"{t:.4f}" for t in v) +
                  f"  spread {max(v) - min(v):.4f}", flush=True)
    x = torch.randn(B, 20480, generator=torch.Generator().manual_seed(1)).to(DEV)
    cfgs = {L: build(B, L) for L in (1, 2, 3)}
    for L, (_, eng, opt) in cfgs.items():
        turn(x, eng, opt, 10)          # the first steps after an engine is built run slower (queues, allocator): keep them out
    times = {L: [] for L in cfgs}
    for _ in range(3):
        for L, (_, eng, opt) in cfgs.items():
            ms, loss = turn(x, eng, opt, args.steps)
            times[L].append(ms)
    for L, v in times.items():
        print(f"train step bf16 B={B} AudioGRUModel(512, 256, num_layers={L}) mean {sum(v) / len(v):.3f} ms/step  turns " +
              " ".join(f"{t:.3f}" for t in v), flush=True)


if __name__ == "__main__":
    main()
