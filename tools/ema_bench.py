"""EMA of the weights at the headline size (AudioEncoder 5 x 512 + GRU 256: 7 414 784 parameters, B = 256, bf16).

Prints one JSON line per measurement:
  kernels  one whole-buffer cpc_adam, cpc_ema and cpc_ema_swap over the headline model's flat buffer, the three alternating in one
           process: mean of --launches back-to-back calls between two events, --rounds windows each, with the GB/s the median implies
           (cpc_adam: 28 bytes per element — p, g, m, v read, p, m, v written; cpc_ema: 12 — p and ema read, ema written; cpc_ema_swap:
           16) and the ratio of the medians cpc_ema / cpc_adam (three streams against seven: 3 / 7 = 0.43 is the expectation).
  trainer  ms per step of ContrastiveEstimationTrainer.train with ema_decay off, on, off, on, off (interleaved in one process): the
           three off runs give the run-to-run spread the difference is read against.

Usage: python tools/ema_bench.py [--batch 256] [--decay 0.999] [--parts kernels,trainer]
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cpc_audio_amd  # noqa: E402,F401
from cpc_audio_amd import _hip  # noqa: E402

L_CLIP = 20480


def _time(fn, launches):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def _headline_model(device):
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
    torch.manual_seed(0)
    return AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=100,
                                      prediction_steps=12, compute_dtype="bf16").to(device)


def kernel_times(args, device):
    from cpc_audio_amd.engine import FusedAdam
    P, L, F = _hip.ptr, C.c_longlong, C.c_float
    model = _headline_model(device)
    model._flatten_parameters(device)
    opt = FusedAdam(model, lr=1e-4, ema_decay=args.decay)
    n = model._flat_param.numel()
    model._flat_grad.copy_(torch.randn(n, device=device, generator=torch.Generator(device=device).manual_seed(1)) * 1e-3)
    p, g, m, v, e = model._flat_param, model._flat_grad, opt.m, opt.v, opt.ema

    def adam():
        _hip.call("cpc_adam", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), None)

    def ema():
        _hip.call("cpc_ema", P(p), P(e), L(n), F(args.decay), 0, 1, None, None)

    def swap():          # (an even number of calls per window: the buffers end where they began)
        _hip.call("cpc_ema_swap", P(p), P(e), L(n))

    us = {"cpc_adam": [], "cpc_ema": [], "cpc_ema_swap": []}
    launches = args.launches + args.launches % 2
    for _ in range(args.rounds):
        for name, fn in (("cpc_adam", adam), ("cpc_ema", ema), ("cpc_ema_swap", swap)):
            fn()          # (_time's own warm-up call makes the swaps odd: one more keeps them even)
            us[name].append(round(_time(fn, launches) * 1e3, 2))

    def median(name):
        return sorted(us[name])[len(us[name]) // 2]

    row = {"part": "kernels", "n": n, "launches": launches}
    for name, per_element in (("cpc_adam", 28), ("cpc_ema", 12), ("cpc_ema_swap", 16)):
        row[name + "_us"] = us[name]
        row[name + "_GB_per_s"] = round(per_element * n / (median(name) * 1e-6) / 1e9, 1)
    row["ema_over_adam"] = round(median("cpc_ema") / median("cpc_adam"), 3)
    row["swap_over_adam"] = round(median("cpc_ema_swap") / median("cpc_adam"), 3)
    print(json.dumps(row), flush=True)
    del model, opt
    torch.cuda.empty_cache()


def trainer_ms(args, device, on, tag):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer

    class Meter:
        def __init__(self):
            self.last = None

        def update(self, v):
            self.last = v

    class Logger:
        def __init__(self):
            self.loss_meter, self.score_meter, self.marks = Meter(), Meter(), []

        def log(self, step):
            self.marks.append(time.perf_counter())

    B = args.batch
    total = args.warmup + args.steps + 1
    model = _headline_model(device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, prediction_steps=12,
                                          ar_size=256)
        tr.verbose = False
        tr.ema_decay = args.decay if on else None
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=total)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    row = {"part": "trainer", "run": tag, "ema_decay": args.decay if on else None, "dtype": "bf16", "B": B,
           "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n, "last_loss": logger.loss_meter.last}
    if on:          # how far the average trails the weights: a run that did not average would print 0
        row["shadow_distance"] = float((tr.last_optimizer.ema - model._flat_param.detach()).norm())
    print(json.dumps(row), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--parts", default="kernels,trainer")
    ap.add_argument("--launches", type=int, default=500, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernels" in parts:
        kernel_times(args, device)
    if "trainer" in parts:
        for on, tag in ((False, "ema off A"), (True, "ema on A"), (False, "ema off B"), (True, "ema on B"), (False, "ema off C")):
            trainer_ms(args, device, on, tag)


if __name__ == "__main__":
    main()
