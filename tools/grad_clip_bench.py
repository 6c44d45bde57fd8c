"""Gradient clipping by global norm at the headline size (AudioEncoder 5 x 512 + GRU 256: 7 414 784 parameters, B = 256, bf16).

Prints one JSON line per measurement:
  kernels    cpc_grad_norm alone over n floats (mean of --launches back-to-back calls between two events, --rounds windows) with the
             GB/s it implies, and one whole-buffer cpc_adam against cpc_adam_clip the same way.
  trainer    ms per step of ContrastiveEstimationTrainer.train with max_grad_norm = None twice (the A/A spread) and with
             max_grad_norm set in between.
  unclipped  the two unclipped runs alone: this part touches nothing the change added, so the same file measures the parent commit.

Usage: python tools/grad_clip_bench.py [--batch 256] [--max-grad-norm 1.0] [--parts kernels,trainer]
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


def kernel_times(args, device):
    n, P, L, F = args.n, _hip.ptr, C.c_longlong, C.c_float
    gen = torch.Generator(device=device).manual_seed(1)
    g = torch.randn(n, device=device, generator=gen) * 1e-3
    p, m, v = torch.randn(n, device=device, generator=gen), torch.zeros(n, device=device), torch.zeros(n, device=device)
    ws = torch.empty(int(_hip.lib().cpc_grad_norm_workspace_floats(n)), device=device)
    state = torch.zeros(4, device=device)

    def norm():
        _hip.call("cpc_grad_norm", P(g), L(n), F(1.0), F(args.max_grad_norm), P(ws), P(state), None)

    def adam():
        _hip.call("cpc_adam", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), None)

    def adam_clip():
        _hip.call("cpc_adam_clip", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), P(state, 1), None)

    us = [round(_time(norm, args.launches) * 1e3, 2) for _ in range(args.rounds)]
    med = sorted(us)[len(us) // 2]
    print(json.dumps({"part": "kernels", "kernel": "cpc_grad_norm", "n": n, "bytes": 4 * n, "launches": args.launches, "us": us,
                      "GB_per_s": round(4 * n / (med * 1e-6) / 1e9, 1), "norm": float(state[0]), "coefficient": float(state[1])}),
          flush=True)
    # the two whole-buffer updates alternate: 28 bytes per element each (p, m, v read and written, g read)
    us_a, us_c = [], []
    for _ in range(args.rounds):
        us_a.append(round(_time(adam, args.launches // 4) * 1e3, 2))
        us_c.append(round(_time(adam_clip, args.launches // 4) * 1e3, 2))
    print(json.dumps({"part": "kernels", "n": n, "cpc_adam_us": us_a, "cpc_adam_clip_us": us_c}), flush=True)


def trainer_ms(args, device, max_grad_norm, tag):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer

    class Meter:
        def __init__(self):
            self.last = None

        def update(self, v):
            self.last = v

    class Logger:
        def __init__(self):
            self.loss_meter, self.score_meter, self.grad_norm_meter, self.marks = Meter(), Meter(), Meter(), []

        def log(self, step):
            self.marks.append(time.perf_counter())

    B = args.batch
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=100,
                                       prediction_steps=12, compute_dtype="bf16").to(device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, prediction_steps=12,
                                          ar_size=256)
        tr.verbose = False
        if max_grad_norm is not None:
            tr.max_grad_norm = max_grad_norm
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=args.warmup + args.steps + 1)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "max_grad_norm": max_grad_norm, "dtype": "bf16", "B": B,
                      "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n,
                      "last_loss": logger.loss_meter.last, "last_grad_norm": logger.grad_norm_meter.last}), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n", type=int, default=7414784, help="elements of the flat gradient buffer (the headline model's)")
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--parts", default="kernels,trainer")
    ap.add_argument("--launches", type=int, default=2000, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernels" in parts:
        kernel_times(args, device)
    if "trainer" in parts:
        trainer_ms(args, device, None, "unclipped A")
        trainer_ms(args, device, args.max_grad_norm, "clipped")
        trainer_ms(args, device, None, "unclipped B")
    if "unclipped" in parts:
        trainer_ms(args, device, None, "unclipped A")
        trainer_ms(args, device, None, "unclipped B")


if __name__ == "__main__":
    main()
