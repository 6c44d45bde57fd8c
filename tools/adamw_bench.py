"""AdamW weight decay and the learning-rate schedule at the headline size (AudioEncoder 5 x 512 + GRU 256: 7 414 784 parameters,
B = 256, bf16).

Prints one JSON line per measurement:
  kernels  one whole-buffer cpc_adam against one whole-buffer cpc_adamw (every second 64-float block decays) over n floats, the two
           alternating in one process: mean of --launches back-to-back calls between two events, --rounds windows each, with the
           GB/s the median implies (28 bytes per element: p, m, v read and written, g read; cpc_adamw adds its bitmap, n / 512 bytes).
  trainer  ms per step of ContrastiveEstimationTrainer.train with weight_decay and lr_schedule at their defaults twice (the A/A
           spread) and with both set in between.
  plain    the two default runs and cpc_adam alone: this part touches nothing the change added, so the same file measures the
           parent commit.
  dev      one whole-buffer cpc_adam against one whole-buffer cpc_adam_dev (its one-thread tick kernel and the update), alternating
           like `kernels`.

Usage: python tools/adamw_bench.py [--batch 256] [--weight-decay 0.01] [--parts kernels,trainer]
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


def kernel_times(args, device, with_adamw):
    n, P, L, F = args.n, _hip.ptr, C.c_longlong, C.c_float
    gen = torch.Generator(device=device).manual_seed(1)
    g = torch.randn(n, device=device, generator=gen) * 1e-3
    p, m, v = torch.randn(n, device=device, generator=gen), torch.zeros(n, device=device), torch.zeros(n, device=device)
    blocks = (n + 63) // 64
    bits = torch.full(((blocks + 31) // 32,), 0x55555555, dtype=torch.int32, device=device)          # every second block decays

    def adam():
        _hip.call("cpc_adam", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), None)

    def adamw():
        _hip.call("cpc_adamw", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), F(args.weight_decay),
                  P(bits), L(0), None, None)

    us_a, us_w = [], []
    for _ in range(args.rounds):
        us_a.append(round(_time(adam, args.launches) * 1e3, 2))
        if with_adamw:
            us_w.append(round(_time(adamw, args.launches) * 1e3, 2))

    def gbs(us, extra=0):
        return round((28 * n + extra) / (sorted(us)[len(us) // 2] * 1e-6) / 1e9, 1)

    row = {"part": "kernels", "n": n, "launches": args.launches, "cpc_adam_us": us_a, "cpc_adam_GB_per_s": gbs(us_a)}
    if with_adamw:
        row.update({"cpc_adamw_us": us_w, "cpc_adamw_GB_per_s": gbs(us_w, 4 * bits.numel())})
    print(json.dumps(row), flush=True)


def dev_times(args, device):
    n, P, L, F = args.n, _hip.ptr, C.c_longlong, C.c_float
    gen = torch.Generator(device=device).manual_seed(1)
    g = torch.randn(n, device=device, generator=gen) * 1e-3
    p, m, v = torch.randn(n, device=device, generator=gen), torch.zeros(n, device=device), torch.zeros(n, device=device)
    state = torch.zeros(4, device=device)

    def adam():
        _hip.call("cpc_adam", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), None)

    def adam_dev():
        _hip.call("cpc_adam_dev", P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), P(state), F(1.0), None)

    us_a, us_d = [], []
    for _ in range(args.rounds):
        us_a.append(round(_time(adam, args.launches) * 1e3, 2))
        us_d.append(round(_time(adam_dev, args.launches) * 1e3, 2))
    print(json.dumps({"part": "dev", "n": n, "launches": args.launches, "cpc_adam_us": us_a, "cpc_adam_dev_us": us_d}), flush=True)


def trainer_ms(args, device, on, tag):
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
            self.loss_meter, self.score_meter, self.lr_meter, self.marks = Meter(), Meter(), Meter(), []

        def log(self, step):
            self.marks.append(time.perf_counter())

    B = args.batch
    total = args.warmup + args.steps + 1
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=100,
                                       prediction_steps=12, compute_dtype="bf16").to(device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, prediction_steps=12,
                                          ar_size=256)
        tr.verbose = False
        if on:
            from cpc_audio_amd.contrastive_estimation_training import LRSchedule
            tr.weight_decay = args.weight_decay
            tr.lr_schedule = LRSchedule("cosine", warmup_steps=args.warmup, total_steps=total, min_lr_ratio=0.1)
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=total)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "weight_decay": args.weight_decay if on else 0.0, "schedule": bool(on),
                      "dtype": "bf16", "B": B, "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n,
                      "last_loss": logger.loss_meter.last, "last_lr": logger.lr_meter.last}), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n", type=int, default=7414784, help="elements of the flat parameter buffer (the headline model's)")
    ap.add_argument("--weight-decay", type=float, default=0.01)
    ap.add_argument("--parts", default="kernels,trainer")
    ap.add_argument("--launches", type=int, default=500, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernels" in parts:
        kernel_times(args, device, True)
    if "trainer" in parts:
        trainer_ms(args, device, False, "default A")
        trainer_ms(args, device, True, "decay + schedule")
        trainer_ms(args, device, False, "default B")
    if "plain" in parts:
        kernel_times(args, device, False)
        trainer_ms(args, device, False, "default A")
        trainer_ms(args, device, False, "default B")
    if "dev" in parts:
        dev_times(args, device)


if __name__ == "__main__":
    main()
