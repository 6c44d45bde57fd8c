"""LAMB trust ratios at the headline size (AudioEncoder 5 x 512 + GRU 256: 7 414 784 parameters, B = 256, bf16).

Prints one JSON line per measurement:
  kernels  one whole-buffer cpc_adamw against one whole-buffer cpc_lamb (three launches) over the headline model's flat buffer — its
           parameter table, every parameter with dim() >= 2 selected —, the two alternating in one process: mean of --launches
           back-to-back calls between two events, --rounds windows each, with the GB/s the median implies (cpc_adamw: 28 bytes per
           element; cpc_lamb: 40 — pass 1 reads p, g, m, v and writes m, v, pass 3 reads p, m, v and writes p — plus the block sums,
           8 bytes per 64 floats written and read once, and the 4-byte map entry per block).
  trainer  ms per step of ContrastiveEstimationTrainer.train with trust_ratio off twice (the A/A spread) and on in between, all
           three with the same weight_decay.

Usage: python tools/lamb_bench.py [--batch 256] [--weight-decay 0.01] [--parts kernels,trainer]
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
    opt = FusedAdam(model, lr=1e-4, weight_decay=args.weight_decay, trust_ratio=True)
    n = model._flat_param.numel()
    model._flat_grad.copy_(torch.randn(n, device=device, generator=torch.Generator(device=device).manual_seed(1)) * 1e-3)
    p, g, m, v = model._flat_param, model._flat_grad, opt.m, opt.v
    head = (P(p), P(g), P(m), P(v), L(n), F(1e-4), F(0.9), F(0.999), F(1e-8), 1, F(1.0), F(args.weight_decay), P(opt.decay_bits), L(0),
            None)
    params = len(opt._lamb_names)

    def adamw():
        _hip.call("cpc_adamw", *head, None)

    def lamb():
        _hip.call("cpc_lamb", *head, C.cast(opt._param_block, C.c_void_p), P(opt._param_block_dev), P(opt._block_param), 0, params,
                  params, F(-1.0), P(opt._lamb_ws), P(opt.trust), None)

    us_w, us_l = [], []
    for _ in range(args.rounds):
        us_w.append(round(_time(adamw, args.launches) * 1e3, 2))
        us_l.append(round(_time(lamb, args.launches) * 1e3, 2))

    def gbs(us, per_element, extra=0):
        return round((per_element * n + extra) / (sorted(us)[len(us) // 2] * 1e-6) / 1e9, 1)

    blocks = n // 64
    print(json.dumps({"part": "kernels", "n": n, "parameters": params, "launches": args.launches, "cpc_adamw_us": us_w,
                      "cpc_adamw_GB_per_s": gbs(us_w, 28, 4 * opt.decay_bits.numel()), "cpc_lamb_us": us_l,
                      "cpc_lamb_GB_per_s": gbs(us_l, 40, blocks * (8 + 8 + 4) + 8 * opt.decay_bits.numel())}), flush=True)
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
        tr.weight_decay = args.weight_decay
        tr.trust_ratio = bool(on)
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=total)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    row = {"part": "trainer", "run": tag, "weight_decay": args.weight_decay, "trust_ratio": bool(on), "dtype": "bf16", "B": B,
           "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n, "last_loss": logger.loss_meter.last}
    if on:
        ratios = [r for _, _, r in tr.last_optimizer.trust_ratios().values()]
        row["ratios_min_max"] = [round(min(ratios), 5), round(max(ratios), 5)]
    print(json.dumps(row), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
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
        kernel_times(args, device)
    if "trainer" in parts:
        trainer_ms(args, device, False, "trust_ratio off A")
        trainer_ms(args, device, True, "trust_ratio on")
        trainer_ms(args, device, False, "trust_ratio off B")


if __name__ == "__main__":
    main()
