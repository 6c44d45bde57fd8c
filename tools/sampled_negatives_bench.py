"""Sampled negatives at the headline size (BASELINE configs[4]: 12 prediction steps x 128 negatives, B = 256).

Prints one JSON line per measurement:
  chain    per-call time of the cpc_nce_loss chain against the cpc_nce_loss_sampled chain (two launches each) on random
           scores at B = 256, K = 12, N = 128, in both storage dtypes, and of cpc_nce_sample_mask (mean of --launches
           back-to-back calls between two events; the two chains alternate for --rounds windows each).
  trainer  ms per step of ContrastiveEstimationTrainer.train (bf16, AudioEncoder 5 x 512, GRU 256, 20480-sample clips) with
           num_negatives = None twice (the A/A spread) and with num_negatives = 128.

Usage: python tools/sampled_negatives_bench.py [--batch 256] [--negatives 128] [--parts chain,trainer]
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


def chain_times(args, device):
    B, K, N, P = args.batch, 12, args.negatives, _hip.ptr
    ld = (B + 7) // 8 * 8
    S = torch.zeros(K, B, ld, device=device)
    S[:, :, :B] = torch.randn(K, B, B, device=device, generator=torch.Generator(device=device).manual_seed(1)) * 3.0
    out = torch.zeros(8, device=device)
    ws = torch.empty(int(_hip.lib().cpc_nce_workspace_floats(B, K)), device=device)
    wss = torch.empty(int(_hip.lib().cpc_nce_sampled_workspace_floats(B, K)), device=device)
    mask = torch.empty(K, B, B, device=device, dtype=torch.uint8)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        code = _hip.dtype_code(dt)
        dS, dST = torch.zeros(K, B, ld, device=device, dtype=dt), torch.zeros(K, B, ld, device=device, dtype=dt)
        draw = [0]

        def dense():
            _hip.call("cpc_nce_loss", P(S), P(dS), P(dST), P(out), P(ws), B, K, ld, 1, C.c_float(1.0), code)

        def sampled():
            draw[0] += 1
            _hip.call("cpc_nce_loss_sampled", P(S), P(dS), P(dST), P(out), P(wss), B, K, ld, 1, C.c_float(1.0), N, C.c_ulonglong(1234),
                      C.c_ulonglong(draw[0]), code)

        # the two chains alternate, --rounds times each: the spread of a chain's own rounds says what a difference is worth
        us_d, us_s = [], []
        for _ in range(args.rounds):
            us_d.append(round(_time(dense, args.launches) * 1e3, 2))
            us_s.append(round(_time(sampled, args.launches) * 1e3, 2))
        med = lambda v: sorted(v)[len(v) // 2]
        print(json.dumps({"part": "chain", "dtype": name, "B": B, "K": K, "N": N, "launches": args.launches, "cpc_nce_loss_us": us_d,
                          "cpc_nce_loss_sampled_us": us_s, "median_difference_us": round(med(us_s) - med(us_d), 2)}), flush=True)
    us_m = _time(lambda: _hip.call("cpc_nce_sample_mask", P(mask), B, K, N, C.c_ulonglong(1234), C.c_ulonglong(5)), args.launches) * 1e3
    print(json.dumps({"part": "chain", "B": B, "K": K, "N": N, "cpc_nce_sample_mask_us": round(us_m, 2)}), flush=True)


def trainer_ms(args, device, negatives, tag):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer

    class Meter:
        def update(self, v):
            pass

    class Logger:
        def __init__(self):
            self.loss_meter, self.score_meter, self.marks = Meter(), Meter(), []

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
        tr.num_negatives, tr.negative_seed = negatives, 1234
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=args.warmup + args.steps + 1)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "num_negatives": negatives, "dtype": "bf16", "B": B,
                      "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n}), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--negatives", type=int, default=128)
    ap.add_argument("--parts", default="chain,trainer")
    ap.add_argument("--launches", type=int, default=5000, help="back-to-back calls per timed window (5000 x 20 us = 0.1 s)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "chain" in parts:
        chain_times(args, device)
    if "trainer" in parts:
        trainer_ms(args, device, None, "unsampled A")
        trainer_ms(args, device, args.negatives, "sampled")
        trainer_ms(args, device, None, "unsampled B")


if __name__ == "__main__":
    main()
