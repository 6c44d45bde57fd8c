"""Grouped negatives at the headline batch (B = 256, K = 12, groups b // 8: runs of eight examples per file).

Prints one JSON line per measurement:
  chain    per-call time of the loss chains (two launches each) on random scores, in both storage dtypes, in the same run:
           cpc_nce_loss, cpc_nce_loss_sampled with N = --negatives, and cpc_nce_loss_grouped in both modes with n_neg = 0 and
           n_neg = --group-negatives (mean of --launches back-to-back calls between two events; the chains alternate for --rounds
           windows each), and of cpc_nce_group_mask.
  trainer  ms per step of ContrastiveEstimationTrainer.train (bf16, AudioEncoder 5 x 512, GRU 256, 20480-sample clips,
           file_batch_size = 8) with negative_groups = None twice (the A/A spread) and with "same_file" and "other_files".

Usage: python tools/grouped_negatives_bench.py [--batch 256] [--parts chain,trainer]
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
    B, K, N, G, P, U = args.batch, 12, args.negatives, args.group_negatives, _hip.ptr, C.c_ulonglong
    ld = (B + 7) // 8 * 8
    S = torch.zeros(K, B, ld, device=device)
    S[:, :, :B] = torch.randn(K, B, B, device=device, generator=torch.Generator(device=device).manual_seed(1)) * 3.0
    groups = (torch.arange(B, device=device) // args.run).to(torch.int32)
    out = torch.zeros(8, device=device)
    ws = torch.empty(int(_hip.lib().cpc_nce_workspace_floats(B, K)), device=device)
    wss = torch.empty(int(_hip.lib().cpc_nce_sampled_workspace_floats(B, K)), device=device)
    wsg = torch.empty(int(_hip.lib().cpc_nce_grouped_workspace_floats(B, K)), device=device)
    mask = torch.empty(K, B, B, device=device, dtype=torch.uint8)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        code = _hip.dtype_code(dt)
        dS, dST = torch.zeros(K, B, ld, device=device, dtype=dt), torch.zeros(K, B, ld, device=device, dtype=dt)
        draw = [0]

        def dense():
            _hip.call("cpc_nce_loss", P(S), P(dS), P(dST), P(out), P(ws), B, K, ld, 1, C.c_float(1.0), code)

        def sampled():
            draw[0] += 1
            _hip.call("cpc_nce_loss_sampled", P(S), P(dS), P(dST), P(out), P(wss), B, K, ld, 1, C.c_float(1.0), N, U(1234), U(draw[0]), code)

        def grouped(mode, n_neg):
            def run():
                draw[0] += 1
                _hip.call("cpc_nce_loss_grouped", P(S), P(dS), P(dST), P(out), P(wsg), B, K, ld, 1, C.c_float(1.0), P(groups), mode, n_neg,
                          U(1234), U(draw[0]), code)
            return run

        chains = {"cpc_nce_loss": dense, f"sampled_N{N}": sampled, "grouped_same_all": grouped(0, 0), "grouped_other_all": grouped(1, 0),
                  f"grouped_same_n{G}": grouped(0, G), f"grouped_other_n{G}": grouped(1, G)}
        # the chains alternate, --rounds times each: the spread of a chain's own windows says what a difference is worth
        us = {k: [] for k in chains}
        for _ in range(args.rounds):
            for k, fn in chains.items():
                us[k].append(round(_time(fn, args.launches) * 1e3, 2))
        print(json.dumps({"part": "chain", "dtype": name, "B": B, "K": K, "run": args.run, "launches": args.launches, "us": us}), flush=True)
    for mode in (0, 1):
        us_m = _time(lambda: _hip.call("cpc_nce_group_mask", P(mask), P(groups), B, K, mode, G, U(1234), U(5)), args.launches) * 1e3
        print(json.dumps({"part": "chain", "B": B, "K": K, "mode": mode, "n_neg": G, "cpc_nce_group_mask_us": round(us_m, 2)}), flush=True)


def trainer_ms(args, device, setting, tag):
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
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, counts=[B // 4] * 16, device=device)
    logger = Logger()
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, prediction_steps=12,
                                          ar_size=256, file_batch_size=args.run)
        tr.verbose = False
        tr.negative_groups = setting
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=args.warmup + args.steps + 1)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "negative_groups": setting, "dtype": "bf16", "B": B, "file_batch_size": args.run,
                      "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n}), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--run", type=int, default=8, help="examples per group: groups[b] = b // run, and the trainer's file_batch_size")
    ap.add_argument("--negatives", type=int, default=128, help="N of the sampled chain")
    ap.add_argument("--group-negatives", type=int, default=16, help="n_neg of the grouped chains that draw")
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
        trainer_ms(args, device, None, "ungrouped A")
        trainer_ms(args, device, "same_file", "same_file")
        trainer_ms(args, device, "other_files", "other_files")
        trainer_ms(args, device, None, "ungrouped B")


if __name__ == "__main__":
    main()
