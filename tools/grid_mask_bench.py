"""Grid masking at configs[2]'s input (B = 128 grids of 629 frames x 256 bins x 2 channels, f32: 165 MB).

Prints one JSON line per measurement:
  kernels  cpc_grid_sum, cpc_grid_mask in place with the zero and with the mean fill (the mean fill's line is the mask launch alone; the
           sum pass has its own), the copy form, and a plain device copy of the same grid (torch's copy_), alternating in one
           process: mean of --launches back-to-back calls between two events, --rounds windows each.  The calls walk a ring of --ring
           grids (input and output of their own each), so that no call finds its grid in the caches the previous one filled.
           GB/s over the median: the grid's bytes for the sum, twice that for the copy form and the copy, and for the in-place form the
           bytes of the masked cells alone (the mean over the ring's draws of 4 Cc bytes per masked cell, from GridMasking.spans).
           The last entry is the in-place call with nothing to mask and spans_out given, one workgroup per clip: what a back-to-back
           launch through ctypes costs whatever it does.
  trainer  ms per step of ContrastiveEstimationTrainer.train on the configs[2]-shaped model (CQT front end, bf16) with grid masking
           off, on, off, on, off (interleaved in one process): the three off runs — the step as it was before the masking existed,
           launch for launch — give the run-to-run spread the difference is read against.

Usage: python tools/grid_mask_bench.py [--batch 128] [--parts kernels,trainer]
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
from cpc_audio_amd import _hip, configs  # noqa: E402
from cpc_audio_amd.grid_masking import GridMasking  # noqa: E402

W_GRID, H_GRID, CC = 629, 256, 2
L_CLIP = 97024
MASKS = dict(freq_masks=(2, 27), time_masks=(2, 40))


def _window(fn, launches):
    """Mean ms of ``launches`` calls fn(i) between two events."""
    for i in range(8):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def kernel_times(args, device):
    B, W, H, Cc, P = args.batch, W_GRID, H_GRID, CC, _hip.ptr
    n = W * H * Cc
    gen = torch.Generator(device=device).manual_seed(0)
    xs = [torch.randn(B, W, H, Cc, device=device, generator=gen) for _ in range(args.ring)]
    ys = [torch.empty(B, W, H, Cc, device=device) for _ in range(args.ring)]
    chunks = _hip.lib().cpc_grid_sum_chunks(n)
    partial = torch.empty(B * chunks * Cc, device=device)
    zero, mean = GridMasking(fill="zero", seed=1, **MASKS), GridMasking(fill="mean", seed=1, **MASKS)
    masked_bytes = sum(int(zero.spans(i, B, W, H)[1].sum()) for i in range(args.ring)) / args.ring * 4 * Cc

    def grid_sum(i):
        _hip.call("cpc_grid_sum", P(xs[i % args.ring]), P(partial), B, n, C.c_longlong(n), Cc)

    spans = torch.zeros(B, 32, dtype=torch.int32, device=device)

    def mask_of(gm, copy, report=False):
        both = xs + ys          # the in-place form stores a sixth of a grid: it walks inputs and outputs alike
        cfgs = [gm.config(step=s, clip_offset=0, W=W) for s in range(args.ring)]

        def run(i):
            x = xs[i % args.ring] if copy else both[i % len(both)]
            _hip.call("cpc_grid_mask", P(x), P(ys[i % args.ring] if copy else x), P(partial), P(spans) if report else None, None, B, W, H,
                      Cc, C.c_longlong(n), C.c_longlong(n), C.byref(cfgs[i % args.ring]))
        return run

    def plain_copy(i):
        ys[i % args.ring].copy_(xs[i % args.ring])

    grid_sum(0)
    fns = {"cpc_grid_sum": (grid_sum, 4 * B * n), "cpc_grid_mask in place, zero fill": (mask_of(zero, False), masked_bytes),
           "cpc_grid_mask in place, mean fill": (mask_of(mean, False), masked_bytes),
           "cpc_grid_mask copy form, zero fill": (mask_of(zero, True), 8 * B * n), "device copy (torch copy_)": (plain_copy, 8 * B * n),
           "cpc_grid_mask in place, no mask, spans_out (one workgroup per clip: the launch floor)":
               (mask_of(GridMasking(seed=1), False, report=True), 0)}
    us = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, (fn, _) in fns.items():
            us[name].append(round(_window(fn, args.launches) * 1e3, 2))
    row = {"part": "kernels", "B": B, "W": W, "H": H, "Cc": Cc, "grid_MB": round(4 * B * n / 1e6, 1), "masked_MB": round(masked_bytes / 1e6, 2),
           "ring": args.ring, "launches": args.launches}
    for name, vals in us.items():
        median = sorted(vals)[len(vals) // 2]
        row[name] = {"us": vals, "GB_per_s": round(fns[name][1] / (median * 1e-6) / 1e9, 1)}
    print(json.dumps(row), flush=True)
    del xs, ys
    torch.cuda.empty_cache()


def trainer_ms(args, device, on, tag):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.audio_model import AudioGRUModel, AudioPredictiveCodingModel
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer
    from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder, cqt_default_dict

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
    torch.manual_seed(0)
    pre = PreprocessingModule(cqt_dict=cqt_default_dict, phase=True).to(device)
    pre.cqt.precision = "bf16x3"
    enc = ScalogramResidualEncoder(args_dict=configs.fresh(configs.scalogram_resnet_architecture_7), preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=60, prediction_steps=16,
                                       compute_dtype="bf16").to(device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, prediction_steps=16,
                                          ar_size=256, preprocessing=pre)
        tr.verbose = False
        tr.grid_masking = GridMasking(fill=args.fill, seed=1, **MASKS) if on else None
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=total)
        torch.cuda.synchronize()
    marks = logger.marks
    steps = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "grid_masking": f"2 + 2 masks, {args.fill} fill" if on else None, "dtype": "bf16", "B": B,
                      "input": list(pre.output.shape), "ms_per_step": round((marks[-1] - marks[args.warmup]) / steps * 1e3, 4),
                      "steps_timed": steps, "last_loss": logger.loss_meter.last}), flush=True)
    del model, tr, pre
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--parts", default="kernels,trainer")
    ap.add_argument("--ring", type=int, default=8, help="grids the kernel calls walk (8 x 2 x 165 MB: beyond every cache)")
    ap.add_argument("--launches", type=int, default=200, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--fill", default="mean", choices=["zero", "mean"], help="the fill of the trainer runs with masking on")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernels" in parts:
        kernel_times(args, device)
    if "trainer" in parts:
        for on, tag in ((False, "off A"), (True, "on A"), (False, "off B"), (True, "on B"), (False, "off C")):
            trainer_ms(args, device, on, tag)


if __name__ == "__main__":
    main()
