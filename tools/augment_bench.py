"""Waveform augmentation at the headline size (B = 256 clips of 20480 samples, f32: 21 MB read and 21 MB written per pass).

Prints one JSON line per measurement:
  kernels  cpc_wave_power and cpc_wave_augment alone, for all stages on, speed off, noise off and both off (the four instantiations of
           the apply kernel), the configurations alternating in one process: mean of --launches back-to-back calls between two events, --rounds windows each.  The calls walk a ring of
           --ring batches (input and output of their own each), so that no call finds its batch in the caches the previous one filled.
           GB/s: B L 4 bytes read for the power pass, 2 B L 4 bytes for the apply pass, over the median.
  trainer  ms per step of ContrastiveEstimationTrainer.train on the headline model with augmentation off, on, off, on, off
           (interleaved in one process): the three off runs — the step as it was before the augmentation existed, launch for launch —
           give the run-to-run spread the difference is read against.

Usage: python tools/augment_bench.py [--batch 256] [--parts kernels,trainer]
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
from cpc_audio_amd.augmentation import WaveAugmentation  # noqa: E402

L_CLIP = 20480
STAGES = dict(speed=0.1, time_drop=(4, 1600), noise_snr_db=(5.0, 20.0), gain_db=(-6.0, 3.0), polarity=0.5)


def _configs():
    return {"all on": WaveAugmentation(seed=1, **STAGES),
            "speed off": WaveAugmentation(seed=1, **{k: v for k, v in STAGES.items() if k != "speed"}),
            "noise off": WaveAugmentation(seed=1, **{k: v for k, v in STAGES.items() if k != "noise_snr_db"}),
            "speed and noise off": WaveAugmentation(seed=1, **{k: v for k, v in STAGES.items() if k not in ("speed", "noise_snr_db")})}


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
    B, L, P = args.batch, L_CLIP, _hip.ptr
    gen = torch.Generator(device=device).manual_seed(0)
    xs = [torch.randn(B, L, device=device, generator=gen) * 0.3 for _ in range(args.ring)]
    ys = [torch.empty(B, L, device=device) for _ in range(args.ring)]
    chunks = _hip.lib().cpc_wave_power_chunks(L)
    partial = torch.empty(B * chunks, device=device)
    _hip.call("cpc_wave_power", P(xs[0]), P(partial), B, L, C.c_longlong(L), L)

    def power(i):
        _hip.call("cpc_wave_power", P(xs[i % args.ring]), P(partial), B, L, C.c_longlong(L), L)

    def apply_of(aug):
        cfg = aug.config(step=3, clip_offset=0, protect_from=L)

        def run(i):
            _hip.call("cpc_wave_augment", P(xs[i % args.ring]), P(ys[i % args.ring]), P(partial), None, B, L, C.c_longlong(L),
                      C.c_longlong(L), C.byref(cfg))
        return run

    fns = {"cpc_wave_power": power}
    fns.update({f"cpc_wave_augment, {name}": apply_of(aug) for name, aug in _configs().items()})
    us = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            us[name].append(round(_window(fn, args.launches) * 1e3, 2))
    row = {"part": "kernels", "B": B, "L": L, "ring": args.ring, "launches": args.launches}
    for name, vals in us.items():
        median = sorted(vals)[len(vals) // 2]
        nbytes = B * L * 4 * (1 if name == "cpc_wave_power" else 2)
        row[name] = {"us": vals, "GB_per_s": round(nbytes / (median * 1e-6) / 1e9, 1)}
    print(json.dumps(row), flush=True)
    del xs, ys
    torch.cuda.empty_cache()


def _headline_model(device):
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
    torch.manual_seed(0)
    return AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=100,
                                      prediction_steps=12, compute_dtype="bf16").to(device)


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
        tr.augmentation = _configs()["all on"] if on else None
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=total)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "augmentation": "all on" if on else None, "dtype": "bf16", "B": B,
                      "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n,
                      "last_loss": logger.loss_meter.last}), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parts", default="kernels,trainer")
    ap.add_argument("--ring", type=int, default=16, help="batches the kernel calls walk (16 x 2 x 21 MB: beyond every cache)")
    ap.add_argument("--launches", type=int, default=400, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
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
