"""Learnable and scheduled temperature at the bench size (AudioEncoder 5 x 512, GRU 256, K = 12, B = 256, 20480-sample clips, bf16).

Prints one JSON line per measurement:
  kernel   per-launch time of the four launches the feature adds, on the engine's own buffers after a real forward pass and loss
           (mean of --launches back-to-back launches between two events): cpc_norm_rows_dev and cpc_norm_rows_bwd_dev over the
           prediction rows (next to cpc_norm_rows / cpc_norm_rows_bwd on the same buffers), cpc_temperature_step over the B K dots
           (lr 0: the state stays) and cpc_temperature_set.
  trainer  ms per step of ContrastiveEstimationTrainer.train (bf16) with NormalizedScoreFunction(0.1) constant, learnable and
           scheduled, alternating in one process for --rounds rounds; the spread of the constant runs (A/A) is the resolution.

Usage: python tools/temperature_bench.py [--batch 256] [--parts kernel,trainer]
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


def build_model(dtype, device):
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256,
                                       visible_steps=100, prediction_steps=12, compute_dtype=dtype)
    return model.to(device)


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


def kernels(args, device):
    from cpc_audio_amd.engine import NORM_EPS, DeviceTemperature, TemperatureSchedule
    model = build_model(args.dtype, device)
    B = args.batch
    eng = model.engine(B, L_CLIP)
    x = torch.randn(B, L_CLIP, device=device) * 0.1
    eng.forward(x)
    tau = args.temperature
    temp = DeviceTemperature(tau, "learnable", device=device)
    eng.nce_forward_backward(False, 1.0, score="normalized", temperature=temp)          # scratch operands, dots, real upstream gradients
    torch.cuda.synchronize()
    K, E, code, P, Lq, F_ = eng.K, eng.E, eng.code, _hip.ptr, C.c_longlong, C.c_float
    R, n, size = B * K, eng._norm, eng.pred.element_size()
    gp = eng.dpred.clone()
    pred_map = (0, Lq(0), Lq(E))
    sched = TemperatureSchedule("cosine", 0.5, tau, 1000)
    ticked = torch.zeros(8, device=device)
    s_min, s_max = temp.bounds
    rows = [
        ("cpc_norm_rows", 2 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows", P(eng.pred), P(n.pn), P(n.inv_p), R, E, *pred_map, F_(1.0 / tau), F_(NORM_EPS), code)),
        ("cpc_norm_rows_dev", 2 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows_dev", P(eng.pred), P(n.pn), P(n.inv_p), R, E, *pred_map, temp.scale_ptr(), F_(NORM_EPS), code)),
        ("cpc_norm_rows_bwd", 3 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows_bwd", P(n.pn), P(n.inv_p), P(gp), R, E, *pred_map, F_(1.0 / tau), F_(NORM_EPS), code)),
        ("cpc_norm_rows_bwd_dev", 3 * R * E * size + 8 * R,
         lambda: _hip.call("cpc_norm_rows_bwd_dev", P(n.pn), P(n.inv_p), P(gp), P(n.dots), R, E, *pred_map, temp.scale_ptr(),
                           F_(NORM_EPS), code)),
        ("cpc_temperature_step", 4 * R + 64,
         lambda: _hip.call("cpc_temperature_step", P(temp.tstate), P(n.dots), R, F_(0.0), F_(0.9), F_(0.999), F_(1e-8), 1, None, F_(1.0),
                           F_(s_min), F_(s_max), None)),
        ("cpc_temperature_set", 32,
         lambda: _hip.call("cpc_temperature_set", P(ticked), *sched.abi_args(), Lq(17), None, Lq(0))),
    ]
    for name, moved, fn in rows:
        ms = _time(fn, args.launches)
        print(json.dumps({"part": "kernel", "kernel": name, "dtype": args.dtype, "n_rows": R, "E": E, "us": round(ms * 1e3, 2),
                          "mb_moved": round(moved / 1e6, 3), "gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1)}), flush=True)
    del eng, model
    torch.cuda.empty_cache()


def trainer_ms(args, device, mode, tag):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction,
                                                               TemperatureSchedule)

    class Meter:
        def update(self, v):
            pass

    class Logger:
        def __init__(self):
            self.loss_meter, self.score_meter, self.marks = Meter(), Meter(), []

        def log(self, step):
            self.marks.append(time.perf_counter())

    B, tau = args.batch, args.temperature
    total = args.warmup + args.steps + 1
    fn = {"constant": lambda: NormalizedScoreFunction(tau),
          "learnable": lambda: NormalizedScoreFunction(tau, learnable=True),
          "scheduled": lambda: NormalizedScoreFunction(schedule=TemperatureSchedule("cosine", 0.5, tau, total))}[mode]()
    model = build_model("bf16", device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, score_function=fn,
                                          prediction_steps=12, ar_size=256)
        tr.verbose = False
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=total)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    ms = (marks[-1] - marks[args.warmup]) / n * 1e3
    print(json.dumps({"part": "trainer", "run": tag, "temperature": mode, "dtype": "bf16", "B": B, "ms_per_step": round(ms, 4),
                      "steps_timed": n, "last_temperature": tr.last_temperature}), flush=True)
    del model, tr
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=0.1)
    ap.add_argument("--parts", default="kernel,trainer")
    ap.add_argument("--launches", type=int, default=2000, help="back-to-back launches per timed kernel window")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernel" in parts:
        kernels(args, device)
    if "trainer" in parts:
        ms = {"constant": [], "learnable": [], "scheduled": []}
        for r in range(args.rounds):
            for mode in ms:
                ms[mode].append(trainer_ms(args, device, mode, f"{mode} {r}"))
        mean = lambda v: sum(v) / len(v)
        spread = max(ms["constant"]) - min(ms["constant"])
        print(json.dumps({"part": "trainer", "aa_spread_ms": round(spread, 4),
                          "learnable_minus_constant_ms": round(mean(ms["learnable"]) - mean(ms["constant"]), 4),
                          "scheduled_minus_constant_ms": round(mean(ms["scheduled"]) - mean(ms["constant"]), 4)}), flush=True)


if __name__ == "__main__":
    main()
