"""Cosine-similarity scores with a temperature at the bench size (AudioEncoder 5 x 512, GRU 256, K = 12, B = 256, 20480-sample clips).

Prints one JSON line per measurement:
  kernel   per-launch time of cpc_norm_rows / cpc_norm_rows_bwd on the engine's own buffers after a real forward pass, over the
           prediction rows (rpi 0) and over the target rows inside the top-layer buffer (mean of --launches back-to-back launches
           between two events), with the GB/s the launch implies: B K x E elements in and out for the forward, two in and one out for
           the backward, plus the f32 inv entries.
  chain    the whole loss chain (scores, loss, gradients with respect to predictions and targets) with score="normalized" against
           score="linear", in both loss branches: means of --launches back-to-back calls, the two chains alternating for --rounds
           windows each in one process.
  trainer  ms per step of ContrastiveEstimationTrainer.train (bf16) with NormalizedScoreFunction(0.1), between two runs with
           linear_score_function: the spread of those two (A/A) is the resolution, a difference below it is reported as none.

Usage: python tools/normalized_scores_bench.py [--dtype bf16|fp32] [--batch 256] [--parts kernel,chain,trainer]
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


def kernel_and_chain(args, device, parts):
    from cpc_audio_amd.engine import NORM_EPS
    model = build_model(args.dtype, device)
    B = args.batch
    eng = model.engine(B, L_CLIP)
    x = torch.randn(B, L_CLIP, device=device) * 0.1
    eng.forward(x)
    tau = args.temperature
    eng.nce_forward_backward(False, 1.0, score="normalized", temperature=tau)          # scratch operands, real upstream gradients
    torch.cuda.synchronize()
    K, E, code, P, Lq, F_ = eng.K, eng.E, eng.code, _hip.ptr, C.c_longlong, C.c_float
    R, T, Ltop = B * K, eng.T, eng.geo.alloc[-1]
    n, tg, size = eng._norm, (T - K) * E, eng.pred.element_size()
    gp, gt = eng.dpred.clone(), eng.dact[-1].clone()
    pred_map, top_map = (0, Lq(0), Lq(E)), (K, Lq(Ltop * E), Lq(E))
    rows = [
        ("cpc_norm_rows", "predictions", 2 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows", P(eng.pred), P(n.pn), P(n.inv_p), R, E, *pred_map, F_(1.0 / tau), F_(NORM_EPS), code)),
        ("cpc_norm_rows", "targets", 2 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows", P(eng.act[-1], tg), P(n.tn, tg), P(n.inv_t), R, E, *top_map, F_(1.0), F_(NORM_EPS), code)),
        ("cpc_norm_rows_bwd", "predictions", 3 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows_bwd", P(n.pn), P(n.inv_p), P(gp), R, E, *pred_map, F_(1.0 / tau), F_(NORM_EPS), code)),
        ("cpc_norm_rows_bwd", "targets", 3 * R * E * size + 4 * R,
         lambda: _hip.call("cpc_norm_rows_bwd", P(n.tn, tg), P(n.inv_t), P(gt, tg), R, E, *top_map, F_(1.0), F_(NORM_EPS), code)),
    ]
    if "kernel" in parts:
        for name, which, moved, fn in rows:
            ms = _time(fn, args.launches)
            print(json.dumps({"part": "kernel", "kernel": name, "rows": which, "dtype": args.dtype, "n_rows": R, "E": E,
                              "us": round(ms * 1e3, 2), "mb_moved": round(moved / 1e6, 3),
                              "gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1)}), flush=True)
    if "chain" in parts:
        med = lambda v: sorted(v)[len(v) // 2]
        for all_t in (False, True):
            run = eng.nce_all_forward_backward if all_t else eng.nce_forward_backward
            linear = lambda: run(False, 1.0, score="linear")
            normalized = lambda: run(False, 1.0, score="normalized", temperature=tau)
            us_l, us_n = [], []
            for _ in range(args.rounds):
                us_l.append(round(_time(linear, args.chain_launches) * 1e3, 2))
                us_n.append(round(_time(normalized, args.chain_launches) * 1e3, 2))
            print(json.dumps({"part": "chain", "all_timesteps": all_t, "fused_route": bool(all_t and eng.fused_scores_ok()),
                              "dtype": args.dtype, "B": B, "K": K, "E": E, "launches": args.chain_launches, "linear_us": us_l,
                              "normalized_us": us_n, "median_difference_us": round(med(us_n) - med(us_l), 2)}), flush=True)
    del eng, model
    torch.cuda.empty_cache()


def trainer_ms(args, device, normalized, tag):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction,
                                                               linear_score_function)

    class Meter:
        def update(self, v):
            pass

    class Logger:
        def __init__(self):
            self.loss_meter, self.score_meter, self.marks = Meter(), Meter(), []

        def log(self, step):
            self.marks.append(time.perf_counter())

    B = args.batch
    model = build_model("bf16", device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    fn = NormalizedScoreFunction(args.temperature) if normalized else linear_score_function
    with contextlib.redirect_stdout(sys.stderr):
        tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0, score_function=fn,
                                          prediction_steps=12, ar_size=256)
        tr.verbose = False
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=args.warmup + args.steps + 1)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    ms = (marks[-1] - marks[args.warmup]) / n * 1e3
    print(json.dumps({"part": "trainer", "run": tag, "score": "normalized" if normalized else "linear", "dtype": "bf16", "B": B,
                      "ms_per_step": round(ms, 4), "steps_timed": n}), flush=True)
    del model, tr
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=0.1)
    ap.add_argument("--parts", default="kernel,chain,trainer")
    ap.add_argument("--launches", type=int, default=2000, help="back-to-back launches per timed kernel window")
    ap.add_argument("--chain-launches", type=int, default=200, help="back-to-back calls per timed chain window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernel" in parts or "chain" in parts:
        kernel_and_chain(args, device, parts)
    if "trainer" in parts:
        a = trainer_ms(args, device, False, "linear A")
        n = trainer_ms(args, device, True, "normalized")
        b = trainer_ms(args, device, False, "linear B")
        spread, diff = abs(a - b), n - (a + b) / 2
        print(json.dumps({"part": "trainer", "aa_spread_ms": round(spread, 4), "normalized_minus_linear_ms": round(diff, 4),
                          "resolved": abs(diff) > spread}), flush=True)


if __name__ == "__main__":
    main()
