"""Difference scores at the bench size (BASELINE configs[1]: AudioEncoder 5 x 512, GRU 256, K = 12, B = 256, 20480-sample clips).

Prints one JSON line per measurement:
  kernel   per-launch time of cpc_diff_scores / cpc_diff_scores_bwd in the default and the all-timesteps layout, on the engine's own
           buffers after a real forward pass (mean of --launches back-to-back launches between two events), with the fraction of
           the 157.3 TF f32 vector peak (2 FLOP per (pair, feature): one subtraction and one fma).  Each pair costs two VALU issue
           slots (v_pk_add_f32 + v_pk_fma_f32) where the peak counts one fma as two FLOP, so 50 % of that peak is the issue ceiling.
  trainer  ms per step of ContrastiveEstimationTrainer.train with difference_score_function + Adam: the engine route, the generic
           route with the same kernels (global_negatives=True keeps it there), and the generic route with the reference's
           broadcast expression (the route before the difference kernels existed), if it fits in memory (reported if not).

Usage: python tools/diff_score_bench.py [--dtype bf16|fp32] [--batch 256] [--parts kernel,trainer] [--old-steps 4]
"""
import argparse
import contextlib
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

PEAK_F32_VECTOR = 157.3e12
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


def kernel_times(args, device):
    import ctypes as C
    model = build_model(args.dtype, device)
    B = args.batch
    eng = model.engine(B, L_CLIP)
    x = torch.randn(B, L_CLIP, device=device) * 0.1
    eng.forward(x)
    K, E, code, P, Lq = eng.K, eng.E, eng.code, _hip.ptr, C.c_longlong
    R = B * K
    # the loss of both branches once: real upstream gradients in dS / dS_all
    eng.nce_forward_backward(False, 1.0, score="difference")
    eng.nce_all_forward_backward(False, 1.0, score="difference")
    torch.cuda.synchronize()
    ld, ld_all = eng.ldS, eng.ldS_all
    G, GT = eng.dS.clone(), eng.dST.clone()
    Ga, GTa = eng.dS_all.clone(), eng.dST_all.clone()
    sums = torch.empty(2, R, device=device)
    work_d, work_a = 2.0 * K * B * B * E, 2.0 * R * R * E
    rows = [
        ("cpc_diff_scores", "default", work_d, lambda: eng.diff_scores(eng.S, eng.ST)),
        ("cpc_diff_scores", "all_timesteps", work_a, lambda: eng.diff_scores_all(eng.S_all, eng.ST_all)),
        ("cpc_diff_scores_bwd", "default", 0.0,
         lambda: _hip.call("cpc_diff_scores_bwd", P(G), P(eng.S), P(sums[0]), P(GT), P(eng.ST), P(sums[1]), B, B, ld, Lq(B * ld), K, code)),
        ("cpc_diff_scores_bwd", "all_timesteps", 0.0,
         lambda: _hip.call("cpc_diff_scores_bwd", P(Ga), P(eng.S_all), P(sums[0]), P(GTa), P(eng.ST_all), P(sums[1]), R, R, ld_all,
                           Lq(0), 1, code)),
    ]
    for name, branch, work, fn in rows:
        ms = _time(fn, args.launches)
        rec = {"part": "kernel", "kernel": name, "branch": branch, "dtype": args.dtype, "B": B, "K": K, "E": E, "us": round(ms * 1e3, 2)}
        if work:
            rec["gflop"] = round(work / 1e9, 3)
            rec["tflops"] = round(work / (ms * 1e-3) / 1e12, 2)
            rec["fraction_of_f32_vector_peak"] = round(work / (ms * 1e-3) / PEAK_F32_VECTOR, 4)
        else:
            mats = 2 * (K * B * B if branch == "default" else R * R)
            moved = mats * (2 * eng.dS.element_size() + 4)          # g read + G written (storage type) + s read (f32)
            rec["gb_per_s"] = round(moved / (ms * 1e-3) / 1e9, 1)
        print(json.dumps(rec), flush=True)
    del eng, model
    torch.cuda.empty_cache()


def broadcast_difference_scores(predicted_z, targets):
    """The reference's expression (contrastive_estimation_training.py:25-33), kept here as the before-measurement only."""
    diff = predicted_z.unsqueeze(3).unsqueeze(4) - targets.permute(1, 0, 2).unsqueeze(0).unsqueeze(1)
    return 1 / torch.sum(diff ** 2, dim=2)


def trainer_ms(args, device, route, all_t):
    from cpc_audio_amd.audio_dataset import SyntheticAudioDataset
    from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, difference_score_function

    class Meter:
        def update(self, v):
            pass

    class Logger:
        def __init__(self):
            self.loss_meter, self.score_meter, self.marks = Meter(), Meter(), []

        def log(self, step):
            self.marks.append(time.perf_counter())

    B = args.batch
    steps, warmup = (args.steps, args.warmup) if route != "broadcast" else (args.old_steps, 1)
    model = build_model(args.dtype, device)
    ds = SyntheticAudioDataset(B * 4, L_CLIP, seed=3, device=device)
    logger = Logger()
    fn = broadcast_difference_scores if route == "broadcast" else difference_score_function
    rec = {"part": "trainer", "route": route, "all_timesteps": all_t, "dtype": args.dtype, "B": B}
    torch.cuda.reset_peak_memory_stats(device)
    try:
        with contextlib.redirect_stdout(sys.stderr):
            tr = ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=device, regularization=1.0,
                                              score_over_all_timesteps=all_t, score_function=fn, prediction_steps=12, ar_size=256)
            tr.verbose = False
            tr.global_negatives = route == "generic"          # single process: only keeps difference scores off the engine route
            rec["engine_route"] = tr._engine_difference()
            torch.cuda.synchronize()
            tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=warmup + steps + 1)
            torch.cuda.synchronize()
        marks = logger.marks
        rec["ms_per_step"] = round((marks[-1] - marks[warmup]) / (len(marks) - 1 - warmup) * 1e3, 3)
        rec["steps_timed"] = len(marks) - 1 - warmup
    except torch.cuda.OutOfMemoryError as e:
        rec["ms_per_step"] = None
        rec["did_not_fit"] = str(e).splitlines()[0][:200]
    rec["peak_gib"] = round(torch.cuda.max_memory_allocated(device) / 2**30, 2)
    print(json.dumps(rec), flush=True)
    del model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parts", default="kernel,trainer")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-steps", type=int, default=4, help="timed steps of the broadcast route")
    ap.add_argument("--routes", default="engine,generic,broadcast")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernel" in parts:
        kernel_times(args, device)
    if "trainer" in parts:
        for all_t in (False, True):
            for route in args.routes.split(","):
                trainer_ms(args, device, route, all_t)


if __name__ == "__main__":
    main()
