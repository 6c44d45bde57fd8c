"""The negative bank at the headline batch (B = 256, K = 12, E = 512).

Prints one JSON line per measurement:
  chain    per-call time of the whole loss chain on random operands — score GEMM, loss launches, both contractions — in-batch
           (cpc_nce_loss, 2 launches) and banked (cpc_nce_loss_banked, 3 launches) for M in --slots-back, M + 1 slots all valid, plus
           the copy of the operands into the ring; mean of --launches back-to-back chains between two events, the chains alternate
           for --rounds windows each; per stage as well (scores / loss / contractions alone).
  nsplit   the target contraction alone (the batched TN GEMM that reduces over the ring's (M + 1) B rows), direct (nsplit = 1, output
           in the storage dtype) against --nsplit f32 slabs + one cpc_reduce_slabs into an f32 [B][K][E] buffer (bf16 storage would
           need a cast to the storage dtype on top, which is not timed: the slab route's figure is a lower bound there).
  trainer  ms per step of ContrastiveEstimationTrainer.train (bf16, AudioEncoder 5 x 512, GRU 256, 20480-sample clips) with
           negative_bank = None twice (the A/A spread) and with every M in --slots-back.

Usage: python tools/negative_bank_bench.py [--batch 256] [--slots-back 1,4,16] [--parts chain,nsplit,trainer]
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
    B, K, E, P, U = args.batch, 12, 512, _hip.ptr, C.c_ulonglong
    ld = (B + 7) // 8 * 8
    gen = torch.Generator(device=device).manual_seed(1)
    out = torch.zeros(8, device=device)
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        code = _hip.dtype_code(dt)
        # operands in the engine's layouts: predictions [B][K][E], targets [B][K][E] (rows of ld K E), gradients alike
        pred = (torch.randn(B, K, E, device=device, generator=gen) * 0.1).to(dt)
        targ = (torch.randn(B, K, E, device=device, generator=gen) * 0.1).to(dt)
        dpred, dtarg = torch.zeros_like(pred), torch.zeros_like(targ)
        dST = torch.zeros(K, B, ld, device=device, dtype=dt)

        def stages(slots):
            N = slots * B
            ring = (torch.randn(N, K, E, device=device, generator=gen) * 0.1).to(dt)
            S = torch.zeros(K, N, ld, device=device)
            dS = torch.zeros(K, N, ld, device=device, dtype=dt)
            banked = slots > 1
            ws = torch.empty(int(_hip.lib().cpc_nce_banked_workspace_floats(B, K, slots) if banked else
                                 _hip.lib().cpc_nce_workspace_floats(B, K)), device=device)
            valid = (1 << slots) - 1

            def store():
                ring[:B].copy_(pred)

            def scores():
                _hip.gemm_nt(P(ring), P(targ), P(S), N, B, E, K * E, K * E, ld, code, a_batch=E, b_batch=E, c_batch=N * ld, batch=K,
                             flags=_hip.GEMM_OUT_F32)

            def loss():
                if banked:
                    _hip.call("cpc_nce_loss_banked", P(S), P(dS), P(dST), P(out), P(ws), B, K, ld, slots, 0, U(valid), 1, C.c_float(1.0), code)
                else:
                    _hip.call("cpc_nce_loss", P(S), P(dS), P(dST), P(out), P(ws), B, K, ld, 1, C.c_float(1.0), code)

            def grads():
                _hip.gemm_tn(P(dST), P(targ), P(dpred), B, B, E, ld, K * E, K * E, code, a_batch=B * ld, b_batch=E, c_batch=E, batch=K)
                _hip.gemm_tn(P(dS), P(ring), P(dtarg), N, B, E, ld, K * E, K * E, code, a_batch=N * ld, b_batch=E, c_batch=E, batch=K)

            def chain():
                if banked:
                    store()
                scores()
                loss()
                grads()
            return {"chain": chain, "scores": scores, "loss": loss, "contractions": grads, "store": store}

        runs = {"in_batch": stages(1)}
        for m in args.slots_back:
            runs[f"M{m}"] = stages(m + 1)
        us = {k: {s: [] for s in v} for k, v in runs.items()}
        for _ in range(args.rounds):          # the chains alternate: the spread of a chain's own windows says what a difference is worth
            for k, v in runs.items():
                for s, fn in v.items():
                    us[k][s].append(round(_time(fn, args.launches) * 1e3, 2))
        print(json.dumps({"part": "chain", "dtype": name, "B": B, "K": K, "E": E, "launches": args.launches, "us": us}), flush=True)


def nsplit_times(args, device):
    B, K, E, P, L = args.batch, 12, 512, _hip.ptr, C.c_longlong
    ld = (B + 7) // 8 * 8
    gen = torch.Generator(device=device).manual_seed(2)
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        code = _hip.dtype_code(dt)
        blk = 64 if dt == torch.bfloat16 else 32
        for m in args.slots_back:
            N = (m + 1) * B
            ring = (torch.randn(N, K, E, device=device, generator=gen) * 0.1).to(dt)
            dS = (torch.randn(K, N, ld, device=device, generator=gen) * 1e-3).to(dt)
            dtarg = torch.zeros(B, K, E, device=device, dtype=dt)
            out32 = torch.zeros(B, K, E, device=device)
            slabs = torch.zeros(max(args.nsplit), B, K, E, device=device)

            def direct():
                _hip.gemm_tn(P(dS), P(ring), P(dtarg), N, B, E, ld, K * E, K * E, code, a_batch=N * ld, b_batch=E, c_batch=E, batch=K)

            def split(n):
                chunk = -(-(-(-N // n)) // blk) * blk

                def run():
                    _hip.gemm_tn(P(dS), P(ring), P(slabs), N, B, E, ld, K * E, K * E, code, a_batch=N * ld, b_batch=E, c_batch=E, batch=K,
                                 nsplit=n, m_chunk=chunk, slab_stride=B * K * E, flags=_hip.GEMM_OUT_F32)
                    _hip.call("cpc_reduce_slabs", P(slabs), P(out32), B, K * E, n, L(B * K * E), 1, L(1), L(K * E), L(0))
                return run

            runs = {"nsplit1": direct}
            runs.update({f"nsplit{n}": split(n) for n in args.nsplit if n * blk <= N})
            us = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    us[k].append(round(_time(fn, args.launches) * 1e3, 2))
            direct()
            ref = dtarg.float().clone()
            err = {}
            for k, fn in runs.items():          # the routes agree (the slab route sums in f32, the direct one rounds once to the storage dtype)
                if k != "nsplit1":
                    fn()
                    err[k] = float((out32 - ref).abs().max() / ref.abs().max())
            print(json.dumps({"part": "nsplit", "dtype": name, "B": B, "K": K, "E": E, "rows": N, "us": us, "max_rel_diff": err}), flush=True)


def trainer_ms(args, device, bank, tag):
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
                                          ar_size=256, file_batch_size=8)
        tr.verbose = False
        tr.negative_bank = bank
        torch.cuda.synchronize()
        tr.train(batch_size=B, epochs=1000, lr=1e-4, num_workers=0, max_steps=args.warmup + args.steps + 1)
        torch.cuda.synchronize()
    marks = logger.marks
    n = len(marks) - 1 - args.warmup
    print(json.dumps({"part": "trainer", "run": tag, "negative_bank": bank, "dtype": "bf16", "B": B,
                      "ms_per_step": round((marks[-1] - marks[args.warmup]) / n * 1e3, 4), "steps_timed": n}), flush=True)
    del model, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--slots-back", default="1,4,16", help="the M values measured")
    ap.add_argument("--parts", default="chain,nsplit,trainer")
    ap.add_argument("--nsplit", default="2,4,8", help="slab counts of the nsplit part")
    ap.add_argument("--launches", type=int, default=1000, help="back-to-back chains per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30, help="at least the largest M: a banked step costs its full price once the ring is full")
    args = ap.parse_args()
    args.slots_back = [int(m) for m in args.slots_back.split(",")]
    args.nsplit = [int(n) for n in args.nsplit.split(",")]
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "chain" in parts:
        chain_times(args, device)
    if "nsplit" in parts:
        nsplit_times(args, device)
    if "trainer" in parts:
        trainer_ms(args, device, None, "no bank A")
        for m in args.slots_back:
            trainer_ms(args, device, m, f"M{m}")
        trainer_ms(args, device, None, "no bank B")


if __name__ == "__main__":
    main()
