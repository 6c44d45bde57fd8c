"""The attention core at the bench size: per-launch times of the short-sequence kernels and the cpc_attn128_* ones, and the train step
of an attention context at 60 and 100 visible steps.

Prints one JSON line per measurement:
  kernel  per-launch time (mean of --launches back-to-back launches between two events, after one warm-up launch) of
          cpc_attn_fwd / cpc_attn_bwd at S = 60 and cpc_attn128_fwd / cpc_attn128_bwd at S = 60, 100 and 128, for B x heads = 2048
          (B = 256, C = 512, 8 heads of 64), bf16: the matrix-pipe kernels
  step    ms per train step (engine.loss_and_grads, mean of --steps after --warmup) of AudioEncoder + AttentionModel
          (attention_architecture_1 with sequence_length 100) at V = 60 and V = 100, K = 12, B = 256, 20480-sample clips, bf16

Usage: python tools/attention_bench.py [--parts kernel,step] [--launches 50] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

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


def kernel_times(args, device):
    B, C, heads = 256, 512, 8
    P = _hip.ptr
    for abi, S in (("cpc_attn", 60), ("cpc_attn128", 60), ("cpc_attn128", 100), ("cpc_attn128", 128)):
        qkv = torch.randn(B * S, 3 * C, device=device).to(torch.bfloat16)
        dout = torch.randn(B * S, C, device=device).to(torch.bfloat16)
        out = torch.empty(B * S, C, device=device, dtype=torch.bfloat16)
        probs = torch.empty(B * heads, S, S, device=device, dtype=torch.bfloat16)
        dqkv = torch.empty(B * S, 3 * C, device=device, dtype=torch.bfloat16)
        fwd = lambda: _hip.call(abi + "_fwd", P(qkv), P(out), P(probs), B, S, C, heads, 0.0, 0, 0, _hip.BF16)
        bwd = lambda: _hip.call(abi + "_bwd", P(qkv), P(probs), P(dout), P(dqkv), B, S, C, heads, 0.0, 0, 0, _hip.BF16)
        for what, fn in (("fwd", fwd), ("bwd", bwd)):
            ms = _time(fn, args.launches)
            print(json.dumps({"part": "kernel", "entry": f"{abi}_{what}", "S": S, "B_heads": B * heads, "head_size": C // heads,
                              "dtype": "bf16", "us_per_launch": round(ms * 1e3, 2)}), flush=True)


def step_times(args, device):
    from cpc_audio_amd import configs
    from cpc_audio_amd.attention_model import AttentionModel
    from cpc_audio_amd.audio_model import AudioEncoder, AudioPredictiveCodingModel
    B, K = 256, 12
    x = torch.randn(B, L_CLIP, device=device) * 0.1
    for V in (60, 100):
        torch.manual_seed(0)
        ar = AttentionModel(dict(configs.fresh(configs.attention_architecture_1), dropout=0.0, sequence_length=100))
        model = AudioPredictiveCodingModel(AudioEncoder(), ar, enc_size=512, ar_size=256, visible_steps=V, prediction_steps=K,
                                           compute_dtype="bf16").to(device)
        eng = model.engine(B, L_CLIP)
        step = lambda: eng.loss_and_grads(x, softplus=True, regularization=1.0)
        for _ in range(args.warmup):
            step()
        ms = _time(step, args.steps)
        print(json.dumps({"part": "step", "V": V, "K": K, "B": B, "context": "attention_architecture_1", "attention_entry": eng.ctx.attn_abi,
                          "dtype": "bf16", "ms_per_step": round(ms, 3)}), flush=True)
        del eng, model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,step")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    if "kernel" in parts:
        kernel_times(args, device)
    if "step" in parts:
        step_times(args, device)


if __name__ == "__main__":
    main()
