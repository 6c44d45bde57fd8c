"""Log-mel front end at configs[2]'s clip size (B = 128 clips of 97 024 samples) beside the CQT front end.

Prints one JSON line per measurement, each the mean of --launches back-to-back calls between two HIP events, --rounds windows:
  dft       the framed DFT GEMM of MelSpectrogram.transform (with cpc_split3_bf16 in the bf16x3 route), ms and TF/s over 2 M N K
            (N = n_fft + 2 useful columns; K = n_fft, 3 n_fft in bf16x3), fp32 and bf16x3.
  kernel    cpc_mel_pointwise alone on that spectrum, ms and the fraction of 8 TB/s over the bytes it must move: every spectrum row
            once (2 n_freq floats) plus the output.  The spectrum (782 MB at n_fft = 2048) is beyond every cache.
  module    MelPreprocessingModule.forward (GEMM + kernel + allocations), both precisions.
  cqt       PreprocessingModule(cqt_default_dict, phase=True).forward on the same clips, both precisions.
  step      one configs[2]-shaped train step (scalogram_resnet_architecture_7 + GRU, bf16, FusedAdam) with each front end.  The CQT
            gives 629 frames from 97 024 samples; the mel step runs on clips of n_fft + 629 hop samples, so that both encoders see a
            (B, 2, 256, 629) input.
Shapes: n_fft 2048, hop 128, 256 bands, delta (--shape big) and mel_default_dict without delta (--shape default).

Usage: python tools/mel_bench.py [--batch 128] [--parts dft,kernel,module,cqt,step]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cpc_audio_amd import _hip, configs  # noqa: E402
from cpc_audio_amd.audio_model import AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.engine import FusedAdam  # noqa: E402
from cpc_audio_amd.mel_spectrogram import MelPreprocessingModule, mel_default_dict  # noqa: E402
from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder, cqt_default_dict  # noqa: E402

L_CLIP = 97024
SHAPES = {"big": (dict(mel_default_dict, n_fft=2048, win_length=2048, hop_length=128, n_mels=256, f_min=30.0), True),
          "default": (dict(mel_default_dict), False)}


def _window(fn, launches):
    """Mean ms of ``launches`` calls between two events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def _rounds(fn, args):
    return [round(_window(fn, args.launches), 4) for _ in range(args.rounds)]


def front_end(args, device, shape, parts):
    mel_dict, delta = SHAPES[shape]
    B = args.batch
    g = torch.Generator().manual_seed(1)
    wave = (torch.randn(B, L_CLIP, generator=g) * 0.1).to(device).unsqueeze(1)
    pre = MelPreprocessingModule(mel_dict, delta=delta).to(device)
    mel = pre.mel
    Tn = mel.frames(L_CLIP)
    base = {"shape": shape, "B": B, "L": L_CLIP, "n_fft": mel.n_fft, "hop": mel.hop_length, "n_mels": mel.n_mels, "delta": delta, "frames": Tn}
    for precision in ("fp32", "bf16x3"):
        mel.precision = precision
        spec, _, lds = mel.transform(wave)
        if "dft" in parts:
            ms = _rounds(lambda: mel.transform(wave), args)
            flops = 2.0 * B * Tn * (mel.n_fft + 2) * mel.n_fft * (3 if precision == "bf16x3" else 1)
            med = sorted(ms)[len(ms) // 2]
            print(json.dumps(dict(base, part="dft", precision=precision, ms=ms, TF_per_s=round(flops / (med * 1e-3) / 1e12, 1))), flush=True)
        if "kernel" in parts and precision == "fp32":
            ms = _rounds(lambda: mel.pointwise(spec, Tn, delta=delta), args)
            W, Cc = (Tn - 1, 2) if delta else (Tn, 1)
            nbytes = 4.0 * B * (Tn * 2 * mel.n_freq + W * mel.n_mels * Cc)
            med = sorted(ms)[len(ms) // 2]
            print(json.dumps(dict(base, part="kernel", ms=ms, MB=round(nbytes / 1e6, 1), GB_per_s=round(nbytes / (med * 1e-3) / 1e9, 1),
                                  fraction_of_8TB_per_s=round(nbytes / (med * 1e-3) / 8e12, 3))), flush=True)
        if "module" in parts:
            print(json.dumps(dict(base, part="module", precision=precision, ms=_rounds(lambda: pre(wave), args))), flush=True)
        del spec
        torch.cuda.empty_cache()
    if "cqt" in parts and shape == "big":
        cq = PreprocessingModule(cqt_dict=cqt_default_dict, phase=True).to(device)
        for precision in ("fp32", "bf16x3"):
            cq.cqt.precision = precision
            out = cq(wave)
            print(json.dumps({"part": "cqt", "precision": precision, "B": B, "L": L_CLIP, "output": list(out.shape),
                              "ms": _rounds(lambda: cq(wave), args)}), flush=True)
        del cq, out
        torch.cuda.empty_cache()


def train_step(args, device, front):
    B, V, K = args.batch, 60, 16
    torch.manual_seed(0)
    if front == "cqt":
        pre = PreprocessingModule(cqt_dict=cqt_default_dict, phase=True).to(device)
        pre.cqt.precision = "bf16x3"
        L = L_CLIP
    else:
        mel_dict, _ = SHAPES["big"]
        pre = MelPreprocessingModule(mel_dict, delta=True).to(device)
        pre.mel.precision = "bf16x3"
        L = mel_dict["n_fft"] + 629 * mel_dict["hop_length"]
    enc = ScalogramResidualEncoder(args_dict=configs.fresh(configs.scalogram_resnet_architecture_7), preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=V, prediction_steps=K,
                                       compute_dtype="bf16").to(device)
    g = torch.Generator().manual_seed(1)
    wave = (torch.randn(B, L, generator=g) * 0.1).to(device)
    opt = None

    def step():
        nonlocal opt
        x = pre(wave.unsqueeze(1))
        eng = model.engine_for(x)
        if opt is None:
            opt = FusedAdam(model, lr=1e-4)
        out = eng.loss_and_grads(x, softplus=True, regularization=1.0)
        opt.step()
        return out, x

    for _ in range(3):
        out, x = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, x = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(json.dumps({"part": "step", "front_end": front, "B": B, "L": L, "input": list(x.shape), "ms_per_step": round(ms, 3),
                      "loss": float(out[0])}), flush=True)
    del model, opt, pre
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--parts", default="dft,kernel,module,cqt,step")
    ap.add_argument("--shape", default="big,default")
    ap.add_argument("--launches", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    parts = args.parts.split(",")
    for shape in args.shape.split(","):
        front_end(args, device, shape, parts)
    if "step" in parts:
        for front in ("cqt", "mel", "cqt", "mel"):
            train_step(args, device, front)


if __name__ == "__main__":
    main()
