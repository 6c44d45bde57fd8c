"""What whole-recording feature extraction costs (feature_extraction.FeatureExtractor; DESIGN.md, "Whole-recording feature extraction").

One hour (--hours) of seeded 16 kHz int16 audio in recordings of mixed length from 3 s to 10 min, the default model (5 x 512 encoder,
GRU 256) in bf16, float32 feature stores with pooling.  Prints one JSON line per measurement:
  extract  device events around whole ``extract`` calls after a warm-up call, --rounds windows, alternating in the same process with
           what the model offered for z alone before: a loop of stand-alone ``encoder(x)`` calls over
           windows of the same size cut by DeviceAudioDataset.device_batch, ``streams`` windows per call.  frames/s, x real time.
  emit     the bytes cpc_feature_emit moves per call of ``extract`` (source rows read, feature rows written); its kernel time comes
           from a separate run under the profiler:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/extract_time.py --once
  sweep    (--sweep) ms per ``extract`` over streams x chunk_frames, --rounds windows each after a warm-up.

Usage: python tools/extract_time.py [--hours 1.0] [--streams 32] [--chunk-frames 1024] [--sweep] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cpc_audio_amd  # noqa: E402,F401
from cpc_audio_amd.audio_dataset import DeviceAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.feature_extraction import FeatureExtractor, plan_schedule  # noqa: E402

RATE = 16000


def _recordings(hours, seed=0):
    """Seeded int16 recordings, log-uniform lengths between 3 s and 10 min, until ``hours`` of audio are full."""
    rng = np.random.default_rng(seed)
    left, out = int(hours * 3600 * RATE), []
    while left > 0:
        n = min(left, int(RATE * np.exp(rng.uniform(np.log(3.0), np.log(600.0)))))
        out.append(rng.integers(-8000, 8000, size=n, dtype=np.int64).astype(np.int16))
        left -= n
    return out


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(vals):
    return sorted(vals)[len(vals) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--chunk-frames", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--once", action="store_true", help="a warm-up and two extract calls only (for a profiler run)")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = AudioPredictiveCodingModel(AudioEncoder(), AudioGRUModel(512, 256), enc_size=512, ar_size=256, visible_steps=100,
                                       prediction_steps=12, compute_dtype="bf16").to(device)
    recs = _recordings(args.hours)
    seconds = sum(len(r) for r in recs) / RATE
    ds, rf = int(model.encoder.downsampling_factor), int(model.encoder.receptive_field)
    R, Tc = args.streams, args.chunk_frames
    window = (Tc - 1) * ds + rf
    data = DeviceAudioDataset(arrays=recs, item_length=window, unique_length=Tc * ds, device=device, storage="int16")
    ex = FeatureExtractor(model, streams=R, chunk_frames=Tc)
    out = ex.extract(data)          # warm-up: the buffers are allocated here
    torch.cuda.synchronize()
    frames = out.total_frames
    if args.once:
        for _ in range(2):
            ex.extract(data)
        torch.cuda.synchronize()
        return
    # the stand-alone encoder call (all frames of a window; model.encode keeps the last visible + prediction steps only), on a copy of
    # the encoder so that its private engine and the model's do not take the parameters from each other
    encoder = AudioEncoder()
    encoder.load_state_dict(model.encoder.state_dict())
    encoder.compute_dtype = torch.bfloat16
    encoder = encoder.to(device)
    batches = [list(range(i, min(i + R, len(data)))) for i in range(0, len(data), R)]

    def encoder_loop():
        with torch.no_grad():
            for idx in batches:
                encoder(data.device_batch(idx).unsqueeze(1))

    encoder_loop()
    torch.cuda.synchronize()
    ms = {"extract": [], "encode_loop_z_only": []}
    for _ in range(args.rounds):
        ms["extract"].append(round(_timed(lambda: ex.extract(data)), 2))
        ms["encode_loop_z_only"].append(round(_timed(encoder_loop), 2))
    med = _median(ms["extract"])
    print(json.dumps({"part": "extract", "recordings": len(recs), "audio_s": round(seconds, 1), "frames": frames, "streams": R,
                      "chunk_frames": Tc, "steps": int(plan_schedule(*zip(*data.file_ranges()), rf, ds, R, Tc).table.shape[0]), "ms": ms,
                      "frames_per_s": round(frames / (med * 1e-3)), "x_real_time": round(seconds / (med * 1e-3)),
                      "encode_loop_windows": len(data), "buffers_MB": round(ex._engine.hbm_bytes() / 1e6, 1)}), flush=True)
    E, H = 512, 256
    print(json.dumps({"part": "emit", "bytes_read": frames * (E + H) * 2, "bytes_written": frames * (E + H) * 4,
                      "launches": "one per step; kernel time: see the profiler run"}), flush=True)
    if args.sweep:
        del ex, out
        for R_, Tc_ in ((16, 1024), (32, 512), (32, 1024), (32, 2048), (64, 256), (64, 512), (64, 1024), (128, 256), (128, 512), (256, 128),
                        (256, 256)):
            ex = FeatureExtractor(model, streams=R_, chunk_frames=Tc_)
            ex.extract(data)
            torch.cuda.synchronize()
            vals = [round(_timed(lambda: ex.extract(data)), 2) for _ in range(args.rounds)]
            print(json.dumps({"part": "sweep", "streams": R_, "chunk_frames": Tc_, "ms": vals,
                              "x_real_time": round(seconds / (_median(vals) * 1e-3)), "buffers_MB": round(ex._engine.hbm_bytes() / 1e6, 1)}),
                  flush=True)
            del ex
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
