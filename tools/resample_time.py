"""What converting a corpus at load costs: --minutes (default 60) of synthetic 44.1 kHz stereo int16 to 16 kHz mono int16 through
DeviceAudioDataset(convert=True)'s chunked path, one file per minute.

Prints one JSON line per measurement:
  device  per round (the first is a warm-up and is not reported): the cpc_resample launches of the load between HIP events (the sum over
          the chunks, ms; GB/s of source read = frames x 4 bytes over that time), and the whole constructor on the host clock, which
          also holds the host-side concatenation of a chunk and its upload.
  host    scipy.signal.upfirdn with the same prototype on one minute (downmix in numpy included), scaled to --minutes; skipped if scipy
          is absent.

Usage: python tools/resample_time.py [--minutes 60] [--rounds 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cpc_audio_amd  # noqa: E402,F401
from cpc_audio_amd import _hip, resampling  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset  # noqa: E402

ORIG, NEW = 44100, 16000


def _prototype(taps, L, W):
    """h [2 W L + 1] back from the polyphase table: taps[p][t] = h[p - (t - W) L + W L]."""
    h = np.zeros(2 * W * L + 1)
    p, t = np.meshgrid(np.arange(L), np.arange(2 * W + 1), indexing="ij")
    j = p - (t - W) * L + W * L
    inside = (j >= 0) & (j <= 2 * W * L)
    h[j[inside]] = taps[inside]
    return h


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--chunk-mb", type=int, default=256)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    minute = rng.integers(-32768, 32768, size=(60 * ORIG, 2), dtype=np.int64).astype(np.int16)
    files = [minute] * args.minutes
    source_bytes = minute.nbytes * args.minutes
    taps, L, M, W = resampling.resample_taps(ORIG, NEW)
    timer = _hip.KernelTimer(only={"cpc_resample"})
    _hip.set_timer(timer)
    rows = []
    for r in range(args.rounds):
        timer.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = DeviceAudioDataset(arrays=files, array_rates=ORIG, item_length=20480, sampling_rate=NEW, convert=True, channels="mean",
                                storage="int16", device=device, convert_chunk_bytes=args.chunk_mb << 20)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        launches, ms, _ = timer.summary()["cpc_resample"]
        if r:
            rows.append({"launches": launches, "kernel_ms": round(ms, 3), "source_GB_per_s": round(source_bytes / (ms * 1e-3) / 1e9, 1),
                         "constructor_s": round(wall, 2)})
        outputs = sum(ds.file_lengths)
        del ds
    _hip.set_timer(None)
    print(json.dumps({"part": "device", "minutes": args.minutes, "source_MB": round(source_bytes / 1e6, 1), "outputs": outputs,
                      "taps": [L, 2 * W + 1], "multiply_adds": outputs * (2 * W + 1), "rounds": rows}), flush=True)
    if args.skip_host:
        return
    try:
        from scipy.signal import upfirdn
    except ImportError:
        print(json.dumps({"part": "host", "skipped": "scipy is not installed"}), flush=True)
        return
    h = _prototype(taps.astype(np.float64), L, W)
    upfirdn(h, np.zeros(1000), L, M)
    t0 = time.perf_counter()
    mono = (minute[:, 0].astype(np.float32) + minute[:, 1].astype(np.float32)) / np.float32(2.0)
    y = upfirdn(h, mono, L, M)
    y = np.rint(np.clip(y, -32768.0, 32767.0)).astype(np.int16)
    one = time.perf_counter() - t0
    print(json.dumps({"part": "host", "one_minute_s": round(one, 3), "scaled_to_minutes": args.minutes,
                      "scaled_s": round(one * args.minutes, 1), "threads": 1, "outputs_per_minute": int(len(y))}), flush=True)


if __name__ == "__main__":
    main()
