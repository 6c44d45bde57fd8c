"""What a batch costs to produce at the headline size (B = 256 windows of 20480 samples: 21 MB of f32 written).

Prints one JSON line per measurement, the routes alternating in one process, --rounds windows each:
  kernels  cpc_window_gather alone for an int16 and for an f32 store (--hours of 16 kHz audio, windows --unique samples apart, random
           examples), beside torch's indexing ``device_data[idx]`` of a materialised (N, L) tensor, the route of SyntheticAudioDataset /
           TensorAudioDataset(device=...): mean of --launches back-to-back calls between two events.  Every call has an output of its own
           out of a ring of --ring, and an index list of its own (already on the device), so no call finds its rows in a cache.
           GB/s: bytes written plus bytes read (B L 4 + B L 2 or 4) over the median.
  batches  the whole host call, index upload and allocation included: DeviceAudioDataset.device_batch(list) and
           device_data[torch.as_tensor(list, device=...)], host clock around --launches calls that end in a synchronise.

Usage: python tools/dataset_feed_time.py [--batch 256] [--hours 1.0]
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
from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset  # noqa: E402

L_CLIP = 20480


def _events(fn, launches):
    """Mean us of ``launches`` calls fn(i) between two events."""
    for i in range(8):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def _host(fn, launches):
    """Mean us of ``launches`` calls fn(i) on the host clock, a synchronise at the end."""
    for i in range(8):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(launches):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / launches * 1e6


def _median(vals):
    return sorted(vals)[len(vals) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hours", type=float, default=1.0, help="audio in the store (16 kHz)")
    ap.add_argument("--unique", type=int, default=2048, help="samples between two windows")
    ap.add_argument("--rows", type=int, default=8192, help="rows of the materialised tensor (8192 x 20480 x 4 B = 671 MB)")
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    B, L, P = args.batch, L_CLIP, _hip.ptr
    rng = np.random.default_rng(0)
    samples = rng.integers(-32768, 32768, size=int(args.hours * 3600 * 16000), dtype=np.int64).astype(np.int16)
    sets = {"int16": DeviceAudioDataset(arrays=[samples], item_length=L, unique_length=args.unique, device=device, storage="int16"),
            "f32": DeviceAudioDataset(arrays=[samples], item_length=L, unique_length=args.unique, device=device, storage="float32")}
    del samples
    n = len(sets["int16"])
    gen = torch.Generator(device=device).manual_seed(0)
    resident = torch.randn(args.rows, L, device=device, generator=gen)
    outs = [torch.empty(B, L, device=device) for _ in range(args.ring)]
    lists = [rng.integers(0, n, size=B).tolist() for _ in range(args.launches)]
    row_lists = [rng.integers(0, args.rows, size=B).tolist() for _ in range(args.launches)]
    idx = [torch.tensor(v, dtype=torch.int64, device=device) for v in lists]
    row_idx = [torch.tensor(v, dtype=torch.int64, device=device) for v in row_lists]

    def gather_of(ds):
        code = 1 if ds.storage == "int16" else 0

        def run(i):
            _hip.call("cpc_window_gather", P(ds._store), code, ds._store_len, P(ds._starts_dev), n, P(idx[i % len(idx)]),
                      P(outs[i % args.ring]), B, L, L, ds._scale)
        return run

    def indexed(i):
        torch.index_select(resident, 0, row_idx[i % len(row_idx)], out=outs[i % args.ring])

    kernels = {"cpc_window_gather int16": gather_of(sets["int16"]), "cpc_window_gather f32": gather_of(sets["f32"]),
               "device_data[idx]": lambda i: resident[row_idx[i % len(row_idx)]], "index_select into a ring": indexed}
    batches = {"device_batch int16": lambda i: sets["int16"].device_batch(lists[i % len(lists)]),
               "device_batch f32": lambda i: sets["f32"].device_batch(lists[i % len(lists)]),
               "device_data[as_tensor(list)]": lambda i: resident[torch.as_tensor(row_lists[i % len(row_lists)], device=device)]}
    read = {"cpc_window_gather int16": 2}
    for part, fns, timer in (("kernels", kernels, _events), ("batches", batches, _host)):
        us = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                us[name].append(round(timer(fn, args.launches), 2))
        row = {"part": part, "B": B, "L": L, "examples": n, "store_MB": {k: round(d.hbm_bytes() / 1e6, 1) for k, d in sets.items()},
               "launches": args.launches}
        for name, vals in us.items():
            row[name] = {"us": vals}
            if part == "kernels":
                row[name]["GB_per_s"] = round(B * L * (4 + read.get(name, 4)) / (_median(vals) * 1e-6) / 1e9, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
