"""What the k-means units cost (clustering.KMeans; DESIGN.md, "K-means units").

N = 359 902 rows of D = 256 (the frame count of tools/extract_time.py's hour of audio), seeded N(0, 1) rows around K seeded means, K in
{64, 512}, rows in f32 and in bf16.  Per (K, dtype) one JSON line:
  assign     ms per cpc_kmeans_assign (labels and distances) against the torch route on the same device and data:
             v = addmm(cnorm, x, c^T, alpha=-2), (min, argmin) over its rows, dist = max(min + |x|^2, 0); bf16 rows are widened by
             x.float() inside the timed region, since the centres must stay f32.  The torch route writes and re-reads the N x K f32 matrix.
  iteration  ms per (cpc_kmeans_assign, cpc_kmeans_update) against the torch route's assignment plus index_add_ sums, bincount counts,
             the empty-cluster rule, the norms and the inertia.
Device events around --reps calls per window, --rounds windows per route, the two routes alternating in one process after a warm-up
of both.  tflops: 2 N K D over the assignment's time; peak_fraction: that over the 157 TFLOPS f32-MFMA peak.  labels_equal: the share
of rows on which the two routes agree (they differ where two centres are nearer to each other than the rounding of either route).

Usage: python tools/kmeans_time.py [--rows 359902] [--dim 256] [--clusters 64 512] [--reps 50] [--rounds 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cpc_audio_amd  # noqa: E402,F401
from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.clustering import KMeans  # noqa: E402

F32_MFMA_PEAK = 157e12
LL = C.c_longlong


def _timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _median(vals):
    return sorted(vals)[len(vals) // 2]


def torch_assign(x, centers, cnorm):
    xf = x.float()
    v = torch.addmm(cnorm, xf, centers.t(), alpha=-2.0)
    m, labels = v.min(1)
    return labels, (m + (xf * xf).sum(1)).clamp_min(0.0), xf


def torch_iteration(x, centers, cnorm):
    labels, dist, xf = torch_assign(x, centers, cnorm)
    K = centers.shape[0]
    sums = torch.zeros_like(centers).index_add_(0, labels, xf)
    counts = torch.bincount(labels, minlength=K)
    new = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], centers)
    return new, (new * new).sum(1), counts, dist.double().sum()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=359902)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--clusters", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, D = args.rows, args.dim
    g = torch.Generator(device=dev).manual_seed(0)
    for K in args.clusters:
        means = torch.randn(K, D, device=dev, generator=g)
        owner = torch.randint(0, K, (N,), device=dev, generator=g)
        x32 = means[owner] + torch.randn(N, D, device=dev, generator=g)
        for dt in (torch.float32, torch.bfloat16):
            x = x32.to(dt)
            km = KMeans(K, iterations=1, seed=0)
            run = km._prepare(x)
            code = _hip.dtype_code(dt)

            def hip_assign():
                _hip.call("cpc_kmeans_assign", _hip.ptr(x), code, LL(N), D, LL(D), _hip.ptr(run.centers), _hip.ptr(run.cnorm), K,
                          _hip.ptr(run.labels), _hip.ptr(run.dist))

            # an iteration that does not move the centres it starts from, so that every repetition does the same work
            new_c, new_n = torch.empty_like(run.centers), torch.empty_like(run.cnorm)

            def hip_iteration():
                hip_assign()
                _hip.call("cpc_kmeans_update", _hip.ptr(x), code, LL(N), D, LL(D), _hip.ptr(run.labels), _hip.ptr(run.dist),
                          _hip.ptr(run.centers), K, _hip.ptr(run.scratch), LL(run.scratch_bytes), _hip.ptr(new_c), _hip.ptr(new_n),
                          _hip.ptr(run.counts), _hip.ptr(run.inertia))

            routes = {"assign": (hip_assign, lambda: torch_assign(x, run.centers, run.cnorm)),
                      "iteration": (hip_iteration, lambda: torch_iteration(x, run.centers, run.cnorm))}
            line = {"N": N, "D": D, "K": K, "dtype": str(dt).replace("torch.", ""), "reps": args.reps}
            for part, (ours, theirs) in routes.items():
                ours()
                theirs()
                torch.cuda.synchronize()
                ms = {"hip": [], "torch": []}
                for _ in range(args.rounds):
                    ms["hip"].append(round(_timed(ours, args.reps), 4))
                    ms["torch"].append(round(_timed(theirs, args.reps), 4))
                line[part] = {"ms": ms, "hip_median": _median(ms["hip"]), "torch_median": _median(ms["torch"]),
                              "speedup": round(_median(ms["torch"]) / _median(ms["hip"]), 3)}
            t = line["assign"]["hip_median"] * 1e-3
            line["tflops"] = round(2.0 * N * K * D / t / 1e12, 2)
            line["peak_fraction"] = round(2.0 * N * K * D / t / F32_MFMA_PEAK, 4)
            hip_assign()
            labels_t, dist_t, _ = torch_assign(x, run.centers, run.cnorm)
            torch.cuda.synchronize()
            line["labels_equal"] = round(float((labels_t == run.labels.long()).double().mean()), 6)
            line["dist_max_abs_diff"] = float((dist_t - run.dist).abs().max())
            line["scratch_MB"] = round(run.scratch_bytes / 1e6, 2)
            print(json.dumps(line), flush=True)
            del x, run, new_c, new_n


if __name__ == "__main__":
    main()
