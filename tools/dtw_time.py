"""What the batched DTW of the ABX evaluation costs (abx.dtw_distance; DESIGN.md, "ABX discriminability").

N = 359 902 seeded N(0, 1) rows of D = 256 (the frame count of tools/extract_time.py's hour of audio), rows in f32 and in bf16, angular
metric, two workloads: 200 000 pairs with lengths uniform in 4 .. 24 and 20 000 pairs with lengths uniform in 64 .. 128.  Per (workload,
dtype) one JSON line comparing cpc_dtw (one launch over the pair table) with a torch route on the same device and the same pairs:
  1. the segments gathered into padded (P, Lmax, D) batches (one index_select per side), bf16 rows widened;
  2. bmm, the normalisation by the row norms, clamp, acos / pi;
  3. the recurrence as 2 Lmax - 1 anti-diagonal steps of tensor ops over (P, Lmax) rows of (cost, length), the result read at
     (La - 1, Lb - 1) of each pair.
The torch route runs in batches of --torch-batch pairs so that its (P, Lmax, Lmax) matrices fit; it writes and re-reads them, the fused
kernel keeps them in LDS.  Device events around --reps calls per window, --rounds windows per route, the two routes alternating in one
process after a warm-up of both.  dist_tflops: 2 D sum La Lb over the kernel's time; peak_fraction: that over the 157 TFLOPS f32-MFMA
peak (the kernel also computes the padding of its 32 x 32 tiles, which this does not count).  The two routes must agree on dist within
the test's bound on a sample of about 500 pairs: per pair tests/abx_reference.py's dtw_tolerance (the largest cell bound of the
angular distance plus the additions of the path), evaluated on the pair's own rows, holds each f32 route to float64, so the two may
differ by twice that; diff_over_bound is the largest difference over that allowance.

Usage: python tools/dtw_time.py [--rows 359902] [--dim 256] [--reps 3] [--rounds 3] [--short 200000] [--long 20000]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cpc_audio_amd  # noqa: E402,F401
from cpc_audio_amd import abx  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import abx_reference  # noqa: E402  (the bounds the tests use)

F32_MFMA_PEAK = 157e12


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


def torch_dtw(x, pairs, lmin, lmax, batch):
    """dist (P,) by the torch route; pairs int64 (P, 4) on the device."""
    out = torch.empty(pairs.shape[0], device=x.device, dtype=torch.float32)
    ar = torch.arange(lmax, device=x.device)
    inf = torch.tensor(float("inf"), device=x.device)
    for p0 in range(0, pairs.shape[0], batch):
        pr = pairs[p0:p0 + batch]
        P = pr.shape[0]
        la, lb = pr[:, 1], pr[:, 3]
        ia = pr[:, 0, None] + torch.minimum(ar[None, :], la[:, None] - 1)          # rows beyond a segment repeat its last row
        ib = pr[:, 2, None] + torch.minimum(ar[None, :], lb[:, None] - 1)
        a = x.index_select(0, ia.reshape(-1)).float().view(P, lmax, -1)
        b = x.index_select(0, ib.reshape(-1)).float().view(P, lmax, -1)
        cos = torch.bmm(a, b.transpose(1, 2)) / (a.norm(dim=2)[:, :, None] * b.norm(dim=2)[:, None, :])
        d = torch.acos(cos.clamp_(-1.0, 1.0)) / math.pi                            # (P, lmax, lmax)
        # anti-diagonal k holds the cells (i, k - i); row i of the state is the value of cell (i, k - i)
        prev_c = torch.full((P, lmax), float("inf"), device=x.device)              # diagonal k - 1
        prev2_c = torch.full((P, lmax), float("inf"), device=x.device)             # diagonal k - 2
        prev_l = torch.zeros((P, lmax), device=x.device, dtype=torch.int32)
        prev2_l = torch.zeros((P, lmax), device=x.device, dtype=torch.int32)
        res_c = torch.zeros(P, device=x.device)
        res_l = torch.ones(P, device=x.device, dtype=torch.int32)
        want_k = la + lb - 2
        for k in range(2 * lmax - 1):
            j = k - ar
            inside = (j >= 0) & (j < lmax)
            dk = d[:, ar, j.clamp(0, lmax - 1)]
            lf_c, lf_l = prev_c, prev_l                                            # (i, j - 1): row i of diagonal k - 1
            up_c, up_l = torch.roll(prev_c, 1, 1), torch.roll(prev_l, 1, 1)        # (i - 1, j): row i - 1 of diagonal k - 1
            dg_c, dg_l = torch.roll(prev2_c, 1, 1), torch.roll(prev2_l, 1, 1)      # (i - 1, j - 1): row i - 1 of diagonal k - 2
            up_c[:, 0] = inf
            dg_c[:, 0] = inf
            if k == 0:
                dg_c[:, 0] = 0.0
            lf_c = torch.where((j > 0)[None, :], lf_c, inf)
            use_dg = (dg_c <= up_c) & (dg_c <= lf_c)
            use_lf = ~use_dg & (lf_c <= up_c)
            m = torch.where(use_dg, dg_c, torch.where(use_lf, lf_c, up_c))
            ln = torch.where(use_dg, dg_l, torch.where(use_lf, lf_l, up_l)) + 1
            cur_c = torch.where(inside[None, :], dk + m, inf)
            hit = want_k == k
            if k >= 2 * lmin - 2:                                                  # (no pair ends on an earlier diagonal)
                row = (la - 1).clamp(max=lmax - 1)[:, None]
                res_c = torch.where(hit, cur_c.gather(1, row)[:, 0], res_c)
                res_l = torch.where(hit, ln.gather(1, row)[:, 0], res_l)
            prev2_c, prev2_l, prev_c, prev_l = prev_c, prev_l, cur_c, ln
        out[p0:p0 + P] = res_c / res_l
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=359902)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--short", type=int, default=200000)
    ap.add_argument("--long", type=int, default=20000)
    ap.add_argument("--torch-batch", type=int, default=0, help="pairs per batch of the torch route (0: 20000 short, 1000 long)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, D = args.rows, args.dim
    g = torch.Generator(device=dev).manual_seed(0)
    x32 = torch.randn(N, D, device=dev, generator=g)
    for name, P, lo, hi, batch in (("short", args.short, 4, 24, 20000), ("long", args.long, 64, 128, 1000)):
        batch = args.torch_batch or batch
        la = torch.randint(lo, hi + 1, (P,), device=dev, generator=g)
        lb = torch.randint(lo, hi + 1, (P,), device=dev, generator=g)
        # A segments from the first half of the rows, B segments from the second: no row is compared with itself (where cos is 1 up
        # to rounding, acos turns one ulp into 3e-4 and the two routes need not agree)
        half = N // 2
        af = (torch.rand(P, device=dev, generator=g) * (half - hi)).long().clamp(0, half - hi)
        bf = half + (torch.rand(P, device=dev, generator=g) * (N - half - hi)).long().clamp(0, N - half - hi)
        pairs = torch.stack([af, la, bf, lb], 1).contiguous()
        flops = 2.0 * D * float((la * lb).sum())
        for dt in (torch.float32, torch.bfloat16):
            x = x32.to(dt)
            ours = lambda: abx.dtw_distance(x, pairs)                              # noqa: E731
            theirs = lambda: torch_dtw(x, pairs, lo, hi, batch)                        # noqa: E731
            ours()
            theirs()
            torch.cuda.synchronize()
            ms = {"hip": [], "torch": []}
            for _ in range(args.rounds):
                ms["hip"].append(round(_timed(ours, args.reps), 4))
                ms["torch"].append(round(_timed(theirs, args.reps), 4))
            t = _median(ms["hip"]) * 1e-3
            sample = pairs[:: max(1, P // 500)].contiguous()
            diffs = (abx.dtw_distance(x, sample) - torch_dtw(x, sample, lo, hi, batch)).abs().cpu().numpy()
            diff, worst = float(diffs.max()), 0.0
            for (af, la, bf, lb), got in zip(sample.cpu().tolist(), diffs):          # each route within the test's bound of float64
                a, b = x[af:af + la].double().cpu().numpy(), x[bf:bf + lb].double().cpu().numpy()
                worst = max(worst, float(got) / (2.0 * abx_reference.dtw_tolerance(a, b, 0)))
            line = {"workload": name, "P": P, "lengths": [lo, hi], "N": N, "D": D, "dtype": str(dt).replace("torch.", ""),
                    "reps": args.reps, "ms": ms, "hip_median": _median(ms["hip"]), "torch_median": _median(ms["torch"]),
                    "speedup": round(_median(ms["torch"]) / _median(ms["hip"]), 3), "dist_tflops": round(flops / t / 1e12, 3),
                    "peak_fraction": round(flops / t / F32_MFMA_PEAK, 5), "pairs_per_s": round(P / t), "sample_pairs": int(sample.shape[0]),
                    "dist_max_abs_diff": diff, "diff_over_bound": round(worst, 4)}
            print(json.dumps(line), flush=True)
            assert worst <= 1.0, f"the two routes differ by {worst} of the bound on the sample"
            del x


if __name__ == "__main__":
    main()
