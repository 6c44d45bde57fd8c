"""The fused score-LSE loss chain (score_over_all_timesteps=True in bf16) entry point by entry point: cpc_score_lse (csrc/gemm.hip,
gemm_nt_persist_kernel<true>), cpc_nce_lse_merge, cpc_nce_fused_grad and cpc_nce_fused_finalize (csrc/nce.hip), each launch against the
plain float64 reference of the same call at the level of its arguments (tests/fused_score_reference.py;
test_fused_score_reference_host.py checks those references against torch.logsumexp, oracle.info_nce_loss and autograd and shows that the
measures used here reject deliberate mistakes).  The older tests (test_hip_kernels.py, test_audio_kernels_gpu.py) keep the whole-tensor
measure, which cannot see 96.7 % to 99.0 % of the gradient's elements.

Conventions (those of test_gemm_kernels_gpu.py).  Every output starts as NaN with sentinels behind it.  Every input element the call may
not read is NaN: the ldp - E / ldt - E padding of P / T, the pad columns [ncols, ld) of S for the gradient pass.  Written elements are
judged against the bound, or the stored bit pattern for the twins; everything else must still be NaN.

Bounds (u = 2^-24; derived in fused_score_reference.py's docstring, none chosen from a device result).
    S        2 (E + 2) u sum |p||t|          (conv1d_reference.bound, u_out = 0, n = E)
    pm       bitwise max of the stored f32 S over the tile's rows;  valid: bitwise S[r][r + diag_off];  colp[.][1], sums[3]: exact
    ps       u (18 + 2.5 spread_tile) ref    against float64 on the stored scores; __expf = exp2(x log2 e) on V_EXP_F32 (1 ulp, CDNA ISA guide)
    lse      u (a + 2.5 spread_c) + u |ref|,  a = 22 + nparts + 2 ln(2 max(nrows, 256 nparts)) + [softplus] (3 + ln nrows)
    dS       2^-8 |ref| + u |score'| ((11 + 2.5 |sp - lse| + [softplus] 4 |sp|) w / n_rows + (K + 19) |reg_c| mean_k |sp| + 7 [diag] / n_rows) + 2^-120
    gradp    (1024 + 2 (K + 7) + 2) u sum m_abs^2;   colp[.][0]: 258 u sum |lse|;   finalize: (n + 2) u sum |terms| through its few roundings
The float32 host emulation alone (test_fused_score_reference_host.py, without the storage term) reaches at most
    S 0.032   ps 0.13   lse 0.17 (merge on synthetic pairs: 0.67)   colp 0.007   dS 0.50 (narrow) / 0.40 (wide)   gradp 0.003
of them; the twins are exact there.

Cases.
    cpc_score_lse       fused_score_reference.score_cases (256 x 256 E 128; 768 x 512 E 192 with ldp 200, ldt 264, lds 516; column strips
                        768 x 256 at diag_off -256 / -512; row strip 256 x 768 at +256 with valid = NULL; diag_off 100 / -300 on 512 x 512: the
                        diagonal crosses tile corners and the rows without a column keep their NaN; diag_off = N / -M: valid untouched) and
                        walk_cases (256 x 8448 at E 128 / 192 / 256: one workgroup walks two tiles, nk = 2 / 3 / 4; 2048 x 8448: eight do; 2304 x
                        4352 E 192: the M tiles spill into a second panel group; 256 x 16640 E 192: more than 512 blocks, the start stagger, two
                        or three tiles), each with the narrow, wide, exact and count recipes.  Multi-tile: S on all rows of every tile that is
                        some workgroup's second or third and of its neighbours and on 64 seeded rows elsewhere; pm, ps, valid everywhere.
                        S = NULL gives the same bits in pm, ps, valid.  A +inf score gives ps = lse = NaN (include/cpc_hip.h).
    cpc_nce_lse_merge   on the pairs of those runs (both score kinds, nrows_total = M and 2 M); synthetic pairs nparts {1, 2, 3, 9} x ncols
                        {4, 255, 256, 257, 520}, narrow / wide, nrows_total = 256 nparts and 4096; columns behind ncols and colp's sentinels intact.
    cpc_nce_fused_grad  fused_score_reference.grad_cases: K {2, 8, 12, 16, 22, 24} x items {1, 15, 16, 17, 33}, ncols {4, 60, 64, 68, 260},
                        ld / ldT larger than needed (and tight), diag_off inside and outside the strip; narrow / wide under the bound, the
                        grad-exact twin bit for bit, dS^T included; dST = NULL and gradp = NULL bitwise equal in dS.
    cpc_nce_fused_finalize   modes 0 / 1 / 2, counts 1, 255, 257, 1000, valid at an offset, out[7] and sums[4..] untouched, the NaN route.
    the chain           256 x 256 and a 2-strip split of 512 x 512 against float64 autograd of oracle.info_nce_loss.
    refusals            every condition of the launchers returns -22 and writes nothing.
"""
import ctypes as C
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import cpc_oracle as O  # noqa: E402

from cpc_audio_amd import _hip  # noqa: E402
import fused_score_reference as R  # noqa: E402
from fused_score_reference import BF16, F32, F64, U24  # noqa: E402
from test_attention_long_gpu import guard_intact, guarded  # noqa: E402

DEV = "cuda:0"
EINVAL = -22
L_, F_ = C.c_longlong, C.c_float
SCORE_CASES, WALK_CASES, GRAD_CASES = R.score_cases(), [(c, a) for c, a, _ in R.walk_cases()], R.grad_cases()


def dev(t64, dt):
    return t64.to(dt).to(DEV)


def bits_equal(a, b):
    """Same stored bit patterns, NaN included."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ======================================================================================================================= cpc_score_lse
def run_score(a, P, T, store=None, valid=None):
    """One launch on fresh NaN buffers -> S [M][lds] or None, pm, ps [M / 256][N], valid [M] or None (device); sentinels asserted."""
    M, N, E = a["M"], a["N"], a["E"]
    store = a["store"] if store is None else store
    valid = a["valid"] if valid is None else valid
    dP, dT = dev(P, BF16), dev(T, BF16)
    sb, S = guarded(M * a["lds"], F32) if store else (None, None)
    pb, pm = guarded(M // 256 * N, F32)
    qb, ps = guarded(M // 256 * N, F32)
    vb, v = guarded(M, F32) if valid else (None, None)
    _hip.call("cpc_score_lse", _hip.ptr(dP), _hip.ptr(dT), _hip.ptr(S), _hip.ptr(pm), _hip.ptr(ps), _hip.ptr(v), M, N, E, L_(a["ldp"]), L_(a["ldt"]),
              L_(a["lds"]), a["diag_off"])
    torch.cuda.synchronize()
    assert guard_intact(pb, pm.numel()) and guard_intact(qb, ps.numel()), "sentinels behind pm / ps"
    assert not store or guard_intact(sb, S.numel()), "sentinels behind S"
    assert not valid or guard_intact(vb, M), "sentinels behind valid"
    return (S.view(M, a["lds"]) if store else None), pm.view(M // 256, N), ps.view(M // 256, N), v


@functools.lru_cache(maxsize=4)
def score_ref(cid, recipe):
    a = dict(SCORE_CASES + WALK_CASES)[cid]
    P, T = R.score_data(recipe, a["M"], a["N"], a["E"], a["ldp"], a["ldt"], a["diag_off"])
    return P, T, R.score_lse_ref(P, T, a["M"], a["N"], a["E"], a["ldp"], a["ldt"], a["diag_off"])


def judge_score(cid, a, recipe, S, pm, ps, valid, ref, rows=None):
    """S (all rows, or the {tile: rows} given), pm, ps, valid of one launch.  Prints the ratios."""
    M, N, E = a["M"], a["N"], a["E"]
    exact = recipe in ("exact", "count")
    got = S.cpu().double()
    assert bool(torch.isnan(got[:, N:]).all()), "pad columns of S written"
    got = got[:, :N]
    assert bool(torch.isfinite(got).all())
    if exact:
        assert float(ref.Sabs.max()) <= R.EXACT_MAX
    if rows is None:
        qS = 0.0 if (exact and R.same_bits(got, ref.S)) else (float("inf") if exact else R.s_ratio(got, ref, E))
    else:
        sel = torch.zeros(M, N, dtype=torch.bool)
        for (mt, nt), rr in rows.items():
            sel[rr, nt * 256:(nt + 1) * 256] = True
        b = R.bound(ref.S[sel], ref.Sabs[sel], E, 0.0)
        err = (got[sel] - ref.S[sel]).abs()
        qS = (0.0 if bool((err == 0).all()) else float("inf")) if exact else float((err / b.clamp_min(1e-300)).max())
    assert R.same_bits(pm, R.tile_pairs(got)[0]), f"{cid} {recipe}: pm is not the maximum of the stored scores, per tile and column"
    if recipe == "count":
        assert R.same_bits(ps, ref.ps), f"{cid}: ps does not count the rows at the maximum"
        qps = 0.0
    else:
        qps = R.ps_ratio(ps, got)
    if valid is not None:
        want, written = R.valid_of(got, a["diag_off"])
        v = valid.cpu().double()
        assert bool(torch.isnan(v[~written]).all()), f"{cid}: valid written where no column r + diag_off exists"
        assert R.same_bits(v[written], want[written]), f"{cid} {recipe}: valid is not S[r][r + diag_off]"
        assert torch.equal(written, ref.valid_written)
    print(f"ratio [score_lse] {cid} {recipe}: S {qS:.4f} ps {qps:.4f}")
    assert qS <= 1.0 and qps <= 1.0, (cid, recipe, qS, qps)
    return got


def run_merge(pm, ps, nparts, ncols, softplus, nrows_total):
    lb, lse = guarded(ncols, F32)
    nb = (ncols + 255) // 256
    cb, colp = guarded(2 * nb, F32)
    _hip.call("cpc_nce_lse_merge", _hip.ptr(pm), _hip.ptr(ps), nparts, ncols, softplus, F_(nrows_total), _hip.ptr(lse), _hip.ptr(colp))
    torch.cuda.synchronize()
    assert guard_intact(lb, ncols) and guard_intact(cb, 2 * nb), "sentinels behind lse / colp"
    return lse, colp.view(nb, 2)


def judge_merge_of_run(cid, a, recipe, got, pm, ps):
    M, N = a["M"], a["N"]
    for softplus in (0, 1):
        for nrows in (float(M), float(2 * M)):
            lse, colp = run_merge(pm, ps, M // 256, N, softplus, nrows)
            q = R.lse_ratio_from_scores(lse, got, softplus, nrows)
            qc = R.colp_ratio(colp, lse, pm, M // 256, N)
            print(f"ratio [lse_merge] {cid} {recipe} softplus {softplus} nrows {nrows:.0f}: lse {q:.4f} colp {qc:.4f}")
            assert q <= 1.0 and qc <= 1.0, (cid, recipe, softplus, nrows, q, qc)


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("cid", [c for c, _ in SCORE_CASES])
def test_score_lse(cid, recipe):
    """The whole S, pm, ps, valid of every small case and recipe; S = NULL gives the same bits; the merge on these pairs."""
    a = dict(SCORE_CASES)[cid]
    P, T, ref = score_ref(cid, recipe)
    S, pm, ps, valid = run_score(a, P, T)
    got = judge_score(cid, a, recipe, S, pm, ps, valid, ref)
    _, pm2, ps2, valid2 = run_score(a, P, T, store=False)
    assert bits_equal(pm2, pm) and bits_equal(ps2, ps) and (valid is None or bits_equal(valid2, valid)), "S = NULL changes pm / ps / valid"
    judge_merge_of_run(cid, a, recipe, got, pm, ps)


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("cid", [c for c, _ in WALK_CASES])
def test_score_lse_multi_tile_walk(cid, recipe):
    """More than one tile per workgroup: the hand-over between tiles at nk = 2, 3 and 4 K stages (see the host mirror in
    test_fused_score_reference_host.py for what each shape is there for)."""
    a = dict(WALK_CASES)[cid]
    P, T, ref = score_ref(cid, recipe)
    S, pm, ps, valid = run_score(a, P, T)
    got = judge_score(cid, a, recipe, S, pm, ps, valid, ref, rows=R.walk_rows(a))
    if recipe == "narrow":
        _, pm2, ps2, valid2 = run_score(a, P, T, store=False)
        assert bits_equal(pm2, pm) and bits_equal(ps2, ps) and bits_equal(valid2, valid), "S = NULL changes pm / ps / valid"
        lse, colp = run_merge(pm, ps, a["M"] // 256, a["N"], 1, float(a["M"]))
        q, qc = R.lse_ratio_from_scores(lse, got, 1, float(a["M"])), R.colp_ratio(colp, lse, pm, a["M"] // 256, a["N"])
        print(f"ratio [lse_merge] {cid}: lse {q:.4f} colp {qc:.4f}")
        assert q <= 1.0 and qc <= 1.0


def test_score_lse_infinite_scores():
    """include/cpc_hip.h: a +inf score (here 2^100 * 2^100, which overflows the f32 accumulator) gives ps = lse = NaN for its tile and
    column (exp(inf - inf)), not lse = +inf as the dense kernels promise; a -inf score beside finite ones counts as exp(-inf) = 0.
    Every other pair is finite.  (A NaN score: test_nan_route_through_the_chain.)"""
    a = R.SC(512, 256, 128)
    P, T = R.score_data("narrow", 512, 256, 128, 128, 128, 0)
    for val in (float("inf"), float("-inf")):
        P2, T2 = P.clone().reshape(512, 128), T.clone().reshape(256, 128)
        P2[:, 5], T2[:, 5], T2[7, :], P2[300, :] = 0.0, 0.0, 0.0, 0.0           # column 7 and row 300 are zero but for their crossing
        P2[300, 5], T2[7, 5] = 2.0 ** 100, math.copysign(2.0 ** 100, val)
        S, pm, ps, _ = run_score(a, P2.reshape(-1), T2.reshape(-1))
        S, pm, ps = S.cpu(), pm.cpu(), ps.cpu()
        assert float(S[300, 7]) == val and float(S[299, 7]) == 0.0 and float(S[300, 8]) == 0.0
        other = torch.ones(2, 256, dtype=torch.bool)
        other[1, 7] = False
        assert bool(torch.isfinite(ps[other]).all()) and bool(torch.isfinite(pm[other]).all())
        lse, _ = run_merge(pm.to(DEV), ps.to(DEV), 2, 256, 0, 512.0)
        lse = lse.cpu()
        assert bool(torch.isfinite(lse[torch.arange(256) != 7]).all())
        if val < 0:
            assert float(pm[1, 7]) == 0.0 and float(ps[1, 7]) == 255.0 and math.isfinite(float(lse[7]))
        else:
            assert float(pm[1, 7]) == val and math.isnan(float(ps[1, 7])) and math.isnan(float(lse[7]))


# ======================================================================================================================= cpc_nce_lse_merge
@pytest.mark.parametrize("nparts", R.MERGE_NPARTS)
def test_lse_merge_synthetic_pairs(nparts):
    for ncols in R.MERGE_NCOLS:
        for wide in (False, True):
            pm, ps = R.merge_data(nparts, ncols, wide)
            dpm, dps = dev(pm, F32), dev(ps, F32)
            for softplus in (0, 1):
                for nrows in (256.0 * nparts, 4096.0):
                    lse, colp = run_merge(dpm, dps, nparts, ncols, softplus, nrows)
                    q = R.lse_ratio_from_pairs(lse, pm, ps, nparts, ncols, softplus, nrows)
                    qc = R.colp_ratio(colp, lse, pm, nparts, ncols)
                    print(f"ratio [lse_merge] nparts {nparts} ncols {ncols} {'wide' if wide else 'narrow'} softplus {softplus} nrows {nrows:.0f}: {q:.4f} {qc:.4f}")
                    assert q <= 1.0 and qc <= 1.0, (nparts, ncols, wide, softplus, nrows, q, qc)
            if wide:                                     # columns wholly below -30: the softplus reference point is 0 and lse ~ log nrows_total
                low = pm.reshape(nparts, ncols).max(0).values < -30
                lse, _ = run_merge(dpm, dps, nparts, ncols, 1, 4096.0)
                assert int(low.sum()) > 0 and float((lse.cpu().double()[low] - math.log(4096.0)).abs().max()) < 1e-6


# ======================================================================================================================= cpc_nce_fused_grad
def run_grad(b, S, lse, softplus, want_T=True, want_gradp=True):
    items, K, ncols, ld, ldT = b["items"], b["K"], b["ncols"], b["ld"], b["ldT"]
    n = items * K
    dS_in, dlse = dev(S, F32), dev(lse, F32)
    db, dS = guarded(n * ld, BF16)
    tb, dST = guarded(ncols * ldT, BF16) if want_T else (None, None)
    nb = int(_hip.lib().cpc_nce_fused_grad_blocks(items, ncols))
    assert nb == ((ncols + 63) // 64) * ((items + 15) // 16)
    gb, gradp = guarded(nb, F32) if want_gradp else (None, None)
    _hip.call("cpc_nce_fused_grad", _hip.ptr(dS_in), _hip.ptr(dlse), _hip.ptr(dS), _hip.ptr(dST), _hip.ptr(gradp), items, K, ncols, L_(ld), L_(ldT),
              b["diag_off"], softplus, F_(b["reg"]), F_(b["n_rows_total"]), F_(b["n_items_total"]))
    torch.cuda.synchronize()
    assert guard_intact(db, n * ld) and (not want_T or guard_intact(tb, ncols * ldT)) and (not want_gradp or guard_intact(gb, nb)), "sentinels"
    return dS, dST, gradp


@pytest.mark.parametrize("cid", [c for c, _ in GRAD_CASES])
def test_fused_grad(cid):
    """dS, dS^T and gradp of every case: narrow and wide data under the per-element bound with both score kinds, the grad-exact twin bit
    for bit; the pad columns of dS and dS^T unwritten; dST = NULL and gradp = NULL give the same bits in dS."""
    a = dict(GRAD_CASES)[cid]
    for recipe, softplus in (("narrow", 0), ("narrow", 1), ("wide", 0), ("wide", 1), ("grad-exact", 0)):
        exact = recipe == "grad-exact"
        S, lse, b = R.grad_data(a, recipe, softplus)
        ref = R.fused_grad_ref(S, lse, b["items"], b["K"], b["ncols"], b["ld"], b["ldT"], b["diag_off"], softplus, b["reg"], b["n_rows_total"],
                               b["n_items_total"])
        dS, dST, gradp = run_grad(b, S, lse, softplus)
        q = R.grad_judge(dS, ref.dS, ref.bound_S, ref.written_S, exact)
        qT = R.grad_judge(dST, ref.dST, ref.bound_T, ref.written_T, exact)
        qg = float(((gradp.cpu().double() - ref.gradp).abs() / ref.bound_gradp.clamp_min(1e-300)).max())
        print(f"ratio [fused_grad] {cid} {recipe} softplus {softplus}: dS {q:.4f} dST {qT:.4f} gradp {qg:.4f}")
        assert q <= 1.0 and qT <= 1.0 and qg <= 1.0, (cid, recipe, softplus, q, qT, qg)
        if recipe == "narrow":
            dS2, _, _ = run_grad(b, S, lse, softplus, want_T=False)
            dS3, _, _ = run_grad(b, S, lse, softplus, want_gradp=False)
            assert bits_equal(dS2, dS) and bits_equal(dS3, dS), "dST = NULL / gradp = NULL changes dS"


# ======================================================================================================================= cpc_nce_fused_finalize
def run_finalize(colp, ncolp, valid, voff, nvalid, gradp, ngrad, sums, mode, n_rows, n_items, K, reg, softplus, out):
    _hip.call("cpc_nce_fused_finalize", _hip.ptr(colp), ncolp, _hip.ptr(valid, voff) if valid is not None else None, nvalid, _hip.ptr(gradp), ngrad,
              _hip.ptr(sums), mode, F_(n_rows), F_(n_items), K, F_(reg), softplus, _hip.ptr(out))
    torch.cuda.synchronize()


@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("count", [1, 255, 257, 1000])
def test_fused_finalize(count, softplus):
    g = R.gen(count + softplus)
    colp = R.rounded(torch.stack([R.normal(g, count).double() * 50 + 700, R.normal(g, count).double() * 30], 1), F32)
    voff = 3
    valid = R.rounded(torch.cat([torch.full((voff,), R.NAN, dtype=F64), R.normal(g, count).double() * 10, torch.full((2,), R.NAN, dtype=F64)]), F32)
    gradp = R.rounded(R.normal(g, count).double().abs() * 5, F32)
    n_rows, n_items, K, reg = 1536.0, 96.0, 16, 0.3
    dc, dv, dg = dev(colp.reshape(-1), F32), dev(valid, F32), dev(gradp, F32)
    nan8 = torch.full((8,), R.NAN, dtype=F64)
    ref = R.fused_finalize_ref(colp, valid[voff:voff + count], gradp, None, 0, n_rows, n_items, K, reg, softplus, nan8)
    ob, out = guarded(8, F32)
    out[6] = 0.0
    run_finalize(dc, count, dv, voff, count, dg, count, None, 0, n_rows, n_items, K, reg, softplus, out)
    o = out.cpu().double()
    assert guard_intact(ob, 8) and math.isnan(float(o[7])) and float(o[5]) == 0.0 and float(o[6]) == 0.0
    for i in range(5):
        q = abs(float(o[i] - ref.out[i])) / max(float(ref.err[i]), 1e-300) if float(ref.err[i]) > 0 else (0.0 if float(o[i]) == float(ref.out[i]) else float("inf"))
        print(f"ratio [finalize] count {count} softplus {softplus} out[{i}]: {q:.4f}")
        assert q <= 1.0, (i, float(o[i]), float(ref.out[i]), float(ref.err[i]))
    # mode 1: sums[0..3] only; mode 2 from them is bitwise mode 0
    sb, sums = guarded(6, F32)
    run_finalize(dc, count, dv, voff, count, dg, count, sums, 1, n_rows, n_items, K, reg, softplus, None)
    s = sums.cpu().double()
    r1 = R.fused_finalize_ref(colp, valid[voff:voff + count], gradp, None, 1, n_rows, n_items, K, reg, softplus, nan8, torch.zeros(4, dtype=F64))
    assert guard_intact(sb, 6) and bool(torch.isnan(s[4:]).all()) and float(s[3]) == float(r1.sums[3])
    for i in range(3):
        assert abs(float(s[i] - r1.sums[i])) <= float(r1.err_sums[i]), (i, float(s[i]), float(r1.sums[i]))
    ob2, out2 = guarded(8, F32)
    out2[6] = 0.0
    run_finalize(None, 0, None, 0, 0, None, 0, sums, 2, n_rows, n_items, K, reg, softplus, out2)
    assert bits_equal(out2[:6], out[:6]) and math.isnan(float(out2[7])) and guard_intact(ob2, 8)
    assert bits_equal(sums[:4], dev(s[:4], F32))         # (mode 2 leaves sums alone)


def test_nan_route_through_the_chain():
    """One NaN element in P: ps, lse and valid are NaN exactly where the reference says (row 300's scores: its tile's pair of every
    column, valid[300]) and nowhere else; out[0] is NaN, out[5] = out[6] = 1; a following clean call leaves out[5] = 0, out[6] = 1."""
    a = R.SC(512, 512, 128)
    P, T = R.score_data("narrow", 512, 512, 128, 128, 128, 0)
    P = P.clone()
    P[300 * 128 + 17] = R.NAN
    S, pm, ps, valid = run_score(a, P, T)
    assert bool(torch.isnan(S[300, :512]).all()) and int(torch.isnan(S).sum()) == 512
    assert bool(torch.isfinite(pm).all()), "fmaxf drops the NaN: the maxima stay finite"
    assert bool(torch.isnan(ps[1]).all()) and bool(torch.isfinite(ps[0]).all())
    v = valid.cpu()
    assert math.isnan(float(v[300])) and int(torch.isnan(v).sum()) == 1
    lse, colp = run_merge(pm, ps, 2, 512, 1, 512.0)
    assert bool(torch.isnan(lse).all()) and bool(torch.isnan(colp[:, 0]).all()) and bool(torch.isfinite(colp[:, 1]).all())
    gradp = torch.ones(4, device=DEV)
    out = torch.full((8,), R.NAN, device=DEV)
    out[6] = 0.0
    run_finalize(colp, 2, valid, 0, 512, gradp, 4, None, 0, 512.0, 64.0, 8, 0.5, 1, out)
    assert math.isnan(float(out[0])) and float(out[5]) == 1.0 and float(out[6]) == 1.0
    P2, _ = R.score_data("narrow", 512, 512, 128, 128, 128, 0)
    _, pm, ps, valid = run_score(a, P2, T)
    lse, colp = run_merge(pm, ps, 2, 512, 1, 512.0)
    run_finalize(colp, 2, valid, 0, 512, gradp, 4, None, 0, 512.0, 64.0, 8, 0.5, 1, out)
    assert math.isfinite(float(out[0])) and float(out[5]) == 0.0 and float(out[6]) == 1.0, "out[6] is sticky"


# ======================================================================================================================= the chain
def device_chain(Pm, Tm, K, diag_off, softplus, reg, n_rows, n_items, lse_in=None):
    (M, E), N = Pm.shape, Tm.shape[0]
    a = R.SC(M, N, E, diag_off=diag_off)
    S, pm, ps, valid = run_score(a, Pm.reshape(-1), Tm.reshape(-1))
    lse, colp = run_merge(pm, ps, M // 256, N, softplus, float(n_rows))
    b = R.GC(M // K, K, N, ld=N, ldT=M, diag_off=diag_off, reg=reg, n_rows_total=float(n_rows), n_items_total=float(n_items))
    dS, dST, gradp = run_grad(b, S.cpu().double().reshape(-1), (lse if lse_in is None else lse_in).cpu().double(), softplus)
    return dict(S=S, valid=valid, lse=lse, colp=colp, dS=dS.view(M, N), dST=dST.view(N, M), gradp=gradp)


def chain_bounds(Pm, Tm, items, K, softplus, reg):
    """float64 autograd of oracle.info_nce_loss and, per element, how far the device may be from it: the bounds of the four kernels plus
    what the GEMM's rounding of a score (eS) and the lse's error (eL) do to a later stage, through that stage's derivative."""
    n, E = Pm.shape
    lin = (Pm @ Tm.T).requires_grad_(True)
    sc = lin.view(items, K, items, K)
    sc = F.softplus(sc) if softplus else sc
    loss, smax = O.info_nce_loss(sc, all_timesteps=True, regularization=reg)
    loss.backward()
    s = lin.detach()
    eS = R.bound(s, Pm.abs() @ Tm.abs().T, E, 0.0)
    sp, g = R.score_tf(s, softplus), R.score_grad(s, softplus)
    lse = torch.logsumexp(sp, 0)
    eL = R.lse_bound(lse, s.max(0).values - s.min(0).values, n // 256, softplus, float(n)) + eS.max(0).values
    fg = R.fused_grad_ref(s.reshape(-1), lse, items, K, n, n, n, 0, softplus, reg, float(n), float(items))
    w = torch.exp(sp - lse[None, :])
    reg_c = 2.0 * reg / (items * items * K * K)
    meS = eS.reshape(items, K, n).mean(1).repeat_interleave(K, 0)
    dsp = lin.grad / g
    sens = g * (w / n) * (eS + eL[None, :]) + g * reg_c * meS + (0.25 if softplus else 0.0) * dsp.abs() * eS
    bnd = R.U8 * lin.grad.abs() + fg.bound_S.reshape(n, n) + sens
    m = sp.reshape(items, K, n).mean(1)
    terms = dict(valid=-torch.diagonal(sp).sum() / n, lse=lse.sum() / n, reg=reg * (m * m).sum() / (items * n))
    e_terms = dict(valid=(torch.diagonal(eS).sum() + (n + 6) * U24 * torch.diagonal(sp).abs().sum()) / n + 2 * U24 * abs(float(terms["valid"])),
                   lse=(eL.sum() + (258 + n // 256 + 2) * U24 * lse.abs().sum()) / n + 2 * U24 * abs(float(terms["lse"])),
                   reg=reg * ((2 * m.abs() * eS.reshape(items, K, n).mean(1)).sum() + float(fg.bound_gradp.sum()) +
                              (fg.gradp.numel() + 2) * U24 * (m * m).sum()) / (items * n) + 4 * U24 * abs(float(terms["reg"])))
    return dict(loss=loss.detach(), smax=smax.detach(), grad=lin.grad, bound=bnd, terms=terms, e_terms=e_terms, lse=lse, eL=eL)


@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("n,W", [(256, 1), (512, 2)])
def test_chain_against_autograd(n, W, softplus):
    """The four entry points in a row at B K = 256 (the smallest shape the engine's fused route accepts) and as the two strips of each of
    two ranks at 512, against float64 autograd of oracle.info_nce_loss: out[2], out[3], out[4] each alone, the gradient per element."""
    K, E, reg = 8, 128, 0.7
    items, nl = n // K, n // W
    g = R.gen(40 + n)
    Pm, Tm = R.rounded(R.normal(g, n, E).double() * (2.0 / math.sqrt(E)), BF16), R.rounded(R.normal(g, n, E).double() * 2.0, BF16)
    want = chain_bounds(Pm, Tm, items, K, softplus, reg)
    tot = torch.zeros(4, device=DEV)
    lse_all = torch.cat([device_chain(Pm, Tm[r * nl:(r + 1) * nl], K, -r * nl, softplus, reg, n, items)["lse"] for r in range(W)]) if W > 1 else None
    for rank in range(W):
        lo = rank * nl
        col = device_chain(Pm, Tm[lo:lo + nl], K, -lo, softplus, reg, n, items)
        q = float(((col["dS"].cpu().double() - want["grad"][:, lo:lo + nl]).abs() / want["bound"][:, lo:lo + nl]).max())
        qT = float(((col["dST"].cpu().double() - want["grad"][:, lo:lo + nl].T).abs() / want["bound"][:, lo:lo + nl].T).max())
        ql = float(((col["lse"].cpu().double() - want["lse"][lo:lo + nl]).abs() / want["eL"][lo:lo + nl]).max())
        print(f"ratio [chain] n {n} rank {rank} softplus {softplus}: dS {q:.4f} dST {qT:.4f} lse {ql:.4f}")
        assert q <= 1.0 and qT <= 1.0 and ql <= 1.0
        if W > 1:
            row = device_chain(Pm[lo:lo + nl], Tm, K, lo, softplus, reg, n, items, lse_in=lse_all)
            q = float(((row["dS"].cpu().double() - want["grad"][lo:lo + nl]).abs() / want["bound"][lo:lo + nl]).max())
            print(f"ratio [chain] n {n} rank {rank} row strip: dS {q:.4f}")
            assert q <= 1.0
            assert bits_equal(row["valid"], col["valid"][lo:lo + nl])
        sums = torch.zeros(4, device=DEV)
        run_finalize(col["colp"].reshape(-1), col["colp"].shape[0], col["valid"], lo, nl, col["gradp"], col["gradp"].numel(), sums, 1, float(n), float(items), K,
                     reg, softplus, None)
        tot[:3] += sums[:3]
        tot[3] = sums[3] if rank == 0 else torch.maximum(tot[3], sums[3])
    out = torch.full((8,), R.NAN, device=DEV)
    out[6] = 0.0
    run_finalize(None, 0, None, 0, 0, None, 0, tot, 2, float(n), float(items), K, reg, softplus, out)
    o = out.cpu().double()
    for i, key in ((2, "valid"), (3, "lse"), (4, "reg")):
        q = abs(float(o[i] - want["terms"][key])) / (float(want["e_terms"][key]) + W * 2 * U24 * abs(float(want["terms"][key])))
        print(f"ratio [chain] n {n} softplus {softplus} out[{i}] ({key}): {q:.4f}")
        assert q <= 1.0, (key, float(o[i]), float(want["terms"][key]))
    e0 = sum(float(v) for v in want["e_terms"].values()) + 4 * U24 * sum(abs(float(v)) for v in want["terms"].values()) * (1 + W)
    assert abs(float(o[0] - want["loss"])) <= e0 and float(o[5]) == 0.0 and float(o[6]) == 0.0
    eS_max = float(R.bound(Pm @ Tm.T, Pm.abs() @ Tm.abs().T, E, 0.0).max())
    assert abs(float(o[1] - want["smax"])) <= eS_max + 4 * U24 * abs(float(want["smax"]))


# ======================================================================================================================= refusals
def test_refusals_write_nothing():
    """Every condition launch_score_lse, launch_nce_lse_merge, launch_nce_fused_grad and launch_nce_fused_finalize test: -22, and every
    output still NaN.  Negative counts of finalize are refused since this work (they read as empty arrays before)."""
    lib, st = _hip.lib(), _hip.stream_ptr()
    bf = torch.ones(1 << 17, device=DEV, dtype=BF16)
    f32 = torch.ones(1 << 17, device=DEV)
    outs = [guarded(1 << 17, F32) for _ in range(4)] + [guarded(1 << 17, BF16) for _ in range(2)]
    (Sb, S), (pb, pm), (qb, ps), (vb, valid), (db, dS), (tb, dST) = outs
    n_checked = 0

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(v.float()).all()) and guard_intact(b, 1 << 17) for b, v in outs)

    def p(t, off=0):
        return None if t is None else C.c_void_p(t.data_ptr() + off)

    ok = dict(P=bf, T=bf, S=S, pm=pm, ps=ps, valid=valid, M=256, N=256, E=128, ldp=128, ldt=128, lds=256, offP=0, offT=0, offS=0)
    for bad in (dict(P=None), dict(T=None), dict(pm=None), dict(ps=None), dict(M=0), dict(N=0), dict(M=300), dict(N=264), dict(E=64), dict(E=0),
                dict(E=160), dict(ldp=132), dict(ldt=132), dict(ldp=120), dict(ldt=120), dict(offP=8), dict(offT=8), dict(lds=258), dict(lds=252),
                dict(offS=8)):
        a = dict(ok, **bad)
        rc = lib.cpc_score_lse(p(a["P"], a["offP"]), p(a["T"], a["offT"]), p(a["S"], a["offS"]), p(a["pm"]), p(a["ps"]), p(a["valid"]), a["M"], a["N"], a["E"],
                               a["ldp"], a["ldt"], a["lds"], 0, st)
        assert rc == EINVAL and untouched(), ("cpc_score_lse", bad, rc)
        n_checked += 1
    ok = dict(pm=f32, ps=f32, nparts=2, ncols=256, lse=S, colp=pm)
    for bad in (dict(pm=None), dict(ps=None), dict(lse=None), dict(colp=None), dict(nparts=0), dict(ncols=0), dict(ncols=-4)):
        a = dict(ok, **bad)
        rc = lib.cpc_nce_lse_merge(p(a["pm"]), p(a["ps"]), a["nparts"], a["ncols"], 1, 512.0, p(a["lse"]), p(a["colp"]), st)
        assert rc == EINVAL and untouched(), ("cpc_nce_lse_merge", bad, rc)
        n_checked += 1
    ok = dict(S=f32, lse=f32, dS=dS, dST=dST, gradp=ps, items=16, K=8, ncols=64, ld=64, ldT=128, offS=0, offL=0, offD=0, offT=0)
    for bad in (dict(S=None), dict(lse=None), dict(dS=None), dict(items=0), dict(K=0), dict(K=7), dict(K=26), dict(K=1), dict(ncols=0), dict(ncols=62),
                dict(ld=68), dict(ld=56), dict(ldT=132), dict(ldT=120), dict(offS=8), dict(offL=8), dict(offD=8), dict(offT=8)):
        a = dict(ok, **bad)
        rc = lib.cpc_nce_fused_grad(p(a["S"], a["offS"]), p(a["lse"], a["offL"]), p(a["dS"], a["offD"]), p(a["dST"], a["offT"]), p(a["gradp"]), a["items"],
                                    a["K"], a["ncols"], a["ld"], a["ldT"], 0, 0, 0.5, 128.0, 16.0, st)
        assert rc == EINVAL and untouched(), ("cpc_nce_fused_grad", bad, rc)
        n_checked += 1
    ok = dict(colp=f32, ncolp=4, valid=f32, nvalid=4, gradp=f32, ngrad=4, sums=pm, mode=0, out=ps)
    for bad in (dict(mode=3), dict(mode=-1), dict(colp=None), dict(valid=None), dict(gradp=None), dict(out=None), dict(mode=1, sums=None),
                dict(mode=2, sums=None), dict(mode=2, out=None), dict(ncolp=-1), dict(nvalid=-1), dict(ngrad=-1), dict(mode=1, ncolp=-1)):
        a = dict(ok, **bad)
        rc = lib.cpc_nce_fused_finalize(p(a["colp"]), a["ncolp"], p(a["valid"]), a["nvalid"], p(a["gradp"]), a["ngrad"], p(a["sums"]), a["mode"], 512.0, 64.0, 8,
                                        0.5, 0, p(a["out"]), st)
        assert rc == EINVAL and untouched(), ("cpc_nce_fused_finalize", bad, rc)
        n_checked += 1
    assert n_checked == 58
