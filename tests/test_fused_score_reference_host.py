"""Host-only checks of tests/fused_score_reference.py, the references test_fused_score_kernels_gpu.py judges cpc_score_lse,
cpc_nce_lse_merge, cpc_nce_fused_grad and cpc_nce_fused_finalize by.  No GPU and no library is needed.

  * the references against independent formulations: lse_merge_ref o score_lse_ref against torch.logsumexp of the (softplus of the)
    scores; the whole chain against oracle.info_nce_loss and float64 autograd at the smallest shape fused_scores_ok accepts
    (B K = 256, E = 128, even K) and on a 2-rank strip decomposition (all predictions x own targets with diag_off = -lo, own
    predictions x all targets with diag_off = +lo): strips and whole agree and both equal autograd;
  * deliberate mistakes, each rejected by the bound on random data and by its exact twin (a failure names the check that was too weak);
  * the old whole-tensor measure rel_err < 1.5e-2 accepts a gradient whose every off-diagonal element is zero, on the old tests' own
    recipes; the share of the elements it cannot see is printed (measured: 96.7 % to 99.0 %, 98.1 % on average);
  * "reference alone": the float32 emulation of each formula against each bound without the storage term (the largest ratios are
    printed; test_fused_score_kernels_gpu.py's docstring records them);
  * the host mirror of the persistent tile walk asserts what each multi-tile GPU case is there for.
"""
import collections
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import cpc_oracle as O  # noqa: E402

import fused_score_reference as R  # noqa: E402
from fused_score_reference import BF16, F32, F64  # noqa: E402


RT = 1e-8         # (exp(softplus(s)) = 1 + exp(s) but beyond torch's threshold 20, where it is exp(s): e^-20 = 2e-9 relative)


def stored(t):
    """float64 -> what a correct kernel stores as f32."""
    return t.float().double()


def run_score(a, recipe, mut=None, dtype=F64):
    P, T = R.score_data(recipe, a["M"], a["N"], a["E"], a["ldp"], a["ldt"], a["diag_off"])
    return R.score_lse_ref(P.to(dtype), T.to(dtype), a["M"], a["N"], a["E"], a["ldp"], a["ldt"], a["diag_off"], mut)


@functools.lru_cache(maxsize=None)
def case_ref(cid, recipe):
    return run_score(dict(R.score_cases())[cid], recipe)


# ======================================================================================================== independent formulations
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("recipe", ["narrow", "wide"])
def test_lse_chain_against_logsumexp(recipe, softplus):
    a = dict(R.score_cases())["768x512-E192-ld"]
    r = case_ref("768x512-E192-ld", recipe)
    P, T = R.score_data(recipe, a["M"], a["N"], a["E"], a["ldp"], a["ldt"], 0)
    want = P.reshape(a["M"], a["ldp"])[:, :a["E"]] @ T.reshape(a["N"], a["ldt"])[:, :a["E"]].T
    torch.testing.assert_close(r.S, want, rtol=1e-13, atol=1e-13)
    m = R.lse_merge_ref(r.pm.reshape(-1), r.ps.reshape(-1), 3, a["N"], softplus, 768.0)
    ref = torch.logsumexp(F.softplus(r.S) if softplus else r.S, 0)          # (exp(softplus(s)) = 1 + exp(s) but for torch's threshold: < e^-20)
    torch.testing.assert_close(m.lse, ref, rtol=0, atol=1e-8)
    assert float(m.colp[1, 1]) == float(r.S[:, 256:].max()) and abs(float(m.colp[0, 0] - ref[:256].sum())) < 1e-6
    if recipe == "wide":           # the recipe holds what it promises: scores beyond +-90, own-target scores above 20, columns wholly below -30
        assert float(r.S.max()) > 90 and float(r.S.min()) < -90 and int((torch.diagonal(r.S) > 20).sum()) >= 3
        low = r.S.max(0).values < -30
        assert int(low.sum()) >= 3
        if softplus:
            assert float((m.lse[low] - math.log(768.0)).abs().max()) < 1e-9
    else:
        spread = r.S.max(0).values - r.S.min(0).values
        assert float(spread.max()) < 12.0


def chain(Pm, Tm, K, diag_off, softplus, reg, n_rows, n_items, lse_in=None):
    """The four references on P [M][E] / T [N][E]: -> score_lse_ref's result + lse, colp, the gradient pieces."""
    (M, E), N = Pm.shape, Tm.shape[0]
    r = R.score_lse_ref(Pm.reshape(-1), Tm.reshape(-1), M, N, E, E, E, diag_off)
    m = R.lse_merge_ref(r.pm.reshape(-1), r.ps.reshape(-1), M // 256, N, softplus, float(n_rows))
    g = R.fused_grad_ref(r.S.reshape(-1), m.lse if lse_in is None else lse_in, M // K, K, N, N, M, diag_off, softplus, reg, float(n_rows), float(n_items))
    r.lse, r.colp, r.g = m.lse, m.colp, g
    return r


def oracle(Pm, Tm, items, K, softplus, reg):
    lin = (Pm @ Tm.T).requires_grad_(True)
    sc = lin.view(items, K, items, K)
    sc = F.softplus(sc) if softplus else sc
    loss, smax = O.info_nce_loss(sc, all_timesteps=True, regularization=reg)
    loss.backward()
    return loss.detach(), smax.detach(), lin.grad


@pytest.mark.parametrize("softplus", [0, 1])
def test_chain_against_oracle_and_autograd(softplus):
    items, K, E, reg = 32, 8, 128, 0.7
    n = items * K
    g = R.gen(5)
    Pm, Tm = R.rounded(R.normal(g, n, E).double() * (2.0 / math.sqrt(E)), BF16), R.rounded(R.normal(g, n, E).double() * 2.0, BF16)
    loss, smax, grad = oracle(Pm, Tm, items, K, softplus, reg)
    r = chain(Pm, Tm, K, 0, softplus, reg, n, items)
    f = R.fused_finalize_ref(r.colp, r.valid, r.g.gradp, None, 0, float(n), float(items), K, reg, softplus, torch.zeros(8, dtype=F64))
    assert abs(float(f.out[0] - loss)) < 1e-10 and abs(float(f.out[1] - smax)) < 1e-12 and float(f.out[5]) == 0
    torch.testing.assert_close(r.g.dS.reshape(n, n), grad, rtol=RT, atol=1e-15)
    torch.testing.assert_close(r.g.dST.reshape(n, n), grad.T, rtol=RT, atol=1e-15)
    # modes 1 and 2 give mode 0
    s = R.fused_finalize_ref(r.colp, r.valid, r.g.gradp, None, 1, float(n), float(items), K, reg, softplus, torch.zeros(8, dtype=F64), torch.zeros(4, dtype=F64))
    f2 = R.fused_finalize_ref(None, None, None, s.sums, 2, float(n), float(items), K, reg, softplus, torch.zeros(8, dtype=F64))
    assert torch.equal(f2.out, f.out)


@pytest.mark.parametrize("softplus", [0, 1])
def test_two_rank_strips_agree_with_the_whole_and_with_autograd(softplus):
    items, K, E, reg, W = 64, 8, 128, 0.3, 2
    n = items * K
    nl = n // W
    g = R.gen(6)
    Pm, Tm = R.rounded(R.normal(g, n, E).double() * (2.0 / math.sqrt(E)), BF16), R.rounded(R.normal(g, n, E).double() * 2.0, BF16)
    loss, smax, grad = oracle(Pm, Tm, items, K, softplus, reg)
    whole = chain(Pm, Tm, K, 0, softplus, reg, n, items)
    torch.testing.assert_close(whole.g.dS.reshape(n, n), grad, rtol=RT, atol=1e-15)
    tot = torch.zeros(4, dtype=F64)
    for rank in range(W):
        lo = rank * nl
        col = chain(Pm, Tm[lo:lo + nl], K, -lo, softplus, reg, n, items)                       # all predictions x own targets
        torch.testing.assert_close(col.lse, whole.lse[lo:lo + nl], rtol=0, atol=1e-12)
        torch.testing.assert_close(col.g.dS.reshape(n, nl), grad[:, lo:lo + nl], rtol=RT, atol=1e-15)
        torch.testing.assert_close(col.g.dST.reshape(nl, n), grad[:, lo:lo + nl].T, rtol=RT, atol=1e-15)
        assert torch.equal(col.valid_written, (torch.arange(n) >= lo) & (torch.arange(n) < lo + nl))
        assert torch.equal(col.valid[lo:lo + nl], whole.valid[lo:lo + nl])
        row = chain(Pm[lo:lo + nl], Tm, K, lo, softplus, reg, n, items, lse_in=whole.lse)      # own predictions x all targets
        torch.testing.assert_close(row.g.dS.reshape(nl, n), grad[lo:lo + nl], rtol=RT, atol=1e-15)
        assert torch.equal(row.valid, whole.valid[lo:lo + nl])
        s = R.fused_finalize_ref(col.colp, col.valid[lo:lo + nl], col.g.gradp, None, 1, float(n), float(items), K, reg, softplus,
                                 torch.zeros(8, dtype=F64), torch.zeros(4, dtype=F64)).sums
        tot[:3] += s[:3]
        tot[3] = s[3] if rank == 0 else torch.maximum(tot[3], s[3])
    f = R.fused_finalize_ref(None, None, None, tot, 2, float(n), float(items), K, reg, softplus, torch.zeros(8, dtype=F64))
    assert abs(float(f.out[0] - loss)) < 1e-10 and abs(float(f.out[1] - smax)) < 1e-12


# ======================================================================================================== deliberate mistakes
def judge_pairs(got, ref, exact):
    """pm bitwise and ps (bound; exact: bitwise) per tile and column against the stored scores of ref -> ratio."""
    S = stored(ref.S)
    if not R.same_bits(got.pm, R.tile_pairs(S)[0]):
        return float("inf")
    if exact:
        return 0.0 if R.same_bits(got.ps, ref.ps) else float("inf")
    return R.ps_ratio(stored(got.ps), S)


@pytest.mark.parametrize("mut", ["drop_row", "swap_tiles"])
def test_pair_measure_rejects(mut):
    cid = "768x512-E192-ld"
    a = dict(R.score_cases())[cid]
    for recipe in ("narrow", "wide", "count"):
        ref, bad = case_ref(cid, recipe), run_score(a, recipe, mut)
        exact = recipe == "count"
        assert judge_pairs(ref, ref, exact) <= 1.0
        if recipe == "wide" and mut == "drop_row":      # (a wide column's smallest term is far below the rounding of its sum)
            continue
        assert judge_pairs(bad, ref, exact) > 1.0, f"{mut}: the {'count twin' if exact else 'bound on ' + recipe + ' data'} is too weak"
    if mut == "swap_tiles":                            # the merged lse cannot see it: the pairs have to be judged per tile
        ref, bad = case_ref(cid, "narrow"), run_score(a, "narrow", mut)
        la, lb = (R.lse_merge_ref(r.pm.reshape(-1), r.ps.reshape(-1), 3, 512, 0, 768.0).lse for r in (ref, bad))
        assert float((la - lb).abs().max()) < 1e-12


def test_count_twin_counts_rows():
    for cid in ("768x512-E192-ld", "256x256-E128"):
        r = case_ref(cid, "count")
        assert float(r.Sabs.max()) <= R.EXACT_MAX and float(case_ref(cid, "exact").Sabs.max()) <= R.EXACT_MAX
        assert bool((r.ps == r.ps.round()).all()) and float(r.ps.min()) >= 1 and float(r.ps.max()) <= 256
        assert torch.equal(r.ps, (r.S.reshape(-1, 256, r.S.shape[1]) == r.pm[:, None, :]).sum(1).double())
        assert len(set(r.ps.reshape(-1).tolist())) > 8                      # the counts differ between tiles and columns
        r32 = run_score(dict(R.score_cases())[cid], "count", dtype=F32)     # exp(-128) is 0 and exp(0) is 1 in f32
        assert R.same_bits(r32.ps, r.ps) and R.same_bits(r32.pm, r.pm) and R.same_bits(r32.S, r.S)


@pytest.mark.parametrize("mut", ["nrows_strip", "no_softplus_term"])
def test_lse_measure_rejects(mut):
    """A column strip: M = 768 rows of a problem with 1536 (the softplus term counts the rows of the whole problem)."""
    cid = "colstrip-768x256-off-256"
    for recipe in ("narrow", "wide", "count"):
        ref = case_ref(cid, recipe)
        S = stored(ref.S)
        good = R.lse_merge_ref(ref.pm.reshape(-1), ref.ps.reshape(-1), 3, 256, 1, 1536.0)
        bad = R.lse_merge_ref(ref.pm.reshape(-1), ref.ps.reshape(-1), 3, 256, 1, 1536.0, mut)
        assert R.lse_ratio_from_scores(stored(good.lse), S, 1, 1536.0) <= 1.0
        assert R.lse_ratio_from_scores(stored(bad.lse), S, 1, 1536.0) > 1.0, f"{mut}: the lse bound on {recipe} data is too weak"
        assert R.lse_ratio_from_pairs(stored(bad.lse), stored(ref.pm), stored(ref.ps), 3, 256, 1, 1536.0) > 1.0, (mut, recipe)


@pytest.mark.parametrize("mut", ["valid_at_r", "valid_off_by_one"])
def test_valid_measure_rejects(mut):
    for cid in ("colstrip-768x256-off-256", "512x512-off+100", "512x512-off-300"):
        a = dict(R.score_cases())[cid]
        for recipe in ("narrow", "exact"):
            ref, bad = case_ref(cid, recipe), run_score(a, recipe, mut)
            want = R.valid_of(stored(ref.S), a["diag_off"])[0]
            ok = lambda v: R.same_bits(torch.nan_to_num(stored(v), nan=-1e30), torch.nan_to_num(want, nan=-1e30))  # noqa: E731
            assert ok(ref.valid) and not ok(bad.valid), f"{mut}: bitwise valid on {recipe} data at {cid} is too weak"


GRAD_CASES = R.grad_cases()


def grad_run(a, recipe, softplus, mut=None, dtype=F64):
    S, lse, b = R.grad_data(a, recipe, softplus)
    return R.fused_grad_ref(S.to(dtype), lse.to(dtype), b["items"], b["K"], b["ncols"], b["ld"], b["ldT"], b["diag_off"], softplus, b["reg"],
                            b["n_rows_total"], b["n_items_total"], mut=mut)


def as_bf16(t):
    return t.to(BF16).double()


def grad_mutant_applies(mut, a):
    r = torch.arange(a["items"] * a["K"]) + a["diag_off"]
    has_diag = bool(((r >= 0) & (r < a["ncols"])).any())
    return {"diag_c_eq_r": has_diag and a["diag_off"] != 0, "lse_neighbour": a["ncols"] > 4, "mean_shift": a["items"] > 1, "reg_strip_items": True,
            "dst_chunk_early": a["items"] % 16 != 0 and a["items"] > 16, "zero_offdiag": True}[mut]


@pytest.mark.parametrize("mut", R.GRAD_MUTANTS)
def test_gradient_measure_rejects(mut):
    n = 0
    for cid, a in GRAD_CASES:
        if not grad_mutant_applies(mut, a):
            continue
        for recipe in ("narrow", "wide", "grad-exact"):
            exact = recipe == "grad-exact"
            if exact and not R.pow2(a["K"]) and mut in ("lse_neighbour", "reg_strip_items", "zero_offdiag"):
                continue                               # (those twins have m = 0 and no softmax term: see grad_data)
            for softplus in ((0,) if exact else (0, 1)):
                ref, bad = grad_run(a, recipe, softplus), grad_run(a, recipe, softplus, mut)
                which = "dST" if mut == "dst_chunk_early" else "dS"
                rv, bv, bw, ww = ((ref.dST, bad.dST, ref.bound_T, ref.written_T) if which == "dST" else (ref.dS, bad.dS, ref.bound_S, ref.written_S))
                assert R.grad_judge(as_bf16(rv), rv, bw, ww, exact) <= 1.0, cid
                q = R.grad_judge(as_bf16(bv), rv, bw, ww, exact)
                assert q > 1.0, f"{mut} at {cid} ({recipe}, softplus {softplus}): the {'grad-exact twin' if exact else 'per-element bound'} is too weak"
                n += 1
    assert n >= 6, (mut, n)


def test_grad_exact_twin_is_exact():
    """Asserted in float64: every gradient of the twin is a bf16 number, and float32 evaluation gives the same bits."""
    for cid, a in GRAD_CASES:
        S, lse, b = R.grad_data(a, "grad-exact", 0)
        assert R.pow2(b["n_rows_total"]) and R.pow2(b["n_items_total"]) and R.pow2(b["reg"])
        r = grad_run(a, "grad-exact", 0)
        w = r.written_S
        assert float((as_bf16(r.dS[w]) - r.dS[w]).abs().max()) < 1e-40, cid        # (float64 keeps the weights e^-128 / n that f32 drops)
        e = grad_run(a, "grad-exact", 0, dtype=F32)
        assert R.grad_judge(e.dS, r.dS, r.bound_S, w, True) == 0.0 and R.grad_judge(e.dST, r.dST, r.bound_T, r.written_T, True) == 0.0, cid
        if R.pow2(a["K"]):
            assert int((r.d[~r.diag] != 0).sum()) > r.d.numel() // 2, cid


# ======================================================================================================== the old measure
def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_old_whole_tensor_measure_accepts_a_gradient_without_its_off_diagonal():
    """test_hip_kernels.py's rel_err(dS, grad) < 1.5e-2 on its own three data recipes, both score kinds: the share of the reference
    gradient's elements that lie below the threshold (a kernel that wrote zero into all of them would pass), and the mutant that zeroes
    every such element (the off-diagonal ones, about 1/R^2 against the diagonal's 1/R) passes the old measure and fails the per-element bound."""
    shares = []
    for items, K, E, reg in ((64, 8, 128, 1.0), (32, 16, 192, 0.01), (64, 12, 512, 0.5)):
        n = items * K
        g = torch.Generator().manual_seed(items + K + E)
        Pm = (torch.randn(n, E, generator=g) * (2.0 / math.sqrt(E))).to(BF16)
        Tm = (torch.randn(n, E, generator=g) * 2.0).to(BF16)
        Pm[0] = Tm[0] * 0.25
        for softplus in (0, 1):
            _, _, grad = oracle(Pm.double(), Tm.double(), items, K, softplus, reg)
            below = grad.abs() < 1.5e-2 * grad.abs().max()
            shares.append(float(below.double().mean()))
            zeroed = torch.where(below, torch.zeros_like(grad), grad)
            assert rel_err(as_bf16(zeroed), grad) < 1.5e-2
            r = chain(Pm.double(), Tm.double(), K, 0, softplus, reg, n, items)
            flat = torch.full_like(r.g.dS, R.NAN)
            flat[r.g.written_S] = as_bf16(torch.where(below, torch.zeros_like(grad), r.g.d)).reshape(-1)
            assert R.grad_judge(flat, r.g.dS, r.g.bound_S, r.g.written_S, False) > 1.0
            one = as_bf16(r.g.d).clone()
            one[n // 2, 3] = 0
            print(f"old measure, one zeroed element: moves by {abs(rel_err(one, grad) - rel_err(as_bf16(r.g.d), grad)):.1e}")
    print("share of gradient elements below the old threshold: " + ", ".join(f"{100 * s:.1f} %" for s in shares))
    assert min(shares) >= 0.96 and sum(shares) / len(shares) >= 0.97          # measured: 96.7 % (64 / 8 / 128, softplus) to 99.0 %


# ======================================================================================================== reference alone
def test_float32_emulation_stays_within_the_bounds():
    worst = collections.defaultdict(float)
    for cid, a in R.score_cases()[:3]:
        for recipe in R.RECIPES:
            r, e = case_ref(cid, recipe), run_score(a, recipe, dtype=F32)
            exact = recipe in ("exact", "count")
            q = R.s_ratio(e.S, r, a["E"])
            assert (q == 0.0) if exact else (q <= 1.0), (cid, recipe, q)
            worst[f"S {recipe}"] = max(worst[f"S {recipe}"], q)
            assert R.same_bits(e.pm, R.tile_pairs(e.S)[0]) and R.same_bits(R.valid_of(e.S, a["diag_off"])[0].nan_to_num(), e.valid.nan_to_num())
            q = R.ps_ratio(e.ps, e.S)
            assert q <= 1.0, (cid, recipe, q)
            worst[f"ps {recipe}"] = max(worst[f"ps {recipe}"], q)
            for softplus in (0, 1):
                nrows = 2.0 * a["M"]
                m = R.lse_merge_ref(e.pm.reshape(-1), e.ps.reshape(-1), a["M"] // 256, a["N"], softplus, nrows)
                q = R.lse_ratio_from_scores(m.lse, e.S, softplus, nrows)
                assert q <= 1.0, (cid, recipe, softplus, q)
                worst[f"lse {recipe}"] = max(worst[f"lse {recipe}"], q)
                q = R.colp_ratio(m.colp, m.lse, e.pm, a["M"] // 256, a["N"])
                assert q <= 1.0
                worst["colp"] = max(worst["colp"], q)
    for nparts in R.MERGE_NPARTS:
        for ncols in R.MERGE_NCOLS:
            for wide in (False, True):
                pm, ps = R.merge_data(nparts, ncols, wide)
                for softplus in (0, 1):
                    for nrows in (256.0 * nparts, 4096.0):
                        m = R.lse_merge_ref(pm.float(), ps.float(), nparts, ncols, softplus, nrows)
                        q = R.lse_ratio_from_pairs(m.lse, pm, ps, nparts, ncols, softplus, nrows)
                        assert q <= 1.0, (nparts, ncols, wide, softplus, q)
                        worst[f"merge {'wide' if wide else 'narrow'}"] = max(worst[f"merge {'wide' if wide else 'narrow'}"], q)
    for cid, a in GRAD_CASES:
        for recipe in ("narrow", "wide"):
            for softplus in (0, 1):
                r, e = grad_run(a, recipe, softplus), grad_run(a, recipe, softplus, dtype=F32)
                q = max(R.grad_judge(e.dS, r.dS, r.bound_S, r.written_S, False, u=0.0), R.grad_judge(e.dST, r.dST, r.bound_T, r.written_T, False, u=0.0))
                assert q <= 1.0, (cid, recipe, softplus, q)
                worst[f"dS {recipe}"] = max(worst[f"dS {recipe}"], q)
                q = float(((e.gradp.double() - r.gradp).abs() / r.bound_gradp.clamp_min(1e-300)).max())
                assert q <= 1.0, (cid, q)
                worst["gradp"] = max(worst["gradp"], q)
    for k in sorted(worst):
        print(f"reference alone {k}: {worst[k]:.4f}")


# ======================================================================================================== tile walk
def test_tile_walk_mirror_shows_what_each_multi_tile_case_is_for():
    w = R.tile_walk(1, 1)
    assert w.blocks == 8 and w.grid == 8 and sum(1 for t in w.walks if not t) == 7
    w = R.tile_walk(1, 33)
    assert w.blocks == 264 and [len(t) for t in w.walks].count(2) == 1 and max(len(t) for t in w.walks) == 2 and not w.stagger
    w = R.tile_walk(8, 33)
    assert w.blocks == 264 and [len(t) for t in w.walks].count(2) == 8 and min(len(t) for t in w.walks) == 1
    w = R.tile_walk(9, 17)
    assert w.blocks == 272 and any(mt == 8 for t in w.walks for mt, _ in t) and max(len(t) for t in w.walks) == 2
    w = R.tile_walk(1, 65)
    assert w.blocks == 520 and w.stagger and sum(1 for t in w.walks if len(t) >= 2) == 32 and {len(t) for t in w.walks} == {0, 2, 3}
    for cid, a, what in R.walk_cases():
        numM, numN = a["M"] // 256, a["N"] // 256
        w = R.tile_walk(numM, numN)
        tiles = [t for wk in w.walks for t in wk]
        assert sorted(tiles) == [(m, n) for m in range(numM) for n in range(numN)], cid          # every tile exactly once
        assert max(len(t) for t in w.walks) >= 2 and R.later_tiles(numM, numN), cid
        assert {"one-two": (numM, numN) == (1, 33), "eight-two": (numM, numN) == (8, 33), "spill": (numM, numN) == (9, 17),
                "stagger": (numM, numN) == (1, 65) and w.stagger}[what], cid
        rows = R.walk_rows(a)
        assert all(len(rows[t]) == 256 for t in R.later_tiles(numM, numN)), cid
    # odd numbers of K stages across a tile change (the next tile starts on the other LDS slot), and the shortest hand-over nk = 2
    assert {a["E"] // 64 for _, a, _ in R.walk_cases()} >= {2, 3, 4}
