"""Plain float64 references of the fused score-LSE loss chain (score_over_all_timesteps=True in bf16: cpc_score_lse in csrc/gemm.hip,
cpc_nce_lse_merge / cpc_nce_fused_grad / cpc_nce_fused_finalize in csrc/nce.hip), each at the level of its entry point's arguments
(flat arrays with leading dimensions, diag_off, nrows_total, n_items_total), the host mirror of the persistent tile walk, the case lists,
the data recipes and the per-element bounds.  Shared by test_fused_score_kernels_gpu.py (the kernels against these references) and
test_fused_score_reference_host.py (these references against torch.logsumexp, oracle.info_nce_loss and autograd, a float32 emulation
against the bounds, the measures against deliberate mistakes).  Nothing here touches a device.  Every reference works in the dtype of
its inputs: float64 gives the reference, float32 the host emulation.

Bounds (u = 2^-24; derived here, none comes from a kernel run).

S       conv1d_reference.bound with u_out = 0 and n = E:  |S - ref| <= 2 (E + 2) u sum_e |p||t|.
pm      bitwise the maximum of the STORED f32 scores over the tile's 256 rows (max is exact).  valid: bitwise S[r][r + diag_off].
ps      against float64 on the stored f32 scores (the GEMM's rounding is not counted twice).  Every term is positive, so the relative
        error of the sum is at most the largest relative error of a term plus that of the summation.  A term is
        exp(s - cm) exp(ma - mm): cm the maximum of the 128 rows of the term's half tile, mm the tile's.  The device takes both with
        __expf, HIP's native exponential: exp2 of x log2(e) on V_EXP_F32, which the CDNA instruction set guide specifies to 1 ulp.
        For an argument x = a - b <= 0: the subtraction rounds (u |x|), the product with log2(e) rounds (u |x log2 e|) and log2(e)
        itself is off by at most u / 2 relative; exp2 turns an absolute error d of its argument into the relative error d ln 2, and
        ln 2 log2 e = 1: 2.5 u |x|, plus 2 u for the 1-ulp instruction.  The arguments of a term telescope, (cm - s) + (mm - ma) <= mm - s
        <= spread of the tile column, so a term is off by u (2 * 2 + 2.5 spread) relative.  Summation: 8 rows per lane, 4 exchange levels,
        one merge of the halves (13 additions over a term) and one product: 14 u.
            |ps - ref| <= u (PS_A + EXP_B spread) ref,   PS_A = 18, EXP_B = 2.5
        (terms below the smallest normal f32 may be flushed: relative to a sum >= 1 that is below 2^-100 and left out).
lse     = ref + log(tot), tot = [softplus] nrows exp(-ref) + sum_parts ps exp(pm - ref), ref = max pm (softplus: max(max pm, 0)).  Against
        float64 on the stored f32 scores.  The third exponential is expf (<= 1 ulp, argument rounding u |x|, under 2.5 u |x|) and its
        argument telescopes with the two above: EXP_B spread_c with spread_c = max - min of the whole column, 3 * 2 u for three
        exponentials; additions 13 + nparts + 1; products 2; logf to 1 ulp of log tot, |log tot| <= L = ln(2 max(nrows, 256 nparts));
        softplus: where ref = 0 > max pm a part's argument is pm itself, |pm| exp(pm) <= 1 / e of a total >= nrows exp(0): 1 u; the term
        nrows exp(-ref) is off by u (ref + 2) of itself, and its share of the total is at most min(1, nrows exp(-ref)): u (2 + ln nrows).
        The relative error of tot is the absolute error of its logarithm:
            |lse - ref| <= u (a + EXP_B spread_c) + u |ref|,   a = 22 + nparts + 2 L + [softplus] (3 + ln nrows)
        (u |ref|: the last addition).  a = 16, b = 2, which a float32 numpy evaluation satisfies, is below what the device's path
        allows: the derived values are used.
dS      = score'(s) ((w - [c == r + diag_off]) / n_rows + reg_c m), w = exp(sp - lse[c]), m = mean_k sp, reg_c = 2 reg / (n_items^2 K^2),
        stored as bf16: 2^-8 |ref| for that rounding plus the f32 terms
            u |score'| ( (11 + 2.5 |sp - lse| + [softplus] 4 |sp|) w / n_rows + (K + 19) |reg_c| mean_k |sp| + 7 [diagonal] / n_rows )
        softplus(s) = log1pf(expf(s)) is off by 4 u relative (two 1-ulp functions), which enters the exponent as an absolute error;
        the exponent's own rounding and __expf as above (2.5 |x| + 2); 1 / n_rows, the product with it, the sum of the two terms,
        the derivative (expf, an addition, a division: 4) and the product with it: 1 each.  reg_c: 4 roundings; m: K additions of terms
        off by 4 u, the product with 1 / K and that constant's rounding; the diagonal subtracts 1 / n_rows (1 u) and rounds once: its
        absolute error is that of the weight, not of the difference.  A floor of 2^-120 covers intermediate values below the smallest
        normal f32, which the device may flush.
gradp, colp[.][0], the sums of finalize:  (n + 2) u sum |terms|  (gradp: n = 1024 + 2 (K + 7), the terms m^2 carry their own
        error; colp and finalize: against float64 on the stored inputs; softplus of a valid score: 4 u more).
colp[.][1], sums[3], out[1] for linear scores: exact.
"""
import math
from types import SimpleNamespace

import torch

from conv1d_reference import BF16, F32, F64, U24, U8, EXACT_MAX, bound, gen, ints, normal, rounded, sparse  # noqa: F401

NAN = float("nan")
TB = 256                      # tile edge of gemm_nt_persist_kernel
NFG_IT, NFG_CW = 16, 64       # workgroup of nce_fused_grad_kernel: items x columns
PS_A, EXP_B = 18.0, 2.5
FLOOR = 2.0 ** -120


# ------------------------------------------------------------------------------------------------------------------ tile walk
def nt_grid_blocks(numM, numN):
    return 8 * ((numM + 7) // 8) * numN


def nt_tile_of_block(bid, numM, numN):
    """-> (mt, nt) or None for a padding block of the 8-XCD grid."""
    xcd, slot = bid & 7, bid >> 3
    mt, nt = (slot // numN) * 8 + xcd, slot % numN
    return (mt, nt) if mt < numM else None


def tile_walk(numM, numN):
    """launch_score_lse's grid = min(256, blocks); workgroup w takes blocks w, w + grid, ...  -> [the tiles of workgroup w, in order]."""
    blocks = nt_grid_blocks(numM, numN)
    grid = min(256, blocks)
    walks = [[t for t in (nt_tile_of_block(b, numM, numN) for b in range(w, blocks, grid)) if t is not None] for w in range(grid)]
    return SimpleNamespace(blocks=blocks, grid=grid, walks=walks, stagger=blocks > 512)


def later_tiles(numM, numN):
    """The tiles some workgroup reaches as its second or later tile."""
    return sorted({t for w in tile_walk(numM, numN).walks for t in w[1:]})


# ------------------------------------------------------------------------------------------------------------------ score_tf
def score_tf(x, softplus):
    """torch.nn.functional.softplus, beta = 1, threshold = 20 (nce.hip score_tf)."""
    if not softplus:
        return x
    return torch.where(x > 20, x, torch.log1p(torch.exp(x.clamp_max(20))))


def score_grad(x, softplus):
    if not softplus:
        return torch.ones_like(x)
    return torch.where(x > 20, torch.ones_like(x), 1 / (1 + torch.exp(-x)))


# ------------------------------------------------------------------------------------------------------------------ cpc_score_lse
def tile_pairs(S, mut=None):
    """S [M][N] -> pm, ps [M / 256][N]: (max, sum exp(s - max)) over each tile's rows."""
    M, N = S.shape
    t = S.reshape(M // TB, TB, N)
    pm = t.max(1).values
    e = torch.exp(t - pm[:, None, :])
    if mut == "drop_row":                                # tile 0, column 1: the row with the smallest term that is not zero in f32 is missing
        e = e.clone()
        col = e[0, :, 1]
        e[0, int(torch.where(col > 1e-37, col, torch.full_like(col, 2.0)).argmin()), 1] = 0
    ps = e.sum(1)
    if mut == "swap_tiles" and M // TB > 1:
        pm, ps = pm.flip(0), ps.flip(0)
    return pm, ps


def valid_of(S, diag_off, mut=None):
    """-> valid [M] (NaN where no column r + diag_off exists: the call leaves those elements alone), written [M]."""
    M, N = S.shape
    off = {"valid_at_r": 0, "valid_off_by_one": diag_off + 1}.get(mut, diag_off)
    c = torch.arange(M) + off
    ok = (c >= 0) & (c < N)
    v = torch.full((M,), NAN, dtype=S.dtype)
    v[ok] = S[torch.arange(M)[ok], c[ok]]
    return v, ok


def score_lse_ref(P, T, M, N, E, ldp, ldt, diag_off, mut=None):
    """P / T: flat arrays, row r at r ldp / c ldt.  -> S, Sabs [M][N], pm, ps, valid, valid_written."""
    Pm = P[(torch.arange(M)[:, None] * ldp + torch.arange(E)[None, :])]
    Tm = T[(torch.arange(N)[:, None] * ldt + torch.arange(E)[None, :])]
    S, Sabs = Pm @ Tm.T + 0.0, Pm.abs() @ Tm.abs().T
    pm, ps = tile_pairs(S, mut)
    valid, vw = valid_of(S, diag_off, mut)
    return SimpleNamespace(S=S, Sabs=Sabs, pm=pm, ps=ps, valid=valid, valid_written=vw)


def s_ratio(got, r, E, rows=None):
    """max |S - ref| / bound over the rows given (all)."""
    got = torch.as_tensor(got).double().cpu()
    ref, Sabs = (r.S, r.Sabs) if rows is None else (r.S[rows], r.Sabs[rows])
    got = got if rows is None else got[rows]
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    b = bound(ref.double(), Sabs.double(), E, 0.0)
    err = (got - ref.double()).abs()
    q = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max())


def _ratio(err, b):
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float((err / b).max()) if err.numel() else 0.0


def ps_ratio(ps, S_stored):
    """ps against float64 on the stored scores, per tile and column."""
    S = torch.as_tensor(S_stored).double().cpu()
    M, N = S.shape
    t = S.reshape(M // TB, TB, N)
    _, ref = tile_pairs(S)
    spread = t.max(1).values - t.min(1).values
    return _ratio((torch.as_tensor(ps).double().cpu() - ref).abs(), U24 * (PS_A + EXP_B * spread) * ref)


def same_bits(a, b):
    a, b = torch.as_tensor(a).float().cpu().contiguous(), torch.as_tensor(b).float().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ cpc_nce_lse_merge
def lse_merge_ref(pm, ps, nparts, ncols, softplus, nrows_total, mut=None):
    """pm / ps flat [nparts][ncols] -> lse [ncols], colp [ceil(ncols / 256)][2] = {sum of the block's lse, max of its pm}."""
    pm, ps = pm.reshape(nparts, ncols), ps.reshape(nparts, ncols)
    if mut == "nrows_strip":
        nrows_total = 256.0 * nparts
    mx = pm.max(0).values
    ref = mx.clamp_min(0) if softplus else mx
    tot = (ps * torch.exp(pm - ref)).sum(0)
    if softplus and mut != "no_softplus_term":
        tot = tot + nrows_total * torch.exp(-ref)
    lse = ref + torch.log(tot)
    nb = (ncols + 255) // 256
    colp = torch.zeros(nb, 2, dtype=pm.dtype)
    for b in range(nb):
        colp[b, 0], colp[b, 1] = lse[b * 256:(b + 1) * 256].sum(), mx[b * 256:(b + 1) * 256].max()
    return SimpleNamespace(lse=lse, colp=colp)


def lse_a(nparts, softplus, nrows_total):
    L = math.log(2.0 * max(nrows_total, 256.0 * nparts))
    return 22.0 + nparts + 2.0 * L + (3.0 + math.log(nrows_total) if softplus else 0.0)


def lse_bound(ref, spread, nparts, softplus, nrows_total):
    return U24 * (lse_a(nparts, softplus, nrows_total) + EXP_B * spread) + U24 * ref.abs()


def lse_ratio_from_scores(lse, S_stored, softplus, nrows_total):
    """lse of a whole-column launch against float64 on the stored scores (nrows_total rows of which S_stored holds all: M == nrows_total,
    or a strip whose softplus term counts the rows of the whole problem)."""
    S = torch.as_tensor(S_stored).double().cpu()
    pm, ps = tile_pairs(S)
    r = lse_merge_ref(pm, ps, S.shape[0] // TB, S.shape[1], softplus, float(nrows_total))
    spread = S.max(0).values - S.min(0).values
    return _ratio((torch.as_tensor(lse).double().cpu() - r.lse).abs(), lse_bound(r.lse, spread, S.shape[0] // TB, softplus, nrows_total))


def lse_ratio_from_pairs(lse, pm, ps, nparts, ncols, softplus, nrows_total):
    """lse against float64 on the stored pairs: the merge alone.  spread = the spread of the parts' maxima (the arguments of its expf)."""
    pm64, ps64 = (torch.as_tensor(t).double().cpu().reshape(nparts, ncols) for t in (pm, ps))
    r = lse_merge_ref(pm64, ps64, nparts, ncols, softplus, float(nrows_total))
    spread = pm64.max(0).values - pm64.min(0).values
    return _ratio((torch.as_tensor(lse).double().cpu() - r.lse).abs(), lse_bound(r.lse, spread, nparts, softplus, nrows_total))


def colp_ratio(colp, lse_stored, pm, nparts, ncols):
    """colp against float64 on the stored lse: [0] within (256 + 2) u sum |lse|, [1] exact.  -> ratio (inf where [1] differs)."""
    lse, pm = torch.as_tensor(lse_stored).double().cpu(), torch.as_tensor(pm).double().cpu().reshape(nparts, ncols)
    colp = torch.as_tensor(colp).double().cpu().reshape(-1, 2)
    q = 0.0
    for b in range((ncols + 255) // 256):
        blk = lse[b * 256:(b + 1) * 256]
        if float(colp[b, 1]) != float(pm[:, b * 256:(b + 1) * 256].max()):
            return float("inf")
        q = max(q, _ratio((colp[b, 0] - blk.sum()).abs().reshape(1), (258 * U24 * blk.abs().sum()).clamp_min(1e-300).reshape(1)))
    return q


# ------------------------------------------------------------------------------------------------------------------ cpc_nce_fused_grad
GRAD_MUTANTS = ["diag_c_eq_r", "lse_neighbour", "mean_shift", "reg_strip_items", "dst_chunk_early", "zero_offdiag"]


def fused_grad_ref(S, lse, items, K, ncols, ld, ldT, diag_off, softplus, reg, n_rows_total, n_items_total, sizeD=None, sizeT=None, mut=None):
    """S flat [items K][ld], lse [ncols] -> dS flat (sizeD elements, NaN where the call does not write), dST flat [ncols][ldT] (sizeT),
    gradp [grid.y][grid.x] flat, the written maps, and bound_f32 / bound_gradp (the f32 terms of the bounds in the module docstring)."""
    R = items * K
    dt = S.dtype
    s = S[(torch.arange(R)[:, None] * ld + torch.arange(ncols)[None, :])]
    sp, g = score_tf(s, softplus), score_grad(s, softplus)
    l = lse[:ncols]
    if mut == "lse_neighbour":                         # element 0 of the group of four for every element
        l = l[torch.arange(ncols) // 4 * 4]
    src = sp
    if mut == "mean_shift":                            # the mean over rows shifted by one: it crosses the item boundary
        src = torch.roll(sp, -1, 0)
    m = src.reshape(items, K, ncols).mean(1)
    mabs = sp.abs().reshape(items, K, ncols).mean(1)
    ni = float(items) if mut == "reg_strip_items" else n_items_total
    reg_c = 2.0 * reg / (ni * ni * K * K)
    w = torch.exp(sp - l[None, :])
    r_idx, c_idx = torch.arange(R)[:, None], torch.arange(ncols)[None, :]
    diag = (c_idx == r_idx + (0 if mut == "diag_c_eq_r" else diag_off)).to(dt)
    mrep, mabs_rep = m.repeat_interleave(K, 0), mabs.repeat_interleave(K, 0)
    d = (w / n_rows_total + reg_c * mrep - diag / n_rows_total) * g
    if mut == "zero_offdiag":
        d = d * diag
    bf = U24 * g.abs() * ((11 + EXP_B * (sp - l[None, :]).abs() + (4 * sp.abs() if softplus else 0)) * w / n_rows_total +
                          (K + 19) * abs(reg_c) * mabs_rep + 7 * diag / n_rows_total) + FLOOR
    sizeD = R * ld if sizeD is None else sizeD
    sizeT = ncols * ldT if sizeT is None else sizeT
    dS, dST = torch.full((sizeD,), NAN, dtype=dt), torch.full((sizeT,), NAN, dtype=dt)
    bS, bT = torch.zeros(sizeD, dtype=dt), torch.zeros(sizeT, dtype=dt)
    wS, wT = torch.zeros(sizeD, dtype=torch.bool), torch.zeros(sizeT, dtype=torch.bool)
    iS = (r_idx * ld + c_idx).reshape(-1)
    dS[iS], bS[iS], wS[iS] = d.reshape(-1), bf.reshape(-1), True
    iT = (c_idx * ldT + r_idx).reshape(-1)             # element (r, c) of dS sits at c ldT + r of dST
    if mut == "dst_chunk_early" and items % NFG_IT and items > NFG_IT:
        first = items // NFG_IT * NFG_IT * K           # the rows of the partial last item block land one block early
        rr = torch.where(torch.arange(R) >= first, torch.arange(R) - NFG_IT * K, torch.arange(R))[:, None]
        keep = (torch.arange(R) < first - NFG_IT * K) | (torch.arange(R) >= first)
        iT2 = (c_idx * ldT + rr)[keep].reshape(-1)
        dST[iT2] = d[keep].reshape(-1)
        wT[iT2] = True
        bT[iT] = bf.reshape(-1)
    else:
        dST[iT], bT[iT], wT[iT] = d.reshape(-1), bf.reshape(-1), True
    gx, gy = (ncols + NFG_CW - 1) // NFG_CW, (items + NFG_IT - 1) // NFG_IT
    gradp, gb = torch.zeros(gy * gx, dtype=dt), torch.zeros(gy * gx, dtype=dt)
    for by in range(gy):
        for bx in range(gx):
            blk = m[by * NFG_IT:(by + 1) * NFG_IT, bx * NFG_CW:(bx + 1) * NFG_CW]
            ab = mabs[by * NFG_IT:(by + 1) * NFG_IT, bx * NFG_CW:(bx + 1) * NFG_CW]
            gradp[by * gx + bx], gb[by * gx + bx] = (blk * blk).sum(), (1024 + 2 * (K + 7) + 2) * U24 * (ab * ab).sum()
    return SimpleNamespace(dS=dS, dST=dST, gradp=gradp, written_S=wS, written_T=wT, bound_S=bS, bound_T=bT, bound_gradp=gb, d=d, diag=diag.bool())


def grad_judge(got, ref, bnd, written, exact, u=U8):
    """The whole flat bf16 output: unwritten elements still NaN, written ones within 2^-8 |ref| + the f32 term, or bit for bit (twin).
    -> ratio (exact: 0 or inf).  u = 0: the float32 emulation, which stores nothing."""
    got = torch.as_tensor(got).double().cpu().reshape(-1)
    if not bool(torch.isnan(got[~written]).all()):
        return float("inf")
    if exact:
        return 0.0 if torch.equal(got[written].to(BF16).view(torch.int16), ref[written].to(BF16).view(torch.int16)) else float("inf")
    r = ref[written].double()
    return _ratio((got[written] - r).abs(), u * r.abs() + bnd[written].double())


# ------------------------------------------------------------------------------------------------------------------ cpc_nce_fused_finalize
def fused_finalize_ref(colp, valid, gradp, sums, mode, n_rows, n_items, K, reg, softplus, out_init, sums_init=None):
    """-> out [8] (from out_init; untouched in mode 1), sums [4] (mode 1), err [8]: the bound of each written out element, err_sums [4]."""
    out, err = out_init.clone(), torch.zeros(8, dtype=F64)
    s4 = None if sums_init is None else sums_init.clone()
    es = torch.zeros(4, dtype=F64)
    if mode != 2:
        sv_t = score_tf(valid, softplus)
        sv, sl, sm, mx = sv_t.sum(), colp.reshape(-1, 2)[:, 0].sum(), gradp.sum(), colp.reshape(-1, 2)[:, 1].max()
        es = torch.tensor([(valid.numel() + 2 + (4 if softplus else 0)) * U24 * float(sv_t.abs().sum()),
                           (colp.numel() // 2 + 2) * U24 * float(colp.reshape(-1, 2)[:, 0].abs().sum()),
                           (gradp.numel() + 2) * U24 * float(gradp.abs().sum()), 0.0], dtype=F64)
    else:
        sv, sl, sm, mx = sums[0], sums[1], sums[2], sums[3]
    if mode == 1:
        s4[0], s4[1], s4[2], s4[3] = sv, sl, sm, mx
        return SimpleNamespace(out=out, sums=s4, err=err, err_sums=es)
    t_valid, t_lse, t_reg = -sv / n_rows, sl / n_rows, reg * sm / (n_items * n_rows)
    out[0], out[1], out[2], out[3], out[4] = t_valid + t_lse + t_reg, score_tf(mx.reshape(1), softplus)[0], t_valid, t_lse, t_reg
    lb = t_valid + t_lse
    bad = bool(lb != lb)
    out[5] = 1.0 if bad else 0.0
    if bad:
        out[6] = 1.0
    e2, e3, e4 = (float(es[0]) / n_rows + 2 * U24 * abs(float(t_valid)), float(es[1]) / n_rows + 2 * U24 * abs(float(t_lse)),
                  abs(reg) * float(es[2]) / (n_items * n_rows) + 4 * U24 * abs(float(t_reg)))
    err[2], err[3], err[4] = e2, e3, e4
    err[0] = e2 + e3 + e4 + 2 * U24 * (abs(float(t_valid)) + abs(float(t_lse)) + abs(float(t_reg)))
    err[1] = 4 * U24 * abs(float(out[1])) if softplus else 0.0
    return SimpleNamespace(out=out, sums=s4, err=err, err_sums=es)


# ------------------------------------------------------------------------------------------------------------------ data: cpc_score_lse
RECIPES = ["narrow", "wide", "exact", "count"]


def score_data(recipe, M, N, E, ldp, ldt, diag_off, seed=0):
    """float64 flat P [M][ldp] / T [N][ldt], exact in bf16, NaN in the ldp - E / ldt - E padding (the call may not read it)."""
    g = gen(seed + M * 7 + N * 13 + E + RECIPES.index(recipe))
    if recipe == "narrow":                             # a column's scores spread over a few units: every row carries ~1/256 of its tile's sum
        P, T = normal(g, M, E).double() / math.sqrt(E), normal(g, N, E).double()
    elif recipe == "wide":                             # scores out to about +-100; own-target scores above 20; columns wholly below -30
        P, T = normal(g, M, E).double() * (30.0 / math.sqrt(E)), normal(g, N, E).double()
        P[:, 0] = 1.0
        for r in range(0, M, 37):                      # a few own-target scores of about 40
            c = r + diag_off
            if 0 <= c < N:
                P[r] = T[c] * (40.0 / E)
                P[r, 0] = 1.0
        T[5::53, 0] = -200.0                           # random part: sd 30, |.| < 170 at 5 sd
    elif recipe == "exact":                            # small integers, thinned: every partial sum in any order is exact
        P = ints(g, -2, 2, M, E)
        T = sparse(g, ints(g, -1, 1, N, E), min(1.0, 40.0 / E))
        T[:, E - 1] = 1.0                              # the last K element of every row counts
    else:                                              # count: s[r][c] = v_c - 128 [group of r is masked in column c]
        P, T = torch.zeros(M, E, dtype=F64), torch.zeros(N, E, dtype=F64)
        grp = torch.randint(0, 4, (M,), generator=g)
        P[torch.arange(M), grp] = 1.0
        P[:, E - 1] = 1.0
        mask = torch.randint(0, 15, (N,), generator=g)             # 4 bits, never all four
        for b in range(4):
            T[:, b] = -128.0 * ((mask >> b) & 1).double()
        T[:, E - 1] = (torch.arange(N) % 7 - 3).double()
    P, T = rounded(P, BF16), rounded(T, BF16)
    Pf, Tf = torch.full((M, ldp), NAN, dtype=F64), torch.full((N, ldt), NAN, dtype=F64)
    Pf[:, :E], Tf[:, :E] = P, T
    return Pf.reshape(-1), Tf.reshape(-1)


def SC(M, N, E, **kw):
    a = dict(M=M, N=N, E=E, ldp=E, ldt=E, lds=N, diag_off=0, valid=True, store=True)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def score_cases():
    """[(id, args)] of cpc_score_lse.  Small: the whole S is judged; multi-tile walks: see test_fused_score_kernels_gpu.py."""
    return [("256x256-E128", SC(256, 256, 128)),
            ("768x512-E192-ld", SC(768, 512, 192, ldp=200, ldt=264, lds=516)),
            ("colstrip-768x256-off-256", SC(768, 256, 128, diag_off=-256)),
            ("colstrip-768x256-off-512", SC(768, 256, 128, diag_off=-512)),
            ("rowstrip-256x768-off+256-novalid", SC(256, 768, 128, diag_off=256, valid=False)),
            ("512x512-off+100", SC(512, 512, 128, diag_off=100)),
            ("512x512-off-300", SC(512, 512, 128, diag_off=-300)),
            ("512x512-off+N", SC(512, 512, 128, diag_off=512)),
            ("512x512-off-M", SC(512, 512, 128, diag_off=-512))]


def walk_cases():
    """The multi-tile walks: (id, args, what the host mirror must show)."""
    return [("256x8448-E128", SC(256, 8448, 128), "one-two"), ("256x8448-E192", SC(256, 8448, 192), "one-two"),
            ("256x8448-E256", SC(256, 8448, 256), "one-two"), ("2048x8448-E128", SC(2048, 8448, 128), "eight-two"),
            ("2304x4352-E192", SC(2304, 4352, 192), "spill"), ("256x16640-E192", SC(256, 16640, 192), "stagger")]


def walk_rows(a):
    """Rows of S judged in a multi-tile case, per N tile: {nt: row indices}.  All rows of the tiles some workgroup reaches as its second
    or later tile and of their neighbours (the tile before and after in the walk's N order); a seeded 64 rows of every other tile."""
    numM, numN = a["M"] // TB, a["N"] // TB
    full = set()
    for mt, nt in later_tiles(numM, numN):
        for dn in (-1, 0, 1):
            if 0 <= nt + dn < numN:
                full.add((mt, nt + dn))
    sub = torch.randperm(TB, generator=gen(11))[:64].sort().values
    return {(mt, nt): (torch.arange(TB) if (mt, nt) in full else sub) + mt * TB for mt in range(numM) for nt in range(numN)}


# ------------------------------------------------------------------------------------------------------------------ data: merge
MERGE_NPARTS, MERGE_NCOLS = [1, 2, 3, 9], [4, 255, 256, 257, 520]


def merge_data(nparts, ncols, wide, seed=0):
    """Synthetic pairs: pm spread over a few units (wide: out to +-100, some columns wholly below -30), ps in [1, 256]."""
    g = gen(seed + nparts * 11 + ncols + (3 if wide else 0))
    pm = normal(g, nparts, ncols).double() * (40.0 if wide else 1.5)
    if wide:
        pm[:, 1::5] = -30.0 - 50.0 * torch.rand(nparts, pm[:, 1::5].shape[1], generator=g).double()
    ps = 1.0 + 255.0 * torch.rand(nparts, ncols, generator=g).double()
    return rounded(pm, F32).reshape(-1), rounded(ps, F32).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ data: gradient
GRAD_K, GRAD_ITEMS, GRAD_NCOLS = [2, 8, 12, 16, 22, 24], [1, 15, 16, 17, 33], [4, 60, 64, 68, 260]


def GC(items, K, ncols, **kw):
    a = dict(items=items, K=K, ncols=ncols, ld=(ncols + 7) // 8 * 8 + 8, ldT=(items * K + 7) // 8 * 8 + 8, diag_off=0, reg=0.5,
             n_rows_total=float(2 * items * K), n_items_total=float(2 * items))
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def grad_cases():
    """[(id, args)].  Every K meets a partial item block (items 15, 17, 33) and a whole one; every ncols both kinds of K kernel; diag_off
    inside the strip and outside it (no diagonal at all); ld / ldT larger than needed throughout, and exactly as needed once."""
    cases = []
    for i, K in enumerate(GRAD_K):
        for j, items in enumerate(GRAD_ITEMS):
            ncols = GRAD_NCOLS[(i + j) % len(GRAD_NCOLS)]
            off = [0, 3, -(items * K) // 2 // 4 * 4 - 1, ncols, -items * K][(i + 2 * j) % 5]       # the last two: no diagonal at all
            cases.append((f"K{K}-items{items}-ncols{ncols}-off{off}", GC(items, K, ncols, diag_off=off)))
    for K in (8, 22):
        for ncols in GRAD_NCOLS:
            cases.append((f"K{K}-items17-ncols{ncols}-tight", GC(17, K, ncols, ld=(ncols + 7) // 8 * 8, ldT=(17 * K + 7) // 8 * 8, diag_off=8)))
    return cases


def pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


def grad_data(a, recipe, softplus, seed=0):
    """-> S flat [items K][ld] (f32-exact float64, NaN in the pad columns), lse [round4(ncols)] and the scalars to pass (the grad-exact twin replaces reg,
    n_rows_total and n_items_total by powers of two)."""
    items, K, ncols, ld = a["items"], a["K"], a["ncols"], a["ld"]
    R = items * K
    g = gen(seed + items * 5 + K * 3 + ncols + len(recipe) + softplus)
    a = dict(a)
    if recipe == "grad-exact":
        assert not softplus
        if pow2(K):
            s = ints(g, -8, 8, R, ncols)
        else:                                          # K not a power of two: every item's column sums to zero (m = 0 exactly), any other grouping of rows does not
            u = ints(g, 1, 8, items, 1, ncols) * (1 - 2 * torch.randint(0, 2, (items, 1, ncols), generator=g).double())
            s = (u * (1 - 2 * (torch.arange(K) % 2).double())[None, :, None]).reshape(R, ncols)
        n_rows, n_items = 1024.0, 64.0
        a.update(n_rows_total=n_rows, n_items_total=n_items, reg=n_items * n_items * K ** 3 / (2.0 * n_rows) if pow2(K) else 0.5)
        lse = torch.full((ncols,), 200.0, dtype=F64)
        if pow2(K):                                    # columns 1, 5, 9, ...: weight exactly 1 (s == lse == 8) but for one row per item (s = -120: weight 0)
            s[:, 1::4], lse[1::4] = 8.0, 8.0
            s[torch.arange(items) * K + torch.randint(0, K, (items,), generator=g), 1::4] = -120.0
    else:
        s = normal(g, R, ncols).double() * (1.0 if recipe == "narrow" else 30.0)
        if recipe == "wide":
            s = s.clamp(-100, 100)
            r = torch.arange(0, R, 7)
            c = r + a["diag_off"]
            ok = (c >= 0) & (c < ncols)
            s[r[ok], c[ok]] = 25.0 + 3.0 * torch.rand(int(ok.sum()), generator=g).double()       # own-target scores above the threshold
        s = rounded(s, F32)
        sp = score_tf(s, softplus)
        lse = torch.logsumexp(sp, 0) + math.log(a["n_rows_total"] / R)                           # (the other strips: as many rows again)
    S = torch.full((R, ld), NAN, dtype=F64)
    S[:, :ncols] = rounded(s, F32)
    return S.reshape(-1), rounded(lse, F32), a
