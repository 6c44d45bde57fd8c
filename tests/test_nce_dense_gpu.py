"""The dense InfoNCE loss chain against float64: cpc_nce_loss (equal-step scores), cpc_nce_loss_all (all timesteps), the NaN guard of
both and of cpc_nce_loss_sampled, their refusals, cpc_gp_score_coeff and cpc_adam_dev.  Every launch runs on buffers with a sentinel
tail (the workspace included, sized by cpc_nce_workspace_floats / cpc_nce_all_workspace_floats), NaN-prefilled outputs and junk in the
input pad columns; the input is compared bit for bit afterwards.  References: oracle.cpc_oracle.info_nce_loss + autograd, the
components from its _loss_terms.

Which shape reaches which loop or specialisation of csrc/nce.hip (a change of a tile or cap constant moves the shape with it):

cpc_nce_loss, (B, K)
  (257, 16)  second trip of nce_col_body's row loop with NCE_CW = 8 (one trip covers 8 x 32 = 256 rows); nce_col_mean_kernel<16>;
             ld = B + 7 = 264, the largest legal row pad; 9 x 9 gradient tiles whose edge tile is one row / column wide;
             K ceil(B / 8) = 528 column partials and ceil(B^2 / 256) = 259 pair partials: second trip of both `i += 256` loops of
             nce_finalize_body
  (256, 12)  the workload shape; nce_col_mean_kernel<12>; ld = B, no pad column
  (65, 5)    run-time K (nce_col_mean_kernel<0>); three tiles per side, the last one wide
  (2, 16)    the smallest batch with <16>
  (1, 3)     one item: the loss is the regulariser alone
  (8, 1)     one prediction step
cpc_nce_loss_all, (B, K), R = B K
  (9, 12)    R = 108: unsplit column pass (R < 8 NCE_ALL_SPLITS = 128) and second trip of the row loop with 32 columns per workgroup
             (one trip covers 8 x 8 = 64 rows); nce_all_grad_kernel<T, *, 12>
  (5, 16)    R = 80: unsplit, second row trip, nce_all_grad_kernel<T, *, 16>; ld = R + 5 (odd)
  (8, 16)    R = 128: the smallest split size, 16 splits of 8 rows
  (10, 13)   R = 130: rows per split = roundup8(ceil(130 / 16)) = 16, so splits 9..15 are empty and hand (-inf, 0) to
             nce_col_merge_kernel; run-time K
  (888, 1)   B R = 788 544 > NCE_ALL_BLOCKS x 256 = 786 432: second trip of the grid-stride loop of nce_all_grad_kernel<T, *, 0>
  (257, 12)  R = 3084: second (to fourth) trip of the <12> gradient kernel; one dtype and score function
neighbours
  cpc_gp_score_coeff (1, 520, 520): 270 400 elements > 1024 blocks x 256: second grid-stride trip; (3, 5, 7): rows != cols
  cpc_adam_dev n = 4 x 2048 x 256 + 7: second trip of the float4 loop of the grid capped at 2048 blocks (n / 4 > 2048 x 256) and a
             three-element scalar tail; cpc_adam beside it runs the same kernel
  cpc_nce_eval's loops: the (70, 2) and (257, 1) cases of tests/test_audio_kernels_gpu.py::test_nce_eval_against_oracle

Bounds: the ones tests/test_hip_kernels.py carries for these kernels (test_nce_loss, test_adam_matches_torch): loss 2e-5 relative,
max score 1e-5 relative, gradients max-norm relative error 2e-5 (f32) / 1e-2 (bf16), Adam 2e-6 absolute."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cpc_audio_amd import _hip
from cpc_audio_amd.sampled_negatives import sampled_negative_mask
from oracle import cpc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U64 = C.c_ulonglong
SENTINEL = -8192.0          # exact in f32 and bf16
TAIL = 64
NAN, INF = float("nan"), float("inf")
DTYPES = [torch.float32, torch.bfloat16]
NEXT20 = float(np.nextafter(np.float32(20.0), np.float32(np.inf)))          # the first float beyond softplus's threshold


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _guarded(shape, fill, dtype=torch.float32):
    """A device buffer of ``shape`` holding ``fill`` (a number or a tensor) with TAIL sentinel elements behind it: (view, whole)."""
    n = int(np.prod(shape))
    whole = torch.full((n + TAIL,), SENTINEL, device=DEV, dtype=dtype)
    whole[:n] = fill.to(DEV).reshape(-1) if torch.is_tensor(fill) else fill
    return whole[:n].view(*shape), whole


def _tails_intact(*wholes):
    return all(bool((w[-TAIL:] == SENTINEL).all()) for w in wholes)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------ float64 references
def _embed(sp):
    """[k][b][b'] equal-step scores as the 4-D tensor [b][k][b'][k'] the oracle takes (zero where k != k': unused in that branch)."""
    return torch.diag_embed(sp.permute(1, 2, 0), dim1=1, dim2=3)


def _oracle(kind, S, B, K, softplus, reg, mask=None):
    """oracle.info_nce_loss + autograd on the f32 scores S ([K][B][B] for "equal" / "sampled", [R][R] for "all") in float64.  ``mask``
    [K][b][b']: the candidate sets of the sampled loss (the masked restatement below; info_nce_loss has no such argument)."""
    lin = S.double().requires_grad_(True)
    sp = F.softplus(lin) if softplus else lin
    if mask is None:
        all_t = kind == "all"
        sc4 = sp.view(B, K, B, K) if all_t else _embed(sp)
        loss, smax = O.info_nce_loss(sc4, all_timesteps=all_t, regularization=reg)
        s, noise, valid = O._loss_terms(sc4, all_t)
        t_valid, t_lse, t_reg = -valid.mean(), noise.mean(), reg * torch.mean(torch.mean(s, dim=1) ** 2)
    else:
        t_valid = -torch.diagonal(sp, dim1=1, dim2=2).mean()
        t_lse = torch.logsumexp(sp.masked_fill(~mask, -INF), dim=1).mean()
        t_reg = reg * (sp.mean(dim=0) ** 2).mean()
        loss, smax = t_valid + t_lse + t_reg, sp.max()
    if bool(torch.isfinite(loss)):
        loss.backward()
    return dict(loss=loss.item(), smax=smax.item(), t_valid=t_valid.item(), t_lse=t_lse.item(), t_reg=t_reg.item(), grad=lin.grad,
                pre_reg=(t_valid + t_lse).item())


def _plain_scores(kind, B, K):
    g = torch.Generator().manual_seed(B * 3 + K + (1000 if kind == "all" else 0))
    S = torch.randn((B * K, B * K) if kind == "all" else (K, B, B), generator=g) * 3.0
    S.view(-1)[0] = 25.0                                  # beyond the softplus threshold, on the diagonal
    return S


def _magnitude_scores(B, K):
    """randn * 10 with the softplus threshold from both sides, a large, a very negative and a zero score in different columns, on
    and off the diagonal."""
    S = torch.randn(K, B, B, generator=torch.Generator().manual_seed(77)) * 10.0
    for k, b, bp, v in [(0, 3, 3, 20.0), (0, 7, 50, 20.0), (1, 10, 4, NEXT20), (1, 11, 11, NEXT20), (2, 64, 64, 25.0), (2, 64, 0, 25.0),
                        (3, 5, 40, -100.0), (3, 41, 41, -100.0), (4, 33, 33, 0.0), (4, 0, 64, 0.0)]:
        S[k, b, bp] = v
    return S


@functools.lru_cache(maxsize=None)
def _case(kind, B, K, softplus, reg, scores="plain"):
    """(scores, reference) of a case, computed once and shared by the storage types; nothing writes to either."""
    S = _plain_scores(kind, B, K) if scores == "plain" else _magnitude_scores(B, K)
    return S, _oracle(kind, S, B, K, softplus, reg)


# ------------------------------------------------------------------------------------------ launches
def _launch(kind, S, B, K, ld, reg, softplus, dt, out=None, sampled=None, check_pads=True):
    """One guarded launch of cpc_nce_loss ("equal"), cpc_nce_loss_sampled ("sampled", sampled = (N, seed, draw)) on S [K][B][B] or of
    cpc_nce_loss_all ("all") on S [R][R] and its transpose.  Returns (out, dS, dST) on the host, the pad columns cut off."""
    code = _hip.dtype_code(dt)
    P = _hip.ptr
    if kind == "all":
        R = B * K
        shape, n = (R, ld), R
        ins = [S, S.T]
        nws = int(_hip.lib().cpc_nce_all_workspace_floats(B, K))
    else:
        shape, n = (K, B, ld), B
        ins = [S]
        nws = int(_hip.lib().cpc_nce_sampled_workspace_floats(B, K) if kind == "sampled" else _hip.lib().cpc_nce_workspace_floats(B, K))
    padded, dev_in = [], []
    for x in ins:
        p = torch.full(shape, 7.0)                      # pad columns hold junk the kernels must ignore
        p[..., :n] = x
        padded.append(p)
        dev_in.append(_guarded(shape, p))
    grads = []
    for _ in range(2):
        # cpc_nce_loss(_sampled) writes zeros into the pad columns; cpc_nce_loss_all never writes there and the engines, which run
        # GEMMs over all ld columns of dS, zero them once when they allocate: here they start as zeros and must still be zeros
        fill = torch.full(shape, NAN)
        if kind == "all":
            fill[..., n:] = 0.0
        grads.append(_guarded(shape, fill, dt))
    if out is None:
        out = _guarded((8,), NAN)
    ws = _guarded((nws,), NAN)
    (dS, dS_w), (dST, dST_w) = grads
    if kind == "all":
        _hip.call("cpc_nce_loss_all", P(dev_in[0][0]), P(dev_in[1][0]), P(dS), P(dST), P(out[0]), P(ws[0]), B, K, ld, softplus,
                  C.c_float(reg), code)
    elif kind == "sampled":
        N, seed, draw = sampled
        _hip.call("cpc_nce_loss_sampled", P(dev_in[0][0]), P(dS), P(dST), P(out[0]), P(ws[0]), B, K, ld, softplus, C.c_float(reg), N,
                  U64(seed), U64(draw), code)
    else:
        _hip.call("cpc_nce_loss", P(dev_in[0][0]), P(dS), P(dST), P(out[0]), P(ws[0]), B, K, ld, softplus, C.c_float(reg), code)
    torch.cuda.synchronize()
    assert _tails_intact(dS_w, dST_w, out[1], ws[1], *(w for _, w in dev_in))
    for (d, _), p in zip(dev_in, padded):
        assert _same_bits(d.cpu(), p), "the input changed"
    if check_pads:
        assert bool((dS[..., n:] == 0).all()) and bool((dST[..., n:] == 0).all())
    return out[0].cpu(), dS[..., :n].cpu(), dST[..., :n].cpu()


def _check(kind, B, K, ld, reg, softplus, dt, scores="plain"):
    S, ref = _case(kind, B, K, softplus, reg, scores)
    out, dS, dST = _launch(kind, S, B, K, ld, reg, softplus, dt)
    gT = ref["grad"].T if kind == "all" else ref["grad"].transpose(1, 2)
    e_s, e_t = _rel(dS, ref["grad"]), _rel(dST, gT)
    print(f"{kind} B={B} K={K} ld={ld} reg={reg} softplus={softplus} {dt}: out {out.tolist()}")
    print(f"   oracle loss {ref['loss']:.9g} max {ref['smax']:.9g} terms {ref['t_valid']:.9g} {ref['t_lse']:.9g} {ref['t_reg']:.9g};"
          f" dS rel {e_s:.3e}, dST rel {e_t:.3e}")
    assert abs(out[0].item() - ref["loss"]) < 2e-5 * max(1.0, abs(ref["loss"]))
    assert abs(out[1].item() - ref["smax"]) < 1e-5 * max(1.0, abs(ref["smax"]))
    for i, name in ((2, "t_valid"), (3, "t_lse"), (4, "t_reg")):
        assert abs(out[i].item() - ref[name]) < 2e-5 * max(1.0, abs(ref[name])), name
    assert out[5].item() == 0.0
    assert math.isnan(out[6].item()) and math.isnan(out[7].item())          # the sticky flag is only ever raised, out[7] is not ours
    t = 2e-5 if dt == torch.float32 else 1e-2
    assert e_s < t
    assert e_t < t


@pytest.mark.parametrize("kind,B,K", [("equal", 6, 4), ("all", 6, 4), ("equal", 1, 3), ("all", 3, 1)])
@pytest.mark.parametrize("softplus", [0, 1])
def test_reference_is_the_oracle(kind, B, K, softplus):
    """What _oracle adds to oracle.info_nce_loss — the 4-D embedding of the equal-step scores, the three components and the masked
    variant — against the oracle itself on the tensor tests/test_hip_kernels.py::test_nce_loss builds (no GPU work)."""
    reg = 0.7
    S = _plain_scores(kind, B, K)
    ref = _oracle(kind, S, B, K, softplus, reg)
    lin = S.double().requires_grad_(True)
    if kind == "all":
        full = lin.view(B, K, B, K)
    else:
        full = torch.zeros(B, K, B, K, dtype=torch.float64)
        for k in range(K):
            full[:, k, :, k] = lin[k]
        assert torch.equal(_embed(S.double()), full.detach())
    sc = F.softplus(full) if softplus else full
    loss, smax = O.info_nce_loss(sc, all_timesteps=kind == "all", regularization=reg)
    loss.backward()
    assert ref["loss"] == loss.item() and ref["smax"] == smax.item()
    assert _rel(ref["grad"], lin.grad) < 1e-14          # (softplus in front of the embedding or behind it: other roundings in autograd)
    assert abs(ref["t_valid"] + ref["t_lse"] + ref["t_reg"] - loss.item()) < 1e-13 * max(1.0, abs(loss.item()))
    assert ref["pre_reg"] == ref["t_valid"] + ref["t_lse"]
    if kind == "equal":          # every row a candidate: the masked restatement is the dense loss
        m = _oracle("sampled", S, B, K, softplus, reg, mask=torch.ones(K, B, B, dtype=torch.bool))
        for name in ("loss", "t_valid", "t_lse", "t_reg"):
            assert abs(m[name] - ref[name]) < 1e-13 * max(1.0, abs(ref[name])), name
        assert m["smax"] == ref["smax"]
        if ref["grad"].abs().max() > 0:
            assert _rel(m["grad"], ref["grad"]) < 1e-13


# ------------------------------------------------------------------------------------------ a. cpc_nce_loss
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,reg", [(257, 16, 257 / 4), (256, 12, 64.0), (65, 5, 0.5), (2, 16, 0.0), (1, 3, 0.5), (8, 1, 0.0)])
def test_nce_loss_against_float64(dt, softplus, B, K, reg):
    """reg = B / 4 at B >= 256: the regulariser's share of the gradient is then of the order of the softmax term; with reg <= 1 it is
    about 1 % of the largest entry and invisible in bf16."""
    _check("equal", B, K, (B + 7) // 8 * 8, reg, softplus, dt)


# ------------------------------------------------------------------------------------------ b. magnitudes
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("softplus", [0, 1])
def test_nce_loss_magnitudes(dt, softplus):
    """Scores randn * 10 with 20.0, nextafter(20, inf), 25, -100 and 0 planted on and off the diagonal."""
    S = _magnitude_scores(65, 5)
    assert S[0, 3, 3].item() == 20.0 and S[1, 10, 4].item() > 20.0 and S[1, 10, 4].item() - 20.0 < 2e-6
    _check("equal", 65, 5, 72, 0.5, softplus, dt, scores="magnitudes")


# ------------------------------------------------------------------------------------------ c. cpc_nce_loss_all
ALL_SHAPES = [(9, 12, 112, 0.5), (5, 16, 85, 1.0), (8, 16, 128, 0.01), (10, 13, 136, 0.5), (888, 1, 888, 0.5)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,ld,reg", ALL_SHAPES)
def test_nce_loss_all_against_float64(dt, softplus, B, K, ld, reg):
    _check("all", B, K, ld, reg, softplus, dt)


def test_nce_loss_all_second_trip_of_the_k12_gradient_kernel():
    """(257, 12): 257 x 3084 pairs on 3072 x 256 threads; bf16 storage, softplus scores (38 MB of scores)."""
    _check("all", 257, 12, 3088, 257 / 4, 1, torch.bfloat16)


# ------------------------------------------------------------------------------------------ d. NaN guard
GUARD = [("equal", 33, 3), ("all", 33, 3), ("all", 10, 13), ("sampled", 33, 3)]
SAMPLED = (7, 1234, 5)          # (N, seed, draw) of the sampled cases


def _guard_setup(kind, B, K):
    ld = (B * K + 7) // 8 * 8 if kind == "all" else (B + 7) // 8 * 8
    S = _plain_scores(kind, B, K)
    mask = sampled_negative_mask(B, K, *SAMPLED) if kind == "sampled" else None
    return ld, S, mask, (SAMPLED if kind == "sampled" else None)


@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("kind,B,K", GUARD)
def test_nan_score_raises_both_flags_and_the_sticky_one_stays(kind, B, K, softplus):
    """A NaN at the last (k, b, b') sets out[5] and out[6]; a clean call into the same out gives out[5] = 0, out[6] still 1 and the
    oracle's loss; cpc_adam and cpc_adam_dev with skip = out + 6 then change nothing."""
    reg = 0.5
    ld, S, mask, smp = _guard_setup(kind, B, K)
    bad = S.clone()
    bad.view(-1)[-1] = NAN
    ref_bad = _oracle(kind, bad, B, K, softplus, reg, mask)
    assert math.isnan(ref_bad["pre_reg"])
    out = _guarded((8,), 0.0)          # the caller zeroes the sticky flag when a run starts
    got, _, _ = _launch(kind, bad, B, K, ld, reg, softplus, torch.float32, out=out, sampled=smp, check_pads=False)
    assert got[5].item() == 1.0 and got[6].item() == 1.0
    assert math.isnan(got[0].item())
    ref = _oracle(kind, S, B, K, softplus, reg, mask)
    got, _, _ = _launch(kind, S, B, K, ld, reg, softplus, torch.float32, out=out, sampled=smp)
    assert got[5].item() == 0.0 and got[6].item() == 1.0 and got[7].item() == 0.0
    assert abs(got[0].item() - ref["loss"]) < 2e-5 * max(1.0, abs(ref["loss"]))
    # the optimizer behind the raised flag
    n = 1003
    g = torch.Generator().manual_seed(3)
    bufs = [_guarded((n,), torch.randn(n, generator=g)) for _ in range(3)] + [_guarded((n,), torch.rand(n, generator=g))]
    state = _guarded((4,), 0.0)
    before = [w.clone() for _, w in bufs + [state]]
    (p, _), (gr, _), (m, _), (v, _) = bufs
    tail = (C.c_longlong(n), C.c_float(1e-3), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8))
    _hip.call("cpc_adam", _hip.ptr(p), _hip.ptr(gr), _hip.ptr(m), _hip.ptr(v), *tail, 1, C.c_float(1.0), _hip.ptr(out[0], 6))
    _hip.call("cpc_adam_dev", _hip.ptr(p), _hip.ptr(gr), _hip.ptr(m), _hip.ptr(v), *tail, _hip.ptr(state[0]), C.c_float(1.0),
              _hip.ptr(out[0], 6))
    torch.cuda.synchronize()
    for (_, w), b in zip(bufs + [state], before):
        assert _same_bits(w, b)


@pytest.mark.parametrize("where", ["diagonal", "off_diagonal"])
@pytest.mark.parametrize("kind,B,K", GUARD)
def test_flag_follows_the_oracle_for_an_infinite_linear_score(kind, B, K, where):
    """Linear scores with one +inf.  On the diagonal the loss before the regulariser is inf - inf = NaN in the oracle too: flag raised.
    Off the diagonal (in a column's candidate set) the oracle's loss is +inf and not NaN: the flag stays 0 and out[0] is +inf."""
    reg = 0.5
    ld, S, mask, smp = _guard_setup(kind, B, K)
    S = S.clone()
    if kind == "all":
        r, c = B * K - 1, (B * K - 1 if where == "diagonal" else 2)
        S[r, c] = INF
    else:
        bp = B - 1
        rows = [b for b in range(B) if b != bp and (mask is None or bool(mask[K - 1, b, bp]))]
        S[K - 1, bp if where == "diagonal" else rows[-1], bp] = INF
    ref = _oracle(kind, S, B, K, 0, reg, mask)
    assert math.isnan(ref["pre_reg"]) if where == "diagonal" else ref["pre_reg"] == INF
    out = _guarded((8,), 0.0)
    got, _, _ = _launch(kind, S, B, K, ld, reg, 0, torch.float32, out=out, sampled=smp, check_pads=False)
    print(f"{kind} {where}: out {got.tolist()}, oracle loss before the regulariser {ref['pre_reg']}")
    flag = 1.0 if math.isnan(ref["pre_reg"]) else 0.0
    assert got[5].item() == flag and got[6].item() == flag
    if where == "off_diagonal":
        assert got[0].item() == INF and ref["loss"] == INF


# ------------------------------------------------------------------------------------------ e. refusals
_COMMON = ["B0", "K0", "ld_small", "dtype", "null_S", "null_dS", "null_dST", "null_out", "null_ws"]
# (ld > B + 7 is a limit of cpc_nce_loss alone; only cpc_nce_loss_all takes the transposed scores)
REFUSALS = [("equal", c) for c in _COMMON + ["ld_big"]] + [("all", c) for c in _COMMON + ["null_ST"]]


@pytest.mark.parametrize("kind,case", REFUSALS)
def test_refused_calls_leave_every_buffer_alone(kind, case):
    """HipCallError, and every buffer — the workspace included — byte-identical afterwards: a refused call launches nothing."""
    B, K = 8, 2
    all_t = kind == "all"
    n = B * K if all_t else B
    ld = n
    rows = B * K
    g = torch.Generator().manual_seed(11)
    nws = int(_hip.lib().cpc_nce_all_workspace_floats(B, K) if all_t else _hip.lib().cpc_nce_workspace_floats(B, K))
    # (rows of n + 8 floats: room for the largest ld passed below)
    bufs = {name: _guarded((rows, n + 8), torch.randn(rows, n + 8, generator=g)) for name in ("S", "ST", "dS", "dST")}
    bufs["out"] = _guarded((8,), torch.randn(8, generator=g))
    bufs["ws"] = _guarded((nws,), torch.randn(nws, generator=g))
    before = {k: w.clone() for k, (_, w) in bufs.items()}
    a = {k: _hip.ptr(v) for k, (v, _) in bufs.items()}
    code = _hip.F32
    if case == "B0":
        B = 0
    elif case == "K0":
        K = 0
    elif case == "ld_small":
        ld = n - 1
    elif case == "ld_big":
        ld = n + 8
    elif case == "dtype":
        code = 2
    else:
        a[case[len("null_"):]] = None
    with pytest.raises(_hip.HipCallError):
        if all_t:
            _hip.call("cpc_nce_loss_all", a["S"], a["ST"], a["dS"], a["dST"], a["out"], a["ws"], B, K, ld, 1, C.c_float(0.5), code)
        else:
            _hip.call("cpc_nce_loss", a["S"], a["dS"], a["dST"], a["out"], a["ws"], B, K, ld, 1, C.c_float(0.5), code)
    torch.cuda.synchronize()
    for name, (_, w) in bufs.items():
        assert _same_bits(w, before[name]), name


# ------------------------------------------------------------------------------------------ f. cpc_gp_score_coeff
def _coeff_inputs(nmat, rows, cols, ld):
    g = torch.Generator().manual_seed(rows * 7 + cols)
    S = torch.randn(nmat, rows, ld, generator=g) * 4.0
    flat = S[:, :, :cols]
    for i, v in enumerate([20.0, NEXT20, 25.0, -30.0]):          # different rows and columns of the last matrix
        flat[nmat - 1, (i * 2) % rows, (i * 3 + 1) % cols] = v
    S[:, :, cols:] = 1e4
    St1, St2 = torch.randn(nmat, rows, ld, generator=g), torch.randn(nmat, rows, ld, generator=g)
    return S, St1, St2


@pytest.mark.parametrize("mode,with_st2", [(0, False), (1, True), (1, False)])
@pytest.mark.parametrize("nmat,rows,cols,ld,ldT", [(3, 5, 7, 8, 8), (1, 520, 520, 520, 520)])
def test_gp_score_coeff_against_float64(nmat, rows, cols, ld, ldT, mode, with_st2):
    """mode 0: autograd of F.softplus on the f32 scores, in float64.  mode 1: sigmoid(s) (1 - sigmoid(s)) (St1 + St2) up to the
    threshold 20 and 0 beyond it.  WT is bitwise the transpose of W; the pad columns of both are never written (the engines rely on
    it)."""
    S, St1, St2 = _coeff_inputs(nmat, rows, cols, ld)
    x = S[:, :, :cols].double().requires_grad_(True)
    if mode == 0:
        F.softplus(x).sum().backward()
        ref = x.grad
    else:
        t = St1[:, :, :cols].double() + (St2[:, :, :cols].double() if with_st2 else 0.0)
        sg = torch.sigmoid(x.detach())
        ref = torch.where(x.detach() > 20.0, torch.zeros_like(sg), sg * (1 - sg) * t)
    ins = [_guarded(s.shape, s) for s in (S, St1, St2)]
    W, W_w = _guarded((nmat, rows, ld), NAN)
    WT, WT_w = _guarded((nmat, cols, ldT), NAN)
    P = _hip.ptr
    _hip.call("cpc_gp_score_coeff", P(ins[0][0]), P(ins[1][0]) if mode else None, P(ins[2][0]) if with_st2 else None, P(W), P(WT), nmat,
              rows, cols, ld, ldT, mode)
    torch.cuda.synchronize()
    assert _tails_intact(W_w, WT_w, *(w for _, w in ins))
    for (d, _), s in zip(ins, (S, St1, St2)):
        assert _same_bits(d.cpu(), s)
    got = W[:, :, :cols].cpu()
    print(f"gp_score_coeff {nmat}x{rows}x{cols} mode {mode} St2 {with_st2}: rel {_rel(got, ref):.3e}")
    assert not torch.isnan(got).any()
    assert _rel(got, ref) < 2e-5
    if mode == 0:          # beyond the threshold the derivative is exactly 1
        assert bool((got[S[:, :, :cols] > 20.0] == 1.0).all()) and int((S[:, :, :cols] > 20.0).sum()) >= 2
    else:
        assert bool((got[S[:, :, :cols] > 20.0] == 0.0).all())
    assert _same_bits(WT[:, :, :rows].cpu(), got.transpose(1, 2))
    assert bool(torch.isnan(W[:, :, cols:]).all()) and bool(torch.isnan(WT[:, :, rows:]).all())


def test_gp_score_coeff_refusals():
    nmat, rows, cols, ld, ldT = 3, 5, 7, 8, 8
    S, St1, St2 = _coeff_inputs(nmat, rows, cols, ld)
    ins = [_guarded(s.shape, s) for s in (S, St1, St2)]
    outs = [_guarded((nmat, rows, ld), 3.0), _guarded((nmat, cols, ldT), 3.0)]
    before = [w.clone() for _, w in ins + outs]
    P = _hip.ptr
    s, t1, t2, w, wt = (P(v) for v, _ in ins + outs)
    for args in [(s, t1, t2, w, wt, nmat, rows, cols, ld, ldT, 2),           # mode 2
                 (s, None, t2, w, wt, nmat, rows, cols, ld, ldT, 1),         # mode 1 without St1
                 (s, t1, t2, w, wt, nmat, rows, cols, cols - 1, ldT, 0),     # ld < cols
                 (s, t1, t2, w, wt, nmat, rows, cols, ld, rows - 1, 0),      # ldT < rows
                 (None, t1, t2, w, wt, nmat, rows, cols, ld, ldT, 0), (s, t1, t2, None, wt, nmat, rows, cols, ld, ldT, 0),
                 (s, t1, t2, w, None, nmat, rows, cols, ld, ldT, 0)]:
        with pytest.raises(_hip.HipCallError):
            _hip.call("cpc_gp_score_coeff", *args)
    torch.cuda.synchronize()
    for (_, wh), b in zip(ins + outs, before):
        assert _same_bits(wh, b)


# ------------------------------------------------------------------------------------------ g. cpc_adam_dev
def test_adam_dev_three_steps_against_float64():
    """Three cpc_adam_dev steps from a zeroed state next to three cpc_adam calls with step = 1, 2, 3, both against
    oracle.adam_update in float64 on the values the kernels receive (lr and the betas as f32).  state[0] holds the step count as int
    bits; state[1] = lr / (1 - b1^t) and state[2] = 1 / sqrt(1 - b2^t) are one float rounding of a double result: 2^-23 relative."""
    n = 4 * 2048 * 256 + 7
    g = torch.Generator().manual_seed(0)
    lr, b1, b2, eps = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))
    p0 = torch.randn(n, generator=g)
    ref = [p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
    dev_side = [[_guarded((n,), p0), _guarded((n,), 0.0), _guarded((n,), 0.0)] for _ in range(2)]          # cpc_adam_dev, cpc_adam
    state, state_w = _guarded((4,), 0.0)
    P = _hip.ptr
    consts = (C.c_longlong(n), C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps))
    for t in range(1, 4):
        grad = torch.randn(n, generator=g)
        O.adam_update(ref[0], grad.double(), ref[1], ref[2], t, lr, beta1=b1, beta2=b2, eps=eps)
        dg, dg_w = _guarded((n,), grad * 2.0)           # the kernels multiply by grad_scale = 0.5 first (exact)
        (p, _), (m, _), (v, _) = dev_side[0]
        _hip.call("cpc_adam_dev", P(p), P(dg), P(m), P(v), *consts, P(state), C.c_float(0.5), None)
        (p, _), (m, _), (v, _) = dev_side[1]
        _hip.call("cpc_adam", P(p), P(dg), P(m), P(v), *consts, t, C.c_float(0.5), None)
        torch.cuda.synchronize()
        st = state.cpu()
        assert st.view(torch.int32)[0].item() == t and st[3].item() == 0.0
        want1, want2 = float(np.float32(lr / (1.0 - b1 ** t))), float(np.float32(1.0 / math.sqrt(1.0 - b2 ** t)))
        assert abs(st[1].item() - want1) <= 2.0 ** -23 * want1, (t, st[1].item(), want1)
        assert abs(st[2].item() - want2) <= 2.0 ** -23 * want2, (t, st[2].item(), want2)
        assert _same_bits(dg.cpu(), grad * 2.0) and _tails_intact(dg_w, state_w)
        for name, side in zip(("cpc_adam_dev", "cpc_adam"), dev_side):
            assert _tails_intact(*(w for _, w in side))
            errs = [(x.double().cpu() - r).abs().max().item() for (x, _), r in zip(side, ref)]
            print(f"{name} step {t}: max |p|, |m|, |v| errors {errs}")
            assert max(errs) < 2e-6, (name, t, errs)
