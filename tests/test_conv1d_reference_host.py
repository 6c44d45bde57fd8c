"""The references of tests/conv1d_reference.py judged on the host, at every case test_conv1d_kernels_gpu.py runs:

  * each reference (explicit index arithmetic) equals float64 F.conv1d / autograd to 1e-12, the w_dgrad layout equals the data
    gradient it has to produce, the reduce permutation equals a plain loop;
  * a float32 host emulation (the same functions on float32 tensors, inputs rounded to the storage type) stays within HALF the
    bound.  With bf16 storage the half applies to the float32 value BEFORE it is rounded to bf16, against the bound without its
    u_out term (a smaller bound): one correct rounding to bf16 uses up to the whole u_out |ref| term on its own (|round(v) - v|
    reaches 2^-8 |v| for v just above a power of two), so no correctly rounded output can stay within half of a bound whose
    rounding term is exactly that; the stored bf16 value is asserted to be within the full bound (which follows: 2^-8 |ref| +
    (1 + 2^-8) 0.5 accumulation term).  With f32 storage the stored value is the float32 value;
  * the metric rejects every deliberate mistake wherever it is expressible (each a transformation of the reference's output or
    layout): a tap shifted by one, stride off by one, kernel flipped, two channels swapped, one pad row not zeroed, the tap >= kw
    entries of w_dgrad filled from tap kw - 1, the dd order of w_dgrad reversed, one slab dropped, s_hi and s_lo exchanged, the
    bias row of the layer-1 slab at row KA = 16 instead of kw;
  * the exact-data twins keep S = sum |a||b| (+ |bias|) <= 256, so every partial sum in any order is an integer the formats hold.

Each test prints the largest emulation ratio of its group (run with -s); the figures are quoted in test_conv1d_kernels_gpu.py.
"""
import collections

import torch
import torch.nn.functional as F

import conv1d_reference as R

DTYPES = [R.F32, R.BF16]


def close(a, b, what):
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= 1e-12 * max(1.0, b.abs().max().item() if b.numel() else 1.0), f"{what}: {err:.2e}"


def emulate(fn, dt, tensors, ref, S, n, what, **kw):
    """fn on float32 copies of tensors -> (ratio of the f32 value against the bound without u_out, ratio of the stored value)."""
    y32 = fn(*[None if t is None else t.float() for t in tensors], **kw)
    pre = R.bound_ratio(y32, ref, S, n, 0.0)
    stored = R.bound_ratio(y32.to(dt), ref, S, n, R.u_out(dt))
    assert pre <= 0.5, f"{what} {R.name(dt)}: float32 emulation at {pre:.3f} of the bound"
    assert stored <= (0.5 if dt == R.F32 else 1.0), f"{what} {R.name(dt)}: stored emulation at {stored:.3f} of the bound"
    return pre, stored


MISTAKES = ["tap shifted", "stride off by one", "kernel flipped", "channels swapped", "columns swapped", "pad row not zeroed",
            "zero taps filled", "dd reversed", "slab dropped", "row dropped", "s_hi and s_lo exchanged", "bias row at KA"]
REJECTED = collections.Counter()


def rejected(mut, ref, S, n, dt, what):
    r = R.bound_ratio(mut, ref, S, n, R.u_out(dt))
    REJECTED[next(m for m in MISTAKES if m in what)] += 1
    assert r > 1.0, f"{what} {R.name(dt)}: the metric accepts the mistake (ratio {r:.3f})"


def test_case_lists_cover_every_axis_value_per_lane_layout():
    fwd, bwd = R.c1_fwd_cases(), R.c1_bwd_cases()
    assert {c[:3] for c in fwd} == set(R.C1_SHAPES) == {c[:3] for c in bwd}
    for C in {s[0] for s in R.C1_SHAPES}:
        mine = [c for c in fwd if c[0] == C]
        assert {c[3] for c in mine} == set(R.C1_FWD_LV) and {c[4] for c in mine} == set(R.C1_FWD_PAD)
        assert {c[5] for c in mine} == {0, 1} == {c[6] for c in mine} and {c[7] for c in mine} == {0, 7}
        mine = [c for c in bwd if c[0] == C]
        assert {c[4] for c in mine} == set(R.C1_BWD_LV) and {c[3] for c in mine} == {3, 5}
        kinds_t = {"one" if c[5] == 1 else "three" if c[5] == 3 else "more" for c in mine if not (c[5] == 3 and -(-c[4] // 64) + 2 == 3)}
        assert kinds_t == {"one", "three", "more"}, (C, kinds_t)
        assert any(c[6] == 1 for c in mine) and any(c[6] == 2 for c in mine) and any(c[6] == c[3] for c in mine)
        assert any(c[3] % c[6] for c in mine), "no case with B not a multiple of nblk_b"
    assert any(c[4] >= 256 for c in fwd)                                      # a workgroup of pad rows only
    assert any(c[5] > -(-c[4] // 64) for c in bwd)                            # more time blocks than 64-position chunks


# ====================================================================================================================== layer 1
def _c1_fwd_torch(x, w, bias, stride, L_valid, L_alloc, relu):
    y = F.conv1d(x[:, None, :], w[:, None, :], bias, stride=stride)[:, :, :L_valid].permute(0, 2, 1)
    y = y.clamp_min(0) if relu else y
    return F.pad(y, (0, 0, 0, L_alloc - L_valid))


def test_layer1_forward_reference_emulation_and_mistakes():
    REJECTED.clear()
    worst = {dt: 0.0 for dt in DTYPES}
    for case in R.c1_fwd_cases():
        C, kw, s, Lv, pad, relu, hb, slack = case
        cid, La = R.c1_fwd_id(case), Lv + pad
        for dt in DTYPES:
            for exact in (False, True):
                x, x_dev, w, bias, ldx = R.c1_fwd_data(case, dt, exact)
                assert ldx == (Lv - 1) * s + kw + slack and bool(torch.isnan(x_dev[:, x.shape[1]:]).all())
                args = dict(stride=s, L_valid=Lv, L_alloc=La, relu=relu)
                ref = R.conv1_fwd(x, w, bias, **args)
                S = R.abs_bound_terms(R.conv1_fwd, x, w, bias, stride=s, L_valid=Lv, L_alloc=La, relu=0)
                close(ref, _c1_fwd_torch(x, w, bias, s, Lv, La, relu), cid)
                assert not bool(ref[:, Lv:].any())
                if exact:
                    assert S.max() <= R.EXACT_MAX and bool((ref == ref.round()).all()) and bool(ref.any()), cid
                    continue
                n = kw + 1
                pre, _ = emulate(R.conv1_fwd, dt, (x, w, bias), ref, S, n, cid, **args)
                worst[dt] = max(worst[dt], pre)
                if kw > 1:
                    rejected(R.conv1_fwd(x, w.roll(1, 1), bias, **args), ref, S, n, dt, cid + " tap shifted")
                    rejected(R.conv1_fwd(x, w.flip(1), bias, **args), ref, S, n, dt, cid + " kernel flipped")
                if Lv > 1:
                    xl = torch.cat([x, x[:, :Lv]], 1)                          # (enough samples for the wider stride)
                    rejected(R.conv1_fwd(xl, w, bias, s + 1, Lv, La, relu), ref, S, n, dt, cid + " stride off by one")
                sw = ref.clone()
                sw[..., [0, 1]] = ref[..., [1, 0]]
                rejected(sw, ref, S, n, dt, cid + " channels swapped")
                if pad:
                    pr = ref.clone()
                    pr[:, Lv] = R.conv1_fwd(x, w, bias, s, 1, 1, 0)[:, 0] + 1e-3     # what the row would hold unzeroed
                    rejected(pr, ref, S, n, dt, cid + " pad row not zeroed")
    print("layer-1 forward: largest float32-emulation ratio", {R.name(k): round(v, 4) for k, v in worst.items()})
    print("  mistakes rejected (cases):", dict(REJECTED))


def test_layer1_backward_reference_emulation_and_mistakes():
    REJECTED.clear()
    worst = {dt: 0.0 for dt in DTYPES}
    for case in R.c1_bwd_cases():
        C, kw, s, B, Lv, nt, nb = case
        cid = R.c1_bwd_id(case)
        for dt in DTYPES:
            for exact in (False, True):
                x, dy, ldx, La = R.c1_bwd_data(case, dt, exact)
                ref = R.conv1_bwd(x, dy, s, kw, Lv)
                S = R.abs_bound_terms(R.conv1_bwd, x, dy, stride=s, kw=kw, L_valid=Lv)
                w = torch.zeros(C, kw, dtype=torch.float64, requires_grad=True)
                b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
                y = F.conv1d(x[:, None, :], w[:, None, :], b, stride=s).permute(0, 2, 1)
                (y * dy[:, :Lv]).sum().backward()
                close(ref[:kw], w.grad.T, cid + " dw")
                close(ref[kw], b.grad, cid + " db")
                if exact:
                    assert S.max() <= R.EXACT_MAX and bool((ref == ref.round()).all()) and bool(ref.any()), cid
                    continue
                n = B * Lv + 1
                pre = R.bound_ratio(R.conv1_bwd(x.float(), dy.float(), s, kw, Lv), ref, S, n, 0.0)     # slabs are f32 in both storage types
                assert pre <= 0.5, (cid, pre)
                worst[dt] = max(worst[dt], pre)
                if kw > 1:
                    rejected(torch.cat([ref[:kw].roll(1, 0), ref[kw:]]), ref, S, n, dt, cid + " tap shifted")
                    rejected(torch.cat([ref[:kw].flip(0), ref[kw:]]), ref, S, n, dt, cid + " kernel flipped")
                if Lv > 1:
                    xl = torch.cat([x, x[:, :Lv]], 1)
                    rejected(R.conv1_bwd(xl, dy, s + 1, kw, Lv), ref, S, n, dt, cid + " stride off by one")
                sw = ref.clone()
                sw[:, [0, 1]] = ref[:, [1, 0]]
                rejected(sw, ref, S, n, dt, cid + " channels swapped")
                if kw < R.C1_KA:
                    # two item blocks write their bias sums at row KA of their (kw + 1)-row slabs, i.e. outside them; the reader sums rows kw
                    parts, per = [R.conv1_bwd(x[:1], dy[:1], s, kw, Lv), R.conv1_bwd(x[1:], dy[1:], s, kw, Lv)], (kw + 1) * C
                    buf = torch.zeros(per + (R.C1_KA + 1) * C, dtype=torch.float64)
                    for z, pt in enumerate(parts):
                        buf[z * per:z * per + kw * C] = pt[:kw].reshape(-1)
                    for z, pt in enumerate(parts):
                        buf[z * per + R.C1_KA * C:z * per + (R.C1_KA + 1) * C] = pt[kw]
                    rejected(buf[:2 * per].view(2, kw + 1, C).sum(0), ref, S, n, dt, cid + " bias row at KA")
                dyp = dy.clone()                                               # (L_alloc = L_valid + 2: there is a pad row)
                dyp[:, Lv] = dy[:, 0] + 1e-3
                rejected(R.conv1_bwd(torch.cat([x, x[:, :s + kw]], 1), dyp, s, kw, Lv + 1), ref, S, n, dt, cid + " pad row not zeroed")
                # one slab dropped: the slabs of two item blocks, the second left out
                half = R.conv1_bwd(x[:1], dy[:1], s, kw, Lv)
                rejected(half, ref, S, n, dt, cid + " slab dropped")
                # the engine's two reduce forms: [C][1][kw] and [C]
                dw = R.reduce_slabs(ref[None, :kw], kw, C, 1, kw, 1, 0, torch.full((C * kw,), float("nan"), dtype=torch.float64))
                close(dw.view(C, kw), w.grad, cid + " reduce form")
    print("layer-1 backward: largest float32-emulation ratio", {R.name(k): round(v, 4) for k, v in worst.items()})
    print("  mistakes rejected (cases):", dict(REJECTED))


# ====================================================================================================================== layers >= 2
def _conv_torch(x, w, bias, dy, s, geo, relu, mask):
    """y, dx, dw by F.conv1d and autograd in float64, channels-first inside."""
    Lv, Lo = geo["Lin_valid"], geo["Lout_valid"]
    xi = x[:, :Lv].permute(0, 2, 1).clone().requires_grad_(True)
    wi = w.clone().requires_grad_(True)
    y = F.conv1d(xi, wi, bias, stride=s)
    assert y.shape[2] == Lo
    (y * dy[:, :Lo].permute(0, 2, 1)).sum().backward()
    yo = y.detach().permute(0, 2, 1)
    yo = yo.clamp_min(0) if relu else yo
    yo = F.pad(yo, (0, 0, 0, geo["Lout_alloc"] - Lo))
    dx = F.pad(xi.grad.permute(0, 2, 1), (0, 0, 0, geo["Lin_alloc"] - Lv))
    if mask:
        dx = dx * (x > 0)
    return yo, dx, wi.grad


def _wgrad_flat(x, dy, s, kw, tail=None):
    """The weight gradient the way the device forms it: every GEMM row m of the FLAT buffer with the window x_flat[m s, m s + kw), pad
    rows included (their windows reach into the next item or into x_tail)."""
    Cin = x.shape[2]
    tail = torch.zeros(max(0, kw - s), Cin, dtype=x.dtype) if tail is None else tail
    flat = torch.cat([x.reshape(-1, Cin), tail], 0)
    M = dy.shape[0] * dy.shape[1]
    win = flat[torch.arange(M)[:, None] * s + torch.arange(kw)[None, :]]               # [M][kw][Cin]
    return torch.einsum("mjc,mo->ocj", win, dy.reshape(M, -1))


def test_conv_references_emulation_and_mistakes():
    REJECTED.clear()
    worst = {}
    for shape in R.CONV_SHAPES:
        Cin, Cout, kw, s = shape
        for dt in DTYPES:
            for exact in (False, True):
                for slack in (False, True):
                    cid = f"{R.conv_id(shape)} {'exact' if exact else 'normal'} slack{int(slack)}"
                    geo, x, w, bias, dy = R.conv_data(shape, dt, exact, slack)
                    D, Lo, La, Li = geo["D"], geo["Lout_valid"], geo["Lout_alloc"], geo["Lin_alloc"]
                    assert La == Lo + D - 1 and Li == s * La and (geo["Lin_valid"] - kw) // s + 1 == Lo and geo["Lin_valid"] <= Li
                    assert geo["x_tail"] == max(0, kw - s) * Cin and geo["dy_head"] == (D - 1) * Cout
                    if slack and s > 1 and kw >= s:
                        assert geo["Lin_valid"] > (Lo - 1) * s + kw or Li == (Lo - 1) * s + kw
                    for relu in (0, 1):
                        for b_ in (bias, None):
                            ref = R.conv_fwd(x, w, b_, s, Lo, La, relu)
                            t_y, t_dx, t_dw = _conv_torch(x, w, b_, dy, s, geo, relu, True)
                            close(ref, t_y, cid + " fwd")
                    fargs = dict(stride=s, Lout_valid=Lo, Lout_alloc=La, relu=1)
                    ref_y = R.conv_fwd(x, w, bias, **fargs)
                    S_y = R.abs_bound_terms(R.conv_fwd, x, w, bias, stride=s, Lout_valid=Lo, Lout_alloc=La, relu=0)
                    ref_dx = R.conv_dgrad(dy, w, s, Li, x)
                    S_dx = R.conv_dgrad(dy.abs(), w.abs(), s, Li, x)
                    close(ref_dx, t_dx, cid + " dgrad masked")
                    close(R.conv_dgrad(dy, w, s, Li), _conv_torch(x, w, bias, dy, s, geo, 1, False)[1], cid + " dgrad")
                    wd = R.w_dgrad_layout(w, s)
                    assert wd.shape == (s * Cin, D * Cout)
                    close(R.dgrad_by_gemm(dy, wd, s, Cin, x), ref_dx, cid + " w_dgrad layout")
                    close(R.w_fwd_layout(w).view(Cout, kw, Cin), w.permute(0, 2, 1), cid + " w_fwd layout")
                    cov = R.covered_positions(shape, geo)
                    assert not bool(R.conv_dgrad(dy, w, s, Li)[:, ~cov].any()) and not bool(ref_dx[:, geo["Lin_valid"]:].any())
                    ref_dw = R.conv_wgrad(x, dy, s, kw)
                    S_dw = R.conv_wgrad(x.abs(), dy.abs(), s, kw)
                    close(ref_dw, t_dw, cid + " wgrad")
                    close(R.slab_layout(ref_dw).view(kw, Cin, Cout), ref_dw.permute(2, 1, 0), cid + " slab layout")
                    close(_wgrad_flat(x, dy, s, kw), ref_dw, cid + " wgrad over the flat buffer")      # windows that leave their item meet zero dy
                    tail = torch.full((geo["x_tail"] // Cin, Cin), 1e4, dtype=torch.float64)
                    close(_wgrad_flat(x, dy, s, kw, tail), ref_dw, cid + " wgrad over the flat buffer, 1e4 in x_tail")
                    rc = R.reduce_slabs(R.slab_layout(ref_dw)[None], kw * Cin, Cout, Cin, Cin * kw, 1, kw,
                                        torch.full((Cout * Cin * kw,), float("nan"), dtype=torch.float64))
                    close(rc.view(Cout, Cin, kw), ref_dw, cid + " conv-weight permutation")
                    if exact:
                        assert max(S_y.max(), S_dx.max(), S_dw.max()) <= R.EXACT_MAX, (cid, S_y.max(), S_dx.max(), S_dw.max())
                        assert all(bool((t == t.round()).all()) and bool(t.any()) for t in (ref_y, ref_dx, ref_dw))
                        continue
                    n_y, n_dx, n_dw = kw * Cin + 1, D * Cout, R.CONV_B * La + 1
                    for key, fn, tensors, ref, S, n, kwargs in (
                            ("fwd", R.conv_fwd, (x, w, bias), ref_y, S_y, n_y, fargs),
                            ("dgrad", R.conv_dgrad, (dy, w), ref_dx, S_dx, n_dx, dict(stride=s, Lin_alloc=Li, x_act=x)),
                            ("wgrad", R.conv_wgrad, (x, dy), ref_dw, S_dw, n_dw, dict(stride=s, kw=kw))):
                        od = R.F32 if key == "wgrad" else dt
                        pre, _ = emulate(fn, od, tensors, ref, S, n, cid + " " + key, **kwargs)
                        worst[(key, dt)] = max(worst.get((key, dt), 0.0), pre)
                    # ---- mistakes
                    if kw > 1:
                        rejected(R.conv_fwd(x, w.roll(1, 2), bias, **fargs), ref_y, S_y, n_y, dt, cid + " fwd tap shifted")
                        rejected(R.conv_fwd(x, w.flip(2), bias, **fargs), ref_y, S_y, n_y, dt, cid + " fwd kernel flipped")
                        rejected(R.conv_dgrad(dy, w.roll(1, 2), s, Li, x), ref_dx, S_dx, n_dx, dt, cid + " dgrad tap shifted")
                        rejected(R.conv_dgrad(dy, w.flip(2), s, Li, x), ref_dx, S_dx, n_dx, dt, cid + " dgrad kernel flipped")
                        rejected(ref_dw.roll(1, 2), ref_dw, S_dw, n_dw, R.F32, cid + " wgrad tap shifted")
                        rejected(ref_dw.flip(2), ref_dw, S_dw, n_dw, R.F32, cid + " wgrad kernel flipped")
                    xl = torch.cat([x, x[:, :Lo]], 1)                          # (enough positions for the wider stride)
                    rejected(R.conv_fwd(xl, w, bias, s + 1, Lo, La, 1), ref_y, S_y, n_y, dt, cid + " fwd stride off by one")
                    wide = R.conv_dgrad(dy, w, s + 1, (La - 1) * (s + 1) + kw + s + 1)[:, :Li] * (x > 0)
                    rejected(wide, ref_dx, S_dx, n_dx, dt, cid + " dgrad stride off by one")
                    xw = torch.cat([x, x[:, :La]], 1)
                    rejected(R.conv_wgrad(xw, dy, s + 1, kw), ref_dw, S_dw, n_dw, R.F32, cid + " wgrad stride off by one")
                    for what, ref, S, n, od, ax in (("fwd", ref_y, S_y, n_y, dt, 2), ("dgrad", ref_dx, S_dx, n_dx, dt, 2),
                                                    ("wgrad co", ref_dw, S_dw, n_dw, R.F32, 0), ("wgrad c", ref_dw, S_dw, n_dw, R.F32, 1)):
                        sw = ref.clone()
                        sw.index_copy_(ax, torch.tensor([0, 1]), ref.index_select(ax, torch.tensor([1, 0])))
                        rejected(sw, ref, S, n, od, cid + f" {what} channels swapped")
                    if La > Lo:
                        pr = ref_y.clone()
                        pr[:, Lo] = ref_y[:, Lo - 1] + 1e-3
                        rejected(pr, ref_y, S_y, n_y, dt, cid + " pad row not zeroed")
                        dyp = dy.clone()
                        dyp[:, Lo] = dy[:, Lo - 1] + 1e-3
                        rejected(R.dgrad_by_gemm(dyp, wd, s, Cin, x), ref_dx, S_dx, n_dx, dt, cid + " dgrad pad row not zeroed")
                        rejected(_wgrad_flat(x, dyp, s, kw), ref_dw, S_dw, n_dw, R.F32, cid + " wgrad pad row not zeroed")
                    if D * s > kw:
                        rejected(R.dgrad_by_gemm(dy, R.w_dgrad_layout(w, s, fill_from_last=True), s, Cin, x), ref_dx, S_dx, n_dx, dt,
                                 cid + " w_dgrad zero taps filled")
                    if D > 1:
                        rejected(R.dgrad_by_gemm(dy, R.w_dgrad_layout(w, s, reverse_dd=True), s, Cin, x), ref_dx, S_dx, n_dx, dt,
                                 cid + " w_dgrad dd reversed")
                    rejected(R.conv_wgrad(x[:2], dy[:2], s, kw), ref_dw, S_dw, n_dw, R.F32, cid + " wgrad slab dropped")
                    if Cin != kw:
                        ex = R.reduce_slabs(R.slab_layout(ref_dw)[None], kw * Cin, Cout, Cin, Cin * kw, kw, 1,
                                            torch.zeros(Cout * Cin * kw * max(kw, Cin), dtype=torch.float64))
                        rejected(ex[:Cout * Cin * kw].view(Cout, Cin, kw), ref_dw, S_dw, n_dw, R.F32, cid + " s_hi and s_lo exchanged")
    print("layers >= 2: largest float32-emulation ratio", {f"{k} {R.name(d)}": round(v, 4) for (k, d), v in sorted(worst.items(), key=str)})
    print("  mistakes rejected (cases):", dict(REJECTED))


def test_w_prep_layouts_at_every_shape():
    """w_fwd_layout / w_dgrad_layout against a plain loop over their definition in csrc/pointwise.hip, at every shape section C runs."""
    for shape in R.PREP_SHAPES:
        Cin, Cout, kw, s = shape
        if Cin * Cout * kw > 70000:
            sub_co, sub_c = [0, 1, 31, 32, Cout - 1], [0, 5, 31, 32, Cin - 1]
        else:
            sub_co, sub_c = range(Cout), range(Cin)
        w = R.normal(R.gen(kw * 7 + s), Cout, Cin, kw).double()
        D = -(-kw // s)
        fw, wd = R.w_fwd_layout(w), R.w_dgrad_layout(w, s).view(s, Cin, D, Cout)
        assert fw.shape == (Cout, kw * Cin)
        for co in sub_co:
            for c in sub_c:
                for j in range(kw):
                    assert fw[co, j * Cin + c] == w[co, c, j]
                for r in range(s):
                    for dd in range(D):
                        tap = r + (D - 1 - dd) * s
                        assert wd[r, c, dd, co] == (w[co, c, tap] if tap < kw else 0.0)


# ====================================================================================================================== reductions
def test_reduce_slabs_reference_emulation_and_mistakes():
    REJECTED.clear()
    worst = 0.0
    for I, J, nslab in R.REDUCE_CASES:
        g = R.gen(I * 7 + J + nslab)
        slabs = R.normal(g, nslab, I, J).float().double()
        isl = R.ints(g, -2, 2, nslab, I, J)
        assert isl.abs().sum(0).max() <= 2 * nslab < 2 ** 24
        total, S = slabs.sum(0), slabs.abs().sum(0)
        for fname, cdiv, s_j, s_hi, s_lo, n_out, off in R.reduce_forms(I, J):
            cid = f"I{I}-J{J}-z{nslab}-{fname}"
            idx = R.reduce_index(I, J, cdiv, s_j, s_hi, s_lo)
            assert idx.unique().numel() == I * J and int(idx.max()) < n_out, cid      # a permutation into out, nothing addressed twice
            out0 = torch.full((n_out,), -7.5, dtype=torch.float64)
            ref = R.reduce_slabs(slabs, I, J, cdiv, s_j, s_hi, s_lo, out0)
            for i in range(0, I, max(1, I // 5)):
                for j in range(0, J, max(1, J // 7)):
                    assert ref[j * s_j + (i // cdiv) * s_hi + (i % cdiv) * s_lo] == total[i, j]
            untouched = torch.ones(n_out, dtype=torch.bool)
            untouched[idx] = False
            assert bool((ref[untouched] == -7.5).all()) and int(untouched.sum()) == n_out - I * J
            Sp = R.reduce_slabs(slabs.abs(), I, J, cdiv, s_j, s_hi, s_lo, torch.zeros(n_out, dtype=torch.float64))
            emu = R.reduce_slabs(slabs.float(), I, J, cdiv, s_j, s_hi, s_lo, out0.float())
            pre = R.bound_ratio(emu, ref, Sp, nslab, 0.0)
            assert pre <= 0.5, (cid, pre)
            worst = max(worst, pre)
            rejected(R.reduce_slabs(slabs[:-1] if nslab > 1 else slabs * 0, I, J, cdiv, s_j, s_hi, s_lo, out0), ref, Sp, nslab, R.F32,
                     cid + " slab dropped")
            if I > 1 and s_hi != s_lo:                                 # (cdiv = 1: s_lo = 0 becomes the row pitch)
                ex = R.reduce_slabs(slabs, I, J, cdiv, s_j, s_lo, s_hi, torch.full((n_out * max(s_hi, s_lo, 2),), -7.5, dtype=torch.float64))
                rejected(ex[:n_out], ref, Sp, nslab, R.F32, cid + " s_hi and s_lo exchanged")
    print(f"reduce_slabs: largest float32-emulation ratio {worst:.4f}")
    print("  mistakes rejected (cases):", dict(REJECTED))


def test_colsum_emulation_and_mistakes():
    REJECTED.clear()
    worst = {dt: 0.0 for dt in DTYPES}
    for M, N in R.COLSUM_SHAPES:
        for dt in DTYPES:
            X = R.rounded(R.normal(R.gen(M + N), M, N), dt)
            ref, S = X.sum(0), X.abs().sum(0)
            pre = R.bound_ratio(X.float().sum(0), ref, S, M, 0.0)
            assert pre <= 0.5, (M, N, pre)
            worst[dt] = max(worst[dt], pre)
            rejected(X[:-1].sum(0) if M > 1 else X.sum(0) * 0, ref, S, M, R.F32, f"colsum {M}x{N} row dropped")
            sw = ref.clone()
            sw[[0, 1]] = ref[[1, 0]]
            rejected(sw, ref, S, M, R.F32, f"colsum {M}x{N} columns swapped")
            Xi = R.ints(R.gen(M), -2, 2, M, N)
            assert Xi.abs().sum(0).max() < 2 ** 24
    print("colsum: largest float32-emulation ratio", {R.name(k): round(v, 4) for k, v in worst.items()})
    print("  mistakes rejected (cases):", dict(REJECTED))


def test_tile_kernel_cases():
    """The wrapper-level tile-kernel cases: conv_fwd on the gathered rows against F.conv1d, conv_wgrad against autograd, the float32
    emulation against the bound, S <= 256 in the exact-data twins, and the fixed rows of tile_rows."""
    Cin, Cout, kw, s = R.TILE_FWD_SHAPE
    La, Lo = R.TILE_FWD_LA, R.TILE_FWD_LA - 1
    worst = 0.0
    for B in R.TILE_FWD_B:
        M = B * La
        rows = R.tile_rows(M, La, Lo, 4096, B)
        last_tile = (M - 1) // 256 * 256
        assert rows.numel() >= 4000 and bool(((rows % La) < Lo).all())
        assert all(r in rows for r in (0, Lo - 1, M - La, M - La + Lo - 1, 255, 256, last_tile - 1, last_tile))
        for exact in (False, True):
            x, w, bias = R.tile_fwd_data(B, exact)
            win = R.gathered_windows(x, rows, La, s, kw)
            assert torch.equal(win[5], x[rows[5] // La, (rows[5] % La) * s:(rows[5] % La) * s + kw])
            ref = R.conv_fwd(win, w, bias, s, 1, 1, 1)[:, 0]
            S = R.abs_bound_terms(R.conv_fwd, win, w, bias, stride=s, Lout_valid=1, Lout_alloc=1, relu=0)[:, 0]
            close(ref, F.conv1d(win.permute(0, 2, 1), w, bias)[:, :, 0].clamp_min(0), f"tile fwd B{B}")
            if exact:
                assert S.max() <= R.EXACT_MAX and bool((ref == ref.round()).all()) and bool(ref.any())
                continue
            pre, _ = emulate(R.conv_fwd, R.BF16, (win, w, bias), ref[:, None], S[:, None], kw * Cin + 1, f"tile fwd B{B}",
                             stride=s, Lout_valid=1, Lout_alloc=1, relu=1)
            worst = max(worst, pre)
            rejected(R.conv_fwd(win, w.roll(1, 2), bias, s, 1, 1, 1)[:, 0], ref, S, kw * Cin + 1, R.BF16, f"tile fwd B{B} tap shifted")
    Cin, Cout, kw, s = R.TILE_WGRAD_SHAPE
    M = R.TILE_WGRAD_B * R.TILE_WGRAD_LA
    for exact in (False, True):
        x, dy = R.tile_wgrad_data(exact)
        ref, S = R.conv_wgrad(x, dy, s, kw), R.conv_wgrad(x.abs(), dy.abs(), s, kw)
        wi = torch.zeros(Cout, Cin, kw, dtype=torch.float64, requires_grad=True)
        y = F.conv1d(x.permute(0, 2, 1), wi, stride=s)
        (y * dy[:, :y.shape[2]].permute(0, 2, 1)).sum().backward()
        close(ref, wi.grad, "tile wgrad")
        if exact:
            assert S.max() <= R.EXACT_MAX and bool((ref == ref.round()).all()) and bool(ref.any())
            continue
        pre, _ = emulate(R.conv_wgrad, R.F32, (x, dy), ref, S, M + R.TILE_WGRAD_NSPLIT, "tile wgrad", stride=s, kw=kw)
        worst = max(worst, pre)
        rejected(ref.roll(1, 2), ref, S, M + R.TILE_WGRAD_NSPLIT, R.F32, "tile wgrad tap shifted")
    print(f"tile-kernel cases: largest float32-emulation ratio {worst:.4f}")


# what test_conv1d_kernels_gpu.py's docstring states per case: forward f32 / bf16, data gradient f32 / bf16
KERNEL_TABLE = {
    (64, 64, 7, 3): ("fast storage", "fast storage", "fast 3 taps", "fast 3 taps"),
    (64, 32, 5, 1): ("fast 5 taps", "fast 5 taps", "fast 5 taps", "generic"),
    (32, 64, 3, 2): ("fast storage", "generic", "fast 2 taps", "fast 2 taps"),
    (64, 64, 4, 4): ("fast storage", "fast storage", "fast storage", "fast storage"),
    (64, 64, 2, 4): ("fast storage", "fast storage", "fast storage", "fast storage"),
    (24, 40, 3, 1): ("generic", "generic", "generic", "generic"),
    (16, 16, 40, 2): ("fast 20 taps", "fast storage", "fast storage", "fast storage"),
    (64, 64, 33, 1): ("fast 33 taps", "fast 33 taps", "fast 33 taps", "fast 33 taps"),
    (64, 64, 8, 4): ("fast 2 taps", "fast 2 taps", "fast 2 taps", "fast 2 taps"),
}


def test_kernel_table_of_the_gpu_module_follows_the_launchers_conditions():
    def word(v):
        return "generic" if v[0] == "generic" else f"fast {v[2]} taps" if v[2] > 1 else "fast storage"

    assert set(KERNEL_TABLE) == set(R.CONV_SHAPES)
    for shape, row in KERNEL_TABLE.items():
        Cin, Cout, kw, s = shape
        geo = R.conv_geometry(shape, False)
        M, D = R.CONV_B * geo["Lout_alloc"], geo["D"]
        got = tuple(word(R.nt_variant(dt, M, N, K, lda)) for N, K, lda in ((Cout, kw * Cin, s * Cin), (s * Cin, D * Cout, Cout))
                    for dt in DTYPES)
        assert got == row, (shape, got)
        assert R.tn_variant(R.BF16, kw * Cin, Cout) == "fast" and R.tn_variant(R.F32, kw * Cin, Cout) == "generic"
