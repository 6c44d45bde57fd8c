"""Host-only checks of tests/gemm_reference.py, the references test_gemm_kernels_gpu.py judges cpc_gemm_nt / cpc_gemm_tn by.  No GPU is
needed, but libcpc_hip.so has to be built: the path test and the argument checks call into it (CPC_GEMM_QUERY_EPI launches nothing).

  * the address-level references against independent formulations: torch.einsum (plain, batched), F.conv1d (overlapped rows), F.conv2d
    (rows gathered from a grid), torch.nn.grad.conv2d_weight (two-level TN rows), a row-sliced matmul (slabs);
  * the case lists reach every kernel path the launchers can pick, and the host mirror of the launchers agrees with _hip.nt_tile,
    _hip.tn_tile and the epilogue form CPC_GEMM_QUERY_EPI reports;
  * "reference alone": the float32 emulation of every case against the bound without its u_out term stays <= 1 (the largest ratio per
    kernel group is printed; test_gemm_kernels_gpu.py's docstring records them);
  * the metric rejects deliberate mistakes, on random data through the bound and on the exact-data twins through equality, at every
    case a mistake applies to; and the whole-tensor measure of the older tests accepts a dropped K element at (2048, 512, 1024) bf16;
  * the argument checks of cpc_gemm_nt, through CPC_GEMM_QUERY_EPI (no launch: 100 + form when every check passes, -22 otherwise).
"""
import collections
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_reference as G
from conv1d_reference import w_fwd_layout
from gemm_reference import BF16, F32, F64, NT, TN

EINVAL = -22
BASE = 0x10000          # a 16-byte-aligned address that is never dereferenced (the query flag launches nothing)

NT_CASES, TN_CASES = G.nt_cases(), G.tn_cases()


@functools.lru_cache(maxsize=None)
def nt_case_data(cid, exact):
    return G.nt_data(dict(NT_CASES)[cid], exact)


@functools.lru_cache(maxsize=None)
def tn_case_data(cid, exact):
    return G.tn_data(dict(TN_CASES)[cid], exact)


@functools.lru_cache(maxsize=None)
def nt_case_ref(cid, exact):
    return G.nt_run_reference(dict(NT_CASES)[cid], nt_case_data(cid, exact))


@functools.lru_cache(maxsize=None)
def tn_case_ref(cid, exact):
    return G.tn_run_reference(dict(TN_CASES)[cid], tn_case_data(cid, exact))


def nt_struct(a, A=BASE, Bt=BASE, Cp=BASE, bias=BASE, mask=BASE, k_ranges=BASE, flags=0, **over):
    """cpc_gemm_nt_args from a gemm_reference.NT dict and raw addresses of 256-byte-aligned allocations (the dict's off* are added)."""
    from cpc_audio_amd import _hip
    es, oes = G.es_of(a["dt"]), (4 if G.nt_out_f32(a) else 2)
    d = dict(a)
    d.update(over)
    return _hip.GemmNTArgs(A + a["offA"] * es, Bt + a["offB"] * es, Cp + a["offC"] * oes, bias + a["off_bias"] * 4 if a["bias"] else None,
                           mask + a["off_mask"] * es if a["mask"] else None, d["M"], d["N"], d["K"], d["lda"], d["ldb"], d["ldc"], d["a_rpi"],
                           d["a_item"], d["b_rpi"], d["b_item"], d["c_rpi"], d["c_item"], d["c_valid"], d["a_batch"], d["b_batch"], d["c_batch"],
                           d["batch"], d["flags"] | flags, _hip.dtype_code(a["dt"]), d.get("a_extent", 0), d.get("b_extent", 0), d["a_rpi2"],
                           d["a_item2"], d["c_rpi2"], d["c_item2"], k_ranges if a["k_ranges"] is not None else None, d["k_taps"],
                           d["k_tap_stride"], d["k_tap_stride_a"])


def nt_query(a, **over):
    """The status of the call with CPC_GEMM_QUERY_EPI: 100 + epilogue form, or -22."""
    from cpc_audio_amd import _hip
    lib = _hip.lib()
    a = dict(a, **over)
    s = nt_struct(a, flags=G.QUERY_EPI)
    if a["bits"]:
        return lib.cpc_gemm_nt_bits(C.byref(s), C.c_void_p(BASE), None, C.c_void_p(0))
    return lib.cpc_gemm_nt(C.byref(s), C.c_void_p(0))


# ======================================================================================================== independent formulations
def full_nan(n, dtype=F64):
    return torch.full((n,), G.NAN, dtype=dtype)


def test_nt_reference_plain_and_batched_against_einsum():
    g = G.gen(1)
    Z, M, N, K, lda, ldb, ldc = 3, 7, 12, 16, 20, 24, 16
    A, B = G.normal(g, Z, M + 1, lda).double(), G.normal(g, Z, N + 2, ldb).double()
    bias, mask = G.normal(g, N).double(), G.normal(g, Z, M + 3, ldc).double()
    a = NT(F32, M, N, K, lda=lda, ldb=ldb, ldc=ldc, batch=Z, a_batch=(M + 1) * lda, b_batch=(N + 2) * ldb, c_batch=(M + 3) * ldc, bias=True,
           mask=True, flags=G.RELU)
    r = G.nt_reference(a, A.reshape(-1), B.reshape(-1), bias, mask.reshape(-1), full_nan(Z * (M + 3) * ldc))
    want = (torch.einsum("zmk,znk->zmn", A[:, :M, :K], B[:, :N, :K]) + bias).clamp_min(0) * (mask[:, :M, :N] > 0)
    got = r.out.reshape(Z, M + 3, ldc)
    torch.testing.assert_close(got[:, :M, :N], want, rtol=1e-12, atol=1e-12)
    assert bool(torch.isnan(got[:, M:]).all()) and bool(torch.isnan(got[:, :, N:]).all())
    assert r.n == K + 1 and torch.equal(r.written.reshape(Z, M + 3, ldc)[:, :M, :N], torch.ones(Z, M, N, dtype=torch.bool))
    S = (torch.einsum("zmk,znk->zmn", A[:, :M, :K].abs(), B[:, :N, :K].abs()) + bias.abs()) * (mask[:, :M, :N] > 0)
    torch.testing.assert_close(r.S.reshape(Z, M + 3, ldc)[:, :M, :N], S, rtol=1e-12, atol=1e-12)
    # plain, pad columns: N % 4 != 0 gives zeros up to the next multiple of 4 and nothing beyond
    a = NT(F32, M, 10, K, lda=lda, ldb=ldb, ldc=16)
    r = G.nt_reference(a, A[0].reshape(-1), B[0].reshape(-1), None, None, full_nan(M * 16))
    got = r.out.reshape(M, 16)
    torch.testing.assert_close(got[:, :10], A[0, :M, :K] @ B[0, :10, :K].T, rtol=1e-12, atol=1e-12)
    assert bool((got[:, 10:12] == 0).all()) and bool(torch.isnan(got[:, 12:]).all())


def test_nt_reference_overlapped_rows_against_conv1d():
    """The strided convolution view (lda = stride C_in < K = kw C_in), items of L_out rows with pad rows zeroed or skipped."""
    g = G.gen(2)
    B, L, Cin, Cout, kw, s, Lout_alloc = 3, 40, 4, 8, 5, 2, 20
    Lout = (L - kw) // s + 1
    x, w, bias = G.normal(g, B, L, Cin).double(), G.normal(g, Cout, Cin, kw).double(), G.normal(g, Cout).double()
    want = F.conv1d(x.permute(0, 2, 1), w, bias, stride=s).permute(0, 2, 1)                      # [B][Lout][Cout]
    flat = torch.cat([x.reshape(-1), torch.zeros(kw * Cin, dtype=F64)])
    for skip in (0, G.SKIP_PAD_ROWS):
        a = NT(F32, B * Lout_alloc, Cout, kw * Cin, lda=s * Cin, a_rpi=Lout_alloc, a_item=L * Cin, c_rpi=Lout_alloc, c_item=Lout_alloc * Cout + 4,
               c_valid=Lout, ldc=Cout, bias=True, flags=skip)
        r = G.nt_reference(a, flat, w_fwd_layout(w).reshape(-1), bias, None, full_nan(B * (Lout_alloc * Cout + 4)))
        got = r.out.reshape(B, Lout_alloc * Cout + 4)
        torch.testing.assert_close(got[:, :Lout * Cout].reshape(B, Lout, Cout), want, rtol=1e-12, atol=1e-12)
        pad = got[:, Lout * Cout:Lout_alloc * Cout]
        assert bool(torch.isnan(pad).all()) if skip else bool((pad == 0).all())
        assert bool(torch.isnan(got[:, Lout_alloc * Cout:]).all())


def test_nt_reference_gathered_taps_against_conv2d():
    """k_taps pieces of kh C elements, one grid column (H C elements) apart: an nn.Conv2d window read from a channels-last grid
    [column][row][channel]; rows = (column, row) in items of H_out rows."""
    g = G.gen(3)
    W, H, Cc, Co, kh, kw = 9, 11, 4, 6, 3, 2
    Wo, Ho = W - kw + 1, H - kh + 1
    grid, w = G.normal(g, W, H, Cc).double(), G.normal(g, Co, Cc, kh, kw).double()
    want = F.conv2d(grid.permute(2, 1, 0)[None], w)[0].permute(2, 1, 0)                          # [Wo][Ho][Co]
    Bt = w.permute(0, 3, 2, 1).reshape(Co, kw * kh * Cc)                                          # [co][(dx, dy, c)]
    a = NT(F32, Wo * Ho, Co, kw * kh * Cc, lda=Cc, a_rpi=Ho, a_item=H * Cc, k_taps=kw, k_tap_stride=kh * Cc, k_tap_stride_a=H * Cc, ldc=8)
    r = G.nt_reference(a, grid.reshape(-1), Bt.reshape(-1), None, None, full_nan(Wo * Ho * 8))
    torch.testing.assert_close(r.out.reshape(Wo, Ho, 8)[:, :, :Co], want, rtol=1e-12, atol=1e-12)
    assert G.nt_geometry(a)["sizeA"] == W * H * Cc                   # the last window ends with the grid


def test_nt_reference_second_level_and_k_ranges():
    """Two-level rows against explicit indexing; K ranges: the exact contract cuts each band's own range out of non-zero data, the union
    contract on data that is zero outside the ranges equals the full product."""
    g = G.gen(4)
    bk = 32
    a = NT(F32, 256, 8, 3 * bk, a_rpi=16, a_item=17 * 3 * bk, a_rpi2=8, a_item2=8 * 17 * 3 * bk + 4, c_rpi=16, c_item=16 * 8, c_valid=16,
           c_rpi2=8, c_item2=130 * 8, ldc=8, k_ranges=[(0, 2), (1, 3)], flags=G.KRANGE_EXACT)
    geo = G.nt_geometry(a)
    A, Bt = G.normal(g, geo["sizeA"]).double(), G.normal(g, geo["sizeB"]).double()
    r = G.nt_reference(a, A, Bt, None, None, full_nan(geo["sizeC"]))
    for m in (0, 15, 16, 127, 128, 255):
        band, item, row = m // 128, (m // 16) % 8, m % 16
        lo, hi = a["k_ranges"][band]
        arow = A[band * a["a_item2"] + item * a["a_item"] + row * 3 * bk:][:3 * bk]
        want = Bt.reshape(8, 3 * bk)[:, lo * bk:hi * bk] @ arow[lo * bk:hi * bk]
        torch.testing.assert_close(r.out[band * 130 * 8 + item * 128 + row * 8:][:8], want, rtol=1e-12, atol=1e-12)
    b = dict(a, flags=0, k_ranges=[(0, 1), (2, 3)] * 8, a_rpi=8, a_rpi2=2, c_rpi=8, c_rpi2=2, c_valid=8, c_item=64, a_item=9 * 3 * bk)
    d = G.nt_data(b, False)
    full = G.nt_run_reference(dict(b, k_ranges=None, a_rpi2=b["a_rpi2"]), d)
    torch.testing.assert_close(G.nt_run_reference(b, d).out, full.out, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert bool((d["A"] == 0).any()) and not bool(G.nt_kmask(b, own=True).all())


def test_tn_reference_two_level_against_conv2d_weight():
    """Rows = (clip, output column, output row) of a channels-last grid [clip][column][row][channel], a_batch stepping over the kernel
    columns: batch entry j is dw[:, :, :, j] of a strided nn.Conv2d."""
    g = G.gen(5)
    Bc, W, H, Cc, Co, kh, kw, s = 2, 9, 11, 4, 8, 3, 2, 2
    Wo, Ho = (W - kw) // s + 1, (H - kh) // s + 1
    grid, dy = G.normal(g, Bc, W, H, Cc).double(), G.normal(g, Bc, Wo, Ho, Co).double()
    want = torch.nn.grad.conv2d_weight(grid.permute(0, 3, 2, 1), (Co, Cc, kh, kw), dy.permute(0, 3, 2, 1), stride=s)   # [Co][C][kh][kw]
    a = TN(F32, Bc * Wo * Ho, kh * Cc, Co, lda=s * Cc, a_rpi=Ho, a_item=s * H * Cc, a_rpi2=Wo, a_item2=W * H * Cc, batch=kw, a_batch=H * Cc,
           b_batch=0, c_batch=kh * Cc * Co)
    flat = torch.cat([grid.reshape(-1), torch.zeros(kh * Cc, dtype=F64)])
    r = G.tn_reference(a, flat, dy.reshape(-1), full_nan(kw * kh * Cc * Co))
    got = r.out.reshape(kw, kh, Cc, Co).permute(3, 2, 1, 0)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((r.n == Bc * Wo * Ho).all())


def test_tn_reference_slabs_against_row_sliced_matmul():
    g = G.gen(6)
    M, I, J, lda, ldb, ldc, chunk, nsplit = 150, 5, 8, 8, 12, 12, 64, 4
    A, B = G.normal(g, M, lda).double(), G.normal(g, M, ldb).double()
    a = TN(F32, M, I, J, lda=lda, ldb=ldb, ldc=ldc, nsplit=nsplit, m_chunk=chunk, slab_stride=I * ldc + 4)
    r = G.tn_reference(a, A.reshape(-1), B.reshape(-1), full_nan(G.tn_geometry(a)["sizeC"]))
    for s in range(nsplit):
        lo, hi = min(M, s * chunk), min(M, (s + 1) * chunk)
        slab = r.out[s * (I * ldc + 4):][:(I - 1) * ldc + J]
        got = torch.stack([slab[i * ldc:i * ldc + J] for i in range(I)])
        torch.testing.assert_close(got, A[lo:hi, :I].T @ B[lo:hi, :J], rtol=1e-12, atol=1e-12)
        assert bool((r.n[s * (I * ldc + 4):][:J] == hi - lo).all())
    assert bool((r.out[3 * (I * ldc + 4):][:J] == 0).all())          # the empty chunk: a zero slab
    assert int(torch.isnan(r.out).sum()) == r.out.numel() - nsplit * I * J
    # c_rpi / c_item output rows
    a = TN(F32, M, I, J, lda=lda, ldb=ldb, ldc=ldc, c_rpi=2, c_item=30)
    r = G.tn_reference(a, A.reshape(-1), B.reshape(-1), full_nan(G.tn_geometry(a)["sizeC"]))
    full = A[:, :I].T @ B[:, :J]
    for i in range(I):
        torch.testing.assert_close(r.out[(i // 2) * 30 + (i % 2) * ldc:][:J], full[i], rtol=1e-12, atol=1e-12)


# ======================================================================================================== paths
def test_case_lists_reach_every_kernel_path_and_the_mirror_agrees_with_the_library():
    from cpc_audio_amd import _hip
    hit = collections.Counter()
    for cid, a in NT_CASES:
        c = G.nt_choice(a)
        assert c is not None, cid
        hit[c["path"]] += 1
        code = _hip.dtype_code(a["dt"])
        if c["path"] != "nt skinny":
            assert c["tile"] == _hip.nt_tile(code, a["M"], a["N"], a["K"], a["flags"], a["batch"]), cid
        assert nt_query(a) == 100 + c["form"], (cid, nt_query(a))
    assert sorted(hit) == sorted(G.NT_PATHS), (set(G.NT_PATHS) - set(hit), set(hit) - set(G.NT_PATHS))
    hit = collections.Counter()
    for cid, a in TN_CASES:
        c = G.tn_choice(a)
        assert c is not None, cid
        hit[c["path"]] += 1
        if c["path"] != "tn skinny":
            assert c["tile"] == _hip.tn_tile(_hip.dtype_code(a["dt"]), a["M"], a["I"], a["J"], max(a["nsplit"], 1), a["m_chunk"], a["flags"]), cid
    assert sorted(hit) == sorted(G.TN_PATHS), (set(G.TN_PATHS) - set(hit), set(hit) - set(G.TN_PATHS))
    # the axes of the NT case list, per kernel group: each value on every kernel that accepts it
    by = collections.defaultdict(list)
    for _, a in NT_CASES:
        by[G.group(G.nt_choice(a)["path"])].append(a)

    def has(grp, cond):
        return any(cond(a) for a in by[grp])

    X, SK = G.KRANGE_EXACT, G.SKIP_PAD_ROWS
    for grp, tile in (("nt generic", 128), ("nt fast128", 128), ("nt 256", 256)):
        Ms = {a["M"] for a in by[grp]}
        assert Ms >= ({1, 17, 127, 128, 129} if tile == 128 else {256, 257}), (grp, sorted(Ms))
        for what, cond in (("N % 4", lambda a: a["N"] % 4), ("N % 8 == 4", lambda a: a["N"] % 8 == 4), ("N = tile", lambda a: a["N"] == tile),
                           ("N > tile", lambda a: a["N"] > tile and a["N"] % tile), ("lda > K", lambda a: a["lda"] > a["K"]),
                           ("lda < K", lambda a: a["lda"] < a["K"] and not a["k_taps"]), ("ldc > N", lambda a: a["ldc"] > G.round4(a["N"])),
                           ("windows", lambda a: a["a_rpi"] and a["c_rpi"] and a["a_rpi"] != a["c_rpi"]), ("b_rpi", lambda a: a["b_rpi"]),
                           ("batch 3", lambda a: a["batch"] == 3 and len({a["a_batch"], a["b_batch"], a["c_batch"]}) == 3 and a["mask"]),
                           ("bias", lambda a: a["bias"]), ("relu", lambda a: a["flags"] & G.RELU), ("mask", lambda a: a["mask"]),
                           ("pad rows zeroed", lambda a: a["c_rpi"] and 0 < a["c_valid"] < a["c_rpi"] and not a["flags"] & SK),
                           ("pad rows skipped", lambda a: a["c_rpi"] and 0 < a["c_valid"] < a["c_rpi"] and a["flags"] & SK)):
            assert has(grp, cond), (grp, what)
        if tile == 128:
            for cv in (0, 1, 8):
                for skip in (0, SK):
                    assert has(grp, lambda a: a["c_rpi"] == 8 and a["c_valid"] == cv and (a["flags"] & SK) == skip), (grp, cv, skip)
        if grp != "nt generic":           # (alignment changes nothing on the generic kernel; rows in bands, K ranges and pieces do not exist there)
            for what, cond in (("bias unaligned", lambda a: a["bias"] and a["off_bias"]), ("C unaligned", lambda a: a["offC"]),
                               ("mask unaligned", lambda a: a["mask"] and a["off_mask"]), ("LINEAR_K", lambda a: a["flags"] & G.LINEAR_K),
                               ("union K ranges", lambda a: a["a_rpi2"] and a["c_rpi2"] and a["k_ranges"] is not None and not a["flags"] & X),
                               ("exact K ranges", lambda a: a["a_rpi2"] and a["c_rpi2"] and a["k_ranges"] is not None and a["flags"] & X),
                               ("gathered pieces", lambda a: a["k_taps"] > 1),
                               ("grid-convolution launch", lambda a: a["mask"] and a["a_rpi2"] and a["c_rpi2"] and a["k_taps"] > 1 and
                                a["k_ranges"] is not None and a["flags"] & X and a["flags"] & SK)):
                assert has(grp, cond), (grp, what)
    assert has("nt fast128", lambda a: a["flags"] & G.OUT_F32) and has("nt generic", lambda a: a["flags"] & G.OUT_F32) and has("nt 256", lambda a: a["flags"] & G.OUT_F32)
    assert {(a["N"], a["K"]) for a in by["nt skinny"]} >= {(8, 4), (16, 20), (32, 32)}
    assert {a["K"] // 64 for _, a in NT_CASES if G.nt_choice(a)["path"] == "nt 256 persistent"} >= {2, 3}          # even and odd stage counts
    assert any(a["M"] == G.PERSIST_M for _, a in NT_CASES) and {a["nsplit"] for _, a in TN_CASES} >= {1, 3, 5}


# ======================================================================================================== reference alone
def test_float32_emulation_stays_within_the_bound_and_twins_are_exact():
    """The float32 host emulation against the bound WITHOUT its u_out term; exact twins: sum |a||b| <= 256 and float32 == float64."""
    worst = collections.defaultdict(float)
    for cases, data, ref, run, choice in ((NT_CASES, nt_case_data, nt_case_ref, G.nt_run_reference, G.nt_choice),
                                          (TN_CASES, tn_case_data, tn_case_ref, G.tn_run_reference, G.tn_choice)):
        for cid, a in cases:
            grp = G.group(choice(a)["path"]) + " " + G.name(a["dt"])
            for exact in (False, True):
                r, e = ref(cid, exact), run(a, data(cid, exact), F32)
                assert torch.equal(e.written, r.written)
                if exact:
                    assert float(r.S.max()) <= G.EXACT_MAX, (cid, float(r.S.max()))
                    assert G.judge(e.out, r, F32, True) == 0.0, cid
                else:
                    q = G.judge(e.out, r, F32, False)
                    assert q <= 1.0, (cid, q)
                    worst[grp] = max(worst[grp], q)
    for grp in sorted(worst):
        print(f"reference alone {grp}: {worst[grp]:.4f}")


# ======================================================================================================== deliberate mistakes
def _stored(ref, odt):
    """The reference as a correct kernel would store it (rounded to the output type): what a mutant is compared with."""
    return ref.out.to(odt).double()


@pytest.mark.parametrize("mut", G.NT_MUTANTS)
def test_metric_rejects_nt_mistakes(mut):
    n = 0
    for cid, a in NT_CASES:
        if not G.nt_mutant_applies(mut, a):
            continue
        n += 1
        odt = G.out_dtype(a)
        chk = (lambda r: r.written) if a["rows"] is not None else (lambda r: None)
        for exact in (False, True):
            r = nt_case_ref(cid, exact)
            assert G.judge(_stored(r, odt), r, odt, exact, chk(r)) <= 1.0, cid                 # (the unmutated output passes)
            bad = G.nt_run_reference(a, nt_case_data(cid, exact), mut=mut)
            assert G.judge(_stored(bad, odt), r, odt, exact, chk(r)) > 1.0, (mut, cid, exact)
    assert n >= 2, (mut, n)


@pytest.mark.parametrize("mut", G.TN_MUTANTS)
def test_metric_rejects_tn_mistakes(mut):
    n = 0
    for cid, a in TN_CASES:
        if not G.tn_mutant_applies(mut, a):
            continue
        n += 1
        odt = G.out_dtype(a)
        for exact in (False, True):
            r = tn_case_ref(cid, exact)
            assert G.judge(_stored(r, odt), r, odt, exact) <= 1.0, cid
            bad = G.tn_run_reference(a, tn_case_data(cid, exact), mut=mut)
            assert G.judge(_stored(bad, odt), r, odt, exact) > 1.0, (mut, cid, exact)
    assert n >= 2, (mut, n)


def test_bound_rejects_truncated_bf16_output_and_the_twins_cannot_see_it():
    n = 0
    for cases, ref in ((NT_CASES, nt_case_ref), (TN_CASES, tn_case_ref)):
        for cid, a in cases:
            if G.out_dtype(a) != BF16 or int((ref(cid, False).out.nan_to_num() != 0).sum()) < 64:     # (a handful of outputs may all truncate by < half an ulp)
                continue
            n += 1
            chk = ref(cid, False).written if a.get("rows") is not None else None
            r = ref(cid, False)
            assert G.judge(G.truncated_bf16(r.out), r, BF16, False, chk) > 1.0, cid
            r = ref(cid, True)
            assert G.judge(G.truncated_bf16(r.out), r, BF16, True, r.written if chk is not None else None) == 0.0, cid
    assert n >= 10


def test_whole_tensor_measure_accepts_a_dropped_k_element():
    """The gap: at (2048, 512, 1024) bf16 the older tests' max |got - ref| / max |ref| < 1.2e-2 accepts an output in which a row has lost
    its last K element; the per-element bound rejects it."""
    a = NT(BF16, 2048, 512, 1024)
    d = G.nt_data(a, False)
    r = G.nt_run_reference(a, d)
    bad = _stored(G.nt_run_reference(a, d, mut="drop_last_k"), BF16)
    old = float((bad - r.out).abs().max() / r.out.abs().max())
    print(f"whole-tensor measure of the mutant: {old:.2e}  (max |ref| = {float(r.out.abs().max()):.0f})")
    assert old < 1.2e-2
    assert G.judge(bad, r, BF16, False) > 1.0


# ======================================================================================================== argument checks
OK = 100


def test_nt_extents():
    for dt in (F32, BF16):
        ch = G.ch_of(dt)
        K = 8 * ch
        a = NT(dt, 10, 8, K, lda=K + ch)
        need_a, need_b = 9 * (K + ch) + K, 7 * K + K
        assert nt_query(a, a_extent=need_a, b_extent=need_b) == OK
        assert nt_query(a, a_extent=need_a - 1) == EINVAL and nt_query(a, b_extent=need_b - 1) == EINVAL
        a = NT(dt, 10, 8, 3 * K, lda=K)                                  # overlapped rows: the last row ends K - lda beyond [M][lda]
        assert nt_query(a, a_extent=9 * K + 3 * K) == OK and nt_query(a, a_extent=10 * K) == EINVAL
        a = NT(dt, 10, 8, K, a_rpi=4, a_item=5 * K + ch, b_rpi=3, b_item=4 * K)
        need_a, need_b = 2 * (5 * K + ch) + K + K, 2 * 4 * K + K + K
        assert nt_query(a, a_extent=need_a, b_extent=need_b) == OK
        assert nt_query(a, a_extent=need_a - 1) == EINVAL and nt_query(a, b_extent=need_b - 1) == EINVAL
        a = NT(dt, 10, 8, K, batch=3, a_batch=11 * K, b_batch=9 * K, c_batch=80)
        need_a, need_b = 2 * 11 * K + 10 * K, 2 * 9 * K + 8 * K
        assert nt_query(a, a_extent=need_a, b_extent=need_b) == OK
        assert nt_query(a, a_extent=need_a - 1) == EINVAL and nt_query(a, b_extent=need_b - 1) == EINVAL
        # the extent check knows neither the second row level nor gathered pieces
        a = NT(dt, 32, 8, K, a_rpi=4, a_item=4 * K, a_rpi2=2, a_item2=8 * K)
        assert nt_query(a) == OK and nt_query(a, a_extent=1 << 30) == EINVAL
        a = NT(dt, 10, 8, 2 * K, lda=ch, k_taps=2, k_tap_stride=K, k_tap_stride_a=2 * K)
        assert nt_query(a) == OK and nt_query(a, a_extent=1 << 30) == EINVAL and nt_query(a, b_extent=8 * 2 * K) == OK


def test_nt_divisibility_conditions():
    for dt in (F32, BF16):
        ch = G.ch_of(dt)
        bk = 8 * ch
        base = NT(dt, 40, 16, bk, lda=bk + ch, ldb=bk + ch, ldc=20)
        assert nt_query(base) == OK
        for field in ("K", "lda", "ldb"):
            assert nt_query(base, **{field: base[field] + ch // 2}) == EINVAL, field
        assert nt_query(base, ldc=22) == EINVAL and nt_query(base, ldc=12) == EINVAL
        assert nt_query(base, N=14) == OK
        assert nt_query(dict(base, bias=True), N=14) == EINVAL and nt_query(dict(base, mask=True), N=14) == EINVAL
        rows = dict(base, a_rpi=8, a_item=9 * (bk + ch), b_rpi=4, b_item=5 * (bk + ch), c_rpi=8, c_item=9 * 20, c_valid=8)
        assert nt_query(rows) == OK
        assert nt_query(rows, a_item=rows["a_item"] + ch // 2) == EINVAL and nt_query(rows, b_item=rows["b_item"] + ch // 2) == EINVAL
        assert nt_query(rows, c_item=rows["c_item"] + 2) == EINVAL
        two = dict(rows, a_rpi2=2, a_item2=20 * (bk + ch), c_rpi2=2, c_item2=400)
        assert nt_query(two) == OK
        assert nt_query(two, a_item2=two["a_item2"] + ch // 2) == EINVAL and nt_query(two, c_item2=402) == EINVAL
        assert nt_query(two, a_rpi=0) == EINVAL and nt_query(two, c_rpi=0) == EINVAL         # a second level needs a first
        # two-level rows, K ranges and gathered pieces exist in the LDS-DMA kernels only: K a whole number of stages, no NO_DMA / FORCE_GENERIC
        assert nt_query(two, K=bk - ch) == EINVAL and nt_query(two, flags=G.NO_DMA) == EINVAL and nt_query(two, flags=G.FORCE_GENERIC) == EINVAL
        kr = dict(rows, k_ranges=[(0, 1)] * 5)
        assert nt_query(kr) == OK and nt_query(kr, K=bk + ch) == EINVAL and nt_query(kr, a_rpi=0) == EINVAL
        taps = NT(dt, 40, 16, 2 * bk, lda=ch, k_taps=2, k_tap_stride=bk, k_tap_stride_a=3 * bk)
        assert nt_query(taps) == OK
        assert nt_query(taps, k_tap_stride=bk + ch) == EINVAL and nt_query(taps, k_tap_stride=bk // 2, k_taps=4) == EINVAL
        assert nt_query(taps, k_tap_stride_a=3 * bk + ch // 2) == EINVAL and nt_query(taps, k_taps=3) == EINVAL
        assert nt_query(taps, k_taps=1) == EINVAL and nt_query(taps, k_taps=-1) == EINVAL and nt_query(taps, k_tap_stride=0) == EINVAL
        assert nt_query(taps, k_taps=0, k_tap_stride=0) == EINVAL                             # k_tap_stride_a without taps
        assert nt_query(taps, k_taps=0, k_tap_stride=0, k_tap_stride_a=0) == OK               # (plain overlapped rows)
        assert nt_query(taps, flags=G.FORCE_GENERIC) == EINVAL


def test_nt_krange_exact_period_and_mask_with_f32_output():
    for dt in (F32, BF16):
        bk = 8 * G.ch_of(dt)
        kr = NT(dt, 512, 256, 2 * bk, a_rpi=128, a_item=128 * 2 * bk, k_ranges=[(0, 1)] * 4, flags=G.KRANGE_EXACT)
        assert nt_query(kr) == OK
        assert nt_query(kr, a_rpi=64) == EINVAL and nt_query(kr, a_rpi=192) == EINVAL
        assert nt_query(kr, a_rpi=64, flags=0) == OK                                         # (without the flag: the union contract)
        assert nt_query(kr, a_rpi=32, a_rpi2=4, a_item2=128 * 2 * bk) == OK and nt_query(kr, a_rpi=32, a_rpi2=3, a_item2=128 * 2 * bk) == EINVAL
        # the period has to be a multiple of the tile the launcher picks: 256 with CPC_GEMM_BIG_TILE (bf16)
        assert nt_query(kr, flags=G.KRANGE_EXACT | G.BIG_TILE) == (EINVAL if dt == BF16 else OK)
        assert nt_query(kr, a_rpi=256, flags=G.KRANGE_EXACT | G.BIG_TILE) == OK
    m = NT(BF16, 40, 16, 64, mask=True)
    assert nt_query(m) == OK and nt_query(m, flags=G.OUT_F32) == EINVAL
    assert nt_query(NT(F32, 40, 16, 32, mask=True)) == OK
    from cpc_audio_amd import _hip
    s = nt_struct(m, flags=G.QUERY_EPI)
    s.A = None
    assert _hip.lib().cpc_gemm_nt(C.byref(s), C.c_void_p(0)) == EINVAL and _hip.lib().cpc_gemm_nt(None, C.c_void_p(0)) == EINVAL


def test_nt_skinny_shapes_refuse_what_the_skinny_kernel_does_not_implement():
    """f32, M = 4096, N = 32, K = 32 takes gemm_nt_skinny_f32_kernel, which knows one row level and the whole K axis: the second row
    levels and K ranges are refused as everywhere (they were accepted and ignored), and a launch that gives them completely takes the
    LDS-DMA kernel that implements them."""
    a = NT(F32, 4096, 32, 32)
    assert G.nt_path(F32, a) == "nt skinny" and nt_query(a) == OK
    assert nt_query(a, c_rpi2=4, c_item2=4096) == EINVAL                                     # no first level
    assert nt_query(a, a_rpi2=4, a_item2=4096) == EINVAL
    assert nt_query(dict(a, k_ranges=[(0, 1)])) == EINVAL                                    # K ranges need items to index
    assert nt_query(a, k_tap_stride_a=64) == EINVAL
    b = dict(a, c_rpi=64, c_item=64 * 32, c_valid=64, c_rpi2=4, c_item2=4 * 64 * 32 + 8)
    assert G.nt_path(F32, b) == "nt fast128 narrow storage" and nt_query(b) == OK
    assert nt_query(b, flags=G.FORCE_GENERIC) == EINVAL and nt_query(b, K=28) == EINVAL      # (no kernel with that row level there)
    for N in (8, 16, 32):
        for K in (4, 20, 32):
            assert G.nt_path(F32, NT(F32, 4096, N, K)) == "nt skinny"
    assert G.nt_path(F32, NT(F32, 4095, 32, 32)) != "nt skinny" and G.nt_path(F32, NT(F32, 4096, 24, 32)) != "nt skinny"
    assert G.nt_path(F32, NT(F32, 4096, 32, 36)) != "nt skinny" and G.nt_path(BF16, NT(BF16, 4096, 32, 32)) != "nt skinny"
