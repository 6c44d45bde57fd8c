"""Plain references of cpc_gemm_nt / cpc_gemm_tn (csrc/gemm.hip) at the level of the argument block of include/cpc_hip.h, the host
mirror of the launchers' kernel choice, the case lists and the data recipes.  Shared by test_gemm_kernels_gpu.py (the kernels against
these references) and test_gemm_reference_host.py (these references against torch.einsum / F.conv1d / F.conv2d /
torch.nn.grad.conv2d_weight, a float32 emulation against the bound, the metric against deliberate mistakes, the argument checks).
Nothing here touches a device.

nt_reference / tn_reference take the FLAT storage arrays (element 0 = the pointer the call passes) and the whole argument block as a
dict (NT() / TN() fill the defaults), and return a Ref: the expected flat output (positions the call must not write keep C_init), S (the
same operation on absolute values), n (the number of summed terms: NT K, + 1 with a bias; TN the rows of the element's slab, per
element) and `written`.  They work in the dtype of their inputs: float64 gives the reference, float32 the host emulation of f32
accumulation.  The bound and its ratio are conv1d_reference's (|got - ref| <= u_out |ref| + 2 (n + 2) 2^-24 S, derived there).
"""
import torch

from conv1d_reference import BF16, F32, F64, EXACT_MAX, bound, bound_ratio, gen, ints, name, normal, rounded, sparse, u_out  # noqa: F401

RELU, OUT_F32, TN_NO_TR, FORCE_GENERIC, SMALL_TILE, NARROW_EPI, NO_DMA, SKIP_PAD_ROWS = 1, 2, 4, 8, 16, 32, 64, 128
LINEAR_K, NO_PERS, DIRECT_MASK, KRANGE_EXACT = 256, 512, 1024, 2048
BIG_TILE, GENERIC_EPI, QUERY_EPI = 0x100000, 0x200000, 0x800000
NAN = float("nan")


def ch_of(dt):
    return 8 if dt == BF16 else 4


def es_of(dt):
    return 2 if dt == BF16 else 4


def round4(n):
    return (n + 3) // 4 * 4


class Ref:
    def __init__(self, out, S, n, written):
        self.out, self.S, self.n, self.written = out, S, n, written


# ------------------------------------------------------------------------------------------------------------------ argument blocks
def NT(dt, M, N, K, **kw):
    """cpc_gemm_nt_args as a dict.  bias / mask: present or not.  off*: the pointer's offset in elements from a 256-byte-aligned
    allocation (alignment is part of the launcher's choice).  k_ranges: list of (lo, hi) stage pairs or None."""
    a = dict(dt=dt, M=M, N=N, K=K, lda=K, ldb=K, ldc=round4(N), a_rpi=0, a_item=0, b_rpi=0, b_item=0, c_rpi=0, c_item=0, c_valid=0,
             a_batch=0, b_batch=0, c_batch=0, batch=1, flags=0, a_rpi2=0, a_item2=0, c_rpi2=0, c_item2=0, k_ranges=None, k_taps=0,
             k_tap_stride=0, k_tap_stride_a=0, bias=False, mask=False, bits=False, offA=0, offB=0, offC=0, off_bias=0, off_mask=0, rows=None)
    assert not set(kw) - set(a), set(kw) - set(a)
    a.update(kw)
    return a


def TN(dt, M, I, J, **kw):
    a = dict(dt=dt, M=M, I=I, J=J, lda=(I + ch_of(dt) - 1) // ch_of(dt) * ch_of(dt), ldb=J, ldc=J, a_rpi=0, a_item=0, b_rpi=0, b_item=0,
             a_batch=0, b_batch=0, c_batch=0, batch=1, nsplit=1, m_chunk=0, slab_stride=0, flags=0, c_rpi=0, c_item=0, a_rpi2=0, a_item2=0,
             offA=0, offB=0)
    assert not set(kw) - set(a), set(kw) - set(a)
    a.update(kw)
    return a


def row_off2(m, rpi, item, ld, rpi2=0, item2=0):
    """include/cpc_hip.h: rpi == 0: m ld; one level: (m / rpi) item + (m % rpi) ld; two: (m / (rpi rpi2)) item2 + ((m / rpi) % rpi2) item + (m % rpi) ld."""
    if rpi == 0:
        return m * ld
    if rpi2 == 0:
        return (m // rpi) * item + (m % rpi) * ld
    return (m // (rpi * rpi2)) * item2 + ((m // rpi) % rpi2) * item + (m % rpi) * ld


def aligned16(off, es):
    return (off * es) % 16 == 0


# ------------------------------------------------------------------------------------------------------------------ launcher mirrors
def nt_out_f32(a):
    return a["dt"] == F32 or bool(a["flags"] & OUT_F32)


def nt_choice(a):
    """launch_gemm_nt restated.  -> dict(path, tile, form) or None where the launcher returns CPC_EINVAL (its own checks; the extent
    and tap-count checks of cpc_gemm_nt, in front of it, are exercised by test_gemm_reference_host.py)."""
    dt, M, N, K, f, batch = a["dt"], a["M"], a["N"], a["K"], a["flags"], max(a["batch"], 1)      # (batch <= 0 means 1)
    ch, es = ch_of(dt), es_of(dt)
    bk = 8 * ch
    oes = 4 if nt_out_f32(a) else 2
    has_mask = a["mask"] or a["bits"]
    if M <= 0 or N <= 0 or K <= 0 or batch <= 0:
        return None
    if K % ch or a["lda"] % ch or a["ldb"] % ch or a["ldc"] % 4:
        return None
    if N % 4 and (a["bias"] or a["mask"]):
        return None
    if a["ldc"] < round4(N) and a["c_rpi"] == 0 and M > 1:
        return None
    if (a["a_rpi"] and a["a_item"] % ch) or (a["b_rpi"] and a["b_item"] % ch) or (a["c_rpi"] and a["c_item"] % 4):
        return None
    c_al = aligned16(a["offC"], oes)
    if (dt == F32 and batch == 1 and N in (8, 16, 32) and K <= 32 and not a["mask"] and a["a_rpi"] == 0 and a["b_rpi"] == 0 and M >= 4096
            and not (f & FORCE_GENERIC) and aligned16(a["offA"], es) and c_al and not a["a_rpi2"] and not a["c_rpi2"]
            and a["k_ranges"] is None and a["k_taps"] <= 1):
        return dict(path="nt skinny", tile=0, form=0)
    fast = K % bk == 0 and not (f & FORCE_GENERIC)
    banded = bool(a["a_rpi2"] or a["c_rpi2"] or a["k_ranges"] is not None)
    if banded and (not fast or (f & NO_DMA)):
        return None
    if (a["a_rpi2"] and (not a["a_rpi"] or a["a_item2"] % ch)) or (a["c_rpi2"] and (not a["c_rpi"] or a["c_item2"] % 4)) or \
            (a["k_ranges"] is not None and not a["a_rpi"]):
        return None
    big_tiles = ((M + 255) // 256) * ((N + 255) // 256)
    big = fast and dt == BF16 and N >= 256 and not (f & SMALL_TILE) and \
        ((M >= 1024 and (big_tiles >= 200 or big_tiles * batch >= 200)) or (bool(f & BIG_TILE) and M >= 256))
    k_taps, ts, tsa = a["k_taps"], a["k_tap_stride"], a["k_tap_stride_a"]
    order = "gathered" if k_taps > 1 else "storage"
    if fast and a["k_ranges"] is None and k_taps == 0 and 0 < a["lda"] < K and K % a["lda"] == 0 and a["lda"] % bk == 0 and not (f & LINEAR_K):
        k_taps, ts, order = K // a["lda"], a["lda"], "tap-innermost"
    if k_taps > 1 and (not fast or k_taps * ts != K or ts % bk or tsa % ch):
        return None
    if tsa and k_taps <= 1:
        return None
    of32 = nt_out_f32(a)
    wide = (fast and dt == BF16 and not of32 and not (f & NARROW_EPI) and N % 8 == 0 and a["ldc"] % 8 == 0 and a["c_item"] % 8 == 0 and
            a["c_item2"] % 8 == 0 and a["c_batch"] % 8 == 0 and c_al and (not a["mask"] or aligned16(a["off_mask"], es)))
    tb = 256 if big else 128
    if (f & KRANGE_EXACT) and a["k_ranges"] is not None:
        per = a["a_rpi"] * (a["a_rpi2"] if a["a_rpi2"] > 0 else 1)
        if per <= 0 or per % tb:
            return None
    dma = not (f & NO_DMA)
    epi_form = (big and dma and batch == 1 and not of32 and wide and has_mask and not a["bias"] and not (f & (RELU | GENERIC_EPI | NARROW_EPI))
                and not banded and a["b_rpi"] == 0 and a["a_rpi"] == a["c_rpi"] and (a["c_rpi"] == 0 or (a["c_rpi"] >= 32 and a["c_valid"] >= 0))
                and N % 256 == 0)
    direct = (fast and dma and dt == BF16 and wide and not (f & NO_PERS) and (not a["bias"] or aligned16(a["off_bias"], 4)) and not a["bits"]
              and (not a["mask"] or bool(f & DIRECT_MASK)))
    if a["bits"] and not (big and dma and dt == BF16 and not of32 and wide and N % 256 == 0 and a["ldc"] % 32 == 0 and a["c_item"] % 32 == 0 and
                          a["c_batch"] % 32 == 0):
        return None
    form = 0 if (not epi_form or direct) else (1 if a["bits"] else 3)
    blocks = 8 * (((M + tb - 1) // tb + 7) // 8) * ((N + tb - 1) // tb)
    if not fast:
        path = "nt generic"
    elif big:
        if of32:
            epi = "narrow"
        elif (direct and not a["mask"] and not banded and batch == 1 and 2 <= K // bk <= 16 and blocks > 512 and M % 32 == 0 and
              (a["a_rpi"] == 0 or a["a_rpi"] % 32 == 0) and a["b_rpi"] == 0 and N % 256 == 0):
            epi = "persistent"
        elif direct:
            epi = "direct"
        elif form:
            epi = "form-bits" if a["bits"] else "form-mask"
        else:
            epi = "staged" if wide else "narrow"
        path = f"nt 256 {epi}"
    else:
        path = f"nt fast128 {'direct' if direct else 'wide' if wide else 'narrow'} {order}" + ("" if dma else " no-dma")
    return dict(path=path, tile=tb, form=form)


def nt_path(dt, a):
    assert dt == a["dt"]
    c = nt_choice(a)
    return c["path"] if c else None


def tn_choice(a):
    """launch_gemm_tn (and the chunk check of cpc_gemm_tn) restated -> dict(path, tile) or None where the call returns CPC_EINVAL."""
    dt, M, I, J, f, batch = a["dt"], a["M"], a["I"], a["J"], a["flags"], max(a["batch"], 1)      # (batch <= 0 means 1)
    ch, es = ch_of(dt), es_of(dt)
    nsplit = a["nsplit"] if a["nsplit"] > 0 else 1
    of32 = dt == F32 or bool(f & OUT_F32)
    if nsplit > 1 and a["m_chunk"] % (64 if dt == BF16 else 32):
        return None
    if M <= 0 or I <= 0 or J <= 0 or batch <= 0:
        return None
    if J % ch or a["lda"] % ch or a["ldb"] % ch or a["ldc"] % 4:
        return None
    if I % ch and a["lda"] < (I + ch - 1) // ch * ch:
        return None
    if (a["a_rpi"] and a["a_item"] % ch) or (a["b_rpi"] and a["b_item"] % ch):
        return None
    if nsplit > 1 and (a["m_chunk"] <= 0 or a["m_chunk"] * nsplit < M or not of32):
        return None
    if a["c_rpi"] and (a["c_item"] % 4 or nsplit > 1):
        return None
    if a["a_rpi2"] and (not a["a_rpi"] or a["a_item2"] % ch):
        return None
    eff = a["m_chunk"] if nsplit > 1 else M
    if (dt == F32 and batch == 1 and I <= 32 and J <= 64 and I * (J // 4) <= 256 and a["c_rpi"] == 0 and a["lda"] >= round4(I) and
            not (f & FORCE_GENERIC) and not a["a_rpi2"]):
        return dict(path="tn skinny", tile=0)
    fast = dt == BF16 and not (f & (FORCE_GENERIC | TN_NO_TR)) and I % 8 == 0 and I >= 8 and J >= 8
    big = fast and I >= 256 and J >= 256 and eff >= 1024 and not (f & SMALL_TILE)
    tb = 256 if big else 128
    if not fast:
        return None if a["a_rpi2"] else dict(path="tn generic", tile=tb)
    plain = a["a_rpi"] == 0 and a["b_rpi"] == 0
    tdma = ((plain or (a["a_item"] % 8 == 0 and a["b_item"] % 8 == 0 and M < (1 << 22))) and not (f & NO_DMA) and a["lda"] % 8 == 0 and
            a["ldb"] % 8 == 0 and J % 8 == 0 and aligned16(a["offA"], es) and aligned16(a["offB"], es) and a["a_batch"] % 8 == 0 and
            a["b_batch"] % 8 == 0)
    if a["a_rpi2"] and not tdma:
        return None
    return dict(path=f"tn {'dma' if tdma else 'fast'} {'plain' if plain else 'rows'} {tb}", tile=tb)


def tn_path(dt, a):
    assert dt == a["dt"]
    c = tn_choice(a)
    return c["path"] if c else None


# ------------------------------------------------------------------------------------------------------------------ NT reference
def nt_geometry(a):
    """Element offsets: a_rows [batch][M], kmap [K] (offset of K index k within a row of A), b_rows [batch][N], c_rows [batch][M]; the
    array sizes the contract needs (last row offset + K; the output up to the last written column group)."""
    M, N, K = a["M"], a["N"], a["K"]
    z = torch.arange(a["batch"])[:, None]
    m, n, k = torch.arange(M)[None, :], torch.arange(N)[None, :], torch.arange(K)
    a_rows = z * a["a_batch"] + row_off2(m, a["a_rpi"], a["a_item"], a["lda"], a["a_rpi2"], a["a_item2"])
    b_rows = z * a["b_batch"] + row_off2(n, a["b_rpi"], a["b_item"], a["ldb"])
    c_rows = z * a["c_batch"] + row_off2(m, a["c_rpi"], a["c_item"], a["ldc"], a["c_rpi2"], a["c_item2"])
    if a["k_taps"] > 1:
        ts = a["k_tap_stride"]
        kmap = (k // ts) * (a["k_tap_stride_a"] or ts) + k % ts
    else:
        kmap = k
    return dict(a_rows=a_rows, b_rows=b_rows, c_rows=c_rows, kmap=kmap, sizeA=int(a_rows.max() + kmap.max()) + 1,
                sizeB=int(b_rows.max()) + K, sizeC=int(c_rows.max()) + round4(N))


def nt_kmask(a, own=False):
    """bool [M][K] of the K indices a row runs, or None without k_ranges.  own (or CPC_GEMM_KRANGE_EXACT): the range of the row's own
    band / item; otherwise the union over the rows of the row's tile (tile height from the launcher mirror)."""
    if a["k_ranges"] is None:
        return None
    M, K = a["M"], a["K"]
    st = 8 * ch_of(a["dt"])
    per = a["a_rpi"] * (a["a_rpi2"] if a["a_rpi2"] > 0 else 1)
    rng = torch.tensor(a["k_ranges"])
    idx = torch.arange(M) // per
    lo, hi = rng[idx, 0], rng[idx, 1]
    if not (own or a["flags"] & KRANGE_EXACT):
        tb = nt_choice(a)["tile"]
        for t0 in range(0, M, tb):
            lo[t0:t0 + tb], hi[t0:t0 + tb] = lo[t0:t0 + tb].min(), hi[t0:t0 + tb].max()
    k = torch.arange(K)[None, :]
    return (k >= lo[:, None] * st) & (k < hi[:, None] * st)


def nt_readable(a):
    """bool masks over A, Bt and the mask array (sized as nt_geometry says): the elements the contract lets the call read."""
    g = nt_geometry(a)
    km = nt_kmask(a) if a["flags"] & KRANGE_EXACT else None
    ra, rb, rm = torch.zeros(g["sizeA"], dtype=torch.bool), torch.zeros(g["sizeB"], dtype=torch.bool), torch.zeros(g["sizeC"], dtype=torch.bool)
    for z in range(a["batch"]):
        ia = g["a_rows"][z][:, None] + g["kmap"][None, :]
        ra[ia[km] if km is not None else ia.reshape(-1)] = True
        rb[(g["b_rows"][z][:, None] + torch.arange(a["K"])[None, :]).reshape(-1)] = True
        rm[(g["c_rows"][z][:, None] + torch.arange(a["N"])[None, :]).reshape(-1)] = True
    return ra, rb, rm


def nt_reference(a, A, Bt, bias, mask, C_init, mut=None):
    """The call on flat arrays.  a['rows']: compute (and mark written) these rows only.  mut: a deliberate mistake (NT_MUTANTS)."""
    M, N, K, f = a["M"], a["N"], a["K"], a["flags"]
    g = nt_geometry(a)
    km = nt_kmask(a)
    rows = torch.arange(M) if a["rows"] is None else a["rows"]
    N4 = round4(N) if (a["ldc"] >= round4(N) or M == 1) else N
    out, S = C_init.clone(), torch.zeros_like(C_init)
    written = torch.zeros(C_init.numel(), dtype=torch.bool)
    kk, nn = torch.arange(K)[None, :], torch.arange(N4)[None, :]
    a_rpi = a["a_rpi"]
    c_valid = a["c_valid"] + (1 if mut == "c_valid_off" else 0)
    for z in range(a["batch"]):
        a_rows = g["a_rows"][z][rows]
        if mut == "item_row_off" and a_rpi:          # rows of every item but the first start one row early
            a_rows = a_rows - (rows >= a_rpi) * a["lda"]
        ar = A[a_rows[:, None] + g["kmap"][None, :]]
        if km is not None:
            ar = torch.where(km[rows], ar, torch.zeros_like(ar))
        b_rows = g["b_rows"][0] + z * (a["a_batch"] if mut == "a_batch_for_b" else a["b_batch"])
        br = Bt[(b_rows[:, None] + kk).clamp_max(Bt.numel() - 1)]
        if mut == "drop_last_k":                     # one row loses its last K element: the first row where that changes something
            hit = ((ar[:, K - 1].abs() > 0) & ((rows % a["c_rpi"]) < a["c_valid"] if a["c_rpi"] else True)).nonzero()
            if hit.numel():
                ar = ar.clone()
                ar[hit[0, 0], K - 1] = 0
        acc, Sacc = ar @ br.T + 0.0, ar.abs() @ br.abs().T        # (+ 0.0: an accumulator that starts at +0 never ends at -0; host BLAS may)
        if mut == "drop_last_chunk":                 # the last 16-byte chunk of K in the last N tile (128 columns)
            c, n0 = ch_of(a["dt"]), (N - 1) // 128 * 128
            acc[:, n0:] -= ar[:, K - c:] @ br[n0:, K - c:].T
        if bias is not None:
            acc = acc + (torch.roll(bias, 1) if mut == "bias_shift" else bias)
            Sacc = Sacc + bias.abs()
        if f & RELU:
            acc = torch.where(acc > 0, acc, torch.zeros_like(acc))
        idx = g["c_rows"][z][rows][:, None] + nn
        vals, Sv = torch.zeros(len(rows), N4, dtype=A.dtype), torch.zeros(len(rows), N4, dtype=A.dtype)
        vals[:, :N], Sv[:, :N] = acc, Sacc
        if mask is not None:
            mk = mask[idx[:, :N]]
            keep = (mk >= 0) if mut == "mask_ge" else (mk > 0)
            vals[:, :N], Sv[:, :N] = torch.where(keep, vals[:, :N], torch.zeros_like(mk)), Sv[:, :N] * keep
        valid = torch.ones(len(rows), dtype=torch.bool) if a["c_rpi"] == 0 else (rows % a["c_rpi"]) < c_valid
        if mut != "pad_not_zeroed":
            vals, Sv = torch.where(valid[:, None], vals, torch.zeros_like(vals)), Sv * valid[:, None]
        if (f & SKIP_PAD_ROWS) and mut != "skip_written":
            idx, vals, Sv = idx[valid], vals[valid], Sv[valid]
        out[idx.reshape(-1)], S[idx.reshape(-1)], written[idx.reshape(-1)] = vals.reshape(-1), Sv.reshape(-1), True
    return Ref(out, S, K + (1 if bias is not None else 0), written)


NT_MUTANTS = ["drop_last_k", "drop_last_chunk", "bias_shift", "item_row_off", "a_batch_for_b", "mask_ge", "pad_not_zeroed", "c_valid_off",
              "skip_written"]


def nt_mutant_applies(mut, a):
    pad = a["c_rpi"] > 0 and a["c_valid"] < a["c_rpi"] and a["M"] > a["c_valid"]
    some = not (a["c_rpi"] and a["c_valid"] <= 0)          # (some row is not a pad row)
    return {"drop_last_k": some, "drop_last_chunk": some, "bias_shift": a["bias"] and some,
            "item_row_off": a["a_rpi"] > 0 and a["M"] > a["a_rpi"] and some,
            "a_batch_for_b": a["batch"] > 1 and a["a_batch"] != a["b_batch"] and some, "mask_ge": (a["mask"] or a["bits"]) and some,
            "pad_not_zeroed": pad and not (a["flags"] & SKIP_PAD_ROWS), "c_valid_off": pad, "skip_written": pad and bool(a["flags"] & SKIP_PAD_ROWS)}[mut]


# ------------------------------------------------------------------------------------------------------------------ TN reference
def tn_geometry(a):
    M, I, J = a["M"], a["I"], a["J"]
    z, m = torch.arange(a["batch"])[:, None], torch.arange(M)[None, :]
    a_rows = z * a["a_batch"] + row_off2(m, a["a_rpi"], a["a_item"], a["lda"], a["a_rpi2"], a["a_item2"])
    b_rows = z * a["b_batch"] + row_off2(m, a["b_rpi"], a["b_item"], a["ldb"])
    nsplit = max(a["nsplit"], 1)
    c_rows = row_off2(torch.arange(I), a["c_rpi"], a["c_item"], a["ldc"])
    ch = ch_of(a["dt"])
    return dict(a_rows=a_rows, b_rows=b_rows, c_rows=c_rows, sizeA=int(a_rows.max()) + (I + ch - 1) // ch * ch, sizeB=int(b_rows.max()) + J,
                sizeC=(a["batch"] - 1) * a["c_batch"] + (nsplit - 1) * a["slab_stride"] + int(c_rows.max()) + J)


def tn_readable(a):
    """A: the I columns of every row, rounded up to whole 16-byte chunks (ragged I: the header wants padded rows); B: the J columns."""
    g = tn_geometry(a)
    ch = ch_of(a["dt"])
    ra, rb = torch.zeros(g["sizeA"], dtype=torch.bool), torch.zeros(g["sizeB"], dtype=torch.bool)
    ra[(g["a_rows"].reshape(-1, 1) + torch.arange((a["I"] + ch - 1) // ch * ch)[None, :]).reshape(-1)] = True
    rb[(g["b_rows"].reshape(-1, 1) + torch.arange(a["J"])[None, :]).reshape(-1)] = True
    return ra, rb


def tn_reference(a, A, B, C_init, mut=None):
    """Slab s = rows [s m_chunk, min(M, (s + 1) m_chunk)) at C + s slab_stride (an empty chunk gives a zero slab); nsplit <= 1: all rows."""
    M, I, J = a["M"], a["I"], a["J"]
    g = tn_geometry(a)
    nsplit = max(a["nsplit"], 1)
    chunk = a["m_chunk"] if nsplit > 1 else M
    blk = 64 if a["dt"] == BF16 else 32
    out, S = C_init.clone(), torch.zeros_like(C_init)
    n = torch.zeros(C_init.numel(), dtype=torch.float64)
    written = torch.zeros(C_init.numel(), dtype=torch.bool)
    c_rows = torch.arange(I) * a["ldc"] if mut == "c_item_ignored" else g["c_rows"]
    for z in range(a["batch"]):
        for s in range(nsplit):
            lo, hi = min(M, s * chunk), min(M, (s + 1) * chunk)
            if mut == "boundary_row" and s > 0 and lo < hi:       # the first row of a chunk goes to the slab before it
                lo += 1
            if mut == "boundary_row" and s + 1 < nsplit and hi < M:
                hi += 1
            if mut == "drop_ragged_stage" and (hi - lo) % blk:   # the last, partial stage of the chunk is lost
                hi -= (hi - lo) % blk
            ar = A[g["a_rows"][z][lo:hi, None] + torch.arange(I)[None, :]]
            br = B[g["b_rows"][z][lo:hi, None] + torch.arange(J)[None, :]]
            idx = (z * a["c_batch"] + s * a["slab_stride"] + c_rows[:, None] + torch.arange(J)[None, :]).reshape(-1)
            out[idx], S[idx], n[idx], written[idx] = (ar.T @ br + 0.0).reshape(-1), (ar.abs().T @ br.abs()).reshape(-1), float(hi - lo), True
    return Ref(out, S, n, written)


TN_MUTANTS = ["drop_ragged_stage", "boundary_row", "c_item_ignored"]


def tn_mutant_applies(mut, a):
    nsplit = max(a["nsplit"], 1)
    chunk = a["m_chunk"] if nsplit > 1 else a["M"]
    blk = 64 if a["dt"] == BF16 else 32
    sizes = [min(a["M"], (s + 1) * chunk) - min(a["M"], s * chunk) for s in range(nsplit)]
    return {"drop_ragged_stage": any(r % blk for r in sizes), "boundary_row": nsplit > 1 and sizes[1] > 0,
            "c_item_ignored": a["c_rpi"] > 0 and a["I"] > a["c_rpi"] and a["c_item"] != a["c_rpi"] * a["ldc"]}[mut]


# ------------------------------------------------------------------------------------------------------------------ judgement
def out_dtype(a):
    return F32 if (a["dt"] == F32 or a["flags"] & OUT_F32) else BF16


def truncated_bf16(t):
    """bf16 by truncation instead of round-to-nearest-even (the deliberate mistake)."""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).double()


def judge(got, ref, odt, exact, checked=None):
    """The whole flat output against a Ref.  Elements the call must not write must still be NaN (inf otherwise); written ones within
    the bound (the ratio is returned) or, for exact data, bit for bit the reference as stored in odt, the sign of zeros included (0 or inf).  checked: judge these
    written elements only (the one launch whose reference covers a subset of the rows)."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    w = ref.written if checked is None else checked
    if checked is None and not bool(torch.isnan(got[~ref.written]).all()):
        return float("inf")
    if exact:          # the stored bit patterns: every zero the call writes (pad rows, masked elements, pad columns) is +0.0
        same = torch.equal(got[w].float().view(torch.int32), ref.out[w].to(odt).float().view(torch.int32))
        return 0.0 if same else float("inf")
    n = ref.n[w] if torch.is_tensor(ref.n) else ref.n
    return bound_ratio(got[w], ref.out[w].double(), ref.S[w].double(), n, u_out(odt))


# ------------------------------------------------------------------------------------------------------------------ data
def mask_values(g, shape, dt, exact):
    """Beside normal values (integers for the twins): +0.0, -0.0, the smallest positive value of the storage type, negative values."""
    m = ints(g, -1, 2, *shape) if exact else rounded(normal(g, *shape), dt)
    tiny = 2.0 ** -133 if dt == BF16 else 2.0 ** -149
    sel = torch.randint(0, 8, shape, generator=g)
    m = torch.where(sel == 0, torch.zeros_like(m), m)
    m = torch.where(sel == 1, torch.full_like(m, -0.0), m)
    return torch.where(sel == 2, torch.full_like(m, tiny), m)


def nt_data(a, exact, seed=0):
    """float64 arrays exact in the storage type: A, Bt, bias (f32-exact) or None, mask or None; and read_A / read_Bt / read_mask, the
    elements the contract lets the call read (device_copy puts NaN everywhere else).  Without CPC_GEMM_KRANGE_EXACT, A is zero outside each row's own
    K range (that contract's precondition; k_ranges cases have no overlapping rows)."""
    dt, K = a["dt"], a["K"]
    geo = nt_geometry(a)
    g = gen(seed + a["M"] * 7 + a["N"] * 13 + K + (5 if exact else 0))
    if exact:
        A = ints(g, -2, 2, geo["sizeA"])
        Bt = sparse(g, ints(g, -1, 1, geo["sizeB"]), min(1.0, 40.0 / K))
        Bt[(geo["b_rows"] + K - 1).reshape(-1)] = 1.0          # (the last K element of every row counts: a kernel that drops it shows)
        bias = ints(g, -2, 2, a["N"]) if a["bias"] else None
    else:
        A = rounded(normal(g, geo["sizeA"]), dt)
        Bt = rounded(normal(g, geo["sizeB"]), dt)
        bias = (normal(g, a["N"]) * 2).float().double() if a["bias"] else None
    mask = mask_values(g, (geo["sizeC"],), dt, exact) if (a["mask"] or a["bits"]) else None
    if a["k_ranges"] is not None and not a["flags"] & KRANGE_EXACT:
        own = nt_kmask(a, own=True)
        for z in range(a["batch"]):
            ia = geo["a_rows"][z][:, None] + geo["kmap"][None, :]
            A[ia[~own]] = 0
    ra, rb, rm = nt_readable(a)
    return dict(A=A, Bt=Bt, bias=bias, mask=mask, read_A=ra, read_Bt=rb, read_mask=rm, sizeC=geo["sizeC"])


def device_copy(d, key):
    """The array as the device gets it: NaN at every element the contract does not let the call read."""
    return torch.where(d["read_" + key], d[key], torch.full((1,), NAN, dtype=F64))


def tn_data(a, exact, seed=0):
    dt = a["dt"]
    geo = tn_geometry(a)
    nsplit = max(a["nsplit"], 1)
    rows = a["m_chunk"] if nsplit > 1 else a["M"]
    g = gen(seed + a["M"] * 7 + a["I"] * 13 + a["J"] + (5 if exact else 0))
    if exact:
        A = ints(g, -2, 2, geo["sizeA"])
        B = sparse(g, ints(g, -1, 1, geo["sizeB"]), min(1.0, 40.0 / rows))
    else:
        A, B = rounded(normal(g, geo["sizeA"]), dt), rounded(normal(g, geo["sizeB"]), dt)
    ra, rb = tn_readable(a)
    return dict(A=A, B=B, read_A=ra, read_B=rb, sizeC=geo["sizeC"])


def nt_run_reference(a, d, dtype=F64, mut=None):
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    return nt_reference(a, cast(d["A"]), cast(d["Bt"]), cast(d["bias"]), cast(d["mask"]), torch.full((d["sizeC"],), NAN, dtype=dtype), mut)


def tn_run_reference(a, d, dtype=F64, mut=None):
    return tn_reference(a, d["A"].to(dtype), d["B"].to(dtype), torch.full((d["sizeC"],), NAN, dtype=dtype), mut)


# ------------------------------------------------------------------------------------------------------------------ cases
PERSIST_M = 256 * 513 + 32


def persist_rows(a):
    """The rows the persistent launch is judged on: a seeded subset (first / last rows, the rows around the 256-row edges of the first
    and last tile, 2048 random ones) plus every pad row."""
    M = a["M"]
    last = (M - 1) // 256 * 256
    fixed = torch.tensor([0, 1, 255, 256, 257, last - 1, last, M - 2, M - 1])
    rows = torch.cat([fixed, torch.randperm(M, generator=gen(11))[:2048]])
    if a["c_rpi"]:
        m = torch.arange(M)
        rows = torch.cat([rows, m[(m % a["c_rpi"]) >= a["c_valid"]]])
    return torch.unique(rows)


def nt_cases():
    """[(id, args)].  ch = 8 bf16 / 4 f32 elements (16 bytes), bk = 8 ch (one K stage), tile 128 (256 with CPC_GEMM_BIG_TILE)."""
    cases = []
    for dt in (F32, BF16):
        ch = ch_of(dt)
        bk, tag = 8 * ch, name(dt)

        def add(cid, M, N, K, **kw):
            cases.append((f"{tag}-{cid}", NT(dt, M, N, K, **kw)))

        # M x K x N edges on the fast and generic kernels; bias / relu; ldc > N; lda > K
        add("M129-N132-K3bk-bias-relu", 129, 132, 3 * bk, bias=True, flags=RELU, ldc=140)
        add("M127-N136-Kbk-bias", 127, 136, bk, bias=True)
        add("M128-N128-Kbk+ch-mask", 128, 128, bk + ch, mask=True, bias=True, lda=bk + 3 * ch)
        add("M1-N6-Kch", 1, 6, ch, ldc=8)
        add("M1-N128-Kbk", 1, 128, bk, bias=True)
        add("M128-N128-Kbk-mask", 128, 128, bk, mask=True, bias=True, lda=bk + 3 * ch)
        add("M127-N12-Kbk+ch", 127, 12, bk + ch, bias=True)
        add("M33-N132-Kbk+ch", 33, 132, bk + ch, bias=True, ldc=140)
        add("M129-N12-Kbk+ch-relu", 129, 12, bk + ch, bias=True, flags=RELU)
        add("M17-N130-Kbk", 17, 130, bk, ldc=136, flags=RELU)
        add("M17-N12-Kbk-ch", 17, 12, bk - ch, lda=bk + ch, bias=True)
        add("M17-N10-K3bk-generic", 17, 10, 3 * bk, flags=FORCE_GENERIC)
        add("M17-N64-Kbk-nopers", 17, 64, bk, flags=NO_PERS, bias=True)
        add("M17-N64-Kbk-bias-unaligned", 17, 64, bk, bias=True, off_bias=1)
        add("M17-N64-Kbk-C-unaligned", 17, 64, bk, offC=4 if dt == BF16 else 2, bias=True, ldc=72)
        add("M40-N64-Kbk-mask-unaligned", 40, 64, bk, mask=True, off_mask=4 if dt == BF16 else 2)
        add("M40-N64-Kbk-mask", 40, 64, bk, mask=True, flags=RELU, bias=True)
        add("M40-N64-Kbk-direct-mask", 40, 64, bk, mask=True, flags=DIRECT_MASK)
        add("M130-N64-K3bk-nodma", 130, 64, 3 * bk, flags=NO_DMA, bias=True)
        add("M130-N64-K3bk-narrow", 130, 64, 3 * bk, flags=NARROW_EPI, bias=True)
        # overlapped rows (lda < K): tap-innermost and, forced, storage order
        add("M130-N24-lda<K-taps", 130, 24, 3 * bk, lda=bk)
        add("M130-N24-lda<K-linear", 130, 24, 3 * bk, lda=bk, flags=LINEAR_K)
        add("M33-N24-lda<K-generic", 33, 24, 3 * ch, lda=ch)
        # windows: A and C items differ; B rows in items
        add("M40-arpi10-crpi5", 40, 24, bk, a_rpi=10, a_item=13 * bk + ch, c_rpi=5, c_item=6 * 32 + 4, c_valid=3, ldc=32, bias=True)
        add("M40-arpi10-crpi5-generic", 40, 24, bk + ch, a_rpi=10, a_item=13 * (bk + ch), c_rpi=5, c_item=6 * 32 + 4, c_valid=3, ldc=32)
        add("M17-N24-brpi3", 17, 24, bk, b_rpi=3, b_item=4 * bk + ch, bias=True)
        add("M17-N24-brpi3-generic", 17, 24, bk - ch, b_rpi=3, b_item=4 * bk)
        # pad rows: c_valid in {0, 1, rpi}, zeroed or skipped, on the fast and the generic kernel
        for K in (bk, bk + ch):
            for cv in (0, 1, 8):
                for skip in (0, SKIP_PAD_ROWS):
                    add(f"crpi8-valid{cv}-skip{int(bool(skip))}-K{K}", 26, 16, K, c_rpi=8, c_item=9 * 16, c_valid=cv, ldc=16,
                        flags=skip, bias=True, a_rpi=8, a_item=8 * (bk + 2 * ch) + ch, lda=bk + 2 * ch)
        add("crpi8-valid5-mask-skip", 26, 16, bk, c_rpi=8, c_item=9 * 16, c_valid=5, ldc=16, flags=SKIP_PAD_ROWS, mask=True)
        add("crpi8-valid5-mask", 26, 16, bk, c_rpi=8, c_item=9 * 16, c_valid=5, ldc=16, mask=True)
        # batches with distinct strides, the mask through c_batch
        for K in (bk, bk + ch):
            add(f"batch3-K{K}", 33, 24, K, batch=3, a_batch=33 * K + 2 * ch, b_batch=24 * K + ch, c_batch=33 * 24 + 8, mask=True, bias=True)
        add("batch1-explicit", 33, 24, bk, batch=1, a_batch=8, b_batch=8, c_batch=8)
        # second row level with K ranges: union contract (zero cuts) and exact contract (period = the tile)
        add("two-level-kranges", 200, 24, 4 * bk, a_rpi=8, a_item=9 * 4 * bk, a_rpi2=3, a_item2=30 * 4 * bk, c_rpi=8, c_item=9 * 24 + 4, c_valid=7,
            c_rpi2=3, c_item2=31 * 24, ldc=24, k_ranges=[(0, 2), (1, 3), (0, 1), (1, 2), (0, 3), (2, 3), (2, 4), (3, 4), (2, 4)], bias=True)
        add("two-level-kranges-exact", 384, 24, 4 * bk, a_rpi=16, a_item=17 * 4 * bk, a_rpi2=8, a_item2=8 * 17 * 4 * bk + ch, c_rpi=16,
            c_item=16 * 24, c_valid=16, c_rpi2=8, c_item2=130 * 24, ldc=24, k_ranges=[(0, 2), (1, 4), (2, 3)], flags=KRANGE_EXACT)
        add("items-kranges-exact", 256, 16, 3 * bk, a_rpi=128, a_item=130 * 3 * bk, k_ranges=[(1, 3), (0, 1)], flags=KRANGE_EXACT)
        # what the grid convolutions launch: mask + two-level rows + gathered pieces + exact K ranges + skipped pad rows
        add("grid-conv-combo", 256, 136, 4 * bk, lda=5 * bk, a_rpi=16, a_item=16 * 5 * bk + ch, a_rpi2=8, a_item2=8 * (16 * 5 * bk + ch) + ch,
            c_rpi=16, c_item=16 * 136, c_valid=14, c_rpi2=8, c_item2=8 * 16 * 136 + 8, ldc=136, k_taps=2, k_tap_stride=2 * bk,
            k_tap_stride_a=3 * bk, k_ranges=[(1, 4), (0, 3)], mask=True, flags=KRANGE_EXACT | SKIP_PAD_ROWS)
        # rows gathered from a grid: 3 pieces of one stage, pieces 2 bk + ch apart in A; with K ranges on top
        add("gathered-taps", 40, 24, 3 * bk, lda=ch, k_taps=3, k_tap_stride=bk, k_tap_stride_a=2 * bk + ch, bias=True)
        add("gathered-taps-kranges-exact", 256, 24, 4 * bk, lda=5 * bk, a_rpi=128, a_item=128 * 5 * bk + ch, k_taps=2, k_tap_stride=2 * bk,
            k_tap_stride_a=3 * bk, k_ranges=[(1, 4), (0, 3)], flags=KRANGE_EXACT)
    # f32 only: the skinny kernel, and the skinny shape with a second output row level (the fast kernel: the skinny one has no such rows)
    for N, K in ((8, 4), (16, 20), (32, 32)):
        cases.append((f"f32-skinny-N{N}-K{K}", NT(F32, 4096, N, K, bias=True, flags=RELU, c_rpi=64, c_item=64 * N + 4, c_valid=60, lda=K + 4)))
    cases.append(("f32-skinny-N32-K32-skip", NT(F32, 4099, 32, 32, c_rpi=64, c_item=64 * 40, c_valid=1, ldc=40, flags=SKIP_PAD_ROWS)))
    cases.append(("f32-skinny-shape-crpi2", NT(F32, 4096, 32, 32, c_rpi=64, c_item=64 * 32 + 4, c_valid=60, c_rpi2=4, c_item2=4 * (64 * 32 + 4) + 8,
                                                bias=True)))
    cases.append(("f32-skinny-shape-A-unaligned", NT(F32, 4096, 8, 4, offA=2, bias=True)))
    # bf16 only: f32 output; the 256 x 256 family at M = 300 .. 600; the persistent kernel
    cases.append(("bf16-outf32-fast", NT(BF16, 129, 20, 64, flags=OUT_F32, bias=True, ldc=24)))
    cases.append(("bf16-outf32-N-ragged", NT(BF16, 33, 18, 64, flags=OUT_F32, ldc=20)))
    cases.append(("bf16-outf32-generic", NT(BF16, 33, 20, 72, flags=OUT_F32, bias=True)))
    cases.append(("bf16-256-direct", NT(BF16, 300, 256, 128, flags=BIG_TILE, bias=True)))
    cases.append(("bf16-256-direct-M256", NT(BF16, 256, 256, 64, flags=BIG_TILE)))
    cases.append(("bf16-256-direct-2N", NT(BF16, 257, 264, 64, flags=BIG_TILE | RELU, bias=True)))
    cases.append(("bf16-256-staged", NT(BF16, 513, 264, 128, flags=BIG_TILE | NO_PERS, bias=True, ldc=272)))
    cases.append(("bf16-256-staged-mask-crpi", NT(BF16, 600, 256, 64, flags=BIG_TILE, mask=True, bias=True, a_rpi=100, a_item=128 * 64, c_rpi=100,
                                                  c_item=128 * 256, c_valid=90)))
    cases.append(("bf16-256-form-mask", NT(BF16, 600, 256, 128, flags=BIG_TILE, mask=True, a_rpi=100, a_item=128 * 128, c_rpi=100, c_item=128 * 256,
                                           c_valid=90)))
    cases.append(("bf16-256-form-mask-skip", NT(BF16, 300, 512, 64, flags=BIG_TILE | SKIP_PAD_ROWS, mask=True, a_rpi=100, a_item=128 * 64, c_rpi=100,
                                                c_item=128 * 512, c_valid=90)))
    cases.append(("bf16-256-narrow-outf32", NT(BF16, 300, 260, 64, flags=BIG_TILE | OUT_F32, bias=True)))
    cases.append(("bf16-256-narrow-N260", NT(BF16, 300, 260, 64, flags=BIG_TILE, bias=True)))
    # the 256 x 256 tile with everything else it accepts
    big = lambda cid, M, N, K, flags=0, **kw: cases.append((f"bf16-256-{cid}", NT(BF16, M, N, K, flags=BIG_TILE | flags, **kw)))  # noqa: E731
    big("batch3", 300, 256, 64, batch=3, a_batch=300 * 64 + 16, b_batch=256 * 64 + 8, c_batch=300 * 256 + 8, mask=True, bias=True)
    big("brpi-lda>K", 300, 264, 64, b_rpi=100, b_item=101 * 64 + 8, bias=True, lda=72)
    big("arpi100-crpi50", 300, 256, 64, a_rpi=100, a_item=128 * 64 + 8, c_rpi=50, c_item=51 * 256, c_valid=47, bias=True)
    big("lda<K-taps", 300, 256, 192, lda=64, bias=True)
    big("lda<K-linear", 300, 256, 192, LINEAR_K, lda=64, bias=True)
    big("two-level-kranges", 600, 256, 256, a_rpi=8, a_item=9 * 256, a_rpi2=3, a_item2=30 * 256, c_rpi=8, c_item=9 * 256, c_valid=7, c_rpi2=3,
        c_item2=31 * 256, k_ranges=[(i % 3, i % 3 + 1 + i % 2) for i in range(25)], mask=True)
    big("two-level-kranges-exact", 512, 256, 256, KRANGE_EXACT, a_rpi=32, a_item=33 * 256, a_rpi2=8, a_item2=8 * 33 * 256 + 8, c_rpi=32,
        c_item=32 * 256, c_valid=32, c_rpi2=8, c_item2=8 * 32 * 256 + 256, k_ranges=[(1, 4), (0, 3)], bias=True)
    big("gathered-taps", 300, 256, 128, lda=8, k_taps=2, k_tap_stride=64, k_tap_stride_a=136, bias=True)
    big("grid-conv-combo", 512, 256, 256, KRANGE_EXACT | SKIP_PAD_ROWS, lda=320, a_rpi=32, a_item=32 * 320 + 8, a_rpi2=8,
        a_item2=8 * (32 * 320 + 8) + 8, c_rpi=32, c_item=32 * 256, c_valid=30, c_rpi2=8, c_item2=8 * 32 * 256 + 256, k_taps=2, k_tap_stride=128,
        k_tap_stride_a=192, k_ranges=[(1, 4), (0, 3)], mask=True)
    big("N258", 300, 258, 64, ldc=264)
    big("bias-unaligned", 300, 256, 64, bias=True, off_bias=1)
    big("C-unaligned", 300, 256, 64, bias=True, offC=4)
    big("mask-unaligned", 300, 256, 64, mask=True, off_mask=4)
    cases.append(("bf16-256-form-bits", NT(BF16, 600, 256, 128, flags=BIG_TILE, bits=True, a_rpi=100, a_item=128 * 128, c_rpi=100, c_item=128 * 256,
                                           c_valid=90)))
    a = NT(BF16, PERSIST_M, 256, 128, bias=True, flags=RELU, a_rpi=160, a_item=160 * 128, c_rpi=160, c_item=160 * 256, c_valid=150)
    a["rows"] = persist_rows(a)
    cases.append(("bf16-256-persistent", a))
    # its twin with K = 192: nk = 3 stages, so every second tile of a workgroup starts on the other LDS slot (the odd-stage tile change)
    a = NT(BF16, PERSIST_M, 256, 192, bias=True, flags=RELU, a_rpi=160, a_item=160 * 192, c_rpi=160, c_item=160 * 256, c_valid=150)
    a["rows"] = persist_rows(a)
    cases.append(("bf16-256-persistent-K192", a))
    return cases


def tn_cases():
    """[(id, args)].  blk = 64 bf16 / 32 f32 rows (one stage).  bf16 items are always multiples of 8 elements (the launcher wants whole
    16-byte chunks), so the item-addressed NON-DMA kernel is reached through CPC_GEMM_NO_DMA and through an unaligned pointer; f32 items
    that are no multiple of 8 run on the generic kernel."""
    cases = []
    for dt in (F32, BF16):
        ch, blk, tag = ch_of(dt), (64 if dt == BF16 else 32), name(dt)

        def add(cid, M, I, J, **kw):
            cases.append((f"{tag}-{cid}", TN(dt, M, I, J, **kw)))

        for M in (1, blk - 1, blk, blk + 1, 3 * blk + 5):
            add(f"M{M}-I16-J24", M, 16, 24, flags=OUT_F32)                   # f32: skinny; bf16: DMA plain
            add(f"M{M}-I40-J72", M, 40, 72, flags=OUT_F32, ldc=80)           # f32: generic (beyond the skinny bounds)
        for nsplit, chunk in ((3, 2 * blk), (5, blk)):
            for I, J in ((16, 24), (40, 136)):
                add(f"split{nsplit}-I{I}-J{J}", 3 * blk + 5, I, J, nsplit=nsplit, m_chunk=chunk, slab_stride=I * J + 8, flags=OUT_F32)
        add("rows-items8", 70, 16, 24, a_rpi=7, a_item=8 * 16 + 8, b_rpi=10, b_item=11 * 24 + 8, flags=OUT_F32, nsplit=3, m_chunk=blk,
            slab_stride=16 * 24)
        add("rows-items-odd", 70, 40, 72, a_rpi=7, a_item=8 * 40 + ch, b_rpi=10, b_item=11 * 72 + ch, flags=OUT_F32)
        add("rows-nodma", 70, 16, 24, a_rpi=7, a_item=8 * 16 + 8, b_rpi=10, b_item=11 * 24 + 8, flags=OUT_F32 | NO_DMA)
        add("A-unaligned", 70, 16, 24, offA=ch // 2, flags=OUT_F32, ldc=28)
        add("B-unaligned-rows", 70, 40, 72, offB=ch // 2, a_rpi=7, a_item=8 * 40, flags=OUT_F32)
        add("batch3", 70, 40, 72, batch=3, a_batch=70 * 40 + 8, b_batch=70 * 72 + 16, c_batch=40 * 72 + 4, flags=OUT_F32)
        add("crpi", 70, 40, 72, c_rpi=8, c_item=9 * 72 + 4, flags=OUT_F32)
        add("ragged-I13", 70, 13, 24, flags=OUT_F32 | FORCE_GENERIC)
        add("ragged-I45", 2 * blk + 1, 45, 72, flags=OUT_F32, nsplit=3, m_chunk=blk, slab_stride=45 * 72)
    cases.append(("bf16-out-bf16", TN(BF16, 70, 40, 72)))
    cases.append(("bf16-out-bf16-generic-crpi", TN(BF16, 70, 13, 24, c_rpi=4, c_item=5 * 24)))
    cases.append(("bf16-no-tr", TN(BF16, 133, 40, 72, flags=OUT_F32 | TN_NO_TR)))
    cases.append(("bf16-two-level", TN(BF16, 150, 16, 24, a_rpi=4, a_item=5 * 16, a_rpi2=3, a_item2=20 * 16 + 8, b_rpi=12, b_item=13 * 24 + 8,
                                       flags=OUT_F32, nsplit=3, m_chunk=64, slab_stride=16 * 24, batch=2, a_batch=16, b_batch=0, c_batch=3 * 16 * 24)))
    cases.append(("f32-skinny-bound", TN(F32, 100, 16, 64, nsplit=5, m_chunk=32, slab_stride=16 * 64 + 4)))
    cases.append(("f32-beyond-skinny", TN(F32, 100, 20, 64, nsplit=5, m_chunk=32, slab_stride=20 * 64 + 4)))
    cases.append(("f32-skinny-ragged-I", TN(F32, 100, 31, 8, a_rpi=9, a_item=10 * 32 + 4)))
    for I, J in ((256, 264), (264, 256)):
        cases.append((f"bf16-256-I{I}-J{J}", TN(BF16, 1024 + 5, I, J, flags=OUT_F32)))
    cases.append(("bf16-256-split", TN(BF16, 2048 + 70, 256, 256, flags=OUT_F32, nsplit=3, m_chunk=1024, slab_stride=256 * 256)))
    cases.append(("bf16-256-small-tile", TN(BF16, 1024 + 5, 256, 264, flags=OUT_F32 | SMALL_TILE)))
    return cases


NT_PATHS = ["nt skinny", "nt generic", "nt fast128 wide storage", "nt fast128 narrow storage", "nt fast128 direct storage",
            "nt fast128 direct tap-innermost", "nt fast128 narrow tap-innermost", "nt fast128 direct gathered", "nt fast128 wide gathered", "nt fast128 narrow gathered",
            "nt fast128 wide storage no-dma", "nt fast128 narrow storage no-dma", "nt 256 staged", "nt 256 direct", "nt 256 persistent",
            "nt 256 form-mask", "nt 256 form-bits", "nt 256 narrow"]
TN_PATHS = ["tn skinny", "tn generic", "tn fast plain 128", "tn fast rows 128", "tn dma plain 128", "tn dma rows 128", "tn dma plain 256"]


def group(path):
    """The kernel behind a path label (the groups the ratios are recorded by)."""
    return " ".join(path.split()[:2])
