"""cpc_gemm_nt / cpc_gemm_tn / cpc_gemm_nt_bits (csrc/gemm.hip) at their edges, every kernel body the launchers can pick, each launch
against a plain float64 reference of the same call at the level of the argument block (tests/gemm_reference.py;
test_gemm_reference_host.py checks those references against torch.einsum / F.conv1d / F.conv2d / conv2d_weight, shows that the metric
used here rejects deliberate mistakes, and holds the argument checks of cpc_gemm_nt).  The older tests of the GEMMs (test_hip_kernels.py,
test_dgrad_epilogue_gpu.py) keep the large shapes and the whole-tensor measure.

Conventions (those of test_conv1d_kernels_gpu.py).  Device inputs are the reference's inputs rounded to the storage type.  Every output
buffer starts as NaN and is followed by sentinels that must be intact afterwards.  Every input element the contract does not let the call
read is NaN: lda - K padding, the rows between items, everything behind last_row_offset + K (a_extent / b_extent are passed exactly),
the elements in front of an unaligned pointer, K outside a row's range under CPC_GEMM_KRANGE_EXACT (without the flag the data is ZERO
outside each row's own range: that contract's precondition), mask elements outside the M x N rows.  The whole flat output is compared:
written elements against the bound (the exact-data twins: the reference's stored bit pattern, so every zero the call writes, in pad rows,
behind the mask and in pad columns, is +0.0), every other element must still be NaN.
Pad columns N .. round4(N) - 1 of a written row (N % 4 != 0: no bias, no mask) are ZERO after every kernel (include/cpc_hip.h; the fast
kernels clamp the B rows, so their last column group zeroes those lanes explicitly).  Every random-data case (seeded normal data)
has an exact-data twin, integers in {-2 .. 2} against {-1, 0, 1} thinned so that sum |a||b| <= 256 (asserted): every partial sum in any
order is an integer both formats hold.  Masks hold +0.0, -0.0, the smallest positive (subnormal) value of the storage type and negative
values beside normal ones.

The bound, per element, no element left out:   |got - ref| <= u_out |ref| + 2 (n + 2) 2^-24 S
S = the same operation on absolute values, n = K (+ 1 with a bias) for NT and the rows of the element's own slab for TN (each slab of a
split launch is judged on its own), u_out = 2^-8 for a bf16 output and 0 for an f32 one.  Derived in conv1d_reference.py, not measured;
no tolerance here comes from a kernel run.  The float32 host emulation alone (test_gemm_reference_host.py, against the bound without its
u_out term) reaches at most

    nt generic   0.15 (f32) / 0.018 (bf16)     nt fast128  0.063 / 0.013     nt 256  0.017 (bf16)     nt skinny  0.17 (f32)
    tn generic   0.17 (f32) / 0.012 (bf16)     tn skinny   0.16 (f32)        tn dma  0.071 (bf16)     tn fast    0.010 (bf16)

of it.  (A stored bf16 output can use the whole u_out |ref| term through its one rounding alone.)

Paths (gemm_reference.nt_choice / tn_choice restate launch_gemm_nt / launch_gemm_tn; their tile is asserted against _hip.nt_tile /
_hip.tn_tile and their epilogue form against CPC_GEMM_QUERY_EPI, on the host and before every launch here).  ch = 8 bf16 / 4 f32
elements (16 bytes), bk = 8 ch (one K stage), blk = 64 bf16 / 32 f32 rows (one TN stage).  NT: generic = K % bk != 0 or CPC_GEMM_FORCE_GENERIC; fast128 epilogues: direct (bf16 in / out, LDS-DMA,
whole 16-byte column groups, 16-byte-aligned C, mask and bias; no mask unless CPC_GEMM_DIRECT_MASK), wide (the same without the register
epilogue: CPC_GEMM_NO_PERS, a mask, an unaligned bias, CPC_GEMM_NO_DMA), narrow (everything else: f32, f32 output, N % 8 != 0, unaligned C or
mask, c_item % 8 != 0); K order storage, tap-innermost (lda < K, K % lda == 0, lda % bk == 0, no CPC_GEMM_LINEAR_K) or gathered (k_taps).

    nt generic            M in {1, 17, 33, 127, 128, 129} x N in {6, 10, 12, 24, 128, 132} at K in {ch, bk - ch, bk + ch, 3 ch} and
                          forced at 3 bk; M33-N24-lda<K-generic, M40-arpi10-crpi5-generic, M17-N24-brpi3-generic,
                          crpi8-valid{0,1,8}-skip{0,1}-K(bk+ch), batch3-K(bk+ch) (f32 and bf16); f32-skinny-shape-A-unaligned,
                          bf16-outf32-generic
    nt fast128 narrow     every other f32 case below; bf16: M129-N132-K3bk-bias-relu, M17-N130-Kbk, M17-N64-Kbk-C-unaligned,
                          M40-N64-Kbk-mask-unaligned, M130-N64-K3bk-narrow, M40-arpi10-crpi5, two-level-kranges, outf32-fast,
                          outf32-N-ragged; f32-skinny-shape-crpi2 (the skinny shape with a second output row level)
    nt fast128 direct     bf16: M1-N128-Kbk, M127-N136-Kbk-bias, M40-N64-Kbk-direct-mask, M130-N24-lda<K-linear, M17-N24-brpi3,
                          crpi8-valid{0,1,8}-skip{0,1}-Kbk, batch1-explicit, two-level-kranges-exact, items-kranges-exact;
                          tap-innermost: M130-N24-lda<K-taps; gathered: gathered-taps, gathered-taps-kranges-exact
    nt fast128 wide       bf16: M128-N128-Kbk-mask, M17-N64-Kbk-nopers, M17-N64-Kbk-bias-unaligned, M40-N64-Kbk-mask,
                          crpi8-valid5-mask(-skip), batch3-Kbk; no-dma: M130-N64-K3bk-nodma; gathered: grid-conv-combo (what the grid
                          convolutions launch: mask + two-level rows + gathered pieces + exact K ranges + skipped pad rows; f32: narrow)
    nt skinny (f32)       skinny-N8-K4, skinny-N16-K20, skinny-N32-K32 (M = 4096, bias, relu, c_rpi), skinny-N32-K32-skip (M = 4099)
    nt 256 (bf16, CPC_GEMM_BIG_TILE, M = 256 .. 600)
                          direct: 256-direct, -direct-M256, -direct-2N, -brpi-lda>K, -arpi100-crpi50, -lda<K-taps, -lda<K-linear,
                          -two-level-kranges-exact, -gathered-taps; staged: 256-staged, -staged-mask-crpi, -batch3, -two-level-kranges,
                          -grid-conv-combo, -bias-unaligned; form-mask: 256-form-mask(-skip); form-bits (cpc_gemm_nt_bits): 256-form-bits;
                          narrow: 256-narrow-outf32, -narrow-N260, -N258, -C-unaligned, -mask-unaligned;
                          persistent: 256-persistent (M = 256 513 + 32, N = 256, K = 128: 520 blocks), -persistent-K192 (3 K stages)
    tn skinny (f32)       I = 16, J = 24 at M in {1, 31, 32, 33, 101}, split3 / split5, rows-items8, rows-nodma, A-unaligned;
                          skinny-bound (I J / 4 = 256), skinny-ragged-I (I = 31)
    tn generic            f32: I = 40, J = 72 at the same M, split3 / split5 (J = 136), rows-items-odd, B-unaligned-rows, batch3, crpi,
                          beyond-skinny (I = 20, J = 64); both: ragged-I13, ragged-I45; bf16: out-bf16-generic-crpi, no-tr
    tn dma plain 128      bf16: all M x (I, J) cases, split3 / split5, batch3, crpi, out-bf16, 256-small-tile
    tn dma rows 128       bf16: rows-items8, rows-items-odd, two-level (a_rpi2, batch = 2 over a_batch, 3 slabs)
    tn fast plain / rows  bf16: A-unaligned / rows-nodma, B-unaligned-rows  (bf16 items are whole 16-byte chunks by the launcher's own check,
                          so the item-addressed non-DMA kernel is reached through CPC_GEMM_NO_DMA and an unaligned pointer)
    tn dma plain 256      bf16: 256-I256-J264, 256-I264-J256 (M = 1029), 256-split (3 chunks of 1024 over M = 2118)

Bitwise A/B relations, re-checked at these shapes where the reference is complete: a case's launch against the same launch with
CPC_GEMM_NO_DMA, CPC_GEMM_NARROW_EPI, CPC_GEMM_NO_PERS, CPC_GEMM_GENERIC_EPI, CPC_GEMM_SMALL_TILE added (or, where the case has the flag,
removed; CPC_GEMM_BIG_TILE removed) wherever that changes the path; TN 256 against 128 tiles.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
import gemm_reference as G  # noqa: E402
from gemm_reference import BF16, F32, TN  # noqa: E402
from test_attention_long_gpu import guard_intact, guarded  # noqa: E402
from test_gemm_reference_host import nt_query, nt_struct  # noqa: E402

DEV = "cuda:0"
EINVAL = -22
NT_CASES, TN_CASES = G.nt_cases(), G.tn_cases()


def operand(t64, dt, off):
    """A float64 host array exact in dt -> device array of dt whose element 0 sits `off` elements after a 256-byte-aligned address
    (NaN in front of it)."""
    buf = torch.full((off + t64.numel(),), G.NAN, device=DEV, dtype=dt)
    buf[off:] = t64.to(dt).to(DEV)
    return buf, buf[off:]


def output(n, dt, off):
    """n NaN elements `off` elements after an aligned address, sentinels behind them."""
    buf, _ = guarded(off + n, dt)
    return buf, buf[off:off + n]


def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def pack_bits(mask):
    """bits[i] bit e = mask[8 i + e] > 0 (include/cpc_hip.h at cpc_sign_bits); NaN (an element the call may not read) gives 0."""
    b = (mask.reshape(-1, 8) > 0).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32, device=mask.device)).sum(1).to(torch.uint8)


def run_nt(a, d, flags=None):
    """One launch of the case (flags: instead of the case's) on fresh buffers -> the flat output (device).  Asserts the path label and
    the queried epilogue form before the launch, the sentinels after it."""
    a = dict(a) if flags is None else dict(a, flags=flags)
    dt, odt = a["dt"], G.out_dtype(a)
    choice = G.nt_choice(a)
    assert choice is not None and nt_query(a) == 100 + choice["form"], (choice, nt_query(a))
    if choice["path"] != "nt skinny":
        assert choice["tile"] == _hip.nt_tile(_hip.dtype_code(dt), a["M"], a["N"], a["K"], a["flags"], a["batch"]), choice
    _, A = operand(G.device_copy(d, "A"), dt, a["offA"])
    _, Bt = operand(G.device_copy(d, "Bt"), dt, a["offB"])
    bias = operand(d["bias"], F32, a["off_bias"])[1] if a["bias"] else None
    mask = operand(G.device_copy(d, "mask"), dt, a["off_mask"])[1] if (a["mask"] or a["bits"]) else None
    kr = torch.tensor(a["k_ranges"], dtype=torch.int32, device=DEV).reshape(-1) if a["k_ranges"] is not None else None
    cbuf, Cv = output(d["sizeC"], odt, a["offC"])
    if a["bits"]:
        bits = pack_bits(mask.float())
        s = nt_struct(a, A.data_ptr() - a["offA"] * A.element_size(), Bt.data_ptr() - a["offB"] * Bt.element_size(),
                      Cv.data_ptr() - a["offC"] * Cv.element_size())
        assert _hip.lib().cpc_gemm_nt_bits(C.byref(s), _hip.ptr(bits), None, _hip.stream_ptr()) == 0
    else:
        _hip.gemm_nt(_hip.ptr(A), _hip.ptr(Bt), _hip.ptr(Cv), a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], _hip.dtype_code(dt),
                     bias=_hip.ptr(bias), mask=_hip.ptr(mask), a_rpi=a["a_rpi"], a_item=a["a_item"], b_rpi=a["b_rpi"], b_item=a["b_item"],
                     c_rpi=a["c_rpi"], c_item=a["c_item"], c_valid=a["c_valid"], a_batch=a["a_batch"], b_batch=a["b_batch"],
                     c_batch=a["c_batch"], batch=a["batch"], flags=a["flags"], a_extent=0 if (a["a_rpi2"] or a["k_taps"]) else A.numel(),
                     b_extent=Bt.numel(), a_rpi2=a["a_rpi2"], a_item2=a["a_item2"], c_rpi2=a["c_rpi2"], c_item2=a["c_item2"],
                     k_ranges=_hip.ptr(kr), k_taps=a["k_taps"], k_tap_stride=a["k_tap_stride"], k_tap_stride_a=a["k_tap_stride_a"])
    torch.cuda.synchronize()
    assert guard_intact(cbuf, a["offC"] + d["sizeC"]), "sentinels behind C"
    assert bool(torch.isnan(cbuf[:a["offC"]].float()).all()), "elements in front of C"
    return Cv


def run_tn(a, d, flags=None):
    a = dict(a) if flags is None else dict(a, flags=flags)
    dt, odt = a["dt"], G.out_dtype(a)
    choice = G.tn_choice(a)
    assert choice is not None
    if choice["path"] != "tn skinny":
        assert choice["tile"] == _hip.tn_tile(_hip.dtype_code(dt), a["M"], a["I"], a["J"], max(a["nsplit"], 1), a["m_chunk"], a["flags"]), choice
    _, A = operand(G.device_copy(d, "A"), dt, a["offA"])
    _, B = operand(G.device_copy(d, "B"), dt, a["offB"])
    cbuf, Cv = output(d["sizeC"], odt, 0)
    _hip.gemm_tn(_hip.ptr(A), _hip.ptr(B), _hip.ptr(Cv), a["M"], a["I"], a["J"], a["lda"], a["ldb"], a["ldc"], _hip.dtype_code(dt),
                 a_rpi=a["a_rpi"], a_item=a["a_item"], b_rpi=a["b_rpi"], b_item=a["b_item"], a_batch=a["a_batch"], b_batch=a["b_batch"],
                 c_batch=a["c_batch"], batch=a["batch"], nsplit=a["nsplit"], m_chunk=a["m_chunk"], slab_stride=a["slab_stride"],
                 flags=a["flags"], c_rpi=a["c_rpi"], c_item=a["c_item"], a_rpi2=a["a_rpi2"], a_item2=a["a_item2"])
    torch.cuda.synchronize()
    assert guard_intact(cbuf, d["sizeC"]), "sentinels behind C"
    return Cv


def verdict(got, ref, odt, exact, path, what, checked=None):
    q = G.judge(got, ref, odt, exact, checked)
    print(f"ratio [{path}] {what}{' exact' if exact else ''}: {q:.4f}")
    if exact:
        assert q == 0.0, f"{what} [{path}]: the exact-data twin differs from the reference (or an element outside the output was written)"
    else:
        assert q <= 1.0, f"{what} [{path}]: |got - ref| reaches {q:.3f} of the bound (inf: NaN, or an element outside the output written)"
    return q


# ======================================================================================================================= NT
# flags whose launch must give the same bits as the default one (same sums in the same order): added where the case lacks them ...
NT_AB_ADD = [G.NO_DMA, G.NARROW_EPI, G.NO_PERS, G.GENERIC_EPI, G.SMALL_TILE]
# ... and removed where it has them
NT_AB_DROP = [G.NO_DMA, G.NARROW_EPI, G.NO_PERS, G.BIG_TILE]


@pytest.mark.parametrize("cid", [c for c, a in NT_CASES if a["rows"] is None])
def test_gemm_nt(cid):
    """Every case of gemm_reference.nt_cases (but the persistent launch, below): the whole flat output against the float64 reference,
    element by element within the bound, unwritten elements still NaN, pad columns N .. round4(N) - 1 zero, sentinels intact; the
    exact-data twin bit for bit; and the A/B flags that apply give the same bits as the case's own launch."""
    a = dict(NT_CASES)[cid]
    path, odt = G.nt_path(a["dt"], a), G.out_dtype(a)
    for exact in (False, True):
        d = G.nt_data(a, exact)
        ref = G.nt_run_reference(a, d)
        if exact:
            assert float(ref.S.max()) <= G.EXACT_MAX
        out = run_nt(a, d)
        verdict(out, ref, odt, exact, path, cid)
        if a["N"] % 4:
            g = G.nt_geometry(a)
            pad = out[(g["c_rows"].reshape(-1, 1) + torch.arange(a["N"], G.round4(a["N"]))[None, :]).reshape(-1).to(DEV)]
            assert bool((pad == 0).all()), "pad columns"
        if exact:
            continue
        alts = [a["flags"] | f for f in NT_AB_ADD if not a["flags"] & f] + [a["flags"] & ~f for f in NT_AB_DROP if a["flags"] & f]
        if a["k_ranges"] is not None and not a["flags"] & G.KRANGE_EXACT:
            alts = [f for f in alts if (G.nt_choice(dict(a, flags=f)) or {}).get("tile") == G.nt_choice(a)["tile"]]   # (same unions)
        for f in alts:
            b = dict(a, flags=f)
            if G.nt_choice(b) is None or G.nt_path(a["dt"], b) == path:
                continue
            assert same_bits(run_nt(a, d, flags=f), out), f"{cid}: {G.nt_path(a['dt'], b)} against {path}"


def test_gemm_nt_persistent():
    """The persistent kernel (more than 512 tiles of 256 x 256; M = 256 513 + 32 ends in a ragged tile): a seeded subset of the rows and
    every pad row against float64, and all rows bitwise against the LDS-staged epilogue (CPC_GEMM_NO_PERS) and the non-persistent
    register epilogue of the 128 x 128 tile."""
    for cid in ("bf16-256-persistent", "bf16-256-persistent-K192"):        # K = 128: two stages per tile; K = 192: three, the odd-stage tile change
        a = dict(NT_CASES)[cid]
        assert G.nt_path(BF16, a) == "nt 256 persistent" and G.nt_path(BF16, dict(a, flags=a["flags"] | G.NO_PERS)) == "nt 256 staged"
        for exact in (False, True):
            d = G.nt_data(a, exact)
            ref = G.nt_run_reference(a, d)
            out = run_nt(a, d)
            verdict(out, ref, BF16, exact, "nt 256 persistent", cid, checked=ref.written)
            m = torch.arange(a["M"])
            pad = out.view(a["M"], a["N"])[((m % a["c_rpi"]) >= a["c_valid"]).to(DEV)]
            assert bool((pad == 0).all()) and not bool(torch.isnan(out.float()).any())
            assert same_bits(run_nt(a, d, flags=a["flags"] | G.NO_PERS), out)
            if not exact:
                assert same_bits(run_nt(a, d, flags=a["flags"] | G.SMALL_TILE), out)


# ======================================================================================================================= TN
@pytest.mark.parametrize("cid", [c for c, _ in TN_CASES])
def test_gemm_tn(cid):
    """Every case of gemm_reference.tn_cases: each slab on its own against float64 (n = the rows of that slab), empty chunks zero slabs,
    everything between and behind the slabs still NaN; the twin bit for bit; the 256 x 256 tile and the 128 x 128 one
    (CPC_GEMM_SMALL_TILE) give the same bits."""
    a = dict(TN_CASES)[cid]
    path, odt = G.tn_path(a["dt"], a), G.out_dtype(a)
    for exact in (False, True):
        d = G.tn_data(a, exact)
        ref = G.tn_run_reference(a, d)
        if exact:
            assert float(ref.S.max()) <= G.EXACT_MAX
        out = run_tn(a, d)
        verdict(out, ref, odt, exact, path, cid)
        if exact or a["dt"] != BF16:
            continue
        b = dict(a, flags=a["flags"] ^ G.SMALL_TILE)
        if G.tn_path(BF16, b) != path:
            assert same_bits(run_tn(a, d, flags=b["flags"]), out), f"{cid}: {G.tn_path(BF16, b)} against {path}"


def test_gemm_tn_refusals_write_nothing():
    """The conditions of cpc_gemm_tn / launch_gemm_tn, with real buffers: -22 and an untouched output.  Among them: the second row level
    of A exists in the bf16 LDS-DMA kernel only, so the f32 shapes of gemm_tn_skinny_f32_kernel (which took it and ignored it) and of
    the generic kernel refuse it."""
    lib = _hip.lib()
    n_checked = 0

    def refused(a):
        nonlocal n_checked
        ok = TN(a["dt"], 100, 40, 72, flags=G.OUT_F32)
        dt = a["dt"]
        assert G.tn_choice(a) is None, a
        A = torch.ones(1 << 16, device=DEV, dtype=dt)
        B = torch.ones(1 << 16, device=DEV, dtype=dt)
        cbuf, Cv = output(1 << 16, G.out_dtype(a), 0)
        es = A.element_size()
        s = _hip.GemmTNArgs(A.data_ptr() + a["offA"] * es, B.data_ptr() + a["offB"] * es, Cv.data_ptr(), a["M"], a["I"], a["J"], a["lda"], a["ldb"],
                            a["ldc"], a["a_rpi"], a["a_item"], a["b_rpi"], a["b_item"], a["a_batch"], a["b_batch"], a["c_batch"], a["batch"], a["nsplit"],
                            a["m_chunk"], a["slab_stride"], a["flags"], _hip.dtype_code(dt), a["c_rpi"], a["c_item"], a["a_rpi2"], a["a_item2"])
        rc = lib.cpc_gemm_tn(C.byref(s), _hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (rc, {k: v for k, v in a.items() if v != ok.get(k)})
        assert bool(torch.isnan(Cv.float()).all()) and guard_intact(cbuf, 1 << 16)
        n_checked += 1

    for dt in (F32, BF16):
        ch, blk = G.ch_of(dt), (64 if dt == BF16 else 32)
        ok = TN(dt, 100, 40, 72, flags=G.OUT_F32)
        assert G.tn_choice(ok) is not None
        for bad in (dict(M=0), dict(I=0), dict(J=0), dict(J=72 + ch // 2), dict(lda=40 + ch // 2), dict(ldb=72 + ch // 2), dict(ldc=74),
                    dict(I=37, lda=32 if dt == BF16 else 36),                                            # ragged I without padded rows
                    dict(a_rpi=10, a_item=400 + ch // 2), dict(b_rpi=10, b_item=720 + ch // 2),
                    dict(nsplit=2, m_chunk=0), dict(nsplit=2, m_chunk=blk // 2), dict(nsplit=2, m_chunk=2 * blk + 1),
                    dict(M=3 * blk, nsplit=2, m_chunk=blk),                                              # the chunks do not cover M
                    dict(c_rpi=8, c_item=8 * 72 + 2), dict(c_rpi=8, c_item=8 * 72, nsplit=2, m_chunk=2 * blk),
                    dict(a_rpi2=2, a_item2=800), dict(a_rpi=10, a_item=400, a_rpi2=2, a_item2=800 + ch // 2)):
            refused(dict(ok, **bad))
        # a well-formed second level outside the bf16 LDS-DMA kernel
        two = dict(a_rpi=10, a_item=400, a_rpi2=2, a_item2=800)
        refused(dict(ok, **two, flags=G.OUT_F32 | G.FORCE_GENERIC))
        if dt == F32:
            refused(dict(ok, **two))                                                                     # the generic f32 kernel
            refused(dict(TN(F32, 100, 16, 24), a_rpi=10, a_item=160, a_rpi2=2, a_item2=320))            # the skinny f32 shape
            refused(dict(TN(F32, 100, 16, 64), a_rpi=10, a_item=160, a_rpi2=2, a_item2=320))
        else:
            assert G.tn_path(BF16, dict(ok, **two)) == "tn dma rows 128"
            refused(dict(ok, **two, flags=G.OUT_F32 | G.NO_DMA))
            refused(dict(ok, **two, flags=G.OUT_F32 | G.TN_NO_TR))
            refused(dict(ok, **two, offA=4))
            refused(dict(ok, **two, a_batch=4, batch=2))
            refused(dict(ok, nsplit=2, m_chunk=64, flags=0))                                             # slabs are f32
    assert n_checked >= 40


def test_nt_refusals_write_nothing():
    """The NT refusals this work added, with real buffers: the f32 skinny shape with a second row level or K ranges, and a piece stride
    without pieces, return -22 and leave the output alone."""
    lib = _hip.lib()
    A = torch.ones(4096 * 40, device=DEV)
    B = torch.ones(32 * 32, device=DEV)
    kr = torch.zeros(64, dtype=torch.int32, device=DEV)
    for over in (dict(c_rpi2=4, c_item2=4096), dict(a_rpi2=4, a_item2=4096), dict(k_ranges=[(0, 1)]), dict(k_tap_stride_a=64)):
        a = dict(G.NT(F32, 4096, 32, 32), **over)
        cbuf, Cv = output(4096 * 32, F32, 0)
        s = nt_struct(a, A.data_ptr(), B.data_ptr(), Cv.data_ptr(), k_ranges=kr.data_ptr())
        rc = lib.cpc_gemm_nt(C.byref(s), _hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (rc, over)
        assert bool(torch.isnan(Cv).all()) and guard_intact(cbuf, 4096 * 32)
