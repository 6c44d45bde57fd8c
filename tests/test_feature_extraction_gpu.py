"""Whole-recording feature extraction on the GPU: the three entry points cpc_stream_gather, cpc_feature_emit and cpc_stream_carry
against host slicing (bit for bit), their guard, and FeatureExtractor end to end against the float64 reference of
tests/feature_extraction_reference.py.

Bounds.  Copies and conversions: torch.equal on the bits.  Pooled sums: 16 * 2^-23 * sum |x| per channel -- the worst case of f32
partial sums over blocks of m = 16 frames taken in order ((m - 1) u sum |x| to first order with u = 2^-24, for the squares m u sum x^2
with each square rounded once, times two for the higher-order terms).  The kernel adds in f64 from the first term (csrc/stream.hip says
why), which lies far inside; the bound stays what f32 partials would have been held to.
End to end, fp32: 1e-4 relative l2, the bound test_lstm_gpu.py puts on calc_test_task_data.  bf16: relative to what the existing
routes give on the same data, measured in the test (see there).  None was obtained by running the code under test.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd import feature_extraction as FE  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset, TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioLSTMModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, softplus_score_function  # noqa: E402
import feature_extraction_reference as R  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
GUARD = 64           # sentinel elements behind every output
SENT = -7.5          # (exact in bf16)
EMIT_FRAMES = 32     # CPC_EMIT_FRAMES
LL = C.c_longlong
IDLE = [0, 0, 0, 0, -1, 0]


def bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def table(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def nan_buffer(n, dt=F32):
    """n elements of NaN followed by GUARD sentinels: (whole buffer, view of the n)."""
    buf = torch.full((n + GUARD,), float("nan"), device=DEV, dtype=dt)
    buf[n:] = SENT
    return buf, buf[:n]


def intact(buf, n):
    return bool((buf[n:].float() == SENT).all())


def make_store(code, n, seed):
    g = torch.Generator().manual_seed(seed)
    if code == 1:
        return torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    return torch.randn(n, generator=g)


# ========================================================================================================================== gather
def gather(store_dev, code, store_len, tab, out, R_, L, ldo, scale, Tc=1 << 20, total=1 << 40, n_rec=1 << 20):
    _hip.call("cpc_stream_gather", _hip.ptr(store_dev), code, LL(store_len), _hip.ptr(tab), _hip.ptr(out), R_, L, LL(ldo), scale, Tc,
              LL(total), n_rec)
    torch.cuda.synchronize()


@pytest.mark.parametrize("L", [1, 5, 257, 4099])
@pytest.mark.parametrize("code", [0, 1], ids=["f32", "int16"])
def test_stream_gather_bit_for_bit(code, L):
    """Windows of n in {0, 1, 3, 4, 5, L - 1, L} samples starting at 0, at an odd offset and at store_len - n, one row each, and an
    idle row, with ldo = L and L + 3: the row is the host's slice (times 1 / 32768 for int16: exact; the f32 store with scale 1 a bit
    copy), exact zeros behind it, NaN between the rows and the sentinels behind the last one intact."""
    store_len = 3 * L + 11
    store = make_store(code, store_len, 100 + L)
    scale = 1.0 / 32768.0 if code == 1 else 1.0
    lengths = sorted({n for n in (0, 1, 3, 4, 5, L - 1, L) if 0 <= n <= L})
    rows = [[first, n, 1, k, k, 0] for k, (n, first) in enumerate((n, f) for n in lengths for f in (0, 7, store_len - n))]
    rows.insert(2, list(IDLE))
    R_ = len(rows)
    store_dev, tab = store.to(DEV), table(rows)
    for ldo in (L, L + 3):
        buf, out = nan_buffer(R_ * ldo)
        gather(store_dev, code, store_len, tab, out, R_, L, ldo, scale)
        assert intact(buf, R_ * ldo)
        got = out.view(R_, ldo).cpu()
        for r, (first, n, _, _, rec, _) in enumerate(rows):
            n = n if rec >= 0 else 0
            want = torch.zeros(L)
            piece = store[first:first + n]
            want[:n] = piece.float() * scale if code == 1 else piece
            assert torch.equal(bits(got[r, :L]), bits(want)), (ldo, r, first, n)
            assert bool(torch.isnan(got[r, L:]).all()), (ldo, r)


def test_stream_gather_larger_grids():
    """The launcher's two larger workgroup forms (R ceil(L / 1024) >= 1024 and R ceil(L / 4096) >= 1024), rows of mixed length."""
    for R_, L in ((512, 2049), (1024, 4099)):
        store_len = 5 * L
        store = make_store(1, store_len, L)
        g = np.random.default_rng(L)
        ns = g.integers(0, L + 1, R_)
        ns[:3] = (0, L, L - 1)
        firsts = np.array([g.integers(0, store_len - n + 1) for n in ns])
        rows = [[int(f), int(n), 1, r, r, 0] for r, (f, n) in enumerate(zip(firsts, ns))]
        buf, out = nan_buffer(R_ * L)
        gather(store.to(DEV), 1, store_len, table(rows), out, R_, L, L, 1.0 / 32768.0)
        assert intact(buf, R_ * L)
        got = out.view(R_, L).cpu()
        want = torch.zeros(R_, L)
        for r, (f, n) in enumerate(zip(firsts, ns)):
            want[r, :n] = store[f:f + n].float() / 32768.0
        assert torch.equal(bits(got), bits(want))


# ============================================================================================================================ emit
def emit(tab, top, top_item, hall, hall_item, src_dt, z, c, out_dt, R_, Tc, E, H, total, n_rec, partial=None, acc_z=None, acc_c=None,
         store_len=1 << 30, L=1 << 20):
    _hip.call("cpc_feature_emit", _hip.ptr(tab), _hip.ptr(top), LL(top_item), _hip.ptr(hall), LL(hall_item), _hip.dtype_code(src_dt),
              _hip.ptr(z), _hip.ptr(c), _hip.dtype_code(out_dt), R_, Tc, E, H, LL(store_len), L, LL(total), n_rec, _hip.ptr(partial),
              _hip.ptr(acc_z), _hip.ptr(acc_c))
    torch.cuda.synchronize()


def _emit_rows(Tc):
    """Rows with 0, 1, Tc - 1 and Tc frames, an idle one and one more full one, their output rows scattered over the store with gaps:
    (rows, total_frames)."""
    counts = [0, 1, max(Tc - 1, 0), Tc, None, Tc]
    order = [3, 0, 5, 1, 2]          # where the rows lie in the store, by row index
    at, place = 2, {}
    for r in order:
        place[r] = at
        at += counts[r] + 3
    rows = [list(IDLE) if n is None else [0, 0, n, place[r], r, 0] for r, n in enumerate(counts)]
    return rows, at + 5


@pytest.mark.parametrize("Tc", [1, 3, 33])
@pytest.mark.parametrize("E,H", [(16, 16), (64, 96), (96, 64), (512, 512)])
@pytest.mark.parametrize("src_dt,out_dt", [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)], ids=["f32-f32", "f32-bf16", "bf16-bf16", "bf16-f32"])
def test_feature_emit_copies(src_dt, out_dt, E, H, Tc):
    """z rows from the top buffer, c rows from rows 1 .. of the hidden states, for rows of 0, 1, Tc - 1 and Tc frames and an idle row,
    scattered over the store; both kinds, and each alone (the other pointer NULL): equal types bit for bit, the two conversions what
    torch's .to(torch.bfloat16) / .float() give; every element of the stores that is not addressed keeps its NaN."""
    rows, total = _emit_rows(Tc)
    R_ = len(rows)
    top_item, hall_item = (Tc + 2) * E, (Tc + 3) * H
    g = torch.Generator().manual_seed(E + 7 * H + Tc)
    top = torch.randn(R_, top_item, generator=g).to(src_dt)
    hall = torch.randn(R_, hall_item, generator=g).to(src_dt)
    top_d, hall_d, tab = top.to(DEV), hall.to(DEV), table(rows)
    for kinds in ("zc", "z", "c"):
        zb, z = nan_buffer(total * E, out_dt)
        cb, c = nan_buffer(total * H, out_dt)
        emit(tab, top_d, top_item, hall_d, hall_item, src_dt, z if "z" in kinds else None, c if "c" in kinds else None, out_dt, R_, Tc, E, H,
             total, R_)
        assert intact(zb, total * E) and intact(cb, total * H)
        for kind, got, src, C_, skip in (("z", z, top, E, 0), ("c", c, hall, H, 1)):
            got = got.view(total, C_).cpu()
            want = torch.full((total, C_), float("nan"), dtype=out_dt)
            if kind in kinds:
                for r, (_, _, n, out, rec, _) in enumerate(rows):
                    if rec >= 0:
                        want[out:out + n] = src[r].view(-1, C_)[skip:skip + n].to(out_dt)
            assert torch.equal(bits(got), bits(want)), (kinds, kind)


def _pool_run(src_dt, data_top, data_hall, steps, E, H, Tc, n_rec):
    """Steps of cpc_feature_emit with pooling on [step][R][...] data; returns the accumulators and the stores."""
    R_ = data_top.shape[1]
    total = sum(row[2] for rows in steps for row in rows if row[4] >= 0)
    nblk = -(-Tc // EMIT_FRAMES)
    z, c = torch.empty(total, E, device=DEV), torch.empty(total, H, device=DEV)
    partial = torch.full((R_ * nblk * 2 * (E + H),), float("nan"), device=DEV, dtype=torch.float64)
    acc_z = torch.zeros(n_rec, 2, E, device=DEV, dtype=torch.float64)
    acc_c = torch.zeros(n_rec, 2, H, device=DEV, dtype=torch.float64)
    for j, rows in enumerate(steps):
        emit(table(rows), data_top[j].to(DEV), Tc * E, data_hall[j].to(DEV), (Tc + 1) * H, src_dt, z, c, F32, R_, Tc, E, H, total, n_rec,
             partial, acc_z, acc_c)
    return acc_z.cpu(), acc_c.cpu(), z.cpu(), c.cpu()


@pytest.mark.parametrize("src_dt", [F32, BF16], ids=["f32", "bf16"])
def test_feature_emit_pooled_sums(src_dt):
    """Three steps (33, 33, 20 frames) of recording 1 on stream 1 beside an idle stream and a short second recording: per channel the
    f64 accumulators hold the sum and the sum of squares of the source values within 16 * 2^-23 * sum |x| (sum x^2) of a float64 sum
    (module docstring), the same bits on a second run, and exact sums for integer-valued data."""
    E, H, Tc, n_rec = 64, 96, 33, 3
    frames = (33, 33, 20)
    steps, at = [], 4          # recording 2 owns rows [0, 4) of the stores, recording 1 rows [4, 90)
    for j, n in enumerate(frames):
        steps.append([list(IDLE), [0, 0, n, at, 1, 1 if j < 2 else 0], [0, 0, 4, 0, 2, 0] if j == 1 else list(IDLE)])
        at += n
    g = torch.Generator().manual_seed(21)
    for integer in (False, True):
        draw = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if integer else (lambda *s: torch.randn(*s, generator=g) * 3.0 + 0.5)
        top = draw(3, 3, Tc * E).to(src_dt)
        hall = draw(3, 3, (Tc + 1) * H).to(src_dt)
        first = _pool_run(src_dt, top, hall, steps, E, H, Tc, n_rec)
        second = _pool_run(src_dt, top, hall, steps, E, H, Tc, n_rec)
        for a, b in zip(first, second):
            assert torch.equal(bits(a), bits(b)), "two runs of the same call sequence differ"
        for acc, src, C_, skip in ((first[0], top, E, 0), (first[1], hall, H, 1)):
            x1 = torch.cat([src[j, 1].view(-1, C_)[skip:skip + n] for j, n in enumerate(frames)]).double()
            x2 = src[1, 2].view(-1, C_)[skip:skip + 4].double()
            assert torch.equal(acc[0], torch.zeros(2, C_, dtype=torch.float64)), "a recording no row named gained something"
            for rec, x in ((1, x1), (2, x2)):
                for row, v in ((0, x), (1, x * x)):
                    want, bound = v.sum(0), 16 * 2.0 ** -23 * v.abs().sum(0)
                    err = (acc[rec, row] - want).abs()
                    if integer:
                        assert torch.equal(acc[rec, row], want), (rec, row)
                    else:
                        print(f"pooled sums {src_dt} rec {rec} row {row}: largest error / bound {(err / bound).max().item():.3f}")
                        assert bool((err <= bound).all()), (rec, row, (err / bound).max().item())


# =========================================================================================================================== carry
def carry(tab, src, dst, R_, H, store_len=1 << 30, L=1 << 20, Tc=1 << 20, total=1 << 40, n_rec=1 << 20):
    n = len(src)
    _hip.call("cpc_stream_carry", _hip.ptr(tab), (C.c_void_p * n)(*[t.data_ptr() for t in src]), (C.c_void_p * n)(*[t.data_ptr() for t in dst]),
              n, R_, H, LL(store_len), L, Tc, LL(total), n_rec)
    torch.cuda.synchronize()


@pytest.mark.parametrize("nstate", [1, 2, 4])
def test_stream_carry_is_exact(nstate):
    """dst = keep ? src : 0 per stream, for 1, 2 and 4 state arrays: kept rows bit for bit, the others exact zeros (an idle row also
    where its keep entry is set), nothing behind the arrays."""
    R_, H = 5, 48
    rows = [[0, 0, 1, 0, 0, 1], [0, 0, 1, 1, 1, 0], [0, 0, 1, 2, 2, 1], [0, 0, 0, 0, -1, 1], [0, 0, 1, 3, 3, 0]]
    keep = torch.tensor([1, 0, 1, 0, 0], dtype=torch.bool)
    g = torch.Generator().manual_seed(nstate)
    src = [torch.randn(R_, H, generator=g).to(DEV) for _ in range(nstate)]
    pairs = [nan_buffer(R_ * H) for _ in range(nstate)]
    carry(table(rows), src, [v for _, v in pairs], R_, H)
    for s, (buf, dst) in zip(src, pairs):
        assert intact(buf, R_ * H)
        want = torch.where(keep[:, None], s.cpu(), torch.zeros(R_, H))
        assert torch.equal(bits(dst.view(R_, H).cpu()), bits(want))


# =========================================================================================================================== guard
def test_offending_rows_are_idle():
    """The extents declared to the calls are smaller than the allocations, and every offending entry is chosen so that even an address
    formed from it stays inside the allocation: a window that leaves [0, store_len] at either end, n_samples > L, n_frames > Tc, output
    rows that leave [0, total_frames] at either end, rec >= n_rec.  Such rows get what an idle row gets -- zeros from the
    gather and the carry, nothing from the emit -- and their good neighbours are served."""
    L, Tc, E, H, R_alloc = 24, 4, 16, 16, 16
    margin, store_len, total, n_rec = 64, 200, 20, 4          # declared; the allocations have ``margin`` more on both sides
    good = [10, L, Tc, 3, 1, 1]
    bad = [[store_len - L + 1, L, 1, 0, 0, 1], [-1, 4, 1, 0, 0, 1], [0, L + 1, 1, 0, 0, 1], [0, -1, 1, 0, 0, 1], [0, L, Tc + 1, 0, 0, 1],
           [0, L, -1, 0, 0, 1], [0, L, 2, total - 1, 0, 1], [0, L, 1, -1, 0, 1], [0, L, 1, 0, n_rec, 1]]
    rows = [good] + bad + [[50, 5, 2, 10, 2, 0]]
    R_ = len(rows)
    assert R_ <= R_alloc
    tab = table(rows)
    # gather: the store sits ``margin`` samples inside its allocation
    alloc = make_store(1, store_len + 2 * margin, 3).to(DEV)
    buf, out = nan_buffer(R_ * (L + 8))
    _hip.call("cpc_stream_gather", _hip.ptr(alloc, margin), 1, LL(store_len), _hip.ptr(tab), _hip.ptr(out), R_, L, LL(L + 8), 1.0, Tc,
              LL(total), n_rec)
    torch.cuda.synchronize()
    assert intact(buf, R_ * (L + 8))
    got, store = out.view(R_, L + 8).cpu(), alloc.cpu()[margin:margin + store_len].float()
    for r, row in enumerate(rows):
        want = torch.zeros(L)
        if row in (good, rows[-1]):
            want[:row[1]] = store[row[0]:row[0] + row[1]]
        assert torch.equal(got[r, :L], want), r
        assert bool(torch.isnan(got[r, L:]).all())
    # emit: the feature stores sit ``margin`` rows inside their allocations, the sources have Tc + 4 rows per stream, the accumulators
    # room for twice n_rec recordings
    g = torch.Generator().manual_seed(4)
    rows_src = Tc + 4
    top, hall = torch.randn(R_, rows_src * E, generator=g), torch.randn(R_, (rows_src + 1) * H, generator=g)
    zb, z = nan_buffer((total + 2 * margin) * E)
    cb, c = nan_buffer((total + 2 * margin) * H)
    acc_z = torch.zeros(2 * n_rec, 2, E, device=DEV, dtype=torch.float64)
    acc_c = torch.zeros(2 * n_rec, 2, H, device=DEV, dtype=torch.float64)
    partial = torch.zeros(R_ * 2 * (E + H), device=DEV, dtype=torch.float64)
    top_d, hall_d = top.to(DEV), hall.to(DEV)
    _hip.call("cpc_feature_emit", _hip.ptr(tab), _hip.ptr(top_d), LL(rows_src * E), _hip.ptr(hall_d), LL((rows_src + 1) * H),
              _hip.F32, _hip.ptr(z, margin * E), _hip.ptr(c, margin * H), _hip.F32, R_, Tc, E, H, LL(store_len), L, LL(total), n_rec,
              _hip.ptr(partial), _hip.ptr(acc_z), _hip.ptr(acc_c))
    torch.cuda.synchronize()
    assert intact(zb, (total + 2 * margin) * E) and intact(cb, (total + 2 * margin) * H)
    for got, src, C_, skip, acc in ((z, top, E, 0, acc_z), (c, hall, H, 1, acc_c)):
        got = got.view(total + 2 * margin, C_).cpu()
        want = torch.full_like(got, float("nan"))
        sums = torch.zeros(2 * n_rec, 2, C_, dtype=torch.float64)
        for r in (0, R_ - 1):
            _, _, n, at, rec, _ = rows[r]
            x = src[r].view(-1, C_)[skip:skip + n]
            want[margin + at:margin + at + n] = x
            sums[rec, 0], sums[rec, 1] = x.double().sum(0), (x.double() ** 2).sum(0)
        assert torch.equal(bits(got), bits(want))
        assert torch.allclose(acc.cpu(), sums, rtol=0, atol=1e-4) and torch.equal(acc.cpu() == 0, sums == 0)
    # carry: only the good row with keep = 1 keeps its state
    src = [torch.randn(R_, H, generator=g).to(DEV)]
    sb, dst = nan_buffer(R_ * H)
    carry(tab, src, [dst], R_, H, store_len, L, Tc, total, n_rec)
    want = torch.zeros(R_, H)
    want[0] = src[0][0].cpu()
    assert intact(sb, R_ * H) and torch.equal(bits(dst.view(R_, H).cpu()), bits(want))


# ====================================================================================================================== end to end
RECS = R.recordings()
CONTEXTS = {"gru": ("gru", 1), "gru2": ("gru", 2), "lstm": ("lstm", 1)}


def _dataset(recs=RECS, **kw):
    return DeviceAudioDataset(arrays=recs, item_length=100, device=DEV, storage="int16", **kw)


def _params(model):
    return {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("streams,Tc", [(2, 16), (3, 7), (8, 64)])
@pytest.mark.parametrize("context", list(CONTEXTS))
def test_extraction_against_float64_reference(context, streams, Tc):
    """Six int16 recordings of 0, 1, 5, 16, 37 and 64 frames through the small encoder and a GRU (1 and 2 layers) or LSTM of 32 units,
    fp32: z and c of every recording within 1e-4 (relative l2) of the float64 reference run on the whole recording, the pooled mean and
    deviation within 1e-4, frame_offsets as counted on the host; where a recording has frames beyond the first chunk, c there is more
    than 1e-2 away from the reference WITHOUT the hand-off; and an array source gives the bits of the dataset source."""
    kind, layers = CONTEXTS[context]
    model = R.model_for(kind, 32, layers).to(DEV)
    params = _params(model)
    ref = R.reference_features(kind, layers, params, RECS)
    ex = FE.FeatureExtractor(model, streams=streams, chunk_frames=Tc)
    out = ex.extract(_dataset())
    torch.cuda.synchronize()
    offsets = [0]
    for f in R.FRAME_COUNTS:
        offsets.append(offsets[-1] + f)
    assert out.frame_offsets == offsets and out.frame_counts == list(R.FRAME_COUNTS) and out.file_indices == list(range(len(RECS)))
    assert out.z.shape == (offsets[-1], R.E_S) and out.c.shape == (offsets[-1], 32) and out.z.dtype == F32 and out.c.dtype == F32
    assert bool(torch.isfinite(out.z).all()) and bool(torch.isfinite(out.c).all())
    worst = {"z": 0.0, "c": 0.0}
    for i, (z_ref, c_ref) in enumerate(ref):
        if R.FRAME_COUNTS[i] == 0:
            continue
        ez, ec = R.rel_l2(out.recording(i, "z"), z_ref), R.rel_l2(out.recording(i, "c"), c_ref)
        worst["z"], worst["c"] = max(worst["z"], ez), max(worst["c"], ec)
        assert ez <= 1e-4 and ec <= 1e-4, (i, ez, ec)
        if R.FRAME_COUNTS[i] > Tc:
            _, c_cut = R.chunked_reference(RECS[i].astype(np.float64) / 32768.0, params, kind, Tc, layers, hand_off=False)
            gap = R.rel_l2(out.recording(i, "c")[Tc:], c_cut[Tc:])
            assert gap > 1e-2, (i, gap)
    assert R.rel_l2(out.z, torch.cat([z for z, _ in ref])) <= 1e-4 and R.rel_l2(out.c, torch.cat([c for _, c in ref])) <= 1e-4
    for kind_, col in (("z", 0), ("c", 1)):
        mean, std = zip(*[R.pooled_reference(pair[col]) for pair in ref])
        got = out.pooled[kind_]
        assert got.mean.dtype == F32 and got.mean.shape == (len(RECS), ref[0][col].shape[1]) == got.std.shape
        em, es = R.rel_l2(got.mean, torch.stack(mean)), R.rel_l2(got.std, torch.stack(std))
        assert em <= 1e-4 and es <= 1e-4, (kind_, em, es)
        assert not got.mean[0].any() and not got.std[0].any(), "a recording without frames has mean and deviation 0"
    print(f"{context} R={streams} Tc={Tc}: largest relative l2 error per recording", {k: f"{v:.2e}" for k, v in worst.items()})
    arrays = ex.extract([torch.from_numpy(r) for r in RECS])
    assert torch.equal(bits(arrays.z), bits(out.z)) and torch.equal(bits(arrays.c), bits(out.c))
    for k in ("z", "c"):
        assert torch.equal(arrays.pooled[k].mean, out.pooled[k].mean) and torch.equal(arrays.pooled[k].std, out.pooled[k].std)


def test_kinds_files_and_out_dtype():
    """features=("z",) / ("c",): the other kind is absent and the one given has the bits of the run with both; ``files`` picks and orders
    recordings; out_dtype=bfloat16 is the float32 store rounded by torch; pool=False gives no pooled part; model.extract_features is the
    same call."""
    model = R.model_for("gru", 32, 1).to(DEV)
    src = _dataset()
    both = FE.FeatureExtractor(model, streams=3, chunk_frames=7).extract(src)
    z_only = FE.FeatureExtractor(model, features=("z",), streams=3, chunk_frames=7, pool=False).extract(src)
    c_only = model.extract_features(src, features=("c",), streams=3, chunk_frames=7)
    assert not hasattr(z_only, "c") and not hasattr(c_only, "z") and z_only.pooled is None and set(c_only.pooled) == {"c"}
    assert torch.equal(bits(z_only.z), bits(both.z)) and torch.equal(bits(c_only.c), bits(both.c))
    picked = model.extract_features(src, files=[4, 0, 2], streams=3, chunk_frames=7)
    assert picked.frame_counts == [37, 0, 5] and picked.file_indices == [4, 0, 2] and picked.frame_offsets == [0, 37, 37, 42]
    # (another schedule puts a recording into other rows of the launches: the same f32 arithmetic, possibly in another order)
    assert R.rel_l2(picked.recording(0), both.recording(4)) <= 1e-6 and R.rel_l2(picked.recording(2, "z"), both.recording(2, "z")) <= 1e-6
    assert R.rel_l2(picked.pooled["c"].mean[0], both.pooled["c"].mean[4]) <= 1e-6
    half = model.extract_features(src, streams=3, chunk_frames=7, out_dtype=BF16)
    assert half.z.dtype == BF16 and torch.equal(bits(half.z), bits(both.z.to(BF16))) and torch.equal(bits(half.c), bits(both.c.to(BF16)))
    assert torch.equal(half.pooled["z"].mean, both.pooled["z"].mean)
    nothing = model.extract_features([np.zeros(R.RF - 1, np.int16)], streams=3, chunk_frames=7)
    assert nothing.z.shape == (0, R.E_S) and nothing.frame_offsets == [0, 0] and not nothing.pooled["c"].std.any()


def _standalone(model, kind, layers):
    """A stand-alone encoder and context network (reset_hidden=False) with the model's weights, in the model's compute type."""
    enc = AudioEncoder(R.SMALL)
    enc.load_state_dict(model.encoder.state_dict())
    ar = AudioLSTMModel(R.E_S, 32, reset_hidden=False) if kind == "lstm" else AudioGRUModel(R.E_S, 32, reset_hidden=False, num_layers=layers)
    ar.load_state_dict(model.autoregressive_model.state_dict())
    enc.compute_dtype = ar.compute_dtype = model.compute_dtype
    return enc.to(DEV), ar.to(DEV)


@pytest.mark.parametrize("context", ["gru", "lstm"])
def test_extraction_bf16_against_the_existing_routes(context):
    """bf16, (streams, chunk_frames) = (3, 7).  z: the error against the float64 reference is at most twice the error of the existing
    model.encoder(recording) on the same frames (the GEMM tile form may change with the row count and reorder sums).  c: at most
    max(2e-2, 2 e), e the error at chunk ends of the existing stand-alone context network (reset_hidden=False) fed the same chunks of
    z.  The test prints the measured errors; DESIGN.md, "Whole-recording feature extraction", records them."""
    kind, layers = CONTEXTS[context]
    Tc = 7
    model = R.model_for(kind, 32, layers, dtype="bf16").to(DEV)
    params = _params(model)
    ref = R.reference_features(kind, layers, params, RECS)
    out = FE.FeatureExtractor(model, streams=3, chunk_frames=Tc).extract(_dataset())
    enc, ar = _standalone(model, kind, layers)
    z_old, ends_old, ends_ref, ends_new = [], [], [], []
    with torch.no_grad():
        for i, rec in enumerate(RECS):
            F_ = R.FRAME_COUNTS[i]
            if F_ == 0:
                continue
            x = (torch.from_numpy(rec).float() / 32768.0).view(1, 1, -1).to(DEV)
            z_old.append(enc(x)[0].T.float().cpu())
            ar.hidden = None
            z_new = out.recording(i, "z").float()
            for f0 in range(0, F_, Tc):
                nf = min(Tc, F_ - f0)
                ends_old.append(ar(z_new[f0:f0 + nf].T.unsqueeze(0).contiguous())[0].float().cpu())
                ends_ref.append(ref[i][1][f0 + nf - 1])
                ends_new.append(out.recording(i, "c")[f0 + nf - 1].float().cpu())
    z_ref, c_ref = torch.cat([z for z, _ in ref]), torch.cat([c for _, c in ref])
    e_z_old, e_z = R.rel_l2(torch.cat(z_old), z_ref), R.rel_l2(out.z, z_ref)
    e_old, e_c, e_c_ends = R.rel_l2(torch.stack(ends_old), torch.stack(ends_ref)), R.rel_l2(out.c, c_ref), R.rel_l2(torch.stack(ends_new), torch.stack(ends_ref))
    print(f"bf16 {context}: z {e_z:.2e} (model.encoder {e_z_old:.2e}); c {e_c:.2e} over all frames, {e_c_ends:.2e} at chunk ends "
          f"(stand-alone context at chunk ends {e_old:.2e})")
    assert e_z <= 2 * e_z_old
    assert e_c <= max(2e-2, 2 * e_old) and e_c_ends <= max(2e-2, 2 * e_old)


# ==================================================================================================================== side effects
class _Meter:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))


class _Logger:
    def __init__(self):
        self.loss_meter, self.score_meter = _Meter(), _Meter()

    def log(self, step):
        pass


def _train(steps, between=None, **attrs):
    """``steps`` train() calls of one fp32 Adam step each on the same trainer; ``between(trainer)`` runs after the first call."""
    model = R.model_for("gru", 32, 1).to(DEV)
    data = torch.randn(8, model.item_length, generator=torch.Generator().manual_seed(11)) * 0.5
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=1.0, score_function=softplus_score_function, prediction_steps=4, ar_size=32)
    tr.verbose = False
    for k, v in attrs.items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    assert tr._fused()
    for i in range(steps):
        random.seed(5 + i)
        tr.train(batch_size=8, epochs=1, lr=2e-4, num_workers=0, max_steps=1)
        torch.cuda.synchronize()
        if i == 0 and between is not None:
            between(tr)
    assert len(logger.loss_meter.values) == steps
    return logger.loss_meter.values, _params(model), tr


def test_extraction_leaves_training_alone():
    """Two fp32 train steps with an extract between them equal two steps without it, bit for bit, in the losses and every parameter;
    autoregressive_model.hidden, model.training and the random states are what they were."""
    seen = {}

    def between(tr):
        m = tr.model
        before = (m.training, m.autoregressive_model.hidden, random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
        seen["out"] = m.extract_features(_dataset(), streams=2, chunk_frames=16)
        torch.cuda.synchronize()
        assert m.training is before[0] and m.autoregressive_model.hidden is before[1] and random.getstate() == before[2]
        assert torch.equal(torch.get_rng_state(), before[3]) and torch.equal(torch.cuda.get_rng_state(DEV), before[4])

    with_extract, plain = _train(2, between), _train(2)
    assert seen["out"].c.shape[0] == sum(R.FRAME_COUNTS)
    assert with_extract[0] == plain[0]
    for k in plain[1]:
        assert torch.equal(bits(with_extract[1][k]), bits(plain[1][k])), k


def test_trainer_extract_features_with_the_averaged_weights():
    """trainer.extract_features(use_ema=True) equals extraction from a model loaded with ema_state_dict(); afterwards the raw weights are
    back bit for bit; without an average it raises ValueError."""
    _, params, tr = _train(2, ema_decay=0.5)
    src = _dataset()
    averaged = tr.extract_features(src, use_ema=True, streams=3, chunk_frames=7)
    raw = tr.extract_features(src, streams=3, chunk_frames=7)
    torch.cuda.synchronize()
    for k, v in _params(tr.model).items():
        assert torch.equal(bits(v), bits(params[k])), k
    twin = R.model_for("gru", 32, 1)
    twin.load_state_dict(tr.ema_state_dict())
    want = twin.to(DEV).extract_features(src, streams=3, chunk_frames=7)
    assert torch.equal(bits(averaged.z), bits(want.z)) and torch.equal(bits(averaged.c), bits(want.c))
    assert not torch.equal(bits(averaged.c), bits(raw.c)), "the average made no difference"
    _, _, plain = _train(1)
    with pytest.raises(ValueError, match="average"):
        plain.extract_features(src, use_ema=True)


# ================================================================================================================== launch pattern
class _Spy:
    """Records the entry-point names that go through _hip.call while active."""

    def __enter__(self):
        self.names, self.real = [], _hip.call

        def spy(name, *a, **kw):
            self.names.append(name)
            return self.real(name, *a, **kw)

        _hip.call = spy
        return self

    def __exit__(self, *exc):
        _hip.call = self.real


class _NoHostTraffic:
    """While active, the torch calls that copy between host and device, synchronise or allocate raise."""

    NAMES = [(torch.Tensor, n) for n in ("to", "cpu", "cuda", "item", "tolist", "numpy", "copy_", "clone", "zero_")] + \
            [(torch, n) for n in ("empty", "zeros", "full", "tensor", "as_tensor", "from_numpy")] + [(torch.cuda, "synchronize")]

    def __enter__(self):
        self.saved = [(o, n, getattr(o, n)) for o, n in self.NAMES]
        for o, n, _ in self.saved:
            def refuse(*a, _n=n, **kw):
                raise AssertionError(f"torch {_n} inside the extraction loop")
            setattr(o, n, refuse)

    def __exit__(self, *exc):
        for o, n, f in self.saved:
            setattr(o, n, f)


@pytest.mark.parametrize("context", ["gru2", "lstm"])
def test_launch_pattern(context, monkeypatch):
    """Per step one cpc_stream_gather, one cpc_feature_emit and one cpc_stream_carry, the table uploaded once, and no torch call that
    copies, synchronises or allocates inside the loop body (FeatureExtractor._step is wrapped, not timed)."""
    kind, layers = CONTEXTS[context]
    model = R.model_for(kind, 32, layers).to(DEV)
    src = _dataset()
    ex = FE.FeatureExtractor(model, streams=2, chunk_frames=16)
    ex.extract(src)          # (the buffers exist from here on)
    sched = FE.plan_schedule(*zip(*src.file_ranges()), R.RF, R.DS, 2, 16)
    n_steps = sched.table.shape[0]
    assert n_steps == 6          # chunks 1, 1, 1, 3, 4 on two streams: 1 + 1 + 4 on the first, 1 + 3 on the second
    body, inside = FE.FeatureExtractor._step, []

    def wrapped(self, eng, run, block):
        with _NoHostTraffic():
            before = len(spy.names)
            body(self, eng, run, block)
            inside.append(spy.names[before:])

    monkeypatch.setattr(FE.FeatureExtractor, "_step", wrapped)
    uploads, real_from_numpy = [], torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: uploads.append(a.shape) or real_from_numpy(a))
    with _Spy() as spy:
        out = ex.extract(src)
    assert len(inside) == n_steps
    for names in inside:
        for entry in ("cpc_stream_gather", "cpc_feature_emit", "cpc_stream_carry"):
            assert names.count(entry) == 1, (entry, names)
        assert names[0] == "cpc_stream_gather" and names.index("cpc_feature_emit") > names.index("cpc_conv1_fwd")
        assert names.count("cpc_lstm_fwd" if kind == "lstm" else "cpc_gru_fwd_h0") == layers
    for entry in ("cpc_stream_gather", "cpc_feature_emit", "cpc_stream_carry"):
        assert spy.names.count(entry) == n_steps
    assert uploads.count((n_steps * 2 * 6,)) == 1, uploads
    assert out.c.shape[0] == sum(R.FRAME_COUNTS)
