"""Grid masking on the GPU: cpc_grid_sum and cpc_grid_mask alone on grids the test writes (spans against the host restatement, the
three fills in the copy and the in-place form, sentinels around and between the clips, the protected frames, determinism), and
trainer.grid_masking behind PreprocessingModule and MelPreprocessingModule on the scalogram fixture model.

Error bound of cpc_grid_sum (u = 2^-24, gamma_d = d u / (1 - d u)): a partial is a summation tree whose depth in roundings is stated
in include/cpc_hip.h — a lane's chain over its four pieces (the first addition, to 0, is exact: 3), the positions of one channel
(log2(4 / Cc): 2, 1, 0), the butterfly over the wave (6) and the four waves (2): d = 13, 12, 11 for Cc = 1, 2, 4.  Every element passes
through at most d roundings, each of relative size u, so |partial - exact| <= gamma_d * sum |x| over the chunk's elements of the channel
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; the float64 reference's own error, 4096 terms of 2^-53, is below
1e-12 of that sum).  The mean adds one rounding per further chunk and one for the division."""
import copy
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset  # noqa: E402
from cpc_audio_amd.audio_model import AudioGRUModel, AudioPredictiveCodingModel  # noqa: E402
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, softplus_score_function  # noqa: E402
from cpc_audio_amd.grid_masking import GridMasking  # noqa: E402
from cpc_audio_amd.mel_spectrogram import MelPreprocessingModule, mel_default_dict  # noqa: E402
from cpc_audio_amd.scalogram_model import PreprocessingModule, ScalogramResidualEncoder  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24
SENTINEL = -12345.5
GUARD = 64
B = 3
SHAPES = [(1, 1, 1), (5, 3, 2), (41, 25, 1), (37, 24, 2), (33, 7, 4), (130, 80, 2)]          # (W, H, Cc)
PADS = [0, 1, 4]
SUM_DEPTH = {1: 13, 2: 12, 4: 11}
LL = C.c_longlong


def gamma(n):
    return n * U / (1.0 - n * U)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Clips:
    """B clips of n floats, ldb apart, in a device buffer with GUARD sentinels in front and behind, NaN in the padding between the
    clips, and ``shift`` floats between the (256-byte aligned) allocation and the first clip."""

    def __init__(self, data, ldb, shift=0):
        self.n, self.ldb, self.shift = data.shape[1], ldb, shift
        host = np.full(GUARD + shift + B * ldb + GUARD, SENTINEL, dtype=np.float32)
        body = host[GUARD + shift:GUARD + shift + B * ldb].reshape(B, ldb)
        body[:, self.n:] = np.nan
        body[:, :self.n] = data
        self.t = torch.from_numpy(host).to(DEV)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.t.data_ptr() + 4 * (GUARD + shift))

    def read(self):
        """(the clips, True when sentinels and padding are as they were written)"""
        host = self.t.cpu().numpy()
        lo = GUARD + self.shift
        body = host[lo:lo + B * self.ldb].reshape(B, self.ldb)
        intact = (host[:lo] == SENTINEL).all() and (host[lo + B * self.ldb:] == SENTINEL).all() and np.isnan(body[:, self.n:]).all()
        return body[:, :self.n].copy(), bool(intact)


def _grid(rng, W, H, Cc, integers=False):
    n = W * H * Cc
    if integers:
        return rng.integers(-8, 9, size=(B, n)).astype(np.float32)
    x = rng.standard_normal((B, n)).astype(np.float32)
    return x + np.float32(0.5) * np.arange(1, Cc + 1, dtype=np.float32)[np.arange(n) % Cc]          # channel means apart from 0


def _masking(W, H, fill="zero", protect_last=0, seed=11):
    return GridMasking(freq_masks=(2, max(1, H // 4)), time_masks=(2, max(1, W // 4)), fill=fill, protect_last=protect_last, seed=seed)


def _sum(x, W, H, Cc):
    """cpc_grid_sum of the clips of ``x`` -> float32 [B, chunks, Cc] (a device tensor)."""
    n = W * H * Cc
    chunks = _hip.lib().cpc_grid_sum_chunks(n)
    partial = torch.full((B * chunks * Cc + 2,), SENTINEL, device=DEV)
    _hip.call("cpc_grid_sum", x.ptr, _hip.ptr(partial), B, n, LL(x.ldb), Cc)
    assert partial[-2:].tolist() == [SENTINEL] * 2
    return partial[:-2].view(B, chunks, Cc)


def _run(gm, x, y, W, H, Cc, step=3, clip_offset=2):
    """One cpc_grid_mask call (behind cpc_grid_sum with the mean fill) -> (spans_out, fill_out) as numpy arrays; y is x in place."""
    spans = torch.full((B, 32), -7, dtype=torch.int32, device=DEV)
    fill = torch.full((B, 4), SENTINEL, device=DEV)
    partial = _sum(x, W, H, Cc) if gm.fill_mode == 2 else None
    cfg = gm.config(step, clip_offset, W)
    _hip.call("cpc_grid_mask", x.ptr, y.ptr, _hip.ptr(partial), _hip.ptr(spans), _hip.ptr(fill), B, W, H, Cc, LL(x.ldb), LL(y.ldb),
              C.byref(cfg))
    torch.cuda.synchronize()
    return spans.cpu().numpy(), fill.cpu().numpy()


def _expected(data, mask, fill, Cc):
    """data [B, n] with fill[b][c] on the masked cells."""
    cells = data.reshape(B, -1, Cc).copy()
    for b in range(B):
        cells[b][mask[b].reshape(-1)] = fill[b, :Cc]
    return cells.reshape(B, -1)


def _check_both_forms(gm, data, W, H, Cc, pad, fill_of):
    """Runs the copy and the in-place form on ``data`` and checks spans, fill, every cell bit for bit and the surroundings.
    fill_of(fill_out) -> the expected fill [B, 4] (the mean-fill cases check fill_out themselves and hand it back)."""
    n = W * H * Cc
    want_spans, mask = gm.spans(3, B, W, H, clip_offset=2)
    outs = []
    for inplace in (False, True):
        x = _Clips(data, n + pad)
        y = x if inplace else _Clips(np.full((B, n), 77.0, dtype=np.float32), n + pad)
        spans, fill = _run(gm, x, y, W, H, Cc)
        assert np.array_equal(spans, want_spans), (inplace, spans, want_spans)
        want_fill = fill_of(fill)
        assert np.array_equal(_bits(fill), _bits(want_fill)), (inplace, fill, want_fill)
        got, intact = y.read()
        assert intact
        assert np.array_equal(_bits(got), _bits(_expected(data, mask, fill, Cc))), inplace
        if not inplace:
            src, intact = x.read()
            assert intact and np.array_equal(_bits(src), _bits(data))          # x is never written
        outs.append(got)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    return mask


def _const(value, Cc):
    want = np.zeros((B, 4), dtype=np.float32)
    want[:, :Cc] = value
    return lambda fill: want


# ------------------------------------------------------------------------------------------------ 1. spans, zero and constant fill
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("W,H,Cc", SHAPES)
def test_zero_and_constant_fill_both_forms(W, H, Cc, pad):
    """spans_out equals GridMasking.spans exactly; masked cells hold the fill and all others the input, bit for bit, in the copy and
    in the in-place form; the NaN padding between the clips and the sentinels around the buffers survive; the in-place form on a grid
    full of NaN leaves NaN exactly off the mask and the fill on it (nothing read feeds a store)."""
    rng = np.random.default_rng(W * 1000 + H * 10 + Cc)
    data = _grid(rng, W, H, Cc)
    n = W * H * Cc
    masked = 0
    for fill, value in (("zero", 0.0), (-3.25, -3.25)):
        gm = _masking(W, H, fill)
        mask = _check_both_forms(gm, data, W, H, Cc, pad, _const(value, Cc))
        masked += int(mask.sum())
        x = _Clips(np.full((B, n), np.nan, dtype=np.float32), n + pad)
        _run(gm, x, x, W, H, Cc)
        got, intact = x.read()
        on = np.repeat(mask.reshape(B, -1), Cc, axis=1)
        assert intact and np.isnan(got[~on]).all() and np.array_equal(_bits(got[on]), _bits(np.full(int(on.sum()), value)))
    if W * H >= 100:
        assert 0 < masked < 2 * B * W * H          # the case masks something and leaves something


# ------------------------------------------------------------------------------------------------ 2. the sums and the mean fill
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("W,H,Cc", SHAPES)
def test_sums_against_float64_and_mean_fill(W, H, Cc, pad):
    """cpc_grid_sum within gamma_d * sum |x| of the float64 sums (the module docstring derives d); the mean within the bound that the
    further chunks and the division add; masked cells equal fill_out bit for bit in both forms."""
    rng = np.random.default_rng(7 + W * 1000 + H * 10 + Cc)
    data = _grid(rng, W, H, Cc)
    n = W * H * Cc
    x = _Clips(data, n + pad)
    partial = _sum(x, W, H, Cc).cpu().numpy()
    chunks = partial.shape[1]
    assert chunks == -(-n // 4096)
    worst = 0.0
    for k in range(chunks):
        piece = data[:, 4096 * k:4096 * (k + 1)].astype(np.float64).reshape(B, -1, Cc)
        exact, mag = piece.sum(axis=1), np.abs(piece).sum(axis=1)
        err = np.abs(partial[:, k, :].astype(np.float64) - exact)
        worst = max(worst, float((err / (U * mag)).max()))
        assert (err <= gamma(SUM_DEPTH[Cc]) * mag).all(), (k, err, mag)
    print(f"({W}, {H}, {Cc}) pad {pad}: worst |partial - exact| / (2^-24 sum|x|) = {worst:.3f} (bound {SUM_DEPTH[Cc]})")
    cells = data.astype(np.float64).reshape(B, W * H, Cc)
    mean64, mag = cells.mean(axis=1), np.abs(cells).sum(axis=1) / (W * H)

    def fill_of(fill):
        assert (np.abs(fill[:, :Cc].astype(np.float64) - mean64) <= gamma(SUM_DEPTH[Cc] + chunks) * mag).all(), (fill, mean64)
        assert not fill[:, Cc:].any()
        return fill

    _check_both_forms(_masking(W, H, "mean"), data, W, H, Cc, pad, fill_of)


@pytest.mark.parametrize("W,H,Cc", SHAPES)
def test_sums_and_mean_exact_data(W, H, Cc):
    """Integers in [-8, 8]: every partial is exact (sums below 2^24), so it equals the float64 sum, and fill_out is the float64 mean
    rounded once to float32 (the quotient of two float32 values: rounding it from float64 is the same as rounding it directly)."""
    rng = np.random.default_rng(3 + W * 1000 + H * 10 + Cc)
    data = _grid(rng, W, H, Cc, integers=True)
    n = W * H * Cc
    x = _Clips(data, n + 1)
    partial = _sum(x, W, H, Cc).cpu().numpy()
    for k in range(partial.shape[1]):
        exact = data[:, 4096 * k:4096 * (k + 1)].astype(np.float64).reshape(B, -1, Cc).sum(axis=1)
        assert np.array_equal(partial[:, k, :].astype(np.float64), exact), k
    want = np.zeros((B, 4), dtype=np.float32)
    want[:, :Cc] = (data.astype(np.float64).reshape(B, W * H, Cc).sum(axis=1) / float(W * H)).astype(np.float32)
    _check_both_forms(_masking(W, H, "mean"), data, W, H, Cc, 1, lambda fill: want)


# ------------------------------------------------------------------------------------------------ 3. protected frames, identity
@pytest.mark.parametrize("W,H,Cc", SHAPES)
def test_protect_last(W, H, Cc):
    """protect_last in {0, 1, W - 1, W}: the last frames are never changed, and with protect_last = W the call is the identity."""
    rng = np.random.default_rng(5 + W * 1000 + H * 10 + Cc)
    data = _grid(rng, W, H, Cc)
    for protect_last in sorted({0, 1, W - 1, W}):
        gm = GridMasking(freq_masks=(2, H), time_masks=(2, W), fill="mean", protect_last=protect_last, seed=5)
        mask = _check_both_forms(gm, data, W, H, Cc, 0, lambda fill: fill)
        assert not mask[:, W - protect_last:, :].any()
        if protect_last == W:
            assert not mask.any()


@pytest.mark.parametrize("W,H,Cc", SHAPES)
def test_all_stages_off_is_the_identity(W, H, Cc):
    rng = np.random.default_rng(6 + W * 1000 + H * 10 + Cc)
    data = _grid(rng, W, H, Cc)
    data[0, 0] = np.nan
    data.view(np.int32)[1, 0] = 0x7FC01234          # a NaN with a payload travels as it is
    for fill in ("zero", 1.5, "mean"):
        mask = _check_both_forms(GridMasking(fill=fill), data, W, H, Cc, 1, lambda fill_out: fill_out)
        assert not mask.any()


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("W,H,Cc", SHAPES)
def test_determinism_and_the_two_load_store_routes(W, H, Cc):
    """Two calls give the same bits; clips at 16-byte aligned addresses (ldb a multiple of 4) and the same clips shifted by one float
    (scalar loads and stores) give the same partial sums, fills and grids."""
    rng = np.random.default_rng(8 + W * 1000 + H * 10 + Cc)
    data = _grid(rng, W, H, Cc)
    n = W * H * Cc
    ldb = (n + 3) // 4 * 4
    gm = _masking(W, H, "mean")
    results = []
    for shift in (0, 0, 1):
        x = _Clips(data, ldb, shift)
        y = _Clips(np.zeros((B, n), dtype=np.float32), ldb, shift)
        partial = _sum(x, W, H, Cc).cpu().numpy()
        spans, fill = _run(gm, x, y, W, H, Cc)
        copied, ok_y = y.read()
        spans2, fill2 = _run(gm, x, x, W, H, Cc)
        inplace, ok_x = x.read()
        assert ok_x and ok_y and np.array_equal(spans, spans2)
        results.append((_bits(partial), _bits(fill), _bits(copied), _bits(inplace), _bits(fill2)))
    for other in results[1:]:
        for a, b_ in zip(results[0], other):
            assert np.array_equal(a, b_)
    assert np.array_equal(results[0][2], results[0][3])


# ------------------------------------------------------------------------------------------------ 5. the Python surface
def test_module_call_layouts_and_outputs():
    """GridMasking.__call__ on the (B, Cc, H, W) view and on the contiguous (B, W, H, Cc) tensor, in place and with ``out``."""
    W, H, Cc = 37, 24, 2
    rng = np.random.default_rng(21)
    base = torch.from_numpy(rng.standard_normal((B, W, H, Cc)).astype(np.float32)).to(DEV)
    gm = _masking(W, H, "mean", protect_last=3)
    _, mask = gm.spans(9, B, W, H, clip_offset=4)
    spans = torch.zeros((B, 32), dtype=torch.int32, device=DEV)
    fill = torch.zeros((B, 4), device=DEV)
    out = gm(base, 9, clip_offset=4, out=torch.empty_like(base), spans_out=spans, fill_out=fill)
    assert np.array_equal(spans.cpu().numpy(), gm.spans(9, B, W, H, clip_offset=4)[0])
    want = torch.from_numpy(_expected(base.cpu().numpy().reshape(B, -1), mask, fill.cpu().numpy(), Cc)).view(B, W, H, Cc).to(DEV)
    assert torch.equal(out, want) and 0 < mask.sum() < mask.size
    view = base.clone().permute(0, 3, 2, 1)          # what the preprocessing modules return
    assert gm(view, 9, clip_offset=4) is view and torch.equal(view.permute(0, 3, 2, 1), want)
    out_view = gm(base.permute(0, 3, 2, 1), 9, clip_offset=4, out=torch.empty_like(view))
    assert tuple(out_view.shape) == (B, Cc, H, W) and torch.equal(out_view, view)
    with pytest.raises(ValueError):
        gm(base, 9, out=torch.empty_like(view))          # another layout
    with pytest.raises(ValueError):
        gm(base.permute(0, 2, 1, 3), 9)          # not dense in either reading
    with pytest.raises(_hip.HipCallError):
        gm(base[:-1], 9, out=base[1:])          # two different buffers whose clips overlap


# ------------------------------------------------------------------------------------------------ 6. through the trainer
MEL_SMALL = dict(mel_default_dict, n_fft=256, win_length=256, hop_length=32, n_mels=24)
START = 5


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


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "scalogram_model.npz"))
    meta = json.load(open(os.path.join(golden_dir, "scalogram_model.json")))
    blocks = copy.deepcopy(meta["blocks"])
    for b in blocks:
        b["kernel_size_1"], b["kernel_size_2"] = tuple(b["kernel_size_1"]), tuple(b["kernel_size_2"])
    return {k: z[k] for k in z.files}, meta, blocks


def _front_end(kind, meta):
    if kind == "cqt":
        return PreprocessingModule(cqt_dict=meta["cqt"], **meta["pre"])
    return MelPreprocessingModule(MEL_SMALL, delta=True)


class _MaskingBeforehand(torch.nn.Module):
    """A preprocessing module that masks its own output: call i at step START + i."""

    def __init__(self, pre, gm):
        super().__init__()
        self.pre, self.gm, self.calls = pre, gm, 0

    def forward(self, x):
        grid = self.pre(x)
        self.gm(grid, START + self.calls)
        self.calls += 1
        return grid


def _mask_of_the_run():
    return GridMasking(freq_masks=(2, 6), time_masks=(2, 12), fill="mean", protect_last=2, seed=31)


def _train(fixture, kind, steps=3, masking="unset", wrap=False, ahead=True, start=START, seen=None, score=softplus_score_function):
    """``steps`` steps of the fixture model behind the front end -> (losses, state_dict, trainer)."""
    g, meta, blocks = fixture
    data = torch.from_numpy(g["data"])
    pre = _front_end(kind, meta)
    enc = ScalogramResidualEncoder(args_dict={'phase': True, 'blocks': copy.deepcopy(blocks), 'activation_register': None},
                                   preprocessing_module=pre)
    model = AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=meta["E"], hidden_size=meta["H"]), enc_size=meta["E"],
                                       ar_size=meta["H"], visible_steps=meta["V"], prediction_steps=meta["K"], compute_dtype="fp32")
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    pre, model = pre.to(DEV), model.to(DEV)
    if seen is not None:
        real = model.engine_for

        def recording(x):
            seen.append(x.detach().clone())
            return real(x)
        model.engine_for = recording
    logger = _Logger()
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, device=DEV), logger=logger, device=DEV,
                                      regularization=1.0, score_function=score, prediction_steps=meta["K"],
                                      ar_size=meta["H"], preprocessing=_MaskingBeforehand(pre, _mask_of_the_run()) if wrap else pre,
                                      validation_set=TensorAudioDataset(data, device=DEV))
    tr.verbose = False
    tr.preprocess_ahead = ahead
    if masking != "unset":
        tr.grid_masking = masking
    random.seed(17)
    tr.train(batch_size=meta["B"], epochs=10, lr=1e-3, num_workers=0, continue_training_at_step=start, max_steps=start + steps)
    torch.cuda.synchronize()
    return list(logger.loss_meter.values), {k: v.detach().clone() for k, v in model.state_dict().items()}, tr, pre


def _same_state(s0, s1):
    return set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)


@pytest.mark.parametrize("kind", ["cqt", "mel"])
def test_trainer_without_masking_is_what_it_was(fixture, kind):
    """grid_masking = None leaves losses and parameters bit-identical to a trainer whose attribute was never assigned."""
    l0, s0, _, _ = _train(fixture, kind)
    l1, s1, _, _ = _train(fixture, kind, masking=None)
    assert len(l0) == 3 and all(np.isfinite(l0)) and l0 == l1 and _same_state(s0, s1)


def _own_score(predicted_z, targets):
    """A score function the trainer does not know: the step takes the generic route (autograd bridge, torch's Adam)."""
    return softplus_score_function(predicted_z, targets)


def test_trainer_generic_route_masks_too(fixture):
    """On the generic route the three masked steps equal those of a trainer without masking whose preprocessing module masks
    beforehand, and differ from the plain ones."""
    l_on, s_on, tr, _ = _train(fixture, "cqt", masking=_mask_of_the_run(), score=_own_score)
    assert not tr._fused() and len(l_on) == 3 and all(np.isfinite(l_on))
    l_wrap, s_wrap, _, _ = _train(fixture, "cqt", wrap=True, score=_own_score)
    assert l_on == l_wrap and _same_state(s_on, s_wrap)
    l_plain, _, _, _ = _train(fixture, "cqt", score=_own_score)
    assert l_plain != l_on


_RUNS = {}


def _masked_run(fixture, kind):
    """The run with masking on that the tests below share: (losses, state_dict, trainer, front end, the engine's inputs)."""
    if kind not in _RUNS:
        seen = []
        _RUNS[kind] = _train(fixture, kind, masking=_mask_of_the_run(), seen=seen) + (seen,)
    return _RUNS[kind]


@pytest.mark.parametrize("kind", ["cqt", "mel"])
def test_trainer_masks_batch_i_at_its_step(fixture, kind):
    """With masking on and continue_training_at_step = 5 the engine receives mask(preprocess(batch i), step = 5 + i) bit for bit, and
    the three steps give the losses and parameters of a trainer without masking whose preprocessing module masks beforehand."""
    g, meta, _ = fixture
    data = torch.from_numpy(g["data"])
    l_on, s_on, _, pre, seen = _masked_run(fixture, kind)
    assert len(seen) == 3 and len(l_on) == 3 and all(np.isfinite(l_on))
    random.seed(17)
    batches = [list(b) for b in FileBatchSampler([data.shape[0]], meta["B"], 1, True, verbose=False)]
    gm = _mask_of_the_run()
    masked_cells = 0
    for i, x in enumerate(seen):
        with torch.no_grad():
            grid = pre(data[batches[i]].to(DEV).unsqueeze(1))
        Bt, Cc, H, W = grid.shape
        want = gm(grid, START + i, out=torch.empty_like(grid))
        assert torch.equal(x.view(torch.int32), want.view(torch.int32)), i
        mask = gm.spans(START + i, Bt, W, H)[1]
        assert not torch.equal(want, grid) and not mask[:, W - 2:, :].any()
        assert torch.equal(want[:, :, :, W - 2:], grid[:, :, :, W - 2:])          # the protected frames
        masked_cells += int(mask.sum())
    assert masked_cells > 0
    l_wrap, s_wrap, _, _ = _train(fixture, kind, wrap=True)
    assert l_on == l_wrap and _same_state(s_on, s_wrap)


@pytest.mark.parametrize("kind", ["cqt", "mel"])
def test_trainer_preprocess_ahead_and_validate(fixture, kind):
    """preprocess_ahead on and off give identical losses and parameters with masking on; the masked run differs from the plain one;
    validate() is identical with and without grid_masking set."""
    l_on, s_on, tr, _, _ = _masked_run(fixture, kind)
    l_off, s_off, _, _ = _train(fixture, kind, masking=_mask_of_the_run(), ahead=False)
    assert l_on == l_off and _same_state(s_on, s_off)
    l_plain, _, _, _ = _train(fixture, kind, masking=None)
    assert l_plain != l_on
    results = []
    for masking in (_mask_of_the_run(), None):
        tr.grid_masking = masking
        random.seed(3)
        results.append(tr.validate(batch_size=8, num_workers=0))
    assert len(results[0]) == len(results[1]) == 4
    for a, b_ in zip(*results):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b_))
