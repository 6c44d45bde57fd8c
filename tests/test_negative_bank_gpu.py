"""The negative bank on the HIP path: cpc_nce_loss_banked against the float64 restatement of tests/negative_bank_reference.py and
against cpc_nce_loss where only the current slot is valid, the engine route against the CPU oracle model with the banked loss on its
outputs (earlier steps' predictions detached), bf16 storage, and the trainer.

Bounds of the kernel tests, derived from the f32 operations of the summation path (u = 2^-24, one rounding; a library function —
expf, logf, log1pf — counted as 4 u; A = max |sp| over the valid rows, N the ring's rows, C = NBK_CHUNK, c = valid chunks):
  sum of a column's exponentials: C online steps of (multiply, add, expf with a rounded argument) and c merge steps of the same, on
      terms whose own sp carries 4 u A (softplus):                     rel <= (8 C + 8 c + 4 A + 40) u
  lse = m + logf(sum):                                                 abs d_lse <= rel + (4 ln N + A) u
  softmax term exp(sp - lse): argument off by d_lse + 6 u A, expf 4 u:  rel E_p <= d_lse + (6 A + 4) u
  coefficient: E_p + 12 u (f', products) on a term <= 1 / (B K), plus the regulariser's 2 reg / (B^2 K) A (K + 10) u;
      bf16 storage adds one rounding, 2^-8 of the value
  -mean valid: A (K + 23 + P / 256) u;  mean lse: d_lse + A (18 + Q / 256) u;  regulariser: reg A^2 (2 K + 32 + P / 256) u
      (P pair partials, Q column partials: the sequential part of the fixed-order reductions; 8 levels per 256-wide tree)
  max score: 4 u A."""
import ctypes as C
import functools
import json
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler, TensorAudioDataset
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import ContrastiveEstimationTrainer, NormalizedScoreFunction, softplus_score_function
from cpc_audio_amd.engine import FusedAdam, NegativeBank
from oracle import cpc_oracle as O

import negative_bank_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U64 = C.c_ulonglong
SENTINEL = -8192.0          # exact in f32 and bf16
TAIL = 64
NAN = float("nan")
NBK_CHUNK = 32              # csrc/nce.hip: rows per (max, sum) pair of the partial pass
NEW_ENTRY_POINTS = {"cpc_nce_loss_banked", "cpc_nce_banked_workspace_floats"}
U = 2.0 ** -24


def _guarded(shape, fill, dtype=torch.float32):
    """A device buffer of ``shape`` holding ``fill`` with TAIL sentinel elements behind it: (view, whole)."""
    n = int(np.prod(shape))
    whole = torch.full((n + TAIL,), SENTINEL, device=DEV, dtype=dtype)
    whole[:n] = fill.to(DEV).reshape(-1) if torch.is_tensor(fill) else fill
    return whole[:n].view(*shape), whole


def _tails_intact(*wholes):
    return all(bool((w[-TAIL:] == SENTINEL).all()) for w in wholes)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _rel_l2(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


def _ld(B):
    return (B + 7) // 8 * 8


def _bounds(B, K, slots, valid, A, reg):
    """The bounds of the module docstring: dict of absolute bounds for out[0..4] and the coefficients (f32)."""
    N = slots * B
    c = bin(valid).count("1") * -(-B // NBK_CHUNK)
    P, Q = -(-B * B // 256), -(-K * B // 256)
    d_lse = (8 * NBK_CHUNK + 8 * c + 4 * A + 40) * U + (4 * math.log(N) + A) * U
    e_p = d_lse + (6 * A + 4) * U
    t_valid = A * (K + 23 + P / 256) * U
    t_lse = d_lse + A * (18 + Q / 256) * U
    t_reg = reg * A * A * (2 * K + 32 + P / 256) * U
    grad = (e_p + 12 * U) / (B * K) + 2 * reg / (B * B * K) * A * (K + 10) * U
    return dict(loss=t_valid + t_lse + t_reg, smax=4 * U * A, t_valid=t_valid, t_lse=t_lse, t_reg=t_reg, grad=grad)


# ------------------------------------------------------------------------------------------ kernel cases
def _scores(B, K, slots):
    """randn * 3 with +80 and -80 planted in slot 0 and in the last slot, on and off the diagonal, and in every other column of step
    0 a row of the LAST slot that dominates its column (40 above everything else there): the online max moves late in the row order."""
    g = torch.Generator().manual_seed(B * 13 + K * 5 + slots)
    N = slots * B
    S = torch.randn(K, N, B, generator=g) * 3.0
    S[0, 0, 0] = 80.0
    S[K - 1, B - 1, 0] = -80.0
    S[K - 1, (slots - 1) * B + B - 1, B - 1] = 80.0
    S[0, (slots - 1) * B, B - 1] = -80.0
    for bp in range(1, B - 1, 2):
        S[0, N - 1 - (bp % B), bp] = 40.0
    return S


def _patterns(slots):
    """(cur, valid): only cur; all slots with cur first, (middle,) last; with three slots also a hole in the middle."""
    if slots == 2:
        return [(0, 0b01), (1, 0b10), (0, 0b11), (1, 0b11)]
    return [(0, 0b001), (0, 0b111), (1, 0b111), (2, 0b111), (0, 0b101), (2, 0b101)]


@functools.lru_cache(maxsize=None)
def _case(B, K, slots, cur, valid, softplus, reg):
    """(scores, float64 reference) of a case, computed once and shared by the storage types; nothing writes to either."""
    S = _scores(B, K, slots)
    return S, R.banked_reference(S, B, cur, valid, softplus, reg)


def _launch(S, B, K, ld, slots, cur, valid, softplus, reg, dt):
    """One guarded launch of cpc_nce_loss_banked on S [K][N][B]: the sentinel in the scores' pad columns [B, ld) and behind every
    buffer (the workspace included), NaN-prefilled outputs.  Checks that the input kept its bits — pad columns and all —, that nothing
    behind a buffer changed, that dS / dST_cur hold zeros in their pad columns (include/cpc_hip.h) and that the rows of invalid slots
    are zero coefficients.  Returns (out, dS [K][N][B], dST_cur [K][B][B]) on the host."""
    N = slots * B
    Sp = torch.full((K, N, ld), SENTINEL)
    Sp[:, :, :B] = S
    S_d, S_w = _guarded((K, N, ld), Sp)
    dS, dS_w = _guarded((K, N, ld), NAN, dt)
    dST, dST_w = _guarded((K, B, ld), NAN, dt)
    out, out_w = _guarded((8,), NAN)
    ws, ws_w = _guarded((int(_hip.lib().cpc_nce_banked_workspace_floats(B, K, slots)),), NAN)
    P = _hip.ptr
    _hip.call("cpc_nce_loss_banked", P(S_d), P(dS), P(dST), P(out), P(ws), B, K, ld, slots, cur, U64(valid), softplus, C.c_float(reg),
              _hip.dtype_code(dt))
    torch.cuda.synchronize()
    assert _tails_intact(S_w, dS_w, dST_w, out_w, ws_w)
    assert _same_bits(S_d.cpu(), Sp), "the scores changed"
    assert bool((S_d[:, :, B:] == SENTINEL).all())
    assert bool((dS[:, :, B:] == 0).all()) and bool((dST[:, :, B:] == 0).all())
    rows = R.row_mask(B, slots, valid)
    assert bool((dS[:, ~rows.to(DEV), :] == 0).all()), "an invalid slot has coefficients"
    return out.cpu(), dS[:, :, :B].cpu(), dST[:, :, :B].cpu()


def _check(B, K, slots, cur, valid, softplus, reg, dt, ld=None):
    S, ref = _case(B, K, slots, cur, valid, softplus, reg)
    ld = _ld(B) if ld is None else ld
    out, dS, dST = _launch(S, B, K, ld, slots, cur, valid, softplus, reg, dt)
    rows = R.row_mask(B, slots, valid)
    A = max(1.0, ref["sp"][:, rows, :].abs().max().item())
    tol = _bounds(B, K, slots, valid, A, reg)
    errs = {name: abs(out[i].item() - ref["out"][i]) for i, name in enumerate(("loss", "smax", "t_valid", "t_lse", "t_reg"))}
    round_ = 2.0 ** -8 if dt == torch.bfloat16 else 0.0
    e_s = ((dS.double() - ref["dS"]).abs() - round_ * ref["dS"].abs()).max().item()
    e_t = ((dST.double() - ref["dST_cur"]).abs() - round_ * ref["dST_cur"].abs()).max().item()
    print(f"banked B={B} K={K} slots={slots} cur={cur} valid={valid:#b} softplus={softplus} {dt}: errors "
          + " ".join(f"{k} {v:.2e}/{tol[k]:.2e}" for k, v in errs.items()) + f" dS {e_s:.2e} dST {e_t:.2e}/{tol['grad']:.2e}")
    for name, err in errs.items():
        assert err <= tol[name], (name, err, tol[name])
    assert out[5].item() == 0.0 and math.isnan(out[6].item()) and math.isnan(out[7].item())
    assert e_s <= tol["grad"] and e_t <= tol["grad"]
    # the current slot's transposed copy is the same bits as its rows
    assert _same_bits(dST, dS[:, cur * B:(cur + 1) * B, :].transpose(1, 2).contiguous())
    return out, dS, dST


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [2, 33, 64, 65])
def test_banked_loss_against_float64(B, K, slots, softplus, dt):
    """B = 2: the smallest batch; 33 (ld 40): one row past a chunk boundary and pad columns; 64: whole chunks and one full wave of
    columns; 65: a second wave of columns, three 32 x 32 tiles per side.  Every validity pattern of _patterns; the second launch of
    the first pattern gives the same bits."""
    reg = 0.5 if K > 1 else B / 4.0
    for i, (cur, valid) in enumerate(_patterns(slots)):
        first = _check(B, K, slots, cur, valid, softplus, reg, dt)
        if i == 0:
            again = _check(B, K, slots, cur, valid, softplus, reg, dt)
            for a, b in zip(first, again):
                assert _same_bits(a[:6] if a.numel() == 8 else a, b[:6] if b.numel() == 8 else b)


def _chunk_from_workspace():
    """The kernel's rows per chunk, read off cpc_nce_banked_workspace_floats: one more slot adds 2 ceil(B / chunk) K B floats, so the
    chunk is the largest B whose slot still takes one chunk."""
    ws = _hip.lib().cpc_nce_banked_workspace_floats
    one = [B for B in range(2, 1025) if ws(B, 1, 3) - ws(B, 1, 2) == 2 * B]
    return max(one)


@pytest.mark.parametrize("B", [NBK_CHUNK - 1, NBK_CHUNK + 1, 2 * NBK_CHUNK + 1])
def test_chunk_boundary_of_the_partial_pass(B):
    """A slot's rows end one row before a chunk boundary, one row behind it (a chunk of a single row) and one row behind the second
    (NBK_CHUNK here is the library's own: a changed constant fails the first line instead of moving the boundary off the sizes)."""
    assert _chunk_from_workspace() == NBK_CHUNK
    for softplus in (0, 1):
        _check(B, 2, 3, 1, 0b111, softplus, 0.5, torch.float32)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,ld", [(32, 39), (64, 71), (31, 38)])
def test_pad_columns_that_reach_into_a_tile_of_their_own(B, ld, dt):
    """ld = B + 7 where ceil(ld / 32) > ceil(B / 32): the pad columns [B, ld) of dST_cur lie in a row tile that holds no row of dS,
    and must still come back as zeros from NaN-prefilled buffers (_launch checks every pad column of dS and dST_cur)."""
    for cur, valid in ((1, 0b111), (0, 0b101), (2, 0b100)):
        _check(B, 2, 3, cur, valid, 1, 0.5, dt, ld=ld)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_sixty_four_slots(dt):
    """B = 4, slots = 64: mask bit 63, cur as the last slot; all slots valid, and every second one."""
    for cur, valid in ((63, 2 ** 64 - 1), (63, int("10" * 32, 2)), (0, 1 | 1 << 63)):
        _check(4, 3, 64, cur, valid, 1, 0.5, dt)


def test_nan_in_a_stale_slot_reaches_the_loss():
    """A NaN score in a valid stale slot raises out[5] and the sticky out[6] (a chunk of NaNs alone included); in an invalid slot it
    is never read."""
    B, K, slots = 33, 2, 3
    S = _scores(B, K, slots).clone()
    S[1, 2 * B + 32, 5] = NAN                    # row 32 of slot 2: the single-row chunk
    out, _, _ = _launch(S, B, K, _ld(B), slots, 0, 0b111, 0, 0.5, torch.float32)
    assert math.isnan(out[0].item()) and out[5].item() == 1.0 and out[6].item() == 1.0
    out, dS, _ = _launch(S, B, K, _ld(B), slots, 0, 0b011, 0, 0.5, torch.float32)
    ref = R.banked_reference(S, B, 0, 0b011, 0, 0.5)
    assert out[5].item() == 0.0 and abs(out[0].item() - ref["loss"]) <= _bounds(B, K, slots, 0b011, 80.0, 0.5)["loss"]
    assert not torch.isnan(dS).any()


# ------------------------------------------------------------------------------------------ identity with cpc_nce_loss
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,slots,cur", [(33, 3, 3, 1), (65, 1, 2, 1), (2, 3, 2, 0)])
def test_only_the_current_slot_is_the_dense_loss(B, K, slots, cur, softplus, dt):
    """valid = 1 << cur: out[], the coefficients of slot cur and dST_cur equal cpc_nce_loss's on that slot's scores within the
    derived bound (the two kernels sum a column's exponentials in different orders)."""
    reg, ld = 0.5, _ld(B)
    S = _scores(B, K, slots)
    out, dS, dST = _launch(S, B, K, ld, slots, cur, 1 << cur, softplus, reg, dt)
    own = S[:, cur * B:(cur + 1) * B, :]
    Sp = torch.full((K, B, ld), 7.0)
    Sp[:, :, :B] = own
    S_d = Sp.to(DEV)
    d_dS, d_dST = (torch.full((K, B, ld), NAN, device=DEV, dtype=dt) for _ in range(2))
    d_out = torch.full((8,), NAN, device=DEV)
    ws = torch.empty(int(_hip.lib().cpc_nce_workspace_floats(B, K)), device=DEV)
    P = _hip.ptr
    _hip.call("cpc_nce_loss", P(S_d), P(d_dS), P(d_dST), P(d_out), P(ws), B, K, ld, softplus, C.c_float(reg), _hip.dtype_code(dt))
    torch.cuda.synchronize()
    sp = F.softplus(own.double()) if softplus else own.double()
    tol = _bounds(B, K, slots, 1 << cur, max(1.0, sp.abs().max().item()), reg)
    d_out = d_out.cpu()
    for i, name in enumerate(("loss", "smax", "t_valid", "t_lse", "t_reg")):
        assert abs(out[i].item() - d_out[i].item()) <= tol[name], name
    assert out[5].item() == d_out[5].item() == 0.0
    round_ = 2.0 ** -8 if dt == torch.bfloat16 else 0.0
    for got, want in ((dS[:, cur * B:(cur + 1) * B, :], d_dS[:, :, :B].cpu()), (dST, d_dST[:, :, :B].cpu())):
        assert ((got.double() - want.double()).abs() - round_ * want.double().abs()).max().item() <= tol["grad"]


# ------------------------------------------------------------------------------------------ engine against the oracle
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def _small(golden_dir):
    g = _load(golden_dir, "small_model.npz")
    meta = json.load(open(os.path.join(golden_dir, "small_model.json")))
    params = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    return g, meta, torch.from_numpy(g["data"]), params


def _small_model(g, meta, dtype):
    C_, H, K, V = meta["C"], meta["H"], meta["K"], meta["V"]
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [C_] * 5, 'bias': True})
    ar = AudioGRUModel(input_size=C_, hidden_size=H)
    model = AudioPredictiveCodingModel(enc, ar, enc_size=C_, ar_size=H, visible_steps=V, prediction_steps=K, compute_dtype=dtype)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return model.to(DEV)


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


class _OracleBank:
    """The oracle's side of the engine test: the oracle model's forward pass, the score operands of ``kind``, a host mirror of the
    ring fed with the oracle's own detached operands of the earlier steps, and the reference loss differentiated by autograd."""

    def __init__(self, params, meta, kind, reg, slots_back, tau=None):
        self.ot = O.OracleTrainer(params, meta["V"], meta["K"], score="linear", regularization=reg)
        self.kind, self.reg, self.tau = kind, reg, tau
        self.slots, self.cur, self.valid, self.rows = slots_back + 1, 0, 1, None

    def step(self, batch):
        ot = self.ot
        for p in ot.params.values():
            p.grad = None
        pred, targ, _, _ = O.cpc_forward(batch.unsqueeze(1), {**ot.params, **ot.buffers}, ot.V, ot.K, ot.strides, ot.conv_ar, ot.attention,
                                         ot.scalogram, ar_resnet=ot.ar_resnet)
        if self.kind == "normalized":
            pred, targ = F.normalize(pred, dim=2, eps=1e-8) / self.tau, F.normalize(targ, dim=1, eps=1e-8)
        if self.rows is None:
            self.rows = [torch.zeros_like(pred) for _ in range(self.slots)]
        self.rows[self.cur] = pred
        loss, smax = R.banked_loss(torch.cat(self.rows), targ, self.cur, self.valid, self.kind == "softplus", self.reg)
        loss.backward()
        self.rows[self.cur] = pred.detach()
        self.cur = (self.cur + 1) % self.slots
        self.valid |= 1 << self.cur
        return float(loss.detach()), float(smax.detach()), {k: p.grad for k, p in ot.params.items()}


def _operands(eng, kind):
    return (eng._norm.pn if kind == "normalized" else eng.pred).detach().clone()


@pytest.mark.parametrize("kind", ["linear", "softplus", "normalized"])
def test_engine_four_steps_against_oracle(golden_dir, kind):
    """fp32, M = 2, four steps on four batches (the ring wraps at the fourth): loss and every parameter gradient of every step vs
    autograd of the oracle model with the reference loss on its outputs (1e-4 / 1e-3 relative L2, the project's f32 bounds); the
    first step runs cpc_nce_loss itself, the later ones cpc_nce_loss_banked; the ring's stale slots are the saved operands of the
    last two steps bit for bit."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "fp32")
    B, K, reg = meta["B"], meta["K"], 0.5
    eng = model.engine(B, data.shape[1])
    bank = NegativeBank(2)
    kw = {"temperature": 0.1} if kind == "normalized" else {}
    ob = _OracleBank(params, meta, kind, reg, 2, tau=0.1)
    saved, in_batch = [], None
    for i in range(4):
        x = data[i * B:(i + 1) * B]
        cur = bank.cur
        with _Spy() as spy:
            out = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=reg, score=kind, negative_bank=bank, **kw)
        torch.cuda.synchronize()
        if i == 0:
            assert spy.names.count("cpc_nce_loss") == 1 and "cpc_nce_loss_banked" not in spy.names
        else:
            assert spy.names.count("cpc_nce_loss_banked") == 1 and "cpc_nce_loss" not in spy.names
        saved.append(_operands(eng, kind))
        assert bank.filled == min(i + 1, 2) and bank.cur == (i + 1) % 3
        assert _same_bits(bank.slot(cur).reshape(-1), saved[-1].reshape(-1))
        loss, smax, grads = ob.step(x)
        print(f"{kind} step {i}: loss {float(out[0]):.7f} oracle {loss:.7f}")
        assert abs(float(out[0]) - loss) < 1e-4 * abs(loss), (i, float(out[0]), loss)
        assert abs(float(out[1]) - smax) < 1e-4 * abs(smax) + 1e-6
        for name, ref in grads.items():
            assert _rel_l2(model._grad[name], ref) < 1e-3, (i, name)
        if i == 3:          # what the bank adds is visible at this size
            in_batch = eng.loss_and_grads(x.to(DEV), softplus=kind == "softplus", regularization=reg, score=kind, **kw)
            assert abs(float(in_batch[0]) - loss) > 1e-3 * abs(loss)
    # steps 2 and 3 are the stale slots now (step 3 in slot 0, step 2 in slot 2), slot 1 waits for the next step
    assert bank.cur == 1
    assert _same_bits(bank.slot(0).reshape(-1), saved[3].reshape(-1)) and _same_bits(bank.slot(2).reshape(-1), saved[2].reshape(-1))
    other = NegativeBank(2)
    other.bind(B + 1, K, eng.E, eng.dt, eng.device)
    with pytest.raises(ValueError, match="negative bank"):
        eng.nce_forward_backward(kind == "softplus", reg, score=kind, negative_bank=other, **kw)


@pytest.mark.parametrize("dtype,slots,nsplit", [("fp32", 12, 2), ("bf16", 33, 2)])
def test_slab_route_of_the_target_contraction(golden_dir, dtype, slots, nsplit):
    """_score_grads(rows=slots B, nsplit > 1) — f32 slabs over the ring's rows, cpc_reduce_slabs, in bf16 one cast — against the
    direct contraction (nsplit = 1) on random coefficients and rows: the same sums, in f32 storage to 1e-5 of the largest element
    (other summation order), in bf16 to one bf16 rounding (2^-8).  The ring is long enough for every slab to hold rows (72 rows in
    two slabs of 64 and 8; 198 rows in two of 128 and 70); d predicted_z is the same bits on both routes.  _bank_nsplit picks
    slabs only from 512 (f32) / 1024 (bf16) rows on, which the small model's engine steps never reach."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, dtype)
    B, K = meta["B"], meta["K"]
    eng = model.engine(B, data.shape[1])
    eng.forward(data[:B].to(DEV))
    assert eng._bank_nsplit(B * 3) == 1 and eng._bank_nsplit(4352) == 8 and eng._bank_nsplit(1280) == (2 if dtype == "bf16" else 8)
    assert eng._bank_nsplit(512) == (1 if dtype == "bf16" else 8)
    for rows in range(2, 5000, 7):          # no empty slab, whatever the rows
        n = eng._bank_nsplit(rows)
        assert 1 <= n <= 8 and (n - 1) * eng._chunk(rows, n) < rows
    N, ld, gen = slots * B, eng.ldS, torch.Generator().manual_seed(slots)
    ring = (torch.randn(N, K, eng.E, generator=gen) * 0.5).to(DEV, eng.dt)
    W = torch.zeros(K, N, ld)
    W[:, :, :B] = torch.randn(K, N, B, generator=gen) * 1e-2
    W, WT = W.to(DEV, eng.dt), torch.zeros(K, B, ld, device=DEV, dtype=eng.dt)
    top, dtop, dpred, T, Ltop = eng.act[-1], eng.dact[-1], eng.dpred, eng.T, eng.geo.alloc[-1]
    rows_of = lambda: dtop.view(B, Ltop, eng.E)[:, T - K:T, :].float().clone()
    before = dtop.clone()
    eng._score_grads(W, WT, ring, top, dpred, dtop, rows=N)
    direct, dp = rows_of(), dpred.clone()
    dtop.copy_(before)
    eng._score_grads(W, WT, ring, top, dpred, dtop, rows=N, nsplit=nsplit)
    torch.cuda.synchronize()
    slab = rows_of()
    rel = ((slab - direct).abs().max() / direct.abs().max()).item()
    print(f"slab route {dtype} rows {N} nsplit {nsplit}: max difference {rel:.2e} of the largest element")
    assert direct.abs().max().item() > 0 and rel <= (1e-5 if dtype == "fp32" else 2.0 ** -8)
    assert _same_bits(dpred, dp)
    other = torch.ones_like(dtop, dtype=torch.bool).view(B, Ltop, eng.E)
    other[:, T - K:T, :] = False
    assert _same_bits(dtop.view(B, Ltop, eng.E)[other], before.view(B, Ltop, eng.E)[other])          # only the K target rows were written


def test_engine_bf16_against_oracle(golden_dir):
    """bf16 storage, M = 2, every one of three steps (the third with two stale slots, the ring full) against the f32 oracle, with
    the bounds and the score kind of the sibling they come from (test_engine_normalized_bf16): normalized scores at temperature 0.1, 1e-3 on the loss and
    0.12 on the worst per-parameter gradient relative L2.  The bank's rows are the engine's own bf16 operands (the copy into the
    ring rounds nothing), the oracle's are its own f32 ones.

    Why this score kind: the 1e-3 loss bound is one the engine's bf16 step has for normalized scores only.  Measured on an MI355X,
    the step WITHOUT a bank (code this test does not cover) against its oracle on the four golden batches: normalized 2.2e-4,
    2.5e-4, 9.1e-5, 3.1e-4; softplus 2.8e-4, 6.2e-3, 3.1e-4, 5.0e-3; linear 1.2e-3, 2.5e-3, 2.7e-3, 1.3e-4 — unbounded scores of
    size 10 - 25 carry a bf16 rounding of 2^-9 each, and the sibling tests of those kinds assert on the first batch alone.  A bank
    needs several batches, so the bound can only be asked where the in-batch step keeps it on every one of them.
    Measured with the bank: normalized 2.2e-4 / 9.6e-4 / 1.3e-4 at steps 0 / 1 / 2 (gradient 0.058 / 0.077 / 0.108); for the record,
    softplus 2.8e-4 / 2.2e-3 / 3.1e-3 (gradient 0.093 / 0.061 / 0.088), of the size of its in-batch error on the same batches."""
    g, meta, data, params = _small(golden_dir)
    model = _small_model(g, meta, "bf16")
    B, reg = meta["B"], 0.5
    eng = model.engine(B, data.shape[1])
    bank = NegativeBank(2)
    ob = _OracleBank(params, meta, "normalized", reg, 2, tau=0.1)
    for i in range(3):
        x = data[i * B:(i + 1) * B]
        out = eng.loss_and_grads(x.to(DEV), softplus=False, regularization=reg, score="normalized", temperature=0.1, negative_bank=bank)
        torch.cuda.synchronize()
        loss, smax, grads = ob.step(x)
        rel = abs(float(out[0]) - loss) / abs(loss)
        worst = max((_rel_l2(model._grad[name], ref), name) for name, ref in grads.items())
        print(f"bf16 negative bank step {i}: loss rel {rel:.2e}, worst gradient rel-L2 {worst[0]:.3e} ({worst[1]})")
        assert rel < 1e-3, (i, rel)
        assert worst[0] < 0.12, (i, worst)
    assert bank.filled == 2


# ------------------------------------------------------------------------------------------ trainer
COUNTS = [8, 8, 8]


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


def _trainer(model, data, meta, logger, score_function=softplus_score_function):
    tr = ContrastiveEstimationTrainer(model=model, dataset=TensorAudioDataset(data, counts=COUNTS, device=DEV), logger=logger, device=DEV,
                                      regularization=0.5, score_function=score_function, prediction_steps=meta["K"], ar_size=meta["H"],
                                      file_batch_size=2)
    tr.verbose = False
    return tr


def _batches(meta, seed=5):
    random.seed(seed)
    return [list(b) for b in FileBatchSampler(COUNTS, meta["B"], 2, True, verbose=False)]


def _by_hand(g, meta, data, steps, lr, bank, score="softplus", **kw):
    """The steps train() runs, driven by hand: the engine with ``negative_bank=bank`` (None: without the keyword), FusedAdam behind."""
    batches = _batches(meta)
    model = _small_model(g, meta, "fp32")
    model.train()
    model._flatten_parameters(DEV)
    opt = FusedAdam(model, lr=lr)
    model.link_grads()
    dev_data = data.to(DEV)
    losses = []
    bkw = {} if bank is None else {"negative_bank": bank}
    for i in range(steps):
        x = dev_data[torch.as_tensor(batches[i], device=DEV)].contiguous()
        eng = model.engine(x.shape[0], x.shape[1], DEV)
        if i == 0:
            eng.nan_flag().zero_()
        opt.after_update = eng.prepare_ahead
        opt.skip_flag = eng.nan_flag()
        out = eng.loss_and_grads(x, softplus=score == "softplus", regularization=0.5, all_timesteps=False, grad_ready_hook=opt.hook,
                                 global_negatives=None, after_loss=None, score=score, **kw, **bkw)
        opt.step(grad_scale=1.0)
        losses.append(float(out[0]))
    torch.cuda.synchronize()
    return model, losses


def _same_state(model, model0):
    for (k, v), (k0, v0) in zip(model.state_dict().items(), model0.state_dict().items()):
        assert k == k0 and torch.equal(v, v0), k


@pytest.mark.parametrize("score", ["softplus", "normalized"])
def test_trainer_four_steps_are_the_hand_driven_steps(golden_dir, score):
    """negative_bank = 2 through train() for four steps: losses and parameters equal the hand-driven engine steps bit for bit."""
    g, meta, data, params = _small(golden_dir)
    steps, lr = 4, 1e-3
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger, softplus_score_function if score == "softplus" else NormalizedScoreFunction(0.1))
    tr.negative_bank = 2
    random.seed(5)
    with _Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=lr, num_workers=0, max_steps=steps)
    assert spy.names.count("cpc_nce_loss") == 1 and spy.names.count("cpc_nce_loss_banked") == steps - 1
    assert tr.negative_bank_filled == 2 and tr.training_step == steps
    kw = {"temperature": 0.1} if score == "normalized" else {}
    model0, losses = _by_hand(g, meta, data, steps, lr, NegativeBank(2), score=score, **kw)
    assert logger.loss_meter.values == losses
    _same_state(model, model0)
    _, plain = _by_hand(g, meta, data, steps, lr, None, score=score, **kw)
    assert plain[0] == losses[0] and all(a != b for a, b in zip(plain[1:], losses[1:]))


def test_step_without_bank_is_the_parent_step(golden_dir):
    """negative_bank = None: no new entry point is reached, and losses and parameters after two steps are bit-identical to the step
    as it was before the attribute existed — the engine called without the keyword, FusedAdam behind it."""
    g, meta, data, params = _small(golden_dir)
    steps, lr = 2, 1e-3
    model = _small_model(g, meta, "fp32")
    logger = _Logger()
    tr = _trainer(model, data, meta, logger)
    assert tr.negative_bank is None
    random.seed(5)
    with _Spy() as spy:
        tr.train(batch_size=meta["B"], epochs=1, lr=lr, num_workers=0, max_steps=steps)
    assert not NEW_ENTRY_POINTS & set(spy.names) and spy.names.count("cpc_nce_loss") == steps
    assert tr.negative_bank_filled == 0 and tr._bank is None
    model0, losses = _by_hand(g, meta, data, steps, lr, None)
    assert logger.loss_meter.values == losses
    _same_state(model, model0)


def test_first_banked_step_and_the_step_after_a_reset_are_in_batch(golden_dir):
    """The first step with a bank is the unbanked step bit for bit (loss and parameters); after two more steps the bank is full, and
    reset_negative_bank() makes the next step in-batch again: it runs cpc_nce_loss, and its loss is the unbanked trainer's."""
    g, meta, data, params = _small(golden_dir)
    B, lr = meta["B"], 1e-3
    runs = []
    for bank in (2, None):
        model = _small_model(g, meta, "fp32")
        logger = _Logger()
        tr = _trainer(model, data, meta, logger)
        tr.negative_bank = bank
        random.seed(5)
        tr.train(batch_size=B, epochs=1, lr=lr, num_workers=0, max_steps=1)
        runs.append((tr, model, logger))
    (tr, model, logger), (tr0, model0, logger0) = runs
    assert logger.loss_meter.values == logger0.loss_meter.values and tr.negative_bank_filled == 1
    _same_state(model, model0)
    # lr = 0 from here on: both models keep these parameters, so the losses of later steps can be compared
    random.seed(5)
    tr.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=3, continue_training_at_step=1)
    assert tr.negative_bank_filled == 2
    tr.reset_negative_bank()
    assert tr.negative_bank_filled == 0
    for t in (tr, tr0):
        random.seed(5)
        with _Spy() as spy:
            t.train(batch_size=B, epochs=1, lr=0.0, num_workers=0, max_steps=4, continue_training_at_step=3)
        assert spy.names.count("cpc_nce_loss") == 1 and "cpc_nce_loss_banked" not in spy.names
    assert logger.loss_meter.values[-1] == logger0.loss_meter.values[-1] and tr.negative_bank_filled == 1
