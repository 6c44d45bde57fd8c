"""The negative bank, the part that needs no GPU: the argument checks of cpc_nce_banked_workspace_floats / cpc_nce_loss_banked (raised
before any launch, so the pointers are never dereferenced), every refusal of the engines and of the trainer (raised before any GPU
work), the ValueErrors for a bad M and for a change of sizes, the ring's bookkeeping, and the float64 reference of
tests/negative_bank_reference.py against the closed form of its own definition."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, NormalizedScoreFunction, TemperatureSchedule,
                                                           difference_score_function, linear_score_function)
from cpc_audio_amd.engine import (CPCEngine, DeviceTemperature, GraphedStep, NegativeBank, check_negative_bank_supported,
                                  select_negatives)
from cpc_audio_amd.scalogram_engine import ScalogramCPCEngine

import negative_bank_reference as R

U64 = C.c_ulonglong


# ------------------------------------------------------------------------------------------ the entry points
def _banked(**kw):
    """cpc_nce_loss_banked with never-dereferenced pointers and one argument changed from an admissible call."""
    P = C.c_void_p(0x1000)          # 8-byte aligned
    a = dict(S=P, dS=P, dST=P, out=P, ws=P, B=8, K=2, ld=8, slots=3, cur=1, valid=0b011, softplus=0, reg=0.5, dtype=_hip.F32)
    a.update(kw)
    return _hip.lib().cpc_nce_loss_banked(a["S"], a["dS"], a["dST"], a["out"], a["ws"], a["B"], a["K"], a["ld"], a["slots"], a["cur"],
                                          U64(a["valid"]), a["softplus"], C.c_float(a["reg"]), a["dtype"], None)


@pytest.mark.parametrize("case", [dict(S=None), dict(dS=None), dict(dST=None), dict(out=None), dict(ws=None),
                                  dict(B=1, ld=8), dict(B=0), dict(B=1025, ld=1025), dict(K=0), dict(K=1025),
                                  dict(slots=1, cur=0, valid=1), dict(slots=65), dict(slots=0),
                                  dict(cur=3), dict(cur=-1), dict(valid=0b101), dict(valid=0), dict(valid=0b1011), dict(valid=1 << 63 | 0b10),
                                  dict(ld=7), dict(ld=16), dict(dtype=2), dict(dtype=-1), dict(ws=C.c_void_p(0x1004))],
                         ids=lambda c: ",".join(f"{k}={'NULL' if v is None else getattr(v, 'value', v)}" for k, v in c.items()))
def test_banked_entry_point_refuses_before_any_launch(case):
    """-22 for a NULL pointer, B outside [2, 1024], K outside [1, 1024], slots outside [2, 64], cur outside [0, slots), bit cur clear, a mask bit at
    or above slots, ld outside [B, B + 7], an unknown dtype and a workspace that is not 8-byte aligned."""
    for name in ("cpc_nce_banked_workspace_floats", "cpc_nce_loss_banked"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert _banked(**case) == -22


def test_banked_workspace_size():
    """Chunk pairs [slots ceil(B / 32)][K][B] of two floats, lse [K][B], ceil(K B / 256) column partials, 3 ceil(B^2 / 256) pair
    partials and B (B + 8) pair means; 0 for sizes that make no sense."""
    ws = _hip.lib().cpc_nce_banked_workspace_floats
    for B, K, slots in [(2, 1, 2), (33, 3, 3), (256, 12, 17), (1024, 16, 64)]:
        cps = -(-B // 32)
        want = 2 * slots * cps * K * B + K * B + -(-K * B // 256) + 3 * -(-B * B // 256) + B * (B + 8)
        assert ws(B, K, slots) == want
    assert ws(0, 2, 2) == 0 and ws(2, 0, 2) == 0 and ws(2, 2, 0) == 0


# ------------------------------------------------------------------------------------------ the ring
def test_ring_bookkeeping():
    """cur and valid over slots + 2 steps, the filled count, the slot views, and reset()."""
    bank = NegativeBank(slots_back=2)
    assert (bank.slots, bank.cur, bank.valid, bank.filled, bank.ring) == (3, 0, 1, 0, None)
    bank.bind(4, 2, 8, torch.float32, "cpu")
    assert tuple(bank.ring.shape) == (12, 2, 8) and not bank.ring.any()
    seen = []
    for step in range(bank.slots + 2):
        seen.append((bank.cur, bank.valid, bank.filled))
        bank.slot(bank.cur).fill_(step + 1.0)
        bank.advance()
    assert seen == [(0, 0b001, 0), (1, 0b011, 1), (2, 0b111, 2), (0, 0b111, 2), (1, 0b111, 2)]
    assert (bank.cur, bank.valid) == (2, 0b111)
    assert [float(bank.slot(i)[0, 0, 0]) for i in range(3)] == [4.0, 5.0, 3.0]          # the ring wrapped: slots 0 and 1 were rewritten
    assert bank.slot(1).data_ptr() == bank.ring[4:].data_ptr()
    bank.reset()
    assert (bank.cur, bank.valid, bank.filled) == (2, 0b100, 0) and not bank.ring.any()
    bank.advance()
    assert (bank.cur, bank.valid, bank.filled) == (0, 0b101, 1)
    bank.bind(4, 2, 8, torch.float32, "cpu")                 # the same sizes again: nothing happens
    big = NegativeBank(63)
    for _ in range(70):
        big.advance()
    assert big.valid == 2 ** 64 - 1 and big.filled == 63 and big.cur == 70 % 64


@pytest.mark.parametrize("bad", [0, -1, 64, 100, 2.0, "2", None, True])
def test_bad_slots_back(bad):
    with pytest.raises(ValueError, match="negative bank"):
        NegativeBank(bad)


def test_size_change_names_both_sizes():
    bank = NegativeBank(1)
    bank.bind(4, 2, 8, torch.float32, "cpu")
    for other in [(6, 2, 8, torch.float32), (4, 3, 8, torch.float32), (4, 2, 16, torch.float32), (4, 2, 8, torch.bfloat16)]:
        with pytest.raises(ValueError) as e:
            bank.bind(*other, "cpu")
        assert "(4, 2, 8, torch.float32" in str(e.value) and f"({other[0]}, {other[1]}, {other[2]}, {other[3]}" in str(e.value)
    assert tuple(bank.ring.shape) == (8, 2, 8)


# ------------------------------------------------------------------------------------------ refusals of the engines
def test_engine_refusals_need_no_device():
    bank = NegativeBank(2)
    ng = (torch.zeros(8, dtype=torch.int32), "same")
    dev_t = object.__new__(DeviceTemperature)
    cases = [(dict(all_timesteps=True), "all-timesteps"), (dict(global_negatives=object()), "global_negatives"),
             (dict(gradient_penalty=10.0), "gradient penalty"), (dict(graphed=True), "captured graph"),
             (dict(negatives=(3, 1, 0)), "sampled or grouped"), (dict(negative_groups=ng), "sampled or grouped"),
             (dict(kind="difference"), "difference"), (dict(kind="normalized", temperature=dev_t), "temperature")]
    for kw, match in cases:
        with pytest.raises(NotImplementedError, match=match):
            check_negative_bank_supported(bank, **kw)
    check_negative_bank_supported(None, all_timesteps=True, global_negatives=object(), gradient_penalty=1.0, graphed=True)
    for kind, temperature in (("linear", None), ("softplus", None), ("normalized", 0.1)):
        check_negative_bank_supported(bank, kind=kind, temperature=temperature)
        assert select_negatives(8, None, None, negative_bank=bank, kind=kind, temperature=temperature) == ("banked", bank)
    with pytest.raises(TypeError, match="NegativeBank"):
        check_negative_bank_supported(2)
    # the engines' own entry points refuse before they read anything of the engine but B: a blank object is enough
    for cls in (CPCEngine, ScalogramCPCEngine):
        blank = object.__new__(cls)
        blank.B = 8
        for kw in (dict(all_timesteps=True), dict(global_negatives=object()), dict(negatives=(3, 1, 0)), dict(negative_groups=ng),
                   dict(score="difference"), dict(score="normalized", temperature=dev_t)):
            with pytest.raises(NotImplementedError):
                cls.loss_and_grads(blank, None, True, 1.0, negative_bank=bank, **kw)
        with pytest.raises(TypeError):
            cls.loss_and_grads(blank, None, True, 1.0, negative_bank=3)
    with pytest.raises(NotImplementedError, match="gradient penalty"):
        ScalogramCPCEngine.loss_and_grads(blank, None, True, 1.0, gradient_penalty=10.0, negative_bank=bank)
    stub = SimpleNamespace(B=8)
    with pytest.raises(NotImplementedError):
        CPCEngine._loss_chain(stub, "linear", True, 1.0, None, None, None, bank)
    with pytest.raises(NotImplementedError):
        CPCEngine.nce_forward_backward(blank, False, 1.0, score="difference", negative_bank=bank)
    with pytest.raises(NotImplementedError, match="captured graph"):
        GraphedStep(None, None, True, 1.0, negative_bank=bank)
    assert (bank.cur, bank.valid, bank.ring) == (0, 1, None)          # no refused call touched the bank


# ------------------------------------------------------------------------------------------ refusals of the trainer
def _tiny_model():
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    return AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                      prediction_steps=2)


class _NoDataset:
    def __len__(self):
        return 24

    def get_example_count_per_file(self):
        raise AssertionError("train() went past its up-front checks")


def _trainer(**kw):
    tr = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=_NoDataset(), device="cpu", file_batch_size=2, **kw)
    tr.verbose = False
    return tr


def test_trainer_refusals_come_before_any_gpu_work():
    tr = _trainer()
    assert tr.negative_bank is None and tr.negative_bank_filled == 0
    tr.reset_negative_bank()                                  # nothing to reset: no error
    for bad in (0, -3, 64, 2.0, "2", True):
        tr.negative_bank = bad
        with pytest.raises(ValueError, match="negative bank"):
            tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.negative_bank = 2
    for attr, value, match in [("score_over_all_timesteps", True, "score_over_all_timesteps"),
                               ("wasserstein_gradient_penalty", True, "gradient_penalty"), ("use_graph", True, "use_graph"),
                               ("global_negatives", True, "global_negatives"), ("num_negatives", 3, "num_negatives"),
                               ("negative_groups", "other_files", "negative_groups")]:
        before = getattr(tr, attr)
        setattr(tr, attr, value)
        with pytest.raises(NotImplementedError, match=match):
            tr.train(batch_size=8, epochs=1, max_steps=1)
        setattr(tr, attr, before)
    for sf, match in [(difference_score_function, "difference"), (NormalizedScoreFunction(0.1, learnable=True), "temperature"),
                      (NormalizedScoreFunction(schedule=TemperatureSchedule("linear", 0.5, 0.1, 10)), "temperature"),
                      (lambda p, t: linear_score_function(p, t), "engine route")]:
        tr2 = _trainer(score_function=sf)
        tr2.negative_bank = 2
        with pytest.raises(NotImplementedError, match=match):
            tr2.train(batch_size=8, epochs=1, max_steps=1)
    tr3 = _trainer(optimizer=torch.optim.SGD)
    tr3.negative_bank = 1
    with pytest.raises(NotImplementedError, match="engine route"):
        tr3.train(batch_size=8, epochs=1, max_steps=1)
    # what is covered passes the checks (and only then reaches the dataset)
    for sf in (linear_score_function, NormalizedScoreFunction(0.1)):
        tr4 = _trainer(score_function=sf)
        tr4.negative_bank = 63
        assert tr4._check_negative_bank() == 63
        kw = tr4._bank_kw(63)
        assert isinstance(kw["negative_bank"], NegativeBank) and kw["negative_bank"].slots == 64
        assert tr4._bank_kw(63)["negative_bank"] is kw["negative_bank"]          # kept across train() calls
        assert tr4._bank_kw(2)["negative_bank"].slots == 3                        # another M: a new bank
        assert tr4._bank_kw(None) == {} and tr4.negative_bank_filled == 0


# ------------------------------------------------------------------------------------------ the reference against its definition
@pytest.mark.parametrize("softplus", [0, 1])
@pytest.mark.parametrize("B,K,slots,cur,valid", [(5, 3, 3, 1, 0b011), (4, 1, 2, 0, 0b01), (3, 2, 4, 3, 0b1011)])
def test_reference_gradient_is_the_stated_formula(B, K, slots, cur, valid, softplus):
    """autograd of banked_terms == the closed form; rows of invalid slots get no gradient; with only bit cur set the loss is the
    in-batch loss of slot cur; the whole-loss form gives the same value and routes no gradient into detached slots."""
    g = torch.Generator().manual_seed(B * 7 + slots)
    S = torch.randn(K, slots * B, B, generator=g) * 3.0
    ref = R.banked_reference(S, B, cur, valid, softplus, 0.7)
    want = R.banked_gradient_formula(S, B, cur, valid, softplus, 0.7)
    assert (ref["dS"] - want).abs().max().item() < 1e-14
    rows = R.row_mask(B, slots, valid)
    assert not ref["dS"][:, ~rows, :].any() and ref["dS"][:, rows, :].abs().min().item() > 0
    assert torch.equal(ref["dST_cur"], ref["dS"][:, cur * B:(cur + 1) * B, :].transpose(1, 2))
    assert abs(ref["out"][2] + ref["out"][3] + ref["out"][4] - ref["loss"]) < 1e-13
    own = S[:, cur * B:(cur + 1) * B, :].double()
    sp = torch.nn.functional.softplus(own) if softplus else own
    dense = -torch.diagonal(sp, dim1=1, dim2=2).mean() + torch.logsumexp(sp, dim=1).mean() + 0.7 * (sp.mean(0) ** 2).mean()
    only = R.banked_reference(S, B, cur, 1 << cur, softplus, 0.7)
    assert abs(only["loss"] - dense.item()) < 1e-13
    if valid != 1 << cur:
        assert ref["out"][3] > only["out"][3]                 # more candidates: a larger log-sum-exp
    # the whole-loss form
    E = 6
    ring = torch.randn(slots * B, K, E, generator=g, dtype=torch.float64)
    targets = torch.randn(B, E, K, generator=g, dtype=torch.float64, requires_grad=True)
    cur_rows = ring[cur * B:(cur + 1) * B].clone().requires_grad_(True)
    full = torch.cat([ring[:cur * B], cur_rows, ring[(cur + 1) * B:]])
    loss, smax = R.banked_loss(full, targets, cur, valid, softplus, 0.7)
    loss.backward()
    t = R.banked_reference(R.banked_scores(ring, targets.detach()).float().double(), B, cur, valid, softplus, 0.7)
    assert abs(loss.item() - t["loss"]) < 1e-5 * max(1.0, abs(t["loss"]))
    dS = R.banked_gradient_formula(R.banked_scores(ring, targets.detach()), B, cur, valid, softplus, 0.7)
    assert (cur_rows.grad - torch.einsum("kbc,cek->bke", dS[:, cur * B:(cur + 1) * B, :], targets.detach())).abs().max().item() < 1e-12
    assert (targets.grad - torch.einsum("krb,rke->bek", dS, ring)).abs().max().item() < 1e-12
