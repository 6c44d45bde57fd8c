"""Sampled negatives, the part that needs no GPU: the host restatement of the sampler (sampled_negative_mask) against the pinned
values of its definition, its set properties, and the refusals of the trainer and the engine, all raised before any GPU work."""
import ctypes as C
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, difference_score_function,
                                                           sampled_negative_mask)
from cpc_audio_amd.engine import CPCEngine, GraphedStep, check_negatives_supported, normalize_negatives
from cpc_audio_amd.sampled_negatives import sampled_negative_keys
from cpc_audio_amd.scalogram_engine import ScalogramCPCEngine


def _digest(m):
    return hashlib.sha256(np.packbits(m.numpy()).tobytes()).hexdigest()[:16]


def test_keys_match_the_pinned_values():
    key = sampled_negative_keys(6, 4, 1234, 5)                   # [k][b'][b]
    assert key[0, 0].tolist() == [733286441, 3586328631, 1225514974, 3040025574, 763871157, 2454872156]
    assert key[3, 5].tolist() == [4106527079, 1123995645, 2899146866, 3594386173, 1677308004, 3890796937]
    assert sampled_negative_keys(2, 1, 0, 0)[0].tolist() == [[3793791033, 755968199], [1012622983, 405998883]]


def test_mask_matches_the_pinned_values():
    m = sampled_negative_mask(6, 4, 2, 1234, 5)
    assert m.dtype == torch.bool and tuple(m.shape) == (4, 6, 6)
    rows = ["".join(str(int(v)) for v in row) for row in m[0]]
    assert rows == ["101100", "010000", "101011", "010100", "110111", "001011"]
    big = sampled_negative_mask(256, 12, 128, 1234, 5)
    assert int(big.sum()) == 396288 and _digest(big) == "70b871b4090e2d43"
    odd = sampled_negative_mask(37, 3, 9, 99, 1000003)
    assert int(odd.sum()) == 1110 and _digest(odd) == "fad36b7e6b9e56fb"


@pytest.mark.parametrize("B,K,N", [(6, 4, 2), (37, 3, 9), (2, 1, 1), (65, 2, 64), (257, 1, 128)])
def test_every_column_has_its_own_row_and_n_negatives(B, K, N):
    m = sampled_negative_mask(B, K, N, 7, 3)
    assert (m.sum(dim=1) == N + 1).all()                          # over the rows b of every column (k, b')
    assert torch.diagonal(m, dim1=1, dim2=2).all()


def test_all_negatives_is_the_dense_loss_and_draws_differ():
    assert sampled_negative_mask(9, 3, 8, 5, 0).all()
    a = sampled_negative_mask(33, 2, 7, 11, 4)
    assert torch.equal(a, sampled_negative_mask(33, 2, 7, 11, 4))
    assert not torch.equal(a, sampled_negative_mask(33, 2, 7, 11, 5))
    assert not torch.equal(a, sampled_negative_mask(33, 2, 7, 12, 4))
    # seed and draw are taken modulo 2^64
    assert torch.equal(sampled_negative_mask(9, 2, 3, 2 ** 64 + 5, 1), sampled_negative_mask(9, 2, 3, 5, 1))
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError):
            sampled_negative_mask(9, 2, bad, 0, 0)


@pytest.mark.parametrize("B,N,seed,draw,col", [(257, 23, 7, 18, 46), (1024, 44, 7, 1, 75)])
def test_key_ties_are_broken_by_the_index(B, N, seed, draw, col):
    """Two draws in which the N-th and the (N + 1)-th smallest key of one column are EQUAL (found by search; the first assertion
    keeps the pin honest): the row with the smaller index is a candidate, the other is not, and the column still has N + 1 ones."""
    key = sampled_negative_keys(B, 1, seed, draw)[0, col]
    rows = np.array([b for b in np.argsort(key, kind="stable") if b != col])       # by (key, b)
    lo, hi = int(rows[N - 1]), int(rows[N])
    assert key[lo] == key[hi] and lo < hi
    m = sampled_negative_mask(B, 1, N, seed, draw)[0, :, col]
    assert bool(m[lo]) and not bool(m[hi]) and int(m.sum()) == N + 1


def _tiny_model():
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    return AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                      prediction_steps=2)


class _NoDataset:
    def get_example_count_per_file(self):
        raise AssertionError("train() went past its up-front checks")


def test_trainer_refusals_come_before_any_gpu_work():
    tr = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=_NoDataset(), device="cpu")
    tr.verbose = False
    assert tr.num_negatives is None and tr.negative_seed == 0
    for bad in (0, 8, 100, -3):
        tr.num_negatives = bad
        with pytest.raises(ValueError, match="num_negatives"):
            tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.num_negatives = 3
    tr.score_over_all_timesteps = True
    with pytest.raises(NotImplementedError, match="score_over_all_timesteps"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.score_over_all_timesteps = False
    tr.wasserstein_gradient_penalty = True
    with pytest.raises(NotImplementedError, match="gradient_penalty"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.wasserstein_gradient_penalty = False
    tr.use_graph = True
    with pytest.raises(NotImplementedError, match="use_graph"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.use_graph = False
    tr.global_negatives = True
    with pytest.raises(NotImplementedError, match="global_negatives"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.global_negatives = False
    # the step's negatives: (N, seed, draw = training_step)
    tr.negative_seed, tr.training_step = 77, 12
    assert tr._negatives_kw() == {"negatives": (3, 77, 12)}
    tr.num_negatives = None
    assert tr._negatives_kw() == {}
    # the other score functions take the same checks
    tr2 = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=_NoDataset(), device="cpu", score_function=difference_score_function)
    tr2.verbose = False
    tr2.num_negatives = 8
    with pytest.raises(ValueError):
        tr2.train(batch_size=8, epochs=1, max_steps=1)


def test_engine_refusals_need_no_device():
    neg = (3, 1, 0)
    with pytest.raises(NotImplementedError, match="all_timesteps"):
        check_negatives_supported(neg, all_timesteps=True)
    with pytest.raises(NotImplementedError, match="global_negatives"):
        check_negatives_supported(neg, global_negatives=object())
    with pytest.raises(NotImplementedError, match="gradient penalty"):
        check_negatives_supported(neg, gradient_penalty=10.0)
    check_negatives_supported(None, all_timesteps=True, global_negatives=object(), gradient_penalty=1.0)
    assert normalize_negatives((3, -1, 2 ** 64 + 4), 8) == (3, 2 ** 64 - 1, 4)
    for bad in (0, 8):
        with pytest.raises(ValueError):
            normalize_negatives((bad, 0, 0), 8)
    # the engines' own entry points refuse before they touch a buffer: a stand-in without any is enough
    stub = SimpleNamespace(B=8)
    with pytest.raises(NotImplementedError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, all_timesteps=True, negatives=neg)
    with pytest.raises(NotImplementedError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, global_negatives=object(), negatives=neg)
    with pytest.raises(ValueError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, negatives=(8, 0, 0))
    with pytest.raises(NotImplementedError):
        ScalogramCPCEngine.loss_and_grads(stub, None, True, 1.0, gradient_penalty=10.0, negatives=neg)
    for kind, temperature in (("difference", None), ("linear", None), ("normalized", 0.1)):      # one selection check for every kind
        with pytest.raises(NotImplementedError):
            CPCEngine._loss_chain(stub, kind, True, 1.0, temperature, neg)
    with pytest.raises(NotImplementedError, match="graph"):
        GraphedStep(None, None, True, 1.0, negatives=neg)


def test_entry_points_check_their_arguments_before_any_launch():
    """cpc_nce_loss_sampled / cpc_nce_sample_mask return CPC_EINVAL (-22) for null pointers, n_neg outside [1, B - 1] and B above
    the supported maximum of 1024: argument checks in front of the launches, so they run without a GPU."""
    lib = _hip.lib()
    P, s = C.c_void_p(0x1000), C.c_void_p(0)
    U = C.c_ulonglong

    def loss(S=P, dS=P, dST=P, out=P, ws=P, B=8, K=2, ld=8, n=3, dtype=_hip.F32):
        return lib.cpc_nce_loss_sampled(S, dS, dST, out, ws, B, K, ld, 1, C.c_float(1.0), n, U(1), U(2), dtype, s)

    for name in ("S", "dS", "dST", "out", "ws"):
        assert loss(**{name: None}) == -22, name
    assert loss(n=0) == -22 and loss(n=8) == -22 and loss(n=-1) == -22
    assert loss(B=1025, ld=1032, n=5) == -22
    assert loss(ld=7) == -22 and loss(ld=16) == -22
    assert loss(dtype=7) == -22
    assert lib.cpc_nce_sample_mask(None, 8, 2, 3, U(1), U(2), s) == -22
    assert lib.cpc_nce_sample_mask(P, 8, 2, 0, U(1), U(2), s) == -22
    assert lib.cpc_nce_sample_mask(P, 8, 2, 8, U(1), U(2), s) == -22
    assert lib.cpc_nce_sample_mask(P, 1025, 2, 5, U(1), U(2), s) == -22
    assert lib.cpc_nce_sampled_workspace_floats(1024, 12) > 0
