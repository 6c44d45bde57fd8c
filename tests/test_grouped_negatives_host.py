"""Grouped negatives, the part that needs no GPU: the host restatement (grouped_negative_mask) against the pinned example of its
definition and against sampled_negative_mask through the two identities, its set properties, file_group_ids, the trainer's index
plumbing on the CPU, and the refusals of the trainer, the engine and the entry points, all raised before any GPU work."""
import ctypes as C
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cpc_audio_amd import _hip
from cpc_audio_amd.audio_dataset import FileBatchSampler
from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioPredictiveCodingModel
from cpc_audio_amd.contrastive_estimation_training import (ContrastiveEstimationTrainer, difference_score_function, file_group_ids,
                                                           grouped_negative_mask, sampled_negative_mask)
from cpc_audio_amd.engine import CPCEngine, GraphedStep, check_negatives_supported, normalize_negative_groups
from cpc_audio_amd.sampled_negatives import empty_negative_sets, group_eligibility
from cpc_audio_amd.scalogram_engine import ScalogramCPCEngine

EXAMPLE = [0, 0, 0, 1, 1, 2]
# (B, K, groups) of the kernel cases of tests/test_grouped_negatives_gpu.py
CASES = [(6, 4, EXAMPLE), (33, 3, [b % 5 for b in range(33)]), (40, 12, [b // 8 for b in range(40)]),
         (257, 2, [(-5, 2 ** 31 - 1, 0)[(7 * b) % 3] for b in range(257)]), (1024, 1, [b // 256 for b in range(1024)])]


def _rows(m):
    return " ".join("".join(str(int(v)) for v in row) for row in m)


@pytest.mark.parametrize("mode,n_neg,rows,ones", [
    ("same", None, "111000 111000 111000 000110 000110 000001", 56),
    ("same", 1, "101000 010000 111000 000110 000110 000001", 44),
    ("other", None, "100111 010111 001111 111101 111011 111111", 112),
    ("other", 1, "100100 010000 001010 000100 110011 001001", 48)])
def test_mask_matches_the_pinned_example(mode, n_neg, rows, ones):
    m = grouped_negative_mask(EXAMPLE, 4, mode, n_neg, seed=1234, draw=5)
    assert m.dtype == torch.bool and tuple(m.shape) == (4, 6, 6)
    assert _rows(m[0]) == rows and int(m.sum()) == ones
    if n_neg is None:
        assert torch.equal(m, grouped_negative_mask(EXAMPLE, 4, mode, 0, seed=1234, draw=5))          # 0 is "all" too
        assert torch.equal(m, grouped_negative_mask(EXAMPLE, 4, mode, None, seed=9, draw=9))          # and draws nothing


@pytest.mark.parametrize("B,K,N,seed,draw", [(6, 4, 2, 1234, 5), (37, 3, 9, 99, 1000003), (256, 12, 128, 1234, 5), (257, 1, 23, 7, 18),
                                             (1024, 1, 44, 7, 1), (9, 2, 8, 0, 0)])
def test_one_group_same_is_the_sampler(B, K, N, seed, draw):
    """Identity 1 (the tie draws (257, 1, 23, 7, 18) and (1024, 1, 44, 7, 1) included): bit for bit, whatever the one id is."""
    want = sampled_negative_mask(B, K, N, seed, draw)
    for gid in (0, -7, 2 ** 31 - 1):
        assert torch.equal(grouped_negative_mask([gid] * B, K, "same", N, seed, draw), want)
    assert torch.equal(grouped_negative_mask(np.full(B, 3, dtype=np.int32), K, "same", N, seed, draw), want)


def test_one_group_same_without_a_count_is_the_dense_loss():
    """Identity 2: all ones; and under "other" one group leaves every target with its own row only."""
    assert grouped_negative_mask([4] * 9, 3, "same").all()
    assert grouped_negative_mask([4] * 9, 3, "same", 8, 5, 0).all()
    assert torch.equal(grouped_negative_mask([4] * 9, 3, "other"), torch.eye(9, dtype=torch.bool).expand(3, 9, 9))
    assert torch.equal(grouped_negative_mask([4] * 9, 3, "other", 5, 1, 2), torch.eye(9, dtype=torch.bool).expand(3, 9, 9))
    # all ids distinct: the mirror image
    assert grouped_negative_mask(list(range(9)), 3, "other").all()
    assert torch.equal(grouped_negative_mask(list(range(9)), 3, "same"), torch.eye(9, dtype=torch.bool).expand(3, 9, 9))


@pytest.mark.parametrize("B,K,groups", CASES)
@pytest.mark.parametrize("mode", ["same", "other"])
def test_every_column_has_its_own_row_and_n_eligible_rows(B, K, groups, mode):
    g = np.asarray(groups, dtype=np.int64)
    elig = torch.from_numpy(group_eligibility(groups, mode))                    # [b'][b]
    assert not torch.diagonal(elig).any()
    assert torch.equal(elig, torch.from_numpy(((g[:, None] == g[None, :]) == (mode == "same")) & ~np.eye(B, dtype=bool)))
    count = elig.sum(dim=1)
    for n_neg in (None, 1, 5) + ((300,) if B == 1024 else ()):
        m = grouped_negative_mask(groups, K, mode, n_neg, seed=1234 + B, draw=5 + K)
        n = count if n_neg is None else count.clamp(max=n_neg)
        assert torch.equal(m.sum(dim=1), (1 + n).expand(K, B))                  # over the rows b of every column (k, b')
        assert torch.diagonal(m, dim1=1, dim2=2).all()
        off = m & ~torch.eye(B, dtype=torch.bool)
        assert not (off & ~elig.t()).any()                                      # only eligible rows are ever chosen
        if n_neg is not None and B > 6 and bool((count > n_neg).any()):          # some column draws: another draw, other rows
            assert not torch.equal(m, grouped_negative_mask(groups, K, mode, n_neg, seed=1234 + B, draw=6 + K))
    assert empty_negative_sets(groups, mode) == int((count == 0).sum())


def test_selection_is_the_sampler_restricted_to_the_eligible_rows():
    """The chosen rows are the eligible rows with the smallest (key, b): every chosen row's composite is below every eligible row's
    that was not chosen."""
    from cpc_audio_amd.sampled_negatives import sampled_negative_keys
    B, K, groups = 33, 3, [b % 5 for b in range(33)]
    key = sampled_negative_keys(B, K, 17, 4)                                    # [k][b'][b]
    comp = key * np.uint64(2 ** 32) + np.arange(B, dtype=np.uint64)
    for mode in ("same", "other"):
        elig = group_eligibility(groups, mode)
        m = grouped_negative_mask(groups, K, mode, 3, 17, 4).numpy().transpose(0, 2, 1)        # [k][b'][b]
        for k in range(K):
            for bp in range(B):
                chosen = m[k, bp] & elig[bp]
                rest = elig[bp] & ~m[k, bp]
                assert chosen.sum() == min(3, elig[bp].sum())
                if rest.any():
                    assert comp[k, bp][chosen].max() < comp[k, bp][rest].min()


def test_arguments_of_the_host_restatement():
    with pytest.raises(ValueError, match="mode"):
        grouped_negative_mask(EXAMPLE, 2, "same_file")
    for bad in (6, -1, 2.5, 100):
        with pytest.raises(ValueError):
            grouped_negative_mask(EXAMPLE, 2, "same", bad)
    # seed and draw are taken modulo 2^64
    assert torch.equal(grouped_negative_mask(EXAMPLE, 2, "other", 1, 2 ** 64 + 5, 1), grouped_negative_mask(EXAMPLE, 2, "other", 1, 5, 1))


def test_file_group_ids():
    ids = file_group_ids([2, 0, 3, 1])
    assert ids.dtype == np.int32 and ids.tolist() == [0, 0, 2, 2, 2, 3]
    assert file_group_ids([]).size == 0
    assert file_group_ids(np.array([8, 8, 8])).tolist() == [0] * 8 + [1] * 8 + [2] * 8


def _tiny_model():
    enc = AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [8] * 5, 'bias': True})
    return AudioPredictiveCodingModel(enc, AudioGRUModel(input_size=8, hidden_size=8), enc_size=8, ar_size=8, visible_steps=4,
                                      prediction_steps=2)


class _NoDataset:
    def __len__(self):
        return 24

    def get_example_count_per_file(self):
        raise AssertionError("train() went past its up-front checks")


def test_trainer_refusals_come_before_any_gpu_work():
    tr = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=_NoDataset(), device="cpu", file_batch_size=2)
    tr.verbose = False
    assert tr.negative_groups is None and tr.negative_group_ids is None and tr.last_empty_negative_sets is None
    for bad in ("same", "other", "same_files", 1, True):
        tr.negative_groups = bad
        with pytest.raises(ValueError, match="negative_groups"):
            tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.negative_groups = "other_files"
    for bad in (list(range(23)), list(range(25)), [[0] * 24], [0.5] * 24, [2 ** 31] * 24):
        tr.negative_group_ids = bad
        with pytest.raises(ValueError, match="negative_group_ids"):
            tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.negative_group_ids = None
    tr.negative_groups, tr.file_batch_size = "same_file", 1
    with pytest.raises(ValueError, match="file_batch_size"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.negative_group_ids = [0] * 24                      # ids of the user's own: file_batch_size does not matter
    assert tr._check_negative_groups()[0] == "same"
    tr.negative_group_ids, tr.file_batch_size = None, 2
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
    # together with num_negatives: its own checks still hold
    tr.num_negatives = 8
    with pytest.raises(ValueError, match="num_negatives"):
        tr.train(batch_size=8, epochs=1, max_steps=1)
    tr.num_negatives = None
    # the other score functions take the same checks
    tr2 = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=_NoDataset(), device="cpu", score_function=difference_score_function)
    tr2.verbose = False
    tr2.negative_groups = "same_file"
    with pytest.raises(ValueError, match="file_batch_size"):
        tr2.train(batch_size=8, epochs=1, max_steps=1)
    # the step's keyword: ids of the batch's examples, and the count of items without an eligible row
    tr.negative_groups = "same_file"
    grouping = ("same", file_group_ids([3, 2, 1]))
    kw = tr._groups_kw(grouping, [0, 1, 2, 3, 4, 5], "cpu")
    groups, mode = kw["negative_groups"]
    assert mode == "same" and groups.dtype == torch.int32 and groups.tolist() == EXAMPLE
    assert tr.last_empty_negative_sets == 1
    assert tr._groups_kw(("other", np.zeros(6, dtype=np.int32)), [5, 4, 3], "cpu")["negative_groups"][0].tolist() == [0, 0, 0]
    assert tr.last_empty_negative_sets == 3
    assert tr._groups_kw(None, [0, 1], "cpu") == {}


class _HostDataset(torch.utils.data.Dataset):
    """No device_data: the DataLoader route.  Example i is a row filled with i."""

    def __init__(self, counts, length=4):
        self.counts = list(counts)
        self.data = torch.arange(sum(counts), dtype=torch.float32).reshape(-1, 1).repeat(1, length)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return self.data[i]

    def get_example_count_per_file(self):
        return self.counts


class _ResidentDataset(_HostDataset):
    def __init__(self, counts):
        super().__init__(counts)
        self.device_data = self.data


@pytest.mark.parametrize("dataset", [_HostDataset, _ResidentDataset])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_indices_travel_with_their_batch(dataset, rank, world, monkeypatch):
    """_batches(with_indices=True) pairs every batch with the example indices it was built from, on the resident and the DataLoader
    route, read one batch ahead or not, and with each rank's own slice under data parallelism; without the flag it yields what it
    always did."""
    import torch.distributed as dist
    from cpc_audio_amd.contrastive_estimation_training import _with_next
    counts, B = [8, 8, 8], 6
    ds = dataset(counts)
    tr = ContrastiveEstimationTrainer(model=_tiny_model(), dataset=ds, device="cpu", file_batch_size=2)
    tr.verbose = False
    random.seed(5)
    want = [list(b) for b in FileBatchSampler(counts, B * world, 2, True, verbose=False)]
    per = B
    want = [b[rank * per:(rank + 1) * per] for b in want]
    assert len(want) >= 2
    if world == 1:
        files = [file_group_ids(counts)[b].tolist() for b in want[:3]]
        assert files == [[1, 1, 1, 1, 0, 0], [2, 2, 0, 0, 2, 2], [1, 1, 2, 2, 0, 0]]

    def run(with_indices, ahead):
        random.seed(5)
        sampler = FileBatchSampler(counts, B * world, 2, True, verbose=False)
        # one process plays rank `rank`: rank 0 drew the lists itself, another rank receives what rank 0 drew
        lists = [list(b) for b in sampler] if rank != 0 else None
        monkeypatch.setattr(dist, "broadcast_object_list", lambda box, src=0: box.__setitem__(0, lists) if rank != 0 else None)
        it = tr._batches(ds, sampler, "cpu", 0, False, rank, world, with_indices=with_indices)
        return list(_with_next(it)) if ahead else [(b, None) for b in it]

    for ahead in (False, True):
        got = run(True, ahead)
        assert len(got) == len(want)
        for i, ((batch, idx), nxt) in enumerate(got):
            assert idx == want[i] and batch[:, 0].tolist() == [float(j) for j in want[i]]
            if ahead and i + 1 < len(got):
                assert nxt[1] == want[i + 1]
        plain = run(False, ahead)
        for (batch, nxt), w in zip(plain, want):
            assert torch.is_tensor(batch) and batch[:, 0].tolist() == [float(j) for j in w]


def test_engine_refusals_need_no_device():
    ng = (torch.zeros(8, dtype=torch.int32), "same")
    with pytest.raises(NotImplementedError, match="all-timesteps"):
        check_negatives_supported(None, all_timesteps=True, negative_groups=ng)
    with pytest.raises(NotImplementedError, match="global_negatives"):
        check_negatives_supported(None, global_negatives=object(), negative_groups=ng)
    with pytest.raises(NotImplementedError, match="gradient penalty"):
        check_negatives_supported(None, gradient_penalty=10.0, negative_groups=ng)
    with pytest.raises(NotImplementedError, match="all_timesteps"):                # together with negatives: the sampled feature's reasons
        check_negatives_supported((3, 1, 0), all_timesteps=True, negative_groups=ng)
    check_negatives_supported(None, negative_groups=ng)
    check_negatives_supported(None, all_timesteps=True, global_negatives=object(), gradient_penalty=1.0, negative_groups=None)
    groups, mode, n_neg, seed, draw = normalize_negative_groups(ng, 8)
    assert groups is ng[0] and (mode, n_neg, seed, draw) == (0, 0, 0, 0)
    assert normalize_negative_groups((ng[0], "other"), 8, (3, -1, 2 ** 64 + 4))[1:] == (1, 3, 2 ** 64 - 1, 4)
    with pytest.raises(ValueError, match="mode"):
        normalize_negative_groups((ng[0], "same_file"), 8)
    with pytest.raises(ValueError):
        normalize_negative_groups(ng, 9)
    with pytest.raises(ValueError):
        normalize_negative_groups(ng, 8, (8, 0, 0))
    with pytest.raises(TypeError):
        normalize_negative_groups((torch.zeros(8, dtype=torch.int64), "same"), 8)
    with pytest.raises(TypeError):
        normalize_negative_groups(([0] * 8, "same"), 8)
    # the engines' own entry points refuse before they touch a buffer: a stand-in without any is enough
    stub = SimpleNamespace(B=8)
    with pytest.raises(NotImplementedError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, all_timesteps=True, negative_groups=ng)
    with pytest.raises(NotImplementedError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, global_negatives=object(), negative_groups=ng)
    with pytest.raises(ValueError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, negative_groups=(ng[0], "files"))
    with pytest.raises(ValueError):
        CPCEngine.loss_and_grads(stub, None, True, 1.0, negative_groups=ng, negatives=(8, 0, 0))
    with pytest.raises(NotImplementedError):
        ScalogramCPCEngine.loss_and_grads(stub, None, True, 1.0, gradient_penalty=10.0, negative_groups=ng)
    for kind, temperature in (("difference", None), ("linear", None), ("normalized", 0.1)):      # one selection check for every kind
        with pytest.raises(NotImplementedError):
            CPCEngine._loss_chain(stub, kind, True, 1.0, temperature, None, ng)
    with pytest.raises(NotImplementedError, match="graph"):
        GraphedStep(None, None, True, 1.0, negative_groups=ng)


def test_entry_points_check_their_arguments_before_any_launch():
    """cpc_nce_loss_grouped / cpc_nce_group_mask return CPC_EINVAL (-22) for null pointers (groups included), B outside [2, 1024],
    ld outside [B, B + 7], a mode outside {0, 1}, n_neg outside [0, B - 1], another dtype and a workspace that is not 8-byte
    aligned: argument checks in front of the launches, so they run without a GPU."""
    lib = _hip.lib()
    for name in ("cpc_nce_grouped_workspace_floats", "cpc_nce_loss_grouped", "cpc_nce_group_mask"):
        assert name in _hip.EXPORTED_SYMBOLS
    P, s = C.c_void_p(0x1000), C.c_void_p(0)          # never dereferenced: the calls below are refused before any launch
    U = C.c_ulonglong

    def loss(S=P, dS=P, dST=P, out=P, ws=P, groups=P, B=8, K=2, ld=8, mode=0, n=3, dtype=_hip.F32):
        return lib.cpc_nce_loss_grouped(S, dS, dST, out, ws, B, K, ld, 1, C.c_float(1.0), groups, mode, n, U(1), U(2), dtype, s)

    def mask(m=P, groups=P, B=8, K=2, mode=0, n=3):
        return lib.cpc_nce_group_mask(m, groups, B, K, mode, n, U(1), U(2), s)

    for name in ("S", "dS", "dST", "out", "ws", "groups"):
        assert loss(**{name: None}) == -22, name
    assert loss(n=8) == -22 and loss(n=-1) == -22
    assert loss(B=1, ld=1, n=0) == -22 and loss(B=1025, ld=1032, n=5) == -22
    assert loss(ld=7) == -22 and loss(ld=16) == -22
    assert loss(mode=2) == -22 and loss(mode=-1) == -22
    assert loss(dtype=7) == -22
    assert loss(K=0) == -22
    assert loss(ws=C.c_void_p(0x1004)) == -22
    assert mask(m=None) == -22 and mask(groups=None) == -22
    assert mask(n=8) == -22 and mask(n=-1) == -22
    assert mask(mode=2) == -22 and mask(mode=-1) == -22
    assert mask(B=1) == -22 and mask(B=1025, n=5) == -22 and mask(K=0) == -22
    assert lib.cpc_nce_grouped_workspace_floats(1024, 12) == lib.cpc_nce_sampled_workspace_floats(1024, 12) > 0
