"""K-means units, the parts that need no GPU: self-checks of the float64 reference (kmeans_reference), the seeded init, the argument
checks of cpc_kmeans_assign / cpc_kmeans_update / cpc_kmeans_scratch_bytes / cpc_kmeans_cnorm (refused before any launch, through
pointers that are never dereferenced), the refusals of cpc_audio_amd.clustering.KMeans, and the condition the label-equality tests
of test_kmeans_gpu.py stand on: on the separated data the smallest margin exceeds 4 tol_n, in float64."""
import ctypes as C

import numpy as np
import pytest
import torch

import cpc_audio_amd
from cpc_audio_amd import _hip
from cpc_audio_amd import clustering as KM
import kmeans_reference as R


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_reference_distances_and_lowest_index():
    rng = np.random.default_rng(3)
    x, c = rng.standard_normal((40, 16)), rng.standard_normal((7, 16))
    direct = ((x[:, None, :] - c[None, :, :]) ** 2).sum(2)
    assert np.abs(R.distances(x, c) - direct).max() < 1e-12
    labels, dist = R.assign(x, c)
    assert (labels == direct.argmin(1)).all() and np.abs(dist - direct.min(1)).max() < 1e-12
    # duplicated centres: the lower index wins
    c2 = np.concatenate([c, c[2:3], c[5:6]])
    labels2, _ = R.assign(x, c2)
    assert (labels2 == labels).all() and labels2.max() < 7
    # a row with a NaN or an infinity: -1 and NaN, nothing else changes
    xb = x.copy()
    xb[3, 5], xb[17, 0] = np.nan, np.inf
    lb, db = R.assign(xb, c)
    assert lb[3] == -1 and lb[17] == -1 and np.isnan(db[3]) and np.isnan(db[17])
    keep = np.ones(40, bool)
    keep[[3, 17]] = False
    assert (lb[keep] == labels[keep]).all() and (db[keep] == dist[keep]).all()
    assert (R.margins(x, c) >= 0).all() and (R.tolerance(x, c) > 0).all()


def test_reference_update_rules():
    rng = np.random.default_rng(4)
    x, old = rng.standard_normal((9, 16)), rng.standard_normal((4, 16))
    labels = np.array([0, 0, 2, -1, 4, 2, 2, 0, 7])          # cluster 1 and 3 empty; -1, 4 = K and 7 skipped
    dist = np.arange(9, dtype=np.float64)
    c, cn, counts, inertia = R.update(x, labels, old, dist)
    assert counts.tolist() == [3, 0, 3, 0]
    assert np.abs(c[0] - x[[0, 1, 7]].mean(0)).max() < 1e-15 and np.abs(c[2] - x[[2, 5, 6]].mean(0)).max() < 1e-15
    assert (c[1] == old[1]).all() and (c[3] == old[3]).all()
    assert np.abs(cn - (c * c).sum(1)).max() == 0 and inertia == 0 + 1 + 2 + 5 + 6 + 7


def test_reference_lloyd_never_raises_the_inertia():
    x, init = R.separated(400, 16, 5, seed=9)
    rng = np.random.default_rng(1)
    start = x[rng.choice(400, 5, replace=False)]          # a poor start, so that the iterations have work to do
    c, counts, labels, inertia, seen = R.lloyd(x, start, 6, round_centers=False)
    assert len(seen) == 6 and counts.sum() == 400
    assert (np.diff(inertia) <= 1e-9 * inertia[0]).all()
    assert (R.assign(x, seen[-1])[0] == labels).all()


def test_seeded_init_is_reproducible_and_sorted():
    for n, k, seed in ((1000, 64, 0), (65, 64, 5), (64, 64, 2), (359902, 512, 0)):
        rows = KM.sample_rows(n, k, seed)
        assert rows.dtype == np.int64 and rows.shape == (k,)
        assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n          # sorted, distinct, in range
        assert (rows == KM.sample_rows(n, k, seed)).all() and (rows == R.sample_rows(n, k, seed)).all()
        assert (rows == np.sort(np.random.default_rng(seed).choice(n, k, replace=False))).all()
    assert (KM.sample_rows(1000, 64, 0) != KM.sample_rows(1000, 64, 1)).any()
    with pytest.raises(ValueError):
        KM.sample_rows(63, 64, 0)
    with pytest.raises(ValueError):
        R.sample_rows(63, 64, 0)


@pytest.mark.parametrize("shape", R.SEPARATED_SHAPES, ids=lambda s: "N%d-D%d-K%d" % s)
def test_separated_data_has_a_margin_above_four_tolerances(shape):
    """The input condition of the label-equality tests: over the four Lloyd iterations of the float64 reference, the smallest
    second-best-minus-best distance exceeds 4 tol_n on both seeds (a kernel within tol_n per candidate cannot then pick another
    centre, with 2 tol_n to spare for centres that differ by their own rounding)."""
    for seed in R.SEPARATED_SEEDS:
        case = R.separated_case(*shape, seed)
        ratio = min(float((R.margins(case["x"], c) / R.tolerance(case["x"], c)).min()) for c in case["seen"])
        print(f"{shape} seed {seed}: smallest margin = {ratio:.3g} tol_n")
        assert ratio > 4.0
        assert case["counts"].sum() == shape[0]


# ---------------------------------------------------------------------------------------------------------------- argument checks
P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
P4 = C.c_void_p(0x1004)         # 4-byte but not 8- / 16-byte aligned
P2 = C.c_void_p(0x1002)
S = C.c_void_p(0)
LL = C.c_longlong
BAD_SHAPES = [dict(x=None), dict(x=P4), dict(dtype=2), dict(dtype=-1), dict(N=0), dict(N=-1), dict(N=2 ** 31), dict(D=0), dict(D=8),
              dict(D=24), dict(D=528, ldx=528), dict(D=-16), dict(K=1), dict(K=0), dict(K=1025), dict(ldx=48), dict(ldx=66),
              dict(dtype=_hip.BF16, ldx=68)]


def test_kmeans_assign_refuses_bad_arguments():
    lib = _hip.lib()

    def call(x=P, dtype=_hip.F32, N=100, D=64, ldx=64, centers=P, cnorm=P, K=8, labels=P, dist=P):
        return lib.cpc_kmeans_assign(x, dtype, LL(N), D, LL(ldx), centers, cnorm, K, labels, dist, S)

    bad = BAD_SHAPES + [dict(centers=None), dict(cnorm=None), dict(labels=None), dict(centers=P4), dict(cnorm=P2), dict(labels=P2),
                        dict(dist=P2)]
    for kw in bad:
        assert call(**kw) == -22, kw


def test_kmeans_update_refuses_bad_arguments():
    lib = _hip.lib()
    need = lib.cpc_kmeans_scratch_bytes(LL(100), 8, 64)
    assert need > 0

    def call(x=P, dtype=_hip.F32, N=100, D=64, ldx=64, labels=P, dist=P, old=P, K=8, scratch=P, nbytes=need, new=P, cnorm=P, counts=P,
             inertia=P):
        return lib.cpc_kmeans_update(x, dtype, LL(N), D, LL(ldx), labels, dist, old, K, scratch, LL(nbytes), new, cnorm, counts, inertia, S)

    bad = BAD_SHAPES + [dict(labels=None), dict(old=None), dict(scratch=None), dict(new=None), dict(cnorm=None), dict(counts=None),
                        dict(dist=None), dict(inertia=None), dict(nbytes=need - 1), dict(nbytes=0), dict(scratch=P4), dict(inertia=P4),
                        dict(labels=P2), dict(dist=P2), dict(old=P2), dict(new=P2), dict(cnorm=P2), dict(counts=P2),
                        dict(N=10 ** 6)]          # (the scratch of 100 rows does not hold 10^6)
    for kw in bad:
        assert call(**kw) == -22, kw


def test_kmeans_scratch_bytes_and_cnorm_refuse_bad_arguments():
    lib = _hip.lib()
    for n, k, d in ((0, 8, 64), (2 ** 31, 8, 64), (100, 1, 64), (100, 1025, 64), (100, 8, 8), (100, 8, 24), (100, 8, 528)):
        assert lib.cpc_kmeans_scratch_bytes(LL(n), k, d) == -22, (n, k, d)
    sizes = [lib.cpc_kmeans_scratch_bytes(LL(n), 64, 256) for n in (1, 1000, 359902, 2 ** 31 - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[2] < 64 << 20          # the measured shape needs a few MB, not a copy of the features

    def cnorm(centers=P, out=P, K=8, D=64):
        return lib.cpc_kmeans_cnorm(centers, out, K, D, S)

    for kw in (dict(centers=None), dict(out=None), dict(K=1), dict(K=1025), dict(D=8), dict(D=24), dict(D=528), dict(centers=P2), dict(out=P2)):
        assert cnorm(**kw) == -22, kw


# ---------------------------------------------------------------------------------------------------------------------- refusals
class _FakeFeatures:
    def __init__(self, **kw):
        self.frame_offsets = [0, 4]
        for k, v in kw.items():
            setattr(self, k, v)


def test_python_refusals_need_no_device():
    assert "clustering" in cpc_audio_amd.__all__
    for kw in (dict(n_clusters=1), dict(n_clusters=1025), dict(n_clusters=8, iterations=0), dict(n_clusters=8, init="kmeans++"),
               dict(n_clusters=8, init=torch.zeros(7, 16)), dict(n_clusters=8, init=torch.zeros(8))):
        with pytest.raises(ValueError):
            KM.KMeans(**kw)
    km = KM.KMeans(4, iterations=2)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="CPU"):
        km.fit(torch.zeros(100, 16))
    with pytest.raises(ValueError, match="CPU"):
        km.assign(torch.zeros(100, 16))
    with pytest.raises(ValueError, match="CPU"):
        km.fit(_FakeFeatures(c=torch.zeros(4, 16)))
    with pytest.raises(ValueError, match="holds no"):
        km.fit(_FakeFeatures(z=torch.zeros(4, 16)), kind="c")
    with pytest.raises(ValueError, match="kind"):
        km.fit(_FakeFeatures(z=torch.zeros(4, 16)), kind="x")
    with pytest.raises(TypeError):
        km.fit([[0.0] * 16] * 8)
    with pytest.raises(RuntimeError):
        km.state_dict()
    with pytest.raises(ValueError):
        km.load_state_dict({"centers": torch.zeros(4, 16), "counts": torch.zeros(4, dtype=torch.int32)})          # a CPU state, no device
    with pytest.raises(ValueError):
        km.load_state_dict({"centers": torch.zeros(5, 16), "counts": torch.zeros(5, dtype=torch.int32)}, device="cuda:0")
    assert torch.equal(torch.get_rng_state(), state)


def test_shape_refusals_come_before_the_device():
    """dtype, shape and stride are judged on tensors of the 'meta' device standing in for device tensors: nothing can be launched on
    them, so a refusal that came later would fail differently."""
    km = KM.KMeans(4, iterations=1)

    class Dev(torch.Tensor):
        is_cuda = True

    def dev(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(Dev)

    with pytest.raises(TypeError, match="float32 or bfloat16"):
        km.fit(dev(100, 16, dtype=torch.float16))
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        km.fit(dev(100, 16, dtype=torch.float64))
    for shape in ((100,), (100, 16, 2), (100, 8), (100, 24), (100, 528), (0, 16)):
        with pytest.raises(ValueError):
            km.fit(dev(*shape))
    with pytest.raises(ValueError, match="contiguous"):
        km.fit(dev(16, 100).t())
    with pytest.raises(ValueError, match="contiguous"):
        km.fit(dev(100, 32)[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        km.fit(dev(100, 18)[:, :16])          # a row stride of 18 floats: rows that do not start at 16-byte pieces
    with pytest.raises(ValueError, match="seed"):
        km.fit(dev(3, 16))
