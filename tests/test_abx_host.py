"""The host side of the ABX evaluation (cpc_audio_amd.abx) and its reference (tests/abx_reference.py): no GPU.  The refusals of
cpc_frame_distance, cpc_dtw and cpc_abx_count come before any launch, so they run on a CPU-only host."""
import ctypes as C

import numpy as np
import pytest
import torch

import cpc_audio_amd
from cpc_audio_amd import _hip
from cpc_audio_amd import abx as A
import abx_reference as R

LL = C.c_longlong
P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any launch
P4 = C.c_void_p(0x1004)         # 4-byte but not 8- / 16-byte aligned
P2 = C.c_void_p(0x1002)
S = C.c_void_p(0)


# ================================================================================================================== reference
def _matrices():
    rng = np.random.default_rng(0)
    shapes = [(1, 1), (1, 7), (7, 1), (1, 128), (128, 1), (2, 2), (5, 9), (9, 5), (17, 17), (40, 23), (64, 65)]
    out = []
    for k in range(400):
        La, Lb = shapes[k % len(shapes)] if k < 200 else (int(rng.integers(1, 30)), int(rng.integers(1, 30)))
        if k % 2:
            out.append(rng.integers(0, 3, size=(La, Lb)).astype(np.float64))          # small integers: most cells tie
        else:
            out.append(rng.random((La, Lb)))
    return out


def test_forward_path_length_equals_the_backtrack():
    ties = 0
    for d in _matrices():
        for dtype in (np.float64, np.float32):
            Cm, Ln = R.dtw_tables(d, dtype)
            assert Ln[-1, -1] == R.backtrack_length(Cm), d.shape
            assert max(d.shape) <= Ln[-1, -1] <= d.shape[0] + d.shape[1] - 1
        if min(d.shape) > 1:
            inner = Cm[1:, 1:]
            ties += int(((Cm[:-1, :-1] == Cm[1:, :-1]) | (Cm[:-1, :-1] == Cm[:-1, 1:]) | (Cm[1:, :-1] == Cm[:-1, 1:])).sum() > inner.size // 4)
    assert ties >= 100, "the tie-heavy matrices do not tie"
    # first row and first column: the only path
    assert R.dtw(np.ones((1, 9)))[:2] == (9.0, 9) and R.dtw(np.ones((9, 1)))[:2] == (9.0, 9) and R.dtw(np.full((1, 1), 2.5))[:2] == (2.5, 1)


def test_diagonal_form_of_the_reference_equals_the_loops():
    for d in _matrices()[::3]:
        for dtype in (np.float64, np.float32):
            Cm, Ln = R.dtw_tables(d, dtype)
            Cd, Ld = R.dtw_tables_by_diagonals(d, dtype)
            assert Cd.dtype == dtype and Cm.tobytes() == Cd.tobytes() and (Ln == Ld).all()


@pytest.mark.parametrize("D", [48, 512])
def test_exact_case_is_exact_and_ties_in_every_way_at_every_place(D):
    """The exact-data case of the GPU test: every distance is an integer of at most 64 D <= 2^15, every cost stays below 2^24 (f32
    holds it exactly), and every kind of tie among the three predecessors occurs next to the first row and column, either side of the
    stripe edge and at a last cell.  (Next to the first row or column the diagonal neighbour is never the largest: costs do not fall
    along the first row and column.)"""
    rows, pairs = R.exact_case(D)
    assert np.abs(rows).max() <= 4 and (rows == np.round(rows)).all()
    assert {(int(p[1]), int(p[3])) for p in pairs} >= {(a, b) for a in R.EXACT_LENGTHS for b in R.EXACT_LENGTHS}
    x = rows.astype(np.float64)
    seen = {p: set() for p in R.TIE_PLACES}
    for af, la, bf, lb in pairs:
        d = R.frame_distances(x[af:af + la], x[bf:bf + lb], 2)
        assert d.max() <= 64 * D and (d == np.round(d)).all()
        Cm, _ = R.dtw_tables_by_diagonals(d)
        assert Cm.max() < 2 ** 24
        assert R.dtw_tables_by_diagonals(d, np.float32)[0].astype(np.float64).tobytes() == Cm.tobytes()
        for place, kinds in R.tie_kinds(Cm).items():
            seen[place] |= kinds
    assert seen["first"] == set(R.TIE_KINDS) - {"left=upper<diagonal"}
    for place in ("row 63", "row 64", "last"):
        assert seen[place] == set(R.TIE_KINDS), (place, seen[place])


def test_tie_order_diagonal_then_left_then_upper():
    # C[0][1] (upper of (1, 1)) = 2, C[1][0] (left) = 2, C[0][0] (diagonal) = 1 or 3
    d = np.array([[1.0, 1.0], [1.0, 5.0]])
    assert R.dtw(d)[:2] == (6.0, 2)                                  # the diagonal wins: 2 cells
    d = np.array([[3.0, -1.0], [-1.0, 5.0]])
    Cm, Ln = R.dtw_tables(d)
    assert Cm[1, 1] == 7.0 and Ln[1, 1] == 3                         # left = upper = 2 below the diagonal 3: the left cell
    d = np.array([[2.0, 0.0, 0.0], [5.0, 1.0, 1.0]])                 # (1, 2): diagonal 2 = upper 2 < left 3: the diagonal
    Cm, Ln = R.dtw_tables(d)
    assert Cm[1, 2] == 3.0 and Ln[1, 2] == Ln[0, 1] + 1 == 3


def test_reference_count_by_loops_and_by_columns_agree():
    rng = np.random.default_rng(1)
    dist = rng.integers(0, 4, size=200).astype(np.float32)
    for task in ((0, 10, 0, 4, 4, 6), (100, 10, 3, 2, 0, 3), (0, 10, 5, 5, 0, 1)):
        assert R.abx_count(dist, task) == R.abx_count_fast(dist, task)
    assert R.abx_count(np.zeros(100, np.float32), (0, 10, 0, 4, 4, 6)) == 4 * 3 * 6          # all ties: one per triple
    assert R.abx_count(dist, (150, 10, 0, 4, 4, 6)) == -2 and R.abx_count(dist, (0, 10, 0, 1, 4, 6)) == -2
    assert R.abx_count(dist, (0, 10, 7, 4, 0, 6)) == -2 and R.abx_count(dist, (0, 10, 0, 4, 4, 0)) == -2
    bad = dist.copy()
    bad[0 * 10 + 0] = np.nan                                           # d(x, x): never read
    assert R.abx_count(bad, (0, 10, 0, 4, 4, 6)) == R.abx_count(dist, (0, 10, 0, 4, 4, 6))
    bad[1 * 10 + 0] = np.nan
    assert R.abx_count(bad, (0, 10, 0, 4, 4, 6)) == -1 == R.abx_count_fast(bad, (0, 10, 0, 4, 4, 6))


# ======================================================================================================================== items
def test_frame_rule_and_dropped_items():
    # 100 frames per second: frame t is kept if (t + 0.5) / 100 lies in [onset, offset)
    first, last = A.frames_of([0.0, 0.005, 0.0051, 0.1, 0.104, 0.1051], [0.0, 0.025, 0.0249, 0.2, 0.106, 0.1149], 100.0)
    assert first.tolist() == [0, 0, 1, 10, 10, 11] and last.tolist() == [0, 2, 2, 20, 11, 11]
    rng = np.random.default_rng(0)
    on = np.concatenate([rng.random(300) * 3, np.arange(40) / 100.0, (np.arange(40) + 0.5) / 100.0])
    off = on + np.concatenate([rng.random(300) * 0.5, np.arange(40) / 200.0, np.arange(40) / 200.0])
    for rate in (100.0, 62.5, 49.95):
        first, last = A.frames_of(on, off, rate)
        for o, f, lo, hi in zip(on, off, first, last):
            kept = [t for t in range(400) if o <= (t + 0.5) / rate < f]
            assert kept == list(range(lo, hi)), (o, f, rate)
    items, report = A.items_from_times([0.0, 0.1, 0.2, 1.0], [0.05, 0.104, 1.6, 2.28], 100.0, file=[0, 1, 2, 3], phone=[5, 6, 7, 8])
    assert report["empty"].tolist() == [1] and report["too_long"].tolist() == [2] and report["dropped"] == 2
    assert report["kept"].tolist() == [0, 3]
    assert items.file.tolist() == [0, 3] and items.first.tolist() == [0, 100] and items.last.tolist() == [5, 228]
    assert items.phone.tolist() == [5, 8] and items.context.tolist() == [0, 0] and items.first.dtype == np.int64
    assert len(items) == 2
    with pytest.raises(ValueError):
        A.Items([0, 1], [0], [1], [0], [0], [0])


def test_read_item_file(tmp_path):
    path = tmp_path / "dev.item"
    path.write_text("#file onset offset #phone prev-phone next-phone speaker\n"
                    "rec_b 0.10 0.20 ae k t spk2\n"
                    "rec_a 0.00 0.08 k sil ae spk1\n"
                    "\n"
                    "rec_a 0.08 0.081 ae k t spk1\n"
                    "rec_b 0.30 0.45 k sil ae spk2\n")
    items, names, report = A.read_item_file(str(path))          # (100 frames per second unless told otherwise)
    assert names == {"files": ["rec_a", "rec_b"], "phones": ["ae", "k"], "contexts": [("k", "t"), ("sil", "ae")], "speakers": ["spk1", "spk2"]}
    assert report["dropped"] == 1 and report["empty"].tolist() == [2]
    assert items.file.tolist() == [1, 0, 1] and items.phone.tolist() == [0, 1, 1] and items.context.tolist() == [0, 1, 1]
    assert items.speaker.tolist() == [1, 0, 1] and items.first.tolist() == [10, 0, 30] and items.last.tolist() == [20, 8, 45]
    items2, names2, _ = A.read_item_file(str(path), 100.0, files=["rec_b", "x", "rec_a"])
    assert items2.file.tolist() == [0, 2, 0] and names2["files"] == ["rec_b", "x", "rec_a"]
    with pytest.raises(ValueError, match="not in the given list"):
        A.read_item_file(str(path), 100.0, files=["rec_b"])
    bad = tmp_path / "bad.item"
    bad.write_text("rec_a 0 1 k a b s\n")
    with pytest.raises(ValueError, match="header"):
        A.read_item_file(str(bad), 100.0)
    bad.write_text("#h\nrec_a 0 1 k a b\n")
    with pytest.raises(ValueError, match="7 columns"):
        A.read_item_file(str(bad), 100.0)


# ===================================================================================================================== planning
def _items(cols):
    return A.Items(*(cols[c] for c in A.COLUMNS))


def test_tables_of_a_hand_made_item_set():
    # two recordings of 50 frames; cell (context 0, speaker 0): phone 1 twice, phone 2 once; cell (context 1, speaker 0): phone 2 once
    cols = dict(file=[0, 1, 0, 0], first=[10, 5, 0, 30], last=[14, 8, 6, 31], phone=[2, 1, 1, 2], context=[0, 0, 0, 1], speaker=[0, 0, 0, 0])
    plan = A.plan_abx(_items(cols), [0, 50, 100])
    # the cell's items group after group: phone 1 = items 1, 2 (input order), phone 2 = item 0
    segs = [(55, 3), (0, 6), (10, 4)]
    want = [a + b for a in segs for b in segs] + [(30, 1, 30, 1)]
    assert plan.pairs.tolist() == [list(w) for w in want]
    assert plan.tasks.tolist() == [[0, 3, 0, 2, 2, 1]]          # (phone 1, phone 2) only: phone 2 holds one item, the other cell one phone
    assert plan.keys.tolist() == [[0, 0, 1, 2]] and plan.picked.tolist() == [1, 2, 0, 3]
    pairs, tasks, keys, picked = R.plan(cols, [0, 50, 100])
    assert (pairs == plan.pairs).all() and (tasks == plan.tasks).all() and (keys == plan.keys).all() and (picked == plan.picked).all()
    pooled = A.plan_abx(_items(cols), [0, 50, 100], by=("context",))
    assert pooled.keys.tolist() == [[0, 1, 2]]
    for kw in (dict(by=()), dict(by=("phone",)), dict(by=("context", "context")), dict(max_group=1), dict(max_group=1025)):
        with pytest.raises(ValueError):
            A.plan_abx(_items(cols), [0, 50, 100], **kw)
    for change in (dict(file=[0, 2, 0, 0]), dict(last=[14, 8, 6, 30]), dict(last=[14, 8, 6, 159]), dict(first=[10, 5, -1, 30]),
                   dict(last=[14, 8, 51, 31]), dict(file=[0, -1, 0, 0])):
        with pytest.raises(ValueError):
            A.plan_abx(_items({**cols, **change}), [0, 50, 100])
    with pytest.raises(ValueError, match="no items"):
        A.plan_abx(_items({c: [] for c in cols}), [0, 50, 100])


@pytest.mark.parametrize("by", [("context", "speaker"), ("context",), ("speaker", "context")])
def test_sub_sampling_consumes_the_generator_in_group_order(by):
    case = R.synthetic_case("mixed")
    items = _items(case["items"])
    for max_group, seed in ((3, 0), (3, 5), (4, 0), (1024, 0)):
        plan = A.plan_abx(items, case["offsets"], max_group=max_group, seed=seed, by=by)
        pairs, tasks, keys, picked = R.plan(case["items"], case["offsets"], max_group, seed, by)
        assert (pairs == plan.pairs).all() and (tasks == plan.tasks).all() and (keys == plan.keys).all() and (picked == plan.picked).all()
        assert plan.tasks[:, [3, 5]].max() <= max_group
    # by hand: the first group in lexicographic order takes the generator's first draw, the second its second
    cols = {c: np.asarray(v) for c, v in case["items"].items()}
    rng = np.random.default_rng(5)
    plan = A.plan_abx(items, case["offsets"], max_group=3, seed=5, by=("context", "speaker"))
    at = 0
    for ctx in (0, 1):
        for spk in (0, 1):
            for ph in (0, 1, 2):
                members = np.flatnonzero((cols["context"] == ctx) & (cols["speaker"] == spk) & (cols["phone"] == ph))
                assert members.size > 3
                keep = members[np.sort(rng.choice(members.size, 3, replace=False))]
                assert plan.picked[at:at + 3].tolist() == keep.tolist()
                at += 3
    other = A.plan_abx(items, case["offsets"], max_group=3, seed=6)
    assert other.picked.tolist() != plan.picked.tolist()


def test_averaging_order_matters_and_is_followed():
    # (context, speaker, p, q): context 0 holds speakers 0, 1, 2, context 1 holds speaker 0; one phone pair plus its mirror
    keys = [(0, 0, 1, 2), (0, 1, 1, 2), (0, 2, 1, 2), (1, 0, 1, 2), (0, 0, 2, 1)]
    scores = [1.0, 0.5, 0.0, 0.9, 0.3]
    mean, table = A.average_scores(keys, scores)
    assert table == {(1, 2): pytest.approx((0.5 + 0.9) / 2, abs=1e-15), (2, 1): pytest.approx(0.3, abs=1e-15)}
    assert mean == pytest.approx((0.7 + 0.3) / 2, abs=1e-15)
    flat = sum(scores) / 5                                            # no levels: 0.54
    by_pair_only = ((1.0 + 0.5 + 0.0 + 0.9) / 4 + 0.3) / 2            # contexts and speakers pooled: 0.45
    assert abs(mean - flat) > 0.03 and abs(mean - by_pair_only) > 0.03
    rmean, rtable = R.average(keys, scores)
    assert abs(rmean - mean) <= 1e-15 and rtable.keys() == table.keys()
    # one level (speakers pooled into the cells)
    mean1, table1 = A.average_scores([(0, 1, 2), (1, 1, 2), (0, 2, 1)], [0.2, 0.6, 1.0])
    assert table1 == {(1, 2): pytest.approx(0.4, abs=1e-15), (2, 1): 1.0} and mean1 == pytest.approx(0.7, abs=1e-15)
    with pytest.raises(ValueError):
        A.average_scores([(0, 0, 1, 2), (0, 0, 1, 2)], [0.1, 0.2])


def test_separated_classes_have_a_margin_above_four_tolerances():
    """For the arrays of the GPU test: in float64 every d(a, x) lies below every d(b, x) by more than four times the tolerance of an f32
    DTW distance, so the reference alone gives the error 0 and rounding cannot change a comparison."""
    case = R.synthetic_case("separated")
    rows = case["rows"].astype(np.float64)
    pairs, tasks, keys, _ = R.plan(case["items"], case["offsets"])
    assert tasks.shape[0] >= 20
    dist, tol = np.zeros(pairs.shape[0]), 0.0
    for i, (af, la, bf, lb) in enumerate(pairs):
        a, b = rows[af:af + la], rows[bf:bf + lb]
        dist[i] = R.dtw(R.frame_distances(a, b, 0))[2]
        tol = max(tol, R.dtw_tolerance(a, b, 0))
    worst = np.inf
    for off, nc, sp, n_p, sq, n_q in tasks:
        cell = dist[off:off + nc * nc].reshape(nc, nc)
        for x in range(n_p):
            same = np.delete(cell[sp:sp + n_p, sp + x], x)
            worst = min(worst, cell[sq:sq + n_q, sp + x].min() - same.max())
    print(f"smallest margin {worst:.4g}, tolerance {tol:.4g}: {worst / tol:.3g} tolerances")
    assert worst > 4 * tol
    valid, scores = R.scores_from(dist, tasks)
    assert valid.all() and (scores == 1.0).all() and R.average(keys, scores)[0] == 1.0


# ==================================================================================================================== refusals
BAD_STORE = [dict(x=None), dict(x=P4), dict(dtype=2), dict(dtype=-1), dict(N=0), dict(N=-1), dict(N=2 ** 31), dict(D=0), dict(D=8),
             dict(D=24), dict(D=528, ldx=528), dict(D=-16), dict(ldx=48), dict(ldx=66), dict(dtype=_hip.BF16, ldx=68), dict(metric=3),
             dict(metric=-1)]


def test_frame_distance_refuses_bad_arguments():
    lib = _hip.lib()

    def call(x=P, dtype=_hip.F32, N=1000, D=64, ldx=64, a_first=0, La=10, b_first=20, Lb=12, metric=0, out=P, ldo=12):
        return lib.cpc_frame_distance(x, dtype, LL(N), D, LL(ldx), LL(a_first), La, LL(b_first), Lb, metric, out, LL(ldo), S)

    bad = BAD_STORE + [dict(out=None), dict(out=P2), dict(La=0), dict(La=129), dict(Lb=0), dict(Lb=129, ldo=129), dict(a_first=-1),
                       dict(a_first=991), dict(b_first=-1), dict(b_first=989), dict(ldo=11), dict(a_first=2 ** 40)]
    for kw in bad:
        assert call(**kw) == -22, kw


def test_dtw_refuses_bad_arguments():
    lib = _hip.lib()

    def call(x=P, dtype=_hip.F32, N=1000, D=64, ldx=64, pairs=P, n=5, metric=0, dist=P, cost=P, path_len=P):
        return lib.cpc_dtw(x, dtype, LL(N), D, LL(ldx), pairs, LL(n), metric, dist, cost, path_len, S)

    bad = BAD_STORE + [dict(pairs=None), dict(pairs=P4), dict(dist=None), dict(dist=P2), dict(cost=P2), dict(path_len=P2), dict(n=0),
                       dict(n=-1), dict(n=2 ** 31)]
    for kw in bad:
        assert call(**kw) == -22, kw


def test_abx_count_refuses_bad_arguments():
    lib = _hip.lib()

    def call(dist=P, n_dist=100, tasks=P, T=3, out=P):
        return lib.cpc_abx_count(dist, LL(n_dist), tasks, LL(T), out, S)

    for kw in (dict(dist=None), dict(tasks=None), dict(out=None), dict(dist=P2), dict(tasks=P4), dict(out=P4), dict(n_dist=0),
               dict(n_dist=-1), dict(T=0), dict(T=-1), dict(T=2 ** 31)):
        assert call(**kw) == -22, kw


class _FakeFeatures:
    def __init__(self, **kw):
        self.frame_offsets = [0, 4]
        for k, v in kw.items():
            setattr(self, k, v)


class _Dev(torch.Tensor):
    is_cuda = True


def _dev(*shape, dtype=torch.float32):
    """A tensor of the 'meta' device standing in for a device tensor: nothing can be launched on it, so a refusal that came after the
    first touch of a device would fail differently."""
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(_Dev)


def test_python_refusals_need_no_device():
    assert "abx" in cpc_audio_amd.__all__
    state = torch.get_rng_state()
    good = np.array([[0, 4, 4, 4]], np.int64)
    items = A.Items([0], [0], [4], [0], [0], [0])
    for call in (lambda x: A.dtw_distance(x, good), lambda x: A.frame_distance(x, (0, 4), (4, 4)), lambda x: A.abx_error(x, items)):
        with pytest.raises(ValueError, match="CPU"):
            call(torch.zeros(100, 16))
        with pytest.raises(ValueError, match="CPU"):
            call(_FakeFeatures(c=torch.zeros(4, 16)))
        with pytest.raises(TypeError):
            call([[0.0] * 16] * 8)
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            call(_dev(100, 16, dtype=torch.float16))
        for shape in ((100,), (100, 16, 2), (100, 8), (100, 24), (100, 528), (0, 16)):
            with pytest.raises(ValueError):
                call(_dev(*shape))
        with pytest.raises(ValueError, match="contiguous"):
            call(_dev(16, 100).t())
        with pytest.raises(ValueError, match="contiguous"):
            call(_dev(100, 18)[:, :16])
    with pytest.raises(ValueError, match="holds no"):
        A.dtw_distance(_FakeFeatures(z=torch.zeros(4, 16)), good, kind="c")
    x = _dev(100, 16)
    for metric in ("euclidean", "kl", 0, None):
        with pytest.raises(ValueError, match="metric"):
            A.dtw_distance(x, good, metric=metric)
        with pytest.raises(ValueError, match="metric"):
            A.frame_distance(x, (0, 4), (4, 4), metric=metric)
        with pytest.raises(ValueError, match="metric"):
            A.abx_error(x, items, metric=metric)
    for pairs in ([[0, 0, 4, 4]], [[0, 129, 4, 4]], [[0, 4, 4, 0]], [[0, 4, 4, 129]], [[-1, 4, 4, 4]], [[97, 4, 4, 4]], [[0, 4, 97, 4]],
                  [[0, 4, -5, 4]], np.zeros((0, 4), np.int64), np.zeros((3, 3), np.int64), np.zeros(4, np.int64),
                  torch.tensor([[0, 4, 4, 200]])):
        with pytest.raises(ValueError):
            A.dtw_distance(x, pairs)
    with pytest.raises(TypeError, match="integers"):
        A.dtw_distance(x, np.array([[0.0, 4.0, 4.0, 4.0]]))
    for a, b in (((0, 0), (4, 4)), ((0, 129), (4, 4)), ((-1, 4), (4, 4)), ((0, 4), (97, 4)), ((0, 4), (4, 0))):
        with pytest.raises(ValueError):
            A.frame_distance(x, a, b)
    with pytest.raises(TypeError, match="Items"):
        A.abx_error(x, {"file": [0]})
    with pytest.raises(ValueError, match="no \\(cell, phone, phone\\) task"):
        A.abx_error(x, items)
    with pytest.raises(ValueError, match="beyond"):
        A.abx_error(x, A.Items([0, 0], [0, 90], [4, 101], [0, 1], [0, 0], [0, 0]))
    with pytest.raises(ValueError, match="max_group"):
        A.abx_error(x, items, max_group=1)
    with pytest.raises(ValueError, match="by"):
        A.abx_error(x, items, by=("file",))
    assert torch.equal(torch.get_rng_state(), state)
