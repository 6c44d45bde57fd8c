"""ABX discriminability on the GPU: cpc_frame_distance, cpc_dtw and cpc_abx_count against tests/abx_reference.py, and
cpc_audio_amd.abx (dtw_distance, frame_distance, abx_error) on top of them.  Every output buffer is followed by sentinels that must stay
intact.

Bounds (u = 2^-24; none was obtained by running the code under test).
  Frame distance.  The kernel forms dot as an f32 fmaf chain of D products (the f32-input MFMA) and each squared norm as two fmaf
    chains of D / 2 products whose ends are added once: within D u sum |a_i b_i| and (D / 2 + 1) u |a|^2 of the exact sums (first
    order), inside the D-chain the bounds below allow for.
      metric 2   max(fma(-2, dot, |a|^2 + |b|^2), 0): the two norms, their sum, the chain of the dot and the fma give at most
                 (D + 2) u (|a|^2 + 2 sum |a_i b_i| + |b|^2); the clamp moves nothing apart.
      metric 1   1 - cos, cos = dot / (sqrt(|a|^2) sqrt(|b|^2)) clamped to [-1, 1]: relative to sum |a_i b_i| / (|a| |b|) the dot
                 contributes D u, each root (D / 4 + 1) u, the product of the roots and the quotient u each, so cos is within
                 (1.5 D + 5) u sum |a_i b_i| / (|a| |b|), inside tol_cos = (2 D + 8) u sum |a_i b_i| / (|a| |b|).  The subtraction
                 from 1 rounds once more, at most u (half an ulp of a value below 2): the (D / 2 + 3) u sum |a_i b_i| / (|a| |b|) that
                 tol_cos leaves cover it where sum |a_i b_i| >= |a| |b| / (D / 2 + 3), which the test asserts of its random rows (a
                 property of the input; the ratio tends to 2 / pi).
      metric 0   acosf(cos) / pi: the value must lie in [acos(min(c + tol_cos, 1)), acos(max(c - tol_cos, -1))] / pi, evaluated in
                 float64 at the float64 cosine c, widened by 4 + 1 f32 ulps of the interval's ends: 1 ulp for the division by the f32
                 value of pi (half an ulp for the rounding, a quarter for the constant), and 4 ulp ASSUMED for acosf: no accuracy
                 statement for acosf was found in the documentation installed with the device library, see DESIGN.md.
  Exact data.  Integer rows of magnitude <= 4, metric 2: every distance is an integer of at most 64 D <= 2^15 and a path of at most
    255 cells stays below 2^24 (asserted by test_abx_host.py for these arrays), so f32 is exact: cost and path_len must equal the
    float64 reference in every bit, dist its numpy.float32 quotient.
  Recurrence.  cpc_dtw against the float32 reference recurrence run on the matrix cpc_frame_distance returns for the same rows: every
    bit of cost, path_len and dist.  The matrices themselves are held to float64 by the first test, so no bound on the data-dependent
    path is needed and no pair is excused.
  Counts.  Integers: exact.
  abx_error.  Scores are ratios of exact integers; the reference's averaging differs by rounding of a few float64 additions: 1e-12.
  Separated classes: test_abx_host.py asserts in float64 that every same-phone distance lies below every other-phone distance by more
    than 4 tolerances of an f32 DTW distance (it is above 600), so every comparison must come out right and the error is exactly 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd import abx as A  # noqa: E402
from cpc_audio_amd import clustering as KM  # noqa: E402
from cpc_audio_amd import feature_extraction as FE  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset  # noqa: E402
import abx_reference as R  # noqa: E402
import feature_extraction_reference as FR  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
GUARD = 64
LL = C.c_longlong
U = 2.0 ** -24
SENT = {torch.int32: -12345, torch.float32: -7.5, torch.int64: -12345}


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def guarded(n, dt):
    """n elements to be written, followed by GUARD sentinels: (whole buffer, view of the n); the n start out as the sentinel too."""
    buf = torch.full((n + GUARD,), SENT[dt], device=DEV, dtype=dt)
    return buf, buf[:n]


def intact(buf, n):
    return bool((buf[n:] == SENT[buf.dtype]).all())


def device_rows(x, dt, pad):
    """x (numpy f32 [N, D]) on the device as dt at a row stride of D + pad, NaN in the padding; returns (view, the values as f64)."""
    N, D = x.shape
    full = torch.full((N, D + pad), float("nan"), device=DEV, dtype=dt)
    full[:, :D] = torch.tensor(x).to(DEV).to(dt)
    view = full[:, :D]
    return view, view.float().double().cpu().numpy()


def run_frame_distance(xv, a, b, metric, ldo_pad=3):
    """cpc_frame_distance into a guarded buffer with a row stride of Lb + ldo_pad; returns the [La, Lb] matrix as numpy f32."""
    N, D = xv.shape
    (af, La), (bf, Lb) = a, b
    ldo = Lb + ldo_pad
    buf, out = guarded(La * ldo, F32)
    _hip.call("cpc_frame_distance", _hip.ptr(xv), _hip.dtype_code(xv.dtype), LL(N), D, LL(xv.stride(0) if N > 1 else D), LL(af), La, LL(bf),
              Lb, metric, _hip.ptr(out), LL(ldo))
    torch.cuda.synchronize()
    assert intact(buf, La * ldo)
    got = out.reshape(La, ldo).cpu().numpy()
    assert (got[:, Lb:] == SENT[F32]).all(), "written beyond the row's Lb values"
    return got[:, :Lb].copy()


def run_dtw(xv, pairs, metric, want_path=True):
    """cpc_dtw on a host pair table; returns (dist, cost, path_len) as numpy after checking the sentinels."""
    N, D = xv.shape
    pd = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int64)).to(DEV)
    P = pd.shape[0]
    dbuf, dist = guarded(P, F32)
    cbuf, cost = guarded(P, F32)
    lbuf, plen = guarded(P, torch.int32)
    _hip.call("cpc_dtw", _hip.ptr(xv), _hip.dtype_code(xv.dtype), LL(N), D, LL(xv.stride(0) if N > 1 else D), _hip.ptr(pd), LL(P), metric,
              _hip.ptr(dist), _hip.ptr(cost) if want_path else None, _hip.ptr(plen) if want_path else None)
    torch.cuda.synchronize()
    assert intact(dbuf, P) and intact(cbuf, P) and intact(lbuf, P)
    if not want_path:
        assert bool((cost == SENT[F32]).all()) and bool((plen == SENT[torch.int32]).all()), "cost / path_len written although NULL was passed"
    return dist.cpu().numpy(), cost.cpu().numpy(), plen.cpu().numpy().astype(np.int64)


# ============================================================================================================ 1. frame distance
# a pruned product: every shape, D, padding, dtype and metric of the issue appears, the long shapes meet the large D
FD_CASES = [((1, 1), 16, 0, F32, 0), ((1, 1), 512, 16, BF16, 2), ((1, 128), 48, 16, F32, 1), ((1, 128), 16, 0, BF16, 0),
            ((128, 1), 512, 0, F32, 2), ((128, 1), 48, 16, BF16, 1), ((31, 33), 16, 16, F32, 2), ((31, 33), 48, 0, BF16, 0),
            ((31, 33), 512, 16, F32, 1), ((64, 64), 48, 0, F32, 0), ((64, 64), 512, 16, BF16, 1), ((64, 64), 16, 0, BF16, 2),
            ((65, 63), 512, 0, F32, 0), ((65, 63), 16, 16, BF16, 1), ((65, 63), 48, 16, F32, 2), ((128, 128), 512, 16, F32, 0),
            ((128, 128), 48, 0, BF16, 2), ((128, 128), 16, 16, F32, 1), ((128, 128), 512, 0, BF16, 0)]


def check_frame_distances(got, a, b, metric, what):
    """The matrix against float64 within the docstring's bounds; prints the largest error as a fraction of the bound."""
    assert np.isfinite(got).all()
    got = got.astype(np.float64)
    want = R.frame_distances(a, b, metric)
    if metric == 2:
        frac = np.abs(got - want) / R.tol_sqeuclidean(a, b)
    elif metric == 1:
        spread = (np.abs(a) @ np.abs(b).T) / np.sqrt((a * a).sum(1)[:, None] * (b * b).sum(1)[None, :])
        assert spread.min() >= 1.0 / (a.shape[1] / 2 + 3), "the bound's room for the last subtraction needs a larger sum |a_i b_i|"
        frac = np.abs(got - want) / R.tol_cos(a, b)
    else:
        lo, hi = R.angular_interval(a, b)
        half = np.maximum((hi - lo) / 2, np.finfo(np.float64).tiny)
        frac = np.abs(got - (lo + hi) / 2) / half
        assert (got >= 0).all() and (got <= 1).all()
    print(f"{what}: largest error {frac.max():.3g} of the bound")
    assert (frac <= 1.0).all()
    if metric != 0:
        assert (got >= 0).all()


@pytest.mark.parametrize("shape,D,pad,dt,metric", FD_CASES, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_frame_distance_against_float64(shape, D, pad, dt, metric):
    La, Lb = shape
    rng = np.random.default_rng(La * 131 + Lb * 7 + D + metric)
    N = La + Lb + 37
    x = rng.standard_normal((N, D)).astype(np.float32)
    xv, xw = device_rows(x, dt, pad)
    af, bf = 5, N - Lb - 3
    got = run_frame_distance(xv, (af, La), (bf, Lb), metric)
    check_frame_distances(got, xw[af:af + La], xw[bf:bf + Lb], metric, f"{shape} D={D} ld={D + pad} {dt} metric {metric}")


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_frame_distance_of_a_segment_against_itself_and_an_overlapping_one(metric, dt):
    rng = np.random.default_rng(metric)
    x = rng.standard_normal((150, 48)).astype(np.float32)
    xv, xw = device_rows(x, dt, 16)
    same = run_frame_distance(xv, (10, 70), (10, 70), metric)
    check_frame_distances(same, xw[10:80], xw[10:80], metric, f"self {dt} metric {metric}")
    assert (same.view(np.int32) == same.T.copy().view(np.int32)).all(), "d(a, b) and d(b, a) differ in a bit"
    over = run_frame_distance(xv, (10, 70), (45, 100), metric)
    check_frame_distances(over, xw[10:80], xw[45:145], metric, f"overlap {dt} metric {metric}")
    # the rows both calls share give the same bits wherever they sit in a tile
    assert (over[35:70, 0:35].view(np.int32) == same[35:70, 35:70].view(np.int32)).all()


# ================================================================================================================ 2. exact data
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [48, 512])
def test_dtw_exact_data_and_planted_ties(D, dt):
    rows, pairs = R.exact_case(D)
    xv, xw = device_rows(rows, dt, 16)
    assert (xw == rows).all()
    dist, cost, plen = run_dtw(xv, pairs, 2)
    for p, (af, la, bf, lb) in enumerate(pairs):
        c64, n64, _ = R.dtw(R.frame_distances(xw[af:af + la], xw[bf:bf + lb], 2))
        assert plen[p] == n64, (p, la, lb)
        assert bits32(cost[p]) == bits32(np.float32(c64)) and float(cost[p]) == c64, (p, la, lb)
        assert bits32(dist[p]) == bits32(np.float32(c64) / np.float32(n64)), (p, la, lb)


# ================================================================================================= 3. the recurrence, bit for bit
def mixed_pairs(P, N, rng):
    """P pairs with lengths 1 .. 128 of every class on both sides, repeated pairs and pairs that share rows."""
    edges = [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128]
    la = np.array([edges[i % len(edges)] if i < 2 * len(edges) else int(rng.integers(1, 129)) for i in range(P)])
    lb = np.array([edges[(i // 2) % len(edges)] if i < 2 * len(edges) else int(rng.integers(1, 129)) for i in range(P)])
    af = np.array([int(rng.integers(0, N - l + 1)) for l in la])
    bf = np.array([int(rng.integers(0, N - l + 1)) for l in lb])
    pairs = np.stack([af, la, bf, lb], 1).astype(np.int64)
    if P >= 8:
        pairs[5] = pairs[2]                                         # a repeated pair
        pairs[6] = (pairs[3, 0], pairs[3, 1], pairs[3, 0], pairs[3, 1])          # a segment against itself
        pairs[7, 2] = max(0, min(N - int(pairs[7, 3]), int(pairs[7, 0]) + 1))    # overlapping segments
    return pairs


def length_class(n):
    return 0 if n == 1 else 1 if n < 32 else 2 if n == 32 else 3 if n < 64 else 4 if n == 64 else 5 if n == 65 else 6 if n < 128 else 7


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("P,dt,D", [(1, F32, 16), (65, BF16, 48), (1000, F32, 32)], ids=["P1", "P65", "P1000"])
def test_dtw_equals_the_f32_recurrence_on_the_kernels_own_matrix(P, dt, D, metric):
    rng = np.random.default_rng(P + metric)
    N = 700
    x = rng.standard_normal((N, D)).astype(np.float32)
    xv, _ = device_rows(x, dt, 16)
    pairs = mixed_pairs(P, N, rng)
    dist, cost, plen = run_dtw(xv, pairs, metric)
    assert np.isfinite(dist).all() and (plen >= np.maximum(pairs[:, 1], pairs[:, 3])).all() and (plen <= pairs[:, 1] + pairs[:, 3] - 1).all()
    # about 40 pairs: the first of every (class of La, class of Lb) met, the hand-made ones, then in order
    sample, seen = [], set()
    for p in range(P):
        k = (length_class(pairs[p, 1]), length_class(pairs[p, 3]))
        if p < 8 or (k not in seen and len(sample) < 40):
            sample.append(p)
            seen.add(k)
    if P >= 65:
        assert {k[0] for k in seen} == set(range(8)) and {k[1] for k in seen} == set(range(8))
    for p in sample:
        af, la, bf, lb = (int(v) for v in pairs[p])
        d = run_frame_distance(xv, (af, la), (bf, lb), metric, ldo_pad=0)
        c32, n32, q32 = R.dtw(d, np.float32)
        assert plen[p] == n32, (p, la, lb)
        assert bits32(cost[p]) == bits32(c32) and bits32(dist[p]) == bits32(q32), (p, la, lb, cost[p], c32)
    # the same bits from a second launch, without the optional outputs, and pair by pair
    again = run_dtw(xv, pairs, metric)
    assert (bits32(again[0]) == bits32(dist)).all() and (bits32(again[1]) == bits32(cost)).all() and (again[2] == plen).all()
    assert (bits32(run_dtw(xv, pairs, metric, want_path=False)[0]) == bits32(dist)).all()
    pd = torch.from_numpy(pairs).to(DEV)
    single = torch.full((P,), SENT[F32], device=DEV)
    for p in range(P):
        _hip.call("cpc_dtw", _hip.ptr(xv), _hip.dtype_code(dt), LL(N), D, LL(xv.stride(0)), _hip.ptr(pd, 4 * p), LL(1), metric,
                  _hip.ptr(single, p), None, None)
    torch.cuda.synchronize()
    assert (bits32(single.cpu().numpy()) == bits32(dist)).all()
    # the Python surface: the same bits from a host table and from a device table
    for table in (pairs, pd):
        d2, c2, l2 = A.dtw_distance(xv, table, metric=["angular", "cosine", "sqeuclidean"][metric], return_path=True)
        assert d2.dtype == F32 and c2.dtype == F32 and l2.dtype == torch.int32 and d2.shape == (P,)
        assert (bits32(d2.cpu().numpy()) == bits32(dist)).all() and (bits32(c2.cpu().numpy()) == bits32(cost)).all()
        assert (l2.cpu().numpy() == plen).all()
    af, la, bf, lb = (int(v) for v in pairs[0])
    m = A.frame_distance(xv, (af, la), (bf, lb), metric=["angular", "cosine", "sqeuclidean"][metric])
    assert m.shape == (la, lb) and (bits32(m.cpu().numpy()) == bits32(run_frame_distance(xv, (af, la), (bf, lb), metric))).all()


# ================================================================================================================= 4. isolation
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_dtw_bad_rows_and_bad_table_rows_touch_no_other_pair(metric, dt):
    rng = np.random.default_rng(9)
    N, D = 600, 48
    x = rng.standard_normal((N, D)).astype(np.float32)
    pairs = mixed_pairs(60, 500, rng)                      # the segments of the clean pairs lie in rows [0, 500)
    clean = run_dtw(device_rows(x, dt, 16)[0], pairs, metric)
    dirty = x.copy()
    dirty[510, 7] = np.nan
    dirty[530, 47] = np.inf
    dirty[550, 0] = -np.inf
    dirty[570, :] = 0.0
    dirty[590, :] = 3e19                                     # finite, with a squared norm that is not (above 2^116: as a non-finite row)
    dirty[592, 5] = -2e19
    # a bad row first, last and in the middle of a segment, on either side, in the first and in the second stripe
    extra = np.array([(510, 1, 0, 5), (0, 5, 510, 1), (500, 11, 10, 70), (20, 100, 505, 6), (440, 100, 100, 100), (100, 128, 403, 128),
                      (530, 3, 30, 3), (549, 2, 549, 2), (450, 101, 0, 1), (590, 1, 0, 4), (40, 70, 588, 5), (592, 1, 592, 1),
                      (570, 1, 0, 4), (0, 4, 565, 6), (560, 11, 3, 3)], np.int64)
    zero_rows = 3                                            # the last three hold the zero row: bad for metrics 0 and 1 only
    table_bad = np.array([(0, 0, 5, 5), (0, 129, 5, 5), (5, 5, 0, 0), (5, 5, 0, 129), (-1, 5, 5, 5), (5, 5, -3, 5), (N - 4, 5, 5, 5),
                          (5, 5, N - 127, 128), (2 ** 40, 5, 5, 5), (5, 2 ** 33, 5, 5), (5, 5, 5, -2 ** 40), (-2 ** 62, 128, 2 ** 62, 128)],
                         np.int64)
    order = np.arange(60 + len(extra) + len(table_bad))
    rng.shuffle(order)
    everything = np.concatenate([pairs, extra, table_bad])[order]
    dist, cost, plen = run_dtw(device_rows(dirty, dt, 16)[0], everything, metric)
    where = np.empty_like(order)
    where[order] = np.arange(order.size)                    # where[i]: the place of pair i of the concatenation
    keep = where[:60]
    assert (bits32(dist[keep]) == bits32(clean[0])).all() and (bits32(cost[keep]) == bits32(clean[1])).all()
    assert (plen[keep] == clean[2]).all()
    n_bad_rows = len(extra) - (zero_rows if metric == 2 else 0)
    bad = np.concatenate([where[60:60 + n_bad_rows], where[60 + len(extra):]])
    assert np.isnan(dist[bad]).all() and np.isnan(cost[bad]).all() and (plen[bad] == -1).all()
    if metric == 2:                                          # a zero row is a row like any other for the squared Euclidean distance
        ok = where[60 + n_bad_rows:60 + len(extra)]
        assert np.isfinite(dist[ok]).all() and (plen[ok] > 0).all()
    # NULL cost and path_len: nothing written where they would be
    d2, _, _ = run_dtw(device_rows(dirty, dt, 16)[0], everything, metric, want_path=False)
    assert (bits32(d2) == bits32(dist)).all()
    # large rows below the limit on the squared norm (48 * 10^32 < 2^116) are rows like any other
    dirty[594:598, :] = 1e16
    big = run_dtw(device_rows(dirty, dt, 16)[0], np.array([(594, 4, 0, 4), (594, 2, 596, 2)], np.int64), metric)
    assert np.isfinite(big[0]).all() and np.isfinite(big[1]).all() and (big[2] >= 2).all()


def test_tables_beyond_one_grid_go_out_in_several_launches():
    """The runtime refuses a grid of 2^32 threads, so one cpc_dtw call holds at most 2^25 pairs per launch and one cpc_abx_count call 2^23
    tasks: tables just beyond that size, made of rows the kernels refuse at once (zeros: a length of 0, a group of 0 items), with real
    rows either side of the edge and at the end.  Every row must be answered, the real ones with the bits of a launch of their own."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    xv, _ = device_rows(x, F32, 0)
    real = mixed_pairs(4, 300, rng)
    want = run_dtw(xv, real, 0)
    edge = 2 ** 25
    P = edge + 5
    spots = [0, edge - 1, edge, P - 1]
    table = torch.zeros((P, 4), device=DEV, dtype=torch.int64)
    table[spots] = torch.from_numpy(real).to(DEV)
    dbuf, dist = guarded(P, F32)
    cbuf, cost = guarded(P, F32)
    lbuf, plen = guarded(P, torch.int32)
    _hip.call("cpc_dtw", _hip.ptr(xv), _hip.F32, LL(300), 16, LL(16), _hip.ptr(table), LL(P), 0, _hip.ptr(dist), _hip.ptr(cost), _hip.ptr(plen))
    torch.cuda.synchronize()
    assert intact(dbuf, P) and intact(cbuf, P) and intact(lbuf, P)
    assert (bits32(dist[spots].cpu().numpy()) == bits32(want[0])).all() and (bits32(cost[spots].cpu().numpy()) == bits32(want[1])).all()
    assert (plen[spots].cpu().numpy() == want[2]).all()
    assert int(torch.isnan(dist).sum()) == P - 4 and int(torch.isnan(cost).sum()) == P - 4 and int((plen == -1).sum()) == P - 4
    del table, dbuf, cbuf, lbuf
    # the counts: 2^23 + 3 tasks
    nc = 6
    d = torch.from_numpy((rng.integers(0, 3, size=nc * nc) * 0.5).astype(np.float32)).to(DEV)
    task = np.array([(0, nc, 0, 3, 3, 3), (0, nc, 2, 4, 0, 2), (0, nc, 0, 2, 2, 4)], np.int64)
    want_c = [R.abx_count(d.cpu().numpy(), t) for t in task]
    edge = 2 ** 23
    T = edge + 3
    spots = [edge - 1, edge, T - 1]
    tasks = torch.zeros((T, 6), device=DEV, dtype=torch.int64)
    tasks[spots] = torch.from_numpy(task).to(DEV)
    obuf, out = guarded(T, torch.int64)
    _hip.call("cpc_abx_count", _hip.ptr(d), LL(nc * nc), _hip.ptr(tasks), LL(T), _hip.ptr(out))
    torch.cuda.synchronize()
    assert intact(obuf, T) and out[spots].cpu().tolist() == want_c and min(want_c) > 0
    assert int((out == -2).sum()) == T - 3


# ================================================================================================================== 5. abx count
def run_count(dist, tasks):
    d = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32)).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(tasks, dtype=np.int64)).to(DEV)
    T = t.shape[0]
    buf, out = guarded(T, torch.int64)
    _hip.call("cpc_abx_count", _hip.ptr(d), LL(d.shape[0]), _hip.ptr(t), LL(T), _hip.ptr(out))
    torch.cuda.synchronize()
    assert intact(buf, T)
    return out.cpu().numpy()


def test_abx_count_against_brute_force():
    rng = np.random.default_rng(3)
    nc = 140
    dist = rng.integers(0, 5, size=2 * nc * nc + 50).astype(np.float32) * 0.25          # five values: ties are common
    tasks = []
    for n_p in (2, 3, 64, 65):
        for n_q in (1, 2, 64, 65):
            off = int(rng.integers(0, 2)) * nc * nc + int(rng.integers(0, 50))
            sp = int(rng.integers(0, nc - n_p - n_q + 1))
            tasks.append((off, nc, sp, n_p, sp + n_p, n_q))
            tasks.append((off, nc, nc - n_p, n_p, int(rng.integers(0, nc - n_p - n_q + 1)), n_q))
    tasks = np.array(tasks, np.int64)
    want = np.array([R.abx_count_fast(dist, t) for t in tasks], np.int64)
    for t in tasks[:6]:
        assert R.abx_count(dist, t) == R.abx_count_fast(dist, t)
    got = run_count(dist, tasks)
    assert (got == want).all() and (want > 0).all()
    # a NaN on the diagonal of group p is never read; one anywhere else the task reads gives -1, and only for the tasks that read it
    off, _, sp, n_p, sq, n_q = (int(v) for v in tasks[10])
    poisoned = dist.copy()
    for k in range(n_p):
        poisoned[off + (sp + k) * nc + sp + k] = np.nan
    assert (run_count(poisoned, tasks[10:11]) == want[10:11]).all()
    poisoned[off + (sq + n_q - 1) * nc + sp + 1] = np.nan
    assert run_count(poisoned, tasks[10:11])[0] == -1
    lone = np.full(4 * 4, 0.5, np.float32)
    lone[1 * 4 + 2] = np.nan                                # item 1 against x = 2
    assert run_count(lone, [(0, 4, 0, 2, 2, 2), (0, 4, 1, 3, 0, 1), (0, 4, 2, 2, 0, 2)]).tolist() == [2 * 1 * 2, -1, -1]
    # out of range: -2, nothing read (the distances of such a task may lie anywhere)
    small = np.zeros(100, np.float32)
    bad = [(0, 10, 0, 1, 4, 6), (0, 10, 0, 1025, 4, 6), (0, 10, 0, 4, 4, 0), (0, 10, 0, 4, 4, 1025), (0, 10, 7, 4, 0, 6), (0, 10, 0, 4, 5, 6),
           (1, 10, 0, 4, 4, 6), (-1, 10, 0, 4, 4, 6), (0, 11, 0, 4, 4, 6), (0, 0, 0, 4, 4, 6), (0, 10, -1, 4, 4, 6), (0, 10, 0, 4, -1, 6),
           (2 ** 40, 10, 0, 4, 4, 6), (0, 2 ** 40, 0, 4, 4, 6), (0, -10, 0, 4, 4, 6), (0, 10, 0, 4, 4, 6)]
    assert run_count(small, bad).tolist() == [-2] * 15 + [4 * 3 * 6]


def test_abx_count_of_the_largest_groups_in_closed_form():
    n = 1024
    dist = np.full(4 * n * n + 7, 0.75, np.float32)         # constant: every comparison ties, one per triple
    got = run_count(dist, [(7, 2 * n, n, n, 0, n), (7, 2 * n, 0, n, n, n)])
    assert got.tolist() == [n * (n - 1) * n] * 2


# ================================================================================================================== 6. abx_error
class Feats:
    """What abx_error needs of a Features object."""

    def __init__(self, rows, offsets, dt=F32):
        self.c = torch.from_numpy(rows).to(DEV).to(dt)
        self.frame_offsets = [int(v) for v in offsets]


def items_of(case):
    return A.Items(*(case["items"][c] for c in A.COLUMNS))


def test_abx_error_is_zero_on_separated_classes_and_a_half_on_tied_ones():
    case = R.synthetic_case("separated")
    res = A.abx_error(Feats(case["rows"], case["offsets"]), items_of(case))
    pairs, tasks, _, _ = R.plan(case["items"], case["offsets"])
    assert res.error == 0.0 and set(res.pair_scores.values()) == {1.0} and sorted(res.pair_scores) == [(p, q) for p in range(3) for q in range(3) if p != q]
    assert res.n_pairs == pairs.shape[0] and res.n_tasks == tasks.shape[0] and res.n_invalid == 0 and res.phones == [0, 1, 2]
    assert res.n_triples == int((tasks[:, 3] * (tasks[:, 3] - 1) * tasks[:, 5]).sum())
    tied = R.synthetic_case("tied")
    res = A.abx_error(Feats(tied["rows"], tied["offsets"]), items_of(tied))
    assert res.pair_scores[(0, 1)] == 0.5 and res.pair_scores[(1, 0)] == 0.5
    assert res.pair_scores[(0, 2)] == 1.0 and res.pair_scores[(2, 1)] == 1.0 and res.error == pytest.approx(1.0 - 5.0 / 6.0, abs=1e-15)


@pytest.mark.parametrize("by", [("context", "speaker"), ("context",)], ids=["within", "pooled"])
@pytest.mark.parametrize("metric,dt,max_group", [("angular", F32, 10), ("cosine", BF16, 4), ("sqeuclidean", F32, 1024)])
def test_abx_error_equals_the_reference_plan_and_counts_on_the_kernels_distances(metric, dt, max_group, by):
    case = R.synthetic_case("mixed")
    feats = Feats(case["rows"], case["offsets"], dt)
    res = A.abx_error(feats, items_of(case), metric=metric, max_group=max_group, seed=3, by=by)
    pairs, tasks, keys, picked = R.plan(case["items"], case["offsets"], max_group, 3, by)
    dist = A.dtw_distance(feats, pairs, metric=metric).cpu().numpy()
    assert np.isfinite(dist).all()
    valid, scores = R.scores_from(dist, tasks)
    mean, table = R.average(keys[valid], scores)
    assert valid.all() and res.n_invalid == 0 and res.n_pairs == pairs.shape[0] and res.n_tasks == tasks.shape[0]
    assert sorted(res.pair_scores) == sorted(table)
    for k, v in table.items():
        assert abs(res.pair_scores[k] - v) <= 1e-12, k
    assert abs(res.error - (1.0 - mean)) <= 1e-12
    assert 0.0 < res.error < 0.5, "the mixed case is meant to make some errors, and fewer than chance"
    if max_group == 4:
        assert tasks[:, [3, 5]].max() == 4
        other = A.abx_error(feats, items_of(case), metric=metric, max_group=max_group, seed=4, by=by)
        assert other.pair_scores != res.pair_scores           # other items picked
    if by == ("context",):
        assert keys.shape[1] == 3
    # a pair that turns out NaN: its tasks are left out and counted
    broken = case["rows"].copy()
    f, first = int(case["items"]["file"][picked[0]]), int(case["items"]["first"][picked[0]])
    broken[case["offsets"][f] + first, 3] = np.nan
    res2 = A.abx_error(Feats(broken, case["offsets"], dt), items_of(case), metric=metric, max_group=max_group, seed=3, by=by)
    d2 = A.dtw_distance(Feats(broken, case["offsets"], dt), pairs, metric=metric).cpu().numpy()
    v2, s2 = R.scores_from(d2, tasks)
    assert 0 < res2.n_invalid == int((~v2).sum()) < tasks.shape[0]
    assert abs(res2.error - (1.0 - R.average(keys[v2], s2)[0])) <= 1e-12


class _NoHostTraffic:
    """While active, the torch calls that copy between host and device, synchronise or allocate raise."""

    NAMES = [(torch.Tensor, n) for n in ("to", "cpu", "cuda", "item", "tolist", "numpy", "copy_", "clone", "zero_", "contiguous")] + \
            [(torch, n) for n in ("empty", "zeros", "full", "tensor", "as_tensor", "from_numpy")] + [(torch.cuda, "synchronize")]

    def __enter__(self):
        self.saved = [(o, n, getattr(o, n)) for o, n in self.NAMES]
        for o, n, _ in self.saved:
            def refuse(*a, _n=n, **kw):
                raise AssertionError(f"torch {_n} between the launches of abx_error")
            setattr(o, n, refuse)

    def __exit__(self, *exc):
        for o, n, f in self.saved:
            setattr(o, n, f)


def test_abx_error_launch_pattern(monkeypatch):
    """abx._launch_abx is wrapped, not timed: inside it no torch call that copies, synchronises or allocates; it holds every launch,
    cpc_dtw in as many launches as the limit on P needs, then cpc_abx_count."""
    case = R.synthetic_case("mixed")
    feats = Feats(case["rows"], case["offsets"])
    want = A.abx_error(feats, items_of(case))
    body, names, inside, real = A._launch_abx, [], [], _hip.call

    def spy(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)

    def wrapped(run):
        with _NoHostTraffic():
            before = len(names)
            body(run)
            inside.append(names[before:])

    monkeypatch.setattr(A, "_launch_abx", wrapped)
    monkeypatch.setattr(_hip, "call", spy)
    got = A.abx_error(feats, items_of(case))
    assert inside == [["cpc_dtw", "cpc_abx_count"]] and names == inside[0]
    assert got == want
    # a limit of 1000 pairs and tasks per launch: more launches, the same result
    monkeypatch.setattr(A, "MAX_PAIRS", 1000)
    names.clear()
    inside.clear()
    got = A.abx_error(feats, items_of(case))
    n_dtw, n_cnt = -(-want.n_pairs // 1000), -(-want.n_tasks // 1000)
    assert n_dtw > 1 and inside == [["cpc_dtw"] * n_dtw + ["cpc_abx_count"] * n_cnt] and names == inside[0]
    assert got == want


# ========================================================================================================= 7. nothing else moved
def test_abx_error_moves_nothing_else():
    """On features extracted by FeatureExtractor: after abx_error the random state of torch, model.training and the feature tensors
    are what they were, and KMeans.fit beside it gives the bits it gave before."""
    model = FR.model_for("gru", 32, 1).to(DEV)
    src = DeviceAudioDataset(arrays=FR.recordings(), item_length=100, device=DEV, storage="int16")
    feats = FE.FeatureExtractor(model, streams=2, chunk_frames=16).extract(src)
    counts = feats.frame_counts
    assert list(counts) == list(FR.FRAME_COUNTS)
    cols = {c: [] for c in A.COLUMNS}
    for f, n in enumerate(counts):                            # segments of 4 frames, two phones alternating, one context and speaker
        for k, first in enumerate(range(0, n - 3, 4)):
            for c, v in zip(A.COLUMNS, (f, first, first + 4, k % 2, 0, 0)):
                cols[c].append(v)
    items = A.Items(*(cols[c] for c in A.COLUMNS))
    km_before = KM.KMeans(4, iterations=3, seed=1).fit(feats, kind="c")
    torch.cuda.synchronize()
    training = model.training
    state = torch.get_rng_state(), torch.cuda.get_rng_state(0)
    z0, c0 = feats.z.clone(), feats.c.clone()
    res = A.abx_error(feats, items, kind="c")
    resz = A.abx_error(feats, items, kind="z", metric="cosine")
    # one cell of two phones, each above max_group = 10 items: 20 items are kept, 400 pairs, 2 tasks
    assert len(items) == 30 and res.n_pairs == resz.n_pairs == 400 and resz.n_tasks == res.n_tasks == 2
    assert res.n_invalid == 0 and 0.0 <= res.error <= 1.0 and res.n_triples == 2 * 10 * 9 * 10
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(0), state[1])
    assert model.training == training
    assert torch.equal(feats.z, z0) and torch.equal(feats.c, c0)
    km_after = KM.KMeans(4, iterations=3, seed=1).fit(feats, kind="c")
    torch.cuda.synchronize()
    assert torch.equal(km_after.centers.view(torch.int32), km_before.centers.view(torch.int32))
    assert torch.equal(km_after.labels, km_before.labels) and torch.equal(km_after.counts, km_before.counts)
    assert torch.equal(km_after.inertia.view(torch.int64), km_before.inertia.view(torch.int64))
    # the result is the reference's plan and counts on the kernel's distances here too
    pairs, tasks, keys, _ = R.plan(cols, feats.frame_offsets)
    dist = A.dtw_distance(feats, pairs).cpu().numpy()
    valid, scores = R.scores_from(dist, tasks)
    assert abs(res.error - (1.0 - R.average(keys[valid], scores)[0])) <= 1e-12
