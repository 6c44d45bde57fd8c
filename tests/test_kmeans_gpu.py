"""K-means units on the GPU: cpc_kmeans_assign, cpc_kmeans_update, cpc_kmeans_cnorm and cpc_kmeans_scratch_bytes against the float64
reference of tests/kmeans_reference.py, and cpc_audio_amd.clustering.KMeans on top of them.  Every output buffer is followed by
sentinels that must stay intact.

Bounds (u = 2^-24; none was obtained by running the code under test).
  Assignment.  The kernel forms v(n, k) = fma(-2, dot, cnorm[k]) with dot an f32 fmaf chain of D products (the f32-input MFMA), and
    dist = max(v + |x_n|^2, 0) with |x_n|^2 another chain of D products.  A chain of D fmaf's is within D u sum |a b| of the exact sum
    (first order), the fma and the last addition round once each, so every candidate lies within
        tol_n = (D + 2) u max_k (|c_k|^2 + 2 sum_i |x_ni c_ki| + |x_n|^2)
    of d64[n, k], the float64 value formed from the very numbers the kernel was given (rows widened, f32 centres, the f32 cnorm that
    was passed in).  The label the kernel returns compares smallest among values each within tol_n, hence d64[n, l] <= min_k d64[n, k]
    + 2 tol_n; the returned dist is within tol_n of max(d64[n, l], 0) (the clamp moves nothing apart).
  Exact data.  Integers of magnitude <= 4 in at most 512 columns: every product, partial sum and norm is an integer below 2^24, so f32
    is exact, labels must be the reference's lowest index on every row and dist must match in every bit.
  Separated data.  test_kmeans_host.py asserts in float64 that the smallest margin exceeds 4 tol_n on these very arrays (it is above
    10^4 tol_n), so the labels must equal the reference's on every row.
  Update.  Centres: 16 * 2^-23 * mean |x| per component over the cluster's rows, the bound test_feature_extraction_gpu.py derives for
    f32 partial sums over blocks of 16 (the kernel sums in f64 and rounds once, far inside).  cnorm: (D + 2) u |c|^2, an f32 chain's
    bound (the kernel: an f64 sum of exact squares, rounded once).  Inertia: N 2^-50 relative to the float64 sum of the same f32
    distances (N - 1 additions of relative error 2^-53, with a factor 8 to spare for the order).  Counts: exact.
  fit.  inertia[i + 1] <= inertia[i] + N max_n tol_n: Lloyd's steps never raise the exact objective, and each of the N distances of an
    assignment is within tol_n of its exact value.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cpc_audio_amd import _hip  # noqa: E402
from cpc_audio_amd import clustering as KM  # noqa: E402
from cpc_audio_amd import feature_extraction as FE  # noqa: E402
from cpc_audio_amd.audio_dataset import DeviceAudioDataset  # noqa: E402
import feature_extraction_reference as FR  # noqa: E402
import kmeans_reference as R  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
GUARD = 64
LL = C.c_longlong
U = 2.0 ** -24
SENT = {torch.int32: -12345, torch.float32: -7.5, torch.float64: -7.5}


def bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def guarded(n, dt):
    """n elements to be written, followed by GUARD sentinels: (whole buffer, view of the n).  The n start out as the sentinel too, so
    that an element the kernel skips shows."""
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


def host_cnorm(c):
    """|c_k|^2 rounded once to f32, as the kernels are given it."""
    return (c.astype(np.float64) ** 2).sum(1).astype(np.float32)


def run_assign(xv, centers, cnorm, want_dist=True):
    """cpc_kmeans_assign on a device view of rows; returns (labels, dist) as numpy after checking the sentinels."""
    N, D = xv.shape
    K = centers.shape[0]
    c_d, n_d = torch.tensor(centers).to(DEV), torch.tensor(cnorm).to(DEV)
    lbuf, lab = guarded(N, torch.int32)
    dbuf, dist = guarded(N, torch.float32)
    _hip.call("cpc_kmeans_assign", _hip.ptr(xv), _hip.dtype_code(xv.dtype), LL(N), D, LL(xv.stride(0) if N > 1 else D), _hip.ptr(c_d),
              _hip.ptr(n_d), K, _hip.ptr(lab), _hip.ptr(dist) if want_dist else None)
    torch.cuda.synchronize()
    assert intact(lbuf, N) and intact(dbuf, N)
    if not want_dist:
        assert bool((dist == SENT[torch.float32]).all()), "dist written although NULL was passed"
    return lab.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def d64_of(xw, centers, cnorm):
    """float64 distances from the numbers the kernel was given (the passed cnorm, not a recomputed one)."""
    c = centers.astype(np.float64)
    return cnorm.astype(np.float64)[None, :] - 2.0 * (xw @ c.T) + (xw * xw).sum(1)[:, None]


# ================================================================================================================== assignment
# a pruned product: every N, K, D, padding and dtype of the issue appears, and the large K meet the large D
RANDOM_CASES = [(1, 2, 16, 0, F32), (63, 3, 48, 16, BF16), (64, 33, 256, 0, F32), (129, 128, 512, 16, F32), (1000, 129, 16, 0, BF16),
                (1000, 1024, 48, 16, F32), (129, 1024, 512, 0, BF16), (63, 128, 256, 16, BF16), (64, 129, 48, 0, F32),
                (1, 1024, 16, 16, BF16), (1000, 2, 256, 0, F32), (129, 3, 16, 16, F32), (1000, 33, 512, 0, BF16), (1000, 64, 256, 0, F32)]


@pytest.mark.parametrize("N,K,D,pad,dt", RANDOM_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_assign_random_data_within_the_chain_bound(N, K, D, pad, dt):
    rng = np.random.default_rng(N * 7 + K * 3 + D)
    x = rng.standard_normal((N, D)).astype(np.float32)
    centers = rng.standard_normal((K, D)).astype(np.float32)
    cnorm = host_cnorm(centers)
    xv, xw = device_rows(x, dt, pad)
    labels, dist = run_assign(xv, centers, cnorm)
    assert labels.min() >= 0 and labels.max() < K
    d64 = d64_of(xw, centers, cnorm)
    tol = R.tolerance(xw, centers)
    picked = d64[np.arange(N), labels]
    over = (picked - d64.min(1)) / tol
    derr = np.abs(dist.astype(np.float64) - np.maximum(picked, 0.0)) / tol
    print(f"N={N} K={K} D={D} ld={D + pad} {dt}: label excess {over.max():.3g} of 2 tol, dist error {derr.max():.3g} tol, "
          f"{int((labels != d64.argmin(1)).sum())} rows off the float64 argmin")
    assert (over <= 2.0).all()
    assert (derr <= 1.0).all()
    # without dist: the same labels, and nothing written where dist would be
    labels2, _ = run_assign(xv, centers, cnorm, want_dist=False)
    assert (labels2 == labels).all()


def _exact_case(N, K, D, dups, seed):
    """Integer rows and centres of magnitude <= 4, centre b a copy of centre a for every (a, b) of dups (a < b), and a third of the rows
    equal to a duplicated centre, so that the tie is at the minimum."""
    rng = np.random.default_rng(seed)
    centers = rng.integers(-4, 5, size=(K, D)).astype(np.float32)
    for a, b in dups:
        centers[b] = centers[a]
    x = rng.integers(-4, 5, size=(N, D)).astype(np.float32)
    near = rng.integers(0, K, size=N)
    x[: N // 2] = centers[near[: N // 2]] + rng.integers(-1, 2, size=(N // 2, D))
    for i in range(N // 3):
        x[i] = centers[dups[i % len(dups)][1 if i % 2 else 0]]
    return np.clip(x, -4, 4), centers


# chunks of 128 centres (K = 200: tiles of 32, a chunk edge at 128) and of 64 (K = 150: chunk edges at 64 and 128); pairs inside one
# lane half, across the halves (3 | 4), across tiles (31 | 32) and across chunks
@pytest.mark.parametrize("K,dups", [(200, [(3, 4), (31, 32), (127, 128), (126, 130), (5, 199), (64, 160)]),
                                    (150, [(3, 4), (63, 64), (127, 128), (62, 66), (0, 149)]), (2, [(0, 1)])], ids=["K200", "K150", "K2"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [48, 512])
def test_assign_exact_data_and_planted_ties(K, dups, dt, D):
    N = 200
    x, centers = _exact_case(N, K, D, dups, seed=K + D)
    cnorm = host_cnorm(centers)
    xv, xw = device_rows(x, dt, 16)
    assert (xw == x).all()
    labels, dist = run_assign(xv, centers, cnorm)
    want_l, want_d = R.assign(xw, centers)
    tied = int((np.ptp(np.sort(R.distances(xw, centers), axis=1)[:, :2], axis=1) == 0).sum())
    assert tied >= N // 3, "the planted ties are not at the minimum"
    assert (labels == want_l).all()
    assert (bits(torch.from_numpy(dist)) == bits(torch.from_numpy(want_d.astype(np.float32)))).all()
    assert (want_d[: N // 3] == 0).all()


@pytest.mark.parametrize("seed", R.SEPARATED_SEEDS)
@pytest.mark.parametrize("shape", R.SEPARATED_SHAPES, ids=lambda s: "N%d-D%d-K%d" % s)
def test_assign_separated_data_equals_the_reference_on_every_row(shape, seed):
    case = R.separated_case(*shape, seed)
    xv, xw = device_rows(case["x"], F32, 0)
    labels, dist = run_assign(xv, case["init"], host_cnorm(case["init"]))
    want_l, want_d = R.assign(xw, case["init"])
    assert (labels == want_l).all()
    assert (np.abs(dist - want_d) <= R.tolerance(xw, case["init"])).all()


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_assign_non_finite_rows(dt):
    N, K, D = 300, 70, 80          # three workgroups, two passes of 32 columns and one of 16
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, D)).astype(np.float32)
    centers = rng.standard_normal((K, D)).astype(np.float32)
    cnorm = host_cnorm(centers)
    clean_l, clean_d = run_assign(device_rows(x, dt, 16)[0], centers, cnorm)
    dirty = x.copy()
    spots = {0: (0, np.nan), 31: (79, np.inf), 32: (33, -np.inf), 127: (64, np.nan), 128: (15, np.inf), 299: (79, np.nan), 200: (40, -np.inf)}
    for row, (col, val) in spots.items():
        dirty[row, col] = val
    dirty[64, :] = np.nan
    bad = sorted(list(spots) + [64])
    labels, dist = run_assign(device_rows(dirty, dt, 16)[0], centers, cnorm)
    assert (labels[bad] == -1).all() and np.isnan(dist[bad]).all()
    keep = np.ones(N, bool)
    keep[bad] = False
    assert (labels[keep] == clean_l[keep]).all()
    assert (bits(torch.from_numpy(dist[keep])) == bits(torch.from_numpy(clean_d[keep]))).all()


# ====================================================================================================================== update
def run_update(xv, labels, dist, old, in_place=False):
    """cpc_kmeans_update; returns dict of numpy outputs after checking the sentinels."""
    N, D = xv.shape
    K = old.shape[0]
    lab_d = torch.from_numpy(labels.astype(np.int32)).to(DEV)
    dist_d = torch.from_numpy(dist.astype(np.float32)).to(DEV)
    old_d = torch.from_numpy(old).to(DEV)
    need = _hip.lib().cpc_kmeans_scratch_bytes(LL(N), K, D)
    assert need > 0
    sbuf = torch.full((need + GUARD,), 0x5A, device=DEV, dtype=torch.uint8)
    cbuf, cen = guarded(K * D, torch.float32)
    if in_place:
        cen.copy_(old_d.reshape(-1))
    nbuf, cn = guarded(K, torch.float32)
    kbuf, cnt = guarded(K, torch.int32)
    ibuf, inert = guarded(1, torch.float64)
    _hip.call("cpc_kmeans_update", _hip.ptr(xv), _hip.dtype_code(xv.dtype), LL(N), D, LL(xv.stride(0) if N > 1 else D), _hip.ptr(lab_d),
              _hip.ptr(dist_d), _hip.ptr(cen) if in_place else _hip.ptr(old_d), K, _hip.ptr(sbuf), LL(need), _hip.ptr(cen), _hip.ptr(cn),
              _hip.ptr(cnt), _hip.ptr(inert))
    torch.cuda.synchronize()
    assert intact(cbuf, K * D) and intact(nbuf, K) and intact(kbuf, K) and intact(ibuf, 1)
    assert bool((sbuf[need:] == 0x5A).all()), "the scratch was overrun"
    assert torch.equal(old_d.cpu(), torch.from_numpy(old)), "the old centres were written"
    return dict(centers=cen.reshape(K, D).cpu().numpy(), cnorm=cn.cpu().numpy(), counts=cnt.cpu().numpy().astype(np.int64),
                inertia=float(inert.cpu().numpy()[0]))


def _hand_made_labels(N, K, mode, rng):
    if mode == "all-in-one":
        return np.full(N, 3, np.int64)
    labels = rng.integers(0, K, size=N)
    labels[labels == 1] = 0                      # cluster 1: empty
    labels[labels == 2] = 4
    labels[N // 2] = 2                           # cluster 2: one row
    labels[[0, 7, N - 1]] = -1                   # skipped: -1, K, far outside on both sides
    labels[[1, 8, N - 2]] = K
    labels[[2, N - 3]] = [K + 1000, -2 ** 31]
    return labels


@pytest.mark.parametrize("mode", ["mixed", "all-in-one"])
@pytest.mark.parametrize("dt,pad", [(F32, 0), (BF16, 16)], ids=["f32", "bf16-padded"])
@pytest.mark.parametrize("N,K,D", [(2501, 6, 48), (1027, 5, 512), (37, 1024, 16)])
def test_update_against_float64(N, K, D, dt, pad, mode):
    rng = np.random.default_rng(N + D)
    x = (rng.standard_normal((N, D)) + 0.5).astype(np.float32)
    old = rng.standard_normal((K, D)).astype(np.float32)
    labels = _hand_made_labels(N, K, mode, rng)
    ok = (labels >= 0) & (labels < K)
    dist = rng.random(N).astype(np.float32) * 3.0
    dist[~ok] = np.nan                           # what a skipped row carries must not reach the inertia
    xv, xw = device_rows(x, dt, pad)
    got = run_update(xv, labels, dist, old)
    want_c, want_n, want_k, want_i = R.update(xw, labels, old, np.where(ok, dist, 0.0))
    assert (got["counts"] == want_k).all()
    if mode == "mixed":
        assert want_k[1] == 0 and want_k[2] == 1
    worst_c = 0.0
    for k in range(K):
        if want_k[k] == 0:
            assert (bits(torch.from_numpy(got["centers"][k])) == bits(torch.from_numpy(old[k]))).all(), k
            continue
        bound = 16 * 2.0 ** -23 * np.abs(xw[labels == k]).mean(0)
        err = np.abs(got["centers"][k].astype(np.float64) - want_c[k])
        worst_c = max(worst_c, float((err / bound).max()))
        if want_k[k] == 1:
            assert (got["centers"][k] == xw[labels == k][0].astype(np.float32)).all()          # the mean of one row is the row
    c64 = got["centers"].astype(np.float64)
    nerr = np.abs(got["cnorm"].astype(np.float64) - (c64 * c64).sum(1)) / ((D + 2) * U * (c64 * c64).sum(1))
    ierr = abs(got["inertia"] - want_i) / (N * 2.0 ** -50 * want_i)
    print(f"N={N} K={K} D={D} {dt} {mode}: centres {worst_c:.3g}, cnorm {nerr.max():.3g}, inertia {ierr:.3g} of their bounds")
    assert worst_c <= 1.0 and (nerr <= 1.0).all() and ierr <= 1.0
    # the same bits from a second call, and from the in-place form
    again, inpl = run_update(xv, labels, dist, old), run_update(xv, labels, dist, old, in_place=True)
    for other in (again, inpl):
        assert (bits(torch.from_numpy(other["centers"])) == bits(torch.from_numpy(got["centers"]))).all()
        assert (bits(torch.from_numpy(other["cnorm"])) == bits(torch.from_numpy(got["cnorm"]))).all()
        assert (other["counts"] == got["counts"]).all()
        assert np.float64(other["inertia"]).tobytes() == np.float64(got["inertia"]).tobytes()
    # cpc_kmeans_cnorm gives the update's bits for the same centres
    cen_d = torch.from_numpy(got["centers"]).to(DEV)
    nbuf, cn = guarded(K, torch.float32)
    _hip.call("cpc_kmeans_cnorm", _hip.ptr(cen_d), _hip.ptr(cn), K, D)
    torch.cuda.synchronize()
    assert intact(nbuf, K) and (bits(cn.cpu()) == bits(torch.from_numpy(got["cnorm"]))).all()


# ========================================================================================================================= fit
def _manual(xv, init, iterations):
    """``iterations`` times (cpc_kmeans_assign, cpc_kmeans_update) by hand from the initial centres, as fit is specified."""
    N, D = xv.shape
    K = init.shape[0]
    centers = init.detach().to(DEV, F32).contiguous().clone()
    cnorm = torch.empty(K, device=DEV)
    labels, dist = torch.empty(N, device=DEV, dtype=torch.int32), torch.empty(N, device=DEV)
    counts, inertia = torch.empty(K, device=DEV, dtype=torch.int32), torch.zeros(iterations, device=DEV, dtype=torch.float64)
    need = _hip.lib().cpc_kmeans_scratch_bytes(LL(N), K, D)
    scratch = torch.empty(need, device=DEV, dtype=torch.uint8)
    code, ldx = _hip.dtype_code(xv.dtype), LL(xv.stride(0))
    _hip.call("cpc_kmeans_cnorm", _hip.ptr(centers), _hip.ptr(cnorm), K, D)
    for i in range(iterations):
        _hip.call("cpc_kmeans_assign", _hip.ptr(xv), code, LL(N), D, ldx, _hip.ptr(centers), _hip.ptr(cnorm), K, _hip.ptr(labels),
                  _hip.ptr(dist))
        _hip.call("cpc_kmeans_update", _hip.ptr(xv), code, LL(N), D, ldx, _hip.ptr(labels), _hip.ptr(dist), _hip.ptr(centers), K,
                  _hip.ptr(scratch), LL(need), _hip.ptr(centers), _hip.ptr(cnorm), _hip.ptr(counts), _hip.ptr(inertia, i))
    torch.cuda.synchronize()
    return centers, counts, labels, inertia


def _same_bits(km, centers, counts, labels, inertia):
    return (torch.equal(bits(km.centers), bits(centers)) and torch.equal(km.counts, counts) and torch.equal(km.labels, labels) and
            torch.equal(bits(km.inertia), bits(inertia)))


@pytest.mark.parametrize("dt,pad", [(F32, 16), (BF16, 0)], ids=["f32-padded", "bf16"])
def test_fit_equals_the_entry_points_by_hand_and_itself(dt, pad):
    N, D, K, its = 1500, 48, 33, 3
    case = R.separated_case(N, D, K, 0)
    xv, xw = device_rows(case["x"], dt, pad)
    init = torch.tensor(case["init"])
    state = torch.get_rng_state(), torch.cuda.get_rng_state(0)
    km = KM.KMeans(K, iterations=its, init=init).fit(xv)
    assert km.centers.dtype == F32 and km.centers.shape == (K, D) and km.labels.dtype == torch.int32 and km.labels.shape == (N,)
    assert km.inertia.dtype == torch.float64 and km.inertia.shape == (its,) and km.counts.shape == (K,)
    assert _same_bits(km, *_manual(xv, init, its))
    km2 = KM.KMeans(K, iterations=its, init=init).fit(xv)
    assert _same_bits(km2, km.centers, km.counts, km.labels, km.inertia)
    # init="sample": the rows the host reference picks, gathered as the initial centres; then the same by-hand equality
    ks = KM.KMeans(K, iterations=its, seed=4)
    rows = R.sample_rows(N, K, 4)
    start = ks._prepare(xv).centers
    assert torch.equal(start.cpu(), torch.from_numpy(xw[rows].astype(np.float32)))
    ks.fit(xv)
    assert _same_bits(ks, *_manual(xv, start, its))
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(0), state[1])


@pytest.mark.parametrize("shape", R.SEPARATED_SHAPES, ids=lambda s: "N%d-D%d-K%d" % s)
def test_fit_on_separated_data_equals_the_float64_lloyd_run(shape):
    N, D, K = shape
    case = R.separated_case(N, D, K, 0)
    xv, xw = device_rows(case["x"], F32, 0)
    km = KM.KMeans(K, iterations=R.SEPARATED_ITERATIONS, init=torch.tensor(case["init"])).fit(xv)
    torch.cuda.synchronize()
    labels, counts = km.labels.cpu().numpy().astype(np.int64), km.counts.cpu().numpy().astype(np.int64)
    assert (labels == case["labels"]).all() and (counts == case["counts"]).all()
    centers = km.centers.cpu().numpy().astype(np.float64)
    worst = 0.0
    for k in range(K):
        bound = 16 * 2.0 ** -23 * np.abs(xw[labels == k]).mean(0)
        worst = max(worst, float((np.abs(centers[k] - case["centers"][k]) / bound).max()))
    inertia = km.inertia.cpu().numpy()
    slack = N * max(float(R.tolerance(xw, c).max()) for c in case["seen"])
    print(f"{shape}: centres {worst:.3g} of the bound; inertia {inertia}, reference {case['inertia']}, slack {slack:.3g}")
    assert worst <= 1.0
    assert (np.diff(inertia) <= slack).all()


class _NoHostTraffic:
    """While active, the torch calls that copy between host and device, synchronise or allocate raise."""

    NAMES = [(torch.Tensor, n) for n in ("to", "cpu", "cuda", "item", "tolist", "numpy", "copy_", "clone", "zero_", "contiguous")] + \
            [(torch, n) for n in ("empty", "zeros", "full", "tensor", "as_tensor", "from_numpy")] + [(torch.cuda, "synchronize")]

    def __enter__(self):
        self.saved = [(o, n, getattr(o, n)) for o, n in self.NAMES]
        for o, n, _ in self.saved:
            def refuse(*a, _n=n, **kw):
                raise AssertionError(f"torch {_n} inside the k-means loop")
            setattr(o, n, refuse)

    def __exit__(self, *exc):
        for o, n, f in self.saved:
            setattr(o, n, f)


def test_fit_loop_body_makes_launches_only(monkeypatch):
    """KMeans._iterate is wrapped, not timed: inside it no torch call that copies, synchronises or allocates, and exactly one
    cpc_kmeans_assign followed by one cpc_kmeans_update."""
    case = R.separated_case(1000, 16, 3, 0)
    xv, _ = device_rows(case["x"], F32, 0)
    body, inside, names, real = KM.KMeans._iterate, [], [], _hip.call

    def spy(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)

    def wrapped(self, run, i):
        with _NoHostTraffic():
            before = len(names)
            body(self, run, i)
            inside.append(names[before:])

    monkeypatch.setattr(KM.KMeans, "_iterate", wrapped)
    monkeypatch.setattr(_hip, "call", spy)
    km = KM.KMeans(3, iterations=5).fit(xv)
    assert inside == [["cpc_kmeans_assign", "cpc_kmeans_update"]] * 5
    assert names.count("cpc_kmeans_cnorm") == 1 and names[0] == "cpc_kmeans_cnorm"
    torch.cuda.synchronize()
    assert int(km.counts.sum()) == 1000


# ================================================================================================================== end to end
def test_units_of_extracted_features_end_to_end():
    """A tiny encoder plus GRU extracted with FeatureExtractor; KMeans.fit(features, kind="c") and assign on it: the labels line up with
    frame_offsets, z works through kind="z", and a state_dict round trip reproduces assign bit for bit."""
    model = FR.model_for("gru", 32, 1).to(DEV)
    src = DeviceAudioDataset(arrays=FR.recordings(), item_length=100, device=DEV, storage="int16")
    training = model.training
    feats = FE.FeatureExtractor(model, streams=2, chunk_frames=16).extract(src)
    total = sum(FR.FRAME_COUNTS)
    assert feats.c.shape == (total, 32) and feats.z.shape == (total, FR.E_S)
    km = KM.KMeans(4, iterations=5, seed=1).fit(feats, kind="c")
    labels, dist = km.assign(feats, return_distance=True)
    torch.cuda.synchronize()
    assert labels.shape == (total,) and labels.dtype == torch.int32 and dist.shape == (total,)
    assert int(labels.min()) >= 0 and int(labels.max()) < 4 and int(km.counts.sum()) == total
    # the labels of a recording are the labels of its rows
    for i, n in enumerate(FR.FRAME_COUNTS):
        lo, hi = feats.frame_offsets[i], feats.frame_offsets[i + 1]
        assert hi - lo == n
        if n:
            assert torch.equal(km.assign(feats.recording(i, "c")), labels[lo:hi])
    d64 = R.distances(feats.c.float().double().cpu().numpy(), km.centers.double().cpu().numpy())
    tol = R.tolerance(feats.c.float().double().cpu().numpy(), km.centers.double().cpu().numpy())
    got = labels.cpu().numpy().astype(np.int64)
    assert (d64[np.arange(total), got] <= d64.min(1) + 2 * tol).all()
    kz = KM.KMeans(3, iterations=2).fit(feats, kind="z")
    assert kz.centers.shape == (3, FR.E_S) and kz.assign(feats, kind="z").shape == (total,)
    with pytest.raises(ValueError):
        km.assign(feats, kind="z")          # 64 columns against centres of 32
    # a saved codebook: on the device or from the host, the same labels and distances in every bit
    state = km.state_dict()
    assert sorted(state) == ["centers", "counts"]
    for st in (state, {k: v.cpu() for k, v in state.items()}):
        twin = KM.KMeans(4).load_state_dict(st, device=DEV)
        l2, d2 = twin.assign(feats, return_distance=True)
        assert torch.equal(l2, labels) and torch.equal(bits(d2), bits(dist)) and torch.equal(twin.counts, km.counts)
    assert model.training == training
