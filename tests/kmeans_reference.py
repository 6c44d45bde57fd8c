"""Float64 numpy reference of the k-means units (cpc_kmeans_assign / cpc_kmeans_update, cpc_audio_amd.clustering.KMeans): the
distances, the lowest-index argmin, the update with its empty-cluster and skipped-label rules, a Lloyd loop, the seeded init, the
error bound of the assignment and the separated data the label-equality tests run on.  Everything here takes the values the kernel
sees (f32 or bf16 rows widened, f32 centres) and computes in float64."""
import numpy as np

U24 = 2.0 ** -24


def sample_rows(n_rows, n_clusters, seed):
    """init="sample": default_rng(seed).choice(N, K, replace=False), sorted; N < K raises."""
    if n_rows < n_clusters:
        raise ValueError("fewer rows than clusters")
    return np.sort(np.random.default_rng(seed).choice(n_rows, n_clusters, replace=False)).astype(np.int64)


def distances(x, centers):
    """d64[n, k] = |c_k|^2 - 2 x_n . c_k + |x_n|^2 in float64, term by term as the kernel forms it."""
    x, c = np.asarray(x, np.float64), np.asarray(centers, np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * (x @ c.T) + (x * x).sum(1)[:, None]


def tolerance(x, centers):
    """tol_n = (D + 2) 2^-24 max_k (|c_k|^2 + 2 sum_i |x_ni c_ki| + |x_n|^2): the bound of an f32 fmaf chain of D products plus the two
    additions, for every candidate of row n."""
    x, c = np.asarray(x, np.float64), np.asarray(centers, np.float64)
    mag = (c * c).sum(1)[None, :] + 2.0 * (np.abs(x) @ np.abs(c).T) + (x * x).sum(1)[:, None]
    return (x.shape[1] + 2) * U24 * mag.max(1)


def assign(x, centers):
    """(labels, dist): the lowest index of the smallest distance (numpy's argmin takes the first), max(d, 0); a row holding a
    non-finite value gets -1 and NaN."""
    x = np.asarray(x, np.float64)
    bad = ~np.isfinite(x).all(1)
    d = distances(np.where(bad[:, None], 0.0, x), centers)
    labels = d.argmin(1).astype(np.int64)
    dist = np.maximum(d[np.arange(x.shape[0]), labels], 0.0)
    labels[bad] = -1
    dist[bad] = np.nan
    return labels, dist


def margins(x, centers):
    """second-best minus best distance per row."""
    d = np.sort(distances(x, centers), axis=1)
    return d[:, 1] - d[:, 0]


def update(x, labels, centers_old, dist=None):
    """(centers, cnorm, counts, inertia): the mean of the rows of every label; a cluster without rows keeps its old centre; labels
    outside [0, K) are skipped; inertia = the sum of dist over the rows that count."""
    x, old = np.asarray(x, np.float64), np.asarray(centers_old, np.float64)
    labels = np.asarray(labels, np.int64)
    K = old.shape[0]
    ok = (labels >= 0) & (labels < K)
    counts = np.bincount(labels[ok], minlength=K).astype(np.int64)
    sums = np.zeros_like(old)
    np.add.at(sums, labels[ok], x[ok])
    centers = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], old)
    inertia = float(np.asarray(dist, np.float64)[ok].sum()) if dist is not None else None
    return centers, (centers * centers).sum(1), counts, inertia


def lloyd(x, centers, iterations, round_centers=True):
    """``iterations`` times (assign, update).  With round_centers the centres are rounded to f32 after every update, as the device
    holds them.  Returns (centers, counts, labels of the last assignment, inertia per iteration, the centres before each assignment)."""
    c = np.asarray(centers, np.float64)
    inertia, seen = [], []
    for _ in range(iterations):
        seen.append(c.copy())
        labels, dist = assign(x, c)
        c, _, counts, s = update(x, labels, c, dist)
        if round_centers:
            c = c.astype(np.float32).astype(np.float64)
        inertia.append(s)
    return c, counts, labels, np.asarray(inertia), seen


def separated(N, D, K, seed):
    """(x f32 [N, D], init f32 [K, D]): K means from N(0, 1) per component, rows = a mean + 0.1 N(0, 1), every cluster owning at least
    one row; the initial centres are the means + 0.02 N(0, 1)."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((K, D))
    owner = np.concatenate([np.arange(K), rng.integers(0, K, size=N - K)]) if N >= K else rng.integers(0, K, size=N)
    rng.shuffle(owner)
    x = (means[owner] + 0.1 * rng.standard_normal((N, D))).astype(np.float32)
    init = (means + 0.02 * rng.standard_normal((K, D))).astype(np.float32)
    return x, init


SEPARATED_SHAPES = [(1000, 16, 3), (517, 256, 8), (1500, 48, 33), (2000, 64, 129), (4096, 512, 1024), (3000, 16, 1024)]
SEPARATED_SEEDS = (0, 1)
SEPARATED_ITERATIONS = 4


_CASES = {}


def separated_case(N, D, K, seed, iterations=SEPARATED_ITERATIONS):
    """The separated data of (N, D, K, seed) with its float64 Lloyd run, computed once and shared by the tests (read-only)."""
    key = (N, D, K, seed, iterations)
    if key not in _CASES:
        x, init = separated(N, D, K, seed)
        centers, counts, labels, inertia, seen = lloyd(x, init, iterations)
        for a in (x, init, centers, counts, labels, inertia, *seen):
            a.setflags(write=False)
        _CASES[key] = dict(x=x, init=init, centers=centers, counts=counts, labels=labels, inertia=inertia, seen=seen)
    return _CASES[key]
