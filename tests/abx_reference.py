"""numpy reference of the ABX evaluation (cpc_audio_amd.abx; include/cpc_hip.h, cpc_frame_distance / cpc_dtw / cpc_abx_count): float64
frame distances and their f32 error bounds, the DTW recurrence with its forward path length in a chosen dtype (float64 for values,
float32 for bits: one numpy.float32 addition per cell), a literal backtrack of the path, the triple count by loops, the planning of
abx_error restated on its own and the averaging.  Shared by test_abx_host.py and test_abx_gpu.py; nothing here runs the code under test.
"""
import numpy as np

U = 2.0 ** -24
ACOS_ULP = 4.0           # ulp of acosf: no accuracy statement for it was found with the device library, so 4 ulp is assumed


# ============================================================================================================ frame distances
def frame_distances(a, b, metric):
    """float64 [La, Lb] distances of the rows of a against the rows of b (float64 arrays holding the values the kernel was given)."""
    dot = a @ b.T
    na, nb = (a * a).sum(1), (b * b).sum(1)
    if metric == 2:
        return np.maximum(na[:, None] + nb[None, :] - 2.0 * dot, 0.0)
    c = np.clip(dot / np.sqrt(na[:, None] * nb[None, :]), -1.0, 1.0)
    return 1.0 - c if metric == 1 else np.arccos(c) / np.pi


def tol_sqeuclidean(a, b):
    """(D + 2) u (|a|^2 + 2 sum |a_i b_i| + |b|^2)."""
    D = a.shape[1]
    return (D + 2) * U * ((a * a).sum(1)[:, None] + 2.0 * (np.abs(a) @ np.abs(b).T) + (b * b).sum(1)[None, :])


def tol_cos(a, b):
    """(2 D + 8) u sum |a_i b_i| / (|a| |b|)."""
    D = a.shape[1]
    return (2 * D + 8) * U * (np.abs(a) @ np.abs(b).T) / np.sqrt((a * a).sum(1)[:, None] * (b * b).sum(1)[None, :])


def angular_interval(a, b):
    """[lo, hi] the angular distance must lie in: acos over cos -/+ tol_cos in float64, widened by ACOS_ULP + 1 f32 ulps of the end."""
    c = np.clip((a @ b.T) / np.sqrt((a * a).sum(1)[:, None] * (b * b).sum(1)[None, :]), -1.0, 1.0)
    t = tol_cos(a, b)
    lo = np.arccos(np.minimum(c + t, 1.0)) / np.pi
    hi = np.arccos(np.maximum(c - t, -1.0)) / np.pi
    ulp = lambda v: np.spacing(np.maximum(v, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)          # noqa: E731
    return lo - (ACOS_ULP + 1) * ulp(lo), hi + (ACOS_ULP + 1) * ulp(hi)


# ========================================================================================================================= dtw
def dtw_tables(d, dtype=np.float64):
    """C and len of the recurrence over the distance matrix d, every + one addition in ``dtype``; the predecessor of an inner cell is
    the diagonal if it is <= both others, else the left if it is <= the upper, else the upper."""
    d = np.asarray(d).astype(dtype)
    La, Lb = d.shape
    Cm, Ln = np.zeros((La, Lb), dtype), np.zeros((La, Lb), np.int64)
    for i in range(La):
        for j in range(Lb):
            if i == 0 and j == 0:
                Cm[0, 0], Ln[0, 0] = d[0, 0], 1
            elif i == 0:
                Cm[0, j], Ln[0, j] = dtype(d[0, j] + Cm[0, j - 1]), j + 1
            elif j == 0:
                Cm[i, 0], Ln[i, 0] = dtype(d[i, 0] + Cm[i - 1, 0]), i + 1
            else:
                dg, lf, up = Cm[i - 1, j - 1], Cm[i, j - 1], Cm[i - 1, j]
                if dg <= up and dg <= lf:
                    m, l = dg, Ln[i - 1, j - 1]
                elif lf <= up:
                    m, l = lf, Ln[i, j - 1]
                else:
                    m, l = up, Ln[i - 1, j]
                Cm[i, j], Ln[i, j] = dtype(d[i, j] + m), l + 1
    return Cm, Ln


def dtw_tables_by_diagonals(d, dtype=np.float64):
    """dtw_tables with the cells of an anti-diagonal computed together (the same additions and comparisons per cell; a border of
    +inf stands for the neighbours that do not exist and a 0 of length 0 for the one before the first cell).  test_abx_host.py holds
    it to the loop form."""
    d = np.asarray(d).astype(dtype)
    La, Lb = d.shape
    Cp = np.full((La + 1, Lb + 1), np.inf, dtype)
    Lp = np.zeros((La + 1, Lb + 1), np.int64)
    Cp[0, 0] = 0
    for k in range(La + Lb - 1):
        i = np.arange(max(0, k - Lb + 1), min(La - 1, k) + 1)
        j = k - i
        dg, lf, up = Cp[i, j], Cp[i + 1, j], Cp[i, j + 1]
        use_dg = (dg <= up) & (dg <= lf)
        use_lf = ~use_dg & (lf <= up)
        m = np.where(use_dg, dg, np.where(use_lf, lf, up))
        l = np.where(use_dg, Lp[i, j], np.where(use_lf, Lp[i + 1, j], Lp[i, j + 1]))
        Cp[i + 1, j + 1] = (d[i, j] + m).astype(dtype)
        Lp[i + 1, j + 1] = l + 1
    return Cp[1:, 1:], Lp[1:, 1:]


def dtw(d, dtype=np.float64):
    """(cost, path_len, dist) of the last cell; dist is the quotient in ``dtype``."""
    Cm, Ln = dtw_tables_by_diagonals(d, dtype)
    cost, n = Cm[-1, -1], int(Ln[-1, -1])
    return cost, n, dtype(cost / dtype(n))


def backtrack_length(Cm):
    """The number of cells of the path a backtrack from the last cell of the cost matrix walks (Libri-light's order: the diagonal
    first, then the left cell, then the upper one)."""
    i, j = Cm.shape[0] - 1, Cm.shape[1] - 1
    n = 1
    while i > 0 or j > 0:
        if i == 0:
            j -= 1
        elif j == 0:
            i -= 1
        else:
            dg, lf, up = Cm[i - 1, j - 1], Cm[i, j - 1], Cm[i - 1, j]
            if dg <= up and dg <= lf:
                i, j = i - 1, j - 1
            elif lf <= up:
                j -= 1
            else:
                i -= 1
        n += 1
    return n


TIE_KINDS = ("diagonal=left", "diagonal=upper", "left=upper<diagonal", "all equal")
TIE_PLACES = ("first", "row 63", "row 64", "last")
EXACT_LENGTHS = (1, 2, 63, 64, 65, 127, 128)


def tie_kinds(Cm):
    """{place: set of tie kinds} among the predecessors of the inner cells of a cost matrix: "first" = cells of row 1 or column 1 (their
    neighbours lie in the first row or column), "row 63" / "row 64" the cells either side of the stripe edge, "last" the last cell."""
    La, Lb = Cm.shape
    seen = {p: set() for p in TIE_PLACES}
    if La < 2 or Lb < 2:
        return seen
    dg, lf, up = Cm[:-1, :-1], Cm[1:, :-1], Cm[:-1, 1:]
    kinds = [(dg == lf) & (dg < up), (dg == up) & (dg < lf), (lf == up) & (lf < dg), (dg == lf) & (dg == up)]
    i, j = np.meshgrid(np.arange(1, La), np.arange(1, Lb), indexing="ij")
    places = {"first": (i == 1) | (j == 1), "row 63": i == 63, "row 64": i == 64, "last": (i == La - 1) & (j == Lb - 1)}
    for p, mask in places.items():
        for name, k in zip(TIE_KINDS, kinds):
            if (k & mask).any():
                seen[p].add(name)
    return seen


def exact_case(D, seed=0):
    """Integer rows of magnitude <= 4 and pairs over them with every length of EXACT_LENGTHS on both sides, several times.  The
    segments walk through few distinct rows, so that the squared distances take few values and the three predecessors tie often;
    test_abx_host.py asserts that every kind of tie occurs at every place.  Returns (rows f32 [N, D], pairs int64 [P, 4])."""
    rng = np.random.default_rng(seed)
    N = 1200
    palette = rng.integers(-4, 5, size=(3, D)).astype(np.float32)
    palette[1] = palette[0]
    palette[1, :2] += np.where(palette[0, :2] > 0, -1, 1)          # (a row one step away in two columns: distance 2)
    rows = palette[rng.integers(0, 3, size=N)]
    rows[N // 2:] = palette[(np.arange(N - N // 2) // 3) % 3]      # runs of three equal rows
    # two rows alternating, against the same sequence one row on: d[i][j] is large where i + j is even and 0 elsewhere, a symmetric
    # matrix with a costly diagonal, so that the left and the upper neighbour of the last cell tie below the diagonal one
    rows[N - 260:] = palette[(np.arange(260) % 2) * 2]
    pairs = [(N - 260, L, N - 259, L) for L in (3, 63, 65, 127)]
    for rep in range(3):
        for la in EXACT_LENGTHS:
            for lb in EXACT_LENGTHS:
                pairs.append((int(rng.integers(0, N - la + 1)), la, int(rng.integers(0, N - lb + 1)), lb))
    return rows, np.array(pairs, np.int64)


# ================================================================================================================== abx count
def abx_count(dist, task):
    """cpc_abx_count's value for one task by loops: -2 out of range, -1 for a NaN that is read."""
    off, nc, sp, n_p, sq, n_q = (int(v) for v in task)
    if not (2 <= n_p <= 1024 and 1 <= n_q <= 1024 and nc >= 1 and 0 <= sp and sp + n_p <= nc and 0 <= sq and sq + n_q <= nc and
            off >= 0 and off + nc * nc <= dist.shape[0]):
        return -2
    cell = dist[off:off + nc * nc].reshape(nc, nc)
    total = 0
    for x in range(n_p):
        col = cell[:, sp + x]
        for a in range(n_p):
            if a == x:
                continue
            da = col[sp + a]
            for b in range(n_q):
                db = col[sq + b]
                if np.isnan(da) or np.isnan(db):
                    return -1
                total += 2 * int(da < db) + int(da == db)
    return total


def abx_count_fast(dist, task):
    """The same value with numpy comparisons per column (for the larger groups)."""
    off, nc, sp, n_p, sq, n_q = (int(v) for v in task)
    cell = dist[off:off + nc * nc].reshape(nc, nc)
    total = 0
    for x in range(n_p):
        da = np.delete(cell[sp:sp + n_p, sp + x], x)
        db = cell[sq:sq + n_q, sp + x]
        if np.isnan(da).any() or np.isnan(db).any():
            return -1
        total += 2 * int((da[:, None] < db[None, :]).sum()) + int((da[:, None] == db[None, :]).sum())
    return total


# =================================================================================================================== planning
def plan(items, row_offsets, max_group=10, seed=0, by=("context", "speaker")):
    """abx_error's tables restated with dictionaries and loops.  items: dict of equal-length integer lists file, first, last, phone,
    context, speaker.  Returns (pairs [P, 4], tasks [T, 6], keys [T, len(by) + 2], picked item indices in table order)."""
    n = len(items["file"])
    groups = {}
    for i in range(n):
        cell = tuple(int(items[b][i]) for b in by)
        groups.setdefault(cell + (int(items["phone"][i]),), []).append(i)
    rng = np.random.default_rng(seed)
    cells = {}
    for gkey in sorted(groups):                                   # lexicographic in (cell key, phone): the order the generator is consumed
        members = groups[gkey]
        if len(members) > max_group:
            keep = np.sort(rng.choice(len(members), max_group, replace=False))
            members = [members[int(k)] for k in keep]
        cells.setdefault(gkey[:-1], []).append((gkey[-1], members))
    pairs, tasks, keys, picked, off = [], [], [], [], 0
    for ckey in sorted(cells):
        flat = [i for _, members in cells[ckey] for i in members]
        nc = len(flat)
        seg = [(int(row_offsets[items["file"][i]]) + int(items["first"][i]), int(items["last"][i]) - int(items["first"][i])) for i in flat]
        for r in range(nc):
            for c in range(nc):
                pairs.append(seg[r] + seg[c])
        picked += flat
        start, s = [], 0
        for _, members in cells[ckey]:
            start.append(s)
            s += len(members)
        for p, (phone_p, mp) in enumerate(cells[ckey]):
            for q, (phone_q, mq) in enumerate(cells[ckey]):
                if p != q and len(mp) >= 2:
                    tasks.append((off, nc, start[p], len(mp), start[q], len(mq)))
                    keys.append(ckey + (phone_p, phone_q))
        off += nc * nc
    return (np.array(pairs, np.int64).reshape(-1, 4), np.array(tasks, np.int64).reshape(-1, 6),
            np.array(keys, np.int64).reshape(-1, len(by) + 2), np.array(picked, np.int64))


def average(keys, scores):
    """Scores averaged over the last by-column within the rest, then the one before, then over the ordered (p, q); float64.
    Returns (mean, {(p, q): score})."""
    levels = len(keys[0]) - 2
    table = {tuple(int(v) for v in k): float(s) for k, s in zip(keys, scores)}
    for level in range(levels - 1, -1, -1):
        sums = {}
        for k, s in table.items():
            sums.setdefault(k[:level] + k[level + 1:], []).append(s)
        table = {k: sum(v) / len(v) for k, v in sums.items()}
    return sum(table.values()) / len(table), table


def scores_from(dist, tasks):
    """(valid mask, scores of the valid tasks) from the DTW distances, counts by numpy comparisons."""
    out = np.array([abx_count_fast(dist, t) for t in tasks], np.int64)
    valid = out >= 0
    denom = 2.0 * tasks[:, 3] * (tasks[:, 3] - 1) * tasks[:, 5]
    return valid, out[valid] / denom[valid]


# ============================================================================================================== synthetic data
D_SYN, REC_FRAMES, N_REC = 16, 300, 4


def synthetic_case(kind, seed=0):
    """A handful of recordings of REC_FRAMES frames of D_SYN columns with items cut from them.  Item segments of phone k are noisy
    copies of template k at varying lengths.
      "separated"  3 orthogonal templates, noise 0.01: every same-phone distance is far below every other-phone distance
      "tied"       phones 0 and 1 share one template, every item is the same 9 frames bit for bit: every comparison ties
      "mixed"      3 templates that overlap, noise 0.6, groups of up to 14 items: errors occur
    Returns dict(rows f32 [N, D], offsets [N_REC + 1], items {column: int64 array})."""
    rng = np.random.default_rng(seed + {"separated": 11, "tied": 22, "mixed": 33}[kind])
    n_phone, t_len = 3, 12
    basis = np.linalg.qr(rng.standard_normal((D_SYN, D_SYN)))[0]
    templates = np.zeros((n_phone, t_len, D_SYN))
    for k in range(n_phone):
        lead, side = basis[2 * k], basis[2 * k + 1]
        if kind == "mixed":
            lead = basis[0] + 0.2 * basis[k + 1]
        for t in range(t_len):
            templates[k, t] = 3.0 * lead + 0.5 * np.sin(0.5 * t) * side
    if kind == "tied":
        templates[1] = templates[0]
    noise = {"separated": 0.01, "tied": 0.0, "mixed": 0.6}[kind]
    rows = rng.standard_normal((N_REC * REC_FRAMES, D_SYN)).astype(np.float32)
    cols = {c: [] for c in ("file", "first", "last", "phone", "context", "speaker")}
    for f in range(N_REC):
        pos, i = 3, 0
        while True:
            L = 9 if kind == "tied" else int(rng.integers(5, 21))
            if pos + L > REC_FRAMES - 2:
                break
            k = i % n_phone
            seg = templates[k][(np.arange(L) * t_len) // L] + noise * rng.standard_normal((L, D_SYN))
            rows[f * REC_FRAMES + pos:f * REC_FRAMES + pos + L] = seg.astype(np.float32)
            for c, v in zip(cols, (f, pos, pos + L, k, (i // n_phone) % 2, f % 2)):
                cols[c].append(v)
            pos += L + int(rng.integers(0, 4))
            i += 1
    offsets = np.arange(N_REC + 1, dtype=np.int64) * REC_FRAMES
    return dict(rows=rows, offsets=offsets, items={c: np.array(v, np.int64) for c, v in cols.items()})


def dtw_tolerance(a, b, metric):
    """What the f32 DTW distance of a pair may differ by from the float64 one: the minimum over paths of sums moves by at most the
    largest per-path error, a path of n <= 255 cells collects n cell errors and n additions of relative error u on partial sums that
    are at most the path's sum, and the division by n leaves the largest cell bound plus 256 u times the mean distance (<= its
    maximum), plus u for the division itself."""
    if metric == 2:
        cell = tol_sqeuclidean(a, b).max()
    elif metric == 1:
        cell = tol_cos(a, b).max() + 2 * U
    else:
        lo, hi = angular_interval(a, b)          # (the f32 value and the float64 value both lie in the interval)
        cell = (hi - lo).max()
    return cell + 257 * U * frame_distances(a, b, metric).max()
