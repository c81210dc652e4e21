"""Helpers of the MODA / MODP scoring tests (tests/test_mod_metrics_host.py, tests/test_mod_metrics_gpu.py): an oracle
for the optimal matching that is independent of the library -- it imports neither the package nor its bindings -- and
the inputs both files share.

The definition (include/bev_mi355x.h, bev_detection_assign_f32), restated: per frame, a pair (i, j) is admissible
when the float32 distance sqrt(dx dx + dy dy) (every operation rounded by itself), widened to a double, is <=
match_dist and finite; the matching is a set of admissible pairs, each prediction and ground truth used at most
once, with the most pairs possible and among those the smallest sum of the (widened) distances.

oracle_frame pads the cost matrix to a square of side n = max(K, G) with BIG = 2 match_dist (n + 1) in every cell
that is not an admissible pair and solves the perfect-matching problem with the O(n^3) Hungarian method in float64.
A perfect matching with t admissible cells costs (n - t) BIG + sum; sum <= n match_dist < BIG / 2, so fewer BIG cells
always wins (the cardinality is maximal) and among equally many the smaller sum does.
"""
import itertools

import numpy as np

F = np.float32


def dist32(p, g):
    """[K, G] float32 distances, gt minus prediction, each operation rounded to float32."""
    with np.errstate(all="ignore"):
        ex = g[None, :, 0].astype(F) - p[:, None, 0].astype(F)
        ey = g[None, :, 1].astype(F) - p[:, None, 1].astype(F)
        sq_x, sq_y = ex * ex, ey * ey
        return np.sqrt(sq_x + sq_y)


def admissible(d32, match_dist):
    with np.errstate(all="ignore"):
        return (d32.astype(np.float64) <= np.float64(match_dist)) & np.isfinite(d32)


def hungarian(C):
    """Minimum-cost perfect matching of a square float64 matrix -> row_of_col [n] (the classical potentials form)."""
    n = len(C)
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(n + 1, np.inf), np.zeros(n + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = C[i0 - 1] - u[i0] - v[1:]
            upd = ~used[1:] & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(used[1:], np.inf, minv[1:])
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return p[1:] - 1


def padded_costs(p, g, match_dist):
    K, G = len(p), len(g)
    n = max(K, G)
    d = dist32(p, g)
    ok = admissible(d, match_dist)
    big = 2.0 * float(match_dist) * (n + 1) if match_dist > 0 else 1.0
    C = np.full((n, n), big)
    C[:K, :G][ok] = d.astype(np.float64)[ok]
    return C, ok, d


def oracle_frame(p, g, match_dist):
    """(tp, sum of the matched distances added in ascending prediction index, [(i, j), ...])."""
    K, G = len(p), len(g)
    if K == 0 or G == 0:
        return 0, 0.0, []
    C, ok, d = padded_costs(p, g, match_dist)
    row_of_col = hungarian(C)
    pairs = sorted((int(i), j) for j, i in enumerate(row_of_col) if i < K and j < G and ok[i, j])
    total = 0.0
    for i, j in pairs:
        total += float(d[i, j])
    return len(pairs), total, pairs


def oracle_batch(preds, gts, match_dist):
    """counts [B, 4] int32 (tp, fp, fn, 0) and sums [B] float64, frame by frame."""
    counts, sums = np.zeros((len(preds), 4), np.int32), np.zeros(len(preds))
    for b, (p, g) in enumerate(zip(preds, gts)):
        tp, sums[b], _ = oracle_frame(p, g, match_dist)
        counts[b, :3] = tp, len(p) - tp, len(g) - tp
    return counts, sums


def exhaustive_frame(p, g, match_dist):
    """Every set of admissible pairs with distinct rows and columns, for small frames: (most pairs, the smallest
    exactly rounded sum among those)."""
    K, G = len(p), len(g)
    if K == 0 or G == 0:
        return 0, 0.0
    d = dist32(p, g)
    ok = admissible(d, match_dist)
    best = (0, 0.0)
    for t in range(min(K, G), 0, -1):
        sums = []
        for rows in itertools.combinations(range(K), t):
            for cols in itertools.permutations(range(G), t):
                if all(ok[i, j] for i, j in zip(rows, cols)):
                    sums.append(float(np.sum([np.float64(d[i, j]) for i, j in zip(rows, cols)])))
        if sums:
            best = (t, min(sums))
            break
    return best


def sum_bound(K, G, match_dist, total):
    """How far the distance sum of a matching found in float64 may sit from the oracle's, n = min(K, G):

        n^2 2^-52 match_dist + n 2^-53 sum.

    The costs are exact doubles (widened float32 values), so only the solver's own additions and the final sum round.
    The matching is built by at most n augmentations, and its cost is the sum of the lengths of the n augmenting
    paths, each the shortest the solver could see.  A path alternates over at most n pairs, so the length the solver
    compares is put together from at most 2 n additions of costs and duals; each rounds by at most 2^-53 of its
    result, and a result here is a difference of path lengths in reduced costs, at most match_dist (one admissible
    pair's cost) where it decides between two candidates.  So a search may take a path that is longer than the best
    one by at most 2 n 2^-53 match_dist = n 2^-52 match_dist, and n searches leave the matching's cost within
    n^2 2^-52 match_dist of the optimum -- for the solver under test and for the oracle alike (the oracle's large
    constant enters every candidate of one comparison equally often once the cardinality is settled).  The final sum
    adds at most n matched distances in a double, each addition within 2^-53 of the running sum: n 2^-53 sum.  On
    inputs without near-ties both sides take the same matching and only the last term can show; exact ties (the
    lattices) give equal multisets of distances or sums that differ by rounding alone."""
    n = min(K, G)
    return n * n * 2.0 ** -52 * match_dist + n * 2.0 ** -53 * abs(total)


def mod_formulas(tp, fp, fn, dist_sum, match_dist):
    """The four numbers from totals, in percent, restated."""
    gt = tp + fn
    return {"moda": 100.0 * (1.0 - (fp + fn) / max(1, gt)),
            "modp": 100.0 * (tp - dist_sum / match_dist) / max(1, tp),
            "precision": 100.0 * tp / max(1, tp + fp), "recall": 100.0 * tp / max(1, gt),
            "tp": tp, "fp": fp, "fn": fn, "gt": gt}


def pack(preds, gts, cap=None):
    """The C entries' layout: pred [B, cap, 4], pred_count [B], gt_xy [N, 2], gt_offset [B + 1]."""
    ks = [len(p) for p in preds]
    cap = max(ks, default=0) if cap is None else cap
    pred = np.zeros((len(preds), cap, 4), F)
    for b, p in enumerate(preds):
        if ks[b]:
            pred[b, :ks[b], :p.shape[1]] = p
    xy = np.concatenate([np.asarray(g, F)[:, :2] for g in gts if len(g)] + [np.zeros((0, 2), F)])
    offset = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    return pred, np.asarray(ks, np.int32), np.ascontiguousarray(xy, dtype=F), offset


def square_frame(rng, K, G, side=1.2):
    """K predictions and G ground truths uniform on a side x side square: at threshold 0.5 nearly every pair of a
    small frame competes."""
    return rng.uniform(0, side, (K, 4)).astype(F), rng.uniform(0, side, (G, 4)).astype(F)


def crowd(seed, n_gt=40, n_near=36, n_stray=6, sigma=0.25, extent=(12.0, 4.0)):
    """The synthetic crowd: n_gt ground truths uniform on 12 x 4 m, one prediction near each of n_near of them
    (jitter sigma per axis) and n_stray anywhere, in shuffled order."""
    rng = np.random.default_rng(seed)
    g = np.zeros((n_gt, 4), F)
    g[:, 0], g[:, 1] = rng.uniform(0, extent[0], n_gt), rng.uniform(0, extent[1], n_gt)
    p = np.zeros((n_near + n_stray, 4), F)
    p[:n_near, :2] = g[rng.permutation(n_gt)[:n_near], :2] + rng.normal(0, sigma, (n_near, 2))
    p[n_near:, 0], p[n_near:, 1] = rng.uniform(0, extent[0], n_stray), rng.uniform(0, extent[1], n_stray)
    return p[rng.permutation(len(p))], g


def sparse_crowd(rng, K, G, spacing=1.0, sigma=0.2):
    """A large frame most of whose predictions have 1-3 partners within 0.5 m: ground truths near the nodes of a
    square lattice of the given spacing, predictions near ground truths drawn with repetition."""
    side = int(np.ceil(np.sqrt(max(G, 1))))
    nodes = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:G].astype(np.float64)
    g = np.zeros((G, 4), F)
    g[:, :2] = nodes * spacing + rng.normal(0, 0.15, (G, 2))
    p = np.zeros((K, 4), F)
    if G:
        p[:, :2] = g[rng.integers(0, G, K), :2] + rng.normal(0, sigma, (K, 2))
    return p, g


def lattice_frames(spacing=0.4):
    """Exact ties: predictions on a 3 x 3 lattice, ground truths on the same lattice shifted by half a cell along x,
    along both axes, and not at all."""
    xs = (np.arange(3) * spacing).astype(F)
    pts = np.zeros((9, 4), F)
    pts[:, 0], pts[:, 1] = np.repeat(xs, 3), np.tile(xs, 3)
    out = []
    for sx, sy in ((spacing / 2, 0.0), (spacing / 2, spacing / 2), (0.0, 0.0)):
        g = pts.copy()
        g[:, 0] += F(sx)
        g[:, 1] += F(sy)
        out.append((pts.copy(), g))
    return out
