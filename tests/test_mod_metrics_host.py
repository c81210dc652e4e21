"""MODA / MODP scoring, host side (no GPU): bev_detection_assign_host (csrc/bev_metrics.h, assign_solve, run by one
worker) and the additions to utils/metrics.py on CPU tensors, against an oracle that does not use the library
(tests/mod_metrics_helper.py: a float64 Hungarian on the padded square matrix).  The oracle itself is pinned three
ways -- exhaustive enumeration for every K, G <= 5, scipy's linear_sum_assignment where scipy imports, and a check
that it imports nothing of the library -- before anything is compared with it.

tp / fp / fn are compared exactly.  The distance sums are compared within mod_metrics_helper.sum_bound, whose
derivation is stated there: n^2 2^-52 match_dist + n 2^-53 sum, n = min(K, G)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import bev_native
import mod_metrics_helper as H
from conftest import GOLDEN  # noqa: F401  (puts the package on the path)
from utils.metrics import DetectionMetrics, compute_metrics, compute_mod_metrics

F = np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(bev_native.LIB_PATH):
        bev_native.build()
    return bev_native.lib()


def assert_frames_equal_oracle(preds, gts, m, what, got=None):
    """The host entry on the batch against the oracle frame by frame: counts exact, sums within the bound."""
    counts, sums = bev_native.detection_assign_host(*H.pack(preds, gts), m) if got is None else got
    want_c, want_s = H.oracle_batch(preds, gts, m)
    assert counts.dtype == np.int32 and sums.dtype == np.float64
    assert np.array_equal(counts, want_c), (what, counts.tolist(), want_c.tolist())
    for b, (p, g) in enumerate(zip(preds, gts)):
        bound = H.sum_bound(len(p), len(g), m, want_s[b])
        print(f"{what} frame {b}: K={len(p)} G={len(g)} tp={counts[b, 0]} sum={sums[b]!r} oracle={want_s[b]!r} "
              f"|d|={abs(sums[b] - want_s[b]):.3e} bound={bound:.3e}")
        assert abs(sums[b] - want_s[b]) <= bound, (what, b, sums[b], want_s[b], bound)
    return counts, sums


# ---- the oracle --------------------------------------------------------------------------------------------------
def test_oracle_equals_exhaustive_enumeration_up_to_5x5():
    rng = np.random.default_rng(0)
    seen = set()
    for K in range(6):
        for G in range(6):
            for _ in range(3):
                p, g = H.square_frame(rng, K, G)
                tp, total, pairs = H.oracle_frame(p, g, 0.5)
                want_tp, want_total = H.exhaustive_frame(p, g, 0.5)
                assert tp == want_tp, (K, G, tp, want_tp)
                assert abs(total - want_total) <= H.sum_bound(K, G, 0.5, want_total), (K, G, total, want_total)
                assert len({i for i, _ in pairs}) == len({j for _, j in pairs}) == tp
                seen.add(tp)
    assert seen >= {0, 1, 2, 3, 4}  # the square is crowded enough to match, sparse enough to miss


def test_oracle_equals_scipy_where_scipy_imports():
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        print("scipy does not import here: the oracle is pinned by the exhaustive enumeration alone")
        return
    rng = np.random.default_rng(1)
    frames = [H.square_frame(rng, K, G, side=2.0) for K, G in ((7, 9), (12, 12), (20, 15), (1, 30))]
    frames += [H.crowd(seed) for seed in range(6)] + H.lattice_frames()
    for p, g in frames:
        C, ok, _ = H.padded_costs(p, g, 0.5)
        rows, cols = linear_sum_assignment(C)
        real = [(i, j) for i, j in zip(rows, cols) if i < len(p) and j < len(g) and ok[i, j]]
        tp, total, _ = H.oracle_frame(p, g, 0.5)
        assert tp == len(real)
        assert abs(total - sum(C[i, j] for i, j in real)) <= H.sum_bound(len(p), len(g), 0.5, total)


def test_oracle_does_not_call_the_library():
    src = inspect.getsource(H)
    code = "\n".join(line for line in src.split('"""')[2::2])  # outside the docstrings
    for word in ("bev_native", "utils", "ctypes", "detection_assign", "detection_match"):
        assert word not in code, word
    imports = [line.strip() for line in src.splitlines() if line.startswith(("import ", "from "))]
    assert imports == ["import itertools", "import numpy as np"], imports


# ---- the host entry against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_small_shape_in_one_ragged_batch(lib, seed):
    """Every K, G in 0 .. 5 (K or G = 0 among them) on a 1.2 x 1.2 m square at 0.5 m: one ragged batch of 36."""
    rng = np.random.default_rng(seed)
    shapes = [(K, G) for K in range(6) for G in range(6)]
    frames = [H.square_frame(rng, K, G) for K, G in shapes]
    counts, _ = assert_frames_equal_oracle([f[0] for f in frames], [f[1] for f in frames], 0.5, f"small[{seed}]")
    assert not counts[:, 3].any() and counts[:, 0].max() >= 3
    for (K, G), c in zip(shapes, counts):
        assert c[0] + c[1] == K and c[0] + c[2] == G


def test_ragged_batches_and_padding(lib):
    """Frames of very different sizes behind one another, cap beyond every count (rows past a count are never read),
    several thresholds, a pending frame in the middle."""
    rng = np.random.default_rng(5)
    shapes = [(30, 41), (0, 7), (150, 170), (9, 0), (64, 65), (3, 90)]
    frames = [H.sparse_crowd(rng, K, G, spacing=0.7) for K, G in shapes]
    preds, gts = [f[0] for f in frames], [f[1] for f in frames]
    for m in (0.5, 0.3, 1.0):
        packed = H.pack(preds, gts, cap=160)
        for b, (K, _) in enumerate(shapes):
            packed[0][b, K:] = NAN
        counts, _ = assert_frames_equal_oracle(preds, gts, m, f"ragged[{m}]",
                                               bev_native.detection_assign_host(*packed, m))
        assert counts[2, 0] > 60
    packed[1][2] = -1
    counts, sums = bev_native.detection_assign_host(*packed, 1.0)
    assert counts[2].tolist() == [0, 0, 0, bev_native.MATCH_STATUS_PENDING] and sums[2] == 0.0
    assert counts[4, 3] == 0 and counts[4, 0] > 0


def test_two_pair_chain_where_greedy_finds_one(lib):
    p = np.asarray([[0, 0, 1, 1], [0.45, 0, 1, 1]], F)
    g = np.asarray([[0.1, 0, 1, 1], [-0.35, 0, 1, 1]], F)
    counts, sums = assert_frames_equal_oracle([p], [g], 0.5, "chain")
    assert counts.tolist() == [[2, 0, 0, 0]]
    assert abs(sums[0] - 0.7) <= 4 * 2.0 ** -24  # four float32 coordinates, each within half an ulp of its decimal
    greedy, _ = bev_native.detection_match_host(*H.pack([p], [g]), 0.5)
    assert greedy.tolist() == [[1, 1, 1, 0]]


def test_cardinality_wins_over_a_smaller_sum(lib):
    """p1 - g0 is 0.02 apart, but taking it leaves p0 (whose only partner is g0) unmatched: the matching is
    p0 - g0 (0.28) and p1 - g1 (0.45)."""
    p = np.asarray([[0, 0, 1, 1], [0.3, 0, 1, 1]], F)
    g = np.asarray([[0.28, 0, 1, 1], [0.75, 0, 1, 1]], F)
    counts, sums = assert_frames_equal_oracle([p], [g], 0.5, "cardinality")
    assert counts.tolist() == [[2, 0, 0, 0]] and abs(sums[0] - 0.73) < 1e-6
    # the same with the roles of the two sides exchanged, and with the cheap pair first in index order
    counts, sums = assert_frames_equal_oracle([g[::-1].copy()], [p[::-1].copy()], 0.5, "cardinality-T")
    assert counts.tolist() == [[2, 0, 0, 0]] and abs(sums[0] - 0.73) < 1e-6


def test_exact_ties_on_a_lattice(lib):
    """3 x 3 lattices at spacing 0.4: many optimal matchings tie exactly; tp and the sum are the oracle's whichever
    of them either side takes."""
    frames = H.lattice_frames()
    for m in (0.5, 0.3, 0.21):
        counts, _ = assert_frames_equal_oracle([f[0] for f in frames], [f[1] for f in frames], m, f"lattice[{m}]")
        assert counts[:, 0].tolist() == ([9, 9, 9] if m >= 0.3 else [9, 0, 9])


@pytest.mark.parametrize("m", [0.5, 0.3, 0.7])
def test_pair_at_the_threshold_is_admitted_and_the_next_float_refused(lib, m):
    thr = F(bev_native.match_thr32(m))
    above = np.nextafter(thr, F(np.inf))
    assert float(thr) <= m < float(above)
    p = np.zeros((1, 4), F)
    for d, tp in ((thr, 1), (above, 0)):
        g = np.asarray([[d, 0, 1, 1]], F)
        counts, sums = assert_frames_equal_oracle([p], [g], m, f"edge[{m}, {d!r}]")
        assert counts.tolist() == [[tp, 1 - tp, 1 - tp, 0]] and sums[0] == (float(d) if tp else 0.0)
    if m == 0.5:  # a pair at exactly the threshold adds nothing to MODP
        got = compute_mod_metrics([torch.zeros(1, 4)], [{"boxes_world": torch.tensor([[0.5, 0, 1, 1]])}], 0.5)
        assert got["tp"] == 1 and got["modp"] == 0.0 and got["moda"] == 100.0


def test_non_finite_coordinates_never_match_and_leave_the_rest_alone(lib):
    rng = np.random.default_rng(9)
    p, g = H.crowd(3)
    clean_c, clean_s = bev_native.detection_assign_host(*H.pack([p], [g]), 0.5)
    bad_p = np.asarray([[NAN, 1, 1, 1], [2, INF, 1, 1], [-INF, NAN, 1, 1]], F)
    bad_g = np.asarray([[INF, 1, 1, 1], [3, NAN, 1, 1]], F)
    for trial in range(4):  # the poisoned rows at random places
        ip = np.sort(rng.choice(len(p) + 1, len(bad_p)))
        ig = np.sort(rng.choice(len(g) + 1, len(bad_g)))
        p2, g2 = np.insert(p, ip, bad_p, axis=0), np.insert(g, ig, bad_g, axis=0)
        counts, sums = assert_frames_equal_oracle([p2], [g2], 0.5, f"nonfinite[{trial}]")
        assert counts[0].tolist() == [clean_c[0, 0], clean_c[0, 1] + 3, clean_c[0, 2] + 2, 0]
        assert sums[0].view(np.uint64) == clean_s[0].view(np.uint64)
    # an infinite threshold admits every finite distance and still no infinite or NaN one
    counts, _ = bev_native.detection_assign_host(*H.pack([p2], [g2]), INF)
    tp = min(len(p), len(g))
    assert counts[0].tolist() == [tp, len(p2) - tp, len(g2) - tp, 0]


def test_six_crowds_optimal_beats_greedy_and_mod_numbers_follow_the_formulas(lib):
    better = 0
    for seed in range(6):
        p, g = H.crowd(seed)
        counts, sums = assert_frames_equal_oracle([p], [g], 0.5, f"crowd[{seed}]")
        greedy, _ = bev_native.detection_match_host(*H.pack([p], [g]), 0.5)
        print(f"crowd[{seed}]: greedy tp {greedy[0, 0]}, optimal tp {counts[0, 0]}")
        assert counts[0, 0] >= greedy[0, 0]
        better += counts[0, 0] > greedy[0, 0]
        tp, total, _ = H.oracle_frame(p, g, 0.5)
        want = H.mod_formulas(tp, len(p) - tp, len(g) - tp, total, 0.5)
        got = compute_mod_metrics([torch.from_numpy(p)], [{"boxes_world": torch.from_numpy(g)}], match_dist=0.5)
        assert sorted(got) == sorted(want)
        for k in ("tp", "fp", "fn", "gt"):
            assert got[k] == want[k] and type(got[k]) is int
        for k in ("moda", "precision", "recall"):  # from integers alone: the same double
            assert got[k] == want[k] and type(got[k]) is float
        # MODP = 100 (tp - sum / m) / tp: the sum's bound, scaled
        assert abs(got["modp"] - want["modp"]) <= 100.0 * H.sum_bound(len(p), len(g), 0.5, total) / (0.5 * tp) + 1e-13
        assert 0.0 < got["modp"] < 100.0 and got["moda"] < got["recall"]
    assert better >= 1


# ---- the Python surface --------------------------------------------------------------------------------------------
def _batches():
    rng = np.random.default_rng(21)
    out = []
    for shapes in ([(12, 15), (0, 4)], [(36, 40)], [(5, 0), (8, 8), (20, 11)]):
        frames = [H.sparse_crowd(rng, K, G, spacing=0.6) for K, G in shapes]
        preds = [torch.from_numpy(f[0]) if len(f[0]) else None for f in frames]
        gts = [{"boxes_world": torch.from_numpy(f[1])} if len(f[1]) else {} for f in frames]
        out.append((frames, preds, gts))
    return out


def test_optimal_instance_totals_equal_the_host_entry_per_frame(lib):
    val = DetectionMetrics(match_dist=0.5, matching="optimal")
    tp = fp = fn = 0
    total = 0.0
    per_batch = []
    for frames, preds, gts in _batches():
        assert val.update(preds, gts) is None
        bt = [0, 0, 0, 0.0]
        for p, g in frames:
            c, s = bev_native.detection_assign_host(*H.pack([p], [g]), 0.5)
            bt = [bt[0] + int(c[0, 0]), bt[1] + int(c[0, 1]), bt[2] + int(c[0, 2]), bt[3] + float(s[0])]
        per_batch.append(bt)
        tp, fp, fn, total = tp + bt[0], fp + bt[1], fn + bt[2], total + bt[3]
    got = val.result_mod()
    assert got == H.mod_formulas(tp, fp, fn, total, 0.5) and got["tp"] > 30 and val.in_flight() == 0
    assert val.result_mod() == got  # does not consume
    # result() keeps its 7-tuple: the per-batch means, from the optimal matching's totals
    res = val.result()
    assert len(res) == 7 and res[4:] == (tp, fp, fn)
    assert res[0] == sum(b[0] / max(1, b[0] + b[1]) for b in per_batch) / 3
    assert res[3] == sum(b[3] / max(1, b[0]) for b in per_batch) / 3
    # compute_mod_metrics of one batch: that batch's totals
    frames, preds, gts = _batches()[2]
    assert compute_mod_metrics(preds, gts) == H.mod_formulas(*per_batch[2], 0.5)
    val.reset()
    assert val.result_mod() == H.mod_formulas(0, 0, 0, 0.0, 0.5) and val.result_mod()["moda"] == 100.0


def test_matching_names(lib):
    with pytest.raises(ValueError):
        DetectionMetrics(0.5, matching="hungarian")
    with pytest.raises(ValueError):
        DetectionMetrics(0.5, matching=None)
    for val in (DetectionMetrics(0.5), DetectionMetrics(0.5, matching="greedy")):
        with pytest.raises(ValueError):
            val.result_mod()
    assert DetectionMetrics(0.5, matching="optimal").matching == "optimal" and DetectionMetrics().matching == "greedy"


def test_default_instance_result_is_bit_for_bit_the_existing_path(lib):
    """The same inputs through compute_metrics (train.py:78, batch by batch, the means of train.py:299-309 taken
    here) and through default-constructed instances."""
    want = [compute_metrics(preds, gts, 0.5) for _, preds, gts in _batches()]
    means = tuple(sum(w[k] for w in want) / len(want) for k in range(4))
    sums = tuple(sum(w[k] for w in want) for k in (4, 5, 6))
    for val in (DetectionMetrics(), DetectionMetrics(0.5), DetectionMetrics(match_dist=0.5, matching="greedy")):
        for _, preds, gts in _batches():
            val.update(preds, gts)
        got = val.result()
        assert got[4:] == sums and sums[0] > 30
        assert [np.float64(v).view(np.uint64) for v in got[:4]] == [np.float64(v).view(np.uint64) for v in means]
    # and the greedy walk on these batches is not the optimal matching: the two instances differ
    opt = DetectionMetrics(0.5, matching="optimal")
    for _, preds, gts in _batches():
        opt.update(preds, gts)
    assert opt.result()[4] >= sums[0]


def _assign_args(null=(), host=False, **kw):
    a = dict(B=2, cap=3, N=4, thr32=0.5, workspace_bytes=0)
    offsets = kw.pop("offsets", [0, 3, 4])
    a.update(kw)
    bufs = dict(pred=np.zeros((2, 3, 4), F), pred_count=np.asarray([3, 1], np.int32), gt_xy=np.zeros((4, 2), F),
                gt_offset=np.asarray(offsets, np.int32), counts=np.full((2, 4), 7, np.int32),
                dist_sum=np.full(2, 7.0))
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in bufs.items()}
    args = [p["pred"], p["pred_count"], a["B"], a["cap"], p["gt_xy"], p["gt_offset"], a["N"], a["thr32"], p["counts"],
            p["dist_sum"]]
    if not host:
        args += [None, a["workspace_bytes"], None]
    return args, bufs


def test_argument_rules_without_a_gpu(lib):
    assert lib.bev_detection_assign_workspace_bytes(2, 1024, 2048) == 0
    assert lib.bev_detection_assign_max_frame() == bev_native.detection_assign_max_frame() >= 1024
    assert bev_native.MATCH_STATUS_TOO_LARGE == -3
    for entry, host in ((lib.bev_detection_assign_f32, False), (lib.bev_detection_assign_host, True)):
        refused = [dict(null=(k,)) for k in ("pred", "pred_count", "gt_xy", "gt_offset", "counts", "dist_sum")]
        refused += [dict(B=-1), dict(cap=-1), dict(N=-1)]
        if host:
            refused += [dict(offsets=o) for o in ([0, 3, 2], [-1, 3, 4], [0, 3, 5], [3, 1, 4])]
        else:
            refused += [dict(workspace_bytes=-1)]
        for kw in refused:
            a, bufs = _assign_args(host=host, **kw)
            assert entry(*a) == bev_native.BEV_ERR_ARGS == -1, (host, kw)
            assert (bufs["counts"] == 7).all() and (bufs["dist_sum"] == 7).all(), (host, kw)  # nothing written
        a, _ = _assign_args(host=host, B=0, null=("pred", "pred_count", "gt_xy", "gt_offset", "counts", "dist_sum"))
        assert entry(*a) == 0  # B == 0: nothing to do
    a, bufs = _assign_args(host=True, cap=0, null=("pred",))
    assert lib.bev_detection_assign_host(*a) == 0 and bufs["counts"].tolist() == [[0, 0, 3, 0], [0, 0, 1, 0]]
    a, bufs = _assign_args(host=True, N=0, null=("gt_xy",), offsets=[0, 0, 0])
    assert lib.bev_detection_assign_host(*a) == 0 and bufs["counts"].tolist() == [[0, 3, 0, 0], [0, 1, 0, 0]]
    assert not bufs["dist_sum"].any()
    a, bufs = _assign_args(host=True)  # all-zero coordinates: everything at distance 0, min(K, G) pairs
    assert lib.bev_detection_assign_host(*a) == 0 and bufs["counts"].tolist() == [[3, 0, 0, 0], [1, 0, 0, 0]]


def test_bindings_and_abi(lib):
    assert lib.bev_abi_version() == bev_native.ABI_VERSION == 18
    for name in ("bev_detection_assign_f32", "bev_detection_assign_host", "bev_detection_assign_workspace_bytes",
                 "bev_detection_assign_max_frame"):
        assert name in bev_native.SIGNATURES and hasattr(lib, name)
    with pytest.raises(ValueError):
        bev_native.detection_assign_host(np.zeros((1, 2, 3), F), np.zeros(1, np.int32), np.zeros((0, 2), F),
                                         np.zeros(2, np.int32), 0.5)
    with pytest.raises(ValueError):
        bev_native.detection_assign_host(np.zeros((1, 2, 4), F), np.zeros(1, np.int32), np.zeros((2, 2), F),
                                         np.asarray([0, 3], np.int32), 0.5)  # offsets past N
    with pytest.raises(bev_native.HipError):  # no CPU fallback behind the device entry
        bev_native.detection_assign(torch.zeros(1, 2, 4), torch.zeros(1, dtype=torch.int32), torch.zeros(0, 2),
                                    torch.zeros(2, dtype=torch.int32), 0.5)
    with pytest.raises(ValueError):
        compute_mod_metrics([torch.zeros(1, 4)], [{}, {}])


def test_host_entry_takes_frames_beyond_the_device_limit(lib):
    """1100 x 1300, sparse: solved on the host (the oracle's O(n^3) is out of reach at this size; what is checked is
    what any optimal matching satisfies: complete counts, no fewer pairs than the greedy walk, every matched distance
    within the threshold)."""
    rng = np.random.default_rng(13)
    p, g = H.sparse_crowd(rng, 1100, 1300, spacing=1.0)
    counts, sums = bev_native.detection_assign_host(*H.pack([p], [g]), 0.5)
    greedy, _ = bev_native.detection_match_host(*H.pack([p], [g]), 0.5)
    assert counts[0, 3] == 0 and counts[0, 0] >= greedy[0, 0] > 500
    assert counts[0, 0] + counts[0, 1] == 1100 and counts[0, 0] + counts[0, 2] == 1300
    assert 0.0 < sums[0] <= 0.5 * counts[0, 0]
