"""Device decode (bev_decode.hip) at the edges of its value domain and of its code paths, against a plain
torch-CPU / numpy fp32 restatement of the reference decode (detector.py:64-125).

`decode_reference` is licensed by `test_decode_reference_matches_committed_fixtures` (CPU): it reproduces both
committed fixtures -- the reference's own outputs -- bit for bit.  Every GPU case then compares
BEVDetector.decode with it: equal counts, bit-identical boxes and scores, same order.  Each case's
preconditions (candidate counts, kept counts, which scores are zero / infinite, the suppression witness
beyond the LDS cache) are asserted from the reference alone.

Cases: signed-zero scores (a negative threshold makes every non-peak cell a candidate of score v * 0.0 = +-0;
torch.argsort treats -0 == +0, so cell order decides), +Inf / NaN / -Inf cells and NaN offsets / sizes, the
candidate counts at which the decode changes path (8191 .. 8193: LDS sort / global sort; 16384: no padding
keys; 16385: the first size with two global compare-exchange steps), and a frame that keeps more boxes than
the large NMS caches in LDS (8192), so that kept centres are read back from global memory.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

DEV = "cuda:0"


def decode_reference(heat, offset, size, bounds, thr, nms):
    """detector.py:64-125 on the CPU, fp32, op by op: peak = max_pool2d(x, 3, 1, 1); x * (x == peak).float();
    `> thr`; candidates in row-major order (torch.where); cx = x_min + (xs.float() + off_x) * res_x (res in
    Python double, fp32 tensor ops), w = size_x * res_x; torch.argsort(descending) made stable (equal scores
    keep cell order -- the order the `levels` fixture pins); greedy loop: a candidate is kept when no kept
    centre is at fp32 distance sqrt(dx*dx + dy*dy) < nms.
    -> (boxes [n,4] per frame, scores [n] per frame, info per frame: ncand, kept, first_sup), first_sup[i]
    being the kept-list position of the first kept box that suppressed sorted candidate i (-1: kept)."""
    heat_t, off_t, size_t = (torch.from_numpy(np.ascontiguousarray(a, np.float32)) for a in (heat, offset, size))
    B, _, H, W = heat_t.shape
    peak = F.max_pool2d(heat_t, kernel_size=3, stride=1, padding=1)
    peaks = heat_t * (heat_t == peak).float()
    off_t, size_t = off_t.permute(0, 2, 3, 1), size_t.permute(0, 2, 3, 1)
    x_min, x_max, y_min, y_max = bounds
    res_x, res_y = (x_max - x_min) / float(W), (y_max - y_min) / float(H)
    boxes_out, scores_out, info = [], [], []
    for b in range(B):
        hm = peaks[b, 0]
        mask = hm > thr
        ys, xs = torch.where(mask)
        scores = hm[mask]
        offs, sizes = off_t[b, ys, xs], size_t[b, ys, xs]
        cx = x_min + (xs.float() + offs[:, 0]) * res_x
        cy = y_min + (ys.float() + offs[:, 1]) * res_y
        boxes = torch.stack([cx, cy, sizes[:, 0] * res_x, sizes[:, 1] * res_y], dim=1).numpy()
        scores = scores.numpy()
        K = boxes.shape[0]
        order = torch.argsort(torch.from_numpy(scores), descending=True, stable=True).numpy()
        kx, ky = np.empty(K, np.float32), np.empty(K, np.float32)
        keep, first_sup, n = [], np.full(K, -1, np.int64), 0
        for pos, i in enumerate(order):
            dx, dy = kx[:n] - boxes[i, 0], ky[:n] - boxes[i, 1]
            close = np.sqrt(dx * dx + dy * dy).astype(np.float64) < nms  # torch.norm(...).item() < nms_dist_m
            if close.any():
                first_sup[pos] = int(np.argmax(close))
                continue
            kx[n], ky[n] = boxes[i, 0], boxes[i, 1]
            keep.append(int(i))
            n += 1
        boxes_out.append(boxes[keep].reshape(-1, 4))
        scores_out.append(scores[keep])
        info.append({"ncand": K, "kept": n, "first_sup": first_sup})
    return boxes_out, scores_out, info


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_decode_reference_matches_committed_fixtures():
    """decode_reference == the reference's own decode, bit for bit, on every committed decode fixture:
    decode_cases.npz (three threshold / NMS settings, B = 2, plateaus, close peaks) and decode_large.npz
    ('noise': 38443 distinct-score candidates and a blob frame; 'levels': 11041 candidates with equal scores
    everywhere, stable order).  CPU only; this is what licenses the reference for the inputs below."""
    from test_decode_gpu import _decode_large_inputs
    d = np.load(os.path.join(GOLDEN, "decode_cases.npz"))
    bounds = tuple(float(x) for x in d["bounds"])
    for thr, nms in ((0.3, 0.5), (0.5, 1.5), (0.95, 0.5)):
        bl, sl, info = decode_reference(d["heat"], d["offset"], d["size"], bounds, thr, nms)
        tag = f"t{int(thr * 100)}_n{int(nms * 10)}"
        assert [x.shape[0] for x in bl] == [int(x) for x in d[tag + "_n"]], tag
        assert np.array_equal(_bits(np.concatenate(bl)), _bits(d[tag + "_boxes"])), tag
        assert np.array_equal(_bits(np.concatenate(sl)), _bits(d[tag + "_scores"])), tag
    d = np.load(os.path.join(GOLDEN, "decode_large.npz"))
    for case, thr, nms in (("noise", 0.05, 2.0), ("levels", 0.1, 1.0)):
        heat, offset, size = _decode_large_inputs(case)
        bl, sl, info = decode_reference(heat, offset, size, (-24.0, 24.0, -7.2, 7.2), thr, nms)
        assert [i["ncand"] for i in info] == [int(x) for x in d[case + "_ncand"]], case
        assert [x.shape[0] for x in bl] == [int(x) for x in d[case + "_n"]], case
        assert np.array_equal(_bits(np.concatenate(bl)), _bits(d[case + "_boxes"])), case
        assert np.array_equal(_bits(np.concatenate(sl)), _bits(d[case + "_scores"])), case


def _run(heat, offset, size, bounds, thr, nms, lazy=False):
    from models.heads.detector import BEVDetector
    H, W = heat.shape[2:]
    det = BEVDetector(in_channels=4, bev_bounds=bounds, bev_size=(H, W)).to(DEV)
    bl, sl = det.decode(torch.from_numpy(heat).to(DEV), torch.from_numpy(offset).to(DEV),
                        torch.from_numpy(size).to(DEV), conf_thresh=thr, nms_dist_m=nms, lazy=lazy)
    return [b.cpu().numpy().reshape(-1, 4) for b in bl], [s.cpu().numpy() for s in sl]


def _assert_same(got, ref, what):
    (gb, gs), (rb, rs) = got, ref
    assert [x.shape[0] for x in gb] == [x.shape[0] for x in rb], what
    for f, (b, s, b0, s0) in enumerate(zip(gb, gs, rb, rs)):
        ds, db = _bits(s) != _bits(s0), (_bits(b) != _bits(b0)).any(axis=1)
        first = int(np.argmax(ds | db)) if (ds | db).any() else -1
        assert not ds.any(), (what, "scores", f, int(ds.sum()), first, s[first:first + 4], s0[first:first + 4])
        assert not db.any(), (what, "boxes", f, int(db.sum()), first)


def _offsets_sizes(rng, B, H, W):
    offset = rng.random((B, 2, H, W), dtype=np.float32)
    size = (rng.random((B, 2, H, W), dtype=np.float32) * np.float32(25.0) + np.float32(5.0)).astype(np.float32)
    return offset, size


# ---- 1. signed zeros -------------------------------------------------------------------------------------------
def _signed_zero_inputs(case):
    H, W = 24, 40
    rng = np.random.default_rng(301)
    if case == "randn":
        # both signs: a non-peak cell scores v * 0.0 = -0.0 (v < 0) or +0.0 (v > 0)
        heat = rng.standard_normal((1, 1, H, W), dtype=np.float32)
    else:
        # exact -0.0 / +0.0 PEAKS (isolated, every neighbour negative: score = v * 1.0 keeps the zero's own
        # sign) next to positive peaks; every other cell is a non-peak of score -0.0
        heat = (-np.float32(0.25) - rng.random((1, 1, H, W), dtype=np.float32)).astype(np.float32)
        sites = [(y, x) for y in range(1, H - 1, 3) for x in range(1, W - 1, 3)]
        vals = np.array([-0.0, 0.0, 0.5, 0.0, -0.0, 0.75], np.float32)
        for k, (y, x) in enumerate(sites):
            heat[0, 0, y, x] = vals[(k * 5 + k // 7) % 6]
    offset, size = _offsets_sizes(rng, 1, H, W)
    return heat, offset, size


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["randn", "zero_peaks"])
def test_decode_signed_zero_scores_keep_cell_order(case):
    """conf_thresh = -1: every non-peak cell is a candidate of score v * 0.0, -0.0 where v < 0 and +0.0 where
    v > 0.  The reference's argsort compares them equal, so zeros of both signs stay in cell order behind the
    positive peaks and before the negative ones, and each kept score carries its own sign bit.  1 m cells,
    offsets in [0, 1), nms 0.25 m: most zero-score cells survive the NMS."""
    heat, offset, size = _signed_zero_inputs(case)
    bounds = (-20.0, 20.0, -12.0, 12.0)
    ref = decode_reference(heat, offset, size, bounds, -1.0, 0.25)
    s0 = ref[1][0]
    neg0 = (_bits(s0) == 0x80000000).sum()
    pos0 = (_bits(s0) == 0).sum()
    assert neg0 > 20 and pos0 > 20 and (s0 > 0).sum() >= 20, (neg0, pos0)
    # the reference itself interleaves the two zeros: some -0.0 is kept before a +0.0 and the other way round
    z = _bits(s0)[s0 == 0]
    assert (np.diff((z >> 31).astype(np.int64)) == 1).any() and (np.diff((z >> 31).astype(np.int64)) == -1).any()
    if case == "randn":
        assert (s0 < 0).any()  # negative peaks above the threshold sort last
    _assert_same(_run(heat, offset, size, bounds, -1.0, 0.25), ref[:2], case)


# ---- 2. special scores -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.3, -1.0])
def test_decode_non_finite_cells(thr):
    """+Inf peaks are kept and sort first (two of them: cell order); a NaN cell and its eight neighbours are no
    candidates (max_pool2d propagates NaN, x == NaN is false, NaN > thr is false); a -Inf cell scores
    -Inf * 0 = NaN or -Inf; the neighbours of a +Inf cell score v * 0.0.  A NaN offset at a candidate makes
    every distance to it NaN: it is kept, suppresses nothing, and its box holds the NaN; a NaN size only
    travels into the box."""
    H, W = 24, 40
    rng = np.random.default_rng(302)
    heat = rng.random((1, 1, H, W), dtype=np.float32)
    heat[0, 0, 3, 5] = heat[0, 0, 17, 30] = np.inf
    heat[0, 0, 10, 10] = heat[0, 0, 0, 39] = np.nan
    heat[0, 0, 20, 4] = heat[0, 0, 20, 5] = heat[0, 0, 6, 33] = -np.inf
    for y, x in ((12, 20), (12, 23), (5, 15)):  # three certain peaks
        heat[0, 0, y, x] = 2.0 + x
    offset, size = _offsets_sizes(rng, 1, H, W)
    offset[0, 0, 12, 20] = np.nan  # next to the peak at (12, 23): 3 cells away, inside nms
    size[0, 1, 5, 15] = np.nan
    size[0, 0, 3, 5] = np.inf
    bounds = (-20.0, 20.0, -12.0, 12.0)
    nms = 4.0
    rb, rs, info = decode_reference(heat, offset, size, bounds, thr, nms)
    b0, s0 = rb[0], rs[0]
    assert np.isinf(s0[:2]).all() and (s0[:2] > 0).all() and b0[0, 0] < b0[1, 0] and np.isfinite(s0[2:]).all()
    assert np.isinf(b0[0, 2])
    assert not np.isnan(s0).any()
    nan_cx = np.isnan(b0[:, 0])
    assert nan_cx.sum() == 1 and s0[nan_cx][0] == 22.0 and (s0 == 25.0).sum() == 1  # neither suppressed the other
    assert (np.isnan(b0[:, 3]) & (s0 == 17.0)).sum() == 1
    # no kept box sits in a NaN cell (offsets < 1: a centre's cell is the floor of its coordinates), nor, above a
    # positive threshold, in its 3x3 window (below a negative one the neighbours are candidates of score v * 0.0)
    cxc, cyc = np.floor(b0[:, 0] + 20.0), np.floor(b0[:, 1] + 12.0)
    r = 1 if thr > 0 else 0
    for y, x in ((10, 10), (0, 39)):
        assert not ((np.abs(cxc - x) <= r) & (np.abs(cyc - y) <= r)).any()
    assert (info[0]["first_sup"] >= 0).any()
    _assert_same(_run(heat, offset, size, bounds, thr, nms), (rb, rs), thr)


@pytest.mark.gpu
@pytest.mark.parametrize("nms,kept", [(0.7, 1), (0.3, 2)])
def test_decode_distance_equal_to_the_rounded_nms_radius(nms, kept):
    """The reference compares `torch.norm(...).item()`, a Python double holding the fp32 distance, with the double
    nms_dist_m.  Two equal neighbouring cells (a plateau: both are peaks, cell order) whose centres are exactly
    f32(nms) apart: f32(0.7) = 0.69999999 < 0.7 suppresses the second, f32(0.3) = 0.30000001 < 0.3 does not --
    comparing against nms rounded to fp32 would keep both."""
    H, W = 8, 8
    bounds = (0.0, 8.0, 0.0, 8.0)  # 1 m cells from the origin: cx = x + off_x exactly
    heat = np.zeros((1, 1, H, W), np.float32)
    heat[0, 0, 3, 0:2] = 0.75
    offset = np.zeros((1, 2, H, W), np.float32)
    offset[0, 0, 3, 0] = np.float32(1.0) - np.float32(nms)  # cell (3, 0): cx = 1 - f32(nms); cell (3, 1): cx = 1
    assert np.float32(1.0) - offset[0, 0, 3, 0] == np.float32(nms) and float(np.float32(nms)) != nms
    size = np.ones((1, 2, H, W), np.float32)
    rb, rs, info = decode_reference(heat, offset, size, bounds, 0.5, nms)
    assert info[0]["ncand"] == 2 and info[0]["kept"] == kept
    _assert_same(_run(heat, offset, size, bounds, 0.5, nms), (rb, rs), nms)


# ---- 3. capacity edges -----------------------------------------------------------------------------------------
H_CAP, W_CAP = 258, 256
BOUNDS_CAP = (-128.0, 128.0, -129.0, 129.0)  # 1 m cells
_CAP_CACHE = {}


def _capacity_frame(K, seed):
    """K isolated peaks at even (y, x) of a 258 x 256 map (129 * 128 = 16512 sites), distinct scores in
    (0.5, 1), zeros elsewhere."""
    rng = np.random.default_rng(seed)
    n_sites = (H_CAP // 2) * (W_CAP // 2)
    sites = rng.permutation(n_sites)[:K]
    rank = rng.permutation(n_sites)[:K].astype(np.float64)
    heat = np.zeros((H_CAP, W_CAP), np.float32)
    heat[2 * (sites // (W_CAP // 2)), 2 * (sites % (W_CAP // 2))] = (0.5 + (rank + 0.5) / (2.0 * n_sites)).astype(
        np.float32)
    return heat


def _capacity_case(Ks):
    if Ks not in _CAP_CACHE:
        heat = np.stack([_capacity_frame(K, 310 + i) for i, K in enumerate(Ks)])[:, None]
        offset, size = _offsets_sizes(np.random.default_rng(320), len(Ks), H_CAP, W_CAP)
        ref = decode_reference(heat, offset, size, BOUNDS_CAP, 0.25, 1.5)
        _CAP_CACHE[Ks] = (heat, offset, size, ref)
    return _CAP_CACHE[Ks]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8191, 8192, 8193, 16384, 16385])
def test_decode_candidate_count_at_path_edges(K):
    """Exactly K candidates in one frame: 8191 / 8192 (the last sizes of the LDS sort, the second without a
    padding key), 8193 (the first of the global sort), 16384 (P = K: no padding keys there either), 16385 (P =
    32768: the first size whose top stage takes two global compare-exchange steps).  Peaks two cells apart with
    offsets in [0, 1) and nms 1.5 m: the NMS both keeps and suppresses thousands."""
    import bev_native as nat
    heat, offset, size, (rb, rs, info) = _capacity_case((K,))
    cap = nat.lib().bev_decode_max_candidates()
    assert info[0]["ncand"] == K and len(np.unique(_bits(heat[heat > 0]))) == K
    assert cap == 8192 and K - cap in (-1, 0, 1, cap, cap + 1)
    assert info[0]["kept"] > 1000 and K - info[0]["kept"] > 500, info[0]["kept"]
    _assert_same(_run(heat, offset, size, BOUNDS_CAP, 0.25, 1.5), (rb, rs), K)


@pytest.mark.gpu
def test_decode_batch_mixing_paths_lazy():
    """One batch whose frames take different paths -- 16385 candidates (global sort), 8193 (global sort, another
    P than the batch's), 0 (no candidate) -- queued with lazy=True and read once."""
    import bev_native as nat
    Ks = (16385, 8193, 0)
    heat, offset, size, (rb, rs, info) = _capacity_case(Ks)
    assert tuple(i["ncand"] for i in info) == Ks and rb[2].shape == (0, 4)
    assert Ks[1] == nat.lib().bev_decode_max_candidates() + 1
    _assert_same(_run(heat, offset, size, BOUNDS_CAP, 0.25, 1.5, lazy=True), (rb, rs), Ks)


# ---- 4. kept list beyond the LDS cache -------------------------------------------------------------------------
_KEPT_CACHE = {}
KEPT_HALF = 22082     # boxes the reference keeps at nms 0.5 (seed 330)
N_SUP_GLOBAL = 1564   # candidates whose first suppressor has kept index >= 8192


def _kept_case(nms):
    if "in" not in _KEPT_CACHE:
        H = W = 160
        rng = np.random.default_rng(330)
        heat = (rng.integers(1, 5, size=(1, 1, H, W)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
        _KEPT_CACHE["in"] = (heat,) + _offsets_sizes(rng, 1, H, W)
    if nms not in _KEPT_CACHE:
        _KEPT_CACHE[nms] = decode_reference(*_KEPT_CACHE["in"], (-80.0, 80.0, -80.0, 80.0), -1.0, nms)
    return _KEPT_CACHE["in"], _KEPT_CACHE[nms]


@pytest.mark.gpu
@pytest.mark.parametrize("nms", [0.5, 0.0])
def test_decode_kept_list_beyond_lds_cache(nms):
    """160 x 160 map of four levels (0.25 .. 1.0), conf_thresh -1: all 25600 cells are candidates (plateau peaks
    in level order, then the non-peaks at +0.0 in cell order), 1 m cells, offsets in [0, 1).
    nms 0.5 m: the reference keeps KEPT_HALF = 22082 boxes, far more than the 8192 kept centres k_large_nms caches in
    LDS, and N_SUP_GLOBAL = 1564 candidates are suppressed ONLY by kept boxes at kept index >= 8192 (their first
    suppressor lies beyond the cache), so the kernel must read kept centres back from global memory.
    nms 0.0: nothing is ever suppressed, all 25600 are kept."""
    (heat, offset, size), (rb, rs, info) = _kept_case(nms)
    bounds = (-80.0, 80.0, -80.0, 80.0)
    assert info[0]["ncand"] == 25600
    if nms == 0.0:
        assert info[0]["kept"] == 25600
    else:
        assert info[0]["kept"] == KEPT_HALF > 8192 + 64
        assert int((info[0]["first_sup"] >= 8192).sum()) == N_SUP_GLOBAL > 0
    _assert_same(_run(heat, offset, size, bounds, -1.0, nms), (rb, rs), nms)


