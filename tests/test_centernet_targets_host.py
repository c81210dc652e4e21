"""CenterNet training targets, host side (no GPU): the per-object arithmetic of csrc/bev_targets.h compiled for the CPU
behind bev_centernet_targets_host, against a numpy float32 restatement of the reference's per-frame, per-object loop
(model_wrapper.py:126-203, 278-300: the first MAX_OBJECTS in-grid objects of a frame fill its slots in order, one
clipped gaussian window per object) with the device's reciprocal forms (a tensor over a Python scalar s is a product
with the caller's reciprocal of s); and the C entries' argument rules.

indices, mask, offset, the set of non-zero heatmap cells and the set of cells equal to 1.0 must match exactly: they
come from +, -, *, /, sqrt and floor alone, which numpy's float32 rounds as the library does.  size_log and the other
heatmap values go through the host's logf / expf (glibc: within 1 ulp), so they are held to 1 ulp of the float64
function value rounded to float32."""
import ctypes
import os

import numpy as np
import pytest

import bev_native

F = np.float32
GRID_A = dict(bev_hw=(60, 180), bounds=(-24.0, 24.0, -7.2, 7.2), M=5)
GRID_B = dict(bev_hw=(37, 53), bounds=(-10.0, 11.2, -7.4, 7.4), M=5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(bev_native.LIB_PATH):
        bev_native.build()
    return bev_native.lib()


def _res(grid):
    (Hb, Wb), (x0, x1, y0, y1) = grid["bev_hw"], grid["bounds"]
    return (x1 - x0) / float(Wb), (y1 - y0) / float(Hb)


def _clamp_min(x, lo):  # torch.clamp(min=lo): NaN stays NaN
    return lo if x < lo else x


def _min(a, b):  # torch.min: NaN wins
    return a if a != a else (b if b != b else (b if b < a else a))


def _radius_ref(wc, hc, ov, min_radius):
    """BEVNet._gaussian_radius_tensor (model_wrapper.py:205-233) for one object, float32 op by op."""
    w, h = _clamp_min(wc, F(1)), _clamp_min(hc, F(1))
    f_1mov, rcp_1pov = F(1 - ov), F(1) / F(1 + ov)

    def root(a, b, c):
        return b + np.sqrt(_clamp_min(b * b - (a * F(4)) * c, F(0)))

    r1 = root(F(1), h + w, ((w * h) * f_1mov) * rcp_1pov) * F(0.5)
    r2 = root(F(4), (h + w) * F(2), (w * f_1mov) * h) / (F(4) * F(2))
    r = _min(r1, r2)
    if ov != 0:
        a3 = F(4 * ov)
        r = _min(r, root(a3, (h + w) * F(-2 * ov), (w * F(ov - 1)) * h) / (a3 * F(2)))
    r = np.floor(_clamp_min(r, F(min_radius)))
    return int(r) if np.isfinite(r) else 0  # a NaN / infinite radius draws nothing


def _ref_targets(boxes, frame, B, grid, ov=0.7, min_radius=2):
    """The reference's loop: (exact parts, float64-rounded parts)."""
    (Hb, Wb), M = grid["bev_hw"], grid["M"]
    res_x, res_y = _res(grid)
    x_min, y_min = F(grid["bounds"][0]), F(grid["bounds"][2])
    rrx, rry = F(1.0 / res_x), F(1.0 / res_y)  # the device's form: the reciprocal in double, then float32
    hm = np.zeros((B, 1, Hb, Wb), F)
    indices = np.zeros((B, M), np.int64)
    mask = np.zeros((B, M), F)
    offset = np.zeros((B, M, 2), F)
    size_log = np.zeros((B, M, 2), F)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        for b in range(B):
            slot = 0
            for i in np.nonzero(np.asarray(frame) == b)[0]:
                gx, gy = (boxes[i, 0] - x_min) * rrx, (boxes[i, 1] - y_min) * rry
                if not (gx >= 0 and gx < F(Wb) and gy >= 0 and gy < F(Hb)) or slot >= M:
                    continue
                cx, cy = np.floor(gx), np.floor(gy)
                w, h = _clamp_min(boxes[i, 2] * rrx, F(1e-3)), _clamp_min(boxes[i, 3] * rry, F(1e-3))
                indices[b, slot] = int(cy) * Wb + int(cx)
                mask[b, slot] = 1
                offset[b, slot] = gx - cx, gy - cy
                size_log[b, slot] = F(np.log(np.float64(w))), F(np.log(np.float64(h)))
                slot += 1
                r = _radius_ref(w, h, ov, min_radius)
                if r <= 0:
                    continue
                cx, cy = int(cx), int(cy)
                s2 = F(((2.0 * r + 1.0) * (1.0 / 6.0)) ** 2 * 2.0)
                ys = np.arange(max(cy - r, 0), min(cy + r, Hb - 1) + 1)
                xs = np.arange(max(cx - r, 0), min(cx + r, Wb - 1) + 1)
                d2 = ((ys - cy) ** 2)[:, None] + ((xs - cx) ** 2)[None, :]
                q = -d2.astype(F) / s2  # float32 division, as the device's
                val = np.exp(q.astype(np.float64)).astype(F)
                win = hm[b, 0, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
                np.maximum(win, val, out=win)
    return hm, indices, mask, offset, size_log


def _check_against_ref(boxes, frame, B, grid, ov=0.7, min_radius=2):
    boxes, frame = np.asarray(boxes, F).reshape(-1, 4), np.asarray(frame, np.int64).reshape(-1)
    got = bev_native.centernet_targets_host(boxes, frame, B, grid["M"], grid["bev_hw"], grid["bounds"], _res(grid), ov,
                                            min_radius)
    ref = _ref_targets(boxes, frame, B, grid, ov, min_radius)
    hm, indices, mask, offset, size_log = got
    rhm, rindices, rmask, roffset, rsize = ref
    assert np.array_equal(indices, rindices)
    assert np.array_equal(mask, rmask)
    assert np.array_equal(offset.view(np.uint32), roffset.view(np.uint32))
    assert np.array_equal(hm > 0, rhm > 0)
    assert np.array_equal(hm == 1, rhm == 1)
    assert np.array_equal(np.isnan(size_log), np.isnan(rsize))
    ok = ~np.isnan(rsize)
    fin = ok & np.isfinite(rsize)
    assert np.array_equal(size_log[ok & ~fin], rsize[ok & ~fin])
    assert (np.abs(size_log[fin] - rsize[fin]) <= np.spacing(np.abs(rsize[fin]))).all()
    assert (np.abs(hm - rhm) <= np.spacing(rhm)).all()
    return got


def _random_case(rng, grid, trial):
    """Batches as tests/test_targets.py draws them: B 1-3, 0-8 objects per frame, centres partly outside the grid,
    frames with boxes, with default-size centres, and empty ones."""
    x0, x1, y0, y1 = grid["bounds"]
    B = int(rng.integers(1, 4))
    boxes, frame = [], []
    for b in range(B):
        n = int(rng.integers(0, 9))
        xy = np.stack([rng.random(n) * (x1 - x0) * 1.25 + x0 - (x1 - x0) * 0.125,
                       rng.random(n) * (y1 - y0) * 1.4 + y0 - (y1 - y0) * 0.2], 1)
        if trial % 3 == 0:
            wh = rng.random((n, 2)) * 3 + 0.01
        elif trial % 3 == 1:
            wh = np.full((n, 2), 0.6)
        else:
            continue
        boxes.append(np.concatenate([xy, wh], 1))
        frame += [b] * n
    boxes = np.concatenate(boxes) if boxes else np.zeros((0, 4))
    return boxes.astype(F), np.asarray(frame, np.int64), B


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["60x180", "37x53"])
def test_host_targets_match_reference_loop_random(lib, grid):
    rng = np.random.default_rng(5)
    drawn = 0
    for trial in range(45):
        boxes, frame, B = _random_case(rng, grid, trial)
        hm = _check_against_ref(boxes, frame, B, grid)[0]
        drawn += int((hm == 1).sum())
    assert drawn > 40


def _world(grid, gx, gy):
    """World coordinates that land on grid position (gx, gy) up to float32 rounding."""
    rx, ry = _res(grid)
    return grid["bounds"][0] + gx * rx, grid["bounds"][2] + gy * ry


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["60x180", "37x53"])
def test_host_targets_edge_cases(lib, grid):
    (Hb, Wb), M = grid["bev_hw"], grid["M"]
    x0, x1, y0, y1 = grid["bounds"]
    rx, ry = _res(grid)
    box = lambda gx, gy, w=0.6, h=0.6: [*_world(grid, gx, gy), w, h]  # noqa: E731
    # centres exactly at gx == 0 (inside) and gx == Wb (outside); x_max itself may round either way, so also 2 x_max
    _, _, mask, _, _ = _check_against_ref([[x0, y0, 0.6, 0.6], [x1, y0 + ry, 0.6, 0.6], [2 * x1 - x0, y0, 1, 1]],
                                          [0, 0, 0], 1, grid)
    assert mask[0, 0] == 1 and mask[0, 2] == 0
    # the four corners (clipped windows), two objects in one cell, overlapping gaussians
    corners = [box(0.5, 0.5, 3, 2), box(Wb - 0.5, 0.5, 2, 3), box(0.5, Hb - 0.5, 1, 1), box(Wb - 0.5, Hb - 0.5, 4, 4)]
    _check_against_ref(corners, [0] * 4, 1, grid)
    hm = _check_against_ref([box(20.3, 11.6), box(20.7, 11.2, 2.5, 1.0), box(23.5, 12.5, 2, 2), box(26.1, 9.9, 3, 3)],
                            [1] * 4, 2, grid)[0]
    assert hm[0].max() == 0 and (hm[1] == 1).sum() == 3
    # more than M in-grid objects, out-of-grid ones in between: the first M in order take the slots
    many = [box(3.5 + 4 * i, 5.5 + 2 * i) if i % 3 else box(-4.0, 1.0) for i in range(12)]
    _, indices, mask, _, _ = _check_against_ref(many, [0] * 12, 1, grid)
    assert mask.sum() == M
    # frames out of order in the array, a frame index equal to B (the padded dummies), a negative one
    _check_against_ref([box(5.5, 5.5), box(9.5, 7.5), box(12.5, 3.5), box(8.5, 8.5), box(1.5, 1.5)], [1, 0, 2, -1, 1],
                       2, grid)
    # GAUSSIAN_MIN_RADIUS = 0 and a one-cell box: radius 0 -- the slot is filled, nothing is drawn
    hm, _, mask, _, _ = _check_against_ref([[*_world(grid, 7.5, 7.5), rx, ry]], [0], 1, grid, min_radius=0)
    assert mask[0, 0] == 1 and hm.max() == 0
    # NaN centre: no slot.  NaN / Inf sizes: the slot with NaN / Inf size_log, nothing drawn
    nan, inf = float("nan"), float("inf")
    hm, _, mask, _, size_log = _check_against_ref(
        [[nan, 0.0, 1, 1], [*_world(grid, 4.5, 4.5), nan, 1.0], [*_world(grid, 9.5, 9.5), 1.0, inf],
         [*_world(grid, 14.5, 4.5), 0.0, -1.0]], [0] * 4, 1, grid)
    assert mask[0].tolist() == [1, 1, 1, 0, 0] and np.isnan(size_log[0, 0, 0]) and size_log[0, 1, 1] == inf
    assert (hm == 1).sum() == 1  # only the zero / negative size (clamped to 1e-3 cells) draws
    # a box far larger than the map: the window is the map
    hm = _check_against_ref([[*_world(grid, Wb / 2, Hb / 2), 300.0, 200.0]], [0], 1, grid)[0]
    assert (hm > 0).all()
    # other overlaps, ov == 0 among them (no r3 root)
    for ov in (0.0, 0.3, 0.5):
        _check_against_ref(corners + [box(20.5, 11.5, 5, 2)], [0] * 5, 1, grid, ov=ov)


def test_host_targets_long_frame(lib):
    """One frame with 300 objects and M = 280; N == 0 and M == 0."""
    grid = dict(GRID_A, M=280)
    rng = np.random.default_rng(9)
    boxes, frame, _ = _random_case(rng, GRID_A, 0)
    n = 300
    xy = np.stack([rng.random(n) * 50 - 25, rng.random(n) * 15 - 7.5], 1)
    boxes = np.concatenate([xy, rng.random((n, 2)) * 2 + 0.05], 1)
    _, _, mask, _, _ = _check_against_ref(boxes, [1] * n, 2, grid)
    assert 200 < mask[1].sum() <= 280 and mask[0].sum() == 0
    got = _check_against_ref(np.zeros((0, 4)), np.zeros(0), 2, GRID_B)
    assert all(not a.any() for a in got)
    got = _check_against_ref(boxes[:5], [0] * 5, 1, dict(GRID_B, M=0))
    assert got[1].shape == (1, 0) and not got[0].any()


def _args(N=1, B=1, M=2, Hb=4, Wb=8, null=(), ws_bytes=None, host=False):
    """One accepted argument set for the C entries (host buffers: the device entry must refuse before it touches
    them), with the named pointers nulled."""
    big = B * M > 4096 or Hb * Wb > 4096  # refused by size: one-element buffers
    b, m, hb, wb = (1, 1, 1, 1) if big else (max(B, 1), max(M, 1), max(Hb, 1), max(Wb, 1))
    bufs = {"boxes": np.zeros((max(N, 1), 4), F), "frame": np.zeros(max(N, 1), np.int64),
            "heatmap": np.zeros((b, 1, hb, wb), F), "indices": np.zeros((b, m), np.int64), "mask": np.zeros((b, m), F),
            "offset": np.zeros((b, m, 2), F), "size_log": np.zeros((b, m, 2), F),
            "workspace": np.zeros(4096, np.int64)}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in bufs.items()}
    scal = bev_native._targets_scalars((-1.0, 1.0, -1.0, 1.0), (0.25, 0.5), 0.7, 2)
    a = [p["boxes"], p["frame"], N, B, M, Hb, Wb, *scal, p["heatmap"], p["indices"], p["mask"], p["offset"],
         p["size_log"]]
    if not host:
        a += [p["workspace"], 4096 * 8 if ws_bytes is None else ws_bytes, None]
    return a, bufs


def test_argument_rules(lib):
    wsb = lib.bev_centernet_targets_workspace_bytes
    assert wsb(3, 5) == 3 * (5 + 1) * 16 and wsb(0, 7) == 0 and wsb(2, 0) == 32
    assert wsb(-1, 5) == 0 and wsb(1, -1) == 0 and wsb(1 << 13, 1 << 12) == 0 and wsb(1 << 12, 1 << 12) > 0
    for entry, host in ((lib.bev_centernet_targets_f32, False), (lib.bev_centernet_targets_host, True)):
        refused = [dict(null=(k,)) for k in ("boxes", "frame", "heatmap", "indices", "mask", "offset", "size_log")]
        refused += [dict(N=-1), dict(B=-1), dict(M=-1), dict(Hb=0), dict(Wb=-3), dict(Hb=1 << 14, Wb=(1 << 14) + 1),
                    dict(B=1 << 13, M=(1 << 11) + 1)]
        if not host:
            refused += [dict(null=("workspace",)), dict(ws_bytes=wsb(1, 2) - 1), dict(ws_bytes=0)]
        for kw in refused:
            a, keep = _args(host=host, **kw)
            assert entry(*a) == bev_native.BEV_ERR_ARGS == -1, (host, kw)
        a, keep = _args(host=host, B=0, null=("heatmap", "indices", "mask", "offset", "size_log", "workspace"))
        assert entry(*a) == 0  # B == 0: nothing to write
    # null boxes / frame are fine when there is nothing to read; null slot outputs when B * M == 0
    a, bufs = _args(host=True, N=0, null=("boxes", "frame"))
    bufs["mask"][:] = 7
    bufs["heatmap"][:] = 7
    assert lib.bev_centernet_targets_host(*a) == 0 and not bufs["mask"].any() and not bufs["heatmap"].any()
    a, bufs = _args(host=True, M=0, null=("indices", "mask", "offset", "size_log"))
    assert lib.bev_centernet_targets_host(*a) == 0


def test_python_surface(lib):
    import torch
    with pytest.raises(ValueError):
        bev_native.centernet_targets_host(np.zeros((3, 5), F), np.zeros(3, np.int64), 1, 2, (4, 8), (-1, 1, -1, 1),
                                          (0.25, 0.5), 0.7, 2)
    with pytest.raises(ValueError):
        bev_native.centernet_targets_host(np.zeros((3, 4), F), np.zeros(2, np.int64), 1, 2, (4, 8), (-1, 1, -1, 1),
                                          (0.25, 0.5), 0.7, 2)
    with pytest.raises(bev_native.HipError):  # no CPU fallback behind the device entry
        bev_native.centernet_targets(torch.zeros(3, 4), torch.zeros(3, dtype=torch.long), 1, 2, (4, 8), (-1, 1, -1, 1),
                                     (0.25, 0.5), 0.7, 2)
    import models.model_wrapper as mw
    assert isinstance(mw.NATIVE_TARGETS, bool)
