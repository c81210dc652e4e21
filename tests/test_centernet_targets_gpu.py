"""CenterNet training targets on the device (bev_native.centernet_targets: csrc/bev_targets.hip, two launches) against
BEVNet._targets_from_boxes' torch ops on the same device (model_wrapper.NATIVE_TARGETS = False): all five tensors
torch.equal -- the kernels replay torch's float32 op sequence.  Grids: 60 x 180 (rows of 16-byte groups) and 37 x 53
(odd: tile seams, unaligned rows), MAX_OBJECTS = 5."""
import copy

import pytest
import torch

import bev_native as nat
import models.model_wrapper as mw
from models.model_wrapper import BEVNet

pytestmark = pytest.mark.gpu

CFG_A = {"MODEL": {"BACKBONE": "resnet18", "PRETRAINED": False, "FEAT_DIM": 8, "OUT_INDEX": 2,
                   "BEV_SIZE": [8, 60, 180], "BEV_BOUNDS": [-24.0, 24.0, -7.2, 7.2], "BEV_PROJ_CH": 0,
                   "BACKBONE_IMPL": "fallback"},
         "LOSS": {"MAX_OBJECTS": 5}, "EVAL": {}}
CFG_B = copy.deepcopy(CFG_A)
CFG_B["MODEL"].update({"BEV_SIZE": [8, 37, 53], "BEV_BOUNDS": [-10.0, 11.2, -7.4, 7.4]})
KEYS = ("heatmap", "indices", "mask", "offset", "size_log")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=[CFG_A, CFG_B], ids=["60x180", "37x53"])
def net(request, dev):
    return BEVNet(request.param).to(dev)


def _targets(net, boxes, frame, B, native):
    old = mw.NATIVE_TARGETS
    try:
        mw.NATIVE_TARGETS = native
        return net._targets_from_boxes(boxes, frame, None, B)
    finally:
        mw.NATIVE_TARGETS = old


def _same(a, b):
    """torch.equal, NaNs in the same places counting as equal."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _assert_parity(net, boxes, frame, B, what="", torch_boxes=None):
    """Native targets of (boxes, frame) == the torch path's (of torch_boxes, where the torch path cannot take the
    same input)."""
    dev = next(net.parameters()).device
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(dev)
    frame = torch.as_tensor(frame, dtype=torch.long).reshape(-1).to(dev)
    got = _targets(net, boxes, frame, B, True)
    tb, tf = (boxes, frame) if torch_boxes is None else torch_boxes
    ref = _targets(net, tb, tf, B, False)
    for k in KEYS:
        assert _same(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))
    return got


def _random_targets(g, trial, net):
    x0, x1, y0, y1 = net.bounds
    B = int(torch.randint(1, 4, (1,), generator=g))
    out = []
    for _ in range(B):
        n = int(torch.randint(0, 9, (1,), generator=g))
        xy = torch.cat([torch.rand(n, 1, generator=g) * (x1 - x0) * 1.25 + x0 - (x1 - x0) * 0.125,
                        torch.rand(n, 1, generator=g) * (y1 - y0) * 1.4 + y0 - (y1 - y0) * 0.2], 1)
        if trial % 3 == 0 and n:
            out.append({"boxes_world": torch.cat([xy, torch.rand(n, 2, generator=g) * 3 + 0.01], 1)})
        elif trial % 3 == 1 and n:
            out.append({"centers_world": xy.double()})
        else:
            out.append({})
    return out


def test_random_batches_equal_torch_path(net, dev):
    g = torch.Generator().manual_seed(5)
    peaks = 0
    for trial in range(24):
        tg = _random_targets(g, trial, net)
        boxes, frame, _ = net._target_boxes(tg, dev)
        peaks += int((_assert_parity(net, boxes, frame, len(tg), trial)["heatmap"] == 1).sum())
    assert peaks > 20


def _world(net, gx, gy):
    return net.bounds[0] + gx * net.res_x, net.bounds[2] + gy * net.res_y


def test_edge_cases_equal_torch_path(net, dev):
    Hb, Wb, M = net.bev_h, net.bev_w, net.max_objects
    x0, x1, y0, y1 = net.bounds
    box = lambda gx, gy, w=0.6, h=0.6: [*_world(net, gx, gy), w, h]  # noqa: E731
    t = _assert_parity(net, [[x0, y0, 0.6, 0.6], [x1, y0 + net.res_y, 0.6, 0.6], [2 * x1 - x0, y0, 1, 1]], [0, 0, 0], 1,
                       "gx == 0 and gx == Wb")
    assert t["mask"][0, 0] == 1 and t["mask"][0, 2] == 0
    corners = [box(0.5, 0.5, 3, 2), box(Wb - 0.5, 0.5, 2, 3), box(0.5, Hb - 0.5, 1, 1), box(Wb - 0.5, Hb - 0.5, 4, 4)]
    t = _assert_parity(net, corners, [0] * 4, 1, "corners")
    assert t["heatmap"][0, 0, 0, 0] == 1 and t["heatmap"][0, 0, Hb - 1, Wb - 1] == 1
    t = _assert_parity(net, [box(20.3, 11.6), box(20.7, 11.2, 2.5, 1.0), box(23.5, 12.5, 2, 2), box(26.1, 9.9, 3, 3)],
                       [1] * 4, 2, "two in one cell, overlapping")
    assert t["indices"][1, 0] == t["indices"][1, 1] and int((t["heatmap"][1] == 1).sum()) == 3
    many = [box(3.5 + 4 * i, 5.5 + 2 * i) if i % 3 else box(-4.0, 1.0) for i in range(12)]
    t = _assert_parity(net, many, [0] * 12, 1, "more than M")
    assert t["mask"].sum() == M


def test_long_frame_runs_the_chunk_loops_twice(net, dev):
    """One frame with 300 objects and M = 280: the slot pass and the tiles' list loop both take a second chunk."""
    g = torch.Generator().manual_seed(9)
    x0, x1, y0, y1 = net.bounds
    n = 300
    boxes = torch.cat([torch.rand(n, 1, generator=g) * (x1 - x0) * 1.02 + x0 - (x1 - x0) * 0.01,
                       torch.rand(n, 1, generator=g) * (y1 - y0) * 1.02 + y0 - (y1 - y0) * 0.01,
                       torch.rand(n, 2, generator=g) * 2 + 0.05], 1)
    old = net.max_objects
    try:
        net.max_objects = 280
        t = _assert_parity(net, boxes, [1] * n, 2, "300 objects")
        assert t["mask"][1].sum() > 256 and t["mask"][0].sum() == 0 and t["indices"].shape == (2, 280)
    finally:
        net.max_objects = old


def test_radius_zero_fills_the_slot_and_draws_nothing(net, dev):
    old = net.gaussian_min_radius
    try:
        net.gaussian_min_radius = 0
        t = _assert_parity(net, [[*_world(net, 7.5, 7.5), net.res_x, net.res_y], [*_world(net, 17.5, 9.5), 8.0, 8.0]],
                           [0, 0], 1, "radius 0")
        assert t["mask"][0, 0] == 1 and int((t["heatmap"] == 1).sum()) == 1
    finally:
        net.gaussian_min_radius = old


def test_frame_index_outside_the_batch_is_ignored(net, dev):
    """A frame index equal to B (or negative) names no frame.  The torch path would index out of range with it, so its
    side of the comparison gets the same boxes without those rows."""
    box = lambda gx, gy, w=0.6, h=0.6: [*_world(net, gx, gy), w, h]  # noqa: E731
    boxes = torch.tensor([box(5.5, 5.5), box(9.5, 7.5), box(12.5, 3.5), box(8.5, 8.5), box(1.5, 1.5), box(3.5, 2.5)])
    frame = torch.tensor([0, 1, 1, 2, 2, -1])
    keep = (frame >= 0) & (frame < 2)
    _assert_parity(net, boxes, frame, 2, "frame == B", torch_boxes=(boxes[keep].to(dev), frame[keep].to(dev)))


def test_non_finite_boxes(net, dev):
    nan, inf = float("nan"), float("inf")
    t = _assert_parity(net, [[nan, 0.0, 1, 1], [*_world(net, 4.5, 4.5), nan, 1.0], [*_world(net, 9.5, 9.5), 1.0, inf],
                             [*_world(net, 14.5, 4.5), 0.0, -1.0]], [0] * 4, 1, "NaN / Inf")
    assert t["mask"][0].tolist() == [1, 1, 1, 0, 0] and bool(t["size_log"][0, 0, 0].isnan())
    assert int((t["heatmap"] == 1).sum()) == 1 and not bool(t["heatmap"].isnan().any())


def test_large_box_needs_no_window_tensor(net, dev, monkeypatch):
    """One box of 10^4 m (a radius of thousands of cells: the torch path's [N, (2R+1)^2] window cannot be allocated)
    among ordinary ones.  The heatmap is compared with a full-grid restatement per object on the device (torch's ops:
    tensor-over-tensor division, max over objects); the slot tensors with the torch path's, its splat skipped."""
    Hb, Wb = net.bev_h, net.bev_w
    boxes = torch.tensor([[*_world(net, 30.5, 20.5), 1e4, 1e4], [*_world(net, 3.5, 4.5), 0.6, 0.6],
                          [*_world(net, 40.5, 30.5), 2.0, 1.0], [*_world(net, 11.5, 7.5), 5e3, 0.5]]).to(dev)
    frame = torch.tensor([0, 0, 1, 1], device=dev)
    got = _targets(net, boxes, frame, 2, True)
    monkeypatch.setattr(BEVNet, "_splat_gaussians", staticmethod(lambda *a: None))
    ref = _targets(net, boxes, frame, 2, False)
    for k in KEYS[1:]:
        assert torch.equal(got[k], ref[k]), k
    gx = (boxes[:, 0] - net.bounds[0]) / net.res_x
    gy = (boxes[:, 1] - net.bounds[2]) / net.res_y
    cx, cy = torch.floor(gx).long(), torch.floor(gy).long()
    radius = nat.gaussian_radius((boxes[:, 2] / net.res_x).clamp(min=1e-3), (boxes[:, 3] / net.res_y).clamp(min=1e-3),
                                 net.gaussian_iou, net.gaussian_min_radius)
    assert int(radius.max()) > 1000
    two_s2 = (((2.0 * radius.double() + 1.0) / 6.0) ** 2 * 2.0).float()
    hm = torch.zeros(2, 1, Hb, Wb, device=dev)
    ys, xs = torch.arange(Hb, device=dev)[:, None], torch.arange(Wb, device=dev)[None, :]
    for i in range(boxes.shape[0]):
        dx, dy = xs - cx[i], ys - cy[i]
        val = torch.exp(-(dx * dx + dy * dy).float() / two_s2[i].expand(Hb, Wb))
        ok = (dx.abs() <= radius[i]) & (dy.abs() <= radius[i])
        b = int(frame[i])
        hm[b, 0] = torch.maximum(hm[b, 0], torch.where(ok, val, torch.zeros_like(val)))
    assert torch.equal(got["heatmap"], hm)
    assert bool((got["heatmap"][0] > 0).all())


def test_device_resident_boxes_make_no_synchronising_call(net, dev):
    """_build_training_targets on boxes that already live on the device: no host synchronisation (the torch path
    reads the largest radius back)."""
    tg = [{"boxes_world": torch.tensor([[1.0, 0.5, 0.6, 0.6], [-3.0, 2.0, 1.6, 0.6]], device=dev)},
          {"boxes_world": torch.tensor([[2.0, -1.5, 0.9, 2.6]], device=dev)}, {}]
    assert mw.NATIVE_TARGETS
    warm = net._build_training_targets(tg)  # the workspace, the library
    torch.cuda.synchronize()
    probe = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the mode is honoured: a read-back raises
            probe.item()
        t = net._build_training_targets(tg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in KEYS:
        assert torch.equal(t[k], warm[k])
    assert t["mask"].sum() == 3


def test_graph_capture_replays_with_new_boxes(net, dev):
    g = torch.Generator().manual_seed(3)
    x0, x1, y0, y1 = net.bounds
    n = 9

    def draw():
        return torch.cat([torch.rand(n, 1, generator=g) * (x1 - x0) * 1.1 + x0 - (x1 - x0) * 0.05,
                          torch.rand(n, 1, generator=g) * (y1 - y0) * 1.1 + y0 - (y1 - y0) * 0.05,
                          torch.rand(n, 2, generator=g) * 3 + 0.05], 1)

    args = (2, net.max_objects, (net.bev_h, net.bev_w), net.bounds, (net.res_x, net.res_y), net.gaussian_iou,
            net.gaussian_min_radius)
    boxes = draw().to(dev)
    frame = torch.tensor([0] * 4 + [1] * 5, device=dev)
    nat.centernet_targets(boxes, frame, *args)  # the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = nat.centernet_targets(boxes, frame, *args)
    for _ in range(3):
        new = draw().to(dev)
        boxes.copy_(new)
        graph.replay()
        eager = nat.centernet_targets(new, frame, *args)
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
        assert outs[2].sum() > 0


def test_loss_bit_identical_with_and_without_native_targets(dev):
    net = BEVNet(CFG_A).to(dev)
    g = torch.Generator().manual_seed(11)
    targets = [{"boxes_world": torch.tensor([[1.0, 0.5, 0.6, 0.6], [-3.0, 2.0, 0.6, 0.6], [30.0, 0.0, 0.6, 0.6]])},
               {"centers_world": torch.tensor([[-20.0, -5.0], [3.0, 3.0]])}]
    B, Hb, Wb = len(targets), net.bev_h, net.bev_w
    p = {"heatmap_logits": torch.randn(B, 1, Hb, Wb, generator=g) * 2,
         "offset": torch.rand(B, 2, Hb, Wb, generator=g), "size_raw": torch.randn(B, 2, Hb, Wb, generator=g)}
    res = []
    old = mw.NATIVE_TARGETS
    try:
        for native in (True, False):
            mw.NATIVE_TARGETS = native
            pd = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
            ls = net.loss(pd, targets, {})
            gr = torch.autograd.grad(ls["total_loss"] * 3.0, [pd[k] for k in sorted(pd)])
            res.append([ls[k].detach().clone() for k in sorted(ls)] + [x.clone() for x in gr])
    finally:
        mw.NATIVE_TARGETS = old
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0]) > 0
