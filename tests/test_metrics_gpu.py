"""Validation scoring on the device (bev_native.detection_match: csrc/bev_metrics.hip, one launch per batch) against
the library's host entry (the same per-pair functions compiled for the CPU, itself pinned to the reference and to a
numpy restatement by tests/test_metrics_host.py): int32 counts and double sums bit for bit, on every size at which the
kernel takes another path -- no work, one lane, a wave and its neighbours, more than one round of 256 predictions, a
frame past the on-chip chunk and winner table (1024 ground truths: the workspace) -- and end to end behind a lazy
decode, the decode's large path included."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN  # noqa: F401  (puts the package on the path)
from test_metrics_host import CASES, SEQ, as_torch, check_tuple, pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
BOUNDS = (-24.0, 24.0, -7.2, 7.2)
# (K, G): the issue's list, one G just past the LDS chunk / table (1024) and one that needs three chunks
SHAPES = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (255, 1), (256, 256), (257, 300), (300, 1025),
          (40, 2050)]


def frame(rng, K, G, style):
    if style == "lattice":  # exact ties and distances equal to the threshold
        return rng.integers(-8, 9, (K, 4)).astype(F) * F(0.25), rng.integers(-8, 9, (G, 4)).astype(F) * F(0.25)
    g = rng.uniform(-20, 20, (G, 4)).astype(F)
    p = rng.uniform(-20, 20, (K, 4)).astype(F)
    for i in range(K if G else 0):
        if rng.random() < 0.8:
            p[i, :2] = g[int(rng.integers(0, G)), :2] + rng.normal(0, 0.25, 2).astype(F)
    return p, g


def both(packed, m):
    """(device counts, sums), (host counts, sums) as numpy arrays."""
    import bev_native as nat
    host = nat.detection_match_host(*packed, m)
    dev = nat.detection_match(*(torch.from_numpy(a).to(DEV) for a in packed), m)
    assert dev[0].dtype == torch.int32 and dev[1].dtype == torch.float64 and dev[0].is_cuda
    return (dev[0].cpu().numpy(), dev[1].cpu().numpy()), host


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), (what, got[1], want[1])


@pytest.mark.parametrize("style", ["plain", "lattice"])
@pytest.mark.parametrize("K,G", SHAPES)
def test_one_frame_equals_host_entry(K, G, style):
    rng = np.random.default_rng(1000 * K + G)
    p, g = frame(rng, K, G, style)
    for m in (0.5, 0.3):
        got, want = both(pack([p], [g]), m)
        assert_same(got, want, (K, G, style, m))
        assert got[0][0, 3] == 0 and got[0][0, 0] + got[0][0, 1] == K and got[0][0, 0] + got[0][0, 2] == G
    if min(K, G) >= 63 and style == "plain":
        assert got[0][0, 0] > 0  # not vacuous


@pytest.mark.parametrize("shapes", [[(0, 5), (65, 63), (257, 300)], [(5, 0), (300, 1025), (1, 1)],
                                    [(40, 2050), (0, 0), (256, 1100)]], ids=["small", "one-long", "two-long"])
def test_ragged_batch_equals_host_entry(shapes):
    """B = 3, ragged: cap beyond most frames' counts (the rows past a count hold NaN and are never read), and each
    long frame's winner table at its own stretch of the workspace."""
    rng = np.random.default_rng(7)
    frames = [frame(rng, K, G, "plain") for K, G in shapes]
    packed = pack([f[0] for f in frames], [f[1] for f in frames], cap=max(K for K, _ in shapes) + 3)
    for b, (K, _) in enumerate(shapes):
        packed[0][b, K:] = np.nan
    got, want = both(packed, 0.5)
    assert_same(got, want, shapes)
    assert got[0][:, 1].tolist() == [K - t for (K, _), t in zip(shapes, got[0][:, 0])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_on_the_device(name):
    """The NaN / Inf / tie / threshold cases: the device entry against the host entry bit for bit, and compute_metrics
    on device tensors against the reference's recorded tuple."""
    from utils.metrics import compute_metrics
    preds, gts, m, prf, counts = CASES[name]
    assert_same(*both(pack(preds, gts), m), name)
    check_tuple(compute_metrics(*as_torch(preds, gts, DEV), match_dist=m), prf, counts, name)


def test_host_ground_truths_and_device_predictions_mix():
    """The loader's layout: boxes_world in host memory, detections on the device."""
    from utils.metrics import compute_metrics
    for name in SEQ:
        preds, gts, m, prf, counts = CASES[name]
        tp, _ = as_torch(preds, gts, DEV)
        _, tg = as_torch(preds, gts, "cpu")
        check_tuple(compute_metrics(tp, tg, match_dist=m), prf, counts, name)


def test_pending_frame_gives_status_minus_one_and_zeros():
    rng = np.random.default_rng(3)
    frames = [frame(rng, 20, 20, "plain") for _ in range(2)]
    packed = pack([f[0] for f in frames], [f[1] for f in frames])
    packed[1][0] = -1
    got, want = both(packed, 0.5)
    assert_same(got, want, "pending")
    assert got[0][0].tolist() == [0, 0, 0, -1] and got[1][0] == 0.0 and got[0][1, 3] == 0 and got[0][1, 0] > 0


def test_large_frame_is_quick():
    """K = 5000, G = 300: the ordered sum adds the matched distances only (at most 300), so the launch stays far
    below the second a walk over all K would be allowed."""
    import bev_native as nat
    rng = np.random.default_rng(5)
    p, g = frame(rng, 5000, 300, "plain")
    packed = pack([p], [g])
    got, want = both(packed, 0.5)  # also the warm-up
    assert_same(got, want, "large")
    assert got[0][0, 0] > 200
    dev = [torch.from_numpy(a).to(DEV) for a in packed]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    nat.detection_match(*dev, 0.5)
    t1.record()
    t1.synchronize()
    print(f"detection_match K=5000 G=300: {t0.elapsed_time(t1):.3f} ms")
    assert t0.elapsed_time(t1) < 1000.0


def _heatmap(seed, B, H, W, peaks):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(F)
    heat = np.zeros((B, 1, H, W), F)
    for b in range(B):
        for _ in range(peaks):
            cy, cx, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.5, 1.0)
            heat[b, 0] = np.maximum(heat[b, 0], (a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 3.0)).astype(F))
    offset = rng.random((B, 2, H, W), dtype=F)
    size = (rng.random((B, 2, H, W), dtype=F) * F(3.0) + F(1.0)).astype(F)
    return [torch.from_numpy(a).to(DEV) for a in (heat, offset, size)]


def _targets_near(boxes_cpu, rng, device):
    """Ground truths for decoded boxes: most of them displaced a little, some far off, some extra."""
    out = []
    for bx in boxes_cpu:
        g = bx.numpy().copy()[: max(1, int(0.8 * len(bx)))]
        g[:, :2] += rng.normal(0, 0.2, g[:, :2].shape).astype(F)
        extra = np.stack([rng.uniform(-24, 24, 3), rng.uniform(-7.2, 7.2, 3), np.ones(3), np.ones(3)], 1).astype(F)
        out.append({"boxes_world": torch.from_numpy(np.concatenate([g, extra])).to(device)})
    return out


@pytest.mark.parametrize("gt_on", ["cpu", DEV])
def test_lazy_decode_to_metrics_takes_no_host_wait(gt_on):
    from models.heads.detector import BEVDetector
    from utils.metrics import DetectionMetrics, compute_metrics
    H, W = 24, 40
    det = BEVDetector(in_channels=4, bev_bounds=BOUNDS, bev_size=(H, W)).to(DEV)
    val, want = DetectionMetrics(0.5), []
    for seed in (1, 2):
        maps = _heatmap(seed, 2, H, W, 12)
        eager = [b.cpu() for b in det.decode(*maps, conf_thresh=0.4)[0]]
        assert min(len(b) for b in eager) >= 3
        targets = _targets_near(eager, np.random.default_rng(seed), gt_on)
        boxes, _ = det.decode(*maps, conf_thresh=0.4, lazy=True)
        val.update(boxes, targets)
        assert not boxes.pending.materialised  # queued behind the decode: nobody waited for it
        want.append(compute_metrics(eager, [{"boxes_world": t["boxes_world"].cpu()} for t in targets], 0.5))
        assert compute_metrics(boxes, targets, 0.5) == want[-1] and not boxes.pending.materialised
        assert compute_metrics([b.to(DEV) for b in eager], targets, 0.5) == want[-1]  # the packed-list path
    got = val.result()
    assert val.in_flight() == 0
    assert got[:4] == tuple(sum(w[k] for w in want) / 2 for k in range(4))
    assert got[4:] == tuple(sum(w[k] for w in want) for k in (4, 5, 6)) and got[4] > 0 and got[5] > 0


def test_large_decode_path_falls_back_and_agrees():
    """One frame with more candidates than bev_decode_max_candidates (a plateau, as tests/test_decode_gpu.py builds
    it): the queued scoring sees the decode's negative count (status -1), and result() materialises that batch and
    scores it again -- the same numbers as the eager path."""
    import bev_native as nat
    from models.heads.detector import BEVDetector
    from utils.metrics import DetectionMetrics, compute_metrics
    H, W = 100, 100
    assert H * W > nat.lib().bev_decode_max_candidates()
    det = BEVDetector(in_channels=4, bev_bounds=BOUNDS, bev_size=(H, W)).to(DEV)
    heat, offset, size = _heatmap(4, 2, H, W, 10)
    heat[0] = 0.5  # every cell a peak
    offset[0] = 0.0
    args = dict(conf_thresh=0.3, nms_dist_m=3.0)
    eager = [b.cpu() for b in det.decode(heat, offset, size, **args)[0]]
    assert len(eager[0]) > 10 and len(eager[1]) >= 3
    targets = _targets_near(eager, np.random.default_rng(8), "cpu")
    boxes, _ = det.decode(heat, offset, size, lazy=True, **args)
    raw = boxes.pending.raw
    counts, _ = nat.detection_match(raw.boxes, raw.kept, torch.zeros(0, 2, device=DEV),
                                    torch.zeros(3, dtype=torch.int32, device=DEV), 0.5)
    assert counts.cpu().tolist()[0] == [0, 0, 0, -1] and counts.cpu().tolist()[1][3] == 0
    val = DetectionMetrics(0.5)
    val.update(boxes, targets)
    assert not boxes.pending.materialised and val.in_flight() == 1
    want = compute_metrics(eager, targets, 0.5)
    assert val.result() == want[:4] + want[4:] and boxes.pending.materialised and want[4] > 0
    assert [len(b) for b in boxes] == [len(b) for b in eager]
