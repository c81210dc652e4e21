"""MODA / MODP scoring on the device (bev_native.detection_assign: k_det_assign of csrc/bev_metrics.hip, one launch
per batch, one wave per frame) against the library's host entry -- the same procedure (csrc/bev_metrics.h,
assign_solve) run by one worker, itself pinned to an independent oracle by tests/test_mod_metrics_host.py: int32 counts,
status and the bits of the double sums, on every size at which the wave's column ownership changes (no work, fewer
columns than lanes, exactly a wave, one past it, several rounds), on exact ties, at the threshold, on non-finite
coordinates, at the device limit and one past it; and end to end behind a lazy decode, its large path included."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import mod_metrics_helper as H
from conftest import GOLDEN, PKG, REPO  # noqa: F401  (puts the package on the path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAN, INF = float("nan"), float("inf")
BOUNDS = (-24.0, 24.0, -7.2, 7.2)
SIZES = [0, 1, 2, 3, 63, 64, 65, 130, 257]


def both(packed, m):
    """(device counts, sums), (host counts, sums) as numpy arrays: one launch for the batch."""
    import bev_native as nat
    host = nat.detection_assign_host(*packed, m)
    dev = nat.detection_assign(*(torch.from_numpy(a).to(DEV) for a in packed), m)
    assert dev[0].dtype == torch.int32 and dev[1].dtype == torch.float64 and dev[0].is_cuda
    return (dev[0].cpu().numpy(), dev[1].cpu().numpy()), host


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), (what, got[1], want[1])


def grid_frame(rng, K, G, style):
    if style == "lattice":  # quarter-metre lattice on a patch that grows with the frame: exact ties, d == threshold
        r = max(2, int(np.sqrt(max(K, G))))
        return rng.integers(-r, r + 1, (K, 4)).astype(F) * F(0.25), rng.integers(-r, r + 1, (G, 4)).astype(F) * F(0.25)
    return H.sparse_crowd(rng, K, G, spacing=0.7)


@pytest.mark.parametrize("style", ["plain", "lattice"])
def test_size_grid_in_one_ragged_launch_equals_host_entry(style):
    """All 81 (K, G) of SIZES x SIZES as one batch: cap = 257 + 3, rows past a frame's count hold NaN."""
    rng = np.random.default_rng(17)
    shapes = [(K, G) for K in SIZES for G in SIZES]
    frames = [grid_frame(rng, K, G, style) for K, G in shapes]
    packed = H.pack([f[0] for f in frames], [f[1] for f in frames], cap=max(SIZES) + 3)
    for b, (K, _) in enumerate(shapes):
        packed[0][b, K:] = NAN
    for m in (0.5, 0.3):
        got, want = both(packed, m)
        assert_same(got, want, (style, m))
        c = got[0]
        assert not c[:, 3].any()
        assert (c[:, 0] + c[:, 1]).tolist() == [K for K, _ in shapes]
        assert (c[:, 0] + c[:, 2]).tolist() == [G for _, G in shapes]
    big = shapes.index((257, 257))
    assert c[big, 0] > 60  # not vacuous
    # the host entry is the oracle's equal on a few of these (the whole grid is the host file's business)
    for b in (shapes.index((63, 65)), shapes.index((130, 64))):
        tp, total, _ = H.oracle_frame(*frames[b], 0.3)
        assert c[b, 0] == tp and abs(got[1][b] - total) <= H.sum_bound(*shapes[b], 0.3, total)


def test_ties_threshold_edges_and_non_finite_coordinates_equal_host_entry():
    import bev_native as nat
    preds, gts = [f[0] for f in H.lattice_frames()], [f[1] for f in H.lattice_frames()]
    thr = F(nat.match_thr32(0.3))
    for d in (thr, np.nextafter(thr, F(np.inf)), F(0.3)):
        preds.append(np.zeros((1, 4), F))
        gts.append(np.asarray([[d, 0, 1, 1]], F))
    p, g = H.crowd(3)
    bad_p = np.asarray([[NAN, 1, 1, 1], [2, INF, 1, 1], [-INF, NAN, 1, 1]], F)
    bad_g = np.asarray([[INF, 1, 1, 1], [3, NAN, 1, 1]], F)
    preds += [p, np.insert(p, [0, 7, len(p)], bad_p, axis=0), bad_p]
    gts += [g, np.insert(g, [3, len(g)], bad_g, axis=0), bad_g]
    for m in (0.3, 0.5, 0.21, INF):
        got, want = both(H.pack(preds, gts), m)
        assert_same(got, want, m)
        assert got[0][-1].tolist() == [0, 3, 2, 0]  # nothing non-finite ever matches
    got, _ = both(H.pack(preds, gts), 0.3)
    assert got[0][3:6, 0].tolist() == [1, 0, 0] and got[1][3] == float(thr)
    clean, dirty = got[0][6], got[0][7]
    assert dirty.tolist() == [clean[0], clean[1] + 3, clean[2] + 2, 0] and got[1][6] == got[1][7]


def test_device_limit_frame_and_one_past_it():
    """1024 x 1024 -- the last index of every LDS array, 16 columns per lane -- equals the host entry; 1025
    predictions, or 1025 ground truths, is the too-large status from the C entry, zeros, and the right numbers from
    compute_mod_metrics, which finishes such a frame with the host entry."""
    import bev_native as nat
    from utils.metrics import DetectionMetrics, compute_mod_metrics, mod_from_totals
    n = nat.detection_assign_max_frame()
    assert n == 1024
    rng = np.random.default_rng(29)
    p, g = H.sparse_crowd(rng, n + 1, n + 1, spacing=1.0)
    d = H.dist32(p[:n], g[:n])
    partners = H.admissible(d, 0.5).sum(1)
    assert np.median(partners) in (1, 2, 3) and (partners <= 3).mean() > 0.5  # most rows have 1-3 partners
    small = H.sparse_crowd(rng, 20, 25, spacing=0.7)
    preds, gts = [small[0], p[:n], p, p[:n], small[0]], [small[1], g[:n], g[:n], g, small[1]]
    packed = H.pack(preds, gts)
    dev = [torch.from_numpy(a).to(DEV) for a in packed]
    nat.detection_assign(*dev, 0.5)  # warm-up
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    counts, sums = nat.detection_assign(*dev, 0.5)
    t1.record()
    t1.synchronize()
    print(f"detection_assign, 5 frames, one 1024 x 1024: {t0.elapsed_time(t1):.3f} ms")
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    host = nat.detection_assign_host(*packed, 0.5)
    assert counts[:, 3].tolist() == [0, 0, nat.MATCH_STATUS_TOO_LARGE, nat.MATCH_STATUS_TOO_LARGE, 0]
    assert not counts[2:4, :3].any() and not sums[2:4].any()
    for b in (0, 1, 4):
        assert np.array_equal(counts[b], host[0][b]) and sums[b].view(np.uint64) == host[1][b].view(np.uint64), b
    assert counts[1, 0] > 400 and host[0][2, 0] >= counts[1, 0]
    # the Python layer completes the two long frames on the host: the totals are the host entry's
    tg = [{"boxes_world": torch.from_numpy(x)} for x in gts]  # ground truths from the loader: host memory
    tp_ = [torch.from_numpy(x).to(DEV) for x in preds]
    total = 0.0
    for v in host[1].tolist():
        total += v
    want = mod_from_totals(int(host[0][:, 0].sum()), int(host[0][:, 1].sum()), int(host[0][:, 2].sum()), total, 0.5)
    assert compute_mod_metrics(tp_, tg, 0.5) == want and want["tp"] > 1200
    val = DetectionMetrics(0.5, matching="optimal")
    val.update(tp_, tg)
    assert val.result_mod() == want and val.in_flight() == 0


def _heatmap(seed, B, H_, W, peaks):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H_, 0:W].astype(F)
    heat = np.zeros((B, 1, H_, W), F)
    for b in range(B):
        for _ in range(peaks):
            cy, cx, a = rng.uniform(0, H_), rng.uniform(0, W), rng.uniform(0.5, 1.0)
            heat[b, 0] = np.maximum(heat[b, 0], (a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 3.0)).astype(F))
    offset = rng.random((B, 2, H_, W), dtype=F)
    size = (rng.random((B, 2, H_, W), dtype=F) * F(3.0) + F(1.0)).astype(F)
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


def _host_totals(boxes_cpu, targets, m):
    """tp, fp, fn, sum of a batch from the host entry, frame sums added in frame order."""
    import bev_native as nat
    c, s = nat.detection_assign_host(*H.pack([b.numpy() for b in boxes_cpu],
                                             [t["boxes_world"].cpu().numpy() for t in targets]), m)
    total = 0.0
    for v in s.tolist():
        total += v
    return int(c[:, 0].sum()), int(c[:, 1].sum()), int(c[:, 2].sum()), total


@pytest.mark.parametrize("gt_on", ["cpu", DEV])
def test_lazy_decode_to_optimal_metrics_takes_no_host_wait(gt_on):
    from models.heads.detector import BEVDetector
    from utils.metrics import DetectionMetrics, compute_mod_metrics, mod_from_totals
    H_, W = 24, 40
    det = BEVDetector(in_channels=4, bev_bounds=BOUNDS, bev_size=(H_, W)).to(DEV)
    val, totals = DetectionMetrics(0.5, matching="optimal"), []
    for seed in (1, 2):
        maps = _heatmap(seed, 2, H_, W, 12)
        eager = [b.cpu() for b in det.decode(*maps, conf_thresh=0.4)[0]]
        assert min(len(b) for b in eager) >= 3
        targets = _targets_near(eager, np.random.default_rng(seed), gt_on)
        boxes, _ = det.decode(*maps, conf_thresh=0.4, lazy=True)
        val.update(boxes, targets)
        assert not boxes.pending.materialised  # queued behind the decode: nobody waited for it
        totals.append(_host_totals(eager, targets, 0.5))
        want = mod_from_totals(*totals[-1], 0.5)
        assert compute_mod_metrics(boxes, targets, 0.5) == want and not boxes.pending.materialised
        assert compute_mod_metrics([b.to(DEV) for b in eager], targets, 0.5) == want  # the packed-list path
    got = val.result_mod()
    assert val.in_flight() == 0
    tp, fp, fn = (sum(t[k] for t in totals) for k in range(3))
    assert got == mod_from_totals(tp, fp, fn, 0.0 + totals[0][3] + totals[1][3], 0.5) and tp > 0 and fp > 0
    assert val.result()[4:] == (tp, fp, fn)


def test_pending_frame_status_and_rescoring_after_the_large_decode_path():
    """A count < 0 is status -1 and zeros from the C entry; behind a decode that left a frame to its large path (a
    plateau, as tests/test_decode_gpu.py builds it) the queued batch is scored again when the result is read."""
    import bev_native as nat
    from models.heads.detector import BEVDetector
    from utils.metrics import DetectionMetrics, mod_from_totals
    rng = np.random.default_rng(3)
    frames = [H.sparse_crowd(rng, 20, 20, spacing=0.7) for _ in range(2)]
    packed = H.pack([f[0] for f in frames], [f[1] for f in frames])
    packed[1][0] = -1
    got, want = both(packed, 0.5)
    assert_same(got, want, "pending")
    assert got[0][0].tolist() == [0, 0, 0, -1] and got[1][0] == 0.0 and got[0][1, 3] == 0 and got[0][1, 0] > 0

    H_, W = 100, 100
    assert H_ * W > nat.lib().bev_decode_max_candidates()
    det = BEVDetector(in_channels=4, bev_bounds=BOUNDS, bev_size=(H_, W)).to(DEV)
    heat, offset, size = _heatmap(4, 2, H_, W, 10)
    heat[0] = 0.5  # every cell a peak
    offset[0] = 0.0
    args = dict(conf_thresh=0.3, nms_dist_m=3.0)
    eager = [b.cpu() for b in det.decode(heat, offset, size, **args)[0]]
    assert len(eager[0]) > 10 and len(eager[1]) >= 3
    targets = _targets_near(eager, np.random.default_rng(8), "cpu")
    boxes, _ = det.decode(heat, offset, size, lazy=True, **args)
    raw = boxes.pending.raw
    counts, _ = nat.detection_assign(raw.boxes, raw.kept, torch.zeros(0, 2, device=DEV),
                                     torch.zeros(3, dtype=torch.int32, device=DEV), 0.5)
    assert counts.cpu().tolist()[0] == [0, 0, 0, -1] and counts.cpu().tolist()[1][3] == 0
    val = DetectionMetrics(0.5, matching="optimal")
    val.update(boxes, targets)
    assert not boxes.pending.materialised and val.in_flight() == 1
    want = mod_from_totals(*_host_totals(eager, targets, 0.5), 0.5)
    assert val.result_mod() == want and boxes.pending.materialised and want["tp"] > 0


def test_bad_offsets_are_a_status_not_a_fault():
    """Device entry only: offsets that decrease or leave [0, N] give status -2 and zeros; the other frames are
    scored."""
    import bev_native as nat
    rng = np.random.default_rng(4)
    frames = [H.sparse_crowd(rng, 10, 12, spacing=0.7) for _ in range(3)]
    packed = list(H.pack([f[0] for f in frames], [f[1] for f in frames]))
    host = nat.detection_assign_host(*packed, 0.5)
    packed[3] = np.asarray([0, 12, 40, 36], np.int32)  # frame 1 runs past N = 36, frame 2 runs backwards
    c, s = nat.detection_assign(*(torch.from_numpy(a).to(DEV) for a in packed), 0.5)
    c, s = c.cpu().numpy(), s.cpu().numpy()
    assert c[1].tolist() == [0, 0, 0, nat.MATCH_STATUS_OFFSETS] and c[2].tolist() == [0, 0, 0, nat.MATCH_STATUS_OFFSETS]
    assert np.array_equal(c[0], host[0][0]) and s[0] == host[1][0] and not s[1:].any()


SCRIPT = """
import sys
sys.path.insert(0, {pkg!r})
import torch
import bev_native as nat
pred = torch.zeros(1, 2, 4, device="cuda:0")
c, s = nat.detection_assign(pred, torch.tensor([2], dtype=torch.int32, device="cuda:0"),
                            torch.zeros(3, 2, device="cuda:0"), torch.tensor([0, 3], dtype=torch.int32, device="cuda:0"),
                            0.5)
torch.cuda.synchronize()
assert c.cpu().tolist() == [[2, 0, 1, 0]]
"""


def test_new_kernel_is_in_the_coverage_tools_launched_list(tmp_path):
    """A kernel trace of one detection_assign call in a child process, read by tools/kernel_coverage.py and matched
    against the kernels it finds compiled in csrc/bev_metrics.hip."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_coverage as kc
    prof = os.path.join(kc.ROCM, "bin", "rocprofv3")
    prof = prof if os.path.exists(prof) else shutil.which("rocprofv3")
    assert prof, "rocprofv3 not found"
    script = tmp_path / "one_assign.py"
    script.write_text(SCRIPT.format(pkg=PKG))
    run = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path / "kt"), "-o", "run",
                          "--", sys.executable, str(script)], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    traces = glob.glob(str(tmp_path / "kt" / "**" / "*kernel_trace.csv"), recursive=True)
    assert traces, os.listdir(tmp_path / "kt")
    launched = kc.read_launches(open(traces[0], newline=""))
    src = os.path.join(PKG, "csrc", "bev_metrics.hip")
    compiled = kc.kernels_from_symbols("bev_metrics.hip", kc.compiled_symbols(src))
    rows = {n: c for _, n, c, _ in kc.match(compiled, launched)}
    mine = [n for n in rows if n.startswith("k_det_assign(")]
    assert len(mine) == 1 and rows[mine[0]] == 1, (rows, list(launched)[:20])
    assert [n for n in rows if n.startswith("k_det_match(")] and len(rows) == 2
