"""Validation scoring, host side (no GPU): bev_detection_match_host (the per-pair arithmetic of csrc/bev_metrics.h
compiled for the CPU) and utils/metrics.py on CPU tensors, against

  * tests/golden/metrics_cases.npz, recorded from the reference's own compute_metrics (train.py:78-104) on inputs
    whose decisions a 1-ulp difference between torch.norm and sqrtf(dx dx + dy dy) cannot flip
    (tests/golden/make_metrics_golden.py asserts that): the three counts exactly, precision / recall / F1 as bit-equal
    doubles, the mean localisation error within relative 2^-22 (each matched distance is within 1 ulp, <= 2^-23
    relative, of torch's, so their mean is; the factor 2 is margin for the double arithmetic);
  * a numpy float32 restatement of the matching rule in this file's own words, bit for bit (counts and the double
    sums), on seeded random frames -- among them frames on a coarse lattice, full of exact ties and of distances equal
    to the threshold, which the fixture's margins exclude;

and the epoch accumulator, the threshold rule, the C entries' argument rules, the ABI number and a two-rank gloo run."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import bev_native
from conftest import GOLDEN, PKG
from utils.metrics import DetectionMetrics, compute_metrics, metrics_from_totals

F = np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(bev_native.LIB_PATH):
        bev_native.build()
    return bev_native.lib()


def load_cases():
    """name -> (preds: list of [K, 4] float32 arrays | None, gts: list of [G, 4] arrays | None (no 'boxes_world'),
    match_dist, (precision, recall, f1, mle), (tp, fp, fn))"""
    d = np.load(os.path.join(GOLDEN, "metrics_cases.npz"))
    pred, gt = d["pred"].view(F), d["gt"].view(F)
    md, prf = d["match_dist"].view(np.float64), d["prf"].view(np.float64)
    out, f, ip, ig = {}, 0, 0, 0
    for c, name in enumerate(d["names"].tolist()):
        preds, gts = [], []
        for _ in range(int(d["frames"][c])):
            k, g = int(d["pred_count"][f]), int(d["gt_count"][f])
            f += 1
            preds.append(None if k < 0 else pred[ip:ip + k])
            gts.append(None if g < 0 else gt[ig:ig + g])
            ip, ig = ip + max(k, 0), ig + max(g, 0)
        out[name] = (preds, gts, float(md[c]), tuple(prf[c].tolist()), tuple(int(v) for v in d["counts"][c]))
    assert ip == len(pred) and ig == len(gt)
    seq = [d["names"][i] for i in d["seq"]]
    return out, seq, d["seq_means"].view(np.float64).tolist(), [int(v) for v in d["seq_counts"]]


CASES, SEQ, SEQ_MEANS, SEQ_COUNTS = load_cases()


def as_torch(preds, gts, device="cpu"):
    tp = [None if p is None else torch.from_numpy(p.copy()).to(device) for p in preds]
    tg = [{} if g is None else {"boxes_world": torch.from_numpy(g.copy()).to(device)} for g in gts]
    return tp, tg


def pack(preds, gts, cap=None):
    """The C entries' layout: pred [B, cap, 4], pred_count [B], gt_xy [N, 2], gt_offset [B + 1]."""
    ks = [0 if p is None else len(p) for p in preds]
    cap = max(ks, default=0) if cap is None else cap
    pred = np.zeros((len(preds), cap, 4), F)
    for b, p in enumerate(preds):
        if ks[b]:
            pred[b, :ks[b]] = p
    gs = [0 if g is None else len(g) for g in gts]
    xy = np.concatenate([np.asarray(g, F).reshape(-1, 4)[:, :2] for g in gts if g is not None and len(g)]
                        + [np.zeros((0, 2), F)])
    offset = np.concatenate([[0], np.cumsum(gs)]).astype(np.int32)
    return pred, np.asarray(ks, np.int32), np.ascontiguousarray(xy), offset


def check_tuple(got, prf, counts, name):
    assert tuple(got[4:]) == counts, (name, got, counts)
    for k in range(3):
        assert np.float64(got[k]).view(np.uint64) == np.float64(prf[k]).view(np.uint64), (name, k, got, prf)
    assert abs(got[3] - prf[3]) <= 2.0 ** -22 * abs(prf[3]), (name, got[3], prf[3])
    assert all(type(v) is float for v in got[:4]) and all(type(v) is int for v in got[4:]), (name, got)


def test_fixture_holds_the_cases_the_rule_needs():
    assert len(CASES) >= 20
    assert CASES["nan_ground_truth"][4] == (0, 1, 2)  # a NaN ground truth poisons its frame
    assert CASES["distance_equals_half"][4] == (3, 1, 1) and CASES["unrepresentable_threshold"][4] == (2, 1, 1)
    assert any(p is None for p in CASES["none_entry_and_missing_key"][0])
    assert any(g is None for g in CASES["none_entry_and_missing_key"][1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_compute_metrics_cpu_against_reference(lib, name):
    preds, gts, m, prf, counts = CASES[name]
    check_tuple(compute_metrics(*as_torch(preds, gts), match_dist=m), prf, counts, name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_entry_against_reference(lib, name):
    preds, gts, m, prf, counts = CASES[name]
    c, s = bev_native.detection_match_host(*pack(preds, gts), m)
    assert c.dtype == np.int32 and s.dtype == np.float64 and not c[:, 3].any()
    total = 0.0
    for v in s.tolist():
        total += v
    tp, fp, fn = (int(c[:, k].sum()) for k in range(3))
    check_tuple(metrics_from_totals(tp, fp, fn, total), prf, counts, name)


def test_default_match_dist_is_the_references(lib):
    preds, gts, m, prf, counts = CASES["contested_ground_truth"]
    assert m == 0.5
    check_tuple(compute_metrics(*as_torch(preds, gts)), prf, counts, "default")


# ---- the rule in this file's own words (numpy float32) --------------------------------------------------------------
def first_min(d):
    """torch.min(d, dim=0): the first NaN if there is one, else the first smallest."""
    nan = np.flatnonzero(np.isnan(d))
    if len(nan):
        return d[nan[0]], int(nan[0])
    j = int(np.flatnonzero(d == d.min())[0])
    return d[j], j


def restated(pred, count, xy, offset, match_dist):
    """Frame by frame, prediction by prediction: counts [B, 4] int32 and the matched distances' double sum."""
    B = len(count)
    counts, sums = np.zeros((B, 4), np.int32), np.zeros(B, np.float64)
    thr = np.float64(match_dist)
    with np.errstate(all="ignore"):
        for b in range(B):
            if count[b] < 0:
                counts[b, 3] = -1
                continue
            g = xy[offset[b]:offset[b + 1]]
            taken = np.zeros(len(g), bool)
            total = np.float64(0)
            for i in range(min(int(count[b]), pred.shape[1])):
                if len(g) == 0:
                    counts[b, 1] += 1
                    continue
                ex, ey = g[:, 0] - pred[b, i, 0], g[:, 1] - pred[b, i, 1]
                sq_x, sq_y = ex * ex, ey * ey  # float32 arrays: every operation rounds by itself
                d, j = first_min(np.sqrt(sq_x + sq_y))
                if np.float64(d) <= thr and not taken[j]:  # the float32 distance widened, against the double
                    taken[j] = True
                    counts[b, 0] += 1
                    total = total + np.float64(d)
                else:
                    counts[b, 1] += 1
            counts[b, 2] = (~taken).sum()
            sums[b] = total
    return counts, sums


def random_batch(rng, style):
    B = int(rng.integers(1, 4))
    preds, gts = [], []
    for _ in range(B):
        K, G = int(rng.integers(0, 40)), int(rng.integers(0, 30))
        if style == "lattice":  # quarter-metre lattice: exact ties, distances exactly 0.25 / 0.5 / 0.625 / ...
            p = rng.integers(-8, 9, (K, 4)).astype(F) * F(0.25)
            g = rng.integers(-8, 9, (G, 4)).astype(F) * F(0.25)
        else:
            g = rng.uniform(-10, 10, (G, 4)).astype(F)
            p = rng.uniform(-10, 10, (K, 4)).astype(F)
            for i in range(min(K, G)):
                p[i, :2] = g[int(rng.integers(0, G)), :2] + rng.normal(0, 0.3, 2).astype(F)
            if style == "nonfinite" and K and G:
                for arr in (p, g):
                    for v in (NAN, INF, -INF):
                        if rng.random() < 0.4:
                            arr[int(rng.integers(0, len(arr))), int(rng.integers(0, 2))] = v
        preds.append(p)
        gts.append(g)
    return preds, gts


@pytest.mark.parametrize("style", ["plain", "lattice", "nonfinite"])
def test_host_entry_equals_the_restated_rule_bit_for_bit(lib, style):
    rng = np.random.default_rng({"plain": 3, "lattice": 4, "nonfinite": 5}[style])
    tp = ties = 0
    for trial in range(40):
        preds, gts = random_batch(rng, style)
        m = [0.5, 0.3, 0.625, 0.25, 1.0, float(F(0.3)), 0.0][trial % 7]
        a = pack(preds, gts)
        if trial % 5 == 0 and len(a[1]) > 1:
            a[1][1] = -1  # the decode's "large path" mark in one frame
        got = bev_native.detection_match_host(*a, m)
        want = restated(*a, m)
        assert np.array_equal(got[0], want[0]), (style, trial, got[0], want[0])
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), (style, trial)
        tp += int(got[0][:, 0].sum())
    assert tp > 40, tp  # the comparison is not vacuous


def test_long_frames_and_padding(lib):
    """G beyond one on-chip chunk (1024), K beyond a workgroup (256), cap beyond the counts: rows past a frame's count
    are never read."""
    rng = np.random.default_rng(11)
    g = rng.uniform(-30, 30, (1100, 4)).astype(F)
    p = (g[rng.permutation(1100)[:300]] + rng.normal(0, 0.2, (300, 4))).astype(F)
    a = pack([p, p[:7]], [g, g[:3]], cap=320)
    a[0][0, 300:] = NAN
    a[0][1, 7:] = 1e30
    got, want = bev_native.detection_match_host(*a, 0.5), restated(*a, 0.5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    assert got[0][0, 0] > 100


def test_threshold_is_the_largest_float32_not_above_match_dist(lib):
    thr = bev_native.match_thr32
    below, at = float(np.nextafter(F(0.3), F(0))), float(F(0.3))
    assert below < 0.3 < at and thr(0.3) == below          # float32(0.3) rounds up: the threshold steps down
    assert thr(0.5) == 0.5 and thr(at) == at and thr(0.7) == float(F(0.7)) < 0.7  # float32(0.7) rounds down: kept
    assert thr(INF) == INF and thr(1e300) == float(np.finfo(F).max) and np.isnan(thr(NAN))
    for m, d, tp in ((0.3, at, 0), (0.3, below, 1), (at, at, 1), (0.7, float(F(0.7)), 1),
                     (0.7, float(np.nextafter(F(0.7), F(1))), 0), (NAN, 0.0, 0), (INF, 3.0, 1)):
        c, s = bev_native.detection_match_host(*pack([np.zeros((1, 4), F)], [np.asarray([[d, 0, 1, 1]], F)]), m)
        assert c.tolist() == [[tp, 1 - tp, 1 - tp, 0]], (m, d, c)
        assert s[0] == (d if tp else 0.0)


def test_detection_metrics_over_the_three_batch_sequence(lib):
    val = DetectionMetrics(match_dist=0.5)
    assert val.result() == (0.0, 0.0, 0.0, 0.0, 0, 0, 0)  # train.py:299-302 with no batch: 0 / max(1, 0)
    for name in SEQ:
        preds, gts, m, _, _ = CASES[name]
        assert val.update(*as_torch(preds, gts)) is None
    got = val.result()
    assert tuple(got[4:]) == tuple(SEQ_COUNTS)
    for k in range(3):
        assert np.float64(got[k]).view(np.uint64) == np.float64(SEQ_MEANS[k]).view(np.uint64), (k, got, SEQ_MEANS)
    assert abs(got[3] - SEQ_MEANS[3]) <= 2.0 ** -22 * SEQ_MEANS[3]
    assert val.in_flight() == 0 and val.result() == got  # result() does not consume
    val.reset()
    assert val.result()[4:] == (0, 0, 0)


def _match_args(null=(), host=False, **kw):
    """One accepted argument set for the C entries (host buffers: the device entry must refuse before it touches
    them), with the named pointers nulled and the named scalars replaced."""
    a = dict(B=2, cap=3, N=4, thr32=0.5, workspace_bytes=0)
    a.update(kw)
    bufs = dict(pred=np.zeros((2, 3, 4), F), pred_count=np.asarray([3, 1], np.int32), gt_xy=np.zeros((4, 2), F),
                gt_offset=np.asarray(kw.pop("offsets", [0, 3, 4]), np.int32), counts=np.full((2, 4), 7, np.int32),
                dist_sum=np.full(2, 7.0), workspace=np.zeros(8192, np.int32))
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in bufs.items()}
    args = [p["pred"], p["pred_count"], a["B"], a["cap"], p["gt_xy"], p["gt_offset"], a["N"], a["thr32"], p["counts"],
            p["dist_sum"]]
    if not host:
        args += [p["workspace"], a["workspace_bytes"], None]
    return args, bufs


def test_argument_rules(lib):
    wsb = lib.bev_detection_match_workspace_bytes
    assert wsb(2, 0) == 0 and wsb(2, 1024) == 0 and wsb(2, 1025) == 1025 * 4
    assert wsb(0, 5000) == 0 and wsb(-1, 5000) == 0
    for entry, host in ((lib.bev_detection_match_f32, False), (lib.bev_detection_match_host, True)):
        refused = [dict(null=(k,)) for k in ("pred", "pred_count", "gt_xy", "gt_offset", "counts", "dist_sum")]
        refused += [dict(B=-1), dict(cap=-1), dict(N=-1)]
        if host:
            refused += [dict(offsets=o) for o in ([0, 3, 2], [-1, 3, 4], [0, 3, 5], [3, 1, 4])]
        else:  # N past the on-chip table needs the workspace
            refused += [dict(N=1025, workspace_bytes=1025 * 4, null=("workspace",)),
                        dict(N=1025, workspace_bytes=1025 * 4 - 1), dict(N=1025, workspace_bytes=0)]
        for kw in refused:
            a, bufs = _match_args(host=host, **kw)
            assert entry(*a) == bev_native.BEV_ERR_ARGS == -1, (host, kw)
            assert (bufs["counts"] == 7).all() and (bufs["dist_sum"] == 7).all(), (host, kw)  # refused: nothing written
        a, bufs = _match_args(host=host, B=0, null=("pred", "pred_count", "gt_xy", "gt_offset", "counts", "dist_sum",
                                                    "workspace"))
        assert entry(*a) == 0  # B == 0: nothing to do
    # null pred / gt_xy are fine when there is nothing to read
    a, bufs = _match_args(host=True, cap=0, null=("pred",))
    assert lib.bev_detection_match_host(*a) == 0 and bufs["counts"].tolist() == [[0, 0, 3, 0], [0, 0, 1, 0]]
    a, bufs = _match_args(host=True, N=0, null=("gt_xy",), offsets=[0, 0, 0])
    assert lib.bev_detection_match_host(*a) == 0 and bufs["counts"].tolist() == [[0, 3, 0, 0], [0, 1, 0, 0]]
    assert not bufs["dist_sum"].any()


def test_abi_number_unchanged(lib):
    assert lib.bev_abi_version() == bev_native.ABI_VERSION == 18
    for name in ("bev_detection_match_f32", "bev_detection_match_host", "bev_detection_match_workspace_bytes"):
        assert name in bev_native.SIGNATURES and hasattr(lib, name)


def test_python_surface(lib):
    with pytest.raises(ValueError):
        bev_native.detection_match_host(np.zeros((1, 2, 3), F), np.zeros(1, np.int32), np.zeros((0, 2), F),
                                        np.zeros(2, np.int32), 0.5)
    with pytest.raises(ValueError):
        bev_native.detection_match_host(np.zeros((1, 2, 4), F), np.zeros(1, np.int32), np.zeros((2, 2), F),
                                        np.asarray([0, 3], np.int32), 0.5)  # offsets past N
    with pytest.raises(bev_native.HipError):  # no CPU fallback behind the device entry
        bev_native.detection_match(torch.zeros(1, 2, 4), torch.zeros(1, dtype=torch.int32), torch.zeros(0, 2),
                                   torch.zeros(2, dtype=torch.int32), 0.5)
    raw = bev_native.DecodeBuffers("boxes", "kept", "stream", "ready")
    pending = bev_native._PendingDecode(lambda: (["b"], ["s"]), raw)
    dets = bev_native.DetectionList(pending, 0)
    assert dets.pending is pending and pending.raw is raw and not pending.materialised
    assert list(dets) == ["b"] and pending.materialised and pending.raw is raw
    with pytest.raises(ValueError):  # fewer prediction entries than frames
        compute_metrics([torch.zeros(1, 4)], [{}, {}])


# ---- two ranks ----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import sys
    sys.path.insert(0, PKG)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        val = DetectionMetrics(0.5)
        for name in SEQ[rank::world]:
            preds, gts, _, _, _ = CASES[name]
            val.update(*as_torch(preds, gts))
        q.put((rank, val.result(group=dist.group.WORLD), val.result()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_return_identical_results(lib):
    import torch.multiprocessing as mp
    from conftest import gather_results
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (everyone, own) for r, everyone, own in gather_results(procs, q, 2, 240)}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[0][0] == res[1][0]  # every rank: the same numbers, bit for bit
    assert res[0][1] != res[1][1]  # ... from different batches
    got = res[0][0]
    order = SEQ[0::2] + SEQ[1::2]  # rank order, then batch order
    assert tuple(got[4:]) == tuple(SEQ_COUNTS)
    for k in range(3):
        want = sum(CASES[n][3][k] for n in order) / 3
        assert np.float64(got[k]).view(np.uint64) == np.float64(want).view(np.uint64), (k, got, want)
    want = sum(CASES[n][3][3] for n in order) / 3
    assert abs(got[3] - want) <= 2.0 ** -22 * want
