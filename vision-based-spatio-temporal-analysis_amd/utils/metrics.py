"""Validation scoring of the reference's loop (train.py:78-104 `compute_metrics`, :291-309 the epoch means) without a
host synchronisation per detection.

The reference walks every prediction of every frame in Python and reads `min_dist.item()` for each; on device
detections that drains the GPU once per prediction.  Here a batch is one native launch (bev_native.detection_match,
csrc/bev_metrics.hip) on the decode's own buffers:

    from utils.metrics import compute_metrics            # the reference's function, one wait per batch
    p, r, f1, mle, tp, fp, fn = compute_metrics(preds['boxes'], batch['targets'], match_dist=0.5)

    from utils.metrics import DetectionMetrics           # no wait per batch at all
    val = DetectionMetrics(match_dist=0.5)
    for batch in dl_val:
        val.update(model(batch)['boxes'], batch['targets'])
    mean_p, mean_r, mean_f1, mean_mle, tps, fps, fns = val.result()

The matching rule is the reference's (include/bev_mi355x.h, bev_detection_match_f32).  What is this library's own
definition: the distance of a pair is sqrtf(dx dx + dy dy) with separately rounded fp32 operations (torch.norm may
differ from it by 1 ulp), and a batch's distance sum is the frames' sums (each added in prediction order, in double)
added in frame order, where the reference adds one flat list -- the same number up to double rounding.

All-CPU inputs are scored by the library's host entry (the same arithmetic, no GPU needed).

MODA / MODP / precision / recall -- what Wildtrack tables report -- need the frame's optimal one-to-one matching, not
the greedy walk (a prediction whose nearest ground truth is taken is a false positive there even when another lies
within range).  The same two shapes, one native launch per batch (bev_native.detection_assign):

    from utils.metrics import compute_mod_metrics
    m = compute_mod_metrics(preds['boxes'], batch['targets'], match_dist=0.5)   # {'moda': ..., 'modp': ..., ...}

    val = DetectionMetrics(match_dist=0.5, matching="optimal")
    for batch in dl_val:
        val.update(model(batch)['boxes'], batch['targets'])
    m = val.result_mod()                                   # from the epoch's totals, in percent; waits once

The matching: the most pairs with distance <= match_dist (the project's <=; MVDet's script uses <, so a pair at
exactly the threshold counts here and adds 0 to MODP), each prediction and ground truth used at most once, and among
those the smallest distance sum (include/bev_mi355x.h, bev_detection_assign_f32).  A frame beyond the device path's
1024 x 1024 is finished by the host entry when the result is read.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

import bev_native as _nat


def metrics_from_totals(tp: int, fp: int, fn: int, dist_sum: float):
    """train.py:100-104 from a batch's totals -> (precision, recall, f1, mle, tp, fp, fn)."""
    precision = tp / max(1, tp + fp)
    recall = tp / max(1, tp + fn)
    f1 = 2 * precision * recall / max(1e-6, precision + recall)
    mle = float(dist_sum / max(1, tp))
    return precision, recall, f1, mle, tp, fp, fn


def mod_from_totals(tp: int, fp: int, fn: int, dist_sum: float, match_dist: float) -> Dict:
    """MODA / MODP / precision / recall in percent from totals over any set of frames (include/bev_mi355x.h):
    MODA = 100 (1 - (FP + FN) / GT) may be negative; MODP = 100 mean(1 - d / match_dist) over the matches."""
    gt = tp + fn
    over = float(dist_sum) / match_dist if dist_sum else 0.0
    return {"moda": 100.0 * (1.0 - (fp + fn) / max(1, gt)), "modp": 100.0 * (tp - over) / max(1, tp),
            "precision": 100.0 * tp / max(1, tp + fp), "recall": 100.0 * tp / max(1, gt),
            "tp": tp, "fp": fp, "fn": fn, "gt": gt}


def _totals(rows: np.ndarray):
    """[B, 5] float64 rows (tp, fp, fn, status, dist_sum) -> (tp, fp, fn, sum), the frames' sums added in frame order."""
    s = 0.0
    for v in rows[:, 4].tolist():
        s += v
    return int(rows[:, 0].sum()), int(rows[:, 1].sum()), int(rows[:, 2].sum()), s


def _gt_centres(gt_targets: Sequence[Dict]) -> List[Optional[torch.Tensor]]:
    """Per frame the [G, 2] fp32 view of boxes_world's first two columns, None for a missing or empty entry
    (centers_world is not consulted, as in the reference)."""
    out = []
    for tgt in gt_targets:
        bx = tgt.get("boxes_world", None)
        if bx is None or bx.numel() == 0:
            out.append(None)
            continue
        bx = torch.as_tensor(bx)
        out.append(bx.reshape(-1, bx.shape[-1])[:, :2].to(torch.float32))
    return out


def _pred_rows(pred_boxes, B: int) -> List[torch.Tensor]:
    if len(pred_boxes) < B:
        raise ValueError(f"compute_metrics: {len(pred_boxes)} prediction entries for {B} frames")
    out = []
    for b in range(B):
        p = pred_boxes[b]
        if p is None:
            p = torch.zeros(0, 4)
        p = torch.as_tensor(p)
        out.append(p.reshape(-1, p.shape[-1])[:, :4].to(torch.float32) if p.numel() else torch.zeros(0, 4))
    return out


def _pack_gt_device(gts, dev):
    """gt_xy [N, 2] fp32 and gt_offset [B + 1] int32 on `dev`.  Host boxes -- how the loader hands them over -- travel
    with the offsets in one pinned, asynchronous copy (the counts are shapes: known without the device)."""
    sizes = [0 if g is None else g.shape[0] for g in gts]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N, live = int(offs[-1]), [g for g in gts if g is not None]
    if all(not g.is_cuda for g in live):
        buf = torch.empty(2 * N + len(offs), dtype=torch.int32).pin_memory()
        if N:
            buf[:2 * N].view(torch.float32).view(N, 2).copy_(torch.cat(live))
        buf[2 * N:] = torch.from_numpy(offs)
        d = buf.to(dev, non_blocking=True)
        return d[:2 * N].view(torch.float32).view(N, 2), d[2 * N:]
    xy = torch.cat([g.to(dev) for g in live]).contiguous()
    return xy, torch.from_numpy(offs).pin_memory().to(dev, non_blocking=True)


def _pack_pred_device(rows, dev):
    """A list of [K, 4] -> pred [B, cap, 4] (cap = the longest frame) and pred_count [B] int32 on `dev`, packed once."""
    kept = torch.tensor([r.shape[0] for r in rows], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    if not rows:
        return torch.zeros(0, 0, 4, device=dev), kept
    rows = [r.to(dev, non_blocking=True) for r in rows]
    return torch.nn.utils.rnn.pad_sequence(rows, batch_first=True).contiguous(), kept


# matching rule -> (device entry, host entry): the same buffers, results and status codes
_RULES = {"greedy": (_nat.detection_match, _nat.detection_match_host),
          "optimal": (_nat.detection_assign, _nat.detection_assign_host)}


def _rule(matching: str):
    if matching not in _RULES:
        raise ValueError(f"matching must be one of {sorted(_RULES)}, got {matching!r}")
    return _RULES[matching]


def _rows(counts, dist_sum) -> torch.Tensor:
    return torch.cat([counts.to(torch.float64), dist_sum[:, None]], dim=1)


class _Batch:
    """One queued batch: its rows arrive in pinned memory behind an event; until they are read the batch keeps what
    a re-run needs (the pending decode and the packed buffers the launch read)."""

    def __init__(self, match_dist, matching="greedy"):
        self.match_dist = match_dist
        self.on_device, self.on_host = _rule(matching)
        self.rows = None      # [B, 5] float64 once known
        self.event = self.pinned = self.pending = self.inputs = None

    def queue_device(self, pred, kept, gt_xy, gt_offset):
        self.inputs = (pred, kept, gt_xy, gt_offset)
        counts, dist_sum = self.on_device(*self.inputs, self.match_dist)
        B = counts.shape[0]
        self.pinned = torch.empty(B, 5, dtype=torch.float64).pin_memory()
        self.pinned.copy_(_rows(counts, dist_sum), non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(pred.device))

    def done(self) -> bool:
        """Known without waiting?  (A batch with a frame on the decode's large path, or one too large for the device
        matching, stays queued for finish().)"""
        if self.rows is None and self.event.query() and not (self.pinned[:, 3] != 0).any():
            self._settle(self.pinned.numpy().copy())
        return self.rows is not None

    def finish(self):
        if self.rows is not None:
            return self.rows
        self.event.synchronize()
        rows = self.pinned.numpy().copy()
        if (rows[:, 3] == _nat.MATCH_STATUS_PENDING).any():
            # the decode left a frame to its large path, which needs a host round trip: materialise, score again
            if self.pending is None:
                raise _nat.HipError("detection metrics: a negative prediction count without a pending decode")
            self.pending.get()
            raw = self.pending.raw
            self.inputs = (raw.boxes, raw.kept) + self.inputs[2:]
            rows = _rows(*self.on_device(*self.inputs, self.match_dist)).cpu().numpy()
        if (rows[:, 3] == _nat.MATCH_STATUS_TOO_LARGE).any():
            # frames beyond the device matching: the host entry, the same procedure, frame by frame
            pred, kept, gt_xy, gt_offset = self.inputs
            kept, offs = kept.cpu().numpy(), gt_offset.cpu().numpy()
            for b in np.flatnonzero(rows[:, 3] == _nat.MATCH_STATUS_TOO_LARGE).tolist():
                k = min(int(kept[b]), pred.shape[1])
                g = gt_xy[int(offs[b]):int(offs[b + 1])].cpu().numpy()
                counts, dist_sum = self.on_host(pred[b:b + 1, :k].cpu().numpy(), np.asarray([k], np.int32), g,
                                                np.asarray([0, len(g)], np.int32), self.match_dist)
                rows[b, :4], rows[b, 4] = counts[0], dist_sum[0]
        if (rows[:, 3] != 0).any():
            raise _nat.HipError(f"detection metrics: frames left with status {rows[:, 3].astype(int).tolist()}")
        return self._settle(rows)

    def _settle(self, rows):
        self.rows = rows
        self.event = self.pinned = self.pending = self.inputs = None  # the decode's buffers are free to go
        return rows


def _queue(pred_boxes, gt_targets, match_dist, matching="greedy") -> _Batch:
    B = len(gt_targets)
    gts = _gt_centres(gt_targets)
    batch = _Batch(float(match_dist), matching)
    lazy = isinstance(pred_boxes, _nat.DetectionList)
    rows = None if lazy else _pred_rows(pred_boxes, B)
    dev = None
    if lazy:
        dev = pred_boxes.pending.raw.boxes.device
    else:
        dev = next((t.device for t in rows + [g for g in gts if g is not None] if t.is_cuda), None)
    if dev is None:  # all on the host: the library's host entry
        cap = max([r.shape[0] for r in rows], default=0)
        pred = np.zeros((B, cap, 4), np.float32)
        for b, r in enumerate(rows):
            pred[b, :r.shape[0]] = r.numpy()
        sizes = [0 if g is None else g.shape[0] for g in gts]
        xy = np.concatenate([g.numpy() for g in gts if g is not None] + [np.zeros((0, 2), np.float32)])
        counts, dist_sum = batch.on_host(pred, np.asarray([r.shape[0] for r in rows], np.int32), xy,
                                         np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), batch.match_dist)
        batch.rows = np.concatenate([counts.astype(np.float64), dist_sum[:, None]], axis=1)
        return batch
    with torch.cuda.device(dev):
        gt_xy, gt_offset = _pack_gt_device(gts, dev)
        if lazy:
            raw = pred_boxes.pending.raw
            if raw.boxes.shape[0] != B:
                raise ValueError(f"compute_metrics: the decode holds {raw.boxes.shape[0]} frames, the targets {B}")
            here = torch.cuda.current_stream(dev)
            if here != raw.stream:
                here.wait_event(raw.ready)
            batch.pending = pred_boxes.pending
            batch.queue_device(raw.boxes, raw.kept, gt_xy, gt_offset)
        else:
            batch.queue_device(*_pack_pred_device(rows, dev), gt_xy, gt_offset)
    return batch


def compute_metrics(pred_boxes, gt_targets, match_dist=0.5):
    """train.py:78 `compute_metrics`: pred_boxes a List[Tensor[K, 4] | None] on either device or the DetectionList of
    `BEVDetector.decode(..., lazy=True)` (its buffers are read in place, nothing is materialised), gt_targets the
    loader's List[Dict] ('boxes_world' on host or device, missing or empty) -> (precision, recall, f1, mle, tp, fp,
    fn) as Python numbers.  One native launch and one host wait for the batch; none of either for all-CPU inputs."""
    return metrics_from_totals(*_totals(_queue(pred_boxes, gt_targets, match_dist).finish()))


def compute_mod_metrics(pred_boxes, gt_targets, match_dist=0.5) -> Dict:
    """MODA / MODP / precision / recall (percent) and tp / fp / fn / gt of a batch under the optimal one-to-one
    matching at match_dist (include/bev_mi355x.h, bev_detection_assign_f32), from the inputs of compute_metrics: one
    native launch and one host wait for the batch; none of either for all-CPU inputs."""
    match_dist = float(match_dist)
    return mod_from_totals(*_totals(_queue(pred_boxes, gt_targets, match_dist, "optimal").finish()), match_dist)


class DetectionMetrics:
    """The validation epoch of train.py:272-309 without a host wait per batch: `update` queues a batch's scoring
    behind its decode and returns, `result` waits once and gives the epoch's numbers.  matching: "greedy", the
    reference's rule, or "optimal", the one-to-one assignment MODA / MODP are defined on (`result_mod`)."""

    def __init__(self, match_dist: float = 0.5, matching: str = "greedy"):
        _rule(matching)
        self.match_dist = float(match_dist)
        self.matching = matching
        self._batches: List[_Batch] = []

    def reset(self):
        self._batches = []

    def update(self, pred_boxes, gt_targets):
        """Queue one batch; never waits for the device.  Earlier batches whose results have arrived (a non-blocking
        query) let go of their decode buffers here, so only batches in flight keep theirs alive."""
        for b in self._batches:
            b.done()
        self._batches.append(_queue(pred_boxes, gt_targets, self.match_dist, self.matching))

    def in_flight(self) -> int:
        """Batches that still hold device buffers."""
        return sum(b.rows is None for b in self._batches)

    def _batch_totals(self, group):
        """Per batch (tp, fp, fn, sum); with `group` every rank's, in rank order, then batch order.  Waits."""
        totals = [_totals(b.finish()) for b in self._batches]
        if group is not None:
            import torch.distributed as dist
            every = [None] * dist.get_world_size(group)
            dist.all_gather_object(every, totals, group=group)
            totals = [t for rank in every for t in rank]
        return totals

    def result(self, group=None):
        """(mean_p, mean_r, mean_f1, mean_mle, tps, fps, fns) as train.py:299-309 computes them: the means of the
        per-batch values, the sums of the counts.  `group`: a torch.distributed process group whose ranks each hold
        part of the batches -- the per-batch totals are all-gathered and taken in rank order, then batch order, so
        every rank returns the same numbers."""
        per = [metrics_from_totals(*t) for t in self._batch_totals(group)]
        n = max(1, len(per))
        mean = lambda k: sum(m[k] for m in per) / n  # noqa: E731
        return (mean(0), mean(1), mean(2), mean(3), sum(m[4] for m in per), sum(m[5] for m in per),
                sum(m[6] for m in per))

    def result_mod(self, group=None) -> Dict:
        """{moda, modp, precision, recall (percent), tp, fp, fn, gt} from the epoch's totals under the optimal
        matching; `group` as in `result`.  Only for matching="optimal": MODA from a greedy matching is not the
        metric."""
        if self.matching != "optimal":
            raise ValueError('result_mod needs DetectionMetrics(matching="optimal")')
        tp = fp = fn = 0
        dist_sum = 0.0
        for t in self._batch_totals(group):
            tp, fp, fn, dist_sum = tp + t[0], fp + t[1], fn + t[2], dist_sum + t[3]
        return mod_from_totals(tp, fp, fn, dist_sum, self.match_dist)
