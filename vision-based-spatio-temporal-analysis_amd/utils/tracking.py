"""Online tracking of the BEV detections: the reference's README, phase 3 -- "a light online tracker (a SORT or DeepSORT
variant) ... pedestrian trajectories with time and ID" -- which the reference has no code for.

A SORT-style tracker on ground-plane points (csrc/bev_track.h: constant-velocity Kalman tracks, the optimal gated
matching of the MODA / MODP scoring between predicted positions and detections, deletion after max_age misses, birth
from unmatched detections, SORT's min_hits reporting).  A batch -- consecutive frames of one sequence -- is one native
launch (bev_native.track_step) queued behind the decode on its own buffers; the tracker's state stays on the device
from launch to launch and the host waits for nothing until a result is read:

    from utils.tracking import BEVTracker
    tracker = BEVTracker(gate=1.0)
    for batch in dl:
        res = tracker.update(model(batch)['boxes'])      # queued; returns at once
        save_tracks_json(boxes, scores, res.ids, out_dir, batch['frame_idx'])   # res.ids waits, once

All-CPU detections go to the library's host entry: the same procedure, the same bits, no GPU needed.

A frame whose decode was left to its large path (more candidates than the on-chip sort holds) has no detection count
on the device until the host finishes it, and a tracker cannot skip a frame.  The launch marks that frame pending,
the later ones stalled, and leaves the state as the frame before left it; when a result is read the tracker
materialises that decode, runs the launch again from that frame, and replays, in order, every later batch that was
queued meanwhile.  Until then those batches keep their buffers.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

import bev_native as _nat

_HELD = _nat.TRACK_STATUS_PENDING | _nat.TRACK_STATUS_STALLED


def _rows(pred_boxes) -> List[torch.Tensor]:
    out = []
    for p in pred_boxes:
        if p is None:
            out.append(torch.zeros(0, 4))
            continue
        p = torch.as_tensor(p)
        out.append(p.reshape(-1, p.shape[-1])[:, :4].to(torch.float32) if p.numel() else torch.zeros(0, 4))
    return out


class TrackResult:
    """The tracks of one batch.  ids: per frame an int32 [K_b] array, the track id of every detection (-1: none yet);
    tracks: per frame a float32 [K_b, 4] array, that track's (x, y, vx, vy) in metres and metres per frame after the
    frame's update; info: int32 [B, 4] (bev_native.TRACK_INFO: status, live tracks, born, dropped).  numpy arrays on
    the host; the first read waits for the launch, once."""

    def __init__(self, tracker, B):
        self._tracker, self.frames = tracker, B
        self._ids = self._tracks = self._info = None   # host arrays once settled
        # while queued on the device
        self._pending = self._inputs = self._dev = self._pinned = self._event = None

    def _read(self):
        if self._ids is None:
            self._tracker._settle(self)
        return self

    @property
    def settled(self) -> bool:
        return self._ids is not None

    @property
    def ids(self) -> List[np.ndarray]:
        return self._read()._ids

    @property
    def tracks(self) -> List[np.ndarray]:
        return self._read()._tracks

    @property
    def info(self) -> np.ndarray:
        return self._read()._info

    # -- device side -------------------------------------------------------------------------------------------
    def _launch(self, first=0):
        """Queue the launch on the current stream, and the copies of its results to pinned memory behind it."""
        t = self._tracker
        pred, kept = self._inputs
        ids, tracks, info = _nat.track_step(pred, kept, t.params, t._state, first=first)
        if self._pinned is None:
            n = ids.shape[1]
            self._pinned = (torch.empty(self.frames, n, dtype=torch.int32).pin_memory(),
                            torch.empty(self.frames, n, 4, dtype=torch.float32).pin_memory(),
                            torch.empty(self.frames, 4, dtype=torch.int32).pin_memory(),
                            torch.empty(self.frames, dtype=torch.int32).pin_memory())
        for dst, src in zip(self._pinned, (ids, tracks, info, kept)):
            dst[first:].copy_(src[first:], non_blocking=True)
        self._dev = (ids, tracks, info)  # alive until the copies have run
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(pred.device))

    def _clean(self) -> bool:
        """Arrived, and every frame tracked?  (No wait.)"""
        return self._event.query() and not (self._pinned[2][:, 0] & ~_nat.TRACK_STATUS_TRUNCATED).any()

    def _finish(self) -> bool:
        """Wait for the batch and complete it; True when a frame had to be replayed."""
        t = self._tracker
        replayed = False
        for _ in range(self.frames + 1):  # every round completes at least one more frame
            self._event.synchronize()
            status = self._pinned[2][:, 0].numpy()
            other = status & ~(_HELD | _nat.TRACK_STATUS_TRUNCATED)
            if other.any():
                raise _nat.HipError(f"BEVTracker: frames left with status {status.tolist()}")
            held = np.flatnonzero(status & _HELD)
            if not len(held):
                break
            f = int(held[0])
            replayed = True
            with torch.cuda.device(t._state.device):
                if status[f] & _nat.TRACK_STATUS_PENDING:
                    # the decode left this frame to its large path, which needs a host round trip: materialise it
                    if self._pending is None:
                        raise _nat.HipError("BEVTracker: a negative detection count without a pending decode")
                    self._pending.get()
                    if f == 0:  # the stall is this launch's own: first == B tracks nothing and clears it
                        _nat.track_step(*self._inputs, t.params, t._state, first=self.frames)
                self._launch(first=f)
        else:
            raise _nat.HipError("BEVTracker: a batch did not complete")
        ids, tracks, info, kept = (p.numpy().copy() for p in self._pinned)
        n = np.minimum(np.minimum(kept, self._inputs[0].shape[1]), ids.shape[1])
        self._store(ids, tracks, info, n)
        return replayed

    def _store(self, ids, tracks, info, n):
        self._ids = [ids[b, :n[b]] for b in range(self.frames)]
        self._tracks = [tracks[b, :n[b]] for b in range(self.frames)]
        self._info = info
        self._pending = self._inputs = self._dev = self._pinned = self._event = None  # the decode's buffers may go


class BEVTracker:
    """One sequence's tracker.  gate: metres between a track's predicted position and a detection that may still be
    matched; a track unmatched for more than max_age frames is deleted; a track is reported once it has min_hits
    consecutive matches (or while the sequence has seen at most min_hits frames); max_tracks <= 1024 table slots.

    q_pos, q_vel, r, p0_vel are variances in m^2 and (m / frame)^2.  The defaults are meant for Wildtrack's
    annotated frames, 2 per second -- a pedestrian at 1.4 m/s moves 0.7 m per frame: measurement noise of 0.2 m
    (r = 0.04: under one 0.27 m BEV cell), a new track's unknown velocity 1 m / frame (p0_vel = 1), a velocity change
    of 0.3 m / frame per frame (q_vel = 0.09), 0.1 m of unmodelled motion (q_pos = 0.01).  They are unvalidated
    defaults: no trained checkpoint or dataset was on hand to tune them.

    device: where the state lives; None takes the first batch's (the CPU for all-CPU detections)."""

    def __init__(self, gate: float = 1.0, max_age: int = 2, min_hits: int = 2, q_pos: float = 0.01,
                 q_vel: float = 0.09, r: float = 0.04, p0_vel: float = 1.0, max_tracks: int = 1024, device=None):
        self.params = _nat.TrackParams(gate, max_age, min_hits, q_pos, q_vel, r, p0_vel, max_tracks)
        self._device = torch.device(device) if device is not None else None
        self._state = None      # [1, bytes] uint8: a device tensor or, on the CPU, a numpy array
        self._loaded = None     # a loaded blob that waits for the first batch to say where the state lives
        self._queue: List[TrackResult] = []

    # -- state -------------------------------------------------------------------------------------------------
    def _ensure_state(self, dev: torch.device):
        if self._device is None:
            self._device = dev
        if self._state is None and self._loaded is not None:
            blob, self._loaded = self._loaded, None
            self._state = blob.numpy().copy() if self._device.type == "cpu" else blob.to(self._device, copy=True)
        if self._state is None:
            self._state = _nat.track_state(self.params.max_tracks, self._device)

    def reset(self):
        """Forget every track: the next frame is a sequence's first.  Batches in flight are dropped; no wait."""
        self._queue, self._loaded = [], None
        if self._state is not None:
            _nat.track_reset(self._state, self.params.max_tracks)

    @property
    def in_flight(self) -> int:
        """Batches that still hold device buffers."""
        return len(self._queue)

    def state_dict(self) -> dict:
        """The state blob and the parameters, so a sequence can resume (waits for what is in flight)."""
        self._drain()
        if self._state is None:
            self._ensure_state(self._device or torch.device("cpu"))
        blob = self._state.cpu().clone() if isinstance(self._state, torch.Tensor) else torch.from_numpy(self._state.copy())
        return {"state": blob, "params": dict(self.params._asdict())}

    def load_state_dict(self, sd: dict):
        params = _nat.TrackParams(**sd["params"])
        blob = torch.as_tensor(sd["state"])
        if blob.dtype != torch.uint8 or tuple(blob.shape) != (1, _nat.track_state_bytes(params.max_tracks)):
            raise ValueError(f"BEVTracker.load_state_dict: state of shape {tuple(blob.shape)} {blob.dtype} for "
                             f"max_tracks={params.max_tracks}")
        self._queue = []
        self.params, self._state, self._loaded = params, None, blob.cpu().clone()
        if self._device is not None:
            self._ensure_state(self._device)

    # -- frames ------------------------------------------------------------------------------------------------
    def update(self, pred_boxes) -> TrackResult:
        """Track one batch of consecutive frames: the lazy DetectionList of `BEVDetector.decode(..., lazy=True)` (its
        buffers are read in place, nothing is materialised) or a list of [K, 4] tensors / None on either device.
        Queues one launch and returns; all-CPU input is tracked by the host entry at once."""
        lazy = isinstance(pred_boxes, _nat.DetectionList)
        if lazy:
            raw = pred_boxes.pending.raw
            src = raw.boxes.device
        else:
            rows = _rows(pred_boxes)
            src = next((r.device for r in rows if r.is_cuda), torch.device("cpu"))
        self._ensure_state(src)
        dev = self._device
        if dev.type == "cpu":
            if lazy:
                rows = _rows(list(pred_boxes))  # a host tracker behind a device decode: materialise
            return self._update_host([r.cpu() for r in rows])
        self._release()
        with torch.cuda.device(dev):
            if lazy and src == dev:
                res = TrackResult(self, raw.boxes.shape[0])
                here = torch.cuda.current_stream(dev)
                if here != raw.stream:
                    here.wait_event(raw.ready)
                res._pending, res._inputs = pred_boxes.pending, (raw.boxes, raw.kept)
            else:
                if lazy:
                    rows = _rows(list(pred_boxes))
                res = TrackResult(self, len(rows))
                kept = torch.tensor([r.shape[0] for r in rows], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
                if rows:
                    pred = torch.nn.utils.rnn.pad_sequence([r.to(dev, non_blocking=True) for r in rows],
                                                           batch_first=True).contiguous()
                else:
                    pred = torch.zeros(0, 0, 4, device=dev)
                res._inputs = (pred, kept)
            if res.frames == 0:
                res._store(np.zeros((0, 0), np.int32), np.zeros((0, 0, 4), np.float32), np.zeros((0, 4), np.int32), [])
                return res
            res._launch()
        self._queue.append(res)
        return res

    def _update_host(self, rows) -> TrackResult:
        res = TrackResult(self, len(rows))
        cap = max([r.shape[0] for r in rows], default=0)
        pred = np.zeros((len(rows), cap, 4), np.float32)
        for b, r in enumerate(rows):
            pred[b, :r.shape[0]] = r.numpy()
        n = np.asarray([r.shape[0] for r in rows], np.int32)
        ids, tracks, info = _nat.track_step_host(pred, n, self.params, self._state)
        bad = info[:, 0] & ~_nat.TRACK_STATUS_TRUNCATED
        if bad.any():
            raise _nat.HipError(f"BEVTracker: frames left with status {info[:, 0].tolist()}")
        res._store(ids, tracks, info, np.minimum(n, ids.shape[1]) if len(rows) else [])
        return res

    def _release(self):
        """Batches at the head of the queue whose results have arrived complete (a non-blocking query) let go of
        their decode buffers."""
        while self._queue and self._queue[0]._clean():
            self._queue.pop(0)._finish()

    def _settle(self, res: TrackResult):
        """Complete the queued batches in order up to `res`; once one of them had to be replayed, every later one too
        (they came back stalled and must run before anything new is queued)."""
        replayed = False
        while self._queue:
            head = self._queue[0]
            replayed = head._finish() or replayed
            self._queue.pop(0)
            if head is res and not replayed:
                break
        if res._ids is None:
            raise _nat.HipError("BEVTracker: this result was dropped by reset() or load_state_dict()")

    def _drain(self):
        while self._queue:
            self._settle(self._queue[-1])
