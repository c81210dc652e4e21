"""What tracking a batch costs when it is queued on the device behind the decode, beside what a host tracker costs:
"materialise the decode's detections on the host, then track them there" -- here with the library's own host entry,
so both arms run the same procedure and differ only in where.

    python tools/track_ab.py [--iters 200 --rounds 7] [--out profiles/NAME.txt]

Two seeded inputs, each a warmed-up sequence (the table is full of live tracks before anything is timed):

  wildtrack   B = 2 frames of about 40 people on 12 x 4 m walking 0.3 m per frame, detections jittered by 0.1 m,
              gate 1 m, a table of 1024
  limit       B = 1 frame of 1024 detections against 1024 tracks, people about 1 m apart (1-3 partners in the gate)

Per input the two arms alternate `rounds` times in one process after a warm-up; a round runs `iters` batches and each
line gives the median, minimum and maximum over the rounds, in ms per batch:

  queued      bev_native.track_step on the device buffers, back to back, between two device events (the allocation of
              the result tensors is inside, as a caller pays it): the device time a batch adds to the stream
  host        per batch: copy boxes and counts to the host (the wait a host tracker needs), bev_track_step_host, on the
              host clock.  The device is idle otherwise, so the copy waits for nothing but itself: behind a real
              forward it would also wait for the whole forward.

Both arms see the same frames over and over from the same restored state, and their outputs are compared bit for bit
before anything is timed.  Then the structural claim: BEVTracker.update behind a busy stream returns without waiting.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bev_native as nat  # noqa: E402
import mod_metrics_helper as H  # noqa: E402
from utils.tracking import BEVTracker  # noqa: E402

F = np.float32


def walk(rng, start, n_frames, step, sigma):
    """n_frames of the points `start` [n, 2] moving `step` per frame with Gaussian jitter, rows shuffled per frame."""
    frames = []
    for t in range(n_frames):
        f = np.zeros((len(start), 4), F)
        f[:, :2] = start + np.asarray(step) * t + rng.normal(0, sigma, start.shape)
        frames.append(f[rng.permutation(len(f))])
    return frames


def inputs():
    rng = np.random.default_rng(0)
    people = np.stack([rng.uniform(0, 12, 40), rng.uniform(0, 4, 40)], 1)
    crowd = H.sparse_crowd(rng, 0, 1024, spacing=1.0)[1][:, :2].astype(np.float64)
    return [("wildtrack  B=2  40 people", walk(rng, people, 6, (0.3, 0.05), 0.1), 2, 1.0),
            ("limit      B=1  1024 x 1024", walk(rng, crowd, 5, (0.05, 0.0), 0.05), 1, 0.1)]


def pack(frames):
    cap = max(len(f) for f in frames)
    pred = np.zeros((len(frames), cap, 4), F)
    for b, f in enumerate(frames):
        pred[b, :len(f)] = f
    return pred, np.asarray([len(f) for f in frames], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/track_ab.py measures on the GPU; none found")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"tools/track_ab.py --iters {a.iters} --rounds {a.rounds}: {torch.cuda.get_device_name(0)}; ms per batch, "
         f"median (min - max) over the rounds, arms alternating in one process")
    P = nat.TrackParams(gate=1.0, max_age=2, min_hits=2, q_pos=0.01, q_vel=0.09, r=0.04, p0_vel=1.0, max_tracks=1024)
    for name, frames, B, scale in inputs():
        warm, timed = pack(frames[:-B]), pack(frames[-B:])
        iters = max(3, int(a.iters * scale))
        # the warmed-up state, on both sides; one timed batch from it, compared
        h0 = nat.track_state(P.max_tracks)
        nat.track_step_host(*warm, P, h0)
        d0 = torch.from_numpy(h0).cuda()
        dev = [torch.from_numpy(x).cuda() for x in timed]
        hs, ds = h0.copy(), d0.clone()
        want = nat.track_step_host(*timed, P, hs)
        got = [t.cpu().numpy() for t in nat.track_step(*dev, P, ds)]
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and ds.cpu().numpy().tobytes() == hs.tobytes()
        live, matched = int(want[2][-1, 1]), int((want[0][-1] >= 0).sum())
        times = {"queued": [], "host": []}
        for r in range(1 + a.rounds):
            ds.copy_(d0)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):  # the same frames again: every track finds its detection where it was
                nat.track_step(*dev, P, ds)
            t1.record()
            t1.synchronize()
            if r:
                times["queued"].append(t0.elapsed_time(t1) / iters)
            hs[:] = h0
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            for _ in range(iters):
                nat.track_step_host(dev[0].cpu().numpy(), dev[1].cpu().numpy(), P, hs)
            c1 = time.perf_counter()
            if r:
                times["host"].append((c1 - c0) / iters * 1e3)
        for what in ("queued", "host"):
            v = times[what]
            emit(f"  {name:28s} {what:6s}: {statistics.median(v):9.4f} ({min(v):.4f} - {max(v):.4f})  live {live} "
                 f"reported {matched}  [{iters} batches a round]")

    # the structural claim: update() queues and returns
    rng = np.random.default_rng(1)
    people = np.stack([rng.uniform(0, 12, 40), rng.uniform(0, 4, 40)], 1)
    stream = [[torch.from_numpy(f).cuda() for f in walk(rng, people + 0.6 * s, 2, (0.3, 0.05), 0.1)] for s in range(20)]
    spin = torch.empty(64 << 20, device="cuda")
    upd, tot, pending = [], [], 0
    for r in range(1 + a.rounds):
        tracker = BEVTracker(max_tracks=1024)
        torch.cuda.synchronize()
        for _ in range(40):  # keep the stream busy: a wait inside update() would have to sit this out
            spin.add_(1.0)
        t0 = time.perf_counter()
        res = [tracker.update(b) for b in stream]
        t1 = time.perf_counter()
        pending = tracker.in_flight
        ids = [r_.ids for r_ in res]
        t2 = time.perf_counter()
        if r:
            upd.append((t1 - t0) / len(stream) * 1e3)
            tot.append((t2 - t0) / len(stream) * 1e3)
    emit(f"BEVTracker, 20 batches of B = 2 behind ~{40 * 64 * 4 * 2 / 1e3:.0f} GB of queued device traffic: host ms per "
         f"batch")
    emit(f"  update() alone                {statistics.median(upd):8.4f} ({min(upd):.4f} - {max(upd):.4f}); batches "
         f"still in flight when the last update returned: {pending} of {len(stream)}")
    emit(f"  update() + reading every ids  {statistics.median(tot):8.4f} ({min(tot):.4f} - {max(tot):.4f}); ids of the "
         f"last frame: {sorted(ids[-1][-1].tolist())[:6]} ...")
    assert pending > 0, "update() waited for the device"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
