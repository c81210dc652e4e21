"""What the optimal matching of the MODA / MODP scoring costs on the device, beside the greedy matching it stands next
to (the algorithms differ: the greedy time is context, not a bar).

    python tools/mod_assign_ab.py [--iters 200 --rounds 7] [--out profiles/NAME.txt]

Four seeded inputs, each scored by bev_native.detection_assign (k_det_assign) and bev_native.detection_match
(k_det_match) on the same device buffers:

  wildtrack   B = 2, 40 ground truths on 12 x 4 m, 36 predictions jittered by 0.25 m plus 6 strays per frame
  batch       B = 32, 130 x 130 per frame, predictions near ground truths 0.7 m apart
  limit       B = 1, 1024 x 1024, ground truths about 1 m apart: most predictions have 1-3 partners within 0.5 m
  dense       B = 1, 1024 x 1024 on 3 x 3 m: every prediction has hundreds of partners (the solver's worst case)

Per input the two entries alternate `rounds` times in one process after a warm-up; a round times `iters` back-to-back
launches between two device events (the allocation of the 16 + 8 B per frame of results is inside, as a caller pays
it) and reports the time per launch; each line gives the median, minimum and maximum over the rounds.  The device
results are compared with the host entries' bit for bit before anything is timed.

Then the structural claims on the wildtrack input behind a lazy decode stand-in: DetectionMetrics(matching="optimal")
.update per batch is timed on the host clock and must not wait (the result rows are still in flight when it returns),
result_mod() waits once.
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
from utils.metrics import DetectionMetrics  # noqa: E402


def inputs():
    rng = np.random.default_rng(0)
    crowds = [H.crowd(s) for s in (0, 1)]
    batch = [H.sparse_crowd(rng, 130, 130, spacing=0.7) for _ in range(32)]
    limit = [H.sparse_crowd(rng, 1024, 1024, spacing=1.0)]
    dense = [H.square_frame(rng, 1024, 1024, side=3.0)]
    return [("wildtrack  B=2  42 x 40", crowds, 1.0), ("batch      B=32 130 x 130", batch, 1.0),
            ("limit      B=1  1024 x 1024", limit, 0.25), ("dense      B=1  1024 x 1024", dense, 0.02)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mod_assign_ab.py measures on the GPU; none found")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"tools/mod_assign_ab.py --iters {a.iters} --rounds {a.rounds}: {torch.cuda.get_device_name(0)}; ms per launch, "
         f"median (min - max) over the rounds, entries alternating in one process")
    for name, frames, scale in inputs():
        packed = H.pack([f[0] for f in frames], [f[1] for f in frames])
        dev = [torch.from_numpy(x).cuda() for x in packed]
        iters = max(3, int(a.iters * scale))
        tps = {}
        for what, entry, host in (("assign", nat.detection_assign, nat.detection_assign_host),
                                  ("greedy", nat.detection_match, nat.detection_match_host)):
            c, s = entry(*dev, 0.5)
            hc, hs = host(*packed, 0.5)
            assert np.array_equal(c.cpu().numpy(), hc) and np.array_equal(s.cpu().numpy().view(np.uint64),
                                                                         hs.view(np.uint64)), (name, what)
            tps[what] = int(hc[:, 0].sum())
        times = {"assign": [], "greedy": []}
        for r in range(1 + a.rounds):
            for what, entry in (("assign", nat.detection_assign), ("greedy", nat.detection_match)):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(iters):
                    entry(*dev, 0.5)
                t1.record()
                t1.synchronize()
                if r:
                    times[what].append(t0.elapsed_time(t1) / iters)
        for what in ("assign", "greedy"):
            v = times[what]
            emit(f"  {name:28s} {what}: {statistics.median(v):9.4f} ({min(v):.4f} - {max(v):.4f})  tp {tps[what]}"
                 f"  [{iters} launches a round]")

    # the structural claims: update() queues and returns, result_mod() waits once
    rng = np.random.default_rng(1)
    stream = []
    for s in range(20):
        fr = [H.crowd(100 + 2 * s), H.crowd(101 + 2 * s)]
        stream.append(([torch.from_numpy(f[0]).cuda() for f in fr], [{"boxes_world": torch.from_numpy(f[1])} for f in fr]))
    spin = torch.empty(64 << 20, device="cuda")
    upd, tot, pending = [], [], 0
    for r in range(1 + a.rounds):
        val = DetectionMetrics(0.5, matching="optimal")
        torch.cuda.synchronize()
        for _ in range(40):  # keep the stream busy: a wait inside update() would have to sit this out
            spin.add_(1.0)
        t0 = time.perf_counter()
        for p, g in stream:
            val.update(p, g)
        t1 = time.perf_counter()
        pending = val.in_flight()
        res = val.result_mod()
        t2 = time.perf_counter()
        if r:
            upd.append((t1 - t0) / len(stream) * 1e3)
            tot.append((t2 - t0) / len(stream) * 1e3)
    emit(f"DetectionMetrics(matching='optimal'), 20 batches of B = 2 behind ~{40 * 64 * 4 * 2 / 1e3:.0f} GB of queued "
         f"device traffic: host ms per batch")
    emit(f"  update() alone                {statistics.median(upd):8.4f} ({min(upd):.4f} - {max(upd):.4f}); batches "
         f"still in flight when the last update returned: {pending} of {len(stream)}")
    emit(f"  update() + one result_mod()   {statistics.median(tot):8.4f} ({min(tot):.4f} - {max(tot):.4f})")
    emit(f"  result_mod(): moda {res['moda']:.2f} modp {res['modp']:.2f} precision {res['precision']:.2f} recall "
         f"{res['recall']:.2f}  tp {res['tp']} fp {res['fp']} fn {res['fn']}")
    assert pending > 0, "update() waited for the device"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
