"""Golden fixture for the validation scoring (utils/metrics.py, csrc/bev_metrics.hip), recorded from the reference's
own `compute_metrics` (train.py:78-104).

Run ONLY where the read-only reference tree exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metrics_golden.py [path/to/reference/project]

`train.py` imports the loader and torchvision at module scope, so it is not imported: the file is parsed and only the
one function definition is executed, with `torch` in scope.  Inputs are this script's own synthetic frames.

What the fixture can pin.  The reference's distance is torch.norm(dim=1) on the CPU, the library's is
sqrtf(dx dx + dy dy) with separately rounded operations; the two differ by 1 ulp on a few per cent of random pairs.
So only decisions that a 1-ulp difference cannot flip are recorded, and this script asserts for every case that
  * every prediction's nearest distance is more than 4 ulp from thr32 (the largest float32 <= match_dist), or the true
    distance is exactly a float32 by construction (axis-aligned offsets from the origin, 3-4-5 triangles scaled by
    powers of two) and both formulas return exactly it;
  * every prediction's nearest and second-nearest distances differ by more than 4 ulp, or are ties by construction
    (the same |dx|, |dy| multiset gives the same value under any formula);
  * a coordinate is finite and small, or literally NaN / +-Inf (no overflow that one formula could avoid).
No case is dropped to satisfy them: the script fails instead.

Output: tests/golden/metrics_cases.npz -- data only, floats as bit patterns.
  names [C]            case names
  match_dist [C] u64   the double's bits
  frames [C]           B per case
  pred_count [sum B]   K per frame, -1 for a None entry;  pred [sum K, 4] u32
  gt_count [sum B]     G per frame, -1 for a dict without 'boxes_world';  gt [sum G, 4] u32
  prf [C, 4] u64       precision, recall, f1, mle;  counts [C, 3] tp, fp, fn
  seq [3]              the cases of the three-batch sequence;  seq_means [4] u64, seq_counts [3]: train.py:299-302
"""
from __future__ import annotations

import ast
import os
import sys
from fractions import Fraction

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/project"
OUT = os.path.join(HERE, "metrics_cases.npz")
F = np.float32
NAN, INF = float("nan"), float("inf")


def reference_function():
    tree = ast.parse(open(os.path.join(REF, "train.py")).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_metrics")
    scope = {"torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), "train.py", "exec"), scope)
    return scope["compute_metrics"]


def up(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, F(np.inf))
    return float(x)


def down(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, F(-np.inf))
    return float(x)


def box(x, y, w=0.6, h=0.6):
    return [x, y, w, h]


def thr32(m):
    t = F(m)
    return float(t) if float(t) <= m else down(t)


def exact_f32(dx, dy):
    """Is sqrt(dx^2 + dy^2) exactly a float32?  (dx, dy float32 values.)"""
    s = Fraction(float(dx)) ** 2 + Fraction(float(dy)) ** 2
    r = F(np.sqrt(float(s)))
    return Fraction(float(r)) ** 2 == s


def check_margins(name, preds, gts, m):
    t = thr32(m)
    for p, g in zip(preds, gts):
        if p is None or g is None or len(p) == 0 or len(g) == 0:
            continue
        p, g = np.asarray(p, F).reshape(-1, 4), np.asarray(g, F).reshape(-1, 4)
        for v in np.concatenate([p[:, :2].ravel(), g[:, :2].ravel()]):
            assert not np.isfinite(v) or abs(v) < 1e6, (name, v)
        with np.errstate(all="ignore"):
            for i in range(len(p)):
                dx, dy = g[:, 0] - p[i, 0], g[:, 1] - p[i, 1]  # float32, as both formulas subtract
                lib = np.sqrt(dx * dx + dy * dy)
                ref = torch.norm(torch.from_numpy(g[:, :2]) - torch.from_numpy(p[i, :2]).unsqueeze(0), dim=1).numpy()
                assert np.array_equal(np.isfinite(lib), np.isfinite(ref)) and np.array_equal(np.isnan(lib),
                                                                                             np.isnan(ref)), name
                if np.isnan(lib).any() or not np.isfinite(lib).any():
                    continue  # NaN at the first NaN's index / all +Inf at index 0: no formula decides
                d64 = np.hypot(dx.astype(np.float64), dy.astype(np.float64))
                order = np.argsort(np.where(np.isfinite(d64), d64, np.inf), kind="stable")
                a = order[0]
                ulp = float(np.spacing(F(d64[a])))
                if abs(d64[a] - t) <= 4 * ulp:
                    assert exact_f32(dx[a], dy[a]) and lib[a] == ref[a] == F(d64[a]), (name, i, "threshold margin")
                if len(order) > 1 and np.isfinite(d64[order[1]]):
                    b = order[1]
                    if d64[b] - d64[a] <= 4 * ulp:
                        same = sorted([abs(dx[a]), abs(dy[a])]) == sorted([abs(dx[b]), abs(dy[b])])
                        assert same, (name, i, "nearest / second-nearest margin")


def random_frames(rng, B, kmax, gmax, noise):
    preds, gts = [], []
    for _ in range(B):
        G, K = int(rng.integers(0, gmax + 1)), int(rng.integers(0, kmax + 1))
        g = np.concatenate([rng.uniform(-20, 20, (G, 2)), rng.uniform(0.3, 1.0, (G, 2))], 1).astype(F)
        p = np.concatenate([rng.uniform(-20, 20, (K, 2)), rng.uniform(0.3, 1.0, (K, 2))], 1).astype(F)
        for i in range(min(K, G)):  # most predictions near some ground truth, a few contested
            j = i if rng.random() < 0.8 else int(rng.integers(0, G))
            p[i, :2] = g[j, :2] + rng.normal(0, noise, 2).astype(F)
        preds.append(p[rng.permutation(K)] if K else p)
        gts.append(g)
    return preds, gts


def cases():
    """(name, preds per frame (list | None), gts per frame (list | None = no 'boxes_world'), match_dist)"""
    c = []
    c.append(("no_gt_with_predictions", [[box(1, 2), box(3, 4), box(-5, 0.5)]], [[]], 0.5))
    c.append(("no_predictions_with_gt", [[]], [[box(1, 2), box(3, 4)]], 0.5))
    c.append(("none_entry_and_missing_key", [None, [box(1, 1), box(2.25, 2)], [box(0, 0)]],
              [[box(1, 1.125)], None, [box(0.25, 0)]], 0.5))
    # two predictions contest g0 while g1 lies in range of the second: the second is FP, no second try
    c.append(("contested_ground_truth", [[box(0.125, 0), box(0.25, 0), box(4, 4)]],
              [[box(0, 0), box(0.625, 0), box(4, 4.25)]], 0.5))
    # first-index ties: the same |dx|, |dy| multiset to two ground truths, prediction at the origin
    c.append(("first_index_ties", [[box(0, 0), box(0, 0), box(8, 8)]],
              [[box(0.25, 0.125), box(-0.125, 0.25), box(0.125, -0.25), box(8, 8)]], 0.5))
    c.append(("tie_first_used_second_free", [[box(0, 0), box(0, 0)]], [[box(0.25, 0), box(0, 0.25)]], 0.5))
    # exactly match_dist (TP), one float32 step above (FP); 3-4-5 at 2^-3: exactly 0.625
    c.append(("distance_equals_half", [[box(0, 0)], [box(0, 0)], [box(0, 0)], [box(0, 0)]],
              [[box(0.5, 0)], [box(0, -0.5)], [box(up(0.5), 0)], [box(0, down(0.5))]], 0.5))
    c.append(("three_four_five", [[box(0, 0)], [box(0, 0)], [box(1, 1)]],
              [[box(0.375, 0.5)], [box(-0.5, 0.375)], [box(1.375, 1.5)]], 0.625))
    c.append(("three_four_five_below", [[box(0, 0)], [box(0, 0)]], [[box(0.375, 0.5)], [box(0.1875, 0.25)]],
              down(0.625)))
    # 0.3 is not a float32: float32(0.3) > 0.3 is FP, the float32 below it is TP
    c.append(("unrepresentable_threshold", [[box(0, 0)], [box(0, 0)], [box(0, 0)]],
              [[box(float(F(0.3)), 0)], [box(0, down(F(0.3)))], [box(0.25, 0)]], 0.3))
    c.append(("nan_prediction", [[box(NAN, 0), box(1, 1), box(2, NAN)]], [[box(1, 1.25), box(5, 5)]], 0.5))
    c.append(("nan_ground_truth", [[box(1, 1)]], [[box(1, 1.25), box(NAN, 0)]], 0.5))
    c.append(("nan_ground_truth_first_of_two", [[box(1, 1), box(7, 7)]], [[box(0, NAN), box(1, 1), box(NAN, NAN)]],
              0.5))
    c.append(("inf_coordinates", [[box(INF, 0), box(1, 1), box(-INF, INF)], [box(2, 2)]],
              [[box(1, 1.25), box(INF, 0), box(3, 3)], [box(INF, INF), box(-INF, 2)]], 0.5))
    c.append(("inf_threshold_all_match", [[box(0, 0), box(10, 10), box(10.5, 10)]], [[box(3, 4), box(10, 10.25)]], INF))
    c.append(("zero_threshold", [[box(1, 1), box(2, 2)]], [[box(1, 1), box(2, 2.5)]], 0.0))
    rng = np.random.default_rng(20)
    p, g = random_frames(rng, 3, 12, 10, 0.2)
    p[1], g[2] = p[1][:0], g[2][:0]  # B = 3 mixing empty and full frames
    c.append(("three_frames_mixed", p, g, 0.5))
    for k in range(3):  # the accumulator's three-batch sequence
        p, g = random_frames(rng, 2, 14, 12, 0.25)
        c.append((f"sequence_{k}", p, g, 0.5))
    p, g = random_frames(rng, 2, 40, 40, 0.3)
    c.append(("forty_by_forty", p, g, 0.7))
    return c


def main():
    ref = reference_function()
    names, md, frames, pc, gc, pr, gr, prf, counts = [], [], [], [], [], [], [], [], []
    tuples = {}
    for name, preds, gts, m in cases():
        check_margins(name, preds, gts, m)
        tp_ = [None if p is None else torch.from_numpy(np.asarray(p, F).reshape(-1, 4)) for p in preds]
        tg_ = [{} if g is None else {"boxes_world": torch.from_numpy(np.asarray(g, F).reshape(-1, 4))} for g in gts]
        out = ref(tp_, tg_, match_dist=m)
        tuples[name] = out
        names.append(name)
        md.append(m)
        frames.append(len(gts))
        for p, g in zip(tp_, tg_):
            pc.append(-1 if p is None else p.shape[0])
            gc.append(g["boxes_world"].shape[0] if g else -1)
            if p is not None:
                pr.append(p.numpy())
            if g:
                gr.append(g["boxes_world"].numpy())
        prf.append([float(v) for v in out[:4]])
        counts.append([int(v) for v in out[4:]])
        print(f"{name:34s} {out}")
    seq = [names.index(f"sequence_{k}") for k in range(3)]
    per = [tuples[names[i]] for i in seq]
    means = [sum(t[k] for t in per) / max(1, len(per)) for k in range(4)]  # train.py:299-302
    sums = [sum(t[k] for t in per) for k in (4, 5, 6)]
    cat = lambda rows: np.concatenate(rows + [np.zeros((0, 4), F)]).astype(F).view(np.uint32)  # noqa: E731
    np.savez_compressed(
        OUT, names=np.asarray(names), match_dist=np.asarray(md, np.float64).view(np.uint64),
        frames=np.asarray(frames, np.int64), pred_count=np.asarray(pc, np.int64), gt_count=np.asarray(gc, np.int64),
        pred=cat(pr), gt=cat(gr), prf=np.asarray(prf, np.float64).view(np.uint64),
        counts=np.asarray(counts, np.int64), seq=np.asarray(seq, np.int64),
        seq_means=np.asarray(means, np.float64).view(np.uint64), seq_counts=np.asarray(sums, np.int64))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
