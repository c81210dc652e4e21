"""What the device colour jitter costs: the reference config's ingest, 2 x 7 frames of 1080 x 1920 -> 270 x 480.

    python tools/image_jitter_ab.py --parent-lib PATH/libbev_mi355x.so [--rounds 7 --iters 50] [--out profiles/NAME.txt]

All device times are HIP events around `iters` launches on resident frames, the arms alternating `rounds` times in one
process after a warm-up; each line gives the median, minimum and maximum over the rounds.

  (a) `bev_image_resize_normalize_u8_f32` of this tree's library against the same entry of a library built from the
      parent commit (`--parent-lib`; both called through ctypes on the same buffers, outputs asserted equal): the uint8
      epilogue became a template flag of that kernel, and its default instance must not have slowed down.  The
      parent's spread between its own rounds is the yardstick.
  (b) `resize_jitter_normalize_on_device` (`bev_image_resize_u8`, then the two passes of
      `bev_image_jitter_normalize_u8_f32`) with half the frames jittered (all four ops, drawn as ColorJitter draws
      them), against (a); also with every frame jittered and with none.
  (c) for context: the CPU time of the host pipeline's `Resize` + `ColorJitter` on the same 14 frames (one thread).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import bev_native as nat  # noqa: E402
from data import transforms as T  # noqa: E402

ENTRY = "bev_image_resize_normalize_u8_f32"


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def line(name, v, unit="us"):
    return f"  {name:58s} median {statistics.median(v):9.2f} {unit}  min {min(v):9.2f}  max {max(v):9.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libbev_mi355x.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("tools/image_jitter_ab.py measures on the GPU; none found")
    B, V, Hs, Ws, H, W = 2, 7, 1080, 1920, 270, 480
    N = B * V
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, size=(B, V, Hs, Ws, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    emit(f"tools/image_jitter_ab.py --rounds {a.rounds} --iters {a.iters}: {B} x {V} frames of {Hs} x {Ws} -> {H} x {W}, "
         f"{torch.cuda.get_device_name(0)}, Pillow {Image.__version__}")

    # (a) the fp32 resize launch: this tree's library against the parent's
    flat = dev.view(N, Hs, Ws, 3)
    plan = nat._resize_plan_dev(dev.device, Hs, Ws, H, W)
    m = (ctypes.c_float * 3)(*T.IMAGENET_MEAN)
    s = (ctypes.c_float * 3)(*T.IMAGENET_STD)
    out_new = torch.empty(N, 3, H, W, device="cuda")
    out_old = torch.empty_like(out_new)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(L, out):
        rc = getattr(L, ENTRY)(nat._ptr(flat), N, Hs, Ws, nat._ptr(plan), H, W, m, s, nat._ptr(out), stream)
        assert rc == 0, rc

    arms = {"this tree": (nat.lib(), out_new)}
    if a.parent_lib:
        old = ctypes.CDLL(os.path.abspath(a.parent_lib))
        getattr(old, ENTRY).restype, getattr(old, ENTRY).argtypes = nat.SIGNATURES[ENTRY]
        old.bev_build_source_hash.restype = ctypes.c_char_p
        arms["parent"] = (old, out_old)
        emit(f"(a) {ENTRY}: this tree (sources {nat.source_hash()}) against the parent's library "
             f"(sources {old.bev_build_source_hash().decode()})")
    else:
        emit(f"(a) {ENTRY}: this tree alone (no --parent-lib)")
    for L, out in arms.values():
        launch(L, out)
    torch.cuda.synchronize()
    if a.parent_lib:
        same = torch.equal(out_new.view(torch.int32), out_old.view(torch.int32))
        emit(f"  outputs bit-identical: {same}")
        assert same
    res = {k: [] for k in arms}
    for _ in range(2 + a.rounds):  # two warm-up rounds
        for k, (L, out) in arms.items():
            res[k].append(timed(lambda: launch(L, out), a.iters))
    for k in arms:
        emit(line(f"{k}", res[k][2:]))
    if a.parent_lib:
        mn, mo = statistics.median(res["this tree"][2:]), statistics.median(res["parent"][2:])
        spread = max(res["parent"][2:]) - min(res["parent"][2:])
        emit(f"  this tree - parent: {mn - mo:+.2f} us ({mn / mo:.4f}x); the parent's own spread over its rounds: "
             f"{spread:.2f} us")

    # (b) resize + jitter + normalize
    emit("(b) resize_jitter_normalize_on_device against resize_normalize_on_device (wrappers, allocation included)")
    torch.manual_seed(0)
    jitter = T.ColorJitter(0.2, 0.2, 0.2, 0.05)
    drawn = torch.stack([jitter.params_record() for _ in range(N)])
    recs = {}
    for name, keep in (("half the frames jittered", [i % 2 == 0 for i in range(N)]), ("every frame jittered", [True] * N),
                       ("no frame jittered", [False] * N)):
        r = drawn.clone()
        r[~torch.tensor(keep)] = 0
        recs[name] = r.view(B, V, 8).cuda()
    half = recs["half the frames jittered"]
    # the arms compute the same frames where the jitter is skipped
    got = T.resize_jitter_normalize_on_device(dev, (H, W), half)
    base = T.resize_normalize_on_device(dev, (H, W))
    skipped = (half[..., 0] == 0)
    assert torch.equal(got[skipped].view(torch.int32), base[skipped].view(torch.int32))
    assert not torch.equal(got[~skipped], base[~skipped])
    del got, base
    fns = {"resize_normalize_on_device (a)": lambda: T.resize_normalize_on_device(dev, (H, W))}
    for name, r in recs.items():
        fns[f"resize_jitter_normalize_on_device, {name}"] = (lambda r=r: T.resize_jitter_normalize_on_device(dev, (H, W), r))
    small = nat.image_resize_u8(flat, (H, W))
    fns["  of it bev_image_resize_u8"] = lambda: nat.image_resize_u8(flat, (H, W))
    fns["  of it the jitter's two passes (half jittered)"] = (
        lambda: nat.image_jitter_normalize_u8(small, half.view(N, 8), T.IMAGENET_MEAN, T.IMAGENET_STD))
    res = {k: [] for k in fns}
    for _ in range(2 + a.rounds):
        for k, fn in fns.items():
            res[k].append(timed(fn, a.iters))
    for k in fns:
        emit(line(k, res[k][2:]))
    ma = statistics.median(res["resize_normalize_on_device (a)"][2:])
    for name in recs:
        mb = statistics.median(res[f"resize_jitter_normalize_on_device, {name}"][2:])
        emit(f"  {name}: {mb / ma:.3f}x of (a), +{mb - ma:.2f} us per batch of {N} frames")

    # (c) the host pipeline's Resize + ColorJitter
    emit("(c) host Resize + ColorJitter of the 14 frames, one thread (context)")
    imgs = [Image.fromarray(f) for f in frames.reshape(N, Hs, Ws, 3)]
    rs = T.Resize((H, W))
    cpu = {"Resize": [], "ColorJitter (every frame)": []}
    for _ in range(3):
        t0 = time.perf_counter()
        small_imgs = [rs(im) for im in imgs]
        t1 = time.perf_counter()
        for im in small_imgs:
            jitter(im)
        t2 = time.perf_counter()
        cpu["Resize"].append((t1 - t0) * 1e3)
        cpu["ColorJitter (every frame)"].append((t2 - t1) * 1e3)
    for k, v in cpu.items():
        emit(line(k, v, "ms"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
