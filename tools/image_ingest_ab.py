"""Interleaved A/B of the camera-frame ingest: host Pillow resize + device normalize (the default path) against the
device resize + normalize launch (`data.transforms.resize_normalize_on_device`), on native-size frames.

    python tools/image_ingest_ab.py --rounds 5 --iters 20 [--out profiles/NAME.txt]

Per geometry (default 2 x 7 frames of 1080 x 1920 -> 270 x 480 and -> 540 x 960) the two arms' outputs are first
asserted bit-identical, then the arms alternate inside one process, `rounds` times each after a warm-up:

  arm a (the default path): Pillow `resize((W, H), BILINEAR)` of every frame on the host (one thread, and a pool of
        16 threads -- Pillow releases the GIL while it resamples), the resized uint8 batch copied into pinned memory,
        H2D, `bev_image_normalize_u8_f32`;
  arm b (the device path):  H2D of the native-size uint8 batch from pinned memory, `bev_image_resize_normalize_u8_f32`.

Arm times are host clock from the first host instruction to the device synchronise after the last launch (the host
resize is part of arm a); the H2D copy and the launches are also timed with HIP events.  The new kernel alone is timed
with HIP events around `iters` launches on resident frames, once on one buffer (87 MB of frames stay in the 256 MiB
Infinity Cache) and once rotating over enough copies to exceed it, and reported with (3 Hs Ws + 12 H W) N bytes over
that time as a fraction of the 8 TB/s HBM peak.  The frames are decoded already in both arms: JPEG / PNG decode is the
same work on either path and is not timed.
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import bev_native as nat  # noqa: E402
from data import transforms as T  # noqa: E402

HBM_PEAK = 8.0e12


def host_resize(frames, hw, pool):
    H, W = hw

    def one(a):
        return np.array(Image.fromarray(a).resize((W, H), Image.BILINEAR))
    return list(pool.map(one, frames)) if pool is not None else [one(a) for a in frames]


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def arm_a(frames, hw, pool, pinned_small, dev_small):
    t0 = time.perf_counter()
    small = host_resize(frames, hw, pool)
    t1 = time.perf_counter()
    for i, s in enumerate(small):
        pinned_small[i] = torch.from_numpy(s)
    e0, e1 = events()
    e0.record()
    dev_small.copy_(pinned_small, non_blocking=True)
    out = T.normalize_on_device(dev_small)
    e1.record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return out, (t2 - t0) * 1e3, (t1 - t0) * 1e3, e0.elapsed_time(e1)


def arm_b(pinned_native, dev_native, hw):
    t0 = time.perf_counter()
    e0, e1 = events()
    e0.record()
    dev_native.copy_(pinned_native, non_blocking=True)
    out = T.resize_normalize_on_device(dev_native, hw)
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return out, (t1 - t0) * 1e3, e0.elapsed_time(e1)


def kernel_alone(bufs, hw, iters):
    for b in bufs:
        T.resize_normalize_on_device(b, hw)
    torch.cuda.synchronize()
    e0, e1 = events()
    e0.record()
    for i in range(iters):
        T.resize_normalize_on_device(bufs[i % len(bufs)], hw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rng_line(name, v, unit="ms"):
    return (f"  {name:46s} median {statistics.median(v):9.3f} {unit}  min {min(v):9.3f}  max {max(v):9.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, nargs=2, default=[2, 7], help="B V")
    ap.add_argument("--native", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--sizes", type=int, nargs="+", default=[270, 480, 540, 960], help="H W pairs")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("tools/image_ingest_ab.py measures on the GPU; none found")
    dev = torch.device("cuda")
    B, V = a.frames
    N = B * V
    Hs, Ws = a.native
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8) for _ in range(N)]
    pinned_native = torch.empty(B, V, Hs, Ws, 3, dtype=torch.uint8).pin_memory()
    for i, f in enumerate(frames):
        pinned_native.view(N, Hs, Ws, 3)[i] = torch.from_numpy(f)
    dev_native = torch.empty(B, V, Hs, Ws, 3, dtype=torch.uint8, device=dev)
    copies = max(2, int(np.ceil(300e6 / pinned_native.numel())))  # > 256 MiB of frames in rotation
    emit(f"tools/image_ingest_ab.py --rounds {a.rounds} --iters {a.iters}: {B} x {V} frames of {Hs} x {Ws}, "
         f"{torch.cuda.get_device_name(0)}, Pillow {Image.__version__}, host pool {a.threads} threads")
    pool = ThreadPoolExecutor(a.threads)
    for H, W in zip(a.sizes[0::2], a.sizes[1::2]):
        hw = (H, W)
        emit(f"geometry {Hs} x {Ws} -> {H} x {W}, N = {N}")
        pinned_small = torch.empty(N, H, W, 3, dtype=torch.uint8).pin_memory()
        dev_small = torch.empty(B, V, H, W, 3, dtype=torch.uint8, device=dev)
        ps = pinned_small
        # 1. the arms compute the same bits (this is also the warm-up of every shape)
        out_a = arm_a(frames, hw, None, ps, dev_small.view(N, H, W, 3))[0].view(B, V, 3, H, W)
        out_b = arm_b(pinned_native, dev_native, hw)[0]
        same = torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
        emit(f"  outputs bit-identical: {same}")
        assert same, "the device resize differs from Pillow + normalize"
        del out_a, out_b
        arm_a(frames, hw, pool, ps, dev_small.view(N, H, W, 3))
        # 2. alternate the arms
        res = {"a1": [], "a1_resize": [], "a1_dev": [], "a16": [], "a16_resize": [], "a16_dev": [], "b": [],
               "b_dev": []}
        for _ in range(a.rounds):
            _, tot, rs, dv = arm_a(frames, hw, None, ps, dev_small.view(N, H, W, 3))
            res["a1"].append(tot), res["a1_resize"].append(rs), res["a1_dev"].append(dv)
            _, tot, dv = arm_b(pinned_native, dev_native, hw)
            res["b"].append(tot), res["b_dev"].append(dv)
            _, tot, rs, dv = arm_a(frames, hw, pool, ps, dev_small.view(N, H, W, 3))
            res["a16"].append(tot), res["a16_resize"].append(rs), res["a16_dev"].append(dv)
        emit(rng_line("arm a, 1 host thread: end to end", res["a1"]))
        emit(rng_line("  of it the Pillow resize of the frames", res["a1_resize"]))
        emit(rng_line("  of it H2D (small batch) + normalize, events", res["a1_dev"]))
        emit(rng_line(f"arm a, {a.threads} host threads: end to end", res["a16"]))
        emit(rng_line("  of it the Pillow resize of the frames", res["a16_resize"]))
        emit(rng_line("  of it H2D (small batch) + normalize, events", res["a16_dev"]))
        emit(rng_line("arm b, device resize: end to end", res["b"]))
        emit(rng_line("  of it H2D (native batch) + the launch, events", res["b_dev"]))
        ma1, ma16, mb = (statistics.median(res[k]) for k in ("a1", "a16", "b"))
        emit(f"  arm b / arm a: {mb / ma1:.3f} of the 1-thread host path, {mb / ma16:.3f} of the {a.threads}-thread one")
        # 3. the new kernel alone
        nbytes = (3 * Hs * Ws + 12 * H * W) * N
        bufs = [dev_native] + [dev_native.clone() for _ in range(copies - 1)]
        for label, bb in ((f"one buffer ({dev_native.numel() / 1e6:.0f} MB, cache-resident)", bufs[:1]),
                          (f"{copies} buffers in rotation ({copies * dev_native.numel() / 1e6:.0f} MB)", bufs)):
            ms = [kernel_alone(bb, hw, a.iters) for _ in range(a.rounds)]
            emit(rng_line(f"kernel alone, {label}", [m * 1e3 for m in ms], "us"))
            med = statistics.median(ms) * 1e-3
            emit(f"    {nbytes / 1e6:.1f} MB per launch -> {nbytes / med / 1e12:.2f} TB/s = "
                 f"{nbytes / med / HBM_PEAK:.3f} of the 8 TB/s peak")
        del bufs
    pool.shutdown()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
