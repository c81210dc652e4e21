"""Single-stream timing of the ResNet stem launch of the bench step (14 x 3 x 1080 x 1920 images) on the split
arithmetic: the fused stem + max-pool (k_stem_x6<true> + k_stem_pool_seams) and the plain stem (k_stem_x6<false>).

    python tools/stem_micro.py --iters 30
    python tools/with_lib.py <other libbev_mi355x.so> tools/stem_micro.py --iters 30     # A/B against another build

One HIP-event pair per call after warm-up; prints the median, minimum and maximum per form.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))

import torch  # noqa: E402

import bev_native as nat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=14)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(a.images, 3, 1080, 1920, device=dev, generator=g)
    w = torch.randn(64, 3, 7, 7, device=dev, generator=g) / 147 ** 0.5
    b = torch.randn(64, device=dev, generator=g) * 0.1
    packed = nat.pack_conv_weight_x6(w)
    forms = {"stem+pool": lambda: nat.conv2d_stem_pool_x6(x, packed, b),
             "stem": lambda: nat.conv2d_stem_x6(x, packed, b, 64, True)}
    for name, fn in forms.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        print(f"{name:10s} {a.images} images: median {statistics.median(us):8.1f} us  min {min(us):8.1f}  "
              f"max {max(us):8.1f}  ({a.iters} calls)", flush=True)


if __name__ == "__main__":
    main()
