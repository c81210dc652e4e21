"""Interleaved A/B of the encoder's conv arithmetics on the bench workload (7 cams x 1080p x 2 frames, eval; ResNet-50
by default, --backbone efficientnet_b0 / efficientnet_b3 for the EfficientNet trunks).

    python tools/encoder_f16_ab.py bf16x6 f16 --iters 10 --rounds 5
    python tools/encoder_f16_ab.py --layers f16 --iters 5          # per-launch table, one stream group
    python tools/encoder_f16_ab.py --backbone efficientnet_b3 --layers f16

Same pattern as tools/encoder_ab.py: the arithmetics alternate inside one process (same clocks, same caches), each timed
with HIP events around `iters` CNNEncoder.forward calls after one warm-up call (which also packs that arithmetic's
panels).  The outputs of different arithmetics are not compared bitwise (they differ by construction): the relative
L2 distance to the first one is printed instead.  Prints one line per (round, arithmetic), the median per arithmetic
and the ratio of the medians to the first.

--layers MODE: every launch of the trunk + proj in that arithmetic (ResNet: the convs; EfficientNet: stem, depthwise, fused
expansion + depthwise, SE gate, pointwise), one stream group, timed with a pair of HIP
events around the launch (mean of `iters` forwards): shape, microseconds, the bytes the launch has to move (operand +
panel + residual + output, each once) and their rate, and the matrix-core rate of its 2 M N K flops.
"""
import argparse
import collections
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))

import torch  # noqa: E402

import bev_native as nat  # noqa: E402
from models.encoders.cnn_encoder import CNNEncoder  # noqa: E402


def layer_table(enc, imgs, mode, iters):
    rows = collections.OrderedDict()
    calls = []

    def wrap(name, shape_of):
        orig = getattr(nat, name)

        def f(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = orig(*a, **k)
            e1.record()
            calls.append((name, shape_of(a, k, y), e0, e1))
            return y
        setattr(nat, name, f)
        return orig

    def bytes_of(*ts):
        return sum(t.numel() * t.element_size() for t in ts if isinstance(t, torch.Tensor))

    def conv_shape(a, k, y):  # conv2d_h16_half(x, packed, bias, Co, KH, KW, stride, pad, ...)
        x, Co, KH, st = a[0], a[3], a[4], a[6]
        M = y.shape[0] * y.shape[1] * y.shape[2]
        desc = f"{KH}x{KH} s{st} {x.shape[3]:4d}->{Co:4d} {str(x.dtype)[-7:]}->{str(y.dtype)[-7:]}"
        return desc, M, Co, KH * KH * x.shape[3], bytes_of(x, a[1], k.get("residual")) + M * Co * y.element_size()

    def any_shape(a, k, y):  # conv2d_h16_any(x, packed, Co, KH, KW, stride, pad, ...)
        x, Co, KH, st = a[0], a[2], a[3], a[5]
        M = y.shape[0] * y.shape[1] * y.shape[2]
        desc = f"{KH}x{KH} s{st} {x.shape[3]:4d}->{Co:4d} {str(x.dtype)[-7:]}->{str(y.dtype)[-7:]}"
        return desc, M, Co, KH * KH * x.shape[3], bytes_of(x, a[1], k.get("residual")) + M * Co * y.element_size()

    def x6_shape(a, k, y):  # conv2d_nhwc_x6(x, packed6, bias, Co, KH, KW, stride, pad, ...)
        x, Co, KH, st = a[0], a[3], a[4], a[6]
        if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
            return "split operand", 0, 0, 0, 0
        M = y.shape[0] * y.shape[1] * y.shape[2]
        desc = f"{KH}x{KH} s{st} {x.shape[3]:4d}->{Co:4d} float32->float32"
        return desc, M, Co, KH * KH * x.shape[3], bytes_of(x, a[1], k.get("residual")) + M * Co * 4

    def stem_shape(a, k, y):
        x = a[0]
        return "stem 7x7 s2 + max-pool 3->64", 0, 0, 0, bytes_of(x, y)

    # EfficientNet launches (both arithmetics); y is (y, SE partials) for the depthwise forms
    def first(y):
        return y[0] if isinstance(y, tuple) else y

    def dt(t):
        return "f16" if t.dtype == torch.float16 else "f32"

    def stem3_shape(a, k, y):  # conv2d_stem3[_h16](x, wt, bias, act)
        M = y.shape[0] * y.shape[1] * y.shape[2]
        return f"stem 3x3 s2    3->{y.shape[3]:4d} f32->{dt(y)}", M, y.shape[3], 27, bytes_of(a[0], y)

    def ir_shape(a, k, y):  # ir_expand_dw[_h16](x, we, be, wd, bd, K, stride)
        x, K, st, y = a[0], a[5], a[6], first(y)
        M, Min = y.shape[0] * y.shape[1] * y.shape[2], x.shape[0] * x.shape[1] * x.shape[2]
        desc = f"expand+dw {K}x{K} s{st} {x.shape[3]:4d}->{y.shape[3]:4d} {dt(x)}->{dt(y)}"
        return desc, M, y.shape[3], round(x.shape[3] * Min / M) + K * K, bytes_of(x, a[1], a[3], y)

    def dw_shape(a, k, y):  # dwconv2d_nhwc[_h16](x, wt, bias, K, stride, pad, act)
        x, K, st, y = a[0], a[3], a[4], first(y)
        M = y.shape[0] * y.shape[1] * y.shape[2]
        return f"dw {K}x{K} s{st} {x.shape[3]:4d} {dt(x)}->{dt(y)}", M, y.shape[3], K * K, bytes_of(x, a[1], y)

    def gate_shape(a, k, y):  # se_gate(psum, hw, w1, b1, w2, b2)
        return f"se gate {a[0].shape[2]:4d} ({a[0].shape[1]} partials)", 0, 0, 0, bytes_of(a[0], a[2], a[4], y)

    def pw16_shape(a, k, y):  # conv2d_pw_h16(x, w, bias, gate=, residual=, f32_out=)
        x = a[0]
        M = y.shape[0] * y.shape[1] * y.shape[2]
        desc = (f"1x1 {x.shape[3]:4d}->{y.shape[3]:4d} f16->{dt(y)}{' gate' if k.get('gate') is not None else ''}"
                f"{' skip' if k.get('residual') is not None else ''}")
        return desc, M, y.shape[3], x.shape[3], bytes_of(x, a[1], k.get("residual"), y)

    def nhwc_shape(a, k, y):  # conv2d_nhwc(x, packed, bias, Co, KH, KW, stride, pad, relu, residual=, ascale=)
        x, Co, KH = a[0], a[3], a[4]
        M = y.shape[0] * y.shape[1] * y.shape[2]
        desc = (f"{KH}x{KH} {x.shape[3]:4d}->{Co:4d} f32->f32{' gate' if k.get('ascale') is not None else ''}"
                f"{' skip' if k.get('residual') is not None else ''}")
        return desc, M, Co, KH * KH * x.shape[3], bytes_of(x, k.get("residual"), y) + 4 * Co * KH * KH * x.shape[3]

    saved = {"conv2d_h16_half": wrap("conv2d_h16_half", conv_shape), "conv2d_h16_any": wrap("conv2d_h16_any", any_shape),
             "conv2d_nhwc_x6": wrap("conv2d_nhwc_x6", x6_shape), "conv2d_stem_pool_x6": wrap("conv2d_stem_pool_x6", stem_shape)}
    for name, shape_of in (("conv2d_stem3", stem3_shape), ("conv2d_stem3_h16", stem3_shape), ("ir_expand_dw", ir_shape),
                           ("ir_expand_dw_h16", ir_shape), ("dwconv2d_nhwc", dw_shape), ("dwconv2d_nhwc_h16", dw_shape),
                           ("se_gate", gate_shape), ("conv2d_pw_h16", pw16_shape), ("conv2d_nhwc", nhwc_shape)):
        saved[name] = wrap(name, shape_of)
    try:
        with torch.no_grad(), nat.conv_arith_mode(mode):
            enc(imgs)
            torch.cuda.synchronize()
            calls.clear()
            for _ in range(iters):
                enc(imgs)
            torch.cuda.synchronize()
    finally:
        for n, f in saved.items():
            setattr(nat, n, f)
    per = len(calls) // iters
    for i, (name, sh, e0, e1) in enumerate(calls):
        rows.setdefault(i % per, (name, sh, []))[2].append(e0.elapsed_time(e1) * 1e3)
    print(f"{'#':>3s} {'launch':42s} {'M':>8s} {'us':>8s} {'MB':>8s} {'TB/s':>6s} {'TFLOP/s':>8s}")
    tot = 0.0
    for i, (name, (desc, M, N, K, nbytes), us) in rows.items():
        u = statistics.median(us)
        tot += u
        print(f"{i:3d} {desc:42s} {M:8d} {u:8.1f} {nbytes / 1e6:8.1f} {nbytes / u / 1e6:6.2f} "
              f"{2.0 * M * N * K / u / 1e6:8.1f}", flush=True)
    print(f"total of the launches' event intervals {tot:8.1f} us ({per} launches per forward, arithmetic {mode})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("modes", nargs="*", default=["bf16x6", "f16"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--stream-groups", type=int, default=2)
    ap.add_argument("--layers", action="store_true", help="per-launch table of the first arithmetic, one stream group")
    a = ap.parse_args()
    for m in a.modes:
        if m not in nat.CONV_ARITHS:
            raise SystemExit(f"unknown arithmetic {m}; have {nat.CONV_ARITHS}")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    enc = CNNEncoder(out_channels=64, backbone=a.backbone, pretrained=False).eval().to(dev)
    imgs = torch.randn(a.frames, 7, 3, 1080, 1920, device=dev)
    resnet = a.backbone.startswith("resnet")  # stream groups: the ResNet plan's
    if a.layers:
        if resnet:
            enc.backbone.stream_groups = 1
        layer_table(enc, imgs, a.modes[0], a.iters)
        return
    if resnet:
        enc.backbone.stream_groups = a.stream_groups
    res = {n: [] for n in a.modes}
    first = None
    with torch.no_grad():
        for rnd in range(a.rounds):
            for name in a.modes:
                with nat.conv_arith_mode(name):
                    out = enc(imgs)  # warm-up (and this arithmetic's panels on the first round)
                    torch.cuda.synchronize()
                    if first is None:
                        first = out.clone()
                    elif rnd == 0:
                        d = float((out.double() - first.double()).norm() / first.double().norm())
                        print(f"{name}: relative L2 distance to {a.modes[0]} {d:.3e}", flush=True)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        enc(imgs)
                    e1.record()
                    torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.iters
                res[name].append(ms)
                print(f"round {rnd} {name:8s} {ms:8.3f} ms/step", flush=True)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        print(f"median {n:8s} {med[n]:8.3f} ms  min {min(v):8.3f}  ratio to {a.modes[0]} {med[n] / med[a.modes[0]]:.3f}",
              flush=True)


if __name__ == "__main__":
    main()
