"""Interleaved A/B of the BEV head's inference arithmetics on the flagship grid (2 frames x 480 x 1440 cells,
in_channels = 130 = BEV_PROJ_CH 128 + the position encoding).

    python tools/head_f16_ab.py --iters 10 --rounds 5 [--out profiles/NAME.txt]

Same pattern as tools/encoder_f16_ab.py: the arithmetics ("f32", the default, and "f16") alternate inside one process
(same clocks, same caches), each timed with HIP events around `iters` BEVDetector.forward_nhwc calls on a resident
operand of that arithmetic's width (operand_channels()) after one warm-up call, which also packs that arithmetic's
panels.  The outputs differ by construction; the relative L2 distance of the 5-channel output to the default's is
printed.  Prints one line per (round, arithmetic), the median, minimum, maximum and spread per arithmetic, the ratio
of the medians, and per arithmetic the per-launch table (bev_native's launch spans: a pair of HIP events around each
conv and each GroupNorm statistics call; median over `iters` forwards) with the matrix-core rate of each conv's
2 M N K flops.  Only the eval head runs: no encoder, warp or decode.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))

import torch  # noqa: E402

import bev_native as nat  # noqa: E402
from models.heads.detector import BEVDetector  # noqa: E402


def launch_table(det, x, mode, iters, emit):
    with torch.no_grad(), nat.head_arith_mode(mode):
        det.forward_nhwc(x)
        torch.cuda.synchronize()
        nat.spans_start()
        for _ in range(iters):
            det.forward_nhwc(x)
        spans = nat.spans_stop()
    B, H, W, cw = x.shape
    M = B * H * W
    convs = [(cw, 512), (512, 128), (128, 128), (128, 5)]
    emit(f"per-launch, arithmetic {mode} (median of {iters} forwards, event pair around each launch)")
    tot = 0.0
    per = len(spans["conv"]) // iters
    for i in range(per):
        us = statistics.median(spans["conv"][i::per]) * 1e3
        tot += us
        ci, co = convs[i]
        emit(f"  conv{i + 1} 3x3 {ci:4d}->{co:4d} M {M:8d} {us:9.1f} us {2.0 * M * co * 9 * ci / us / 1e6:8.1f} TFLOP/s")
    per = len(spans["groupnorm"]) // iters
    for i in range(per):
        us = statistics.median(spans["groupnorm"][i::per]) * 1e3
        tot += us
        emit(f"  groupnorm statistics {i + 1} ({convs[i][1]:4d} channels) {us:9.1f} us")
    emit(f"  total of the launches' event intervals {tot:9.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("modes", nargs="*", default=["f32", "f16"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--grid", type=int, nargs=2, default=[480, 1440])
    ap.add_argument("--in-channels", type=int, default=130)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    for m in a.modes:
        if m not in nat.HEAD_ARITHS:
            raise SystemExit(f"unknown head arithmetic {m}; have {nat.HEAD_ARITHS}")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    torch.manual_seed(0)
    H, W = a.grid
    det = BEVDetector(in_channels=a.in_channels, bev_size=(H, W)).eval().to(dev)
    with torch.no_grad():  # every parameter random: the CenterNet init zeroes the offset head
        for h in (det.heatmap_head, det.offset_head, det.size_head):
            h.weight.normal_(0.0, 0.05)
    feat = torch.randn(a.frames, H, W, a.in_channels, device=dev)
    ops = {}
    with torch.no_grad():
        for m in a.modes:
            with nat.head_arith_mode(m):
                x = torch.zeros(a.frames, H, W, det.operand_channels(), device=dev)
            x[..., :a.in_channels] = feat
            ops[m] = x
    del feat
    emit(f"tools/head_f16_ab.py {' '.join(a.modes)} --iters {a.iters} --rounds {a.rounds}: BEVDetector.forward_nhwc, eval, "
         f"{a.frames} x {H} x {W} cells, in_channels {a.in_channels} "
         f"(operand widths {', '.join(f'{m} {ops[m].shape[-1]}' for m in a.modes)}), {torch.cuda.get_device_name(0)}")
    res = {n: [] for n in a.modes}
    first = None
    with torch.no_grad():
        for rnd in range(a.rounds):
            for name in a.modes:
                with nat.head_arith_mode(name):
                    out = det.forward_nhwc(ops[name])  # warm-up (and this arithmetic's panels on the first round)
                    y = torch.cat([out["heatmap_logits"], out["offset_raw"], out["size_raw"]], dim=1)
                    torch.cuda.synchronize()
                    if first is None:
                        first = y.double()
                    elif rnd == 0:
                        d = float((y.double() - first).norm() / first.norm())
                        emit(f"{name}: relative L2 distance of the 5-channel output to {a.modes[0]} {d:.3e}")
                    del out, y
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        det.forward_nhwc(ops[name])
                    e1.record()
                    torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.iters
                res[name].append(ms)
                emit(f"round {rnd} {name:4s} {ms:8.3f} ms/forward")
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        emit(f"median {n:4s} {med[n]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  spread {max(v) - min(v):6.3f}  "
             f"ratio to {a.modes[0]} {med[n] / med[a.modes[0]]:.3f}")
    for n in a.modes:
        launch_table(det, ops[n], n, a.iters, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
