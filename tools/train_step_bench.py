"""Training-step timing (BASELINE config 3 shape, one GPU): ResNet-50 trunk + proj -> IPM warp -> head.

    python tools/train_step_bench.py [--steps 5] [--bevnet] [--amp] [--fp32-kernels] [--torch-targets | --ab-targets R]
                                        [--native-adam | --ab-adam R]

Default: the hot path alone -- CNNEncoder (trunk trainable, native forward + backward) -> fused warp
+ mean (native forward + backward) -> sum(out * r) -> Adam step.  --bevnet: the full BEVNet (encoder,
per-view warp, concat, BEV proj, CenterNet head, focal/L1 loss) with the reference's training step
(train.py:249-255, fp32; --amp: the RUNTIME.USE_AMP branch, autocast(float16) + GradScaler, train.py:238-247,
with fp16-operand convs unless --fp32-kernels).  7 cameras x 3 x 1080 x 1920 synthetic images, Appendix-B rig, B = 1.
Prints one JSON line: ms per training step and frames/s.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd"))

import torch  # noqa: E402

import bev_rig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bevnet", action="store_true")
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--proj-ch", type=int, default=128, help="BEVNet BEV_PROJ_CH (configs/wildtrack.yaml:14: 128)")
    ap.add_argument("--fp32-kernels", action="store_true")
    ap.add_argument("--tune", action="append", default=[], metavar="NAME=V", help="bev_tune knob (A/B); repeatable")
    ap.add_argument("--no-mask-bytes", action="store_true", help="A/B: bn3's backward re-reads the fp32 block output "
                    "instead of the forward's ReLU mask bytes (trunk_grad.RELU_MASK_BYTES)")
    ap.add_argument("--torch-loss", action="store_true", help="A/B: the focal and L1 losses as torch ops")
    ap.add_argument("--torch-targets", action="store_true", help="A/B: the CenterNet targets as torch ops "
                    "(model_wrapper.NATIVE_TARGETS off)")
    ap.add_argument("--ab-targets", type=int, default=0, metavar="ROUNDS", help="A/B in one process: ROUNDS times a "
                    "native-targets run then a torch-targets run of --steps steps each, one JSON line per run")
    ap.add_argument("--native-adam", action="store_true", help="bev_optim.Adam (one launch per step, no GradScaler "
                    "host wait) in place of torch.optim.Adam")
    ap.add_argument("--ab-adam", type=int, default=0, metavar="ROUNDS", help="A/B in one process: ROUNDS times a "
                    "torch.optim.Adam run then a bev_optim.Adam run of --steps steps each, one JSON line per run")
    ap.add_argument("--eager-decode", action="store_true", help="A/B: BEVNet.forward synchronises on its decode")
    ap.add_argument("--loss-graph", action="store_true", help="A/B: BEVNet.loss as a replayed graph pair "
                    "(model_wrapper.LOSS_GRAPHS)")
    ap.add_argument("--device-targets", action="store_true", help="A/B: the targets already on the device (the "
                    "reference's loop, train.py:228-243, leaves them in host memory)")
    ap.add_argument("--no-pool-arg", action="store_true", help="A/B: the stem max-pool saves its input and the backward "
                    "re-scans it for the argmax instead of taking the forward's argmax bytes (trunk_grad.MAXPOOL_ARG)")
    a = ap.parse_args()
    import bev_native
    import bev_optim
    bev_native.AMP_HALF_CONVS = not a.fp32_kernels
    if a.no_mask_bytes:
        from models.encoders import trunk_grad
        trunk_grad.RELU_MASK_BYTES = False
    if a.no_pool_arg:
        from models.encoders import trunk_grad
        trunk_grad.MAXPOOL_ARG = False
    import models.model_wrapper as _mw
    _mw.LAZY_DECODE = not a.eager_decode
    _mw.NATIVE_LOSS = not a.torch_loss
    _mw.NATIVE_TARGETS = not a.torch_targets
    _mw.LOSS_GRAPHS = a.loss_graph
    for kv in a.tune:
        name, v = kv.split("=")
        bev_native.tune(getattr(bev_native, "TUNE_" + name.upper()), int(v))
    scaler = torch.amp.GradScaler("cuda") if a.amp else None
    arm = {"adam": "native" if a.native_adam else "torch"}  # which optimizer step() uses (each keeps its own state)
    dev = torch.device("cuda:0")
    V, H, W = 7, 1080, 1920
    K, Rt = bev_rig.rig(V, H, W, 1)
    Kd, Rtd = torch.from_numpy(K).to(dev), torch.from_numpy(Rt).to(dev)
    images = torch.randn(1, V, 3, H, W, device=dev)
    if a.bevnet:
        from models.model_wrapper import BEVNet
        cfg = {"MODEL": {"BACKBONE": a.backbone, "PRETRAINED": False, "FEAT_DIM": 64, "OUT_INDEX": 2,
                         "BEV_SIZE": [32, 480, 1440], "BEV_BOUNDS": [-24.0, 24.0, -7.2, 7.2], "BEV_PROJ_CH": a.proj_ch},
               "LOSS": {}, "EVAL": {"CONF_THRESH": 0.99}}
        model = BEVNet(cfg).to(dev)
        batch = {"images": images, "calib": {"intrinsic": Kd, "extrinsic": Rtd}}
        # the loader's targets stay in host memory, as in the reference's loop (train.py:228-243 moves only the
        # images and the calibration)
        targets = [{"boxes_world": torch.tensor([[1.0, 0.5, 0.6, 0.6], [-3.0, 2.0, 0.6, 0.6]],
                                                device=dev if a.device_targets else "cpu")}]
        with torch.no_grad():
            model.eval()(batch)
        model.train()
        opts = {"torch": torch.optim.Adam(model.parameters(), lr=1e-4),
                "native": bev_optim.Adam(model.parameters(), lr=1e-4)}

        def step():
            opt = opts[arm["adam"]]
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=scaler is not None):
                loss = model.loss(model(batch), targets, {})["total_loss"]
            if scaler is None:
                loss.backward()
                opt.step()
            else:
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()
            return loss
    else:
        from models.encoders.cnn_encoder import CNNEncoder
        from models.fusion.geometry import GeometryTransformer
        enc = CNNEncoder(out_channels=64, backbone=a.backbone, pretrained=False).to(dev)
        geom = GeometryTransformer(480, 1440, (-24.0, 24.0, -7.2, 7.2))
        with torch.no_grad():
            enc.eval()(images)
        enc.train()
        opts = {"torch": torch.optim.Adam(enc.parameters(), lr=1e-4),
                "native": bev_optim.Adam(enc.parameters(), lr=1e-4)}
        r = torch.randn(1, 64, 480, 1440, device=dev)

        def step():
            opt = opts[arm["adam"]]
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=scaler is not None):
                out = geom.forward_fused(enc(images), Kd, Rtd, (H, W), "mean")
                loss = (out.float() * r).sum()
            if scaler is None:
                loss.backward()
                opt.step()
            else:
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()
            return loss
    for _ in range(a.warmup):
        step()

    def run(native_targets: bool, adam: str = arm["adam"]):
        _mw.NATIVE_TARGETS = native_targets
        arm["adam"] = adam
        step()  # the arm's own first step (workspace, allocator) stays out of the timing
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        updated = [p for g in opts[adam].param_groups for p in g["params"] if p.grad is not None]
        print(json.dumps({"what": "bevnet train step" if a.bevnet else "hot-path train step", "backbone": a.backbone,
                          "tune": a.tune, "bev": [480, 1440], "cameras": V, "img": [H, W], "feat_dim": 64,
                          "bev_proj_ch": a.proj_ch if a.bevnet else None,
                          "amp": a.amp, "half_convs": a.amp and not a.fp32_kernels,
                          "decode": "eager" if a.eager_decode else "lazy",
                          "loss_impl": "torch" if a.torch_loss else "native",
                          "targets_impl": "native" if native_targets else "torch",
                          "targets": "device" if a.device_targets else "host", "adam_impl": adam,
                          "adam_tensors": len(updated), "adam_elems": sum(p.numel() for p in updated),
                          "ms_per_step": round(dt * 1e3, 2), "frames_per_s": round(1.0 / dt, 3),
                          "loss": float(loss)}), flush=True)

    if a.ab_adam:
        for _ in range(a.ab_adam):
            run(not a.torch_targets, "torch")
            run(not a.torch_targets, "native")
    elif a.ab_targets:
        for _ in range(a.ab_targets):
            run(True)
            run(False)
    else:
        run(not a.torch_targets)

if __name__ == "__main__":
    main()
