"""Operands cached from parameters and buffers against the writers that bypass torch.

Every inference path keeps operands derived from its parameters and buffers -- packed MFMA panels, BatchNorm-folded
weights and biases, fp16-rounded copies -- each under a key (t.data_ptr(), t._version).  torch's in-place ops advance
the version counter; the native writers go through raw pointers and have to do it themselves
(bev_native.mark_written): bev_optim's Adam / AdamW step and the train-mode BatchNorm's running-statistics update.

Pattern of every case: build module A; run it once in eval mode (fills the caches, as bev_dist.materialize_lazy does);
apply a writer; run A again; compare with a twin -- a fresh instance of the same class, its lazy layers created by one
forward, loaded with A's state_dict() through load_state_dict (copy_, which advances versions), so it runs the same
kernels on the same operand bits.

  1. A's output equals the twin's bit for bit.
  2. The case is not vacuous: the twin's output differs from A's output before the writer by more than 100 x the
     float64 bar the suite uses for that module.  fp32-class modules (test_backbone_gpu.py, test_head_gpu.py):
     max |d| > 100 * 1e-4 * max |out|.  "f16" arithmetics (test_encoder_f16_gpu.py, test_encoder_effnet_f16_gpu.py,
     test_head_f16_gpu.py): those tests carry two bars, 1.5 x the relative L2 error and 2 x the max error of the
     float64 restatement R64 of the fp16 roundings; the criterion here is the first one, relL2(d) > 100 * 1.5 *
     relL2(R64 - exact), computed from the twin's state with those tests' own restatements.  (100 x the second bar is
     200 x an error of up to one fp16 ulp of the largest output and more after several layers: it can exceed the
     output's whole range, which no writer could meet.)
  3. Float64 anchor, single layer and head: the twin against float64 torch on the CPU built from the same state, with
     the bar and the helper of the module's own test, so the bit comparison is not of two equally wrong results.

Writers
  W1  bev_optim.Adam / AdamW, one step, lr 1e-2, p.grad = randn assigned by hand; plain and through
      torch.amp.GradScaler("cuda").
  W2  W1 through a scaler whose scaled gradients overflow (found_inf set): nothing moves; the output equals the twin's
      and the output before the writer (a re-pack is allowed).
  W3  the native BatchNorm running statistics: one train() forward with batch statistics, every parameter
      requires_grad False, under no_grad (the frozen-trunk configuration) -- bev_native.batchnorm_train_fwd; the same
      under autocast(float16) -- batchnorm_finalize_tiles where the fp16 conv takes the statistics in its epilogue.
      Single layer: both entries called directly, momentum 0.5.
  W4  control: mul_ / add_ under no_grad, and load_state_dict.

Sites: VERSION_KEY_SITES below -- every `._version` read of the package, by file, with the cases that cover it
(tests/test_weight_cache_host.py pins the counts to the code, so a new cache cannot appear without a case here).
"""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-2
NONVACUOUS = 100.0

# file (under the package) -> (number of `._version` reads, the caches they key, the cases below that cover them)
VERSION_KEY_SITES = {
    "models/encoders/resnet.py": (2, "FoldedConv.prepare: a, b, d (_fproj, _fb); FoldedTail.prepare: b"),
    "models/encoders/efficientnet.py": (4, "FoldedDW.prepare, _stem3_key, ('irw', ..): c default; ('h16', ..): c f16"),
    "models/encoders/cnn_encoder.py": (2, "_proj_h16 (weight and bias, one line): d efficientnet f16"),
    "models/heads/detector.py": (2, "_Packed.get: e f32 (_panels), e f16 (_panels_f16); _heads_f16: e f16"),
    "models/model_wrapper.py": (1, "BEVNet._view_panels: f, g (eval), h (training forward)"),
}


# ---------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# sites
# ---------------------------------------------------------------------------
class Site:
    """One cached path: build() a fresh module on the device in eval mode, run(m) -> list of output tensors."""
    conv_arith, head_arith = "bf16x6", "f32"
    has_bn = False   # W3 reaches it
    anchored = False  # has a float64 anchor

    @property
    def f16(self):
        return self.conv_arith == "f16" or self.head_arith == "f16"

    def _input(self, shape, seed):
        self._x, self._x_spec = None, (shape, seed)

    @property
    def x(self):
        """The site's input, created on the device at first use (collection needs no GPU)."""
        if self._x is None:
            shape, seed = self._x_spec
            self._x = torch.randn(*shape, generator=_gen(seed)).to(DEV)
        return self._x

    @contextlib.contextmanager
    def modes(self):
        import bev_native as nat
        with nat.conv_arith_mode(self.conv_arith), nat.head_arith_mode(self.head_arith):
            yield

    def eval_run(self, m):
        m.eval()
        with torch.no_grad(), self.modes():
            outs = self.run(m)
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs]

    def train_run(self, m, autocast):
        """W3: one train() forward with batch statistics, nothing trainable, no autograd."""
        for p in m.parameters():
            p.requires_grad_(False)
        m.train()
        with torch.no_grad(), self.modes(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            self.run(m)
        m.eval()

    def r64_rel_l2(self, twin):
        """relL2(R64 - exact) of the f16 arithmetic on the twin's state (the module's own test's restatement)."""
        raise NotImplementedError

    def anchor(self, twin, outs):
        raise NotImplementedError


class _Layer(torch.nn.Module):
    """conv 64 -> 64, 3x3, + BatchNorm through one FoldedConv (the ResNet trunk's executor)."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False)
        self.bn = torch.nn.BatchNorm2d(64)
        self._fc = None

    def forward(self, x):
        from models.encoders.resnet import FoldedConv
        if self._fc is None:
            self._fc = FoldedConv(self.conv, self.bn, split_ok=True, half_ok=True)
        return self._fc(x, relu=True)


class LayerSite(Site):
    has_bn = anchored = True

    def __init__(self, arith):
        self.conv_arith = arith
        self.name = f"a_foldedconv_{arith}"
        self._input((2, 9, 11, 64), 2)

    def build(self):
        torch.manual_seed(1)
        return _Layer().eval().to(DEV)

    def run(self, m):
        return [m(self.x)]

    def _refs(self, twin):
        from test_encoder_f16_gpu import _fold
        x = self.x.double().cpu().permute(0, 3, 1, 2)
        w, b = _fold(twin.conv, twin.bn, torch.float64, "cpu")
        exact = F.conv2d(x, w, b, 1, 1).clamp_min(0).permute(0, 2, 3, 1)
        w, b = _fold(twin.conv, twin.bn, torch.float32, "cpu")  # folded in fp32, rounded once by the pack
        r64 = F.conv2d(x.half().double(), w.half().double(), b.double(), 1, 1).clamp_min(0).half().double()
        return exact, r64.permute(0, 2, 3, 1)

    def r64_rel_l2(self, twin):
        exact, r64 = self._refs(twin)
        return _rel_l2(r64, exact)

    def anchor(self, twin, outs):
        exact, r64 = self._refs(twin)
        got = outs[0].double().cpu()
        assert got.shape == exact.shape
        if not self.f16:  # test_backbone_gpu.py: max |err| <= 1e-4 * max |ref|
            err, lim = float((got - exact).abs().max()), 1e-4 * float(exact.abs().max())
            print(f"  anchor {self.name}: max|err| {err:.3e} bar {lim:.3e}")
            assert err <= lim
            return
        l2n, l2r = _rel_l2(got, exact), _rel_l2(r64, exact)  # test_encoder_f16_gpu.py (g)
        mxn, mxr = float((got - exact).abs().max()), float((r64 - exact).abs().max())
        print(f"  anchor {self.name}: relL2 native {l2n:.3e} R64 {l2r:.3e}; max native {mxn:.3e} R64 {mxr:.3e}")
        assert l2r > 1e-5 and l2n <= 1.5 * l2r and mxn <= 2.0 * mxr


def _identity_proj(C):
    proj = torch.nn.Conv2d(C, C, 1)
    with torch.no_grad():
        proj.weight.copy_(torch.eye(C).view(C, C, 1, 1))
        proj.bias.zero_()
    return proj


class _Shim:
    """What the encoder tests' float64 restatements read of a CNNEncoder, around a bare trunk: the identity as the
    proj (exact in fp16, so the restatement's proj step returns the trunk output)."""

    def __init__(self, backbone, C):
        self.backbone, self.proj, self.out_index = backbone, _identity_proj(C), 2


class TrunkSite(Site):
    has_bn = True

    def __init__(self, kind, arith, groups=None):
        self.kind, self.conv_arith, self.groups = kind, arith, groups
        self.name = f"{'b' if kind == 'resnet50' else 'c'}_{kind}_{arith}" + (f"_sg{groups}" if groups else "")
        self._input((2, 3, 64, 96), 3)

    def build(self):
        from models.encoders.efficientnet import efficientnet_b0
        from models.encoders.resnet import resnet50
        torch.manual_seed(4)
        m = (resnet50 if self.kind == "resnet50" else efficientnet_b0)().eval().to(DEV)
        if self.groups:
            m.stream_groups = self.groups
        return m

    def run(self, m):
        return [m.forward_features_nhwc(self.x, 2)]

    def r64_rel_l2(self, twin):
        if self.kind == "resnet50":
            from test_encoder_f16_gpu import _forward64
        else:
            from test_encoder_effnet_f16_gpu import _forward64
        C = 512 if self.kind == "resnet50" else twin.feature_channels[2]
        shim = _Shim(twin, C)
        return _rel_l2(_forward64(shim, self.x, True), _forward64(shim, self.x, False))


class EncoderSite(Site):
    def __init__(self, tag, backbone, impl, arith):
        self.backbone, self.impl, self.conv_arith = backbone, impl, arith
        self.has_bn = impl != "fallback"
        self.name = f"d_encoder_{tag}"
        self._input((2, 3, 64, 96), 5)

    def build(self):
        from models.encoders.cnn_encoder import CNNEncoder
        torch.manual_seed(6)
        return CNNEncoder(out_channels=16, backbone=self.backbone, pretrained=False, out_index=2,
                          backbone_impl=self.impl).eval().to(DEV)

    def run(self, m):
        return [m(self.x)]  # [1, 2, 16, Hf, Wf]

    def r64_rel_l2(self, twin):
        if self.backbone.startswith("resnet"):
            from test_encoder_f16_gpu import _forward64
        else:
            from test_encoder_effnet_f16_gpu import _forward64
        return _rel_l2(_forward64(twin, self.x, True), _forward64(twin, self.x, False))


class HeadSite(Site):
    anchored = True
    CIN, H, W = 18, 12, 20

    def __init__(self, arith):
        self.head_arith = arith
        self.name = f"e_head_{arith}"
        self._input((1, self.H, self.W, self.CIN), 7)

    def build(self):
        from models.heads.detector import BEVDetector
        torch.manual_seed(8)
        return BEVDetector(in_channels=self.CIN, bev_size=(self.H, self.W)).eval().to(DEV)

    def run(self, m):
        x = F.pad(self.x, (0, m.operand_channels() - self.CIN)).contiguous()
        out = m.forward_nhwc(x)
        return [out["heatmap_logits"], out["offset_raw"], out["size_raw"]]

    @staticmethod
    def _y(outs):
        return torch.cat(outs, dim=1).permute(0, 2, 3, 1).double().cpu()  # [B, H, W, 5]

    def _refs(self, twin):
        from test_head_f16_gpu import _forward64
        det = copy.deepcopy(twin).cpu()
        x = self.x.cpu()
        return _forward64(det, x, False), _forward64(det, x, True)

    def r64_rel_l2(self, twin):
        exact, r64 = self._refs(twin)
        return _rel_l2(r64, exact)

    def anchor(self, twin, outs):
        if not self.f16:  # test_head_gpu.py: |got - ref| <= 1e-4 |ref| + 1e-4 max |ref|
            from test_head_gpu import close, reference_head
            ref, _ = reference_head(twin, self.x.double().cpu().permute(0, 3, 1, 2))
            for k, got in zip(("heatmap_logits", "offset_raw", "size_raw"), outs):
                close(got, ref[k], 1e-4, 1e-4, f"anchor {self.name} {k}")
            return
        exact, r64 = self._refs(twin)  # test_head_f16_gpu.py (d)
        got = self._y(outs)
        l2n, l2r = _rel_l2(got, exact), _rel_l2(r64, exact)
        mxn, mxr = float((got - exact).abs().max()), float((r64 - exact).abs().max())
        print(f"  anchor {self.name}: relL2 native {l2n:.3e} R64 {l2r:.3e}; max native {mxn:.3e} R64 {mxr:.3e}")
        assert l2r > 1e-5 and l2n <= 1.5 * l2r and mxn <= 2.0 * mxr


def _sites():
    s = [LayerSite(a) for a in ("f32", "bf16x6", "f16")]
    s += [TrunkSite("resnet50", a, g) for a in ("f32", "bf16x6", "f16") for g in (1, 2)]
    s += [TrunkSite("efficientnet_b0", a) for a in ("bf16x6", "f16")]
    s += [EncoderSite("resnet18_fproj", "resnet18", "native", "bf16x6"),
          EncoderSite("resnet18_fproj_f16", "resnet18", "native", "f16"),
          EncoderSite("effnet_b0_proj_h16", "efficientnet_b0", "native", "f16"),
          EncoderSite("fallback_fb", "resnet18", "fallback", "bf16x6")]
    s += [HeadSite("f32"), HeadSite("f16")]
    return s


SITES = {s.name: s for s in _sites()}
BN_SITES = [n for n, s in SITES.items() if s.has_bn]
MODULE_BN_SITES = [n for n in BN_SITES if not isinstance(SITES[n], LayerSite)]
LAYER_SITES = [n for n, s in SITES.items() if isinstance(s, LayerSite)]


# ---------------------------------------------------------------------------
# the pattern
# ---------------------------------------------------------------------------
def _moved(site, twin, y0, yT):
    """Requirement 2's figures: (how far the twin's output is from A's before the writer, the bar) per output."""
    if site.f16:
        cat = (lambda ys: torch.cat([y.double().reshape(-1) for y in ys]))
        return [(_rel_l2(cat(y0), cat(yT)), 1.5 * site.r64_rel_l2(twin))]
    return [(float((t.double() - a.double()).abs().max()), 1e-4 * float(t.double().abs().max()))
            for a, t in zip(y0, yT)]


def coherence(site, writer, moves=True):
    A = site.build()
    y0 = site.eval_run(A)  # fills every cache
    state0 = {k: v.detach().clone() for k, v in A.state_dict().items()}
    writer(site, A)
    y1 = site.eval_run(A)
    T = site.build()
    site.eval_run(T)  # lazily built layers
    T.load_state_dict(A.state_dict())
    yT = site.eval_run(T)
    figures = _moved(site, T, y0, yT)
    for i, (d, bar) in enumerate(figures):
        print(f"  {site.name} output {i}: twin vs before the writer {d:.3e}, bar {bar:.3e}, margin "
              f"{d / bar if bar > 0 else float('inf'):.1f} x")
    if site.anchored:
        site.anchor(T, yT)
    if moves:
        for i, (d, bar) in enumerate(figures):
            assert d > NONVACUOUS * bar, f"{site.name} output {i}: vacuous, moved {d:.3e} <= 100 x {bar:.3e}"
    else:  # W2: nothing moved
        for k, v in A.state_dict().items():
            assert torch.equal(v, state0[k]), f"{site.name}: {k} moved under found_inf"
        for i, (a, b) in enumerate(zip(y1, y0)):
            assert _same_bits(a, b), f"{site.name} output {i}: differs from the output before the skipped step"
    for i, (a, t) in enumerate(zip(y1, yT)):
        assert _same_bits(a, t), (f"{site.name} output {i}: stale operands, {int((_bits(a) != _bits(t)).sum())} of "
                                  f"{a.numel()} values differ from the twin's, max |d| "
                                  f"{float((a.double() - t.double()).abs().max()):.3e}")


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------
def _assign_grads(params, scale):
    g = torch.Generator(device=DEV).manual_seed(9)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=DEV) * scale  # 2^127: |randn| >= 2 overflows to inf


def w1(cls_name, scaled, overflow=False):
    def writer(site, m):
        import bev_optim
        params = list(m.parameters())
        opt = getattr(bev_optim, cls_name)(params, lr=LR)
        scale = 2.0 ** 127 if overflow else 1024.0 if scaled else 1.0
        _assign_grads(params, scale)
        if scaled or overflow:
            scaler = torch.amp.GradScaler("cuda", init_scale=scale)
            scaler.scale(torch.zeros((), device=DEV))  # creates the scaler's device scalars
            scaler.step(opt)
            scaler.update()
            assert scaler.get_scale() == (scale / 2 if overflow else scale)
        else:
            opt.step()
        for p in params:
            p.grad = None
    return writer


def w3_train_forward(autocast):
    def writer(site, m):
        site.train_run(m, autocast)
    return writer


def w3_direct(entry):
    """The single layer: the two native entries that update running statistics, called on the layer's buffers."""
    def writer(site, m):
        import bev_native as nat
        bn = m.bn
        if entry == "train_fwd":
            z = (torch.randn(2, 9, 11, 64, generator=_gen(10)) * 1.5 + 0.3).to(DEV)
            nat.batchnorm_train_fwd(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, 0.5)
        else:  # the autocast path's pair: the fp16 conv with the statistics in its epilogue, then the finalize
            with nat._half_mode(True):
                packed = nat.pack_conv_weight(m.conv.weight.detach())
            z, tiles = nat.conv2d_nhwc_h16_bnstats(site.x * 2.0 + 0.3, packed, 64, 3, 3, 1, 1)
            nat.batchnorm_finalize_tiles(tiles, z.numel() // 64, bn.weight, bn.bias, bn.running_mean,
                                         bn.running_var, bn.eps, 0.5)
    return writer


def w4_inplace(site, m):
    g = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.1).add_(torch.randn(p.shape, generator=g, device=DEV) * LR)
        for name, b in m.named_buffers():
            if name.endswith("running_var"):
                b.mul_(1.2)
            elif name.endswith("running_mean"):
                b.add_(0.05)


def w4_load_state_dict(site, m):
    donor = site.build()
    site.eval_run(donor)
    w4_inplace(site, donor)
    m.load_state_dict(donor.state_dict())


W1_FORMS = [("Adam", False), ("Adam", True), ("AdamW", False), ("AdamW", True)]
W1_IDS = ["adam", "adam_scaler", "adamw", "adamw_scaler"]


@pytest.mark.parametrize("form", W1_FORMS, ids=W1_IDS)
@pytest.mark.parametrize("site", sorted(SITES))
def test_w1_native_adam_step(site, form):
    coherence(SITES[site], w1(*form))


@pytest.mark.parametrize("cls_name", ["Adam", "AdamW"])
@pytest.mark.parametrize("site", sorted(SITES))
def test_w2_found_inf_moves_nothing(site, cls_name):
    coherence(SITES[site], w1(cls_name, True, overflow=True), moves=False)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("site", sorted(MODULE_BN_SITES))
def test_w3_train_forward_running_statistics(site, autocast):
    coherence(SITES[site], w3_train_forward(autocast))


@pytest.mark.parametrize("entry", ["train_fwd", "finalize_tiles"])
@pytest.mark.parametrize("site", sorted(LAYER_SITES))
def test_w3_batchnorm_entries_on_one_layer(site, entry):
    coherence(SITES[site], w3_direct(entry))


@pytest.mark.parametrize("writer", [w4_inplace, w4_load_state_dict], ids=["inplace", "load_state_dict"])
@pytest.mark.parametrize("site", sorted(SITES))
def test_w4_control_torch_writers(site, writer):
    coherence(SITES[site], writer)


# ---------------------------------------------------------------------------
# (f), (g), (h): BEVNet after training steps
# ---------------------------------------------------------------------------
_BEVNET = {}
OUT_KEYS = ("heatmap_logits", "offset", "size")


def _bevnet_case(kind):
    """BEVNet (test_train.py's configuration, V = 3, 128 x 224): materialize_lazy, two bev_dist.train_step calls --
    "native": everything trainable, bev_optim.AdamW; "frozen": encoder.freeze() and torch.optim.Adam, so the only
    native writer is the trunk's train-mode BatchNorm -- then A's eval() forward and its train-mode loss with no step
    taken, and the same of the twin (the loss twice)."""
    if kind in _BEVNET:
        return _BEVNET[kind]
    import bev_dist
    import bev_optim
    import bev_rig
    from models.model_wrapper import BEVNet
    from test_train import _bevnet_cfg
    B, V, H, W = 1, 3, 128, 224
    K, Rt = bev_rig.rig(V, H, W, B)
    batch = {"images": torch.randn(B, V, 3, H, W, generator=_gen(1)).to(DEV),
             "calib": {"intrinsic": torch.from_numpy(K).to(DEV), "extrinsic": torch.from_numpy(Rt).to(DEV)}}
    targets = [{"boxes_world": torch.tensor([[1.0, 0.5, 0.6, 0.6], [-3.0, 2.0, 0.6, 0.6]], device=DEV)}]

    def build():
        torch.manual_seed(0)
        m = BEVNet(_bevnet_cfg()).to(DEV)
        if kind == "frozen":
            m.encoder.freeze()
        bev_dist.materialize_lazy(m, batch)  # one eval() forward: every cache holds the initial weights
        return m

    def eval_outputs(m):
        m.eval()
        with torch.no_grad():
            out = m(batch)
        torch.cuda.synchronize()
        return [out[k].detach().clone() for k in OUT_KEYS]

    def train_loss(m):
        m.train()
        preds = m(batch)
        loss = m.loss(preds, targets, {})["total_loss"].detach().double().cpu()
        torch.cuda.synchronize()
        return float(loss)

    A = build()
    y0 = eval_outputs(A)
    A.train()
    if kind == "native":
        opt = bev_optim.AdamW(A.parameters(), lr=LR)
    else:
        opt = torch.optim.Adam([p for p in A.parameters() if p.requires_grad], lr=LR)
    losses = [bev_dist.train_step(A, batch, targets, opt)["total_loss"] for _ in range(2)]
    opt.zero_grad(set_to_none=True)
    state = {k: v.detach().clone() for k, v in A.state_dict().items()}
    y1 = eval_outputs(A)
    loss_a = train_loss(A)
    T = build()
    T.load_state_dict(state)
    yT = eval_outputs(T)
    loss_t = [train_loss(T), train_loss(T)]
    res = dict(y0=y0, y1=y1, yT=yT, loss0=losses[0], loss_a=loss_a, loss_t=loss_t)
    _BEVNET[kind] = res
    return res


def _check_eval(res, what):
    for k, a0, a, t in zip(OUT_KEYS, res["y0"], res["y1"], res["yT"]):
        d, bar = float((t.double() - a0.double()).abs().max()), 1e-4 * float(t.double().abs().max())
        print(f"  {what} {k}: twin vs before training {d:.3e}, bar {bar:.3e}, margin {d / bar:.1f} x")
        assert d > NONVACUOUS * bar, f"{what} {k}: vacuous"
    for k, a, t in zip(OUT_KEYS, res["y1"], res["yT"]):
        assert _same_bits(a, t), (f"{what} {k}: eval() after training ran on stale operands, "
                                  f"{int((_bits(a) != _bits(t)).sum())} of {a.numel()} values differ from the "
                                  f"twin's, max |d| {float((a.double() - t.double()).abs().max()):.3e}")


@pytest.mark.timeout(240)
def test_f_bevnet_eval_after_native_adamw_steps():
    _check_eval(_bevnet_case("native"), "f_bevnet")


@pytest.mark.timeout(240)
def test_g_bevnet_eval_after_frozen_trunk_steps():
    _check_eval(_bevnet_case("frozen"), "g_bevnet_frozen")


@pytest.mark.timeout(240)
def test_h_bevnet_training_forward_after_native_adamw_steps():
    """The training forward reads BEVNet._view_panels too: after two native steps, A's train-mode loss (no step
    taken) against the twin's.  Allowed difference: the twin's own run-to-run difference.  On the MI355X the
    training forward and the loss are deterministic: the twin's two losses are equal to the last bit (run-to-run
    difference 0), so A's loss has to be the twin's exactly.  (Without the version advance in the optimizer step
    the first panels are kept: A then gave 7.4361 against its twin's 7.3333.)"""
    res = _bevnet_case("native")
    la, (t1, t2), l0 = res["loss_a"], res["loss_t"], res["loss0"]
    print(f"  h_bevnet loss: before training {l0!r}, A {la!r}, twin {t1!r} and {t2!r} (run to run {abs(t1 - t2):.3e})")
    assert abs(t1 - l0) > NONVACUOUS * 1e-4 * abs(t1), "vacuous: the loss did not move"
    assert abs(la - t1) <= abs(t1 - t2), f"training forward on stale panels: loss {la!r} vs the twin's {t1!r}"
