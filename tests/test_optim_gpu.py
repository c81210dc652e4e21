"""Adam / AdamW update on the device (k_adam_step, csrc/bev_optim.hip) against bev_adam_step_host -- the same
per-element function compiled for the CPU -- bit for bit on p, exp_avg, exp_avg_sq and the step counters (a NaN
matches a NaN: which NaN an operation returns is not part of the definition), and bev_optim.Adam on device parameters
against the numpy restatement of tests/test_optim_host.py.

Every tensor of the entry-level tests is carved from a larger buffer full of a sentinel, at a chosen element offset:
the 16-byte path, the dword path (one or all operands only 4-B aligned) and the tails are launched, and nothing
outside a tensor may change.  Sizes sit around the chunk (bev_adam_chunk_elems) and the 16-byte group."""
import numpy as np
import pytest
import torch

import bev_native
import bev_optim
from test_optim_host import (DECAYS, GRAD_SCALES, STEPS, F, check_step_equals_restatement, host_step, make_tensors,
                             poke_nonfinite, restate, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8           # sentinel elements on both sides of a carved tensor (a multiple of 4: offset 0 stays 16-B aligned)
SENTINEL = -12345.678
KEYS = ("p", "g", "m", "v")


def chunk():
    return bev_native.adam_chunk_elems()


class Carved:
    """Host tensors (dicts of float32 arrays, as test_optim_host.make_tensors) on the device, each array inside its
    own sentinel-filled buffer at element offset PAD + off[key]."""

    def __init__(self, tensors, offsets):
        self.n = [t["p"].size for t in tensors]
        self.bufs, self.views = [], []
        for t, off in zip(tensors, offsets):
            bufs, views = {}, {}
            for k in KEYS:
                buf = torch.full((t[k].size + 2 * PAD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
                assert buf.data_ptr() % 16 == 0
                view = buf[PAD + off[k]: PAD + off[k] + t[k].size]
                view.copy_(torch.from_numpy(t[k]))
                bufs[k], views[k] = buf, view
            self.bufs.append(bufs)
            self.views.append(views)
        self.offsets = offsets
        self.step_in = torch.tensor([float(t["step"][0]) for t in tensors], dtype=torch.float32, device=DEV)
        self.step_out = torch.full((len(tensors),), -7.0, dtype=torch.float32, device=DEV)

    def launch(self, hyper, grad_scale=None, found_inf=None):
        recs = [(v["p"].data_ptr(), v["g"].data_ptr(), v["m"].data_ptr(), v["v"].data_ptr(),
                 self.step_in.data_ptr() + 4 * i, self.step_out.data_ptr() + 4 * i, n)
                for i, (v, n) in enumerate(zip(self.views, self.n))]
        table, chunks = bev_native.adam_table(recs)
        table_dev = torch.from_numpy(table.reshape(-1)).to(DEV)
        gs = None if grad_scale is None else torch.tensor([grad_scale], dtype=torch.float32, device=DEV)
        fi = None if found_inf is None else torch.tensor([found_inf], dtype=torch.float32, device=DEV)
        bev_native.adam_step(table_dev, len(recs), chunks, *hyper, grad_scale=gs, found_inf=fi)
        torch.cuda.synchronize()

    def check(self, want):
        """want: the host tensors after the same update."""
        steps = self.step_out.cpu().numpy()
        for i, (bufs, views, t, off) in enumerate(zip(self.bufs, self.views, want, self.offsets)):
            for k in KEYS:
                same_bits(views[k].cpu().numpy(), t[k], f"tensor {i} (n = {self.n[i]}) {k}")
                whole = bufs[k].cpu().numpy()
                lo = PAD + off[k]
                outside = np.concatenate([whole[:lo], whole[lo + self.n[i]:]])
                assert (outside.view(np.uint32) == np.array(SENTINEL, F).view(np.uint32)).all(), \
                    f"tensor {i} (n = {self.n[i]}) {k}: a write outside the tensor"
            same_bits(steps[i:i + 1], t["step"], f"tensor {i} step")


def run_case(tensors, offsets, hyper, grad_scale=None, found_inf=None):
    dev = Carved(tensors, offsets)
    dev.launch(hyper, grad_scale, found_inf)
    host_step(tensors, hyper, grad_scale=grad_scale, found_inf=found_inf)
    dev.check(tensors)


ALIGNMENTS = {
    "aligned": lambda i: dict(p=0, g=0, m=0, v=0),
    "g_misaligned": lambda i: dict(p=0, g=1 + i % 3, m=0, v=0),  # a view into a flat gradient bucket
    "all_misaligned": lambda i: dict(p=1 + i % 3, g=1 + (i + 1) % 3, m=1 + (i + 2) % 3, v=1 + i % 3),
}


def boundary_sizes():
    C = chunk()
    return [1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3]


@pytest.mark.parametrize("alignment", sorted(ALIGNMENTS))
def test_sizes_around_group_and_chunk(alignment):
    sizes = boundary_sizes()
    tensors = make_tensors(np.random.default_rng(21), sizes, 5)
    offsets = [ALIGNMENTS[alignment](i) for i in range(len(sizes))]
    run_case(tensors, offsets, (1e-3, 0.9, 0.999, 1e-8, 1e-2, True))


def test_mixed_alignment_in_one_launch():
    sizes = boundary_sizes()
    tensors = make_tensors(np.random.default_rng(22), sizes, 0)
    kinds = sorted(ALIGNMENTS)
    offsets = [ALIGNMENTS[kinds[i % 3]](i) for i in range(len(sizes))]
    run_case(tensors, offsets, (1e-3, 0.9, 0.999, 1e-8, 1e-4, False))


@pytest.mark.parametrize("beta1", (0.9, 0.3))
@pytest.mark.parametrize("decay", sorted(DECAYS))
@pytest.mark.parametrize("step", STEPS)
def test_step_inputs(step, decay, beta1):
    """The host test's value cases: update numbers 1 .. 2^20, both decays and none, both lerp branches, gradients
    from 1e-6 to 1e2, with non-finite and extreme gradients in the last two tensors."""
    wd, decoupled = DECAYS[decay]
    rng = np.random.default_rng(step % 1000 + 17)
    tensors = make_tensors(rng, [257] * len(GRAD_SCALES) + [64, 9], step, scales=GRAD_SCALES + [1.0, 1.0])
    poke_nonfinite(tensors[-2:])
    offsets = [ALIGNMENTS["aligned" if i % 2 == 0 else "all_misaligned"](i) for i in range(len(tensors))]
    run_case(tensors, offsets, (1e-3, beta1, 0.999, 1e-8, wd, decoupled))


@pytest.mark.parametrize("alignment", ("aligned", "all_misaligned"))
def test_scaler_scalars_on_the_device(alignment):
    sizes = [5, 300, chunk() + 1]
    offsets = [ALIGNMENTS[alignment](i) for i in range(len(sizes))]
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-4, False)
    # found_inf set: nothing moves, the counters stay
    tensors = make_tensors(np.random.default_rng(23), sizes, 4)
    before = [{k: a.copy() for k, a in t.items()} for t in tensors]
    dev = Carved(tensors, offsets)
    dev.launch(hyper, grad_scale=1024.0, found_inf=1.0)
    dev.check(before)
    # found_inf clear, a scale that is no power of two
    run_case(make_tensors(np.random.default_rng(24), sizes, 4), offsets, hyper, grad_scale=12345.678, found_inf=0.0)
    # a power of two on scaled gradients: the unscaled call's bits
    a = make_tensors(np.random.default_rng(25), sizes, 4)
    b = [{k: x.copy() for k, x in t.items()} for t in a]
    for t in b:
        t["g"] *= F(65536.0)
    host_step(a, hyper)
    dev = Carved(b, offsets)
    dev.launch(hyper, grad_scale=65536.0)
    for t, want in zip(b, a):
        want["g"] = t["g"]
    dev.check(a)


# ---------------------------------------------------------------------------
# bev_optim.Adam on device parameters
# ---------------------------------------------------------------------------
def dev_params(rng, shapes):
    return [torch.nn.Parameter(torch.from_numpy(np.asarray(rng.standard_normal(s), dtype=F)).to(DEV)) for s in shapes]


def snapshot(opt, params):
    def num(t):
        return t.detach().cpu().numpy().copy()
    return [{"p": num(p), "g": None if p.grad is None else num(p.grad),
             "m": num(opt.state[p]["exp_avg"]) if p in opt.state else np.zeros(tuple(p.shape), F),
             "v": num(opt.state[p]["exp_avg_sq"]) if p in opt.state else np.zeros(tuple(p.shape), F),
             "step": float(opt.state[p]["step"]) if p in opt.state else 0.0} for p in params]


def check_update(opt, params, before, hyper, grad_scale=None):
    for i, (p, b) in enumerate(zip(params, before)):
        if b["g"] is None:
            assert np.array_equal(p.detach().cpu().numpy().view(np.uint32), b["p"].view(np.uint32))
            continue
        rp, rm, rv, rs = restate(b["p"], b["g"], b["m"], b["v"], b["step"], *hyper, grad_scale=grad_scale)
        same_bits(p.detach().cpu().numpy(), rp, f"param {i}")
        same_bits(opt.state[p]["exp_avg"].cpu().numpy(), rm, f"param {i} exp_avg")
        same_bits(opt.state[p]["exp_avg_sq"].cpu().numpy(), rv, f"param {i} exp_avg_sq")
        st = opt.state[p]["step"]
        assert st.dtype == torch.float32 and st.dim() == 0 and st.device == p.device and float(st) == float(rs)


def test_300_tensors_some_without_gradient():
    rng = np.random.default_rng(31)
    C = chunk()
    sizes = [int(s) for s in rng.integers(1, 700, 300)]
    sizes[7], sizes[123], sizes[299] = C + 5, 3 * C, C
    params = dev_params(rng, [(s,) for s in sizes])
    opt = bev_optim.Adam(params, lr=1e-3, weight_decay=1e-4)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-4, False)
    for it in range(3):
        for i, p in enumerate(params):
            p.grad = None if (i + it) % 5 == 0 else torch.from_numpy(rng.standard_normal(sizes[i]).astype(F)).to(DEV)
        before = snapshot(opt, params)
        opt.step()
        check_update(opt, params, before, hyper)
    assert len(opt._tables) == 1  # one launch per step: one group, one device


def test_two_param_groups_and_layouts():
    rng = np.random.default_rng(32)
    a, b, c = dev_params(rng, [(40,), (9, 2), (2, 3, 4, 5)])
    c.data = c.data.contiguous(memory_format=torch.channels_last)
    opt = bev_optim.AdamW([{"params": [a], "lr": 1e-2}, {"params": [b, c], "weight_decay": 0.1, "betas": (0.3, 0.99)}],
                          lr=1e-3)
    for _ in range(2):
        for p in (a, b, c):
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(F)).to(DEV)  # c's: another layout
        before = snapshot(opt, [a, b, c])
        opt.step()
        check_update(opt, [a], before[:1], (1e-2, 0.9, 0.999, 1e-8, 1e-2, True))
        check_update(opt, [b, c], before[1:], (1e-3, 0.3, 0.99, 1e-8, 0.1, True))
    assert opt.state[c]["exp_avg"].stride() == c.stride()


def test_state_dict_from_torch_on_the_device():
    rng = np.random.default_rng(33)
    shapes = [(17,), (4, 6)]
    tp = dev_params(rng, shapes)
    topt = torch.optim.Adam(tp, lr=1e-3, weight_decay=1e-4)
    for _ in range(2):
        for p in tp:
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(F)).to(DEV)
        topt.step()
    ps = [torch.nn.Parameter(p.detach().clone()) for p in tp]
    opt = bev_optim.Adam(ps, lr=1e-3, weight_decay=1e-4)
    opt.load_state_dict(topt.state_dict())  # torch keeps `step` on the host: it moves to the device at the first step
    for p in ps:
        p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(F)).to(DEV)
    before = snapshot(opt, ps)
    assert all(b["step"] == 2.0 for b in before)
    opt.step()
    check_update(opt, ps, before, (1e-3, 0.9, 0.999, 1e-8, 1e-4, False))


def test_scaler_step_does_not_wait():
    """GradScaler.step + update with bev_optim.Adam: no synchronising call, on the first step (state and table are
    created) and on a later one (cached table), with and without an overflow."""
    rng = np.random.default_rng(34)
    params = dev_params(rng, [(1000,), (33, 3), (5,)])
    ws = [torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(F)).to(DEV) for p in params]
    bad = [w.clone() for w in ws]
    bad[1][2, 1] = float("inf")
    opt = bev_optim.Adam(params, lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, False)
    for it, weights in enumerate((ws, ws, bad, ws)):
        opt.zero_grad(set_to_none=True)
        scaler.scale(sum((p * w).sum() for p, w in zip(params, weights))).backward()
        before = snapshot(opt, params)
        scale = scaler.get_scale()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt)
            scaler.update()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        if weights is bad:
            after = snapshot(opt, params)
            for b, a in zip(before, after):
                assert all(np.array_equal(np.asarray(a[k], F).view(np.uint32), np.asarray(b[k], F).view(np.uint32))
                           for k in ("p", "m", "v", "step"))
            assert scaler.get_scale() == scale / 2
        else:
            check_update(opt, params, before, hyper, grad_scale=scale)
            assert scaler.get_scale() == scale


# ---------------------------------------------------------------------------
# a model's training step: accumulation, GradScaler, an overflow
# ---------------------------------------------------------------------------
def tiny_bevnet():
    import bev_rig
    from models.model_wrapper import BEVNet
    cfg = {"MODEL": {"BACKBONE": "resnet18", "PRETRAINED": False, "FEAT_DIM": 8, "OUT_INDEX": 2,
                     "BEV_SIZE": [8, 8, 16], "BEV_BOUNDS": [-24.0, 24.0, -7.2, 7.2], "BEV_PROJ_CH": 0,
                     "BACKBONE_IMPL": "fallback"},
           "LOSS": {"MAX_OBJECTS": 4}, "EVAL": {}}
    V, H, W = 2, 32, 64
    torch.manual_seed(0)
    net = BEVNet(cfg).to(DEV)
    K, Rt = bev_rig.rig(V, H, W, 1)
    gen = torch.Generator().manual_seed(1)
    batch = {"images": torch.randn(1, V, 3, H, W, generator=gen).to(DEV),
             "calib": {"intrinsic": torch.from_numpy(K).to(DEV), "extrinsic": torch.from_numpy(Rt).to(DEV)}}
    targets = [{"boxes_world": torch.tensor([[1.0, 0.5, 0.6, 0.6], [-3.0, 2.0, 0.6, 0.6]])}]
    with torch.no_grad():
        net.eval()(batch)  # the lazily built modules
    net.train()
    return net, batch, targets, cfg["LOSS"]


def test_model_step_with_accumulation_and_overflow():
    import bev_dist
    net, batch, targets, loss_cfg = tiny_bevnet()
    idle = torch.nn.Parameter(torch.ones(5, device=DEV))  # never gets a gradient: the trunk stages past out_index
    params = list(net.parameters()) + [idle]
    opt = bev_optim.Adam(params, lr=1e-3, weight_decay=1e-4)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-4, False)
    seen = []

    def before_update(optimizer, args, kwargs):
        seen.append((snapshot(opt, params), float(opt.grad_scale), float(opt.found_inf)))

    opt.register_step_pre_hook(before_update)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    updates = 0
    for micro in range(4):  # two accumulation cycles: updates after micro-steps 1 and 3
        if micro % 2 == 1:
            grads_before = [None if p.grad is None else p.grad.clone() for p in params]
        bev_dist.train_step(net, batch, targets, opt, loss_cfg, scaler, accum_steps=2, micro_step=micro)
        if micro % 2 == 0:
            assert len(seen) == updates, "the optimizer stepped inside an accumulation cycle"
            if micro == 0:
                assert len(opt.state) == 0
            continue
        updates += 1
        assert len(seen) == updates
        before, scale, found = seen[-1]
        assert found == 0.0 and scale == 2.0 ** 10
        # the second micro-step added to the first one's gradients
        grown = [b["g"] is not None and g0 is not None and not np.array_equal(b["g"], g0.cpu().numpy())
                 for b, g0 in zip(before, grads_before)]
        assert any(grown)
        assert sum(b["g"] is not None for b in before) >= 10
        check_update(opt, params, before, hyper, grad_scale=scale)
        assert all(float(opt.state[p]["step"]) == updates for p in params if p.grad is not None)
        assert idle not in opt.state and idle.grad is None
    # a cycle whose scaled gradients overflow: nothing moves, the scale is halved
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 60)
    for micro in (4, 5):
        bev_dist.train_step(net, batch, targets, opt, loss_cfg, scaler, accum_steps=2, micro_step=micro)
    assert len(seen) == 3
    before, scale, found = seen[-1]
    assert found != 0.0 and scale == 2.0 ** 60
    after = snapshot(opt, params)
    for i, (b, a) in enumerate(zip(before, after)):
        for k in ("p", "m", "v"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (i, k)
        assert a["step"] == b["step"]
    assert scaler.get_scale() == 2.0 ** 59
    assert idle not in opt.state
