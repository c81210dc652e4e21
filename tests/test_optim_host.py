"""Adam / AdamW update, host side (no GPU): bev_adam_step_host (the per-element function of csrc/bev_optim.h compiled
for the CPU) and bev_optim.Adam / AdamW on CPU parameters, against

  * `restate`, a numpy float32 restatement of the defined sequence in this file's own words, bit for bit (NaN results
    compared by position: which NaN an operation returns is not part of the definition);
  * float64 torch.optim.Adam, by the error of torch's own fp32 single-tensor Adam on the same gradients;

and the state-dict exchange with torch.optim.Adam, a scheduler, torch.amp.GradScaler("cpu"), the C entries' argument
rules and the constructor's refusals."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import bev_native
import bev_optim

F = np.float32
NAN, INF = float("nan"), float("inf")
DECAYS = {"none": (0.0, False), "coupled": (1e-4, False), "decoupled": (1e-2, True)}
STEPS = (0, 1, 2, 9, 999, 2 ** 20 - 1)  # the update numbers 1, 2, 3, 10, 1000, 2^20, set through the state


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(bev_native.LIB_PATH):
        bev_native.build()
    return bev_native.lib()


def ipow(b: float, t: int) -> float:
    """b^t in double by square-and-multiply, lowest bit of t first."""
    r, x = 1.0, b
    while t:
        if t & 1:
            r = r * x
        t >>= 1
        if t:
            x = x * x
    return r


def restate(p, g, m, v, step, lr, beta1, beta2, eps, wd, decoupled, grad_scale=None):
    """The defined update on float32 numpy arrays: -> (p, m, v, step) after it.  Every line is one rounding."""
    p, g, m, v = (np.array(a, dtype=F) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if grad_scale is not None:
            g = g * F(1.0 / float(F(grad_scale)))
        if wd != 0:
            if decoupled:
                p = p * F(1.0 - lr * wd)
            else:
                d = p * F(wd)
                g = g + d
        w1 = F(1.0 - beta1)
        diff = g - m
        if w1 < F(0.5):
            t_ = w1 * diff
            m = m + t_
        else:
            t_ = diff * (F(1.0) - w1)
            m = g - t_
        a = v * F(beta2)
        b = F(1.0 - beta2) * g
        b = b * g
        v = a + b
        t = int(step) + 1
        bc1 = 1.0 - ipow(beta1, t)
        bc2 = 1.0 - ipow(beta2, t)
        ss, bs = F(lr / bc1), F(math.sqrt(bc2))
        den = np.sqrt(v)
        den = den / bs
        den = den + F(eps)
        q = m / den
        u = ss * q
        p = p - u
    for arr in (p, m, v):
        assert arr.dtype == F
    return p, m, v, F(F(step) + F(1.0))


def same_bits(got, want, what=""):
    """Equal bit for bit, except that a NaN matches any NaN."""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs at other places"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.flatnonzero(bad)[:4]}: " \
                          f"{got.ravel()[np.flatnonzero(bad)[:4]]} vs {want.ravel()[np.flatnonzero(bad)[:4]]}"


def host_step(tensors, hyper, grad_scale=None, found_inf=None):
    """bev_adam_step_host on a list of dicts of float32 arrays (p, g, m, v, step [1]); p, m, v, step updated in
    place as the optimizer would (step through a second buffer)."""
    outs = [np.full(1, -7.0, F) for _ in tensors]
    recs = [(t["p"].ctypes.data, t["g"].ctypes.data, t["m"].ctypes.data, t["v"].ctypes.data, t["step"].ctypes.data,
             o.ctypes.data, t["p"].size) for t, o in zip(tensors, outs)]
    table, _ = bev_native.adam_table(recs)
    bev_native.adam_step_host(table, len(recs), *hyper, grad_scale=grad_scale, found_inf=found_inf)
    for t, o in zip(tensors, outs):
        t["step"][:] = o


def make_tensors(rng, sizes, step, scales=None):
    ts = []
    for i, n in enumerate(sizes):
        sc = 1.0 if scales is None else scales[i]
        ts.append({"p": rng.standard_normal(n).astype(F), "g": (rng.standard_normal(n) * sc).astype(F),
                   "m": (rng.standard_normal(n) * 0.1 * sc).astype(F),
                   "v": (rng.random(n) * 0.01 * sc * sc).astype(F), "step": np.full(1, step, F)})
    return ts


def check_against_restatement(step_fn, rng, sizes, step, hyper, scales=None, grad_scale=None, poke=None):
    ts = make_tensors(rng, sizes, step, scales)
    if poke is not None:
        poke(ts)
    before = [{k: a.copy() for k, a in t.items()} for t in ts]
    step_fn(ts, hyper, grad_scale=grad_scale)
    for i, (t, b) in enumerate(zip(ts, before)):
        p, m, v, s = restate(b["p"], b["g"], b["m"], b["v"], b["step"][0], *hyper, grad_scale=grad_scale)
        same_bits(t["p"], p, f"tensor {i} p")
        same_bits(t["m"], m, f"tensor {i} exp_avg")
        same_bits(t["v"], v, f"tensor {i} exp_avg_sq")
        same_bits(t["step"], [s], f"tensor {i} step")
        assert np.array_equal(t["g"].view(np.uint32), b["g"].view(np.uint32)), "the gradient was modified"


# one tensor per gradient scale 10^k, k = -6 .. 2
GRAD_SCALES = [10.0 ** k for k in range(-6, 3)]


@pytest.mark.parametrize("beta1", (0.9, 0.3))
@pytest.mark.parametrize("decay", sorted(DECAYS))
@pytest.mark.parametrize("step", STEPS)
def test_host_entry_equals_restatement(lib, step, decay, beta1):
    wd, decoupled = DECAYS[decay]
    hyper = (1e-3, beta1, 0.999, 1e-8, wd, decoupled)
    rng = np.random.default_rng(step % 1000 + 17)
    check_against_restatement(host_step, rng, [257] * len(GRAD_SCALES), step, hyper, scales=GRAD_SCALES)


def poke_nonfinite(ts):
    for t in ts:
        n = t["g"].size
        for i, val in zip(range(0, n, max(1, n // 7)), (NAN, INF, -INF, 3.0e38, -3.0e38, 1e-45, 0.0)):
            t["g"][i] = val


@pytest.mark.parametrize("beta1", (0.9, 0.3))
@pytest.mark.parametrize("decay", sorted(DECAYS))
def test_host_entry_nonfinite_gradients(lib, decay, beta1):
    wd, decoupled = DECAYS[decay]
    hyper = (1e-3, beta1, 0.999, 1e-8, wd, decoupled)
    check_against_restatement(host_step, np.random.default_rng(5), [64, 9], 3, hyper, poke=poke_nonfinite)


def test_host_entry_found_inf_leaves_everything(lib):
    ts = make_tensors(np.random.default_rng(6), [33, 1], 4)
    before = [{k: a.copy() for k, a in t.items()} for t in ts]
    host_step(ts, (1e-3, 0.9, 0.999, 1e-8, 1e-2, True), grad_scale=1024.0, found_inf=1.0)
    for t, b in zip(ts, before):
        for k in t:
            assert np.array_equal(t[k].view(np.uint32), b[k].view(np.uint32)), k
    host_step(ts, (1e-3, 0.9, 0.999, 1e-8, 1e-2, True), grad_scale=1024.0, found_inf=0.0)
    assert all(t["step"][0] == 5.0 and not np.array_equal(t["p"], b["p"]) for t, b in zip(ts, before))


@pytest.mark.parametrize("decay", sorted(DECAYS))
def test_host_entry_grad_scale_power_of_two(lib, decay):
    wd, decoupled = DECAYS[decay]
    hyper = (1e-3, 0.9, 0.999, 1e-8, wd, decoupled)
    a = make_tensors(np.random.default_rng(8), [100, 7], 2)
    b = [{k: x.copy() for k, x in t.items()} for t in a]
    for t in b:
        t["g"] *= F(65536.0)  # exact
    host_step(a, hyper)
    host_step(b, hyper, grad_scale=65536.0)
    for ta, tb in zip(a, b):
        for k in ("p", "m", "v", "step"):
            assert np.array_equal(ta[k].view(np.uint32), tb[k].view(np.uint32)), k
    # and a scale that is no power of two follows the restatement's inv = float(1 / double(scale))
    check_against_restatement(host_step, np.random.default_rng(9), [50], 2, hyper, grad_scale=12345.678)


# ---------------------------------------------------------------------------
# accuracy: error against float64 Adam, measured by torch's own fp32 error
# ---------------------------------------------------------------------------
ACCURACY = {"adam": (0.0, False), "adam_wd": (1e-4, False), "adamw": (1e-2, True)}


def run_optimizer(make, p0, grads, dtype):
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dtype))
    opt = make([p])
    for g in grads:
        p.grad = torch.from_numpy(g.copy()).to(dtype)
        opt.step()
    return p.detach().double().numpy(), opt, p


def accuracy_errors(seed, wd, decoupled, steps=50, n=20000):
    # the three seeds also walk the gradient scale over the range a scaled loss covers
    scale = (1e-4, 1.0, 1e2)[seed]
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(F)
    grads = [(rng.standard_normal(n) * scale).astype(F) for _ in range(steps)]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ref, _, _ = run_optimizer(lambda ps: torch.optim.Adam(ps, foreach=False, decoupled_weight_decay=decoupled, **kw),
                              p0, grads, torch.float64)
    tor, _, _ = run_optimizer(lambda ps: torch.optim.Adam(ps, foreach=False, decoupled_weight_decay=decoupled, **kw),
                              p0, grads, torch.float32)
    cls = bev_optim.AdamW if decoupled else bev_optim.Adam
    ours, _, _ = run_optimizer(lambda ps: cls(ps, **kw), p0, grads, torch.float32)
    return np.abs(ours - ref).max(), np.abs(tor - ref).max()


@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("config", sorted(ACCURACY))
def test_accuracy_against_float64_adam(lib, config, seed):
    ours, tor = accuracy_errors(seed, *ACCURACY[config])
    print(f"{config} seed {seed}: max |p - f64| ours {ours:.3e} torch fp32 {tor:.3e} ratio {ours / tor:.3f}")
    assert ours <= 1.5 * tor


# ---------------------------------------------------------------------------
# bev_optim.Adam on CPU parameters
# ---------------------------------------------------------------------------
def cpu_params(rng, shapes):
    return [torch.nn.Parameter(torch.from_numpy(np.asarray(rng.standard_normal(s), dtype=F))) for s in shapes]


def set_grads(params, rng, scale=1.0):
    for p in params:
        p.grad = torch.from_numpy(np.asarray(rng.standard_normal(tuple(p.shape)) * scale, dtype=F))


def snapshot(opt, params):
    return [{"p": p.detach().numpy().copy(), "g": None if p.grad is None else p.grad.numpy().copy(),
             "m": opt.state[p]["exp_avg"].numpy().copy() if p in opt.state else np.zeros(tuple(p.shape), F),
             "v": opt.state[p]["exp_avg_sq"].numpy().copy() if p in opt.state else np.zeros(tuple(p.shape), F),
             "step": float(opt.state[p]["step"]) if p in opt.state else 0.0} for p in params]


def check_step_equals_restatement(opt, params, before, hyper, grad_scale=None):
    for i, (p, b) in enumerate(zip(params, before)):
        if b["g"] is None:
            assert np.array_equal(p.detach().numpy(), b["p"])
            continue
        rp, rm, rv, rs = restate(b["p"], b["g"], b["m"], b["v"], b["step"], *hyper, grad_scale=grad_scale)
        same_bits(p.detach().numpy(), rp, f"param {i}")
        same_bits(opt.state[p]["exp_avg"].numpy(), rm, f"param {i} exp_avg")
        same_bits(opt.state[p]["exp_avg_sq"].numpy(), rv, f"param {i} exp_avg_sq")
        assert float(opt.state[p]["step"]) == float(rs)


def test_optimizer_cpu_steps_and_state_layout(lib):
    rng = np.random.default_rng(11)
    params = cpu_params(rng, [(3, 5), (7,), (2, 3, 4, 5), ()])
    params[2].data = params[2].data.contiguous(memory_format=torch.channels_last)
    opt = bev_optim.Adam(params, lr=2e-3, weight_decay=1e-4)
    hyper = (2e-3, 0.9, 0.999, 1e-8, 1e-4, False)
    for it in range(3):
        set_grads(params, rng)
        if it == 1:
            params[1].grad = None  # skipped: no state change, no step
        before = snapshot(opt, params)
        opt.step()
        check_step_equals_restatement(opt, params, before, hyper)
    st = opt.state[params[2]]
    assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].device == params[2].device
    assert st["exp_avg"].stride() == params[2].stride() and st["exp_avg_sq"].stride() == params[2].stride()
    assert float(opt.state[params[1]]["step"]) == 2.0 and float(st["step"]) == 3.0
    assert set(opt.param_groups[0]) == set(torch.optim.Adam([torch.zeros(1)]).param_groups[0])


def test_optimizer_gradient_in_another_layout(lib):
    rng = np.random.default_rng(12)
    (p,) = cpu_params(rng, [(2, 3, 4, 5)])
    opt = bev_optim.AdamW([p], lr=1e-3)
    g = torch.from_numpy(rng.standard_normal((2, 3, 4, 5)).astype(F)).contiguous(memory_format=torch.channels_last)
    p.grad = g
    before = snapshot(opt, [p])
    opt.step()
    check_step_equals_restatement(opt, [p], before, (1e-3, 0.9, 0.999, 1e-8, 1e-2, True))
    assert p.grad is g  # the copy in p's layout is the kernel's operand only


def test_two_param_groups(lib):
    rng = np.random.default_rng(13)
    a, b = cpu_params(rng, [(40,), (9, 2)])
    opt = bev_optim.Adam([{"params": [a], "lr": 1e-2}, {"params": [b], "weight_decay": 0.1, "betas": (0.3, 0.99)}],
                         lr=1e-3)
    for _ in range(2):
        set_grads([a, b], rng)
        before = snapshot(opt, [a, b])
        opt.step()
        check_step_equals_restatement(opt, [a], before[:1], (1e-2, 0.9, 0.999, 1e-8, 0.0, False))
        check_step_equals_restatement(opt, [b], before[1:], (1e-3, 0.3, 0.99, 1e-8, 0.1, False))


def test_state_dict_from_torch_and_back(lib):
    rng = np.random.default_rng(14)
    shapes = [(17,), (4, 6)]
    init = [rng.standard_normal(s).astype(F) for s in shapes]
    grads = [[rng.standard_normal(s).astype(F) for s in shapes] for _ in range(5)]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-4, False)

    def fresh(cls, **extra):
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
        return ps, cls(ps, **kw, **extra)

    def feed(ps, opt, gs):
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()

    tp, topt = fresh(torch.optim.Adam, foreach=False)
    for gs in grads[:3]:
        feed(tp, topt, gs)
    # torch -> ours: one more step of ours is the restatement on torch's state
    ps, opt = fresh(bev_optim.Adam)
    for p, q in zip(ps, tp):
        p.data.copy_(q.data)
    opt.load_state_dict(topt.state_dict())
    assert all(float(opt.state[p]["step"]) == 3.0 for p in ps)
    for p, g in zip(ps, grads[3]):
        p.grad = torch.from_numpy(g.copy())
    before = snapshot(opt, ps)
    for b, q in zip(before, tp):
        assert np.array_equal(b["m"], topt.state[q]["exp_avg"].numpy())
    opt.step()
    check_step_equals_restatement(opt, ps, before, hyper)
    assert all(float(opt.state[p]["step"]) == 4.0 for p in ps)
    # ours -> torch: torch steps on, and ends where a float64 run of all five steps ends, within the accuracy bar
    tp2, topt2 = fresh(torch.optim.Adam, foreach=False)
    for p, q in zip(tp2, ps):
        p.data.copy_(q.data)
    topt2.load_state_dict(opt.state_dict())
    feed(tp2, topt2, grads[4])
    assert all(float(topt2.state[p]["step"]) == 5.0 for p in tp2)
    feed(tp, topt, grads[3])
    feed(tp, topt, grads[4])  # torch alone, fp32
    dp = [torch.nn.Parameter(torch.from_numpy(a.copy()).double()) for a in init]
    dopt = torch.optim.Adam(dp, foreach=False, **kw)
    for gs in grads:
        for p, g in zip(dp, gs):
            p.grad = torch.from_numpy(g.copy()).double()
        dopt.step()
    for p_mixed, p_torch, p_ref in zip(tp2, tp, dp):
        e_mixed = (p_mixed.detach().double() - p_ref.detach()).abs().max().item()
        e_torch = (p_torch.detach().double() - p_ref.detach()).abs().max().item()
        assert e_mixed <= 1.5 * e_torch, (e_mixed, e_torch)
    # the dict itself has torch's shape
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert set(sd["param_groups"][0]) == set(tsd["param_groups"][0])
    assert set(sd["state"][0]) == set(tsd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_scheduler_changes_the_lr_used(lib):
    rng = np.random.default_rng(15)
    (p,) = cpu_params(rng, [(31,)])
    opt = bev_optim.Adam([p], lr=1e-2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    for e in range(3):
        set_grads([p], rng)
        before = snapshot(opt, [p])
        opt.step()
        check_step_equals_restatement(opt, [p], before, (1e-2 * 0.5 ** e, 0.9, 0.999, 1e-8, 0.0, False))
        sched.step()
    assert opt.param_groups[0]["lr"] == 1e-2 * 0.125


def test_grad_scaler_cpu_skips_and_halves(lib):
    rng = np.random.default_rng(16)
    params = cpu_params(rng, [(21,), (5,)])
    opt = bev_optim.Adam(params, lr=1e-3)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, False)
    assert opt._step_supports_amp_scaling

    def scaled_step(poison):
        ws = [torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(F)) for p in params]
        if poison:
            ws[1][2] = INF
        opt.zero_grad(set_to_none=True)
        scaler.scale(sum((p * w).sum() for p, w in zip(params, ws))).backward()  # grad = scale * w
        before = snapshot(opt, params)
        scale = scaler.get_scale()
        scaler.step(opt)
        scaler.update()
        return before, scale

    before, scale = scaled_step(False)
    check_step_equals_restatement(opt, params, before, hyper, grad_scale=scale)
    assert scaler.get_scale() == 1024.0
    before, scale = scaled_step(True)  # the overflow: nothing moves, the scale halves
    for p, b in zip(params, before):
        assert np.array_equal(p.detach().numpy().view(np.uint32), b["p"].view(np.uint32))
        assert np.array_equal(opt.state[p]["exp_avg"].numpy().view(np.uint32), b["m"].view(np.uint32))
        assert np.array_equal(opt.state[p]["exp_avg_sq"].numpy().view(np.uint32), b["v"].view(np.uint32))
        assert float(opt.state[p]["step"]) == 1.0
    assert scaler.get_scale() == 512.0
    before, scale = scaled_step(False)
    assert scale == 512.0
    check_step_equals_restatement(opt, params, before, hyper, grad_scale=scale)
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params)
    assert not hasattr(opt, "found_inf")  # the scaler takes its tensors back


# ---------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------
def test_c_entries_argument_rules(lib):
    E = bev_native.BEV_ERR_ARGS
    assert lib.bev_adam_chunk_elems() > 0 and lib.bev_adam_chunk_elems() % 4 == 0
    assert lib.bev_adam_table_bytes(0) == 0 and lib.bev_adam_table_bytes(3) == 3 * 8 * 8
    table = np.zeros((1, 8), np.int64)
    tp = ctypes.c_void_p(table.ctypes.data)
    ok = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0)
    # the device entry refuses before any HIP call (no GPU here)
    assert lib.bev_adam_step_f32(None, 1, 1, *ok, None, None, None) == E
    assert lib.bev_adam_step_f32(tp, -1, 1, *ok, None, None, None) == E
    assert lib.bev_adam_step_f32(tp, 1, 0, *ok, None, None, None) == E  # fewer chunks than tensors
    assert lib.bev_adam_step_f32(tp, 1, 2 ** 31, *ok, None, None, None) == E
    assert lib.bev_adam_step_f32(ctypes.c_void_p(table.ctypes.data + 4), 1, 1, *ok, None, None, None) == E
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-9), (NAN, 0.9), (0.9, NAN)):
        assert lib.bev_adam_step_f32(tp, 1, 1, 1e-3, b1, b2, 1e-8, 0.0, 0, None, None, None) == E
        assert lib.bev_adam_step_host(tp, 1, 1e-3, b1, b2, 1e-8, 0.0, 0, None, None) == E
    assert lib.bev_adam_step_f32(None, 0, 0, *ok, None, None, None) == 0  # T == 0: a no-op
    assert lib.bev_adam_step_host(None, 0, *ok, None, None) == 0
    assert lib.bev_adam_step_host(None, 1, *ok, None, None) == E
    assert lib.bev_adam_step_host(tp, -1, *ok, None, None) == E
    assert lib.bev_adam_step_host(tp, 1, *ok, None, None) == E  # null step pointers
    step = np.zeros(2, F)
    table[0, 4], table[0, 5], table[0, 6] = step.ctypes.data, step.ctypes.data + 4, -1
    assert lib.bev_adam_step_host(tp, 1, *ok, None, None) == E  # n < 0
    table[0, 6] = 5
    assert lib.bev_adam_step_host(tp, 1, *ok, None, None) == E  # n > 0 with null tensors
    table[0, 6] = 0
    assert lib.bev_adam_step_host(tp, 1, *ok, None, None) == 0 and step[1] == 1.0  # an empty tensor counts its step
    with pytest.raises(bev_native.HipError):
        bev_native.adam_step(torch.zeros(8, dtype=torch.int64), 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, False)  # CPU table


def test_constructor_and_step_refusals(lib):
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)),
               dict(betas=(0.9, 1.0)), dict(weight_decay=-1.0), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            bev_optim.Adam([p], **kw)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(ValueError):
            bev_optim.Adam([torch.nn.Parameter(torch.zeros(4, dtype=dt))])
    opt = bev_optim.Adam([p])
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]})
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(ValueError):
        opt.step()
    p.grad = torch.zeros(4)
    opt.param_groups[0]["amsgrad"] = True  # e.g. through a loaded state dict
    with pytest.raises(ValueError):
        opt.step()
    opt.param_groups[0]["amsgrad"] = False
    opt.step()
    w = bev_optim.AdamW([p])
    assert w.param_groups[0]["weight_decay"] == 1e-2 and w.param_groups[0]["decoupled_weight_decay"] is True
    assert bev_optim.Adam([p]).param_groups[0]["decoupled_weight_decay"] is False
