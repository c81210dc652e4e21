"""The packed-weight caches' contract, host side (no GPU): every cache of operands derived from a parameter is keyed
on (t.data_ptr(), t._version), so a writer that goes through raw pointers has to advance the version counter itself
(bev_native.mark_written).

  * bev_optim.Adam / AdamW on CPU parameters (bev_adam_step_host) advance the counter of the parameter, exp_avg and
    exp_avg_sq at every step, so a key taken before the step differs after it;
  * the site table of tests/test_weight_cache_gpu.py names every `._version` read of the package, by file: a new
    cache cannot appear without a coherence case there."""
import os
import re

import numpy as np
import pytest
import torch

import bev_native
import bev_optim
from conftest import PKG
from test_optim_host import cpu_params, lib, set_grads  # noqa: F401  (lib: the fixture that builds the library)


def key(t):
    return (t.data_ptr(), t._version)


@pytest.mark.parametrize("cls_name", ["Adam", "AdamW"])
def test_cpu_step_advances_version_counters(lib, cls_name):  # noqa: F811
    rng = np.random.default_rng(41)
    params = cpu_params(rng, [(3, 5), (7,), (2, 3, 4, 5), ()])
    idle = torch.nn.Parameter(torch.ones(4))  # never gets a gradient: not written, not marked
    opt = getattr(bev_optim, cls_name)(params + [idle], lr=1e-2)
    for it in range(3):
        set_grads(params, rng)
        values = [p.detach().clone() for p in params]
        keys = [key(p) for p in params]
        state_keys = [(key(opt.state[p]["exp_avg"]), key(opt.state[p]["exp_avg_sq"])) if p in opt.state else None
                      for p in params]
        opt.step()
        for p, v0, k0, sk0 in zip(params, values, keys, state_keys):
            assert not torch.equal(p.detach(), v0)  # the values moved ...
            assert p.data_ptr() == k0[0] and p._version > k0[1]  # ... in place, and the counter says so
            assert key(p) != k0
            st = opt.state[p]
            if sk0 is not None:
                assert st["exp_avg"]._version > sk0[0][1] and st["exp_avg_sq"]._version > sk0[1][1]
                assert key(st["exp_avg"]) != sk0[0] and key(st["exp_avg_sq"]) != sk0[1]
            else:  # created by this step and written by it
                assert st["exp_avg"]._version > 0 and st["exp_avg_sq"]._version > 0
        assert idle._version == 0 and idle not in opt.state
    assert all(p._version >= 3 for p in params)  # one advance per step, as torch.optim.Adam's in-place ops give


def test_cpu_step_under_found_inf_is_marked_too(lib):  # noqa: F811
    """found_inf lives with the scaler and is not read by step(): a skipped step is marked as written (one needless
    re-pack), and nothing moved."""
    rng = np.random.default_rng(42)
    params = cpu_params(rng, [(9,)])
    opt = bev_optim.Adam(params, lr=1e-2)
    set_grads(params, rng)
    opt.step()
    before = params[0].detach().clone()
    v0 = params[0]._version
    opt.grad_scale, opt.found_inf = torch.tensor(1024.0), torch.tensor(1.0)
    try:
        opt.step()
    finally:
        del opt.grad_scale, opt.found_inf
    assert torch.equal(params[0].detach(), before) and params[0]._version > v0


def test_mark_written_skips_none_and_takes_leaves():
    p, b = torch.nn.Parameter(torch.zeros(3)), torch.zeros(2)
    bev_native.mark_written(p, None, b)
    assert (p._version, b._version) == (1, 1)
    with torch.no_grad():
        bev_native.mark_written(p)
    assert p._version == 2
    bev_native.mark_written()
    bev_native.mark_written(None, None)


def _version_reads():
    """`._version` occurrences by file, under models/ and in bev_*.py of the package."""
    files = [os.path.join(PKG, f) for f in sorted(os.listdir(PKG)) if re.fullmatch(r"bev_\w+\.py", f)]
    for root, _, names in os.walk(os.path.join(PKG, "models")):
        files += [os.path.join(root, n) for n in sorted(names) if n.endswith(".py")]
    counts = {}
    for path in files:
        with open(path) as fh:
            n = len(re.findall(r"\._version\b", fh.read()))
        if n:
            counts[os.path.relpath(path, PKG).replace(os.sep, "/")] = n
    return counts


def test_site_table_names_every_version_key_in_the_code():
    from test_weight_cache_gpu import VERSION_KEY_SITES
    counts = _version_reads()
    assert counts == {f: n for f, (n, _) in VERSION_KEY_SITES.items()}, (
        "a cache keyed on a version counter was added, moved or removed: give it a coherence case in "
        "tests/test_weight_cache_gpu.py and update VERSION_KEY_SITES")
    assert counts == {"models/encoders/resnet.py": 2, "models/encoders/efficientnet.py": 4,
                      "models/encoders/cnn_encoder.py": 2, "models/heads/detector.py": 2,
                      "models/model_wrapper.py": 1}
