"""Colour jitter for the device ingest, host side (no GPU): the per-pixel arithmetic of csrc/bev_image_jitter.h,
compiled for the CPU behind bev_image_jitter_u8_host, against Pillow (PIL.ImageEnhance and the RGB <-> HSV conversions
`data.transforms._adjust_hue` goes through); the records `ColorJitter.params_record` draws; the C entries' argument
rules and the Python surface.  Every comparison is uint8 equality: there are no tolerances.

One case cannot be written the way one would first write it: the hue shift byte 128 is not the byte of any factor
`_adjust_hue` accepts (uint8(f * 255) is 0..127 for 0 <= f <= 0.5 and 129..255 for -0.5 <= f < 0; -0.5 gives 129), so
`_hue_reference` takes `_adjust_hue`'s own steps with the byte given directly, and is itself held to `_adjust_hue` on
every byte a factor reaches.
"""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from conftest import PKG, REPO

ENTRIES = ("bev_image_resize_u8", "bev_image_jitter_workspace_bytes", "bev_image_jitter_normalize_u8_f32",
           "bev_image_jitter_u8_host")
B, C, S, H = 1, 2, 3, 4                                  # op codes of a record's word 0
HUE_FACTORS = {0: 0.0, 1: 1.5 / 255, 12: 12.5 / 255, 243: -13.5 / 255, 128: None}   # shift byte -> a factor giving it
FACTORS = (0.0, 0.5, 0.8, 1.0, 1.2, 2.0)                 # both blend branches, and the clip at 255


@pytest.fixture(scope="module")
def lib():
    import bev_native
    if not os.path.exists(bev_native.LIB_PATH):
        bev_native.build()
    return bev_native.lib()


def record(ops=(), fb=1.0, fc=1.0, fs=1.0, hue_byte=0):
    """One 8-word record (include/bev_mi355x.h) from an op list and the parameters."""
    rec = np.zeros(8, dtype=np.int32)
    rec[0] = sum(code << (4 * i) for i, code in enumerate(ops))
    rec[1:4] = np.array([fb, fc, fs], dtype=np.float32).view(np.int32)
    rec[4] = hue_byte
    return rec


def _hue_reference(img, byte):
    """`_adjust_hue` with the shift byte given directly: its steps, and its result wherever a factor gives the byte."""
    from data import transforms as T
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(byte)
    out = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    factor = HUE_FACTORS.get(byte)
    if factor is not None:
        assert int(T._hue_shift_byte(factor)) == byte
        assert np.array_equal(np.array(T._adjust_hue(img, factor)), np.array(out))
    return out


def pil_jitter(arr, ops, fb=1.0, fc=1.0, fs=1.0, hue_byte=0):
    """[H, W, 3] uint8 -> the frame after the ops in that order, through PIL.ImageEnhance and `_adjust_hue`'s steps."""
    img = Image.fromarray(arr)
    for code in ops:
        if code == B:
            img = ImageEnhance.Brightness(img).enhance(fb)
        elif code == C:
            img = ImageEnhance.Contrast(img).enhance(fc)
        elif code == S:
            img = ImageEnhance.Color(img).enhance(fs)
        elif code == H:
            img = _hue_reference(img, hue_byte)
    return np.array(img)


def all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def contents(rng, Hh, Ww):
    grey = rng.integers(0, 256, size=(Hh, Ww, 1), dtype=np.uint8)
    return {"random": rng.integers(0, 256, size=(Hh, Ww, 3), dtype=np.uint8),
            "0/255": (rng.integers(0, 2, size=(Hh, Ww, 3), dtype=np.uint8) * 255).astype(np.uint8),
            "grey": np.repeat(grey, 3, axis=2)}


def half_frames(k, Hh, Ww):
    """Grey frames (L == the grey level) whose mean L is exactly k + 0.5, and one pixel's worth below it."""
    flat = np.full(Hh * Ww, k, dtype=np.uint8)
    flat[1::2] = k + 1                                   # H * W is even: half the pixels each
    exact = np.repeat(flat.reshape(Hh, Ww, 1), 3, axis=2)
    below = exact.copy()
    below[Hh - 1, Ww - 1] = k                            # an odd index: was k + 1
    assert int(exact[..., 0].sum()) * 2 == (2 * k + 1) * Hh * Ww and int(below[..., 0].sum()) == int(exact[..., 0].sum()) - 1
    return {"exact": exact, "below": below}


ORDERS = list(itertools.permutations((B, C, S, H)))
ORDER_PARAMS = dict(fb=1.13, fc=0.87, fs=1.19, hue_byte=9)


def order_batch():
    """The 24 op orders with all four ops on one 37 x 53 random frame: frames [24, 37, 53, 3], records [24, 8] and the
    PIL results.  Contrast's mean differs with what precedes it, so this pins where in the list it is taken."""
    arr = np.random.default_rng(24).integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    frames = np.stack([arr] * len(ORDERS))
    recs = np.stack([record(o, **ORDER_PARAMS) for o in ORDERS])
    want = np.stack([pil_jitter(arr, o, **ORDER_PARAMS) for o in ORDERS])
    return frames, recs, want


@pytest.mark.parametrize("byte", [0, 1, 12, 128, 243])
def test_hue_over_all_colours(lib, byte):
    """All 2^24 colours through hue alone; shift byte 0 is the pure RGB -> HSV -> RGB round trip."""
    import bev_native as nat
    img = all_colours()
    got = nat.image_jitter_u8_host(img[None], record((H,), hue_byte=byte)[None])[0]
    want = np.array(_hue_reference(Image.fromarray(img), byte))
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (int(bad.sum()), img[bad][:4], got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("code", [B, C, S])
def test_blend_branches(lib, code):
    import bev_native as nat
    rng = np.random.default_rng(code)
    for name, arr in contents(rng, 37, 53).items():
        for f in FACTORS:
            got = nat.image_jitter_u8_host(arr[None], record((code,), fb=f, fc=f, fs=f)[None])[0]
            want = pil_jitter(arr, (code,), fb=f, fc=f, fs=f)
            assert np.array_equal(got, want), (code, name, f)


@pytest.mark.parametrize("k", [0, 127, 254])
def test_contrast_mean_rounds_half_up(lib, k):
    import bev_native as nat
    for name, arr in half_frames(k, 6, 8).items():
        for f in (0.5, 0.8, 1.2):
            got = nat.image_jitter_u8_host(arr[None], record((C,), fc=f)[None])[0]
            assert np.array_equal(got, pil_jitter(arr, (C,), fc=f)), (k, name, f)
    # the two frames round to different means, and that shows in the result
    a, b = (nat.image_jitter_u8_host(x[None], record((C,), fc=0.0)[None])[0] for x in half_frames(k, 6, 8).values())
    assert (a == k + 1).all() and (b == k).all()


def test_all_op_orders(lib):
    import bev_native as nat
    frames, recs, want = order_batch()
    got = nat.image_jitter_u8_host(frames, recs)
    for i, o in enumerate(ORDERS):
        assert np.array_equal(got[i], want[i]), o
    assert len({want[i].tobytes() for i in range(len(ORDERS))}) > 12      # the order matters
    # an empty list, a code outside 1..4 and codes after the terminator leave the frame as it is
    same = nat.image_jitter_u8_host(frames[:3], np.stack([record(()), record((7, 15)), record((0, B), fb=0.5)]))
    assert np.array_equal(same, frames[:3])
    assert np.array_equal(nat.image_jitter_u8_host(frames[:1], record((9, B), fb=0.5)[None])[0],
                          pil_jitter(frames[0], (B,), fb=0.5))


class _Spy:
    """A ColorJitter whose get_params keeps what it drew."""

    def __init__(self, *a, **kw):
        from data import transforms as T

        class Spy(T.ColorJitter):
            def get_params(inner):
                inner.drawn = super().get_params()
                return inner.drawn
        self.jitter = Spy(*a, **kw)


@pytest.mark.parametrize("args", [(0.2, 0.2, 0.2, 0.05), (0.4, 0.0, 0.3, 0.5), (0.0, 0.3, 0.0, 0.0)])
def test_params_record_is_the_draw_of_call(lib, args):
    import bev_native as nat
    from data import transforms as T
    arr = np.random.default_rng(3).integers(0, 256, size=(19, 23, 3), dtype=np.uint8)
    enabled = [v != 0.0 for v in args]
    for seed in range(6):
        cj = _Spy(*args).jitter
        torch.manual_seed(seed)
        want_img = np.array(cj(Image.fromarray(arr)))
        after_call = torch.get_rng_state()
        fn_idx, b, c, s, h = cj.drawn
        torch.manual_seed(seed)
        rec = T.ColorJitter(*args).params_record()
        assert torch.equal(torch.get_rng_state(), after_call)
        assert rec.dtype == torch.int32 and rec.shape == (8,)
        r = rec.numpy()
        ops = [(int(r[0]) >> (4 * i)) & 15 for i in range(8)]
        assert ops == [i + 1 for i in fn_idx.tolist() if enabled[i]] + [0] * (8 - sum(enabled))
        for word, f in ((1, b), (2, c), (3, s)):
            assert r[word] == np.array([1.0 if f is None else f], dtype=np.float32).view(np.int32)[0]
        assert r[4] == (0 if h is None else int(T._hue_shift_byte(h))) and (r[5:] == 0).all()
        assert np.array_equal(nat.image_jitter_u8_host(arr[None], r[None])[0], want_img), seed


def _seed_for(applied):
    g = torch.Generator()
    for seed in range(1 << 16):
        g.manual_seed(seed)
        if (0.5 >= float(torch.rand(1, generator=g))) == applied:
            return seed
    raise AssertionError("no seed found")


@pytest.mark.parametrize("applied", [True, False])
def test_native_size_jitter_draws_as_random_apply(lib, applied):
    import bev_native as nat
    from data import transforms as T
    arr = np.random.default_rng(4).integers(0, 256, size=(21, 17, 3), dtype=np.uint8)
    seed = _seed_for(applied)
    torch.manual_seed(seed)
    want = np.array(T.RandomApply([T.ColorJitter(0.2, 0.2, 0.2, 0.05)], p=0.5)(Image.fromarray(arr)))
    after = torch.get_rng_state()
    assert np.array_equal(want, arr) != applied
    tf = T.build_transforms((8, 8), normalize=False, resize=False, jitter=True)
    assert [type(s) for s in tf.transforms] == [T.NativeSizeJitter]
    torch.manual_seed(seed)
    frame, rec = tf(Image.fromarray(arr))
    assert torch.equal(torch.get_rng_state(), after)
    assert frame.dtype == torch.uint8 and np.array_equal(frame.numpy(), arr)
    assert rec.dtype == torch.int32 and rec.shape == (8,) and bool(rec[0] != 0) == applied
    assert applied or not rec.any()
    assert np.array_equal(nat.image_jitter_u8_host(arr[None], rec.numpy()[None])[0], want)


def test_hue_shift_byte_helper():
    """`_adjust_hue` and the records share one expression for the byte."""
    from data import transforms as T
    for f in (0.0, 0.05, -0.05, 0.5, -0.5, 0.0123, -0.0456):
        assert T._hue_shift_byte(f) == np.array(f * 255).astype(np.uint8)
    assert all(int(T._hue_shift_byte(f)) == b for b, f in HUE_FACTORS.items() if f is not None)


def test_header_library_and_signatures(lib):
    import bev_native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bev_mi355x.h")).read(), flags=re.S)
    exported = {line.split()[-1] for line in subprocess.check_output(
        ["nm", "-D", "--defined-only", os.path.join(PKG, "libbev_mi355x.so")], text=True).splitlines() if line.strip()}
    for e in ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % e, txt)
        assert m, e
        assert e in exported and e in bev_native.SIGNATURES and hasattr(lib, e)
        assert len(bev_native.SIGNATURES[e][1]) == len(m.group(1).split(",")), e
    assert bev_native.SIGNATURES["bev_image_jitter_workspace_bytes"][0] is ctypes.c_int64
    assert lib.bev_abi_version() == bev_native.ABI_VERSION == 18      # new entries only: the number stays


# Argument order of the two launches and one accepted argument set each; the addresses are made up and never handed to
# a kernel: every row is answered (0 for N == 0, BEV_ERR_ARGS otherwise) before any HIP call.
_JIT_ORDER = "src N H W params mean std workspace workspace_bytes out stream".split()
_RS_ORDER = "src N Hs Ws plan_dev H W out_u8 stream".split()
_JIT_ROWS = (
    [({}, 0), (dict(src=0x10003), 0), (dict(out=0x30004), 0), (dict(workspace_bytes=0), 0)]
    + [(dict({k: None}, N=n), -1) for k in ("src", "params", "mean", "std", "workspace", "out") for n in (0, 2)]
    + [(dict({k: v}, N=n), -1) for k in ("H", "W") for v in (0, -1) for n in (0, 2)]
    + [(dict(N=-1), -1)]
    + [(dict(N=2, workspace_bytes=b), -1) for b in (0, 8, 15)]           # 8 bytes per frame
    + [(dict(params=0x20002, N=n), -1) for n in (0, 2)]                  # int32 records: 4-B aligned
    + [(dict(workspace=0x40004, N=n), -1) for n in (0, 2)]               # 64-bit sums: 8-B aligned
    + [(dict(out=0x30002, N=n), -1) for n in (0, 2)]
)
_RS_ROWS = (
    [({}, 0), (dict(src=0x10001), 0), (dict(out_u8=0x30001), 0), (dict(Hs=8, Ws=8, H=8, W=8), 0),
     (dict(Hs=17 * 3, Ws=17 * 5, H=3, W=5), 0)]
    + [(dict({k: None}, N=n), -1) for k in ("src", "plan_dev", "out_u8") for n in (0, 2)]
    + [(dict({k: v}, N=n), -1) for k in ("Hs", "Ws", "H", "W") for v in (0, -1) for n in (0, 2)]
    + [(dict(N=-1), -1)]
    + [(dict(Hs=17 * 3 + 1, Ws=17 * 5, H=3, W=5, N=n), -1) for n in (0, 2)]   # past the downscale limit
    + [(dict(plan_dev=0x20002, N=n), -1) for n in (0, 2)]
)


def test_launch_argument_rules_without_gpu(lib):
    mean, std = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    jit = dict(src=0x10000, N=0, H=16, W=24, params=0x20000, mean=mean, std=std, workspace=0x40000,
               workspace_bytes=64, out=0x30000, stream=None)
    rs = dict(src=0x10000, N=0, Hs=64, Ws=96, plan_dev=0x20000, H=16, W=24, out_u8=0x30000, stream=None)
    bad = []
    for fn, base, order, rows in ((lib.bev_image_jitter_normalize_u8_f32, jit, _JIT_ORDER, _JIT_ROWS),
                                  (lib.bev_image_resize_u8, rs, _RS_ORDER, _RS_ROWS)):
        for changes, want in rows:
            args = dict(base)
            args.update(changes)
            assert want == -1 or args["N"] == 0, "only empty or rejected calls: nothing may reach a kernel"
            got = fn(*[args[k] for k in order])
            if got != want:
                bad.append((changes, want, got))
    assert not bad, bad
    assert [lib.bev_image_jitter_workspace_bytes(n) for n in (-1, 0, 1, 14)] == [0, 0, 8, 112]


def test_host_entry_argument_rules(lib):
    src = np.zeros((2, 4, 5, 3), dtype=np.uint8)
    out = np.full(src.size + 1, 7, dtype=np.uint8)
    rec = np.zeros((2, 8), dtype=np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.bev_image_jitter_u8_host(p(src), 2, 4, 5, p(rec), p(out)) == 0
    assert (out[:-1] == 0).all() and out[-1] == 7        # nothing written past the frames
    assert lib.bev_image_jitter_u8_host(p(src), 0, 4, 5, p(rec), p(out)) == 0
    for args in ((None, 2, 4, 5, p(rec), p(out)), (p(src), 2, 4, 5, None, p(out)), (p(src), 2, 4, 5, p(rec), None),
                 (p(src), -1, 4, 5, p(rec), p(out)), (p(src), 2, 0, 5, p(rec), p(out)),
                 (p(src), 2, 4, -1, p(rec), p(out))):
        assert lib.bev_image_jitter_u8_host(*args) == -1


def test_python_surface_raises(lib, tmp_path):
    import bev_native as nat
    from data import transforms as T
    from data.wildtrack_loader import WildtrackDataset
    arr = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    for bad in (float("nan"), -0.25, float("inf")):
        for word in ("fb", "fc", "fs"):
            with pytest.raises(ValueError):
                nat.image_jitter_u8_host(arr, record((B, C, S), **{word: bad})[None])
    with pytest.raises(ValueError):
        nat.image_jitter_u8_host(arr, record((C, B, C))[None])           # one mean per frame
    with pytest.raises(ValueError):
        nat.image_jitter_u8_host(arr, np.zeros((2, 8), dtype=np.int32))  # one record per frame
    with pytest.raises(ValueError):
        nat.image_jitter_u8_host(arr, np.zeros((1, 8), dtype=np.int64))
    with pytest.raises(ValueError):
        nat.image_jitter_u8_host(arr[0], np.zeros((1, 8), dtype=np.int32))
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    rec = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(nat.HipError, match="no CPU fallback"):
        nat.image_resize_u8(x, (4, 4))
    with pytest.raises(nat.HipError, match="no CPU fallback"):
        nat.image_jitter_normalize_u8(x, rec, T.IMAGENET_MEAN, T.IMAGENET_STD)
    with pytest.raises(nat.HipError, match="no CPU fallback"):
        T.resize_jitter_normalize_on_device(x, (4, 4), rec)
    with pytest.raises(nat.HipError, match="no CPU fallback"):
        T.jitter_normalize_on_device(x, rec)
    with pytest.raises(ValueError):
        T.build_transforms((8, 8), normalize=False, jitter=True)         # the host pipeline jitters by itself
    with pytest.raises(ValueError):
        WildtrackDataset({"DATA": {"DATA_ROOT": str(tmp_path), "VIEWS": 7, "IMG_SIZE": [3, 8, 8]}}, jitter=True)
    for name in ("NativeSizeJitter", "jitter_normalize_on_device", "resize_jitter_normalize_on_device"):
        assert name in T.__all__


def test_resize_false_without_jitter_still_draws_nothing():
    from data import transforms as T
    arr = np.random.default_rng(2).integers(0, 256, size=(41, 57, 3), dtype=np.uint8)
    torch.manual_seed(11)
    before = torch.get_rng_state()
    for tf in (T.build_transforms((20, 30), normalize=False, resize=False),
               T.build_transforms((20, 30), normalize=False, resize=False, jitter=False)):
        got = tf(Image.fromarray(arr))
        assert torch.equal(torch.get_rng_state(), before)
        assert isinstance(got, torch.Tensor) and np.array_equal(got.numpy(), arr)
        assert [type(s) for s in tf.transforms] == [T.ToUint8HWC]


def test_dataset_items_carry_the_records(tmp_path):
    from data import transforms as T
    from data.wildtrack_loader import WildtrackDataset, collate_fn
    from test_image_resize_host import _write_tree
    arrays = _write_tree(tmp_path, (45, 77))
    cfg = {"DATA": {"DATA_ROOT": str(tmp_path), "VIEWS": 7, "IMG_SIZE": [3, 12, 20], "BATCH_SIZE": 2}}
    torch.manual_seed(7)
    host = WildtrackDataset(cfg)
    host[0], host[1]
    after = torch.get_rng_state()
    ds = WildtrackDataset(cfg, native_size=True, jitter=True)
    torch.manual_seed(7)
    batch = collate_fn([ds[0], ds[1]])
    assert torch.equal(torch.get_rng_state(), after)     # the host pipeline's draws, in its order
    assert batch["images"].shape == (2, 7, 45, 77, 3) and batch["images"].dtype == torch.uint8
    assert batch["jitter"].shape == (2, 7, 8) and batch["jitter"].dtype == torch.int32
    assert np.array_equal(batch["images"][1, 3].numpy(), arrays[(3, 1)])
    # batches of the other modes are what they were
    assert "jitter" not in collate_fn([WildtrackDataset(cfg, native_size=True)[0]])
    assert "jitter" not in collate_fn([host[0]])
