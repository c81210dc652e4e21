"""Device resize of camera frames, host side (no GPU): the coefficient tables of bev_image_resize_plan against
Pillow, the C entries' argument rules, and the Python surface of the native-size ingest.

Pillow's 8-bit BILINEAR resize (ImagingResample) is integer arithmetic on 22-bit fixed-point coefficients: a
horizontal pass to a uint8 intermediate, then a vertical pass over it.  `_two_passes` restates the passes in numpy on
the tables the kernel reads (bev_native.image_resize_plan), and must reproduce Pillow's output byte for byte.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import PKG, REPO

SHAPES = [((64, 96), (16, 24)), ((37, 53), (11, 17)), ((9, 7), (20, 31)), ((50, 10), (7, 33)), ((40, 24), (10, 24)),
          ((24, 40), (24, 10)), ((16, 16), (15, 17)), ((130, 70), (9, 64)), ((270, 480), (67, 121))]
ENTRIES = ("bev_image_resize_plan_bytes", "bev_image_resize_plan", "bev_image_resize_normalize_u8_f32")


@pytest.fixture(scope="module")
def lib():
    import bev_native
    if not os.path.exists(bev_native.LIB_PATH):
        bev_native.build()
    return bev_native.lib()


def _one_pass(a, bounds, coeffs):
    """a [n_in, ...] uint8 resampled along axis 0: out[i] = clip8((2^21 + sum_t a[lo + t] * k[i][t]) >> 22), int32."""
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.uint8)
    for i, (lo, taps) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << 21, dtype=np.int32)
        for t in range(taps):
            acc = acc + a[lo + t].astype(np.int32) * np.int32(coeffs[i, t])
        out[i] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def _two_passes(a, plan, out_hw):
    Hs, Ws = a.shape[:2]
    H, W = out_hw
    if Ws != W:  # horizontal first, to a uint8 intermediate [Hs, W, 3]
        a = _one_pass(a.transpose(1, 0, 2), plan["x"]["bounds"], plan["x"]["coeffs"]).transpose(1, 0, 2)
    if Hs != H:
        a = _one_pass(a, plan["y"]["bounds"], plan["y"]["coeffs"])
    return a


def _contents(rng, Hs, Ws):
    return {"random": rng.integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8),
            "0/255": (rng.integers(0, 2, size=(Hs, Ws, 3), dtype=np.uint8) * 255).astype(np.uint8)}


@pytest.mark.parametrize("in_hw,out_hw", SHAPES)
def test_plan_tables_reproduce_pillow(lib, in_hw, out_hw):
    import bev_native as nat
    plan = nat.image_resize_plan(in_hw, out_hw)
    for axis, n_in, n_out in (("x", in_hw[1], out_hw[1]), ("y", in_hw[0], out_hw[0])):
        t = plan[axis]
        assert t["coeffs"].dtype == np.int32 and t["coeffs"].shape == (n_out, t["ksize"])
        assert t["bounds"].dtype == np.int32 and t["bounds"].shape == (n_out, 2)
        lo, taps = t["bounds"][:, 0], t["bounds"][:, 1]
        # a window has at most ksize - 1 taps: the launch picks its unrolled kernel instances from ksize by that
        assert (lo >= 0).all() and (taps >= 1).all() and (taps <= t["ksize"] - 1).all() and (lo + taps <= n_in).all()
        assert (t["coeffs"] >= 0).all()
        # rounding each of `taps` coefficients moves the row sum by less than one each
        assert (np.abs(t["coeffs"].sum(axis=1, dtype=np.int64) - (1 << 22)) <= taps).all()
        assert all((t["coeffs"][i, taps[i]:] == 0).all() for i in range(n_out))
    # a skipped pass equals the pass run with its identity coefficients
    rng = np.random.default_rng(sum(in_hw) * 1000 + sum(out_hw))
    for name, a in _contents(rng, *in_hw).items():
        want = np.array(Image.fromarray(a).resize((out_hw[1], out_hw[0]), Image.BILINEAR))
        got = _two_passes(a, plan, out_hw)
        assert got.shape == want.shape and np.array_equal(got, want), (name, in_hw, out_hw)
        for axis, same in (("x", in_hw[1] == out_hw[1]), ("y", in_hw[0] == out_hw[0])):
            if same:
                src = a.transpose(1, 0, 2) if axis == "x" else a
                assert np.array_equal(_one_pass(src, plan[axis]["bounds"], plan[axis]["coeffs"]), src)


def test_plan_ksize_pins(lib):
    import bev_native as nat
    p = nat.image_resize_plan((64, 96), (16, 24))          # exact 4x on both axes
    assert p["x"]["ksize"] == 9 and p["y"]["ksize"] == 9
    p = nat.image_resize_plan((9, 7), (20, 31))            # any upscale
    assert p["x"]["ksize"] == 3 and p["y"]["ksize"] == 3
    p = nat.image_resize_plan((12, 16), (12, 16))          # the identity: k = {1 << 22, 0}
    assert p["x"]["ksize"] == 3 and (p["x"]["coeffs"][:, 0] == 1 << 22).all() and (p["x"]["coeffs"][:, 1:] == 0).all()
    assert (p["y"]["bounds"][:, 0] == np.arange(12)).all()
    p = nat.image_resize_plan((1080, 1920), (270, 480))    # the shipped configuration
    assert p["x"]["ksize"] == 9 and p["x"]["coeffs"].shape == (480, 9) and p["y"]["coeffs"].shape == (270, 9)
    with pytest.raises(ValueError):
        nat.image_resize_plan((18, 8), (1, 8))             # past the downscale limit
    with pytest.raises(ValueError):
        nat.image_resize_plan((0, 8), (1, 8))


def test_header_library_and_signatures(lib):
    import bev_native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bev_mi355x.h")).read(), flags=re.S)
    exported = {line.split()[-1] for line in subprocess.check_output(
        ["nm", "-D", "--defined-only", os.path.join(PKG, "libbev_mi355x.so")], text=True).splitlines() if line.strip()}
    for e in ENTRIES:
        assert re.search(r"\b%s\s*\(" % e, txt), e
        assert e in exported and e in bev_native.SIGNATURES and hasattr(lib, e)
    assert lib.bev_abi_version() == bev_native.ABI_VERSION == 18


# Argument order of the launch and one accepted argument set; the addresses are made up and never handed to a kernel:
# every row is answered (0 for N == 0, BEV_ERR_ARGS otherwise) before any HIP call.
_ORDER = "src N Hs Ws plan_dev H W mean std out stream".split()
_LIMIT = dict(Hs=17 * 3, Ws=17 * 5, H=3, W=5)       # in_size == 17 * out_size on both axes: the stated limit (35 taps)
_ROWS = (
    [({}, 0), (dict(src=0x10001), 0), (dict(out=0x30004), 0), (_LIMIT, 0), (dict(Hs=8, Ws=8, H=8, W=8), 0)]
    + [(dict({k: None}, N=n), -1) for k in ("src", "plan_dev", "mean", "std", "out") for n in (0, 2)]
    + [(dict({k: v}, N=n), -1) for k in ("Hs", "Ws", "H", "W") for v in (0, -1) for n in (0, 2)]
    + [(dict(N=-1), -1)]
    + [(dict(_LIMIT, Hs=17 * 3 + 1, N=n), -1) for n in (0, 2)]   # one source row past the limit
    + [(dict(_LIMIT, Ws=17 * 5 + 1, N=n), -1) for n in (0, 2)]
    + [(dict(plan_dev=0x20002, N=n), -1) for n in (0, 2)]        # the int32 tables are 4-B aligned
)


def test_launch_argument_rules_without_gpu(lib):
    mean, std = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    base = dict(src=0x10000, N=0, Hs=64, Ws=96, plan_dev=0x20000, H=16, W=24, mean=mean, std=std, out=0x30000,
                stream=None)
    bad = []
    for changes, want in _ROWS:
        args = dict(base)
        args.update(changes)
        assert want == -1 or args["N"] == 0, "only empty or rejected calls: nothing may reach a kernel"
        got = lib.bev_image_resize_normalize_u8_f32(*[args[k] for k in _ORDER])
        if got != want:
            bad.append((changes, want, got))
    assert not bad, bad


def test_plan_bytes_and_plan_argument_rules(lib):
    # the blob's size is a function of the four sizes: int32 bounds [n][2] + coefficients [n][ksize] per axis
    assert lib.bev_image_resize_plan_bytes(64, 96, 16, 24) == 4 * (24 * (2 + 9) + 16 * (2 + 9))
    assert lib.bev_image_resize_plan_bytes(9, 7, 20, 31) == 4 * (31 * (2 + 3) + 20 * (2 + 3))
    assert lib.bev_image_resize_plan_bytes(2160, 3840, 270, 480) > 0          # 4K -> 270 rows
    # at the limit (in_size == 17 * out_size: ksize 35) and just past it, per axis
    assert lib.bev_image_resize_plan_bytes(51, 85, 3, 5) == 4 * (5 * (2 + 35) + 3 * (2 + 35))
    assert lib.bev_image_resize_plan_bytes(52, 85, 3, 5) == 0
    assert lib.bev_image_resize_plan_bytes(51, 86, 3, 5) == 0
    assert lib.bev_image_resize_plan_bytes(48, 80, 3, 5) == 4 * (5 * (2 + 33) + 3 * (2 + 33))   # 16x: 33 taps
    assert lib.bev_image_resize_plan_bytes(1, 1, 4096, 4096) > 0              # any upscale
    for bad in ((0, 8, 4, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 4, -1), ((1 << 24) + 1, 8, 1 << 24, 8)):
        assert lib.bev_image_resize_plan_bytes(*bad) == 0, bad
    n = lib.bev_image_resize_plan_bytes(64, 96, 16, 24)
    buf = np.full(n // 4 + 1, -7, dtype=np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.bev_image_resize_plan(64, 96, 16, 24, p, n) == 0 and buf[-1] == -7 and (buf[:-1] >= 0).all()
    assert lib.bev_image_resize_plan(64, 96, 16, 24, None, n) == -1
    assert lib.bev_image_resize_plan(64, 96, 16, 24, p, n - 4) == -1
    assert lib.bev_image_resize_plan(64, 96, 16, 24, p, n + 4) == -1
    assert lib.bev_image_resize_plan(52, 85, 3, 5, p, n) == -1


def test_build_transforms_native_size_mode():
    from data import transforms as T
    assert "resize_normalize_on_device" in T.__all__
    with pytest.raises(ValueError):
        T.build_transforms((20, 30), normalize=True, resize=False)
    with pytest.raises(ValueError):
        T.build_transforms((20, 30), resize=False)
    arr = np.random.default_rng(2).integers(0, 256, size=(41, 57, 3), dtype=np.uint8)
    torch.manual_seed(11)
    before = torch.get_rng_state()
    tf = T.build_transforms((20, 30), normalize=False, resize=False)
    got = tf(Image.fromarray(arr))
    assert torch.equal(torch.get_rng_state(), before)      # no RandomApply / ColorJitter draw
    assert got.dtype == torch.uint8 and got.shape == (41, 57, 3) and np.array_equal(got.numpy(), arr)
    assert [type(s) for s in tf.transforms] == [T.ToUint8HWC]
    # the other modes are what they were
    assert [type(s) for s in T.build_transforms((20, 30)).transforms] == [T.Resize, T.RandomApply, T.ToTensor,
                                                                         T.Normalize]
    assert [type(s) for s in T.build_transforms((20, 30), normalize=False).transforms] == [T.Resize, T.RandomApply,
                                                                                          T.ToUint8HWC]


def test_cpu_tensor_and_bad_shapes_raise(lib):
    import bev_native as nat
    from data import transforms as T
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(nat.HipError, match="no CPU fallback"):
        nat.image_resize_normalize_u8(x, (4, 4), T.IMAGENET_MEAN, T.IMAGENET_STD)
    with pytest.raises(nat.HipError, match="no CPU fallback"):
        T.resize_normalize_on_device(x, (4, 4))


def _write_tree(root, frame_hw, views=7, frames=2, seed=0):
    """A tiny synthetic Wildtrack tree of PNG frames, as the fixture of tests/test_data_wildtrack.py builds one."""
    from test_data_wildtrack import CAMS, _rig, _write_extrinsic, _write_intrinsic
    (root / "calibration" / "intrinsic_zero").mkdir(parents=True)
    (root / "calibration" / "extrinsic").mkdir(parents=True)
    for v, name in enumerate(CAMS[:views]):
        K, rvec, tvec = _rig(v)
        _write_intrinsic(root / "calibration" / "intrinsic_zero" / f"intr_{name}.xml", K)
        _write_extrinsic(root / "calibration" / "extrinsic" / f"extr_{name}.xml", rvec, tvec)
    rng = np.random.default_rng(seed)
    arrays = {}
    for i in range(1, views + 1):
        d = root / "Image_subsets" / f"C{i}"
        d.mkdir(parents=True)
        for f in range(frames):
            arr = rng.integers(0, 256, size=frame_hw + (3,), dtype=np.uint8)
            Image.fromarray(arr).save(d / f"{5 * f:08d}.png")
            arrays[(i - 1, f)] = arr
    return arrays


def test_dataset_native_size(tmp_path, capsys):
    from data.wildtrack_loader import WildtrackDataset, collate_fn
    arrays = _write_tree(tmp_path, (45, 77))
    cfg = {"DATA": {"DATA_ROOT": str(tmp_path), "VIEWS": 7, "IMG_SIZE": [3, 12, 20], "BATCH_SIZE": 2}}
    ds = WildtrackDataset(cfg, native_size=True)
    assert ds.images_uint8 and ds.native_size and ds.img_size == (12, 20)
    torch.manual_seed(5)
    before = torch.get_rng_state()
    x = ds[1]["images"]
    assert torch.equal(torch.get_rng_state(), before)
    assert x.dtype == torch.uint8 and x.shape == (7, 45, 77, 3)
    for v in range(7):
        assert np.array_equal(x[v].numpy(), arrays[(v, 1)])
    assert torch.equal(ds[1]["images"], x)                 # the same pixels on a second read
    b = collate_fn([ds[0], ds[1]])
    assert b["images"].shape == (2, 7, 45, 77, 3) and b["images"].dtype == torch.uint8
    # the other modes are what they were
    assert WildtrackDataset(cfg)[0]["images"].shape == (7, 3, 12, 20)
    assert WildtrackDataset(cfg, images_uint8=True)[0]["images"].shape == (7, 12, 20, 3)
