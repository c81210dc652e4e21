"""Device resize of camera frames (bev_image_resize_normalize_u8_f32): Resize + ToTensor + Normalize in one launch,
bit for bit what the CPU transforms (PIL's BILINEAR resize, then torch) produce.

The kernel's tiles are 64 output columns by TH output rows (TH = 16 while the tile's source rows fit its LDS
intermediate, else 8, 4, 2, 1); the geometries below cross the tile seams in both directions, end in partial tiles,
take the float4 store path (W % 4 == 0, 16-B aligned output) and the scalar one, and reach the downscale limit.
"""
import numpy as np
import pytest
import torch
from PIL import Image

from data import transforms as T
from test_image_resize_host import SHAPES, _write_tree

pytestmark = pytest.mark.gpu

GEOMETRIES = [(i, o, 3) for i, o in SHAPES] + [
    ((12, 16), (12, 16), 3),      # the identity: forwards to the normalize kernels
    ((5, 5), (1, 1), 3),
    ((33, 35), (2, 3), 3),
    ((51, 85), (3, 5), 3),        # in_size == 17 * out_size on both axes: the downscale limit (35 taps)
    ((340, 136), (20, 8), 2),     # the limit with TH = 8 (a 16-row tile's 291 source rows do not fit): 3 row tiles
    # 3 x 3 tiles of 64 x 16: column seams at 64 and 128, row seams at 16 and 32, partial tiles at both far edges
    # (22 columns, 8 rows); W % 4 != 0: scalar stores
    ((96, 200), (40, 150), 2),
    # the same seams on the float4 store path (W % 4 == 0): far tiles of 4 columns and 4 rows
    ((70, 300), (36, 132), 2),
    # the horizontal pass runs unrolled for windows of up to 4, 8 and 12 taps and looped beyond: 2x (4 taps), 4x (8),
    # 5x (10) and 6.5x (13) along x
    ((20, 260), (10, 130), 2), ((20, 260), (10, 65), 2), ((20, 250), (10, 50), 2), ((20, 260), (10, 40), 2),
    ((1080, 1920), (270, 480), 1),  # the shipped configuration: 8 x 17 tiles
]


def _reference(frames, out_hw):
    """[N, Hs, Ws, 3] uint8 numpy -> [N, 3, H, W] fp32 through the transforms classes on the CPU."""
    rs, tt, nm = T.Resize(out_hw), T.ToTensor(), T.Normalize(T.IMAGENET_MEAN, T.IMAGENET_STD)
    return torch.stack([nm(tt(rs(Image.fromarray(a)))) for a in frames])


def _contents(rng, n, Hs, Ws):
    corners = np.zeros((4, Hs, Ws, 3), dtype=np.uint8)  # one bright pixel per image, one image per corner
    for i, (y, x) in enumerate(((0, 0), (0, Ws - 1), (Hs - 1, 0), (Hs - 1, Ws - 1))):
        corners[i, y, x] = (255, 200 + i, 131)
    return {"random": rng.integers(0, 256, size=(n, Hs, Ws, 3), dtype=np.uint8),
            "0/255": (rng.integers(0, 2, size=(n, Hs, Ws, 3), dtype=np.uint8) * 255).astype(np.uint8),
            "corners": corners}


def _same_bits(got, want):
    return got.shape == want.shape and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("in_hw,out_hw,n", GEOMETRIES)
def test_bit_exact_against_the_cpu_transforms(in_hw, out_hw, n):
    import bev_native as nat
    rng = np.random.default_rng(in_hw[0] * 7 + in_hw[1] * 3 + out_hw[0])
    for name, frames in _contents(rng, n, *in_hw).items():
        want = _reference(frames, out_hw)
        dev = torch.from_numpy(frames).cuda()
        got = nat.image_resize_normalize_u8(dev, out_hw, T.IMAGENET_MEAN, T.IMAGENET_STD)
        assert got.dtype == torch.float32 and _same_bits(got, want), (name, in_hw, out_hw)
        if in_hw == out_hw:
            assert _same_bits(T.normalize_on_device(dev), want)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_source_and_output(offset):
    """src starting 1, 2, 3 bytes into a buffer with odd Ws (3 * Ws not a multiple of 4); out= only 4-B aligned, with
    W % 4 == 0 (the geometry that would otherwise take the float4 stores) and with odd W."""
    import bev_native as nat
    rng = np.random.default_rng(offset)
    for (Hs, Ws), (H, W) in (((37, 53), (12, 20)), ((21, 75), (9, 67))):
        frames = rng.integers(0, 256, size=(2, Hs, Ws, 3), dtype=np.uint8)
        want = _reference(frames, (H, W))
        buf = torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda")
        buf[offset:offset + frames.size] = torch.from_numpy(frames).cuda().reshape(-1)
        src = buf[offset:offset + frames.size].view(2, Hs, Ws, 3)
        assert src.data_ptr() % 4 == offset and src.is_contiguous()
        assert _same_bits(nat.image_resize_normalize_u8(src, (H, W), T.IMAGENET_MEAN, T.IMAGENET_STD), want)
        obuf = torch.full((want.numel() + 4,), float("nan"), device="cuda")
        out = obuf[1:1 + want.numel()].view(2, 3, H, W)
        assert out.data_ptr() % 16 == 4
        got = nat.image_resize_normalize_u8(src, (H, W), T.IMAGENET_MEAN, T.IMAGENET_STD, out=out)
        assert got.data_ptr() == out.data_ptr() and _same_bits(out, want)
        assert torch.isnan(obuf[0]) and torch.isnan(obuf[1 + want.numel():]).all()  # nothing written around it


def test_wrapper_shapes_and_plan_cache():
    import bev_native as nat
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, size=(2, 3, 40, 72, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(4, 33, 61, 3), dtype=np.uint8)
    want_a = _reference(a.reshape(6, 40, 72, 3), (10, 18)).view(2, 3, 3, 10, 18)
    want_b = _reference(b, (17, 30))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for _ in range(3):  # two geometries alternating in one process: each keeps its own tables
        got = T.resize_normalize_on_device(da, (10, 18))
        assert got.shape == (2, 3, 3, 10, 18) and _same_bits(got, want_a)
        got = T.resize_normalize_on_device(db, (17, 30))
        assert got.shape == (4, 3, 17, 30) and _same_bits(got, want_b)
    dev = torch.cuda.current_device()
    assert (dev, 40, 72, 10, 18) in nat._RESIZE_PLANS and (dev, 33, 61, 17, 30) in nat._RESIZE_PLANS
    with pytest.raises(ValueError):
        nat.image_resize_normalize_u8(da, (10, 18), T.IMAGENET_MEAN, T.IMAGENET_STD)          # 5-D
    with pytest.raises(ValueError):
        nat.image_resize_normalize_u8(db.float(), (10, 18), T.IMAGENET_MEAN, T.IMAGENET_STD)  # dtype
    with pytest.raises(ValueError):
        nat.image_resize_normalize_u8(db, (1, 30), T.IMAGENET_MEAN, T.IMAGENET_STD)           # 33 rows -> 1: past 17x


def _seed_without_jitter(draws):
    """A torch seed whose first `draws` RandomApply draws all skip the jitter (p < torch.rand(1), p = 0.5)."""
    g = torch.Generator()
    for seed in range(1 << 20):
        g.manual_seed(seed)
        if all(0.5 < float(torch.rand(1, generator=g)) for _ in range(draws)):
            return seed
    raise AssertionError("no seed found")


def test_native_size_batch_equals_the_host_pipeline(tmp_path):
    """WildtrackDataset(native_size=True) -> collate_fn -> .cuda() -> resize_normalize_on_device equals the batch of
    WildtrackDataset(cfg) on the draws where RandomApply skips the jitter, and feeds BEVNet."""
    from data.wildtrack_loader import WildtrackDataset, collate_fn
    from models.model_wrapper import BEVNet
    _write_tree(tmp_path, (108, 192))
    cfg = {"DATA": {"DATA_ROOT": str(tmp_path), "VIEWS": 7, "IMG_SIZE": [3, 54, 96], "BATCH_SIZE": 2},
           "LOSS": {"DEFAULT_BOX_WH": [0.5, 0.7]},
           "MODEL": {"BACKBONE": "resnet18", "PRETRAINED": False, "FEAT_DIM": 32, "OUT_INDEX": 2,
                     "BEV_SIZE": [32, 24, 72], "BEV_BOUNDS": [-24.0, 24.0, -7.2, 7.2], "BEV_PROJ_CH": 32}}
    seed = _seed_without_jitter(14)
    torch.manual_seed(seed)
    draws = [float(torch.rand(1)) for _ in range(14)]
    assert all(0.5 < d for d in draws), draws
    host = WildtrackDataset(cfg)
    torch.manual_seed(seed)
    want = collate_fn([host[0], host[1]])["images"]        # 2 frames x 7 views: the 14 draws above
    native = WildtrackDataset(cfg, native_size=True)
    batch = collate_fn([native[0], native[1]])
    assert batch["images"].shape == (2, 7, 108, 192, 3) and batch["images"].dtype == torch.uint8
    images = T.resize_normalize_on_device(batch["images"].cuda(), native.img_size)
    assert images.shape == (2, 7, 3, 54, 96) and _same_bits(images, want)
    calib = {k: [[m.cuda() for m in per] for per in batch["calib"][k]] for k in ("intrinsic", "extrinsic")}
    torch.manual_seed(0)
    net = BEVNet(cfg).cuda().eval()
    with torch.no_grad():
        out = net({"images": images, "calib": calib})
    assert out["heatmap_logits"].shape[-2:] == (24, 72) and torch.isfinite(out["heatmap_logits"]).all()
