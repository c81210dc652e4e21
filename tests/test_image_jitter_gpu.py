"""Colour jitter on the device (bev_image_resize_u8 + bev_image_jitter_normalize_u8_f32): bit for bit what the CPU
transforms on PIL produce, compared as fp32 bit patterns against Normalize(ToTensor(.)) of the jittered uint8 frame --
the PIL classes' and the host entry's (bev_image_jitter_u8_host, itself held to PIL by test_image_jitter_host.py).

The jitter kernels give a workgroup 1024 pixels of one frame on the vector path (H * W % 4 == 0, src 4-B and out 16-B
aligned; a lane = 4 pixels) and 256 on the scalar one: 37 x 53 frames take the scalar path with a partial last
workgroup, 96 x 200 frames the vector path with 18.75 workgroups per frame, so contrast's sum spans them.
"""
import numpy as np
import pytest
import torch
from PIL import Image

from data import transforms as T
from test_image_jitter_host import (B, C, H, ORDERS, S, all_colours, half_frames, order_batch, pil_jitter, record)
from test_image_resize_host import SHAPES, _write_tree

pytestmark = pytest.mark.gpu

MEAN, STD = T.IMAGENET_MEAN, T.IMAGENET_STD


def _normalized(frames_u8):
    """[N, H, W, 3] uint8 numpy -> [N, 3, H, W] fp32: ToTensor + Normalize on the CPU."""
    tt, nm = T.ToTensor(), T.Normalize(MEAN, STD)
    return torch.stack([nm(tt(Image.fromarray(a))) for a in frames_u8])


def _same_bits(got, want):
    return got.shape == want.shape and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


def _decode(rec):
    ops = [(int(rec[0]) >> (4 * i)) & 15 for i in range(8)]
    fb, fc, fs = (float(v) for v in rec[1:4].view(np.float32))
    return dict(ops=ops[:ops.index(0)], fb=fb, fc=fc, fs=fs, hue_byte=int(rec[4]))


def _pil_batch(frames, recs):
    return np.stack([pil_jitter(a, **_decode(r)) for a, r in zip(frames, recs)])


def _check_batch(frames, recs, want_u8=None, pil=True):
    """The device against the host entry and (pil) the PIL classes, whose results agree; then a second launch."""
    import bev_native as nat
    host = nat.image_jitter_u8_host(frames, recs)
    if pil:
        if want_u8 is None:
            want_u8 = _pil_batch(frames, recs)
        assert np.array_equal(host, want_u8)
    else:
        want_u8 = host
    want = _normalized(want_u8)
    dev = torch.from_numpy(frames).cuda()
    got = nat.image_jitter_normalize_u8(dev, torch.from_numpy(recs), MEAN, STD)        # records from the CPU
    assert got.dtype == torch.float32 and _same_bits(got, want)
    again = nat.image_jitter_normalize_u8(dev, torch.from_numpy(recs).cuda(), MEAN, STD)  # ... and on the device
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))                 # two launches, equal bits
    return got


def test_all_op_orders_scalar_path():
    frames, recs, want = order_batch()                   # N = 24, 37 x 53: H * W is odd
    _check_batch(frames, recs, want)


def test_per_frame_records_vector_path():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(5, 96, 200, 3), dtype=np.uint8)
    recs = np.stack([record((C, H, B, S), fb=0.85, fc=1.17, fs=0.93, hue_byte=250),
                     record(()),                                         # not jittered: the normalize kernel's result
                     record((S, B, H), fb=1.2, fs=0.8, hue_byte=12),     # no contrast: pass 1 leaves at once
                     record((B, S, H, C), fb=1.07, fc=0.81, fs=1.2, hue_byte=3),
                     record((C,), fc=1.2)])
    got = _check_batch(frames, recs)
    import bev_native as nat
    assert _same_bits(got[1:2], nat.image_normalize_u8(torch.from_numpy(frames[1:2]).cuda(), MEAN, STD).cpu())
    assert _same_bits(T.jitter_normalize_on_device(torch.from_numpy(frames).cuda().view(1, 5, 96, 200, 3),
                                                   torch.from_numpy(recs).view(1, 5, 8)), got.cpu().view(1, 5, 3, 96, 200))


def test_contrast_rounding_across_workgroups():
    frames, recs = [], []
    for k in (0, 127, 254):
        for arr in half_frames(k, 96, 200).values():
            for f in (0.0, 0.8, 1.2):
                frames.append(arr)
                recs.append(record((C,), fc=f))
    got = _check_batch(np.stack(frames), np.stack(recs))
    # factor 0 shows the mean itself: k + 1 on the exact-half frame, k one pixel below it
    x = got.cpu()
    assert not _same_bits(x[0], x[3]) and not _same_bits(x[6], x[9]) and not _same_bits(x[12], x[15])


def test_hue_over_all_colours():
    """Against the host entry, which test_image_jitter_host.py holds to Pillow on this frame and these bytes."""
    img = all_colours()                                  # 4096 x 4096: 16384 workgroups of the vector path
    frames = np.stack([img, img])
    recs = np.stack([record((H,), hue_byte=12), record((H,), hue_byte=243)])
    _check_batch(frames, recs, pil=False)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_source_and_output(offset):
    """src starting 1, 2, 3 bytes into a buffer; out= only 4-B aligned, with NaN guards around it; 40 x 52 would
    otherwise take the vector path, 37 x 53 never does."""
    import bev_native as nat
    rng = np.random.default_rng(offset)
    for Hh, Ww in ((40, 52), (37, 53)):
        frames = rng.integers(0, 256, size=(2, Hh, Ww, 3), dtype=np.uint8)
        recs = np.stack([record((H, C, S, B), fb=1.1, fc=0.9, fs=1.15, hue_byte=7), record((B, C), fb=0.8, fc=1.2)])
        want = _normalized(_pil_batch(frames, recs))
        buf = torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda")
        buf[offset:offset + frames.size] = torch.from_numpy(frames).cuda().reshape(-1)
        src = buf[offset:offset + frames.size].view(2, Hh, Ww, 3)
        assert src.data_ptr() % 4 == offset and src.is_contiguous()
        assert _same_bits(nat.image_jitter_normalize_u8(src, torch.from_numpy(recs), MEAN, STD), want)
        obuf = torch.full((want.numel() + 4,), float("nan"), device="cuda")
        out = obuf[1:1 + want.numel()].view(2, 3, Hh, Ww)
        assert out.data_ptr() % 16 == 4
        got = nat.image_jitter_normalize_u8(torch.from_numpy(frames).cuda(), torch.from_numpy(recs), MEAN, STD, out=out)
        assert got.data_ptr() == out.data_ptr() and _same_bits(out, want)
        assert torch.isnan(obuf[0]) and torch.isnan(obuf[1 + want.numel():]).all()      # nothing written around it


# ((20, 260), (10, 40)): 6.5x along x, the looped instance (NG = 0).  SHAPES hold windows of up to 4 and 8 taps (NG = 1,
# 2) but none of 9 to 12, so two 5x geometries are added for NG = 3.  Each instance meets W % 4 == 0 (dword stores) and
# the byte stores (any W with out= one byte into a buffer).
RESIZE_SHAPES = SHAPES + [((96, 200), (40, 150)), ((20, 260), (10, 40)), ((20, 250), (10, 50)), ((20, 260), (10, 52))]


@pytest.mark.parametrize("in_hw,out_hw", RESIZE_SHAPES)
def test_resize_u8_equals_pil(in_hw, out_hw):
    import bev_native as nat
    rng = np.random.default_rng(in_hw[0] * 7 + in_hw[1] * 3 + out_hw[0])
    frames = rng.integers(0, 256, size=(2,) + in_hw + (3,), dtype=np.uint8)
    want = np.stack([np.array(T.Resize(out_hw)(Image.fromarray(a))) for a in frames])
    dev = torch.from_numpy(frames).cuda()
    got = nat.image_resize_u8(dev, out_hw)
    assert got.dtype == torch.uint8 and got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    # out= one byte into a buffer (byte stores), guards untouched
    obuf = torch.full((want.size + 2,), 77, dtype=torch.uint8, device="cuda")
    out = obuf[1:1 + want.size].view(want.shape)
    nat.image_resize_u8(dev, out_hw, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and int(obuf[0]) == 77 and int(obuf[-1]) == 77


def test_resize_u8_identity_and_wrapper_rules():
    import bev_native as nat
    frames = np.random.default_rng(1).integers(0, 256, size=(3, 12, 16, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    assert np.array_equal(nat.image_resize_u8(dev, (12, 16)).cpu().numpy(), frames)     # a device copy
    nat.image_resize_u8(dev, (5, 9))
    assert (torch.cuda.current_device(), 12, 16, 5, 9) in nat._RESIZE_PLANS             # the shared plan cache
    with pytest.raises(ValueError):
        nat.image_resize_u8(dev.float(), (5, 9))
    with pytest.raises(ValueError):
        nat.image_resize_u8(dev, (5, 9), out=torch.empty(3, 5, 9, 3, device="cuda"))    # dtype
    rec = torch.zeros(3, 8, dtype=torch.int32)
    with pytest.raises(ValueError):
        nat.image_jitter_normalize_u8(dev, rec[:2], MEAN, STD)
    with pytest.raises(ValueError):
        nat.image_jitter_normalize_u8(dev, rec.float(), MEAN, STD)
    with pytest.raises(ValueError):
        nat.image_jitter_normalize_u8(dev, rec, MEAN, STD, out=torch.empty(3, 3, 16, 12, device="cuda"))
    bad = rec.clone()
    bad[1] = torch.from_numpy(record((B,), fb=float("nan")))
    with pytest.raises(ValueError):
        nat.image_jitter_normalize_u8(dev, bad, MEAN, STD)
    bad[1] = torch.from_numpy(record((S,), fs=-0.5))
    with pytest.raises(ValueError):
        nat.image_jitter_normalize_u8(dev, bad, MEAN, STD)


def test_resize_jitter_normalize_on_device():
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, size=(2, 3, 96, 200, 3), dtype=np.uint8)
    recs = np.stack([record(o, fb=0.9, fc=1.1, fs=0.85, hue_byte=246) for o in ORDERS[3:9]]).reshape(2, 3, 8)
    recs[1, 1] = 0
    for out_hw in ((40, 150), (24, 52)):
        resized = [T.Resize(out_hw)(Image.fromarray(a)) for a in frames.reshape(6, 96, 200, 3)]
        want_u8 = np.stack([pil_jitter(np.array(im), **_decode(r)) for im, r in zip(resized, recs.reshape(6, 8))])
        want = _normalized(want_u8).view(2, 3, 3, *out_hw)
        got = T.resize_jitter_normalize_on_device(torch.from_numpy(frames).cuda(), out_hw, torch.from_numpy(recs))
        assert got.shape == want.shape and _same_bits(got, want)
        flat = T.resize_jitter_normalize_on_device(torch.from_numpy(frames).cuda().view(6, 96, 200, 3), out_hw,
                                                   torch.from_numpy(recs).view(6, 8).cuda())
        assert _same_bits(flat, want.view(6, 3, *out_hw))


def _seed_with_a_mix(draws):
    """A torch seed whose first RandomApply draws of 2 x 7 frames (p < torch.rand(1), p = 0.5) apply the jitter to some
    and skip it for others -- found by running the host pipeline's own draws."""
    jitter = T.ColorJitter(0.2, 0.2, 0.2, 0.05)
    for seed in range(64):
        torch.manual_seed(seed)
        applied = []
        for _ in range(draws):
            applied.append(not (0.5 < torch.rand(1)))
            if applied[-1]:
                jitter.get_params()
        if 4 <= sum(applied) <= draws - 4:
            return seed, applied
    raise AssertionError("no seed found")


def test_native_size_jittered_batch_equals_the_host_pipeline(tmp_path):
    """WildtrackDataset(native_size=True, jitter=True) -> collate_fn -> .cuda() -> resize_jitter_normalize_on_device
    equals the batch of WildtrackDataset(cfg) after the same seed, jittered and skipped frames alike, and feeds BEVNet."""
    from data.wildtrack_loader import WildtrackDataset, collate_fn
    from models.model_wrapper import BEVNet
    _write_tree(tmp_path, (108, 192))
    cfg = {"DATA": {"DATA_ROOT": str(tmp_path), "VIEWS": 7, "IMG_SIZE": [3, 54, 96], "BATCH_SIZE": 2},
           "LOSS": {"DEFAULT_BOX_WH": [0.5, 0.7]},
           "MODEL": {"BACKBONE": "resnet18", "PRETRAINED": False, "FEAT_DIM": 32, "OUT_INDEX": 2,
                     "BEV_SIZE": [32, 24, 72], "BEV_BOUNDS": [-24.0, 24.0, -7.2, 7.2], "BEV_PROJ_CH": 32}}
    seed, applied = _seed_with_a_mix(14)
    host = WildtrackDataset(cfg)
    torch.manual_seed(seed)
    want = collate_fn([host[0], host[1]])["images"]        # 2 frames x 7 views
    after = torch.get_rng_state()
    native = WildtrackDataset(cfg, native_size=True, jitter=True)
    torch.manual_seed(seed)
    batch = collate_fn([native[0], native[1]])
    assert torch.equal(torch.get_rng_state(), after)
    assert batch["images"].shape == (2, 7, 108, 192, 3) and batch["images"].dtype == torch.uint8
    assert batch["jitter"].shape == (2, 7, 8) and batch["jitter"].dtype == torch.int32
    assert (batch["jitter"][..., 0] != 0).reshape(-1).tolist() == applied
    assert 4 <= sum(applied) <= 10                         # both jittered and skipped frames
    images = T.resize_jitter_normalize_on_device(batch["images"].cuda(), native.img_size, batch["jitter"])
    assert images.shape == (2, 7, 3, 54, 96) and _same_bits(images, want)
    calib = {k: [[m.cuda() for m in per] for per in batch["calib"][k]] for k in ("intrinsic", "extrinsic")}
    torch.manual_seed(0)
    net = BEVNet(cfg).cuda().eval()
    with torch.no_grad():
        out = net({"images": images, "calib": calib})
    assert out["heatmap_logits"].shape[-2:] == (24, 72) and torch.isfinite(out["heatmap_logits"]).all()
