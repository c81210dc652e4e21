"""Image transforms -- drop-in for project/data/transforms.py.

The reference builds `T.Compose([T.Resize(img_size), T.RandomApply([T.ColorJitter(0.2, 0.2, 0.2,
0.05)], p=0.5), T.ToTensor(), T.Normalize(IMAGENET_MEAN, IMAGENET_STD)])` (transforms.py:12-19)
from torchvision, which this image (and many ROCm deployments) does not ship.  This module restates
each step on PIL + torch with torchvision's semantics for PIL inputs, drawing its random numbers
from torch's global generator in the same order (RandomApply: `torch.rand(1)`; ColorJitter:
`torch.randperm(4)`, then one `uniform_` per enabled factor), so a seeded run makes the same
augmentation choices:

* Resize((H, W)): `img.resize((W, H), Image.BILINEAR)` (torchvision's PIL path);
* ColorJitter: brightness / contrast / saturation through `PIL.ImageEnhance` (Brightness,
  Contrast, Color) and hue by rotating the HSV hue byte (uint8 wrap-around), in the order of
  the drawn permutation;
* ToTensor + Normalize: `(float(u8) / 255 - mean) / std`.

The last two steps are split off by `build_transforms(..., normalize=False)`: the pipeline then
stops at an 8-bit HWC array, the batch crosses PCIe at a quarter of the fp32 bytes and
`normalize_on_device` (HIP kernel `bev_image_normalize_u8_f32`) produces the bit-identical fp32
[N, 3, H, W] input on the GPU.

`resize_normalize_on_device` (HIP kernel `bev_image_resize_normalize_u8_f32`) moves `Resize` to the
device as well: native-size uint8 frames in, the [N, 3, H, W] fp32 input out, in one launch and
bit-identical to `Normalize(ToTensor(Resize(img)))` (PIL's resize is integer arithmetic on
fixed-point coefficients, which the kernel repeats).  Its host side is
`build_transforms(img_size, normalize=False, resize=False)`: the deterministic ingest, which only
decodes to uint8 HWC -- no `Resize`, and no `ColorJitter` either, drawing nothing from the RNG.

`resize_jitter_normalize_on_device` moves the jitter too, and with it the whole pipeline.  In the
reference the jitter sits between `Resize` and `ToTensor` (and runs at inference as well, p = 0.5,
the same transform for every split: a quirk), so it cannot run on the host in front of a device
resize: the enhancements are not linear in the pixels, and the resize rounds to uint8 before them.
What stays on the host is the random draws alone: `build_transforms(img_size, normalize=False,
resize=False, jitter=True)` is `NativeSizeJitter`, which decodes the frame and draws as
`RandomApply([ColorJitter])` does -- `torch.rand(1)`, then, only if the jitter applies,
`ColorJitter.params_record()`: `randperm(4)` and one `uniform_` per factor -- so a seeded run
leaves the global generator where the host pipeline leaves it, and returns the frame with an
8-word record (the op order, the three factors as fp32 bits, the hue shift byte; all zero when
the jitter is skipped).  On the device `bev_image_resize_u8` writes the resized uint8 frames and
`bev_image_jitter_normalize_u8_f32` applies each frame's record -- PIL.ImageEnhance's blends and
Pillow's RGB <-> HSV conversions restated operation for operation -- then ToTensor + Normalize:
bit-identical to `Normalize(ToTensor(ColorJitter(Resize(img))))` on every draw.
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import numpy as np
import torch
from PIL import Image, ImageEnhance

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

__all__ = ["build_transforms", "Compose", "Resize", "RandomApply", "ColorJitter", "ToTensor", "Normalize",
           "ToUint8HWC", "NativeSizeJitter", "normalize_on_device", "resize_normalize_on_device",
           "jitter_normalize_on_device", "resize_jitter_normalize_on_device", "IMAGENET_MEAN", "IMAGENET_STD"]


class Compose:
    def __init__(self, fns: Sequence[Callable]):
        self.transforms = list(fns)

    def __call__(self, x):
        for f in self.transforms:
            x = f(x)
        return x


class Resize:
    """torchvision T.Resize((H, W)) on a PIL image: bilinear PIL resize to exactly (H, W)."""

    def __init__(self, size: Tuple[int, int]):
        self.size = (int(size[0]), int(size[1]))

    def __call__(self, img: Image.Image) -> Image.Image:
        H, W = self.size
        if img.size == (W, H):
            return img
        return img.resize((W, H), Image.BILINEAR)


class RandomApply:
    """Apply the transforms with probability p; one `torch.rand(1)` draw per call."""

    def __init__(self, fns: Sequence[Callable], p: float = 0.5):
        self.transforms = list(fns)
        self.p = float(p)

    def __call__(self, img):
        if self.p < torch.rand(1):
            return img
        for f in self.transforms:
            img = f(img)
        return img


def _range(value: float, center: float = 1.0, bound=(0.0, float("inf"))) -> Tuple[float, float]:
    lo, hi = center - float(value), center + float(value)
    return max(lo, bound[0]), min(hi, bound[1])


def _hue_shift_byte(hue_factor: float) -> np.ndarray:
    """What torchvision adds to the HSV hue byte (uint8 wrap-around); also word 4 of a jitter record."""
    return np.array(hue_factor * 255).astype(np.uint8)


def _adjust_hue(img: Image.Image, hue_factor: float) -> Image.Image:
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError(f"hue_factor ({hue_factor}) is not in [-0.5, 0.5].")
    mode = img.mode
    if mode in {"L", "1", "I", "F"}:
        return img
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += _hue_shift_byte(hue_factor)  # uint8 wrap-around, as torchvision
    h = Image.fromarray(np_h, "L")
    return Image.merge("HSV", (h, s, v)).convert(mode)


class ColorJitter:
    """torchvision T.ColorJitter(brightness, contrast, saturation, hue) for PIL images."""

    def __init__(self, brightness: float = 0.0, contrast: float = 0.0, saturation: float = 0.0, hue: float = 0.0):
        self.brightness = _range(brightness) if brightness else None
        self.contrast = _range(contrast) if contrast else None
        self.saturation = _range(saturation) if saturation else None
        self.hue = _range(hue, center=0.0, bound=(-0.5, 0.5)) if hue else None

    def get_params(self):
        fn_idx = torch.randperm(4)
        b = None if self.brightness is None else float(torch.empty(1).uniform_(*self.brightness))
        c = None if self.contrast is None else float(torch.empty(1).uniform_(*self.contrast))
        s = None if self.saturation is None else float(torch.empty(1).uniform_(*self.saturation))
        h = None if self.hue is None else float(torch.empty(1).uniform_(*self.hue))
        return fn_idx, b, c, s, h

    def __call__(self, img: Image.Image) -> Image.Image:
        fn_idx, b, c, s, h = self.get_params()
        for fn_id in fn_idx.tolist():
            if fn_id == 0 and b is not None:
                img = ImageEnhance.Brightness(img).enhance(b)
            elif fn_id == 1 and c is not None:
                img = ImageEnhance.Contrast(img).enhance(c)
            elif fn_id == 2 and s is not None:
                img = ImageEnhance.Color(img).enhance(s)
            elif fn_id == 3 and h is not None:
                img = _adjust_hue(img, h)
        return img


    def params_record(self) -> torch.Tensor:
        """Draws exactly as `__call__` does and returns the draw as the device kernel's record, int32 [8]
        (include/bev_mi355x.h): word 0 the enabled ops in the drawn order, four bits each (1 brightness, 2 contrast,
        3 saturation, 4 hue; 0 ends the list); words 1-3 the three factors as fp32 bits (the float Pillow's blend
        converts the Python double to); word 4 the hue shift byte; words 5-7 zero."""
        fn_idx, b, c, s, h = self.get_params()
        rec = np.zeros(8, dtype=np.int32)
        ops = [fn_id + 1 for fn_id in fn_idx.tolist() if (b, c, s, h)[fn_id] is not None]
        rec[0] = sum(code << (4 * i) for i, code in enumerate(ops))
        rec[1:4] = np.array([1.0 if f is None else f for f in (b, c, s)], dtype=np.float32).view(np.int32)
        rec[4] = 0 if h is None else int(_hue_shift_byte(h))
        return torch.from_numpy(rec)


class NativeSizeJitter:
    """The host side of the device jitter: `RandomApply([jitter], p)` for a frame that is resized and jittered on the
    GPU.  One `torch.rand(1)` per call as RandomApply, then (only if the jitter applies) the jitter's own draws;
    returns the frame as [Hs, Ws, 3] uint8 with its int32 [8] record (all zero: not jittered)."""

    def __init__(self, jitter: ColorJitter, p: float = 0.5):
        self.jitter = jitter
        self.p = float(p)

    def __call__(self, img: Image.Image) -> Tuple[torch.Tensor, torch.Tensor]:
        frame = ToUint8HWC()(img)
        if self.p < torch.rand(1):
            return frame, torch.zeros(8, dtype=torch.int32)
        return frame, self.jitter.params_record()


class ToUint8HWC:
    """PIL RGB image -> [H, W, 3] uint8 tensor (what ToTensor reads, before the float conversion)."""

    def __call__(self, img: Image.Image) -> torch.Tensor:
        return torch.from_numpy(np.array(img.convert("RGB"), dtype=np.uint8, copy=True))


class ToTensor:
    """PIL RGB image -> [3, H, W] float32 in [0, 1]: permute, then `.float().div(255)`."""

    def __call__(self, img: Image.Image) -> torch.Tensor:
        t = ToUint8HWC()(img).permute(2, 0, 1).contiguous()
        return t.to(dtype=torch.float32).div(255)


class Normalize:
    def __init__(self, mean: Sequence[float], std: Sequence[float]):
        self.mean = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
        self.std = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        return t.sub(self.mean).div(self.std)


def _reference_jitter() -> ColorJitter:
    return ColorJitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.05)


def build_transforms(img_size=(256, 256), normalize: bool = True, resize: bool = True, jitter: bool = False) -> Compose:
    """The reference pipeline (transforms.py:12-19).  normalize=False stops at uint8 HWC; resize=False (needs
    normalize=False) only decodes to uint8 HWC at the frame's own size, without jitter and without a draw; with
    jitter=True (needs resize=False) it also makes the pipeline's draws and returns (frame, record) for
    resize_jitter_normalize_on_device (see module doc)."""
    if jitter and resize:
        raise ValueError("build_transforms(jitter=True) asks for the draws of the device jitter: it requires "
                         "resize=False (with resize=True the jitter runs on the host, as always)")
    if not resize:
        if normalize:
            raise ValueError("build_transforms(resize=False) hands native-size uint8 frames to "
                             "resize_normalize_on_device: it requires normalize=False")
        return Compose([NativeSizeJitter(_reference_jitter(), p=0.5) if jitter else ToUint8HWC()])
    steps: List[Callable] = [
        Resize(img_size),
        RandomApply([_reference_jitter()], p=0.5),
    ]
    steps += [ToTensor(), Normalize(IMAGENET_MEAN, IMAGENET_STD)] if normalize else [ToUint8HWC()]
    return Compose(steps)


def normalize_on_device(images_u8: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """[B, V, H, W, 3] (or [N, H, W, 3]) uint8 on the GPU -> [B, V, 3, H, W] fp32 ToTensor + Normalize.

    One HIP launch (`bev_image_normalize_u8_f32`); bit-identical to ToTensor + Normalize on the CPU.
    """
    import bev_native as nat

    lead = images_u8.shape[:-3]
    H, W = images_u8.shape[-3], images_u8.shape[-2]
    flat = images_u8.reshape(-1, H, W, 3)
    out = nat.image_normalize_u8(flat, mean, std)
    return out.view(*lead, 3, H, W)


def resize_normalize_on_device(images_u8: torch.Tensor, img_size, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """[B, V, Hs, Ws, 3] (or [N, Hs, Ws, 3]) uint8 on the GPU, at the frames' native size -> [B, V, 3, H, W] fp32
    Resize(img_size) + ToTensor + Normalize.

    One HIP launch (`bev_image_resize_normalize_u8_f32`); bit-identical to PIL's BILINEAR resize followed by ToTensor +
    Normalize on the CPU.  A downscale of more than 17x per axis (more than 35 taps) is refused.
    """
    import bev_native as nat

    lead = images_u8.shape[:-3]
    Hs, Ws = images_u8.shape[-3], images_u8.shape[-2]
    H, W = int(img_size[0]), int(img_size[1])
    flat = images_u8.reshape(-1, Hs, Ws, 3)
    out = nat.image_resize_normalize_u8(flat, (H, W), mean, std)
    return out.view(*lead, 3, H, W)


def _flat_params(params: torch.Tensor, lead) -> torch.Tensor:
    if tuple(params.shape) != tuple(lead) + (8,):
        raise ValueError(f"jitter records must be int32 {tuple(lead) + (8,)}, got {tuple(params.shape)}")
    return params.reshape(-1, 8)


def jitter_normalize_on_device(images_u8: torch.Tensor, params: torch.Tensor, mean=IMAGENET_MEAN,
                               std=IMAGENET_STD) -> torch.Tensor:
    """[B, V, H, W, 3] (or [N, H, W, 3]) uint8 on the GPU, already at the output size, and the frames' jitter records
    [B, V, 8] (or [N, 8]) int32, on the CPU or the GPU -> [B, V, 3, H, W] fp32 ColorJitter + ToTensor + Normalize.

    HIP kernels of `bev_image_jitter_normalize_u8_f32`; bit-identical to the CPU transforms with the same draws.
    """
    import bev_native as nat

    lead = images_u8.shape[:-3]
    H, W = images_u8.shape[-3], images_u8.shape[-2]
    out = nat.image_jitter_normalize_u8(images_u8.reshape(-1, H, W, 3), _flat_params(params, lead), mean, std)
    return out.view(*lead, 3, H, W)


def resize_jitter_normalize_on_device(images_u8: torch.Tensor, img_size, params: torch.Tensor, mean=IMAGENET_MEAN,
                                      std=IMAGENET_STD) -> torch.Tensor:
    """[B, V, Hs, Ws, 3] (or [N, Hs, Ws, 3]) uint8 on the GPU, at the frames' native size, and the frames' jitter
    records [B, V, 8] (or [N, 8]) int32 (the batch's "jitter" of WildtrackDataset(native_size=True, jitter=True)), on
    the CPU or the GPU -> [B, V, 3, H, W] fp32: the reference's whole transform, Resize(img_size) +
    RandomApply(ColorJitter) + ToTensor + Normalize with the draws the records hold.

    `bev_image_resize_u8` (the resized uint8 frames), then `bev_image_jitter_normalize_u8_f32`; bit-identical to the
    CPU pipeline on PIL.  A downscale of more than 17x per axis is refused.
    """
    import bev_native as nat

    lead = images_u8.shape[:-3]
    Hs, Ws = images_u8.shape[-3], images_u8.shape[-2]
    H, W = int(img_size[0]), int(img_size[1])
    flat_params = _flat_params(params, lead)
    resized = nat.image_resize_u8(images_u8.reshape(-1, Hs, Ws, 3), (H, W))
    out = nat.image_jitter_normalize_u8(resized, flat_params, mean, std)
    return out.view(*lead, 3, H, W)
