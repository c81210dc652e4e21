"""Helpers of tests/test_size_rules_gpu.py: guarded device operands, band references in float64, block checksums and
the memory condition.  Nothing here caches a tensor."""
import gc
import time

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
GIB = 1 << 30
CAP = 32 * GIB  # no test holds more at once
LIMITS = (1 << 31, 1 << 32, 1 << 33)
CHUNK = 1 << 27  # elements per pass of the chunked whole-tensor checks
BLOCK = 1 << 20  # elements per checksum


def out_hw(H, W, K, s, p, d):
    return (H + 2 * p - d * (K - 1) - 1) // s + 1, (W + 2 * p - d * (K - 1) - 1) // s + 1


def need(nbytes):
    """Skip unless `nbytes` (what the test allocates at its peak, <= 32 GiB by construction) is free."""
    assert nbytes <= CAP, (nbytes, CAP)
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < nbytes + GIB:
        pytest.skip(f"needs {nbytes / GIB:.1f} GiB + 1 GiB of slack, {free / GIB:.1f} of {total / GIB:.1f} GiB free")


class Meter:
    """Wall time and peak device memory of one test; the peak is asserted to stay under the cap."""

    def __init__(self, name):
        self.name, self.notes = name, []

    def __enter__(self):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        self.base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()
        return self

    def note(self, text):
        self.notes.append(text)

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        wall = time.perf_counter() - self.t0
        peak = torch.cuda.max_memory_allocated() - self.base
        gc.collect()
        torch.cuda.empty_cache()
        print(f"\nSIZE-RULES {self.name}: wall {wall:.2f} s, peak {peak / GIB:.2f} GiB" +
              "".join(f"; {n}" for n in self.notes))
        if et is None:
            assert peak <= CAP, (self.name, peak)
        return False


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def guarded(shape, g, dtype=torch.float32, guard_pixels=128, scale=None, shift=None, guard_elems=None):
    """randn (* scale + shift) of `shape` (channels last) on the device as a slice of a NaN-filled allocation: >=
    guard_pixels pixels (one 128-row tile, or more where the caller's taps reach further) of NaN on each side, the
    slice 16-byte aligned.  guard_elems: the guard in elements, for a tensor that has no channel dimension."""
    numel = 1
    for s in shape:
        numel *= s
    pad = (guard_pixels * shape[-1] if guard_elems is None else guard_elems) + 64
    buf = torch.full((2 * pad + numel,), float("nan"), device=DEV, dtype=dtype)
    v = buf[pad:pad + numel].view(shape)
    flat = v.view(-1)
    for i in range(0, numel, CHUNK):  # chunked: the fp16 generator goes through an fp32 temporary
        n = min(CHUNK, numel - i)
        torch.randn(n, generator=g, device=DEV, dtype=dtype, out=flat[i:i + n])
        if scale is not None:
            flat[i:i + n].mul_(scale)
        if shift is not None:
            flat[i:i + n].add_(shift)
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + numel:]).all())
    return v


def filled(shape, dtype=torch.float32, value=float("nan")):
    return torch.full(shape, value, device=DEV, dtype=dtype)


def nonzero(w):
    return torch.where(w == 0, torch.ones_like(w), w)


def all_finite(t):
    flat = t.reshape(-1)
    return all(bool(torch.isfinite(flat[i:i + CHUNK]).all()) for i in range(0, flat.numel(), CHUNK))


def all_nan(t):
    flat = t.reshape(-1)
    return all(bool(torch.isnan(flat[i:i + CHUNK]).all()) for i in range(0, flat.numel(), CHUNK))


def checksums(t):
    """One int64 sum of the int32 words of every 2^20-element block (and of the ragged tail): a copy of the whole
    tensor's bits small enough to keep while the other form runs."""
    flat = t.reshape(-1)
    if (flat.numel() * flat.element_size()) % 4 != 0:
        flat = flat[:flat.numel() - flat.numel() % (4 // flat.element_size())]  # at most one element dropped
    words = flat.view(torch.int32)
    wpb = BLOCK * t.element_size() // 4
    full = words.numel() // wpb
    sums = []
    step = max(1, CHUNK // BLOCK)
    for b in range(0, full, step):
        nb = min(step, full - b)
        sums.append(words[b * wpb:(b + nb) * wpb].view(nb, wpb).sum(1, dtype=torch.int64))
    if words.numel() > full * wpb:
        sums.append(words[full * wpb:].sum(dtype=torch.int64).reshape(1))
    return torch.cat(sums)


def crossing_rows(row_elems, esize, total_rows):
    """The rows of a [total_rows][row_elems] tensor in which a byte offset crosses 2^31, 2^32 or 2^33, or an element
    index crosses 2^31."""
    rows = set()
    for lim in LIMITS:
        rows.add(lim // (row_elems * esize))
    rows.add((1 << 31) // row_elems)
    return sorted(r for r in rows if 0 < r < total_rows)


def plane_crossing_rows(row_elems, esize, rows, planes):
    """For a [planes][rows][row_elems] tensor (the split planes): the row, within its plane, of every crossing of
    2^31 / 2^32 / 2^33 bytes and of 2^31 / 2^32 elements counted from the allocation's base, whichever plane holds it."""
    out = set()
    for p in range(planes):
        for lim in list(LIMITS) + [esize << 31, esize << 32]:
            r = (lim - p * rows * row_elems * esize) // (row_elems * esize)
            if lim >= p * rows * row_elems * esize and 0 < r < rows:
                out.add(r)
    return sorted(out)


def merge(rows, total):
    """Row numbers -> sorted list of [r0, r1) bands holding every row and its two neighbours."""
    want = sorted({q for r in rows for q in (r - 1, r, r + 1) if 0 <= q < total})
    bands = []
    for r in want:
        if bands and bands[-1][1] == r:
            bands[-1][1] = r + 1
        else:
            bands.append([r, r + 1])
    return [tuple(b) for b in bands]


def conv_bands(N, H, W, Ci, Co, K, s, p, d, x_esize=4, y_esize=4, x_rows=()):
    """Output-row bands (n, oy0, oy1) of a conv: first rows, last rows, both sides of every crossing of the output,
    and the output rows whose taps read the input rows of every crossing of the input (x_rows: further input rows,
    numbered over all images)."""
    Ho, Wo = out_hw(H, W, K, s, p, d)
    rows = {0, N * Ho - 1}
    rows.update(crossing_rows(Wo * Co, y_esize, N * Ho))
    for gi in list(crossing_rows(W * Ci, x_esize, N * H)) + list(x_rows):
        for r in (gi - 1, gi):
            n, iy = divmod(r, H)
            rows.add(n * Ho + min(Ho - 1, max(0, (iy + p) // s)))
    out = []
    for r0, r1 in merge(rows, N * Ho):
        while r0 < r1:  # a band stays inside one image
            n, oy = divmod(r0, Ho)
            e = min(r1, (n + 1) * Ho)
            out.append((n, oy, oy + e - r0))
            r0 = e
    return out


def conv_band_ref(x, w64, band, K, s, p, d, round_x=None):
    """float64 conv (CPU, torch.nn.functional) of the output rows of `band` with the input halo that goes with them:
    -> (z [rows, Wo, Co], sum of |terms| [rows, Wo, Co])."""
    n, oy0, oy1 = band
    H = x.shape[1]
    iy0, iy1 = oy0 * s - p, (oy1 - 1) * s - p + d * (K - 1) + 1
    lo, hi = max(iy0, 0), min(iy1, H)
    xs = x[n, lo:hi]
    if round_x is not None:
        xs = xs.to(round_x)
    xs = xs.cpu().double().permute(2, 0, 1)[None]
    xs = F.pad(xs, (p, p, lo - iy0, iy1 - hi))
    z = F.conv2d(xs, w64, None, stride=s, dilation=d)[0].permute(1, 2, 0)
    mag = F.conv2d(xs.abs(), w64.abs(), None, stride=s, dilation=d)[0].permute(1, 2, 0)
    assert z.shape[0] == oy1 - oy0, (z.shape, band)
    return z, mag


def row_bands(M, row_elems_list, extra=()):
    """Bands [m0, m1) of the rows of [M][C] matrices (row_elems_list: (C, element size) of every operand and output):
    the first and last 256 rows and 256 rows on both sides of every crossing (extra: further rows)."""
    marks = {0, M} | set(extra)
    for C, esize in row_elems_list:
        for lim in LIMITS:
            marks.add(lim // (C * esize))
        marks.add((1 << 31) // C)
    bands = []
    for m in sorted(q for q in marks if 0 <= q <= M):
        lo, hi = max(0, m - 256), min(M, m + 256)
        if bands and lo <= bands[-1][1]:
            bands[-1][1] = hi
        elif hi > lo:
            bands.append([lo, hi])
    return [tuple(b) for b in bands]
