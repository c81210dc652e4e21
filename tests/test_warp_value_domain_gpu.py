"""The forward warp / fusion kernels (bev_warp.hip: the per-view warp, the fused warp+fuse kernels, k_fuse) on
non-finite, extreme and subnormal features, against the CPU oracle (oracle/bev_oracle.c, built with
-fno-fast-math, denormals kept).

Comparison, everywhere: isnan(got) == isnan(ref) elementwise and bit equality (uint32 view) wherever the
reference is not NaN.  NaN payloads are not compared; there is no tolerance.

What the cases pin:
  * poison -- ONE NaN / +Inf / -Inf in an otherwise unit-scale tensor, at a pixel chosen from oracle.taps:
    (a) read by a valid tap of view 0, (b) the same in the last view's last channel, (c) read under a tap weight
    that is exactly 0.0 (the reference multiplies a valid tap even at weight 0: 0 * Inf = NaN), (d) read by no
    cell at all but inside a 16 x 16 tile's footprint box, which the fused kernels stage into LDS (the reference
    selects 0 for an invalid tap: nothing may leak).  Each poison sits in a channel of its own, so one tensor
    carries a dozen of them; +Inf against -Inf and NaN against NaN in two views of one cell ride along.
  * torch.max's rules: NaN propagates, a view that misses a cell contributes +0 (all-negative features).
  * magnitude -- randn * 2^125 (sums over views overflow in some cells) and randn * 2^-140 (every feature
    subnormal; products of subnormals round, so the oracle runs on the scaled input itself).
  * the mean's division by V for V inside and outside the Markstein set, on those inputs and on +Inf.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("sum", "mean", "max")
GEOMS = ["warp_w2_b2_small", "warp_w3_v3", "warp_w6_degenerate", "warp_w7_tiny"]
DIV_V = [2, 3, 6, 7, 10, 16]  # 6 and 10 are outside MARKSTEIN_EXACT_V (div_rcp through double)
# (BEV_TUNE_WARP_KERNEL, WARP_POOL_KB, WARP_SPAN): the pools of test_warp_gpu.KERNEL_CASES (direct-global,
# one-view-batch and block-decomposed paths); kernel 2 with span staging off and everywhere
NHWC_CONFIGS = [(3, 0, 0), (3, 1, 0), (3, 4, 0), (3, 16, 0),
                (2, 0, 0), (2, 8, 0), (2, 16, 0), (2, 24, 0), (2, 0, 100), (2, 8, 100), (2, 16, 100), (2, 24, 100),
                (1, 0, 0)]
ENTRIES = ["per_view", "fused_nchw", "nhwc", "k_fuse"]
ENTRY_C = {"per_view": 5, "fused_nchw": 13, "nhwc": 64, "k_fuse": 5}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mismatch(got, ref):
    """Elements that break the rule: NaN exactly where the reference is NaN, the reference's bits elsewhere."""
    gn, rn = np.isnan(got), np.isnan(ref)
    return (gn != rn) | (~rn & (bits(got) != bits(ref)))


# ---- geometries -------------------------------------------------------------------------------------------------
class Geom:
    def __init__(self, name, oracle):
        from models.fusion.geometry import GeometryTransformer
        self.name = name
        if name.startswith("rig"):
            from bev_rig import rig
            self.B, self.V, self.Hf, self.Wf, self.img = 1, int(name[3:]), 34, 60, (270, 480)
            self.K, self.Rt = rig(self.V, 270, 480, 1)
            self.g = GeometryTransformer(48, 144, (-24.0, 24.0, -7.2, 7.2))
            self.seed = 500 + self.V
        else:
            d = np.load(os.path.join(GOLDEN, name + ".npz"))
            self.B, self.V, self.Hf, self.Wf = (int(d[k]) for k in ("B", "V", "Hf", "Wf"))
            self.img = (int(d["img_h"]), int(d["img_w"]))
            self.K, self.Rt = d["K"], d["Rt"]
            self.g = GeometryTransformer(int(d["bev_h"]), int(d["bev_w"]), tuple(float(x) for x in d["bounds"]))
            self.seed = 400 + int(d["seed"])
        self.Hb, self.Wb = self.g.bev_h, self.g.bev_w
        ops = [oracle.homography_operands(self.K[b, v], self.Rt[b, v]) for b in range(self.B) for v in range(self.V)]
        H = oracle.homography(np.stack([o[0] for o in ops]), np.stack([o[1] for o in ops]))
        xs, ys = oracle.bev_axes(self.Hb, self.Wb, self.g.bounds)
        # x0y0 [N,Hb,Wb,2], wts [N,Hb,Wb,4], valid [N,Hb,Wb] (bit k: tap k = nw, ne, sw, se), N = b * V + v
        self.x0y0, self.wts, self.valid = oracle.taps(H, xs, ys, self.Hf, self.Wf, self.img)
        self.oracle = oracle

    def feats(self, C, scale=None):
        f = np.random.default_rng(self.seed + C).standard_normal(size=(self.B, self.V, C, self.Hf, self.Wf),
                                                                 dtype=np.float32)
        return f if scale is None else (f * np.float32(scale)).astype(np.float32)

    def reference(self, feats):
        """(per-view maps [B,V,C,Hb,Wb], {mode: fused [B,C,Hb,Wb]}) from the oracle."""
        pv = self.oracle.geometry_forward(feats, self.K, self.Rt, self.img, self.Hb, self.Wb, self.g.bounds)
        return pv, {m: self.oracle.fuse(pv, m) for m in MODES}

    # -- which pixels the cells read, from the oracle's taps ----------------------------------------------------
    def tap_pixels(self, n, k, cells=None):
        """(cell ys, cell xs, pixel ys, pixel xs, weights) of tap k's valid reads in view n (cells: a bool mask)."""
        m = ((self.valid[n] >> k) & 1).astype(bool)
        if cells is not None:
            m &= cells
        cy, cx = np.nonzero(m)
        return cy, cx, self.x0y0[n, cy, cx, 1] + (k >> 1), self.x0y0[n, cy, cx, 0] + (k & 1), self.wts[n, cy, cx, k]

    def read_mask(self, n, cells=None):
        r = np.zeros((self.Hf, self.Wf), bool)
        for k in range(4):
            _, _, py, px, _ = self.tap_pixels(n, k, cells)
            r[py, px] = True
        return r

    def read_pixel(self, n):
        """A pixel read by a valid tap of view n with the largest weight any cell gives that view, and the cell."""
        best = None
        for k in range(4):
            cy, cx, py, px, w = self.tap_pixels(n, k)
            if len(w) and (best is None or w.max() > best[0]):
                i = int(np.argmax(w))
                best = (float(w[i]), (int(py[i]), int(px[i])), (int(cy[i]), int(cx[i])))
        return best

    def zero_weight_pixel(self):
        """(n, pixel, cell) of a valid tap whose weight is exactly 0.0, or None."""
        for n in range(self.B * self.V):
            for k in range(4):
                cy, cx, py, px, w = self.tap_pixels(n, k)
                z = np.nonzero(w == 0.0)[0]
                if len(z):
                    i = int(z[len(z) // 2])
                    return n, (int(py[i]), int(px[i])), (int(cy[i]), int(cx[i]))
        return None

    def unread_staged_pixel(self):
        """(n, pixel) of a view's pixel that NO cell reads as a valid tap and that lies inside the footprint box
        (bounding box of the valid taps) of some 16 x 16 BEV tile, or None."""
        for n in range(self.B * self.V):
            read = self.read_mask(n)
            for ty in range(0, self.Hb, 16):
                for tx in range(0, self.Wb, 16):
                    cells = np.zeros((self.Hb, self.Wb), bool)
                    cells[ty:ty + 16, tx:tx + 16] = True
                    ys, xs = np.nonzero(self.read_mask(n, cells))
                    if not len(ys):
                        continue
                    box = np.zeros_like(read)
                    box[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = True
                    py, px = np.nonzero(box & ~read)
                    if len(py):
                        i = len(py) // 2
                        return n, (int(py[i]), int(px[i]))
        return None

    def common_cell(self, first_view=None):
        """(cell, (n_i, pixel_i), (n_j, pixel_j)): a cell of frame 0 that two views i < j both read through a valid
        tap of nonzero weight (i == first_view if given), or None."""
        for i in range(self.V) if first_view is None else (first_view,):
            for j in range(i + 1, self.V):
                both = (self.valid[i] == 15) & (self.valid[j] == 15)
                both &= (self.wts[i, ..., 0] > 0) & (self.wts[j, ..., 0] > 0)
                cy, cx = np.nonzero(both)
                if len(cy):
                    y, x = int(cy[len(cy) // 2]), int(cx[len(cy) // 2])
                    pi = (int(self.x0y0[i, y, x, 1]), int(self.x0y0[i, y, x, 0]))
                    pj = (int(self.x0y0[j, y, x, 1]), int(self.x0y0[j, y, x, 0]))
                    return (y, x), (i, pi), (j, pj)
        return None


_GEOM = {}


def geom(name, oracle):
    if name not in _GEOM:
        _GEOM.clear()
        _CASES.clear()
        _GEOM[name] = Geom(name, oracle)
    return _GEOM[name]


# ---- running the kernels ----------------------------------------------------------------------------------------
def _nhwc(feats_np):
    ft = torch.from_numpy(feats_np).to(DEV)
    return ft.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)  # channels-last storage


def run_entry(entry, G, feats, per_view, modes=MODES):
    """-> [(label, got, which reference)]: every launch of one forward entry on `feats`."""
    import bev_native as nat
    from models.fusion.fusion import SimpleFusion
    Kt, Rtt = torch.from_numpy(G.K).to(DEV), torch.from_numpy(G.Rt).to(DEV)
    out = []
    with torch.no_grad():
        if entry == "per_view":
            got = G.g(torch.from_numpy(feats).to(DEV), Kt, Rtt, img_size=G.img)
            out.append(("per_view", got.cpu().numpy(), "per_view"))
        elif entry == "fused_nchw":
            ft = torch.from_numpy(feats).to(DEV)
            for m in modes:
                out.append((f"fused_nchw/{m}", G.g.forward_fused(ft, Kt, Rtt, G.img, m).cpu().numpy(), m))
        elif entry == "nhwc":
            f = _nhwc(feats)
            for kid, pool, span in NHWC_CONFIGS:
                with nat.tuned(WARP_KERNEL=kid, WARP_POOL_KB=pool, WARP_SPAN=span):
                    for m in modes:
                        got = G.g.forward_fused(f, Kt, Rtt, G.img, m).cpu().numpy()
                        out.append((f"nhwc k{kid} pool{pool} span{span}/{m}", got, m))
        else:
            pv = torch.from_numpy(per_view).to(DEV)
            for m in modes:
                out.append((f"k_fuse/{m}", SimpleFusion(m)(pv).cpu().numpy(), m))
    return out


def check(entry, G, feats, per_view, refs, what, modes=MODES):
    bad = []
    for label, got, which in run_entry(entry, G, feats, per_view, modes):
        ref = per_view if which == "per_view" else refs[which]
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        mm = mismatch(got, ref)
        if mm.any():
            ax = got.ndim - 3  # the channel axis of [B,(V,)C,Hb,Wb]
            per_c = mm.sum(axis=tuple(a for a in range(got.ndim) if a != ax))
            i = tuple(int(x[0]) for x in np.nonzero(mm))
            bad.append((label, int(mm.sum()), {int(c): int(k) for c, k in enumerate(per_c) if k}, i,
                        float(got[i]), float(ref[i])))
    assert not bad, (what, bad[:6], len(bad))


# ---- 1. poison --------------------------------------------------------------------------------------------------
_CASES = {}
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def poison_rounds(G, C):
    """Feature tensors [B,V,C,Hf,Wf] (unit-scale randn) each carrying one poison item per channel, with the
    oracle's outputs and the unpoisoned outputs: [(feats, items, per_view, refs)], clean (per_view, refs).
    An item: (kind, value name, channel, [(b, v, y, x, value)], witness cell or None).  The last channel of
    round r holds placement (b) with the r-th value; the other channels take the remaining items in turn."""
    key = ("poison", G.name, C)
    if key in _CASES:
        return _CASES[key]
    V = G.V
    plain = []
    _, pa, cell_a = G.read_pixel(0)
    for vn in VALUES:
        plain.append(("a", vn, [(0, 0) + pa + (VALUES[vn],)], cell_a))
    zw = G.zero_weight_pixel()
    if zw is not None:
        n, p, cell = zw
        for vn in VALUES:
            plain.append(("c", vn, [(n // V, n % V) + p + (VALUES[vn],)], (n // V,) + cell))
    un = G.unread_staged_pixel()
    if un is not None:
        n, p = un
        for vn in VALUES:
            plain.append(("d", vn, [(n // V, n % V) + p + (VALUES[vn],)], None))
    cc = G.common_cell()
    if cc is not None:
        cell, (i, pi), (j, pj) = cc
        plain.append(("inf_pair", "+inf/-inf", [(0, i) + pi + (np.inf,), (0, j) + pj + (-np.inf,)], cell))
    cc0 = G.common_cell(first_view=0) or cc
    if cc0 is not None:
        cell, (i, pi), (j, pj) = cc0
        plain.append(("nan_pair", "nan/nan", [(0, i) + pi + (np.nan,), (0, j) + pj + (np.nan,)], cell))
    n_last = G.B * V - 1
    _, pb, cell_b = G.read_pixel(n_last)
    last = [("b", vn, [(G.B - 1, V - 1) + pb + (VALUES[vn],)], cell_b) for vn in VALUES]
    base = G.feats(C)
    clean = G.reference(base)
    queue = list(plain)
    rounds = []
    for r in range(max(3, -(-len(plain) // (C - 1)))):
        f, items = base.copy(), []
        for c in range(C - 1):
            if not queue:
                break
            kind, vn, places, cell = queue.pop(0)
            items.append((kind, vn, c, places, cell))
        if r < 3:
            kind, vn, places, cell = last[r]
            items.append((kind, vn, C - 1, places, cell))
        for kind, vn, c, places, cell in items:
            for b, v, y, x, val in places:
                f[b, v, c, y, x] = val
        rounds.append((f, items) + G.reference(f))
    _CASES[key] = (rounds, clean, {"c": zw is not None, "d": un is not None, "pair": cc is not None})
    return _CASES[key]


def assert_poison_preconditions(G, rounds, clean):
    """From the reference alone: (a)-(c) its non-finite set in the item's channel is neither empty nor everything
    (per view and in sum / mean; in max too unless the value is -Inf, which any other view's sample or a missing
    view's +0 outbids); (c) with +-Inf: NaN at the witness cell (0 * Inf); (d) the channel is entirely finite and
    bit-equal to the unpoisoned reference; the pairs: NaN at the common cell in sum (Inf - Inf) / in max."""
    clean_pv, clean_refs = clean
    for f, items, pv, refs in rounds:
        for kind, vn, c, places, cell in items:
            what = (G.name, kind, vn, c)
            if kind in ("a", "b", "c"):
                for m in MODES:
                    nf = ~np.isfinite(refs[m][:, c])
                    if m != "max" or vn != "-inf":
                        assert nf.any() and not nf.all(), what + (m,)
                nf = ~np.isfinite(pv[:, :, c])
                assert nf.any() and not nf.all(), what
            if kind == "c" and vn != "nan":
                b, y, x = cell
                assert all(np.isnan(refs[m][b, c, y, x]) for m in MODES), what
            if kind == "d":
                assert np.isfinite(pv[:, :, c]).all(), what
                assert np.array_equal(bits(pv[:, :, c]), bits(clean_pv[:, :, c])), what
                for m in MODES:
                    assert np.array_equal(bits(refs[m][:, c]), bits(clean_refs[m][:, c])), what + (m,)
            if kind == "inf_pair":
                assert np.isnan(refs["sum"][0, c, cell[0], cell[1]]) and np.isnan(refs["sum"][:, c]).sum() >= 1, what
            if kind == "nan_pair":
                assert np.isnan(refs["max"][0, c, cell[0], cell[1]]), what


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", GEOMS)
def test_poison(name, entry, oracle):
    """One non-finite value per channel, placed from the oracle's taps (module docstring), through every forward
    entry: the per-view warp (NCHW, C 5), forward_fused on NCHW C 13 (generic-stride staging, a partial chunk) and
    on channels-last C 64 under every kernel / LDS pool / span-staging choice, and k_fuse on the oracle's own
    per-view maps; sum, mean and max."""
    G = geom(name, oracle)
    C = ENTRY_C[entry]
    rounds, clean, have = poison_rounds(G, C)
    kinds = {it[0] for r in rounds for it in r[1]}
    assert {"a", "b"} <= kinds
    assert_poison_preconditions(G, rounds, clean)
    for r, (f, items, pv, refs) in enumerate(rounds):
        check(entry, G, f, pv, refs, (name, entry, "round", r, [(it[0], it[1], it[2]) for it in items]))


@pytest.mark.parametrize("name", GEOMS)
def test_poison_placements_exist(name, oracle):
    """The geometry offers the placements that test_poison can only take where they exist: a valid tap of weight
    exactly 0.0 (c), an unread pixel inside a tile's footprint box (d), a cell two views share.  A geometry
    without one skips here, with the reason, instead of passing silently there."""
    G = geom(name, oracle)
    _, _, have = poison_rounds(G, 5)
    missing = [k for k, v in have.items() if not v]
    if missing:
        pytest.skip(f"{name}: the oracle's taps hold no placement {missing}")


# ---- torch.max: NaN propagates, a view that misses a cell contributes +0 -----------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", GEOMS)
def test_max_of_all_negative_features(name, entry, oracle):
    """Every feature negative: the max over views is +0 (bits 0) in every cell that some view misses (that view's
    sample is +0) and negative in every cell that all views read through four valid taps."""
    G = geom(name, oracle)
    C = ENTRY_C[entry]
    key = ("neg", name, C)
    if key not in _CASES:
        f = (-np.abs(G.feats(C)) - np.float32(0.5)).astype(np.float32)
        _CASES[key] = (f,) + G.reference(f)
    f, pv, refs = _CASES[key]
    valid = G.valid.reshape(G.B, G.V, G.Hb, G.Wb)
    missed = (valid == 0).any(axis=1)[:, None].repeat(C, axis=1)
    seen = (valid == 15).all(axis=1)[:, None].repeat(C, axis=1)
    assert missed.any() and (bits(refs["max"])[missed] == 0).all()
    assert (refs["max"][seen] < 0).all()
    if name in ("warp_w2_b2_small", "warp_w3_v3"):
        assert seen.any(), "no cell seen by every view"
    check(entry, G, f, pv, refs, (name, entry, "all-negative"), modes=("max",))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", GEOMS)
def test_max_keeps_the_first_of_a_signed_zero_tie(name, entry, oracle):
    """Every feature -0.0: a view's sample is -0.0 where all four taps are valid and +0.0 where it misses the cell.
    torch.max replaces only on `>`, so the FIRST view decides a -0 / +0 tie: -0.0 where view 0 reads the cell (later
    views that miss it contribute +0, which is not greater), +0.0 where view 0 misses it.  The sum is +0 everywhere
    (it starts from +0)."""
    G = geom(name, oracle)
    C = ENTRY_C[entry]
    key = ("negzero", name, C)
    if key not in _CASES:
        f = np.full((G.B, G.V, C, G.Hf, G.Wf), -0.0, np.float32)
        _CASES[key] = (f,) + G.reference(f)
    f, pv, refs = _CASES[key]
    valid = G.valid.reshape(G.B, G.V, G.Hb, G.Wb)
    first_reads = (valid[:, 0] == 15)[:, None].repeat(C, axis=1)
    first_misses = (valid[:, 0] == 0)[:, None].repeat(C, axis=1)
    later_misses = (valid[:, 1:] == 0).any(axis=1)[:, None].repeat(C, axis=1)
    assert (first_reads & later_misses).any() and first_misses.any()
    assert (bits(refs["max"])[first_reads] == 0x80000000).all() and (bits(refs["max"])[first_misses] == 0).all()
    assert (bits(refs["sum"]) == 0).all() and (bits(refs["mean"]) == 0).all()
    check(entry, G, f, pv, refs, (name, entry, "all -0.0"))


# ---- 2. magnitude -----------------------------------------------------------------------------------------------
def magnitude_case(G, C, kind):
    key = ("mag", G.name, C, kind)
    if key not in _CASES:
        f = G.feats(C, 2.0 ** 125 if kind == "huge" else 2.0 ** -140)
        pv, refs = G.reference(f)
        if kind == "huge":
            assert np.isfinite(f).all()
            assert np.isinf(refs["sum"]).any() and np.isfinite(refs["sum"]).any() and not np.isnan(refs["sum"]).any()
        else:
            tiny = np.float32(2.0 ** -126)
            assert (np.abs(f) < tiny).all() and (f != 0).any()
            for r in (pv, refs["sum"], refs["mean"], refs["max"]):
                assert ((r != 0) & (np.abs(r) < tiny)).any()
        _CASES[key] = (f, pv, refs)
    return _CASES[key]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,kind", [("warp_w2_b2_small", "huge"), ("warp_w2_b2_small", "subnormal"),
                                       ("warp_w6_degenerate", "subnormal")])
def test_magnitude(name, kind, entry, oracle):
    """randn * 2^125: every feature finite, the reference's sum over views is +-Inf in some cells and finite in
    others (the 7 views of warp_w2_b2_small; the 4 barely overlapping views of the degenerate rig never overflow,
    and a larger scale would make the features themselves infinite).  randn * 2^-140: every feature subnormal,
    the reference's outputs hold nonzero subnormals.  Each compared with the oracle run on the scaled input
    itself."""
    G = geom(name, oracle)
    f, pv, refs = magnitude_case(G, ENTRY_C[entry], kind)
    check(entry, G, f, pv, refs, (name, entry, kind))


# ---- 3. the mean's division by V --------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["fused_nchw", "nhwc", "k_fuse"])
@pytest.mark.parametrize("V", DIV_V)
def test_mean_division(V, entry, oracle):
    """mean = sum / f32(V) as a true IEEE division on sums that are +-Inf, NaN (Inf - Inf cannot arise here, but
    0 * Inf does), near FLT_MAX and subnormal: V cameras of the Appendix-B rig, 34 x 60 maps, 48 x 144 BEV, every
    fused kernel and k_fuse, mean mode."""
    G = geom(f"rig{V}", oracle)
    C = ENTRY_C[entry]
    for kind in ("huge", "subnormal", "+inf"):
        key = ("div", V, C, kind)
        if key not in _CASES:
            if kind == "+inf":
                f = G.feats(C)
                _, p, cell = G.read_pixel(V // 2)
                f[0, V // 2, C // 2, p[0], p[1]] = np.inf
                pv, refs = G.reference(f)
                m = refs["mean"][0, C // 2]
                assert np.isinf(m).any() and np.isfinite(m).any()
            else:
                f = G.feats(C, 2.0 ** 125 if kind == "huge" else 2.0 ** -140)
                pv, refs = G.reference(f)
                m = refs["mean"]
                if kind == "huge":
                    assert np.isfinite(f).all() and np.isfinite(m).any()
                    assert (np.abs(refs["sum"]) > np.float32(2.0 ** 127)).any()  # sums near / beyond FLT_MAX
                else:
                    assert ((m != 0) & (np.abs(m) < np.float32(2.0 ** -126))).any()
            _CASES[key] = (f, pv, refs)
        f, pv, refs = _CASES[key]
        check(entry, G, f, pv, refs, ("rig", V, entry, kind), modes=("mean",))
