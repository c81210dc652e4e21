// bev_image.hip -- camera-image ingest for gfx950: 8-bit RGB (HWC, what PIL decodes) ->
// normalised fp32 planes (NCHW, what the backbone stem reads).
//
// Replaces the tail of the reference's per-image transform pipeline
// (data/transforms.py:12-19): T.ToTensor() (uint8 HWC -> float CHW, / 255) followed by
// T.Normalize(mean, std) ((x - mean[c]) / std[c]), applied per camera image in the
// DataLoader workers (data/wildtrack_loader.py:368-374).  Here the decoded, resized, jittered
// 8-bit images cross PCIe (1/4 of the fp32 bytes) and this kernel writes the [N, 3, H, W]
// input the stem reads.  Arithmetic is torch's, op for op (float(u8) / 255.0f, then
// - mean, then / std, each IEEE-rounded; -ffp-contract=off), so the output is bit-identical
// to the reference's CPU transform.
//
// Layout: one thread = 4 consecutive pixels of one image (12 source bytes = 3 dwords,
// one float4 per output plane); HBM-bound (3 B read + 12 B written per pixel).
//
// bev_image_resize_normalize_u8_f32 puts T.Resize((H, W)) (transforms.py:13, torchvision's PIL path:
// img.resize((W, H), Image.BILINEAR)) in front of that tail, in the same launch, for frames that
// arrive at their native size.  Pillow's resize (ImagingResample, 8 bits per channel) is integer
// arithmetic on 22-bit fixed-point coefficients: a horizontal pass to a uint8 intermediate, then a
// vertical pass over it, each  clip8((2^21 + sum src * k) >> 22).  The coefficients are computed on the
// host in double exactly as Pillow computes them (bev_image_resize_plan) and copied to the device once
// per geometry, so the kernel repeats Pillow's integer sums and the output is bit-identical to
// Normalize(ToTensor(Resize(img))).
//
// Layout of k_img_resize_norm: one 256-thread workgroup = a tile of TH x 64 output pixels of one image
// (TH = 16, 8, 4, 2 or 1: the largest whose intermediate fits RS_INTER_BYTES of LDS).  Phase 1: the
// horizontal pass for the R source rows the tile's vertical taps cover (about scale * TH + ksize rows;
// neighbouring tiles recompute the overlap), one lane per intermediate pixel (consecutive lanes =
// consecutive columns of one row).  A lane loads its tap window from the source as aligned dwords and
// realigns them in registers (src may start at any byte), 4 taps = 12 bytes at a time; geometries whose
// windows have at most 4, 8 or 12 taps (ksize_x <= 5, 9, 13: every downscale up to 5.5x) run a kernel
// instance with that round unrolled, a row's loads issued together and the coefficients in registers.
// Measured against loading the window byte by byte and against staging the tile's source row segments
// in LDS with coalesced dword loads first: both lost.  The intermediate goes to LDS as
// one dword per pixel (r | g << 8 | b << 16), never to HBM.  Phase 2: the vertical pass, one lane per
// 4 consecutive output pixels (one ds_read_b128 per tap), then norm1 and one float4 per plane,
// non-temporal, when W % 4 == 0 and out is 16-B aligned (scalar stores otherwise).  HBM traffic per
// image: 3 * Hs * Ws bytes read (+ the tiles' row overlap, which L2 serves) and 12 * H * W written.
//
// bev_image_resize_u8 + bev_image_jitter_normalize_u8_f32 put the step between the two on the device as well:
// T.RandomApply([T.ColorJitter(0.2, 0.2, 0.2, 0.05)], p=0.5) (transforms.py:14).  The resize kernel's second epilogue
// stores the resized uint8 frame; the jitter kernels apply each frame's drawn op list (a record of eight words, drawn
// on the host in the reference's order) with the per-pixel functions of bev_image_jitter.h -- Pillow's ImagingBlend
// and RGB <-> HSV conversions, type for type -- then norm1.  Contrast needs the mean of L over the frame as its
// predecessors leave it: pass 1 sums L per frame (exact integers, one 64-bit atomic per workgroup), pass 2 applies the
// whole list.  Per output pixel that adds 3 B written and 3 + 3 B read to the 12 B written (DESIGN.md §4 has the times).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/bev_mi355x.h"
#include "bev_image_jitter.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Norm {
    float mean[3], std[3];
};

__device__ __forceinline__ float norm1(unsigned v, float m, float s) {
    float x = (float)v / 255.0f;
    x = x - m;
    return x / s;
}

// vector path: H*W % 4 == 0, src 4-B aligned, out 16-B aligned
__global__ void k_img_norm_v4(const uint32_t *__restrict__ src, int64_t quads_per_img, int64_t total, Norm nm,
                              float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t n = t / quads_per_img, q = t - n * quads_per_img;
    const uint32_t w0 = src[3 * t], w1 = src[3 * t + 1], w2 = src[3 * t + 2];
    // bytes b0..b11 = r0 g0 b0 r1 g1 b1 r2 g2 b2 r3 g3 b3
    const unsigned b[12] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, w0 >> 24,
                            w1 & 255u, (w1 >> 8) & 255u, (w1 >> 16) & 255u, w1 >> 24,
                            w2 & 255u, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
    const int64_t plane = 4 * quads_per_img;
    f32x4 *o = (f32x4 *)(out + n * 3 * plane) + q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = nm.mean[c], s = nm.std[c];
        const f32x4 v = {norm1(b[c], m, s), norm1(b[3 + c], m, s), norm1(b[6 + c], m, s), norm1(b[9 + c], m, s)};
        __builtin_nontemporal_store(v, o + c * (plane / 4));
    }
}

__global__ void k_img_norm_scalar(const uint8_t *__restrict__ src, int64_t hw, int64_t total, Norm nm,
                                  float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // pixel
    if (t >= total) return;
    const int64_t n = t / hw, p = t - n * hw;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(n * 3 + c) * hw + p] = norm1(src[3 * t + c], nm.mean[c], nm.std[c]);
}

// ---- Resize (Pillow BILINEAR) + ToTensor + Normalize ----------------------------------------------------
constexpr int RS_TW = 64;              // output columns per tile
constexpr int RS_MAX_KSIZE = 35;       // taps per output pixel and axis at the downscale limit (17x)
constexpr int RS_MAX_SIZE = 1 << 24;   // rows / columns of either image
constexpr int RS_INTER_BYTES = 40960;  // LDS for the uint8 intermediate of one tile

struct RsAxis {
    double scale, support, ss;
    int ksize;
};

// Pillow's precompute_coeffs prologue for one axis; false for a geometry the kernel does not take.
bool rs_axis(int in_size, int out_size, RsAxis *a) {
    if (in_size <= 0 || out_size <= 0 || in_size > RS_MAX_SIZE || out_size > RS_MAX_SIZE) return false;
    a->scale = (double)((float)in_size - 0.0f) / out_size;
    const double filterscale = a->scale < 1.0 ? 1.0 : a->scale;
    a->support = 1.0 * filterscale;
    a->ksize = (int)ceil(a->support) * 2 + 1;
    a->ss = 1.0 / filterscale;
    return a->ksize <= RS_MAX_KSIZE;  // in_size <= 17 * out_size
}

double rs_triangle(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// bounds [out_size][2] = (xmin, xmax), coeffs [out_size][ksize] (zero past xmax)
void rs_fill_axis(int in_size, int out_size, const RsAxis &a, int32_t *bounds, int32_t *coeffs) {
    double w[RS_MAX_KSIZE];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * a.scale;
        int xmin = (int)(center - a.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + a.support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = rs_triangle((x + xmin - center + 0.5) * a.ss);
            ww += w[x];
        }
        int32_t *k = coeffs + (int64_t)xx * a.ksize;
        for (int x = 0; x < a.ksize; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << 22)) : (int32_t)(0.5 + v * (1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

__device__ __forceinline__ unsigned rs_clip8(int acc) {
    const int v = acc >> 22;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// 4 taps = 12 bytes (r g b of 4 source pixels) of the byte stream that starts `sh` bytes into dword d[0]
__device__ __forceinline__ void rs_taps4(const uint32_t *d, int sh, const int *kk, int &a0, int &a1, int &a2) {
    const int s8 = 8 * sh;
    const uint32_t w0 = (uint32_t)((((uint64_t)d[1] << 32) | d[0]) >> s8);  // r0 g0 b0 r1
    const uint32_t w1 = (uint32_t)((((uint64_t)d[2] << 32) | d[1]) >> s8);  // g1 b1 r2 g2
    const uint32_t w2 = (uint32_t)((((uint64_t)d[3] << 32) | d[2]) >> s8);  // b2 r3 g3 b3
    a0 += (int)(w0 & 255u) * kk[0] + (int)(w0 >> 24) * kk[1] + (int)((w1 >> 16) & 255u) * kk[2] +
          (int)((w2 >> 8) & 255u) * kk[3];
    a1 += (int)((w0 >> 8) & 255u) * kk[0] + (int)(w1 & 255u) * kk[1] + (int)(w1 >> 24) * kk[2] +
          (int)((w2 >> 16) & 255u) * kk[3];
    a2 += (int)((w0 >> 16) & 255u) * kk[0] + (int)((w1 >> 8) & 255u) * kk[1] + (int)(w2 & 255u) * kk[2] +
          (int)(w2 >> 24) * kk[3];
}

// Horizontal pass of one lane, unrolled: column tx = tid % 64 of the intermediate rows tid / 64, + 4, ... < R.  The lane
// reads its tap window as aligned dwords (`base` = the source rounded down to 4 B, boff0 = the byte offset from it
// of the window in the tile's first source row) and realigns them in registers; taps come in groups of 4 (12 bytes,
// 3 realigned dwords), a tap past the window has coefficient 0, and a dword past last_dw (the one that holds the
// batch's last byte) is never loaded.  NG groups cover every window of the geometry, so the 3 NG + 1 loads of a
// row are issued together and the coefficients stay in registers.
template <int NG>
__device__ __forceinline__ void rs_hpass(const uint32_t *__restrict__ base, int64_t boff0, int64_t row_bytes,
                                         int64_t last_dw, const int32_t *k, int xmax, int R, bool live,
                                         uint32_t *inter) {
    const int tid = threadIdx.x;
    int kr[4 * NG];
#pragma unroll
    for (int j = 0; j < 4 * NG; ++j) kr[j] = (live && j < xmax) ? k[j] : 0;
    for (int r = tid / RS_TW; r < R; r += 256 / RS_TW) {
        uint32_t px = 0;
        if (live) {
            const int64_t boff = boff0 + r * row_bytes;
            const int64_t j0 = boff >> 2;
            const int sh = (int)(boff & 3);
            const int lim = (int)min(last_dw - j0, (int64_t)(3 * NG));
            uint32_t d[3 * NG + 1];
#pragma unroll
            for (int j = 0; j < 3 * NG + 1; ++j) d[j] = base[j0 + min(j, lim)];
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma unroll
            for (int g = 0; g < NG; ++g) rs_taps4(d + 3 * g, sh, kr + 4 * g, a0, a1, a2);
            px = rs_clip8(a0) | (rs_clip8(a1) << 8) | (rs_clip8(a2) << 16);
        }
        inter[r * RS_TW + tid % RS_TW] = px;
    }
}

// dynamic LDS: inter [rcap][64] dwords | x coeffs [64][ksx] | y coeffs [TH][ksy] | x bounds [64][2] | y bounds [TH][2]
// NG = 1, 2, 3: every horizontal window has at most 4 NG taps (ksize_x <= 4 NG + 1); NG = 0: any window
// U8: the epilogue stores the resized frame itself, [N][H][W][3] uint8 (out_v: uint8; vec: W % 4 == 0 and out 4-B aligned,
// a lane's 4 pixels = 3 dwords), for the jitter that follows; otherwise norm1 and the fp32 planes (out_v: float)
template <int NG, bool U8>
__global__ __launch_bounds__(256) void k_img_resize_norm(const uint8_t *__restrict__ src, int Hs, int Ws, int H, int W,
                                                         const int32_t *__restrict__ xb, const int32_t *__restrict__ xk,
                                                         const int32_t *__restrict__ yb, const int32_t *__restrict__ yk,
                                                         int ksx, int ksy, int TH, int rcap, int tiles_x, int tiles_y,
                                                         int64_t last_dw, Norm nm, void *__restrict__ out_v, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];
    uint32_t *inter = rs_lds;
    int32_t *sxk = (int32_t *)(inter + rcap * RS_TW);
    int32_t *syk = sxk + RS_TW * ksx;
    int32_t *sxb = syk + TH * ksy;
    int32_t *syb = sxb + 2 * RS_TW;
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int x0 = (b % tiles_x) * RS_TW;
    b /= tiles_x;
    const int y0 = (b % tiles_y) * TH;
    const int n = b / tiles_y;
    const int tw = min(RS_TW, W - x0), th = min(TH, H - y0);

    // the tile's rows of the plan; windows clamped to the source so that no plan can make a load leave it
    for (int i = tid; i < tw; i += 256) {
        const int lo = min(max(xb[2 * (x0 + i)], 0), Ws - 1);
        sxb[2 * i] = lo;
        sxb[2 * i + 1] = max(min(min(xb[2 * (x0 + i) + 1], NG > 0 ? min(ksx, 4 * NG) : ksx), Ws - lo), 0);
    }
    for (int i = tid; i < th; i += 256) {
        const int lo = min(max(yb[2 * (y0 + i)], 0), Hs - 1);
        syb[2 * i] = lo;
        syb[2 * i + 1] = max(min(min(yb[2 * (y0 + i) + 1], ksy), Hs - lo), 0);
    }
    for (int i = tid; i < tw * ksx; i += 256) sxk[i] = xk[(int64_t)x0 * ksx + i];
    for (int i = tid; i < th * ksy; i += 256) syk[i] = yk[(int64_t)y0 * ksy + i];
    __syncthreads();

    // source rows [r0, r0 + R): from the first tap of the tile's first row to the last tap of its last row
    const int r0 = syb[0];
    const int R = max(min(syb[2 * (th - 1)] + syb[2 * (th - 1) + 1] - r0, rcap), 0);

    // horizontal pass -> uint8 intermediate in LDS, one dword per pixel.  The source is read as dwords from its 4-B
    // aligned base: byte (src & 3) + j of that stream is source byte j.
    const uint32_t *base = (const uint32_t *)((uintptr_t)src & ~(uintptr_t)3);
    const int64_t img_off = (int64_t)((uintptr_t)src & 3) + (int64_t)n * Hs * Ws * 3;
    if constexpr (NG > 0) {
        const int tx = tid % RS_TW;
        const bool live = tx < tw;
        const int xmin = live ? sxb[2 * tx] : 0, xmax = live ? sxb[2 * tx + 1] : 0;
        rs_hpass<NG>(base, img_off + ((int64_t)r0 * Ws + xmin) * 3, (int64_t)Ws * 3, last_dw, sxk + tx * ksx, xmax, R,
                     live, inter);
    } else {
        for (int i = tid; i < R * RS_TW; i += 256) {
            const int r = i / RS_TW, tx = i % RS_TW;
            uint32_t px = 0;
            if (tx < tw) {
                const int xmin = sxb[2 * tx], xmax = sxb[2 * tx + 1];
                const int64_t boff = img_off + ((int64_t)(r0 + r) * Ws + xmin) * 3;
                const int64_t j0 = boff >> 2;
                const int sh = (int)(boff & 3);
                const int32_t *k = sxk + tx * ksx;
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                for (int t = 0; t < xmax; t += 4) {  // 4 taps per round; taps past the window have coefficient 0
                    uint32_t d[4];
                    int kk[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        d[j] = base[min(j0 + 3 * (t / 4) + j, last_dw)];
                        kk[j] = t + j < xmax ? k[t + j] : 0;
                    }
                    rs_taps4(d, sh, kk, a0, a1, a2);
                }
                px = rs_clip8(a0) | (rs_clip8(a1) << 8) | (rs_clip8(a2) << 16);
            }
            inter[i] = px;
        }
    }
    __syncthreads();

    // vertical pass out of LDS, normalise, store the three planes
    const int64_t plane = (int64_t)H * W;
    float *o = (float *)out_v + (int64_t)n * 3 * plane;
    for (int q = tid; q < th * (RS_TW / 4); q += 256) {
        const int ty = q / (RS_TW / 4), qx = q % (RS_TW / 4);
        if (4 * qx >= tw) continue;
        const int ymin = max(syb[2 * ty] - r0, 0);
        const int ymax = min(syb[2 * ty + 1], R - ymin);
        const int32_t *k = syk + ty * ksy;
        int acc[4][3];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[p][c] = 1 << 21;
        for (int t = 0; t < ymax; ++t) {
            const uint4 v = *(const uint4 *)(inter + (ymin + t) * RS_TW + 4 * qx);
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
            const int kk = k[t];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[p][c] += (int)((w4[p] >> (8 * c)) & 255u) * kk;
        }
        const int64_t at = (int64_t)(y0 + ty) * W + x0 + 4 * qx;
        if constexpr (U8) {
            uint8_t *o8 = (uint8_t *)out_v + ((int64_t)n * plane + at) * 3;
            if (vec) {
                uint32_t w[3] = {0, 0, 0};
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) w[(3 * p + c) / 4] |= rs_clip8(acc[p][c]) << (8 * ((3 * p + c) % 4));
#pragma unroll
                for (int j = 0; j < 3; ++j) ((uint32_t *)o8)[j] = w[j];
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (4 * qx + p >= tw) break;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o8[3 * p + c] = (uint8_t)rs_clip8(acc[p][c]);
                }
            }
        } else if (vec) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float m = nm.mean[c], s = nm.std[c];
                const f32x4 f = {norm1(rs_clip8(acc[0][c]), m, s), norm1(rs_clip8(acc[1][c]), m, s),
                                 norm1(rs_clip8(acc[2][c]), m, s), norm1(rs_clip8(acc[3][c]), m, s)};
                __builtin_nontemporal_store(f, (f32x4 *)(o + c * plane + at));
            }
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (4 * qx + p >= tw) break;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane + at + p] = norm1(rs_clip8(acc[p][c]), nm.mean[c], nm.std[c]);
            }
        }
    }
}

// ---- ColorJitter + ToTensor + Normalize ------------------------------------------------------------------
// A workgroup of 256 lanes takes JIT_PX(VEC) consecutive pixels of ONE frame (grid = blocks per frame x N), so the
// frame's record is wave-uniform: s_loads, and the op-order branches of bev_jitter::apply do not diverge.  VEC: a lane
// = 4 consecutive pixels, as k_img_norm_v4 (H*W % 4 == 0, src 4-B aligned, out 16-B aligned); otherwise one pixel.
namespace jit = bev_jitter;

template <bool VEC>
constexpr int JIT_PX = VEC ? 1024 : 256;

// a lane's pixels of frame n: index i0 .. i0 + NP - 1 < hw (false: none)
template <bool VEC>
__device__ __forceinline__ bool jit_load(const uint8_t *__restrict__ src, int64_t n, int blk, int64_t hw,
                                         unsigned (&c)[VEC ? 4 : 1][3], int64_t &i0) {
    i0 = (int64_t)blk * JIT_PX<VEC> + (int64_t)threadIdx.x * (VEC ? 4 : 1);
    if (i0 >= hw) return false;
    if constexpr (VEC) {
        const uint32_t *s = (const uint32_t *)src + (n * hw + i0) / 4 * 3;
        const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
        const unsigned b[12] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, w0 >> 24,
                                w1 & 255u, (w1 >> 8) & 255u, (w1 >> 16) & 255u, w1 >> 24,
                                w2 & 255u, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[p][k] = b[3 * p + k];
    } else {
        const uint8_t *s = src + (n * hw + i0) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[0][k] = s[k];
    }
    return true;
}

// Pass 1: sum of L over each frame whose list holds contrast, of the frame as its predecessors in the list leave it.
// Integer sums: one 64-bit atomic add per workgroup gives the same total in any order.
template <bool VEC>
__global__ __launch_bounds__(256) void k_img_jitter_sum(const uint8_t *__restrict__ src, int64_t hw, int bpf,
                                                        const uint32_t *__restrict__ params,
                                                        unsigned long long *__restrict__ sums) {
    __shared__ unsigned wave_sum[4];
    const int n = blockIdx.x / bpf, blk = blockIdx.x - n * bpf;
    const jit::Rec j = jit::load_rec(params + (int64_t)n * jit::REC_WORDS);
    if (!jit::has_contrast(j.ops)) return;  // the whole workgroup: the record is the frame's
    constexpr int NP = VEC ? 4 : 1;
    unsigned c[NP][3];
    int64_t i0;
    unsigned sum = 0;
    if (jit_load<VEC>(src, n, blk, hw, c, i0)) {
        jit::apply<NP, true>(j, 0, c);
#pragma unroll
        for (int p = 0; p < NP; ++p) sum += jit::luma(c[p][0], c[p][1], c[p][2]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(sums + n, (unsigned long long)wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3]);
}

// Pass 2: the whole list (contrast's mean from pass 1), norm1, the three planes.
template <bool VEC>
__global__ __launch_bounds__(256) void k_img_jitter_norm(const uint8_t *__restrict__ src, int64_t hw, int bpf,
                                                         const uint32_t *__restrict__ params,
                                                         const unsigned long long *__restrict__ sums, Norm nm,
                                                         float *__restrict__ out) {
    const int n = blockIdx.x / bpf, blk = blockIdx.x - n * bpf;
    const jit::Rec j = jit::load_rec(params + (int64_t)n * jit::REC_WORDS);
    constexpr int NP = VEC ? 4 : 1;
    unsigned c[NP][3];
    int64_t i0;
    if (!jit_load<VEC>(src, n, blk, hw, c, i0)) return;
    if (j.ops != 0) {
        const int m = jit::has_contrast(j.ops) ? jit::contrast_mean(sums[n], hw) : 0;
        jit::apply<NP, false>(j, m, c);
    }
    float *o = out + (int64_t)n * 3 * hw + i0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float m = nm.mean[k], s = nm.std[k];
        if constexpr (VEC) {
            const f32x4 v = {norm1(c[0][k], m, s), norm1(c[1][k], m, s), norm1(c[2][k], m, s), norm1(c[3][k], m, s)};
            __builtin_nontemporal_store(v, (f32x4 *)(o + k * hw));
        } else {
            o[k * hw] = norm1(c[0][k], m, s);
        }
    }
}

// the geometry of a resize launch, shared by the fp32 and the uint8 entry
struct RsLaunch {
    RsAxis ax, ay;
    int TH, rcap;
    int64_t tiles_x, tiles_y, blocks;
    size_t lds;
};

bool rs_launch(int N, int Hs, int Ws, int H, int W, RsLaunch *g) {
    if (!rs_axis(Ws, W, &g->ax) || !rs_axis(Hs, H, &g->ay)) return false;
    // the tallest tile whose source rows fit the intermediate: R <= (TH - 1) * scale + 2 * support + 1 <= rcap
    g->TH = 16;
    for (;; g->TH /= 2) {
        g->rcap = (int)ceil((g->TH - 1) * g->ay.scale) + g->ay.ksize + 1;
        if ((int64_t)g->rcap * RS_TW * 4 <= RS_INTER_BYTES || g->TH == 1) break;
    }
    g->tiles_x = (W + RS_TW - 1) / RS_TW;
    g->tiles_y = (H + g->TH - 1) / g->TH;
    g->blocks = g->tiles_x * g->tiles_y * N;
    g->lds = 4 * ((size_t)g->rcap * RS_TW + (size_t)RS_TW * g->ax.ksize + (size_t)g->TH * g->ay.ksize + 2 * RS_TW +
                  2 * g->TH);
    return g->blocks <= 0x7fffffff;
}

template <bool U8>
int rs_run(const uint8_t *src, int N, int Hs, int Ws, const void *plan_dev, int H, int W, const RsLaunch &g,
           const Norm &nm, void *out, int vec, void *stream) {
    const int32_t *xb = (const int32_t *)plan_dev, *xk = xb + 2 * (int64_t)W;
    const int32_t *yb = xk + (int64_t)W * g.ax.ksize, *yk = yb + 2 * (int64_t)H;
    const int64_t last_dw = ((int64_t)((uintptr_t)src & 3) + (int64_t)N * Hs * Ws * 3 - 1) >> 2;
    // a window has at most ksize - 1 taps: up to 4, 8, 12 of them run unrolled (downscales up to 5.5x), more looped
    auto kern = g.ax.ksize <= 5 ? k_img_resize_norm<1, U8> : g.ax.ksize <= 9 ? k_img_resize_norm<2, U8> :
                g.ax.ksize <= 13 ? k_img_resize_norm<3, U8> : k_img_resize_norm<0, U8>;
    hipLaunchKernelGGL(kern, dim3((unsigned)g.blocks), dim3(256), g.lds, (hipStream_t)stream, src, Hs, Ws, H, W, xb, xk,
                       yb, yk, g.ax.ksize, g.ay.ksize, g.TH, g.rcap, (int)g.tiles_x, (int)g.tiles_y, last_dw, nm, out,
                       vec);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int bev_image_normalize_u8_f32(const uint8_t *src, int N, int H, int W, const float *mean,
                                          const float *stdv, float *out, void *stream) {
    if (!src || !out || !mean || !stdv || N < 0 || H <= 0 || W <= 0) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c];
        nm.std[c] = stdv[c];
    }
    const int64_t hw = (int64_t)H * W;
    const bool vec = (hw % 4 == 0) && (((uintptr_t)src & 3) == 0) && (((uintptr_t)out & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        const int64_t total = (int64_t)N * (hw / 4);
        hipLaunchKernelGGL(k_img_norm_v4, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           (const uint32_t *)src, hw / 4, total, nm, out);
    } else {
        const int64_t total = (int64_t)N * hw;
        hipLaunchKernelGGL(k_img_norm_scalar, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, hw, total,
                           nm, out);
    }
    return (int)hipGetLastError();
}

extern "C" int64_t bev_image_resize_plan_bytes(int Hs, int Ws, int H, int W) {
    RsAxis ax, ay;
    if (!rs_axis(Ws, W, &ax) || !rs_axis(Hs, H, &ay)) return 0;
    return 4 * ((int64_t)W * (2 + ax.ksize) + (int64_t)H * (2 + ay.ksize));
}

extern "C" int bev_image_resize_plan(int Hs, int Ws, int H, int W, void *host_buf, int64_t bytes) {
    RsAxis ax, ay;
    if (!host_buf || ((uintptr_t)host_buf & 3) || !rs_axis(Ws, W, &ax) || !rs_axis(Hs, H, &ay)) return BEV_ERR_ARGS;
    if (bytes != bev_image_resize_plan_bytes(Hs, Ws, H, W)) return BEV_ERR_ARGS;
    int32_t *xb = (int32_t *)host_buf, *xk = xb + 2 * (int64_t)W;
    int32_t *yb = xk + (int64_t)W * ax.ksize, *yk = yb + 2 * (int64_t)H;
    rs_fill_axis(Ws, W, ax, xb, xk);
    rs_fill_axis(Hs, H, ay, yb, yk);
    return 0;
}

extern "C" int bev_image_resize_normalize_u8_f32(const uint8_t *src, int N, int Hs, int Ws, const void *plan_dev, int H,
                                                 int W, const float *mean, const float *stdv, float *out,
                                                 void *stream) {
    if (!src || !plan_dev || !out || !mean || !stdv || N < 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0)
        return BEV_ERR_ARGS;
    RsAxis ax, ay;
    if (((uintptr_t)plan_dev & 3) || !rs_axis(Ws, W, &ax) || !rs_axis(Hs, H, &ay)) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    RsLaunch g;
    if (!rs_launch(N, Hs, Ws, H, W, &g)) return BEV_ERR_ARGS;
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c];
        nm.std[c] = stdv[c];
    }
    const int vec = (W % 4 == 0) && (((uintptr_t)out & 15) == 0);
    return rs_run<false>(src, N, Hs, Ws, plan_dev, H, W, g, nm, out, vec, stream);
}

extern "C" int bev_image_resize_u8(const uint8_t *src, int N, int Hs, int Ws, const void *plan_dev, int H, int W,
                                   uint8_t *out_u8, void *stream) {
    if (!src || !plan_dev || !out_u8 || N < 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return BEV_ERR_ARGS;
    RsAxis ax, ay;
    if (((uintptr_t)plan_dev & 3) || !rs_axis(Ws, W, &ax) || !rs_axis(Hs, H, &ay)) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    if (Hs == H && Ws == W)
        return (int)hipMemcpyAsync(out_u8, src, (size_t)N * H * W * 3, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    RsLaunch g;
    if (!rs_launch(N, Hs, Ws, H, W, &g)) return BEV_ERR_ARGS;
    const int vec = (W % 4 == 0) && (((uintptr_t)out_u8 & 3) == 0);
    return rs_run<true>(src, N, Hs, Ws, plan_dev, H, W, g, Norm{}, out_u8, vec, stream);
}

extern "C" int64_t bev_image_jitter_workspace_bytes(int N) { return N > 0 ? 8 * (int64_t)N : 0; }

extern "C" int bev_image_jitter_normalize_u8_f32(const uint8_t *src, int N, int H, int W, const int32_t *params,
                                                 const float *mean, const float *stdv, void *workspace,
                                                 int64_t workspace_bytes, float *out, void *stream) {
    if (!src || !params || !mean || !stdv || !workspace || !out || N < 0 || H <= 0 || W <= 0) return BEV_ERR_ARGS;
    if (((uintptr_t)params & 3) || ((uintptr_t)workspace & 7) || ((uintptr_t)out & 3)) return BEV_ERR_ARGS;
    if (workspace_bytes < bev_image_jitter_workspace_bytes(N)) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    const int64_t hw = (int64_t)H * W;
    const bool vec = (hw % 4 == 0) && (((uintptr_t)src & 3) == 0) && (((uintptr_t)out & 15) == 0);
    const int64_t bpf = (hw + (vec ? 1024 : 256) - 1) / (vec ? 1024 : 256);
    if (bpf * N > 0x7fffffff) return BEV_ERR_ARGS;
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c];
        nm.std[c] = stdv[c];
    }
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, 8 * (size_t)N, st);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)(bpf * N)), block(256);
    const uint32_t *rec = (const uint32_t *)params;
    unsigned long long *sums = (unsigned long long *)workspace;
    if (vec) {
        hipLaunchKernelGGL(k_img_jitter_sum<true>, grid, block, 0, st, src, hw, (int)bpf, rec, sums);
        hipLaunchKernelGGL(k_img_jitter_norm<true>, grid, block, 0, st, src, hw, (int)bpf, rec, sums, nm, out);
    } else {
        hipLaunchKernelGGL(k_img_jitter_sum<false>, grid, block, 0, st, src, hw, (int)bpf, rec, sums);
        hipLaunchKernelGGL(k_img_jitter_norm<false>, grid, block, 0, st, src, hw, (int)bpf, rec, sums, nm, out);
    }
    return (int)hipGetLastError();
}

extern "C" int bev_image_jitter_u8_host(const uint8_t *src, int N, int H, int W, const int32_t *params,
                                        uint8_t *out_u8) {
    if (!src || !params || !out_u8 || N < 0 || H <= 0 || W <= 0 || ((uintptr_t)params & 3)) return BEV_ERR_ARGS;
    const int64_t hw = (int64_t)H * W;
    for (int n = 0; n < N; ++n) {
        const jit::Rec j = jit::load_rec((const uint32_t *)params + (int64_t)n * jit::REC_WORDS);
        const uint8_t *s = src + n * hw * 3;
        uint8_t *o = out_u8 + n * hw * 3;
        int m = 0;
        if (jit::has_contrast(j.ops)) {
            uint64_t sum = 0;
            for (int64_t i = 0; i < hw; ++i) {
                unsigned c[1][3] = {{s[3 * i], s[3 * i + 1], s[3 * i + 2]}};
                jit::apply<1, true>(j, 0, c);
                sum += jit::luma(c[0][0], c[0][1], c[0][2]);
            }
            m = jit::contrast_mean(sum, hw);
        }
        for (int64_t i = 0; i < hw; ++i) {
            unsigned c[1][3] = {{s[3 * i], s[3 * i + 1], s[3 * i + 2]}};
            jit::apply<1, false>(j, m, c);
            for (int k = 0; k < 3; ++k) o[3 * i + k] = (uint8_t)c[0][k];
        }
    }
    return 0;
}
