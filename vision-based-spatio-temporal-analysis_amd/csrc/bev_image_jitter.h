// bev_image_jitter.h -- the per-pixel arithmetic of T.ColorJitter on 8-bit RGB, as torchvision's PIL path computes
// it (data/transforms.py:14: T.RandomApply([T.ColorJitter(0.2, 0.2, 0.2, 0.05)], p=0.5)), for the kernels of
// bev_image.hip and the host entry bev_image_jitter_u8_host alike.
//
// Brightness / contrast / saturation are PIL.ImageEnhance: Image.blend(degenerate, image, factor), which is Pillow's
// ImagingBlend (Blend.c) per channel in C `float`, with the degenerate image black, the rounded mean of the L
// conversion, or the L conversion itself.  Hue is torchvision's _adjust_hue: RGB -> HSV, the hue byte plus a shift
// byte (uint8 wrap-around), HSV -> RGB, both conversions Pillow's Convert.c (rgb2hsv_row / hsv2rgb_row), which mix
// float and double the way C's promotion rules say.  Every expression below keeps Pillow's types and operation
// order, and the sources that include this header are compiled with -ffp-contract=off, so that no product fuses into
// an FMA on the host or on the device: the results are Pillow's bit for bit (tests/test_image_jitter_host.py checks
// the hue path over all 2^24 colours).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BEV_JIT_FN __host__ __device__ __forceinline__
#else
#define BEV_JIT_FN static inline
#endif

namespace bev_jitter {

// op codes of a record's word 0, four bits per op in application order; 0 ends the list, any other code is a no-op
enum { OP_END = 0, OP_BRIGHTNESS = 1, OP_CONTRAST = 2, OP_SATURATION = 3, OP_HUE = 4, MAX_OPS = 8, REC_WORDS = 8 };

struct Rec {  // words 0..4 of a frame's record
    uint32_t ops;
    float fb, fc, fs;  // brightness, contrast, saturation factors
    unsigned hue;      // hue shift byte
};

BEV_JIT_FN float bits_f32(uint32_t u) {
    union {
        uint32_t u;
        float f;
    } v;
    v.u = u;
    return v.f;
}

BEV_JIT_FN Rec load_rec(const uint32_t *w) {
    Rec j;
    j.ops = w[0];
    j.fb = bits_f32(w[1]);
    j.fc = bits_f32(w[2]);
    j.fs = bits_f32(w[3]);
    j.hue = w[4] & 255u;
    return j;
}

BEV_JIT_FN bool has_contrast(uint32_t ops) {
    for (int i = 0; i < MAX_OPS; ++i) {
        const unsigned code = (ops >> (4 * i)) & 15u;
        if (code == OP_END) break;
        if (code == OP_CONTRAST) return true;
    }
    return false;
}

// ImagingBlend(degenerate d, pixel p, alpha a), one channel: one fp32 multiply, one fp32 add, truncation.
BEV_JIT_FN unsigned blend(unsigned d, unsigned p, float a) {
    const float prod = a * (float)((int)p - (int)d);
    const float t = (float)(int)d + prod;
    if (a >= 0.0f && a <= 1.0f) return (unsigned)(int)t & 255u;  // interpolation: t is within 0..255
    if (t <= 0.0f) return 0u;
    if (t >= 255.0f) return 255u;
    return (unsigned)(int)t;
}

// Pillow's RGB -> L (ITU-R 601-2, 16-bit fixed point, rounded)
BEV_JIT_FN unsigned luma(unsigned r, unsigned g, unsigned b) {
    return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;
}

BEV_JIT_FN unsigned clip8(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// Convert.c rgb2hsv_row
BEV_JIT_FN void rgb2hsv(unsigned r, unsigned g, unsigned b, unsigned &uh, unsigned &us, unsigned &uv) {
    const unsigned maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const unsigned minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    uv = maxc;
    if (minc == maxc) {
        uh = 0;
        us = 0;
        return;
    }
    const float cr = (float)(int)(maxc - minc);
    const float s = cr / (float)(int)maxc;
    const float rc = (float)(int)(maxc - r) / cr;
    const float gc = (float)(int)(maxc - g) / cr;
    const float bc = (float)(int)(maxc - b) / cr;
    float h;
    if (r == maxc) {
        h = bc - gc;
    } else if (g == maxc) {
        h = (float)((2.0 + (double)rc) - (double)bc);  // the literal is a double: summed in double, rounded once
    } else {
        h = (float)((4.0 + (double)gc) - (double)rc);
    }
    // fmod(h / 6.0 + 1.0, 1.0): the argument lies in [5/6, 11/6], where fmod is x or the exact x - 1
    const double x = (double)h / 6.0 + 1.0;
    h = (float)(x >= 1.0 ? x - 1.0 : x);
    uh = clip8((int)((double)h * 255.0));
    us = clip8((int)((double)s * 255.0));
}

BEV_JIT_FN unsigned hsv_round8(double x) {  // float p = round(x); CLIP8(p)
    const float p = (float)round(x);
    return p <= 0.0f ? 0u : (p >= 255.0f ? 255u : (unsigned)(int)p);
}

// Convert.c hsv2rgb_row
BEV_JIT_FN void hsv2rgb(unsigned h, unsigned s, unsigned v, unsigned &r, unsigned &g, unsigned &b) {
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double h6 = (double)(int)h * 6.0 / 255.0;
    const float i = (float)floor(h6);
    const float f = (float)(h6 - (double)i);
    const float fs = (float)((double)(float)(int)s / 255.0);
    const double fv = (double)(float)(int)v;
    const float fsf = fs * f;  // float * float: an fp32 product
    const unsigned p = hsv_round8(fv * (1.0 - (double)fs));
    const unsigned q = hsv_round8(fv * (1.0 - (double)fsf));
    const unsigned t = hsv_round8(fv * (1.0 - (double)fs * (1.0 - (double)f)));
    switch ((int)i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// A record's op list on NP pixels c[p] = (r, g, b), each op on every pixel before the next (the op branch is
// uniform over the frame).  PRE: stop in front of the first contrast -- what its mean is taken over; otherwise m is
// that mean (a list that names contrast twice uses it for both, which ColorJitter never draws).
template <int NP, bool PRE>
BEV_JIT_FN void apply(const Rec &j, int m, unsigned (&c)[NP][3]) {
#pragma unroll 1
    for (int i = 0; i < MAX_OPS; ++i) {
        const unsigned code = (j.ops >> (4 * i)) & 15u;
        if (code == OP_END) break;
        if (code == OP_BRIGHTNESS) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int k = 0; k < 3; ++k) c[p][k] = blend(0u, c[p][k], j.fb);
        } else if (code == OP_CONTRAST) {
            if (PRE) return;
            const unsigned d = clip8(m);
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int k = 0; k < 3; ++k) c[p][k] = blend(d, c[p][k], j.fc);
        } else if (code == OP_SATURATION) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const unsigned d = luma(c[p][0], c[p][1], c[p][2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) c[p][k] = blend(d, c[p][k], j.fs);
            }
        } else if (code == OP_HUE) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                unsigned h, s, v;
                rgb2hsv(c[p][0], c[p][1], c[p][2], h, s, v);
                hsv2rgb((h + j.hue) & 255u, s, v, c[p][0], c[p][1], c[p][2]);
            }
        }
    }
}

// ImageEnhance.Contrast's degenerate value: int(sum(L) / count + 0.5), in double
BEV_JIT_FN int contrast_mean(uint64_t sum_l, int64_t count) { return (int)((double)sum_l / (double)count + 0.5); }

}  // namespace bev_jitter
