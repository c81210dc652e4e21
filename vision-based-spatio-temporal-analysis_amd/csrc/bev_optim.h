// bev_optim.h -- the per-element arithmetic of the Adam / AdamW parameter update (the reference's train.py:46-52
// optim.Adam / optim.AdamW stepped at train.py:238-255), for the kernel of bev_optim.hip and the host entry
// bev_adam_step_host alike.
//
// The update is torch's _single_tensor_adam op for op with every fused multiply-add split into its two roundings;
// the sources that include this header are compiled with -ffp-contract=off, so that no product fuses on the host or
// on the device.  It is DEFINED as this fp32 sequence, every operation rounded once, in the order written:
//
//   g  = grad                                   ; with a grad_scale: g = g * inv, inv = float(1.0 / double(scale))
//   coupled decay   (Adam,  wd != 0):  g = g + p * float(wd)
//   decoupled decay (AdamW, wd != 0):  p = p * float(1.0 - lr * wd)           (double arithmetic, then one cast)
//   w1 = float(1.0 - beta1)
//   m  = (w1 < 0.5f) ? m + w1 * (g - m) : g - (g - m) * (1.0f - w1)           (torch's lerp, both branches)
//   v  = v * float(beta2) + (float(1.0 - beta2) * g) * g
//   t  = step + 1 ;  bc1 = 1 - beta1^t ;  bc2 = 1 - beta2^t                   (double; beta^t by ipow below)
//   ss = float(lr / bc1) ;  bs = float(sqrt(bc2))                             (double division and root, one cast each)
//   den = sqrtf(v) / bs + float(eps)
//   p  = p - ss * (m / den)
//
// The double division and square root and the fp32 division and square root are the correctly rounded IEEE operations
// on both sides, so host and device agree bit for bit (tests/test_optim_gpu.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BEV_OPT_FN __host__ __device__ __forceinline__
#else
#define BEV_OPT_FN static inline
#endif

namespace bev_optim {

enum { DECAY_NONE = 0, DECAY_COUPLED = 1, DECAY_DECOUPLED = 2 };

// One tensor's record of the table (include/bev_mi355x.h): eight 64-bit words.
enum {
    REC_P = 0,
    REC_G = 1,
    REC_M = 2,
    REC_V = 3,
    REC_STEP_IN = 4,
    REC_STEP_OUT = 5,
    REC_N = 6,
    REC_CHUNK0 = 7,
    REC_WORDS = 8
};

constexpr int CHUNK = 2048;  // elements per workgroup of the kernel

struct Hyper {  // what a launch shares: the hyperparameters, each already in the type the sequence above uses it in
    double lr, beta1, beta2;
    float w1, one_minus_w1, b2, w2, eps, wd, decay_mul;
    int decay;
};

BEV_OPT_FN Hyper make_hyper(double lr, double beta1, double beta2, double eps, double wd, int decoupled) {
    Hyper h;
    h.lr = lr;
    h.beta1 = beta1;
    h.beta2 = beta2;
    h.w1 = (float)(1.0 - beta1);
    h.one_minus_w1 = 1.0f - h.w1;
    h.b2 = (float)beta2;
    h.w2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.wd = (float)wd;
    h.decay_mul = (float)(1.0 - lr * wd);
    h.decay = wd == 0.0 ? DECAY_NONE : (decoupled ? DECAY_DECOUPLED : DECAY_COUPLED);
    return h;
}

// b^t for t >= 1 by square-and-multiply, least significant bit of t first: r starts at 1, x at b; for each bit of t
// from the lowest, a set bit multiplies r by x, and x is squared while higher bits remain.
BEV_OPT_FN double ipow(double b, uint32_t t) {
    double r = 1.0, x = b;
    while (t) {
        if (t & 1u) r = r * x;
        t >>= 1;
        if (t) x = x * x;
    }
    return r;
}

// The step counter is an fp32 scalar, as torch keeps it; the update it counts is number t = step + 1.  Counters that
// are not a count (negative, NaN, 2^31 or more) are taken as 0.
BEV_OPT_FN uint32_t step_number(float step) {
    return (step >= 0.0f && step < 2147483648.0f) ? (uint32_t)step + 1u : 1u;
}

struct StepScalars {
    float ss, bs;
};

BEV_OPT_FN StepScalars step_scalars(const Hyper &h, float step) {
    const uint32_t t = step_number(step);
    const double bc1 = 1.0 - ipow(h.beta1, t);
    const double bc2 = 1.0 - ipow(h.beta2, t);
    StepScalars s;
    s.ss = (float)(h.lr / bc1);
    s.bs = (float)sqrt(bc2);
    return s;
}

BEV_OPT_FN float inv_scale(float scale) { return (float)(1.0 / (double)scale); }

// One element.  scaled: g is multiplied by inv first.  g is a value: the gradient in memory is never written.
BEV_OPT_FN void update(const Hyper &h, const StepScalars &s, bool scaled, float inv, float &p, float g, float &m,
                       float &v) {
    // selects, not branches: the kernel's body stays one straight line behind its loads
    const float gs = g * inv;
    g = scaled ? gs : g;
    const float gd = g + p * h.wd;
    g = h.decay == DECAY_COUPLED ? gd : g;
    const float pd = p * h.decay_mul;
    p = h.decay == DECAY_DECOUPLED ? pd : p;
    const float diff = g - m;
    const float m_lo = m + h.w1 * diff;
    const float m_hi = g - diff * h.one_minus_w1;
    m = h.w1 < 0.5f ? m_lo : m_hi;
    const float a = v * h.b2;
    const float b = (h.w2 * g) * g;
    v = a + b;
    const float den = sqrtf(v) / s.bs + h.eps;
    const float q = m / den;
    const float u = s.ss * q;
    p = p - u;
}

}  // namespace bev_optim
