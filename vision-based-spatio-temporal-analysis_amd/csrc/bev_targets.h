// bev_targets.h -- the per-object arithmetic of BEVNet's CenterNet training targets (model_wrapper.py:126-203,
// 278-300 of the reference; BEVNet._targets_from_boxes / _splat_gaussians / _gaussian_radius_tensor here), for the
// kernels of bev_targets.hip, k_gauss_radius of bev_head.hip and the host entry bev_centernet_targets_host alike.
//
// Every expression is the float32 op sequence torch runs on the device, op by op (the sources that include this
// header are compiled with -ffp-contract=off: no product fuses into an FMA, on the host or on the device):
//   * a tensor times a Python scalar is x * (float)s; a tensor over a Python scalar is a product with the scalar's
//     reciprocal (torch's device division by a host scalar; the caller passes that reciprocal as torch rounds it); a
//     tensor over a tensor is a true division;
//   * x ** 2 is a product; clamp / min propagate NaN like torch's;
//   * 2 sigma^2 = ((2 r + 1) * (1 / 6)) ** 2 * 2 in double (the reference's Python-float denominator as the device
//     computes it from radius.double()), rounded to float.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BEV_TGT_FN __host__ __device__ __forceinline__
#else
#define BEV_TGT_FN static inline
#endif

namespace bev_targets {

// the Python-scalar operands of the radius formula as torch casts them: f_1mov = (float)(1 - ov), rcp_1pov = 1.0f /
// (float)(1 + ov), f_4ov = (float)(4 ov), f_m2ov = (float)(-2 ov), f_ovm1 = (float)(ov - 1); ov_zero: r3 = +inf
struct RadiusConsts {
    float f_1mov, rcp_1pov, f_4ov, f_m2ov, f_ovm1;
    int ov_zero;
    float min_radius;
};

// the grid: gx = (x - x_min) * rcp_res_x, inside when 0 <= gx < Wb and 0 <= gy < Hb
struct Grid {
    int Hb, Wb;
    float x_min, y_min, rcp_res_x, rcp_res_y;
};

BEV_TGT_FN float clamp_min(float x, float lo) { return x < lo ? lo : x; }  // NaN stays NaN
BEV_TGT_FN float min_nan(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
BEV_TGT_FN float root(float a, float b, float c) {
    const float t = clamp_min(b * b - (a * 4.0f) * c, 0.0f);  // b ** 2 - 4 * a * c, clamp(min=0)
    return b + sqrtf(t);
}

// floor(r).to(int64).  The device keeps its conversion (a NaN gives 0 there); the host, where the cast of a NaN or of
// a value past the int64 range is undefined, gives 0 for both: no gaussian is drawn
BEV_TGT_FN int64_t floor_i64(float r) {
    const float f = floorf(r);
#if defined(__HIP_DEVICE_COMPILE__)
    return (int64_t)f;
#else
    return (f != f || f >= 9.2233720368547758e18f || f <= -9.2233720368547758e18f) ? 0 : (int64_t)f;
#endif
}

// model_wrapper.py:205-233 for one object: width / height in cells -> radius
BEV_TGT_FN int64_t gaussian_radius(float wc, float hc, const RadiusConsts &k) {
    const float w = clamp_min(wc, 1.0f), h = clamp_min(hc, 1.0f);
    const float r1 = root(1.0f, h + w, ((w * h) * k.f_1mov) * k.rcp_1pov) * 0.5f;
    const float a2 = 4.0f;
    const float r2 = root(a2, (h + w) * 2.0f, (w * k.f_1mov) * h) / (a2 * 2.0f);
    float r = min_nan(r1, r2);
    if (!k.ov_zero) {
        const float a3 = k.f_4ov;
        const float r3 = root(a3, (h + w) * k.f_m2ov, (w * k.f_ovm1) * h) / (a3 * 2.0f);
        r = min_nan(r, r3);
    }
    return floor_i64(clamp_min(r, k.min_radius));
}

// one box (cx, cy, w, h in world units) on the grid
struct Object {
    bool inside;        // 0 <= gx < Wb and 0 <= gy < Hb (false for a NaN centre)
    int cx, cy;         // floor(gx), floor(gy): meaningful when inside
    float off_x, off_y; // gx - floor(gx), gy - floor(gy)
    float log_w, log_h; // log(clamp(w * rcp_res_x, min=1e-3)), the same for h
    float w_cells, h_cells;
};

BEV_TGT_FN Object object_on_grid(float bx, float by, float bw, float bh, const Grid &g) {
    Object o;
    const float gx = (bx - g.x_min) * g.rcp_res_x;
    const float gy = (by - g.y_min) * g.rcp_res_y;
    o.inside = gx >= 0.0f && gx < (float)g.Wb && gy >= 0.0f && gy < (float)g.Hb;
    const float fx = floorf(gx), fy = floorf(gy);
    o.cx = o.inside ? (int)fx : 0;
    o.cy = o.inside ? (int)fy : 0;
    o.off_x = gx - fx;
    o.off_y = gy - fy;
    o.w_cells = clamp_min(bw * g.rcp_res_x, 1e-3f);
    o.h_cells = clamp_min(bh * g.rcp_res_y, 1e-3f);
    o.log_w = logf(o.w_cells);
    o.log_h = logf(o.h_cells);
    return o;
}

// 2 sigma^2 of a radius-r gaussian, sigma = (2 r + 1) / 6
BEV_TGT_FN float two_sigma2(int64_t r) {
    const double s = (2.0 * (double)r + 1.0) * (1.0 / 6.0);
    return (float)((s * s) * 2.0);
}

// an entry of the heatmap pass's object list: the window is |dx| <= r and |dy| <= r.  r is clamped to the larger grid
// side (in 64 bits, before it narrows): with the centre inside the grid any larger radius covers the same cells
struct alignas(16) Splat {
    int cx, cy, r;
    float s2;
};

BEV_TGT_FN Splat make_splat(int cx, int cy, int64_t radius, const Grid &g) {
    Splat s;
    const int64_t cap = g.Hb > g.Wb ? g.Hb : g.Wb;
    s.cx = cx;
    s.cy = cy;
    s.r = (int)(radius < cap ? radius : cap);
    s.s2 = two_sigma2(radius);
    return s;
}

// the gaussian of one object at cell (x, y); 0 outside its window (every value inside is > 0)
BEV_TGT_FN float splat_at(const Splat &s, int x, int y) {
    const int dx = x - s.cx, dy = y - s.cy;
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if (ax > s.r || ay > s.r) return 0.0f;
    const int64_t d2 = (int64_t)dx * dx + (int64_t)dy * dy;
    return expf(-(float)d2 / s.s2);
}

}  // namespace bev_targets
