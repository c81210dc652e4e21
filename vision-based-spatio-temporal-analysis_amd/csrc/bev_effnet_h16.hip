// bev_effnet_h16.hip -- the EfficientNet trunk in the "f16" inference arithmetic (bev_native.conv_arith_mode("f16"))
// for gfx950: what the reference's validation forward computes in eval() under autocast(float16) (train.py:285-286)
// on its shipped backbone (configs/wildtrack.yaml: efficientnet_b0, OUT_INDEX 2).  Activations are stored in fp16
// from the stem to the trunk output, the BN-folded weights are rounded once to fp16, every sum is accumulated in
// fp32 and every stored value is rounded once (RNE) after bias / residual / activation:
//
//   k_dwconv_r16  the depthwise-separable block's depthwise conv: k_dwconv_r's row runs (bev_effnet.hip) on fp16
//                 storage; fp32 fmaf chain from the bias, ky-major then kx-minor; SE partials of the ROUNDED outputs.
//   k_irdw_h16    k_irdw's expansion + depthwise pass with the staged row and the ring in fp16 and the expansion
//                 on v_mfma_f32_16x16x32_f16 (one MFMA for Ci <= 32, two for 40 / 48 instead of Ci / 4).
//   k_pw_h16      wave-streaming 1x1 conv on v_mfma_f32_32x32x16_f16 (k_pw_mfma's scheme, bev_conv.hip): optional SE
//                 gate in the operand load (a = f16(float(y16) * gate)), optional fp16 residual, fp16 or fp32 output.
//
// The stem with an fp16 store is k_stem3 itself (bev_effnet.hip, bev_conv2d_stem3_h16); the SE gate is
// bev_se_gate_f32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bev_mi355x.h"
#include "bev_act.h"
#include "bev_mfma.h"

namespace {

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float act_f(float t, int act) {
    if (act == 1) return relu_f(t);
    if (act == 2) return silu_hw(t);
    return t;
}

// ---- depthwise ---------------------------------------------------------------------------------------------------
// k_dwconv_r's scheme: a thread owns one channel quad (8 B of fp16) of R consecutive outputs of one row; every
// kernel row's (R - 1) S + K input pixels are loaded once into registers (all rows up front for 3 x 3) and applied
// to the R outputs.  Out-of-range pixels read as 0 (exact).  The SE partial of a workgroup sums the rounded outputs
// (the values a later reader of y sees) in a fixed order.
constexpr int DW_NT = 256;
template <int S> constexpr int dw_run_len() { return S == 1 ? 8 : 4; }
inline int dw16_blocks(int Ho, int Wo, int C, int stride) {
    const int R = stride == 1 ? dw_run_len<1>() : dw_run_len<2>(), PB = DW_NT / (C / 4);
    return (int)(((int64_t)Ho * ((Wo + R - 1) / R) + PB - 1) / PB);
}

__device__ __forceinline__ f32x4 ld_h4(const _Float16 *p) {
    const h16x4 v = *(const h16x4 *)p;
    return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

template <int K, int S, bool UP>
__global__ __launch_bounds__(DW_NT) void k_dwconv_r16(const _Float16 *__restrict__ x, int H, int W, int C,
                                                      const _Float16 *__restrict__ wt, const float *__restrict__ bias,
                                                      int pad, int act, _Float16 *__restrict__ y, int Ho, int Wo,
                                                      float *__restrict__ psum, int nb) {
    constexpr int R = dw_run_len<S>(), IC = (R - 1) * S + K;
    __shared__ f32x4 red[DW_NT];
    const int CH4 = C >> 2, PB = DW_NT / CH4;  // channel quads, runs per workgroup
    const int tid = threadIdx.x, pl = tid / CH4, q = tid - pl * CH4;
    const int n = blockIdx.y, blk = blockIdx.x;
    const int rpr = (Wo + R - 1) / R;
    const int64_t ri = (int64_t)blk * PB + pl;
    const bool active = pl < PB && ri < (int64_t)Ho * rpr;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const int oy = (int)(ri / rpr), ox0 = (int)(ri - (int64_t)oy * rpr) * R;
        const int ix0 = ox0 * S - pad;
        f32x4 w[K * K];
#pragma unroll
        for (int t = 0; t < K * K; ++t) w[t] = ld_h4(wt + (int64_t)t * C + q * 4);
        const f32x4 b = *(const f32x4 *)(bias + q * 4);
        f32x4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = b;
        const _Float16 *xn = x + (int64_t)n * H * W * C + q * 4;
        h16x4 vu[UP ? K : 1][IC];
        const h16x4 z4 = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        if (UP) {  // every row's loads in flight at once (out-of-range rows read as 0)
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const int iy = oy * S - pad + ky;
                const bool rin = iy >= 0 && iy < H;
                const _Float16 *xr = xn + (int64_t)(rin ? iy : 0) * W * C;
#pragma unroll
                for (int c = 0; c < IC; ++c) {
                    const int ix = ix0 + c;
                    vu[UP ? ky : 0][c] = (rin && ix >= 0 && ix < W) ? *(const h16x4 *)(xr + (int64_t)ix * C) : z4;
                }
            }
        }
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = oy * S - pad + ky;
            h16x4 v[IC];
            if (UP) {
#pragma unroll
                for (int c = 0; c < IC; ++c) v[c] = vu[UP ? ky : 0][c];
            } else {
                if (iy < 0 || iy >= H) continue;
                const _Float16 *xr = xn + (int64_t)iy * W * C;
#pragma unroll
                for (int c = 0; c < IC; ++c) {
                    const int ix = ix0 + c;
                    v[c] = (ix >= 0 && ix < W) ? *(const h16x4 *)(xr + (int64_t)ix * C) : z4;
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const h16x4 vv = v[r * S + kx];
                    const f32x4 ww = w[ky * K + kx];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[r][u] = __builtin_fmaf((float)vv[u], ww[u], acc[r][u]);
                }
            }
        }
        _Float16 *yr = y + (((int64_t)n * Ho + oy) * Wo + ox0) * C + q * 4;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (ox0 + r >= Wo) break;
            h16x4 o;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                o[u] = (_Float16)act_f(acc[r][u], act);
                s[u] += (float)o[u];
            }
            *(h16x4 *)(yr + (int64_t)r * C) = o;
        }
    }
    if (psum == nullptr) return;
    red[tid] = s;
    __syncthreads();
    if (pl == 0) {  // fixed order over the runs: deterministic partial
        for (int l = 1; l < PB; ++l) s += red[l * CH4 + q];
        *(f32x4 *)(psum + ((int64_t)n * nb + blk) * C + q * 4) = s;
    }
}

// ---- fused expansion + depthwise -----------------------------------------------------------------------------------
// k_irdw's decomposition (bev_effnet.hip): a workgroup owns a strip of TC output columns x IR_RSEG output rows x 48
// channels (3 waves x 16), stages each input row it needs once (32 pixels, one row ahead in registers), every wave
// expands it into its ring of the last K rows and every output row is the K x K taps of that ring.  Here the staged
// row and the ring hold fp16, and the expansion is one v_mfma_f32_16x16x32_f16 per 32 input channels with the
// weights as the A operand (lane l: channel l & 15, k = 8 (l >> 4) + j, in registers for the whole workgroup) and the
// pixels as B (lane l: pixel l & 15, the same k: one 16-B LDS read), so D[channel 4 (l >> 4) + r][pixel l & 15] leaves
// a lane with four consecutive channels of one pixel: one 8-B ring write.  K is zero-padded to 32 / 64 (both
// operands).  h = f16(SiLU(acc + be)), 0 outside the image; the taps convert the ring's halves to fp32 and keep
// k_dwconv's fp32 fmaf chain from the bias; y is rounded once and the SE partials sum the rounded values.
// LDS strides (64 banks x 4 B): the staged row's pixel stride is KP + 8 halves (80 / 144 B: the 16 lanes of a 16-B
// read group hit 16 distinct 4-bank slots); the ring's pixel stride is 16 halves at stride 1 and 24 at stride 2, so
// the 32 lanes of an 8-B tap read (8 pixels x 4 quads, pixels S apart) cover the 64 banks once.
constexpr int IR_W = 3, IR_IC = 32, IR_RSEG = 16;
template <int K, int S> constexpr int ir_tc() { return (IR_IC - K) / S + 1; }

template <int K, int S, int CI>
__global__ __launch_bounds__(64 * IR_W) void k_irdw_h16(const _Float16 *__restrict__ x, int H, int W,
                                                        const _Float16 *__restrict__ we, const float *__restrict__ be,
                                                        const _Float16 *__restrict__ wd, const float *__restrict__ bd,
                                                        int Cm, _Float16 *__restrict__ y, int Ho, int Wo,
                                                        float *__restrict__ psum, int strips, int segs) {
    constexpr int TC = ir_tc<K, S>(), PAD = K / 2, KP = CI <= 32 ? 32 : 64, NM = KP / 32, XS = KP + 8, C8 = CI / 8;
    constexpr int HS = S == 1 ? 16 : 24;
    static_assert(CI % 8 == 0 && CI <= 64 && IR_IC * C8 <= 64 * IR_W, "CI");
    __shared__ __attribute__((aligned(16))) _Float16 xs[IR_IC * XS];                   // one staged input row
    __shared__ __attribute__((aligned(16))) _Float16 ring[IR_W][K][IR_IC * HS];        // the last K expanded rows per wave
    __shared__ __attribute__((aligned(16))) float wds[K * K][16 * IR_W];               // depthwise weights of the 48 channels
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x, sxi = blk % strips, syi = blk / strips, n = blockIdx.y;
    const int chw = blockIdx.z * 16 * IR_W, ch0 = chw + wave * 16;
    const int c0 = sxi * TC, r0 = syi * IR_RSEG;
    const int ix0 = c0 * S - PAD;
    const int rows_out = min(IR_RSEG, Ho - r0);
    const int l15 = lane & 15, lq = lane >> 4;
    // expansion weights (A operand): channel ch0 + l15, k = 32 m + 8 lq + j; zero past CI
    h16x8 aw[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const int k = 32 * m + 8 * lq;
        h16x8 v = {};
        if (k < CI) v = *(const h16x8 *)(we + (int64_t)(ch0 + l15) * CI + k);
        aw[m] = v;
    }
    const f32x4 bexp = *(const f32x4 *)(be + ch0 + 4 * lq);  // D rows: channels ch0 + 4 lq + r
    for (int e = tid; e < K * K * 16 * IR_W; e += 64 * IR_W) {
        const int t = e / (16 * IR_W), c = e - t * (16 * IR_W);
        wds[t][c] = (float)wd[(int64_t)t * Cm + chw + c];
    }
    for (int e = tid; e < IR_IC * (XS - CI) / 8; e += 64 * IR_W) {  // the K padding (and the stride pad) of the staged row
        constexpr int ZP = (XS - CI) / 8;
        const int px = e / ZP, z = e - px * ZP;
        *(h16x8 *)(xs + px * XS + CI + 8 * z) = (h16x8){};
    }
    const int p = lane >> 2, q = lane & 3;  // depthwise: output pixel p (+16 per pass), channel quad q
    const f32x4 bdw = *(const f32x4 *)(bd + ch0 + 4 * q);
    f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
    const _Float16 *xn = x + (int64_t)n * H * W * CI;
    _Float16 *hr = &ring[wave][0][0];
    // the next input row's 16-B piece of this thread, loaded one row ahead
    const int lpx = tid / C8, lc8 = tid - lpx * C8;
    const bool lact = tid < IR_IC * C8;
    h16x8 pre = {};
    auto load_row = [&](int iy) {
        const int ix = ix0 + lpx;
        h16x8 v = {};
        if (lact && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
            v = *(const h16x8 *)(xn + ((int64_t)iy * W + ix) * CI + 8 * lc8);
        pre = v;
    };
    auto expand_row = [&](int iy) {  // stage + expand input row iy into ring slot iy mod K (iy may be outside)
        __syncthreads();  // the previous row's staged pixels are no longer read
        const bool rin = (unsigned)iy < (unsigned)H;
        if (lact) *(h16x8 *)(xs + lpx * XS + 8 * lc8) = pre;
        load_row(iy + 1);
        __syncthreads();
        const int slot = ((iy % K) + K) % K;
#pragma unroll
        for (int g = 0; g < IR_IC / 16; ++g) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const h16x8 bx = *(const h16x8 *)(xs + (g * 16 + l15) * XS + 32 * m + 8 * lq);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[m], bx, acc, 0, 0, 0);
            }
            const int px = g * 16 + l15, ix = ix0 + px;
            const bool in = rin && (unsigned)ix < (unsigned)W;
            h16x4 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) hv[r] = in ? (_Float16)silu_hw(acc[r] + bexp[r]) : (_Float16)0.0f;
            *(h16x4 *)(hr + slot * IR_IC * HS + px * HS + 4 * lq) = hv;
        }
    };
    int iy_next = r0 * S - PAD;
    load_row(iy_next);
    for (int ro = 0; ro < rows_out; ++ro) {
        const int r = r0 + ro, iy_top = r * S - PAD;
        while (iy_next < iy_top + K) expand_row(iy_next++);
        // this wave's ring writes precede its reads (LDS is in order within a wave)
#pragma unroll
        for (int pp = 0; pp < (TC + 15) / 16; ++pp) {
            const int px = pp * 16 + p, c = c0 + px;
            if (px < TC && c < Wo) {
                f32x4 acc = bdw;
#pragma unroll
                for (int ky = 0; ky < K; ++ky) {
                    const int slot = (((iy_top + ky) % K) + K) % K;
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const h16x4 h = *(const h16x4 *)(hr + slot * IR_IC * HS + (px * S + kx) * HS + 4 * q);
                        const f32x4 w = *(const f32x4 *)(&wds[ky * K + kx][wave * 16 + 4 * q]);
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf((float)h[u], w[u], acc[u]);
                    }
                }
                h16x4 o;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    o[u] = (_Float16)silu_hw(acc[u]);
                    ssum[u] += (float)o[u];
                }
                *(h16x4 *)(y + (((int64_t)n * Ho + r) * Wo + c) * Cm + ch0 + 4 * q) = o;
            }
        }
    }
    // squeeze partials: the 16 pixel lanes of each channel quad, fixed order
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) ssum[u] += __shfl_xor(ssum[u], o);
    }
    if (p == 0) *(f32x4 *)(psum + ((int64_t)n * strips * segs + blk) * Cm + ch0 + 4 * q) = ssum;
}

// ---- pointwise -----------------------------------------------------------------------------------------------------
// Every wave owns 32 pixels and is independent (no block barrier).  Lane (i = lane & 31, h = lane >> 5) loads the
// 16-B pieces k in [16 s + 8 h, 16 s + 8 h + 8) of its pixel's row, s < NS = ceil(Ci / 16) -- the k slots lane
// (i, h) feeds in v_mfma_f32_32x32x16_f16, so the two half-waves read adjacent pieces and the k order is the
// natural one; pieces past Ci are zero.  With a gate the piece becomes f16(float(x) * gate[n][k]) as it is loaded.
// The operand stays in registers over the 32-channel output blocks; the weights' matching pieces (row co = block +
// i, zero past Co / Ci) are read per block.  D[(r & 3) + 8 (r >> 2) + 4 h][i] goes through a wave-private LDS tile
// and leaves as 8 channels per lane: (acc + bias) + residual, rounded once to fp16 (one 16-B store) or left fp32
// (two); every residual load of a block is issued before its first store.
constexpr int PW_ER = 36;  // LDS tile row stride (floats)

struct PwArgs {
    const _Float16 *x, *w, *res;
    const float *bias, *gate;
    void *y;
    int64_t M, HW;
    int Ci, Co, ldy;
};

template <int NS, bool F32OUT>
__global__ __launch_bounds__(256) void k_pw_h16(PwArgs a) {
    __shared__ __attribute__((aligned(16))) float epi[4][32 * PW_ER];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const int64_t mw = ((int64_t)blockIdx.x * 4 + wave) * 32;  // the wave's first pixel
    if (mw >= a.M) return;
    const int64_t m = mw + i < a.M ? mw + i : a.M - 1;
    const int Ci = a.Ci;
    h16x8 av[NS];
    {
        const _Float16 *xp = a.x + m * Ci;
        const float *gp = a.gate ? a.gate + (m / a.HW) * Ci : nullptr;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = 16 * s + 8 * h;
            h16x8 v = {};
            if (k < Ci) {
                v = *(const h16x8 *)(xp + k);
                if (gp) {
                    const f32x4 g0 = *(const f32x4 *)(gp + k), g1 = *(const f32x4 *)(gp + k + 4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        v[u] = (_Float16)((float)v[u] * g0[u]);
                        v[4 + u] = (_Float16)((float)v[4 + u] * g1[u]);
                    }
                }
            }
            av[s] = v;
        }
    }
    float *E = epi[wave];
    const int c8 = lane & 3, prow = lane >> 2;  // epilogue: 8 channels of rows prow and prow + 16
    const int nbt = (a.Co + 31) / 32;
    for (int nb = 0; nb < nbt; ++nb) {
        const int cow = nb * 32 + i;
        const _Float16 *wr = a.w + (int64_t)(cow < a.Co ? cow : 0) * Ci;
        f32x16 acc = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = 16 * s + 8 * h;
            h16x8 bv = {};
            if (k < Ci && cow < a.Co) bv = *(const h16x8 *)(wr + k);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[s], bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) E[((r & 3) + 8 * (r >> 2) + 4 * h) * PW_ER + i] = acc[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int co = nb * 32 + 8 * c8;
        if (co < a.Co) {  // Co % 8 == 0: a group of 8 is inside or outside
            f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
            if (a.bias) {
                b0 = *(const f32x4 *)(a.bias + co);
                b1 = *(const f32x4 *)(a.bias + co + 4);
            }
            h16x8 rv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int64_t mo = mw + prow + 16 * t;
                rv[t] = (a.res && mo < a.M) ? *(const h16x8 *)(a.res + mo * a.Co + co) : (h16x8){};
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int pr = prow + 16 * t;
                const int64_t mo = mw + pr;
                if (mo >= a.M) continue;
                f32x4 o0 = *(const f32x4 *)(E + pr * PW_ER + 8 * c8) + b0;
                f32x4 o1 = *(const f32x4 *)(E + pr * PW_ER + 8 * c8 + 4) + b1;
                if (a.res) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        o0[u] += (float)rv[t][u];
                        o1[u] += (float)rv[t][4 + u];
                    }
                }
                if constexpr (F32OUT) {
                    float *yp = (float *)a.y + mo * a.ldy + co;
                    *(f32x4 *)yp = o0;
                    *(f32x4 *)(yp + 4) = o1;
                } else {
                    h16x8 o;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        o[u] = (_Float16)o0[u];
                        o[4 + u] = (_Float16)o1[u];
                    }
                    *(h16x8 *)((_Float16 *)a.y + mo * a.ldy + co) = o;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <bool F32OUT>
void launch_pw(int ns, dim3 g, hipStream_t st, const PwArgs &a) {
    const dim3 b(256);
    // the trunk's widths (Ci 24 / 32, 40 / 48, 96, 144, 192, 240, 288) exactly; anything else in the next size up
    if (ns <= 2) hipLaunchKernelGGL((k_pw_h16<2, F32OUT>), g, b, 0, st, a);
    else if (ns <= 3) hipLaunchKernelGGL((k_pw_h16<3, F32OUT>), g, b, 0, st, a);
    else if (ns <= 6) hipLaunchKernelGGL((k_pw_h16<6, F32OUT>), g, b, 0, st, a);
    else if (ns <= 9) hipLaunchKernelGGL((k_pw_h16<9, F32OUT>), g, b, 0, st, a);
    else if (ns <= 12) hipLaunchKernelGGL((k_pw_h16<12, F32OUT>), g, b, 0, st, a);
    else if (ns <= 15) hipLaunchKernelGGL((k_pw_h16<15, F32OUT>), g, b, 0, st, a);
    else if (ns <= 18) hipLaunchKernelGGL((k_pw_h16<18, F32OUT>), g, b, 0, st, a);
    else hipLaunchKernelGGL((k_pw_h16<32, F32OUT>), g, b, 0, st, a);
}

inline bool mis16(const void *p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" {

int bev_dwconv_h16_psum_blocks(int Ho, int Wo, int C, int stride) {
    if (Ho <= 0 || Wo <= 0 || C <= 0 || C % 8 != 0 || C > 256 || (stride != 1 && stride != 2)) return BEV_ERR_ARGS;
    return dw16_blocks(Ho, Wo, C, stride);
}

int bev_dwconv2d_h16(const void *x, int N, int H, int W, int C, const void *wt, const float *bias, int K, int stride,
                     int pad, int act, void *y, int Ho, int Wo, float *psum, void *stream) {
    if (!x || !wt || !bias || !y || N < 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || C > 256 || pad < 0 ||
        act < 0 || act > 2)
        return BEV_ERR_ARGS;
    if ((K != 3 && K != 5) || (stride != 1 && stride != 2)) return BEV_ERR_ARGS;
    if (Ho != (H + 2 * pad - K) / stride + 1 || Wo != (W + 2 * pad - K) / stride + 1 || Ho <= 0 || Wo <= 0)
        return BEV_ERR_ARGS;
    if (mis16(x) || mis16(wt) || mis16(bias) || mis16(y) || mis16(psum) || x == y) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    const int nb = dw16_blocks(Ho, Wo, C, stride);
    const dim3 grid(nb, N), block(DW_NT);
    hipStream_t st = (hipStream_t)stream;
    const _Float16 *xh = (const _Float16 *)x, *wh = (const _Float16 *)wt;
    _Float16 *yh = (_Float16 *)y;
#define DW16(KK, SS, UU) \
    hipLaunchKernelGGL((k_dwconv_r16<KK, SS, UU>), grid, block, 0, st, xh, H, W, C, wh, bias, pad, act, yh, Ho, Wo, psum, nb)
    if (K == 3 && stride == 1) DW16(3, 1, true);
    else if (K == 3) DW16(3, 2, true);
    else if (stride == 1) DW16(5, 1, false);
    else DW16(5, 2, false);
#undef DW16
    return last();
}

int bev_ir_expand_dw_h16(const void *x, int N, int H, int W, int Ci, const void *we, const float *be, int Cm,
                         const void *wd, const float *bd, int K, int stride, void *y, int Ho, int Wo, float *psum,
                         void *stream) {
    if (!x || !we || !be || !wd || !bd || !y || !psum || N < 0 || H <= 0 || W <= 0 || Cm <= 0 || Cm % 48 != 0)
        return BEV_ERR_ARGS;
    if ((Ci != 16 && Ci != 24 && Ci != 32 && Ci != 40 && Ci != 48) || (K != 3 && K != 5) || (stride != 1 && stride != 2))
        return BEV_ERR_ARGS;
    const int pad = K / 2;
    if (Ho != (H + 2 * pad - K) / stride + 1 || Wo != (W + 2 * pad - K) / stride + 1 || Ho <= 0 || Wo <= 0)
        return BEV_ERR_ARGS;
    if (mis16(x) || mis16(we) || mis16(be) || mis16(bd) || mis16(y) || mis16(psum) || ((uintptr_t)wd & 1) != 0 || x == y)
        return BEV_ERR_ARGS;
    if ((int64_t)H * W * Ci >= ((int64_t)1 << 31) || (int64_t)Ho * Wo * Cm >= ((int64_t)1 << 31)) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    const int tc = (IR_IC - K) / stride + 1, strips = (Wo + tc - 1) / tc, segs = (Ho + IR_RSEG - 1) / IR_RSEG;
    const dim3 grid(strips * segs, N, Cm / 48), block(64 * IR_W);
    hipStream_t st = (hipStream_t)stream;
    const _Float16 *xh = (const _Float16 *)x, *weh = (const _Float16 *)we, *wdh = (const _Float16 *)wd;
    _Float16 *yh = (_Float16 *)y;
#define IRDW(KK, SS, CC)                                                                                              \
    hipLaunchKernelGGL((k_irdw_h16<KK, SS, CC>), grid, block, 0, st, xh, H, W, weh, be, wdh, bd, Cm, yh, Ho, Wo, psum, \
                       strips, segs)
#define IRDW_CI(KK, SS)                                                                                            \
    do {                                                                                                           \
        if (Ci == 16) IRDW(KK, SS, 16);                                                                            \
        else if (Ci == 24) IRDW(KK, SS, 24);                                                                       \
        else if (Ci == 32) IRDW(KK, SS, 32);                                                                       \
        else if (Ci == 40) IRDW(KK, SS, 40);                                                                       \
        else IRDW(KK, SS, 48);                                                                                     \
    } while (0)
    if (K == 3 && stride == 1) IRDW_CI(3, 1);
    else if (K == 3) IRDW_CI(3, 2);
    else if (stride == 1) IRDW_CI(5, 1);
    else IRDW_CI(5, 2);
#undef IRDW_CI
#undef IRDW
    return last();
}

int bev_conv2d_pw_h16(const void *x, int N, int H, int W, int Ci, const void *w, const float *bias, const float *gate,
                      const void *residual, int Co, void *y, int y_half, int ldy, void *stream) {
    if (!x || !w || !y || N < 0 || H <= 0 || W <= 0 || Ci <= 0 || Ci % 8 != 0 || Ci > 512 || Co <= 0 || Co % 8 != 0)
        return BEV_ERR_ARGS;
    if ((y_half != 0 && y_half != 1) || ldy < Co || ldy % 8 != 0) return BEV_ERR_ARGS;
    if (mis16(x) || mis16(w) || mis16(bias) || mis16(gate) || mis16(residual) || mis16(y)) return BEV_ERR_ARGS;
    if (y == x || y == residual) return BEV_ERR_ARGS;
    if (N == 0) return 0;
    PwArgs a;
    a.x = (const _Float16 *)x;
    a.w = (const _Float16 *)w;
    a.res = (const _Float16 *)residual;
    a.bias = bias;
    a.gate = gate;
    a.y = y;
    a.HW = (int64_t)H * W;
    a.M = a.HW * N;
    a.Ci = Ci;
    a.Co = Co;
    a.ldy = ldy;
    const int64_t blocks = (a.M + 127) / 128;
    if (blocks > 0x7fffffff) return BEV_ERR_ARGS;
    const dim3 grid((unsigned)blocks);
    const int ns = (Ci + 15) / 16;
    if (y_half) launch_pw<false>(ns, grid, (hipStream_t)stream, a);
    else launch_pw<true>(ns, grid, (hipStream_t)stream, a);
    return last();
}

}  // extern "C"
