// bev_conv_x6.hip -- fp32 convolutions on the bf16 matrix cores through an exact three-way operand split.
//
// Same contract as bev_conv2d_f32 (the timm trunk convs of CNNEncoder._encode_single, cnn_encoder.py:26,41-46):
//     y[m][n] = act( sum_k A[m][k] * W[k][n] + bias[n] (+ res[m][n]) )
// with fp32 operands and fp32 accumulation.  Every fp32 value v is written EXACTLY as the sum of three bf16
// values by round-to-nearest-even splitting:
//     h = bf16(v),  m = bf16(v - h),  l = bf16(v - h - m)        v == h + m + l  (8 + 8 + 8 significand bits;
// both subtractions are exact in fp32 because each residual is a multiple of ulp(v) below half an ulp of the
// previous term), |m| <= 2^-9 |v|, |l| <= 2^-18 |v|.
// Range of "EXACTLY" (tests/test_conv_value_domain_gpu.py): finite |v| < 0x7F7F8000 (~3.396e38) whose pieces stay
// bf16 / fp32 normals.  |v| >= 0x7F7F8000 (FLT_MAX is one) rounds to h = Inf, and then, as for v = +-Inf, r = v - h
// is NaN: a non-finite operand, or a finite one past that limit, gives NaN (not +-Inf) in every output of its
// receptive field and nowhere else -- non-finite in, non-finite out, never a finite wrong number (the ReLU epilogues
// keep a NaN, bev_act.h).  Measured on an MI355X: operands scaled by 2^-30 .. 2^30 each (outputs 2^-60 .. 2^60 times
// unit scale) give bit-identical scaled outputs; at 2^-50 x 2^-50 (outputs ~2^-100, the low planes' products fp32
// subnormal) and 2^50 x 2^50 the result still meets the 1e-5 max|ref| float64 bar (5.5e-7 seen, as at unit scale).
// A product a*b is then the sum of nine bf16 x bf16 products, each EXACT in fp32; six of them are kept (x6_dot below:
// which, in what order, and why the other three are dropped) and all of them accumulate into the fp32 MFMA
// accumulator.  The result is an fp32 GEMM whose per-product error (<= 2^-26 relative) is below the fp32 rounding of the running sum it is added to, so it is exactly as accurate as
// the exact-f32 MFMA path (tests/test_conv_x6_gpu.py measures both against float64), at 6 bf16 MFMAs per 16-deep
// k slice instead of 8 fp32 32x32x2 MFMAs per 16: v_mfma_f32_32x32x16_bf16 is 32 cycles, v_mfma_f32_32x32x2_f32
// 64 (MI355X_MICROARCH.md), so the matrix-core time per output falls from 512 to 192 cycles (2.67x).
// Summation order differs from the fp32 kernel: fp32-tolerance equal, not bitwise.
//
// Implicit GEMM, m = (image, oy, ox), n = output channel, k = (ky, kx, ci), NHWC activations with Ci % 16 == 0
// (a K step = one tap and 16 consecutive channels), or the dual-source 1x1 form of bev_conv2d_dual_f32 (bottleneck
// conv3 + downsample shortcut as one GEMM over K = [h | x[::s]]).  256 threads = WM x WN waves, each TM x TN MFMA
// tiles of 32 x 32.  Per K step the block stages A (global fp32 -> registers -> split -> three bf16 LDS planes) and
// B (weights split once at pack time: panel [Co_pad][K_pad / 16][3][16] bf16, one 96-B run per row and step);
// LDS rows of 24 bf16 (48 B = 3 odd 16-B slots: the 16-lane ds_read_b128 fragment groups are conflict-free);
// double-buffered LDS, two register sets prefetched two K steps ahead, one barrier per step.  Fragment map
// (cdna_hip_programming.md §3): lane l holds A[row l & 31][k 8 (l >> 5) + j] and B[k 8 (l >> 5) + j][col l & 31].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/bev_mi355x.h"
#include "bev_act.h"
#include "bev_mfma.h"
#include "bev_tune.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int XBK = 16;   // K step
constexpr int XROW = 24;  // bf16 per LDS row (48 B)

__device__ __attribute__((aligned(16))) float g_xzero4[4] = {0.f, 0.f, 0.f, 0.f};  // never written

__host__ __device__ inline int64_t kpad_x(int K) { return (K + XBK - 1) / XBK * XBK; }
__host__ __device__ inline int64_t copad_x(int Co) { return (Co + 127) / 128 * 128; }

// v == h + m + l exactly (see the header); RNE conversions (v_cvt_pk_bf16_f32), exact fp32 residuals.
__device__ __forceinline__ void split3(float v, __bf16 &h, __bf16 &m, __bf16 &l) {
    h = (__bf16)v;
    const float r = v - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

// split3 of two elements at once: the same RNE conversions and exact fp32 differences in the same order, written on
// vectors so that every conversion is one half of a v_cvt_pk_bf16_f32 and every pair of subtractions one v_pk_add_f32
// (bit-identical to split3 per element, NaN / Inf / subnormal included: tests/test_conv_x6_buf_gpu.py).
__device__ __forceinline__ void split3x2(f32x2 v, bf16x2 &h, bf16x2 &m, bf16x2 &l) {
    h = __builtin_convertvector(v, bf16x2);
    const f32x2 r = v - __builtin_convertvector(h, f32x2);
    m = __builtin_convertvector(r, bf16x2);
    l = __builtin_convertvector(r - __builtin_convertvector(m, f32x2), bf16x2);
}
// ... of a float4, as the three bf16x4 that the staging and the split epilogue store
__device__ __forceinline__ void split3x4(f32x4 v, bf16x4 &h, bf16x4 &m, bf16x4 &l) {
    bf16x2 h0, m0, l0, h1, m1, l1;
    split3x2((f32x2){v[0], v[1]}, h0, m0, l0);
    split3x2((f32x2){v[2], v[3]}, h1, m1, l1);
    h = __builtin_shufflevector(h0, h1, 0, 1, 2, 3);
    m = __builtin_shufflevector(m0, m1, 0, 1, 2, 3);
    l = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
}

// Operand staging by raw buffer loads (k_conv_x6 / k_conv_x6b, BUFA).  One descriptor per operand and workgroup, built
// from readfirstlane'd halves so that the compiler holds it in SGPRs (no waterfall loop around the loads).  The range
// check of a raw buffer covers the VGPR offset alone, not the SGPR soffset: a lane that must not load carries
// X6_VOUT, out of range of any descriptor of at most 2^31 - 16 bytes, and the hardware returns zeros -- no pointer
// select, no branch.
template <int PB>
__device__ __forceinline__ auto x6_bload(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    if constexpr (PB == 16) return __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, 0);
    else return __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, 0);
}
constexpr int X6_VOUT = (int)0x80000000;
constexpr int64_t X6_BUF_MAX = ((int64_t)1 << 31) - 16;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x6_rsrc(const void *p, int64_t bytes) {
    const uint64_t u = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    const int nb = __builtin_amdgcn_readfirstlane((int)(bytes < X6_BUF_MAX ? bytes : X6_BUF_MAX));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
}

// The split product of one 16-deep k slice, c += A B for a 32 x 32 tile: six v_mfma_f32_32x32x16_bf16 over the planes
// a[p], b[p] (p = 0, 1, 2: h, m, l), in the order
//     hh + hm + mh + hl + lh + mm          (dropped: ml + lm + ll <= 2^-26 |a b|, below fp32's 2^-24 rounding)
// -- the six of the nine plane products that are larger than 2^-27 |a b|.  Every kernel of this file forms its
// products here and nowhere else: the one order is what makes the chain kernels bit-identical to the two launches they
// replace, and k_conv_x6s (pre-split operand) to k_conv_x6 / k_conv_x6b (fp32 operand split while staging).
__device__ __forceinline__ void x6_dot(f32x16 &c, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
}

// OIHW fp32 -> split panel in MFMA B-fragment order: [Co_pad / 32][K_pad / 16][plane h, m, l][lane 64][8] bf16,
// lane l of the (32-column block, 16-deep slice, plane) fragment holds W[32 cb + (l & 31)][16 s + 8 (l >> 5) + j],
// j = 0..7 -- one coalesced 1-KiB load per wave and fragment (k = (ky*KW + kx)*Ci + ci).
__host__ __device__ inline int64_t frag_index(int n, int k, int p, int64_t S) {
    return (((int64_t)(n >> 5) * S + (k >> 4)) * 3 + p) * 512 + (((k >> 3) & 1) * 32 + (n & 31)) * 8 + (k & 7);
}

__global__ void k_pack_x6(const float *__restrict__ w, int Co, int Ci, int KH, int KW, int64_t Kp, int64_t Cop,
                          __bf16 *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Kp * Cop) return;
    const int n = (int)(t / Kp);
    const int k = (int)(t % Kp);
    const int K = Ci * KH * KW;
    float v = 0.0f;
    if (n < Co && k < K) {
        const int ci = k % Ci, r = k / Ci, kx = r % KW, ky = r / KW;
        v = w[(((int64_t)n * Ci + ci) * KH + ky) * KW + kx];
    }
    __bf16 h, m, l;
    split3(v, h, m, l);
    const int64_t S = Kp / XBK;
    out[frag_index(n, k, 0, S)] = h;
    out[frag_index(n, k, 1, S)] = m;
    out[frag_index(n, k, 2, S)] = l;
}

struct ConvX {  // filled by conv_x6()
    const float *__restrict__ x = nullptr;
    const __bf16 *__restrict__ wp = nullptr;
    const float *__restrict__ bias = nullptr;
    const float *__restrict__ res = nullptr;
    float *__restrict__ y = nullptr;
    int N = 0, H = 0, W = 0, Ci = 0, Co = 0, KH = 0, KW = 0, stride = 0, pad = 0, dil = 0, Ho = 0, Wo = 0, act = 0,
        ldy = 0, Kp = 0;
    int64_t M = 0;
    // dual-source 1x1: k in [Ci, Ci + Ci2) reads x2 [N][H2][W2][Ci2] at (oy*stride2, ox*stride2)
    const float *__restrict__ x2 = nullptr;
    int Ci2 = 0, H2 = 0, W2 = 0, stride2 = 0;
    // pre-split operand / output planes: xs [3][N][H][W][Ci], ys [3][M][Co] bf16 (plane strides xps / yps)
    const __bf16 *__restrict__ xs = nullptr;
    __bf16 *__restrict__ ys = nullptr;
    int64_t xps = 0, yps = 0;
    // chained pointwise conv (k_conv_x6b CHAIN): y = act2(h (*) W2 + bias2 + res), h = act(this conv + bias)
    const __bf16 *__restrict__ wp2 = nullptr;
    const float *__restrict__ bias2 = nullptr;
    int Co2 = 0, act2 = 0;
    // the next block's 1x1 conv1 in the chain's epilogue (x6_chain_epilogue NXT): ys = act3(y (*) W3' + bias3), split
    const __bf16 *__restrict__ wp3 = nullptr;
    const float *__restrict__ bias3 = nullptr;
    int Co3 = 0, act3 = 0;
    int nta = 0;  // 1: A (activation) loads non-temporal (BEV_TUNE_CONV_X6_NT, the last layer of a trunk)
};

// A run-time activation code as a compile-time one: dispatched once per kernel (wave-uniform), so the element
// loops that apply it carry no scalar branch.
template <int ACT>
__device__ __forceinline__ float act_c(float t) {
    if constexpr (ACT == 2) return silu_hw(t);
    else if constexpr (ACT == 1) return relu_f(t);
    else return t;
}

template <class F>
__device__ __forceinline__ void act_dispatch(int act, F &&f) {
    if (act == 2) f(std::integral_constant<int, 2>{});
    else if (act == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

// The wave's (TM*32) x (TN*32) accumulator tile goes through LDS, 32 rows per pass (4 * 32 * (TN * 32 + 4) floats
// for the block), so every lane stores whole float4 row pieces; each pass issues all its residual loads at once (the
// memory-bound 1x1 layers).  Same scheme as bev_conv.hip's epilogue.  With a.ys the result is stored split.
template <int TN>
__host__ __device__ constexpr int x6_epi_bytes() { return 4 * 32 * (TN * 32 + 4) * 4; }

template <int TM, int TN>
__device__ __forceinline__ void x6_epilogue(const ConvX &a, float *lds, const f32x16 (&acc)[TM][TN], int wave,
                                            int lane, int wn, int wm, int64_t m0, int n0) {
    const int r32 = lane & 31, h = lane >> 5;
    constexpr int WC = TN * 32, ER = WC + 4;
    constexpr int C4 = WC / 4, RPI = 64 / C4, NQ = 32 / RPI;
    float *E = lds + wave * (32 * ER);
    const int c4 = lane % C4, rq = lane / C4;
    const int n = n0 + wn * WC + c4 * 4;
    const bool nvec = ((a.Co & 3) == 0) && ((a.ldy & 3) == 0) && (n + 3 < a.Co);
    // each pass's residual loads go out before its LDS traffic (the first pass's before the barrier)
    float4 rv[NQ];
    auto res_load = [&](int i) {
        const int64_t mb = m0 + wm * TM * 32 + i * 32;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int64_t m = mb + rq + RPI * q;
            rv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.res && m < a.M && nvec) rv[q] = *(const float4 *)(a.res + m * a.Co + n);
        }
    };
    res_load(0);
    __syncthreads();  // every wave is done with the staging buffers
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) {
        if (nvec) bv = *(const float4 *)(a.bias + n);
        else {
            bv.x = n < a.Co ? a.bias[n] : 0.f;
            bv.y = n + 1 < a.Co ? a.bias[n + 1] : 0.f;
            bv.z = n + 2 < a.Co ? a.bias[n + 2] : 0.f;
            bv.w = n + 3 < a.Co ? a.bias[n + 3] : 0.f;
        }
    }
    act_dispatch(a.act, [&](auto ac) {  // the activation is a compile-time constant of the element loops
        constexpr int ACT = decltype(ac)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // same-wave LDS operations complete in order: the previous pass's reads precede these writes
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) E[((r & 3) + 8 * (r >> 2) + 4 * h) * ER + j * 32 + r32] = acc[i][j][r];
            const int64_t mbase = m0 + wm * TM * 32 + i * 32;
            if (i > 0) res_load(i);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int row = rq + RPI * q;
                const int64_t m = mbase + row;
                if (m >= a.M) continue;
                const float4 v = *(const float4 *)(E + row * ER + c4 * 4);
                float o[4] = {v.x + bv.x, v.y + bv.y, v.z + bv.z, v.w + bv.w};
                if (a.ys) {  // split output planes (the next conv's pre-split operand); ldy == Co, Co % 4 == 0
                    if (a.res) {
                        const float4 rr = rv[q];
                        o[0] += rr.x, o[1] += rr.y, o[2] += rr.z, o[3] += rr.w;
                    }
                    bf16x4 hv, mv, lv;
                    split3x4((f32x4){act_c<ACT>(o[0]), act_c<ACT>(o[1]), act_c<ACT>(o[2]), act_c<ACT>(o[3])}, hv, mv,
                             lv);
                    __bf16 *yp = a.ys + m * a.Co + n;
                    if (n < a.Co) {
                        *(bf16x4 *)yp = hv;
                        *(bf16x4 *)(yp + a.yps) = mv;
                        *(bf16x4 *)(yp + 2 * a.yps) = lv;
                    }
                    continue;
                }
                float *yp = a.y + m * a.ldy + n;
                if (nvec) {
                    if (a.res) {
                        o[0] += rv[q].x;
                        o[1] += rv[q].y;
                        o[2] += rv[q].z;
                        o[3] += rv[q].w;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) o[u] = act_c<ACT>(o[u]);
                    *(float4 *)yp = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (n + u >= a.Co) break;
                        float t = o[u];
                        if (a.res) t += a.res[m * a.Co + n + u];
                        yp[u] = act_c<ACT>(t);
                    }
                }
            }
        }
    });
}

// The addressing of BUFA's A rows, shared by k_conv_x6 and k_conv_x6b.  The descriptor of x starts at the first image
// the tile touches (n_first = m0 / (Ho Wo)) MINUS the bytes of pad rows and pad pixels, xbias = pad (W + 1) Ci 4: a
// row's VGPR offset at tap (0, 0), ((n - n_first) H W + iy0 W + ix0) Ci 4 + xbias, is then never negative, the tap
// and channel part ((ky dil W + kx dil) Ci + ci0) 4 travels in soffset, and the two add up to an address inside the
// tensor for every lane that is not masked (the bytes in front of the tensor are never read).  conv_x6() sends a
// call here only if the images one tile can touch, plus xbias, stay below 2^31 - 16 bytes; num_records runs to the
// tensor's end or to that cap.  Dual form: x2 [N][H2][W2][Ci2], no padding, a descriptor of its own.
// lin: x is read as the matrix [M][Ci] (1x1 / stride 1 / pad 0, and the dual form's x) -- output row m reads operand
// row m, so the descriptor starts at the tile's own first row m0 (inside the first image the tile touches: the size
// rule holds all the more), a row's offset is (m - m0) Ci 4, and the kernel's prologue divides nothing: neither
// n_first nor a row's (n, oy, ox) is needed.
struct X6Desc {
    __amdgpu_buffer_rsrc_t rx, rx2;
    int64_t n_first;
    int xbias;
    bool lin;
};
template <bool DUAL>
__device__ __forceinline__ X6Desc x6_desc(const ConvX &a, int64_t m0) {
    X6Desc d;
    d.lin = DUAL || (a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0);
    d.n_first = 0;
    d.xbias = 0;
    if (d.lin) {
        d.rx = x6_rsrc(a.x + m0 * a.Ci, (a.M - m0) * a.Ci * 4);
    } else {
        d.n_first = m0 / ((int64_t)a.Ho * a.Wo);
        d.xbias = a.pad * (a.W + 1) * a.Ci * 4;
        const int64_t img = (int64_t)a.H * a.W * a.Ci * 4;
        d.rx = x6_rsrc((const char *)a.x + d.n_first * img - d.xbias, (a.N - d.n_first) * img + d.xbias);
    }
    if (DUAL) {
        d.n_first = m0 / ((int64_t)a.Ho * a.Wo);
        const int64_t img2 = (int64_t)a.H2 * a.W2 * a.Ci2 * 4;
        d.rx2 = x6_rsrc((const char *)a.x2 + d.n_first * img2, (a.N - d.n_first) * img2);
    } else {
        d.rx2 = d.rx;
    }
    return d;
}

template <int WM, int WN, int TM, int TN, bool DUAL, bool BUFA = false>
__global__ __launch_bounds__(256, 2) void k_conv_x6(ConvX a) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int APL = BM * XROW, BPL = BN * XROW;  // bf16 per operand plane
    constexpr int STAGE = 3 * (APL + BPL);            // bf16 per LDS stage
    constexpr int AQ = BM / 64;                       // A float4 per thread and K step: rows tid / 4 + 64 q
    // B staging: the step's BN rows x 96 B in pieces of PB bytes (16, or 8 when 16-B pieces do not divide evenly
    // over the 256 threads), BQ whole pieces per thread -- no conditional loads
    constexpr int PB = ((BN * 6) % 256 == 0) ? 16 : 8;
    constexpr int PPR = 96 / PB;  // pieces per row
    constexpr int BQ = BN * PPR / 256;
    static_assert(BN * PPR % 256 == 0, "B pieces per thread");
    typedef typename std::conditional<PB == 16, u32x4, u32x2>::type bpiece;  // native vectors stay in VGPRs
    constexpr int EPIB = x6_epi_bytes<TN>();
    constexpr int LDSB = (2 * STAGE * 2 > EPIB) ? 2 * STAGE * 2 : EPIB;
    static_assert(BM % 64 == 0, "A staging rows");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDSB];
    __bf16 *lds = (__bf16 *)lds_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (SGPR)
    const int wm = wave / WN, wn = wave % WN;
    const int n_tiles = (a.Co + BN - 1) / BN;
    const unsigned bid = xcd_block(blockIdx.x, gridDim.x);  // the n_tiles blocks of the same A rows on one XCD
    const int64_t m0 = (int64_t)(bid / n_tiles) * BM;
    const int n0 = (bid % n_tiles) * BN;

    // A staging rows: (tid >> 2) + 64 q, channel quad aq of the 16-channel K step
    const int aq = tid & 3;
    int64_t pb[AQ], p2[AQ];
    int iy0[AQ], ix0[AQ];
    bool rok[AQ];
    // BUFA: row q's byte offsets at tap (0, 0) in x / x2 (see X6Desc), and the offset its next load uses: vr, or
    // X6_VOUT while the row (m >= M) or its tap (outside the image) reads zeros
    X6Desc dsc;
    if constexpr (BUFA) dsc = x6_desc<DUAL>(a, m0);
    unsigned vr[AQ], vr2[AQ];
    int vo[AQ], vo2[AQ];
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
        const int64_t m = m0 + (tid >> 2) + 64 * q;
        rok[q] = m < a.M;
        if constexpr (BUFA && !DUAL) {
            if (dsc.lin) {  // wave-uniform: no division in this prologue
                vr[q] = (unsigned)((tid >> 2) + 64 * q) * (unsigned)a.Ci * 4u + 16u * aq;
                vr2[q] = 0;
                iy0[q] = ix0[q] = 0;
                pb[q] = p2[q] = 0;
                continue;
            }
        }
        const int64_t mm = rok[q] ? m : 0;
        const int ox = (int)(mm % a.Wo);
        const int64_t t = mm / a.Wo;
        const int oy = (int)(t % a.Ho);
        const int64_t n = t / a.Ho;
        if (DUAL) {
            pb[q] = mm * a.Ci + 4 * aq;
            p2[q] = ((n * a.H2 + (int64_t)oy * a.stride2) * a.W2 + (int64_t)ox * a.stride2) * a.Ci2 + 4 * aq;
            iy0[q] = ix0[q] = 0;
        } else {
            pb[q] = n * a.H * a.W * a.Ci + 4 * aq;
            p2[q] = 0;
            iy0[q] = oy * a.stride - a.pad;
            ix0[q] = ox * a.stride - a.pad;
        }
        if constexpr (BUFA) {  // 32-bit byte offsets from the descriptors' bases (wrapping arithmetic for dead rows)
            const unsigned nr = (unsigned)(int)(n - dsc.n_first);
            if (DUAL) {
                vr[q] = (unsigned)(int)(m - m0) * (unsigned)a.Ci * 4u + 16u * aq;
                vr2[q] = ((nr * a.H2 + (unsigned)(oy * a.stride2)) * a.W2 + (unsigned)(ox * a.stride2)) *
                             (unsigned)a.Ci2 * 4u + 16u * aq;
            } else {
                vr[q] = ((nr * a.H + (unsigned)iy0[q]) * a.W + (unsigned)ix0[q]) * (unsigned)a.Ci * 4u + 16u * aq +
                        (unsigned)dsc.xbias;
                vr2[q] = 0;
            }
        }
    }
    const int64_t bstep = 3 * 512;  // bf16 per 16-deep slice of a 32-column block (fragment-order panel)
    const __bf16 *brow[BQ];
    int bvo[BQ];
    __amdgpu_buffer_rsrc_t rw;
    if constexpr (BUFA) rw = x6_rsrc(a.wp, copad_x(a.Co) * (int64_t)a.Kp * 6);
    int bdst[BQ];  // LDS offset (bf16) of the piece inside the B part of a stage
#pragma unroll
    for (int i = 0; i < BQ; ++i) {
        const int pc = tid + 256 * i;
        const int row = pc / PPR, byte = (pc % PPR) * PB;  // byte of the row's 96-B (plane, 16 k) run
        const int pl = byte / 32, hk = (byte % 32) / 16, sub = (byte % 16) / 2;
        brow[i] = a.wp + frag_index(n0 + row, 8 * hk, pl, a.Kp / XBK) + sub;
        bvo[i] = (int)((frag_index(n0 + row, 8 * hk, pl, a.Kp / XBK) + sub) * 2);  // BUFA: its byte offset in the panel
        bdst[i] = pl * BPL + row * XROW + 8 * hk + sub;
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};

    f32x4 va0[AQ], va1[AQ];
    bpiece vb0[BQ], vb1[BQ];
    int ky = 0, kx = 0, ci0 = 0, k0 = 0;  // tap / channel (or dual k) of the step being loaded
    int64_t kb = 0;                       // bf16 offset of that step in a panel row
    // BUFA: the byte offset of tap (ky, kx) (wave-uniform, for soffset) and the rows' validity there -- once per tap,
    // Ci / 16 K steps share it; a 1x1 conv computes it here and never again
    int soff = 0;
    auto x6_tap = [&]() {
        const int dy = ky * a.dil, dx = kx * a.dil;
        soff = (dy * a.W + dx) * a.Ci * 4;
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int iy = iy0[q] + dy, ix = ix0[q] + dx;
            // & not &&: three compares and one select, no branch and no exec-masked region
            const bool in = rok[q] & ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            vo[q] = in ? (int)vr[q] : X6_VOUT;
            vo2[q] = rok[q] ? (int)vr2[q] : X6_VOUT;
        }
    };
    if constexpr (BUFA) x6_tap();
#define X6_GLOAD(VA, VB)                                                                                   \
    do {                                                                                                   \
        if constexpr (BUFA) {                                                                              \
            if (DUAL) {                                                                                    \
                if (k0 < a.Ci) {                                                                           \
                    _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] = __builtin_bit_cast(             \
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(dsc.rx, vo[q], k0 * 4, 0));           \
                } else {                                                                                   \
                    _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] = __builtin_bit_cast(             \
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(dsc.rx2, vo2[q], (k0 - a.Ci) * 4, 0)); \
                }                                                                                          \
                k0 += XBK;                                                                                 \
            } else {                                                                                       \
                _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] = __builtin_bit_cast(                 \
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(dsc.rx, vo[q], soff, 0));                 \
                soff += XBK * 4;                                                                           \
                ci0 += XBK;                                                                                \
                if (ci0 == a.Ci) {                                                                         \
                    ci0 = 0;                                                                               \
                    if (++kx == a.KW) {                                                                    \
                        kx = 0;                                                                            \
                        ++ky;                                                                              \
                    }                                                                                      \
                    x6_tap();                                                                              \
                }                                                                                          \
            }                                                                                              \
            _Pragma("unroll") for (int i = 0; i < BQ; ++i) VB[i] = __builtin_bit_cast(                     \
                bpiece, x6_bload<PB>(rw, bvo[i], (int)kb * 2));                                            \
            kb += bstep;                                                                                   \
            break;                                                                                         \
        }                                                                                                  \
        if (DUAL) {                                                                                        \
            const bool first = k0 < a.Ci;                                                                  \
            const float *src = first ? a.x + k0 : a.x2 + (k0 - a.Ci);                                      \
            _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] =                                         \
                *(const f32x4 *)(rok[q] ? src + (first ? pb[q] : p2[q]) : g_xzero4);                      \
            k0 += XBK;                                                                                     \
        } else {                                                                                           \
            const int dy = ky * a.dil, dx = kx * a.dil;                                                    \
            _Pragma("unroll") for (int q = 0; q < AQ; ++q) {                                               \
                const int iy = iy0[q] + dy, ix = ix0[q] + dx;                                              \
                const bool in = rok[q] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;    \
                VA[q] = *(const f32x4 *)(in ? a.x + pb[q] + ((int64_t)iy * a.W + ix) * a.Ci + ci0 : g_xzero4); \
            }                                                                                              \
            ci0 += XBK;                                                                                    \
            if (ci0 == a.Ci) {                                                                             \
                ci0 = 0;                                                                                   \
                if (++kx == a.KW) {                                                                        \
                    kx = 0;                                                                                \
                    ++ky;                                                                                  \
                }                                                                                          \
            }                                                                                              \
        }                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < BQ; ++i) VB[i] = *(const bpiece *)(brow[i] + kb);          \
        kb += bstep;                                                                                       \
    } while (0)
#define X6_SWRITE(BUF, VA, VB)                                                                             \
    do {                                                                                                   \
        __bf16 *As = lds + (BUF) * STAGE;                                                                  \
        __bf16 *Bs = As + 3 * APL;                                                                         \
        _Pragma("unroll") for (int q = 0; q < AQ; ++q) {                                                   \
            bf16x4 hv, mv, lv;                                                                             \
            split3x4(VA[q], hv, mv, lv);                                                                   \
            __bf16 *d = As + ((tid >> 2) + 64 * q) * XROW + 4 * aq;                                        \
            *(bf16x4 *)d = hv;                                                                             \
            *(bf16x4 *)(d + APL) = mv;                                                                     \
            *(bf16x4 *)(d + 2 * APL) = lv;                                                                 \
        }                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < BQ; ++i) *(bpiece *)(Bs + bdst[i]) = VB[i];                \
    } while (0)
    const int r32 = lane & 31, h = lane >> 5;
    // one 16-deep k slice: x6_dot per (A tile, B tile) pair
#define X6_MFMA(BUF)                                                                                       \
    do {                                                                                                   \
        const __bf16 *As = lds + (BUF) * STAGE;                                                            \
        const __bf16 *Bs = As + 3 * APL;                                                                   \
        bf16x8 fa[TM][3], fb[TN][3];                                                                       \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
            _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                  \
                fa[i][p] = *(const bf16x8 *)(As + p * APL + (wm * TM * 32 + i * 32 + r32) * XROW + 8 * h); \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
            _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                  \
                fb[j][p] = *(const bf16x8 *)(Bs + p * BPL + (wn * TN * 32 + j * 32 + r32) * XROW + 8 * h); \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
                x6_dot(acc[i][j], fa[i], fb[j]);                                                           \
    } while (0)

    const int nk = a.Kp / XBK;
    X6_GLOAD(va0, vb0);
    if (nk > 1) X6_GLOAD(va1, vb1);
    X6_SWRITE(0, va0, vb0);
    __syncthreads();
    // Invariant at the loop head: LDS buffer 0 holds step ks, register set 1 holds step ks + 1.
    int ks = 0;
    for (; ks + 3 < nk; ks += 2) {
        X6_GLOAD(va0, vb0);  // step ks + 2
        X6_MFMA(0);
        X6_SWRITE(1, va1, vb1);  // step ks + 1 (buffer 1's readers passed the last barrier)
        __syncthreads();
        X6_GLOAD(va1, vb1);  // step ks + 3
        X6_MFMA(1);
        X6_SWRITE(0, va0, vb0);  // step ks + 2
        __syncthreads();
    }
    if (ks + 2 < nk) {
        X6_GLOAD(va0, vb0);
        X6_MFMA(0);
        X6_SWRITE(1, va1, vb1);
        __syncthreads();
        X6_MFMA(1);
        X6_SWRITE(0, va0, vb0);
        __syncthreads();
        X6_MFMA(0);
    } else if (ks + 1 < nk) {
        X6_MFMA(0);
        X6_SWRITE(1, va1, vb1);
        __syncthreads();
        X6_MFMA(1);
    } else {
        X6_MFMA(0);
    }
#undef X6_MFMA
#undef X6_SWRITE
#undef X6_GLOAD
    x6_epilogue<TM, TN>(a, (float *)lds_raw, acc, wave, lane, wn, wm, m0, n0);
}

// ---------------------------------------------------------------------------
// Chained bottleneck body in the split arithmetic (bev_conv2d_chain_x6_f32): timm Bottleneck without a downsample,
// act3(bn3(conv3(act2(bn2(conv2(h1))))) + x).  The block's BM x BN tile of h2 = act(conv2 + b2) holds EVERY channel
// of h2 for its BM pixels (BN == Co), so it is split once into three bf16 planes in LDS ([3][BM][BN + 8]: rows of
// odd 16-B slot counts) and conv3 (1x1, K2 = BN) runs on it there: h2 never makes its HBM round trip.  Each wave
// takes a 32-row band and walks Co2 in 32-column blocks; the W3 fragments reach it through LDS (LDS-DMA from the
// fragment-order panel, one step ahead); a block's residual is loaded one block ahead; residual and output are
// addressed by buffer instructions (row in the VGPR offset, so rows past M read 0 / are dropped).
// ---------------------------------------------------------------------------
// this wave's older vector-memory operations have completed except the newest N (vmcnt retires in issue order), its
// LDS reads have returned, and every wave of the workgroup has got here
template <int N>
__device__ __forceinline__ void x6_wait_barrier() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// LDS of a chain kernel's epilogue: the three h2 planes, then one W3 stage (the second stage overlays the planes
// once every wave holds its h2 fragments in registers): WPB column blocks x 4 slices x 3 planes of 1 KiB
template <int BM, int BN>
__host__ __device__ constexpr int x6_chain_lds_bytes() { return 3 * BM * (BN + 8) * 2 + (4 / (BM / 32)) * 12288; }

// The chain epilogue.  h2 = act(conv2 + b2) is split into the three LDS planes; every wave then takes the h2
// fragments of its 32-row band (all S2 slices, three planes) into registers ONCE and walks Co2 in 32-column blocks:
// wave = (band, part), part = which of the WPB column blocks of a step (WPB = 2 for the 64-row tile, so the four
// waves of a workgroup always work on the same W3 stage and the panel is read once per tile).  The W3 panel (the
// dual's [W3 | Wds]) reaches the MFMAs through LDS: a step = 4 slices x WPB column blocks = 12 WPB fragment runs
// of 1 KiB, copied by LDS-DMA one step ahead into one of two stages and read back as ds_read_b128, so no MFMA waits
// on a vector-memory load of its own.  The stages: [HB, HB + 12 WPB KiB) after the planes, and [0, 12 WPB KiB) over
// the planes, which are dead once the fragments are in registers (the barrier of step 0 orders the two).
// Issue order per step s (the vmcnt waits below count on it; vmcnt retires in issue order):
//     wait for this wave's DMAs of step s, barrier | DMAs of step s + 1 | first step of a block: bias2 + residual
//     of the NEXT block | 24 MFMAs | last step of a block: the block's 16 stores.
// The wait in front of step s therefore leaves in flight exactly what was issued after the DMAs of step s: the
// previous block's stores and the look-ahead residual are never drained in front of an MFMA, and a residual load
// has two steps of MFMAs to arrive.  The residual sits in two register sets used alternately (no copies).
// X2S > 0: the dual form (block 0 of a stage, bev_conv2d_chain_dual_x6_f32): conv3's K continues with the X2S
// 16-deep slices of the shortcut operand x2 at the lane row's strided pixel (the 1x1 downsample), split in registers
// once per wave and reused by every block; the panel is the dual tail's [W3 | Wds].
// Per output element: slices ascending, the six products of a slice in the mainloop's order, (acc + bias2) +
// residual, then act2 -- the separate launches' arithmetic.
// NXT > 0 (the 128 x 64 tile, one step per block; bev_conv2d_chain_conv1_x6_f32): the NEXT block's 1x1 conv1 over
// y, NXT output channels, runs here too, so y is not read back for it.  A wave's 32 x 32 block of y belongs to the 32
// rows whose conv1 output it computes, and the block's 32 channels are two 16-deep slices of conv1's K: the block's
// o (the stored values) is split (split3x2), written as three bf16 planes [32][40] (80-B rows: 5 odd 16-B slots)
// into a wave-private LDS area and read back as the A fragments of the two slices -- a same-wave round trip, LDS
// operations of one wave complete in order, no barrier -- then 6 NXT / 32 MFMAs per slice against conv1's panel
// fragments accumulate into accn.  K order of conv1: blocks ascending, the two slices ascending, x6_dot's products:
// a 1x1 k_conv_x6b / k_conv_x6s over the same K does exactly that, so h' is bit-identical to the separate launch.
// conv1's panel runs of a step (2 slices x NXT / 32 column blocks x 3 planes of 1 KiB) are staged like W3, by DMAs
// issued right behind the step's W3 DMAs into a stage next to the W3 stage.  LDS after the fragments are taken:
//     [0, 12 K) W3 stage 1 | [12 K, 24 K) conv1 stage 1 | [24 K, 54 K) four y blocks of 7.5 KiB | HB = 54 K:
//     W3 stage 0 | conv1 stage 0 | 78 K
// Issue order per step with NXT: wait, barrier | W3 DMAs of step s + 1 | conv1 DMAs of step s + 1 | bias2 + residual
// of the next block | 24 MFMAs | 16 stores | y block through LDS (lgkmcnt only) | 6 NXT / 16 MFMAs.  Behind a step's
// DMAs (both kinds together) there are still the R look-ahead loads and the 16 stores: the count R + 16 holds.
// After the last block: h' = act3(accn + bias3), split, through the same LDS area as 16-B row pieces to the three
// planes of ys; rows at or past M are not stored.
template <int WM, int WN, int TM, int TN, int X2S = 0, int NXT = 0>
__device__ __forceinline__ void x6_chain_epilogue(const ConvX &a, unsigned char *lds_raw, const f32x16 (&acc)[TM][TN],
                                                  int wave, int lane, int wm, int wn, int64_t m0) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32, HR = BN + 8, HPL = BM * HR;
    constexpr int NB = BM / 32, WPB = 4 / NB;  // 32-row bands; waves per band (each one column block of a step)
    static_assert(NB * WPB == 4, "chain epilogue: 4 waves over the 32-row bands");
    constexpr int S2 = BN / 16;   // 16-deep slices of conv3's K from h2
    constexpr int ST = S2 + X2S;  // slices of the panel
    constexpr int U = ST / 4;     // steps (4 slices) per column block
    static_assert(ST % 4 == 0, "chain epilogue: whole 4-slice steps");
    constexpr int HB = 3 * HPL * 2;  // bytes of the h2 planes = offset of W3 stage 0
    constexpr int PW = WPB * 3;      // 1-KiB DMA pieces per wave and step
    static_assert(HB % 1024 == 0, "W3 stage 0 starts on a fragment boundary");
    // the next conv: NJ column blocks of 32, a stage of 2 NJ 3 fragment runs, y blocks of three [32][YP] planes
    constexpr int NJ = NXT / 32, W3B = 12 * WPB * 1024, NXB = 6 * NJ * 1024, YP = 40, YPL = 32 * YP;
    constexpr int YB0 = W3B + NXB, YBW = 3 * YPL * 2;  // first y block, bytes per wave
    static_assert(NXT == 0 || (NXT % 64 == 0 && WPB == 1 && U == 1 && X2S == 0), "next conv: the 128 x 64 plain chain");
    static_assert(NXT == 0 || YB0 + 4 * YBW <= HB, "stages 1 and the y blocks overlay the dead h2 planes");
    __bf16 *H = (__bf16 *)lds_raw;
    const int r32 = lane & 31, hh = lane >> 5;
    const int band = (wave % NB) * 32, part = wave / NB;
    const int64_t rows = (a.M - m0 < BM) ? a.M - m0 : BM;
    const int64_t base = m0 * a.Co2;
    const float *resp = a.res ? a.res + base : a.y + base;
    const float *biasp = a.bias2 ? a.bias2 : a.y;
    const int64_t resb = rows * a.Co2 * 4, biasb = a.bias2 ? (int64_t)a.Co2 * 4 : 0;  // no bias2: an empty buffer (0)
    const int vo = ((band + 4 * hh) * a.Co2 + r32) * 4;  // lane part of a res / y address
    const int NG = a.Co2 / (32 * WPB);                    // column blocks of this wave: 32 (g WPB + part), g < NG
    // bias2 ([16]) and residual ([0..15], HR) of the wave's block at column c0.  !live (the look-ahead of the last
    // block): the same instructions on empty buffers -- no memory access, and the loop's vmcnt counts hold as they are
    auto res_load = [&](auto hr, int c0, float(&rv)[17], bool live) {
        const __amdgpu_buffer_rsrc_t rr = buffer_rsrc(resp, live ? resb : 0);
        const __amdgpu_buffer_rsrc_t rb = buffer_rsrc(biasp, live ? biasb : 0);
        rv[16] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, r32 * 4, c0 * 4, 0));
        if constexpr (decltype(hr)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                rv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                      rr, vo + ((r & 3) + 8 * (r >> 2)) * a.Co2 * 4, c0 * 4, 0));
        }
    };
    const unsigned lbase = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(lds_raw));
    const __bf16 *wsrc = a.wp2 + lane * 8;
    // this wave's share of step (g, u)'s fragment runs -> the stage at byte sbo: piece q = (column block of the
    // step, slice of the step, plane) is panel run ((g WPB + cbl) ST + 4 u) 3 + q % 12
    auto issue_w3 = [&](int g, int u, unsigned sbo) {
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int q = wave + 4 * i, cbl = q / 12, r = q % 12;
            lds_dma16(wsrc + (((int64_t)(g * WPB + cbl) * ST + 4 * u) * 3 + r) * 512,
                      lbase + sbo + (unsigned)(q * 1024));
        }
    };
    // NXT: this wave's share of the next conv's runs for y block g (slices 2 g, 2 g + 1 of its K = Co2) -> the stage
    // behind the W3 stage at sbo: piece q = (column block, slice, plane) is panel run ((cb S3 + 2 g) 3 + q % 6)
    const __bf16 *nsrc = a.wp3 + lane * 8;
    auto issue_nx = [&](int g, unsigned sbo) {
        const int S3 = a.Co2 / 16;
#pragma unroll
        for (int i = 0; i < NJ * 6 / 4; ++i) {
            const int q = wave + 4 * i, cbl = q / 6, r = q % 6;
            lds_dma16(nsrc + (((int64_t)cbl * S3 + 2 * g) * 3 + r) * 512, lbase + sbo + (unsigned)(W3B + q * 1024));
        }
    };
    // first block's residual: requested before the h2 staging, so its latency overlaps it
    float rv[2][17];
    if (a.res) res_load(std::true_type{}, 32 * part, rv[0], true);
    else res_load(std::false_type{}, 32 * part, rv[0], true);
    float b3[NJ > 0 ? NJ : 1];  // the next conv's bias of this lane's columns
#pragma unroll
    for (int j = 0; j < NJ; ++j) b3[j] = a.bias3 ? a.bias3[32 * j + r32] : 0.0f;
    __syncthreads();  // every wave is done with the staging buffers
    issue_w3(0, 0, HB);
    if constexpr (NXT > 0) issue_nx(0, HB);
    act_dispatch(a.act, [&](auto ac) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = wn * TN * 32 + j * 32 + r32;
                const float bj = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {  // two rows (r, r + 1) per split3x2
                    bf16x2 h_, m_, l_;
                    split3x2((f32x2){act_c<decltype(ac)::value>(acc[i][j][r] + bj),
                                     act_c<decltype(ac)::value>(acc[i][j][r + 1] + bj)},
                             h_, m_, l_);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int row = wm * TM * 32 + i * 32 + ((r + e) & 3) + 8 * ((r + e) >> 2) + 4 * hh;
                        H[row * HR + col] = h_[e];
                        H[HPL + row * HR + col] = m_[e];
                        H[2 * HPL + row * HR + col] = l_[e];
                    }
                }
            }
    });
    __syncthreads();
    bf16x8 fa[ST][3];  // conv3's A fragments of the band: h2, then the split shortcut operand (dual form)
    {
        const __bf16 *ap = H + (band + r32) * HR + 8 * hh;
#pragma unroll
        for (int t = 0; t < S2; ++t)
#pragma unroll
            for (int p = 0; p < 3; ++p) fa[t][p] = *(const bf16x8 *)(ap + p * HPL + 16 * t);
    }
    if constexpr (X2S > 0) {
        int64_t m = m0 + band + r32;
        const bool ok = m < a.M;
        m = ok ? m : 0;
        const int ox = (int)(m % a.Wo);
        const int64_t q = m / a.Wo;
        const int oy = (int)(q % a.Ho);
        const int64_t n = q / a.Ho;
        const float *xp = a.x2 + ((n * a.H2 + (int64_t)oy * a.stride2) * a.W2 + (int64_t)ox * a.stride2) * a.Ci2 + 8 * hh;
#pragma unroll
        for (int t = 0; t < X2S; ++t) {
            f32x4 v0 = ok ? *(const f32x4 *)(xp + 16 * t) : (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 v1 = ok ? *(const f32x4 *)(xp + 16 * t + 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                __bf16 h_, m_, l_;
                split3(e < 4 ? v0[e] : v1[e - 4], h_, m_, l_);
                fa[S2 + t][0][e] = h_, fa[S2 + t][1][e] = m_, fa[S2 + t][2][e] = l_;
            }
        }
    }
    // everything this wave has issued so far is complete: the counted waits of the loop start from an empty queue
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const __amdgpu_buffer_rsrc_t ry = buffer_rsrc(a.y + base, rows * a.Co2 * 4);
    // NXT: the wave's LDS block and the next conv's accumulators.  put_block: 16 C-layout values per lane (column r32,
    // rows (r & 3) + 8 (r >> 2) + 4 hh) split into the three planes; frag: 16-B piece c of row `row`, plane p (A
    // fragment of slice t: row r32, piece 2 t + hh)
    __bf16 *Y = (__bf16 *)(lds_raw + YB0 + wave * YBW);
    f32x16 accn[NJ > 0 ? NJ : 1];
#pragma unroll
    for (int j = 0; j < NJ; ++j) accn[j] = (f32x16){0};
    auto put_block = [&](const float(&o)[16]) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            bf16x2 h_, m_, l_;
            split3x2((f32x2){o[r], o[r + 1]}, h_, m_, l_);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                __bf16 *yp = Y + (((r + e) & 3) + 8 * ((r + e) >> 2) + 4 * hh) * YP + r32;
                yp[0] = h_[e];
                yp[YPL] = m_[e];
                yp[2 * YPL] = l_[e];
            }
        }
        asm volatile("" ::: "memory");  // the reads below follow these writes (one wave: LDS keeps their order)
    };
    auto frag = [&](int p, int row, int c) { return *(const bf16x8 *)(Y + p * YPL + row * YP + 8 * c); };
    // one column block: rc = its bias2 / residual (loaded during the previous block), rn = the next block's
    auto block = [&](auto hr, auto a2, int g, float(&rc)[17], float(&rn)[17]) {
        constexpr bool HAS_RES = decltype(hr)::value;
        constexpr int R = HAS_RES ? 17 : 1;  // loads of one res_load
        const bool more = g + 1 < NG;
        const int c0 = 32 * (g * WPB + part);
        f32x16 acc2 = (f32x16){0};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // in flight behind this step's DMAs (issued one step ago): see the issue order above
            if constexpr (U == 1) x6_wait_barrier<R + 16>();
            else if (u == 0) x6_wait_barrier<16>();
            else if (u == 1) x6_wait_barrier<R>();
            else x6_wait_barrier<0>();
            const unsigned sbo = ((g * U + u) & 1) ? 0u : (unsigned)HB;
            if (u + 1 < U) issue_w3(g, u + 1, (unsigned)HB - sbo);
            else if (more) issue_w3(g + 1, 0, (unsigned)HB - sbo);
            if constexpr (NXT > 0) {
                if (more) issue_nx(g + 1, (unsigned)HB - sbo);
            }
            if (u == 0) {
                res_load(hr, c0 + 32 * WPB, rn, more);
                asm volatile("" ::: "memory");  // the loads stay here, in front of the step's LDS reads and MFMAs
            }
            const __bf16 *Bs = (const __bf16 *)(lds_raw + sbo) + part * (12 * 512) + lane * 8;
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) {
                const int t = 4 * u + sl;
                bf16x8 fb[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) fb[p] = *(const bf16x8 *)(Bs + (sl * 3 + p) * 512);
                x6_dot(acc2, fa[t], fb);
            }
        }
        const float bj = rc[16];
        float ov[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float o = acc2[r] + bj;
            if constexpr (HAS_RES) o += rc[r];
            o = act_c<decltype(a2)::value>(o);
            ov[r] = o;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), ry,
                                                  vo + ((r & 3) + 8 * (r >> 2)) * a.Co2 * 4, c0 * 4, 0);
        }
        if constexpr (NXT > 0) {  // the next conv over this block's 32 channels of y: slices 2 g, 2 g + 1 of its K
            put_block(ov);
            bf16x8 ya[2][3];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) ya[t][p] = frag(p, r32, 2 * t + hh);
            const unsigned sbo = (g & 1) ? 0u : (unsigned)HB;
            const __bf16 *Ns = (const __bf16 *)(lds_raw + sbo + W3B) + lane * 8;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    bf16x8 fb[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) fb[p] = *(const bf16x8 *)(Ns + ((j * 2 + t) * 3 + p) * 512);
                    x6_dot(accn[j], ya[t], fb);
                }
        }
    };
    auto run = [&](auto hr, auto a2) {
        // the first block's residual has arrived (the wait above); using it here tells the compiler so, and its own
        // waits inside the loop count from the loop's loads alone
        asm volatile("" ::"v"(rv[0][16]));
        if constexpr (decltype(hr)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(rv[0][r]));
        }
        for (int g = 0; g < NG; g += 2) {
            block(hr, a2, g, rv[0], rv[1]);
            if (g + 1 < NG) block(hr, a2, g + 1, rv[1], rv[0]);
        }
    };
    act_dispatch(a.act2, [&](auto a2) {
        if (a.res) run(std::true_type{}, a2);
        else run(std::false_type{}, a2);
    });
    if constexpr (NXT > 0) {
        // h' = act3(accn + bias3), split; through the wave's LDS block (free: the last block's fragments are in
        // registers) so that a lane stores 16-B row pieces: lane -> (row lane / 4 (+ 16), piece lane % 4), 64 B a row
        act_dispatch(a.act3, [&](auto a3) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float ov[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) ov[r] = act_c<decltype(a3)::value>(accn[j][r] + b3[j]);
                put_block(ov);
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int row = 16 * i + (lane >> 2), c = lane & 3;
                        const bf16x8 v = frag(p, row, c);
                        const int64_t m = m0 + band + row;
                        if (m < a.M) *(bf16x8 *)(a.ys + p * a.yps + m * NXT + 32 * j + 8 * c) = v;
                    }
                asm volatile("" ::: "memory");  // the next column block's writes follow these reads
            }
        });
    }
}

// ---------------------------------------------------------------------------
// k_conv_x6b: Ci % 32 == 0 (every ResNet trunk layer).  K step 32 (two 16-deep slices, 48 MFMAs per wave and
// step for a 64 x 64 wave tile: twice the work per barrier of k_conv_x6).  Only A goes through LDS (three bf16
// planes, rows of 40 bf16 = 80 B = 5 odd 16-B slots: conflict-free fragment groups); the B fragments are read
// straight from the fragment-order panel into registers (one coalesced 1-KiB load per fragment and plane), one
// slice ahead of their MFMAs, so the LDS per stage is A's alone (30 KiB for 128 rows).
// ---------------------------------------------------------------------------
constexpr int YBK = 32;
constexpr int YROW = 40;

// CHAIN: 0 none, 1 chain, 2 chain + shortcut; NT: non-temporal activation loads (BEV_TUNE_CONV_X6_NT)
// BUFA: operand and weight fragments by raw buffer loads (X6Desc above; BEV_TUNE_CONV_X6_BUF), else 64-bit pointers
template <int WM, int WN, int TM, int TN, bool DUAL, int CHAIN = 0, bool NT = false, bool BUFA = false>
__global__ __launch_bounds__(256, 2) void k_conv_x6b(ConvX a) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int APL = BM * YROW;                 // bf16 per A plane
    constexpr int STAGE = 3 * APL;                 // bf16 per LDS stage
    constexpr int AQ = BM / 32;                    // A float4 per thread and K step: rows tid / 8 + 32 q
    constexpr int EPIB = CHAIN ? x6_chain_lds_bytes<BM, BN>() : x6_epi_bytes<TN>();
    constexpr int LDSB = (2 * STAGE * 2 > EPIB) ? 2 * STAGE * 2 : EPIB;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDSB];
    __bf16 *lds = (__bf16 *)lds_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (SGPR)
    const int wm = wave / WN, wn = wave % WN;
    const int n_tiles = (a.Co + BN - 1) / BN;
    const unsigned bid = xcd_block(blockIdx.x, gridDim.x);  // the n_tiles blocks of the same A rows on one XCD
    const int64_t m0 = (int64_t)(bid / n_tiles) * BM;
    const int n0 = (bid % n_tiles) * BN;

    const int aq = tid & 7;
    int64_t pb[AQ], p2[AQ];
    int iy0[AQ], ix0[AQ];
    bool rok[AQ];
    // BUFA: row q's byte offsets at tap (0, 0) in x / x2 (see X6Desc), and the offset its next load uses: vr, or
    // X6_VOUT while the row (m >= M) or its tap (outside the image) reads zeros
    X6Desc dsc;
    if constexpr (BUFA) dsc = x6_desc<DUAL>(a, m0);
    unsigned vr[AQ], vr2[AQ];
    int vo[AQ], vo2[AQ];
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
        const int64_t m = m0 + (tid >> 3) + 32 * q;
        rok[q] = m < a.M;
        if constexpr (BUFA && !DUAL) {
            if (dsc.lin) {  // wave-uniform: no division in this prologue
                vr[q] = (unsigned)((tid >> 3) + 32 * q) * (unsigned)a.Ci * 4u + 16u * aq;
                vr2[q] = 0;
                iy0[q] = ix0[q] = 0;
                pb[q] = p2[q] = 0;
                continue;
            }
        }
        const int64_t mm = rok[q] ? m : 0;
        const int ox = (int)(mm % a.Wo);
        const int64_t t = mm / a.Wo;
        const int oy = (int)(t % a.Ho);
        const int64_t n = t / a.Ho;
        if (DUAL) {
            pb[q] = mm * a.Ci + 4 * aq;
            p2[q] = ((n * a.H2 + (int64_t)oy * a.stride2) * a.W2 + (int64_t)ox * a.stride2) * a.Ci2 + 4 * aq;
            iy0[q] = ix0[q] = 0;
        } else {
            pb[q] = n * a.H * a.W * a.Ci + 4 * aq;
            p2[q] = 0;
            iy0[q] = oy * a.stride - a.pad;
            ix0[q] = ox * a.stride - a.pad;
        }
        if constexpr (BUFA) {  // 32-bit byte offsets from the descriptors' bases (wrapping arithmetic for dead rows)
            const unsigned nr = (unsigned)(int)(n - dsc.n_first);
            if (DUAL) {
                vr[q] = (unsigned)(int)(m - m0) * (unsigned)a.Ci * 4u + 16u * aq;
                vr2[q] = ((nr * a.H2 + (unsigned)(oy * a.stride2)) * a.W2 + (unsigned)(ox * a.stride2)) *
                             (unsigned)a.Ci2 * 4u + 16u * aq;
            } else {
                vr[q] = ((nr * a.H + (unsigned)iy0[q]) * a.W + (unsigned)ix0[q]) * (unsigned)a.Ci * 4u + 16u * aq +
                        (unsigned)dsc.xbias;
                vr2[q] = 0;
            }
        }
    }
    // B: this wave's fragments of column blocks (n0 + wn TN 32) / 32 + j; slice g of block cb, plane p at
    // wb + (cb_rel * S + g) * 1536 + p * 512 (bf16), lane part l * 8
    const int64_t S = a.Kp / XBK;
    const __bf16 *wb = a.wp + ((int64_t)((n0 + wn * TN * 32) >> 5) * S) * 1536 + lane * 8;
    const int nslice = a.Kp / XBK;
    // BUFA: the fragments by raw buffer loads, the lane part of the address in the VGPR offset and the (block, slice,
    // plane) part in soffset, as k_conv_x6s loads them
    __amdgpu_buffer_rsrc_t rw;
    if constexpr (BUFA) rw = x6_rsrc(a.wp, copad_x(a.Co) / 32 * (int64_t)nslice * 3072);
    const int cb0 = (n0 + wn * TN * 32) >> 5;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};

    f32x4 va0[AQ], va1[AQ];
    bf16x8 bs0[TN][3], bs1[TN][3];  // B fragments of the even / odd slices
    int ky = 0, kx = 0, ci0 = 0, k0 = 0;
    // BUFA: the byte offset of tap (ky, kx) (wave-uniform, for soffset) and the rows' validity there -- once per tap,
    // Ci / 32 K steps share it; a 1x1 conv computes it here and never again
    int soff = 0;
    auto x6_tap = [&]() {
        const int dy = ky * a.dil, dx = kx * a.dil;
        soff = (dy * a.W + dx) * a.Ci * 4;
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int iy = iy0[q] + dy, ix = ix0[q] + dx;
            // & not &&: three compares and one select, no branch and no exec-masked region
            const bool in = rok[q] & ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            vo[q] = in ? (int)vr[q] : X6_VOUT;
            vo2[q] = rok[q] ? (int)vr2[q] : X6_VOUT;
        }
    };
    if constexpr (BUFA) x6_tap();
    constexpr int AUX = NT ? 2 : 0;  // the buffer load's cache policy: nt
#define X6B_GLOAD(VA)                                                                                      \
    do {                                                                                                   \
        if constexpr (BUFA) {                                                                              \
            if (DUAL) {                                                                                    \
                if (k0 < a.Ci) {                                                                           \
                    _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] = __builtin_bit_cast(             \
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(dsc.rx, vo[q], k0 * 4, AUX));         \
                } else {                                                                                   \
                    _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] = __builtin_bit_cast(             \
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(dsc.rx2, vo2[q], (k0 - a.Ci) * 4, AUX)); \
                }                                                                                          \
                k0 += YBK;                                                                                 \
            } else {                                                                                       \
                _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] = __builtin_bit_cast(                 \
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(dsc.rx, vo[q], soff, AUX));               \
                soff += YBK * 4;                                                                           \
                ci0 += YBK;                                                                                \
                if (ci0 == a.Ci) {                                                                         \
                    ci0 = 0;                                                                               \
                    if (++kx == a.KW) {                                                                    \
                        kx = 0;                                                                            \
                        ++ky;                                                                              \
                    }                                                                                      \
                    x6_tap();                                                                              \
                }                                                                                          \
            }                                                                                              \
            break;                                                                                         \
        }                                                                                                  \
        if (DUAL) {                                                                                        \
            const bool first = k0 < a.Ci;                                                                  \
            const float *src = first ? a.x + k0 : a.x2 + (k0 - a.Ci);                                      \
            _Pragma("unroll") for (int q = 0; q < AQ; ++q) VA[q] =                                         \
                *(const f32x4 *)(rok[q] ? src + (first ? pb[q] : p2[q]) : g_xzero4);                      \
            k0 += YBK;                                                                                     \
        } else {                                                                                           \
            const int dy = ky * a.dil, dx = kx * a.dil;                                                    \
            _Pragma("unroll") for (int q = 0; q < AQ; ++q) {                                               \
                const int iy = iy0[q] + dy, ix = ix0[q] + dx;                                              \
                const bool in = rok[q] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;    \
                const f32x4 *ap_ = (const f32x4 *)(in ? a.x + pb[q] + ((int64_t)iy * a.W + ix) * a.Ci + ci0 : g_xzero4); \
                if (NT) VA[q] = __builtin_nontemporal_load(ap_);                                          \
                else VA[q] = *ap_;                                                                        \
            }                                                                                              \
            ci0 += YBK;                                                                                    \
            if (ci0 == a.Ci) {                                                                             \
                ci0 = 0;                                                                                   \
                if (++kx == a.KW) {                                                                        \
                    kx = 0;                                                                                \
                    ++ky;                                                                                  \
                }                                                                                          \
            }                                                                                              \
        }                                                                                                  \
    } while (0)
#define X6B_SWRITE(BUF, VA)                                                                                \
    do {                                                                                                   \
        __bf16 *As = lds + (BUF) * STAGE;                                                                  \
        _Pragma("unroll") for (int q = 0; q < AQ; ++q) {                                                   \
            bf16x4 hv, mv, lv;                                                                             \
            split3x4(VA[q], hv, mv, lv);                                                                   \
            __bf16 *d = As + ((tid >> 3) + 32 * q) * YROW + 4 * aq;                                        \
            *(bf16x4 *)d = hv;                                                                             \
            *(bf16x4 *)(d + APL) = mv;                                                                     \
            *(bf16x4 *)(d + 2 * APL) = lv;                                                                 \
        }                                                                                                  \
    } while (0)
#define X6B_BLOAD(BS, G)                                                                                   \
    do {                                                                                                   \
        const int g_ = (G) < nslice ? (G) : nslice - 1; /* past the end: a harmless re-read */             \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
            _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                \
                if constexpr (BUFA)                                                                        \
                    BS[j][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(           \
                                                              rw, lane * 16, (((cb0 + j) * nslice + g_) * 3 + p) * 1024, 0)); \
                else BS[j][p] = *(const bf16x8 *)(wb + ((int64_t)j * S + g_) * 1536 + p * 512);           \
            }                                                                                              \
    } while (0)
    const int r32 = lane & 31, h = lane >> 5;
#define X6B_SLICE(AS, KK, BC)                                                                              \
    do {                                                                                                   \
        bf16x8 fa[TM][3];                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
            _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                  \
                fa[i][p] = *(const bf16x8 *)(AS + p * APL + (wm * TM * 32 + i * 32 + r32) * YROW + 16 * (KK) + 8 * h); \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
                x6_dot(acc[i][j], fa[i], BC[j]);                                                           \
    } while (0)
    // MFMAs of K step KS from LDS buffer BUF: slice 2 KS (B in bs0), slice 2 KS + 1 (B in bs1, loaded by the caller
    // BEFORE the step's A prefetch), the next step's slice 0 loaded into bs0 in between.  Order matters: vmcnt
    // retires loads in issue order, so a B fragment loaded after an A prefetch would make its first use wait for
    // that prefetch too (half a K step of cover instead of a whole one).
#define X6B_MFMA(BUF, KS)                                                                                  \
    do {                                                                                                   \
        const __bf16 *As = lds + (BUF) * STAGE;                                                            \
        X6B_SLICE(As, 0, bs0);                                                                             \
        X6B_BLOAD(bs0, 2 * (KS) + 2);                                                                      \
        X6B_SLICE(As, 1, bs1);                                                                             \
    } while (0)

    const int nk = a.Kp / YBK;
    X6B_BLOAD(bs0, 0);
    X6B_GLOAD(va0);
    if (nk > 1) X6B_GLOAD(va1);
    X6B_SWRITE(0, va0);
    __syncthreads();
    int ks = 0;
    for (; ks + 3 < nk; ks += 2) {
        X6B_BLOAD(bs1, 2 * ks + 1);
        X6B_GLOAD(va0);  // step ks + 2
        X6B_MFMA(0, ks);
        X6B_SWRITE(1, va1);  // step ks + 1
        __syncthreads();
        X6B_BLOAD(bs1, 2 * ks + 3);
        X6B_GLOAD(va1);  // step ks + 3
        X6B_MFMA(1, ks + 1);
        X6B_SWRITE(0, va0);  // step ks + 2
        __syncthreads();
    }
    if (ks + 2 < nk) {
        X6B_BLOAD(bs1, 2 * ks + 1);
        X6B_GLOAD(va0);
        X6B_MFMA(0, ks);
        X6B_SWRITE(1, va1);
        __syncthreads();
        X6B_BLOAD(bs1, 2 * ks + 3);
        X6B_MFMA(1, ks + 1);
        X6B_SWRITE(0, va0);
        __syncthreads();
        X6B_BLOAD(bs1, 2 * ks + 5);
        X6B_MFMA(0, ks + 2);
    } else if (ks + 1 < nk) {
        X6B_BLOAD(bs1, 2 * ks + 1);
        X6B_MFMA(0, ks);
        X6B_SWRITE(1, va1);
        __syncthreads();
        X6B_BLOAD(bs1, 2 * ks + 3);
        X6B_MFMA(1, ks + 1);
    } else {
        X6B_BLOAD(bs1, 2 * ks + 1);
        X6B_MFMA(0, ks);
    }
#undef X6B_MFMA
#undef X6B_SLICE
#undef X6B_BLOAD
#undef X6B_SWRITE
#undef X6B_GLOAD
    if constexpr (CHAIN > 0) {
        x6_chain_epilogue<WM, WN, TM, TN, CHAIN == 2 ? 4 : 0>(a, lds_raw, acc, wave, lane, wm, wn, m0);
        return;
    }
    x6_epilogue<TM, TN>(a, (float *)lds_raw, acc, wave, lane, wn, wm, m0, n0);
}

// ---------------------------------------------------------------------------
// k_conv_x6s: A from PRE-SPLIT activation planes (xs [3][N][H][W][Ci] bf16, written split by the producing conv's
// epilogue -- the 3x3 bottleneck conv2 reads the conv1 output it would otherwise split 9 times, once per tap)
// staged global -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging VGPRs, no ds_write, no split VALU).  One
// DMA instruction moves 16 rows x 64 B of one plane; the 16-B chunk c of row r sits at chunk c ^ ((r >> 2) & 3),
// so the 16-lane fragment groups (16 consecutive rows, one chunk) hit 16 distinct slots.  B fragments by buffer
// loads from the fragment-order panel: the lane part of the address in the VGPR, the (block, slice, plane) part in
// the SGPR soffset (no address VALU).  NHWC, Ci % 32 == 0.  Same per-output K order as k_conv_x6 / k_conv_x6b:
// bit-identical results on the same split operands.
// ---------------------------------------------------------------------------
// CHAIN (bev_conv2d_chain_x6_f32 / _dual_ with a pre-split xs): the mainloop above, then x6_chain_epilogue exactly
// as k_conv_x6b's chain runs it -- the layer1 / layer2 bottleneck bodies take conv1's split output, so conv2 (the
// 3x3, whose fp32 operand the register-staged kernel splits once per tap) stages by DMA alone.
// BLDS (the chains): B goes through LDS too -- the K step's BN / 32 x 2 slices x 3 planes of the fragment-order panel
// are 1-KiB runs, one DMA instruction each, read back as conflict-free ds_read_b128 (lane l at 16 l) -- so every
// vector-memory operation of the loop is a DMA issued one K step ahead and waited for at the step's end.  (With B
// in registers hipcc re-issued the fragment loads next to their MFMAs and waited on each: L2 latency per slice.)
//
// STRIP (the layer1 chains: 3x3 / stride 1 / pad 1 / Ci = 64, 128 x 64 tile; BEV_TUNE_CONV_X6_STRIP): the taps
// kx = 0, 1, 2 of one ky read the same h1 pixels shifted by one, and a tile is 128 consecutive pixels in (n, oy, ox)
// order -- so a STRIP of 130 consecutive pixels per ky serves all three kx, staged once instead of three times
// (A bytes L2 -> LDS per workgroup 432 KiB -> 162 KiB; with B's 216 KiB the mainloop moves 0.58x the bytes).
// LDS: two half-strips (channels 0..31, 32..63) of 3 planes x 144 rows x 64 B (130 rows used: 9 DMA groups of 16),
// the chunk swizzle above -- conflict-free for 16 consecutive rows from ANY start row, so the shifted fragment reads
// stay conflict-free -- then the two B stages: 55,296 + 24,576 = 79,872 B (two workgroups per CU).
// Strip row sr of tap row ky holds pixel q = p + (ky - 1) W, p = m0 - 1 + sr; zero when p is outside [0, M) or
// y_p + ky - 1 outside [0, H): the tap above / below the image or in another image.  A horizontal edge cannot be
// zeroed there (a pixel valid for one output is out of bounds for its neighbour): the lane whose output has ox == 0
// (ox == W - 1) takes a zero A fragment in the kx = 0 (kx = 2) slices, by a select, so a NaN / Inf in the
// neighbouring row's pixel does not leak.  K steps in today's order (ky, kx, channel half): output row R reads strip
// row R + kx of the step's half.  Half-strip 0 of ky + 1 is issued in step (ky, 2, half 1) -- its last reader was
// the step before -- and half-strip 1 of ky in step (ky, 0, half 0); each is waited for at the end of the step that
// issues it, B stays one step ahead: no further buffers, no bubble.  Same slices, same x6_dot: bit-identical.
__device__ __forceinline__ void x6s_strip_mainloop(const ConvX &a, unsigned char *lds_raw, f32x16 (&acc)[1][2],
                                                   int wave, int lane, int64_t m0) {
    constexpr int SROWS = 144, SUSED = 130;  // strip rows staged / read (rows 0 .. 127 + 2)
    constexpr int SPL = SROWS * 32;          // bf16 per strip plane
    constexpr int HSB = 3 * SPL * 2;         // bytes per half-strip
    constexpr int BSTB = 2 * 6 * 1024;       // bytes per B stage: [cb 2][slice 2][plane 3] fragment runs of 1 KiB
    constexpr int NPC = 27;                  // DMA pieces (plane, 16-row group) per half-strip
    constexpr int NP = (NPC + 3) / 4;        // ... per wave: piece q = wave + 4 i
    constexpr int YOUT = -(1 << 30);         // "row" of a strip pixel that is never inside the image
    const __bf16 *lds = (const __bf16 *)lds_raw;
    const unsigned lbase = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(lds_raw));
    const int r32 = lane & 31, h = lane >> 5;

    // DMA: lane l of a piece copies strip row 16 g + (l >> 2), physical chunk l & 3 = logical chunk
    // (l & 3) ^ ((row >> 2) & 3) (16 g >> 2 is a multiple of 4: the same for every group)
    const int lc = (lane & 3) ^ ((lane >> 4) & 3);
    const int64_t loff = (m0 - 1 + (lane >> 2)) * 64 + 8 * lc;  // lane part of the source offset (bf16)
    int yv[NP];  // image row of this lane's strip pixel in piece i, YOUT outside [0, M) and for rows never read
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int g = (wave + 4 * i) % 9;
        const int sr = 16 * g + (lane >> 2);
        const int64_t p = m0 - 1 + sr;
        const bool ok = sr < SUSED && p >= 0 && p < a.M;
        yv[i] = ok ? (int)((p / a.W) % a.H) : YOUT;
    }
    auto issue_strip = [&](int half, int ky) {
        const int64_t so = (int64_t)(ky - 1) * a.W * 64 + half * 32;
        const unsigned d0 = lbase + (unsigned)(half * HSB);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = wave + 4 * i;  // wave-uniform
            if (q < NPC) {
                const int pl = q / 9, g = q % 9;
                const bool in = (unsigned)(yv[i] + ky - 1) < (unsigned)a.H;
                const __bf16 *src = a.xs + (loff + so + (int64_t)g * (16 * 64) + pl * a.xps);
                lds_dma16(in ? (const void *)src : (const void *)g_xzero4, d0 + (unsigned)(pl * SPL * 2 + g * 1024));
            }
        }
    };
    const int S = a.Kp / XBK;  // 16-deep slices (36)
    const __bf16 *bsrc = a.wp + lane * 8;
    int kstep = 0;
    auto issue_b = [&](int buf) {  // piece q = (cb, slice, plane) of K step kstep: panel run ((cb S + 2 ks + sl) 3 + p)
        const unsigned db = lbase + (unsigned)(2 * HSB + buf * BSTB);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int q = wave + 4 * i, cbl = q / 6, r = q % 6;
            lds_dma16(bsrc + ((int64_t)cbl * S + 2 * kstep + r / 3) * 1536 + (r % 3) * 512, db + (unsigned)(q * 1024));
        }
        ++kstep;
    };

    // this lane's output row (A fragment row r32 of the wave's band) and its horizontal edges
    const int R = wave * 32 + r32;
    const int ox = (int)((m0 + R) % a.W);
    const bool e0 = ox == 0, e2 = ox == a.W - 1;
    const bool any0 = __builtin_amdgcn_ballot_w64(e0) != 0, any2 = __builtin_amdgcn_ballot_w64(e2) != 0;

    issue_b(0);
    issue_strip(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {  // K step (ky, kx, half)
            const int kx = t >> 1, half = t & 1;
            if (t < 5 || ky < 2) issue_b((t + 1) & 1);
            if (t == 0) issue_strip(1, ky);
            if (t == 5 && ky < 2) issue_strip(0, ky + 1);
            const __bf16 *As = lds + half * (3 * SPL);
            const __bf16 *Bs = (const __bf16 *)(lds_raw + 2 * HSB + (t & 1) * BSTB) + lane * 8;
            const int r = R + kx;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 fb[2][3], fa[3];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int p = 0; p < 3; ++p) fb[j][p] = *(const bf16x8 *)(Bs + ((j * 2 + kk) * 3 + p) * 512);
                const int ph = (2 * kk + h) ^ ((r >> 2) & 3);
#pragma unroll
                for (int p = 0; p < 3; ++p) fa[p] = *(const bf16x8 *)(As + p * SPL + r * 32 + ph * 8);
                if ((kx == 0 && any0) || (kx == 2 && any2)) {  // wave-uniform: most waves hold no edge pixel
                    const bool z = kx == 0 ? e0 : e2;
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        u32x4 v = __builtin_bit_cast(u32x4, fa[p]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = z ? 0u : v[e];
                        fa[p] = __builtin_bit_cast(bf16x8, v);
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) x6_dot(acc[0][j], fa, fb[j]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMAs of the next step landed
            __syncthreads();                                   // everyone's; this step's buffers are free again
        }
    }
}

template <int WM, int WN, int TM, int TN, int CHAIN = 0, bool STRIP = false>
__global__ __launch_bounds__(256, CHAIN ? 2 : 3) void k_conv_x6s(ConvX a) {
    constexpr bool BLDS = CHAIN > 0;
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int APL = BM * 32;     // bf16 per A plane per stage (64-B rows)
    constexpr int BST = BLDS ? BN / 32 * 6 * 512 : 0;  // bf16 of B per stage: [cb][slice][plane][64 lanes][8]
    constexpr int STAGE = 3 * APL + BST;  // bf16 per stage
    constexpr int RW = BM / 4;       // rows staged by each wave
    constexpr int RG = RW / 16;      // 16-row DMA groups per wave and plane
    constexpr int BPW = BLDS ? BN / 32 * 6 / 4 : 0;  // B pieces (1 KiB) per wave and K step
    constexpr int EPIB = CHAIN ? x6_chain_lds_bytes<BM, BN>() : x6_epi_bytes<TN>();
    constexpr int MAINB = STRIP ? 2 * (3 * 144 * 64) + 2 * BST * 2 : 2 * STAGE * 2;  // STRIP: half-strips + B stages
    constexpr int LDSB = (MAINB > EPIB) ? MAINB : EPIB;
    static_assert(RW % 16 == 0, "whole DMA groups per wave");
    static_assert(!BLDS || (BN / 32 * 6) % 4 == 0, "whole B pieces per wave");
    static_assert(!STRIP || (CHAIN > 0 && WM == 4 && WN == 1 && TM == 1 && TN == 2), "strip: the 128 x 64 chains");
    // CHAIN 3: the chain plus the next block's conv1 (x6_chain_epilogue NXT = 64), strip-staged only; its epilogue
    // puts a conv1 stage behind W3 stage 0: h2 planes + 2 x 12 KiB, exactly the strip mainloop's LDS
    static_assert(CHAIN != 3 || (STRIP && LDSB >= 3 * BM * (BN + 8) * 2 + 2 * 12288), "next conv: strip form, LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDSB];
    const __bf16 *lds = (const __bf16 *)lds_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (SGPR)
    const int wm = wave / WN, wn = wave % WN;
    const int n_tiles = (a.Co + BN - 1) / BN;
    const unsigned bid = xcd_block(blockIdx.x, gridDim.x);  // the n_tiles blocks of the same A rows on one XCD
    const int64_t m0 = (int64_t)(bid / n_tiles) * BM;
    const int n0 = (bid % n_tiles) * BN;

    if constexpr (STRIP) {  // Ci = Co = 64, 3x3 / 1 / 1 (conv_x6() checks): one column tile, n0 = 0
        f32x16 sacc[1][2] = {{(f32x16){0}, (f32x16){0}}};
        x6s_strip_mainloop(a, lds_raw, sacc, wave, lane, m0);
        x6_chain_epilogue<WM, WN, TM, TN, CHAIN == 2 ? 4 : 0, CHAIN == 3 ? 64 : 0>(a, lds_raw, sacc, wave, lane, wm, wn,
                                                                                     m0);
        return;
    }

    // DMA rows of this lane: wave * RW + 16 g + (lane >> 2); physical chunk lane & 3 holds logical chunk
    // (lane & 3) ^ ((row >> 2) & 3)
    int64_t abase[RG];
    int aiy[RG], aix[RG];
    bool aok[RG];
#pragma unroll
    for (int g = 0; g < RG; ++g) {
        const int row = wave * RW + 16 * g + (lane >> 2);
        const int lc = (lane & 3) ^ ((row >> 2) & 3);
        const int64_t m = m0 + row;
        aok[g] = m < a.M;
        const int64_t mm = aok[g] ? m : 0;
        const int ox = (int)(mm % a.Wo);
        const int64_t t = mm / a.Wo;
        const int oy = (int)(t % a.Ho);
        const int64_t n = t / a.Ho;
        aiy[g] = oy * a.stride - a.pad;
        aix[g] = ox * a.stride - a.pad;
        abase[g] = ((n * a.H + aiy[g]) * a.W + aix[g]) * a.Ci + 8 * lc;
    }
    const unsigned lbase = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(lds_raw));
    const int S = a.Kp / XBK;  // 16-deep slices
    int ky = 0, kx = 0, ci0 = 0, kstep = 0;
    const __bf16 *bsrc = a.wp + (int64_t)(n0 >> 5) * S * 1536 + lane * 8;  // the block's first column block
    auto issue = [&](int buf) {
        if constexpr (BLDS) {  // piece q = (cb, slice, plane) of this K step: panel run ((cb S + 2 ks + sl) 3 + p)
            const unsigned db = lbase + (unsigned)(buf * STAGE * 2 + 3 * APL * 2);
#pragma unroll
            for (int i = 0; i < BPW; ++i) {
                const int q = wave + 4 * i, cbl = q / 6, r = q % 6;
                lds_dma16(bsrc + ((int64_t)cbl * S + 2 * kstep + r / 3) * 1536 + (r % 3) * 512,
                      db + (unsigned)(q * 1024));
            }
            ++kstep;
        }
        const int64_t toff = ((int64_t)ky * a.dil * a.W + kx * a.dil) * a.Ci + ci0;
        const unsigned d0 = lbase + (unsigned)(buf * STAGE * 2) + (unsigned)(wave * RW * 64);
#pragma unroll
        for (int g = 0; g < RG; ++g) {
            const int iy = aiy[g] + ky * a.dil, ix = aix[g] + kx * a.dil;
            const bool in = aok[g] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const __bf16 *src = a.xs + abase[g] + toff;
#pragma unroll
            for (int p = 0; p < 3; ++p)
                lds_dma16(in ? (const void *)(src + p * a.xps) : (const void *)g_xzero4,
                      d0 + (unsigned)(p * APL * 2 + g * 1024));
        }
        ci0 += YBK;
        if (ci0 == a.Ci) {
            ci0 = 0;
            if (++kx == a.KW) {
                kx = 0;
                ++ky;
            }
        }
    };

    const __amdgpu_buffer_rsrc_t rw = buffer_rsrc(a.wp, copad_x(a.Co) / 32 * (int64_t)S * 3072);
    const int cb0 = (n0 + wn * TN * 32) >> 5;
    const int vl = lane * 16;
    bf16x8 bs0[TN][3], bs1[TN][3];
#define X6S_BLOAD(BS, G)                                                                                   \
    do {                                                                                                   \
        const int g_ = (G) < S ? (G) : S - 1;                                                              \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
            _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                  \
                BS[j][p] = __builtin_bit_cast(                                                             \
                    bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, vl, (((cb0 + j) * S + g_) * 3 + p) * 1024, 0)); \
    } while (0)
    const int r32 = lane & 31, h = lane >> 5;
#define X6S_SLICE(AS, KK, BC)                                                                              \
    do {                                                                                                   \
        bf16x8 fa[TM][3];                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                   \
            const int R = wm * TM * 32 + i * 32 + r32;                                                     \
            const int ph = (2 * (KK) + h) ^ ((R >> 2) & 3);                                                \
            _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                  \
                fa[i][p] = *(const bf16x8 *)(AS + p * APL + R * 32 + ph * 8);                              \
        }                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
                x6_dot(acc[i][j], fa[i], BC[j]);                                                           \
    } while (0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
    const int nk = a.Kp / YBK;
    if constexpr (BLDS) {
        issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int ks = 0; ks < nk; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < nk) issue(cur ^ 1);
            const __bf16 *As = lds + cur * STAGE;
            const __bf16 *Bs = As + 3 * APL + lane * 8;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 fb[TN][3];
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int p = 0; p < 3; ++p) fb[j][p] = *(const bf16x8 *)(Bs + (((wn * TN + j) * 2 + kk) * 3 + p) * 512);
                X6S_SLICE(As, kk, fb);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMAs of step ks + 1 landed
            __syncthreads();                                   // everyone's; buffer cur is free again
        }
    } else {
        X6S_BLOAD(bs0, 0);
        issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int ks = 0; ks < nk; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < nk) issue(cur ^ 1);
            const __bf16 *As = lds + cur * STAGE;
            X6S_BLOAD(bs1, 2 * ks + 1);
            X6S_SLICE(As, 0, bs0);
            X6S_BLOAD(bs0, 2 * ks + 2);
            X6S_SLICE(As, 1, bs1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of step ks + 1 landed
            __syncthreads();                                   // all of it; buffer cur is free again
        }
    }
#undef X6S_SLICE
#undef X6S_BLOAD
    if constexpr (CHAIN > 0) {
        x6_chain_epilogue<WM, WN, TM, TN, CHAIN == 2 ? 4 : 0>(a, lds_raw, acc, wave, lane, wm, wn, m0);
        return;
    }
    x6_epilogue<TM, TN>(a, (float *)lds_raw, acc, wave, lane, wn, wm, m0, n0);
}

__global__ void k_split3(const float *__restrict__ x, int64_t n, __bf16 *__restrict__ out) {
    const int64_t t = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);  // elements t, t + 1
    if (t >= n) return;
    const bool two = t + 1 < n;
    bf16x2 h, m, l;
    split3x2((f32x2){x[t], two ? x[t + 1] : 0.0f}, h, m, l);
    out[t] = h[0];
    out[t + n] = m[0];
    out[t + 2 * n] = l[0];
    if (two) {
        out[t + 1] = h[1];
        out[t + 1 + n] = m[1];
        out[t + 1 + 2 * n] = l[1];
    }
}

int g_x6_tile = 0;  // 0 automatic, 1 = 128 x 128, 2 = 128 x 64
int g_x6_nt = 0;    // BEV_TUNE_CONV_X6_NT: 1 = non-temporal activation loads in the 32-deep kernels
int g_x6_kernel = 0;  // 0 automatic (k_conv_x6b wherever it applies), 1 = k_conv_x6 (16-deep K steps) everywhere
int g_x6_strip = 1;   // BEV_TUNE_CONV_X6_STRIP: 1 = the strip-staged mainloop in the layer1 chains, 0 = one staging per tap
int g_x6_buf = 1;     // BEV_TUNE_CONV_X6_BUF: 1 = fp32 operands staged by raw buffer loads where the size rule holds

// one workgroup per BM x BN output tile; `kernel` = the k_conv_x6 / k_conv_x6b / k_conv_x6s instance with that tile
// (BM = WM TM 32, BN = WN TN 32)
int launch_x6(void (*kernel)(ConvX), int BM, int BN, const ConvX &a, hipStream_t st) {
    const int64_t blocks = ((a.M + BM - 1) / BM) * ((a.Co + BN - 1) / BN);
    if (blocks >= ((int64_t)1 << 31)) return BEV_ERR_ARGS;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return last();
}

// What a tensor entry point asks for.  An entry fills what it has and leaves the rest at these defaults, under which
// the rules of conv_x6() that do not concern it hold by themselves: a null pointer is aligned, and the dual form's
// first operand is the 1x1 / stride 1 conv over x [N][Ho][Wo][Ci] that needs no geometry check of its own.
enum X6Form { X6_PLAIN, X6_DUAL, X6_CHAIN, X6_CHAIN_DUAL, X6_CHAIN_NEXT };
struct X6Call {
    X6Form form;
    // the conv (of a chain: the first, conv2 of the bottleneck): exactly one of x (fp32) and xs (pre-split planes)
    const float *x = nullptr;
    const uint16_t *xs = nullptr, *packed = nullptr;
    const float *bias = nullptr, *res = nullptr;
    float *y = nullptr;
    uint16_t *ys = nullptr;  // plain only: split output planes in place of y
    int N = 0, H = 0, W = 0, Ci = 0, Co = 0, KH = 1, KW = 1, stride = 1, pad = 0, dil = 1, act = 0, ldy = 0, Ho = 0,
        Wo = 0;
    // second operand (dual, chain-dual): x2 [N][H2][W2][Ci2] read at (oy stride2, ox stride2)
    const float *x2 = nullptr;
    int H2 = 0, W2 = 0, Ci2 = 0, stride2 = 0;
    // second conv (chain, chain-dual): 1x1 over the first one's Co channels; res and y belong to it
    const uint16_t *packed2 = nullptr;
    const float *bias2 = nullptr;
    int Co2 = 0, act2 = 0;
    // third conv (chain-next): the next block's 1x1 conv1 over y, its output split into ys ([3][M][Co3])
    const uint16_t *packed3 = nullptr;
    const float *bias3 = nullptr;
    int Co3 = 0, act3 = 0;
};

// The one host path of the split convs: validates, fills ConvX, picks the kernel instance.
int conv_x6(const X6Call &c, hipStream_t st) {
    const bool next = c.form == X6_CHAIN_NEXT;  // a chain that writes y AND the next conv's split output ys
    const bool chain = c.form == X6_CHAIN || c.form == X6_CHAIN_DUAL || next;
    const bool second = c.form == X6_DUAL || c.form == X6_CHAIN_DUAL;  // has x2
    // chain-next: only what its one kernel instance covers (the strip-staged layer1 body, 64 next channels)
    if (next && (!c.xs || !c.y || !c.ys || !c.packed3 || c.KH != 3 || c.KW != 3 || c.stride != 1 || c.pad != 1 ||
                 c.Ci != 64 || c.Co != 64 || c.Co3 != 64 || c.act3 < 0 || c.act3 > 2 ||
                 (((uintptr_t)c.packed3 | (uintptr_t)c.ys) & 15) != 0))
        return BEV_ERR_ARGS;
    if ((!c.x == !c.xs) || !c.packed || (!next && !c.y == !c.ys) || c.N < 0 || c.H <= 0 || c.W <= 0 || c.Co <= 0 ||
        c.KH <= 0 || c.KW <= 0 || c.stride <= 0 || c.pad < 0 || c.dil <= 0 || c.act < 0 || c.act > 2)
        return BEV_ERR_ARGS;
    // one tap and 16 channels per K step; 32 for a pre-split operand and in the chains (k_conv_x6b / k_conv_x6s only).
    // The chains check no more of Ci than this.
    if ((!chain && c.Ci <= 0) || c.Ci % (chain || c.xs ? YBK : XBK) != 0) return BEV_ERR_ARGS;
    if (second && (!c.x2 || c.H2 <= 0 || c.W2 <= 0 || c.Ci2 <= 0 || c.stride2 <= 0)) return BEV_ERR_ARGS;
    if (c.form == X6_DUAL && c.Ci2 % XBK != 0) return BEV_ERR_ARGS;
    if (chain && (!c.packed2 || c.act2 < 0 || c.act2 > 2 || c.Co2 <= 0 || c.Co2 % 64 != 0)) return BEV_ERR_ARGS;
    // the chain epilogue holds all of h2: 64 or 128 channels; with the shortcut operand the layer1 block-0 shape only
    // (64-channel h2 and a 64-channel x2, 4 slices kept in registers)
    if (c.form == X6_CHAIN && c.Co != 64 && c.Co != 128) return BEV_ERR_ARGS;
    if (c.form == X6_CHAIN_DUAL && (c.Co != 64 || c.Ci2 != 64)) return BEV_ERR_ARGS;
    if (c.Ho != conv_out(c.H, c.pad, c.dil, c.KH, c.stride) || c.Wo != conv_out(c.W, c.pad, c.dil, c.KW, c.stride) ||
        c.Ho <= 0 || c.Wo <= 0)
        return BEV_ERR_ARGS;
    if (second && (c.Ho != conv_out(c.H2, 0, 1, 1, c.stride2) || c.Wo != conv_out(c.W2, 0, 1, 1, c.stride2)))
        return BEV_ERR_ARGS;
    if ((((uintptr_t)c.x | (uintptr_t)c.xs | (uintptr_t)c.x2 | (uintptr_t)c.packed | (uintptr_t)c.packed2) & 15) != 0)
        return BEV_ERR_ARGS;
    // y rows of ldy >= Co floats; dense for a residual and for split output (a chain's y: dense rows of Co2)
    if (!chain && (c.ldy < c.Co || (c.res && c.ldy != c.Co))) return BEV_ERR_ARGS;
    if (!next && c.ys && (c.ldy != c.Co || c.Co % 4 != 0 || ((uintptr_t)c.ys & 7) != 0)) return BEV_ERR_ARGS;
    if (c.N == 0) return 0;
    // two waves share each 32-row band of the 64-row tile (checked behind the empty call's answer: test_capi.py pins it)
    if (c.form == X6_CHAIN && c.Co != 64 && c.Co2 % 128 != 0) return BEV_ERR_ARGS;

    ConvX a;
    a.x = c.x, a.wp = (const __bf16 *)c.packed, a.bias = c.bias, a.res = c.res, a.y = c.y;
    a.N = c.N, a.H = c.H, a.W = c.W, a.Ci = c.Ci, a.Co = c.Co, a.KH = c.KH, a.KW = c.KW, a.stride = c.stride;
    a.pad = c.pad, a.dil = c.dil, a.Ho = c.Ho, a.Wo = c.Wo, a.act = c.act, a.ldy = chain ? c.Co2 : c.ldy;
    a.Kp = (int)kpad_x(c.form == X6_DUAL ? c.Ci + c.Ci2 : c.Ci * c.KH * c.KW);  // dual: one GEMM over K = [x | x2]
    a.M = (int64_t)c.N * c.Ho * c.Wo;
    a.x2 = c.x2, a.Ci2 = c.Ci2, a.H2 = c.H2, a.W2 = c.W2, a.stride2 = c.stride2;
    a.xs = (const __bf16 *)c.xs, a.ys = (__bf16 *)c.ys;
    a.xps = (int64_t)c.N * c.H * c.W * c.Ci, a.yps = a.M * (next ? c.Co3 : c.Co);
    a.wp2 = (const __bf16 *)c.packed2, a.bias2 = c.bias2, a.Co2 = c.Co2, a.act2 = c.act2;
    a.wp3 = (const __bf16 *)c.packed3, a.bias3 = c.bias3, a.Co3 = c.Co3, a.act3 = c.act3;

    // The chains.  A pre-split operand (conv1 handed over its output split) is staged by LDS-DMA (k_conv_x6s), same K
    // order.  h2 of 128 channels: the 64 x 128 tile (h2 planes 52 KiB of LDS).
    // The layer1 shape of a pre-split operand (3x3 / 1 / 1 over 64 channels, 128 x 64 tile): one strip per tap row.
    const bool strip = g_x6_strip && c.xs && c.KH == 3 && c.KW == 3 && c.stride == 1 && c.pad == 1 && c.dil == 1 &&
                       c.Ci == 64;
    // An fp32 operand (k_conv_x6 / k_conv_x6b) is staged by raw buffer loads (BUFA) where 32-bit offsets from a
    // per-workgroup base reach everything one tile can touch: span images of x (a tile of BM <= 128 output pixels
    // lies in at most BM / (Ho Wo) + 2 images) plus the padding bias of X6Desc, the same for x2, each below
    // 2^31 - 16 bytes, and a panel below 2 GiB.  Otherwise, and with BEV_TUNE_CONV_X6_BUF = 0, the pointer form.
    const int64_t span = std::min<int64_t>(c.N, 128 / ((int64_t)c.Ho * c.Wo) + 2);
    const int64_t kp2 = kpad_x(c.form == X6_DUAL ? c.Ci + c.Ci2 : c.Ci * c.KH * c.KW);
    const bool buf = g_x6_buf && c.x &&
                     span * c.H * c.W * c.Ci * 4 + (int64_t)c.pad * (c.W + 1) * c.Ci * 4 < X6_BUF_MAX &&
                     (!second || span * c.H2 * c.W2 * c.Ci2 * 4 < X6_BUF_MAX) &&
                     copad_x(c.Co) * kp2 * 6 < ((int64_t)1 << 31);
#define X6_PICK(K, ...) (buf ? K<__VA_ARGS__, true> : K<__VA_ARGS__, false>)
    // chain-next: its one (strip-staged) instance, whatever BEV_TUNE_CONV_X6_STRIP says
    if (next) return launch_x6(k_conv_x6s<4, 1, 1, 2, 3, true>, 128, 64, a, st);
    if (c.form == X6_CHAIN_DUAL && strip) return launch_x6(k_conv_x6s<4, 1, 1, 2, 2, true>, 128, 64, a, st);
    if (c.form == X6_CHAIN_DUAL)
        return launch_x6(c.xs ? k_conv_x6s<4, 1, 1, 2, 2> : X6_PICK(k_conv_x6b, 4, 1, 1, 2, false, 2, false), 128, 64, a,
                         st);
    if (c.form == X6_CHAIN && c.Co == 64 && strip) return launch_x6(k_conv_x6s<4, 1, 1, 2, 1, true>, 128, 64, a, st);
    if (c.form == X6_CHAIN && c.Co == 64)
        return launch_x6(c.xs ? k_conv_x6s<4, 1, 1, 2, 1> : X6_PICK(k_conv_x6b, 4, 1, 1, 2, false, 1, false), 128, 64, a,
                         st);
    if (c.form == X6_CHAIN)
        return launch_x6(c.xs ? k_conv_x6s<2, 2, 1, 2, 1> : X6_PICK(k_conv_x6b, 2, 2, 1, 2, false, 1, false), 64, 128, a,
                         st);
    // One conv (plain, dual): the 128 x 64 tile (t == 2) up to 64 output channels, else 128 x 128
    const bool dual = c.form == X6_DUAL;
    a.nta = g_x6_nt;
    const int t = g_x6_tile ? g_x6_tile : (a.Co <= 64 ? 2 : 1);
    if (a.xs) return t == 2 ? launch_x6(k_conv_x6s<4, 1, 1, 2>, 128, 64, a, st)
                            : launch_x6(k_conv_x6s<2, 2, 2, 2>, 128, 128, a, st);
    // automatic = the 32-deep-step kernel wherever it applies: single 1x1 layers measured faster on the 16-deep
    // kernel in isolation, but the ResNet-50 encoder (two stream groups) is fastest with the 32-deep kernel
    // everywhere (r03 tools/trunk_ab.py: 16.24 ms vs 16.34 with 1x1 / dual layers on the 16-deep one, 16.43 all)
    const bool wide = a.Ci % YBK == 0 && (!dual || a.Ci2 % YBK == 0) && g_x6_kernel != 1;
    if (wide && t == 2 && !dual && a.nta)
        return launch_x6(X6_PICK(k_conv_x6b, 4, 1, 1, 2, false, 0, true), 128, 64, a, st);
    if (wide && t == 2)
        return launch_x6(dual ? X6_PICK(k_conv_x6b, 4, 1, 1, 2, true, 0, false)
                              : X6_PICK(k_conv_x6b, 4, 1, 1, 2, false, 0, false), 128, 64, a, st);
    if (wide)
        return launch_x6(dual ? X6_PICK(k_conv_x6b, 2, 2, 2, 2, true, 0, false)
                              : X6_PICK(k_conv_x6b, 2, 2, 2, 2, false, 0, false), 128, 128, a, st);
    if (t == 2)
        return launch_x6(dual ? X6_PICK(k_conv_x6, 4, 1, 1, 2, true) : X6_PICK(k_conv_x6, 4, 1, 1, 2, false), 128, 64,
                         a, st);
    return launch_x6(dual ? X6_PICK(k_conv_x6, 2, 2, 2, 2, true) : X6_PICK(k_conv_x6, 2, 2, 2, 2, false), 128, 128, a,
                     st);
#undef X6_PICK
}

// ---------------------------------------------------------------------------
// ResNet stem (7x7 / stride 2 / pad 3 over Ci = 3 NCHW images, Co <= 64) on the split arithmetic
// ---------------------------------------------------------------------------
// timm conv1 (cnn_encoder.py:26; first layer of CNNEncoder._encode_single) -- the same contract as bev_conv.hip's
// exact-f32 k_stem, with the products of the other trunk layers: per 16-deep k slice six v_mfma_f32_32x32x16_bf16
// (32 cycles each) instead of eight v_mfma_f32_32x32x2_f32 (64 cycles), 2.67x fewer matrix-core cycles.
// Workgroup = 8 waves, tile = 8 output rows x 64 columns x 64 channels, wave w owns output row w (2 x 2 MFMA tiles
// of 32 pixels x 32 channels).
// K order inside the kernel: k' = (ky, ci, kx8) -- 21 runs (ky, ci) of 8 slots, slots 0..6 = kx, slot 7 padding; a
// 16-deep slice is two runs, half-wave h of slice sl takes run 2 sl + h: 22 runs = 11 slices, the 22nd run padding.
// A lane's 8 fragment elements are then 8 CONTIGUOUS input columns of one patch row (stride 2: output column ox,
// slot j = patch column 2 ox + j).  The tile's input patch (3 ch x 21 rows x 133 cols) is split into h / m / l once,
// when it is written to LDS (each input value serves ~12 (tap, pixel) products), as three row-major bf16 planes
// [ci][row][PITCH], so a plane's A fragment is 16 contiguous bytes at the dword 32 mt + r32 of its row: two
// ds_read2_b32 (dword alignment is all they need) straight into the registers the MFMA reads -- per slice one select
// of the half-wave's run offset and no per-element packing (the (ky, kx, ci) order this replaced cost one select,
// two LDS reads and ~5 shift / and / perm per element: ~190 VALU for a slice's 24 MFMAs).
// Padding that must not leak: slot 7 is patch column 2 ox + 7, input column 2 ox + 4 -- OUTSIDE the pixel's 7x7 field
// (and, for ox = 63, the never-written column 133) -- so a NaN / Inf there times its zero weight would be a NaN
// outside the receptive field: that half-dword is cleared in every plane fragment (one v_and each).  The padded 22nd
// run reads run 0 (inside the field) against zero weights.
// The weights come as the generic split panel (k = (ky, kx, ci), 147 -> 160); its first two 32-column blocks are
// permuted into the k' order while they are copied into LDS, once per persistent workgroup
// ([cb 2][slice 11][plane 3][lane 64][8], 66 KiB, slot 7 and run 21 zero), so B fragments are conflict-free
// ds_read_b128.  Persistent over tiles; the next tile's patch is fetched into registers during the MFMAs.
// fp32-tolerance equal to k_stem (summation order), as every split conv is to its exact-f32 counterpart.
namespace stem6 {
constexpr int TW = 64, TH = 8, NTHR = 512;
constexpr int PR = 2 * TH + 5;  // 21 input rows
constexpr int PC = 2 * TW + 5;  // 133 input columns
// Row pitch in bf16: >= 134 (slot 7 of output column 63 is column 133) and even (rows start on a dword).  A
// ds_read2_b32 is served as two ds_read_b32, each in two groups of 32 lanes with banks (a / 4) mod 32: the two
// half-waves (different runs, so different rows) are different groups and never conflict whatever the pitch, and a
// half-wave's 32 lanes read 32 consecutive dwords -- conflict-free.  136 = the smallest such pitch that also starts
// every row on a 16-byte boundary.
constexpr int PITCH = 136;
constexpr int PLANE = 3 * PR * PITCH;  // bf16 per plane
constexpr int PER_T = 17;              // patch elements staged per thread (stem6_fetch)
constexpr int NRUN = 3 * 7;           // (ky, ci) runs
constexpr int NS = (NRUN + 2) / 2;    // 11 16-deep k' slices
constexpr int WB = 2 * NS * 3 * 512;  // bf16 of the two permuted 32-column blocks
constexpr int S_PANEL = 10;           // the generic panel's slices (147 -> 160)
// bf16 offset of run (ky, ci) = (run / 3, run % 3) relative to the patch row of output row 0; the padded run reads run 0
__host__ __device__ constexpr int roff(int run) { return run >= NRUN ? 0 : ((run % 3) * PR + run / 3) * PITCH; }
static_assert(PITCH >= 2 * TW + 6 && PITCH % 2 == 0, "slot 7 of the last output column inside the row");
static_assert(4 * 34 * 64 * 4 <= 3 * PLANE * 2, "the pool epilogue's row exchange fits in the patch");
}  // namespace stem6

struct StemX6Args {
    const float *__restrict__ x;
    const __bf16 *__restrict__ wp;
    const float *__restrict__ bias;
    float *__restrict__ y;  // the stem output [N, Ho, Wo, Co], or (POOL) the max-pooled one [N, Hp, Wp, 64]
    int H, W, Co, Ho, Wo, relu, nTx, nTy;
    int64_t ntiles;
    // POOL only: per tile, the horizontally pooled last stem row (the next tile row's pooled row 0 needs it:
    // [ntiles][32][64]) and the last stem column's vertical window maxima for pooled rows 0..4 ([ntiles][5][64])
    float *__restrict__ edge_b, *__restrict__ edge_r;
    int Hp, Wp;
};

// Which patch elements a thread stages (the same for every tile, so a tile costs no index arithmetic beyond its
// origin): column c = tid & 127 of the 63 plane rows cr = ci * 21 + r = (tid >> 7) + 4 i, i = 0..15, and, as element 16,
// one of the 63 x 5 elements of columns 128..132 (row tid >> 3, column 128 + (tid & 7)).  Elements outside the image
// (the conv's zero padding) or outside the patch are loaded from the image's first pixel and zeroed at stem6_put by
// the returned mask (bit i = element i is a pixel of the image).
__device__ __forceinline__ unsigned stem6_fetch(const StemX6Args &a, int64_t t, int tid, float (&pv)[stem6::PER_T]) {
    using namespace stem6;
    const int tx = (int)(t % a.nTx);
    const int64_t r_ = t / a.nTx;
    const int ty = (int)(r_ % a.nTy);
    const int64_t img = r_ / a.nTy;
    const int row0 = 2 * ty * TH - 3, col0 = 2 * tx * TW - 3;
    const float *xi = a.x + img * 3 * (int64_t)a.H * a.W;
    unsigned in = 0;
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
        const int cr = i < PER_T - 1 ? (tid >> 7) + 4 * i : tid >> 3;
        const int c = i < PER_T - 1 ? (tid & 127) : 2 * TW + (tid & 7);
        const int ci = (cr >= PR) + (cr >= 2 * PR), r = cr - ci * PR;
        const int gy = row0 + r, gx = col0 + c;
        const bool ok = cr < 3 * PR && c < PC && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        pv[i] = xi[ok ? ((int64_t)ci * a.H + gy) * a.W + gx : 0];
        in |= (unsigned)ok << i;
    }
    return in;
}

// split once, when the patch is written: three ds_write_b16 per element at compile-time offsets of the thread's base
__device__ __forceinline__ void stem6_put(__bf16 *pl, int tid, const float (&pv)[stem6::PER_T], unsigned in) {
    using namespace stem6;
    __bf16 *q = pl + (tid >> 7) * PITCH + (tid & 127);
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
        const bool last = i == PER_T - 1;
        // plane row 4 i + (tid >> 7) exists (i = 15: rows 60..62); the tail element is a column < 133 of a row < 63
        if (last ? (tid >> 3) < 3 * PR && (tid & 7) < PC - 2 * TW : i < PER_T - 2 || (tid >> 7) < 3 * PR - 4 * i) {
            __bf16 *o = last ? pl + (tid >> 3) * PITCH + 2 * TW + (tid & 7) : q + 4 * i * PITCH;
            __bf16 hh, mm, ll;
            split3((in >> i) & 1u ? pv[i] : 0.0f, hh, mm, ll);
            o[0] = hh;
            o[PLANE] = mm;
            o[2 * PLANE] = ll;
        }
    }
}

// the pooled maximum of relu'd stem values (>= +0, or NaN: the ReLU keeps a NaN and so does this maximum, as
// k_maxpool_rows and torch's max_pool2d do)
__device__ __forceinline__ float pool_mx(float m, float v) { return max_nan(m, v); }

// POOL: timm's stem max-pool (3x3 / s2 / p1, cnn_encoder.py:26 features_only) fused into the epilogue.  The stem
// output is relu'd (>= +0), so a window's padding and the tile's rows / columns past the image may count as +0 without
// changing any maximum: every pooled value is the max over a set of non-negative values, whatever the grouping --
// bit-identical to k_maxpool_rows over the stem output.  A NaN stem value (a NaN or Inf pixel under it) makes every
// pooled value whose window holds it NaN, in any grouping too: pool_mx keeps a NaN, as k_maxpool_rows does.  Tile (ty, tx) = stem rows 8ty..8ty+7 x columns
// 64tx..64tx+63 owns pooled rows 4ty..4ty+3 x columns 32tx..32tx+31; pooled row 4ty needs stem row 8ty-1 (tile ty-1)
// and pooled column 32tx stem column 64tx-1 (tile tx-1): each tile stores its own part of those seam outputs and
// exports its last row / column parts (edge_b / edge_r), which k_stem_pool_seams folds in afterwards.
// Lane (h, r32) holds channel r32 (+32) of stem columns 32mt + 8b + 4h + u (u = 0..3): pooled columns 16mt + 4b + 2h
// (+1) are 3-maxima of its own values and, for the even one, the other half-wave's u = 3 value of the preceding
// group (a cross-half shuffle); wave w = stem row w: the odd waves hand their 34 row maxima to the even ones through
// LDS, the even wave 2p combines rows 2p-1..2p+1 into pooled row p.
template <bool POOL>
__global__ __launch_bounds__(stem6::NTHR, 1) void k_stem_x6(StemX6Args a) {
    using namespace stem6;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[WB * 2 + 3 * PLANE * 2];
    __bf16 *wl = (__bf16 *)lds_raw;
    __bf16 *pl = (__bf16 *)(lds_raw + WB * 2);  // the h, m, l planes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
    // the split panel's blocks 0 and 1, permuted from k = (ky, kx, ci) into [cb][slice][plane][64 lanes][8] of the k'
    // order: fragment lane (h, n) of slice sl holds run 2 sl + h of channel 32 cb + n, slot 7 and run 21 zero
    for (int f = tid; f < WB / 8; f += NTHR) {
        const int ln = f & 63, fr = f >> 6, p = fr % 3, sl = (fr / 3) % NS, cb = fr / (3 * NS);
        const int run = 2 * sl + (ln >> 5), ky = run / 3, ci = run - 3 * ky, n = 32 * cb + (ln & 31);
        const unsigned short *src = reinterpret_cast<const unsigned short *>(a.wp);
        unsigned w[8];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
            w[kx] = run < NRUN ? (unsigned)src[frag_index(n, (ky * 7 + kx) * 3 + ci, p, S_PANEL)] : 0u;
        reinterpret_cast<u32x4 *>(wl)[f] = (u32x4){w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6]};
    }
    float pv[PER_T];
    int64_t t = blockIdx.x;
    unsigned pin = stem6_fetch(a, t < a.ntiles ? t : 0, tid, pv);
    stem6_put(pl, tid, pv, pin);
    __syncthreads();

    // output row `wave`, column r32 (+ 32 for the second M tile): slot 0 of run 0 in the h plane
    const __bf16 *P = pl + wave * 2 * PITCH + 2 * r32;
    const float b0 = (r32 < a.Co) ? a.bias[r32] : 0.0f;
    const float b1 = (32 + r32 < a.Co) ? a.bias[32 + r32] : 0.0f;
    for (; t < a.ntiles; t += gridDim.x) {
        const int64_t tn = t + gridDim.x;
        pin = stem6_fetch(a, tn < a.ntiles ? tn : t, tid, pv);  // in flight during the MFMAs
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            int hv = h;
            asm volatile("" : "+v"(hv));  // per slice: the run select stays one cndmask, not 11 hoisted lane offsets
            const __bf16 *Pr = P + (hv ? roff(2 * sl + 1) : roff(2 * sl));  // the half-wave's run
            int wo = lane * 8;
            asm volatile("" : "+v"(wo));  // per slice: the weight fragments are re-read, not held across tiles
            const __bf16 *wlb = wl + wo;  // (the offset, not the pointer, is opaque: the reads stay ds_read_b128)
            bf16x8 fb[2][3];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    fb[j][p] = *(const bf16x8 *)(wlb + ((j * NS + sl) * 3 + p) * 512);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                bf16x8 fa[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    // slots 0..7 = patch columns 2 ox .. 2 ox + 7 of the run's row; slot 7 (outside the field) cleared
                    const unsigned *q = reinterpret_cast<const unsigned *>(Pr + p * PLANE + 64 * mt);
                    fa[p] = __builtin_bit_cast(bf16x8, (u32x4){q[0], q[1], q[2], q[3] & 0xffffu});
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) x6_dot(acc[mt][j], fa, fb[j]);
            }
            __builtin_amdgcn_sched_barrier(0);  // one slice of operands live at a time
        }
        // epilogue: D[row][col], col = channel r32 (+32), row = pixel (r & 3) + 8 (r >> 2) + 4 h (+32)
        if constexpr (POOL) {
            const int tx = (int)(t % a.nTx);
            const int64_t r_ = t / a.nTx;
            const int ty = (int)(r_ % a.nTy);
            const int64_t img = r_ / a.nTy;
            const int oy = ty * TH + wave;
            const int oxb = tx * TW;
            float hp[2][4][2][2];  // [mt][b][pc][j]: pooled column 16 mt + 4 b + 2 h + pc, channel r32 + 32 j
            float pa3[2][2][4];    // the other half-wave's u = 3 value of group (mt, b)
            float c63[2];          // stem column 63 (lanes h = 1)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        float v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int ox = oxb + 32 * mt + 8 * b + 4 * h + u;
                            const float z = acc[mt][j][4 * b + u] + (j ? b1 : b0);
                            v[u] = oy < a.Ho && ox < a.Wo ? relu_f(z) : 0.0f;  // the stem's ReLU (a NaN stays)
                        }
                        pa3[mt][j][b] = __shfl_xor(v[3], 32);
                        hp[mt][b][1][j] = pool_mx(pool_mx(v[1], v[2]), v[3]);
                        hp[mt][b][0][j] = pool_mx(v[0], v[1]);
                        if (mt == 1 && b == 3) c63[j] = v[3];
                    }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float prev0 = b > 0 ? pa3[mt][j][b - 1] : (mt > 0 ? pa3[mt - 1][j][3] : 0.0f);
                        hp[mt][b][0][j] = pool_mx(hp[mt][b][0][j], h ? pa3[mt][j][b] : prev0);
                    }
            __syncthreads();  // every wave is done reading the patch: its LDS holds the row exchange
            float *xl = reinterpret_cast<float *>(pl);  // [odd wave][34][64 lanes]
            if (wave & 1) {
                float *o = xl + (wave >> 1) * 34 * 64 + lane;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int pc = 0; pc < 2; ++pc)
#pragma unroll
                            for (int j = 0; j < 2; ++j) o[(((mt * 4 + b) * 2 + pc) * 2 + j) * 64] = hp[mt][b][pc][j];
                o[32 * 64] = c63[0];
                o[33 * 64] = c63[1];
            }
            __syncthreads();
            // the row above (p = 0 has none: it re-reads the row below, unused) and below: all 68 reads issued before
            // the first maximum, not one LDS round trip per value
            const int p = wave >> 1;
            float uv[34], dv[34];
            if (!(wave & 1)) {
                const float *up = xl + (p > 0 ? p - 1 : p) * 34 * 64 + lane, *dn = xl + p * 34 * 64 + lane;
#pragma unroll
                for (int e = 0; e < 34; ++e) {
                    dv[e] = dn[e * 64];
                    uv[e] = up[e * 64];
                }
            }
            // The next patch goes into LDS BEFORE this tile's stores are issued: stem6_put waits for its loads with
            // counted vmcnt, which -- loads and stores sharing that counter, in order -- would wait for every store
            // issued after them too (a store's round trip per tile, on all eight waves).  Issued last, the stores
            // drain during the next tile's MFMAs.
            __syncthreads();  // the row exchange is read
            stem6_put(pl, tid, pv, pin);
            const int64_t tile = t;
            if (wave == TH - 1) {  // the last row: next tile row's pooled row 0, and column 63 alone (pooled row 4)
                float *eb = a.edge_b + tile * (32 * 64);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int pc = 0; pc < 2; ++pc)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
                                eb[(16 * mt + 4 * b + 2 * h + pc) * 64 + r32 + 32 * j] = hp[mt][b][pc][j];
                if (h) {
                    a.edge_r[(tile * 5 + 4) * 64 + r32] = c63[0];
                    a.edge_r[(tile * 5 + 4) * 64 + 32 + r32] = c63[1];
                }
            } else if (!(wave & 1)) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int pc = 0; pc < 2; ++pc)
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const int e = ((mt * 4 + b) * 2 + pc) * 2 + j;
                                const float m = pool_mx(hp[mt][b][pc][j], dv[e]);
                                hp[mt][b][pc][j] = p > 0 ? pool_mx(m, uv[e]) : m;
                            }
                float e0 = pool_mx(c63[0], dv[32]), e1 = pool_mx(c63[1], dv[33]);
                if (p > 0) {
                    e0 = pool_mx(e0, uv[32]);
                    e1 = pool_mx(e1, uv[33]);
                }
                if (h) {
                    a.edge_r[(tile * 5 + p) * 64 + r32] = e0;
                    a.edge_r[(tile * 5 + p) * 64 + 32 + r32] = e1;
                }
                const int prow = ty * (TH / 2) + p;
                if (prow < a.Hp) {
                    float *yr = a.y + ((img * a.Hp + prow) * (int64_t)a.Wp) * 64;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int b = 0; b < 4; ++b)
#pragma unroll
                            for (int pc = 0; pc < 2; ++pc) {
                                const int Q = tx * (TW / 2) + 16 * mt + 4 * b + 2 * h + pc;
                                if (Q < a.Wp) {
                                    yr[(int64_t)Q * 64 + r32] = hp[mt][b][pc][0];
                                    yr[(int64_t)Q * 64 + 32 + r32] = hp[mt][b][pc][1];
                                }
                            }
                }
            }
        } else {
            const int tx = (int)(t % a.nTx);
            const int64_t r_ = t / a.nTx;
            const int ty = (int)(r_ % a.nTy);
            const int64_t img = r_ / a.nTy;
            const int oy = ty * TH + wave;
            const int oxb = tx * TW;
            __syncthreads();  // every wave is done reading the patch
            stem6_put(pl, tid, pv, pin);  // before the stores, as in the pooled form
            if (oy < a.Ho) {
                float *yr = a.y + ((img * a.Ho + oy) * (int64_t)a.Wo) * a.Co;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ox = oxb + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (ox < a.Wo) {
                            float v0 = acc[mt][0][r] + b0, v1 = acc[mt][1][r] + b1;
                            if (a.relu) {
                                v0 = relu_f(v0);
                                v1 = relu_f(v1);
                            }
                            float *yp = yr + (int64_t)ox * a.Co;
                            if (r32 < a.Co) yp[r32] = v0;
                            if (32 + r32 < a.Co) yp[32 + r32] = v1;
                        }
                    }
            }
        }
        __syncthreads();  // the next patch is in LDS
    }
}

// The seam outputs of the fused stem max-pool: pooled row 4ty of tile (ty, tx) takes edge_b of tile (ty-1, tx),
// pooled column 32tx edge_r of tile (ty, tx-1), their corner edge_r row 4 of tile (ty-1, tx-1).  One thread per
// (tile, seam output, 4 channels): 35 seam outputs (32 columns of row 0, rows 1..3 of column 0) x 16 float4.
__global__ __launch_bounds__(256) void k_stem_pool_seams(float *__restrict__ y, const float *__restrict__ edge_b,
                                                         const float *__restrict__ edge_r, int nTx, int nTy,
                                                         int64_t ntiles, int Hp, int Wp) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t tile = g / (35 * 16);
    if (tile >= ntiles) return;
    const int k = (int)(g - tile * (35 * 16)), s = k >> 4, c4 = k & 15;
    const int tx = (int)(tile % nTx);
    const int64_t r_ = tile / nTx;
    const int ty = (int)(r_ % nTy);
    const int64_t img = r_ / nTy;
    const int p = s < 32 ? 0 : s - 31, q = s < 32 ? s : 0;
    const int P = ty * (stem6::TH / 2) + p, Q = tx * (stem6::TW / 2) + q;
    if (P >= Hp || Q >= Wp || (p == 0 && ty == 0 && (q > 0 || tx == 0))) return;  // no seam contribution
    float4 *yp = reinterpret_cast<float4 *>(y + (((img * Hp + P) * (int64_t)Wp + Q) * 64)) + c4;
    float4 m = *yp;
    auto mx = [](float4 a, float4 b) {
        return make_float4(pool_mx(a.x, b.x), pool_mx(a.y, b.y), pool_mx(a.z, b.z), pool_mx(a.w, b.w));
    };
    if (p == 0 && ty > 0) m = mx(m, reinterpret_cast<const float4 *>(edge_b + ((tile - nTx) * 32 + q) * 64)[c4]);
    if (q == 0 && tx > 0) {
        m = mx(m, reinterpret_cast<const float4 *>(edge_r + ((tile - 1) * 5 + p) * 64)[c4]);
        if (p == 0 && ty > 0)
            m = mx(m, reinterpret_cast<const float4 *>(edge_r + ((tile - nTx - 1) * 5 + 4) * 64)[c4]);
    }
    *yp = m;
}

// The stem kernels' arguments without the pooled form's edge buffers; one persistent workgroup per CU at most.
StemX6Args stem_x6_args(const float *x, int N, int H, int W, const uint16_t *packed, const float *bias, int Co,
                        int relu, float *y, int Ho, int Wo) {
    StemX6Args a;
    a.x = x, a.wp = (const __bf16 *)packed, a.bias = bias, a.y = y;
    a.H = H, a.W = W, a.Co = Co, a.Ho = Ho, a.Wo = Wo, a.relu = relu;
    a.nTx = (Wo + stem6::TW - 1) / stem6::TW;
    a.nTy = (Ho + stem6::TH - 1) / stem6::TH;
    a.ntiles = (int64_t)N * a.nTx * a.nTy;
    a.edge_b = a.edge_r = nullptr;
    a.Hp = a.Wp = 0;
    return a;
}
unsigned stem_x6_grid(const StemX6Args &a) { return (unsigned)(a.ntiles < cu_count() ? a.ntiles : cu_count()); }

}  // namespace

namespace bev {
int conv_x6_tune(int knob, int value) {
    if (knob == BEV_TUNE_CONV_X6_TILE) return swap_knob(g_x6_tile, value, 2);
    if (knob == BEV_TUNE_CONV_X6_STRIP) return swap_knob(g_x6_strip, value, 1);
    if (knob == BEV_TUNE_CONV_X6_BUF) return swap_knob(g_x6_buf, value, 1);
    return swap_knob(knob == BEV_TUNE_CONV_X6_NT ? g_x6_nt : g_x6_kernel, value, 1);
}
}  // namespace bev

extern "C" {

int64_t bev_conv_packed_size_x6(int Co, int Ci, int KH, int KW) {
    if (Co <= 0 || Ci <= 0 || KH <= 0 || KW <= 0) return BEV_ERR_ARGS;
    return copad_x(Co) * kpad_x(Ci * KH * KW) * 3;
}

int bev_conv_pack_weights_x6(const float *w, int Co, int Ci, int KH, int KW, uint16_t *packed, void *stream) {
    if (!w || !packed || Co <= 0 || Ci <= 0 || KH <= 0 || KW <= 0) return BEV_ERR_ARGS;
    const int64_t Kp = kpad_x(Ci * KH * KW), Cop = copad_x(Co), n = Kp * Cop;
    hipLaunchKernelGGL(k_pack_x6, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Co, Ci, KH,
                       KW, Kp, Cop, (__bf16 *)packed);
    return last();
}

int bev_conv2d_x6_f32(const float *x, const uint16_t *xs, int N, int H, int W, int Ci, const uint16_t *packed,
                      const float *bias, const float *residual, int Co, int KH, int KW, int stride, int pad,
                      int dilation, int act, float *y, uint16_t *ys, int ldy, int Ho, int Wo, void *stream) {
    X6Call c{X6_PLAIN};
    c.x = x, c.xs = xs, c.packed = packed, c.bias = bias, c.res = residual, c.y = y, c.ys = ys;
    c.N = N, c.H = H, c.W = W, c.Ci = Ci, c.Co = Co, c.KH = KH, c.KW = KW, c.stride = stride, c.pad = pad;
    c.dil = dilation, c.act = act, c.ldy = ldy, c.Ho = Ho, c.Wo = Wo;
    return conv_x6(c, (hipStream_t)stream);
}

int bev_split3_f32(const float *x, int64_t n, uint16_t *planes, void *stream) {
    if (!x || !planes || n < 0) return BEV_ERR_ARGS;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_split3, dim3((unsigned)((n + 511) / 512)), dim3(256), 0, (hipStream_t)stream, x, n,
                       (__bf16 *)planes);
    return last();
}

int bev_conv2d_dual_x6_f32(const float *x, int N, int Ho, int Wo, int Ci, const float *x2, int H2, int W2, int Ci2,
                           int stride2, const uint16_t *packed, const float *bias, int Co, int act, float *y,
                           void *stream) {
    X6Call c{X6_DUAL};  // the 1x1 / stride 1 conv over x [N][Ho][Wo][Ci], K continued with x2's channels
    c.x = x, c.packed = packed, c.bias = bias, c.y = y;
    c.N = N, c.H = c.Ho = Ho, c.W = c.Wo = Wo, c.Ci = Ci, c.Co = c.ldy = Co, c.act = act;
    c.x2 = x2, c.H2 = H2, c.W2 = W2, c.Ci2 = Ci2, c.stride2 = stride2;
    return conv_x6(c, (hipStream_t)stream);
}

int bev_conv2d_chain_x6_f32(const float *x, const uint16_t *xs, int N, int H, int W, int Ci,
                            const uint16_t *packed, const float *bias, int Co, int KH, int KW, int stride, int pad,
                            int act, const uint16_t *packed2, const float *bias2, int Co2, const float *residual,
                            int act2, float *y, int Ho, int Wo, void *stream) {
    X6Call c{X6_CHAIN};
    c.x = x, c.xs = xs, c.packed = packed, c.bias = bias, c.res = residual, c.y = y;
    c.N = N, c.H = H, c.W = W, c.Ci = Ci, c.Co = Co, c.KH = KH, c.KW = KW, c.stride = stride, c.pad = pad;
    c.act = act, c.Ho = Ho, c.Wo = Wo;
    c.packed2 = packed2, c.bias2 = bias2, c.Co2 = Co2, c.act2 = act2;
    return conv_x6(c, (hipStream_t)stream);
}

int bev_conv2d_chain_conv1_x6_f32(const float *x, const uint16_t *xs, int N, int H, int W, int Ci,
                                   const uint16_t *packed, const float *bias, int Co, int KH, int KW, int stride,
                                   int pad, int act, const uint16_t *packed2, const float *bias2, int Co2,
                                   const float *residual, int act2, float *y, const uint16_t *packed3,
                                   const float *bias3, int Co3, int act3, uint16_t *ys3, int Ho, int Wo, void *stream) {
    X6Call c{X6_CHAIN_NEXT};
    c.x = x, c.xs = xs, c.packed = packed, c.bias = bias, c.res = residual, c.y = y, c.ys = ys3;
    c.N = N, c.H = H, c.W = W, c.Ci = Ci, c.Co = Co, c.KH = KH, c.KW = KW, c.stride = stride, c.pad = pad;
    c.act = act, c.Ho = Ho, c.Wo = Wo;
    c.packed2 = packed2, c.bias2 = bias2, c.Co2 = Co2, c.act2 = act2;
    c.packed3 = packed3, c.bias3 = bias3, c.Co3 = Co3, c.act3 = act3;
    return conv_x6(c, (hipStream_t)stream);
}

int bev_conv2d_chain_dual_x6_f32(const float *x, const uint16_t *xs, int N, int H, int W, int Ci,
                                 const uint16_t *packed, const float *bias, int Co, int KH, int KW, int stride,
                                 int pad, int act, const float *x2, int H2, int W2, int Ci2, int stride2,
                                 const uint16_t *packed2, const float *bias2, int Co2, int act2, float *y, int Ho,
                                 int Wo, void *stream) {
    X6Call c{X6_CHAIN_DUAL};
    c.x = x, c.xs = xs, c.packed = packed, c.bias = bias, c.y = y;
    c.N = N, c.H = H, c.W = W, c.Ci = Ci, c.Co = Co, c.KH = KH, c.KW = KW, c.stride = stride, c.pad = pad;
    c.act = act, c.Ho = Ho, c.Wo = Wo;
    c.x2 = x2, c.H2 = H2, c.W2 = W2, c.Ci2 = Ci2, c.stride2 = stride2;
    c.packed2 = packed2, c.bias2 = bias2, c.Co2 = Co2, c.act2 = act2;
    return conv_x6(c, (hipStream_t)stream);
}

int bev_conv2d_stem_x6_f32(const float *x, int N, int H, int W, const uint16_t *packed, const float *bias, int Co,
                           int relu, float *y, int Ho, int Wo, void *stream) {
    if (!x || !packed || !bias || !y || N <= 0 || H <= 0 || W <= 0 || Co <= 0 || Co > 64 ||
        Ho != conv_out(H, 3, 1, 7, 2) || Wo != conv_out(W, 3, 1, 7, 2) || (((uintptr_t)packed) & 15) != 0)
        return BEV_ERR_ARGS;
    const StemX6Args a = stem_x6_args(x, N, H, W, packed, bias, Co, relu, y, Ho, Wo);
    hipLaunchKernelGGL(k_stem_x6<false>, dim3(stem_x6_grid(a)), dim3(stem6::NTHR), 0, (hipStream_t)stream, a);
    return last();
}

int64_t bev_conv2d_stem_pool_x6_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return BEV_ERR_ARGS;
    const StemX6Args a = stem_x6_args(nullptr, N, H, W, nullptr, nullptr, 64, 1, nullptr, conv_out(H, 3, 1, 7, 2),
                                      conv_out(W, 3, 1, 7, 2));
    return a.ntiles * (32 + 5) * 64 * (int64_t)sizeof(float);
}

int bev_conv2d_stem_pool_x6_f32(const float *x, int N, int H, int W, const uint16_t *packed, const float *bias,
                                int Co, float *y, int Hp, int Wp, void *workspace, int64_t workspace_bytes,
                                void *stream) {
    const int Ho = conv_out(H, 3, 1, 7, 2), Wo = conv_out(W, 3, 1, 7, 2);
    if (!x || !packed || !bias || !y || !workspace || N <= 0 || H <= 0 || W <= 0 || Co != 64 ||
        Hp != conv_out(Ho, 1, 1, 3, 2) || Wp != conv_out(Wo, 1, 1, 3, 2) ||
        (((uintptr_t)packed | (uintptr_t)y | (uintptr_t)workspace) & 15) != 0)
        return BEV_ERR_ARGS;
    if (workspace_bytes < bev_conv2d_stem_pool_x6_workspace(N, H, W)) return BEV_ERR_ARGS;
    StemX6Args a = stem_x6_args(x, N, H, W, packed, bias, Co, 1, y, Ho, Wo);
    a.edge_b = (float *)workspace;
    a.edge_r = a.edge_b + a.ntiles * 32 * 64;
    a.Hp = Hp, a.Wp = Wp;
    hipLaunchKernelGGL(k_stem_x6<true>, dim3(stem_x6_grid(a)), dim3(stem6::NTHR), 0, (hipStream_t)stream, a);
    const int64_t nthr = a.ntiles * 35 * 16;
    hipLaunchKernelGGL(k_stem_pool_seams, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y,
                       a.edge_b, a.edge_r, a.nTx, a.nTy, a.ntiles, Hp, Wp);
    return last();
}

}  // extern "C"
