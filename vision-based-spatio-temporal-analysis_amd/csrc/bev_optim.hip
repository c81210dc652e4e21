// bev_optim.hip -- the Adam / AdamW parameter update of the reference's training step (train.py:46-52, 238-255) for
// every tensor of a parameter group in one launch, aware of GradScaler's device scalars: no host read of found_inf,
// no launch per tensor and per op.  The arithmetic is csrc/bev_optim.h, shared with bev_adam_step_host.
//
//   k_adam_step    one workgroup of 256 threads per chunk of bev_optim::CHUNK (2048) elements; a tensor of n elements
//                  owns max(1, ceil(n / CHUNK)) consecutive chunks starting at its record's first-chunk word, and a
//                  workgroup finds its tensor by bisection over those words (uniform loads of a table that stays in
//                  the scalar cache).
//     traffic      28 B per element (p, g, m, v read; p, m, v written), nothing to reuse: the 16-byte loads of a
//                  chunk -- two per lane and array, 32 KiB per workgroup -- are all issued before the first use, and
//                  the per-step scalars (two integer powers, a division and a root in double) are computed behind
//                  them.  Plain stores: p, m and v are read again by the next step.
//     paths        16-byte loads and stores when p, g, m and v of the tensor are all 16-B aligned (chunks start at
//                  multiples of 2048 elements, so alignment carries over), with the last n % 4 elements as dwords;
//                  a dword path for tensors that are only 4-B aligned (views into a flat bucket)
//                  and for tensors of fewer than four elements.
//     steps        a workgroup reads its tensor's counter from step_in; the tensor's first workgroup alone writes
//                  step_out, a different buffer, so no workgroup reads what another of the launch writes.
//     found_inf    non-zero (or NaN): step_out = step_in and nothing else is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bev_mi355x.h"
#include "bev_optim.h"

namespace {

namespace bo = bev_optim;

constexpr int OT = 256;                     // threads per workgroup (4 waves)
constexpr int VPT = bo::CHUNK / (4 * OT);   // 16-byte groups per lane and array
constexpr int EPT = bo::CHUNK / OT;         // elements per lane on the dword path
typedef __attribute__((address_space(1))) float gfloat;     // the table's pointers are global memory: no flat loads
typedef float nfloat4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) nfloat4 gfloat4;
static_assert(VPT * 4 * OT == bo::CHUNK && VPT >= 1, "a chunk is a whole number of 16-byte groups per lane");

__device__ __forceinline__ void update4(const bo::Hyper &h, const bo::StepScalars &s, bool scaled, float inv,
                                        nfloat4 &P, nfloat4 G, nfloat4 &M, nfloat4 &V) {
    float p[4] = {P.x, P.y, P.z, P.w}, m[4] = {M.x, M.y, M.z, M.w}, v[4] = {V.x, V.y, V.z, V.w};
    const float g[4] = {G.x, G.y, G.z, G.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) bo::update(h, s, scaled, inv, p[j], g[j], m[j], v[j]);
    P = nfloat4{p[0], p[1], p[2], p[3]};
    M = nfloat4{m[0], m[1], m[2], m[3]};
    V = nfloat4{v[0], v[1], v[2], v[3]};
}

__global__ __launch_bounds__(OT) void k_adam_step(const int64_t *__restrict__ table, int T, bo::Hyper h,
                                                  const float *__restrict__ grad_scale,
                                                  const float *__restrict__ found_inf) {
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    // the last tensor whose first chunk is <= c (workgroup-uniform)
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)mid * bo::REC_WORDS + bo::REC_CHUNK0] <= c) lo = mid;
        else hi = mid - 1;
    }
    const int64_t *rec = table + (int64_t)lo * bo::REC_WORDS;
    const int64_t local = c - rec[bo::REC_CHUNK0];
    const int64_t n = rec[bo::REC_N];
    if (local < 0 || local > (INT64_MAX / bo::CHUNK)) return;  // not a chunk of this table
    const int64_t start = local * bo::CHUNK;
    if (local > 0 && start >= n) return;  // past the tensor's end (its first chunk still counts the step)
    const float step = *(const gfloat *)(uintptr_t)rec[bo::REC_STEP_IN];
    const bool skip = found_inf != nullptr && !(*found_inf == 0.0f);
    if (local == 0 && tid == 0) *(gfloat *)(uintptr_t)rec[bo::REC_STEP_OUT] = skip ? step : step + 1.0f;
    if (skip || start >= n) return;
    const int len = n - start < bo::CHUNK ? (int)(n - start) : bo::CHUNK;
    gfloat *p = (gfloat *)(uintptr_t)rec[bo::REC_P] + start;
    const gfloat *g = (const gfloat *)(uintptr_t)rec[bo::REC_G] + start;
    gfloat *m = (gfloat *)(uintptr_t)rec[bo::REC_M] + start;
    gfloat *v = (gfloat *)(uintptr_t)rec[bo::REC_V] + start;
    const bool scaled = grad_scale != nullptr;
    const bool vec = ((rec[bo::REC_P] | rec[bo::REC_G] | rec[bo::REC_M] | rec[bo::REC_V]) & 15) == 0;
    // Loads are unconditional at an index clamped into the chunk, stores are guarded: every load of the chunk is in
    // flight before the first wait, whatever the chunk's length.
    if (vec && len >= 4) {
        const int nvec = len >> 2;
        nfloat4 P[VPT], G[VPT], M[VPT], V[VPT];
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int i = min(tid + k * OT, nvec - 1);
            P[k] = ((const gfloat4 *)p)[i];
            G[k] = ((const gfloat4 *)g)[i];
            M[k] = ((const gfloat4 *)m)[i];
            V[k] = ((const gfloat4 *)v)[i];
        }
        const int e = min(4 * nvec + tid, len - 1);  // the tail: at most three elements
        float tp = p[e], tg = g[e], tm = m[e], tv = v[e];
        const bo::StepScalars s = bo::step_scalars(h, step);
        const float inv = scaled ? bo::inv_scale(*grad_scale) : 1.0f;
#pragma unroll
        for (int k = 0; k < VPT; ++k) update4(h, s, scaled, inv, P[k], G[k], M[k], V[k]);
        bo::update(h, s, scaled, inv, tp, tg, tm, tv);
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int i = tid + k * OT;
            if (i < nvec) {
                ((gfloat4 *)p)[i] = P[k];
                ((gfloat4 *)m)[i] = M[k];
                ((gfloat4 *)v)[i] = V[k];
            }
        }
        if (4 * nvec + tid < len) {
            p[e] = tp;
            m[e] = tm;
            v[e] = tv;
        }
    } else {
        float P[EPT], G[EPT], M[EPT], V[EPT];
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int i = min(tid + k * OT, len - 1);
            P[k] = p[i];
            G[k] = g[i];
            M[k] = m[i];
            V[k] = v[i];
        }
        const bo::StepScalars s = bo::step_scalars(h, step);
        const float inv = scaled ? bo::inv_scale(*grad_scale) : 1.0f;
#pragma unroll
        for (int k = 0; k < EPT; ++k) bo::update(h, s, scaled, inv, P[k], G[k], M[k], V[k]);
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int i = tid + k * OT;
            if (i < len) {
                p[i] = P[k];
                m[i] = M[k];
                v[i] = V[k];
            }
        }
    }
}

// the checks the entries share; 0 when the arguments are usable, 1 for the no-op
int check_args(const void *table, int T, double beta1, double beta2) {
    if (T < 0) return BEV_ERR_ARGS;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return BEV_ERR_ARGS;
    if (T == 0) return 1;
    if (!table || ((uintptr_t)table & 7)) return BEV_ERR_ARGS;
    return 0;
}

}  // namespace

extern "C" {

int64_t bev_adam_table_bytes(int T) { return T <= 0 ? 0 : (int64_t)T * bo::REC_WORDS * (int64_t)sizeof(int64_t); }

int bev_adam_chunk_elems(void) { return bo::CHUNK; }

int bev_adam_step_f32(const void *table_dev, int T, int64_t total_chunks, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int decoupled, const float *grad_scale_dev,
                      const float *found_inf_dev, void *stream) {
    const int rc = check_args(table_dev, T, beta1, beta2);
    if (rc) return rc < 0 ? rc : 0;
    if (total_chunks < T || total_chunks > INT32_MAX) return BEV_ERR_ARGS;  // every tensor owns at least one chunk
    const bo::Hyper h = bo::make_hyper(lr, beta1, beta2, eps, weight_decay, decoupled);
    hipLaunchKernelGGL(k_adam_step, dim3((unsigned)total_chunks), dim3(OT), 0, (hipStream_t)stream,
                       (const int64_t *)table_dev, T, h, grad_scale_dev, found_inf_dev);
    return (int)hipGetLastError();
}

int bev_adam_step_host(const void *table_host, int T, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int decoupled, const float *grad_scale, const float *found_inf) {
    const int rc = check_args(table_host, T, beta1, beta2);
    if (rc) return rc < 0 ? rc : 0;
    const int64_t *table = (const int64_t *)table_host;
    for (int t = 0; t < T; ++t) {
        const int64_t *rec = table + (int64_t)t * bo::REC_WORDS;
        if (rec[bo::REC_N] < 0 || !rec[bo::REC_STEP_IN] || !rec[bo::REC_STEP_OUT]) return BEV_ERR_ARGS;
        if (rec[bo::REC_N] > 0 && (!rec[bo::REC_P] || !rec[bo::REC_G] || !rec[bo::REC_M] || !rec[bo::REC_V]))
            return BEV_ERR_ARGS;
    }
    const bo::Hyper h = bo::make_hyper(lr, beta1, beta2, eps, weight_decay, decoupled);
    const bool skip = found_inf != nullptr && !(*found_inf == 0.0f);
    const bool scaled = grad_scale != nullptr;
    const float inv = scaled ? bo::inv_scale(*grad_scale) : 1.0f;
    for (int t = 0; t < T; ++t) {
        const int64_t *rec = table + (int64_t)t * bo::REC_WORDS;
        const float step = *(const float *)(uintptr_t)rec[bo::REC_STEP_IN];
        *(float *)(uintptr_t)rec[bo::REC_STEP_OUT] = skip ? step : step + 1.0f;
        if (skip) continue;
        float *p = (float *)(uintptr_t)rec[bo::REC_P];
        const float *g = (const float *)(uintptr_t)rec[bo::REC_G];
        float *m = (float *)(uintptr_t)rec[bo::REC_M];
        float *v = (float *)(uintptr_t)rec[bo::REC_V];
        const bo::StepScalars s = bo::step_scalars(h, step);
        for (int64_t i = 0; i < rec[bo::REC_N]; ++i) bo::update(h, s, scaled, inv, p[i], g[i], m[i], v[i]);
    }
    return 0;
}

}  // extern "C"
