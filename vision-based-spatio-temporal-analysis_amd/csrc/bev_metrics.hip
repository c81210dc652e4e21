// bev_metrics.hip -- the validation scoring of the reference's loop (train.py:78-104, compute_metrics) for a whole
// batch in one launch, on the decode's own output buffers: per frame TP / FP / FN and the sum of the matched
// distances.  The reference walks every prediction in Python and reads min_dist.item() for each -- one host
// synchronisation per prediction when the detections are device tensors.
//
// The greedy pass is only apparently sequential.  A prediction's nearest ground truth (d_i, j_i) does not depend on
// which ground truths are used, and the true positive of ground truth j is the lowest i with j_i == j and d_i within
// the threshold (every later such i finds j used and is a false positive; there is no second try).  So:
//
//   k_det_match    one workgroup per frame.
//     1. nearest   each thread owns predictions tid, tid + 256, ...; the frame's ground truths pass through LDS
//                  MT_CHUNK at a time (any G: a frame that fits one chunk is staged once) and every thread visits
//                  them in ascending index, which is where the first-index and NaN rules live (bev_metrics.h).  A
//                  prediction within the threshold does an integer atomicMin of its index on its ground truth's entry
//                  of the winner table -- LDS for G <= MT_TABLE, else the frame's stretch of the workspace.
//     2. counts    TP = entries that have a winner, FP = K - TP, FN = G - TP.
//     3. sum       the matched distances add up in a double in ascending prediction index, as the reference's list
//                  does: per 256 predictions the winner table is inverted into LDS, the matched threads recompute
//                  their distance (the same function of the same operands) and thread 0 adds them in thread order --
//                  min(K, G) sequential additions at the most, none for the other predictions.
//
// Integer minima and a fixed addition order: the outputs are deterministic, and bev_detection_match_host (the literal
// greedy walk over the same per-pair functions) gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/bev_mi355x.h"
#include "bev_metrics.h"

namespace {

namespace mt = bev_metrics;

constexpr int MT_T = 256;                // threads per workgroup (4 waves)
constexpr int MT_CHUNK = 1024;           // ground truths per LDS chunk
constexpr int MT_TABLE = 1024;           // winner-table entries in LDS; a longer frame's table is in the workspace
constexpr int MT_NONE = 0x7fffffff;      // no winner

// the winner table of one frame: LDS, or -- one workgroup's private stretch of global memory -- device-scope atomics
// throughout, so that no access is served from a stale L1 line
struct Winners {
    int *lds, *glb;  // glb != nullptr: the workspace
    __device__ __forceinline__ void clear(int j) const {
        if (glb) __hip_atomic_store(glb + j, MT_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else lds[j] = MT_NONE;
    }
    __device__ __forceinline__ void offer(int j, int i) const { atomicMin(glb ? glb + j : lds + j, i); }
    __device__ __forceinline__ int get(int j) const {
        return glb ? __hip_atomic_load(glb + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : lds[j];
    }
    __device__ __forceinline__ void publish() const {  // called by every thread between two phases
        if (glb) __threadfence();
        __syncthreads();
    }
};

__global__ __launch_bounds__(MT_T) void k_det_match(const float *__restrict__ pred,
                                                    const int32_t *__restrict__ pred_count, int cap,
                                                    const float *__restrict__ gt_xy,
                                                    const int32_t *__restrict__ gt_offset, int N, float thr32,
                                                    int32_t *__restrict__ counts, double *__restrict__ dist_sum,
                                                    int *__restrict__ ws) {
    __shared__ float2 gts[MT_CHUNK];
    __shared__ int table[MT_TABLE];
    __shared__ int slot[MT_T];
    __shared__ float dl[MT_T];
    __shared__ unsigned long long wmask[MT_T / 64];
    __shared__ int tp_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    int K = pred_count[b];
    const int g0 = gt_offset[b], g1 = gt_offset[b + 1];
    int32_t *out = counts + 4 * (int64_t)b;
    // everything below is workgroup-uniform until the threads take their predictions
    const int status = K < 0 ? mt::STATUS_PENDING : (g0 < 0 || g1 < g0 || g1 > N) ? mt::STATUS_OFFSETS : mt::STATUS_OK;
    if (status != mt::STATUS_OK) {
        if (tid == 0) {
            out[mt::TP] = out[mt::FP] = out[mt::FN] = 0;
            out[mt::STATUS] = status;
            dist_sum[b] = 0.0;
        }
        return;
    }
    K = K < cap ? K : cap;  // the decode never writes more rows than the frame has
    const int G = g1 - g0;
    if (K == 0 || G == 0) {  // nothing to match: every prediction is a false positive, every ground truth a miss
        if (tid == 0) {
            out[mt::TP] = 0;
            out[mt::FP] = K;
            out[mt::FN] = G;
            out[mt::STATUS] = mt::STATUS_OK;
            dist_sum[b] = 0.0;
        }
        return;
    }
    const float *P = pred + 4 * (int64_t)b * cap;
    const float *Gt = gt_xy + 2 * (int64_t)g0;
    const Winners win = {table, G > MT_TABLE ? ws + g0 : nullptr};
    for (int j = tid; j < G; j += MT_T) win.clear(j);
    if (tid == 0) tp_s = 0;
    win.publish();

    // 1. nearest ground truth per prediction, lowest prediction index per ground truth
    int staged = -1;
    for (int i0 = 0; i0 < K; i0 += MT_T) {
        const int i = i0 + tid;
        const bool active = i < K;
        const float px = active ? P[4 * (int64_t)i] : 0.0f, py = active ? P[4 * (int64_t)i + 1] : 0.0f;
        mt::Nearest n = mt::nearest_init();
        for (int c0 = 0; c0 < G; c0 += MT_CHUNK) {
            const int cn = G - c0 < MT_CHUNK ? G - c0 : MT_CHUNK;
            if (c0 != staged) {
                __syncthreads();  // the previous chunk has been read
                for (int j = tid; j < cn; j += MT_T)
                    gts[j] = make_float2(Gt[2 * (int64_t)(c0 + j)], Gt[2 * (int64_t)(c0 + j) + 1]);
                __syncthreads();
                staged = c0;
            }
            if (active)
                for (int j = 0; j < cn; ++j) {
                    const float2 g = gts[j];
                    mt::nearest_visit(n, mt::pair_dist(px, py, g.x, g.y), c0 + j);
                }
        }
        if (active && mt::within(n.d, thr32)) win.offer(n.j, i);
    }
    win.publish();

    // 2. the counts
    int mine = 0;
    for (int j = tid; j < G; j += MT_T) mine += win.get(j) != MT_NONE;
    if (mine) atomicAdd(&tp_s, mine);
    __syncthreads();
    const int tp = tp_s;

    // 3. the matched distances, added in ascending prediction index (thread 0 holds the sum)
    double sum = 0.0;
    if (tp > 0)
        for (int i0 = 0; i0 < K; i0 += MT_T) {
            slot[tid] = -1;
            __syncthreads();
            for (int j = tid; j < G; j += MT_T) {  // a prediction has one nearest: no two j name the same slot
                const int w = win.get(j);
                if (w >= i0 && w - i0 < MT_T) slot[w - i0] = j;
            }
            __syncthreads();
            const int j = slot[tid];
            if (j >= 0) {
                const int64_t i = i0 + tid;
                dl[tid] = mt::pair_dist(P[4 * i], P[4 * i + 1], Gt[2 * (int64_t)j], Gt[2 * (int64_t)j + 1]);
            }
            const unsigned long long m = __ballot(j >= 0);
            if ((tid & 63) == 0) wmask[tid >> 6] = m;
            __syncthreads();
            if (tid == 0)
                for (int w = 0; w < MT_T / 64; ++w)
                    for (unsigned long long left = wmask[w]; left; left &= left - 1)
                        sum += (double)dl[64 * w + __ffsll((long long)left) - 1];
            // the next round writes dl / wmask only after its own barriers, which thread 0 reaches after this loop
        }
    if (tid == 0) {
        out[mt::TP] = tp;
        out[mt::FP] = K - tp;
        out[mt::FN] = G - tp;
        out[mt::STATUS] = mt::STATUS_OK;
        dist_sum[b] = sum;
    }
}

// k_det_assign    the optimal matching (MODA / MODP): one wave per frame runs bev_metrics::assign_solve, the very
// procedure of the host entry, with its 64 lanes as the workers -- each owns the ground truths lane, lane + 64, ...,
// the one reduction per search step is a lexicographic (k, s, index) minimum over the wave by lane exchanges, and the
// barriers are those of a one-wave workgroup.  Coordinates, duals, tentative distances and the matching of a frame of
// up to ASSIGN_DEVICE_MAX x ASSIGN_DEVICE_MAX sit in 59 KiB of LDS; there is no cost matrix and no workspace.
constexpr int AS_T = 64;
constexpr int AS_MAX = mt::ASSIGN_DEVICE_MAX;

struct WaveExec {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return AS_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ mt::Best reduce(mt::Best b) const {
        for (int off = AS_T / 2; off; off >>= 1) {
            mt::Best o;
            o.v.k = __shfl_xor(b.v.k, off, AS_T);
            o.v.s = __shfl_xor(b.v.s, off, AS_T);
            o.j = __shfl_xor(b.j, off, AS_T);
            if (mt::best_before(o, b)) b = o;
        }
        return b;  // a total order: every lane holds the same element
    }
};

__global__ __launch_bounds__(AS_T) void k_det_assign(const float *__restrict__ pred,
                                                     const int32_t *__restrict__ pred_count, int cap,
                                                     const float *__restrict__ gt_xy,
                                                     const int32_t *__restrict__ gt_offset, int N, float thr32,
                                                     int32_t *__restrict__ counts, double *__restrict__ dist_sum) {
    __shared__ double us[AS_MAX], vs[AS_MAX], sps[AS_MAX];
    __shared__ float px[AS_MAX], py[AS_MAX], gx[AS_MAX], gy[AS_MAX];
    __shared__ int32_t uk[AS_MAX], vk[AS_MAX], spk[AS_MAX];
    __shared__ int16_t path[AS_MAX], colrow[AS_MAX], rowcol[AS_MAX];
    __shared__ uint8_t sc[AS_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    int K = pred_count[b];
    const int g0 = gt_offset[b], g1 = gt_offset[b + 1];
    int32_t *out = counts + 4 * (int64_t)b;
    // wave-uniform from here on
    int status = K < 0 ? mt::STATUS_PENDING : (g0 < 0 || g1 < g0 || g1 > N) ? mt::STATUS_OFFSETS : mt::STATUS_OK;
    K = K < cap ? K : cap;
    const int G = g1 - g0;
    if (status == mt::STATUS_OK && (K > AS_MAX || G > AS_MAX)) status = mt::STATUS_TOO_LARGE;
    if (status != mt::STATUS_OK || K == 0 || G == 0) {
        if (tid == 0) {
            out[mt::TP] = 0;
            out[mt::FP] = status == mt::STATUS_OK ? K : 0;
            out[mt::FN] = status == mt::STATUS_OK ? G : 0;
            out[mt::STATUS] = status;
            dist_sum[b] = 0.0;
        }
        return;
    }
    const float *P = pred + 4 * (int64_t)b * cap;
    const float *Gt = gt_xy + 2 * (int64_t)g0;
    for (int i = tid; i < K; i += AS_T) {
        px[i] = P[4 * (int64_t)i];
        py[i] = P[4 * (int64_t)i + 1];
    }
    for (int j = tid; j < G; j += AS_T) {
        gx[j] = Gt[2 * (int64_t)j];
        gy[j] = Gt[2 * (int64_t)j + 1];
    }
    const mt::AssignState<int16_t> S = {px, py, gx, gy, uk, vk, spk, us, vs, sps, path, colrow, rowcol, sc};
    int32_t tp = 0;
    double sum = 0.0;
    mt::assign_solve(WaveExec(), S, K, G, thr32, &tp, &sum);  // its first barrier publishes the coordinates
    if (tid == 0) {
        out[mt::TP] = tp;
        out[mt::FP] = K - tp;
        out[mt::FN] = G - tp;
        out[mt::STATUS] = mt::STATUS_OK;
        dist_sum[b] = sum;
    }
}

// the checks the entries share; 0 when the arguments are usable
int check_args(const void *pred, const void *pred_count, int B, int cap, const void *gt_xy, const void *gt_offset,
               int N, const void *counts, const void *dist_sum) {
    if (B < 0 || cap < 0 || N < 0) return BEV_ERR_ARGS;
    if (B == 0) return 0;
    if (!pred_count || !gt_offset || !counts || !dist_sum) return BEV_ERR_ARGS;
    if (cap > 0 && !pred) return BEV_ERR_ARGS;
    if (N > 0 && !gt_xy) return BEV_ERR_ARGS;
    return 0;
}

}  // namespace

extern "C" {

int64_t bev_detection_match_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= MT_TABLE) return 0;  // no frame can outgrow the LDS table
    return (int64_t)N * (int64_t)sizeof(int);
}

int bev_detection_match_f32(const float *pred, const int32_t *pred_count, int B, int cap, const float *gt_xy,
                            const int32_t *gt_offset, int N, float thr32, int32_t *counts, double *dist_sum,
                            void *workspace, int64_t workspace_bytes, void *stream) {
    const int rc = check_args(pred, pred_count, B, cap, gt_xy, gt_offset, N, counts, dist_sum);
    if (rc) return rc;
    if (B == 0) return 0;
    const int64_t need = bev_detection_match_workspace_bytes(B, N);
    if (need > 0 && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need)) return BEV_ERR_ARGS;
    hipLaunchKernelGGL(k_det_match, dim3(B), dim3(MT_T), 0, (hipStream_t)stream, pred, pred_count, cap, gt_xy,
                       gt_offset, N, thr32, counts, dist_sum, need > 0 ? (int *)workspace : nullptr);
    return (int)hipGetLastError();
}

int bev_detection_match_host(const float *pred, const int32_t *pred_count, int B, int cap, const float *gt_xy,
                             const int32_t *gt_offset, int N, float thr32, int32_t *counts, double *dist_sum) {
    const int rc = check_args(pred, pred_count, B, cap, gt_xy, gt_offset, N, counts, dist_sum);
    if (rc) return rc;
    if (B == 0) return 0;
    if (gt_offset[0] < 0 || gt_offset[B] > N) return BEV_ERR_ARGS;
    for (int b = 0; b < B; ++b)
        if (gt_offset[b + 1] < gt_offset[b]) return BEV_ERR_ARGS;
    std::vector<char> used;
    for (int b = 0; b < B; ++b) {
        int32_t *out = counts + 4 * (int64_t)b;
        out[mt::TP] = out[mt::FP] = out[mt::FN] = 0;
        out[mt::STATUS] = mt::STATUS_OK;
        dist_sum[b] = 0.0;
        if (pred_count[b] < 0) {
            out[mt::STATUS] = mt::STATUS_PENDING;
            continue;
        }
        const int K = pred_count[b] < cap ? pred_count[b] : cap, G = gt_offset[b + 1] - gt_offset[b];
        const float *P = pred + 4 * (int64_t)b * cap;
        const float *Gt = gt_xy + 2 * (int64_t)gt_offset[b];
        used.assign((size_t)G, 0);
        int tp = 0;
        double sum = 0.0;
        for (int i = 0; i < K && G > 0; ++i) {  // the reference's walk, prediction by prediction
            mt::Nearest n = mt::nearest_init();
            for (int j = 0; j < G; ++j)
                mt::nearest_visit(n, mt::pair_dist(P[4 * (int64_t)i], P[4 * (int64_t)i + 1], Gt[2 * (int64_t)j],
                                                   Gt[2 * (int64_t)j + 1]), j);
            if (mt::within(n.d, thr32) && !used[n.j]) {
                used[n.j] = 1;
                ++tp;
                sum += (double)n.d;
            }
        }
        out[mt::TP] = tp;
        out[mt::FP] = K - tp;
        out[mt::FN] = G - tp;
        dist_sum[b] = sum;
    }
    return 0;
}

int64_t bev_detection_assign_workspace_bytes(int B, int cap, int N) {
    (void)B, (void)cap, (void)N;
    return 0;  // a frame the kernel takes fits its LDS; a larger one is left to the host entry (STATUS_TOO_LARGE)
}

int bev_detection_assign_max_frame(void) { return AS_MAX; }

int bev_detection_assign_f32(const float *pred, const int32_t *pred_count, int B, int cap, const float *gt_xy,
                             const int32_t *gt_offset, int N, float thr32, int32_t *counts, double *dist_sum,
                             void *workspace, int64_t workspace_bytes, void *stream) {
    const int rc = check_args(pred, pred_count, B, cap, gt_xy, gt_offset, N, counts, dist_sum);
    if (rc) return rc;
    if (workspace_bytes < 0) return BEV_ERR_ARGS;
    (void)workspace;
    if (B == 0) return 0;
    hipLaunchKernelGGL(k_det_assign, dim3(B), dim3(AS_T), 0, (hipStream_t)stream, pred, pred_count, cap, gt_xy,
                       gt_offset, N, thr32, counts, dist_sum);
    return (int)hipGetLastError();
}

int bev_detection_assign_host(const float *pred, const int32_t *pred_count, int B, int cap, const float *gt_xy,
                              const int32_t *gt_offset, int N, float thr32, int32_t *counts, double *dist_sum) {
    const int rc = check_args(pred, pred_count, B, cap, gt_xy, gt_offset, N, counts, dist_sum);
    if (rc) return rc;
    if (B == 0) return 0;
    if (gt_offset[0] < 0 || gt_offset[B] > N) return BEV_ERR_ARGS;
    for (int b = 0; b < B; ++b)
        if (gt_offset[b + 1] < gt_offset[b]) return BEV_ERR_ARGS;
    std::vector<float> px, py, gx, gy;
    std::vector<int32_t> uk, vk, spk, path, colrow, rowcol;
    std::vector<double> us, vs, sps;
    std::vector<uint8_t> sc;
    for (int b = 0; b < B; ++b) {
        int32_t *out = counts + 4 * (int64_t)b;
        out[mt::TP] = out[mt::FP] = out[mt::FN] = 0;
        out[mt::STATUS] = mt::STATUS_OK;
        dist_sum[b] = 0.0;
        if (pred_count[b] < 0) {
            out[mt::STATUS] = mt::STATUS_PENDING;
            continue;
        }
        const int K = pred_count[b] < cap ? pred_count[b] : cap, G = gt_offset[b + 1] - gt_offset[b];
        int32_t tp = 0;
        double sum = 0.0;
        if (K > 0 && G > 0) {
            const float *P = pred + 4 * (int64_t)b * cap;
            const float *Gt = gt_xy + 2 * (int64_t)gt_offset[b];
            const size_t k = (size_t)K, g = (size_t)G;
            px.resize(k), py.resize(k), uk.resize(k), us.resize(k), rowcol.resize(k);
            gx.resize(g), gy.resize(g), vk.resize(g), vs.resize(g), spk.resize(g), path.resize(g), colrow.resize(g);
            sc.resize(g), sps.resize(k > g ? k : g);
            for (int i = 0; i < K; ++i) px[i] = P[4 * (int64_t)i], py[i] = P[4 * (int64_t)i + 1];
            for (int j = 0; j < G; ++j) gx[j] = Gt[2 * (int64_t)j], gy[j] = Gt[2 * (int64_t)j + 1];
            const mt::AssignState<int32_t> S = {px.data(), py.data(), gx.data(),   gy.data(),     uk.data(),
                                                vk.data(), spk.data(), us.data(),  vs.data(),     sps.data(),
                                                path.data(), colrow.data(), rowcol.data(), sc.data()};
            mt::assign_solve(mt::SerialExec(), S, K, G, thr32, &tp, &sum);
        }
        out[mt::TP] = tp;
        out[mt::FP] = K - tp;
        out[mt::FN] = G - tp;
        dist_sum[b] = sum;
    }
    return 0;
}

}  // extern "C"
