// bev_metrics.h -- the per-pair arithmetic of the validation scoring (train.py:78-104 of the reference,
// compute_metrics), for the kernel of bev_metrics.hip and the host entry bev_detection_match_host alike.
//
// One prediction p against the ground truths g_0 .. g_{G-1} of its frame (the sources that include this header are
// compiled with -ffp-contract=off: the two products and their sum round separately, on the host and on the device):
//   * d_j = sqrtf(dx * dx + dy * dy), dx = g_j.x - p.x, dy = g_j.y - p.y (gt minus prediction, as the reference
//     subtracts), the square root correctly rounded;
//   * the nearest is torch.min(dists, dim=0): the smallest distance at its first index, and a NaN wins over every
//     number -- the first NaN, at its index;
//   * the match test is d <= thr32, thr32 the largest float32 <= the caller's double threshold: the reference compares
//     the float32 distance, widened, with the double.  A NaN distance fails it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BEV_MET_FN __host__ __device__ __forceinline__
#else
#define BEV_MET_FN static inline
#endif

namespace bev_metrics {

// counts[b][4]
enum { TP = 0, FP = 1, FN = 2, STATUS = 3 };
// status: the frame is complete; its prediction count is the decode's "finished by the large path" mark (< 0); its
// ground-truth offsets decrease or leave [0, N] (device entry: the host entry refuses those before it starts)
enum { STATUS_OK = 0, STATUS_PENDING = -1, STATUS_OFFSETS = -2 };

BEV_MET_FN float pair_dist(float px, float py, float gx, float gy) {
    const float dx = gx - px, dy = gy - py;
    return sqrtf(dx * dx + dy * dy);
}

// the running (best, j) of one prediction over ground truths visited in ascending index
struct Nearest {
    float d;
    int j;  // -1: nothing visited yet
};

BEV_MET_FN Nearest nearest_init() {
    Nearest n = {0.0f, -1};
    return n;
}

// does d at a later index replace best?  Never once best is NaN; a NaN or a strictly smaller distance does
BEV_MET_FN bool takes_over(float best, float d) { return best == best && (d != d || d < best); }

BEV_MET_FN void nearest_visit(Nearest &n, float d, int j) {
    if (n.j < 0 || takes_over(n.d, d)) {
        n.d = d;
        n.j = j;
    }
}

BEV_MET_FN bool within(float d, float thr32) { return d <= thr32; }  // false for a NaN on either side

}  // namespace bev_metrics
