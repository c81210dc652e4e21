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

// ---------------------------------------------------------------------------------------------------------------------
// Optimal one-to-one matching of a frame (MODA / MODP scoring; bev_detection_assign_f32 / _host).
//
// A pair (i, j) is admissible when its pair_dist is within thr32 (and finite: an infinite distance under an infinite
// threshold has no place in a sum).  The matching has the most admissible pairs possible and, among those, the
// smallest sum of the distances taken as doubles.  It is found as a linear assignment in which every prediction also
// has a private dummy partner, over costs that are pairs (k, s) ordered lexicographically and added componentwise: a
// real pair costs (0, d), a dummy (1, 0).  Minimising that cost minimises the number of dummies first -- so the
// cardinality is maximal by construction, with no penalty constant that a floating-point addition could absorb: k is
// an integer -- and the distance sum second.
//
// The solver is the shortest-augmenting-path method (Jonker-Volgenant; the row-by-row form of Crouse's rectangular
// variant): predictions enter in ascending index, each by one Dijkstra search over reduced costs from the entering row
// to the nearest free column (real or dummy), then the duals of the scanned rows and columns move and the path is
// flipped.  There is no cost matrix: a row's scan recomputes pair_dist from the coordinates.  The one reduction, "the
// unscanned column of least tentative distance", is lexicographic in (k, s, column index) -- a total order, so `lanes`
// workers that each own the columns lane, lane + lanes, ... and merge their bests pick the column a sequential scan
// picks, and get its value, not an equal one.  A real column precedes a dummy of the same distance; of two dummies the
// one whose row was scanned first.  assign_solve below is that whole procedure, written once over an executor: the
// kernel runs it with the 64 lanes of a wave, the host entry with one -- the same statements on the same operands, so
// the outputs agree bit for bit, tied inputs included.
//
// What rounds: the costs are exact doubles; the tentative distances and the dual updates are double additions.  A
// rounding there can only make the search prefer a matching whose sum is within the accumulated error of the optimum;
// it cannot change the cardinality (the k components are integers) and cannot keep the search from ending (every
// step scans a new column or ends at a dummy).
// ---------------------------------------------------------------------------------------------------------------------
enum { STATUS_TOO_LARGE = -3 };  // device entry: the frame has more predictions or ground truths than ASSIGN_DEVICE_MAX
enum { ASSIGN_DEVICE_MAX = 1024 };
enum { ROW_FREE = -1, ROW_DUMMY = -2 };  // rowcol[i] when it is no column
enum { LEX_NONE = 0x7fffffff };          // k of "no tentative distance yet"

BEV_MET_FN bool admissible(float d, float thr32) { return within(d, thr32) && d <= 3.402823466e+38f; }

struct Lex {
    int32_t k;
    double s;
};

BEV_MET_FN bool lex_less(const Lex &a, const Lex &b) { return a.k < b.k || (a.k == b.k && a.s < b.s); }

// a tentative distance with its column (j < 0: none)
struct Best {
    Lex v;
    int j;
};

// does a come before b in (k, s, j)?
BEV_MET_FN bool best_before(const Best &a, const Best &b) {
    if (lex_less(a.v, b.v)) return true;
    if (lex_less(b.v, a.v)) return false;
    return (uint32_t)a.j < (uint32_t)b.j;
}

// The working arrays of one frame (LDS in the kernel, vectors on the host).  px, py, uk, us, rowcol: one entry per
// prediction; gx, gy, vk, vs, spk, path, colrow, sc: one per ground truth; sps: max(K, G) entries (it also carries the
// matched distances to the final sum).  Idx holds a row or column index and ROW_FREE / ROW_DUMMY.
template <typename Idx>
struct AssignState {
    float *px, *py, *gx, *gy;
    int32_t *uk, *vk, *spk;   // k components of the row duals, the column duals and the tentative distances
    double *us, *vs, *sps;    // their s components
    Idx *path, *colrow, *rowcol;
    uint8_t *sc;              // column scanned in the current search
};

// One worker: the sequential executor of the host entry (the kernel's is in bev_metrics.hip).
struct SerialExec {
    BEV_MET_FN int lane() const { return 0; }
    BEV_MET_FN int lanes() const { return 1; }
    BEV_MET_FN void sync() const {}
    BEV_MET_FN Best reduce(const Best &b) const { return b; }
};

// Solves one frame (K >= 0 predictions, G >= 0 ground truths, coordinates already in S) and leaves tp and the matched
// distances' sum (added in ascending prediction index) in *tp_out / *sum_out of worker 0.  Every worker of the
// executor calls it with the same arguments; ex.sync() orders their accesses to S.
template <typename Idx, typename Exec>
BEV_MET_FN void assign_solve(const Exec &ex, const AssignState<Idx> &S, int K, int G, float thr32, int32_t *tp_out,
                             double *sum_out) {
    const int lane = ex.lane(), L = ex.lanes();
    for (int j = lane; j < G; j += L) {
        S.vk[j] = 0;
        S.vs[j] = 0.0;
        S.colrow[j] = (Idx)ROW_FREE;
    }
    for (int i = lane; i < K; i += L) {
        S.uk[i] = 0;
        S.us[i] = 0.0;
        S.rowcol[i] = (Idx)ROW_FREE;
    }
    ex.sync();
    for (int cur = 0; cur < K; ++cur) {
        // a worker's columns are its own throughout the search: spk / sps / path / sc need no barrier until the flip
        for (int j = lane; j < G; j += L) {
            S.spk[j] = LEX_NONE;  // sps[j] is read only once spk[j] says it was written
            S.sc[j] = 0;
        }
        Lex minv = {0, 0.0};          // the distance of the row being scanned
        Lex dval = {LEX_NONE, 0.0};   // the nearest dummy so far, and whose it is
        int drow = -1, sink = -1, i = cur;
        for (;;) {
            const Lex ui = {S.uk[i], S.us[i]};
            const Lex cand = {minv.k + 1 - ui.k, minv.s - ui.s};  // row i's dummy: cost (1, 0), dual (0, 0)
            if (lex_less(cand, dval)) {
                dval = cand;
                drow = i;
            }
            const float px = S.px[i], py = S.py[i];
            Best best = {{LEX_NONE, 0.0}, -1};
            for (int j = lane; j < G; j += L) {
                if (S.sc[j]) continue;
                const float d = pair_dist(px, py, S.gx[j], S.gy[j]);
                Lex sp = {S.spk[j], 0.0};
                if (sp.k != LEX_NONE) sp.s = S.sps[j];
                if (admissible(d, thr32)) {
                    const Lex r = {minv.k - ui.k - S.vk[j], ((minv.s + (double)d) - ui.s) - S.vs[j]};
                    if (lex_less(r, sp)) {
                        sp = r;
                        S.spk[j] = r.k;
                        S.sps[j] = r.s;
                        S.path[j] = (Idx)i;
                    }
                }
                if (sp.k != LEX_NONE && lex_less(sp, best.v)) {
                    best.v = sp;
                    best.j = j;
                }
            }
            best = ex.reduce(best);
            if (best.j < 0 || lex_less(dval, best.v)) {  // a dummy is strictly nearer than every real column
                minv = dval;
                break;
            }
            minv = best.v;
            if (best.j % L == lane) S.sc[best.j] = 1;
            const int r = S.colrow[best.j];
            if (r < 0) {
                sink = best.j;
                break;
            }
            i = r;
        }
        // the duals of what the search scanned (a scanned column's row is scanned too; the real sink has no row)
        for (int j = lane; j < G; j += L) {
            if (!S.sc[j]) continue;
            const int r = S.colrow[j];
            if (r < 0) continue;
            const int32_t tk = minv.k - S.spk[j];
            const double ts = minv.s - S.sps[j];
            S.uk[r] += tk;
            S.us[r] = S.us[r] + ts;
            S.vk[j] -= tk;
            S.vs[j] = S.vs[j] - ts;
        }
        if (lane == 0) {
            S.uk[cur] += minv.k;
            S.us[cur] = S.us[cur] + minv.s;
        }
        ex.sync();
        if (lane == 0) {  // flip the path: back from the sink to the entering row, whose rowcol is ROW_FREE
            int j = sink;
            if (sink < 0) {
                j = S.rowcol[drow];
                S.rowcol[drow] = (Idx)ROW_DUMMY;
            }
            for (int n = 0; j >= 0 && n <= G; ++n) {
                const int r = S.path[j];
                S.colrow[j] = (Idx)r;
                const int next = S.rowcol[r];
                S.rowcol[r] = (Idx)j;
                j = next;
            }
        }
        ex.sync();
    }
    for (int i = lane; i < K; i += L) {
        const int c = S.rowcol[i];
        S.sps[i] = c >= 0 ? (double)pair_dist(S.px[i], S.py[i], S.gx[c], S.gy[c]) : 0.0;
    }
    ex.sync();
    if (lane == 0) {
        int32_t tp = 0;
        double sum = 0.0;
        for (int i = 0; i < K; ++i)
            if (S.rowcol[i] >= 0) {
                ++tp;
                sum += S.sps[i];
            }
        *tp_out = tp;
        *sum_out = sum;
    }
}

}  // namespace bev_metrics
