// bev_track.h -- the online tracker on the BEV detections (the reference's README, phase 3: a light SORT-style
// tracker that gives every pedestrian a stable id over time; the reference has no code for it), for the kernel of
// bev_track.hip and the host entry bev_track_step_host alike.  The sources that include this header are compiled with
// -ffp-contract=off, and every statement below is the same on both sides: the outputs and the state agree bit for bit.
//
// A track is a ground-plane point under a constant-velocity model with isotropic noise: x, y, vx, vy (metres, metres
// per frame) and one 2 x 2 covariance p00, p01, p11 that the two axes share -- with equal noise on both axes the x and
// the y filter are two copies of one 2-state filter, with the same covariance and the same scalar gains.  All filter
// arithmetic is in double.  Beside it: id (>= 0), streak (consecutive frames with a match), misses (frames since the
// last match), age (frames since birth).
//
// One frame (frame_step), in this order:
//   1. predict   every live track in slot order:  x += vx, y += vy;  p00 = ((p00 + p01) + (p01 + p11)) + q_pos on the
//                old values, p01 = p01 + p11, p11 = p11 + q_vel;  misses += 1, age += 1.
//   2. associate rows = the live tracks in slot order at ((float)x, (float)y), columns = the frame's detections in
//                decode order; bev_metrics::assign_solve, unchanged, with the gate as its threshold: the most pairs
//                within the gate, among those the smallest distance sum, ties by its lowest-index rule.  A non-finite
//                position on either side is inadmissible by its rule.
//   3. update    a matched track with its detection z (as doubles):  s = p00 + r, k0 = p00 / s, k1 = p01 / s;  per
//                axis e = z - x, x += k0 e, v += k1 e;  then from the old values p11 = p11 - k1 p01,
//                p01 = p01 - k0 p01, p00 = p00 - k0 p00;  streak += 1, misses = 0.  An unmatched track: streak = 0.
//   4. delete    tracks with misses > max_age; the table is compacted stably (the survivors keep their order) and
//                the slots behind them are zeroed.
//   5. birth     every unmatched detection with finite x and y, in ascending detection index, appends a track at z
//                with v = 0, p00 = r, p01 = 0, p11 = p0_vel, streak 1, misses 0, age 1, id = next_id++.  When the
//                table is full the detection founds nothing (and takes no id); the frame's DROPPED count rises.
//   6. report    detection c gets the id of the track it updated or founded when that track has streak >= min_hits or
//                the sequence has seen at most min_hits frames (SORT's warm-up rule), else -1; with the id the
//                track's (x, y, vx, vy) after the update as float32, zeros with -1.
//
// The procedure is written once over an executor (bev_metrics.h): the kernel runs it with the 64 lanes of a wave, the
// host entry with one worker.  Beside the solver's lane / lanes / sync / reduce an executor here has
//     int prefix(bool flag, int *total)   the number of lower lanes whose flag is set, and of all lanes
// which is what the stable compaction and the births in detection order need; nothing else crosses lanes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/bev_mi355x.h"
#include "bev_metrics.h"

namespace bev_track {

namespace mt = bev_metrics;

enum { TRACK_MAX = mt::ASSIGN_DEVICE_MAX };  // tracks of a table, and tracked detections of a frame
enum { MAX_FRAMES = 65536 };                 // frames of one launch

// info[f][4]
enum { STATUS = 0, LIVE = 1, BORN = 2, DROPPED = 3 };
// status bits.  TRUNCATED: the frame has more than TRACK_MAX detections, the first TRACK_MAX were tracked.  PENDING:
// the frame's detection count is the decode's "finished by the large path" mark (< 0); STALLED: an earlier frame of
// the sequence is pending -- neither frame was tracked.  BAD_STATE: the state blob is not one bev_track_reset made
// for this max_tracks (nothing was read beyond its header, nothing written).
enum { ST_OK = 0, ST_TRUNCATED = 1, ST_PENDING = 2, ST_STALLED = 4, ST_BAD_STATE = 8 };

// The state blob of one sequence: HDR_WORDS int32, then seven arrays of max_tracks doubles (x, y, vx, vy, p00, p01,
// p11), then four of max_tracks int32 (id, streak, misses, age), rounded up to 16 bytes.  Slots at and behind `count`,
// the unused header words and the tail padding are zero, always: two runs that agree agree in every byte.
enum { H_MAGIC = 0, H_MAX = 1, H_COUNT = 2, H_NEXT_ID = 3, H_FRAMES = 4, H_STALLED = 5, HDR_WORDS = 8 };
enum { MAGIC = 0x4b525442 };  // "BTRK"
enum { N_DOUBLES = 7, N_INTS = 4 };

BEV_MET_FN int64_t state_bytes(int max_tracks) {
    return ((int64_t)HDR_WORDS * 4 + (int64_t)max_tracks * (N_DOUBLES * 8 + N_INTS * 4) + 15) & ~(int64_t)15;
}

BEV_MET_FN bool params_ok(const bev_track_params &P) {
    const double big = 1.7976931348623157e308;
    if (!(P.thr32 >= 0.0f)) return false;  // a NaN gate too
    if (!(P.q_pos >= 0.0 && P.q_pos <= big && P.q_vel >= 0.0 && P.q_vel <= big && P.p0_vel >= 0.0 && P.p0_vel <= big))
        return false;
    if (!(P.r > 0.0 && P.r <= big)) return false;
    return P.max_tracks >= 1 && P.max_tracks <= TRACK_MAX && P.max_age >= 0 && P.min_hits >= 1;
}

// the track table: LDS arrays in the kernel, the blob's own arrays on the host
struct Table {
    double *x, *y, *vx, *vy, *p00, *p01, *p11;
    int32_t *id, *streak, *misses, *age;
};

// a blob's arrays (base: 8-byte aligned)
BEV_MET_FN Table table_of(void *blob, int max_tracks) {
    double *d = (double *)((char *)blob + HDR_WORDS * 4);
    int32_t *n = (int32_t *)(d + (int64_t)N_DOUBLES * max_tracks);
    const int64_t m = max_tracks;
    Table T = {d, d + m, d + 2 * m, d + 3 * m, d + 4 * m, d + 5 * m, d + 6 * m, n, n + m, n + 2 * m, n + 3 * m};
    return T;
}

struct Track {
    double x, y, vx, vy, p00, p01, p11;
    int32_t id, streak, misses, age;
};

BEV_MET_FN Track get(const Table &T, int i) {
    Track t = {T.x[i], T.y[i], T.vx[i], T.vy[i], T.p00[i], T.p01[i], T.p11[i], T.id[i], T.streak[i], T.misses[i], T.age[i]};
    return t;
}

BEV_MET_FN void put(const Table &T, int i, const Track &t) {
    T.x[i] = t.x, T.y[i] = t.y, T.vx[i] = t.vx, T.vy[i] = t.vy;
    T.p00[i] = t.p00, T.p01[i] = t.p01, T.p11[i] = t.p11;
    T.id[i] = t.id, T.streak[i] = t.streak, T.misses[i] = t.misses, T.age[i] = t.age;
}

BEV_MET_FN Track no_track() {
    Track t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0};
    return t;
}

BEV_MET_FN int32_t count_up(int32_t v) { return v < 0x7fffffff ? v + 1 : v; }  // a counter saturates, it never wraps

BEV_MET_FN Track predict(Track t, const bev_track_params &P) {
    t.x += t.vx;
    t.y += t.vy;
    const double p00 = ((t.p00 + t.p01) + (t.p01 + t.p11)) + P.q_pos;
    t.p01 = t.p01 + t.p11;
    t.p11 = t.p11 + P.q_vel;
    t.p00 = p00;
    t.misses = count_up(t.misses);
    t.age = count_up(t.age);
    return t;
}

BEV_MET_FN Track update(Track t, double zx, double zy, const bev_track_params &P) {
    const double s = t.p00 + P.r, k0 = t.p00 / s, k1 = t.p01 / s;
    const double ex = zx - t.x, ey = zy - t.y;
    t.x += k0 * ex;
    t.vx += k1 * ex;
    t.y += k0 * ey;
    t.vy += k1 * ey;
    t.p11 = t.p11 - k1 * t.p01;
    t.p01 = t.p01 - k0 * t.p01;
    t.p00 = t.p00 - k0 * t.p00;
    t.streak = count_up(t.streak);
    t.misses = 0;
    return t;
}

BEV_MET_FN Track found(double zx, double zy, int32_t id, const bev_track_params &P) {
    Track t = {zx, zy, 0.0, 0.0, P.r, 0.0, P.p0_vel, id, 1, 0, 1};
    return t;
}

BEV_MET_FN bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for a NaN

BEV_MET_FN int32_t id_after(int32_t next_id, int n) { return (int32_t)(((uint32_t)next_id + (uint32_t)n) & 0x7fffffffu); }

// One worker (the host entry).
struct SerialExec : mt::SerialExec {
    BEV_MET_FN int prefix(bool flag, int *total) const {
        *total = flag;
        return 0;
    }
};

// the header words a sequence's walk reads and writes: every worker holds the same copy
struct Seq {
    int32_t count, next_id, frames_seen, stalled;
};

// ids / out rows from `from` to TRACK_MAX: no detection, no track
template <typename Exec>
BEV_MET_FN void blank(const Exec &ex, int32_t *ids, float *out, int from) {
    for (int j = from + ex.lane(); j < TRACK_MAX; j += ex.lanes()) {
        ids[j] = -1;
        out[4 * j] = out[4 * j + 1] = out[4 * j + 2] = out[4 * j + 3] = 0.0f;
    }
}

// One frame of one sequence.  det: the frame's [D][4] rows (x, y read), D <= TRACK_MAX; M: the table's slots.  Every
// worker calls it with the same arguments; S's arrays hold TRACK_MAX entries each.
template <typename Idx, typename Exec>
BEV_MET_FN void frame_step(const Exec &ex, const Table &T, const mt::AssignState<Idx> &S, Seq &q, int M,
                           const bev_track_params &P, const float *det, int D, int status, int32_t *ids, float *out,
                           int32_t *info) {
    const int lane = ex.lane(), L = ex.lanes();
    q.frames_seen = count_up(q.frames_seen);
    // 1. predict, and the solver's coordinates
    for (int i = lane; i < q.count; i += L) {
        const Track t = predict(get(T, i), P);
        put(T, i, t);
        S.px[i] = (float)t.x;
        S.py[i] = (float)t.y;
    }
    for (int j = lane; j < D; j += L) {
        S.gx[j] = det[4 * (int64_t)j];
        S.gy[j] = det[4 * (int64_t)j + 1];
    }
    // 2. associate (its first barrier publishes the coordinates)
    int32_t pairs = 0;
    double sum = 0.0;
    mt::assign_solve(ex, S, q.count, D, P.thr32, &pairs, &sum);
    ex.sync();  // worker 0 is through with the solver's arrays
    // 3. update: a worker's tracks are its own
    for (int i = lane; i < q.count; i += L) {
        const int c = S.rowcol[i];
        if (c >= 0) put(T, i, update(get(T, i), (double)S.gx[c], (double)S.gy[c], P));
        else T.streak[i] = 0;
    }
    ex.sync();
    // 4. delete and compact, L slots at a time in ascending order: a survivor moves to a slot at or below its own,
    // and every slot of a group is read before any is written.  uk[i]: where track i went (-1: deleted)
    int live = 0;
    for (int base = 0; base < q.count; base += L) {
        const int i = base + lane;
        const bool keep = i < q.count && T.misses[i] <= P.max_age;
        Track t = no_track();
        if (keep) t = get(T, i);
        int total = 0;
        const int rank = ex.prefix(keep, &total);
        ex.sync();
        if (i < q.count) S.uk[i] = keep ? live + rank : -1;
        if (keep) put(T, live + rank, t);
        live += total;
    }
    ex.sync();
    for (int i = live + lane; i < q.count; i += L) put(T, i, no_track());
    // vk[j]: the slot of the track detection j updated (a matched track has misses 0: it survives), -1: none
    for (int j = lane; j < D; j += L) {
        const int r = S.colrow[j];
        S.vk[j] = r >= 0 ? S.uk[r] : -1;
    }
    ex.sync();  // the freed slots are zero before a birth writes one
    // 5. birth, L detections at a time in ascending order (detection j is worker j % L's, above and below)
    int wants = 0;
    for (int base = 0; base < D; base += L) {
        const int j = base + lane;
        const bool cand = j < D && S.vk[j] < 0 && finite32(S.gx[j]) && finite32(S.gy[j]);
        int total = 0;
        const int k = wants + ex.prefix(cand, &total);
        if (cand && k < M - live) {
            put(T, live + k, found((double)S.gx[j], (double)S.gy[j], id_after(q.next_id, k), P));
            S.vk[j] = live + k;
        }
        wants += total;
    }
    const int born = wants < M - live ? wants : M - live;
    q.count = live + born;
    q.next_id = id_after(q.next_id, born);
    ex.sync();  // the updated, moved and founded tracks are visible
    // 6. report
    for (int j = lane; j < D; j += L) {
        const int slot = S.vk[j];
        const bool shown = slot >= 0 && (T.streak[slot] >= P.min_hits || q.frames_seen <= P.min_hits);
        ids[j] = shown ? T.id[slot] : -1;
        out[4 * j] = shown ? (float)T.x[slot] : 0.0f;
        out[4 * j + 1] = shown ? (float)T.y[slot] : 0.0f;
        out[4 * j + 2] = shown ? (float)T.vx[slot] : 0.0f;
        out[4 * j + 3] = shown ? (float)T.vy[slot] : 0.0f;
    }
    blank(ex, ids, out, D);
    if (lane == 0) {
        info[STATUS] = status;
        info[LIVE] = q.count;
        info[BORN] = born;
        info[DROPPED] = wants - born;
    }
    ex.sync();  // the next frame's predict writes what this report read
}

// The frames first .. B - 1 of one sequence, in time order.  pred [B][cap][4], pred_count [B], ids [B][TRACK_MAX],
// out [B][TRACK_MAX][4], info [B][4] are the sequence's own rows.  A frame whose count is negative cannot be skipped
// (the tracker is sequential): it is marked PENDING, every later frame STALLED, q.stalled is set and the table is
// left as the frame before it left it.
template <typename Idx, typename Exec>
BEV_MET_FN void walk(const Exec &ex, const Table &T, const mt::AssignState<Idx> &S, Seq &q, int M,
                     const bev_track_params &P, const float *pred, const int32_t *pred_count, int B, int cap, int first,
                     int32_t *ids, float *out, int32_t *info) {
    for (int b = first; b < B; ++b) {
        int32_t *ids_b = ids + (int64_t)b * TRACK_MAX, *info_b = info + 4 * (int64_t)b;
        float *out_b = out + 4 * (int64_t)b * TRACK_MAX;
        const int K = pred_count[b];
        if (q.stalled || K < 0) {
            blank(ex, ids_b, out_b, 0);
            if (ex.lane() == 0) {
                info_b[STATUS] = q.stalled ? ST_STALLED : ST_PENDING;
                info_b[LIVE] = info_b[BORN] = info_b[DROPPED] = 0;
            }
            q.stalled = 1;
            continue;
        }
        const int n = K < cap ? K : cap, D = n < TRACK_MAX ? n : TRACK_MAX;
        frame_step(ex, T, S, q, M, P, pred + 4 * (int64_t)b * cap, D, n > TRACK_MAX ? ST_TRUNCATED : ST_OK, ids_b,
                   out_b, info_b);
    }
}

// a frame of a launch that found a blob it cannot use
template <typename Exec>
BEV_MET_FN void refuse(const Exec &ex, int B, int first, int status, int32_t *ids, float *out, int32_t *info) {
    for (int b = first; b < B; ++b) {
        blank(ex, ids + (int64_t)b * TRACK_MAX, out + 4 * (int64_t)b * TRACK_MAX, 0);
        if (ex.lane() == 0) {
            int32_t *info_b = info + 4 * (int64_t)b;
            info_b[STATUS] = status;
            info_b[LIVE] = info_b[BORN] = info_b[DROPPED] = 0;
        }
    }
}

// is this header one of a usable blob of M slots?
BEV_MET_FN bool header_ok(const int32_t *h, int M) {
    return h[H_MAGIC] == MAGIC && h[H_MAX] == M && h[H_COUNT] >= 0 && h[H_COUNT] <= M && h[H_NEXT_ID] >= 0 &&
           h[H_FRAMES] >= 0;
}

}  // namespace bev_track
