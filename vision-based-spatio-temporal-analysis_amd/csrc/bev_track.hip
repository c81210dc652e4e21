// bev_track.hip -- the online tracker on the BEV detections (the reference's README, phase 3; csrc/bev_track.h is the
// procedure), one launch per batch on the decode's own output buffers: no host synchronisation, no allocation, no
// atomics, nothing a graph capture cannot record.
//
//   k_track_step   one workgroup of one wave per sequence, as k_det_assign has per frame.  The wave stages the
//                  sequence's track table from its state blob into LDS beside the solver's arrays, walks the launch's
//                  frames in time order through bev_track::frame_step -- the very procedure of the host entry, with
//                  the 64 lanes as its workers -- and writes the table back once, after the last frame: the blob has
//                  one writer per launch and launches on a stream are ordered, so nothing can observe it in between.
//                  Only slots below the larger of the two counts are written; the rest were zero and stay zero.
//   k_track_reset  one workgroup writes an empty blob: zeros and the header.
//
// LDS: the solver's 59 KiB (three double, four float, three int32, three int16 arrays and one of bytes, 1024 entries
// each) and the table's 72 KiB (seven double and four int32 arrays) = 131 KiB of gfx950's 160 KiB: one workgroup,
// which is one wave, per CU.  A sequence is a chain of dependent searches, latency-bound by design like the
// assignment kernel; S sequences occupy S CUs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bev_mi355x.h"
#include "bev_track.h"

namespace {

namespace tr = bev_track;
namespace mt = bev_metrics;

constexpr int TR_T = 64;
constexpr int TR_MAX = tr::TRACK_MAX;
constexpr int RESET_T = 256;

struct WaveExec {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return TR_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ mt::Best reduce(mt::Best b) const {
        for (int off = TR_T / 2; off; off >>= 1) {
            mt::Best o;
            o.v.k = __shfl_xor(b.v.k, off, TR_T);
            o.v.s = __shfl_xor(b.v.s, off, TR_T);
            o.j = __shfl_xor(b.j, off, TR_T);
            if (mt::best_before(o, b)) b = o;
        }
        return b;  // a total order: every lane holds the same element
    }
    __device__ __forceinline__ int prefix(bool flag, int *total) const {
        const unsigned long long m = __ballot(flag);
        *total = __popcll(m);
        return __popcll(m & ((1ull << threadIdx.x) - 1ull));
    }
};

__global__ __launch_bounds__(TR_T) void k_track_step(const float *__restrict__ pred,
                                                     const int32_t *__restrict__ pred_count, int B, int cap, int first,
                                                     bev_track_params P, char *__restrict__ states, int64_t stride,
                                                     int32_t *__restrict__ ids, float *__restrict__ out,
                                                     int32_t *__restrict__ info) {
    __shared__ double us[TR_MAX], vs[TR_MAX], sps[TR_MAX];
    __shared__ double tx[TR_MAX], ty[TR_MAX], tvx[TR_MAX], tvy[TR_MAX], tp00[TR_MAX], tp01[TR_MAX], tp11[TR_MAX];
    __shared__ float px[TR_MAX], py[TR_MAX], gx[TR_MAX], gy[TR_MAX];
    __shared__ int32_t uk[TR_MAX], vk[TR_MAX], spk[TR_MAX];
    __shared__ int32_t t_id[TR_MAX], t_streak[TR_MAX], t_misses[TR_MAX], t_age[TR_MAX];
    __shared__ int16_t path[TR_MAX], colrow[TR_MAX], rowcol[TR_MAX];
    __shared__ uint8_t sc[TR_MAX];
    const int64_t f0 = (int64_t)blockIdx.x * B;  // the sequence's first frame
    const int tid = threadIdx.x, M = P.max_tracks;
    char *blob = states + (int64_t)blockIdx.x * stride;
    int32_t *hdr = (int32_t *)blob;
    pred += 4 * f0 * cap;
    pred_count += f0;
    ids += f0 * TR_MAX;
    out += 4 * f0 * TR_MAX;
    info += 4 * f0;
    const WaveExec ex;
    // wave-uniform from here on: every lane reads the same header words
    if (!tr::header_ok(hdr, M)) {
        tr::refuse(ex, B, first, tr::ST_BAD_STATE, ids, out, info);
        return;
    }
    tr::Seq q = {hdr[tr::H_COUNT], hdr[tr::H_NEXT_ID], hdr[tr::H_FRAMES], first > 0 ? 0 : hdr[tr::H_STALLED]};
    if (q.stalled) {  // an earlier launch met a pending frame: only the host's replay (first > 0) goes on
        tr::refuse(ex, B, first, tr::ST_STALLED, ids, out, info);
        return;
    }
    const tr::Table G = tr::table_of(blob, M);
    const tr::Table T = {tx, ty, tvx, tvy, tp00, tp01, tp11, t_id, t_streak, t_misses, t_age};
    const mt::AssignState<int16_t> S = {px, py, gx, gy, uk, vk, spk, us, vs, sps, path, colrow, rowcol, sc};
    const int count_in = q.count;
    for (int i = tid; i < count_in; i += TR_T) tr::put(T, i, tr::get(G, i));
    __syncthreads();
    tr::walk(ex, T, S, q, M, P, pred, pred_count, B, cap, first, ids, out, info);
    __syncthreads();
    const int hi = count_in > q.count ? count_in : q.count;
    for (int i = tid; i < hi; i += TR_T) tr::put(G, i, i < q.count ? tr::get(T, i) : tr::no_track());
    if (tid == 0) {
        hdr[tr::H_COUNT] = q.count;
        hdr[tr::H_NEXT_ID] = q.next_id;
        hdr[tr::H_FRAMES] = q.frames_seen;
        hdr[tr::H_STALLED] = q.stalled;
    }
}

__global__ __launch_bounds__(RESET_T) void k_track_reset(int32_t *__restrict__ blob, int words, int max_tracks) {
    for (int w = threadIdx.x; w < words; w += RESET_T)
        blob[w] = w == tr::H_MAGIC ? (int32_t)tr::MAGIC : w == tr::H_MAX ? max_tracks : 0;
}

int check_reset(const void *state, int max_tracks) {
    if (!state || ((uintptr_t)state & 15) || max_tracks < 1 || max_tracks > TR_MAX) return BEV_ERR_ARGS;
    return 0;
}

// the checks the two step entries share; 0 when the arguments are usable
int check_step(const void *pred, const void *pred_count, int S, int B, int cap, int first, const bev_track_params &P,
               const void *states, int64_t stride, const void *ids, const void *out, const void *info) {
    if (S < 0 || B < 0 || B > tr::MAX_FRAMES || cap < 0 || first < 0 || first > B) return BEV_ERR_ARGS;
    if (!tr::params_ok(P)) return BEV_ERR_ARGS;
    if (S == 0 || B == 0) return 0;
    if (!pred_count || !states || !ids || !out || !info) return BEV_ERR_ARGS;
    if (cap > 0 && !pred) return BEV_ERR_ARGS;
    if (((uintptr_t)states & 15) || (stride & 15) || stride < tr::state_bytes(P.max_tracks)) return BEV_ERR_ARGS;
    return 0;
}

}  // namespace

extern "C" {

int64_t bev_track_state_bytes(int max_tracks) {
    if (max_tracks < 1 || max_tracks > TR_MAX) return BEV_ERR_ARGS;
    return tr::state_bytes(max_tracks);
}

int bev_track_max_frame(void) { return TR_MAX; }

int bev_track_reset(void *state, int max_tracks, void *stream) {
    const int rc = check_reset(state, max_tracks);
    if (rc) return rc;
    hipLaunchKernelGGL(k_track_reset, dim3(1), dim3(RESET_T), 0, (hipStream_t)stream, (int32_t *)state,
                       (int)(tr::state_bytes(max_tracks) / 4), max_tracks);
    return (int)hipGetLastError();
}

int bev_track_reset_host(void *state, int max_tracks) {
    const int rc = check_reset(state, max_tracks);
    if (rc) return rc;
    memset(state, 0, (size_t)tr::state_bytes(max_tracks));
    int32_t *hdr = (int32_t *)state;
    hdr[tr::H_MAGIC] = (int32_t)tr::MAGIC;
    hdr[tr::H_MAX] = max_tracks;
    return 0;
}

int bev_track_step_f32(const float *pred, const int32_t *pred_count, int S, int B, int cap, int first,
                       bev_track_params params, void *states, int64_t state_stride_bytes, int32_t *ids,
                       float *track_out, int32_t *info, void *stream) {
    const int rc = check_step(pred, pred_count, S, B, cap, first, params, states, state_stride_bytes, ids, track_out,
                              info);
    if (rc) return rc;
    if (S == 0 || B == 0) return 0;
    hipLaunchKernelGGL(k_track_step, dim3(S), dim3(TR_T), 0, (hipStream_t)stream, pred, pred_count, B, cap, first,
                       params, (char *)states, state_stride_bytes, ids, track_out, info);
    return (int)hipGetLastError();
}

int bev_track_step_host(const float *pred, const int32_t *pred_count, int S, int B, int cap, int first,
                        bev_track_params params, void *states, int64_t state_stride_bytes, int32_t *ids,
                        float *track_out, int32_t *info) {
    const int rc = check_step(pred, pred_count, S, B, cap, first, params, states, state_stride_bytes, ids, track_out,
                              info);
    if (rc) return rc;
    if (S == 0 || B == 0) return 0;
    const int M = params.max_tracks;
    const size_t n = TR_MAX;
    std::vector<float> px(n), py(n), gx(n), gy(n);
    std::vector<int32_t> uk(n), vk(n), spk(n), path(n), colrow(n), rowcol(n);
    std::vector<double> us(n), vs(n), sps(n);
    std::vector<uint8_t> sc(n);
    const mt::AssignState<int32_t> A = {px.data(), py.data(), gx.data(),   gy.data(),     uk.data(),
                                        vk.data(), spk.data(), us.data(),  vs.data(),     sps.data(),
                                        path.data(), colrow.data(), rowcol.data(), sc.data()};
    const tr::SerialExec ex;
    for (int s = 0; s < S; ++s) {
        const int64_t f0 = (int64_t)s * B;
        char *blob = (char *)states + (int64_t)s * state_stride_bytes;
        int32_t *hdr = (int32_t *)blob;
        int32_t *ids_s = ids + f0 * TR_MAX, *info_s = info + 4 * f0;
        float *out_s = track_out + 4 * f0 * TR_MAX;
        if (!tr::header_ok(hdr, M)) {
            tr::refuse(ex, B, first, tr::ST_BAD_STATE, ids_s, out_s, info_s);
            continue;
        }
        tr::Seq q = {hdr[tr::H_COUNT], hdr[tr::H_NEXT_ID], hdr[tr::H_FRAMES], first > 0 ? 0 : hdr[tr::H_STALLED]};
        if (q.stalled) {
            tr::refuse(ex, B, first, tr::ST_STALLED, ids_s, out_s, info_s);
            continue;
        }
        // the table is worked on in place: its slots at and behind the count are zero before and after every frame
        tr::walk(ex, tr::table_of(blob, M), A, q, M, params, pred + 4 * f0 * cap, pred_count + f0, B, cap, first, ids_s,
                 out_s, info_s);
        hdr[tr::H_COUNT] = q.count;
        hdr[tr::H_NEXT_ID] = q.next_id;
        hdr[tr::H_FRAMES] = q.frames_seen;
        hdr[tr::H_STALLED] = q.stalled;
    }
    return 0;
}

}  // extern "C"
