// bev_targets.hip -- BEVNet's CenterNet training targets in two launches (model_wrapper.py:126-203, 278-300 of the
// reference; BEVNet._targets_from_boxes / _splat_gaussians here, which build them from ~40 small torch ops and an
// [N, (2R+1)^2] window tensor).
//
//   k_tgt_slots    one workgroup per frame walks all N boxes in array order, 256 at a time: the boxes of its frame
//                  whose centre is inside the grid are ranked by a wave64 ballot + prefix count, the first M in order
//                  take the slots.  Writes every element of indices / mask / offset / size_log [B][M] and, for the
//                  heatmap pass, the frame's compact list of (cx, cy, radius, 2 sigma^2) of the slotted objects with
//                  radius > 0, plus its length.  A frame value is only ever compared with the workgroup's frame.
//   k_tgt_heatmap  one workgroup per 64 x 16 tile of heatmap [B][1][Hb][Wb]: loads the frame's list 256 entries at a
//                  time, keeps the objects whose window meets the tile (ballot compaction into LDS), and computes each
//                  of its cells as the maximum over them -- every cell stored exactly once (zeros included), as a
//                  16-byte store where the rows allow.  No atomics, no radius bound, no window tensor.
//
// The per-object arithmetic is bev_targets.h (torch's float32 op sequence), shared with bev_centernet_targets_host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bev_mi355x.h"
#include "bev_targets.h"

namespace {

namespace tg = bev_targets;

constexpr int TG_T = 256;                      // threads per workgroup (4 waves)
constexpr int TG_TILE_W = 64, TG_TILE_H = 16;  // heatmap tile: 4 cells of a row per thread
constexpr int64_t TG_MAX_CELLS = (int64_t)1 << 28;  // Hb * Wb
constexpr int64_t TG_MAX_SLOTS = (int64_t)1 << 24;  // B * M

// the workspace: per frame one 16-byte header (word 0 = the list's length) and M list entries
__host__ __device__ inline int64_t ws_frame_entries(int M) { return (int64_t)M + 1; }

// this thread's rank among the workgroup's threads with `pred` set, in thread order, and their number.  Called by
// every thread of the workgroup; wave_cnt is LDS [TG_T / 64].  The leading barrier also orders whatever LDS the caller
// read before the call against what it writes after it.
__device__ __forceinline__ int block_rank(bool pred, int *wave_cnt, int &total) {
    const unsigned long long m = __ballot(pred);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TG_T / 64; ++w) {
        const int c = wave_cnt[w];
        before += w < wave ? c : 0;
        tot += c;
    }
    total = tot;
    return before + r;
}

__global__ __launch_bounds__(TG_T) void k_tgt_slots(const float *__restrict__ boxes, const int64_t *__restrict__ frame,
                                                    int N, int M, tg::Grid g, tg::RadiusConsts k,
                                                    int64_t *__restrict__ indices, float *__restrict__ mask,
                                                    float *__restrict__ offset, float *__restrict__ size_log,
                                                    tg::Splat *__restrict__ ws) {
    __shared__ int wave_cnt[TG_T / 64];
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * M;
    tg::Splat *head = ws + (int64_t)b * ws_frame_entries(M);
    tg::Splat *list = head + 1;
    int kept = 0, drawn = 0;  // workgroup-uniform
    for (int64_t i0 = 0; i0 < N && kept < M; i0 += TG_T) {
        const int64_t i = i0 + threadIdx.x;
        tg::Object o;
        o.inside = false;
        if (i < N && frame[i] == (int64_t)b)
            o = tg::object_on_grid(boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], g);
        int n_in, n_draw;
        const int slot = kept + block_rank(o.inside, wave_cnt, n_in);
        const bool sel = o.inside && slot < M;
        const int64_t radius = sel ? tg::gaussian_radius(o.w_cells, o.h_cells, k) : 0;
        const bool draw = sel && radius > 0;
        const int at = drawn + block_rank(draw, wave_cnt, n_draw);
        if (sel) {
            indices[row + slot] = (int64_t)o.cy * g.Wb + o.cx;
            mask[row + slot] = 1.0f;
            offset[2 * (row + slot)] = o.off_x;
            offset[2 * (row + slot) + 1] = o.off_y;
            size_log[2 * (row + slot)] = o.log_w;
            size_log[2 * (row + slot) + 1] = o.log_h;
        }
        if (draw) list[at] = tg::make_splat(o.cx, o.cy, radius, g);  // at < M: the drawn are among the slotted
        kept += n_in;
        drawn += n_draw;
    }
    kept = kept < M ? kept : M;
    for (int s = kept + threadIdx.x; s < M; s += TG_T) {  // the empty slots
        indices[row + s] = 0;
        mask[row + s] = 0.0f;
        offset[2 * (row + s)] = 0.0f;
        offset[2 * (row + s) + 1] = 0.0f;
        size_log[2 * (row + s)] = 0.0f;
        size_log[2 * (row + s) + 1] = 0.0f;
    }
    if (threadIdx.x == 0) {
        tg::Splat h = {drawn, 0, 0, 0.0f};
        *head = h;
    }
}

// VEC: Wb % 4 == 0 and a 16-byte aligned heatmap -- every thread's 4 cells are one aligned float4
template <bool VEC>
__global__ __launch_bounds__(TG_T) void k_tgt_heatmap(const tg::Splat *__restrict__ ws, int M, int Hb, int Wb,
                                                      int tiles_x, int tiles_y, float *__restrict__ hm) {
    __shared__ tg::Splat live[TG_T];
    __shared__ int wave_cnt[TG_T / 64];
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int x0 = tx * TG_TILE_W, y0 = ty * TG_TILE_H;
    const int x1 = (x0 + TG_TILE_W < Wb ? x0 + TG_TILE_W : Wb) - 1;
    const int y1 = (y0 + TG_TILE_H < Hb ? y0 + TG_TILE_H : Hb) - 1;
    const tg::Splat *head = ws + (int64_t)b * ws_frame_entries(M);
    const tg::Splat *list = head + 1;
    int count = head->cx;
    count = count < 0 ? 0 : (count < M ? count : M);  // never read past the frame's list
    const int x = x0 + (threadIdx.x % (TG_TILE_W / 4)) * 4, y = y0 + threadIdx.x / (TG_TILE_W / 4);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c0 = 0; c0 < count; c0 += TG_T) {
        const int j = c0 + threadIdx.x;
        tg::Splat s = {0, 0, 0, 1.0f};
        bool hit = false;
        if (j < count) {
            s = list[j];
            hit = s.cx + s.r >= x0 && s.cx - s.r <= x1 && s.cy + s.r >= y0 && s.cy - s.r <= y1;
        }
        int n_live;
        const int at = block_rank(hit, wave_cnt, n_live);
        if (hit) live[at] = s;
        __syncthreads();
        if (y < Hb) {
            for (int q = 0; q < n_live; ++q) {
                const tg::Splat o = live[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = tg::splat_at(o, x + e, y);
                    v[e] = a > v[e] ? a : v[e];
                }
            }
        }
    }
    if (y >= Hb) return;
    float *dst = hm + ((int64_t)b * Hb + y) * Wb + x;
    if (VEC) {
        if (x < Wb) *(float4 *)dst = make_float4(v[0], v[1], v[2], v[3]);  // Wb % 4 == 0: x + 3 < Wb
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x + e < Wb) dst[e] = v[e];
    }
}

// the checks both entries share; 0 when the arguments are usable
int check_args(const void *boxes, const void *frame, int N, int B, int M, int Hb, int Wb, const void *heatmap,
               const void *indices, const void *mask, const void *offset, const void *size_log) {
    if (N < 0 || B < 0 || M < 0 || Hb <= 0 || Wb <= 0) return BEV_ERR_ARGS;
    if ((int64_t)Hb * Wb > TG_MAX_CELLS || (int64_t)B * M > TG_MAX_SLOTS) return BEV_ERR_ARGS;
    if (N > 0 && (!boxes || !frame)) return BEV_ERR_ARGS;
    if (B > 0 && !heatmap) return BEV_ERR_ARGS;
    if ((int64_t)B * M > 0 && (!indices || !mask || !offset || !size_log)) return BEV_ERR_ARGS;
    return 0;
}

}  // namespace

extern "C" {

int64_t bev_centernet_targets_workspace_bytes(int B, int M) {
    if (B < 0 || M < 0 || (int64_t)B * M > TG_MAX_SLOTS) return 0;
    return (int64_t)B * ws_frame_entries(M) * (int64_t)sizeof(tg::Splat);
}

int bev_centernet_targets_f32(const float *boxes, const int64_t *frame, int N, int B, int M, int Hb, int Wb,
                              float x_min, float y_min, float rcp_res_x, float rcp_res_y, float f_1mov, float rcp_1pov,
                              float f_4ov, float f_m2ov, float f_ovm1, int ov_zero, float min_radius, float *heatmap,
                              int64_t *indices, float *mask, float *offset, float *size_log, void *workspace,
                              int64_t workspace_bytes, void *stream) {
    const int rc = check_args(boxes, frame, N, B, M, Hb, Wb, heatmap, indices, mask, offset, size_log);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < bev_centernet_targets_workspace_bytes(B, M))
        return BEV_ERR_ARGS;
    const int tiles_x = (Wb + TG_TILE_W - 1) / TG_TILE_W, tiles_y = (Hb + TG_TILE_H - 1) / TG_TILE_H;
    const int64_t tiles = (int64_t)B * tiles_x * tiles_y;
    if (tiles > 0x7fffffff) return BEV_ERR_ARGS;
    const tg::Grid g = {Hb, Wb, x_min, y_min, rcp_res_x, rcp_res_y};
    const tg::RadiusConsts k = {f_1mov, rcp_1pov, f_4ov, f_m2ov, f_ovm1, ov_zero, min_radius};
    hipStream_t st = (hipStream_t)stream;
    tg::Splat *ws = (tg::Splat *)workspace;
    hipLaunchKernelGGL(k_tgt_slots, dim3(B), dim3(TG_T), 0, st, boxes, frame, N, M, g, k, indices, mask, offset,
                       size_log, ws);
    if (Wb % 4 == 0 && ((uintptr_t)heatmap & 15) == 0)
        hipLaunchKernelGGL(k_tgt_heatmap<true>, dim3((unsigned)tiles), dim3(TG_T), 0, st, ws, M, Hb, Wb, tiles_x,
                           tiles_y, heatmap);
    else
        hipLaunchKernelGGL(k_tgt_heatmap<false>, dim3((unsigned)tiles), dim3(TG_T), 0, st, ws, M, Hb, Wb, tiles_x,
                           tiles_y, heatmap);
    return (int)hipGetLastError();
}

int bev_centernet_targets_host(const float *boxes, const int64_t *frame, int N, int B, int M, int Hb, int Wb,
                               float x_min, float y_min, float rcp_res_x, float rcp_res_y, float f_1mov,
                               float rcp_1pov, float f_4ov, float f_m2ov, float f_ovm1, int ov_zero, float min_radius,
                               float *heatmap, int64_t *indices, float *mask, float *offset, float *size_log) {
    const int rc = check_args(boxes, frame, N, B, M, Hb, Wb, heatmap, indices, mask, offset, size_log);
    if (rc) return rc;
    const tg::Grid g = {Hb, Wb, x_min, y_min, rcp_res_x, rcp_res_y};
    const tg::RadiusConsts k = {f_1mov, rcp_1pov, f_4ov, f_m2ov, f_ovm1, ov_zero, min_radius};
    const int64_t cells = (int64_t)Hb * Wb;
    for (int b = 0; b < B; ++b) {
        float *hm = heatmap + b * cells;
        for (int64_t c = 0; c < cells; ++c) hm[c] = 0.0f;
        const int64_t row = (int64_t)b * M;
        for (int64_t s = 0; s < M; ++s) {
            indices[row + s] = 0;
            mask[row + s] = 0.0f;
            offset[2 * (row + s)] = offset[2 * (row + s) + 1] = 0.0f;
            size_log[2 * (row + s)] = size_log[2 * (row + s) + 1] = 0.0f;
        }
        int64_t slot = 0;
        for (int64_t i = 0; i < N && slot < M; ++i) {
            if (frame[i] != (int64_t)b) continue;
            const float *bx = boxes + 4 * i;
            const tg::Object o = tg::object_on_grid(bx[0], bx[1], bx[2], bx[3], g);
            if (!o.inside) continue;
            indices[row + slot] = (int64_t)o.cy * Wb + o.cx;
            mask[row + slot] = 1.0f;
            offset[2 * (row + slot)] = o.off_x;
            offset[2 * (row + slot) + 1] = o.off_y;
            size_log[2 * (row + slot)] = o.log_w;
            size_log[2 * (row + slot) + 1] = o.log_h;
            ++slot;
            const int64_t radius = tg::gaussian_radius(o.w_cells, o.h_cells, k);
            if (radius <= 0) continue;
            const tg::Splat sp = tg::make_splat(o.cx, o.cy, radius, g);
            const int ya = sp.cy - sp.r > 0 ? sp.cy - sp.r : 0, yb = sp.cy + sp.r < Hb - 1 ? sp.cy + sp.r : Hb - 1;
            const int xa = sp.cx - sp.r > 0 ? sp.cx - sp.r : 0, xb = sp.cx + sp.r < Wb - 1 ? sp.cx + sp.r : Wb - 1;
            for (int y = ya; y <= yb; ++y)
                for (int x = xa; x <= xb; ++x) {
                    const float a = tg::splat_at(sp, x, y);
                    float *cell = hm + (int64_t)y * Wb + x;
                    if (a > *cell) *cell = a;
                }
        }
    }
    return 0;
}

}  // extern "C"
