// bev_tune.h -- internal: the per-source halves of bev_tune() (bev_conv.hip), which sets the performance knobs.
// Results never depend on them.
#pragma once

namespace bev {

// What setting a knob does: a value outside 0..max is refused (-1 = BEV_ERR_ARGS), else the previous value is returned.
inline int swap_knob(int &slot, int value, int max) {
    if (value < 0 || value > max) return -1;
    const int old = slot;
    slot = value;
    return old;
}

// knob = BEV_TUNE_WARP_* (include/bev_mi355x.h); returns the previous value or BEV_ERR_ARGS.
int warp_tune(int knob, int value);

// LDS image of the warp backward (bev_warp_bwd.hip) in floats: BEV_TUNE_WARP_BWD_POOL, 0 = the maximum.
constexpr int WARP_BWD_POOL_MAX = 19968;  // 78 KiB: two workgroups per CU (k_warp_bwd_runs holds 256 VGPRs)
int warp_bwd_pool_floats();

// knob = BEV_TUNE_WGRAD_MFMA (bev_train.hip).
int train_tune(int knob, int value);

// BEV_TUNE_CONV_X6_TILE / _KERNEL / _NT / _STRIP / _BUF (bev_conv_x6.hip).
int conv_x6_tune(int knob, int value);

// BEV_TUNE_CONV_H16_KERNEL (bev_conv_h16.hip): forward tile width / the 32-deep k_conv_h16 (1); weight gradient: 1 =
// k_wgrad_h16b always, else k_wgrad_h16c where it applies.
int conv_h16_tune(int value);
// BEV_TUNE_CONV_H16_BUF (bev_conv_h16.hip).
int conv_h16_buf_tune(int value);

// BEV_TUNE_DW_RUN (bev_effnet.hip).
int dw_tune(int value);
int stem3_tune(int value);

}  // namespace bev
