// The crop -> frame map of the kernels that read the observed frame through a crop window (warp.hip: k_warp, k_depth_agreement;
// icp.hip: k_icp_pairs): ONE definition, so the texel a crop pixel reads is the same in all of them, bit for bit.
#pragma once
#include "fp_common.h"

__device__ __forceinline__ int nn_index(float x) { return (int)rintf(x); }  // half-to-even like grid_sample nearest

// crop_inverse: the per-hypothesis constants, the inverse of the scale + translate crop transform tf = [sx 0 tx; 0 sy ty; 0 0 1],
// computed by ONE lane of a workgroup into LDS (inv[0..3] = 1/sx, 1/sy, -tx/sx, -ty/sy).  crop_to_frame: the frame coordinates of
// crop pixel (i, j) as grid_sample(align_corners=False) sees them; nn_index of them is the texel a nearest read takes.
__device__ __forceinline__ void crop_inverse(float sx, float tx, float sy, float ty, float* inv) {
  inv[0] = 1.0f / sx;
  inv[1] = 1.0f / sy;
  inv[2] = (-tx) / sx;
  inv[3] = (-ty) / sy;
}

__device__ __forceinline__ void crop_to_frame(int i, int j, float i00, float i02, float i11, float i12, float cW, float cH, float& ix,
                                              float& iy) {
  const float xs = fmaf((float)i, i00, i02), ys = fmaf((float)j, i11, i12);
  ix = fmaf(xs, cW, -0.5f);
  iy = fmaf(ys, cH, -0.5f);
}

// The frame constants W/(W-1), H/(H-1) and the row / column of a crop pixel (an emulated integer division) come from the host: float
// division there is the same IEEE operation, the integer division a multiply-shift.
struct WarpConst { float cW, cH; unsigned mul_ow, shr_ow; };

static inline WarpConst warp_const(int H, int W, int ow) {
  WarpConst wc;
  wc.cW = (float)W / (float)(W - 1);
  wc.cH = (float)H / (float)(H - 1);
  {   // p / ow for p < oh * ow <= 2^20 as umulhi(p, mul) >> shr (exact: ceil(2^(31+lg) / ow) with lg = ceil(log2 ow)); 0 = divisor 1
    wc.mul_ow = 0; wc.shr_ow = 0;
    if (ow > 1) {
      int lg = 0;
      while ((1u << lg) < (unsigned)ow) ++lg;
      const int sh = 31 + lg;
      wc.mul_ow = (unsigned)(((1ull << sh) + (unsigned)ow - 1) / (unsigned)ow);
      wc.shr_ow = (unsigned)(sh - 32);
    }
  }
  return wc;
}
