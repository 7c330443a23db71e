// What the reconstruction entry points (tsdf.hip, tsdf_raycast.hip, tsdf_components.hip, texture_bake.hip) share, one copy: the walk
// over a stack of posed RGB-D views (k_tsdf_integrate projects a voxel into every view, k_texture_bake a texel: the fused mesh and its
// texture skip the same views and round to the same pixel because both call the pieces below), the volume's grid and the two small
// functions its surface is read with, and the checks of the arguments the entry points have in common.  The files are SRCS_EXACT
// (-ffp-contract=off): the operations written here are the ones executed, in this order and bracketing (include/fp_amd.h defines
// them); the numpy restatements (tests/tsdf_model.py, texture_bake_model.py, tsdf_raycast_model.py) each state them again on their own.
#pragma once
#include "fp_common.h"

#include <math.h>

namespace recon {

__device__ __forceinline__ bool finite4(float a, float b, float c, float d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

// ---- The posed views: depth (V,H,W), rgb (V,H,W,3), masks (V,H,W) or NULL, poses (V,4,4) object-to-camera, Ks (V,3,3) float64.
// (fp_views, of fp_common.h, is the table of intrinsics the crop stages index by row; this is a stack of whole frames.)
struct ViewStack {
  const float* depth;
  const float* rgb;
  const uint8_t* masks;
  const float* poses;
  const double* Ks;
  int V, H, W;
};

struct Pinhole {
  float fx, fy, cx, cy;
};

// The walk, in the order a kernel calls its pieces for view v = 0 .. V-1; what a kernel does between them and with the pixel (the
// bake's facing test before the pixel, the fusion's carving of unmasked pixels after it) is its own.
// 1. view v's pose T and camera; false: the view is skipped (an intrinsic or a pose element that is not finite, or a skew).  Wave-uniform.
__device__ __forceinline__ bool load_view(const ViewStack& in, int v, const float*& T, Pinhole& cam) {
  T = in.poses + (size_t)v * 16;
  const double* Kd = in.Ks + (size_t)v * 9;
  const float fx = (float)Kd[0], skew = (float)Kd[1], cx = (float)Kd[2], fy = (float)Kd[4], cy = (float)Kd[5];
  bool ok = finite4(fx, fy, cx, cy) && skew == 0.f;
#pragma unroll
  for (int k = 0; k < 16; k += 4) ok = ok && finite4(T[k], T[k + 1], T[k + 2], T[k + 3]);
  cam = Pinhole{fx, fy, cx, cy};
  return ok;
}

// 2. the point (px, py, pz) of the object frame in the camera's; the caller goes on only where Z > 0
__device__ __forceinline__ void to_camera(const float* T, float px, float py, float pz, float& X, float& Y, float& Z) {
  X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
  Y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
  Z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
}

// 3. the pixel (X, Y, Z), Z > 0, falls on, rounded half up; false: outside the frame.  p indexes depth and masks, 3 p rgb.
__device__ __forceinline__ bool pixel_of(const ViewStack& in, int v, const Pinhole& cam, float X, float Y, float Z, size_t& p) {
  const float Wf = (float)in.W, Hf = (float)in.H;
  const float fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
  const float uf = floorf(((fx * X) / Z + cx) + 0.5f), vf = floorf(((fy * Y) / Z + cy) + 0.5f);
  if (!(uf >= 0.f && uf < Wf && vf >= 0.f && vf < Hf)) return false;
  p = ((size_t)v * in.H + (size_t)(int)vf) * in.W + (size_t)(int)uf;
  return true;
}

// ---- The volume: voxel (ix, iy, iz) of nz x ny x nx, x fastest, stands at (ox, oy, oz) + (ix, iy, iz) * s
struct Grid {
  int nz, ny, nx;
  float ox, oy, oz, s;
};

// the gradient of tsdf along one axis at voxel `at` (coordinate c of n along it, n >= 2, `stride` voxels apart)
__device__ __forceinline__ float axis_gradient(const float* __restrict__ f, size_t at, size_t stride, int c, int n) {
  if (c == 0) return f[at + stride] - f[at];
  if (c == n - 1) return f[at] - f[at - stride];
  return 0.5f * (f[at + stride] - f[at - stride]);
}

__device__ __forceinline__ float lerp_from_a(float a, float b, float t) { return a + t * (b - a); }

// ---- The arguments the entry points have in common, checked once.  `who` is the entry point's name; the caller does
// `if (int st = recon::check_...(who, ...)) return st;` and puts the checks of its own arguments where they have always been.
static inline int check_grid(const char* who, int nz, int ny, int nx) {
  FP_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1 && nz <= FP_TSDF_MAX_DIM && ny <= FP_TSDF_MAX_DIM && nx <= FP_TSDF_MAX_DIM,
             "%s: volume %d x %d x %d (nz, ny, nx) has a dimension outside 1..%d", who, nz, ny, nx, FP_TSDF_MAX_DIM);
  FP_REQUIRE((long long)nz * ny * nx <= (1ll << 30), "%s: volume %d x %d x %d has more than 2^30 voxels", who, nz, ny, nx);
  return FP_OK;
}

static inline int check_origin(const char* who, const float* origin, float voxel) {
  FP_REQUIRE(origin, "%s: NULL origin", who);
  FP_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "%s: origin (%g, %g, %g) is not finite", who,
             (double)origin[0], (double)origin[1], (double)origin[2]);
  FP_REQUIRE(isfinite(voxel) && voxel > 0.f, "%s: voxel=%g must be finite and > 0", who, (double)voxel);
  return FP_OK;
}

// the sizes of a view stack; `hint` ends the V message: what the caller can do about too many views, or ""
static inline int check_view_stack(const char* who, int V, int H, int W, const char* hint) {
  FP_REQUIRE(V >= 0 && V <= 4096, "%s: V=%d outside 0..4096%s", who, V, hint);
  FP_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d must be >= 1", who, H, W);
  FP_REQUIRE((long long)H * W <= (1ll << 28), "%s: more than 2^28 pixels (%d x %d)", who, H, W);
  return FP_OK;
}

static inline int check_min_depth(const char* who, float d) {
  FP_REQUIRE(isfinite(d) && d >= 0.f, "%s: min_depth=%g must be finite and >= 0", who, (double)d);
  return FP_OK;
}
static inline int check_min_weight(const char* who, float w) {
  FP_REQUIRE(isfinite(w), "%s: min_weight=%g must be finite", who, (double)w);
  return FP_OK;
}

}  // namespace recon
