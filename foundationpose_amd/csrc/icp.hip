// One Gauss-Newton step of point-to-plane ICP per hypothesis (fp_icp_point_plane; the definition is in include/fp_amd.h): the render of
// the model at a pose (camera-frame xyz and unit normal crops) against the observed points the REFINE warp reads through the same crop
// window.  Two launches on the caller's stream, no atomics, no memset, no allocation, no synchronisation:
//   k_icp_pairs   grid (chunks of 256 crop pixels, n), one lane per crop pixel as k_depth_agreement: the float32 residual r and
//                 Jacobian row J of the pixel's pair (or nothing), then the 28 products J_i*J_j (i <= j), J_i*r and r*r as float64
//                 (exact: each is the product of two float32 values), summed over the wave by an xor tree (run transposed), over the workgroup's four
//                 waves in index order through LDS; one row of 28 sums + the pair count per workgroup goes to partial[n][chunk].
//   k_icp_finish  one wave per hypothesis: lane t < 29 adds column t of the hypothesis' partial rows in chunk order; lane 0 then damps,
//                 factors (LDL^T without pivoting), solves and updates the pose in float64, and writes system[n] and poses_out[n].
// A chunk is 256 consecutive crop pixels summed in one fixed order and the chunks are added in index order: the order of every sum
// depends on (oh, ow) alone, so row n of a batch has the bits of the call on hypothesis n alone and every replay the bits of the first
// run.  A lane without a pair adds +0.  Compiled with -ffp-contract=off (SRCS_EXACT): the float32 per-pixel values are the ones the numpy
// restatement (tests/icp_model.py) computes, bit for bit.
#include "fp_common.h"
#include "crop_map.h"
#include "icp_solve.h"

namespace {

using namespace icp_solve;   // the wave tree, the chunk sums, the solve and the update: shared with mesh_icp.hip

constexpr int kCols = kTerms + 1;      // + the pair count

__global__ __launch_bounds__(kThreads) void k_icp_pairs(const float* __restrict__ xyz_crops, const float* __restrict__ normal_crops,
                                                        const float* __restrict__ xyz_map, const float* __restrict__ tfs, fp_views vt,
                                                        int H, int W, const float* __restrict__ poses, int oh, int ow, float max_dist,
                                                        WarpConst wc, int C, double* __restrict__ partial) {
  __shared__ float inv_tf[4];
  __shared__ double red[kWaves][kTerms];
  __shared__ int cnt[kWaves];
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    const float* tf = tfs + (size_t)n * 9;
    crop_inverse(tf[0], tf[2], tf[4], tf[5], inv_tf);
  }
  __syncthreads();
  const int npx = oh * ow;
  const int px = blockIdx.x * kThreads + threadIdx.x;
  const int v = fp_view_of(vt, n);
  const float md2 = max_dist * max_dist;
  float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r = 0.f;
  bool pair = false;
  if (px < npx) {   // no early return: every lane takes part in the shuffles, the ballot and the barrier below
    const int j = wc.mul_ow ? (int)(__umulhi((unsigned)px, wc.mul_ow) >> wc.shr_ow) : px;
    const int i = px - j * ow;
    const size_t o = ((size_t)n * npx + px) * 3;
    const float p0 = xyz_crops[o], p1 = xyz_crops[o + 1], p2 = xyz_crops[o + 2];
    const float m0 = normal_crops[o], m1 = normal_crops[o + 1], m2 = normal_crops[o + 2];
    float ix, iy;
    crop_to_frame(i, j, inv_tf[0], inv_tf[2], inv_tf[1], inv_tf[3], wc.cW, wc.cH, ix, iy);
    const int qx = nn_index(ix), qy = nn_index(iy);
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
    if (v >= 0 && qx >= 0 && qx < W && qy >= 0 && qy < H) {
      const float* q = xyz_map + (((size_t)v * H + qy) * W + qx) * 3;
      q0 = q[0]; q1 = q[1]; q2 = q[2];
    }
    const bool model = p2 > 0.f && dot3f(m0, m0, m1, m1, m2, m2) > 0.f;
    const bool valid = model && q2 >= 0.001f;
    const float e0 = q0 - p0, e1 = q1 - p1, e2 = q2 - p2;
    pair = valid && dot3f(e0, e0, e1, e1, e2, e2) <= md2;
    if (pair) {
      const float* P = poses + (size_t)n * 16;
      const float a0 = p0 - P[3], a1 = p1 - P[7], a2 = p2 - P[11];
      r = dot3f(m0, e0, m1, e1, m2, e2);
      J[0] = a1 * m2 - a2 * m1;
      J[1] = a2 * m0 - a0 * m2;
      J[2] = a0 * m1 - a1 * m0;
      J[3] = m0; J[4] = m1; J[5] = m2;
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long bp = __ballot(pair);
  if (lane == 0) cnt[wave] = __popcll(bp);
  // the 28 float64 terms of this pixel summed over the wave, then over the workgroup's four waves in index order (icp_solve.h)
  wave_sums<kTerms>(J, r, 0.0, bp, lane, red[wave]);
  __syncthreads();
  chunk_sums<kTerms>(red, cnt, partial + ((size_t)n * C + blockIdx.x) * kRow);
}

__global__ __launch_bounds__(64) void k_icp_finish(const double* __restrict__ partial, int C, const float* __restrict__ poses_in,
                                                   double damping, int min_pairs, double* __restrict__ system,
                                                   float* __restrict__ poses_out) {
  __shared__ double sum[kCols];
  const int n = blockIdx.x, lane = threadIdx.x;
  if (lane < kCols) {
    const double* p = partial + (size_t)n * C * kRow + lane;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += p[(size_t)c * kRow];
    sum[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  solve_and_update(sum, sum[kTerms], poses_in + (size_t)n * 16, damping, min_pairs, system + (size_t)n * 40,
                   poses_out ? poses_out + (size_t)n * 16 : nullptr);
}

inline size_t workspace_of(int N, int oh, int ow) { return (size_t)N * (size_t)fp_cdiv(oh * ow, kThreads) * kRow * sizeof(double); }

}  // namespace

extern "C" size_t fp_icp_workspace_bytes(int N, int oh, int ow) {
  if (N <= 0 || oh <= 0 || ow <= 0 || (long long)oh * ow > (1 << 20)) return 0;
  return workspace_of(N, oh, ow);
}

extern "C" int fp_icp_point_plane(const float* xyz_crops, const float* normal_crops, const float* xyz_map, const float* tf_to_crops,
                                  const int32_t* view, int V, int H, int W, const float* poses_in, int N, int oh, int ow, float max_dist,
                                  double damping, int min_pairs, double* system, float* poses_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  FP_REQUIRE(N >= 0 && N <= 65535, "fp_icp_point_plane: N=%d outside 0..65535 (the grid limit; chunk the batch)", N);
  FP_REQUIRE(oh >= 1 && ow >= 1 && H >= 1 && W >= 1 && V >= 1,
             "fp_icp_point_plane: sizes must be >= 1 (oh=%d, ow=%d, H=%d, W=%d, V=%d)", oh, ow, H, W, V);
  FP_REQUIRE((long long)oh * ow <= (1 << 20), "fp_icp_point_plane: crop %dx%d has more than 2^20 pixels", oh, ow);
  FP_REQUIRE(view || V == 1, "fp_icp_point_plane: view is NULL but there are %d views", V);
  FP_REQUIRE(max_dist >= 0.f && __builtin_isfinite(max_dist), "fp_icp_point_plane: max_dist=%g must be finite and >= 0",
             (double)max_dist);
  FP_REQUIRE(damping >= 0.0 && __builtin_isfinite(damping), "fp_icp_point_plane: damping=%g must be finite and >= 0", damping);
  FP_REQUIRE(min_pairs >= 6, "fp_icp_point_plane: min_pairs=%d must be >= 6 (the unknowns of a step)", min_pairs);
  if (N == 0) return FP_OK;
  FP_REQUIRE(xyz_crops && normal_crops && xyz_map && tf_to_crops && poses_in && system, "fp_icp_point_plane: NULL tensor");
  const size_t need = workspace_of(N, oh, ow);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
             "fp_icp_point_plane: workspace too small or not 8-byte aligned (%zu < %zu bytes, see fp_icp_workspace_bytes)",
             workspace_bytes, need);
  if (poses_out) {   // a lane reads its poses_in row after another workgroup may have written poses_out: the two must not share bytes
    const uintptr_t a = (uintptr_t)poses_in, b = (uintptr_t)poses_out, len = (uintptr_t)N * 16 * sizeof(float);
    FP_REQUIRE(a + len <= b || b + len <= a, "fp_icp_point_plane: poses_in and poses_out overlap");
  }
  const hipStream_t st = (hipStream_t)stream;
  const int C = fp_cdiv(oh * ow, kThreads);
  const fp_views vt = {nullptr, view, V};
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_icp_pairs, dim3(C, N), dim3(kThreads), 0, st, xyz_crops, normal_crops, xyz_map, tf_to_crops, vt, H, W, poses_in,
                     oh, ow, max_dist, warp_const(H, W, ow), C, partial);
  FP_CHECK_LAUNCH("fp_icp_point_plane (pairs)");
  hipLaunchKernelGGL(k_icp_finish, dim3(N), dim3(64), 0, st, (const double*)partial, C, poses_in, damping, min_pairs, system, poses_out);
  FP_CHECK_LAUNCH("fp_icp_point_plane (finish)");
  return FP_OK;
}
