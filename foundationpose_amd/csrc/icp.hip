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

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTerms = 28;             // 21 of A's upper triangle, 6 of b, r*r
constexpr int kCols = kTerms + 1;      // + the pair count
constexpr int kRow = 32;               // doubles per partial row (kCols padded: a row is 256 bytes)

__device__ __forceinline__ float dot3f(float a0, float b0, float a1, float b1, float a2, float b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}
__device__ __forceinline__ double dot3d(double a0, double b0, double a1, double b1, double a2, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// A's upper triangle, row-major: entry (i, j), i <= j
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

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
  // The 28 float64 terms of this pixel (all +0 without a pair) in the order of system[n]: A's upper triangle row-major (a, b < 6), then
  // b (J_a * r), then r * r; padded to 32.  Every term is summed over the wave by the xor tree s += s of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2,
  // ^ 1.  The 32 trees run transposed: at the level of lane bit o a lane keeps the half of its terms that its bit selects and trades
  // the other half with lane ^ o, so each level moves half as many values as the one before (31 exchanges and one last full one,
  // instead of 6 x 28).  Each kept sum is own + partner's, the additions of the plain tree: the same bits.  After the five halving
  // levels lane l holds term (l >> 1) (its bits reversed, below) summed over the lanes of its parity; the level of bit 0 completes it.
  // A wave without a pair (most of a crop is background) skips the tree: its sums are the +0 the tree would give.
  if (bp != 0ull) {   // wave-uniform
    double v[32];
#pragma unroll
    for (int a = 0; a < 7; ++a) {
#pragma unroll
      for (int b = a; b < 7; ++b)
        v[b < 6 ? tri(a, b) : (a < 6 ? 21 + a : 27)] = (double)(a < 6 ? J[a] : r) * (double)(b < 6 ? J[b] : r);
    }
#pragma unroll
    for (int i = kTerms; i < 32; ++i) v[i] = 0.0;
#pragma unroll
    for (int o = 32, h = 16; o > 1; o >>= 1, h >>= 1) {
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int i = 0; i < h; ++i) {
        const double keep = up ? v[i + h] : v[i], send = up ? v[i] : v[i + h];
        v[i] = keep + __shfl_xor(send, o, 64);
      }
    }
    const double s = v[0] + __shfl_xor(v[0], 1, 64);
    // the term this lane ends with: bit 5 of the lane chose the upper 16, bit 4 the upper 8 of those, ..., bit 1 the upper one of two
    const int col = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
    if (!(lane & 1) && col < kTerms) red[wave][col] = s;
  } else if (lane < kTerms) {
    red[wave][lane] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kCols) {
    double* o = partial + ((size_t)n * C + blockIdx.x) * kRow;
    if (threadIdx.x < kTerms) {
      double s = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += red[w][threadIdx.x];
      o[threadIdx.x] = s;
    } else {
      int s = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) s += cnt[w];
      o[kTerms] = (double)s;
    }
  }
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
  const float* Pin = poses_in + (size_t)n * 16;
  bool pose_ok = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) pose_ok = pose_ok && __builtin_isfinite(Pin[i]);
  const double pairs = sum[kTerms];
  int status = !pose_ok ? 2 : (pairs < (double)min_pairs ? 1 : 0);
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (status == 0) {
    // A_lambda = A + damping * diag(A); LDL^T without pivoting, column by column (the order is written out in include/fp_amd.h)
    double L[6][6], d[6], vk[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = sum[tri(j, j)] + damping * sum[tri(j, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) {
        vk[k] = L[j][k] * d[k];
        s = s - L[j][k] * vk[k];
      }
      d[j] = s;
      ok = ok && s > 0.0 && __builtin_isfinite(s);
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double u = sum[tri(j, i)];
#pragma unroll
        for (int k = 0; k < j; ++k) u = u - L[i][k] * vk[k];
        L[i][j] = u / s;
      }
    }
    if (ok) {
      double y[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double u = sum[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) u = u - L[i][k] * y[k];
        y[i] = u;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double u = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) u = u - L[k][i] * x[k];
        x[i] = u;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) ok = ok && __builtin_isfinite(x[i]);
    }
    if (!ok) {
      status = 2;
#pragma unroll
      for (int i = 0; i < 6; ++i) x[i] = 0.0;
    }
  }
  double* o = system + (size_t)n * 40;
#pragma unroll
  for (int i = 0; i < kTerms; ++i) o[i] = sum[i];
  o[28] = pairs;
  o[29] = (double)status;
#pragma unroll
  for (int i = 0; i < 6; ++i) o[30 + i] = x[i];
#pragma unroll
  for (int i = 36; i < 40; ++i) o[i] = 0.0;
  if (!poses_out) return;
  float* Pout = poses_out + (size_t)n * 16;
  if (status != 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) Pout[i] = Pin[i];
    return;
  }
  // dR = cos I + sin [k]x + (1 - cos) k k^T with k = w / theta (Rodrigues); I + [w]x below theta = 1e-12
  const double w0 = x[0], w1 = x[1], w2 = x[2];
  const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  double dR[3][3];
  if (th < 1e-12) {
    dR[0][0] = 1.0; dR[0][1] = -w2; dR[0][2] = w1;
    dR[1][0] = w2;  dR[1][1] = 1.0; dR[1][2] = -w0;
    dR[2][0] = -w1; dR[2][1] = w0;  dR[2][2] = 1.0;
  } else {
    const double k0 = w0 / th, k1 = w1 / th, k2 = w2 / th, c = cos(th), s = sin(th), c1 = 1.0 - c;
    dR[0][0] = c + c1 * (k0 * k0);       dR[0][1] = c1 * (k0 * k1) - s * k2;  dR[0][2] = c1 * (k0 * k2) + s * k1;
    dR[1][0] = c1 * (k0 * k1) + s * k2;  dR[1][1] = c + c1 * (k1 * k1);       dR[1][2] = c1 * (k1 * k2) - s * k0;
    dR[2][0] = c1 * (k0 * k2) - s * k1;  dR[2][1] = c1 * (k1 * k2) + s * k0;  dR[2][2] = c + c1 * (k2 * k2);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Pout[i * 4 + j] = (float)dot3d(dR[i][0], (double)Pin[j], dR[i][1], (double)Pin[4 + j], dR[i][2], (double)Pin[8 + j]);
    Pout[i * 4 + 3] = (float)((double)Pin[i * 4 + 3] + x[3 + i]);
  }
#pragma unroll
  for (int i = 12; i < 16; ++i) Pout[i] = Pin[i];
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
