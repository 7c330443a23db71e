// What one Gauss-Newton step of point-to-plane ICP is made of once the float32 Jacobian row J and residual r of every pair exist: the
// one copy that icp.hip (fp_icp_point_plane) and mesh_icp.hip (fp_mesh_icp_step) share.  The definition, down to the operation, is in
// include/fp_amd.h; both files are compiled with -ffp-contract=off (SRCS_EXACT), so the operations written here are the ones executed
// and the two entry points sum, solve and update with the same bits for the same terms.
//   wave_sums      the 28 float64 products of a lane's (J, r), and one further float64 term of the caller's, summed over the wave
//                  by the xor tree (run transposed) into one LDS row per wave
//   chunk_sums     the workgroup's waves added in index order into one row of the partial table, with the pair count
//   solve_and_update  the damped LDL^T solve, the status and the Rodrigues update of one float32 transform, by one lane
#pragma once
#include "fp_common.h"

namespace icp_solve {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTerms = 28;             // 21 of A's upper triangle, 6 of b, r*r
constexpr int kTree = 32;              // terms a wave tree carries (kTerms padded: the caller's extra term is number 28)
constexpr int kRow = 32;               // doubles per partial row (a row is 256 bytes)

__device__ __forceinline__ float dot3f(float a0, float b0, float a1, float b1, float a2, float b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}
__device__ __forceinline__ double dot3d(double a0, double b0, double a1, double b1, double a2, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// A's upper triangle, row-major: entry (i, j), i <= j
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// The 28 float64 terms of this lane (all +0 without a pair) in the order of system[n]: A's upper triangle row-major (a, b < 6), then
// b (J_a * r), then r * r; term 28 is `extra` (a further float64 term of the caller's, +0 where there is none); padded to 32.  Every
// term is summed over the wave by the xor tree s += s of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  The 32 trees run transposed: at the
// level of lane bit o a lane keeps the half of its terms that its bit selects and trades the other half with lane ^ o, so each level
// moves half as many values as the one before (31 exchanges and one last full one, instead of 6 x 28).  Each kept sum is own +
// partner's, the additions of the plain tree: the same bits.  After the five halving levels lane l holds term (l >> 1) (its bits
// reversed, below) summed over the lanes of its parity; the level of bit 0 completes it.  A wave without a pair (`any` == 0,
// wave-uniform) skips the tree: its sums are the +0 the tree would give.  The first kStore terms go to red[0..kStore-1].  Every lane
// of the wave must call this (it shuffles).
template <int kStore>
__device__ __forceinline__ void wave_sums(const float (&J)[6], float r, double extra, unsigned long long any, int lane,
                                          double* __restrict__ red) {
  static_assert(kStore >= kTerms && kStore <= kTree, "the tree carries 32 terms");
  if (any != 0ull) {   // wave-uniform
    double v[kTree];
#pragma unroll
    for (int a = 0; a < 7; ++a) {
#pragma unroll
      for (int b = a; b < 7; ++b)
        v[b < 6 ? tri(a, b) : (a < 6 ? 21 + a : 27)] = (double)(a < 6 ? J[a] : r) * (double)(b < 6 ? J[b] : r);
    }
    v[kTerms] = extra;
#pragma unroll
    for (int i = kTerms + 1; i < kTree; ++i) v[i] = 0.0;
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
    if (!(lane & 1) && col < kStore) red[col] = s;
  } else if (lane < kStore) {
    red[lane] = 0.0;
  }
}

// After a barrier: the waves' rows added in index order, and the waves' pair counts, into one row of the partial table: o[0..kStore-1]
// the sums, o[kStore] the count.  Threads 0..kStore of the workgroup write.
template <int kStore>
__device__ __forceinline__ void chunk_sums(const double (*red)[kStore], const int* cnt, double* __restrict__ o) {
  if (threadIdx.x < kStore) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += red[w][threadIdx.x];
    o[threadIdx.x] = s;
  } else if (threadIdx.x == kStore) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += cnt[w];
    o[kStore] = (double)s;
  }
}

// One lane: the step of the transform Pin (16 float32, row-major 4x4) from its 28 sums and pair count -> the row o of `system`
// (40 float64: the sums, pairs, status, x, four zeros) and, where asked for, the updated transform Pout.
__device__ __forceinline__ void solve_and_update(const double* sum, double pairs, const float* __restrict__ Pin, double damping,
                                                 int min_pairs, double* __restrict__ o, float* __restrict__ Pout) {
  bool pose_ok = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) pose_ok = pose_ok && __builtin_isfinite(Pin[i]);
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
#pragma unroll
  for (int i = 0; i < kTerms; ++i) o[i] = sum[i];
  o[28] = pairs;
  o[29] = (double)status;
#pragma unroll
  for (int i = 0; i < 6; ++i) o[30 + i] = x[i];
#pragma unroll
  for (int i = 36; i < 40; ++i) o[i] = 0.0;
  if (!Pout) return;
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

}  // namespace icp_solve
