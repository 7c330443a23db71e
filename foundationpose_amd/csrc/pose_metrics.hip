// Pose-error metrics on the device: ADD, ADD-S and their symmetry-aware forms (BOP's minimum over the symmetry set of the mean and of
// the maximum = MSSD) for N poses against their ground truths in one call (fp_pose_errors; the definition is in include/fp_amd.h).
// Three launches on the caller's stream, no atomics, no allocation, no synchronisation:
//   k_pose_tf      one lane per (pose n, transform y): T = inv(pose_n) * gt_g (y = 0) or T * S_{y-1} (y >= 1) in float64, rounded to
//                  float32 into the workspace
//   k_point_errors grid (workgroup of kQ chunks of 256 model points, y, n): a lane owns kQ query points q_j = T_y p_j in registers.
//                  y = 0 gives ADD's d_j and, for ADD-S, runs the queries against every model point: the targets stream through LDS
//                  in tiles of 16-byte points and every lane reads the same address (a broadcast, no bank conflict), so one LDS read
//                  (ds_read_b96: the slot's fourth word is unused) feeds 64 lanes x kQ queries.  A pair is 9 floating-point
//                  operations, compiled to 8.5 VALU instructions (v_min3_f32 takes two candidates); with the reads and the loop
//                  about 9.5 (kQ = 2) to 10 (kQ = 1) instructions.  y >= 1 gives d_j under symmetry y-1.  Each chunk's
//                  float64 sums (and float32 maximum) go to partial[n][y][chunk] in the workspace.
//   k_pose_finish  one wave per pose: adds the partials of a transform in index order, takes the minima over the symmetries, writes
//                  the row (NaN for a column that was not asked for or a ground-truth index out of range).
// A chunk is 256 consecutive points summed in one fixed order, and the chunks are added in index order: the order of every sum depends
// on P alone, so row n of a batch has the bits of the call on pose n alone, and every replay has the bits of the first run.  Compiled
// with -ffp-contract=off (SRCS_EXACT): the float32 per-point values are the ones the numpy restatement (tests/pose_errors_model.py)
// computes, bit for bit.
// fp_mspd (BOP's maximum symmetry-aware projection distance, in pixels) is the small sibling of the mssd column: one workgroup per pose,
// a float32 maximum per symmetry and the minimum over them, exact in any order (k_mspd below; restated in tests/bop_errors_model.py).
#include "fp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 1024;            // target points per LDS tile (16 KiB)
constexpr int kFillWorkgroups = 512;   // workgroups that fill the chip (256 CUs x 2)
constexpr int kBatch = 8;              // targets read from the LDS ahead of their use (kTile is a multiple)
constexpr int kFlagsAll = FP_ERR_ADD | FP_ERR_ADDS | FP_ERR_SYM;

// Queries per lane (kQ).  One broadcast LDS read per target costs the CU's LDS about 4 cycles and a SIMD 8.5 VALU instructions x 2
// cycles per query: with one query per lane four SIMDs ask for 16 LDS cycles in every 17, so two queries per lane run faster -- once there
// are workgroups enough to fill the chip.  Measured: 252 poses x 2 501 points 0.41 ms with one, 0.28 with two,
// 0.36 with four; one pose x 2 501 points 0.074 with one, 0.11 with two.  The partial sums are per chunk of kThreads points whatever
// kQ is, so the choice never changes a bit of the result.
inline int queries_per_lane(int N, int P) { return (long long)N * fp_cdiv(P, kThreads) >= 2 * kFillWorkgroups ? 2 : 1; }

// workspace: partial[N][1+S][C][2] float64 with C = ceil(P / kThreads), then tf[N][1+S][12] float32
struct Layout {
  size_t partial_bytes, total;
  int C;
};
inline Layout layout_of(int N, int P, int S) {
  Layout L;
  L.C = fp_cdiv(P, kThreads);
  L.partial_bytes = (size_t)N * (size_t)(1 + S) * (size_t)L.C * 2 * sizeof(double);
  L.total = L.partial_bytes + (size_t)N * (size_t)(1 + S) * 12 * sizeof(float);
  return L;
}

// ground truth of pose n, or -1 (an index outside 0..G-1: the row reads nothing and is NaN)
__device__ __forceinline__ int gt_of(const int32_t* gt_index, int G, int n) {
  const int g = gt_index ? gt_index[n] : (G == 1 ? 0 : n);
  return (unsigned)g < (unsigned)G ? g : -1;
}

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

__global__ __launch_bounds__(kThreads) void k_pose_tf(const float* __restrict__ poses, const double* __restrict__ gt,
                                                      const int32_t* __restrict__ gt_index, const double* __restrict__ sym, int G,
                                                      int N, int S, float* __restrict__ tf) {
  const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (long long)N * (1 + S)) return;
  const int n = (int)(id / (1 + S)), y = (int)(id - (long long)n * (1 + S));
  const int g = gt_of(gt_index, G, n);
  if (g < 0) return;
  const float* A = poses + (size_t)n * 16;
  const double* B = gt + (size_t)g * 16;
  double R[3][3], t[3];
  const double d0 = B[3] - (double)A[3], d1 = B[7] - (double)A[7], d2 = B[11] - (double)A[11];
#pragma unroll
  for (int i = 0; i < 3; ++i) {   // inv(pose) = [R^T | -R^T t]:  T = [R_p^T R_g | R_p^T (t_g - t_p)]
    const double a0 = (double)A[i], a1 = (double)A[4 + i], a2 = (double)A[8 + i];
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = dot3(a0, B[j], a1, B[4 + j], a2, B[8 + j]);
    t[i] = dot3(a0, d0, a1, d1, a2, d2);
  }
  float* o = tf + (size_t)id * 12;
  if (y == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      o[i * 4 + 0] = (float)R[i][0]; o[i * 4 + 1] = (float)R[i][1]; o[i * 4 + 2] = (float)R[i][2]; o[i * 4 + 3] = (float)t[i];
    }
  } else {   // T_s = T * S_s = [R S_R | R S_t + t]
    const double* Sm = sym + (size_t)(y - 1) * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) o[i * 4 + j] = (float)dot3(R[i][0], Sm[j], R[i][1], Sm[4 + j], R[i][2], Sm[8 + j]);
      o[i * 4 + 3] = (float)(dot3(R[i][0], Sm[3], R[i][1], Sm[7], R[i][2], Sm[11]) + t[i]);
    }
  }
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

template <int kQ>
__global__ __launch_bounds__(kThreads) void k_point_errors(const float* __restrict__ pts, int P, const int32_t* __restrict__ gt_index,
                                                           int G, int S, int C, int flags, const float* __restrict__ tf,
                                                           double* __restrict__ partial) {
  __shared__ float4 tile[kTile];
  __shared__ double red[kQ][kWaves][2];
  const int c = blockIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (gt_of(gt_index, G, n) < 0) return;                     // uniform: the whole workgroup leaves
  if (y == 0 && !(flags & (FP_ERR_ADD | FP_ERR_ADDS))) return;
  const float* T = tf + ((size_t)n * (1 + S) + y) * 12;
  float qx[kQ], qy[kQ], qz[kQ], d[kQ], e[kQ];
  bool live[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int j = (c * kQ + k) * kThreads + threadIdx.x;
    live[k] = j < P;
    const int jj = live[k] ? j : P - 1;
    const float x = pts[(size_t)jj * 3], yv = pts[(size_t)jj * 3 + 1], z = pts[(size_t)jj * 3 + 2];
    qx[k] = ((T[0] * x + T[1] * yv) + T[2] * z) + T[3];
    qy[k] = ((T[4] * x + T[5] * yv) + T[6] * z) + T[7];
    qz[k] = ((T[8] * x + T[9] * yv) + T[10] * z) + T[11];
    d[k] = sqrtf(dist2(qx[k], qy[k], qz[k], x, yv, z));
    e[k] = 0.f;
  }
  if (y == 0 && (flags & FP_ERR_ADDS)) {
    float best[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) best[k] = __builtin_inff();
    for (int base = 0; base < P; base += kTile) {
      const int cnt = min(kTile, P - base);
      __syncthreads();                                       // the previous tile has been read by every wave
      const int cnt8 = (cnt + kBatch - 1) & ~(kBatch - 1);   // padded with copies of the tile's last point: the minimum is the same
      for (int i = threadIdx.x; i < cnt8; i += kThreads) {
        const float* p = pts + (size_t)(base + min(i, cnt - 1)) * 3;
        tile[i] = make_float4(p[0], p[1], p[2], 0.f);
      }
      __syncthreads();
      // kBatch targets are read before the first is used, so a wave waits for the LDS once per batch.  (Written as batches because
      // the loop vectoriser would pair two targets into packed-fp32 instructions, which this library is built without: Makefile.)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
      for (int i = 0; i < cnt8; i += kBatch) {
        float4 p[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) p[b] = tile[i + b];
#pragma unroll
        for (int b = 0; b < kBatch; ++b)
#pragma unroll
          for (int k = 0; k < kQ; ++k) best[k] = fminf(best[k], dist2(qx[k], qy[k], qz[k], p[b].x, p[b].y, p[b].z));
      }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) e[k] = sqrtf(best[k]);
  }
  // One partial per chunk of kThreads points, summed in a fixed order (xor tree in the wave, then the waves in index order), whatever
  // kQ is: chunk c * kQ + k is this workgroup's query k.  A lane beyond P adds +0.
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    double a = live[k] ? (double)d[k] : 0.0, b = live[k] ? (double)e[k] : 0.0;
    float m = live[k] ? d[k] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
      m = fmaxf(m, __shfl_xor(m, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[k][wave][0] = a; red[k][wave][1] = y == 0 ? b : (double)m; }
  }
  __syncthreads();
  const int chunk = c * kQ + threadIdx.x;
  if (threadIdx.x < kQ && chunk < C) {
    double a = red[threadIdx.x][0][0], b = red[threadIdx.x][0][1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      a += red[threadIdx.x][w][0];
      b = y == 0 ? b + red[threadIdx.x][w][1] : fmax(b, red[threadIdx.x][w][1]);
    }
    double* o = partial + (((size_t)n * (1 + S) + y) * C + chunk) * 2;
    o[0] = a;
    o[1] = b;
  }
}

// a transform with a NaN or an infinity (a non-finite pose, ground truth or symmetry, or one beyond float32): its columns are NaN --
// the minima and maxima of the reductions would drop a NaN and report +inf or 0, which reads as a number
__device__ __forceinline__ bool tf_finite(const float* T) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && __builtin_isfinite(T[i]);
  return ok;
}

__global__ __launch_bounds__(64) void k_pose_finish(const double* __restrict__ partial, const float* __restrict__ tf,
                                                    const int32_t* __restrict__ gt_index, int G, int P, int S, int C, int flags,
                                                    double* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const double nan = __builtin_nan("");
  double add = nan, adds = nan, add_sym = nan, mssd = nan;
  const float* T0 = tf + (size_t)n * (1 + S) * 12;
  if (gt_of(gt_index, G, n) >= 0 && tf_finite(T0)) {
    const double* base = partial + (size_t)n * (1 + S) * C * 2;
    if (lane == 0 && (flags & (FP_ERR_ADD | FP_ERR_ADDS))) {
      double a = 0.0, b = 0.0;
      for (int c = 0; c < C; ++c) { a += base[c * 2]; b += base[c * 2 + 1]; }
      if (flags & FP_ERR_ADD) add = a / (double)P;
      if (flags & FP_ERR_ADDS) adds = b / (double)P;
    }
    if (flags & FP_ERR_SYM) {
      double best_mean = __builtin_inf(), best_max = __builtin_inf();
      bool finite = true;
      for (int s = lane; s < S; s += 64) {
        finite = finite && tf_finite(T0 + (size_t)(1 + s) * 12);
        const double* ps = base + (size_t)(1 + s) * C * 2;
        double a = 0.0, m = 0.0;
        for (int c = 0; c < C; ++c) { a += ps[c * 2]; m = fmax(m, ps[c * 2 + 1]); }
        best_mean = fmin(best_mean, a / (double)P);
        best_max = fmin(best_max, m);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        best_mean = fmin(best_mean, __shfl_xor(best_mean, o, 64));
        best_max = fmin(best_max, __shfl_xor(best_max, o, 64));
      }
      if (__ballot(!finite) == 0ull) {
        add_sym = best_mean;
        mssd = best_max;
      }
    }
  }
  if (lane == 0) {
    double* o = out + (size_t)n * 4;
    o[0] = add; o[1] = adds; o[2] = add_sym; o[3] = mssd;
  }
}

// fp_mspd: one workgroup per pose.  Per symmetry s the first 12 lanes form M_s = gt_g * S_s in float64 and leave it in LDS as float32;
// every lane then projects its points (a stride of kThreads apart) under the pose and under M_s and keeps the float32 maximum of the
// pixel distances; the workgroup's maximum (exact in any order) goes into the minimum over s.  `bad` collects what makes the row NaN.
struct fp_k4 { float fx, fy, cx, cy; };

__device__ __forceinline__ void project(const float* T, float x, float y, float z, const fp_k4& K, float& u, float& v, bool& bad) {
  const float X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  const float Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  const float Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
  bad = bad || !(Z > 0.f);
  u = (K.fx * X) / Z + K.cx;
  v = (K.fy * Y) / Z + K.cy;
}

__global__ __launch_bounds__(kThreads) void k_mspd(const float* __restrict__ pts, int P, const double* __restrict__ sym, int S,
                                                   const float* __restrict__ poses, const double* __restrict__ gt,
                                                   const int32_t* __restrict__ gt_index, int G, fp_k4 K, double* __restrict__ out) {
  __shared__ float M[12];
  __shared__ float red[kWaves];
  __shared__ int red_bad[kWaves];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int g = gt_of(gt_index, G, n);
  if (g < 0) {                                              // uniform
    if (tid == 0) out[n] = __builtin_nan("");
    return;
  }
  float A[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) A[i] = poses[(size_t)n * 16 + i];
  bool bad = !tf_finite(A);
  const double* B = gt + (size_t)g * 16;
  float best = __builtin_inff();
  const int Y = S > 0 ? S : 1;
  for (int s = 0; s < Y; ++s) {
    __syncthreads();                                        // the previous M has been read by every wave
    if (tid < 12) {
      const int i = tid >> 2, j = tid & 3;
      double v = B[tid];
      if (S > 0) {
        const double* Sm = sym + (size_t)s * 16;
        v = dot3(B[i * 4], Sm[j], B[i * 4 + 1], Sm[4 + j], B[i * 4 + 2], Sm[8 + j]);
        if (j == 3) v += B[i * 4 + 3];
      }
      M[tid] = (float)v;
    }
    __syncthreads();
    bad = bad || !tf_finite(M);
    float m = 0.f;
    for (int p = tid; p < P; p += kThreads) {
      const float x = pts[(size_t)p * 3], y = pts[(size_t)p * 3 + 1], z = pts[(size_t)p * 3 + 2];
      float ua, va, ub, vb;
      project(A, x, y, z, K, ua, va, bad);
      project(M, x, y, z, K, ub, vb, bad);
      const float du = ua - ub, dv = va - vb;
      m = fmaxf(m, sqrtf(du * du + dv * dv));               // (a NaN distance is dropped here; everything that makes one sets `bad`)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) m = w == 0 ? red[0] : fmaxf(m, red[w]);
    best = fminf(best, m);
  }
  const bool wave_bad = __ballot(bad) != 0ull;
  __syncthreads();
  if ((tid & 63) == 0) red_bad[tid >> 6] = wave_bad;
  __syncthreads();
  if (tid == 0) {
    bool any_bad = false;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) any_bad = any_bad || red_bad[w] != 0;
    out[n] = any_bad ? __builtin_nan("") : (double)best;
  }
}

}  // namespace

extern "C" size_t fp_pose_errors_workspace_bytes(int N, int P, int S) {
  if (N <= 0 || P <= 0 || S < 0) return 0;
  return layout_of(N, P, S).total;
}

extern "C" int fp_pose_errors(const float* model_pts, int P, const double* sym_tfs, int S, const float* poses, const double* gt,
                              const int32_t* gt_index, int G, int N, int flags, double* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  FP_REQUIRE(N >= 0 && N <= 65535, "fp_pose_errors: N=%d outside 0..65535 (the grid limit; chunk the batch)", N);
  FP_REQUIRE(P >= 1 && P <= (1 << 22), "fp_pose_errors: P=%d outside 1..2^22", P);
  FP_REQUIRE(G >= 1, "fp_pose_errors: G=%d must be >= 1", G);
  FP_REQUIRE(S >= 0 && S <= 4096, "fp_pose_errors: S=%d outside 0..4096", S);
  FP_REQUIRE(flags != 0 && !(flags & ~kFlagsAll), "fp_pose_errors: flags=0x%x must be a non-empty set of FP_ERR_ADD | ADDS | SYM", flags);
  FP_REQUIRE(S == 0 || sym_tfs, "fp_pose_errors: sym_tfs is NULL but S=%d", S);
  FP_REQUIRE(!(flags & FP_ERR_SYM) || S >= 1, "fp_pose_errors: FP_ERR_SYM needs a symmetry set (S=0)");
  FP_REQUIRE(gt_index || G == 1 || G == N, "fp_pose_errors: gt_index is NULL but G=%d is neither 1 nor N=%d", G, N);
  if (N == 0) return FP_OK;
  FP_REQUIRE(model_pts && poses && gt && out, "fp_pose_errors: NULL tensor");
  const Layout L = layout_of(N, P, S);
  FP_REQUIRE(workspace && workspace_bytes >= L.total && ((uintptr_t)workspace & 7) == 0,
             "fp_pose_errors: workspace too small or not 8-byte aligned (%zu < %zu bytes, see fp_pose_errors_workspace_bytes)",
             workspace_bytes, L.total);
  const hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  float* tf = (float*)((char*)workspace + L.partial_bytes);
  const int Y = (flags & FP_ERR_SYM) ? 1 + S : 1;            // transforms the point kernel visits; the tables keep the 1+S stride
  const long long ntf = (long long)N * (1 + S);
  hipLaunchKernelGGL(k_pose_tf, dim3((unsigned)((ntf + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, poses, gt, gt_index, sym_tfs,
                     G, N, S, tf);
  FP_CHECK_LAUNCH("fp_pose_errors (transforms)");
  const int q = queries_per_lane(N, P);
  const dim3 grid(fp_cdiv(L.C, q), Y, N);
  if (q == 2)
    hipLaunchKernelGGL(k_point_errors<2>, grid, dim3(kThreads), 0, st, model_pts, P, gt_index, G, S, L.C, flags, tf, partial);
  else
    hipLaunchKernelGGL(k_point_errors<1>, grid, dim3(kThreads), 0, st, model_pts, P, gt_index, G, S, L.C, flags, tf, partial);
  FP_CHECK_LAUNCH("fp_pose_errors (points)");
  hipLaunchKernelGGL(k_pose_finish, dim3(N), dim3(64), 0, st, partial, tf, gt_index, G, P, S, L.C, flags, out);
  FP_CHECK_LAUNCH("fp_pose_errors (finish)");
  return FP_OK;
}

extern "C" int fp_mspd(const float* model_pts, int P, const double* sym_tfs, int S, const float* poses, const double* gt,
                       const int32_t* gt_index, int G, int N, const float* K, double* out, void* stream) {
  FP_REQUIRE(N >= 0 && N <= (1 << 20), "fp_mspd: N=%d outside 0..2^20", N);
  FP_REQUIRE(P >= 1 && P <= (1 << 22), "fp_mspd: P=%d outside 1..2^22", P);
  FP_REQUIRE(G >= 1, "fp_mspd: G=%d must be >= 1", G);
  FP_REQUIRE(S >= 0 && S <= 4096, "fp_mspd: S=%d outside 0..4096", S);
  FP_REQUIRE(S == 0 || sym_tfs, "fp_mspd: sym_tfs is NULL but S=%d", S);
  FP_REQUIRE(K, "fp_mspd: NULL K");
  FP_REQUIRE(K[1] == 0.f, "fp_mspd: K has a skew of %g; the projection is defined without one", (double)K[1]);
  FP_REQUIRE(gt_index || G == 1 || G == N, "fp_mspd: gt_index is NULL but G=%d is neither 1 nor N=%d", G, N);
  if (N == 0) return FP_OK;
  FP_REQUIRE(model_pts && poses && gt && out, "fp_mspd: NULL tensor");
  const fp_k4 k4{K[0], K[4], K[2], K[5]};
  hipLaunchKernelGGL(k_mspd, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, model_pts, P, sym_tfs, S, poses, gt, gt_index, G, k4, out);
  FP_CHECK_LAUNCH("fp_mspd");
  return FP_OK;
}
