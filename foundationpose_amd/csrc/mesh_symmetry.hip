// How far does each of T candidate transforms move a mesh's surface off itself (fp_mesh_transform_residuals; the definition, down to
// the float32 operation, is in include/fp_amd.h): per transform t and surface sample i the squared distance d2(t, i) from the
// transformed sample to the nearest triangle, then per transform the maximum over the samples and the number of samples above each
// of up to four thresholds.  Three launches on the caller's stream, no allocation, no synchronisation, integer atomics only:
//   init, scan   mesh_scan.hip's nearest_dist2_of_pairs.  The (transform, sample) pairs are numbered n = t * Q + i and a lane owns one
//                of them, so a detector's 64 samples fill a workgroup with four transforms instead of leaving three quarters of it
//                idle.  The lane forms its own p' = ((r0*x + r1*y) + r2*z) + t per row and scans the triangles as
//                fp_mesh_point_distance does (one copy, the same bits), but keeps no face: cell[n] = the bits of the smallest dd, by a
//                32-bit atomic minimum (floats >= 0 order as their bits do), or the bits of +inf when no triangle answers.
//   k_ms_finish  one workgroup per transform: the maximum of its Q cells (again on the bits; +inf is the largest of them) and the
//                counts, reduced through LDS with integer atomics; dist2, where asked for, is the cells written out.
// A minimum, a maximum and an integer count commute exactly, so the outputs have one value whatever the chunking and the arrival
// order.  Compiled with -ffp-contract=off (SRCS_EXACT): the numpy restatement (tests/mesh_symmetry_model.py) computes the same bits.
// fp_mesh_grid_transform_residuals is the same call with a grid: the scan then walks the shells of a uniform grid around each p'
// (mesh_grid.h); the cells are the interface, so every output is made by k_ms_finish as above.
#include "mesh_scan.h"

namespace {

constexpr int kThreads = 256;   // lanes of a finish workgroup, striding over a transform's samples
constexpr int kMaxThresholds = 4;

__global__ __launch_bounds__(kThreads) void k_ms_finish(const unsigned* __restrict__ cell, int Q, const float* __restrict__ thr2, int L,
                                                        float* __restrict__ max_d2, int32_t* __restrict__ over,
                                                        float* __restrict__ dist2) {
  __shared__ unsigned s_max;
  __shared__ int s_over[kMaxThresholds];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  if (tid == 0) s_max = 0u;                           // the bits of +0: the maximum over no sample
  if (tid < kMaxThresholds) s_over[tid] = 0;
  float thr[kMaxThresholds];
#pragma unroll
  for (int l = 0; l < kMaxThresholds; ++l) thr[l] = l < L ? thr2[l] : __builtin_inff();   // nothing is above +inf
  __syncthreads();
  unsigned mx = 0u;
  int cnt[kMaxThresholds] = {0, 0, 0, 0};
  for (int i = tid; i < Q; i += kThreads) {
    const unsigned u = cell[(size_t)t * Q + i];
    const float d = __uint_as_float(u);
    mx = u > mx ? u : mx;
#pragma unroll
    for (int l = 0; l < kMaxThresholds; ++l) cnt[l] += d > thr[l] ? 1 : 0;   // strictly: +inf counts; never above a NaN threshold
    if (dist2) dist2[(size_t)t * Q + i] = d;
  }
  if (mx) atomicMax(&s_max, mx);
#pragma unroll
  for (int l = 0; l < kMaxThresholds; ++l)
    if (cnt[l]) atomicAdd(&s_over[l], cnt[l]);
  __syncthreads();
  if (tid == 0) max_d2[t] = __uint_as_float(s_max);
  if (over && tid < L) over[(size_t)t * L + tid] = s_over[tid];
}

// fp_mesh_transform_residuals (gridded: no) and fp_mesh_grid_transform_residuals (gridded: yes) are one call, the scan exchanged
int transform_residuals(const char* name, bool gridded, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                        const float* points, int Q, const float* tfs, int T, const float* thr2, int L, float* max_d2, int32_t* over,
                        float* dist2, void* workspace, size_t workspace_bytes, void* stream) {
  if (int st = mesh_scan::check_pairs(name, T, Q, F, Nv, gridded, grid)) return st;
  FP_REQUIRE(L >= 0 && L <= kMaxThresholds, "%s: L=%d outside 0..%d", name, L, kMaxThresholds);
  if (T == 0) return FP_OK;
  FP_REQUIRE(max_d2, "%s: NULL max_d2", name);
  FP_REQUIRE(L == 0 || (thr2 && over), "%s: NULL thr2 or over with L=%d", name, L);
  FP_REQUIRE(Q == 0 || (points && tfs), "%s: NULL points or tfs", name);
  if (int st = mesh_scan::check_mesh(name, Q > 0, pos, Nv, faces, F)) return st;
  if (int st = mesh_scan::check_workspace(name, workspace, workspace_bytes, fp_mesh_transform_residuals_workspace_bytes(T, Q), 4,
                                          "fp_mesh_transform_residuals_workspace_bytes"))
    return st;
  const hipStream_t st = (hipStream_t)stream;
  unsigned* cell = (unsigned*)workspace;
  if (Q > 0)
    if (int e = mesh_scan::nearest_dist2_of_pairs(name, pos, Nv, faces, F, gridded ? grid : nullptr, points, Q, tfs, T, cell, st)) return e;
  hipLaunchKernelGGL(k_ms_finish, dim3(T), dim3(kThreads), 0, st, cell, Q, thr2, L, max_d2, L > 0 ? over : nullptr, Q > 0 ? dist2 : nullptr);
  return mesh_scan::launched(name, "finish");
}

}  // namespace

extern "C" size_t fp_mesh_transform_residuals_workspace_bytes(int T, int Q) {
  return T > 0 && Q > 0 ? (size_t)T * (size_t)Q * sizeof(unsigned) : 0;
}

extern "C" int fp_mesh_transform_residuals(const float* pos, int Nv, const int32_t* faces, int F, const float* points, int Q,
                                           const float* tfs, int T, const float* thr2, int L, float* max_d2, int32_t* over,
                                           float* dist2, void* workspace, size_t workspace_bytes, void* stream) {
  return transform_residuals("fp_mesh_transform_residuals", false, pos, Nv, faces, F, nullptr, points, Q, tfs, T, thr2, L, max_d2, over,
                             dist2, workspace, workspace_bytes, stream);
}

extern "C" int fp_mesh_grid_transform_residuals(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                                                const float* points, int Q, const float* tfs, int T, const float* thr2, int L,
                                                float* max_d2, int32_t* over, float* dist2, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  return transform_residuals("fp_mesh_grid_transform_residuals", true, pos, Nv, faces, F, grid, points, Q, tfs, T, thr2, L, max_d2, over,
                             dist2, workspace, workspace_bytes, stream);
}
