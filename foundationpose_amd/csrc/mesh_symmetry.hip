// How far does each of T candidate transforms move a mesh's surface off itself (fp_mesh_transform_residuals; the definition, down to
// the float32 operation, is in include/fp_amd.h): per transform t and surface sample i the squared distance d2(t, i) from the
// transformed sample to the nearest triangle, then per transform the maximum over the samples and the number of samples above each
// of up to four thresholds.  Three launches on the caller's stream, no allocation, no synchronisation, integer atomics only:
//   k_ms_init    cell[t * Q + i] = the bits of +inf ("no triangle answered yet")
//   k_ms_scan    grid (tile of kThreads (transform, sample) pairs, chunk of faces).  The pairs are numbered n = t * Q + i and a lane owns
//                one of them, so a detector's 64 samples fill a workgroup with four transforms instead of leaving three quarters of it
//                idle.  The lane forms its own p' = ((r0*x + r1*y) + r2*z) + t per row and keeps it in registers; the chunk's
//                triangles pass through LDS in tiles of kTile and are read by broadcast, with mesh_distance.hip's own staging and
//                closest-point walk (mesh_closest.h: one copy, the same bits).  The lane keeps the smallest dd of its chunk and
//                merges it into cell[n] with one 32-bit atomic minimum on its bits: floats >= 0 order as their bits do.
//   k_ms_finish  one workgroup per transform: the maximum of its Q cells (again on the bits; +inf is the largest of them) and the
//                counts, reduced through LDS with integer atomics; dist2, where asked for, is the cells written out.
// A minimum, a maximum and an integer count commute exactly, so the outputs have one value whatever the chunking and the arrival
// order.  Compiled with -ffp-contract=off (SRCS_EXACT): the numpy restatement (tests/mesh_symmetry_model.py) computes the same bits.
#include "fp_common.h"
#include "mesh_closest.h"

namespace {

using namespace mesh_closest;

constexpr int kThreads = 256;          // (transform, sample) pairs per workgroup, one per lane
constexpr int kTile = 256;             // triangles per LDS tile: 4 float4 each, 16 KiB -- as k_md_scan: 8 workgroups of 4 waves a CU
constexpr int kChunkMin = 1024;        // the fewest faces a workgroup scans (unless the mesh has fewer)
constexpr int kFillWorkgroups = 2048;  // workgroups wanted in flight (256 CUs x 8 of 4 waves)
constexpr int kMaxThresholds = 4;
constexpr unsigned kInfBits = 0x7f800000u;

static_assert(kChunkMin % kTile == 0, "a chunk is whole tiles");
static_assert(kTile == kThreads, "a tile is staged by one pass of the workgroup");

__global__ __launch_bounds__(kThreads) void k_ms_init(unsigned* __restrict__ cell, int n_pairs) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n < n_pairs) cell[n] = kInfBits;
}

__global__ __launch_bounds__(kThreads) void k_ms_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                      const float* __restrict__ points, int Q, const float* __restrict__ tfs,
                                                      int n_pairs, int chunk, unsigned* __restrict__ cell) {
  __shared__ float4 tile[kTile * kTileFloat4];
  const int tid = threadIdx.x;
  const int n = blockIdx.x * kThreads + tid;          // n_pairs <= 2^30: no overflow
  const bool live = n < n_pairs;
  const int nn = live ? n : n_pairs - 1;
  const int t = nn / Q, i = nn - t * Q;
  const v3 x = load3(points + (size_t)i * 3);
  const float* __restrict__ m = tfs + (size_t)t * 16;
  // rows 0..2 of the matrix as given; ((r0*x + r1*y) + r2*z) + t, one float32 operation each, in this order
  const v3 p{((m[0] * x.x + m[1] * x.y) + m[2] * x.z) + m[3], ((m[4] * x.x + m[5] * x.y) + m[6] * x.z) + m[7],
             ((m[8] * x.x + m[9] * x.y) + m[10] * x.z) + m[11]};
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  for (int base = f0; base < f1; base += kTile) {
    const int cnt = min(kTile, f1 - base);
    __syncthreads();                                  // the previous tile has been read by every wave
    if (tid < cnt) stage_triangle(tile, tid, pos, Nv, faces, base + tid);
    __syncthreads();
    // (the loop vectoriser would pair two triangles into packed-fp32 instructions, which this library is built without: Makefile)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(2)
    for (int k = 0; k < cnt; ++k) {
      const float dd = staged_distance2(p, tile, k);
      // dd < best holds for no NaN and no +inf (best starts at +inf): exactly the candidates with dd <= FLT_MAX that improve
      best = dd < best ? dd : best;
    }
  }
  // best >= 0 (a sum of squares), never NaN; -0 cannot arise from (x*x + y*y) + z*z
  if (live && best < __builtin_inff()) __hip_atomic_fetch_min(cell + n, __float_as_uint(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

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

}  // namespace

extern "C" size_t fp_mesh_transform_residuals_workspace_bytes(int T, int Q) {
  return T > 0 && Q > 0 ? (size_t)T * (size_t)Q * sizeof(unsigned) : 0;
}

extern "C" int fp_mesh_transform_residuals(const float* pos, int Nv, const int32_t* faces, int F, const float* points, int Q,
                                           const float* tfs, int T, const float* thr2, int L, float* max_d2, int32_t* over,
                                           float* dist2, void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "fp_mesh_transform_residuals";
  FP_REQUIRE(T >= 0 && Q >= 0, "%s: T=%d or Q=%d is negative", name, T, Q);
  FP_REQUIRE((long long)T * (long long)Q <= (1ll << 30) && T <= (1 << 30), "%s: T=%d times Q=%d is above 2^30", name, T, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  FP_REQUIRE(L >= 0 && L <= kMaxThresholds, "%s: L=%d outside 0..%d", name, L, kMaxThresholds);
  if (T == 0) return FP_OK;
  FP_REQUIRE(max_d2, "%s: NULL max_d2", name);
  FP_REQUIRE(L == 0 || (thr2 && over), "%s: NULL thr2 or over with L=%d", name, L);
  FP_REQUIRE(Q == 0 || (points && tfs), "%s: NULL points or tfs", name);
  FP_REQUIRE(Q == 0 || F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(Q == 0 || F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  const size_t need = fp_mesh_transform_residuals_workspace_bytes(T, Q);
  FP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0),
             "%s: workspace too small or not 4-byte aligned (%zu < %zu bytes, see fp_mesh_transform_residuals_workspace_bytes)", name,
             workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned* cell = (unsigned*)workspace;
  const int n_pairs = T * Q;
  if (n_pairs > 0) {
    const int tiles = fp_cdiv(n_pairs, kThreads);
    hipLaunchKernelGGL(k_ms_init, dim3(tiles), dim3(kThreads), 0, st, cell, n_pairs);
    FP_CHECK_LAUNCH("fp_mesh_transform_residuals (init)");
    if (F > 0) {
      const int chunk = chunk_faces(tiles, F, kTile, kChunkMin, kFillWorkgroups);
      hipLaunchKernelGGL(k_ms_scan, dim3(tiles, fp_cdiv(F, chunk)), dim3(kThreads), 0, st, pos, Nv, faces, F, points, Q, tfs, n_pairs, chunk,
                         cell);
      FP_CHECK_LAUNCH("fp_mesh_transform_residuals (scan)");
    }
  }
  hipLaunchKernelGGL(k_ms_finish, dim3(T), dim3(kThreads), 0, st, cell, Q, thr2, L, max_d2, L > 0 ? over : nullptr, Q > 0 ? dist2 : nullptr);
  FP_CHECK_LAUNCH("fp_mesh_transform_residuals (finish)");
  return FP_OK;
}
